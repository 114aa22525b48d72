#!/usr/bin/env python3
"""Time of DeviceSeq.erase_sites (csrc/pwm_erase.hip: one pwm_erase_kernel launch per matrix, erase_apply_kernel, one read-back) over
resident reads at the C3 shape (10 M x 150 bp, generated in HBM) for the M = 16 matrices of tools/bench_library.py on both strands
at their p = 10^-4 thresholds.  Beside it, in the same process and on the same inputs: library_sites (the batched best-window pass:
what scoring the same matrices costs when nothing per position is kept).  Every erase_sites run starts from the original mask
(reset() outside the timed span), so every run does the same work.  Times are HIP-event times around all 16 matrices, median of
--reps runs after a warm-up of each path.  Prints one JSON object."""
import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from bench_library import library_matrices  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--read_len", type=int, default=150)
    ap.add_argument("--matrices", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps must be at least 5")
    from kmap_amd import _ffi, synth
    from kmap_amd.pwm import pwm_threshold, pwm_weights
    assert _ffi.device_count() >= 1, "no HIP device"
    ds = synth.synth_reads_dev(args.reads, args.read_len, 3)
    rng = np.random.default_rng(7)
    Ws = [np.ascontiguousarray(pwm_weights(C4), np.int32) for C4 in library_matrices(args.matrices, rng)]
    ts = [pwm_threshold(W, 1e-4)[0] for W in Ws]
    L = args.read_len
    out = {"device": _ffi.device_arch(), "reads": args.reads, "read_len": L, "positions": ds.n, "reps": args.reps,
           "matrices": args.matrices, "widths": [int(W.shape[1]) for W in Ws], "thresholds": ts}
    ev0, ev1 = _ffi.Event(), _ffi.Event()
    kept = {}

    def erase():
        kept["erase"] = ds.erase_sites(Ws, ts, True)

    def sites():
        kept["sites"] = ds.library_sites(Ws, ts, True, max_len=L)

    def timed(call, before=None):
        runs = []
        for rep in range(args.reps + 1):                           # the first run is the warm-up of this path
            if before is not None:
                before()
                _ffi.sync()
            ev0.record()
            call()
            ev1.record()
            _ffi.sync()
            if rep:
                runs.append(ev0.elapsed_ms(ev1))
        return {"ms_median": statistics.median(runs), "ms_min": min(runs), "ms_max": max(runs)}

    out["library_sites"] = timed(sites)
    out["erase_sites"] = timed(erase, before=ds.reset)
    n_hits, n_cov, n_new = kept["erase"]
    assert (n_hits >= kept["sites"][2]).all() and (n_cov <= n_hits * np.array(out["widths"])).all() and 0 < n_new <= int(n_cov.sum())
    out["n_hits"], out["n_covered"], out["n_new"] = n_hits.tolist(), n_cov.tolist(), int(n_new)
    out["ratio_erase_to_sites"] = out["erase_sites"]["ms_median"] / out["library_sites"]["ms_median"]
    out["per_matrix_ms"] = {k: out[k]["ms_median"] / args.matrices for k in ("library_sites", "erase_sites")}
    ds.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
