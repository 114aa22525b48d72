#!/usr/bin/env python3
"""Time of one lockstep refinement round of discover_pwms (csrc/pwm_sites.hip: the batched best-(score, loc)-per-read kernel and
sites_count_kernel, one read-back per batch) over resident reads at the C3 shape (10 M x 150 bp, generated in HBM) for the M = 16
matrices of tools/bench_library.py on both strands at their p = 10^-4 thresholds.  Beside it, in the same process and on the same
inputs: library_sites (the pass it extends; the ratio shows what the counting kernel adds), and the path it replaces -- 16 x
pwm_counts(select_best=True), refine_pwm's own iteration.  That path must give the same 16 matrices, which is checked.  Times are
HIP-event times around all 16 matrices, median of --reps runs after a warm-up of each path.  Prints one JSON object."""
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

    def counts():
        kept["counts"] = ds.library_counts(Ws, ts, True)

    def sites():
        kept["sites"] = ds.library_sites(Ws, ts, True, max_len=L)

    def per_matrix():
        kept["per_matrix"] = [ds.pwm_counts(W, t, True, True) for W, t in zip(Ws, ts)]

    def timed(call):
        call()                                                     # warm-up of this path
        _ffi.sync()
        ms = []
        for _ in range(args.reps):
            ev0.record()
            call()
            ev1.record()
            _ffi.sync()
            ms.append(ev0.elapsed_ms(ev1))
        return {"ms_median": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms)}

    out["per_matrix_pwm_counts"] = timed(per_matrix)
    out["library_sites"] = timed(sites)
    out["library_counts"] = timed(counts)
    Cs, n_sel, n_minus = kept["counts"]
    for m, (C1, _, sel, minus) in enumerate(kept["per_matrix"]):
        np.testing.assert_array_equal(Cs[m], C1, err_msg=f"matrix {m}")
        assert (int(n_sel[m]), int(n_minus[m])) == (sel, minus), m
    np.testing.assert_array_equal(n_sel, kept["sites"][2])
    out["n_selected"], out["n_minus"] = n_sel.tolist(), n_minus.tolist()
    out["ratio_counts_to_sites"] = out["library_counts"]["ms_median"] / out["library_sites"]["ms_median"]
    out["ratio_counts_to_per_matrix"] = out["library_counts"]["ms_median"] / out["per_matrix_pwm_counts"]["ms_median"]
    out["per_matrix_ms"] = {k: out[k]["ms_median"] / args.matrices for k in ("per_matrix_pwm_counts", "library_sites", "library_counts")}
    ds.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
