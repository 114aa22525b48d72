#!/usr/bin/env python3
"""Time of motif_centrality's device pass (csrc/pwm_sites.hip: the batched best-(score, loc)-per-read kernel and the offset / length
histogram kernel, one read-back per batch) over resident reads at the C3 shape (10 M x 150 bp, generated in HBM) for the M = 16
matrices of tools/bench_library.py on both strands at their p = 10^-4 thresholds.  Beside it, in the same process and on the same
inputs: library_histograms (csrc/pwm_library.hip, the score-only pass this one extends), and the path it replaces -- 16 x
(read_scores + fetch of score and loc + np.bincount on the host).  That path must give the same histograms, which is checked.  Times
are HIP-event times around all 16 matrices, median of --reps runs after a warm-up of each path.  Prints one JSON object."""
import argparse
import ctypes as C
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
    from kmap_amd.motif_discovery import ReadScores
    from kmap_amd.pwm import pwm_threshold, pwm_weights
    assert _ffi.device_count() >= 1, "no HIP device"
    ds = synth.synth_reads_dev(args.reads, args.read_len, 3)
    rng = np.random.default_rng(7)
    Ws = [np.ascontiguousarray(pwm_weights(C4), np.int32) for C4 in library_matrices(args.matrices, rng)]
    plans = [pwm_threshold(W, 1e-4) for W in Ws]
    ts, los, nbs = [p[0] for p in plans], [p[1] for p in plans], [p[2] - p[1] + 1 for p in plans]
    L = args.read_len
    out = {"device": _ffi.device_arch(), "reads": args.reads, "read_len": L, "positions": ds.n, "reps": args.reps,
           "matrices": args.matrices, "widths": [int(W.shape[1]) for W in Ws], "thresholds": ts}
    ev0, ev1 = _ffi.Event(), _ffi.Event()
    kept = {}

    def sites():
        kept["sites"] = ds.library_sites(Ws, ts, True, max_len=L)

    def histograms():
        kept["histograms"] = ds.library_histograms(Ws, los, nbs, True)

    rs = ReadScores(ds.n_seq)                                       # allocated once: the calls are timed, not hipMalloc
    n_scored = _ffi.i64(0)

    def per_matrix():
        D, Hlen = np.zeros((len(Ws), 2 * L + 1), np.int64), np.zeros((len(Ws), L + 1), np.int64)
        for m, (W, t) in enumerate(zip(Ws, ts)):
            _ffi.check(_ffi.lib().kmap_readscore_packed_dev(ds.codes.ptr, ds.inval_orig.ptr, ds.n, ds.borders.ptr, ds.n_seq, W.shape[1],
                                                            _ffi.ptr(W), 1, rs.score.ptr, rs.loc.ptr, rs.strand.ptr, C.byref(n_scored), None))
            score, loc, _ = rs.fetch()
            site = (loc >= 0) & (score >= t)                        # every read has L bases here
            D[m] = np.bincount(2 * loc[site].astype(np.int64) + W.shape[1] - L + L, minlength=2 * L + 1)
            Hlen[m, L] = int(site.sum())
        kept["per_matrix"] = (D, Hlen)

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

    out["per_matrix_fetch_bincount"] = timed(per_matrix)
    out["library_histograms"] = timed(histograms)
    out["library_sites"] = timed(sites)
    D, Hlen, n_sites, too_long = kept["sites"]
    assert not too_long.any()
    np.testing.assert_array_equal(D, kept["per_matrix"][0])
    np.testing.assert_array_equal(Hlen, kept["per_matrix"][1])
    out["n_sites"] = n_sites.tolist()
    out["ratio_sites_to_histograms"] = out["library_sites"]["ms_median"] / out["library_histograms"]["ms_median"]
    out["ratio_sites_to_per_matrix"] = out["library_sites"]["ms_median"] / out["per_matrix_fetch_bincount"]["ms_median"]
    out["per_matrix_ms"] = {k: out[k]["ms_median"] / args.matrices for k in ("per_matrix_fetch_bincount", "library_histograms", "library_sites")}
    rs.close()
    ds.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
