#!/usr/bin/env python3
"""Time of rank_motif_library's device pass (csrc/pwm_library.hip: the batched best-score-per-read kernel and the flat histogram
kernel, one read-back per batch) over resident reads at the C3 shape (10 M x 150 bp, generated in HBM) for M = 16 matrices of widths
spread over 6 .. 31 on both strands, and beside it, in the same process, the path it replaces: 16 x (read_scores + histogram), the
per-matrix calls evaluate_pwm makes (csrc/pwm_readscore.hip), into result arrays allocated once.  Both produce the same 16
histograms, which is checked.  Times are HIP-event times around all 16 matrices, median of --reps runs after a warm-up of each path.
Prints one JSON object."""
import argparse
import ctypes as C
import json
import statistics
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def library_matrices(n_mat, rng):
    """count matrices as a library holds them: widths spread evenly over 6 .. 31, ~90 % consensus base per column"""
    out = []
    for w in np.linspace(6, 31, n_mat).round().astype(int).tolist():
        C4 = rng.integers(2, 6, size=(4, w))
        C4[rng.integers(0, 4, w), np.arange(w)] = 90
        out.append(C4)
    return out


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
    from kmap_amd.device_seq import LIBRARY_BATCH, LIBRARY_BATCH_CHUNKS
    from kmap_amd.motif_discovery import ReadScores
    from kmap_amd.pwm import pwm_threshold, pwm_weights
    assert _ffi.device_count() >= 1, "no HIP device"
    ds = synth.synth_reads_dev(args.reads, args.read_len, 3)
    rng = np.random.default_rng(7)
    Ws = [np.ascontiguousarray(pwm_weights(C4), np.int32) for C4 in library_matrices(args.matrices, rng)]
    ranges = [pwm_threshold(W, 1e-4)[1:] for W in Ws]
    los, nbs = [lo for lo, _ in ranges], [hi - lo + 1 for lo, hi in ranges]
    out = {"device": _ffi.device_arch(), "reads": args.reads, "read_len": args.read_len, "positions": ds.n, "reps": args.reps,
           "matrices": args.matrices, "widths": [int(W.shape[1]) for W in Ws], "bins": nbs, "batch": LIBRARY_BATCH,
           "batch_chunks": LIBRARY_BATCH_CHUNKS}
    ev0, ev1 = _ffi.Event(), _ffi.Event()
    kept = {}

    def batched():
        kept["batched"] = ds.library_histograms(Ws, los, nbs, True)

    rs = ReadScores(ds.n_seq)                                       # allocated once: the calls are timed, not hipMalloc
    n_scored = _ffi.i64(0)

    def sequential():
        hists, scored = [], []
        for W, lo, nb in zip(Ws, los, nbs):
            _ffi.check(_ffi.lib().kmap_readscore_packed_dev(ds.codes.ptr, ds.inval_orig.ptr, ds.n, ds.borders.ptr, ds.n_seq, W.shape[1],
                                                            _ffi.ptr(W), 1, rs.score.ptr, rs.loc.ptr, rs.strand.ptr, C.byref(n_scored), None))
            hists.append(rs.histogram(lo, nb))
            scored.append(n_scored.value)
        kept["sequential"] = (hists, scored)

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

    out["sequential"] = timed(sequential)
    out["batched"] = timed(batched)
    hists, outside, scored = kept["batched"]
    assert not outside.any() and scored.tolist() == kept["sequential"][1]
    for a, b in zip(hists, kept["sequential"][0]):
        np.testing.assert_array_equal(a, b)
    out["ratio_batched_to_sequential"] = out["batched"]["ms_median"] / out["sequential"]["ms_median"]
    out["per_matrix_ms"] = {k: out[k]["ms_median"] / args.matrices for k in ("sequential", "batched")}
    rs.close()
    ds.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
