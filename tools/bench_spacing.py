#!/usr/bin/env python3
"""Time of motif_spacing's device pass (csrc/pwm_spacing.hip: the primary-site kernel, the batched best-non-overlapping-window kernel
and the gap / room histogram kernel, one read-back per batch) over resident reads at the C3 shape (10 M x 150 bp, generated in HBM)
for the M = 16 matrices of tools/bench_library.py on both strands at their p = 10^-4 thresholds, max_gap 150, the matrix with the
most information (the largest best score) as the primary; its read_scores are made once, outside the timed calls, as the verb does.
Beside it, in the same process and on the same inputs: library_sites (csrc/pwm_sites.hip, the pass this one extends), and the path
it replaces -- 16 x (scan_pwm + fetch of the hit list + the reduction of definitions 2 - 4 in numpy on the host).  That path must
give the same histograms, which is checked.  Times are HIP-event times around all 16 matrices, median of --reps runs after a warm-up
of each path.  Prints one JSON object."""
import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from bench_library import library_matrices  # noqa: E402


def host_pairs(hits, loc, score, minus, ploc, pminus, L, w, wP, G):
    """(S, R, n_pair, n_far) of DESIGN.md section 19 from one matrix's hit list (hits per read; loc, score, strand per hit in read
    order): the hits of primary reads that do not overlap the primary window, per read the best one -- the largest score, then the
    smallest loc --, then gap, quadrant and rooms.  Every read has L bases here."""
    read = np.repeat(np.arange(len(hits), dtype=np.int64), hits)
    loc, p = loc.astype(np.int64), ploc[read]
    keep = (p >= 0) & ((loc + w <= p) | (loc >= p + wP))
    read, loc, score, minus, p = read[keep], loc[keep], score[keep].astype(np.int64), minus[keep].astype(bool), p[keep]
    S, R = np.zeros((4, G + 1), np.int64), np.zeros((G + 2, G + 2), np.int64)
    if len(read) == 0:
        return S, R, 0, 0
    order = np.lexsort((loc, -score, read))
    best = order[np.concatenate([[True], read[order][1:] != read[order][:-1]])]
    read, loc, minus, p = read[best], loc[best], minus[best], p[best]
    left, sP = loc + w <= p, pminus[read]
    g = np.where(left, p - loc - w, loc - p - wP)
    near = g <= G
    left_room, right_room = np.minimum(np.maximum(p - w + 1, 0), G + 1), np.minimum(np.maximum(L - p - wP - w + 1, 0), G + 1)
    quadrant = 2 * (~left ^ sP).astype(np.int64) + (minus != sP)
    u, d = np.where(sP, right_room, left_room), np.where(sP, left_room, right_room)
    np.add.at(S, (quadrant[near], g[near]), 1)
    np.add.at(R, (u[near], d[near]), 1)
    return S, R, len(read), int((~near).sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--read_len", type=int, default=150)
    ap.add_argument("--matrices", type=int, default=16)
    ap.add_argument("--max_gap", type=int, default=150)
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
    plans = [pwm_threshold(W, 1e-4) for W in Ws]
    ts = [p[0] for p in plans]
    i_prim = int(np.argmax([p[2] for p in plans]))                  # the largest best score: the most information
    W_P, tP, wP = Ws[i_prim], ts[i_prim], int(Ws[i_prim].shape[1])
    L, G = args.read_len, args.max_gap
    out = {"device": _ffi.device_arch(), "reads": args.reads, "read_len": L, "positions": ds.n, "reps": args.reps,
           "matrices": args.matrices, "widths": [int(W.shape[1]) for W in Ws], "thresholds": ts, "max_gap": G,
           "primary": i_prim, "primary_width": wP, "primary_threshold": tP}
    ev0, ev1 = _ffi.Event(), _ffi.Event()
    kept = {}
    rs = ds.read_scores(W_P, True)                                  # the primary's best window of every read: made once
    p_score, p_loc, p_strand = rs.fetch()
    ploc, pminus = np.where((p_loc >= 0) & (p_score >= tP), p_loc, -1).astype(np.int64), p_strand.astype(bool)

    def spacing():
        kept["spacing"] = ds.library_spacing(rs, wP, tP, Ws, ts, True, G)

    def sites():
        kept["sites"] = ds.library_sites(Ws, ts, True, max_len=L)

    def per_matrix():
        rows = []
        for W, t in zip(Ws, ts):
            hits, loc, score, strand = ds.scan_pwm(W, t, True)
            rows.append(host_pairs(hits, loc, score, strand, ploc, pminus, L, int(W.shape[1]), wP, G))
        kept["per_matrix"] = rows

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

    out["per_matrix_scan_fetch_reduce"] = timed(per_matrix)
    out["library_sites"] = timed(sites)
    out["library_spacing"] = timed(spacing)
    S, R, n_primary, n_pair, n_far = kept["spacing"]
    assert n_primary == int((ploc >= 0).sum())
    for m, (Sm, Rm, pairs, far) in enumerate(kept["per_matrix"]):
        np.testing.assert_array_equal(S[m], Sm)
        np.testing.assert_array_equal(R[m], Rm)
        assert (int(n_pair[m]), int(n_far[m])) == (pairs, far)
    out["n_primary"], out["n_pair"], out["n_far"] = int(n_primary), n_pair.tolist(), n_far.tolist()
    out["ratio_spacing_to_sites"] = out["library_spacing"]["ms_median"] / out["library_sites"]["ms_median"]
    out["ratio_spacing_to_per_matrix"] = out["library_spacing"]["ms_median"] / out["per_matrix_scan_fetch_reduce"]["ms_median"]
    out["per_matrix_ms"] = {k: out[k]["ms_median"] / args.matrices for k in ("per_matrix_scan_fetch_reduce", "library_sites", "library_spacing")}
    rs.close()
    ds.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
