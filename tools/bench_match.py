#!/usr/bin/env python3
"""Times of match_motifs' three device stages (csrc/motif_match.hip: column-score histograms, null tables, pairs) for a seeded
synthetic library of --motifs count matrices of widths 6 .. 20 matched all against all on both strands, min_overlap 5: HIP events
around each stage, median of --reps runs after a warm-up.  Beside them, in the same process, the host path -- the same definitions
in numpy with Python loops over targets and offsets -- on a sample of --host_queries queries against the whole library, checked
against the device's results for those queries, and its time scaled to all queries: an extrapolation, not a measurement.  Prints
one JSON object."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def synthetic_library(n, rng):
    """count matrices of 40 sites, widths 6 .. 20; every fifth motif is a resampled (every other time reverse-complemented) copy
    of an earlier one, so that there are families to find"""
    out = []
    for i in range(n):
        if i % 5 == 4:
            C = out[int(rng.integers(0, i))]
            C = np.stack([rng.multinomial(40, (c + 0.5) / (c + 0.5).sum()) for c in C.T]).T
            out.append(C[::-1, ::-1].copy() if i % 10 == 9 else C)
            continue
        w = int(rng.integers(6, 21))
        p = np.full((w, 4), 0.05)
        p[np.arange(w), rng.integers(0, 4, w)] = 0.85
        out.append(np.stack([rng.multinomial(40, row) for row in p]).T)
    return out


def host_path(sample, cols, t_width, t_col0, min_overlap, revcom):
    """[(p_best, o, strand, L, x)] per sampled query and target: DESIGN.md section 17 in numpy"""
    fwd = np.concatenate(cols).astype(np.int64)
    lib = np.concatenate([fwd, fwd[:, ::-1]]) if revcom else fwd       # the reverse complement's columns: the bases reversed
    min_tw, results = int(t_width.min()), []
    for q in sample:
        uq = cols[q].astype(np.int64)
        w = len(uq)
        d2 = ((uq[:, None, :] - lib[None, :, :]) ** 2).sum(axis=2)
        s = (1448 - np.floor(np.sqrt(d2.astype(np.float64))).astype(np.int64)) // 16
        h = np.stack([np.bincount(row, minlength=91) for row in s]) / float(len(lib))
        sf, ml = {}, min(min_overlap, w, min_tw)
        for a in range(w):
            pmf = None
            for b in range(a, w):
                pmf = h[b] if pmf is None else np.convolve(pmf, h[b])
                if b - a + 1 >= ml:
                    sf[(a, b)] = np.cumsum(pmf[::-1])[::-1]
        row = []
        for t in range(len(cols)):
            wt, c0 = int(t_width[t]), int(t_col0[t])
            m = min(min_overlap, w, wt)
            mats = [s[:, c0:c0 + wt]] + ([s[:, len(fwd) + c0:len(fwd) + c0 + wt][:, ::-1]] if revcom else [])
            best = None
            for strand, S in enumerate(mats):
                for o in range(-(wt - m), w - m + 1):
                    a, b = max(0, o), min(w, wt + o) - 1
                    x = int(np.trace(S, offset=-o))
                    key = (float(sf[(a, b)][x]), -(b - a + 1), strand, o)
                    if best is None or key < best[0]:
                        best = (key, x)
            row.append((best[0][0], best[0][3], best[0][2], -best[0][1], best[1]))
        results.append(row)
    return results


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--motifs", type=int, default=2000)
    ap.add_argument("--host_queries", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=17)
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps must be at least 5")
    from kmap_amd import _ffi
    from kmap_amd import motif_match as K
    assert _ffi.device_count() >= 1, "no HIP device"
    rng = np.random.default_rng(args.seed)
    motifs = synthetic_library(args.motifs, rng)
    cols = [K.quantise_columns(C) for C in motifs]
    t_width = np.array([len(c) for c in cols], np.int64)
    t_col0 = np.concatenate([[0], np.cumsum(t_width[:-1])])
    out = {"device": _ffi.device_arch(), "motifs": args.motifs, "columns": int(t_width.sum()), "n_pairs": args.motifs ** 2, "revcom": True,
           "min_overlap": 5, "reps": args.reps,
           "table_bytes": 8 * sum(K.table_doubles(int(w), min(5, int(w), int(t_width.min()))) for w in t_width)}

    K.match_motifs(motifs, motifs, True, 5)                            # warm-up
    runs = []
    for _ in range(args.reps):
        ms = {}
        res = K.match_motifs(motifs, motifs, True, 5, stage_ms=ms)
        runs.append(ms)
    out["batches"] = runs[0]["batches"]
    for stage in ("histograms", "tables", "pairs"):
        v = [r[stage] for r in runs]
        out[stage] = {"ms_median": statistics.median(v), "ms_min": min(v), "ms_max": max(v)}
    out["device_ms_median_sum"] = sum(out[s]["ms_median"] for s in ("histograms", "tables", "pairs"))
    p_match, e_value, _ = K.pair_statistics(res.p_best, t_width, t_width, 5, True, all_against_all=True)
    out["families_at_e_0.01"] = len(set(K.families(args.motifs, K.family_links(e_value, 0.01))[0]))

    sample = sorted(rng.choice(args.motifs, size=min(args.host_queries, args.motifs), replace=False).tolist())
    t0 = time.perf_counter()
    host = host_path(sample, cols, t_width, t_col0, 5, True)
    host_s = time.perf_counter() - t0
    worst = 0.0
    for q, row in zip(sample, host):
        for t, (p, o, strand, L, x) in enumerate(row):
            worst = max(worst, abs(res.p_best[q, t] - p) / p)
            if abs(res.p_best[q, t] - p) <= 1e-9 * p and (res.o[q, t], res.strand[q, t]) != (o, strand):
                continue                                               # a tie within rounding between two configurations
            assert (res.o[q, t], res.strand[q, t], res.L[q, t], res.x[q, t]) == (o, strand, L, x), (q, t)
    assert worst <= 1e-9, worst
    out["host_numpy"] = {"queries": len(sample), "seconds": host_s, "p_best_max_rel_diff_to_device": worst,
                         "extrapolated_seconds_all_queries": host_s * args.motifs / len(sample)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
