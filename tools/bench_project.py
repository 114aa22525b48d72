#!/usr/bin/env python3
"""Times `project_kmers` on a seeded synthetic input: M query k-mers onto a map of N sampled k-mers (mutants of two consensuses
plus noise, repeated like a sample; the anchors are a seeded scatter -- only the time is of interest here).  The neighbour-sum
rows of the reference set are built once (that part is `visualize_kmers`' own and is reported, not timed as projection); the
selection and the rows part (query sums + probabilities + start + descent, blocked by the byte budget) are timed apart, each after
a warm-up of the same shape, by a host clock around work that ends in a device synchronise.  Prints one JSON line.

    python tools/bench_project.py                      # M = N = 50 000, k = 8, n_iter = 100
    python tools/bench_project.py --queries 5000 --refs 20000 --kmer_len 12
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def make_refs(n, k, rng):
    n_uniq = max(1, int(0.35 * n))
    cons = rng.integers(0, 4, size=(2, k))
    bases = rng.integers(0, 4, size=(n_uniq, k))
    label = np.full(n_uniq, 2, np.int32)
    for g in (0, 1):
        rows = np.arange(g * n_uniq // 5, (g + 1) * n_uniq // 5)
        keep = rng.random((len(rows), k)) < 0.8
        bases[rows] = np.where(keep, cons[g], bases[rows])
        label[rows] = g
    kh = np.zeros(n_uniq, np.uint64)
    for p in range(k):
        kh = (kh << np.uint64(2)) | bases[:, p].astype(np.uint64)
    kh, first = np.unique(kh, return_index=True)
    label = label[first]
    cnts = np.ones(len(kh), np.int64)
    np.add.at(cnts, rng.integers(0, len(kh), n - len(kh)), 1)
    return np.repeat(kh, cnts), np.repeat(label, cnts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=50_000)
    ap.add_argument("--refs", type=int, default=50_000)
    ap.add_argument("--kmer_len", type=int, default=8)
    ap.add_argument("--n_iter", type=int, default=100)
    ap.add_argument("--n_neighbour", type=int, default=20)
    ap.add_argument("--repeat", type=int, default=2)
    a = ap.parse_args()
    from kmap_amd import _ffi
    from kmap_amd.kmer_count import get_hash_dtype
    from kmap_amd.projection import DEFAULT_BYTE_BUDGET, hd_prob_lut_projected, project_knn, project_rows
    from kmap_amd.visualization import dedupe_sums_rows, sums_rows_from_kmers
    assert _ffi.device_count() >= 1, "no HIP device: nothing to measure"
    rng = np.random.default_rng(2026)
    k, n, m, n_nb = a.kmer_len, a.refs, a.queries, a.n_neighbour
    dt = get_hash_dtype(k)
    ref, lab = make_refs(n, k, rng)
    ref = ref.astype(dt)
    xy = np.round(rng.normal(0, 8, size=(2, n)), 3).astype(np.float32)
    q = np.where(rng.random(m) < 0.5, ref[rng.integers(0, n, m)].astype(np.uint64) ^ (np.uint64(1) << rng.integers(0, 2 * k, m).astype(np.uint64)),
                 rng.integers(0, 4 ** k, m).astype(np.uint64)).astype(dt)
    t0 = time.perf_counter()
    sums_d, lds = sums_rows_from_kmers(ref, lab, k, [k, k], n_nb, None, natural_diag=True, matrix_fallback=False)
    sums_d, rowmap_d, stored = dedupe_sums_rows(sums_d, n, lds, n=n)
    _ffi.sync()
    sref_s = time.perf_counter() - t0
    lut = hd_prob_lut_projected(k, n_nb)
    try:
        knn_s, rows_s, block_rows = [], [], 0
        for rep in range(a.repeat + 1):                    # the first pass is the warm-up of both shapes
            t1 = time.perf_counter()
            kh, nb, nb_dist, flipped = project_knn(q, ref, k, n_nb, True)
            t2 = time.perf_counter()
            xy_q, _, _, block_rows = project_rows(nb, sums_d, lds, n, lut, xy, a.n_iter, 0.01, rowmap_d, stored, DEFAULT_BYTE_BUDGET)
            t3 = time.perf_counter()
            if rep:
                knn_s.append(t2 - t1)
                rows_s.append(t3 - t2)
    finally:
        sums_d.free()
        if rowmap_d is not None:
            rowmap_d.free()
    pairs = float(m) * n
    print(json.dumps({"bench": "project_kmers", "queries": m, "refs": n, "kmer_len": k, "n_iter": a.n_iter, "n_neighbour": n_nb,
                      "stored_sums_rows": int(stored), "block_rows": int(block_rows), "flipped": int(flipped.sum()),
                      "finite": bool(np.isfinite(xy_q).all()), "sref_build_s": round(sref_s, 3),
                      "knn_s": round(min(knn_s), 4), "rows_s": round(min(rows_s), 4),
                      "all_knn_s": [round(v, 4) for v in knn_s], "all_rows_s": [round(v, 4) for v in rows_s],
                      "knn_gpairs_per_s": round(pairs / min(knn_s) / 1e9, 1),
                      "descent_gpairs_per_s": round(pairs * a.n_iter / min(rows_s) / 1e9, 1)}))


if __name__ == "__main__":
    main()
