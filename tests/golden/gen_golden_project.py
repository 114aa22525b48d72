#!/usr/bin/env python3
"""Generate tests/golden/project_maps.npz: seeded reference sets for the project_kmers tests and a map for each, embedded by
this repository's CPU oracle (oracle.kmap) -- the tests need anchors that are an equilibrium of the map's own forces, which a
random scatter is not.

    python tests/golden/gen_golden_project.py

Per set <tag> in (k8n300, k16n300, k8n1100, k16n1100):
  <tag>_kh / <tag>_cnts / <tag>_label   unique k-mers (uint64), their repeat counts and labels as sample_kmers.pkl holds them: label 0 =
                                        mutants of a full-length consensus, label 1 = of a consensus two bases shorter than k (the
                                        label rule of the Hamming matrix applies), label 2 = noise
  <tag>_clens                           consensus lengths [k, k - 2]
  <tag>_xy                              float32 [2, N] map of the expanded set, rounded to 3 decimals like low_dim_data.tsv
"""
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent.parent))
N_NB = 20


def make_set(k, n, seed):
    rng = np.random.default_rng(seed)
    n_uniq = int(0.75 * n)
    cons = rng.integers(0, 4, size=(2, k))
    bases = np.empty((n_uniq, k), np.int64)
    label = np.empty(n_uniq, np.int64)
    for i in range(n_uniq):
        g = 0 if i < n_uniq // 5 else (1 if i < 2 * n_uniq // 5 else 2)
        label[i] = g
        if g == 2:
            bases[i] = rng.integers(0, 4, size=k)
            continue
        b = cons[g].copy()
        clen = k if g == 0 else k - 2
        for p in rng.choice(clen, size=rng.integers(0, 3), replace=False):
            b[p] = (b[p] + rng.integers(1, 4)) % 4
        if g == 1:
            b[clen:] = rng.integers(0, 4, size=k - clen)
        bases[i] = b
    kh = np.zeros(n_uniq, np.uint64)
    for p in range(k):
        kh = (kh << np.uint64(2)) | bases[:, p].astype(np.uint64)
    kh, first = np.unique(kh, return_index=True)                  # sample_kmers.pkl holds unique k-mers
    label = label[first]
    order = np.argsort(label, kind="stable")
    kh, label = kh[order], label[order]
    cnts = np.ones(len(kh), np.int64)
    while cnts.sum() < n:
        cnts[rng.integers(0, len(kh))] += 1
    return kh, cnts, label, np.array([k, k - 2], np.int32)


def main():
    from oracle import oracle as O
    out = {}
    for k, n, seed, iters in ((8, 300, 81, 2500), (16, 300, 161, 2500), (8, 1100, 82, 1500), (16, 1100, 162, 1500)):
        tag = f"k{k}n{n}"
        kh, cnts, label, clens = make_set(k, n, seed)
        D = O.hamdist_matrix_u8(np.repeat(kh, cnts), np.repeat(label, cnts).astype(np.int32), k, clens).astype(np.int64)
        nb = O.knn_select_stable(D, N_NB)
        xy = O.kmap(D, k, n_neighbour=N_NB, n_max_iter=iters, random_seed=5, nb=nb)
        out.update({f"{tag}_kh": kh, f"{tag}_cnts": cnts, f"{tag}_label": label, f"{tag}_clens": clens,
                    f"{tag}_xy": np.round(xy.astype(np.float64), 3).astype(np.float32)})
        print(tag, len(kh), "unique,", int(cnts.sum()), "points, |xy| <=", float(np.abs(xy).max()))
    np.savez_compressed(HERE / "project_maps.npz", **out)


if __name__ == "__main__":
    main()
