"""numpy and Python restatement of DESIGN.md section 17 (match_motifs), independent of csrc/motif_match.hip and of the arithmetic in
kmap_amd/motif_match.py: the yardstick of tests/test_match_host.py and tests/test_gpu_match.py.  Plain loops; meant for a few
hundred pairs."""
import math

import numpy as np


def quantise(C, pseudocount=1.0):
    """int64 [4, w]: u[b][j] = rint(1024 f[b][j]), f = (C + a / 4) / (sum_b C + a) in float64"""
    C = np.asarray(C, np.float64)
    a = float(pseudocount)
    return np.rint(1024.0 * ((C + a / 4) / (C.sum(axis=0) + a))).astype(np.int64)


def revcomp(u):
    """u_rc[b][j] = u[3 - b][w - 1 - j]"""
    return u[::-1, ::-1]


def col_score(x, y):
    d2 = int(sum((int(a) - int(b)) ** 2 for a, b in zip(x, y)))
    return (1448 - math.isqrt(d2)) // 16


def score_matrix(uq, ut):
    """S[i][j] = s(query column i, target column j)"""
    return np.array([[col_score(uq[:, i], ut[:, j]) for j in range(ut.shape[1])] for i in range(uq.shape[1])], np.int64)


def library_columns(targets_u, revcom):
    """the columns the null counts: those of every target and, with revcom, of every reverse-complemented target; int64 [N, 4]"""
    cols = [u.T for u in targets_u] + ([revcomp(u).T for u in targets_u] if revcom else [])
    return np.concatenate(cols)


def col_scores_vec(x, cols):
    """s(x, y) for every row y of cols, in exact integers"""
    d2 = ((cols - np.asarray(x, np.int64)[None, :]) ** 2).sum(axis=1)
    e = np.array([math.isqrt(int(v)) for v in d2], np.int64)
    return (1448 - e) // 16


def null_hist(uq, lib_cols):
    """uint32 [w_q, 91]"""
    H = np.zeros((uq.shape[1], 91), np.uint32)
    for i in range(uq.shape[1]):
        H[i] = np.bincount(col_scores_vec(uq[:, i], lib_cols), minlength=91)
    return H


def null_tables(H, n_null, min_len=1):
    """{(a, b): (pmf, sf)} for every range of at least min_len columns; float64"""
    h = H.astype(np.float64) / float(n_null)
    out = {}
    for a in range(len(H)):
        pmf = None
        for b in range(a, len(H)):
            pmf = h[b].copy() if pmf is None else np.convolve(pmf, h[b])
            if b - a + 1 >= min_len:
                out[(a, b)] = (pmf, np.cumsum(pmf[::-1])[::-1])
    return out


def configurations(uq, ut, tables, min_overlap, revcom, scores=None):
    """[(p, o, strand, L, x)] of one pair, strand 0 '+' / 1 '-'; `scores` = (score_matrix(uq, ut), score_matrix(uq, revcomp(ut))) when
    the caller has them already"""
    wq, wt = uq.shape[1], ut.shape[1]
    m = min(min_overlap, wq, wt)
    cfgs = []
    for strand, u in enumerate([ut, revcomp(ut)] if revcom else [ut]):
        S = score_matrix(uq, u) if scores is None else scores[strand]
        for o in range(-(wt - m), wq - m + 1):
            a, b = max(0, o), min(wq, wt + o) - 1
            x = int(sum(S[i][i - o] for i in range(a, b + 1)))
            cfgs.append((float(tables[(a, b)][1][x]), o, strand, b - a + 1, x))
    return cfgs


def best_configuration(cfgs):
    """the smallest p; among exactly equal doubles the larger L, then + before -, then the smaller o"""
    return min(cfgs, key=lambda c: (c[0], -c[3], c[2], c[1]))


def n_cfg(wq, wt, min_overlap, revcom):
    m = min(min_overlap, wq, wt)
    return (wq + wt - 2 * m + 1) * (2 if revcom else 1)


def p_match(p_best, n):
    return 1.0 if p_best == 1.0 else -math.expm1(n * math.log1p(-p_best))


def bh(p):
    """Benjamini-Hochberg, written out: q of the i-th smallest of n = min over j >= i of p_(j) n / j, at most 1"""
    p = list(p)
    order = sorted(range(len(p)), key=lambda i: p[i])
    q, run = [0.0] * len(p), 1.0
    for rank in range(len(p), 0, -1):
        i = order[rank - 1]
        run = min(run, p[i] * len(p) / rank)
        q[i] = run
    return q


def random_counts(rng, w, nsites=40, sharp=0.8):
    """a count matrix [4, w] of a random motif: `sharp` of the columns dominated by one base"""
    C = np.zeros((4, w), np.int64)
    for j in range(w):
        if rng.random() < sharp:
            p = np.full(4, 0.05)
            p[rng.integers(0, 4)] = 0.85
        else:
            p = rng.dirichlet(np.ones(4))
        C[:, j] = rng.multinomial(nsites, p)
    return C
