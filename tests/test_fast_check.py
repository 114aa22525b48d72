"""The checker of the FAST force kernels, checked on the CPU: the float64 oracle (ko_embed_forces_rows_f64) against a numpy
restatement, the f32 oracle inside the per-element bound, and the power of the bound on planted pairs (tests/_fast_check.py)."""
import numpy as np
import pytest

from oracle import baseline as B
from oracle import oracle as O
from tests import _fast_check as F


def _numpy_f64(P, rows, y):
    y = y.astype(np.float64)
    n = y.shape[1]
    g, m, loss = np.zeros((2, len(rows))), np.zeros((2, len(rows))), np.zeros(len(rows))
    for t, i in enumerate(rows):
        j = np.arange(n) != i
        d = y[:, i:i + 1] - y[:, j]
        q = np.clip(1.0 / (1.0 + (d * d).sum(0)), 1e-3, 1 - 1e-3)
        p = P[t, j].astype(np.float64)
        g[:, t] = (q / (1 - q) * (p - q) * d).sum(1)
        m[:, t] = (q / (1 - q) * (np.abs(p) + q) * np.abs(d)).sum(1)
        up = np.arange(n)[j] > i
        full = -p * np.log(q) - (1 - p) * np.log(1 - q)
        ce = np.where(p < 1e-10, -np.log(1 - q), np.where(p > 1 - 1e-10, -np.log(q), full))
        loss[t] = ce[up].sum()
    return g, m, loss


def _inputs(n, scale, seed):
    rng = np.random.default_rng(seed)
    y = (rng.standard_normal((2, n)) * scale).astype(np.float32)
    y[:, n // 3] = y[:, 0]                                                  # a coincident pair
    P = rng.random((n, n)).astype(np.float32) * 0.3
    P[rng.random((n, n)) < 0.2] = 0.0
    P[rng.random((n, n)) < 0.05] = 1e-11
    P[rng.random((n, n)) < 0.05] = 1.0
    return y, P


@pytest.mark.parametrize("n,scale", [(1, 1.0), (2, 1.0), (7, 1e-3), (65, 1.0), (300, 30.0), (300, 1e16)])
def test_f64_oracle_equals_numpy(n, scale):
    y, P = _inputs(n, scale, n)
    rows = np.arange(n, dtype=np.int64)[::-1].copy()
    g, m, loss = O.embed_forces_rows_f64(P[rows], rows, y)
    gw, mw, lw = _numpy_f64(P[rows], rows, y)
    np.testing.assert_allclose(g, gw, rtol=0, atol=1e-12 * max(mw.max(), 1e-300))
    np.testing.assert_allclose(m, mw, rtol=1e-12, atol=0)
    np.testing.assert_allclose(loss, lw, rtol=1e-12, atol=0)
    assert np.all(m >= np.abs(g))


@pytest.mark.parametrize("n,scale", [(64, 1.0), (513, 1.0), (1000, 30.0), (2000, 1e-3)])
def test_f32_oracle_within_bound(n, scale):
    """the reference's own f32 arithmetic (kb_embed_forces_rows: j ascending, no FMA) lies inside the bound around the float64
    value with its own kappa: n - 1 sequential adds and the f32 1 - q, which loses up to 999 ulps next to the q clip"""
    y, P = _inputs(n, scale, 5)
    rows = np.unique(np.r_[0, n - 1, np.random.default_rng(1).integers(0, n, 100)]).astype(np.int64)
    g32 = B.embed_forces_rows(P[rows], rows, y, threads=4)
    g, m, _ = O.embed_forces_rows_f64(P[rows], rows, y)
    F.assert_forces_close(g32, g, m, F.kappa_worst("ref32", n), rows, "f32 oracle")


def _planted(n):
    pl = F.Planted(n, F.structural_pairs(n), seed=3)
    rows = F.check_rows(n, planted=pl)
    g, m, _ = F.reference(pl, rows, pl.coords)
    return pl, rows, g, m


@pytest.mark.parametrize("n", [1000, 4099])
def test_planted_pairs_make_the_check_fail_at_their_rows(n):
    """with a planted pair removed from the float64 reference, or its sign flipped, the comparison fails at exactly the pair's
    two rows: the device value stands in as the float64 value rounded to f32 (a kernel exact up to its last rounding)"""
    pl, rows, g, m = _planted(n)
    g_dev = g.astype(np.float32)
    kappa = max(F.KAPPA_ROWS, F.KAPPA_SYM, F.KAPPA_CYCLIC)
    F.assert_forces_close(g_dev, g, m, kappa, rows, "rounded")
    assert pl.assert_visible(rows, m, kappa) >= F.POWER
    assert len(pl.pairs) >= 8
    pos = {int(r): t for t, r in enumerate(rows)}
    terms = pl.pair_terms()
    for (i, j), tm in zip(pl.pairs, terms):
        for factor in (1.0, 2.0):                                 # removed (g - term) / negated (g - 2 term)
            gw = g.copy()
            gw[:, pos[i]] -= factor * tm
            gw[:, pos[j]] += factor * tm
            bad = F.failing_rows(g_dev, gw, m, kappa)
            assert sorted(rows[bad].tolist()) == [i, j], ((i, j), factor, rows[bad].tolist())


def test_planted_layout():
    """background pairs are clamped (d2 >= 999), each planted pair sits inside [0.01, 1] and dominates both rows"""
    n = 2100
    pl = F.Planted(n, F.structural_pairs(n), seed=3)
    y = pl.coords.astype(np.float64)
    partner = {}
    for i, j in pl.pairs:
        partner[i], partner[j] = j, i
    for i in (0, 255, 256, 700, 1022, n - 1, 1234):
        d2 = ((y[:, i:i + 1] - y) ** 2).sum(0)
        d2[i] = np.inf
        if i in partner:
            assert 0.009 <= d2[partner[i]] <= 1.01
            d2[partner[i]] = np.inf
        assert d2.min() >= 999.0
    S = pl.sums_rows(np.arange(n))
    np.testing.assert_array_equal(S, S.T)


def test_kappa_capped_by_worst_case():
    """kappa() is the measured constant wherever the summation structure allows more, and never above the worst case"""
    for n in (2, 7, 513, 16383, 16384, 20480, 200_000):
        for fam, world in (("rows", 1), ("sym", 1), ("cyclic", 8)):
            assert F.kappa(fam, n, world) <= F.kappa_worst(fam, n, world)
    assert F.kappa("rows", 16383) == F.KAPPA_ROWS and F.kappa("sym", 16384) == F.KAPPA_SYM
    assert F.kappa("cyclic", 16384, 2) == F.KAPPA_CYCLIC
