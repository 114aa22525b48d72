"""tests/_seq_model.py against the oracle, on any CPU: the model has to say what the reference says, bit for bit, before
tests/test_gpu_seq_forms.py holds every form of the SEQ force kernel to it."""
import math

import numpy as np
import pytest

from tests import _seq_model as M

NS = [1, 2, 7, 8, 9, 300, 701]
COORDS = ["clustered", 1.0, 30.0, 1e3, 1e16]
GEOMETRIES = [(1, 512), (2, 256), (4, 128), (8, 64), (16, 32), (32, 64)]   # (rows per wave, columns per batch) of the SEQ forms


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


def _coords(n, kind):
    return M.clustered(n, n + 1) if kind == "clustered" else M.uniform(n, n + int(kind) % 1000, kind)


def _sources(n, seed):
    """(name, full n x n float32 P) of the two probability sources: f32 rows, and u16 sums through a LUT (with a row map)"""
    rng = np.random.default_rng(seed)
    P = np.maximum(rng.random((n, n), dtype=np.float32), np.float32(1e-6))     # no p < 1e-10: see the loss test
    P[rng.random((n, n)) < 0.05] = 1.0
    lut = np.exp(-np.arange(3201) / 400.0).astype(np.float32)
    rowmap = np.cumsum(rng.random(n) < 0.6).astype(np.int64)
    rowmap -= rowmap[0]
    sums = rng.integers(0, 3201, size=(int(rowmap[-1]) + 1, n + 5), dtype=np.uint16)      # pitch > n
    return {"f32": (P, lambda rows: P[rows]),
            "lut": (lut[sums[rowmap, :n]], lambda rows: M.p_rows_lut(lut, sums, rows, n, rowmap))}


def _subsets(n):
    rng = np.random.default_rng(n)
    out = [np.arange(n)]
    if n > 2:
        out += [np.array([n - 1]), np.array([0, n - 2, n - 1]), np.sort(rng.choice(n, size=max(1, n // 5), replace=False))]
    return out


@pytest.mark.parametrize("kind", COORDS)
@pytest.mark.parametrize("n", NS)
def test_model_equals_oracle_bit_for_bit(O, n, kind):
    ld = _coords(n, kind)
    q = O.cal_ld_prob_mat(ld)
    for name, (P, p_of) in _sources(n, n + 11).items():
        want = O.gradient_loss(P, q, ld) / np.float32(4.0)
        assert want.dtype == np.float32
        for rows in _subsets(n):
            np.testing.assert_array_equal(M.q_rows(ld, rows).view(np.uint32), q[rows].view(np.uint32))
            got = M.grad_rows(ld, rows, p_of(rows))
            np.testing.assert_array_equal(got.view(np.uint32), want[:, rows].view(np.uint32), err_msg=f"{name} {len(rows)} rows")
    if n >= 300:
        assert np.abs(want).max() > 0


@pytest.mark.parametrize("kind", COORDS)
@pytest.mark.parametrize("n", NS)
def test_loss_rows_agrees_with_the_oracle(O, n, kind):
    """The oracle's cross_entropy rounds every term to float32 and adds the n x n terms (zeros included) with numpy's pairwise
    float32 sum; the model adds float64 terms.  With u = 2^-24, per term: two f32 logs (<= 2 ulp each), 1 - p, 1 - q, two
    products and a difference of terms of one sign, the final cast -- <= 9 u relative, all terms positive.  The pairwise sum of
    N = n^2 numbers: blocks of 128 added as 8 interleaved chains of 16 (<= 15 + 3 roundings) and log2(N / 128) levels above them.
    The final f32 * 2 is exact.  Bound: (9 + 18 + ceil(log2(N / 128)) + 1) u relative; the inputs have no p < 1e-10 (the oracle's eps
    branch, which the device does not have), and p = 1 changes a term by < 1e-10 * ln(1000) against a term >= 1e-3."""
    ld = _coords(n, kind)
    q = O.cal_ld_prob_mat(ld)
    for name, (P, p_of) in _sources(n, n + 12).items():
        assert P.min() >= 1e-10
        ref = float(O.cross_entropy(P, q)) / 2
        got = M.loss_rows(ld, np.arange(n), p_of(np.arange(n)))
        levels = max(0, math.ceil(math.log2(max(n * n, 128) / 128)))
        tol = (9 + 18 + levels + 1) * 2.0 ** -24
        print(f"n={n} {kind} {name}: model {got!r} oracle {ref!r} rel {abs(got - ref) / max(abs(ref), 1e-300):.3g} bound {tol:.3g}")
        assert abs(got - ref) <= tol * abs(ref), (name, got, ref)
        # a row subset is the sum of its rows
        if n > 2:
            a, b = np.arange(0, n, 2), np.arange(1, n, 2)
            parts = M.loss_rows(ld, a, p_of(a)) + M.loss_rows(ld, b, p_of(b))
            assert abs(parts - got) <= 1e-12 * abs(got)


@pytest.mark.parametrize("n", [2560, 4096])
def test_clustered_coordinates_mix_far_and_near_tiles(n):
    """a condition on the generator, not a measurement: at every geometry the GPU file runs, `clustered` gives both far tiles and
    tiles that divide, so that no case runs one class only"""
    ld = M.clustered(n, 3)
    for rw, cb in GEOMETRIES:
        s = M.far_share(ld, rw, cb)
        assert 0.3 <= s <= 0.9, (rw, cb, s)
    d2max = float(np.max((ld[0].astype(np.float64)[:, None] - ld[0]) ** 2))
    assert d2max > 1e30                                   # the generic-division class is present


def test_generator_edges():
    ld = M.clustered(300, 1)
    assert np.array_equal(ld[:, 4], ld[:, 5]) and 0 < np.abs(ld[:, 17] - ld[:, 16]).max() < 2e-4
    assert (np.abs(ld).max(axis=0) >= 2.4e15).sum() == 3
    assert M.clustered(1, 0).shape == (2, 1) and M.uniform(2, 0, 1.0).shape == (2, 2)


def test_row_sums_feel_every_term_on_clustered_coordinates():
    """the points at 1e16 would make every row sum the rounding noise of three terms of ~1e13 (blind to the order and the value of
    all other terms); with the clipped q as their probability the terms vanish.  Measured by a deliberately wrong sum order
    (adjacent columns swapped, what a lane mix-up in a kernel does): most rows change bits -- without the pinning none does."""
    n = 2561
    ld = M.clustered(n, 5)
    rng = np.random.default_rng(5)
    P = np.maximum(rng.random((n, n), dtype=np.float32), np.float32(1e-6))
    swap = np.arange(n - 1) ^ 1                            # columns (0, 1), (2, 3), ... swapped; the last column stays
    swap = np.concatenate([swap, [n - 1]])

    def changed(P):
        x, y = ld[0], ld[1]
        rows = np.arange(0, n, 7)
        dx, dy = x[rows, None] - x[None, :], y[rows, None] - y[None, :]
        q = np.maximum(np.minimum(np.float32(1) / (np.float32(1) + (dx * dx + dy * dy)), M.Q_HI), M.Q_LO)
        tx = (q / (np.float32(1) - q)) * (P[rows] - q) * dx
        tx[np.arange(len(rows)), rows] = 0
        a = np.cumsum(tx, axis=1, dtype=np.float32)[:, -1]
        np.testing.assert_array_equal(a.view(np.uint32), M.grad_rows(ld, rows, P[rows])[0].view(np.uint32))
        b = np.cumsum(tx[:, swap], axis=1, dtype=np.float32)[:, -1]
        return float((a.view(np.uint32) != b.view(np.uint32)).mean())

    blind = changed(P)
    P[:, M.huge_points(ld)] = M.Q_LO
    assert len(M.huge_points(ld)) == 3
    seeing = changed(P)
    print(f"rows whose bits change under a swapped order: {blind:.3f} without, {seeing:.3f} with the pinned probabilities")
    assert seeing > 0.5 and blind < 0.05           # measured: 0.61 and 0.00 (a swap of two terms need not change the rounded sum)
