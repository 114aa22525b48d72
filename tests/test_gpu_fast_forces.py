"""The FAST force kernels (kmap_amd/csrc/embed_fast.hip) per element against the float64 oracle: |g - g64| <= kappa u M at every
checked coordinate (tests/_fast_check.py), on planted pairs at the positions where a tile, block, lane tail or shard edge can
drop or double one pair, on natural k-mer inputs, and at coordinate scales from 1e-3 to 1e16.  The loss against the float64
cross-entropy under a stated relative bound.  And the drop-in float operators at multi-block shapes."""
import functools

import numpy as np
import pytest

from tests import _fast_check as F

pytestmark = pytest.mark.gpu

# |loss - loss64| <= LOSS_REL |loss64|.  Every clamped pair (q = 1e-3) carries the f32 rounding of 1 - q (0.999 -> 0.99900001287):
# -1.29e-8 of its -ln(1 - q) = 1.0005e-3, a systematic -1.29e-5 relative for the background pairs of the planted inputs, which the
# reference's own f32 arithmetic shares.  The row kernel's one log2 per eight (1 - q) factors adds its own offset (see the
# measurements in DESIGN section 2).
LOSS_REL = 4e-5


def _ld(n):
    return (n + 7) // 8 * 8


def _sums_dev(pl, ld, rows, n_rows=None):
    """device uint16 sums [n_rows x ld] of the Planted `pl` for the global rows `rows` (rows past len(rows) stay zero)"""
    import torch
    n = pl.n
    rows = np.asarray(rows, np.int64)
    n_rows = len(rows) if n_rows is None else n_rows
    a = torch.as_tensor(pl.a, device="cuda")
    S = torch.zeros((max(n_rows, 1), ld), dtype=torch.int16, device="cuda")
    for c0 in range(0, len(rows), 4096):
        r = torch.as_tensor(rows[c0:c0 + 4096], device="cuda")
        S[c0:c0 + len(r), :n] = ((a[r, None] + a[None, :]) % len(F.BG_P)).to(torch.int16)
    pos = {int(r): t for t, r in enumerate(rows)}
    for (i, j), c in pl.code.items():
        if i in pos:
            S[pos[i], j] = c
        if j in pos:
            S[pos[j], i] = c
    torch.cuda.synchronize()
    return S


def _run(n, coords, src, ld, lut=None, row0=0, nrows=None, cyclic=None):
    """one FAST force evaluation -> (gradient [2, n] or message [2 n + MSG_EXTRA], loss or None)"""
    from kmap_amd import _ffi, visualization as V
    from kmap_amd.distributed import MSG_EXTRA
    sess = V.EmbedSession(n, 1, 0.01, V.EMBED_FAST, row0=row0, nrows=nrows, cyclic=cyclic)
    try:
        if lut is None:
            _ffi.check(_ffi.lib().kmap_embed_set_prob_f32(sess._h, src.data_ptr(), ld))
        else:
            lut = np.ascontiguousarray(lut, np.float32)
            _ffi.check(_ffi.lib().kmap_embed_set_prob_lut(sess._h, src.data_ptr(), ld, _ffi.ptr(lut), len(lut)))
        sess.set_coords(coords)
        if cyclic is not None:
            m_d = _ffi.DeviceBuffer((2 * n + MSG_EXTRA) * 4)
            m_d.zero()
            sess.forces_msg(m_d.ptr)
            _ffi.sync()
            out = m_d.to_numpy(np.float32, (2 * n + MSG_EXTRA,)), None
            m_d.free()
            return out
        g_d, l_d = _ffi.DeviceBuffer(2 * n * 4), _ffi.DeviceBuffer(8)
        g_d.zero()
        sess.forces(g_d.ptr, l_d.ptr)
        _ffi.sync()
        out = g_d.to_numpy(np.float32, (2, n)), float(l_d.to_numpy(np.float64, (1,))[0])
        g_d.free()
        l_d.free()
        return out
    finally:
        sess.close()


@functools.lru_cache(maxsize=None)
def _planted(n, extra=()):
    pl = F.Planted(n, F.structural_pairs(n, extra), seed=n % 9973)
    return pl


@functools.lru_cache(maxsize=None)
def _loss64(n, extra=()):
    pl = _planted(n, extra)
    return F.total_loss64(pl.p_rows, n, pl.coords)


def _report(family, n, tag, r, power=None, loss_rel=None):
    extra = (f" power={power:.0f}" if power is not None else "") + (f" loss_rel={loss_rel:.3e}" if loss_rel is not None else "")
    print(f"FASTCHECK {family} n={n} {tag} err/(uM)={r:.3f}{extra}")


def _check_planted(family, kappa, n, g, pl, rows=None, tag=""):
    rows = F.check_rows(n, planted=pl) if rows is None else rows
    g64, M, _ = F.reference(pl, rows, pl.coords)
    r = F.assert_forces_close(g[:, rows], g64, M, kappa, rows, f"{family} n={n} {tag}")
    power = pl.assert_visible(rows, M, kappa)
    return r, power


# ---- row-wise kernel ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 7, 63, 64, 65, 511, 512, 513, 1000, 4099, 16383])
@pytest.mark.parametrize("source", ["lut", "f32"])
def test_row_kernel_planted_pairs(n, source):
    """forces_fast_kernel (n < 16 384) with the u16 sums + LUT source and the f32 matrix source (LUTSRC = false, umap()'s)"""
    import torch
    pl = _planted(n)
    ld = _ld(n) if source == "lut" else n + (n % 2)        # f32 rows: also a pitch that is no multiple of 8
    S = _sums_dev(pl, ld, np.arange(n))
    if source == "f32":
        src = torch.as_tensor(pl.lut, device="cuda")[S.long()]
        g, loss = _run(n, pl.coords, src, ld)
    else:
        g, loss = _run(n, pl.coords, S, ld, lut=pl.lut)
    r, power = _check_planted("rows", F.kappa("rows", n), n, g, pl, tag=source) if pl.pairs else (0.0, None)
    if not pl.pairs:
        rows = np.arange(n)
        g64, M, _ = F.reference(pl, rows, pl.coords)
        r = F.assert_forces_close(g, g64, M, F.kappa("rows", n), rows, f"rows n={n}")
    L64 = _loss64(n)
    rel = abs(loss - L64) / L64
    _report("rows", n, source, r, power, rel)
    assert rel <= LOSS_REL, (loss, L64)


def test_row_kernel_loss_resolves_one_pair():
    """at n = 1000 and 4099 one planted pair's cross-entropy stands >= 10x above the loss bound"""
    for n in (1000, 4099):
        pl = _planted(n)
        assert pl.pair_ce().max() >= 10 * LOSS_REL * _loss64(n), (n, pl.pair_ce().max(), _loss64(n))


@pytest.mark.parametrize("n", [16384, 20480])
def test_row_kernel_forced_at_large_n(n, monkeypatch):
    """KMAP_EMBED_SYM=0: the row-wise kernel where the symmetric one would run"""
    monkeypatch.setenv("KMAP_EMBED_SYM", "0")
    pl = _planted(n)
    S = _sums_dev(pl, _ld(n), np.arange(n))
    g, loss = _run(n, pl.coords, S, _ld(n), lut=pl.lut)
    r, power = _check_planted("rows", F.kappa("rows", n), n, g, pl, tag="sym=0")
    rel = abs(loss - _loss64(n)) / _loss64(n)
    _report("rows", n, "sym=0", r, power, rel)
    assert rel <= LOSS_REL


@pytest.mark.parametrize("n,row0,nrows", [(4099, 0, 1001), (4099, 1001, 2047), (4099, 3048, 1051), (20480, 7777, 12703)])
def test_row_sharded_session(n, row0, nrows):
    """a row-sharded session (row0, nrows), odd nrows: the clamped duplicate row of F_RPW = 2 is discarded, the last row is
    computed; other rows stay untouched"""
    last = row0 + nrows - 1
    extra = ((last, 17 if last > 40 else n - 30), (row0, row0 + nrows + 5))
    pl = _planted(n, extra)
    assert (last, 17 if last > 40 else n - 30) in pl.pairs or (17, last) in pl.pairs
    S = _sums_dev(pl, _ld(n), np.arange(row0, row0 + nrows))
    g, _ = _run(n, pl.coords, S, _ld(n), lut=pl.lut, row0=row0, nrows=nrows)
    assert not g[:, :row0].any() and not g[:, row0 + nrows:].any()
    rows = F.check_rows(n, planted=pl, rows_extra=[row0, row0 + 1, last - 1, last])
    rows = rows[(rows >= row0) & (rows <= last)]
    g64, M, _ = F.reference(pl, rows, pl.coords)
    r = F.assert_forces_close(g[:, rows], g64, M, F.kappa("rows", n), rows, f"rows shard {row0}+{nrows}")
    pos = {int(x): t for t, x in enumerate(rows)}
    inside = [(i, j) for i, j in pl.pairs if i in pos and j in pos]
    assert any(last in p for p in inside) or any(last in p for p in pl.pairs)
    _report("rows", n, f"shard{row0}+{nrows}", r)


# ---- symmetric kernel ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,ld", [(16384, 16384), (16385, 16392), (16384 + 255, 16640), (16384 + 3 * 256 + 77, 17232),
                                  (16384 + 3 * 256 + 77, 17230), (20480, 20480)])
def test_sym_kernel_planted_pairs(n, ld):
    """forces_sym2_kernel + sym_reduce_kernel: interior tiles, diagonal tiles, the right-edge tile, the ragged bottom block; a
    pitch that is no multiple of 8 sends every tile through the masked path"""
    pl = _planted(n)
    S = _sums_dev(pl, ld, np.arange(n))
    g, loss = _run(n, pl.coords, S, ld, lut=pl.lut)
    r, power = _check_planted("sym", F.kappa("sym", n), n, g, pl, tag=f"ld={ld}")
    rel = abs(loss - _loss64(n)) / _loss64(n)
    _report("sym", n, f"ld={ld}", r, power, rel)
    assert rel <= LOSS_REL


@pytest.mark.parametrize("world", [2, 3, 5, 8])
def test_cyclic_shards_planted_pairs(world):
    """kmap_embed_create_cyclic: each rank's session in turn, messages summed in f32 in rank order (the all-reduce); the gradient
    per element and the loss decoded from the limbs against float64; every rank owns planted rows"""
    from kmap_amd import visualization as V
    from kmap_amd.distributed import MSG_EXTRA, loss_from_limbs
    n = 16384 + 3 * 256 + 77
    ld = _ld(n)
    pl = _planted(n)
    owners = {(i // 256) % world for p in pl.pairs for i in p}
    assert owners == set(range(world))
    msum = np.zeros(2 * n + MSG_EXTRA, np.float32)
    for rank in range(world):
        blocks = V.cyclic_blocks(n, world, rank)
        rows = np.concatenate([np.arange(r0, r0 + 256) for r0, _ in blocks])
        rows = np.where(rows < n, rows, -1)
        S = _sums_dev(pl, ld, rows[rows >= 0], n_rows=len(rows))
        m, _ = _run(n, pl.coords, S, ld, lut=pl.lut, cyclic=(world, rank))
        msum = msum + m
        del S
    g = msum[:2 * n].reshape(2, n)
    r, power = _check_planted("cyclic", F.kappa("cyclic", n, world), n, g, pl, tag=f"world={world}")
    rel = abs(loss_from_limbs(msum[2 * n:]) - _loss64(n)) / _loss64(n)
    _report("cyclic", n, f"world={world}", r, power, rel)
    assert rel <= LOSS_REL


def test_cyclic_one_block_per_rank_and_too_few_blocks():
    """world = 8 over exactly 8 row blocks (the last one ragged) works; fewer blocks than ranks is refused at create"""
    from kmap_amd import _ffi, visualization as V
    from kmap_amd.distributed import MSG_EXTRA
    n, world = 7 * 256 + 77, 8
    pl = _planted(n)
    msum = np.zeros(2 * n + MSG_EXTRA, np.float32)
    for rank in range(world):
        (r0, nr), = V.cyclic_blocks(n, world, rank)
        rows = np.arange(r0, r0 + nr)
        S = _sums_dev(pl, _ld(n), rows, n_rows=256)
        m, _ = _run(n, pl.coords, S, _ld(n), lut=pl.lut, cyclic=(world, rank))
        msum = msum + m
    r, power = _check_planted("cyclic", F.kappa("cyclic", n, world), n, msum[:2 * n].reshape(2, n), pl, tag="world=8 one block")
    _report("cyclic", n, "one-block", r, power)
    for n_bad in (1, 7 * 256):
        with pytest.raises(ValueError, match="row blocks"):
            V.EmbedSession(n_bad, 1, 0.01, V.EMBED_FAST, cyclic=(world, world - 1))


# ---- natural inputs and coordinate scales -------------------------------------------------------------------------------------
def _scaled_coords(n, scale, seed):
    rng = np.random.default_rng(seed)
    y = rng.standard_normal((2, n)) * scale
    if scale <= 1e-3:
        y[:, 1::5] = y[:, 0::5][:, :y[:, 1::5].shape[1]]                # coincident points
    # pairs at d2 just inside / outside both clamp edges (1/999 and 999)
    edges = [(1 / 999) * (1 - 2e-6), (1 / 999) * (1 + 2e-6), 999 * (1 - 2e-6), 999 * (1 + 2e-6)]
    for t, d2 in enumerate(edges):
        i, j = 3 + 7 * t, 4 + 7 * t
        if j < n:
            y[:, j] = y[:, i] + np.sqrt(d2 / 2)
    return y.astype(np.float32)


@pytest.mark.parametrize("scale", [1e-3, 1.0, 30.0, 1e3, 1e16])
@pytest.mark.parametrize("n", [1000, 16385])
def test_coordinate_scales(n, scale):
    """random coordinates (coincident points at 1e-3, squared distances past 1e30 at 1e16, pairs next to both clamp edges)"""
    pl = _planted(n)
    coords = _scaled_coords(n, scale, 11)
    S = _sums_dev(pl, _ld(n), np.arange(n))
    g, _ = _run(n, coords, S, _ld(n), lut=pl.lut)
    rows = F.check_rows(n, rows_extra=range(0, 40))
    g64, M, _ = F.reference(pl, rows, coords)
    fam, kappa = ("rows", F.kappa("rows", n)) if n < 16384 else ("sym", F.kappa("sym", n))
    r = F.assert_forces_close(g[:, rows], g64, M, kappa, rows, f"{fam} n={n} scale={scale}")
    _report(fam, n, f"scale={scale:g}", r)


@pytest.mark.parametrize("n", [1000, 20000])
def test_natural_kmer_inputs(n, monkeypatch):
    """the k-mer neighbour sums and normal coordinates of test_symmetric_fast_kernel_matches_seq_per_step: row-wise and (n =
    20 000) symmetric kernel per element"""
    from kmap_amd import _ffi, visualization as V
    from kmap_amd.hamdist import hamdist_matrix_dev, pitch_for
    rng = np.random.default_rng(3)
    k = 8
    kh = rng.integers(0, 4 ** k, size=n, dtype=np.uint64).astype(np.uint32)
    lab = np.zeros(n, np.int32)
    ldd = pitch_for(n)
    kh_d, lab_d = _ffi.DeviceBuffer.from_numpy(kh), _ffi.DeviceBuffer.from_numpy(lab)
    D_d = _ffi.DeviceBuffer(n * ldd)
    hamdist_matrix_dev(kh_d.ptr, lab_d.ptr, n, k, [k], D_d.ptr, ldd)
    nb_d = V.knn_select_dev(D_d.ptr, ldd, n, 20)
    lut = V.hd_prob_lut(k, 20, 400 * k)
    coords = rng.standard_normal((2, n)).astype(np.float32)
    sums_d, lds = V.knn_sums_dev(D_d.ptr, ldd, nb_d, n, 20)
    rows = F.check_rows(n)

    def p_rows(rr):
        return np.stack([lut[sums_d.to_numpy(np.uint16, (lds,), offset=int(r) * lds * 2)[:n]] for r in rr])

    g64, M, _ = F.reference(p_rows, rows, coords)
    for sym in (("1", "0") if n >= 16384 else ("1",)):
        monkeypatch.setenv("KMAP_EMBED_SYM", sym)
        sess = V.EmbedSession(n, 1, 0.01, V.EMBED_FAST)
        _ffi.check(_ffi.lib().kmap_embed_set_prob_lut(sess._h, sums_d.ptr, lds, _ffi.ptr(lut), len(lut)))
        sess.set_coords(coords)
        g_d = _ffi.DeviceBuffer(2 * n * 4)
        sess.forces(g_d.ptr)
        _ffi.sync()
        g = g_d.to_numpy(np.float32, (2, n))
        sess.close()
        g_d.free()
        fam, kappa = ("sym", F.kappa("sym", n)) if (n >= 16384 and sym == "1") else ("rows", F.kappa("rows", n))
        r = F.assert_forces_close(g[:, rows], g64, M, kappa, rows, f"{fam} natural n={n}")
        _report(fam, n, "natural", r)
    for b in (sums_d, D_d, nb_d, kh_d, lab_d):
        b.free()


# ---- drop-in float operators --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 257, 1000, 3001])
def test_dropin_operators_multi_block(n):
    """cal_ld_prob_mat_taichi / gradient_loss_taichi bit for bit against the oracle, cross_entropy_taichi within one f32 ulp of
    the float64 sum of the oracle's f32 terms (the device sums in f64 and rounds once)"""
    from kmap_amd import visualization as V
    from oracle import oracle as O
    rng = np.random.default_rng(n)
    ld = (rng.standard_normal((2, n)) * 2).astype(np.float32)
    if n > 4:
        ld[:, 3] = ld[:, 2]                                            # coincident: q clipped to 0.999
    q = V.cal_ld_prob_mat_taichi(ld)
    np.testing.assert_array_equal(q.view(np.uint32), O.cal_ld_prob_mat(ld).view(np.uint32))
    p = rng.random((n, n)).astype(np.float32) * 0.5
    p[rng.random((n, n)) < 0.3] = 0.0
    p[rng.random((n, n)) < 0.02] = 1.0
    g = V.gradient_loss_taichi(p, q, ld)
    np.testing.assert_array_equal(g.view(np.uint32), O.gradient_loss(p, q, ld).view(np.uint32))
    loss = V.cross_entropy_taichi(p, q)
    eps, one = np.float32(1e-10), np.float32(1)
    qq = np.where(q < eps, eps, np.where(q > one - eps, one - eps, q)).astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        full = -p * np.log(qq) - (one - p) * np.log(one - qq)
        ce = np.where(p < eps, -np.log(one - qq), np.where(p > one - eps, -np.log(qq), full)).astype(np.float32)
    want = np.float32(2.0 * np.triu(ce, 1).astype(np.float64).sum())
    assert abs(int(np.float32(loss).view(np.int32)) - int(want.view(np.int32))) <= 1, (loss, want)
    if n == 1:
        assert loss == 0.0


@pytest.mark.parametrize("n,n_nb", [(300, 1), (300, 7), (1000, 33), (3001, 7)])
def test_knn_smooth_f32_matrix_multi_block(n, n_nb):
    from kmap_amd import visualization as V
    from oracle import oracle as O
    rng = np.random.default_rng(n + n_nb)
    x = rng.standard_normal((n, 3))
    D = np.sqrt(((x[:, None] - x[None]) ** 2).sum(-1))
    nb = np.argpartition(D, n_nb, axis=1)[:, :n_nb]
    np.testing.assert_array_equal(V.knn_smooth(D, n_nb, neighbor_inds_mat=nb), O.knn_smooth(D, n_nb, nb=nb))
