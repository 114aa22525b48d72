"""motif_centrality on the GPU (csrc/pwm_sites.hip).  The yardstick is never the new kernel: it is the numpy
restatement of tests/_sites_model.py (per read the best window of tests/_readscore_model.py, the site reads reduced to the offset and
length histograms), and as a second witness the per-matrix device path DeviceSeq.read_scores(...).fetch() reduced the same way.
D, Hlen, n_sites and n_too_long are compared as equal integers; the verb's table field by field with the run on the model."""
from pathlib import Path

import numpy as np
import pytest

from tests import _readscore_model as M
from tests import _sites_model as S
from tests._batch_model import batches
from tests._refine_model import asym_matrix, make_reads, window_scores

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
LIB = ROOT / "tests" / "golden" / "library"


def check_against(got, want):
    """library_sites' result against np_library_sites'"""
    for g, w, what in zip(got, want, ("D", "Hlen", "n_sites", "n_too_long")):
        assert g.dtype == np.int64 and g.shape == w.shape, what
        np.testing.assert_array_equal(g, w, err_msg=what)
    np.testing.assert_array_equal(got[0].sum(axis=1), got[2])
    np.testing.assert_array_equal(got[1].sum(axis=1), got[2])


# ---- 1. read geometry -----------------------------------------------------------------------------------------------------------------
W_NAMES = (4, 9, 16, 31, "zero")


@pytest.fixture(scope="module")
def geometry():
    """~3000 reads on under 40 000 positions (fixed seed): lengths 0 .. 30 at random, so reads begin and end inside one group of 16
    positions and cross group boundaries; lengths w - 1, w, w + 1 of every width used; one read of 2100 bases, which spans a whole
    wave tile with no read start; 1200 reads of one base in a run (512 starts per tile); 2 % invalid bases, among them first bases
    of reads; n no multiple of 16.  The model's window scores per matrix are computed once."""
    from kmap_amd.motif_discovery import DeviceSeq
    rng = np.random.default_rng(1810)
    lengths = [int(x) for x in rng.integers(0, 31, 600)] + [0, 3, 4, 5, 8, 9, 10, 15, 16, 17, 30, 31, 32, 0]
    i_long = len(lengths)
    lengths += [2100] + [1] * 1200 + [int(x) for x in rng.integers(0, 31, 1150)] + [31] * 8 + [7, 8, 9, 33]
    if (sum(lengths) + len(lengths) - 1) % 16 == 0:
        lengths[-1] += 1
    seq, borders = make_reads(lengths, rng, frac_invalid=0.02, last_separator=False)
    n = len(seq)
    assert 2900 < len(borders) < 3100 and n < 40_000 and n % 16 != 0
    first_tile, last_tile = borders[i_long, 0] // 1024 + 1, (borders[i_long, 1] - 1) // 1024 - 1
    assert last_tile >= first_tile and not ((borders[:, 0] >= first_tile * 1024) & (borders[:, 0] < (first_tile + 1) * 1024)).any()
    ones = borders[i_long + 1:i_long + 1201, 0]
    tile = ones[0] // 1024 + 1
    assert ((ones >= tile * 1024) & (ones < (tile + 1) * 1024)).sum() == 512
    length = borders[:, 1] - borders[:, 0]
    inside_group = (length > 0) & (borders[:, 0] // 16 == (borders[:, 1] - 1) // 16)
    assert inside_group.sum() > 100 and ((length > 0) & ~inside_group).sum() > 100
    Ws = {w: asym_matrix(w, rng) for w in W_NAMES if w != "zero"}
    Ws["zero"] = np.zeros((4, 8), np.int32)                  # every window ties
    scored = {k: window_scores(seq, W) for k, W in Ws.items()}
    ds = DeviceSeq(seq, borders)
    yield ds, seq, borders, Ws, scored
    ds.close()


@pytest.mark.parametrize("revcom", [True, False])
def test_geometry_every_scorable_read_a_site(geometry, revcom):
    """t = the smallest score: every read with a valid window is a site read, and n_sites is library_histograms' n_scored"""
    ds, seq, borders, Ws, scored = geometry
    mats, sc = [Ws[k] for k in W_NAMES], [scored[k] for k in W_NAMES]
    ts = [M.score_range(W)[0] for W in mats]
    want = S.np_library_sites(seq, borders, mats, ts, revcom, scored=sc)
    got = ds.library_sites(mats, ts, revcom)
    check_against(got, want)
    assert got[0].shape == (5, 2 * 2100 + 1) and got[1].shape == (5, 2101) and not got[3].any()
    _, _, n_scored = ds.library_histograms(mats, ts, [M.score_range(W)[1] - t + 1 for W, t in zip(mats, ts)], revcom)
    np.testing.assert_array_equal(got[2], n_scored)
    assert got[2][0] > got[2][3] > 0                         # reads of 4 .. 30 bases are sites for the narrow matrix only
    assert got[1][3][31] > 0 and got[1][0][4] > 0 and got[1][4][2100] == 1      # L = w; the long read


@pytest.mark.parametrize("revcom", [True, False])
def test_tie_rule_across_lanes_and_tiles(geometry, revcom):
    """an all-zero matrix: every window ties, so the best loc of every scorable read must be its first valid window -- for the long
    read that is decided across the lanes of a tile and across tiles; then the same with the long read past max_len"""
    ds, seq, borders, Ws, scored = geometry
    valid = scored["zero"][0]
    L = borders[:, 1] - borders[:, 0]
    D = np.zeros(2 * 2100 + 1, np.int64)
    first_locs = []
    for (s, e), ln in zip(borders.tolist(), L.tolist()):
        v = np.nonzero(valid[s:max(e - 7, s)])[0]
        if len(v):
            first_locs.append(int(v[0]))
            D[2 * int(v[0]) + 8 - ln + 2100] += 1
    assert sum(x > 0 for x in first_locs) > 50               # reads whose first valid window is not at loc 0
    got = ds.library_sites([Ws["zero"]], [0], revcom)
    np.testing.assert_array_equal(got[0][0], D)
    check_against(got, S.np_library_sites(seq, borders, [Ws["zero"]], [0], revcom, scored=[scored["zero"]]))
    short = ds.library_sites([Ws["zero"]], [0], revcom, max_len=2000)
    check_against(short, S.np_library_sites(seq, borders, [Ws["zero"]], [0], revcom, 2000, scored=[scored["zero"]]))
    assert short[3].tolist() == [1] and short[2][0] == got[2][0] - 1 and short[0].shape == (1, 4001)


@pytest.mark.parametrize("revcom", [True, False])
def test_thresholds(geometry, revcom):
    from kmap_amd.pwm import pwm_threshold
    ds, seq, borders, Ws, scored = geometry
    mats, sc, ts = [], [], []
    for k in (4, 9, 16, 31):
        t_p, lo, hi = pwm_threshold(Ws[k], 1e-2)
        assert lo < t_p <= hi
        mats += [Ws[k]] * 3
        sc += [scored[k]] * 3
        ts += [lo, hi + 1, t_p]
    want = S.np_library_sites(seq, borders, mats, ts, revcom, scored=sc)
    got = ds.library_sites(mats, ts, revcom)
    check_against(got, want)
    assert not got[2][1::3].any() and not got[0][1::3].any()                     # t = hi + 1: nothing
    assert (got[2][2::3] < got[2][0::3]).all() and got[2][2::3][:2].all()        # p = 10^-2: fewer sites than reads, some for the narrow ones


# ---- 2. batching ----------------------------------------------------------------------------------------------------------------------
def test_batches_permutation_and_prefixes(geometry):
    from kmap_amd.pwm import pwm_threshold
    ds, seq, borders, _, _ = geometry
    rng = np.random.default_rng(1811)
    widths = [31, 5, 13, 8, 29, 4, 17, 6, 20, 7, 25, 4, 14, 28, 6, 19, 31, 16, 8]
    assert len(widths) == 19 and min(widths) == 4 and max(widths) == 31
    closed = batches(widths)
    assert len(closed) >= 3 and {"matrices", "chunks"} <= {why for _, why in closed}
    mats = [asym_matrix(w, rng) for w in widths]
    ts = [pwm_threshold(W, 1e-2)[0] if i % 2 else M.score_range(W)[0] for i, W in enumerate(mats)]
    want = S.np_library_sites(seq, borders, mats, ts, True)
    got = ds.library_sites(mats, ts, True)
    check_against(got, want)
    assert got[2].all()
    perm = rng.permutation(19)
    assert (perm != np.arange(19)).any()
    check_against(ds.library_sites([mats[i] for i in perm], [ts[i] for i in perm], True), tuple(a[perm] for a in want))
    for n in (1, 8, 9):
        check_against(ds.library_sites(mats[:n], ts[:n], True), tuple(a[:n] for a in want))
    check_against(ds.library_sites(mats[7:10], ts[7:10], False), S.np_library_sites(seq, borders, mats[7:10], ts[7:10], False))


# ---- 3. the two histogram forms -------------------------------------------------------------------------------------------------------
def test_block_private_and_global_bins_agree(geometry):
    ds, seq, borders, Ws, scored = geometry
    mats = [Ws[9], Ws["zero"], Ws[31]]
    ts = [M.score_range(W)[0] for W in mats]
    assert 3 * 2100 + 2 <= 32768 < 3 * 11_000 + 2
    small, big = ds.library_sites(mats, ts, True), ds.library_sites(mats, ts, True, max_len=11_000)
    assert big[0].shape == (3, 22_001) and big[1].shape == (3, 11_001)
    np.testing.assert_array_equal(big[0][:, 11_000 - 2100:11_000 + 2101], small[0])
    np.testing.assert_array_equal(big[1][:, :2101], small[1])
    assert not big[0][:, :11_000 - 2100].any() and not big[0][:, 11_000 + 2101:].any() and not big[1][:, 2101:].any()
    np.testing.assert_array_equal(big[2], small[2])
    check_against(big, S.np_library_sites(seq, borders, mats, ts, True, 11_000, scored=[scored[9], scored["zero"], scored[31]]))


# ---- 4. degenerate sizes, refused arguments -------------------------------------------------------------------------------------------
def test_degenerate_sizes_and_errors(geometry):
    from kmap_amd import _ffi
    ds, seq, borders, Ws, scored = geometry
    lib = _ffi.lib()
    W = Ws[9]
    t = M.score_range(W)[0]
    D, Hlen, sites, too_long = ds.library_sites([], [], True)
    assert D.shape == (0, 4201) and Hlen.shape == (0, 2101) and sites.shape == (0,) and too_long.shape == (0,)

    def call(widths, weights, n=ds.n, n_seq=ds.n_seq, max_len=10, codes=ds.codes.ptr, pos=True):
        wd, thr = np.array(widths, np.int32), np.array([t, t], np.int32)
        out = np.full((2, 21), 7, np.uint64), np.full((2, 11), 7, np.uint64), np.full(2, -5, np.int64), np.full(2, -5, np.int64)
        rc = lib.kmap_readscore_sites_library_dev(codes, ds.inval_orig.ptr, n, ds.borders.ptr, n_seq, len(widths), _ffi.ptr(wd), weights,
                                                  _ffi.ptr(thr), 1, max_len, _ffi.ptr(out[0]) if pos else None, _ffi.ptr(out[1]),
                                                  _ffi.ptr(out[2]), _ffi.ptr(out[3]), None)
        return rc, out

    def untouched(out):
        return (out[0] == 7).all() and (out[1] == 7).all() and (out[2] == -5).all() and (out[3] == -5).all()
    grid = np.zeros((2, 4, 32), np.int32)
    grid[:, :, :9] = W
    # no reads, no positions: zeros
    for kw in (dict(n_seq=0), dict(n=0)):
        rc, out = call([9, 9], _ffi.ptr(grid), **kw)
        assert rc == 0 and not any(a.any() for a in out)
    # reads longer than max_len = 10 are counted apart
    rc, out = call([9, 9], _ffi.ptr(grid))
    want = S.np_sites(seq, borders, W, t, True, 10, scored[9])
    assert rc == 0 and want[3] > 100
    for m in range(2):
        np.testing.assert_array_equal(out[0][m].astype(np.int64), want[0])
        np.testing.assert_array_equal(out[1][m].astype(np.int64), want[1])
        assert (int(out[2][m]), int(out[3][m])) == want[2:]
    # width 3 and 32, a weight behind the width or too large, null arrays, negative sizes: KMAP_E_INVAL naming the entry, nothing written
    for widths in ([3, 9], [9, 32]):
        rc, out = call(widths, _ffi.ptr(grid))
        assert rc == -1 and "readscore_sites_library" in _ffi.last_error() and f"width={3 if 3 in widths else 32}" in _ffi.last_error()
        assert untouched(out)
        with pytest.raises(ValueError, match="library_sites: .*width (3|32)"):
            ds.library_sites([np.zeros((4, w), np.int32) for w in widths], [0, 0], True)
    rc, out = call([8, 9], _ffi.ptr(grid))
    assert rc == -1 and "behind its width" in _ffi.last_error() and untouched(out)
    huge = grid.copy()
    huge[1, 2, 3] = 2 ** 31 // 31
    rc, out = call([9, 9], _ffi.ptr(huge))
    assert rc == -1 and "int32" in _ffi.last_error() and untouched(out)
    assert call([9, 9], None)[0] == -1 and call([9, 9], _ffi.ptr(grid), n=-1)[0] == -1 and call([9, 9], _ffi.ptr(grid), n_seq=-1)[0] == -1
    assert call([9, 9], _ffi.ptr(grid), codes=None)[0] == -1 and call([9, 9], _ffi.ptr(grid), pos=False)[0] == -1
    rc, out = call([9, 9], _ffi.ptr(grid), max_len=-1)
    assert rc == -1 and "max_len" in _ffi.last_error() and untouched(out)
    rc, out = call([9, 9], _ffi.ptr(grid), max_len=2 ** 20 + 1)
    assert rc == -4 and "2^20" in _ffi.last_error() and untouched(out)
    with pytest.raises(ValueError, match="2\\^20"):
        ds.library_sites([W], [t], True, max_len=2 ** 20 + 1)
    # and the next call is as good as the first
    check_against(ds.library_sites([W], [t], True), S.np_library_sites(seq, borders, [W], [t], True, scored=[scored[9]]))


def test_reads_that_only_exist_on_the_device(geometry):
    """reads handed over as device arrays, their lengths unknown to the host: max_len comes from the borders, fetched once"""
    from kmap_amd.motif_discovery import DeviceSeq
    ds, seq, borders, Ws, scored = geometry
    raw, bd = _buffers(seq, borders)
    twin = DeviceSeq.from_device(raw, len(seq), bd, len(borders))
    try:
        assert twin.read_len is None
        t = M.score_range(Ws[16])[0]
        check_against(twin.library_sites([Ws[16]], [t], True), S.np_library_sites(seq, borders, [Ws[16]], [t], True, scored=[scored[16]]))
        assert twin.read_len is not None and twin.max_read_len() == 2100
    finally:
        twin.close()
        bd.free()


def _buffers(seq, borders):
    from kmap_amd import _ffi
    return _ffi.DeviceBuffer.from_numpy(seq), _ffi.DeviceBuffer.from_numpy(np.ascontiguousarray(borders, np.int64))


# ---- 5. the second witness ------------------------------------------------------------------------------------------------------------
def test_against_the_per_matrix_device_path(geometry):
    from kmap_amd.pwm import pwm_threshold
    ds, seq, borders, Ws, _ = geometry
    mats = [Ws[4], Ws[16], Ws[31]]
    ts = [pwm_threshold(Ws[4], 1e-2)[0], M.score_range(Ws[16])[0], M.score_range(Ws[31])[0]]
    got = ds.library_sites(mats, ts, True)
    for m, (W, t) in enumerate(zip(mats, ts)):
        rs = ds.read_scores(W, True)
        try:
            score, loc, _ = rs.fetch()
        finally:
            rs.close()
        D, Hlen, n, too_long = S.sites_from_scores(score, loc, borders, W.shape[1], t, 2100)
        np.testing.assert_array_equal(got[0][m], D)
        np.testing.assert_array_equal(got[1][m], Hlen)
        assert (int(got[2][m]), int(got[3][m])) == (n, too_long) and n > 0


# ---- 6. the verb end to end -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("control", [False, True])
def test_verb_end_to_end(tmp_path, monkeypatch, capsys, control):
    """the seeded reads of tests/test_centrality_host.py: centrality_rank.csv of the run on the device equals, field by field, the
    one of the run through the model-backed DeviceSeq"""
    import kmap_amd.kmer_count as K
    import kmap_amd.motif_discovery as D
    from kmap_amd import centrality as C
    res, ctl, *_ = S.write_planted(tmp_path)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    lib = [str(LIB / "three.meme"), str(LIB / "mixed")]
    ctl = str(ctl) if control else None
    real = C._motif_centrality(str(res), lib, ctl, output_dir=str(tmp_path / "device"), top_hist=2)
    monkeypatch.setattr(D, "DeviceSeq", S.ModelSeq)
    monkeypatch.setattr(K, "encode_fasta", lambda path: M.encode_fasta_np(path))
    model = C._motif_centrality(str(res), lib, ctl, output_dir=str(tmp_path / "model"), top_hist=2)
    capsys.readouterr()
    a = (tmp_path / "device" / "centrality_rank.csv").read_text().split("\n")
    b = (tmp_path / "model" / "centrality_rank.csv").read_text().split("\n")
    cols = a[0].split(",")
    assert len(a) == len(b) == 6 and len(cols) == (21 if control else 18) and a[0] == b[0]
    for line_a, line_b in zip(a[1:], b[1:]):
        for name, x, y in zip(cols, line_a.split(","), line_b.split(",")):
            assert x == y, name
    assert a[1].split(",")[1] == "M1_CAATCGATAGC" and float(a[1].split(",")[cols.index("q_bh")]) < 0.01
    assert sorted(p.name for p in (tmp_path / "device").iterdir()) == sorted(p.name for p in (tmp_path / "model").iterdir())
    for p in (tmp_path / "device").iterdir():
        assert p.read_bytes() == (tmp_path / "model" / p.name).read_bytes(), p.name
    for x, y in zip(real, model):
        np.testing.assert_array_equal(x["D"], y["D"])
        np.testing.assert_array_equal(x["Hlen"], y["Hlen"])
