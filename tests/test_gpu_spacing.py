"""motif_spacing on the GPU (csrc/pwm_spacing.hip).  The yardstick is never the new kernel: it is the numpy
restatement of tests/_spacing_model.py (the primary's best window per read from tests/_readscore_model.py, section 11's hits of every
other matrix, per primary read the best hit that does not overlap the primary window, the pair reads reduced to the gap and room
histograms), and as a second witness the hit lists of DeviceSeq.scan_pwm -- another kernel -- reduced the same way with the fetched
read_scores of the primary.  S, R, n_primary, n_pair and n_far are compared as equal integers; the verb's files byte for byte with
the run on the model."""
from pathlib import Path

import numpy as np
import pytest

from tests import _readscore_model as M
from tests import _spacing_model as S
from tests._batch_model import batches
from tests._refine_model import asym_matrix, make_reads, window_scores

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
WP = 9                                                       # the primary matrix's width in the geometry tests


def check_against(got, want):
    """library_spacing's result against np_library_spacing's, and the invariants of definition 4"""
    for g, w, what in zip(got, want, ("S", "R", "n_primary", "n_pair", "n_far")):
        if what == "n_primary":
            assert isinstance(g, int) and g == w, what
            continue
        assert g.dtype == np.int64 and g.shape == w.shape, what
        np.testing.assert_array_equal(g, w, err_msg=what)
    np.testing.assert_array_equal(got[0].sum(axis=(1, 2)), got[3] - got[4])
    np.testing.assert_array_equal(got[1].sum(axis=(1, 2)), got[3] - got[4])
    assert (got[3] <= got[2]).all() and not got[1][:, 0, 0].any()


class Primary:
    """the ReadScores of a primary matrix, kept for the tests of one module"""

    def __init__(self, ds, seq, borders, W):
        self.W, self.scored = W, window_scores(seq, W)
        self.lo, self.hi = M.score_range(W)
        self.rs = {rc: ds.read_scores(W, rc) for rc in (True, False)}

    def close(self):
        for rs in self.rs.values():
            rs.close()


# ---- 1. read geometry -----------------------------------------------------------------------------------------------------------------
W_NAMES = (4, 9, 16, 31, "primary")


@pytest.fixture(scope="module")
def geometry():
    """~3000 reads on under 60 000 positions (fixed seed): lengths 0 .. 60 at random, so reads begin and end inside one group of 16
    positions and cross group boundaries and hold from none to many windows beside the primary one; lengths wP + w - 1, wP + w and
    wP + w + 1 of every width used (no room, room for exactly one window at gap 0, for two); one read of 2100 bases, whose primary
    and secondary windows lie in different lanes and tiles and which spans a tile with no read start; 1200 reads of one base in a
    run; empty reads that share their start with the read behind them; 2 % invalid bases; n no multiple of 16.  The model's window
    scores per matrix are computed once."""
    from kmap_amd.motif_discovery import DeviceSeq
    rng = np.random.default_rng(1910)
    edge = [WP + w + x for w in (4, 9, 16, 31) for x in (-1, 0, 1)]
    lengths = [int(x) for x in rng.integers(0, 61, 700)] + edge * 3
    i_long = len(lengths)
    lengths += [2100] + [1] * 1200 + [int(x) for x in rng.integers(0, 61, 950)] + edge * 3 + [7, 8, 9, 33]
    if (sum(lengths) + len(lengths) - 1) % 16 == 0:
        lengths[-1] += 1
    seq, borders = make_reads(lengths, rng, frac_invalid=0.02, last_separator=False)
    # empty reads in front of reads 5, 6 (two of them), 900 and the long one: they start where that read starts
    at = [5, 6, 6, 900, i_long]
    borders = np.insert(borders, at, np.stack([borders[at, 0], borders[at, 0]], axis=1), axis=0)
    i_long = int(np.nonzero(borders[:, 1] - borders[:, 0] == 2100)[0][0])
    n = len(seq)
    assert 2900 < len(borders) < 3100 and n < 60_000 and n % 16 != 0 and (np.diff(borders[:, 0]) >= 0).all()
    assert (np.diff(borders[:, 0]) == 0).sum() == 5
    first_tile, last_tile = borders[i_long, 0] // 1024 + 1, (borders[i_long, 1] - 1) // 1024 - 1
    assert last_tile >= first_tile and not ((borders[:, 0] >= first_tile * 1024) & (borders[:, 0] < (first_tile + 1) * 1024)).any()
    rng = np.random.default_rng(1911)
    Ws = {w: asym_matrix(w, rng) for w in (4, 9, 16, 31)}
    ds = DeviceSeq(seq, borders)
    prim = Primary(ds, seq, borders, asym_matrix(WP, rng))
    Ws["primary"] = prim.W
    scored = {k: window_scores(seq, W) for k, W in Ws.items() if k != "primary"}
    scored["primary"] = prim.scored
    yield ds, seq, borders, Ws, scored, prim, i_long
    prim.close()
    ds.close()


def model(geometry, tP, names, ts, revcom, G):
    ds, seq, borders, Ws, scored, prim, _ = geometry
    return S.np_library_spacing(seq, borders, prim.W, tP, [Ws[k] for k in names], ts, revcom, G, prim.scored, [scored[k] for k in names])


@pytest.mark.parametrize("revcom", [True, False])
def test_geometry_every_scorable_read_a_primary_read(geometry, revcom):
    """both thresholds at the smallest score: every read with a valid primary window is a primary read and every valid window that
    does not overlap it a candidate; the primary matrix is also a secondary one, which needs a second, non-overlapping site"""
    ds, seq, borders, Ws, scored, prim, i_long = geometry
    mats = [Ws[k] for k in W_NAMES]
    ts = [M.score_range(W)[0] for W in mats]
    G = 20
    want = model(geometry, prim.lo, W_NAMES, ts, revcom, G)
    got = ds.library_spacing(prim.rs[revcom], WP, prim.lo, mats, ts, revcom, G)
    check_against(got, want)
    Sg, R, n_primary, n_pair, n_far = got
    assert Sg.shape == (5, 4, G + 1) and R.shape == (5, G + 2, G + 2)
    assert n_primary == prim.rs[revcom].n_scored and n_pair[0] > n_pair[1] > n_pair[3] > 0 and n_far.all()
    assert 0 < n_pair[4] < n_pair[1] + 200                   # the primary matrix against itself: reads with two sites
    # windows that touch the primary window on either side, and windows as far as G
    for m in range(3):
        assert Sg[m, 0, 0] + Sg[m, 1, 0] > 0 and Sg[m, 2, 0] + Sg[m, 3, 0] > 0 and Sg[m, :, G].sum() > 0
    assert (Sg[:, 1].any() and Sg[:, 3].any()) if revcom else not (Sg[:, 1].any() or Sg[:, 3].any())
    # reads with room for one window only: rooms (0, 1) and (1, 0)
    assert R[0, 0, 1] > 0 and R[0, 1, 0] > 0 and R[0, G + 1, G + 1] > 0
    # the long read alone, from the model: its two windows lie in different lanes of different tiles
    score, loc, strand = M.np_read_scores(seq, borders, prim.W, revcom, prim.scored)
    other_lane = other_tile = 0
    for k, t in zip((4, 9, 16, 31), ts):
        r, l, p, sc, _ = S.np_hits(seq, borders, Ws[k], t, revcom, scored[k])
        free = (r == i_long) & ((l + k <= loc[i_long]) | (l >= loc[i_long] + WP))
        best = l[free][np.lexsort((l[free], -sc[free]))[0]]
        other_lane += (borders[i_long, 0] + best) // 16 != (borders[i_long, 0] + loc[i_long]) // 16
        other_tile += (borders[i_long, 0] + best) // 1024 != (borders[i_long, 0] + loc[i_long]) // 1024
    assert other_lane == 4 and other_tile >= 2


@pytest.mark.parametrize("revcom", [True, False])
def test_thresholds(geometry, revcom):
    """primary thresholds lo, p = 10^-2 and hi + 1 (no primary read: everything zero) against secondary thresholds lo, hi + 1 and
    p = 10^-2 for every width"""
    from kmap_amd.pwm import pwm_threshold
    ds, seq, borders, Ws, scored, prim, _ = geometry
    names, ts = [], []
    for k in (4, 9, 16, 31):
        t_p, lo, hi = pwm_threshold(Ws[k], 1e-2)
        assert lo < t_p <= hi
        names += [k] * 3
        ts += [lo, hi + 1, t_p]
    mats = [Ws[k] for k in names]
    tP_p = pwm_threshold(prim.W, 1e-2)[0]
    assert prim.lo < tP_p <= prim.hi
    seen = []
    for tP in (prim.lo, tP_p, prim.hi + 1):
        want = model(geometry, tP, names, ts, revcom, 150)
        got = ds.library_spacing(prim.rs[revcom], WP, tP, mats, ts, revcom)      # max_gap 150 is the default
        check_against(got, want)
        assert got[0].shape == (12, 4, 151) and got[1].shape == (12, 152, 152)
        assert not got[3][1::3].any() and not got[0][1::3].any()                  # t = hi + 1: no secondary site
        seen.append((got[2], got[3]))
    assert seen[0][0] > seen[1][0] > 0 and seen[2][0] == 0 and not seen[2][1].any()
    assert (seen[1][1][0::3] < seen[0][1][0::3]).all() and seen[1][1][0] > 0 and seen[0][1][2] > 0


@pytest.mark.parametrize("revcom", [True, False])
def test_tie_rule_and_exclusion_edges(geometry, revcom):
    """all-zero primary and secondary matrices: every window ties, so the primary site is the read's first valid window of 9 and the
    secondary site the first valid window of 8 that does not overlap it -- one that ends at or before the primary's first base if
    there is any, else the first one at or behind its last base.  Stated here without the model."""
    ds, seq, borders, _, _, _, i_long = geometry
    ZP, Z = np.zeros((4, 9), np.int32), np.zeros((4, 8), np.int32)
    valid9, valid8 = window_scores(seq, ZP)[0], window_scores(seq, Z)[0]
    G = 150
    Sx, Rx = np.zeros((4, G + 1), np.int64), np.zeros((G + 2, G + 2), np.int64)
    n_primary = n_pair = n_far = touching = 0
    for s, e in borders.tolist():
        v9 = np.nonzero(valid9[s:max(e - 8, s)])[0]
        if len(v9) == 0:
            continue
        n_primary += 1
        p, L = int(v9[0]), e - s
        v8 = np.nonzero(valid8[s:max(e - 7, s)])[0]
        free = [int(x) for x in v8 if x + 8 <= p or x >= p + 9]
        if not free:
            continue
        n_pair += 1
        loc = free[0]
        g = p - loc - 8 if loc < p else loc - p - 9
        touching += g == 0
        if g > G:
            n_far += 1
            continue
        Sx[0 if loc < p else 2, g] += 1                      # every tie is '+': upstream is left, the strands are the same
        Rx[min(max(p - 7, 0), G + 1), min(max(L - p - 16, 0), G + 1)] += 1
    assert n_pair > 500 and touching > 300 and Sx[0].sum() > 5 and Sx[2, 1:].sum() > 5
    rs = ds.read_scores(ZP, revcom)
    try:
        got = ds.library_spacing(rs, 9, 0, [Z], [0], revcom, G)
        np.testing.assert_array_equal(got[0][0], Sx)
        np.testing.assert_array_equal(got[1][0], Rx)
        assert (got[2], int(got[3][0]), int(got[4][0])) == (n_primary, n_pair, n_far)
        want = S.np_library_spacing(seq, borders, ZP, 0, [Z], [0], revcom, G)
        check_against(got, want)
        check_against(ds.library_spacing(rs, 9, 0, [Z], [0], revcom, 0), S.np_library_spacing(seq, borders, ZP, 0, [Z], [0], revcom, 0))
    finally:
        rs.close()


# ---- 2. the largest gap ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gap_reads():
    """for every G of (0, 5, 150, 511) four reads of 1100 random bases with the primary consensus planted forward at loc 540 and
    the partner's consensus forward exactly G and G + 1 bases to its right, and exactly G and G + 1 bases to its left"""
    from kmap_amd.motif_discovery import DeviceSeq
    from kmap_amd.pwm import pwm_weights
    rng = np.random.default_rng(1912)
    seq, borders = make_reads([1100] * 16, rng, frac_invalid=0.0)
    wP, w = len(S.PRIMARY), len(S.UNIFORM)
    planted = []
    for i, (G, right, extra) in enumerate((G, right, extra) for G in (0, 5, 150, 511) for right in (True, False) for extra in (0, 1)):
        s, g = int(borders[i, 0]), G + extra
        at = 540 + wP + g if right else 540 - g - w
        assert 0 <= at and at + w <= 1100
        seq[s + 540:s + 540 + wP] = S._codes(S.PRIMARY, False)
        seq[s + at:s + at + w] = S._codes(S.UNIFORM, False)
        planted.append((g, right))
    W_P, W = pwm_weights(S.consensus_counts(S.PRIMARY), 1.0), pwm_weights(S.consensus_counts(S.UNIFORM), 1.0)
    ds = DeviceSeq(seq, borders)
    rs = ds.read_scores(W_P, True)
    yield ds, rs, seq, borders, W_P, W, planted
    rs.close()
    ds.close()


@pytest.mark.parametrize("G", [0, 5, 150, 511])
def test_gap_exactly_max_gap_and_one_more(gap_reads, G):
    ds, rs, seq, borders, W_P, W, planted = gap_reads
    tP, t = M.score_range(W_P)[1], M.score_range(W)[1]      # the consensus itself and nothing else
    got = ds.library_spacing(rs, W_P.shape[1], tP, [W], [t], True, G)
    check_against(got, S.np_library_spacing(seq, borders, W_P, tP, [W], [t], True, G))
    Sg, R, n_primary, n_pair, n_far = got
    assert n_primary == 16 and n_pair[0] == 16
    near = [(g, right) for g, right in planted if g <= G]
    assert n_far[0] == 16 - len(near) and ((G, True) in near) and ((G, False) in near) and ((G + 1, True) in planted)
    want = np.zeros((4, G + 1), np.int64)
    for g, right in near:
        want[2 if right else 0, g] += 1                      # a '+' primary: downstream is right; both sites forward
    np.testing.assert_array_equal(Sg[0], want)
    assert Sg[0][0, G] >= 1 and Sg[0][2, G] >= 1 and n_far[0] >= 2
    assert R[0].sum() == len(near) and R[0][min(540 - 10 + 1, G + 1), min(1100 - 540 - 11 - 10 + 1, G + 1)] == len(near)


# ---- 3. batching ----------------------------------------------------------------------------------------------------------------------
def test_batches_permutation_and_prefixes(geometry):
    from kmap_amd.pwm import pwm_threshold
    ds, seq, borders, _, _, prim, _ = geometry
    rng = np.random.default_rng(1913)
    widths = [31, 5, 13, 8, 29, 4, 17, 6, 20, 7, 25, 4, 14, 28, 6, 19, 31, 16, 8]
    assert len(widths) == 19 and min(widths) == 4 and max(widths) == 31
    closed = batches(widths)
    assert len(closed) >= 3 and {"matrices", "chunks"} <= {why for _, why in closed}
    mats = [asym_matrix(w, rng) for w in widths]
    ts = [pwm_threshold(W, 1e-2)[0] if i % 2 else M.score_range(W)[0] for i, W in enumerate(mats)]
    G = 5
    want = S.np_library_spacing(seq, borders, prim.W, prim.lo, mats, ts, True, G, prim.scored)
    got = ds.library_spacing(prim.rs[True], WP, prim.lo, mats, ts, True, G)
    check_against(got, want)
    assert got[3][0::2].all() and got[4][0::2].all()
    perm = rng.permutation(19)
    assert (perm != np.arange(19)).any()

    def pick(res, idx):
        return res[0][idx], res[1][idx], res[2], res[3][idx], res[4][idx]
    check_against(ds.library_spacing(prim.rs[True], WP, prim.lo, [mats[i] for i in perm], [ts[i] for i in perm], True, G), pick(want, perm))
    for n in (1, 8, 9):
        check_against(ds.library_spacing(prim.rs[True], WP, prim.lo, mats[:n], ts[:n], True, G), pick(want, slice(0, n)))
    check_against(ds.library_spacing(prim.rs[False], WP, prim.lo, mats[7:10], ts[7:10], False, G),
                  S.np_library_spacing(seq, borders, prim.W, prim.lo, mats[7:10], ts[7:10], False, G, prim.scored))


# ---- 4. degenerate sizes, refused arguments -------------------------------------------------------------------------------------------
def test_degenerate_sizes_and_errors(geometry):
    from kmap_amd import _ffi
    ds, seq, borders, Ws, scored, prim, _ = geometry
    lib = _ffi.lib()
    W = Ws[9]
    t = M.score_range(W)[0]
    rs = prim.rs[True]
    Sg, R, n_primary, n_pair, n_far = ds.library_spacing(rs, WP, prim.lo, [], [], True, 7)
    assert Sg.shape == (0, 4, 8) and R.shape == (0, 9, 9) and n_pair.shape == (0,) and n_far.shape == (0,) and n_primary == rs.n_scored

    def call(widths, weights, n=ds.n, n_seq=ds.n_seq, max_gap=10, codes=ds.codes.ptr, gaps=True, prim_width=WP, score=rs.score.ptr):
        wd, thr = np.array(widths, np.int32), np.array([t, t], np.int32)
        out = (np.full((2, 4, 11), 7, np.uint64), np.full((2, 12, 12), 7, np.uint64), np.full(1, -5, np.int64), np.full(2, -5, np.int64),
               np.full(2, -5, np.int64))
        rc = lib.kmap_readscore_spacing_library_dev(codes, ds.inval_orig.ptr, n, ds.borders.ptr, n_seq, score, rs.loc.ptr, rs.strand.ptr,
                                                    prim_width, prim.lo, len(widths), _ffi.ptr(wd), weights, _ffi.ptr(thr), 1, max_gap,
                                                    _ffi.ptr(out[0]) if gaps else None, _ffi.ptr(out[1]), _ffi.ptr(out[2]),
                                                    _ffi.ptr(out[3]), _ffi.ptr(out[4]), None)
        return rc, out

    def untouched(out):
        return (out[0] == 7).all() and (out[1] == 7).all() and all((a == -5).all() for a in out[2:])
    grid = np.zeros((2, 4, 32), np.int32)
    grid[:, :, :9] = W
    # no reads: zeros; no positions: the primary reads are counted, there is no pair
    rc, out = call([9, 9], _ffi.ptr(grid), n_seq=0)
    assert rc == 0 and not any(a.any() for a in out)
    rc, out = call([9, 9], _ffi.ptr(grid), n=0)
    assert rc == 0 and not any(a.any() for a in (out[0], out[1], out[3], out[4])) and out[2][0] == rs.n_scored
    # the plain call, both matrices alike
    rc, out = call([9, 9], _ffi.ptr(grid))
    want = S.np_library_spacing(seq, borders, prim.W, prim.lo, [W], [t], True, 10, prim.scored, [scored[9]])
    assert rc == 0 and want[4][0] > 100
    for m in range(2):
        np.testing.assert_array_equal(out[0][m].astype(np.int64), want[0][0])
        np.testing.assert_array_equal(out[1][m].astype(np.int64), want[1][0])
        assert (int(out[2][0]), int(out[3][m]), int(out[4][m])) == (want[2], int(want[3][0]), int(want[4][0]))
    # width 3 and 32, a weight behind the width or too large, null arrays, negative sizes: KMAP_E_INVAL naming the entry, nothing written
    for widths in ([3, 9], [9, 32]):
        rc, out = call(widths, _ffi.ptr(grid))
        assert rc == -1 and "readscore_spacing_library" in _ffi.last_error() and f"width={3 if 3 in widths else 32}" in _ffi.last_error()
        assert untouched(out)
        with pytest.raises(ValueError, match="library_spacing: .*width (3|32)"):
            ds.library_spacing(rs, WP, prim.lo, [np.zeros((4, w), np.int32) for w in widths], [0, 0], True)
    for pw in (3, 32):
        rc, out = call([9, 9], _ffi.ptr(grid), prim_width=pw)
        assert rc == -1 and f"prim_width={pw}" in _ffi.last_error() and untouched(out)
    rc, out = call([8, 9], _ffi.ptr(grid))
    assert rc == -1 and "behind its width" in _ffi.last_error() and untouched(out)
    huge = grid.copy()
    huge[1, 2, 3] = 2 ** 31 // 31
    rc, out = call([9, 9], _ffi.ptr(huge))
    assert rc == -1 and "int32" in _ffi.last_error() and untouched(out)
    assert call([9, 9], None)[0] == -1 and call([9, 9], _ffi.ptr(grid), n=-1)[0] == -1 and call([9, 9], _ffi.ptr(grid), n_seq=-1)[0] == -1
    for kw in (dict(codes=None), dict(gaps=False), dict(score=None)):
        rc, out = call([9, 9], _ffi.ptr(grid), **kw)
        assert rc == -1 and "null pointer" in _ffi.last_error() and untouched(out)
    rc, out = call([9, 9], _ffi.ptr(grid), max_gap=-1)
    assert rc == -1 and "max_gap" in _ffi.last_error() and untouched(out)
    rc, out = call([9, 9], _ffi.ptr(grid), max_gap=512)
    assert rc == -4 and "511" in _ffi.last_error() and untouched(out)
    with pytest.raises(ValueError, match="max_gap 512"):
        ds.library_spacing(rs, WP, prim.lo, [W], [t], True, max_gap=512)
    # and the next call is as good as the first
    check_against(ds.library_spacing(rs, WP, prim.lo, [W], [t], True, 10), want)


# ---- 5. the second witness ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("revcom", [True, False])
def test_against_scan_pwm_hit_lists(geometry, revcom):
    """scan_pwm's hits -- pass A's hit bits and the sparse traversal, not the dense per-read pass -- and the fetched read_scores of
    the primary, reduced on the host by definitions 2 - 4"""
    from kmap_amd.pwm import pwm_threshold
    ds, seq, borders, Ws, _, prim, _ = geometry
    mats = [Ws[4], Ws[16], Ws[31], prim.W]
    ts = [pwm_threshold(Ws[4], 1e-2)[0], M.score_range(Ws[16])[0], M.score_range(Ws[31])[0], prim.lo]
    tP, G = pwm_threshold(prim.W, 0.05)[0], 30
    got = ds.library_spacing(prim.rs[revcom], WP, tP, mats, ts, revcom, G)
    ploc, pstrand, n_primary = S.primary_sites(*prim.rs[revcom].fetch(), tP)
    assert got[2] == n_primary > 100
    for m, (W, t) in enumerate(zip(mats, ts)):
        hits, loc, score, strand = ds.scan_pwm(W, t, revcom)
        read = np.repeat(np.arange(len(hits)), hits)
        Sm, Rm, n_pair, n_far = S.reduce_pairs(read, loc, score, strand, ploc, pstrand, borders, W.shape[1], WP, G)
        np.testing.assert_array_equal(got[0][m], Sm)
        np.testing.assert_array_equal(got[1][m], Rm)
        assert (int(got[3][m]), int(got[4][m])) == (n_pair, n_far) and n_pair > 0


# ---- 6. the verb end to end -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("revcom", [None, False])
def test_verb_end_to_end(tmp_path, monkeypatch, capsys, revcom):
    """the seeded reads of tests/test_spacing_host.py: every file of the run on the device equals the one of the run through the
    model-backed DeviceSeq"""
    import kmap_amd.motif_discovery as D
    from kmap_amd import spacing as C
    res, primary, files, *_ = S.write_planted(tmp_path)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    lib = [str(f) for f in files] + [str(ROOT / "tests" / "golden" / "library" / "three.meme")]
    kw = dict(revcom_mode=revcom, max_gap=60, top_hist=3)
    real = C._motif_spacing(str(res), str(primary), lib, output_dir=str(tmp_path / "device"), **kw)
    monkeypatch.setattr(D, "DeviceSeq", S.ModelSeq)
    model_run = C._motif_spacing(str(res), str(primary), lib, output_dir=str(tmp_path / "model"), **kw)
    capsys.readouterr()
    a = (tmp_path / "device" / "spacing_rank.csv").read_text().split("\n")
    b = (tmp_path / "model" / "spacing_rank.csv").read_text().split("\n")
    cols = a[0].split(",")
    assert len(a) == len(b) == 7 and len(cols) == 21 and a[0] == b[0]
    for line_a, line_b in zip(a[1:], b[1:]):
        for name, x, y in zip(cols, line_a.split(","), line_b.split(",")):
            assert x == y, name
    first = dict(zip(cols, a[1].split(",")))
    assert first["name"] in (S.FIXED, "M2_ACCTACGTA") and float(first["q_bh"]) < 0.01
    assert (first["best_side"], first["best_strand"], first["best_gap"]) == ("downstream", "same", "3")
    assert sorted(p.name for p in (tmp_path / "device").iterdir()) == sorted(p.name for p in (tmp_path / "model").iterdir())
    assert len(list((tmp_path / "device").iterdir())) == 5
    for p in (tmp_path / "device").iterdir():
        assert p.read_bytes() == (tmp_path / "model" / p.name).read_bytes(), p.name
    for x, y in zip(real, model_run):
        np.testing.assert_array_equal(x["S"], y["S"])
        np.testing.assert_array_equal(x["R"], y["R"])
        assert (x["n_primary"], x["n_pairs"], x["n_far"]) == (y["n_primary"], y["n_pairs"], y["n_far"])
