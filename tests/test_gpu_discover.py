"""discover_pwms on the GPU (csrc/pwm_sites.hip: sites_count_kernel behind the batched scoring pass).  The
yardstick is never the new kernel: it is tests/_refine_model.py's np_counts with select_best -- section 13's selection and count in
numpy -- and as a second witness the per-matrix device path DeviceSeq.pwm_counts.  Count matrices, n_selected and n_minus are
compared as equal integers; the verb's table field by field with the run of the same core on the numpy models."""
from pathlib import Path

import numpy as np
import pytest

from tests import _discover_model as DM
from tests import _readscore_model as M
from tests._batch_model import batches
from tests._refine_model import asym_matrix, make_reads, np_counts, window_scores

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
GOLD = ROOT / "tests" / "golden"
W_NAMES = (4, 9, 16, 31, "zero", "palindrome")


def model(seq, borders, Ws, ts, revcom, scored=None):
    """library_counts on the model: (list of C', n_selected, n_minus)"""
    got = [np_counts(seq, borders, W, t, revcom, True, None if scored is None else scored[i]) for i, (W, t) in enumerate(zip(Ws, ts))]
    return [g[0] for g in got], np.array([g[2] for g in got], np.int64), np.array([g[3] for g in got], np.int64)


def check_against(got, want, Ws):
    Cs, n_sel, n_minus = got
    assert len(Cs) == len(want[0]) == len(Ws) and n_sel.dtype == np.int64 and n_minus.dtype == np.int64
    assert n_sel.shape == n_minus.shape == (len(Ws),)
    for m, (C, Cw, W) in enumerate(zip(Cs, want[0], Ws)):
        assert C.dtype == np.int64 and C.shape == (4, W.shape[1]), m
        np.testing.assert_array_equal(C, Cw, err_msg=f"matrix {m}")
        assert (C.sum(axis=0) == n_sel[m]).all(), m         # every column sums to n_selected
    np.testing.assert_array_equal(n_sel, want[1])
    np.testing.assert_array_equal(n_minus, want[2])


# ---- 1. read geometry -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def geometry():
    """~3000 reads on under 40 000 positions (fixed seed), built as tests/test_gpu_sites.py builds its own: lengths 0 .. 30 at random,
    so reads begin and end inside one group of 16 positions and cross group boundaries; lengths w - 1, w, w + 1 of every width used;
    one read of 2100 bases; 1200 reads of one base in a run; 2 % invalid bases, among them first bases of reads; n no multiple of 16.
    The model's window scores per matrix are computed once."""
    from kmap_amd.motif_discovery import DeviceSeq
    rng = np.random.default_rng(2110)
    lengths = [int(x) for x in rng.integers(0, 31, 600)] + [0, 3, 4, 5, 8, 9, 10, 15, 16, 17, 30, 31, 32, 0]
    i_long = len(lengths)
    lengths += [2100] + [1] * 1200 + [int(x) for x in rng.integers(0, 31, 1150)] + [31] * 8 + [7, 8, 9, 33]
    if (sum(lengths) + len(lengths) - 1) % 16 == 0:
        lengths[-1] += 1
    seq, borders = make_reads(lengths, rng, frac_invalid=0.02, last_separator=False)
    n = len(seq)
    assert 2900 < len(borders) < 3100 and n < 40_000 and n % 16 != 0 and borders[i_long, 1] - borders[i_long, 0] == 2100
    length = borders[:, 1] - borders[:, 0]
    inside_group = (length > 0) & (borders[:, 0] // 16 == (borders[:, 1] - 1) // 16)
    assert inside_group.sum() > 100 and ((length > 0) & ~inside_group).sum() > 100
    Ws = {w: asym_matrix(w, rng) for w in W_NAMES if isinstance(w, int)}
    Ws["zero"] = np.zeros((4, 8), np.int32)                  # every window ties
    half = rng.integers(-300, 201, size=(4, 10)).astype(np.int32)
    Ws["palindrome"] = half + half[::-1, ::-1]               # W[b][j] == W[3 - b][w - 1 - j]: rc == fwd for every window
    scored = {k: window_scores(seq, W) for k, W in Ws.items()}
    ds = DeviceSeq(seq, borders)
    yield ds, seq, borders, Ws, scored
    ds.close()


@pytest.mark.parametrize("revcom", [True, False])
def test_thresholds_against_the_model(geometry, revcom):
    """widths 4, 9, 16 and 31 (the three-code-word window) at lo (every scorable read selected), hi + 1 (nothing) and p = 10^-2"""
    from kmap_amd.pwm import pwm_threshold
    ds, seq, borders, Ws, scored = geometry
    mats, sc, ts = [], [], []
    for k in (4, 9, 16, 31):
        t_p, lo, hi = pwm_threshold(Ws[k], 1e-2)
        lo_rc, hi_rc = M.score_range(Ws[k])
        assert lo_rc <= lo < t_p <= hi <= hi_rc
        mats += [Ws[k]] * 3
        sc += [scored[k]] * 3
        ts += [lo_rc, hi_rc + 1, t_p]
    want = model(seq, borders, mats, ts, revcom, sc)
    got = ds.library_counts(mats, ts, revcom)
    check_against(got, want, mats)
    Cs, n_sel, n_minus = got
    assert not n_sel[1::3].any() and not any(C.any() for C in Cs[1::3]) and not n_minus[1::3].any()     # t = hi + 1: all zeros
    assert (n_sel[2::3] < n_sel[0::3]).all() and n_sel[2::3][:2].all()
    assert (n_minus[0::3] > 0).all() and (n_minus[0::3] < n_sel[0::3]).all() if revcom else not n_minus.any()
    # n_selected is library_sites' n_sites, and at lo library_histograms' n_scored
    np.testing.assert_array_equal(n_sel, ds.library_sites(mats, ts, revcom)[2])
    assert n_sel[0] > n_sel[9] > 0                           # reads of 4 .. 30 bases are sites for the narrow matrix only
    # the second witness: the per-matrix device path
    for m in (0, 2, 5, 6, 9, 11):
        C1, _, sel, minus = ds.pwm_counts(mats[m], ts[m], revcom, True)
        np.testing.assert_array_equal(Cs[m], C1)
        assert (int(n_sel[m]), int(n_minus[m])) == (sel, minus)


def test_cells_behind_the_width_are_zero(geometry):
    """the C entry's [n_mat][4][32] grids, prefilled: every cell is written, those behind the width with 0"""
    from kmap_amd import _ffi
    ds, seq, borders, Ws, scored = geometry
    widths = np.array([9, 31, 4], np.int32)
    weights = np.zeros((3, 4, 32), np.int32)
    for m, w in enumerate(widths.tolist()):
        weights[m, :, :w] = Ws[w]
    thr = np.array([M.score_range(Ws[int(w)])[0] for w in widths], np.int32)
    counts, sel, minus = np.full((3, 4, 32), 7, np.uint64), np.full(3, -5, np.int64), np.full(3, -5, np.int64)
    rc = _ffi.lib().kmap_readscore_counts_library_dev(ds.codes.ptr, ds.inval_orig.ptr, ds.n, ds.borders.ptr, ds.n_seq, 3, _ffi.ptr(widths),
                                                      _ffi.ptr(weights), _ffi.ptr(thr), 1, _ffi.ptr(counts), _ffi.ptr(sel),
                                                      _ffi.ptr(minus), None)
    assert rc == 0
    for m, w in enumerate(widths.tolist()):
        want = np_counts(seq, borders, Ws[w], int(thr[m]), True, True, scored[w])
        np.testing.assert_array_equal(counts[m, :, :w].astype(np.int64), want[0])
        assert not counts[m, :, w:].any() and (int(sel[m]), int(minus[m])) == want[2:]


@pytest.mark.parametrize("revcom", [True, False])
def test_ties(geometry, revcom):
    """the all-zero matrix at t = 0: the first valid window of every scorable read, every window '+'; a reverse-palindromic matrix:
    rc == fwd everywhere, so no window is on '-' and both strand settings count the same"""
    ds, seq, borders, Ws, scored = geometry
    valid = scored["zero"][0]
    C = np.zeros((4, 8), np.int64)
    n_first = later = 0
    for s, e in borders.tolist():
        v = np.nonzero(valid[s:max(e - 7, s)])[0]
        if len(v):
            n_first, later = n_first + 1, later + (v[0] > 0)
            C[seq[s + v[0]:s + v[0] + 8], np.arange(8)] += 1
    assert later > 50                                        # reads whose first valid window is not at loc 0
    got = ds.library_counts([Ws["zero"]], [0], revcom)
    np.testing.assert_array_equal(got[0][0], C)
    assert got[1].tolist() == [n_first] and got[2].tolist() == [0]
    check_against(got, model(seq, borders, [Ws["zero"]], [0], revcom, [scored["zero"]]), [Ws["zero"]])
    P = Ws["palindrome"]
    np.testing.assert_array_equal(scored["palindrome"][1], scored["palindrome"][2])
    t = M.score_range(P)[0]
    got = ds.library_counts([P, P], [t, 0], revcom)
    check_against(got, model(seq, borders, [P, P], [t, 0], revcom, [scored["palindrome"]] * 2), [P, P])
    assert got[2].tolist() == [0, 0] and got[1][0] > got[1][1] > 0
    if revcom:
        other = ds.library_counts([P, P], [t, 0], False)
        for a, b in zip(got[0], other[0]):
            np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("revcom", [True, False])
def test_sites_at_the_array_end_and_at_a_group_end(revcom):
    """w = 31: the best window of the last read ends at position n - 1 (its last code word is the array's last), and the best window
    of another read starts at the read's first base, at an array position = 15 (mod 16), so that it spans three code words"""
    from kmap_amd.motif_discovery import DeviceSeq
    rng = np.random.default_rng(2111)
    W = asym_matrix(31, rng)
    best = W.argmax(axis=0).astype(np.uint8)
    lengths = [14, 40, 20, 33, 5, 36]
    seq, borders = make_reads(lengths, rng, frac_invalid=0.0, last_separator=False)
    seq[borders[:, 0]] = rng.integers(0, 4, len(borders))    # make_reads marks some first and last bases invalid: not here
    seq[borders[:, 1] - 1] = rng.integers(0, 4, len(borders))
    n = len(seq)
    assert borders[1, 0] % 16 == 15 and borders[-1, 1] == n and n % 16 != 0
    seq[borders[1, 0]:borders[1, 0] + 31] = best
    seq[n - 31:] = best
    hi = int(W.max(axis=0).sum())
    ds = DeviceSeq(seq, borders)
    try:
        got = ds.library_counts([W, W], [hi, M.score_range(W)[0]], revcom)
        check_against(got, model(seq, borders, [W, W], [hi, M.score_range(W)[0]], revcom), [W, W])
        assert got[1].tolist() == [2, 3] and got[2][0] == 0           # three reads have 31 bases or more
        want = np.zeros((4, 31), np.int64)
        want[best, np.arange(31)] = 2
        np.testing.assert_array_equal(got[0][0], want)
        rs = ds.read_scores(W, revcom)
        try:
            score, loc, _ = rs.fetch()
        finally:
            rs.close()
        assert (int(score[1]), int(loc[1])) == (hi, 0) and (int(score[5]), int(loc[5])) == (hi, 36 - 31)
    finally:
        ds.close()


# ---- 2. batching ------------------------------------------------------------------------------------------------------------------
def test_batches_permutation_and_prefixes(geometry):
    from kmap_amd.pwm import pwm_threshold
    ds, seq, borders, _, _ = geometry
    rng = np.random.default_rng(2112)
    widths = [31, 5, 13, 8, 29, 4, 17, 6, 20, 7, 25, 4, 14, 28, 6, 19, 31, 16, 8]
    assert len(widths) == 19 and min(widths) == 4 and max(widths) == 31
    closed = batches(widths)
    assert len(closed) >= 3 and {"matrices", "chunks"} <= {why for _, why in closed}
    mats = [asym_matrix(w, rng) for w in widths]
    ts = [pwm_threshold(W, 1e-2)[0] if i % 2 else M.score_range(W)[0] for i, W in enumerate(mats)]
    want = model(seq, borders, mats, ts, True)
    got = ds.library_counts(mats, ts, True)
    check_against(got, want, mats)
    assert got[1].all()
    again = ds.library_counts(mats, ts, True)                # two calls give identical arrays
    for a, b in zip(got[0], again[0]):
        assert a.tobytes() == b.tobytes()
    assert got[1].tobytes() == again[1].tobytes() and got[2].tobytes() == again[2].tobytes()
    perm = rng.permutation(19)
    assert (perm != np.arange(19)).any()
    check_against(ds.library_counts([mats[i] for i in perm], [ts[i] for i in perm], True),
                  ([want[0][i] for i in perm], want[1][perm], want[2][perm]), [mats[i] for i in perm])
    for n in (1, 8, 9):
        check_against(ds.library_counts(mats[:n], ts[:n], True), (want[0][:n], want[1][:n], want[2][:n]), mats[:n])
    check_against(ds.library_counts(mats[7:10], ts[7:10], False), model(seq, borders, mats[7:10], ts[7:10], False), mats[7:10])


# ---- 3. degenerate sizes, refused arguments ---------------------------------------------------------------------------------------
def test_degenerate_sizes_and_errors(geometry):
    from kmap_amd import _ffi
    from kmap_amd.motif_discovery import DeviceSeq
    ds, seq, borders, Ws, scored = geometry
    Cs, n_sel, n_minus = ds.library_counts([], [], True)
    assert Cs == [] and n_sel.shape == n_minus.shape == (0,) and n_sel.dtype == np.int64
    none = DeviceSeq(np.zeros(0, np.uint8), np.zeros((0, 2), np.int64))
    try:
        Cs, n_sel, n_minus = none.library_counts([Ws[9], Ws[31]], [0, 0], True)
        assert [C.shape for C in Cs] == [(4, 9), (4, 31)] and not any(C.any() for C in Cs) and not n_sel.any() and not n_minus.any()
    finally:
        none.close()
    lib = _ffi.lib()
    W = Ws[9]
    t = M.score_range(W)[0]

    def call(widths, weights, n=ds.n, n_seq=ds.n_seq, codes=ds.codes.ptr, counts=True):
        wd, thr = np.array(widths, np.int32), np.array([t, t], np.int32)
        out = np.full((2, 4, 32), 7, np.uint64), np.full(2, -5, np.int64), np.full(2, -5, np.int64)
        rc = lib.kmap_readscore_counts_library_dev(codes, ds.inval_orig.ptr, n, ds.borders.ptr, n_seq, len(widths), _ffi.ptr(wd), weights,
                                                   _ffi.ptr(thr), 1, _ffi.ptr(out[0]) if counts else None, _ffi.ptr(out[1]),
                                                   _ffi.ptr(out[2]), None)
        return rc, out

    def untouched(out):
        return (out[0] == 7).all() and (out[1] == -5).all() and (out[2] == -5).all()
    grid = np.zeros((2, 4, 32), np.int32)
    grid[:, :, :9] = W
    for kw in (dict(n_seq=0), dict(n=0)):                    # no reads, no positions: zeros
        rc, out = call([9, 9], _ffi.ptr(grid), **kw)
        assert rc == 0 and not any(a.any() for a in out)
    for widths in ([3, 9], [9, 32]):
        rc, out = call(widths, _ffi.ptr(grid))
        assert rc == -1 and "readscore_counts_library" in _ffi.last_error() and f"width={3 if 3 in widths else 32}" in _ffi.last_error()
        assert untouched(out)
    rc, out = call([8, 9], _ffi.ptr(grid))
    assert rc == -1 and "behind its width" in _ffi.last_error() and untouched(out)
    huge = grid.copy()
    huge[1, 2, 3] = 2 ** 31 // 31
    rc, out = call([9, 9], _ffi.ptr(huge))
    assert rc == -1 and "int32" in _ffi.last_error() and untouched(out)
    rc, out = call([9, 9], _ffi.ptr(grid), n_seq=2 ** 32)
    assert rc == -1 and "2^32" in _ffi.last_error() and untouched(out)
    assert call([9, 9], None)[0] == -1 and call([9, 9], _ffi.ptr(grid), n=-1)[0] == -1 and call([9, 9], _ffi.ptr(grid), n_seq=-1)[0] == -1
    assert call([9, 9], _ffi.ptr(grid), codes=None)[0] == -1 and call([9, 9], _ffi.ptr(grid), counts=False)[0] == -1
    # and the next call is as good as the first
    check_against(ds.library_counts([W], [t], True), model(seq, borders, [W], [t], True, [scored[9]]), [W])


# ---- 4. the verb end to end -------------------------------------------------------------------------------------------------------
def test_verb_end_to_end(tmp_path, monkeypatch, capsys):
    """tests/golden/test.fa against its device shuffle (klet 2, seed 0): discovered_rank.csv of the run on the device equals, field
    by field, the run of the same core on the numpy models with the same seeds"""
    from kmap_amd import discover as D
    from kmap_amd.enrichment import _enrich_kmers
    from kmap_amd.kmer_count import _preproc, hash2kmer
    from kmap_amd.library import read_motif_library
    from kmap_amd.shuffle import _shuffle_reads
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    res, ctl = tmp_path / "res", tmp_path / "control.fa"
    _preproc(str(GOLD / "test.fa"), str(res))
    _shuffle_reads(str(res), klet=2, seed=0, output_file=str(ctl))
    real = D._discover_pwms(str(res), str(ctl), n_seeds=16, output_dir=str(tmp_path / "device"))
    printed = capsys.readouterr().out
    assert "discover_pwms: 16 seeds of length 8, 2 families, both strands" in printed
    # the seeds are enrich_kmers' first 16 rows with z > 0
    _, kh, a, b, z = _enrich_kmers(str(res), str(ctl), [8], output_dir=str(tmp_path / "enrich"))["kmers"][8]
    rows = [(hash2kmer(int(h), 8), int(x), int(y), float(v)) for h, x, y, v in zip(kh, a, b, z) if v > 0][:16]
    seeds = [(st["seed"], st["seed_fg"], st["seed_control"], st["seed_z"]) for st in real]
    assert seeds == rows and len(seeds) == 16
    # the same core on the models
    seq, borders = M.encode_fasta_np(GOLD / "test.fa")
    cseq, cborders = M.encode_fasta_np(ctl)
    want = D.discover_core(seeds, DM.counts_fn(seq, borders, True), DM.hist_fn(seq, borders, cseq, cborders, True), DM.match_fn, True)
    D.write_discovery(tmp_path / "model", want, 1.0, True)
    x = (tmp_path / "device" / D.RANK_FILE).read_text().split("\n")
    y = (tmp_path / "model" / D.RANK_FILE).read_text().split("\n")
    cols = x[0].split(",")
    assert len(x) == len(y) == 18 and x[0] == y[0] and x[0] + "\n" == D.RANK_HEADER
    for line_x, line_y in zip(x[1:], y[1:]):
        for name, u, v in zip(cols, line_x.split(","), line_y.split(",")):
            assert u == v, name
    for name in (D.TRACE_FILE, D.MEME_FILE):
        assert (tmp_path / "device" / name).read_bytes() == (tmp_path / "model" / name).read_bytes(), name
    for st_r, st_m in zip(real, want):
        np.testing.assert_array_equal(st_r["counts"], st_m["counts"])
        assert st_r["status"] == st_m["status"] == "converged"
    reps = read_motif_library(tmp_path / "device" / D.MEME_FILE)
    assert len(reps) == 2 and sorted(p.name for p in (tmp_path / "device" / D.MATRIX_DIR).iterdir()) == \
        sorted(p.name for p in (tmp_path / "model" / D.MATRIX_DIR).iterdir())
    for m in reps:
        st = next(s for s in real if s["name"] == m.name)
        np.testing.assert_array_equal(m.counts, st["counts"])
