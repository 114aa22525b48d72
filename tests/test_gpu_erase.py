"""Erasing the sites of weight matrices on the GPU (csrc/pwm_erase.hip).  The only witness is
tests/_erase_model.py's np_erase -- section 11's hits from tests/_refine_model.py, their cover in numpy -- and nothing is compared
with the code under test: the downloaded reads, the raw mask words and the three kinds of counts are compared as equal integers."""
from pathlib import Path

import numpy as np
import pytest

from tests import _discover_model as DM
from tests import _erase_model as EM
from tests import _footprint as FP
from tests import _readscore_model as M
from tests._refine_model import asym_matrix, edge_reads, encode_fasta_np, make_reads, np_counts, np_hits

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
GOLD = ROOT / "tests" / "golden"
TILE = 62 * 16                                               # positions a wave tile owns
BLOCK = 4 * TILE                                             # and a block of four waves


def words_of(buf, groups):
    from kmap_amd import _ffi
    out = buf.to_numpy(np.uint16, (groups,))
    _ffi.sync()
    return out


def check_erase(ds, seq, borders, Ws, ts, revcom, use_work, work=None):
    """one erase_sites call against the model: `work` = the working reads before the call as a uint8 array (default: seq);
    returns the working reads behind it"""
    work = seq if work is None else work
    before = words_of(ds.inval_work, ds.groups)
    n_data = (len(seq) + 15) // 16
    np.testing.assert_array_equal(before[:n_data], EM.mask_words(work))
    want, hits, cov, n_new = EM.np_erase(work if use_work else seq, borders, Ws, ts, revcom, out=work)
    got_hits, got_cov, got_new = ds.erase_sites(Ws, ts, revcom, use_work=use_work)
    assert got_hits.dtype == got_cov.dtype == np.int64 and got_hits.shape == got_cov.shape == (len(Ws),) and isinstance(got_new, int)
    np.testing.assert_array_equal(got_hits, hits)
    np.testing.assert_array_equal(got_cov, cov)
    assert got_new == n_new
    np.testing.assert_array_equal(ds.download(), want)
    after = words_of(ds.inval_work, ds.groups)
    np.testing.assert_array_equal(after[:n_data], EM.mask_words(want))
    np.testing.assert_array_equal(after[n_data:], before[n_data:])           # the halo words
    assert not (before & ~after).any()                                       # old bits stay
    assert int(sum(bin(int(x)).count("1") for x in (after & ~before))) == n_new
    return want


# ---- 1. thresholds, widths, strands -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def geometry():
    """~300 reads on about 9 000 positions (fixed seed): more than two blocks' worth of 62-group wave tiles, n no multiple of 16,
    2 % invalid bases; the model's window scores per matrix are not kept, every call is small"""
    from kmap_amd.motif_discovery import DeviceSeq
    rng = np.random.default_rng(2210)
    lengths = [int(x) for x in rng.integers(0, 61, 290)] + [3, 4, 5, 8, 9, 10, 15, 16, 17, 30, 31, 32, 0, 33]
    if (sum(lengths) + len(lengths) - 1) % 16 == 0:
        lengths[-1] += 1
    seq, borders = make_reads(lengths, rng, frac_invalid=0.02, last_separator=False)
    assert 2 * BLOCK < len(seq) < 3 * BLOCK and len(seq) % 16 != 0
    Ws = {w: asym_matrix(w, rng) for w in (4, 9, 16, 31)}
    for a in (seq, borders):
        a.setflags(write=False)
    ds = DeviceSeq(seq, borders)
    codes = ds.codes.to_numpy(np.uint32, (ds.groups,)).copy()
    orig = words_of(ds.inval_orig, ds.groups).copy()
    yield ds, seq, borders, Ws
    # whatever the tests did: the codes and the original mask never change
    np.testing.assert_array_equal(ds.codes.to_numpy(np.uint32, (ds.groups,)), codes)
    np.testing.assert_array_equal(words_of(ds.inval_orig, ds.groups), orig)
    ds.close()


def valid_runs_cover(seq, w):
    """every valid run of at least w positions"""
    valid = np.concatenate([[False], np.asarray(seq) != 255, [False]])
    edge = np.diff(valid.astype(np.int8))
    cover = np.zeros(len(seq), bool)
    for s, e in zip(np.nonzero(edge == 1)[0], np.nonzero(edge == -1)[0]):
        if e - s >= w:
            cover[s:e] = True
    return cover


@pytest.mark.parametrize("revcom", [True, False])
@pytest.mark.parametrize("w", [4, 9, 16, 31])
def test_thresholds_against_the_model(geometry, w, revcom):
    from kmap_amd.pwm import pwm_threshold
    ds, seq, borders, Ws = geometry
    W = Ws[w]
    t_p = pwm_threshold(W, 1e-2)[0]
    lo, hi = M.score_range(W)
    # lo: every valid window hits, so every valid run of at least w positions goes and shorter runs stay
    ds.reset()
    left = check_erase(ds, seq, borders, [W], [lo], revcom, True)
    cover = valid_runs_cover(seq, w)
    np.testing.assert_array_equal(left == 255, (seq == 255) | cover)
    assert cover.any() and (left != 255).sum() == (seq != 255).sum() - cover.sum()
    # hi + 1: nothing
    ds.reset()
    left = check_erase(ds, seq, borders, [W], [hi + 1], revcom, True)
    np.testing.assert_array_equal(left, seq)
    # p = 10^-2, and the three together: the union is the lo cover, the per-matrix numbers are the single calls'
    ds.reset()
    left = check_erase(ds, seq, borders, [W], [t_p], revcom, True)
    assert w == 31 or (seq != 255).sum() - cover.sum() < (left != 255).sum() < (seq != 255).sum()    # some, not all
    ds.reset()
    check_erase(ds, seq, borders, [W, W, W], [t_p, hi + 1, lo], revcom, True)
    ds.reset()
    np.testing.assert_array_equal(ds.download(), seq)        # reset() undoes it


@pytest.mark.parametrize("shift,w", [(-1, 9), (0, 9), (1, 9), (-1, 31), (0, 31), (1, 31)])
def test_reads_at_group_tile_and_block_edges(shift, w):
    """tests/_refine_model.py's edge reads: reads that start one position around group, tile and block edges, no invalid base
    inside a read, the last read ends where the array ends"""
    from kmap_amd.motif_discovery import DeviceSeq
    from kmap_amd.pwm import pwm_threshold
    seq, borders, W, _, _ = edge_reads(shift, w)
    ds = DeviceSeq(seq, borders)
    try:
        left = check_erase(ds, seq, borders, [W], [M.score_range(W)[0]], True, True)
        np.testing.assert_array_equal(left == 255, (seq == 255) | valid_runs_cover(seq, w))
        ds.reset()
        check_erase(ds, seq, borders, [W], [pwm_threshold(W, 1e-2)[0]], False, True)
    finally:
        ds.close()


# ---- 2. placed sites --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("revcom", [True, False])
def test_placed_sites(revcom):
    """one read of 9 001 bases.  A w = 31 matrix at its best score, planted: at position 0; at a position = 15 (mod 16), so the hit
    covers three groups; on the last position of the first wave tile and of the first block's last tile; ending at n - 1.  A w = 9
    matrix that wants nine A: a run of twelve A is four overlapping hits; nine A right behind a planted w = 31 site are adjacent hits
    of two matrices."""
    from kmap_amd.motif_discovery import DeviceSeq
    rng = np.random.default_rng(2211)
    n = 9001
    W31 = asym_matrix(31, rng)
    best = W31.argmax(axis=0).astype(np.uint8)
    WA = np.full((4, 9), -400, np.int32)
    WA[0] = 200
    seq = rng.integers(0, 4, n).astype(np.uint8)
    seq[rng.choice(np.arange(5000, 8000), 40, replace=False)] = 255
    starts31 = [0, 16 * 20 + 15, TILE - 1, BLOCK - 1, 2000, n - 31]
    for p in starts31:
        seq[p:p + 31] = best
    seq[2031:2040] = 0                                       # adjacent to the site at 2000
    assert best[-1] != 0                                     # (the last column wants C): no nine A start inside the site at 2000
    seq[2040] = 1
    seq[2999], seq[3012] = 1, 1
    seq[3000:3012] = 0                                       # twelve A
    borders = np.array([[0, n]], np.int64)
    hi31, hiA = int(W31.max(axis=0).sum()), 9 * 200
    p31 = np_hits(seq, borders, W31, hi31, revcom)[2].tolist()
    pA = np_hits(seq, borders, WA, hiA, revcom)[2].tolist()
    assert set(starts31) <= set(p31) and {2031, 3000, 3001, 3002, 3003} <= set(pA) and 2032 not in pA and 3004 not in pA
    assert (16 * 20 + 15) % 16 == 15 and (TILE - 1 + 31) // 16 - (TILE - 1) // 16 == 2
    ds = DeviceSeq(seq, borders)
    try:
        left = check_erase(ds, seq, borders, [W31, WA], [hi31, hiA], revcom, True)
        for p in starts31:
            assert (left[p:p + 31] == 255).all()
        assert (left[2000:2040] == 255).all() and left[2040] == 1
        assert left[2999] == 1 and (left[3000:3012] == 255).all() and left[3012] == 1
        assert left[31] != 255 and left[n - 32] != 255 and left[TILE - 2] != 255 and left[BLOCK - 2] != 255
        ds.reset()
        hits, _, _ = ds.erase_sites([WA, W31], [hiA, hi31], revcom)
        assert hits[0] == len(pA) and hits[1] == len(p31)
    finally:
        ds.close()


# ---- 3. the order of the matrices; two runs ---------------------------------------------------------------------------------------
def test_permutation_prefixes_and_two_runs(geometry):
    from kmap_amd.pwm import pwm_threshold
    ds, seq, borders, _ = geometry
    rng = np.random.default_rng(2212)
    widths = [31, 5, 13, 8, 29, 4, 17, 6, 20, 7, 25, 4, 14, 28, 6, 19, 31, 16, 8]
    assert len(widths) == 19
    mats = [asym_matrix(w, rng) for w in widths]
    ts = [pwm_threshold(W, 1e-2 if i % 2 else 1e-3)[0] for i, W in enumerate(mats)]
    ds.reset()
    left = check_erase(ds, seq, borders, mats, ts, True, True)
    words = words_of(ds.inval_work, ds.groups).copy()
    ds.reset()
    first = ds.erase_sites(mats, ts, True)
    assert words_of(ds.inval_work, ds.groups).tobytes() == words.tobytes()   # two runs: the same bytes
    assert first[0].all() and (first[1] > 0).all()
    perm = rng.permutation(19)
    assert (perm != np.arange(19)).any()
    ds.reset()
    second = ds.erase_sites([mats[i] for i in perm], [ts[i] for i in perm], True)
    assert words_of(ds.inval_work, ds.groups).tobytes() == words.tobytes() and second[2] == first[2]
    np.testing.assert_array_equal(second[0], first[0][perm])
    np.testing.assert_array_equal(second[1], first[1][perm])
    np.testing.assert_array_equal(ds.download(), left)
    for n in (1, 8, 9):
        ds.reset()
        check_erase(ds, seq, borders, mats[:n], ts[:n], True, True)
    ds.reset()
    check_erase(ds, seq, borders, mats[7:10], ts[7:10], False, True)
    ds.reset()


# ---- 4. a mask that is there already ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("revcom", [True, False])
def test_premasked_aliased_and_not(geometry, revcom):
    from kmap_amd.pwm import pwm_threshold
    ds, seq, borders, Ws = geometry
    A, B = Ws[9], Ws[16]
    tA, tB = pwm_threshold(A, 1e-2)[0], pwm_threshold(B, 3e-2)[0]
    hits_orig = len(np_hits(seq, borders, B, tB, revcom)[2])
    for use_work in (True, False):
        ds.reset()
        work = check_erase(ds, seq, borders, [A], [tA], revcom, False)       # the pre-mask
        assert (work == 255).sum() > (seq == 255).sum()
        hits_work = len(np_hits(work, borders, B, tB, revcom)[2])
        assert 0 < hits_work < hits_orig                     # a window that touches a masked position is not a hit
        left = check_erase(ds, seq, borders, [B], [tB], revcom, use_work, work=work)
        assert ((work == 255) <= (left == 255)).all() and (left == 255).sum() > (work == 255).sum()
        if use_work:
            again = ds.erase_sites([B], [tB], revcom, use_work=True)         # every hit now touches an erased position
            assert again[0].tolist() == [0] and again[1].tolist() == [0] and again[2] == 0
            np.testing.assert_array_equal(ds.download(), left)
        else:
            again = ds.erase_sites([B], [tB], revcom, use_work=False)        # the original mask: the same hits, no new bit
            assert again[0].tolist() == [hits_orig] and again[2] == 0
    ds.reset()


# ---- 5. the write footprint -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("aliased", [True, False])
def test_guard_bands_around_the_output_mask(geometry, aliased):
    """the raw entry on an output mask inside guard bands (tests/_footprint.py): only its data words change, the halo words and
    every byte around it stay; the codes and the evaluated mask are not written"""
    import ctypes

    from kmap_amd import _ffi
    from kmap_amd.pwm import pwm_threshold
    ds, seq, borders, Ws = geometry
    mats = [Ws[31], Ws[4]]
    ts = [pwm_threshold(W, 1e-2)[0] for W in mats]
    n_mat, widths, weights, thr = 2, np.array([31, 4], np.int32), np.zeros((2, 4, 32), np.int32), np.array(ts, np.int32)
    weights[0, :, :31], weights[1, :, :4] = mats
    orig = words_of(ds.inval_orig, ds.groups).copy()
    n_data = (len(seq) + 15) // 16
    want, hits, cov, n_new = EM.np_erase(seq, borders, mats, ts, True)

    def case(out_fill, in_fill):
        out = FP.Guarded(ds.groups * 2, fill=out_fill, name="inval_out")
        out.upload(orig)
        codes = FP.Guarded.of(ds.codes.to_numpy(np.uint32, (ds.groups,)), fill=in_fill, name="codes")
        ev = out if aliased else FP.Guarded.of(orig, fill=in_fill, name="inval_eval")
        got = np.full(2, -5, np.int64), np.full(2, -5, np.int64), _ffi.i64(-5)
        try:
            FP.ok(_ffi.lib().kmap_erase_pwm_sites_dev(codes.ptr, ev.ptr, ds.n, n_mat, _ffi.ptr(widths), _ffi.ptr(weights), _ffi.ptr(thr), 1,
                                                      out.ptr, _ffi.ptr(got[0]), _ffi.ptr(got[1]), ctypes.byref(got[2])))
            FP.guards(out, codes, ev)
            np.testing.assert_array_equal(codes.payload(np.uint32), ds.codes.to_numpy(np.uint32, (ds.groups,)))
            if not aliased:
                np.testing.assert_array_equal(ev.payload(np.uint16), orig)
            words = out.payload(np.uint16)
            np.testing.assert_array_equal(words[:n_data], EM.mask_words(want))
            np.testing.assert_array_equal(words[n_data:], orig[n_data:])
            assert got[0].tolist() == hits.tolist() and got[1].tolist() == cov.tolist() and got[2].value == n_new
        finally:
            FP.free(codes, *(() if aliased else (ev,)))
        return [out]
    FP.run_twice(case)


# ---- 6. degenerate sizes, refused arguments ---------------------------------------------------------------------------------------
def test_degenerate_sizes_and_errors(geometry):
    import ctypes

    from kmap_amd import _ffi
    from kmap_amd.motif_discovery import DeviceSeq
    ds, seq, borders, Ws = geometry
    ds.reset()
    hits, cov, n_new = ds.erase_sites([], [], True)
    assert hits.shape == cov.shape == (0,) and hits.dtype == np.int64 and n_new == 0
    np.testing.assert_array_equal(ds.download(), seq)
    none = DeviceSeq(np.zeros(0, np.uint8), np.zeros((0, 2), np.int64))
    try:
        hits, cov, n_new = none.erase_sites([Ws[9], Ws[31]], [0, 0], True)
        assert hits.tolist() == [0, 0] and cov.tolist() == [0, 0] and n_new == 0
    finally:
        none.close()
    lib = _ffi.lib()
    W = Ws[9]
    t = M.score_range(W)[0]
    before = words_of(ds.inval_work, ds.groups).copy()

    def call(widths, weights, n=ds.n, n_mat=None, codes=ds.codes.ptr, ev=ds.inval_orig.ptr, out=ds.inval_work.ptr, hits=True, new=True):
        wd, thr = np.array(widths, np.int32), np.array([t, t], np.int32)
        res = np.full(2, -5, np.int64), np.full(2, -5, np.int64), _ffi.i64(-5)
        rc = lib.kmap_erase_pwm_sites_dev(codes, ev, n, len(widths) if n_mat is None else n_mat, _ffi.ptr(wd), weights, _ffi.ptr(thr), 1,
                                          out, _ffi.ptr(res[0]) if hits else None, _ffi.ptr(res[1]), ctypes.byref(res[2]) if new else None)
        return rc, res

    def untouched(res):
        same = words_of(ds.inval_work, ds.groups).tobytes() == before.tobytes()
        return same and (res[0] == -5).all() and (res[1] == -5).all() and res[2].value == -5
    grid = np.zeros((2, 4, 32), np.int32)
    grid[:, :, :9] = W
    rc, res = call([9, 9], _ffi.ptr(grid), n=0)              # no position: zeros, the mask stays
    assert rc == 0 and not res[0].any() and not res[1].any() and res[2].value == 0
    rc, res = call([9, 9], _ffi.ptr(grid), n_mat=0)          # no matrix: n_new alone is written
    assert rc == 0 and res[2].value == 0 and (res[0] == -5).all()
    assert words_of(ds.inval_work, ds.groups).tobytes() == before.tobytes()
    for widths in ([3, 9], [9, 32]):
        rc, res = call(widths, _ffi.ptr(grid))
        assert rc == -1 and "erase_pwm_sites_dev" in _ffi.last_error() and f"width={3 if 3 in widths else 32}" in _ffi.last_error()
        assert untouched(res)
    rc, res = call([8, 9], _ffi.ptr(grid))
    assert rc == -1 and "behind its width" in _ffi.last_error() and untouched(res)
    huge = grid.copy()
    huge[1, 2, 3] = 2 ** 31 // 31
    rc, res = call([9, 9], _ffi.ptr(huge))
    assert rc == -1 and "int32" in _ffi.last_error() and untouched(res)
    for kw in (dict(n=-1), dict(n_mat=-1), dict(codes=None), dict(ev=None), dict(out=None), dict(hits=False), dict(new=False)):
        rc, res = call([9, 9], _ffi.ptr(grid), **kw)
        assert rc == -1 and "erase_pwm_sites_dev" in _ffi.last_error() and untouched(res), kw
    assert call([9, 9], None)[0] == -1
    # and the next call is as good as the first
    check_erase(ds, seq, borders, [W], [t], True, True)
    ds.reset()


# ---- 7. the callers of the working mask -------------------------------------------------------------------------------------------
def test_counts_on_the_erased_reads(geometry):
    from kmap_amd.kmer_count import DeviceCounts
    from kmap_amd.pwm import pwm_threshold
    ds, seq, borders, Ws = geometry
    ds.reset()
    A = Ws[9]
    left = check_erase(ds, seq, borders, [A], [pwm_threshold(A, 3e-2)[0]], True, True)
    assert (left == 255).sum() > (seq == 255).sum() + 500
    mats = [Ws[4], Ws[16], Ws[9]]
    ts = [pwm_threshold(W, 1e-2)[0] for W in mats]
    for use_work, arr in ((True, left), (False, seq)):
        Cs, n_sel, n_minus = ds.library_counts(mats, ts, True, use_work=use_work)
        for m, (W, t) in enumerate(zip(mats, ts)):
            want = np_counts(arr, borders, W, t, True, True)
            np.testing.assert_array_equal(Cs[m], want[0])
            assert (int(n_sel[m]), int(n_minus[m])) == want[2:]
    Cs, n_sel, _ = ds.library_counts(mats, ts, True)         # the default is the original reads
    assert int(n_sel[2]) == np_counts(seq, borders, mats[2], ts[2], True, True)[2] > np_counts(left, borders, mats[2], ts[2], True, True)[2]
    dc = DeviceCounts()
    try:
        for use_work, arr in ((True, left), (False, seq)):
            # one strand: tests/_discover_model.py's kmer_table as it is.  Both strands: the kernels merge the per-read counts of a
            # k-mer and of its reverse complement (a palindrome counts twice), kmer_table takes the lower hash first: the merged
            # restatement of tests/_erase_model.py is the witness there
            for revcom, want in ((False, DM.kmer_table(arr, borders, 8, False)), (True, EM.merged_kmer_table(arr, borders, 8))):
                ds.count(dc, 8, True, revcom, use_work=use_work)
                uniq, cnt = dc.fetch()
                assert dict(zip(uniq.tolist(), cnt.tolist())) == want, (use_work, revcom)
        assert sum(DM.kmer_table(left, borders, 8, False).values()) < sum(DM.kmer_table(seq, borders, 8, False).values())
    finally:
        dc.close()
    ds.reset()


# ---- 8. the verbs end to end ------------------------------------------------------------------------------------------------------
def write_fasta(path, seq, borders):
    with open(path, "w") as fh:
        for i, (s, e) in enumerate(np.asarray(borders).tolist()):
            fh.write(f">r{i}\n" + "".join("ACGTN"[min(int(b), 4)] for b in seq[s:e]) + "\n")


def test_discover_pwms_with_two_rounds(tmp_path, monkeypatch, capsys):
    """the 400 x 40 reads with a dominant and a weaker planted word against their device shuffle: the verb with --erase_rounds 2
    equals, field by field, discover_rounds on the numpy models"""
    from kmap_amd import discover as D
    from kmap_amd.kmer_count import _preproc
    from kmap_amd.shuffle import _shuffle_reads
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    seq, borders = EM.planted_reads(2201)
    fa, res, ctl = tmp_path / "reads.fa", tmp_path / "res", tmp_path / "control.fa"
    write_fasta(fa, seq, borders)
    _preproc(str(fa), str(res))
    _shuffle_reads(str(res), klet=2, seed=0, output_file=str(ctl))
    real = D._discover_pwms(str(res), str(ctl), n_seeds=3, output_dir=str(tmp_path / "device"), erase_rounds=2)
    printed = capsys.readouterr().out
    assert "round 1: 1 matrix erased" in printed and "discover_pwms: 6 seeds of length 8, 2 families, both strands" in printed
    rseq, rborders = encode_fasta_np(fa)
    np.testing.assert_array_equal(rseq, seq)
    cseq, cborders = encode_fasta_np(ctl)
    mr = EM.ModelReads(rseq, rborders, cseq, cborders, True, merged=True)       # the seeds as the device's strand merge counts them
    want, log = D.discover_rounds(mr.seeds_fn(8, 2, 3), mr.counts_fn, mr.erase_fn, mr.hist_fn(), DM.match_fn, True, 2)
    assert [st["round"] for st in want] == [1, 1, 1, 2, 2, 2] and len(log) == 1
    assert [(st["seed"], st["seed_fg"], st["seed_control"], st["seed_z"], st["round"]) for st in real] == \
        [(st["seed"], st["seed_fg"], st["seed_control"], st["seed_z"], st["round"]) for st in want]
    D.write_discovery(tmp_path / "model", want, 1.0, True, log)
    x = (tmp_path / "device" / D.RANK_FILE).read_text().split("\n")
    y = (tmp_path / "model" / D.RANK_FILE).read_text().split("\n")
    cols = x[0].split(",")
    assert len(x) == len(y) == 8 and x[0] == y[0] and cols[-1] == "round"
    for line_x, line_y in zip(x[1:], y[1:]):
        for name, u, v in zip(cols, line_x.split(","), line_y.split(",")):
            assert u == v, name
    for name in (D.TRACE_FILE, D.MEME_FILE, D.ERASE_FILE):
        assert (tmp_path / "device" / name).read_bytes() == (tmp_path / "model" / name).read_bytes(), name
    for st_r, st_m in zip(real, want):
        np.testing.assert_array_equal(st_r["counts"], st_m["counts"])


def test_erase_pwm_sites_verb(tmp_path, monkeypatch, capsys):
    """tests/golden/test.fa with the two golden count matrices: the FASTA the verb writes, encoded again, is np_erase's array"""
    from kmap_amd import erase as E
    from kmap_amd.kmer_count import _preproc
    from kmap_amd.library import load_library
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    res = tmp_path / "res"
    _preproc(str(GOLD / "test.fa"), str(res))
    files = [str(GOLD / "report_testfa" / "cntmat_motif0_CAATCGATAGC.csv"), str(GOLD / "report_testfa" / "cntmat_motif1_ACCTACGTA.csv")]
    motifs, ts, n_hits, n_cov, n_new = E._erase_pwm_sites(str(res), files)
    assert "erase_pwm_sites: 2 motifs" in capsys.readouterr().out
    seq, borders = encode_fasta_np(GOLD / "test.fa")
    _, _, Ws, plans = load_library("test", files, 20, 1.0, 1e-4)
    assert [p[0] for p in plans] == ts
    want, hits, cov, new = EM.np_erase(seq, borders, Ws, ts, True)
    assert n_hits.tolist() == hits.tolist() and n_cov.tolist() == cov.tolist() and n_new == new and hits.min() > 100
    got, got_borders = encode_fasta_np(res / E.OUTPUT_FILE)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(got_borders, borders)
    assert (res / E.OUTPUT_FILE).read_bytes().startswith(b">shuffled_0_0\n")
    info = (res / E.INFO_FILE).read_text().split("\n")
    assert info[0] + "\n" == E.INFO_HEADER and len(info) == 5 and info[3] == f"total,,,,{int(hits.sum())},{new}"
    for line, m, t, h, c in zip(info[1:3], motifs, ts, hits, cov):
        assert line.split(",")[0] == m.name and line.split(",")[3:] == [str(t), str(h), str(c)]
    out = tmp_path / "elsewhere" / "left.fa"                 # what is left is a --fasta_file for preproc
    E._erase_pwm_sites(str(res), files[:1], revcom_mode=False, output_file=str(out))
    _preproc(str(out), str(tmp_path / "res2"))
    want1 = EM.np_erase(seq, borders, Ws[:1], ts[:1], False)[0]
    np.testing.assert_array_equal(encode_fasta_np(out)[0], want1)
    assert (out.parent / E.INFO_FILE).exists()
