"""evaluate_pwm on the GPU (csrc/pwm_readscore.hip) against the numpy restatement of tests/_readscore_model.py (DESIGN.md section
14): per read the valid window with the largest score, the smallest loc on a tie, its strand; the histogram of those scores; the
verb's files.  Every comparison is exact integer equality (files: equal bytes)."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

from tests import _readscore_model as M
from tests._refine_model import asym_matrix, make_reads, np_hits, window_scores

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
GOLD = ROOT / "tests" / "golden"
MOTIF0, MOTIF1 = GOLD / "report_testfa" / "cntmat_motif0_CAATCGATAGC.csv", GOLD / "report_testfa" / "cntmat_motif1_ACCTACGTA.csv"
INT32_MIN = -2 ** 31


def plant(seq, borders, W, rng, every=5):
    """the matrix's best window (and, in every other such read, its reverse complement) written into every `every`-th read that has room"""
    w = W.shape[1]
    top = np.argmax(W, axis=0).astype(np.uint8)
    for k, (s, e) in enumerate(borders[::every]):
        if e - s >= w:
            at = int(rng.integers(s, e - w + 1))
            seq[at:at + w] = top if k % 2 == 0 else 3 - top[::-1]


def device_scores(ds, W, revcom):
    """(score, loc, strand, n_scored) of DeviceSeq.read_scores, fetched"""
    rs = ds.read_scores(W, revcom)
    try:
        return rs.fetch() + (rs.n_scored,)
    finally:
        rs.close()


def check(got, want):
    score, loc, strand, n_scored = got
    assert (score.dtype, loc.dtype, strand.dtype) == (np.int32, np.int32, np.uint8)
    np.testing.assert_array_equal(loc, want[1], err_msg="loc")
    np.testing.assert_array_equal(score, want[0], err_msg="score")
    np.testing.assert_array_equal(strand, want[2], err_msg="strand")
    assert n_scored == int((want[1] >= 0).sum())
    unscorable = loc < 0
    assert (score[unscorable] == INT32_MIN).all() and (loc[unscorable] == -1).all() and (strand[unscorable] == 0).all()


def run_case(seq, borders, W, revcoms=(True, False), scored=None):
    """the device against the model for one read set; returns the model's results per strand mode"""
    from kmap_amd.motif_discovery import DeviceSeq
    scored = window_scores(seq, W) if scored is None else scored
    ds = DeviceSeq(seq, borders)
    out = {}
    try:
        for revcom in revcoms:
            out[revcom] = M.np_read_scores(seq, borders, W, revcom, scored)
            check(device_scores(ds, W, revcom), out[revcom])
    finally:
        ds.close()
    return out


_CASES = {}


def reads_case(w):
    """~3000 reads of lengths 0..70 per width with planted instances, built once: (DeviceSeq, seq, borders, W, (valid, fwd, rc))"""
    if w not in _CASES:
        from kmap_amd.motif_discovery import DeviceSeq
        rng = np.random.default_rng(3000 + w)
        special = [w - 1, w, w + 1, 0, 1, 15, 16, 17, 31, 32, 33, 47, 48]
        lengths = np.concatenate([special, rng.integers(0, 71, 2990), special[::-1]])
        lengths = lengths[rng.permutation(len(lengths))]
        seq, borders = make_reads(lengths, rng)
        W = asym_matrix(w, rng)
        plant(seq, borders, W, rng)
        _CASES[w] = (DeviceSeq(seq, borders), seq, borders, W, window_scores(seq, W))
    return _CASES[w]


# ---- 1. widths and strands ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("revcom", [True, False])
@pytest.mark.parametrize("w", [4, 5, 16, 17, 31])
def test_widths_and_strands(w, revcom):
    ds, seq, borders, W, scored = reads_case(w)
    want = M.np_read_scores(seq, borders, W, revcom, scored)
    got = device_scores(ds, W, revcom)
    check(got, want)
    score, loc, strand, n_scored = got
    lo, hi = M.score_range(W)
    assert 0 < n_scored < len(borders) and (score[loc >= 0] == hi).sum() > 100             # the planted windows are found
    if revcom:
        assert 0 < strand.sum() < n_scored
    else:
        assert not strand.any()
    # a read has a scan_pwm hit at t exactly when it is scorable and its best score is >= t
    for t in (int(np.quantile(score[loc >= 0], 0.7)), hi, lo):
        reads_hit = np.unique(np_hits(seq, borders, W, t, revcom, scored)[0])
        np.testing.assert_array_equal(np.nonzero((loc >= 0) & (score >= t))[0], reads_hit)


# ---- 2. read lengths ------------------------------------------------------------------------------------------------------------
def test_read_lengths():
    """lengths 0, 1, w - 1, w, w + 1 mixed; a read of invalid bases only; reads whose only N leaves windows on one side"""
    rng = np.random.default_rng(31)
    w = 8
    lengths = np.concatenate([np.tile([0, 1, w - 1, w, w + 1], 60), [30, 12, 12, 40, 0, 0, 1, 1]])
    lengths = lengths[rng.permutation(len(lengths))]
    starts = np.concatenate([[0], np.cumsum(lengths + 1)[:-1]])
    borders = np.stack([starts, starts + lengths], axis=1)
    seq = rng.integers(0, 4, int((lengths + 1).sum())).astype(np.uint8)
    seq[borders[:, 1]] = 255
    r30, r40 = int(np.nonzero(lengths == 30)[0][0]), int(np.nonzero(lengths == 40)[0][0])
    seq[borders[r30, 0]:borders[r30, 1]] = 255               # every base invalid
    left, right = [int(r) for r in np.nonzero(lengths == 12)[0]]
    seq[borders[left, 0] + w] = 255                          # positions 0 .. 7 form the only window
    seq[borders[right, 0] + 3] = 255                         # the only window starts at 4
    seq[borders[r40, 0] + 20] = 255                          # windows on both sides
    W = asym_matrix(w, rng)
    want = run_case(seq, borders, W)[True]
    assert want[1][r30] == -1 and want[1][left] == 0 and want[1][right] == 4 and want[1][r40] >= 0
    assert (want[1][lengths < w] == -1).all() and (want[1][lengths == w] == 0).all() and set(want[1][lengths == w + 1]) == {0, 1}


# ---- 3. read starts at the group, wave-tile and block edges -----------------------------------------------------------------------
@pytest.mark.parametrize("shift", [-1, 0, 1])
def test_read_starts_at_tile_edges(shift):
    """reads that start exactly at 16, 1024 and 4096 (+ shift); n is no multiple of 16 and the last read ends where the array ends"""
    rng = np.random.default_rng(32 + shift)
    w = 9
    lengths, at = [], 0
    for target in (16 + shift, 1024 + shift, 4096 + shift, 4096 + 1024 + 16 + shift):
        while target - at > 90:
            lengths.append(int(rng.integers(20, 60)))
            at += lengths[-1] + 1
        lengths.append(target - at - 1)                      # the next read starts at the target
        at = target
    lengths += [37, 23]
    seq, borders = make_reads(lengths, rng, frac_invalid=0.01, last_separator=False)
    assert {16 + shift, 1024 + shift, 4096 + shift, 5136 + shift} <= set(borders[:, 0].tolist())
    assert len(seq) % 16 != 0 and borders[-1, 1] == len(seq)
    W = asym_matrix(w, rng)
    plant(seq, borders, W, rng, every=3)
    seq[borders[-1, 0]:] = rng.integers(1, 4, 23)            # no A, the first column's best base, before ...
    seq[len(seq) - w:] = np.argmax(W, axis=0)                # ... the last window of the array: the last read's best
    want = run_case(seq, borders, W)[True]
    assert want[1][-1] == 23 - w and want[0][-1] == M.score_range(W)[1]


# ---- 4. many read starts in one tile ----------------------------------------------------------------------------------------------
def test_many_read_starts_in_a_tile():
    """2000 reads of one base (512 read starts per tile), 1200 empty reads (1024 per tile), normal reads around and between"""
    rng = np.random.default_rng(33)
    lengths = [50] + [1] * 2000 + [60] + [0] * 1200 + [45, 1, 0, 1, 30]
    seq, borders = make_reads(lengths, rng, frac_invalid=0.0)
    W = asym_matrix(6, rng)
    want = run_case(seq, borders, W)[True]
    assert (want[1] >= 0).sum() == 4 and want[1][2001] >= 0 and want[1][3202] >= 0 and want[1][-1] >= 0


# ---- 5. ties ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("revcom", [True, False])
def test_the_smallest_loc_wins_a_score_tie(revcom):
    rng = np.random.default_rng(34)
    w = 8
    W = asym_matrix(w, rng)
    W[rng.integers(0, 4, w), np.arange(w)] = 250             # one best base per column
    top = np.argmax(W, axis=0).astype(np.uint8)
    lengths = np.full(300, 70)
    seq, borders = make_reads(lengths, rng, frac_invalid=0.0)
    first = rng.integers(0, 15, 300)
    for (s, _), f in zip(borders, first):
        for at in (f, f + 20, f + 45):                       # the same best window three times; across groups and lanes
            seq[s + at:s + at + w] = top
    want = run_case(seq, borders, W, (revcom,))[revcom]
    np.testing.assert_array_equal(want[1], first)
    assert (want[0] == M.score_range(W)[1]).all() and not want[2].any()


def test_equal_strands_give_plus():
    """a window equal to its own reverse complement scores the same on both strands under any matrix: '+'"""
    rng = np.random.default_rng(35)
    w = 8
    half = rng.integers(0, 4, w // 2)
    pal = np.concatenate([half, 3 - half[::-1]]).astype(np.uint8)
    W = rng.integers(-300, 0, size=(4, w)).astype(np.int32)
    W[pal, np.arange(w)] = 250                               # the palindrome is the best window on '+' ...
    W[3 - pal[::-1], np.arange(w)] = 250                     # ... (and, being its own reverse complement, on '-')
    seq, borders = make_reads(np.full(200, 40), rng, frac_invalid=0.0)
    for s, _ in borders[::2]:
        seq[s + 11:s + 11 + w] = pal
    valid, fwd, rc = window_scores(seq, W)
    assert (fwd[borders[::2, 0] + 11] == rc[borders[::2, 0] + 11]).all() and (rc > fwd).sum() > 100
    want = run_case(seq, borders, W, (True,), (valid, fwd, rc))[True]
    assert (want[1][::2] == 11).all() and not want[2][::2].any() and want[2][1::2].any()


@pytest.mark.parametrize("w", [6, 9])
def test_self_reverse_complement_matrix_is_never_minus(w):
    ds, seq, borders, _, _ = reads_case(17 if w == 9 else 5)
    rng = np.random.default_rng(40 + w)
    half = rng.integers(-300, 201, size=(4, w)).astype(np.int32)
    key = np.arange(w)[None, :] * 4 + np.arange(4)[:, None]   # entry (b, j) and its partner (3 - b, w - 1 - j) get the same weight
    W = np.ascontiguousarray(np.where(key <= key[::-1, ::-1], half, half[::-1, ::-1]), dtype=np.int32)
    np.testing.assert_array_equal(W, W[::-1, ::-1])
    scored = window_scores(seq, W)
    both, fwd_only = device_scores(ds, W, True), device_scores(ds, W, False)
    check(both, M.np_read_scores(seq, borders, W, True, scored))
    assert both[3] > 1000 and not both[2].any()
    for a, b in zip(both, fwd_only):
        np.testing.assert_array_equal(a, b)


# ---- 6. every score below zero ------------------------------------------------------------------------------------------------------
def test_negative_scores():
    ds, seq, borders, _, _ = reads_case(16)
    rng = np.random.default_rng(36)
    W = rng.integers(-400, -1, size=(4, 16)).astype(np.int32)
    scored = window_scores(seq, W)
    assert scored[1].max() < 0 and scored[2].max() < 0
    for revcom in (True, False):
        want = M.np_read_scores(seq, borders, W, revcom, scored)
        got = device_scores(ds, W, revcom)
        check(got, want)
        assert (got[0][got[1] >= 0] < 0).all() and (got[0][got[1] >= 0] > INT32_MIN).all()


# ---- 7. sizes -------------------------------------------------------------------------------------------------------------------
def test_seventy_thousand_reads():
    rng = np.random.default_rng(37)
    seq, borders = make_reads(np.full(70_000, 20), rng, frac_invalid=0.005)
    want = run_case(seq, borders, asym_matrix(8, rng), (True,))[True]
    assert (want[1][65_536:] >= 0).sum() > 4000


def test_a_read_across_196_tiles():
    rng = np.random.default_rng(38)
    seq, borders = make_reads([40, 200_000, 0, 35], rng, frac_invalid=0.001)
    assert (borders[1, 1] - 1) // 1024 - borders[1, 0] // 1024 + 1 == 196
    W = asym_matrix(31, rng)
    top = np.argmax(W, axis=0)
    for at in (150_000, 150_040, 199_000):                   # the best window three times, far into the read
        seq[borders[1, 0] + at:borders[1, 0] + at + 31] = top
    want = run_case(seq, borders, W)[True]
    assert want[1][1] == 150_000 and want[1][2] == -1


def test_more_tiles_than_one_sweep_of_the_grid():
    """60 000 x 150 bp = 9.06 M positions = 8848 wave tiles > the 8192 one sweep of 2048 blocks of 4 waves covers.  The scores of
    the model are evaluated once per distinct 8-mer and gathered by the window's code (the array is too long for a window matrix);
    the layout is uniform, so the best window of every read is an argmax over a (reads, 151) table -- the first maximum is the
    smallest loc -- which the lexsort model confirms on the first 3000 reads."""
    from kmap_amd.motif_discovery import DeviceSeq
    rng = np.random.default_rng(39)
    w, n_reads, length = 8, 60_000, 150
    seq, borders = make_reads(np.full(n_reads, length), rng, frac_invalid=0.002)
    n = len(seq)
    assert (n + 1023) // 1024 > 8192
    W = asym_matrix(w, rng)
    kmers = ((np.arange(4 ** w)[:, None] >> (2 * (w - 1 - np.arange(w)))[None, :]) & 3).astype(np.uint8)
    tab_fwd = np.concatenate([window_scores(row, W)[1][::w] for row in kmers.reshape(256, 256 * w)])
    tab_rc = np.concatenate([window_scores(row, W)[2][::w] for row in kmers.reshape(256, 256 * w)])
    bad = np.concatenate([[0], np.cumsum(seq == 255)])
    valid = (bad[w:] - bad[:-w]) == 0
    x = np.where(seq == 255, 0, seq).astype(np.int32)
    code = np.zeros(n - w + 1, np.int32)
    for j in range(w):
        code = code * 4 + x[j:n - w + 1 + j]
    fwd, rc = tab_fwd[code], tab_rc[code]
    table = np.full(n_reads * (length + 1), INT32_MIN, np.int64)
    table[:n - w + 1] = np.where(valid, np.maximum(fwd, rc), INT32_MIN)
    table = table.reshape(n_reads, length + 1)
    loc = np.argmax(table, axis=1)
    score = table[np.arange(n_reads), loc]
    minus = np.zeros(n_reads * (length + 1), bool)
    minus[:n - w + 1] = rc > fwd
    want = (np.where(score > INT32_MIN, score, INT32_MIN).astype(np.int32), np.where(score > INT32_MIN, loc, -1).astype(np.int32),
            np.where(score > INT32_MIN, minus.reshape(n_reads, length + 1)[np.arange(n_reads), loc], 0).astype(np.uint8))
    head = 3000
    n_head = int(borders[head, 0])
    direct = M.np_read_scores(seq[:n_head], borders[:head], W, True)
    for a, b in zip(want, direct):
        np.testing.assert_array_equal(a[:head], b)
    ds = DeviceSeq(seq, borders)
    try:
        check(device_scores(ds, W, True), want)
    finally:
        ds.close()


# ---- 8. the golden reads against the existing kernels -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def testfa():
    from kmap_amd.kmer_count import encode_fasta
    from kmap_amd.motif_discovery import DeviceSeq
    seq, borders = encode_fasta(str(GOLD / "test.fa"))
    ds = DeviceSeq(seq, borders)
    yield ds, np.asarray(seq), np.asarray(borders).reshape(-1, 2)
    ds.close()


@pytest.mark.parametrize("matrix,thresholds,reads_hit_1e4", [(MOTIF1, (576, 1062, 1255), 377), (MOTIF0, (457, 962, 1356), 374)])
def test_golden_reads_against_scan_pwm(testfa, matrix, thresholds, reads_hit_1e4):
    from kmap_amd.pwm import pwm_threshold, pwm_weights, read_count_matrix
    ds, seq, borders = testfa
    W = pwm_weights(read_count_matrix(matrix), 1.0)
    assert tuple(pwm_threshold(W, p)[0] for p in (1e-3, 1e-4, 1e-5)) == thresholds
    got = device_scores(ds, W, True)
    check(got, M.np_read_scores(seq, borders, W, True))
    score, loc, strand, _ = got
    for t in thresholds:
        lazy = ds.scan_pwm_lazy(W, t, True)
        n_reads_hit = lazy.n_reads_hit
        del lazy
        above = (loc >= 0) & (score >= t)
        assert int(above.sum()) == n_reads_hit
        if t == thresholds[1]:
            assert n_reads_hit == reads_hit_1e4
        # per read with a hit: the best of scan_pwm's own hits (largest score, then smallest loc) is the read's best window
        hits, pos, scores, strands = ds.scan_pwm(W, t, True)
        read = np.repeat(np.arange(len(hits)), hits)
        order = np.lexsort((pos, -scores.astype(np.int64), read))
        keep = order[np.concatenate([[True], read[order][1:] != read[order][:-1]])]
        np.testing.assert_array_equal(read[keep], np.nonzero(above)[0])
        np.testing.assert_array_equal(pos[keep], loc[above])
        np.testing.assert_array_equal(scores[keep], score[above])
        np.testing.assert_array_equal(strands[keep], strand[above])


# ---- 9. the histogram entry -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [4, 16])
def test_histogram_entry(w):
    """w = 4 has fewer than 4096 different scores (block-private bins), w = 16 more (global bins)"""
    from kmap_amd import _ffi
    ds, seq, borders, W, scored = reads_case(w)
    lo, hi = M.score_range(W)
    assert (hi - lo + 1 <= 4096) == (w == 4)
    want = M.np_read_scores(seq, borders, W, True, scored)
    rs = ds.read_scores(W, True)
    try:
        score, loc, _ = rs.fetch()
        hist = rs.histogram(lo, hi - lo + 1)
        assert hist.dtype == np.uint64
        np.testing.assert_array_equal(hist, np.bincount(score[loc >= 0].astype(np.int64) - lo, minlength=hi - lo + 1))
        np.testing.assert_array_equal(hist, M.np_histogram(want[0], want[1], lo, hi - lo + 1)[0])
        assert int(hist.sum()) == rs.n_scored
        # a range that leaves reads out on both sides: they are counted, and in no bin
        q1, q3 = (int(q) for q in np.quantile(score[loc >= 0], [0.25, 0.75]))
        for a, n_bins in ((q1, q3 - q1), (q1, 5000), (lo - 10, 4096), (hi + 1, 3), (q1, 0)):
            narrow, outside = np.full(n_bins, 7, np.uint64), _ffi.i64(-1)
            assert _ffi.lib().kmap_readscore_hist_dev(rs.score.ptr, rs.loc.ptr, rs.n_seq, a, n_bins, _ffi.ptr(narrow), C.byref(outside), None) == 0
            want_hist, want_outside = M.np_histogram(want[0], want[1], a, n_bins)
            np.testing.assert_array_equal(narrow, want_hist)
            assert outside.value == want_outside and int(narrow.sum()) + outside.value == rs.n_scored
        assert M.np_histogram(want[0], want[1], q1, q3 - q1)[1] > 100
        with pytest.raises(ValueError, match="outside"):
            rs.histogram(q1, q3 - q1)
        # more than 2^22 bins: KMAP_E_UNSUP, nothing written
        big, outside = np.full(8, 7, np.uint64), _ffi.i64(-1)
        assert _ffi.lib().kmap_readscore_hist_dev(rs.score.ptr, rs.loc.ptr, rs.n_seq, lo, 2 ** 22 + 1, _ffi.ptr(big), C.byref(outside), None) == -4
        assert "2^22" in _ffi.last_error() and (big == 7).all() and outside.value == -1
        with pytest.raises(ValueError, match="2\\^22"):
            rs.histogram(lo, 2 ** 22 + 1)
        assert _ffi.lib().kmap_readscore_hist_dev(rs.score.ptr, rs.loc.ptr, rs.n_seq, lo, -1, _ffi.ptr(big), C.byref(outside), None) == -1
        assert _ffi.lib().kmap_readscore_hist_dev(None, rs.loc.ptr, rs.n_seq, lo, 8, _ffi.ptr(big), C.byref(outside), None) == -1
        assert _ffi.lib().kmap_readscore_hist_dev(rs.score.ptr, rs.loc.ptr, rs.n_seq, lo, 8, None, C.byref(outside), None) == -1
        np.testing.assert_array_equal(rs.histogram(lo, hi - lo + 1), hist)
    finally:
        rs.close()


# ---- 10. the verb end to end ------------------------------------------------------------------------------------------------------
CONTROL_SEED = 7


def write_control(path, borders):
    """uniform random reads, as many and as long as the foreground's"""
    rng = np.random.default_rng(CONTROL_SEED)
    with open(path, "w") as fh:
        for i, (s, e) in enumerate(borders.tolist()):
            fh.write(f">control_{i}\n" + "".join("ACGT"[b] for b in rng.integers(0, 4, e - s)) + "\n")


def test_verb_end_to_end(tmp_path, testfa, capsys):
    from kmap_amd import evaluate as E
    from kmap_amd.kmer_count import _preproc
    from kmap_amd.pwm import _scan_pwm, pwm_consensus, pwm_threshold, pwm_weights, read_count_matrix
    _, seq, borders = testfa
    res, ctl = tmp_path / "res", tmp_path / "control.fa"
    _preproc(str(GOLD / "test.fa"), str(res))
    write_control(ctl, borders)
    ctl_seq, ctl_borders = M.encode_fasta_np(ctl)
    np.testing.assert_array_equal(ctl_borders, borders)
    files = [str(MOTIF0), str(MOTIF1)]
    out = tmp_path / "out1"
    capsys.readouterr()
    results = E._evaluate_pwm(str(res), str(ctl), files, read_scores=True, output_dir=str(out))   # p = 1e-4, a = 1, revcom_mode of the config (true)
    printed = capsys.readouterr().out
    lines, names = [], []
    for i, f in enumerate(files):
        Cm = read_count_matrix(f)
        W = pwm_weights(Cm, 1.0)
        t, lo, hi = pwm_threshold(W, 1e-4)
        cons = pwm_consensus(Cm)
        fg, bg = M.np_read_scores(seq, borders, W, True), M.np_read_scores(ctl_seq, ctl_borders, W, True)
        Hf, Hc = M.np_histogram(fg[0], fg[1], lo, hi - lo + 1)[0], M.np_histogram(bg[0], bg[1], lo, hi - lo + 1)[0]
        st = E.evaluate_histograms(Hf, Hc, lo, t, 10)
        lines.append(E.eval_line(i, Cm.shape[1], cons, 1.0, True, int((fg[1] < 0).sum()), int((bg[1] < 0).sum()), st))
        names += [E.HIST_FILE.format(i=i, consensus=cons), E.READS_FILE.format(i=i, consensus=cons)]
        E.write_score_hist(tmp_path / "want_hist.csv", Hf, Hc, lo)
        E.write_read_scores(tmp_path / "want_reads.tsv", *fg)
        assert (out / names[-2]).read_bytes() == (tmp_path / "want_hist.csv").read_bytes()
        assert (out / names[-1]).read_bytes() == (tmp_path / "want_reads.tsv").read_bytes()
        np.testing.assert_array_equal(results[i]["Hf"], Hf)
        np.testing.assert_array_equal(results[i]["Hc"], Hc)
        assert results[i]["best"] == st["best"] and results[i]["U2"] == st["U2"]
        # sanity, not a measurement: 401 of the 1002 reads carry the motif, so about 0.7 is expected
        assert st["auroc"] > 0.6 and st["mw_z"] > 5 and st["best"] is not None and st["best"][3] > 5
        assert st["n_fg"] + results[i]["fg_unscorable"] == len(borders) == st["n_control"] + results[i]["control_unscorable"]
        assert f"motif {i} {cons}" in printed
    E.write_eval_table(tmp_path / "want_eval.csv", lines)
    assert (out / "pwm_eval.csv").read_bytes() == (tmp_path / "want_eval.csv").read_bytes()
    assert sorted(p.name for p in out.iterdir()) == sorted(names + ["pwm_eval.csv"])
    # a(t_p) is scan_pwm's reads-with-a-hit on the same directory
    _scan_pwm(str(res), files, output_dir=str(tmp_path / "scan"))
    info = (tmp_path / "scan" / "pwm_info.csv").read_text().splitlines()
    table = (out / "pwm_eval.csv").read_text().splitlines()
    cols = table[0].split(",")
    for i in range(2):
        row = dict(zip(cols, table[1 + i].split(",")))
        assert row["fg_reads_p"] == info[1 + i].split(",")[-1] == ("374", "377")[i]
        assert row["threshold_p"] == info[1 + i].split(",")[6] == ("962", "1062")[i]
    # a second run writes the same bytes; without --read_scores no per-read file; forward strand, a score threshold, the default directory
    E._evaluate_pwm(str(res), str(ctl), files, read_scores=True, output_dir=str(tmp_path / "out2"))
    for name in names + ["pwm_eval.csv"]:
        assert (tmp_path / "out2" / name).read_bytes() == (out / name).read_bytes(), name
    fwd = E._evaluate_pwm(str(res), str(ctl), [files[1]], min_score=10.62, revcom_mode=False, min_reads=10 ** 6)
    assert sorted(p.name for p in (res / "pwm_eval").iterdir()) == ["pwm_eval.csv", "score_hist_motif0_ACCTACGTA.csv"]
    W = pwm_weights(read_count_matrix(files[1]), 1.0)
    fg = M.np_read_scores(seq, borders, W, False)
    assert fwd[0]["threshold_p"] == 1062 and fwd[0]["fg_reads_p"] == int(((fg[1] >= 0) & (fg[0] >= 1062)).sum()) and fwd[0]["best"] is None
    assert (res / "pwm_eval" / "pwm_eval.csv").read_text().splitlines()[1].endswith(",,,,,nan")
    assert "no best threshold" in capsys.readouterr().out


# ---- 11. errors and neighbours ------------------------------------------------------------------------------------------------------
def test_errors_and_the_scan_handle_is_left_alone():
    from kmap_amd import _ffi
    ds, seq, borders, W, scored = reads_case(16)
    lib = _ffi.lib()
    t = int(np.quantile(scored[1][scored[0]], 0.99))
    want = M.np_read_scores(seq, borders, W, True, scored)
    pwm_before = ds.scan_pwm(W, t, True)
    assert pwm_before[0].sum() > 0
    check(device_scores(ds, W, True), want)
    kept = [np.empty_like(a) for a in pwm_before]            # the scan's lists are still the handle's
    assert lib.kmap_pwm_scan_fetch(ds._scan, *[_ffi.ptr(a) for a in kept]) == 0
    for a, b, c in zip(pwm_before, kept, ds.scan_pwm(W, t, True)):
        np.testing.assert_array_equal(a, b)
        np.testing.assert_array_equal(a, c)
    # width outside 4..31, NULL weights, NULL result arrays, a negative size: KMAP_E_INVAL with a message, nothing written
    out = [_ffi.DeviceBuffer(ds.n_seq * 4), _ffi.DeviceBuffer(ds.n_seq * 4), _ffi.DeviceBuffer(ds.n_seq)]
    for b in out:
        check_rc = lib.kmap_memset(b.ptr, 7, b.nbytes, None)
        assert check_rc == 0
    n_scored = _ffi.i64(-5)

    def call(width, weights, score=out[0].ptr, n=ds.n, n_seq=ds.n_seq, codes=ds.codes.ptr):
        return lib.kmap_readscore_packed_dev(codes, ds.inval_orig.ptr, n, ds.borders.ptr, n_seq, width, weights, 1, score, out[1].ptr,
                                             out[2].ptr, C.byref(n_scored), None)
    Wc = np.ascontiguousarray(W, np.int32)
    for width in (3, 32):
        Wb = np.zeros((4, width), np.int32)
        assert call(width, _ffi.ptr(Wb)) == -1 and str(width) in _ffi.last_error()
        with pytest.raises(ValueError):
            ds.read_scores(Wb, True)
    assert call(16, None) == -1 and "weights" in _ffi.last_error()
    assert call(16, _ffi.ptr(Wc), n=-1) == -1 and call(16, _ffi.ptr(Wc), n_seq=-1) == -1
    assert n_scored.value == -5
    assert call(16, _ffi.ptr(Wc), score=None) == -1 and call(16, _ffi.ptr(Wc), codes=None) == -1
    _ffi.sync()
    assert (out[0].to_numpy(np.uint8, (ds.n_seq * 4,)) == 7).all() and (out[2].to_numpy(np.uint8, (ds.n_seq,)) == 7).all()
    with pytest.raises(ValueError):
        ds.read_scores(np.zeros((3, 8), np.int32), True)
    # no reads: nothing is written; no positions: every read is unscorable
    assert call(16, _ffi.ptr(Wc), n_seq=0) == 0 and n_scored.value == 0
    _ffi.sync()
    assert (out[1].to_numpy(np.uint8, (ds.n_seq * 4,)) == 7).all()
    n_scored.value = -5
    assert call(16, _ffi.ptr(Wc), n=0) == 0 and n_scored.value == 0
    _ffi.sync()
    assert (out[0].to_numpy(np.int32, (ds.n_seq,)) == INT32_MIN).all() and (out[1].to_numpy(np.int32, (ds.n_seq,)) == -1).all()
    assert not out[2].to_numpy(np.uint8, (ds.n_seq,)).any()
    for b in out:
        b.free()
    check(device_scores(ds, W, True), want)                  # and the next call is as good as the first
