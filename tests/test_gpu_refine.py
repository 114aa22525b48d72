"""refine_pwm on the GPU (csrc/pwm_refine.hip) against the numpy restatement of tests/_refine_model.py: the
hits of section 11, the selection (every hit, or per read the largest score and the smallest loc on a tie) and the count matrix of
the selected windows' oriented bases.  Every comparison is exact integer equality."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

from tests import _refine_model as M
from tests._refine_model import asym_matrix, make_reads

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
GOLD = ROOT / "tests" / "golden"
MOTIF0, MOTIF1 = GOLD / "report_testfa" / "cntmat_motif0_CAATCGATAGC.csv", GOLD / "report_testfa" / "cntmat_motif1_ACCTACGTA.csv"


def check(got, want):
    """(C', n_hits, n_selected, n_minus) of DeviceSeq.pwm_counts against the model's"""
    assert got[0].dtype == np.int64 and got[0].shape == want[0].shape
    np.testing.assert_array_equal(got[0], want[0], err_msg="counts")
    assert tuple(int(x) for x in got[1:]) == tuple(int(x) for x in want[1:]), "n_hits, n_selected, n_minus"
    np.testing.assert_array_equal(got[0].sum(axis=0), np.full(got[0].shape[1], got[2]))   # every column sums to n_selected


_CASES = {}


def reads_case(w):
    """~3000 reads of lengths 0..70 per width, built once: (DeviceSeq, seq, borders, W, (valid, fwd, rc))"""
    if w not in _CASES:
        from kmap_amd.motif_discovery import DeviceSeq
        rng = np.random.default_rng(2000 + w)
        special = [w - 1, w, w + 1, 0, 15, 16, 17, 31, 32, 33, 47, 48]
        lengths = np.concatenate([special, rng.integers(0, 71, 2990), special[::-1]])
        lengths = lengths[rng.permutation(len(lengths))]
        seq, borders = make_reads(lengths, rng)
        W = asym_matrix(w, rng)
        _CASES[w] = (DeviceSeq(seq, borders), seq, borders, W, M.window_scores(seq, W))
    return _CASES[w]


# ---- 1. the kernels against the model ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("revcom", [True, False])
@pytest.mark.parametrize("w", [4, 5, 16, 17, 31])
def test_kernel_against_model(w, revcom):
    ds, seq, borders, W, scored = reads_case(w)
    valid, fwd, rc = scored
    score = np.maximum(fwd, rc) if revcom else fwd
    lo, hi = int(W.min(axis=0).sum()), int(W.max(axis=0).sum())
    assert valid.sum() > 5000 and not valid.all()
    t_q = int(np.quantile(score[valid], 0.99))
    for best in (True, False):
        for t, kind in ((t_q, "quantile"), (lo, "all"), (hi + 1, "none")):
            want = M.np_counts(seq, borders, W, t, revcom, best, scored)
            got = ds.pwm_counts(W, t, revcom, best)
            check(got, want)
            counts, n_hits, n_sel, n_minus = got
            if kind == "none":
                assert n_hits == n_sel == n_minus == 0 and not counts.any()
                continue
            reads_hit = len(np.unique(M.np_hits(seq, borders, W, t, revcom, scored)[0]))
            if best:
                assert n_sel == reads_hit and n_sel < n_hits
            else:
                assert n_sel == n_hits
            if kind == "all":
                assert n_hits == int(valid.sum())
                if not best:
                    np.testing.assert_array_equal(counts.sum(axis=0), np.full(w, int(valid.sum())))
            else:
                assert 0 < n_hits < 0.1 * valid.sum()
            if revcom:
                assert 0 < n_minus < n_sel
            else:
                assert n_minus == 0


# ---- 1b. the sparse traversal at the group, wave-tile and block edges ------------------------------------------------------------
@pytest.mark.parametrize("w", [9, 31])
@pytest.mark.parametrize("shift", [-1, 0, 1])
def test_read_starts_at_tile_edges(shift, w):
    """reads that start exactly at 16, 1024, 2048, 4096 and 5136 (+ shift), tests/_refine_model.py edge_reads: every window a hit (a
    lane walks all 16 bits and every border) and one in ten (the search for a lane's first hit places the read)"""
    from kmap_amd.motif_discovery import DeviceSeq
    seq, borders, W, scored, _ = M.edge_reads(shift, w)
    valid, fwd, rc = scored
    lo = int(W.min(axis=0).sum())
    ds = DeviceSeq(seq, borders)
    try:
        for revcom in (True, False):
            M.check_edge_hits(shift, w, M.np_hits(seq, borders, W, lo, revcom, scored), revcom)
            for t in (lo, int(np.quantile((np.maximum(fwd, rc) if revcom else fwd)[valid], 0.9))):
                for best in (True, False):
                    want = M.np_counts(seq, borders, W, t, revcom, best, scored)
                    assert (want[1] == valid.sum()) if t == lo else (0 < want[1] < 0.2 * valid.sum())
                    check(ds.pwm_counts(W, t, revcom, best), want)
    finally:
        ds.close()


# ---- 2. ties --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("revcom", [True, False])
def test_best_takes_the_smaller_loc_on_a_score_tie(revcom):
    """two different windows with the same top score in one read: A and C weigh the same in column 0, so which of the two was
    selected shows in C'[:, 0]"""
    from kmap_amd.motif_discovery import DeviceSeq
    rng = np.random.default_rng(21)
    w = 8
    W = asym_matrix(w, rng)
    W[rng.integers(0, 4, w), np.arange(w)] = 250            # one best base per column ...
    W[:, 0] = [200, 200, -410, -420]                         # ... but two in the first
    top = np.argmax(W, axis=0).astype(np.uint8)
    hi = int(W.max(axis=0).sum())
    with_a, with_c = top.copy(), top.copy()
    with_a[0], with_c[0] = 0, 1
    n_x, n_y, n_plain = 150, 90, 60
    lengths = np.full(n_x + n_y + n_plain, 40)
    starts = np.arange(len(lengths)) * 41
    seq = rng.integers(0, 4, int((lengths + 1).sum())).astype(np.uint8)
    seq[starts + 40] = 255
    for i, s in enumerate(starts[:n_x + n_y]):
        first, second = (with_c, with_a) if i < n_x else (with_a, with_c)
        seq[s + 5:s + 5 + w], seq[s + 20:s + 20 + w] = first, second
    borders = np.stack([starts, starts + lengths], axis=1)
    want = M.np_counts(seq, borders, W, hi, revcom, True)
    r, loc, _, score, minus = M.np_hits(seq, borders, W, hi, revcom)
    assert (score == hi).all() and not minus.any() and set(loc.tolist()) == {5, 20} and len(r) == 2 * (n_x + n_y)
    ds = DeviceSeq(seq, borders)
    try:
        got = ds.pwm_counts(W, hi, revcom, True)
        check(got, want)
        assert got[1:] == (2 * (n_x + n_y), n_x + n_y, 0)
        np.testing.assert_array_equal(got[0][:, 0], [n_y, n_x, 0, 0])            # the window at loc 5, never the one at loc 20
        np.testing.assert_array_equal(got[0][:, 1:].max(axis=0), np.full(w - 1, n_x + n_y))
        every = ds.pwm_counts(W, hi, revcom, False)
        check(every, M.np_counts(seq, borders, W, hi, revcom, False))
        np.testing.assert_array_equal(every[0][:, 0], [n_x + n_y, n_x + n_y, 0, 0])
    finally:
        ds.close()


@pytest.mark.parametrize("w", [6, 9, 16])
def test_self_reverse_complement_matrix_counts_plus_only(w):
    ds, seq, borders, _, _ = reads_case(16 if w == 16 else 17 if w == 9 else 5)
    rng = np.random.default_rng(40 + w)
    half = rng.integers(-300, 201, size=(4, w)).astype(np.int32)
    key = np.arange(w)[None, :] * 4 + np.arange(4)[:, None]   # entry (b, j) and its partner (3 - b, w - 1 - j) get the same weight
    W = np.ascontiguousarray(np.where(key <= key[::-1, ::-1], half, half[::-1, ::-1]), dtype=np.int32)
    np.testing.assert_array_equal(W, W[::-1, ::-1])          # equal to its own reverse complement
    scored = M.window_scores(seq, W)
    np.testing.assert_array_equal(scored[1], scored[2])
    for t in (int(W.min(axis=0).sum()), int(np.quantile(scored[1][scored[0]], 0.9))):
        for best in (True, False):
            got = ds.pwm_counts(W, t, True, best)
            check(got, M.np_counts(seq, borders, W, t, True, best, scored))
            assert got[2] > 100 and got[3] == 0
            fwd_only = ds.pwm_counts(W, t, False, best)
            np.testing.assert_array_equal(got[0], fwd_only[0])
            assert got[1:] == fwd_only[1:]


# ---- 3. more than 65 535 reads ------------------------------------------------------------------------------------------------
def test_seventy_thousand_reads():
    from kmap_amd.motif_discovery import DeviceSeq
    rng = np.random.default_rng(2)
    seq, borders = make_reads(np.full(70_000, 20), rng, frac_invalid=0.005)
    W = asym_matrix(8, rng)
    scored = M.window_scores(seq, W)
    t = int(np.quantile(np.maximum(scored[1], scored[2])[scored[0]], 0.95))
    r = M.np_hits(seq, borders, W, t, True, scored)[0]
    assert (r >= 65_536).sum() > 1000 and len(r) > len(np.unique(r)) > 20_000
    ds = DeviceSeq(seq, borders)
    try:
        got = ds.pwm_counts(W, t, True, True)
        check(got, M.np_counts(seq, borders, W, t, True, True, scored))
        assert got[2] == len(np.unique(r))
    finally:
        ds.close()


# ---- 4. a read across many tiles ----------------------------------------------------------------------------------------------
def test_long_read():
    from kmap_amd.motif_discovery import DeviceSeq
    rng = np.random.default_rng(3)
    seq, borders = make_reads([40, 200_000, 0, 35], rng, frac_invalid=0.001)
    W = asym_matrix(31, rng)
    scored = M.window_scores(seq, W)
    t = int(np.quantile(np.maximum(scored[1], scored[2])[scored[0]], 0.99))
    r = M.np_hits(seq, borders, W, t, True, scored)[0]
    in_long = int((r == 1).sum())
    assert in_long > 255 and not (r == 2).any()
    ds = DeviceSeq(seq, borders)
    try:
        best = ds.pwm_counts(W, t, True, True)
        check(best, M.np_counts(seq, borders, W, t, True, True, scored))
        assert best[1] == len(r) and best[2] == len(np.unique(r)) <= 3           # exactly one window of the long read
        every = ds.pwm_counts(W, t, True, False)
        check(every, M.np_counts(seq, borders, W, t, True, False, scored))
        assert every[2] == len(r) >= in_long
    finally:
        ds.close()


# ---- 5. more tiles than one sweep of the persistent grid -----------------------------------------------------------------------
def test_grid_stride_keeps_the_block_histograms():
    """60 000 x 150 bp = 9.06 M positions = 8848 wave tiles > the 8192 one sweep of 2048 blocks of 4 waves covers.  The scores of
    the model, evaluated once per distinct 8-mer and gathered by the window's code (the array is too long for a window matrix)."""
    from kmap_amd.motif_discovery import DeviceSeq
    rng = np.random.default_rng(5)
    w = 8
    seq, borders = make_reads(np.full(60_000, 150), rng, frac_invalid=0.002)
    n = len(seq)
    assert (n + 1023) // 1024 > 8192
    W = asym_matrix(w, rng)
    kmers = ((np.arange(4 ** w)[:, None] >> (2 * (w - 1 - np.arange(w)))[None, :]) & 3).astype(np.uint8)
    # each row of 256 8-mers laid end to end: the windows at multiples of w are the 8-mers themselves
    tab_fwd = np.concatenate([M.window_scores(row, W)[1][::w] for row in kmers.reshape(256, 256 * w)])
    tab_rc = np.concatenate([M.window_scores(row, W)[2][::w] for row in kmers.reshape(256, 256 * w)])
    bad = np.concatenate([[0], np.cumsum(seq == 255)])
    valid = (bad[w:] - bad[:-w]) == 0
    x = np.where(seq == 255, 0, seq).astype(np.int32)
    code = np.zeros(n - w + 1, np.int32)
    for j in range(w):
        code = code * 4 + x[j:n - w + 1 + j]
    scored = (valid, tab_fwd[code], tab_rc[code])
    sl = slice(1000, 1400)                                    # the gathered scores are the model's own on a stretch
    direct = M.window_scores(seq[sl.start:sl.stop + w - 1], W)
    np.testing.assert_array_equal(scored[1][sl], direct[1])
    np.testing.assert_array_equal(scored[2][sl], direct[2])
    np.testing.assert_array_equal(scored[0][sl], direct[0])
    t = int(np.quantile(np.maximum(scored[1], scored[2])[::97], 0.999))
    p = M.np_hits(seq, borders, W, t, True, scored)[2]
    assert 2000 < len(p) < 50_000 and p.min() < 1024 * 1000 and p.max() > 1024 * 8500   # hits in the first sweep and in the second
    ds = DeviceSeq(seq, borders)
    try:
        for best in (True, False):
            check(ds.pwm_counts(W, t, True, best), M.np_counts(seq, borders, W, t, True, best, scored))
    finally:
        ds.close()


# ---- 6. the golden reads and matrices ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def testfa():
    from kmap_amd.kmer_count import encode_fasta
    from kmap_amd.motif_discovery import DeviceSeq
    seq, borders = encode_fasta(str(GOLD / "test.fa"))
    ds = DeviceSeq(seq, borders)
    yield ds, np.asarray(seq), np.asarray(borders).reshape(-1, 2)
    ds.close()


# start, flank, select, max_iter -> threshold / hits / selected / minus per iteration, status, consensus (p = 1e-4, a = 1, both strands)
ANCHORS = [
    ("motif1", 0, "best", 20, [(1062, 488, 377, 6), (712, 411, 385, 3), (708, 411, 385, 2), (708, 411, 385, 2)], "converged", "ACCTACGTA"),
    ("motif1", 2, "best", 20, [(1062, 453, 358, 6), (501, 405, 381, 4), (508, 399, 381, 3), (512, 399, 382, 3), (524, 397, 382, 3)],
     "converged", "GGACCTACGTACC"),
    ("motif0", 0, "all", 20, [(962, 507, 507, 133), (877, 506, 506, 133), (873, 506, 506, 133)], "converged", "CAATCGATAGC"),
    ("motif0", 0, "best", 20, [(962, 507, 374, 3), (722, 398, 373, 1), (716, 377, 372, 1), (708, 376, 372, 1)], "converged", "AAATCGATAGC"),
    ("motif0", 2, "all", 5, {0: (962, 449, 449, 117), 4: (894, 585, 585, 275)}, "max_iter", "CGCAATCGATAGCGT"),
]


@pytest.mark.parametrize("start,flank,select,max_iter,rows,status,consensus", ANCHORS)
def test_golden_reads(testfa, start, flank, select, max_iter, rows, status, consensus):
    from kmap_amd.pwm import pwm_consensus, read_count_matrix
    from kmap_amd.refine import refine_matrix
    ds, seq, borders = testfa
    model_seq, model_borders = M.encode_fasta_np(GOLD / "test.fa")
    assert seq.dtype == np.uint8 and seq.shape == (45_979,)
    np.testing.assert_array_equal(seq, model_seq)            # the array the anchors were computed on
    np.testing.assert_array_equal(borders, model_borders)
    C0 = read_count_matrix(MOTIF0 if start == "motif0" else MOTIF1)
    best = select == "best"
    want = refine_matrix(C0, M.model_count_fn(model_seq, model_borders, True, best), flank, 1e-4, 1.0, max_iter)
    got = refine_matrix(C0, lambda W, t: ds.pwm_counts(W, t, True, best), flank, 1e-4, 1.0, max_iter)
    np.testing.assert_array_equal(got[0], want[0])           # the model is the arbiter ...
    assert got[1] == want[1] and got[2] == want[2]
    assert got[1] == status and pwm_consensus(got[0]) == consensus               # ... the listed figures a second anchor
    if isinstance(rows, dict):
        assert len(got[2]) == max_iter
        for i, row in rows.items():
            assert got[2][i][1:5] == row
    else:
        assert [r[1:5] for r in got[2]] == rows


# ---- 7. the verb end to end ---------------------------------------------------------------------------------------------------
def test_verb_end_to_end(tmp_path, testfa, capsys):
    from kmap_amd.kmer_count import _preproc
    from kmap_amd.pwm import _scan_pwm, pwm_consensus, read_count_matrix
    from kmap_amd.refine import _refine_pwm, refine_matrix, trace_line
    _, seq, borders = testfa
    res = tmp_path / "res"
    _preproc(str(GOLD / "test.fa"), str(res))
    files = [str(MOTIF0), str(MOTIF1)]
    out = tmp_path / "out1"
    capsys.readouterr()
    runs = _refine_pwm(str(res), files, flank=2, output_dir=str(out))            # best, p = 1e-4, a = 1, revcom_mode of the config (true)
    printed = capsys.readouterr().out
    want = [refine_matrix(read_count_matrix(f), M.model_count_fn(seq, borders, True, True), 2) for f in files]
    cons = [pwm_consensus(w[0]) for w in want]
    assert cons[1] == "GGACCTACGTACC"
    names = [f"refined_cntmat_motif{i}_{c}.csv" for i, c in enumerate(cons)]
    assert sorted(f.name for f in out.iterdir()) == sorted(names + ["refine_info.csv", "refine_trace.csv"])
    for i, (run, exp) in enumerate(zip(runs, want)):
        np.testing.assert_array_equal(run[0], exp[0])
        assert run[1] == exp[1] and run[2] == exp[2]
        np.testing.assert_array_equal(read_count_matrix(out / names[i]), exp[0])
        assert f"motif {i} " in printed and cons[i] in printed
    trace = (out / "refine_trace.csv").read_text().splitlines(keepends=True)
    assert trace[0] == "motif,iteration,threshold,n_hits,n_selected,n_minus,consensus,information_bits,cells_changed\n"
    assert trace[1:] == [trace_line(i, row) for i, exp in enumerate(want) for row in exp[2]]
    assert trace[1 + len(want[0][2])].startswith("1,1,1062,453,358,6,") and len(trace[1].split(",")) == 9
    assert all(len(ln.split(",")[7].split(".")[1]) == 3 for ln in trace[1:])   # %.3f
    info = (out / "refine_info.csv").read_text().splitlines()
    assert info[0] == "motif,matrix_file,width_in,flank,width,select,pseudocount,p_value,status,iterations,consensus_in,consensus,refined_file"
    assert info[1] == f"0,{files[0]},11,2,15,best,1.0,0.0001,{want[0][1]},{len(want[0][2])},CAATCGATAGC,{cons[0]},{names[0]}"
    assert info[2] == f"1,{files[1]},9,2,13,best,1.0,0.0001,converged,5,ACCTACGTA,GGACCTACGTACC,{names[1]}"
    # scan_pwm takes the refined file as it is
    per = _scan_pwm(str(res), [str(out / names[1])], output_dir=str(tmp_path / "scan"))
    assert (tmp_path / "scan" / "pwm_conseq.txt").read_text() == "GGACCTACGTACC\n" and len(per[0][1]) == want[1][2][-1][2] == 397
    # a second run writes the same bytes
    _refine_pwm(str(res), files, flank=2, output_dir=str(tmp_path / "out2"))
    for name in names + ["refine_info.csv", "refine_trace.csv"]:
        assert (tmp_path / "out2" / name).read_bytes() == (out / name).read_bytes(), name
    # forward strand only, every hit, a limit of two iterations, the default directory
    fwd = _refine_pwm(str(res), [files[1]], select="all", revcom_mode=False, max_iter=2)
    exp = refine_matrix(read_count_matrix(files[1]), M.model_count_fn(seq, borders, False, False), 0, max_iter=2)
    np.testing.assert_array_equal(fwd[0][0], exp[0])
    assert fwd[0][1:] == exp[1:] and all(row[4] == 0 for row in fwd[0][2]) and fwd[0][2][0][1:4] == (1062, 377, 377)
    assert (res / "pwm_refine" / "refine_info.csv").read_text().splitlines()[1].split(",")[5] == "all"


# ---- 8. errors and neighbours ---------------------------------------------------------------------------------------------------
def test_errors_and_the_scan_handle_is_left_alone():
    from kmap_amd import _ffi
    from kmap_amd.kmer_count import kmer2hash
    ds, seq, borders, W, scored = reads_case(16)
    lib = _ffi.lib()
    t = int(np.quantile(scored[1][scored[0]], 0.99))
    ham_before = ds.scan(8, kmer2hash("ACGTACGT"), 2, True)
    assert ham_before[0].sum() > 0
    hits, mind, pos = np.empty(ds.n_seq, np.int32), np.empty(ds.n_seq, np.int8), np.empty(len(ham_before[1]), np.int32)
    assert lib.kmap_scan_fetch(ds._scan, _ffi.ptr(hits), _ffi.ptr(mind), _ffi.ptr(pos)) == 0
    want = M.np_counts(seq, borders, W, t, True, True, scored)
    check(ds.pwm_counts(W, t, True, True), want)
    # the Hamming run's lists and minimum distances are still the handle's
    hits2, mind2, pos2 = np.empty_like(hits), np.empty_like(mind), np.empty_like(pos)
    assert lib.kmap_scan_fetch(ds._scan, _ffi.ptr(hits2), _ffi.ptr(mind2), _ffi.ptr(pos2)) == 0
    for a, b in ((hits, hits2), (mind, mind2), (pos, pos2), (hits, ham_before[0]), (pos, ham_before[1])):
        np.testing.assert_array_equal(a, b)
    # a PWM scan before and after: identical lists, and its handle state survives a pwm_counts too
    pwm_before = ds.scan_pwm(W, t, True)
    check(ds.pwm_counts(W, t, False, False), M.np_counts(seq, borders, W, t, False, False, scored))
    kept = [np.empty_like(a) for a in pwm_before]
    assert lib.kmap_pwm_scan_fetch(ds._scan, *[_ffi.ptr(a) for a in kept]) == 0
    for a, b, c in zip(pwm_before, kept, ds.scan_pwm(W, t, True)):
        np.testing.assert_array_equal(a, b)
        np.testing.assert_array_equal(a, c)
    ham_after = ds.scan(8, kmer2hash("ACGTACGT"), 2, True)
    np.testing.assert_array_equal(ham_after[0], ham_before[0])
    np.testing.assert_array_equal(ham_after[1], ham_before[1])
    # width outside 4..31, NULL weights, select_best = 2: KMAP_E_INVAL with a message
    nums = [_ffi.i64(7) for _ in range(3)]
    out = np.full((4, 32), 7, np.int64)

    def call(width, weights, select_best):
        return lib.kmap_refine_counts_packed_dev(ds.codes.ptr, ds.inval_orig.ptr, ds.n, ds.borders.ptr, ds.n_seq, width, weights, 0, 1,
                                                 select_best, _ffi.ptr(out), C.byref(nums[0]), C.byref(nums[1]), C.byref(nums[2]), None)
    for width in (3, 32):
        Wb = np.zeros((4, width), np.int32)
        assert call(width, _ffi.ptr(Wb), 1) == -1 and str(width) in _ffi.last_error()            # KMAP_E_INVAL
        with pytest.raises(ValueError):
            ds.pwm_counts(Wb, 0, True, True)
    Wc = np.ascontiguousarray(W, np.int32)
    assert call(16, None, 1) == -1 and "weights" in _ffi.last_error()
    assert call(16, _ffi.ptr(Wc), 2) == -1 and "select_best" in _ffi.last_error()
    assert (out == 7).all()                                  # a refused call writes nothing
    with pytest.raises(ValueError):
        ds.pwm_counts(np.zeros((3, 8), np.int32), 0, True, True)
    with pytest.raises(ValueError):
        ds.pwm_counts(Wc, 2 ** 31, True, True)
    check(ds.pwm_counts(W, t, True, True), want)             # and the next call is as good as the first
    # no reads, or no positions: zeros
    for n, n_seq in ((ds.n, 0), (0, ds.n_seq), (0, 0)):
        out[:] = 7
        assert lib.kmap_refine_counts_packed_dev(ds.codes.ptr, ds.inval_orig.ptr, n, ds.borders.ptr, n_seq, 16, _ffi.ptr(Wc), -10 ** 6, 1, 1,
                                                 _ffi.ptr(out), C.byref(nums[0]), C.byref(nums[1]), C.byref(nums[2]), None) == 0
        assert not out.ravel()[:64].any() and (out.ravel()[64:] == 7).all() and [x.value for x in nums] == [0, 0, 0]
