"""rank_motif_library on the GPU (csrc/pwm_library.hip).  The yardstick is never the new kernel: on small inputs
it is the numpy restatement of tests/_readscore_model.py (per read the best window score, reduced to a histogram), on the large one
the existing per-matrix device path DeviceSeq.read_scores(...).histogram(...).  Histograms, n_outside and n_scored are compared as
equal integers; the verb's table field by field with evaluate_pwm's."""
from pathlib import Path

import numpy as np
import pytest

from tests import _readscore_model as M
from tests._refine_model import asym_matrix, make_reads, window_scores

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
GOLD = ROOT / "tests" / "golden"
LIB = GOLD / "library"
MOTIF0 = GOLD / "report_testfa" / "cntmat_motif0_CAATCGATAGC.csv"


def model(seq, borders, W, revcom, lo=None, n_bins=None, scored=None):
    """(histogram, n_outside, n_scored) of one matrix; the default range is every possible score"""
    if lo is None:
        lo, hi = M.score_range(W)
        n_bins = hi - lo + 1
    score, loc, _ = M.np_read_scores(seq, borders, W, revcom, scored)
    hist, outside = M.np_histogram(score, loc, lo, n_bins)
    return hist, outside, int((loc >= 0).sum())


def full_ranges(Ws):
    los = [M.score_range(W)[0] for W in Ws]
    return los, [M.score_range(W)[1] - lo + 1 for W, lo in zip(Ws, los)]


def check_against(got, want):
    """library_histograms' result against [(histogram, n_outside, n_scored)] per matrix"""
    hists, outside, scored = got
    assert len(hists) == len(outside) == len(scored) == len(want)
    assert outside.dtype == np.int64 and scored.dtype == np.int64
    for m, (h, o, s) in enumerate(want):
        assert hists[m].dtype == np.uint64 and hists[m].shape == h.shape
        np.testing.assert_array_equal(hists[m], h, err_msg=f"histogram of matrix {m}")
        assert (int(outside[m]), int(scored[m])) == (o, s), f"matrix {m}"
        assert int(hists[m].sum()) + o == s


# ---- 1. edges -----------------------------------------------------------------------------------------------------------------------
def edge_reads():
    """(seq, borders, Ws): ~300 reads of lengths 0..200 (fixed seed) and: a read that begins in the last group of the first wave tile and ends in the
    second tile, a read across three tiles, empty reads that share their start with the read behind them, 2 % invalid bases, n no
    multiple of 16; the best window of matrix `minus` planted as its reverse complement only.  A plain function: the stale-state
    cases of tests/test_gpu_stale_state.py run on the same reads."""
    rng = np.random.default_rng(1600)
    lengths, at = [], 0
    while 1015 - at > 210:                                   # random reads up to the first tile's end ...
        lengths.append(int(rng.integers(0, 201)))
        at += lengths[-1] + 1
    lengths.append(1015 - at - 1)                            # ... so that the next one starts at 1015: lane 63 of the first tile
    i_cross = len(lengths)
    lengths += [60]                                          # 1015 .. 1075: ends in the second tile
    i_long = len(lengths) + 3
    lengths += [int(x) for x in rng.integers(0, 201, 3)] + [2100]
    lengths += [int(x) for x in rng.integers(0, 201, 290 - len(lengths))] + [0, 3, 4, 5, 30, 31, 32, 0, 0, 77]
    if (sum(lengths) + len(lengths) - 1) % 16 == 0:          # positions: the reads and a 255 behind every one but the last
        lengths[-1] += 1
    seq, borders = make_reads(lengths, rng, frac_invalid=0.02, last_separator=False)
    assert borders[i_cross, 0] == 1015 and borders[i_cross, 0] // 1024 == 0 and (borders[i_cross, 1] - 1) // 1024 == 1
    assert (borders[i_long, 1] - 1) // 1024 - borders[i_long, 0] // 1024 >= 2 and len(seq) % 16 != 0
    # empty reads that share a start: two in front of five reads each (the borders still ascend; the read behind them is the last
    # one that starts there, so its windows are its own)
    extra = [i_cross, i_long, 7, 100, len(lengths) - 1]
    rows = []
    for r, b in enumerate(borders.tolist()):
        if r in extra:
            rows += [[b[0], b[0]], [b[0], b[0]]]
        rows.append(b)
    borders = np.array(rows, np.int64)
    assert (np.diff(borders[:, 0]) >= 0).all() and len(borders) == 300 + 2 * len(extra)
    Ws = {w: asym_matrix(w, rng) for w in (4, 5, 11, 16, 17, 31)}
    Ws["ties"] = np.full((4, 8), 7, np.int32)                # every window ties
    Ws["minus"] = asym_matrix(12, rng)
    top = np.argmax(Ws["minus"], axis=0).astype(np.uint8)
    n_planted = 0
    for s, e in borders[::4]:
        if e - s >= 40:
            seq[s + 20:s + 32] = 3 - top[::-1]
            n_planted += 1
    assert n_planted > 20
    return seq, borders, Ws


@pytest.fixture(scope="module")
def edge_set():
    """edge_reads() on the device; the model's scores per matrix are computed once"""
    from kmap_amd.motif_discovery import DeviceSeq
    seq, borders, Ws = edge_reads()
    scored = {k: window_scores(seq, W) for k, W in Ws.items()}
    ds = DeviceSeq(seq, borders)
    yield ds, seq, borders, Ws, scored
    ds.close()


@pytest.mark.parametrize("revcom", [True, False])
def test_edges_all_widths_in_one_call(edge_set, revcom):
    ds, seq, borders, Ws, scored = edge_set
    names = [4, 5, 11, 16, 17, 31, "ties", "minus"]
    mats = [Ws[k] for k in names]
    want = [model(seq, borders, Ws[k], revcom, scored=scored[k]) for k in names]
    los, nbs = full_ranges(mats)
    check_against(ds.library_histograms(mats, los, nbs, revcom), want)
    by = dict(zip(names, want))
    length = borders[:, 1] - borders[:, 0]
    # scorable for the narrow matrix and not for the wide one: reads of 4 .. 30 bases exist, and n_scored says so
    assert ((length >= 4) & (length < 31)).sum() > 20 and by[4][2] > by[31][2] > 0
    assert by[4][1] == 0 and all(o == 0 for _, o, _ in want)
    # every window ties: all scorable reads in the one bin of the score 8 x 7
    assert by["ties"][0].tolist() == [by["ties"][2]] and M.score_range(Ws["ties"]) == (56, 56)
    # the planted windows are the best score on the minus strand only
    hi = M.score_range(Ws["minus"])[1]
    assert (by["minus"][0][-1] > 20) == revcom and (revcom or by["minus"][0][-1] == 0)
    assert by["minus"][0].shape == (hi - M.score_range(Ws["minus"])[0] + 1,)


# ---- 2. batching ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_set():
    from kmap_amd.motif_discovery import DeviceSeq
    rng = np.random.default_rng(1601)
    seq, borders = make_reads(rng.integers(0, 71, 1500), rng)
    ds = DeviceSeq(seq, borders)
    yield ds, seq, borders
    ds.close()


def test_batch_sizes_and_order(small_set):
    """M = 1, B, B + 1 and 2 B + 1 narrow matrices (three chunks each: the matrix count ends a batch), five of 31 columns (the chunk
    budget ends it), and both mixed; a permutation of the matrices permutes the results and changes nothing else"""
    from kmap_amd.device_seq import LIBRARY_BATCH as B, LIBRARY_BATCH_CHUNKS as CH
    ds, seq, borders = small_set
    rng = np.random.default_rng(1602)
    assert B >= 2 and 3 * B <= CH < 8 * 5
    narrow = [asym_matrix(int(w), rng) for w in rng.integers(9, 13, 2 * B + 1)]
    wide = [asym_matrix(31, rng) for _ in range(5)]
    mats = narrow + wide
    want = [model(seq, borders, W, True) for W in mats]
    for n in (1, B, B + 1, 2 * B + 1):
        los, nbs = full_ranges(mats[:n])
        check_against(ds.library_histograms(mats[:n], los, nbs, True), want[:n])
    los, nbs = full_ranges(wide)
    check_against(ds.library_histograms(wide, los, nbs, True), want[2 * B + 1:])
    los, nbs = full_ranges(mats)
    check_against(ds.library_histograms(mats, los, nbs, True), want)
    perm = rng.permutation(len(mats))
    assert (perm != np.arange(len(mats))).any()
    check_against(ds.library_histograms([mats[i] for i in perm], [los[i] for i in perm], [nbs[i] for i in perm], True),
                  [want[i] for i in perm])
    fwd = [model(seq, borders, W, False) for W in mats[B - 1:B + 2]]
    los, nbs = full_ranges(mats[B - 1:B + 2])
    check_against(ds.library_histograms(mats[B - 1:B + 2], los, nbs, False), fwd)


# ---- 3. the two histogram forms, ranges narrower than the scores ------------------------------------------------------------------------
def test_histogram_forms_and_narrow_ranges(small_set):
    from kmap_amd.device_seq import LIBRARY_LDS_BINS
    ds, seq, borders = small_set
    rng = np.random.default_rng(1603)
    small, big = asym_matrix(9, rng), asym_matrix(16, rng) * 10
    (lo_s, hi_s), (lo_b, hi_b) = M.score_range(small), M.score_range(big)
    assert hi_s - lo_s + 1 <= LIBRARY_LDS_BINS < hi_b - lo_b + 1 <= 2 ** 22       # block-private bins; global bins
    sc_s, sc_b = window_scores(seq, small), window_scores(seq, big)
    best_s, loc_s, _ = M.np_read_scores(seq, borders, small, True, sc_s)
    best_b, loc_b, _ = M.np_read_scores(seq, borders, big, True, sc_b)
    q1, q3 = (int(q) for q in np.quantile(best_s[loc_s >= 0], [0.25, 0.75]))
    med_b = int(np.median(best_b[loc_b >= 0]))
    cases = [(small, lo_s, hi_s - lo_s + 1), (big, lo_b, hi_b - lo_b + 1),     # everything inside, either form
             (small, q1, q3 - q1),                                           # reads outside on both sides, private bins
             (big, med_b, LIBRARY_LDS_BINS + 1),                             # reads outside, global bins
             (big, med_b, LIBRARY_LDS_BINS),                                 # the same matrix, the largest private range
             (small, hi_s + 1, 3), (big, lo_b - 10, 5), (small, q1, 0)]      # nothing inside; no bin at all
    want = [model(seq, borders, W, True, lo, nb, sc_s if W is small else sc_b) for W, lo, nb in cases]
    assert want[0][1] == want[1][1] == 0 and want[2][1] > 100 and want[3][1] > 100 and want[4][1] > 100
    assert want[5][1] == want[5][2] and want[7][0].shape == (0,) and want[7][1] == want[7][2]
    check_against(ds.library_histograms([c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases], True), want)


# ---- 4. more tiles than one sweep of the grid --------------------------------------------------------------------------------------------
def test_persistent_stride_against_the_per_matrix_path():
    """60 000 x 150 bp = 9.06 M positions = 8848 wave tiles, more than 2048 blocks x 4 waves: a wave takes a second tile whatever the
    grid.  Three matrices; the yardstick is read_scores + histogram of each, the existing device path."""
    from kmap_amd.motif_discovery import DeviceSeq
    rng = np.random.default_rng(1604)
    seq, borders = make_reads(np.full(60_000, 150), rng, frac_invalid=0.002)
    assert (len(seq) + 1023) // 1024 > 2048 * 4
    mats = [asym_matrix(w, rng) for w in (8, 31, 13)]
    los, nbs = full_ranges(mats)
    ds = DeviceSeq(seq, borders)
    try:
        want = []
        for W, lo, nb in zip(mats, los, nbs):
            rs = ds.read_scores(W, True)
            try:
                want.append((rs.histogram(lo, nb), 0, rs.n_scored))
            finally:
                rs.close()
        assert all(50_000 < s <= 60_000 for _, _, s in want)
        check_against(ds.library_histograms(mats, los, nbs, True), want)
    finally:
        ds.close()


# ---- 5. degenerate sizes, refused arguments ------------------------------------------------------------------------------------------------
def test_degenerate_sizes_and_errors(small_set):
    from kmap_amd import _ffi
    ds, seq, borders = small_set
    lib = _ffi.lib()
    rng = np.random.default_rng(1605)
    W = asym_matrix(10, rng)
    lo, hi = M.score_range(W)
    want = model(seq, borders, W, True)
    hists, outside, scored = ds.library_histograms([], [], [], True)
    assert hists == [] and outside.shape == (0,) and scored.shape == (0,)

    def call(widths, weights, n=ds.n, n_seq=ds.n_seq, n_bins=(8, 8), codes=ds.codes.ptr, hist=True):
        wd, lo_a, nb = np.array(widths, np.int32), np.array([lo, lo], np.int32), np.array(n_bins, np.int64)
        out = np.full(16, 7, np.uint64), np.full(2, -5, np.int64), np.full(2, -5, np.int64)
        rc = lib.kmap_readscore_library_dev(codes, ds.inval_orig.ptr, n, ds.borders.ptr, n_seq, len(widths), _ffi.ptr(wd), weights,
                                            _ffi.ptr(lo_a), _ffi.ptr(nb), 1, _ffi.ptr(out[0]) if hist else None, _ffi.ptr(out[1]),
                                            _ffi.ptr(out[2]), None)
        return rc, out
    grid = np.zeros((2, 4, 32), np.int32)
    grid[:, :, :10] = W
    # no reads, no positions: zeros
    for kw in (dict(n_seq=0), dict(n=0)):
        rc, (h, o, s) = call([10, 10], _ffi.ptr(grid), **kw)
        assert rc == 0 and not h.any() and not o.any() and not s.any()
    # width 3 and 32, a weight behind the width, a weight too large for an int32 score, null arrays, negative sizes: KMAP_E_INVAL with
    # a message that names the entry, nothing written
    for widths in ([3, 10], [10, 32]):
        rc, out = call(widths, _ffi.ptr(grid))
        assert rc == -1 and "readscore_library" in _ffi.last_error() and f"width={min(widths) if 3 in widths else 32}" in _ffi.last_error()
        assert (out[0] == 7).all() and (out[1] == -5).all() and (out[2] == -5).all()
        bad = [np.zeros((4, w), np.int32) for w in widths]
        with pytest.raises(ValueError, match="library_histograms: .*width (3|32)"):
            ds.library_histograms(bad, [0, 0], [4, 4], True)
    rc, out = call([9, 10], _ffi.ptr(grid))
    assert rc == -1 and "behind its width" in _ffi.last_error() and (out[1] == -5).all()
    huge = grid.copy()
    huge[1, 2, 3] = 2 ** 31 // 31
    rc, out = call([10, 10], _ffi.ptr(huge))
    assert rc == -1 and "int32" in _ffi.last_error() and (out[1] == -5).all()
    assert call([10, 10], None)[0] == -1 and call([10, 10], _ffi.ptr(grid), n=-1)[0] == -1 and call([10, 10], _ffi.ptr(grid), n_seq=-1)[0] == -1
    assert call([10, 10], _ffi.ptr(grid), codes=None)[0] == -1 and call([10, 10], _ffi.ptr(grid), hist=False)[0] == -1
    assert call([10, 10], _ffi.ptr(grid), n_bins=(8, -1))[0] == -1
    rc, out = call([10, 10], _ffi.ptr(grid), n_bins=(8, 2 ** 22 + 1))
    assert rc == -4 and "2^22" in _ffi.last_error() and (out[0] == 7).all()
    with pytest.raises(ValueError, match="2\\^22"):
        ds.library_histograms([W], [lo], [2 ** 22 + 1], True)
    # and the next call is as good as the first
    check_against(ds.library_histograms([W], [lo], [hi - lo + 1], True), [want])


# ---- 6. the verb end to end -------------------------------------------------------------------------------------------------------------
def test_verb_end_to_end(tmp_path, capsys):
    """preproc + shuffle_reads on the golden reads, then the three-motif MEME file and a count matrix scan_motif wrote: every row of
    library_rank.csv equals, field by field from `width` on, the row evaluate_pwm writes for the same counts given as a CSV file"""
    from kmap_amd import evaluate as E
    from kmap_amd import library as L
    from kmap_amd.kmer_count import _preproc
    from kmap_amd.shuffle import _shuffle_reads
    res, ctl = tmp_path / "res", tmp_path / "control.fa"
    _preproc(str(GOLD / "test.fa"), str(res))
    _shuffle_reads(str(res), 2, 11, 1, str(ctl))
    out = tmp_path / "out"
    capsys.readouterr()
    results = L._rank_motif_library(str(res), str(ctl), [str(LIB / "three.meme"), str(MOTIF0)], top_hist=1, output_dir=str(out))
    printed = capsys.readouterr().out
    assert [st["rank"] for st in results] == [0, 1, 2]
    assert sorted(st["motif"].name for st in results) == ["M1_CAATCGATAGC", "M2_ACCTACGTA", "cntmat_motif0_CAATCGATAGC"]
    # the same counts through evaluate_pwm, in rank order
    files = []
    for st in results:
        files.append(tmp_path / f"{st['motif'].name}.csv")
        np.savetxt(files[-1], st["motif"].counts, delimiter=",", fmt="%d")
    E._evaluate_pwm(str(res), str(ctl), [str(f) for f in files], output_dir=str(tmp_path / "eval"))
    capsys.readouterr()
    ev = (tmp_path / "eval" / "pwm_eval.csv").read_text().split("\n")
    table = (out / "library_rank.csv").read_text().split("\n")
    ev_cols, cols = ev[0].split(","), table[0].split(",")
    assert cols[:4] == ["rank", "name", "altname", "source"] and cols[4:-2] == ev_cols[1:] and cols[-2:] == ["log10_p", "q_bh"]
    assert len(table) == 5 and table[-1] == ""
    z = []
    for rank, st in enumerate(results):
        row, ev_row = table[1 + rank].split(","), ev[1 + rank].split(",")
        assert len(row) == len(cols) and row[:4] == [str(rank), st["motif"].name, st["motif"].altname, st["motif"].source]
        for name, a, b in zip(ev_cols[1:], row[4:-2], ev_row[1:]):
            assert a == b, f"rank {rank}, column {name}"
        assert float(row[-2]) == L.log10_p_of_z(st["mw_z"]) and float(row[-1]) == st["q_bh"]
        z.append(float(row[cols.index("mw_z")]))
    assert z == sorted(z, reverse=True) and z[0] > 5           # 401 of the 1002 reads carry the first motif
    np.testing.assert_array_equal([st["q_bh"] for st in results], L.bh_qvalues([10.0 ** st["log10_p"] for st in results]))
    top = results[0]["motif"].name
    assert sorted(p.name for p in out.iterdir()) == ["library_rank.csv", f"score_hist_0_{top}.csv", "skipped.csv"]
    ev_hist = [p for p in (tmp_path / "eval").iterdir() if p.name.startswith("score_hist_motif0_")]
    assert len(ev_hist) == 1 and (out / f"score_hist_0_{top}.csv").read_bytes() == ev_hist[0].read_bytes()
    assert (out / "skipped.csv").read_text().split("\n")[1].startswith("M3_long,too_wide,")
    assert printed.startswith(f"0 {top}") and "3 motifs ranked, 1 skipped" in printed
