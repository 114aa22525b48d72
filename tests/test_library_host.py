"""Host side of rank_motif_library (no GPU): the MEME and directory readers on the hand-written fixtures of tests/golden/library, the
Benjamini-Hochberg q-values against an example worked by hand, the p of the Mann-Whitney z, the ranking, the verb's files with the
device pass replaced by the numpy model of tests/_readscore_model.py, its argument errors (raised before the library is loaded), a
library file that lacks the new entry point, and the CLI verb.  The definitions are DESIGN.md section 16."""
import ctypes
import math
import pickle
import re
from pathlib import Path

import numpy as np
import pytest

from tests import _readscore_model as M
from tests._refine_model import make_reads

ROOT = Path(__file__).resolve().parent.parent
GOLD = ROOT / "tests" / "golden"
LIB = GOLD / "library"
MOTIF1 = GOLD / "report_testfa" / "cntmat_motif1_ACCTACGTA.csv"


def consensus_counts(consensus, hi, lo):
    C = np.full((4, len(consensus)), lo, np.int64)
    C[["ACGT".index(c) for c in consensus], np.arange(len(consensus))] = hi
    return C


# ---- 1. the readers -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["three.meme", "three_crlf.meme"])
def test_meme_three_motifs(name):
    """nsites= 50 (0.88 -> 44, 0.04 -> 2); no nsites: the default (0.85 x 20 = 17, 0.05 x 20 = 1); w = 40 is skipped; the version,
    ALPHABET, strands:, URL and background lines are passed over; Windows line ends read the same"""
    from kmap_amd.library import read_meme, read_motif_library
    if name == "three_crlf.meme":
        assert (LIB / name).read_bytes().count(b"\r\n") > 60
    motifs = read_motif_library(LIB / name)
    assert [(m.name, m.altname) for m in motifs] == [("M1_CAATCGATAGC", "planted_a"), ("M2_ACCTACGTA", ""), ("M3_long", "too_wide")]
    assert all(m.source == str(LIB / name) for m in motifs)
    np.testing.assert_array_equal(motifs[0].counts, consensus_counts("CAATCGATAGC", 44, 2))
    np.testing.assert_array_equal(motifs[1].counts, consensus_counts("ACCTACGTA", 17, 1))
    assert motifs[0].counts.dtype == np.int64 and motifs[0].skip is None and motifs[1].skip is None
    assert motifs[2].counts is None and "40" in motifs[2].skip and "4..31" in motifs[2].skip
    np.testing.assert_array_equal(read_meme(LIB / name, nsites_default=40)[1].counts, consensus_counts("ACCTACGTA", 34, 2))
    np.testing.assert_array_equal(read_meme(LIB / name, nsites_default=40)[0].counts, motifs[0].counts)


def test_meme_errors_name_file_and_line(tmp_path):
    from kmap_amd.library import read_meme, read_motif_library
    for name, line, word in (("bad_alength.meme", 11, "alength= 20"), ("bad_row_sum.meme", 14, "sums to 0.9000"),
                             ("bad_row.meme", 15, "four probabilities")):
        with pytest.raises(ValueError, match=re.escape(f"{name}:{line}: ") + ".*" + re.escape(word)):
            read_motif_library(LIB / name)
    head = "MEME version 4\n\n"
    cases = {"no_motif.meme": (head + "ALPHABET= ACGT\n", "no MOTIF"),
             "early.meme": (head + "letter-probability matrix: alength= 4 w= 4\n", "early.meme:3: .*first MOTIF"),
             "short.meme": (head + "MOTIF X\nletter-probability matrix: alength= 4 w= 5\n0.25 0.25 0.25 0.25\n", "short.meme:4: .*w= 5"),
             "anon.meme": (head + "MOTIF\n", "anon.meme:3: .*identifier"),
             "negative.meme": (head + "MOTIF X\nletter-probability matrix: alength= 4 w= 4\n1.5 -0.5 0 0\n", "negative.meme:5: ")}
    for name, (text, word) in cases.items():
        (tmp_path / name).write_text(text)
        with pytest.raises(ValueError, match=word):
            read_meme(tmp_path / name)
    with pytest.raises(ValueError, match="nsites_default"):
        read_meme(LIB / "three.meme", nsites_default=0)
    with pytest.raises(ValueError, match="missing"):
        read_motif_library(tmp_path / "nowhere.meme")
    (tmp_path / "empty").mkdir()
    with pytest.raises(ValueError, match="no \\*.csv or \\*.meme"):
        read_motif_library(tmp_path / "empty")


def test_meme_details(tmp_path):
    """a motif without a matrix, a narrow one, nsites below 1, a matrix without w=, a comma in a name"""
    from kmap_amd.library import read_meme
    f = tmp_path / "d.meme"
    row = "0.7 0.1 0.1 0.1\n"
    f.write_text("MEME version 5\n\nMOTIF only_a_name\n\nMOTIF narrow\nletter-probability matrix: alength= 4 w= 3 nsites= 9\n" + row * 3
                 + "MOTIF zero,sites alt\nletter-probability matrix: alength= 4 w= 4 nsites= 0\n" + row * 4
                 + "MOTIF open\nletter-probability matrix: nsites= 10\n" + row * 5 + "\nMOTIF last\nletter-probability matrix: w= 4 nsites= 10.4\n" + row * 4)
    motifs = read_meme(f)
    assert [m.name for m in motifs] == ["only_a_name", "narrow", "zero_sites", "open", "last"]
    assert "no letter-probability matrix" in motifs[0].skip and "width 3" in motifs[1].skip
    np.testing.assert_array_equal(motifs[2].counts, np.array([[14] * 4, [2] * 4, [2] * 4, [2] * 4]))
    assert motifs[3].counts.shape == (4, 5) and (motifs[3].counts[0] == 7).all()
    assert motifs[4].counts.shape == (4, 4) and (motifs[4].counts[0] == 7).all()


def test_directory_and_detection_by_content(tmp_path):
    from kmap_amd.library import read_motif_library
    from kmap_amd.pwm import read_count_matrix
    motifs = read_motif_library(LIB / "mixed")
    assert [(m.name, m.altname, Path(m.source).name) for m in motifs] == [("a_counts", "", "a_counts.csv"), ("B1", "one", "b_one.meme")]
    np.testing.assert_array_equal(motifs[0].counts, read_count_matrix(LIB / "mixed" / "a_counts.csv"))
    np.testing.assert_array_equal(motifs[1].counts, consensus_counts("TTGACA", 21, 3))
    # the content decides, not the name
    (tmp_path / "counts.meme").write_text(MOTIF1.read_text())
    (tmp_path / "meme.csv").write_text((LIB / "mixed" / "b_one.meme").read_text())
    a, b = read_motif_library(tmp_path / "counts.meme"), read_motif_library(tmp_path / "meme.csv")
    assert [m.name for m in a] == ["counts"] and [m.name for m in b] == ["B1"]
    np.testing.assert_array_equal(a[0].counts, read_count_matrix(MOTIF1))
    (tmp_path / "junk.csv").write_text("hello\n")
    with pytest.raises(ValueError, match="junk.csv"):
        read_motif_library(tmp_path / "junk.csv")


# ---- 2. q-values, p, ranking ------------------------------------------------------------------------------------------------------
def test_bh_qvalues_worked_example():
    """n = 10; the nan counts as 1.  Ascending (stable): 0.001 0.01 0.02 0.04 0.04 0.04 0.3 0.5 0.9 1 at ranks j = 1 .. 10;
    p n / j = 0.01 0.05 1/15 0.1 0.08 1/15 3/7 0.625 1 1; the running minimum from the largest p: 0.01 0.05 1/15 1/15 1/15 1/15 3/7
    0.625 1 1 -- the three tied p get the q of the last of them, and the 0.02 in front of them happens to share it."""
    from kmap_amd.library import bh_qvalues
    p = [0.04, 0.001, math.nan, 0.04, 0.5, 0.01, 0.02, 0.3, 0.04, 0.9]
    want = [1 / 15, 0.01, 1.0, 1 / 15, 0.625, 0.05, 1 / 15, 3 / 7, 1 / 15, 1.0]
    q = bh_qvalues(p)
    assert q.dtype == np.float64 and q.shape == (10,)
    np.testing.assert_allclose(q, want, rtol=1e-14, atol=0)
    assert q[0] == q[3] == q[8]
    np.testing.assert_array_equal(bh_qvalues([]), np.zeros(0))
    np.testing.assert_array_equal(bh_qvalues([0.3]), [0.3])
    np.testing.assert_array_equal(bh_qvalues([math.nan, math.nan]), [1.0, 1.0])
    np.testing.assert_array_equal(bh_qvalues([0.9, 0.8, 0.0]), [0.9, 0.9, 0.0])      # 0.9 x 3 / 3; min(0.8 x 3 / 2, 0.9); 0


def test_p_of_z_and_rank_order():
    from kmap_amd.library import log10_p_of_z, rank_order
    assert log10_p_of_z(math.nan) == 0.0
    assert log10_p_of_z(0.0) == pytest.approx(math.log10(0.5), rel=1e-14)
    for z in (-2.0, 1.0, 3.0, 8.0):
        assert log10_p_of_z(z) == pytest.approx(math.log10(0.5 * math.erfc(z / math.sqrt(2.0))), rel=1e-12)
    assert log10_p_of_z(60.0) < -700                          # far past the smallest double: the logarithm is still finite
    names = ["d", "b", "c", "a", "e", "f"]
    z = [1.5, math.nan, 7.0, 1.5, math.nan, -3.0]
    assert [names[i] for i in rank_order(names, z)] == ["c", "a", "d", "f", "b", "e"]


# ---- 3. the verb on the numpy model -----------------------------------------------------------------------------------------------
class ModelSeq:
    """DeviceSeq's part in the verb, on the host: library_histograms is the model's best score per read, reduced to histograms"""
    calls = []

    def __init__(self, seq, borders):
        self.seq, self.borders = np.asarray(seq, np.uint8), np.asarray(borders, np.int64).reshape(-1, 2)
        self.n_seq = len(self.borders)

    def library_histograms(self, Ws, los, n_bins, revcom):
        ModelSeq.calls.append((len(Ws), bool(revcom)))
        hists, outside, scored = [], [], []
        for W, lo, nb in zip(Ws, los, n_bins):
            score, loc, _ = M.np_read_scores(self.seq, self.borders, W, revcom)
            h, o = M.np_histogram(score, loc, lo, nb)
            hists.append(h)
            outside.append(o)
            scored.append(int((loc >= 0).sum()))
        return hists, np.array(outside, np.int64), np.array(scored, np.int64)

    def close(self):
        pass


@pytest.fixture
def planted(tmp_path, monkeypatch):
    """a preproc result directory of 240 reads (every third one carries CAATCGATAGC, every fifth the reverse complement of
    ACCTACGTA) and a control FASTA of random reads; the device replaced by ModelSeq"""
    import kmap_amd.kmer_count as K
    import kmap_amd.motif_discovery as D
    rng = np.random.default_rng(160)
    seq, borders = make_reads(rng.integers(0, 60, 240), rng, frac_invalid=0.01)
    code = {c: i for i, c in enumerate("ACGT")}
    for k, (s, e) in enumerate(borders):
        if k % 3 == 0 and e - s >= 11:
            at = int(rng.integers(s, e - 10))
            seq[at:at + 11] = [code[c] for c in "CAATCGATAGC"]
        elif k % 5 == 0 and e - s >= 9:
            at = int(rng.integers(s, e - 8))
            seq[at:at + 9] = [code[c] for c in "TACGTAGGT"]
    res = tmp_path / "res"
    res.mkdir()
    (res / K.FileNameDict["config_file"]).write_text((ROOT / "kmap_amd" / "default_config.toml").read_text())
    with open(res / K.FileNameDict["processed_fasta_file"], "wb") as fh:
        pickle.dump(seq, fh)
    with open(res / K.FileNameDict["processed_fasta_seqboarder_file"], "wb") as fh:
        pickle.dump(borders, fh)
    ctl = tmp_path / "control.fa"
    with open(ctl, "w") as fh:
        for i in range(200):
            fh.write(f">c{i}\n" + "".join("ACGT"[b] for b in rng.integers(0, 4, int(rng.integers(0, 60)))) + "\n")
    monkeypatch.setattr(D, "DeviceSeq", ModelSeq)
    monkeypatch.setattr(K, "encode_fasta", lambda path: M.encode_fasta_np(path))
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    ModelSeq.calls = []
    return res, ctl, seq, borders


def test_verb_ordering_and_files(planted, tmp_path, capsys):
    from kmap_amd import evaluate as E
    from kmap_amd import library as L
    from kmap_amd.pwm import pwm_consensus, pwm_threshold, pwm_weights
    res, ctl, seq, borders = planted
    ctl_seq, ctl_borders = M.encode_fasta_np(ctl)
    out = tmp_path / "out"
    files = [str(LIB / "three.meme"), str(LIB / "mixed"), str(MOTIF1)]
    results = L._rank_motif_library(str(res), str(ctl), files, top_hist=2, output_dir=str(out))
    printed = capsys.readouterr().out
    assert ModelSeq.calls == [(5, True), (5, True)]            # reads and control: one call each for the whole library
    # the rows, computed here motif by motif
    motifs = [m for f in files for m in L.read_motif_library(f)]
    assert [m.name for m in motifs] == ["M1_CAATCGATAGC", "M2_ACCTACGTA", "M3_long", "a_counts", "B1", "cntmat_motif1_ACCTACGTA"]
    rows = []
    for m in motifs:
        if m.skip:
            continue
        W = pwm_weights(m.counts, 1.0)
        t, lo, hi = pwm_threshold(W, 1e-4)
        fg, bg = M.np_read_scores(seq, borders, W, True), M.np_read_scores(ctl_seq, ctl_borders, W, True)
        Hf, Hc = M.np_histogram(fg[0], fg[1], lo, hi - lo + 1)[0], M.np_histogram(bg[0], bg[1], lo, hi - lo + 1)[0]
        st = E.evaluate_histograms(Hf, Hc, lo, t, 10)
        tail = E.eval_line(0, m.counts.shape[1], pwm_consensus(m.counts), 1.0, True, int((fg[1] < 0).sum()), int((bg[1] < 0).sum()), st)
        rows.append(dict(m=m, z=st["mw_z"], tail=tail.rstrip("\n").split(",", 1)[1], Hf=Hf, Hc=Hc, lo=lo))
    assert all(r["z"] == r["z"] for r in rows)
    q = L.bh_qvalues([10.0 ** L.log10_p_of_z(r["z"]) for r in rows])
    for r, qi in zip(rows, q.tolist()):
        r["q"] = qi
    rows.sort(key=lambda r: (-r["z"], r["m"].name))
    # sanity of the read set, not a measurement: a third of the reads carry M1's motif, so it leads, far from chance
    assert rows[0]["m"].name == "M1_CAATCGATAGC" and rows[0]["z"] > 3 and rows[0]["q"] < 0.01
    table = (out / "library_rank.csv").read_text().split("\n")
    assert table[0] + "\n" == L.RANK_HEADER and table[-1] == "" and len(table) == 2 + len(rows)
    assert table[0] == ("rank,name,altname,source,width,consensus,pseudocount,revcom,n_fg,n_control,fg_unscorable,control_unscorable,auroc,"
                        "mw_z,threshold_p,threshold_p_bits,fg_reads_p,control_reads_p,log2_fold_p,z_p,threshold_best,threshold_best_bits,"
                        "fg_reads_best,control_reads_best,z_best,log10_p,q_bh")
    cols = table[0].split(",")
    for rank, (line, r) in enumerate(zip(table[1:], rows)):
        m = r["m"]
        assert line == f"{rank},{m.name},{m.altname},{m.source},{r['tail']},{L.log10_p_of_z(r['z'])!r},{r['q']!r}"
        assert len(line.split(",")) == len(cols)
        assert results[rank]["motif"].name == m.name and results[rank]["rank"] == rank and results[rank]["q_bh"] == r["q"]
        np.testing.assert_array_equal(results[rank]["Hf"], r["Hf"])
    z = [float(line.split(",")[cols.index("mw_z")]) for line in table[1:-1]]
    assert z == sorted(z, reverse=True)
    assert (out / "skipped.csv").read_text() == f"name,altname,source,reason\nM3_long,too_wide,{LIB / 'three.meme'},width 40 outside 4..31\n"
    names = [f"score_hist_{k}_{rows[k]['m'].name}.csv" for k in range(2)]
    assert sorted(p.name for p in out.iterdir()) == sorted(names + ["library_rank.csv", "skipped.csv"])
    for k in range(2):
        E.write_score_hist(tmp_path / "want.csv", rows[k]["Hf"], rows[k]["Hc"], rows[k]["lo"])
        assert (out / names[k]).read_bytes() == (tmp_path / "want.csv").read_bytes()
    assert printed.count("\n") == len(rows) + 1 and printed.startswith("0 M1_CAATCGATAGC planted_a: auroc")
    assert f"rank_motif_library: 5 motifs ranked, 1 skipped, both strands: {out}" in printed
    # a second run writes the same bytes; the default directory, the forward strand, no histograms
    L._rank_motif_library(str(res), str(ctl), files, top_hist=2, output_dir=str(tmp_path / "out2"))
    for p in out.iterdir():
        assert (tmp_path / "out2" / p.name).read_bytes() == p.read_bytes()
    fwd = L._rank_motif_library(str(res), str(ctl), [str(LIB / "three.meme")], revcom_mode=False)
    assert sorted(p.name for p in (res / "pwm_library").iterdir()) == ["library_rank.csv", "skipped.csv"]
    assert ModelSeq.calls[-1] == (2, False) and len(fwd) == 2
    assert (res / "pwm_library" / "library_rank.csv").read_text().split("\n")[1].split(",")[cols.index("revcom")] == "0"


def test_nan_z_ranks_last_with_p_one(planted, tmp_path, monkeypatch):
    """no control read is long enough for the matrices: nf > 0, nc = 0, every z is nan -- ranked by name, p = 1, q = 1"""
    from kmap_amd import library as L
    res, ctl, _, _ = planted
    ctl.write_text(">a\nACG\n>b\nTT\n")
    results = L._rank_motif_library(str(res), str(ctl), [str(LIB / "three.meme")], output_dir=str(tmp_path / "o"))
    assert [st["motif"].name for st in results] == ["M1_CAATCGATAGC", "M2_ACCTACGTA"]
    lines = (tmp_path / "o" / "library_rank.csv").read_text().split("\n")[1:3]
    assert all(line.endswith(",nan,0.0,1.0") or line.endswith(",0.0,1.0") for line in lines)
    assert all(st["log10_p"] == 0.0 and st["q_bh"] == 1.0 and st["control_unscorable"] == 2 for st in results)


def test_value_errors_come_before_the_library(planted, tmp_path, monkeypatch):
    import kmap_amd.motif_discovery as D
    from kmap_amd import _ffi, evaluate
    from kmap_amd import library as L

    def no_lib():
        raise AssertionError("the library was loaded before the arguments were checked")

    class NoSeq:
        def __init__(self, *a):
            no_lib()
    monkeypatch.setattr(_ffi, "lib", no_lib)
    monkeypatch.setattr(D, "DeviceSeq", NoSeq)
    res, ctl, _, _ = planted
    out = tmp_path / "out"
    only_wide = tmp_path / "wide.meme"
    only_wide.write_text("MEME version 4\n\nMOTIF W\nletter-probability matrix: alength= 4 w= 32\n" + "0.25 0.25 0.25 0.25\n" * 32)
    zero = tmp_path / "zero.csv"
    zero.write_text("1,2,3,0\n1,2,3,4\n1,2,3,4\n1,2,3,4\n")
    ok = dict(library_files=[str(LIB / "three.meme")], output_dir=out)
    bad = [(dict(), tmp_path / "nowhere", ctl, "config.toml"),
           (dict(), res, tmp_path / "missing.fa", "control"),
           (dict(library_files=[]), res, ctl, "no library file"),
           (dict(library_files=[str(tmp_path / "nowhere.meme")]), res, ctl, "nowhere.meme"),
           (dict(library_files=[str(LIB / "three.meme"), str(LIB / "bad_alength.meme")]), res, ctl, "bad_alength.meme:11"),
           (dict(library_files=[str(only_wide)]), res, ctl, "none of the 1 motifs.*W: width 32"),
           (dict(library_files=[str(zero)], pseudocount=0.0), res, ctl, "zero.csv: motif zero: .*pseudocount"),
           (dict(pseudocount=-1.0), res, ctl, "pseudocount"),
           (dict(p_value=float("nan")), res, ctl, "p_value"),
           (dict(nsites_default=0), res, ctl, "nsites_default"),
           (dict(min_reads=0), res, ctl, "min_reads"),
           (dict(top_hist=-1), res, ctl, "top_hist")]
    for change, r, c, word in bad:
        with pytest.raises(ValueError, match=word):
            L._rank_motif_library(r, c, **{**ok, **change})
    assert not out.exists()
    with pytest.raises(AssertionError, match="the library was loaded"):
        L._rank_motif_library(res, ctl, **ok)
    assert not out.exists()
    # more than 2^22 different scores: the motif is skipped, not fatal -- and fatal when nothing else is left
    wide = np.zeros((4, 9), np.int32)
    wide[0], wide[1] = 240_000, -240_000
    assert 9 * 480_000 + 1 > evaluate.MAX_BINS
    monkeypatch.setattr(L, "pwm_weights", lambda C, a: wide)
    with pytest.raises(ValueError, match="none of the 3 motifs.*2\\^22"):
        L._rank_motif_library(res, ctl, **ok)
    assert not out.exists()


def test_too_many_scores_is_skipped(planted, tmp_path, monkeypatch):
    from kmap_amd import library as L
    from kmap_amd.pwm import pwm_weights
    res, ctl, _, _ = planted
    wide = np.zeros((4, 9), np.int32)
    wide[0], wide[1] = 240_000, -240_000
    monkeypatch.setattr(L, "pwm_weights", lambda C, a: wide if C.shape[1] == 9 else pwm_weights(C, a))
    results = L._rank_motif_library(res, ctl, [str(LIB / "three.meme")], output_dir=tmp_path / "o")
    assert [st["motif"].name for st in results] == ["M1_CAATCGATAGC"]
    skipped = (tmp_path / "o" / "skipped.csv").read_text().split("\n")
    assert skipped[1].startswith("M2_ACCTACGTA,,") and "more than 2^22 different scores" in skipped[1] and skipped[2].startswith("M3_long,")


def test_other_ranks_do_nothing(monkeypatch):
    from kmap_amd.library import _rank_motif_library
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "1")
    assert _rank_motif_library("nowhere", "missing.fa", []) is None


# ---- 4. the library's entry -------------------------------------------------------------------------------------------------------
def test_symbol_registered_and_batch_constants():
    from kmap_amd import _ffi, device_seq
    header = (ROOT / "include" / "kmap_hip.h").read_text()
    name = "kmap_readscore_library_dev"
    assert name in _ffi.exported_symbols() and f"int {name}(" in header
    res, args = _ffi._SIGS[name]
    assert res is _ffi.i32 and len(args) == 15
    src = (ROOT / "kmap_amd" / "csrc" / "pwm_library.hip").read_text()
    batch = (ROOT / "kmap_amd" / "csrc" / "pwm_batch.h").read_text()
    assert int(re.search(r"constexpr int PB_MAX_MAT = (\d+);", batch).group(1)) == device_seq.LIBRARY_BATCH
    assert int(re.search(r"constexpr int PB_MAX_CHUNKS = (\d+);", batch).group(1)) == device_seq.LIBRARY_BATCH_CHUNKS
    assert int(re.search(r"constexpr int64_t LB_HIST_LDS_BINS = (\d+);", src).group(1)) == device_seq.LIBRARY_LDS_BINS
    assert device_seq.LIBRARY_BATCH_CHUNKS >= 8               # the widest matrix has 8 chunks of 4 columns: a batch is never empty


def test_library_histograms_checks_come_before_the_library(monkeypatch):
    from kmap_amd import _ffi
    from kmap_amd.device_seq import DeviceSeq

    def no_lib():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_ffi, "lib", no_lib)
    ds = object.__new__(DeviceSeq)
    ok = np.zeros((4, 8), np.int32)
    for Ws, los, nbs, word in (([np.zeros((4, 3), np.int32)], [0], [1], "width 3"), ([ok, np.zeros((4, 32), np.int32)], [0, 0], [1, 1], "matrix 1 has width 32"),
                               ([np.zeros((3, 8), np.int32)], [0], [1], "shape"), ([ok], [0], [2 ** 22 + 1], "2\\^22"), ([ok], [0], [-1], "bins"),
                               ([ok], [2 ** 31], [4], "int32"), ([ok], [0, 1], [4], "1 matrices, 2 range starts")):
        with pytest.raises(ValueError, match="library_histograms: .*" + word):
            ds.library_histograms(Ws, los, nbs, True)


def test_a_library_file_without_the_entry_point(planted, monkeypatch):
    """a libkmap_hip.so built before this verb existed: loading it names the missing symbol and how to rebuild, as KmapError -- the
    error of a missing library file -- and that is what the verb raises"""
    import kmap_amd.motif_discovery as D
    from kmap_amd import _ffi, device_seq
    from kmap_amd import library as L

    class Stale:
        def __getattr__(self, name):
            if name == "kmap_readscore_library_dev":
                raise AttributeError(name)
            return lambda *a: 0
    monkeypatch.setattr(_ffi, "_lib", None)
    monkeypatch.setattr(_ffi, "LIB_PATH", ROOT / "README.md")    # any file that exists: CDLL below does not open it
    monkeypatch.setattr(ctypes, "CDLL", lambda *a, **k: Stale())
    with pytest.raises(_ffi.KmapError, match="out of date.*kmap_readscore_library_dev.*build"):
        _ffi.lib()
    assert _ffi._lib is None
    monkeypatch.setattr(D, "DeviceSeq", device_seq.DeviceSeq)    # the real one
    res, ctl, _, _ = planted
    with pytest.raises(_ffi.KmapError, match="kmap_readscore_library_dev"):
        L._rank_motif_library(res, ctl, [str(LIB / "three.meme")])
    assert not (res / "pwm_library").exists()


# ---- 5. the verb's command line -----------------------------------------------------------------------------------------------------
def test_cli_options_and_defaults(monkeypatch):
    from click.testing import CliRunner
    from kmap_amd import library
    from kmap_amd.cli import cli
    calls = []
    monkeypatch.setattr(library, "_rank_motif_library", lambda *a: calls.append(a))
    runner = CliRunner()
    r = runner.invoke(cli, ["rank_motif_library", "--res_dir", "D", "--control_fasta_file", "C.fa", "--library_file", "L"])
    assert r.exit_code == 0, r.output
    assert calls[-1] == ("D", "C.fa", ["L"], 1e-4, 1.0, 20, None, 10, 0, None)
    r = runner.invoke(cli, ["rank_motif_library", "--res_dir", "D", "--control_fasta_file", "C.fa", "--library_file", "L", "--library_file", "L2",
                            "--p_value", "1e-3", "--pseudocount", "0.5", "--nsites_default", "100", "--revcom_mode", "False", "--min_reads", "3",
                            "--top_hist", "5", "--output_dir", "O"])
    assert r.exit_code == 0, r.output
    assert calls[-1] == ("D", "C.fa", ["L", "L2"], 1e-3, 0.5, 100, False, 3, 5, "O")
    for missing in (["--control_fasta_file", "C.fa", "--library_file", "L"], ["--res_dir", "D", "--library_file", "L"],
                    ["--res_dir", "D", "--control_fasta_file", "C.fa"]):
        assert runner.invoke(cli, ["rank_motif_library"] + missing).exit_code == 2
    assert len(calls) == 2
    r = runner.invoke(cli, ["rank_motif_library", "--help"])
    for opt in ("--res_dir", "--control_fasta_file", "--library_file", "--p_value", "--pseudocount", "--nsites_default", "--revcom_mode",
                "--min_reads", "--top_hist", "--output_dir"):
        assert opt in r.output, opt
    assert "rank_motif_library" in runner.invoke(cli, ["--help"]).output
    import kmap_amd.cli as cli_module
    assert "rank_motif_library" in cli_module.__doc__
    assert "rank_motif_library" in (ROOT / "README.md").read_text()
