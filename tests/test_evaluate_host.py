"""Host side of evaluate_pwm (no GPU): the rank statistic against a brute-force average-rank computation in exact rationals, the
threshold sweep against a direct loop over every threshold, the three writers byte for byte, every argument error (raised before the
library is loaded) and the CLI verb.  The definitions are DESIGN.md section 14."""
import math
from decimal import Decimal, getcontext
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
GOLD = ROOT / "tests" / "golden"
MOTIF1 = GOLD / "report_testfa" / "cntmat_motif1_ACCTACGTA.csv"


# ---- 1. rank_stats ----------------------------------------------------------------------------------------------------------------
def brute_rank_stats(Hf, Hc):
    """(U2, auroc, mw_z) from the pooled sample itself: average ranks as Fractions, U = R_f - nf (nf + 1) / 2, the tie-corrected
    variance as a Fraction, one square root (60 decimal digits) at the end"""
    sample = sorted([(s, 0) for s, c in enumerate(Hf) for _ in range(int(c))] + [(s, 1) for s, c in enumerate(Hc) for _ in range(int(c))])
    nf, nc = int(sum(Hf)), int(sum(Hc))
    N = nf + nc
    rank_f, i, ties = Fraction(0), 0, 0
    while i < N:
        j = i
        while j < N and sample[j][0] == sample[i][0]:
            j += 1
        mid = Fraction(i + 1 + j, 2)                         # the average of the ranks i + 1 .. j
        rank_f += mid * sum(1 for k in range(i, j) if sample[k][1] == 0)
        ties += (j - i) ** 3 - (j - i)
        i = j
    U = rank_f - Fraction(nf * (nf + 1), 2)
    U2 = 2 * U
    assert U2.denominator == 1
    if nf == 0 or nc == 0:
        return int(U2), math.nan, math.nan
    var = Fraction(nf * nc, 12) * ((N + 1) - Fraction(ties, N * (N - 1)))
    if var == 0:
        return int(U2), math.nan, math.nan
    getcontext().prec = 60
    z = (Decimal(U.numerator) / Decimal(U.denominator) - Decimal(nf * nc) / 2) / (Decimal(var.numerator) / Decimal(var.denominator)).sqrt()
    return int(U2), float(Fraction(int(U2), 2 * nf * nc)), float(z)


def rank_cases():
    rng = np.random.default_rng(14)
    cases = []
    for _ in range(40):
        bins = int(rng.integers(1, 30))
        cases.append((rng.integers(0, 6, bins), rng.integers(0, 6, bins)))
    for _ in range(10):                                      # heavy ties: two or three scores hold everything
        bins = int(rng.integers(2, 4))
        cases.append((rng.integers(20, 60, bins), rng.integers(20, 60, bins)))
    cases += [(np.array([0, 0, 17, 0]), np.array([0, 0, 9, 0])),                    # all scores equal
              (np.array([0, 0, 0, 4, 3]), np.array([5, 2, 1, 0, 0])),               # disjoint, the foreground above
              (np.array([5, 2, 1, 0, 0]), np.array([0, 0, 0, 4, 3])),               # disjoint, the foreground below
              (np.array([0, 0, 0]), np.array([3, 1, 2])), (np.array([3, 1, 2]), np.array([0, 0, 0])),
              (np.array([0]), np.array([0])), (np.array([1, 0]), np.array([0, 1])), (np.array([1]), np.array([1]))]
    return cases


def test_rank_stats_against_average_ranks():
    from kmap_amd.evaluate import rank_stats
    seen_nan = seen_z = 0
    for Hf, Hc in rank_cases():
        got, want = rank_stats(Hf.astype(np.uint64), Hc.astype(np.uint64)), brute_rank_stats(Hf.tolist(), Hc.tolist())
        assert isinstance(got[0], int) and got[0] == want[0], (Hf, Hc)
        if math.isnan(want[1]):
            assert math.isnan(got[1]) and math.isnan(got[2]) and math.isnan(want[2]), (Hf, Hc)
            seen_nan += 1
        else:
            assert got[1] == want[1], (Hf, Hc, got, want)
            assert math.isclose(got[2], want[2], rel_tol=1e-12), (Hf, Hc, got, want)
            seen_z += 1
    assert seen_nan >= 5 and seen_z >= 50
    assert rank_stats(np.array([0, 0, 0, 4, 3]), np.array([5, 2, 1, 0, 0]))[1] == 1.0
    assert rank_stats(np.array([5, 2, 1, 0, 0]), np.array([0, 0, 0, 4, 3]))[1] == 0.0
    assert rank_stats(np.array([2, 2]), np.array([2, 2]))[1:] == (0.5, 0.0)
    assert rank_stats(np.array([0, 0, 0, 4, 3]), np.array([5, 2, 1, 0, 0]))[2] > 0 > rank_stats(np.array([5, 2, 1, 0, 0]), np.array([0, 0, 0, 4, 3]))[2]
    U2, auroc, z = rank_stats(np.array([10 ** 7, 3 * 10 ** 6], np.uint64), np.array([9 * 10 ** 6, 10 ** 6], np.uint64))   # the C3 size: exact in Python ints
    assert U2 == 10 ** 7 * 9 * 10 ** 6 + 3 * 10 ** 6 * (2 * 9 * 10 ** 6 + 10 ** 6) and auroc == U2 / (2 * 13 * 10 ** 6 * 10 ** 7) and z > 0
    for bad in ((np.zeros(3), np.zeros(3, np.int64)), (np.zeros(3, np.int64), np.zeros(4, np.int64)), (np.array([-1, 2]), np.array([1, 2]))):
        with pytest.raises(ValueError):
            rank_stats(*bad)


# ---- 2. threshold_sweep -----------------------------------------------------------------------------------------------------------
def direct_sweep(Hf, Hc, lo, min_reads):
    from kmap_amd.enrichment import enrich_z
    nf, nc = int(sum(Hf)), int(sum(Hc))
    best = None
    for i in range(len(Hf)):                                 # every integer t of [lo, hi]
        a, b = int(sum(Hf[i:])), int(sum(Hc[i:]))
        if a + b < min_reads:
            continue
        z = enrich_z(a, b, nf, nc)
        if best is None or (z, lo + i) > (best[3], best[0]):
            best = (lo + i, a, b, z)
    return best


def test_threshold_sweep_against_a_direct_loop():
    from kmap_amd.evaluate import evaluate_histograms, reads_at, threshold_sweep
    rng = np.random.default_rng(15)
    n_best_inside = 0
    for _ in range(60):
        bins = int(rng.integers(1, 60))
        Hf, Hc = rng.integers(0, 8, bins) * (rng.random(bins) < 0.4), rng.integers(0, 8, bins) * (rng.random(bins) < 0.4)
        lo, min_reads = int(rng.integers(-500, 500)), int(rng.integers(1, 12))
        got = threshold_sweep(Hf, Hc, lo, min_reads)
        assert got == direct_sweep(Hf.tolist(), Hc.tolist(), lo, min_reads), (Hf, Hc, lo, min_reads)
        n_best_inside += got is not None and lo < got[0] < lo + bins - 1
    assert n_best_inside > 20
    # equal z on a stretch of thresholds (no read between them) and between two read sets that do not differ: the largest t
    Hf = np.array([3, 0, 0, 3, 0, 0, 2, 0])
    assert threshold_sweep(Hf, Hf, -3, 1) == (3, 2, 2, 0.0) == direct_sweep(Hf.tolist(), Hf.tolist(), -3, 1)
    assert threshold_sweep(Hf, Hf, -3, 5) == (0, 5, 5, 0.0) == direct_sweep(Hf.tolist(), Hf.tolist(), -3, 5)
    # min_reads above every a + b: no candidate
    assert threshold_sweep(Hf, Hf, -3, 17) is None and direct_sweep(Hf.tolist(), Hf.tolist(), -3, 17) is None
    assert threshold_sweep(np.zeros(4, np.int64), np.zeros(4, np.int64), 0, 1) is None
    for bad in (0, -1, 1.5):
        with pytest.raises(ValueError, match="min_reads"):
            threshold_sweep(Hf, Hf, 0, bad)
    # a threshold above hi, below lo, inside
    Hc = np.array([4, 0, 1, 0, 0, 0, 0, 0])
    assert reads_at(Hf, Hc, 10, 18) == (0, 0) and reads_at(Hf, Hc, 10, 10 ** 6) == (0, 0)
    assert reads_at(Hf, Hc, 10, -50) == (8, 5) and reads_at(Hf, Hc, 10, 12) == (5, 1) and reads_at(Hf, Hc, 10, 13) == (5, 0)
    st = evaluate_histograms(Hf, Hc, 10, 18, 17)
    assert (st["fg_reads_p"], st["control_reads_p"], st["z_p"], st["best"]) == (0, 0, 0.0, None)
    assert (st["n_fg"], st["n_control"], st["threshold_p"]) == (8, 5, 18) and st["log2_fold_p"] == math.log2(1 / 9) - math.log2(1 / 6)


# ---- 3. the writers ---------------------------------------------------------------------------------------------------------------
def test_writers_byte_for_byte(tmp_path):
    from kmap_amd.enrichment import enrich_z, log2_fold
    from kmap_amd.evaluate import (eval_line, evaluate_histograms, rank_stats, write_eval_table, write_read_scores,
                                   write_score_hist)
    Hf, Hc = np.array([1, 0, 2, 0, 5], np.uint64), np.array([4, 0, 3, 0, 1], np.uint64)
    st = evaluate_histograms(Hf, Hc, 1058, 1062, 2)
    U2, auroc, mw_z = rank_stats(Hf, Hc)
    assert (U2, auroc) == (1 * 4 + 2 * 11 + 5 * 15, 101 / 128) and st["best"] == (1062, 5, 1, enrich_z(5, 1, 8, 8))
    lines = [eval_line(0, 9, "ACCTACGTA", 1.0, True, 2, 0, st),
             eval_line(1, 4, "ACGT", 0.5, False, 0, 3, evaluate_histograms(Hf, Hc, 1058, 1070, 100)),
             eval_line(2, 4, "AAAA", 1, False, 1, 1, evaluate_histograms(Hf[:0], Hc[:0], 0, 0, 10))]
    write_eval_table(tmp_path / "e.csv", lines)
    want = ("motif,width,consensus,pseudocount,revcom,n_fg,n_control,fg_unscorable,control_unscorable,auroc,mw_z,"
            "threshold_p,threshold_p_bits,fg_reads_p,control_reads_p,log2_fold_p,z_p,"
            "threshold_best,threshold_best_bits,fg_reads_best,control_reads_best,z_best\n"
            "0,9,ACCTACGTA,1.0,1,8,8,2,0,0.7890625,2.059798192794945,1062,10.62,5,1,1.5849625007211563,2.065591117977289,"
            "1062,10.62,5,1,2.065591117977289\n"
            "1,4,ACGT,0.5,0,8,8,0,3,0.7890625,2.059798192794945,1070,10.70,0,0,0.0,0.0,,,,,nan\n"
            "2,4,AAAA,1.0,0,0,0,1,1,nan,nan,0,0.00,0,0,0.0,0.0,,,,,nan\n")
    assert (tmp_path / "e.csv").read_text() == want
    # repr: the shortest text that reads back the same double
    assert (repr(mw_z), repr(log2_fold(5, 1, 8, 8)), repr(enrich_z(5, 1, 8, 8))) == ("2.059798192794945", "1.5849625007211563", "2.065591117977289")
    write_score_hist(tmp_path / "h.csv", Hf, Hc, 1058)
    assert (tmp_path / "h.csv").read_text() == "score,fg_reads,control_reads\n1058,1,4\n1060,2,3\n1062,5,1\n"
    write_score_hist(tmp_path / "h0.csv", Hf[:0], Hc[:0], -7)
    assert (tmp_path / "h0.csv").read_text() == "score,fg_reads,control_reads\n"
    score = np.array([1062, -2 ** 31, -5, 0, 1255], np.int32)
    loc, strand = np.array([7, -1, 0, 31, 100000], np.int32), np.array([0, 0, 1, 1, 0], np.uint8)
    write_read_scores(tmp_path / "r.tsv", score, loc, strand)
    assert (tmp_path / "r.tsv").read_text() == ("seq_ind\tscore\tloc\tstrand\n0\t10.62\t7\t+\n1\tNA\tNA\tNA\n2\t-0.05\t0\t-\n3\t0.00\t31\t-\n"
                                                "4\t12.55\t100000\t+\n")


# ---- 4. errors come before the library ------------------------------------------------------------------------------------------
@pytest.fixture
def res_dir(tmp_path):
    """a tiny hand-made preproc result directory (one read, ACGT) and a control file"""
    import pickle
    from kmap_amd.kmer_count import FileNameDict
    res = tmp_path / "res"
    res.mkdir()
    (res / FileNameDict["config_file"]).write_text((ROOT / "kmap_amd" / "default_config.toml").read_text())
    with open(res / FileNameDict["processed_fasta_file"], "wb") as fh:
        pickle.dump(np.array([0, 1, 2, 3, 255], np.uint8), fh)
    with open(res / FileNameDict["processed_fasta_seqboarder_file"], "wb") as fh:
        pickle.dump(np.array([[0, 4]], np.int64), fh)
    ctl = tmp_path / "control.fa"
    ctl.write_text(">c\nACGT\n")
    return res, ctl


def test_value_errors_come_before_the_library(res_dir, tmp_path, monkeypatch):
    from kmap_amd import _ffi, pwm
    from kmap_amd.evaluate import _evaluate_pwm
    from kmap_amd.kmer_count import FileNameDict

    def no_lib():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_ffi, "lib", no_lib)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    res, ctl = res_dir
    out = tmp_path / "out"
    bad_matrix, short_matrix = tmp_path / "bad.csv", tmp_path / "short.csv"
    bad_matrix.write_text("1,2,3,4\n1,2,x,4\n1,2,3,4\n1,2,3,4\n")
    short_matrix.write_text("1,2,3\n1,2,3\n1,2,3\n1,2,3\n")
    zero_matrix = tmp_path / "zero.csv"
    zero_matrix.write_text("1,2,3,0\n1,2,3,4\n1,2,3,4\n1,2,3,4\n")
    ok = dict(matrix_files=[str(MOTIF1)], p_value=1e-4, min_score=None, pseudocount=1.0, revcom_mode=None, min_reads=10,
              read_scores=True, output_dir=out)
    bad = [(dict(), tmp_path / "nowhere", ctl, "config.toml"),
           (dict(), res, tmp_path / "missing.fa", "control"),
           (dict(), res, None, "control"),
           (dict(matrix_files=[]), res, ctl, "no matrix"),
           (dict(matrix_files=[str(MOTIF1), str(bad_matrix)]), res, ctl, "bad.csv"),
           (dict(matrix_files=[str(short_matrix)]), res, ctl, "width"),
           (dict(matrix_files=[str(zero_matrix)], pseudocount=0.0), res, ctl, "pseudocount"),
           (dict(pseudocount=-1.0), res, ctl, "pseudocount"),
           (dict(p_value=-0.5), res, ctl, "p_value"),
           (dict(p_value=float("nan")), res, ctl, "p_value"),
           (dict(min_score=float("inf")), res, ctl, "min_score"),
           (dict(min_reads=0), res, ctl, "min_reads"),
           (dict(min_reads=2.5), res, ctl, "min_reads")]
    for change, r, c, word in bad:
        with pytest.raises(ValueError, match=word):
            _evaluate_pwm(r, c, **{**ok, **change})
    # more than 2^22 different scores: no matrix file gets there (a weight is at least 100 log2 of the smallest double), so the weights
    # are put in the verb's way
    wide = np.zeros((4, 9), np.int32)
    wide[0], wide[1] = 240_000, -240_000
    with monkeypatch.context() as m:
        m.setattr(pwm, "pwm_weights", lambda C, a: wide)       # load_matrices, the matrix loop the verb shares with scan_pwm
        with pytest.raises(ValueError, match="2\\^22"):
            _evaluate_pwm(res, ctl, **ok)
        wide[1] = -226_000                                   # 9 x 466 000 + 1 = 4 194 001 <= 2^22: the library is what comes next
        with pytest.raises(AssertionError, match="the library was loaded"):
            _evaluate_pwm(res, ctl, **ok)
    assert not out.exists()
    with pytest.raises(AssertionError, match="the library was loaded"):
        _evaluate_pwm(res, ctl, **ok)
    assert not out.exists()
    (res / FileNameDict["processed_fasta_file"]).unlink()
    with pytest.raises(ValueError, match="input.bin.pkl"):
        _evaluate_pwm(res, ctl, **ok)


def test_other_ranks_do_nothing(monkeypatch):
    from kmap_amd.evaluate import _evaluate_pwm
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "1")
    assert _evaluate_pwm("nowhere", "missing.fa", []) is None


# ---- 5. the verb ------------------------------------------------------------------------------------------------------------------
def test_cli_options_and_defaults(monkeypatch):
    from click.testing import CliRunner
    from kmap_amd import evaluate
    from kmap_amd.cli import cli
    calls = []
    monkeypatch.setattr(evaluate, "_evaluate_pwm", lambda *a: calls.append(a))
    runner = CliRunner()
    r = runner.invoke(cli, ["evaluate_pwm", "--res_dir", "D", "--control_fasta_file", "C.fa", "--matrix_file", "F"])
    assert r.exit_code == 0, r.output
    assert calls[-1] == ("D", "C.fa", ["F"], 1e-4, None, 1.0, None, 10, False, None)
    r = runner.invoke(cli, ["evaluate_pwm", "--res_dir", "D", "--control_fasta_file", "C.fa", "--matrix_file", "F", "--matrix_file", "F2",
                            "--p_value", "1e-3", "--min_score", "10.62", "--pseudocount", "0.5", "--revcom_mode", "False", "--min_reads", "3",
                            "--read_scores", "--output_dir", "O"])
    assert r.exit_code == 0, r.output
    assert calls[-1] == ("D", "C.fa", ["F", "F2"], 1e-3, 10.62, 0.5, False, 3, True, "O")
    for missing in (["--control_fasta_file", "C.fa", "--matrix_file", "F"], ["--res_dir", "D", "--matrix_file", "F"],
                    ["--res_dir", "D", "--control_fasta_file", "C.fa"]):
        assert runner.invoke(cli, ["evaluate_pwm"] + missing).exit_code == 2
    assert len(calls) == 2
    r = runner.invoke(cli, ["evaluate_pwm", "--help"])
    for opt in ("--res_dir", "--control_fasta_file", "--matrix_file", "--p_value", "--min_score", "--pseudocount", "--revcom_mode",
                "--min_reads", "--read_scores", "--output_dir"):
        assert opt in r.output, opt
    assert "evaluate_pwm" in runner.invoke(cli, ["--help"]).output
    import kmap_amd.cli as cli_module
    assert "evaluate_pwm" in cli_module.__doc__


# ---- 6. the library's entries -----------------------------------------------------------------------------------------------------
def test_symbols_registered():
    from kmap_amd import _ffi
    header = (ROOT / "include" / "kmap_hip.h").read_text()
    for name in ("kmap_readscore_packed_dev", "kmap_readscore_hist_dev"):
        assert name in _ffi.exported_symbols() and f"int {name}(" in header
    assert not [s for s in _ffi.exported_symbols() if s.startswith("kmap_pwm_") and "readscore" in s]
