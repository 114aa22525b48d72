"""Host side of scan_pwm (no GPU): the count-matrix parser, the weights, the exact p-value threshold against plain enumeration of all
4^w sequences, the CLI verb and the registration of the two kmap_pwm_* symbols.  The definitions are DESIGN.md section 11."""
import itertools
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
GOLD = ROOT / "tests" / "golden" / "report_testfa"
MOTIF0, MOTIF1 = GOLD / "cntmat_motif0_CAATCGATAGC.csv", GOLD / "cntmat_motif1_ACCTACGTA.csv"

W_MOTIF1 = [[178, -246, -349, -393, 194, -406, -323, -308, 187],
            [-250, 180, 144, -359, -456, 192, -369, -393, -301],
            [-260, -276, 13, -456, -406, -323, 189, -406, -282],
            [-216, -246, -331, 193, -406, -421, -316, 191, -369]]


def all_scores(W):
    """forward score of every one of the 4^w sequences, by enumeration"""
    W = np.asarray(W, np.int64)
    w = W.shape[1]
    seqs = np.array(list(itertools.product(range(4), repeat=w)), np.int64)
    return W[seqs, np.arange(w)].sum(axis=1)


def brute_threshold(scores, p):
    """smallest integer t with #{score >= t} <= p 4^w, searched upwards from the minimum"""
    limit = p * len(scores)
    for t in range(int(scores.min()), int(scores.max()) + 2):
        if np.count_nonzero(scores >= t) <= limit:
            return t
    raise AssertionError("unreachable: N(max + 1) = 0")


def test_golden_weights_and_consensus():
    from kmap_amd.pwm import pwm_consensus, pwm_weights, read_count_matrix
    C1, C0 = read_count_matrix(MOTIF1), read_count_matrix(MOTIF0)
    assert C1.dtype == np.int64 and C1.shape == (4, 9) and C0.shape == (4, 11)
    np.testing.assert_array_equal(C1, np.loadtxt(MOTIF1, delimiter=",", dtype=np.int64))
    W1, W0 = pwm_weights(C1), pwm_weights(C0)
    assert W1.dtype == np.int32 and W0.dtype == np.int32
    assert W1.tolist() == W_MOTIF1
    assert (int(W0.min()), int(W0.max())) == (-602, 194)
    assert pwm_consensus(C0) == "CAATCGATAGC" and pwm_consensus(C1) == "ACCTACGTA"
    # the written-out definition, a = 1
    f = (C1 + 0.25) / (C1.sum(axis=0) + 1.0)
    np.testing.assert_array_equal(W1, np.rint(np.log2(f / 0.25) * 100).astype(np.int32))
    # ties: the first of A, C, G, T
    assert pwm_consensus(np.array([[1, 0, 2, 2], [1, 3, 2, 0], [0, 3, 1, 2], [0, 0, 2, 2]])) == "ACAA"


@pytest.mark.parametrize("w", [4, 6, 8])
def test_threshold_against_enumeration(w):
    from kmap_amd.pwm import pwm_threshold, score_counts
    rng = np.random.default_rng(100 + w)
    W = rng.integers(-3000, 201, size=(4, w)).astype(np.int32)
    W[:, w // 2] = -17                                        # a column that cannot tell the bases apart
    scores = all_scores(W)
    lo, dist = score_counts(W)
    assert lo == scores.min() and lo + len(dist) - 1 == scores.max() and dist.dtype == np.int64
    np.testing.assert_array_equal(dist, np.bincount(scores - lo))
    for m in (0, 1, 7, 4 ** w // 2):
        p = (m + 0.5) / 4 ** w                                 # p 4^w = m + 0.5 never ties with a count
        t, smin, smax = pwm_threshold(W, p)
        assert (smin, smax) == (scores.min(), scores.max())
        assert t == brute_threshold(scores, p), (w, m)
        assert np.count_nonzero(scores >= t) <= m and (t == smin or np.count_nonzero(scores >= t - 1) > m)
    assert pwm_threshold(W, 1.0)[0] == scores.min()


def test_threshold_above_the_maximum_when_the_best_score_is_shared():
    from kmap_amd.pwm import pwm_threshold
    W = np.array([[5, 1, -3, 0], [5, -2, -4, -9], [-1, -2, -5, -9], [-7, -8, -6, -9]], np.int32)   # A and C tie in column 0
    scores = all_scores(W)
    assert np.count_nonzero(scores == scores.max()) == 2
    p = 0.5 / 4 ** 4
    assert pwm_threshold(W, p)[0] == scores.max() + 1 == brute_threshold(scores, p)
    assert pwm_threshold(W, 1.5 / 4 ** 4)[0] == scores.max() + 1            # one sequence allowed, two share the best score
    assert pwm_threshold(W, 2.5 / 4 ** 4)[0] == scores.max()
    assert pwm_threshold(W, 0.0)[0] == scores.max() + 1


def test_golden_thresholds():
    from kmap_amd.pwm import pwm_threshold, pwm_weights, read_count_matrix
    for path, want in ((MOTIF0, (457, 962, 1356)), (MOTIF1, (576, 1062, 1255))):
        W = pwm_weights(read_count_matrix(path))
        assert tuple(pwm_threshold(W, p)[0] for p in (1e-3, 1e-4, 1e-5)) == want
    W1 = pwm_weights(read_count_matrix(MOTIF1))
    scores = all_scores(W1)                                                    # 4^9 sequences: the DP against enumeration
    for p in (1e-3, 1e-4, 1e-5):
        assert pwm_threshold(W1, p)[0] == brute_threshold(scores, p)


def test_width_31_does_not_overflow():
    from kmap_amd.pwm import pwm_threshold, score_counts
    rng = np.random.default_rng(31)
    W = rng.integers(-3000, 201, size=(4, 31)).astype(np.int32)
    lo, dist = score_counts(W)
    assert dist.dtype == np.int64 and (dist >= 0).all()
    assert sum(int(x) for x in dist) == 4 ** 31                              # N(min score), summed in Python integers
    assert int(np.cumsum(dist[::-1])[-1]) == 4 ** 31                         # and as the int64 running sum the threshold uses
    t, smin, smax = pwm_threshold(W, 1e-4)
    assert smin == lo == int(W.min(axis=0).sum()) and smax == int(W.max(axis=0).sum()) and smin < t <= smax
    n_ge = np.cumsum(dist[::-1])[::-1]
    assert int(n_ge[t - lo]) <= 1e-4 * 4 ** 31 < int(n_ge[t - 1 - lo])
    # the largest counts the definitions allow for: 10^9 per column, |score| < 10^5
    from kmap_amd.pwm import pwm_weights
    C = np.zeros((4, 31), np.int64)
    C[0] = 10 ** 9
    Wb = pwm_weights(C)
    assert Wb.dtype == np.int32 and abs(int(Wb.min(axis=0).sum())) < 10 ** 5 and int(Wb.max(axis=0).sum()) < 10 ** 5
    assert pwm_threshold(Wb, 1e-4)[2] == 31 * 200


@pytest.mark.parametrize("text,what", [
    ("1,2,3,4\n1,2,3,4\n1,2,3,4\n", "3 rows"),
    ("1,2,3,4\n1,2,3,4\n1,2,3,4\n1,2,3,4\n1,2,3,4\n", "5 rows"),
    ("1,2,3,4\n1,2,3\n1,2,3,4\n1,2,3,4\n", "equal length"),
    ("1,2,3,4\n1,-2,3,4\n1,2,3,4\n1,2,3,4\n", "non-negative integers"),
    ("1,2,3,4\n1,2,3,4\n1,1.5,3,4\n1,2,3,4\n", "non-negative integers"),
    ("1 2 3 4\n1 2 3 4\n1 2 3 4\n1 2 3 4\n", "non-negative integers"),
    ("1,2,3\n1,2,3\n1,2,3\n1,2,3\n", "width 3"),
    ("\n".join(",".join("1" * 1 for _ in range(32)) for _ in range(4)) + "\n", "width 32"),
    ("", "0 rows"),
])
def test_parser_rejects(tmp_path, text, what):
    from kmap_amd.pwm import read_count_matrix
    f = tmp_path / "bad_matrix.csv"
    f.write_text(text)
    with pytest.raises(ValueError, match=rf"bad_matrix\.csv.*{what}"):
        read_count_matrix(f)


def test_parser_reads_what_savetxt_writes(tmp_path):
    from kmap_amd.pwm import pwm_weights, read_count_matrix
    rng = np.random.default_rng(5)
    for w in (4, 31):
        C = rng.integers(0, 10 ** 9, size=(4, w))
        C[2, 1] = 0
        f = tmp_path / f"m{w}.csv"
        np.savetxt(f, C, delimiter=",", fmt="%d")
        got = read_count_matrix(f)
        assert got.dtype == np.int64
        np.testing.assert_array_equal(got, C)
    # a zero count: fine with a pseudocount, no finite weight without one
    C = np.array([[5, 0, 1, 2], [1, 9, 1, 2], [1, 1, 7, 2], [1, 1, 1, 2]])
    W = pwm_weights(C, 1.0)
    assert W[0, 1] == int(np.rint(np.log2((0.25 / 12) / 0.25) * 100))
    with pytest.raises(ValueError, match="zero count"):
        pwm_weights(C, 0.0)
    np.testing.assert_array_equal(pwm_weights(C + 1, 0.0), np.rint(np.log2((C + 1) / (C + 1).sum(axis=0) / 0.25) * 100).astype(np.int32))
    with pytest.raises(ValueError):
        pwm_weights(C, -1.0)


def test_min_score_threshold_is_the_decimal_ceiling():
    from kmap_amd.pwm import min_score_threshold
    assert [min_score_threshold(s) for s in (10.62, 9.62, 4.57, 12.55, 13.56, 0.0, -0.5, 3.001, -3.001, 7)] == \
        [1062, 962, 457, 1255, 1356, 0, -50, 301, -300, 700]


def test_only_rank_zero_scans_and_bad_input_writes_nothing(tmp_path, monkeypatch):
    """the other ranks of a torch.distributed launch return at once; a bad matrix is reported before any output exists"""
    from kmap_amd._toml import dump_toml
    from kmap_amd.kmer_count import FileNameDict, read_default_config_file
    from kmap_amd.pwm import _scan_pwm
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "1")
    assert _scan_pwm(str(tmp_path / "no_such_dir"), [str(MOTIF0)]) is None
    monkeypatch.setenv("RANK", "0")
    with pytest.raises(ValueError, match="config.toml is missing"):
        _scan_pwm(str(tmp_path / "no_such_dir"), [str(MOTIF0)])
    monkeypatch.delenv("WORLD_SIZE")
    monkeypatch.delenv("RANK")
    res = tmp_path / "res"
    res.mkdir()
    dump_toml(read_default_config_file(), res / "config.toml")
    reads = [FileNameDict["processed_fasta_file"], FileNameDict["processed_fasta_seqboarder_file"]]
    for name in reads:                       # the two read files are looked for before a matrix is read or the device touched
        with pytest.raises(ValueError, match=re.escape(name) + " is missing: not a result directory of preproc"):
            _scan_pwm(str(res), [str(MOTIF0)], output_dir=str(tmp_path / "out"))
        (res / name).write_bytes(b"")
    bad = tmp_path / "bad_matrix.csv"
    bad.write_text("1,2,3,4\n1,2,3,4\n1,2,3,4\n")
    with pytest.raises(ValueError, match=r"bad_matrix\.csv"):
        _scan_pwm(str(res), [str(MOTIF0), str(bad)], output_dir=str(tmp_path / "out"))
    zero = tmp_path / "zero.csv"
    zero.write_text("5,0,1,2\n1,9,1,2\n1,1,7,2\n1,1,1,2\n")
    with pytest.raises(ValueError, match=r"zero\.csv.*zero count"):
        _scan_pwm(str(res), [str(zero)], pseudocount=0.0, output_dir=str(tmp_path / "out"))
    assert not (tmp_path / "out").exists() and sorted(p.name for p in res.iterdir()) == sorted(["config.toml"] + reads)


def test_cli_lists_scan_pwm():
    from click.testing import CliRunner
    from kmap_amd.cli import cli
    r = CliRunner().invoke(cli, ["--help"])
    assert r.exit_code == 0 and "scan_pwm" in r.output
    r = CliRunner().invoke(cli, ["scan_pwm", "--help"])
    assert r.exit_code == 0
    for opt in ("--res_dir", "--matrix_file", "--p_value", "--min_score", "--pseudocount", "--revcom_mode", "--output_dir"):
        assert opt in r.output
    assert "per strand" in " ".join(r.output.split())
    r = CliRunner().invoke(cli, ["scan_pwm", "--res_dir", "x"])
    assert r.exit_code != 0 and "--matrix_file" in r.output                          # required


def test_pwm_symbols_are_registered():
    from kmap_amd import _ffi
    header = (ROOT / "include" / "kmap_hip.h").read_text()
    declared = set(re.findall(r"\b(kmap_pwm_[A-Za-z0-9_]+)\s*\(", header))
    assert declared == {"kmap_pwm_scan_packed_dev", "kmap_pwm_scan_fetch"}
    assert declared <= set(_ffi.exported_symbols())
    for name in declared:
        res, args = _ffi._SIGS[name]
        proto = re.sub(r"/\*.*?\*/", "", re.search(rf"int {name}\s*\(([^;]*)\);", header).group(1))
        assert len(args) == proto.count(",") + 1, name                               # one ctypes argument per C parameter
