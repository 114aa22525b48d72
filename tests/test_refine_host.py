"""refine_pwm on the host (kmap_amd/refine.py): the loop over the numpy model of tests/_refine_model.py on the
golden reads and matrices, its four ways to stop through stub count functions, the padding, the information content and the files."""
import re
from pathlib import Path

import numpy as np
import pytest

from tests import _refine_model as M

ROOT = Path(__file__).resolve().parent.parent
GOLD = ROOT / "tests" / "golden"
MOTIF0, MOTIF1 = GOLD / "report_testfa" / "cntmat_motif0_CAATCGATAGC.csv", GOLD / "report_testfa" / "cntmat_motif1_ACCTACGTA.csv"

# start, flank, select, max_iter -> threshold / hits / selected / minus per iteration, status, consensus (p = 1e-4, a = 1, both strands)
ANCHORS = [
    ("motif1", 0, "best", 20, [(1062, 488, 377, 6), (712, 411, 385, 3), (708, 411, 385, 2), (708, 411, 385, 2)], "converged", "ACCTACGTA"),
    ("motif1", 2, "best", 20, [(1062, 453, 358, 6), (501, 405, 381, 4), (508, 399, 381, 3), (512, 399, 382, 3), (524, 397, 382, 3)],
     "converged", "GGACCTACGTACC"),
    ("motif0", 0, "all", 20, [(962, 507, 507, 133), (877, 506, 506, 133), (873, 506, 506, 133)], "converged", "CAATCGATAGC"),
    ("motif0", 0, "best", 20, [(962, 507, 374, 3), (722, 398, 373, 1), (716, 377, 372, 1), (708, 376, 372, 1)], "converged", "AAATCGATAGC"),
    ("motif0", 2, "all", 5, {0: (962, 449, 449, 117), 4: (894, 585, 585, 275)}, "max_iter", "CGCAATCGATAGCGT"),
]


@pytest.fixture(scope="module")
def testfa():
    return M.encode_fasta_np(GOLD / "test.fa")


@pytest.mark.parametrize("start,flank,select,max_iter,rows,status,consensus", ANCHORS)
def test_loop_over_the_model_reproduces_the_anchors(testfa, start, flank, select, max_iter, rows, status, consensus):
    from kmap_amd.pwm import pwm_consensus, read_count_matrix
    from kmap_amd.refine import refine_matrix
    seq, borders = testfa
    assert len(seq) == 45_979 and len(borders) == 1002
    C0 = read_count_matrix(MOTIF0 if start == "motif0" else MOTIF1)
    result, got_status, trace = refine_matrix(C0, M.model_count_fn(seq, borders, True, select == "best"), flank, 1e-4, 1.0, max_iter)
    assert got_status == status and pwm_consensus(result) == consensus and result.shape == (4, C0.shape[1] + 2 * flank)
    assert [r[0] for r in trace] == list(range(1, len(trace) + 1))
    if isinstance(rows, dict):
        assert len(trace) == max_iter
        for i, want in rows.items():
            assert trace[i][1:5] == want
    else:
        assert [r[1:5] for r in trace] == rows
    if status == "converged":
        assert trace[-1][7] == 0 and all(r[7] > 0 for r in trace[:-1])          # cells_changed
    assert (result.sum(axis=0) == trace[-1][3]).all()                           # every column sums to n_selected
    if flank == 2 and start == "motif1":
        assert "GGACCTACGTAC" in consensus                                       # twelve of the planted AGGACCTACGTAC


def _stub(mats):
    """count_fn that hands out the given matrices in turn, (C, n_hits, n_selected, n_minus) with n_selected = a column's sum"""
    it = iter(mats)

    def fn(W, t):
        C = np.asarray(next(it), np.int64)
        n = int(C[:, 0].sum())
        return C, n + 1, n, 0
    return fn


def _mat(seed, w=6, n=40):
    rng = np.random.default_rng(seed)
    return np.stack([np.bincount(rng.integers(0, 4, n), minlength=4) for _ in range(w)], axis=1).astype(np.int64)


def test_the_four_ways_to_stop():
    from kmap_amd.refine import pad_matrix, refine_matrix
    A, B, C, D = (_mat(s) for s in range(4))
    # converged: C' equals the matrix it was scanned with
    res, status, trace = refine_matrix(A, _stub([B, C, C, D]))
    assert status == "converged" and len(trace) == 3 and np.array_equal(res, C)
    # cycle: C' equals an earlier matrix of the run, not the last one -- the input counts as one
    res, status, trace = refine_matrix(A, _stub([B, C, B, D]))
    assert status == "cycle" and len(trace) == 3 and np.array_equal(res, B)
    res, status, trace = refine_matrix(A, _stub([B, A, D]))
    assert status == "cycle" and len(trace) == 2 and np.array_equal(res, A)
    # max_iter: the limit, and the last matrix is the result
    res, status, trace = refine_matrix(A, _stub([B, C, D, A]), max_iter=3)
    assert status == "max_iter" and len(trace) == 3 and np.array_equal(res, D)
    # no_hits at once: the padded input comes back
    Z = np.zeros((4, 10), np.int64)
    res, status, trace = refine_matrix(A, _stub([Z]), flank=2)
    assert status == "no_hits" and len(trace) == 1 and trace[0][3] == 0 and np.array_equal(res, pad_matrix(A, 2))
    assert res.shape == (4, 10) and not res[:, :2].any() and not res[:, -2:].any() and np.array_equal(res[:, 2:8], A)
    # no_hits later: the last matrix built from a selected window
    res, status, trace = refine_matrix(A, _stub([B, np.zeros((4, 6), np.int64), C]))
    assert status == "no_hits" and len(trace) == 2 and np.array_equal(res, B)
    with pytest.raises(ValueError):
        refine_matrix(A, _stub([B]), max_iter=0)
    with pytest.raises(ValueError):
        refine_matrix(A, _stub([np.zeros((4, 7), np.int64)]))                    # a count_fn that changes the width


def test_flank_columns_weigh_nothing_in_the_first_iteration():
    from kmap_amd.pwm import pwm_weights, read_count_matrix
    from kmap_amd.refine import refine_matrix
    C0 = read_count_matrix(MOTIF1)
    seen = []

    def fn(W, t):
        seen.append((np.array(W), t))
        return np.zeros((4, W.shape[1]), np.int64), 0, 0, 0
    refine_matrix(C0, fn, flank=3)
    W, t = seen[0]
    assert W.shape == (4, 15) and W.dtype == np.int32
    assert not W[:, :3].any() and not W[:, -3:].any()
    np.testing.assert_array_equal(W[:, 3:12], pwm_weights(C0, 1.0))
    assert t == 1062                                                             # the core's own threshold: 4^6 flank sequences per core sequence


def test_width_limit_and_pseudocount_zero():
    from kmap_amd.refine import pad_matrix, refine_matrix
    C = _mat(5, w=11) + 1
    assert pad_matrix(C, 10).shape == (4, 31)
    res, status, _ = refine_matrix(C, _stub([np.zeros((4, 31), np.int64)]), flank=10)
    assert status == "no_hits" and res.shape == (4, 31)
    with pytest.raises(ValueError, match="32"):
        pad_matrix(_mat(5, w=12), 10)
    with pytest.raises(ValueError, match="32"):
        refine_matrix(_mat(5, w=12), _stub([]), flank=10)
    with pytest.raises(ValueError):
        pad_matrix(C, -1)
    # a = 0: fine without a flank as long as no count is zero, an error with one (a zero column has no finite weight)
    refine_matrix(C, _stub([C]), pseudocount=0.0)
    with pytest.raises(ValueError, match="zero count"):
        refine_matrix(C, _stub([C]), flank=1, pseudocount=0.0)


def test_information_bits():
    from kmap_amd.refine import information_bits
    for w in (4, 9, 31):
        onehot = np.zeros((4, w), np.int64)
        onehot[np.arange(w) % 4, np.arange(w)] = 17
        assert information_bits(onehot, 0.0) == 2.0 * w
        assert information_bits(np.full((4, w), 5), 0.0) == 0.0
        assert information_bits(np.full((4, w), 5), 1.0) == 0.0
        assert 0 < information_bits(onehot, 1.0) < 2.0 * w
    assert information_bits(np.zeros((4, 6), np.int64), 1.0) == 0.0               # empty columns: the pseudocount alone, uniform
    assert information_bits(np.zeros((4, 6), np.int64), 0.0) == 0.0
    col = np.array([[6], [2], [0], [0]]).repeat(4, axis=1)
    assert information_bits(col, 0.0) == pytest.approx(4 * (2 + 0.75 * np.log2(0.75) + 0.25 * np.log2(0.25)), rel=1e-15)


def test_written_matrix_round_trips(tmp_path, testfa):
    from kmap_amd.pwm import pwm_consensus, read_count_matrix
    from kmap_amd.refine import refine_matrix
    seq, borders = testfa
    result, _, _ = refine_matrix(read_count_matrix(MOTIF1), M.model_count_fn(seq, borders, True, True), 2)
    path = tmp_path / f"refined_cntmat_motif0_{pwm_consensus(result)}.csv"
    np.savetxt(path, result, delimiter=",", fmt="%d")
    back = read_count_matrix(path)
    assert back.dtype == np.int64
    np.testing.assert_array_equal(back, result)


def test_verb_checks_its_input_before_the_device(tmp_path, monkeypatch):
    from kmap_amd._toml import dump_toml
    from kmap_amd.kmer_count import FileNameDict, read_default_config_file
    from kmap_amd.refine import _refine_pwm
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "1")
    assert _refine_pwm(str(tmp_path / "no_such_dir"), [str(MOTIF0)]) is None     # rank 0 works alone
    monkeypatch.setenv("RANK", "0")
    with pytest.raises(ValueError, match="config.toml is missing"):
        _refine_pwm(str(tmp_path / "no_such_dir"), [str(MOTIF0)])
    monkeypatch.delenv("WORLD_SIZE")
    monkeypatch.delenv("RANK")
    res = tmp_path / "res"
    res.mkdir()
    dump_toml(read_default_config_file(), res / "config.toml")
    out = tmp_path / "out"
    reads = [FileNameDict["processed_fasta_file"], FileNameDict["processed_fasta_seqboarder_file"]]
    for name in reads:                       # the two read files are looked for before a matrix is read or the device touched
        with pytest.raises(ValueError, match=re.escape(name) + " is missing: not a result directory of preproc"):
            _refine_pwm(str(res), [str(MOTIF0)], output_dir=str(out))
        (res / name).write_bytes(b"")
    with pytest.raises(ValueError, match="no matrix file"):
        _refine_pwm(str(res), [], output_dir=str(out))
    with pytest.raises(ValueError, match="select"):
        _refine_pwm(str(res), [str(MOTIF0)], select="first", output_dir=str(out))
    with pytest.raises(ValueError, match="max_iter"):
        _refine_pwm(str(res), [str(MOTIF0)], max_iter=0, output_dir=str(out))
    with pytest.raises(ValueError, match=r"cntmat_motif0.*33"):
        _refine_pwm(str(res), [str(MOTIF1), str(MOTIF0)], flank=11, output_dir=str(out))     # 9 + 22 = 31 passes, 11 + 22 does not
    with pytest.raises(ValueError, match=r"cntmat_motif1.*zero count"):
        _refine_pwm(str(res), [str(MOTIF1)], flank=1, pseudocount=0.0, output_dir=str(out))
    assert not out.exists() and sorted(p.name for p in res.iterdir()) == sorted(["config.toml"] + reads)


def test_cli_lists_refine_pwm():
    from click.testing import CliRunner
    from kmap_amd.cli import cli
    r = CliRunner().invoke(cli, ["--help"])
    assert r.exit_code == 0 and "refine_pwm" in r.output
    r = CliRunner().invoke(cli, ["refine_pwm", "--help"])
    assert r.exit_code == 0
    for opt in ("--res_dir", "--matrix_file", "--flank", "--select", "--p_value", "--pseudocount", "--revcom_mode", "--max_iter", "--output_dir"):
        assert opt in r.output
    r = CliRunner().invoke(cli, ["refine_pwm", "--res_dir", "x"])
    assert r.exit_code != 0 and "--matrix_file" in r.output
    r = CliRunner().invoke(cli, ["refine_pwm", "--res_dir", "x", "--matrix_file", "m", "--select", "first"])
    assert r.exit_code != 0 and "first" in r.output


def test_refine_symbol_is_registered():
    from kmap_amd import _ffi
    header = (ROOT / "include" / "kmap_hip.h").read_text()
    name = "kmap_refine_counts_packed_dev"
    assert name in _ffi.exported_symbols()
    res, args = _ffi._SIGS[name]
    proto = re.sub(r"/\*.*?\*/", "", re.search(rf"int {name}\s*\(([^;]*)\);", header).group(1))
    assert len(args) == proto.count(",") + 1 == 15
