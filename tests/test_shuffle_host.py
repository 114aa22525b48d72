"""Host side of shuffle_reads (no GPU): the restatement of DESIGN.md section 15 in tests/_shuffle_model.py -- what a shuffle keeps,
that it is uniform over what it may return, its two forms against each other --, the verb's argument errors (raised before the
library is loaded), the CLI verb, the FASTA writer byte for byte and the library's new entry."""
import pickle
from pathlib import Path

import numpy as np
import pytest

from tests import _shuffle_model as M

ROOT = Path(__file__).resolve().parent.parent
CODE = {c: i for i, c in enumerate("ACGT")}
SEED = 15


@pytest.fixture(autouse=True)
def model_draws_are_the_package_s():
    """the model stands for the package only while its draws are the package's; without kmap_amd.shuffle no test here says anything"""
    from kmap_amd import shuffle
    assert (M.GOLDEN, M.mix64(SEED), M.copy_seed(SEED, 1)) == (shuffle.GOLDEN, shuffle.mix64(SEED), shuffle.copy_seed(SEED, 1))


def encode(text):
    """ACGT -> 0..3, anything else -> 255"""
    return np.array([CODE.get(c, 255) for c in text], np.uint8)


def mixed_array(rng, n_reads=300):
    """reads of lengths 0..70 over alphabets of one to four letters, a 255 behind each, some N inside"""
    parts = []
    for _ in range(n_reads):
        parts += [rng.integers(0, rng.integers(1, 5), rng.integers(0, 71)).astype(np.uint8), np.array([255], np.uint8)]
    seq = np.concatenate(parts)
    seq[rng.random(len(seq)) < 0.02] = 255
    return seq


# ---- 1. the draws and the trees ---------------------------------------------------------------------------------------------------
def test_draws_are_the_package_s():
    from kmap_amd import shuffle
    for x in (0, 1, 2 ** 64 - 1, 0x0123456789ABCDEF):
        assert M.mix64(x) == shuffle.mix64(x) < 2 ** 64
        for c in (0, 1, 7):
            assert M.copy_seed(x, c) == shuffle.copy_seed(x, c) < 2 ** 64
    assert M.mix64(0) == 0xE220A8397B1DCDAF                  # splitmix64's first output for the seed 0
    assert len({M.copy_seed(0, c) for c in range(100)}) == 100
    assert all(0 <= M.draw(M.segment_key(3, 5), i, b) < b for i in range(50) for b in (1, 2, 3, 1000, 2 ** 63 - 1))
    h = np.array([0, 1, 2 ** 64 - 1, 0x0123456789ABCDEF, 2 ** 63], np.uint64)
    b = np.array([2 ** 63 - 1, 2 ** 64 - 1, 2 ** 64 - 1, 12345678901234567, 3], np.uint64)
    assert M.np_mulhi(h, b).tolist() == [(int(x) * int(y)) >> 64 for x, y in zip(h, b)]
    assert M.np_mix64(h).tolist() == [M.mix64(int(x)) for x in h]


def test_sixteen_trees_per_root():
    for z in range(4):
        assert len(M.TREES[z]) == 16 == int(M.VALID[z].sum())
        for t in M.TREES[z]:
            assert all(tv != v for v, tv in zip(M.others(z), t))             # no self-loop is a tree edge


# ---- 2. what a shuffle keeps --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("klet", [1, 2])
def test_invariants_and_the_two_forms(klet):
    rng = np.random.default_rng(150 + klet)
    seq = mixed_array(rng)
    seq = np.concatenate([seq, rng.integers(0, 4, 700).astype(np.uint8)])                    # a long segment, and no 255 at the end
    out = M.shuffle_array(seq, klet, SEED)
    np.testing.assert_array_equal(out == 255, seq == 255)
    assert out.dtype == np.uint8 and (out[out != 255] < 4).all()
    np.testing.assert_array_equal(M.base_counts(out), M.base_counts(seq))
    starts, lens = M.segments(seq)
    if klet == 2:
        for got, want in zip(M.pair_counts(out), M.pair_counts(seq)):
            np.testing.assert_array_equal(got, want)
        for s, n in zip(starts[lens <= 3], lens[lens <= 3]):
            np.testing.assert_array_equal(out[s:s + n], seq[s:s + n])
    moved = sum(not np.array_equal(out[s:s + n], seq[s:s + n]) for s, n in zip(starts, lens))
    assert moved > len(starts) // 3
    # the scalar form, segment by segment
    for s, n in zip(starts.tolist(), lens.tolist()):
        assert out[s:s + n].tolist() == M.shuffle_segment(seq[s:s + n], s, klet, SEED)
    # the seed and the position of a segment, nothing else, decide
    assert not np.array_equal(M.shuffle_array(seq, klet, SEED + 1), out)
    np.testing.assert_array_equal(M.shuffle_array(seq, klet, SEED), out)
    shifted = M.shuffle_array(np.concatenate([[255], seq]).astype(np.uint8), klet, SEED)[1:]
    assert not np.array_equal(shifted, out)
    s, n = int(starts[np.argmax(lens)]), int(lens.max())
    alone = np.full(len(seq), 255, np.uint8)
    alone[s:s + n] = seq[s:s + n]
    np.testing.assert_array_equal(M.shuffle_array(alone, klet, SEED)[s:s + n], out[s:s + n])


def test_one_and_two_letter_reads():
    seq = encode("AAAAAAAAAAAAAAAAAAAAN" + "ACACACACACACACACACN" + "TTTTTTTTTTTTG" + "N" + "CCCCCCCCCA")
    for klet in (1, 2):
        out = M.shuffle_array(seq, klet, SEED)
        assert out[:20].tolist() == [0] * 20
        np.testing.assert_array_equal(M.base_counts(out), M.base_counts(seq))
    out = M.shuffle_array(seq, 2, SEED)
    assert out[21:39].tolist() == encode("ACACACACACACACACAC").tolist()          # AC x 9, CA x 8: one walk
    assert out[40:53].tolist() == encode("TTTTTTTTTTTTG").tolist()              # the last base occurs once: one walk
    assert out[54:].tolist() == encode("CCCCCCCCCA").tolist()


# ---- 3. uniform over what it may return ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("text,klet,n_arrangements", [("GATTACAGATTC", 2, 36), ("AAACCAGTCAGA", 2, 120), ("AACGT", 1, 60)])
def test_uniform(text, klet, n_arrangements):
    from scipy.stats import chi2
    x = encode(text)
    every = M.all_arrangements(x, klet)
    assert len(every) == n_arrangements and tuple(x.tolist()) in every
    n = 2000 * n_arrangements
    seq = np.tile(np.concatenate([x, [255]]).astype(np.uint8), n)
    out = M.shuffle_array(seq, klet, SEED).reshape(n, len(x) + 1)[:, :-1]
    seen, counts = np.unique(out, axis=0, return_counts=True)
    assert [tuple(r) for r in seen.tolist()] == every
    stat = float(((counts - 2000.0) ** 2 / 2000.0).sum())
    print(f"{text} klet {klet}: chi2 {stat:.1f} at {n_arrangements - 1} degrees of freedom")
    assert stat < chi2.ppf(1 - 1e-9, n_arrangements - 1)


# ---- 4. the verb's arguments --------------------------------------------------------------------------------------------------------
@pytest.fixture
def res_dir(tmp_path):
    """a tiny hand-made preproc result directory: ACGTNAC, an empty read, GG"""
    from kmap_amd.kmer_count import FileNameDict
    res = tmp_path / "res"
    res.mkdir()
    with open(res / FileNameDict["processed_fasta_file"], "wb") as fh:
        pickle.dump(np.array([0, 1, 2, 3, 255, 0, 1, 255, 255, 2, 2, 255], np.uint8), fh)
    with open(res / FileNameDict["processed_fasta_seqboarder_file"], "wb") as fh:
        pickle.dump(np.array([[0, 7], [8, 8], [9, 11]], np.int64), fh)
    return res


def test_value_errors_come_before_the_library(res_dir, tmp_path, monkeypatch):
    from kmap_amd import _ffi
    from kmap_amd.kmer_count import FileNameDict
    from kmap_amd.shuffle import _shuffle_reads

    def no_lib():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_ffi, "lib", no_lib)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    out = tmp_path / "out" / "control.fa"
    ok = dict(klet=2, seed=0, n_copies=1, output_file=str(out))
    bad = [(dict(), tmp_path / "nowhere", "input.bin.pkl"),
           (dict(klet=0), res_dir, "klet"), (dict(klet=3), res_dir, "klet"), (dict(klet=1.5), res_dir, "klet"),
           (dict(klet=True), res_dir, "klet"),
           (dict(n_copies=0), res_dir, "n_copies"), (dict(n_copies=-2), res_dir, "n_copies"), (dict(n_copies=1.5), res_dir, "n_copies"),
           (dict(seed=-1), res_dir, "seed"), (dict(seed=2 ** 64), res_dir, "seed"), (dict(seed=0.5), res_dir, "seed")]
    for change, r, word in bad:
        with pytest.raises(ValueError, match=word):
            _shuffle_reads(r, **{**ok, **change})
    for good in (dict(), dict(klet=1), dict(seed=2 ** 64 - 1), dict(n_copies=3)):
        with pytest.raises(AssertionError, match="the library was loaded"):
            _shuffle_reads(res_dir, **{**ok, **good})
    assert not out.parent.exists()
    (res_dir / FileNameDict["processed_fasta_seqboarder_file"]).unlink()
    with pytest.raises(ValueError, match="seqboarder"):
        _shuffle_reads(res_dir, **ok)


def test_other_ranks_do_nothing(monkeypatch):
    from kmap_amd.shuffle import _shuffle_reads
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "1")
    assert _shuffle_reads("nowhere", klet=7) is None


def test_cli_options_and_defaults(monkeypatch):
    from click.testing import CliRunner
    from kmap_amd import shuffle
    from kmap_amd.cli import cli
    calls = []
    monkeypatch.setattr(shuffle, "_shuffle_reads", lambda *a: calls.append(a))
    runner = CliRunner()
    r = runner.invoke(cli, ["shuffle_reads", "--res_dir", "D"])
    assert r.exit_code == 0, r.output
    assert calls[-1] == ("D", 2, 0, 1, None)
    r = runner.invoke(cli, ["shuffle_reads", "--res_dir", "D", "--klet", "1", "--seed", str(2 ** 64 - 1), "--n_copies", "3",
                            "--output_file", "O.fa"])
    assert r.exit_code == 0, r.output
    assert calls[-1] == ("D", 1, 2 ** 64 - 1, 3, "O.fa")
    assert runner.invoke(cli, ["shuffle_reads"]).exit_code == 2
    assert runner.invoke(cli, ["shuffle_reads", "--res_dir", "D", "--klet", "two"]).exit_code == 2
    assert len(calls) == 2
    r = runner.invoke(cli, ["shuffle_reads", "--help"])
    for opt in ("--res_dir", "--klet", "--seed", "--n_copies", "--output_file"):
        assert opt in r.output, opt
    assert "shuffle_reads" in runner.invoke(cli, ["--help"]).output
    import kmap_amd.cli as cli_module
    assert "shuffle_reads" in cli_module.__doc__
    # the two verbs the file is for still demand a control file
    for verb in ("enrich_kmers", "evaluate_pwm"):
        assert runner.invoke(cli, [verb, "--res_dir", "D", "--matrix_file", "F"]).exit_code == 2


# ---- 5. the writer ------------------------------------------------------------------------------------------------------------------
def test_fasta_writer_bytes(tmp_path):
    from kmap_amd import shuffle
    seq = np.array([0, 1, 2, 3, 255, 0, 1, 255, 255, 2, 2, 255], np.uint8)
    borders = np.array([[0, 7], [8, 8], [9, 11]], np.int64)
    other = np.array([3, 2, 1, 0, 255, 1, 0, 255, 255, 2, 2, 255], np.uint8)
    path = tmp_path / "two.fa"
    with open(path, "wb") as fh:
        shuffle.write_fasta_records(fh, seq, borders, 0)
        shuffle.write_fasta_records(fh, other, borders, 1)
    assert path.read_bytes() == (b">shuffled_0_0\nACGTNAC\n>shuffled_0_1\n\n>shuffled_0_2\nGG\n"
                                 b">shuffled_1_0\nTGCANCA\n>shuffled_1_1\n\n>shuffled_1_2\nGG\n")
    with open(path, "wb") as fh:                             # no reads: nothing
        shuffle.write_fasta_records(fh, np.zeros(0, np.uint8), np.zeros((0, 2), np.int64), 0)
    assert path.read_bytes() == b""
    # more reads than one write holds: the second chunk starts where the first ended
    n = shuffle.WRITE_CHUNK + 3
    seq = np.tile(np.array([2, 0, 255], np.uint8), n)
    borders = np.stack([np.arange(n) * 3, np.arange(n) * 3 + 2], axis=1)
    with open(path, "wb") as fh:
        shuffle.write_fasta_records(fh, seq, borders, 4)
    lines = path.read_bytes().split(b"\n")
    assert len(lines) == 2 * n + 1 and lines[-1] == b"" and set(lines[1::2]) == {b"GA"}
    assert lines[0] == b">shuffled_4_0" and lines[2 * shuffle.WRITE_CHUNK] == b">shuffled_4_%d" % shuffle.WRITE_CHUNK
    assert shuffle.unchanged_by_definition(np.array([0, 1, 2, 3, 255, 0, 1, 255, 255, 2, 255, 1, 1, 1, 1, 1], np.uint8), 2) == (4, 12, 2)
    assert shuffle.unchanged_by_definition(np.array([0, 1, 2, 3, 255, 0, 1, 255, 255, 2, 255, 1, 1, 1, 1, 1], np.uint8), 1) == (4, 12, 1)


# ---- 6. the library's entry ---------------------------------------------------------------------------------------------------------
def test_symbol_registered():
    from kmap_amd import _ffi
    header = (ROOT / "include" / "kmap_hip.h").read_text()
    assert "kmap_shuffle_packed_dev" in _ffi.exported_symbols() and "int kmap_shuffle_packed_dev(" in header
    res, args = _ffi._SIGS["kmap_shuffle_packed_dev"]
    assert res is _ffi.i32 and len(args) == 8 and args[4] is _ffi.u64
    if _ffi.LIB_PATH.exists():                               # built: the library exports it
        import ctypes
        assert hasattr(ctypes.CDLL(str(_ffi.LIB_PATH)), "kmap_shuffle_packed_dev")
    assert (ROOT / "kmap_amd" / "csrc" / "shuffle.hip").exists()
