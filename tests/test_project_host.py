"""Host side of project_kmers (no GPU): the LUT3 chain, the k-mer file parser, the anchor file checks, the CLI verb and the
registration of the kmap_project_* symbols."""
import pickle
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent


@pytest.mark.parametrize("k,n_nb", [(8, 20), (16, 20), (6, 5), (12, 7)])
def test_lut3_is_the_written_out_chain(k, n_nb):
    """hd_prob_lut_projected = hd_prob_lut's chain with three float32 divisions, over s = 0 .. n_nb^3 k"""
    from kmap_amd.projection import hd_prob_lut_projected
    got = hd_prob_lut_projected(k, n_nb)
    s = np.arange(n_nb ** 3 * k + 1, dtype=np.float32)
    S = ((s / np.float32(n_nb)) / np.float32(n_nb)) / np.float32(n_nb)
    assert S.dtype == np.float32
    T = 16.0 / (1 + np.exp(-(0.2 * k - 0.2) * (S - k / 2)))
    want = np.exp(-T / 0.5).astype("float32")
    assert got.dtype == np.float32 and got.shape == want.shape
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("k,n_nb", [(8, 20), (16, 20), (6, 5), (12, 7)])
def test_lut3_at_stride_n_nb_is_the_maps_lut(k, n_nb):
    """A query whose n_nb neighbour rows are all the same row s has the sum n_nb s and must get that row's p: f32(n_nb s) is exact
    (< 2^24) and the correctly rounded quotient of an exact multiple is exact, so LUT3[n_nb s] == LUT[s] bit for bit."""
    from kmap_amd.projection import hd_prob_lut_projected
    from kmap_amd.visualization import hd_prob_lut
    assert n_nb ** 3 * k < 2 ** 24
    s = np.arange(n_nb * n_nb * k + 1, dtype=np.float32)
    np.testing.assert_array_equal((s * np.float32(n_nb)) / np.float32(n_nb), s)        # the extra division undoes the factor exactly
    lut = hd_prob_lut(k, n_nb, n_nb * n_nb * k)
    lut3 = hd_prob_lut_projected(k, n_nb)
    np.testing.assert_array_equal(lut3[::n_nb][:len(lut)].view(np.uint32), lut.view(np.uint32))


def test_kmer_file_parser(tmp_path):
    from kmap_amd.kmer_count import kmer2hash
    from kmap_amd.projection import read_kmer_file
    f = tmp_path / "q.txt"
    f.write_text("ACGTACGT\n\n  \nacgtTTTT\r\n\nGGGGCCCC")
    given, kh = read_kmer_file(f, 8)
    assert given == ["ACGTACGT", "acgtTTTT", "GGGGCCCC"]                               # written back as given; case folded for the hash
    assert kh.dtype == np.uint32
    assert kh.tolist() == [int(kmer2hash(s)) for s in ("ACGTACGT", "ACGTTTTT", "GGGGCCCC")]
    f.write_text("ACGTACGTACGTACGT\nTTTTTTTTTTTTTTTT\n")
    given, kh = read_kmer_file(f, 16)
    assert kh.dtype == np.uint64 and kh.tolist() == [int(kmer2hash("ACGTACGTACGTACGT")), 4 ** 16 - 1]
    f.write_text("\n\n")
    given, kh = read_kmer_file(f, 8)
    assert given == [] and len(kh) == 0


@pytest.mark.parametrize("text,lineno,what", [("ACGTACGT\n\nACGTACG\n", 3, "bases"), ("ACGTACGT\nACGTACGTA\n", 2, "bases"),
                                              ("\nACGTACGT\nACGTNCGT\n", 3, "outside ACGT"), ("ACGUACGT\n", 1, "outside ACGT"),
                                              ("ACGTACGÄ\n", 1, "outside ACGT")])
def test_kmer_file_parser_rejects(tmp_path, text, lineno, what):
    from kmap_amd.projection import read_kmer_file
    f = tmp_path / "q.txt"
    f.write_text(text, encoding="utf-8")
    with pytest.raises(ValueError, match=rf"q\.txt:{lineno}: .*{what}"):
        read_kmer_file(f, 8)


def _fake_res_dir(tmp, n_rows=None, labels=None):
    """a result directory as far as project_kmers reads it: config.toml, sample_kmers.pkl, low_dim_data.tsv"""
    from kmap_amd._toml import dump_toml
    from kmap_amd.kmer_count import kmer2hash, read_default_config_file
    res = tmp / "res"
    res.mkdir(parents=True)
    dump_toml(read_default_config_file(), res / "config.toml")
    samp_kh = np.array(sorted(int(kmer2hash(s)) for s in ("ACGTACGT", "ACGTACGA", "TTTTACGT")), np.uint32)
    samp_cnts = np.array([2, 1, 3])
    samp_label = np.array([0, 0, 1])
    with open(res / "sample_kmers.pkl", "wb") as fh:
        pickle.dump([samp_kh, samp_cnts, samp_label, ["ACGTACGT"]], fh)
    want_labels = np.repeat(samp_label, samp_cnts).tolist()
    labels = want_labels if labels is None else labels
    n_rows = len(want_labels) if n_rows is None else n_rows
    with open(res / "low_dim_data.tsv", "w") as fh:
        fh.write("x\ty\tlabel\n" + "".join(f"{0.5 * i:3.3f}\t{-0.25 * i:3.3f}\t{labels[i % len(labels)]}\n" for i in range(n_rows)))
    return res


@pytest.mark.parametrize("bad,lineno", [("ACGTACGT\nACGTAC\n", 2), ("acgtacgt\n\nACGTACGX\n", 3)])
def test_bad_kmer_file_writes_nothing(tmp_path, bad, lineno):
    """the k-mer file is validated before the device is touched and before any output exists"""
    from kmap_amd.projection import _project_kmers
    res = _fake_res_dir(tmp_path)
    before = sorted(p.name for p in res.iterdir())
    q = tmp_path / "q.txt"
    q.write_text(bad)
    out = tmp_path / "out.tsv"
    for output_file in (None, str(out)):
        with pytest.raises(ValueError, match=rf"q\.txt:{lineno}:"):
            _project_kmers(str(res), str(q), output_file, 10)
    assert not out.exists() and sorted(p.name for p in res.iterdir()) == before


def test_anchor_file_must_match_the_sample(tmp_path):
    from kmap_amd.projection import _project_kmers, read_anchors
    q = tmp_path / "q.txt"
    q.write_text("ACGTACGT\n")
    res = _fake_res_dir(tmp_path / "a", n_rows=5)
    with pytest.raises(ValueError, match=r"low_dim_data\.tsv: 5 points, sample_kmers\.pkl has 6"):
        _project_kmers(str(res), str(q), None, 10)
    res = _fake_res_dir(tmp_path / "b", labels=[0, 0, 0, 1, 1, 0])
    with pytest.raises(ValueError, match=r"low_dim_data\.tsv: labels differ"):
        _project_kmers(str(res), str(q), None, 10)
    assert not (res / "projected_kmers.tsv").exists()
    res = _fake_res_dir(tmp_path / "c")
    xy = read_anchors(res, 6, [0, 0, 0, 1, 1, 1])
    assert xy.dtype == np.float32 and xy.shape == (2, 6)
    np.testing.assert_array_equal(xy, np.array([[0.5 * i for i in range(6)], [-0.25 * i for i in range(6)]], np.float32))


def test_only_rank_zero_projects(tmp_path, monkeypatch):
    """under a torch.distributed launch the other ranks return before they read or write anything"""
    from kmap_amd.projection import _project_kmers
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "1")
    assert _project_kmers(str(tmp_path / "no_such_dir"), str(tmp_path / "no_such_file"), None, 10) is None
    monkeypatch.setenv("RANK", "0")
    with pytest.raises(ValueError, match="config.toml is missing"):
        _project_kmers(str(tmp_path / "no_such_dir"), str(tmp_path / "no_such_file"), None, 10)
    assert list(tmp_path.iterdir()) == []


def test_cli_lists_project_kmers():
    from click.testing import CliRunner
    from kmap_amd.cli import cli
    r = CliRunner().invoke(cli, ["--help"])
    assert r.exit_code == 0 and "project_kmers" in r.output
    r = CliRunner().invoke(cli, ["project_kmers", "--help"])
    assert r.exit_code == 0
    for opt in ("--res_dir", "--kmer_file", "--output_file", "--n_iter"):
        assert opt in r.output
    r = CliRunner().invoke(cli, ["project_kmers", "--kmer_file", "x"])
    assert r.exit_code != 0 and "--res_dir" in r.output                              # required


def test_project_symbols_are_registered():
    from kmap_amd import _ffi
    header = (ROOT / "include" / "kmap_hip.h").read_text()
    declared = set(re.findall(r"\b(kmap_project_[A-Za-z0-9_]+)\s*\(", header))
    assert declared == {"kmap_project_knn_u32_dev", "kmap_project_knn_u64_dev", "kmap_project_prob_dev", "kmap_project_descend_dev"}
    assert declared <= set(_ffi.exported_symbols())
    for name in declared:
        res, args = _ffi._SIGS[name]
        proto = re.search(rf"int {name}\s*\(([^;]*)\);", header).group(1)
        assert len(args) == proto.count(",") + 1, name                               # one ctypes argument per C parameter
