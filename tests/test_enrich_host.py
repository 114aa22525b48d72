"""Host side of enrich_kmers (no GPU): the z / fold functions against exact rational arithmetic, the three writers byte for byte,
every argument error (raised before the library is loaded) and the CLI verb.  The definitions are DESIGN.md section 12."""
import math
import subprocess
import sys
from decimal import Decimal, getcontext
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent


def exact_z(a, b, Nf, Nb):
    """D / sqrt(s) from exact rationals, rounded to float once (60 decimal digits in between)"""
    if Nf + Nb == 0:
        return 0.0
    D = a * Nb - b * Nf
    s = Fraction((a + b) * (Nf + Nb - a - b) * Nf * Nb, Nf + Nb)
    if s <= 0:
        return 0.0
    getcontext().prec = 60
    return float(Decimal(D) / (Decimal(s.numerator) / Decimal(s.denominator)).sqrt())


def test_z_against_fractions():
    from kmap_amd.enrichment import enrich_z
    rng = np.random.default_rng(5)
    cases = [(579, 4, 106335, 106407), (0, 0, 10, 10), (5, 0, 5, 0), (3, 3, 100, 100), (1, 7, 1000, 900),
             (2 ** 32 - 1, 2 ** 33 - 2, 2 ** 52 - 1, 2 ** 52 - 1), (2 ** 32 - 1, 0, 2 ** 52 - 1, 2 ** 52 - 1), (0, 0, 0, 0), (4, 4, 4, 4)]
    for _ in range(300):
        Nf, Nb = int(rng.integers(1, 2 ** 40)), int(rng.integers(1, 2 ** 40))
        cases.append((int(rng.integers(0, min(Nf, 2 ** 32))), int(rng.integers(0, min(Nb, 2 ** 33))), Nf, Nb))
    for a, b, Nf, Nb in cases:
        got, want = enrich_z(a, b, Nf, Nb), exact_z(a, b, Nf, Nb)
        assert not math.isnan(got)
        # six roundings of 2^-53 reach z: 16 leaves a margin
        assert abs(got - want) <= 16 * 2.0 ** -53 * abs(want), (a, b, Nf, Nb, got, want)
    assert enrich_z(3, 3, 100, 100) == 0.0 and math.copysign(1.0, enrich_z(3, 3, 100, 100)) == 1.0
    assert enrich_z(5, 0, 5, 0) == 0.0            # empty control
    assert enrich_z(4, 4, 4, 4) == 0.0            # every window is this k-mer
    assert enrich_z(1, 7, 1000, 900) < 0


def test_log2_fold():
    from kmap_amd.enrichment import log2_fold
    for a, b, Nf, Nb, pc in [(579, 4, 106335, 106407, 1.0), (0, 0, 10, 20, 0.5), (7, 0, 100, 0, 1.0), (1, 1, 2, 2, 0.0)]:
        want = math.log2((a + pc) / (Nf + pc)) - math.log2((b + pc) / (Nb + pc))
        assert log2_fold(a, b, Nf, Nb, pc) == want
    assert log2_fold(0, 3, 10, 10, 0.0) == -math.inf
    assert math.isnan(log2_fold(0, 0, 0, 0, 0.0))


def test_kmer_table_bytes(tmp_path):
    from kmap_amd.enrichment import write_kmer_table
    kh = np.array([3427, 0, 65535], np.uint64)            # AATCCGAT (the lower strand of ATCGGATT), AAAAAAAA, TTTTTTTT
    a, b = np.array([579, 3, 2], np.int64), np.array([4, 0, 9], np.int64)
    z = np.array([23.8512345678, 0.0, -2.5], np.float64)
    write_kmer_table(tmp_path / "t.tsv", 8, kh, a, b, z, 106335, 106407, 1.0)
    want = ("rank\tkmer\trevcom_kmer\tfg_count\tcontrol_count\tfg_share\tcontrol_share\tlog2_fold\tz\n"
            "1\tAATCCGAT\tATCGGATT\t579\t4\t5.445056e-03\t3.759151e-05\t6.85896\t23.8512\n"
            "2\tAAAAAAAA\tTTTTTTTT\t3\t0\t2.821272e-05\t0.000000e+00\t2.00098\t0\n"
            "3\tTTTTTTTT\tAAAAAAAA\t2\t9\t1.880848e-05\t8.458090e-05\t-1.73599\t-2.5\n")
    assert (tmp_path / "t.tsv").read_text() == want
    write_kmer_table(tmp_path / "e.tsv", 8, kh[:0], a[:0], b[:0], z[:0], 0, 0, 1.0)
    assert (tmp_path / "e.tsv").read_text() == want.split("\n")[0] + "\n"


def test_info_and_motif_table_bytes(tmp_path):
    from kmap_amd.enrichment import motif_row, write_info_table, write_motif_table
    from kmap_amd.kmer_count import MotifDef
    write_info_table(tmp_path / "i.csv", [dict(k=8, dedupe=True, revcom=True, n_fg_uniq=31323, n_control_uniq=52591, Nf=106335, Nb=106407,
                                               min_count=2, n_eligible=20000, n_written=50)])
    assert (tmp_path / "i.csv").read_text() == ("k,dedupe,revcom,n_fg_uniq,n_control_uniq,Nf,Nb,min_count,n_eligible,n_written\n"
                                                "8,1,1,31323,52591,106335,106407,2,20000,50\n")
    d = MotifDef(8, 0.0125, 1, 1.0, 0.1, 2.0)
    lines = [motif_row("ATCGGATT", d, 700, 50, 106335, 106407, 1.0), motif_row("A" * 40, None, 0, 0, 0, 0)]
    write_motif_table(tmp_path / "m.csv", lines)
    want = ("conseq,k,max_ham_dist,fg_mass,control_mass,Nf,Nb,fg_share,control_share,fg_ratio,control_ratio,log2_fold,z\n"
            "ATCGGATT,8,1,700,50,106335,106407,6.582969e-03,4.698939e-04,0.526638,0.0375915,3.78182,23.7859\n"
            + "A" * 40 + ",40,,,,,,,,,,,\n")
    assert (tmp_path / "m.csv").read_text() == want


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
    from kmap_amd import _ffi
    from kmap_amd.enrichment import _enrich_kmers
    from kmap_amd.kmer_count import FileNameDict

    def no_lib():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_ffi, "lib", no_lib)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    res, ctl = res_dir
    out = tmp_path / "out"
    ok = dict(kmer_len=[8], top_n=10, min_count=2, pseudocount=1.0, conseq_file=None, output_dir=out)
    bad = [(dict(), tmp_path / "nowhere", ctl, "config.toml"),
           (dict(), res, tmp_path / "missing.fa", "control"),
           (dict(kmer_len=[0]), res, ctl, "kmer_len"),
           (dict(kmer_len=[8, 32]), res, ctl, "kmer_len"),
           (dict(top_n=0), res, ctl, "top_n"),
           (dict(min_count=0), res, ctl, "min_count"),
           (dict(pseudocount=float("nan")), res, ctl, "pseudocount"),
           (dict(pseudocount=-1.0), res, ctl, "pseudocount"),
           (dict(conseq_file=tmp_path / "no_conseq.txt"), res, ctl, "consensus"),
           (dict(kmer_len=[]), res, ctl, "nothing to do")]
    for change, r, c, word in bad:
        with pytest.raises(ValueError, match=word):
            _enrich_kmers(r, c, **{**ok, **change})
    cons = tmp_path / "cons.txt"
    cons.write_text("ACGTN\n")
    with pytest.raises(ValueError, match="letters"):
        _enrich_kmers(res, ctl, **{**ok, "conseq_file": cons})
    assert not out.exists()
    # with valid arguments the library is what comes next
    with pytest.raises(AssertionError, match="the library was loaded"):
        _enrich_kmers(res, ctl, **ok)
    assert not out.exists()
    (res / FileNameDict["processed_fasta_file"]).unlink()
    with pytest.raises(ValueError, match="input.bin.pkl"):
        _enrich_kmers(res, ctl, **ok)


def test_other_ranks_do_nothing(res_dir, monkeypatch):
    from kmap_amd.enrichment import _enrich_kmers
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "1")
    assert _enrich_kmers("nowhere", "missing.fa", [0]) is None


def test_cli_lists_the_options():
    r = subprocess.run([sys.executable, "-m", "kmap_amd", "enrich_kmers", "--help"], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    for opt in ("--res_dir", "--control_fasta_file", "--kmer_len", "--top_n", "--min_count", "--pseudocount", "--conseq_file", "--output_dir"):
        assert opt in r.stdout, opt
    r = subprocess.run([sys.executable, "-m", "kmap_amd", "--help"], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert "enrich_kmers" in r.stdout


def test_symbols_registered():
    from kmap_amd import _ffi
    header = (ROOT / "include" / "kmap_hip.h").read_text()
    for name in ("create", "destroy", "set_control", "run", "result_dev", "select", "fetch"):
        assert f"kmap_enrich_{name}" in _ffi.exported_symbols() and f"kmap_enrich_{name}(" in header
