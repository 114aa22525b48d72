"""Host side of motif_centrality (no GPU): c(L, w, a) against the enumeration of windows, E, V and z against exact fractions on
hand-made histograms of mixed lengths, the tie rule, the candidate count, Bonferroni and the nan cases of the best region, the verb's
files with the device pass replaced by the numpy model of tests/_sites_model.py on seeded reads with one motif planted at the centre
and one planted uniformly, its argument errors (raised before the library is loaded or a directory made), the library's entry and the
CLI verb.  The definitions are DESIGN.md section 18."""
import math
import re
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

from tests import _readscore_model as M
from tests import _sites_model as S

ROOT = Path(__file__).resolve().parent.parent
LIB = ROOT / "tests" / "golden" / "library"


# ---- 1. the null ----------------------------------------------------------------------------------------------------------------------
def test_windows_within_against_enumeration():
    from kmap_amd.centrality import windows_within
    for w in range(1, 41):
        for L in range(w, 41):
            d = [2 * loc + w - L for loc in range(L - w + 1)]
            assert min(d) == -(L - w) and max(d) == L - w and all((x - (L - w)) % 2 == 0 for x in d)
            for a in range(46):
                assert windows_within(L, w, a) == sum(abs(x) <= a for x in d), (L, w, a)
    for L, w, a in ((7, 8, 0), (9, 8, -1)):
        with pytest.raises(ValueError):
            windows_within(L, w, a)


def hand_made(w=8):
    """(D, Hlen, sites): reads of lengths 8 (one window), 9, 20, 21 and 50 with sites at chosen offsets; max_len 60"""
    sites = {8: [0, 0, 0], 9: [-1, 1, 1, 1, -1], 20: [0, 0, 2, -2, 12, -12, 4], 21: [1, -1, 1, 1, 3, -13, 13, 5, -5, 1, -1],
             50: [0, 2, -42, 42]}
    max_len = 60
    D, Hlen = np.zeros(2 * max_len + 1, np.int64), np.zeros(max_len + 1, np.int64)
    for L, ds in sites.items():
        for d in ds:
            assert abs(d) <= L - w and (d - (L - w)) % 2 == 0
            D[d + max_len] += 1
            Hlen[L] += 1
    return D, Hlen, sites


def exact_curve(sites, w, a):
    """(k, E, V) of section 18 in exact fractions, by enumeration of every read's windows"""
    k, E, V = 0, Fraction(0), Fraction(0)
    for L, ds in sites.items():
        inside = sum(abs(2 * loc + w - L) <= a for loc in range(L - w + 1))
        q = Fraction(inside, L - w + 1)
        k += sum(abs(d) <= a for d in ds)
        E += len(ds) * q
        V += len(ds) * q * (1 - q)
    return k, E, V


def test_mean_variance_z_against_fractions():
    """the sums have at most max_len terms of doubles: rtol 1e-9 is far above their rounding"""
    from kmap_amd.centrality import best_region, region_curve, sites_within
    w = 8
    D, Hlen, sites = hand_made(w)
    k, E, V = region_curve(D, Hlen, w)
    assert len(k) == len(E) == len(V) == 50 - w + 1 and k.dtype == np.int64
    zs = {}
    for a in range(len(k)):
        ke, Ee, Ve = exact_curve(sites, w, a)
        assert int(k[a]) == ke == sites_within(D, a)
        assert E[a] == pytest.approx(float(Ee), rel=1e-9) and V[a] == pytest.approx(float(Ve), rel=1e-9, abs=1e-300)
        assert (V[a] > 0) == (Ve > 0)
        if Ve > 0:
            zs[a] = (ke - float(Ee)) / math.sqrt(float(Ve))
    assert V[-1] == 0 and sites_within(D, 1000) == int(Hlen.sum()) == 30     # every window of every read: no variance left
    for min_half in (0, 3, 20):
        st = best_region(D, Hlen, w, min_half=min_half, min_sites=10)
        cand = {a: z for a, z in zs.items() if a >= min_half}
        a_best = min(a for a, z in cand.items() if z >= max(cand.values()) * (1 - 1e-12))
        assert st["half_width_x2"] == a_best and st["n_regions"] == len(cand) and st["n_sites"] == 30
        assert st["z"] == pytest.approx(cand[a_best], rel=1e-9)
        ke, Ee, Ve = exact_curve(sites, w, a_best)
        assert st["sites_in_region"] == ke and st["expected_in_region"] == pytest.approx(float(Ee), rel=1e-9)
        assert st["variance"] == pytest.approx(float(Ve), rel=1e-9)
    with pytest.raises(ValueError, match="width"):
        region_curve(D, Hlen, 9)                             # a site read of 8 bases under 9 columns
    bad = D.copy()
    bad[0] = 1
    with pytest.raises(ValueError, match="outside"):
        region_curve(bad, Hlen, w)


def one_length(L, w, offsets, max_len=None):
    max_len = L if max_len is None else max_len
    D, Hlen = np.zeros(2 * max_len + 1, np.int64), np.zeros(max_len + 1, np.int64)
    for d in offsets:
        D[d + max_len] += 1
    Hlen[L] = len(offsets)
    return D, Hlen


def test_best_region_ties_candidates_bonferroni_and_nan():
    from kmap_amd.centrality import best_region
    from kmap_amd.library import log10_p_of_z
    # m = L - w = 20 is even: the offsets are even, so an odd a holds the windows of a - 1 -- k, E, V and z are the same doubles,
    # and the smaller a wins.  All 12 sites at d = 0, +-2: the best region is a = 2 and a = 3 ties with it.
    D, Hlen = one_length(30, 10, [0] * 6 + [2] * 3 + [-2] * 3)
    st = best_region(D, Hlen, 10)
    assert st["half_width_x2"] == 2 and st["sites_in_region"] == 12 and st["n_sites"] == 12
    assert st["expected_in_region"] == pytest.approx(12 * 3 / 21, rel=1e-12)
    assert st["z"] == pytest.approx((12 - 12 * 3 / 21) / math.sqrt(12 * (3 / 21) * (18 / 21)), rel=1e-12)
    assert st["n_regions"] == 20                             # a = 0 .. 19; at a = 20 every window is inside: V = 0
    assert st["log10_p"] == log10_p_of_z(st["z"]) and st["log10_p_adj"] == min(0.0, st["log10_p"] + math.log10(20))
    tie = best_region(D, Hlen, 10, min_half=3)               # a = 3 is now the smallest candidate of the tie
    assert tie["half_width_x2"] == 3 and tie["z"] == st["z"] and tie["n_regions"] == 17
    assert tie["log10_p_adj"] == min(0.0, st["log10_p"] + math.log10(17))
    # m = 21 is odd: no window has |d| <= 0, q = 0 and a = 0 is no candidate
    D, Hlen = one_length(31, 10, [1] * 6 + [-1] * 6)
    st = best_region(D, Hlen, 10)
    assert st["half_width_x2"] == 1 and st["n_regions"] == 20 and st["z"] == pytest.approx((12 - 12 * 2 / 22) / math.sqrt(12 * (2 / 22) * (20 / 22)), rel=1e-12)
    # a weak z: Bonferroni stops at p = 1
    D, Hlen = one_length(30, 10, list(range(-20, 21, 2)))
    st = best_region(D, Hlen, 10)
    assert st["log10_p"] < 0 and st["log10_p_adj"] == 0.0
    # fewer than min_sites, or no candidate (every site read has one window, or min_half past the last one): nan z, p = 1
    D, Hlen = one_length(30, 10, [0] * 9)
    for st, regions in ((best_region(D, Hlen, 10), 20), (best_region(D, Hlen, 10, min_sites=9, min_half=20), 0),
                        (best_region(*one_length(10, 10, [0] * 40), 10), 0), (best_region(*one_length(30, 10, []), 10), 0)):
        assert st["z"] != st["z"] and st["half_width_x2"] is None and st["sites_in_region"] is None
        assert st["log10_p"] == 0.0 and st["log10_p_adj"] == 0.0 and st["n_regions"] == regions
    assert best_region(D, Hlen, 10, min_sites=9)["half_width_x2"] == 0
    for kw in (dict(min_half=-1), dict(min_sites=0), dict(min_half=1.5)):
        with pytest.raises(ValueError, match="min_"):
            best_region(D, Hlen, 10, **kw)


# ---- 2. the verb on the numpy model ---------------------------------------------------------------------------------------------------
@pytest.fixture
def planted(tmp_path, monkeypatch):
    """the seeded reads of tests/_sites_model.py as a result directory and a control FASTA; the device replaced by its model"""
    import kmap_amd.kmer_count as K
    import kmap_amd.motif_discovery as D
    made = S.write_planted(tmp_path)
    monkeypatch.setattr(D, "DeviceSeq", S.ModelSeq)
    monkeypatch.setattr(K, "encode_fasta", lambda path: M.encode_fasta_np(path))
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    S.ModelSeq.calls = []
    return made


INT, BITS, HALF = re.compile(r"-?\d+"), re.compile(r"-?\d+\.\d\d"), re.compile(r"\d+\.\d")
FORMATS = dict(rank=INT, width=INT, threshold=INT, threshold_bits=BITS, n_sites=INT, half_width_x2=INT, half_width_bases=HALF,
               sites_in_region=INT, n_regions=INT, control_sites=INT, control_in_region=INT)
FLOATS = ("expected_in_region", "z", "log10_p", "log10_p_adj", "q_bh", "z_vs_control")


def check_table(path, results, control):
    from kmap_amd import centrality as C
    table = path.read_text().split("\n")
    cols = table[0].split(",")
    assert table[0] == ("rank,name,altname,source,width,consensus,threshold,threshold_bits,n_sites,half_width_x2,half_width_bases,"
                        "sites_in_region,expected_in_region,z,log10_p,n_regions,log10_p_adj,q_bh"
                        + (",control_sites,control_in_region,z_vs_control" if control else ""))
    assert table[-1] == "" and len(table) == 2 + len(results)
    rows = [dict(zip(cols, line.split(","))) for line in table[1:-1]]
    for rank, (row, st) in enumerate(zip(rows, results)):
        assert len(row) == len(cols) and row["rank"] == str(rank) == str(st["rank"])
        for name, pattern in FORMATS.items():
            if name in row:
                assert pattern.fullmatch(row[name]), (name, row[name])
        for name in FLOATS:
            if name in row:
                assert repr(float(row[name])) == row[name], (name, row[name])
        m = st["motif"]
        assert (row["name"], row["altname"], row["source"], int(row["width"])) == (m.name, m.altname, m.source, m.counts.shape[1])
        assert int(row["threshold"]) == st["threshold"] and row["threshold_bits"] == "%.2f" % (st["threshold"] / 100)
        assert int(row["half_width_x2"]) == st["half_width_x2"] and row["half_width_bases"] == "%.1f" % (st["half_width_x2"] / 2)
        assert int(row["n_sites"]) == st["n_sites"] and int(row["sites_in_region"]) == st["sites_in_region"]
        assert float(row["z"]) == st["z"] and float(row["q_bh"]) == st["q_bh"] and float(row["log10_p_adj"]) == st["log10_p_adj"]
        assert C.rank_line(rank, m, st["threshold"], st, control) == table[1 + rank] + "\n"
    z = [float(r["z"]) for r in rows]
    assert z == sorted(z, reverse=True)
    return rows


def test_verb_on_planted_reads(planted, tmp_path, capsys):
    """The model ranks the centred motif first (seed fixed after checking that on the CPU): q_bh < 0.01 in a region of at most 6
    bases; the uniformly planted one is not central."""
    from kmap_amd import centrality as C
    from kmap_amd.enrichment import enrich_z
    from kmap_amd.library import bh_qvalues, read_motif_library
    from kmap_amd.pwm import pwm_threshold, pwm_weights
    res, ctl, seq, borders, cseq, cborders = planted
    out = tmp_path / "out"
    lib = str(LIB / "three.meme")
    results = C._motif_centrality(str(res), [lib], output_dir=str(out), top_hist=1)
    printed = capsys.readouterr().out
    assert S.ModelSeq.calls == [(2, True, None)]             # one call for the whole library, no control
    assert [st["motif"].name for st in results] == ["M1_CAATCGATAGC", "M2_ACCTACGTA"]
    centred, uniform = results
    assert centred["q_bh"] < 0.01 and centred["half_width_x2"] <= 12 and centred["n_sites"] >= 300
    assert uniform["q_bh"] > 0.05 and uniform["n_sites"] >= 300
    # every figure again, from the model and the definitions
    motifs = [m for m in read_motif_library(lib) if m.skip is None]
    want = []
    for m in motifs:
        W = pwm_weights(m.counts, 1.0)
        t = pwm_threshold(W, 1e-4)[0]
        D, Hlen, n, too_long = S.np_sites(seq, borders, W, t, True, 100)
        st = C.best_region(D, Hlen, W.shape[1])
        assert too_long == 0 and n == st["n_sites"] == int(D.sum())
        want.append((m.name, t, D, st))
    q = bh_qvalues([10.0 ** st["log10_p_adj"] for _, _, _, st in want])
    for (name, t, D, st), qi, got in zip(want, q.tolist(), results):
        assert got["motif"].name == name and got["threshold"] == t and got["q_bh"] == qi
        np.testing.assert_array_equal(got["D"], D)
        for key in ("n_sites", "n_regions", "half_width_x2", "sites_in_region", "expected_in_region", "z", "log10_p", "log10_p_adj"):
            assert got[key] == st[key], key
    check_table(out / "centrality_rank.csv", results, False)
    assert (out / "skipped.csv").read_text() == f"name,altname,source,reason\nM3_long,too_wide,{lib},width 40 outside 4..31\n"
    assert sorted(p.name for p in out.iterdir()) == ["centrality_rank.csv", "site_offsets_0_M1_CAATCGATAGC.csv", "skipped.csv"]
    offsets = (out / "site_offsets_0_M1_CAATCGATAGC.csv").read_text().split("\n")
    D = centred["D"]
    assert offsets[0] == "offset_x2,fg_sites" and offsets[-1] == ""
    assert offsets[1:-1] == [f"{i - 100},{int(D[i])}" for i in np.nonzero(D)[0]]
    assert all(int(line.split(",")[0]) % 2 == 1 for line in offsets[1:-1])       # 100 - 11 is odd
    assert printed.count("\n") == 3 and printed.startswith("0 M1_CAATCGATAGC planted_a: at ")
    assert f"motif_centrality: 2 motifs ranked, 1 skipped, both strands: {out}" in printed

    # with a control, the forward strand, a threshold in bits, the default directory and all histograms
    S.ModelSeq.calls = []
    with_ctl = C._motif_centrality(str(res), [lib], str(ctl), min_score=9.0, revcom_mode=False, min_half=2)
    assert S.ModelSeq.calls == [(2, False, None), (2, False, None)]
    out2 = res / "motif_centrality"
    rows = check_table(out2 / "centrality_rank.csv", with_ctl, True)
    assert sorted(p.name for p in out2.iterdir()) == ["centrality_rank.csv", "site_offsets_0_M1_CAATCGATAGC.csv",
                                                      "site_offsets_1_M2_ACCTACGTA.csv", "skipped.csv"]
    for st, row, m in zip(with_ctl, rows, motifs):
        W = pwm_weights(m.counts, 1.0)
        assert st["threshold"] == 900 and row["threshold_bits"] == "9.00" and st["half_width_x2"] >= 2
        Dc, _, nc, _ = S.np_sites(cseq, cborders, W, 900, False, 100)
        kc = int(Dc[100 - st["half_width_x2"]:100 + st["half_width_x2"] + 1].sum())
        assert (st["control_sites"], st["control_in_region"]) == (nc, kc) == (int(row["control_sites"]), int(row["control_in_region"]))
        assert st["z_vs_control"] == enrich_z(st["sites_in_region"], kc, st["n_sites"], nc) == float(row["z_vs_control"])
        lines = (out2 / f"site_offsets_{st['rank']}_{m.name}.csv").read_text().split("\n")
        assert lines[0] == "offset_x2,fg_sites,control_sites"
        both = np.nonzero((st["D"] != 0) | (Dc != 0))[0]
        assert lines[1:-1] == [f"{i - 100},{int(st['D'][i])},{int(Dc[i])}" for i in both]
    assert with_ctl[0]["z_vs_control"] > 3                   # random reads have their chance sites anywhere
    # a second run writes the same bytes
    C._motif_centrality(str(res), [lib], str(ctl), min_score=9.0, revcom_mode=False, min_half=2, output_dir=str(tmp_path / "again"))
    for p in out2.iterdir():
        assert (tmp_path / "again" / p.name).read_bytes() == p.read_bytes()


def test_no_region_rows_rank_last(planted, tmp_path):
    """a threshold no window reaches: no site, nan z, p = 1, q = 1, empty region fields, ranked by name"""
    from kmap_amd import centrality as C
    res = planted[0]
    results = C._motif_centrality(str(res), [str(LIB / "three.meme")], min_score=60.0, output_dir=str(tmp_path / "o"))
    assert [st["motif"].name for st in results] == ["M1_CAATCGATAGC", "M2_ACCTACGTA"]
    assert all(st["n_sites"] == 0 and st["z"] != st["z"] and st["q_bh"] == 1.0 for st in results)
    lines = (tmp_path / "o" / "centrality_rank.csv").read_text().split("\n")[1:3]
    assert all(line.endswith(",6000,60.00,0,,,,,nan,0.0,0,0.0,1.0") for line in lines)
    assert (tmp_path / "o" / "site_offsets_0_M1_CAATCGATAGC.csv").read_text() == "offset_x2,fg_sites\n"


def test_value_errors_come_before_the_library(planted, tmp_path, monkeypatch):
    import kmap_amd.motif_discovery as D
    from kmap_amd import _ffi
    from kmap_amd import centrality as C

    def no_lib():
        raise AssertionError("the library was loaded before the arguments were checked")

    class NoSeq:
        def __init__(self, *a):
            no_lib()
    monkeypatch.setattr(_ffi, "lib", no_lib)
    monkeypatch.setattr(D, "DeviceSeq", NoSeq)
    res, ctl = planted[:2]
    out = tmp_path / "out"
    only_wide = tmp_path / "wide.meme"
    only_wide.write_text("MEME version 4\n\nMOTIF W\nletter-probability matrix: alength= 4 w= 32\n" + "0.25 0.25 0.25 0.25\n" * 32)
    zero = tmp_path / "zero.csv"
    zero.write_text("1,2,3,0\n1,2,3,4\n1,2,3,4\n1,2,3,4\n")
    ok = dict(library_files=[str(LIB / "three.meme")], output_dir=out)
    bad = [(dict(res_dir=tmp_path / "nowhere"), "config.toml"),
           (dict(control_fasta_file=tmp_path / "missing.fa"), "control"),
           (dict(library_files=[]), "no library file"),
           (dict(library_files=[str(tmp_path / "nowhere.meme")]), "nowhere.meme"),
           (dict(library_files=[str(LIB / "three.meme"), str(LIB / "bad_alength.meme")]), "bad_alength.meme:11"),
           (dict(library_files=[str(only_wide)]), "none of the 1 motifs.*W: width 32"),
           (dict(library_files=[str(zero)], pseudocount=0.0), "zero.csv: motif zero: .*pseudocount"),
           (dict(pseudocount=-1.0), "pseudocount"),
           (dict(p_value=float("nan")), "p_value"),
           (dict(min_score=float("inf")), "min_score"),
           (dict(nsites_default=0), "nsites_default"),
           (dict(min_half=-1), "min_half"),
           (dict(min_sites=0), "min_sites"),
           (dict(top_hist=-1), "top_hist")]
    for change, word in bad:
        with pytest.raises(ValueError, match=word):
            C._motif_centrality(**{"res_dir": res, **ok, **change})
    assert not out.exists() and not (res / "motif_centrality").exists()
    with pytest.raises(AssertionError, match="the library was loaded"):
        C._motif_centrality(res, **ok)
    assert not out.exists()


def test_too_long_site_reads_are_an_error(planted, tmp_path, monkeypatch):
    from kmap_amd import centrality as C
    monkeypatch.setattr(S.ModelSeq, "library_sites", lambda self, Ws, ts, revcom, max_len=None:
                        S.np_library_sites(self.seq, self.borders, Ws, ts, revcom, 50))
    with pytest.raises(ValueError, match="M1_CAATCGATAGC.*longer"):
        C._motif_centrality(planted[0], [str(LIB / "three.meme")], output_dir=tmp_path / "o")
    assert not (tmp_path / "o").exists()


def test_other_ranks_do_nothing(monkeypatch):
    from kmap_amd.centrality import _motif_centrality
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "1")
    assert _motif_centrality("nowhere", []) is None


# ---- 3. the library's entry -----------------------------------------------------------------------------------------------------------
def test_symbol_registered_and_constants():
    from kmap_amd import _ffi, device_seq
    header = (ROOT / "include" / "kmap_hip.h").read_text()
    name = "kmap_readscore_sites_library_dev"
    assert name in _ffi.exported_symbols() and f"int {name}(" in header
    res, args = _ffi._SIGS[name]
    assert res is _ffi.i32 and len(args) == 16
    assert not name.startswith("kmap_pwm_")
    src = (ROOT / "kmap_amd" / "csrc" / "pwm_sites.hip").read_text()
    batch = (ROOT / "kmap_amd" / "csrc" / "pwm_batch.h").read_text()
    assert int(re.search(r"constexpr int PB_MAX_MAT = (\d+);", batch).group(1)) == device_seq.LIBRARY_BATCH
    assert int(re.search(r"constexpr int PB_MAX_CHUNKS = (\d+);", batch).group(1)) == device_seq.LIBRARY_BATCH_CHUNKS
    assert 1 << int(re.search(r"constexpr int64_t ST_MAX_LEN = 1ll << (\d+);", src).group(1)) == device_seq.SITES_MAX_LEN


def test_library_sites_checks_come_before_the_library(monkeypatch):
    from kmap_amd import _ffi
    from kmap_amd.device_seq import DeviceSeq

    def no_lib():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_ffi, "lib", no_lib)
    ds = object.__new__(DeviceSeq)
    ds.n_seq, ds.read_len = 2, np.array([5, 2 ** 20 + 1], np.int64)
    ok = np.zeros((4, 8), np.int32)
    for Ws, ts, max_len, word in (([np.zeros((4, 3), np.int32)], [0], 10, "width 3"),
                                  ([ok, np.zeros((4, 32), np.int32)], [0, 0], 10, "matrix 1 has width 32"),
                                  ([np.zeros((3, 8), np.int32)], [0], 10, "shape"), ([ok], [2 ** 31], 10, "int32"),
                                  ([ok], [0, 1], 10, "1 matrices, 2 thresholds"), ([ok], [0], -1, "max_len -1"),
                                  ([ok], [0], 2 ** 20 + 1, "max_len 1048577"), ([ok], [0], 2.5, "max_len 2.5"),
                                  ([ok], [0], None, "longest read has 1048577")):
        with pytest.raises(ValueError, match="library_sites: .*" + word):
            ds.library_sites(Ws, ts, True, max_len)


# ---- 4. the verb's command line -------------------------------------------------------------------------------------------------------
def test_cli_options_and_defaults(monkeypatch):
    from click.testing import CliRunner
    from kmap_amd import centrality
    from kmap_amd.cli import cli
    calls = []
    monkeypatch.setattr(centrality, "_motif_centrality", lambda *a: calls.append(a))
    runner = CliRunner()
    r = runner.invoke(cli, ["motif_centrality", "--res_dir", "D", "--library_file", "L"])
    assert r.exit_code == 0, r.output
    assert calls[-1] == ("D", ["L"], None, 1e-4, None, 1.0, 20, None, 0, 10, 5, None)
    r = runner.invoke(cli, ["motif_centrality", "--res_dir", "D", "--library_file", "L", "--library_file", "L2", "--control_fasta_file", "C.fa",
                            "--p_value", "1e-3", "--min_score", "8.5", "--pseudocount", "0.5", "--nsites_default", "100",
                            "--revcom_mode", "False", "--min_half", "4", "--min_sites", "3", "--top_hist", "0", "--output_dir", "O"])
    assert r.exit_code == 0, r.output
    assert calls[-1] == ("D", ["L", "L2"], "C.fa", 1e-3, 8.5, 0.5, 100, False, 4, 3, 0, "O")
    for missing in (["--library_file", "L"], ["--res_dir", "D"]):
        assert runner.invoke(cli, ["motif_centrality"] + missing).exit_code == 2
    assert len(calls) == 2
    r = runner.invoke(cli, ["motif_centrality", "--help"])
    for opt in ("--res_dir", "--library_file", "--control_fasta_file", "--p_value", "--min_score", "--pseudocount", "--nsites_default",
                "--revcom_mode", "--min_half", "--min_sites", "--top_hist", "--output_dir"):
        assert opt in r.output, opt
    assert "motif_centrality" in runner.invoke(cli, ["--help"]).output
    import kmap_amd.cli as cli_module
    assert "motif_centrality" in cli_module.__doc__
    assert "motif_centrality" in (ROOT / "README.md").read_text()
