"""Host side of motif_cooccurrence (no GPU): the hypergeometric moments against the enumeration of the distribution, the exact
tail against the direct sum of binomial coefficients, the tested rule, Benjamini-Hochberg over the tested pairs, the order of the
written rows, the files' text field by field for a hand-made count matrix, the verb on a model-backed DeviceSeq, and the errors
that must come before the device is touched."""
import math
import re
from pathlib import Path

import numpy as np
import pytest

from tests import _cooccurrence_model as CM
from tests import _sites_model as S

ROOT = Path(__file__).resolve().parent.parent
LIB = ROOT / "tests" / "golden" / "library"


def two_by_two(n_i, n_j, n_both):
    return np.array([[n_i, n_both], [n_both, n_j]], np.int64)


# ---- 1. the statistic -----------------------------------------------------------------------------------------------------------------
def test_moments_against_the_enumerated_distribution():
    from kmap_amd.cooccurrence import pair_stats
    checked = 0
    for N in range(2, 13):
        for n_i in range(N + 1):
            for n_j in range(N + 1):
                lo = max(0, n_i + n_j - N)
                st = pair_stats(two_by_two(n_i, n_j, lo), N, 0.0)
                mean, var = CM.comb_moments(N, n_i, n_j)
                assert st["expected"][0] == pytest.approx(mean, rel=1e-13, abs=1e-13)
                assert st["variance"][0] == pytest.approx(var, rel=1e-12, abs=1e-13)
                assert bool(st["tested"][0]) == (var > 1e-13)                 # min_expected 0: every pair whose count can vary
                if st["tested"][0]:
                    assert st["z"][0] == pytest.approx((lo - mean) / math.sqrt(var), rel=1e-12, abs=1e-12)
                checked += 1
    assert checked == sum((N + 1) ** 2 for N in range(2, 13))


def test_exact_tail_against_the_direct_sum():
    from kmap_amd.cooccurrence import log10_p_exact
    rng = np.random.default_rng(2002)
    cases = [(N, n_i, n_j) for N in (1, 2, 7, 12) for n_i in range(N + 1) for n_j in range(N + 1)]
    cases += [(int(N), int(rng.integers(0, N + 1)), int(rng.integers(0, N + 1))) for N in rng.integers(13, 61, 150)]
    cases += [(60, 30, 30), (60, 1, 59), (60, 60, 17), (60, 0, 5), (59, 40, 45)]
    n = 0
    for N, n_i, n_j in cases:
        lo, hi = max(0, n_i + n_j - N), min(n_i, n_j)
        for k in sorted({lo, hi, (lo + hi) // 2, min(lo + 1, hi), max(hi - 1, lo)}):          # either end of the support included
            for upper in (True, False):
                assert log10_p_exact(k, n_i, n_j, N, upper) == pytest.approx(CM.comb_log10_p_exact(k, n_i, n_j, N, upper), abs=1e-9)
                n += 1
    assert n > 1500
    assert log10_p_exact(0, 5, 5, 60, True) == 0.0 and log10_p_exact(5, 5, 5, 60, False) == 0.0      # the whole support: capped
    assert log10_p_exact(30, 30, 30, 60, True) == pytest.approx(math.log10(2.0 / math.comb(60, 30)), abs=1e-9)
    for bad in ((6, 5, 5, 60), (-1, 5, 5, 60), (0, 40, 40, 60), (1, 61, 5, 60)):
        with pytest.raises(ValueError, match="log10_p_exact"):
            log10_p_exact(*bad, True)


def test_the_forty_decades_cut_changes_nothing_that_counts():
    """a long tail: the terms more than 40 decades under the largest are left out, the sum keeps twelve digits"""
    from kmap_amd.cooccurrence import log10_p_exact
    N, n_i, n_j, k = 5000, 1500, 1200, 420                  # E = 360
    full = CM.comb_log10_p_exact(k, n_i, n_j, N, True)
    assert full < -3 and log10_p_exact(k, n_i, n_j, N, True) == pytest.approx(full, abs=1e-9)
    full = CM.comb_log10_p_exact(300, n_i, n_j, N, False)
    assert full < -3 and log10_p_exact(300, n_i, n_j, N, False) == pytest.approx(full, abs=1e-9)


HAND_N = 1000
HAND_C = np.array([[400, 250, 80, 4],
                   [250, 300, 30, 3],
                   [80, 30, 200, 0],
                   [4, 3, 0, 10]], np.int64)
HAND_CONTROL_N = 900
HAND_CONTROL = np.array([[380, 120, 70, 5],
                         [120, 290, 60, 2],
                         [70, 60, 210, 1],
                         [5, 2, 1, 12]], np.int64)


def test_stats_equal_the_pairwise_model_and_the_tested_rule():
    from kmap_amd.cooccurrence import pair_stats
    st = pair_stats(HAND_C, HAND_N)
    want = CM.np_pair_stats(HAND_C, HAND_N)
    assert [(int(a), int(b)) for a, b in zip(st["i"], st["j"])] == [(r["i"], r["j"]) for r in want] == [(0, 1), (0, 2), (0, 3), (1, 2),
                                                                                                       (1, 3), (2, 3)]
    assert st["tested"].tolist() == [True, True, False, True, False, False] == [r["tested"] for r in want]     # n = 10: E = 4, 3, 2
    assert st["n_tests"] == 3 == want[0]["n_tests"]
    for p, r in enumerate(want):
        assert (int(st["n_i"][p]), int(st["n_j"][p]), int(st["n_both"][p])) == (r["n_i"], r["n_j"], r["n_both"])
        assert st["expected"][p] == r["expected"] and st["variance"][p] == r["variance"]
        if r["tested"]:
            assert st["z"][p] == r["z"] and st["log10_p"][p] == r["log10_p"] and st["q_bh"][p] == pytest.approx(r["q_bh"], rel=1e-15)
        else:
            assert math.isnan(st["z"][p]) and math.isnan(st["log10_p"][p]) and math.isnan(st["q_bh"][p])
    assert want[0]["direction"] == "together" and want[1]["z"] == 0.0 and want[1]["direction"] == "none" and want[3]["direction"] == "apart"
    assert st["log10_p"][1] == 0.0 and st["q_bh"][1] == 1.0
    # the rule's three parts, one at a time: E, n_i - E and n_j - E against min_expected = 5
    for n_i, n_j, N, tested in ((50, 100, 1000, True), (49, 100, 1000, False), (100, 49, 1000, False), (995, 990, 1000, False),
                                (990, 995, 1000, False), (500, 990, 1000, True), (500, 991, 1000, False), (1000, 500, 1000, False)):
        st1 = pair_stats(two_by_two(n_i, n_j, max(0, n_i + n_j - N)), N)
        assert bool(st1["tested"][0]) == tested == CM.np_pair_stats(two_by_two(n_i, n_j, max(0, n_i + n_j - N)), N)[0]["tested"]
        assert st1["n_tests"] == int(tested)
    assert pair_stats(np.zeros((1, 1), np.int64), 10)["n_tests"] == 0 and len(pair_stats(np.zeros((0, 0), np.int64), 0)["z"]) == 0
    assert not pair_stats(np.zeros((3, 3), np.int64), 0)["tested"].any()                                    # no reads at all
    for bad, N in ((HAND_C[:3], 1000), (HAND_C - 1, 1000), (HAND_C, 399), (np.array([[5, 6], [6, 9]]), 10), (np.array([[5, 3], [2, 9]]), 10),
                   (HAND_C.astype(np.float64), 1000)):
        with pytest.raises(ValueError):
            pair_stats(bad, N)
    with pytest.raises(ValueError, match="min_expected"):
        pair_stats(HAND_C, HAND_N, -1.0)


def test_bh_over_the_tested_pairs_only():
    """a library with many rare motifs: their pairs are not tested and do not dilute the q-values of the others"""
    from kmap_amd.cooccurrence import pair_stats
    from kmap_amd.library import bh_qvalues
    rng = np.random.default_rng(2003)
    N, m = 2000, 12
    bits = rng.random((m, N)) < np.array([0.3] * 5 + [0.001] * 7)[:, None]
    bits[1] |= bits[0] & (rng.random(N) < 0.5)
    C = CM.np_pair_counts(bits)
    st = pair_stats(C, N)
    assert st["n_tests"] == 10 and st["tested"].sum() == 10 and len(st["z"]) == 66
    np.testing.assert_array_equal(st["q_bh"][st["tested"]], bh_qvalues(10.0 ** st["log10_p"][st["tested"]]))
    assert np.isnan(st["q_bh"][~st["tested"]]).all()
    want = CM.np_pair_stats(C, N)
    np.testing.assert_allclose(st["q_bh"][st["tested"]], [r["q_bh"] for r in want if r["tested"]], rtol=1e-15)
    p01 = 10.0 ** st["log10_p"][0]
    assert st["q_bh"][0] <= p01 * 10 and st["q_bh"][0] < p01 * 66                    # ten tests, not sixty-six


def test_rank_order_and_ties():
    from kmap_amd.cooccurrence import pair_stats, select_rows
    # five motifs with the same margin; pairs (0, 1) and (2, 3) share the same count, (0, 2) one fewer, the others are at the mean
    N, n = 1000, 100
    C = np.full((5, 5), 10, np.int64)
    np.fill_diagonal(C, n)
    C[0, 1] = C[1, 0] = C[2, 3] = C[3, 2] = 40
    C[0, 2] = C[2, 0] = 39
    C[1, 4] = C[4, 1] = 0                                        # the most negative z: |z| decides, not z
    st = pair_stats(C, N)
    assert st["tested"].all()

    def pairs_of(names, top_n):
        return [(int(st["i"][p]), int(st["j"][p])) for p in select_rows(st, names, top_n)]
    got = pairs_of(["a", "b", "c", "d", "e"], 4)
    assert got == [(0, 1), (2, 3), (0, 2), (1, 4)]
    assert pairs_of(["c", "d", "a", "b", "e"], 2) == [(2, 3), (0, 1)]            # the tie goes by the names, not by the index
    assert pairs_of(["a", "z", "a", "b", "e"], 2) == [(2, 3), (0, 1)]            # ... first name equal: the second decides
    everything = pairs_of(["a", "b", "c", "d", "e"], 0)
    assert len(everything) == 10 and everything[:4] == got
    z = np.abs(st["z"][select_rows(st, ["a", "b", "c", "d", "e"], 0)])
    assert (np.diff(z) <= 0).all()
    order = CM.model_order(CM.np_pair_stats(C, N), ["a", "b", "c", "d", "e"], 0)
    assert [(r["i"], r["j"]) for r in order] == everything
    # untested pairs are written only by top_n 0, behind the tested ones, by their names
    st = pair_stats(HAND_C, HAND_N)
    names = ["m3", "m1", "m2", "m0"]
    rows = [(int(st["i"][p]), int(st["j"][p])) for p in select_rows(st, names, 0)]
    assert rows[:3] == [(0, 1), (1, 2), (0, 2)] and rows[3:] == [(1, 3), (2, 3), (0, 3)]
    assert len(select_rows(st, names, 1000)) == 3 and len(select_rows(st, names, 2)) == 2


# ---- 2. the files ---------------------------------------------------------------------------------------------------------------------
def hand_motifs():
    from kmap_amd.library import LibraryMotif
    rng = np.random.default_rng(2004)
    names = [("beta", "B,1", 8), ("alpha", "", 11), ("gamma", "G", 6), ("rare", "", 31)]
    return [LibraryMotif(n, alt, f"lib{i}.meme", rng.integers(0, 30, (4, w)).astype(np.int64)) for i, (n, alt, w) in enumerate(names)]


@pytest.mark.parametrize("control", [False, True])
def test_file_text_field_by_field(tmp_path, control):
    from kmap_amd import cooccurrence as CO
    from kmap_amd.enrichment import enrich_z
    from kmap_amd.pwm import pwm_consensus
    motifs, ts = hand_motifs(), [812, -40, 1234, 0]
    names = [m.name for m in motifs]
    Cc, Nc = (HAND_CONTROL, HAND_CONTROL_N) if control else (None, None)
    rows, st = CO.pair_rows(HAND_C, HAND_N, names, 5.0, 0, Cc, Nc)
    CO.write_tables(tmp_path, motifs, ts, rows, HAND_C, HAND_N, Cc, Nc, write_matrix=True)
    text = (tmp_path / "cooccurrence_pairs.csv").read_text().split("\n")
    cols = text[0].split(",")
    assert cols == ("rank,name_i,altname_i,width_i,name_j,altname_j,width_j,n_i,n_j,n_both,expected,z,direction,log10_p,log10_p_exact,"
                    "n_tests,q_bh".split(",") + (["control_i", "control_j", "control_both", "z_vs_control"] if control else []))
    assert len(text) == 8 and text[7] == ""
    want = CM.model_order(CM.np_pair_stats(HAND_C, HAND_N), names, 0)
    assert [(r["i"], r["j"]) for r in want] == [(0, 1), (1, 2), (0, 2), (1, 3), (0, 3), (2, 3)]      # alpha + rare before beta + rare
    for rank, (line, r) in enumerate(zip(text[1:7], want)):
        f = dict(zip(cols, line.split(",")))
        assert len(line.split(",")) == len(cols)
        mi, mj = motifs[r["i"]], motifs[r["j"]]
        assert (f["rank"], f["name_i"], f["altname_i"], f["width_i"]) == (str(rank), mi.name, mi.altname, str(mi.counts.shape[1]))
        assert (f["name_j"], f["altname_j"], f["width_j"]) == (mj.name, mj.altname, str(mj.counts.shape[1]))
        assert (f["n_i"], f["n_j"], f["n_both"], f["n_tests"]) == (str(r["n_i"]), str(r["n_j"]), str(r["n_both"]), "3")
        assert f["expected"] == repr(r["expected"])
        if r["tested"]:
            assert f["z"] == repr(r["z"]) and f["direction"] == r["direction"] and f["log10_p"] == repr(r["log10_p"])
            assert float(f["q_bh"]) == pytest.approx(r["q_bh"], rel=1e-15) and f["q_bh"] == repr(float(f["q_bh"]))
            exact = 0.0 if r["z"] == 0 else CM.comb_log10_p_exact(r["n_both"], r["n_i"], r["n_j"], HAND_N, r["z"] > 0)
            assert float(f["log10_p_exact"]) == pytest.approx(exact, abs=1e-9)
        else:
            assert f["z"] == f["direction"] == f["log10_p"] == f["log10_p_exact"] == f["q_bh"] == ""
        if control:
            ci, cj, cij = int(HAND_CONTROL[r["i"], r["i"]]), int(HAND_CONTROL[r["j"], r["j"]]), int(HAND_CONTROL[r["i"], r["j"]])
            assert (f["control_i"], f["control_j"], f["control_both"]) == (str(ci), str(cj), str(cij))
            assert f["z_vs_control"] == repr(enrich_z(r["n_both"], cij, HAND_N, HAND_CONTROL_N))
    assert text[1].startswith("0,beta,B_1,8,alpha,,11,400,300,250,120.0,") and ",together," in text[1]
    assert text[2].split(",")[12] == "apart" and text[3].split(",")[11:15] == ["0.0", "none", "0.0", "0.0"]
    # top_n cuts the tested rows and never writes an untested one
    assert [(r["i"], r["j"]) for r in CO.pair_rows(HAND_C, HAND_N, names, 5.0, 2)[0]] == [(0, 1), (1, 2)]
    assert len(CO.pair_rows(HAND_C, HAND_N, names, 5.0, 1000)[0]) == 3

    pres = (tmp_path / "motif_presence.csv").read_text().split("\n")
    assert pres[0] == "name,altname,source,width,consensus,threshold,threshold_bits,n_present,share" + (
        ",control_present,control_share" if control else "")
    assert len(pres) == 6 and pres[5] == ""
    for i, (line, m, t) in enumerate(zip(pres[1:5], motifs, ts)):
        want_line = [m.name, m.altname, m.source, str(m.counts.shape[1]), pwm_consensus(m.counts), str(t), f"{t / 100:.2f}",
                     str(int(HAND_C[i, i])), repr(int(HAND_C[i, i]) / HAND_N)]
        if control:
            want_line += [str(int(HAND_CONTROL[i, i])), repr(int(HAND_CONTROL[i, i]) / HAND_CONTROL_N)]
        assert line.split(",") == want_line
    assert pres[2].split(",")[5:9] == ["-40", "-0.40", "300", "0.3"]

    mat = (tmp_path / "pair_counts.tsv").read_text().split("\n")
    assert mat[0] == "\tbeta\talpha\tgamma\trare" and len(mat) == 6 and mat[5] == ""
    assert mat[1] == "beta\t400\t250\t80\t4" and mat[4] == "rare\t4\t3\t0\t10"


# ---- 3. the verb on the model -------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def model_run(tmp_path, monkeypatch):
    import kmap_amd.kmer_count as K
    import kmap_amd.motif_discovery as D
    from tests import _readscore_model as M
    res, ctl, seq, borders, cseq, cborders = S.write_planted(tmp_path)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(D, "DeviceSeq", CM.ModelSeq)
    monkeypatch.setattr(K, "encode_fasta", lambda path: M.encode_fasta_np(path))
    return res, ctl, seq, borders, cseq, cborders


def test_verb_on_the_model(model_run, tmp_path, capsys):
    from kmap_amd import cooccurrence as CO
    from kmap_amd.pwm import pwm_threshold, pwm_weights
    res, ctl, seq, borders, cseq, cborders = model_run
    lib = [str(LIB / "three.meme"), str(LIB / "mixed")]
    out = tmp_path / "o"
    got = CO._motif_cooccurrence(str(res), lib, str(ctl), output_dir=str(out), top_n=0, write_matrix=True)
    printed = capsys.readouterr().out
    names = [m.name for m in got["motifs"]]
    assert names[:2] == ["M1_CAATCGATAGC", "M2_ACCTACGTA"] and len(names) == 4
    Ws = [pwm_weights(m.counts, 1.0) for m in got["motifs"]]
    assert got["thresholds"] == [pwm_threshold(W, 1e-4)[0] for W in Ws]
    bits = CM.np_presence(seq, borders, Ws, got["thresholds"], True)
    np.testing.assert_array_equal(got["pair_counts"], CM.np_pair_counts(bits))
    np.testing.assert_array_equal(got["control_pair_counts"], CM.np_pair_counts(CM.np_presence(cseq, cborders, Ws, got["thresholds"], True)))
    assert got["n_reads"] == 600 == got["control_reads"]
    # a_counts is M2's matrix again: the two are together by construction, in every read.  The planted halves exclude each other:
    # 300 reads hold M1, the other 300 hold M2
    first, second = got["rows"][:2]
    assert (names[first["i"]], names[first["j"]]) == ("M2_ACCTACGTA", "a_counts") and first["direction"] == "together"
    assert first["n_both"] == first["n_i"] == first["n_j"] == 300
    assert (names[second["i"]], names[second["j"]]) == ("M1_CAATCGATAGC", "M2_ACCTACGTA") and second["direction"] == "apart"
    assert second["n_both"] < 10 and second["z"] < -20 and second["log10_p_exact"] < -50 and second["q_bh"] < 1e-50
    assert sorted(p.name for p in out.iterdir()) == ["cooccurrence_pairs.csv", "motif_presence.csv", "pair_counts.tsv", "skipped.csv"]
    assert (out / "skipped.csv").read_text().split("\n")[1].startswith("M3_long,too_wide,")
    assert len((out / "cooccurrence_pairs.csv").read_text().split("\n")) == 1 + 6 + 1
    assert f"of 6 pairs tested, 1 skipped, both strands: {out}" in printed and printed.startswith("0 M2_ACCTACGTA + a_counts: 300 reads hold both ")
    assert len(printed.strip().split("\n")) == 7
    # the defaults: res_dir/motif_cooccurrence, no control columns, no matrix, the forward strand on request
    fwd = CO._motif_cooccurrence(str(res), lib, revcom_mode=False, min_score=9.0)
    assert "forward strand" in capsys.readouterr().out and fwd["thresholds"] == [900] * 4 and "control_reads" not in fwd
    d = res / "motif_cooccurrence"
    assert sorted(p.name for p in d.iterdir()) == ["cooccurrence_pairs.csv", "motif_presence.csv", "skipped.csv"]
    assert (d / "cooccurrence_pairs.csv").read_text().split("\n")[0].endswith(",n_tests,q_bh")
    np.testing.assert_array_equal(fwd["pair_counts"], CM.np_pair_counts(CM.np_presence(seq, borders, Ws, [900] * 4, False)))


def test_errors_come_before_the_device(tmp_path, monkeypatch):
    import kmap_amd.motif_discovery as D
    from kmap_amd import cooccurrence as CO
    res, ctl, *_ = S.write_planted(tmp_path)
    res, out, three = str(res), tmp_path / "o", str(LIB / "three.meme")
    monkeypatch.delenv("WORLD_SIZE", raising=False)

    class NoDevice:
        def __init__(self, *a, **k):
            raise AssertionError("the device was touched")
    monkeypatch.setattr(D, "DeviceSeq", NoDevice)
    only_wide = tmp_path / "wide.meme"
    only_wide.write_text("MEME version 4\n\nMOTIF W\nletter-probability matrix: alength= 4 w= 32\n" + "0.25 0.25 0.25 0.25\n" * 32)
    ok = dict(library_files=[three], output_dir=out)
    bad = [(dict(res_dir=tmp_path / "nowhere"), "config.toml"),
           (dict(library_files=[]), "no library file"),
           (dict(library_files=[str(tmp_path / "nowhere.meme")]), "nowhere.meme"),
           (dict(control_fasta_file=str(tmp_path / "nowhere.fa")), "nowhere.fa"),
           (dict(library_files=[three, str(LIB / "bad_alength.meme")]), "bad_alength.meme:11"),
           (dict(library_files=[str(only_wide)]), "none of the 1 motifs.*W: width 32"),
           (dict(top_n=-1), "top_n -1"),
           (dict(top_n=2.5), "top_n 2.5"),
           (dict(min_expected=-0.5), "min_expected -0.5"),
           (dict(min_expected=float("nan")), "min_expected nan"),
           (dict(pseudocount=-1.0), "pseudocount"),
           (dict(p_value=float("nan")), "p_value"),
           (dict(min_score=float("inf")), "min_score"),
           (dict(nsites_default=0), "nsites_default")]
    for change, word in bad:
        with pytest.raises(ValueError, match=word):
            CO._motif_cooccurrence(**{"res_dir": res, **ok, **change})
    assert not out.exists() and not (Path(res) / "motif_cooccurrence").exists()
    with pytest.raises(AssertionError, match="the device was touched"):
        CO._motif_cooccurrence(res, **ok)
    assert not out.exists()


def test_other_ranks_do_nothing(monkeypatch):
    from kmap_amd.cooccurrence import _motif_cooccurrence
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "1")
    assert _motif_cooccurrence("nowhere", []) is None


# ---- 4. the model's own pieces ----------------------------------------------------------------------------------------------------------
def test_model_pack_and_pair_counts():
    rng = np.random.default_rng(2005)
    bits = rng.random((7, 200)) < 0.3
    planes = CM.np_pack(bits)
    assert planes.shape == (7, 4) and planes.dtype == np.uint64
    assert int(planes[0, 0]) & 1 == int(bits[0, 0]) and (int(planes[3, 1]) >> 5) & 1 == int(bits[3, 69])
    assert not (planes[:, 3] >> np.uint64(8)).any()                               # 200 = 3 x 64 + 8: the tail is zero
    np.testing.assert_array_equal(CM.np_unpack(planes, 200), bits)
    np.testing.assert_array_equal(np.packbits(bits, axis=1, bitorder="little"), planes.view(np.uint8)[:, :25])
    C = CM.np_pair_counts(bits)
    np.testing.assert_array_equal(C, bits.astype(np.int64) @ bits.astype(np.int64).T)
    assert C.dtype == np.int64


# ---- 5. the library's entries and the command line ------------------------------------------------------------------------------------------
def test_symbols_registered_and_constants():
    from kmap_amd import _ffi, cooccurrence, device_seq
    header = (ROOT / "include" / "kmap_hip.h").read_text()
    for name, n_args in (("kmap_presence_library_dev", 14), ("kmap_bitrows_pair_counts_dev", 5)):
        assert name in _ffi.exported_symbols() and f"int {name}(" in header
        res, args = _ffi._SIGS[name]
        assert res is _ffi.i32 and len(args) == n_args
        declared = header[header.index(f"int {name}("):]
        declared = re.sub(r"/\*.*?\*/", "", declared[:declared.index(";")], flags=re.S)
        assert declared.count(",") + 1 == n_args
    src = (ROOT / "kmap_amd" / "csrc" / "bit_pairs.hip").read_text()
    assert int(re.search(r"constexpr int BP_K = (\d+);", src).group(1)) == device_seq.BIT_PAIRS_K
    assert int(re.search(r"constexpr int64_t BP_MIN_SLICE = (\d+);", src).group(1)) == device_seq.BIT_PAIRS_MIN_SLICE
    assert int(re.search(r"constexpr int BP_MAX_ROWS = (\d+);", src).group(1)) == device_seq.BIT_PAIRS_MAX_ROWS == cooccurrence.MAX_MOTIFS
    assert device_seq.BIT_PAIRS_MIN_SLICE % device_seq.BIT_PAIRS_K == 0
    src = (ROOT / "kmap_amd" / "csrc" / "pwm_presence.hip").read_text()
    batch = (ROOT / "kmap_amd" / "csrc" / "pwm_batch.h").read_text()
    assert int(re.search(r"constexpr int PB_MAX_MAT = (\d+);", batch).group(1)) == device_seq.LIBRARY_BATCH
    # the scoring kernel exists once, in the header: the presence planes go through its batch pass with the score key
    assert "__global__" in batch and "pwm_batch_kernel" not in re.sub(r"//.*", "", src) and "pwm_key_batches<ScoreKey>(" in src


def test_library_presence_checks_come_before_the_library(monkeypatch):
    from kmap_amd import _ffi
    from kmap_amd.device_seq import DeviceSeq

    def no_lib():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_ffi, "lib", no_lib)
    ds = object.__new__(DeviceSeq)
    ds.n_seq = 2
    ok = np.zeros((4, 8), np.int32)
    for kw, word in ((dict(Ws=[np.zeros((4, 3), np.int32)], thresholds=[0]), "width 3"),
                     (dict(Ws=[ok, np.zeros((4, 32), np.int32)], thresholds=[0, 0]), "matrix 1 has width 32"),
                     (dict(Ws=[np.zeros((3, 8), np.int32)], thresholds=[0]), "shape"), (dict(Ws=[ok], thresholds=[2 ** 31]), "int32"),
                     (dict(Ws=[ok], thresholds=[0, 1]), "1 matrices, 2 thresholds")):
        with pytest.raises(ValueError, match="library_presence: .*" + word):
            ds.library_presence(revcom=True, **kw)
    with pytest.raises(AssertionError, match="the library was loaded"):
        ds.library_presence([ok], [0], True)


def test_cli_options_and_defaults(monkeypatch):
    from click.testing import CliRunner
    from kmap_amd import cooccurrence
    from kmap_amd.cli import cli
    calls = []
    monkeypatch.setattr(cooccurrence, "_motif_cooccurrence", lambda *a: calls.append(a))
    runner = CliRunner()
    r = runner.invoke(cli, ["motif_cooccurrence", "--res_dir", "D", "--library_file", "L"])
    assert r.exit_code == 0, r.output
    assert calls[-1] == ("D", ["L"], None, 1e-4, None, 1.0, 20, None, 5.0, 1000, False, None)
    r = runner.invoke(cli, ["motif_cooccurrence", "--res_dir", "D", "--library_file", "L", "--library_file", "L2", "--control_fasta_file", "C",
                            "--p_value", "1e-3", "--min_score", "8.5", "--pseudocount", "0.5", "--nsites_default", "100", "--revcom_mode",
                            "False", "--min_expected", "2", "--top_n", "0", "--write_matrix", "--output_dir", "O"])
    assert r.exit_code == 0, r.output
    assert calls[-1] == ("D", ["L", "L2"], "C", 1e-3, 8.5, 0.5, 100, False, 2.0, 0, True, "O")
    for missing in (["--library_file", "L"], ["--res_dir", "D"]):
        assert runner.invoke(cli, ["motif_cooccurrence"] + missing).exit_code == 2
    assert len(calls) == 2
    r = runner.invoke(cli, ["motif_cooccurrence", "--help"])
    for opt in ("--res_dir", "--library_file", "--control_fasta_file", "--p_value", "--min_score", "--pseudocount", "--nsites_default",
                "--revcom_mode", "--min_expected", "--top_n", "--write_matrix", "--output_dir"):
        assert opt in r.output, opt
    assert "motif_cooccurrence" in runner.invoke(cli, ["--help"]).output
    import kmap_amd.cli as cli_module
    assert "motif_cooccurrence" in cli_module.__doc__
    assert "motif_cooccurrence" in (ROOT / "README.md").read_text()
