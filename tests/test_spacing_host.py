"""Host side of motif_spacing (no GPU): the null's bin probabilities against the enumeration of every admissible window of a read, E
against exact fractions on hand-made room histograms, the Poisson tail against a sum of the pmf, the tie rule, the candidate count,
Bonferroni and the no-bin cases of the best bin, the verb's files with the device pass replaced by the numpy model of
tests/_spacing_model.py on seeded reads with one partner planted at a fixed gap and one planted uniformly, its argument errors
(raised before the library is loaded or a directory made), the library's entry and the CLI verb.  The definitions are DESIGN.md
section 19."""
import math
import re
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

from tests import _spacing_model as S

ROOT = Path(__file__).resolve().parent.parent
LIB = ROOT / "tests" / "golden" / "library"


def one_read(u, d, G):
    R = np.zeros((G + 2, G + 2), np.int64)
    R[u, d] = 1
    return R


# ---- 1. the null ----------------------------------------------------------------------------------------------------------------------
def test_bin_probabilities_against_enumeration():
    """every window of width w of a read of length L that does not overlap the primary window and lies within G bases of it, on
    each of the s strands, is equally likely: the share of them in bin (quadrant, g) must be the pi that rooms() and expected_bins()
    give, exactly (a bin holds one window position or none)"""
    from kmap_amd.spacing import expected_bins, rooms
    checked = 0
    for G in (0, 5, 60):
        for wP in (4, 7):
            for w in (4, 7):
                for L in range(wP, 41):
                    for p in range(L - wP + 1):
                        for minus in (False, True):
                            bins = {}
                            for loc in range(L - w + 1):
                                left, right = loc + w <= p, loc >= p + wP
                                if not (left or right):
                                    continue
                                g = p - loc - w if left else loc - p - wP
                                if g > G:
                                    continue
                                downstream = right != minus
                                bins[(downstream, g)] = bins.get((downstream, g), 0) + 1
                            u, d = rooms(L, p, wP, w, G, minus)
                            assert u + d == len(bins) and set(bins.values()) <= {1}
                            assert u == sum(1 for k in bins if not k[0]) and d == sum(1 for k in bins if k[0])
                            if not bins:
                                continue
                            for revcom, s in ((True, 2), (False, 1)):
                                E = expected_bins(one_read(u, d, G), revcom)
                                for q in range(4):
                                    for g in range(G + 1):
                                        inside = (bool(q >> 1), g) in bins and (revcom or not q & 1)
                                        assert E[q, g] == (1.0 / (s * len(bins)) if inside else 0.0), (G, wP, w, L, p, minus, q, g)
                                checked += 1
    assert checked > 10_000
    for bad in ((10, -1, 4, 4, 5), (10, 7, 4, 4, 5), (10, 0, 4, 0, 5), (10, 0, 4, 4, -1)):
        with pytest.raises(ValueError, match="rooms"):
            rooms(*bad, False)


def hand_made(G):
    """a room histogram with reads of many rooms, among them one-sided ones and the caps G + 1"""
    rng = np.random.default_rng(1920 + G)
    R = np.zeros((G + 2, G + 2), np.int64)
    for u, d, c in ((0, 1, 3), (1, 0, 2), (G + 1, G + 1, 1000), (G + 1, 0, 7), (0, G + 1, 11), (1, 1, 5), (G // 2 + 1, G // 3 + 1, 123_456)):
        R[u, d] += c
    for _ in range(40):
        u, d = int(rng.integers(0, G + 2)), int(rng.integers(0, G + 2))
        if u + d:
            R[u, d] += int(rng.integers(1, 10_000))
    return R


@pytest.mark.parametrize("G", [0, 5, 60, 511])
def test_expected_against_fractions(G):
    """definition 5 in exact fractions; the float sums have at most (G + 2)^2 <= 263 169 positive doubles, so their error is about
    3e-11 relative: rtol 1e-9"""
    from kmap_amd.spacing import expected_bins
    R = hand_made(G)
    for revcom, s in ((True, 2), (False, 1)):
        exact = [[Fraction(0)] * (G + 1) for _ in range(4)]
        for u, d in zip(*np.nonzero(R)):
            share = Fraction(int(R[u, d]), s * int(u + d))
            for opposite in range(s):
                for g in range(int(u)):
                    exact[opposite][g] += share
                for g in range(int(d)):
                    exact[2 + opposite][g] += share
        E = expected_bins(R, revcom)
        assert E.shape == (4, G + 1) and E.dtype == np.float64
        for q in range(4):
            for g in range(G + 1):
                assert (E[q, g] > 0) == (exact[q][g] > 0)
                assert E[q, g] == pytest.approx(float(exact[q][g]), rel=1e-9, abs=0)
        assert E.sum() == pytest.approx(float(R.sum()), rel=1e-9)          # the invariant: sum E = sum R
        assert sum(sum(row) for row in exact) == int(R.sum())
        if not revcom:
            assert not E[1].any() and not E[3].any()


# ---- 2. the tail ----------------------------------------------------------------------------------------------------------------------
def test_poisson_tail_against_the_pmf():
    """P(X >= k) from the pmf in exact fractions times exp(-mu), summed with math.fsum; where the tail is close to 1 its log10 is
    taken from the lower tail, which does not cancel.  rtol 1e-9 on log10 p."""
    from kmap_amd.spacing import log10_poisson_sf
    for mu_f in (Fraction(1, 100), Fraction(137, 100), Fraction(1), Fraction(5, 2), Fraction(7), Fraction(20), Fraction(1999, 100)):
        mu = float(mu_f)
        pmf = [float(mu_f ** j / math.factorial(j)) * math.exp(-mu) for j in range(400)]
        assert math.fsum(pmf) == pytest.approx(1.0, rel=1e-12)
        for k in range(1, 41):
            upper, lower = math.fsum(pmf[k:]), math.fsum(pmf[:k])
            want = math.log10(upper) if upper < 0.5 else math.log1p(-lower) / math.log(10.0)
            got = log10_poisson_sf(k, mu)
            assert got == pytest.approx(want, rel=1e-9, abs=0), (k, mu)
            assert 10.0 ** got == pytest.approx(upper, rel=1e-9)
        assert log10_poisson_sf(0, mu) == 0.0
    assert log10_poisson_sf(0, 0.0) == 0.0 and log10_poisson_sf(3, 0.0) == -math.inf and log10_poisson_sf(1, 0) == -math.inf
    far = log10_poisson_sf(200, 1.37)
    assert math.isfinite(far) and far < -300
    assert far == pytest.approx((200 * math.log(1.37) - 1.37 - math.lgamma(201.0) + math.log1p(1.37 / 201 * (1 + 1.37 / 202))) / math.log(10), rel=1e-6)
    ks = [log10_poisson_sf(k, 3.3) for k in range(60)]
    assert all(a > b for a, b in zip(ks, ks[1:]))                           # strictly falling in k, across the switch at the mean
    for bad in ((-1, 1.0), (1.5, 1.0), (1, -0.1), (1, math.nan), (1, math.inf), (True, 1.0)):
        with pytest.raises(ValueError, match="log10_poisson_sf"):
            log10_poisson_sf(*bad)


# ---- 3. the best bin ------------------------------------------------------------------------------------------------------------------
def full_rooms(G, n):
    R = np.zeros((G + 2, G + 2), np.int64)
    R[G + 1, G + 1] = n
    return R


def test_best_bin_ties_candidates_bonferroni_and_no_bin():
    from kmap_amd.spacing import best_bin, log10_poisson_sf
    G = 9
    # 40 reads with full rooms on both sides: with both strands every one of the 4 x 10 bins expects 40 / 40 = 1
    S_ = np.zeros((4, G + 1), np.int64)
    S_[3, 4], S_[1, 7], S_[1, 2] = 12, 12, 12                # three equal bins: the smallest quadrant, then the smallest gap
    S_[0, 0] = 4
    st = best_bin(S_, full_rooms(G, 40), True)
    assert (st["quadrant"], st["gap"], st["pairs_in_bin"], st["n_in_range"], st["n_bins"]) == (1, 2, 12, 40, 40)
    assert st["expected_in_bin"] == pytest.approx(1.0, rel=1e-12)
    assert st["log10_p"] == log10_poisson_sf(12, st["expected_in_bin"]) and st["log10_p"] < -8
    assert st["log10_p_adj"] == st["log10_p"] + math.log10(40)
    # the forward strand alone: quadrants 1 and 3 are no candidates, a pair read there is an error
    with pytest.raises(ValueError, match="no read has room"):
        best_bin(S_, full_rooms(G, 40), False)
    S_f = np.zeros((4, G + 1), np.int64)
    S_f[2, 5], S_f[0, 5], S_f[0, 6] = 15, 15, 10
    st = best_bin(S_f, full_rooms(G, 40), False)
    assert (st["quadrant"], st["gap"], st["n_bins"]) == (0, 5, 20) and st["expected_in_bin"] == pytest.approx(2.0, rel=1e-12)
    assert st["log10_p_adj"] == st["log10_p"] + math.log10(20)
    # one-sided rooms: only the bins some read has room for are candidates
    R = np.zeros((G + 2, G + 2), np.int64)
    R[0, 3] = 12
    S_one = np.zeros((4, G + 1), np.int64)
    S_one[2, 0], S_one[2, 1], S_one[3, 2], S_one[3, 0] = 3, 3, 3, 3
    st = best_bin(S_one, R, True)
    assert st["n_bins"] == 6 and (st["quadrant"], st["gap"]) == (2, 0) and st["expected_in_bin"] == pytest.approx(2.0, rel=1e-12)
    # a weak bin: Bonferroni stops at p = 1
    assert st["log10_p"] < 0 and st["log10_p_adj"] == 0.0
    # fewer than min_pairs in range, or nothing at all: no bin, p = 1
    few = np.zeros((4, G + 1), np.int64)
    few[2, 3] = 9
    for st, bins in ((best_bin(few, full_rooms(G, 9), True), 40), (best_bin(np.zeros((4, G + 1), np.int64), full_rooms(G, 0), True), 0)):
        assert st["quadrant"] is None and st["gap"] is None and st["pairs_in_bin"] is None and st["expected_in_bin"] != st["expected_in_bin"]
        assert st["log10_p"] == 0.0 and st["log10_p_adj"] == 0.0 and st["n_bins"] == bins
    assert best_bin(few, full_rooms(G, 9), True, min_pairs=9)["gap"] == 3
    # histograms that cannot be a pass's result
    with pytest.raises(ValueError, match="different reads"):
        best_bin(few, full_rooms(G, 10), True)
    with pytest.raises(ValueError, match="without room"):
        best_bin(few, one_read(0, 0, G) * 9, True)
    with pytest.raises(ValueError, match="expected"):
        best_bin(few[:, :5], full_rooms(G, 9), True)
    with pytest.raises(ValueError, match="negative"):
        best_bin(-few, full_rooms(G, 9), True)
    for kw in (dict(min_pairs=0), dict(min_pairs=2.5)):
        with pytest.raises(ValueError, match="min_pairs"):
            best_bin(few, full_rooms(G, 9), True, **kw)


# ---- 4. the verb on the numpy model ---------------------------------------------------------------------------------------------------
@pytest.fixture
def planted(tmp_path, monkeypatch):
    """the seeded reads of tests/_spacing_model.py as a result directory; the device replaced by its model"""
    import kmap_amd.motif_discovery as D
    made = S.write_planted(tmp_path)
    monkeypatch.setattr(D, "DeviceSeq", S.ModelSeq)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    S.ModelSeq.calls = []
    return made


INT, BITS = re.compile(r"-?\d+"), re.compile(r"-?\d+\.\d\d")
FORMATS = dict(rank=INT, width=INT, threshold=INT, threshold_bits=BITS, n_primary=INT, n_pairs=INT, n_in_range=INT, n_far=INT,
               best_side=re.compile("upstream|downstream"), best_strand=re.compile("same|opposite"), best_gap=INT, pairs_in_bin=INT,
               n_bins=INT)
FLOATS = ("expected_in_bin", "log10_p", "log10_p_adj", "q_bh")
BIN_FIELDS = ("best_side", "best_strand", "best_gap", "pairs_in_bin", "expected_in_bin")


def check_table(path, results):
    from kmap_amd import spacing as C
    table = path.read_text().split("\n")
    cols = table[0].split(",")
    assert table[0] == ("rank,name,altname,source,width,consensus,threshold,threshold_bits,n_primary,n_pairs,n_in_range,n_far,best_side,"
                        "best_strand,best_gap,pairs_in_bin,expected_in_bin,log10_p,n_bins,log10_p_adj,q_bh")
    assert table[-1] == "" and len(table) == 2 + len(results)
    rows = [dict(zip(cols, line.split(","))) for line in table[1:-1]]
    for rank, (row, st) in enumerate(zip(rows, results)):
        assert len(row) == len(cols) == 21 and row["rank"] == str(rank) == str(st["rank"])
        has_bin = st["quadrant"] is not None
        for name, pattern in FORMATS.items():
            if has_bin or name not in BIN_FIELDS:
                assert pattern.fullmatch(row[name]), (name, row[name])
        for name in FLOATS:
            if has_bin or name not in BIN_FIELDS:
                assert repr(float(row[name])) == row[name], (name, row[name])
        m = st["motif"]
        assert (row["name"], row["altname"], row["source"], int(row["width"])) == (m.name, m.altname, m.source, m.counts.shape[1])
        assert int(row["threshold"]) == st["threshold"] and row["threshold_bits"] == "%.2f" % (st["threshold"] / 100)
        assert (int(row["n_primary"]), int(row["n_pairs"]), int(row["n_far"])) == (st["n_primary"], st["n_pairs"], st["n_far"])
        assert int(row["n_in_range"]) == st["n_in_range"] == st["n_pairs"] - st["n_far"] == int(st["S"].sum()) == int(st["R"].sum())
        if has_bin:
            q = st["quadrant"]
            assert (row["best_side"], row["best_strand"]) == (("upstream", "downstream")[q >> 1], ("same", "opposite")[q & 1])
            assert int(row["best_gap"]) == st["gap"] and int(row["pairs_in_bin"]) == st["pairs_in_bin"] == int(st["S"][q, st["gap"]])
            assert float(row["expected_in_bin"]) == st["expected_in_bin"]
        else:
            assert all(row[name] == "" for name in BIN_FIELDS) and row["log10_p"] == "0.0" and row["log10_p_adj"] == "0.0"
        assert float(row["log10_p"]) == st["log10_p"] and float(row["log10_p_adj"]) == st["log10_p_adj"] and float(row["q_bh"]) == st["q_bh"]
        assert int(row["n_bins"]) == st["n_bins"]
        assert C.rank_line(rank, m, st["threshold"], st) == table[1 + rank] + "\n"
    with_bin = [float(r["log10_p_adj"]) for r in rows if r["best_gap"]]
    assert with_bin == sorted(with_bin) and all(r["best_gap"] == "" for r in rows[len(with_bin):])
    return rows


def check_histogram(path, st):
    lines = path.read_text().split("\n")
    assert lines[0] == "side,strand,gap,pairs,expected" and lines[-1] == ""
    want = []
    for q in range(4):
        for g in np.nonzero(st["S"][q])[0]:
            want.append(f"{('upstream', 'downstream')[q >> 1]},{('same', 'opposite')[q & 1]},{g},{int(st['S'][q, g])},{float(st['E'][q, g])!r}")
    assert lines[1:-1] == want and len(want) > 0


def test_verb_on_planted_reads(planted, tmp_path, capsys):
    """The model ranks the partner planted 3 bases downstream first, in the bin (downstream, same, 3) with q_bh < 0.01; the
    uniformly planted one has q_bh > 0.05; the primary against itself finds no second site (seed fixed after checking seeds
    1900 - 1911 on the CPU, both strand settings: log10_p_adj of the fixed partner <= -131 with 92 - 200 pairs in the bin, the
    uniform motif's q_bh >= 0.134, at most one self pair)."""
    from kmap_amd import spacing as C
    from kmap_amd.library import bh_qvalues
    from kmap_amd.pwm import pwm_threshold, pwm_weights
    res, primary, files, seq, borders = planted
    out = tmp_path / "out"
    results = C._motif_spacing(str(res), str(primary), [str(f) for f in files], max_gap=60, output_dir=str(out), top_hist=2)
    printed = capsys.readouterr().out
    assert S.ModelSeq.calls == [("read_scores", 11, True), ("library_spacing", 11, 3, True, 60)]
    assert [st["motif"].name for st in results] == [S.FIXED, S.UNIFORM, S.PRIMARY]
    fixed, uniform, itself = results
    assert (fixed["quadrant"], fixed["gap"]) == (2, 3) and fixed["q_bh"] < 0.01 and fixed["pairs_in_bin"] >= 92
    assert fixed["log10_p_adj"] <= -131 and fixed["n_primary"] >= 400
    assert uniform["q_bh"] > 0.05 and uniform["n_pairs"] >= 150 and uniform["quadrant"] is not None
    assert itself["quadrant"] is None and itself["n_pairs"] <= 1 and itself["q_bh"] == 1.0
    # every figure again, from the model and the definitions
    Ws = [pwm_weights(S.consensus_counts(w), 1.0) for w in (S.PRIMARY, S.FIXED, S.UNIFORM)]
    ts = [pwm_threshold(W, 1e-4)[0] for W in Ws]
    Sg, R, n_primary, n_pair, n_far = S.np_library_spacing(seq, borders, Ws[0], ts[0], Ws, ts, True, 60)
    want = [C.best_bin(Sg[i], R[i], True) for i in range(3)]
    q = bh_qvalues([10.0 ** st["log10_p_adj"] for st in want]).tolist()
    for i, name in enumerate((S.PRIMARY, S.FIXED, S.UNIFORM)):
        got = next(st for st in results if st["motif"].name == name)
        assert got["threshold"] == ts[i] and got["q_bh"] == q[i] and got["n_primary"] == n_primary
        assert (got["n_pairs"], got["n_far"]) == (int(n_pair[i]), int(n_far[i]))
        np.testing.assert_array_equal(got["S"], Sg[i])
        np.testing.assert_array_equal(got["R"], R[i])
        for key in ("n_in_range", "n_bins", "quadrant", "gap", "pairs_in_bin", "log10_p", "log10_p_adj"):
            assert got[key] == want[i][key], key
    check_table(out / "spacing_rank.csv", results)
    assert (out / "skipped.csv").read_text() == "name,altname,source,reason\n"
    assert sorted(p.name for p in out.iterdir()) == ["skipped.csv", f"spacing_0_{S.FIXED}.csv", f"spacing_1_{S.UNIFORM}.csv", "spacing_rank.csv"]
    check_histogram(out / f"spacing_0_{S.FIXED}.csv", fixed)
    check_histogram(out / f"spacing_1_{S.UNIFORM}.csv", uniform)
    assert printed.count("\n") == 5 and printed.startswith(f"primary {S.PRIMARY}: at ")
    assert f"0 {S.FIXED}: at " in printed and "3 bases downstream on the same strand" in printed
    assert f"motif_spacing: 3 motifs ranked, 0 skipped, both strands: {out}" in printed

    # the forward strand, thresholds in bits, a MEME library with a motif to skip, the primary by name, the default directory
    S.ModelSeq.calls = []
    lib = str(LIB / "three.meme")
    fwd = C._motif_spacing(str(res), lib, [lib, str(files[1])], primary_name="M1_CAATCGATAGC", primary_min_score=9.0, min_score=8.0,
                           revcom_mode=False, max_gap=60, min_pairs=5)
    assert S.ModelSeq.calls == [("read_scores", 11, False), ("library_spacing", 11, 3, False, 60)]
    out2 = res / "motif_spacing"
    rows = check_table(out2 / "spacing_rank.csv", fwd)
    assert (out2 / "skipped.csv").read_text() == f"name,altname,source,reason\nM3_long,too_wide,{lib},width 40 outside 4..31\n"
    assert all(st["threshold"] == 800 and row["threshold_bits"] == "8.00" for st, row in zip(fwd, rows))
    assert sorted(st["motif"].name for st in fwd[:2]) == ["ACCTACGTA", "M2_ACCTACGTA"] and fwd[2]["motif"].name == "M1_CAATCGATAGC"
    by_name = {st["motif"].name: st for st in fwd}
    assert all(st["quadrant"] in (None, 0, 2) and not st["S"][1].any() and not st["S"][3].any() for st in fwd)
    Sg, R, n_primary, n_pair, n_far = S.np_library_spacing(seq, borders, Ws[0], 900, [Ws[1]], [800], False, 60)
    np.testing.assert_array_equal(by_name["ACCTACGTA"]["S"], Sg[0])
    np.testing.assert_array_equal(by_name["ACCTACGTA"]["R"], R[0])
    assert fwd[0]["n_primary"] == n_primary < 300 and all((st["quadrant"], st["gap"]) == (2, 3) for st in fwd[:2])
    # a second run writes the same bytes
    C._motif_spacing(str(res), lib, [lib, str(files[1])], primary_name="M1_CAATCGATAGC", primary_min_score=9.0, min_score=8.0,
                     revcom_mode=False, max_gap=60, min_pairs=5, output_dir=str(tmp_path / "again"))
    assert len(list(out2.iterdir())) == 5
    for p in out2.iterdir():
        assert (tmp_path / "again" / p.name).read_bytes() == p.read_bytes()


def test_no_bin_rows_rank_last_by_name(planted, tmp_path):
    """a primary threshold no window reaches: no primary read, no pair, p = 1, q = 1, empty bin fields, ranked by name"""
    from kmap_amd import spacing as C
    res, primary, files = planted[:3]
    results = C._motif_spacing(str(res), str(primary), [str(f) for f in files], primary_min_score=60.0, output_dir=str(tmp_path / "o"))
    assert [st["motif"].name for st in results] == sorted([S.PRIMARY, S.FIXED, S.UNIFORM])
    assert all(st["n_primary"] == 0 and st["n_pairs"] == 0 and st["quadrant"] is None and st["q_bh"] == 1.0 for st in results)
    lines = (tmp_path / "o" / "spacing_rank.csv").read_text().split("\n")[1:4]
    assert all(line.endswith(",0,0,0,0,,,,,,0.0,0,0.0,1.0") for line in lines)
    assert (tmp_path / "o" / f"spacing_0_{S.FIXED}.csv").read_text() == "side,strand,gap,pairs,expected\n"


def test_value_errors_come_before_the_library(planted, tmp_path, monkeypatch):
    import kmap_amd.motif_discovery as D
    from kmap_amd import _ffi
    from kmap_amd import spacing as C

    def no_lib():
        raise AssertionError("the library was loaded before the arguments were checked")

    class NoSeq:
        def __init__(self, *a):
            no_lib()
    monkeypatch.setattr(_ffi, "lib", no_lib)
    monkeypatch.setattr(D, "DeviceSeq", NoSeq)
    res, primary, files = planted[:3]
    out = tmp_path / "out"
    three = str(LIB / "three.meme")
    only_wide = tmp_path / "wide.meme"
    only_wide.write_text("MEME version 4\n\nMOTIF W\nletter-probability matrix: alength= 4 w= 32\n" + "0.25 0.25 0.25 0.25\n" * 32)
    zero = tmp_path / "zero.csv"
    zero.write_text("1,2,3,0\n1,2,3,4\n1,2,3,4\n1,2,3,4\n")
    ok = dict(primary_file=str(primary), library_files=[str(files[1])], output_dir=out)
    bad = [(dict(res_dir=tmp_path / "nowhere"), "config.toml"),
           (dict(library_files=[]), "no library file"),
           (dict(library_files=[str(tmp_path / "nowhere.meme")]), "nowhere.meme"),
           (dict(primary_file=str(tmp_path / "nowhere.csv")), "nowhere.csv"),
           (dict(primary_file=three), "holds 2 motifs.*exactly one"),
           (dict(primary_file=three, primary_name="M9"), "holds 0 motifs.*named M9"),
           (dict(primary_file=three, primary_name="M3_long"), "holds 0 motifs"),
           (dict(primary_file=str(only_wide)), "holds 0 motifs"),
           (dict(library_files=[three, str(LIB / "bad_alength.meme")]), "bad_alength.meme:11"),
           (dict(library_files=[str(only_wide)]), "none of the 1 motifs.*W: width 32"),
           (dict(library_files=[str(zero)], pseudocount=0.0), "zero.csv: motif zero: .*pseudocount"),
           (dict(primary_file=str(zero), pseudocount=0.0), "zero.csv: motif zero: .*pseudocount"),
           (dict(pseudocount=-1.0), "pseudocount"),
           (dict(p_value=float("nan")), "p_value"),
           (dict(min_score=float("inf")), "min_score"),
           (dict(primary_min_score=float("nan")), "min_score"),
           (dict(nsites_default=0), "nsites_default"),
           (dict(max_gap=-1), "max_gap -1"),
           (dict(max_gap=512), "max_gap 512"),
           (dict(max_gap=2.5), "max_gap 2.5"),
           (dict(min_pairs=0), "min_pairs"),
           (dict(top_hist=-1), "top_hist")]
    for change, word in bad:
        with pytest.raises(ValueError, match=word):
            C._motif_spacing(**{"res_dir": res, **ok, **change})
    assert not out.exists() and not (res / "motif_spacing").exists()
    with pytest.raises(AssertionError, match="the library was loaded"):
        C._motif_spacing(res, **ok)
    assert not out.exists()


def test_other_ranks_do_nothing(monkeypatch):
    from kmap_amd.spacing import _motif_spacing
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "1")
    assert _motif_spacing("nowhere", "nothing", []) is None


# ---- 5. the library's entry -----------------------------------------------------------------------------------------------------------
def test_symbol_registered_and_constants():
    from kmap_amd import _ffi, device_seq, spacing
    header = (ROOT / "include" / "kmap_hip.h").read_text()
    name = "kmap_readscore_spacing_library_dev"
    assert name in _ffi.exported_symbols() and f"int {name}(" in header
    res, args = _ffi._SIGS[name]
    assert res is _ffi.i32 and len(args) == 22
    declared = header[header.index(f"int {name}("):]
    declared = re.sub(r"/\*.*?\*/", "", declared[:declared.index(";")], flags=re.S)
    assert declared.count(",") + 1 == 22
    assert not name.startswith("kmap_pwm_")
    src = (ROOT / "kmap_amd" / "csrc" / "pwm_spacing.hip").read_text()
    batch = (ROOT / "kmap_amd" / "csrc" / "pwm_batch.h").read_text()
    assert int(re.search(r"constexpr int PB_MAX_MAT = (\d+);", batch).group(1)) == device_seq.LIBRARY_BATCH
    assert int(re.search(r"constexpr int PB_MAX_CHUNKS = (\d+);", batch).group(1)) == device_seq.LIBRARY_BATCH_CHUNKS
    assert int(re.search(r"constexpr int SP_MAX_GAP = (\d+);", src).group(1)) == device_seq.SPACING_MAX_GAP == spacing.MAX_GAP == 511


def test_library_spacing_checks_come_before_the_library(monkeypatch):
    from kmap_amd import _ffi
    from kmap_amd.device_seq import DeviceSeq, ReadScores

    def no_lib():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_ffi, "lib", no_lib)
    ds = object.__new__(DeviceSeq)
    ds.n_seq = 2
    rs, other = object.__new__(ReadScores), object.__new__(ReadScores)
    rs.n_seq, other.n_seq = 2, 3
    ok = np.zeros((4, 8), np.int32)
    good = dict(primary=rs, prim_width=9, prim_threshold=0, Ws=[ok], thresholds=[0], revcom=True, max_gap=10)
    for change, word in ((dict(Ws=[np.zeros((4, 3), np.int32)]), "width 3"),
                         (dict(Ws=[ok, np.zeros((4, 32), np.int32)], thresholds=[0, 0]), "matrix 1 has width 32"),
                         (dict(Ws=[np.zeros((3, 8), np.int32)]), "shape"), (dict(thresholds=[2 ** 31]), "int32"),
                         (dict(prim_threshold=-2 ** 31 - 1), "int32"), (dict(thresholds=[0, 1]), "1 matrices, 2 thresholds"),
                         (dict(prim_width=3), "primary matrix has width 3"), (dict(prim_width=32), "primary matrix has width 32"),
                         (dict(prim_width=8.5), "primary matrix has width 8.5"), (dict(max_gap=-1), "max_gap -1"),
                         (dict(max_gap=512), "max_gap 512"), (dict(max_gap=2.5), "max_gap 2.5"), (dict(max_gap=True), "max_gap True"),
                         (dict(primary=other), "ReadScores of these 2 reads"), (dict(primary=(1, 2, 3)), "ReadScores of these 2 reads")):
        with pytest.raises(ValueError, match="library_spacing: .*" + word):
            ds.library_spacing(**{**good, **change})
    with pytest.raises(AssertionError, match="the library was loaded"):
        ds.library_spacing(**good)


# ---- 6. the verb's command line -------------------------------------------------------------------------------------------------------
def test_cli_options_and_defaults(monkeypatch):
    from click.testing import CliRunner
    from kmap_amd import spacing
    from kmap_amd.cli import cli
    calls = []
    monkeypatch.setattr(spacing, "_motif_spacing", lambda *a: calls.append(a))
    runner = CliRunner()
    r = runner.invoke(cli, ["motif_spacing", "--res_dir", "D", "--primary_file", "P", "--library_file", "L"])
    assert r.exit_code == 0, r.output
    assert calls[-1] == ("D", "P", ["L"], None, 1e-4, None, None, 1.0, 20, None, 150, 10, 5, None)
    r = runner.invoke(cli, ["motif_spacing", "--res_dir", "D", "--primary_file", "P", "--primary_name", "N", "--library_file", "L",
                            "--library_file", "L2", "--p_value", "1e-3", "--primary_min_score", "9.5", "--min_score", "8.5",
                            "--pseudocount", "0.5", "--nsites_default", "100", "--revcom_mode", "False", "--max_gap", "60",
                            "--min_pairs", "3", "--top_hist", "0", "--output_dir", "O"])
    assert r.exit_code == 0, r.output
    assert calls[-1] == ("D", "P", ["L", "L2"], "N", 1e-3, 9.5, 8.5, 0.5, 100, False, 60, 3, 0, "O")
    for missing in (["--library_file", "L", "--primary_file", "P"], ["--res_dir", "D", "--primary_file", "P"],
                    ["--res_dir", "D", "--library_file", "L"]):
        assert runner.invoke(cli, ["motif_spacing"] + missing).exit_code == 2
    assert len(calls) == 2
    r = runner.invoke(cli, ["motif_spacing", "--help"])
    for opt in ("--res_dir", "--primary_file", "--primary_name", "--library_file", "--p_value", "--primary_min_score", "--min_score",
                "--pseudocount", "--nsites_default", "--revcom_mode", "--max_gap", "--min_pairs", "--top_hist", "--output_dir"):
        assert opt in r.output, opt
    assert "motif_spacing" in runner.invoke(cli, ["--help"]).output
    import kmap_amd.cli as cli_module
    assert "motif_spacing" in cli_module.__doc__ and "ten verbs the reference does not have" in cli_module.__doc__
    assert "motif_spacing" in (ROOT / "README.md").read_text()
