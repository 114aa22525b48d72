"""Host side of what the library verbs share (no GPU): device_seq._pack_library, the one place where a list of weight matrices becomes
the arrays of the batched entry points (csrc/pwm_batch.h), and library.py's load_library, open_read_sets and write_skipped, the
prologue and epilogue of rank_motif_library, motif_centrality, motif_spacing and motif_cooccurrence.  Every error text is asked for
under two caller names: the helpers speak in the name of whoever calls them."""
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
GOLD = ROOT / "tests" / "golden"
LIB = GOLD / "library"
MOTIF1 = GOLD / "report_testfa" / "cntmat_motif1_ACCTACGTA.csv"
CALLERS = ("library_sites", "some_later_verb")


# ---- 1. _pack_library -----------------------------------------------------------------------------------------------------------------
def test_pack_library_arrays():
    from kmap_amd.device_seq import _pack_library
    rng = np.random.default_rng(2201)
    Ws = [rng.integers(-900, 900, (4, w)) for w in (4, 31, 9)]                  # int64 in, a list of lists among them
    n_mat, widths, weights, thr = _pack_library("x", [Ws[0], Ws[1].tolist(), Ws[2]], [5, -2 ** 31, 2 ** 31 - 1])
    assert n_mat == 3 and widths.dtype == weights.dtype == thr.dtype == np.int32
    assert widths.tolist() == [4, 31, 9] and weights.shape == (3, 4, 32) and thr.tolist() == [5, -2 ** 31, 2 ** 31 - 1]
    assert weights.flags["C_CONTIGUOUS"] and widths.flags["C_CONTIGUOUS"]
    for m, W in enumerate(Ws):
        np.testing.assert_array_equal(weights[m, :, :W.shape[1]], W)
        assert not weights[m, :, W.shape[1]:].any()                             # zeros behind the width: the entry points' rule
    n_mat, widths, weights, thr = _pack_library("x", Ws)                        # without thresholds
    assert n_mat == 3 and thr is None and widths.tolist() == [4, 31, 9]
    n_mat, widths, weights, thr = _pack_library("x", [], [])
    assert n_mat == 0 and widths.shape == (0,) and weights.shape == (0, 4, 32) and thr.shape == (0,)


@pytest.mark.parametrize("who", CALLERS)
def test_pack_library_errors_under_the_callers_name(who):
    from kmap_amd.device_seq import _pack_library
    ok = np.zeros((4, 8), np.int32)
    bad = [(([ok, np.zeros((3, 8))], [0, 0]), f"{who}: weights of shape (3, 8), expected (4, width) with rows A, C, G, T"),
           (([ok, np.zeros(8)], [0, 0]), f"{who}: weights of shape (8,), expected (4, width) with rows A, C, G, T"),
           (([ok], [2 ** 31]), f"{who}: threshold {2 ** 31} does not fit int32"),
           (([ok], [-2 ** 31 - 1]), f"{who}: threshold {-2 ** 31 - 1} does not fit int32"),
           (([ok, ok], [0]), f"{who}: 2 matrices, 1 thresholds"),
           (([ok], [0, 0, 0]), f"{who}: 1 matrices, 3 thresholds"),
           (([ok, np.zeros((4, 3), np.int32)], [0, 0]), f"{who}: matrix 1 has width 3, outside 4..31"),
           (([np.zeros((4, 32), np.int32)], None), f"{who}: matrix 0 has width 32, outside 4..31")]
    for args, text in bad:
        with pytest.raises(ValueError, match="^" + re.escape(text) + "$"):
            _pack_library(who, *args)


def test_the_five_methods_pack_through_it(monkeypatch):
    """every batched method of DeviceSeq raises _pack_library's texts under its own name, before the library is loaded"""
    from kmap_amd import _ffi
    from kmap_amd.device_seq import DeviceSeq, ReadScores

    def no_lib():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_ffi, "lib", no_lib)
    ds = object.__new__(DeviceSeq)                                              # no device: the checks need none
    ds.n_seq = 0
    narrow, ok = np.zeros((4, 3), np.int32), np.zeros((4, 8), np.int32)
    calls = {"library_histograms": lambda Ws: ds.library_histograms(Ws, [0] * len(Ws), [1] * len(Ws), True),
             "library_sites": lambda Ws: ds.library_sites(Ws, [0] * len(Ws), True, max_len=10),
             "library_counts": lambda Ws: ds.library_counts(Ws, [0] * len(Ws), True),
             "library_spacing": lambda Ws: ds.library_spacing(object.__new__(ReadScores), 8, 0, Ws, [0] * len(Ws), True),
             "library_presence": lambda Ws: ds.library_presence(Ws, [0] * len(Ws), True)}
    for who, call in calls.items():
        with pytest.raises(ValueError, match=re.escape(f"{who}: matrix 1 has width 3, outside 4..31")):
            call([ok, narrow])
        with pytest.raises(ValueError, match=re.escape(f"{who}: weights of shape (8,), expected (4, width)")):
            call([np.zeros(8)])


# ---- 2. load_library ------------------------------------------------------------------------------------------------------------------
def test_load_library_motifs_weights_and_plans():
    from kmap_amd.library import load_library, read_motif_library
    from kmap_amd.pwm import pwm_threshold, pwm_weights
    files = [str(LIB / "three.meme"), str(MOTIF1)]
    motifs, skipped, Ws, plans = load_library("v", files, 20, 1.0, 1e-4)
    assert [m.name for m in motifs] == ["M1_CAATCGATAGC", "M2_ACCTACGTA", "cntmat_motif1_ACCTACGTA"]
    assert [m.name for m in skipped] == ["M3_long"] and "width 40" in skipped[0].skip
    assert len(Ws) == len(plans) == 3
    for m, W, plan in zip(motifs, Ws, plans):
        np.testing.assert_array_equal(W, pwm_weights(m.counts, 1.0))
        assert plan == tuple(pwm_threshold(W, 1e-4)) and plan[1] < plan[0] <= plan[2]
    # pseudocount, p_value and nsites_default reach the weights, the thresholds and the reader
    _, _, Ws2, plans2 = load_library("v", files, 40, 0.5, 1e-2)
    want = [m for f in files for m in read_motif_library(f, 40) if m.skip is None]
    for m, W, plan in zip(want, Ws2, plans2):
        np.testing.assert_array_equal(W, pwm_weights(m.counts, 0.5))
        assert plan == tuple(pwm_threshold(W, 1e-2))
    assert plans2[1][0] < plans[1][0] or not np.array_equal(Ws2[1], Ws[1])


def test_load_library_fixed_threshold_replaces_every_t():
    from kmap_amd.library import load_library
    files = [str(LIB / "three.meme"), str(MOTIF1)]
    _, _, Ws, plans = load_library("v", files, 20, 1.0, 1e-4)
    motifs, skipped, Ws_f, fixed = load_library("v", files, 20, 1.0, 1e-4, t_fixed=-123)
    assert [p[0] for p in fixed] == [-123] * 3 and all(p[0] != -123 for p in plans)
    assert [p[1:] for p in fixed] == [p[1:] for p in plans]                     # the score range stays the matrix's own
    assert len(motifs) == 3 and len(skipped) == 1 and all(np.array_equal(a, b) for a, b in zip(Ws, Ws_f))
    assert [p[0] for p in load_library("v", files, 20, 1.0, 1e-4, t_fixed=0)[3]] == [0, 0, 0]      # 0 is a threshold, not "none"


def test_load_library_veto_and_skipped_in_file_order(tmp_path):
    """the veto sees (W, t, lo, hi) of every motif that has weights and its reason becomes the motif's skip; the skipped motifs come
    in file order whichever of the two reasons left them out, and a motif that is already skipped is not offered to the veto"""
    from kmap_amd.library import load_library
    from kmap_amd.pwm import pwm_threshold
    second = tmp_path / "second.meme"
    second.write_text((LIB / "three.meme").read_text().replace("MOTIF M", "MOTIF N"))
    files = [str(LIB / "three.meme"), str(MOTIF1), str(second)]
    seen = []

    def veto(W, t, lo, hi):
        seen.append(W.shape[1])
        assert (t, lo, hi) == tuple(pwm_threshold(W, 1e-4))
        return f"width {W.shape[1]} is vetoed" if W.shape[1] == 9 else None
    motifs, skipped, Ws, plans = load_library("v", files, 20, 1.0, 1e-4, veto=veto)
    assert seen == [11, 9, 9, 11, 9]                                            # the two of 40 columns never had weights
    assert [m.name for m in motifs] == ["M1_CAATCGATAGC", "N1_CAATCGATAGC"] and [W.shape[1] for W in Ws] == [11, 11] and len(plans) == 2
    assert [m.name for m in skipped] == ["M2_ACCTACGTA", "M3_long", "cntmat_motif1_ACCTACGTA", "N2_ACCTACGTA", "N3_long"]
    assert [m.skip for m in skipped] == ["width 9 is vetoed", skipped[1].skip, "width 9 is vetoed", "width 9 is vetoed", skipped[4].skip]
    assert "width 40" in skipped[1].skip and "width 40" in skipped[4].skip


@pytest.mark.parametrize("who", ("motif_centrality", "some_later_verb"))
def test_load_library_errors(who, tmp_path):
    from kmap_amd.library import load_library
    only_wide = tmp_path / "wide.meme"
    only_wide.write_text("MEME version 4\n\nMOTIF W\nletter-probability matrix: alength= 4 w= 32\n" + "0.25 0.25 0.25 0.25\n" * 32)
    zero = tmp_path / "zero.csv"
    zero.write_text("1,2,3,0\n1,2,3,4\n1,2,3,4\n1,2,3,4\n")
    three = str(LIB / "three.meme")
    with pytest.raises(ValueError, match="^" + re.escape(f"{who}: none of the 1 motifs of the library can be scored (the first: W: width 32 "
                                                         "outside 4..31)") + "$"):
        load_library(who, [str(only_wide)], 20, 1.0, 1e-4)
    with pytest.raises(ValueError, match="^" + re.escape(f"{who}: none of the 3 motifs of the library can be scored (the first: "
                                                         "M1_CAATCGATAGC: no)") + "$"):
        load_library(who, [three], 20, 1.0, 1e-4, veto=lambda W, t, lo, hi: "no")
    with pytest.raises(ValueError, match="^" + re.escape(f"{zero}: motif zero: ") + ".*pseudocount"):      # the motif's name, not the caller's
        load_library(who, [three, str(zero)], 20, 0.0, 1e-4)
    with pytest.raises(ValueError, match=re.escape(f"{three}: motif M1_CAATCGATAGC: ") + ".*p_value"):
        load_library(who, [three], 20, 1.0, float("nan"))
    with pytest.raises(ValueError, match="bad_alength.meme:11"):
        load_library(who, [three, str(LIB / "bad_alength.meme")], 20, 1.0, 1e-4)
    with pytest.raises(ValueError, match="nowhere.meme is missing"):
        load_library(who, [str(tmp_path / "nowhere.meme")], 20, 1.0, 1e-4)
    with pytest.raises(ValueError, match="nsites_default 0 < 1"):
        load_library(who, [three], 0, 1.0, 1e-4)


# ---- 3. the read sets and skipped.csv ---------------------------------------------------------------------------------------------------
def test_open_read_sets_opens_in_order_and_closes_both(monkeypatch):
    import kmap_amd.kmer_count as K
    import kmap_amd.motif_discovery as D
    from kmap_amd.library import open_read_sets
    log = []

    class Seq:
        def __init__(self, seq, borders):
            if seq == "broken":
                raise ValueError("no such reads")
            self.name = seq
            log.append(("open", seq, borders))

        def close(self):
            log.append(("close", self.name))
    monkeypatch.setattr(D, "DeviceSeq", Seq)
    monkeypatch.setattr(K, "load_array_pickle", lambda path: f"<{path}>")
    monkeypatch.setattr(K, "encode_fasta", lambda path: ("broken" if "broken" in path else f"seq of {path}", f"borders of {path}"))
    with open_read_sets("s", "b") as (fg, ctl):
        assert fg.name == "<s>" and ctl is None
    assert log == [("open", "<s>", "<b>"), ("close", "<s>")]
    del log[:]
    with pytest.raises(RuntimeError, match="inside"):
        with open_read_sets("s", "b", Path("c.fa")) as (fg, ctl):
            assert (fg.name, ctl.name) == ("<s>", "seq of c.fa")
            raise RuntimeError("inside")
    assert log == [("open", "<s>", "<b>"), ("open", "seq of c.fa", "borders of c.fa"), ("close", "seq of c.fa"), ("close", "<s>")]
    del log[:]
    with pytest.raises(ValueError, match="no such reads"):                     # the control fails to open: the foreground is closed
        with open_read_sets("s", "b", "broken.fa"):
            raise AssertionError("not reached")
    assert log == [("open", "<s>", "<b>"), ("close", "<s>")]


def test_write_skipped(tmp_path):
    from kmap_amd.library import SKIPPED_HEADER, LibraryMotif, write_skipped
    write_skipped(tmp_path, [])
    assert (tmp_path / "skipped.csv").read_text() == SKIPPED_HEADER == "name,altname,source,reason\n"
    write_skipped(tmp_path, [LibraryMotif("a,b", "alt", "lib.meme", skip="width 40 outside 4..31"),
                             LibraryMotif("c", "", "dir/x.csv", skip="scores from -5 to 7: too many, really")])
    assert (tmp_path / "skipped.csv").read_text() == (SKIPPED_HEADER + "a_b,alt,lib.meme,width 40 outside 4..31\n"
                                                      "c,,dir/x.csv,scores from -5 to 7: too many_ really\n")
