"""Erasing found sites on the host (kmap_amd/discover.py: discover_rounds; kmap_amd/erase.py): the rounds on the
numpy models (tests/_erase_model.py) for reads with a dominant and a weaker planted motif, one round against discover_core byte for
byte, the early stops, the argument checks, the new entry's prototype and the two command lines.  No GPU."""
import re
from pathlib import Path

import numpy as np
import pytest

from tests import _discover_model as DM
from tests import _erase_model as EM
from tests._refine_model import encode_fasta_np, np_hits
from tests._shuffle_model import shuffle_array

ROOT = Path(__file__).resolve().parent.parent
COMPLEMENT = str.maketrans("ACGT", "TGCA")
READS_SEED = 2201                                            # of planted_reads; the condition below was checked on the models alone


def revcom_text(s):
    return s.translate(COMPLEMENT)[::-1]


# ---- 1. the model itself ----------------------------------------------------------------------------------------------------------
def test_model_erases_the_cover_of_every_hit():
    """np_erase against an explicit loop over the hits: a small array, two matrices, both strand settings"""
    from tests._refine_model import asym_matrix, make_reads, window_scores
    rng = np.random.default_rng(2200)
    seq, borders = make_reads([30, 0, 7, 45, 12, 60], rng, frac_invalid=0.03)
    Ws = [asym_matrix(5, rng), asym_matrix(9, rng)]
    ts = []
    for W in Ws:                                             # the eighth best forward score: a few hits on either setting
        valid, fwd, _ = window_scores(seq, W)
        ts.append(int(np.sort(fwd[valid])[-8]))
    for revcom in (True, False):
        erased, n_hits, n_cov, n_new = EM.np_erase(seq, borders, Ws, ts, revcom)
        want = seq.copy()
        for m, (W, t) in enumerate(zip(Ws, ts)):
            p = np_hits(seq, borders, W, t, revcom)[2]
            assert len(p) == n_hits[m] and n_hits[m] > 0
            cover = set()
            for s in p.tolist():
                cover |= set(range(s, s + W.shape[1]))
                want[s:s + W.shape[1]] = 255
            assert len(cover) == n_cov[m]
        np.testing.assert_array_equal(erased, want)
        assert n_new == int(((want == 255) & (seq != 255)).sum()) > 0
        again = EM.np_erase(erased, borders, Ws, ts, revcom)  # every hit touched an erased position: nothing is left
        assert not again[1].any() and again[3] == 0
        np.testing.assert_array_equal(again[0], erased)
    words = EM.mask_words(np.array([0, 255, 1] + [2] * 14, np.uint8))
    assert words.tolist() == [0x4000, 0x7FFF]


# ---- 2. the rounds on the models --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def planted():
    seq, borders = EM.planted_reads(READS_SEED)
    cseq = shuffle_array(seq, 2, 0)
    for a in (seq, borders, cseq):
        a.setflags(write=False)
    assert len(borders) == 400 and (borders[:, 1] - borders[:, 0] == 40).all()
    return seq, borders, cseq


def run_rounds(planted, R, n_seeds=3, **kw):
    from kmap_amd.discover import discover_rounds
    seq, borders, cseq = planted
    mr = EM.ModelReads(seq, borders, cseq, borders, True)
    matches = []

    def match_fn(*args):
        matches.append(len(args[0]))
        return DM.match_fn(*args)
    res, log = discover_rounds(mr.seeds_fn(8, 2, n_seeds), mr.counts_fn, mr.erase_fn, mr.hist_fn(), match_fn, True, R, **kw)
    return res, log, mr, matches


def rep_texts(res):
    from kmap_amd.pwm import pwm_consensus
    return [(pwm_consensus(st["counts"]), st) for st in sorted(res, key=lambda st: st["rank"]) if st["is_representative"]]


def holds(text, word):
    return word in text or word in revcom_text(text)


def test_one_round_misses_the_weaker_motif(planted):
    res, log, mr, matches = run_rounds(planted, 1)
    assert len(res) == 3 and log == [] and mr.seed_calls == [1] and mr.erase_calls == [] and matches == [3]
    assert {st["family"] for st in res} == {0} and all(st["round"] == 1 for st in res)
    reps = rep_texts(res)
    assert len(reps) == 1 and "CCTACGTA" in reps[0][0]
    assert not any("CTGATGCA" in t or "TGCATCAG" in t for t, _ in reps)
    assert not any(holds(st["seed"], "TGATGC") for st in res)        # every seed is a variant of the dominant word


def test_two_rounds_find_it(planted):
    from kmap_amd.library import bh_qvalues
    from kmap_amd.pwm import pwm_threshold, pwm_weights
    one = run_rounds(planted, 1)[0]
    res, log, mr, matches = run_rounds(planted, 2)
    assert len(res) == 6 and mr.seed_calls == [1, 2] and mr.erase_calls == [1]
    assert matches == [3, 6]                                 # round 1's own families, then one call over the union
    # round 1 is the run without erasure, seed by seed, but for what is computed over all seeds
    for a, b in zip(one, res[:3]):
        np.testing.assert_array_equal(a["counts"], b["counts"])
        assert (a["seed"], a["name"], a["status"], a["trace"], a["mw_z"], a["log10_p"]) == \
            (b["seed"], b["name"], b["status"], b["trace"], b["mw_z"], b["log10_p"])
    assert [st["round"] for st in res] == [1, 1, 1, 2, 2, 2]
    assert [st["seed_rank"] for st in res] == list(range(6)) and [st["name"].split("_")[0] for st in res] == [f"seed{i}" for i in range(6)]
    assert sorted(st["rank"] for st in res) == list(range(6))
    z = [st["mw_z"] for st in sorted(res, key=lambda st: st["rank"])]
    assert z == sorted(z, reverse=True)
    want_q = bh_qvalues([10.0 ** st["log10_p"] for st in res]).tolist()
    assert [st["q_bh"] for st in res] == want_q and res[0]["q_bh"] > one[0]["q_bh"]      # over 6 seeds, not 3
    reps = rep_texts(res)
    assert len(reps) == 2 and "CCTACGTA" in reps[0][0] and reps[0][1]["round"] == 1
    second = reps[1]
    assert ("CTGATGCA" in second[0] or "TGCATCAG" in second[0]) and second[1]["round"] == 2
    assert {st["family"] for st in res[:3]} == {reps[0][1]["family"]} and {st["family"] for st in res[3:]} == {second[1]["family"]}
    # the log: round 1's representative at its p-value threshold, the model's own numbers
    assert len(log) == 1 and log[0]["round"] == 1 and len(log[0]["rows"]) == 1
    st = next(s for s in res[:3] if s["is_representative"])
    W = pwm_weights(st["counts"], 1.0)
    t = pwm_threshold(W, 1e-4)[0]
    seq, borders, cseq = planted
    _, fh, fc, f_new = EM.np_erase(seq, borders, [W], [t], True)
    _, ch, cc, c_new = EM.np_erase(cseq, borders, [W], [t], True)
    assert log[0]["rows"][0] == (st["name"], t, int(fh[0]), int(fc[0]), int(ch[0]), int(cc[0]))
    assert (log[0]["fg_new"], log[0]["control_new"]) == (f_new, c_new) and f_new > 1000 > c_new
    assert int((mr.work == 255).sum()) == int((seq == 255).sum()) + f_new
    # the evaluation saw the original reads: the second motif's matrix scores reads the erasure did not touch
    assert second[1]["mw_z"] > 3 and second[1]["n_fg"] == 400


def test_files_of_two_rounds(planted, tmp_path):
    from kmap_amd import discover as D
    res, log, _, _ = run_rounds(planted, 2)
    D.write_discovery(tmp_path, res, 1.0, True, log)
    rank = (tmp_path / D.RANK_FILE).read_text().split("\n")
    assert rank[0] + "\n" == D.RANK_HEADER[:-1] + ",round\n" and len(rank) == 8
    by_name = {ln.split(",")[1]: ln.split(",")[-1] for ln in rank[1:-1]}
    assert by_name == {st["name"]: str(st["round"]) for st in res}
    assert all(D.rank_line(st, 1.0, True)[:-1] + f",{st['round']}" in rank for st in res)
    trace = (tmp_path / D.TRACE_FILE).read_text().split("\n")
    assert trace[0] + "\n" == D.TRACE_HEADER[:-1] + ",round\n" and len(trace) == 2 + sum(st["iterations"] for st in res)
    assert all(ln.split(",")[-1] == str(res[int(ln.split(",")[0])]["round"]) for ln in trace[1:-1])
    erase = (tmp_path / D.ERASE_FILE).read_text().split("\n")
    assert erase[0] == "round,name,threshold,fg_hits,fg_covered,control_hits,control_covered"
    assert erase[1] == "1," + ",".join(str(x) for x in log[0]["rows"][0])
    assert erase[2:] == ["round,fg_new,control_new", f"1,{log[0]['fg_new']},{log[0]['control_new']}", ""]
    # an empty log still marks a run that asked for rounds
    D.write_discovery(tmp_path / "none", res, 1.0, True, [])
    assert (tmp_path / "none" / D.ERASE_FILE).read_text() == D.ERASE_HEADER + D.ERASE_TOTALS_HEADER


def test_one_round_is_discover_core_byte_for_byte(tmp_path):
    from kmap_amd import discover as D
    seq, borders = encode_fasta_np(ROOT / "tests" / "golden" / "test.fa")
    cseq = shuffle_array(seq, 2, 0)
    seeds = DM.top_seeds(seq, borders, cseq, borders, 8, True, 2, 4)
    core = D.discover_core(seeds, DM.counts_fn(seq, borders, True), DM.hist_fn(seq, borders, cseq, borders, True), DM.match_fn, True)
    mr = EM.ModelReads(seq, borders, cseq, borders, True)
    res, log = D.discover_rounds(mr.seeds_fn(8, 2, 4), DM.counts_fn(seq, borders, True), mr.erase_fn, mr.hist_fn(), DM.match_fn, True, 1)
    assert log == [] and mr.erase_calls == [] and len(res) == 4
    D.write_discovery(tmp_path / "core", core, 1.0, True)
    D.write_discovery(tmp_path / "rounds", res, 1.0, True)
    for name in (D.RANK_FILE, D.TRACE_FILE, D.MEME_FILE):
        assert (tmp_path / "core" / name).read_bytes() == (tmp_path / "rounds" / name).read_bytes(), name
    assert (tmp_path / "rounds" / D.RANK_FILE).read_text().startswith(D.RANK_HEADER)
    assert not (tmp_path / "rounds" / D.ERASE_FILE).exists()
    assert sorted(p.name for p in (tmp_path / "core" / D.MATRIX_DIR).iterdir()) == \
        sorted(p.name for p in (tmp_path / "rounds" / D.MATRIX_DIR).iterdir())


# ---- 3. the early stops -----------------------------------------------------------------------------------------------------------
def test_early_stops(planted):
    from kmap_amd.discover import discover_rounds
    seq, borders, cseq = planted
    # (a) a later round without a seed ends the run; round 1 without one is the error
    mr = EM.ModelReads(seq, borders, cseq, borders, True)
    first = mr.seeds_fn(8, 2, 3)
    res, log = discover_rounds(lambda r: first(r) if r == 1 else [], mr.counts_fn, mr.erase_fn, mr.hist_fn(), DM.match_fn, True, 5)
    assert len(res) == 3 and len(log) == 1 and mr.erase_calls == [1] and all(st["round"] == 1 for st in res)
    with pytest.raises(ValueError, match="no seed"):
        discover_rounds(lambda r: [], mr.counts_fn, mr.erase_fn, mr.hist_fn(), DM.match_fn, True, 3)
    # (b) nothing to erase: no matrix of the round was built from a selected window
    mr = EM.ModelReads(seq, borders, cseq, borders, True)

    def no_window(Ws, ts):
        z = np.zeros(len(Ws), np.int64)
        return [np.zeros((4, W.shape[1]), np.int64) for W in Ws], z, z
    res, log = discover_rounds(mr.seeds_fn(8, 2, 3), no_window, mr.erase_fn, mr.hist_fn(), DM.match_fn, True, 4)
    assert len(res) == 3 and {st["status"] for st in res} == {"no_hits"} and not any(st["n_selected"] for st in res)
    assert log == [] and mr.erase_calls == [] and mr.seed_calls == [1]
    # (c) an erasure that takes no position from the reads ends the run: the next round would be this one again
    mr = EM.ModelReads(seq, borders, cseq, borders, True)
    calls = []

    def erase_nothing(Ws, ts):
        calls.append(len(Ws))
        z = np.zeros(len(Ws), np.int64)
        return z, z, 0, z, z, 0
    res, log = discover_rounds(mr.seeds_fn(8, 2, 3), mr.counts_fn, erase_nothing, mr.hist_fn(), DM.match_fn, True, 4)
    assert calls == [1] and len(res) == 3 and len(log) == 1 and log[0]["fg_new"] == 0 and mr.seed_calls == [1]
    # (d) the last round erases nothing
    res, log, mr, _ = run_rounds(planted, 2)
    assert mr.erase_calls == [1] and len(log) == 1


# ---- 4. argument errors -----------------------------------------------------------------------------------------------------------
def test_erase_rounds_errors():
    from kmap_amd.discover import check_arguments, discover_rounds
    for bad in (0, 17, -1, 1.5, True):
        with pytest.raises(ValueError, match="erase_rounds .* outside 1..16"):
            check_arguments(erase_rounds=bad)
        with pytest.raises(ValueError, match="erase_rounds .* outside 1..16"):
            discover_rounds(None, None, None, None, None, True, bad)
    check_arguments(erase_rounds=1)
    check_arguments(erase_rounds=16)


def test_verb_argument_errors_come_first(tmp_path, monkeypatch):
    from kmap_amd import _ffi
    from kmap_amd import discover as D
    from kmap_amd import erase as E
    from tests._sites_model import write_planted
    monkeypatch.delenv("WORLD_SIZE", raising=False)

    def no_lib():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_ffi, "lib", no_lib)
    res, ctl, *_ = write_planted(tmp_path)
    with pytest.raises(ValueError, match="erase_rounds 0 outside 1..16"):
        D._discover_pwms(str(res), str(ctl), erase_rounds=0, output_dir=str(tmp_path / "out"))
    with pytest.raises(ValueError, match="erase_rounds 17 outside 1..16"):
        D._discover_pwms(str(res), str(ctl), erase_rounds=17, output_dir=str(tmp_path / "out"))
    assert not (tmp_path / "out").exists()
    lib_file = ROOT / "tests" / "golden" / "report_testfa" / "cntmat_motif1_ACCTACGTA.csv"
    out = tmp_path / "erased.fa"
    ok = dict(res_dir=str(res), library_files=[str(lib_file)], output_file=str(out))
    bad = [(dict(library_files=[]), "erase_pwm_sites: no library file given"),
           (dict(library_files=[str(tmp_path / "missing.meme")]), "missing.meme"),
           (dict(res_dir=str(tmp_path / "nowhere")), "not a result directory"),
           (dict(p_value=float("nan")), "p_value"),
           (dict(pseudocount=-1.0), "pseudocount"),
           (dict(min_score=float("nan")), "min_score")]
    for change, word in bad:
        with pytest.raises(ValueError, match=word):
            E._erase_pwm_sites(**{**ok, **change})
    assert not out.exists() and not (tmp_path / E.INFO_FILE).exists()
    with pytest.raises(AssertionError, match="the library was loaded"):
        E._erase_pwm_sites(**ok)
    assert not out.exists()
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "1")
    assert E._erase_pwm_sites("nowhere", []) is None


def test_erase_sites_checks_come_before_the_library(monkeypatch):
    from kmap_amd import _ffi
    from kmap_amd.device_seq import DeviceSeq

    def no_lib():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_ffi, "lib", no_lib)
    ds = object.__new__(DeviceSeq)
    ds.n_seq = 2
    ok = np.zeros((4, 8), np.int32)
    for Ws, ts, word in (([np.zeros((4, 3), np.int32)], [0], "width 3"),
                         ([ok, np.zeros((4, 32), np.int32)], [0, 0], "matrix 1 has width 32"),
                         ([np.zeros((3, 8), np.int32)], [0], "shape"), ([ok], [2 ** 31], "int32"), ([ok], [-2 ** 31 - 1], "int32"),
                         ([ok], [0, 1], "1 matrices, 2 thresholds"), ([ok, ok], [0], "2 matrices, 1 thresholds")):
        for use_work in (True, False):
            with pytest.raises(ValueError, match="^erase_sites: .*" + word):
                ds.erase_sites(Ws, ts, True, use_work=use_work)


# ---- 5. the entry's prototype -----------------------------------------------------------------------------------------------------
def test_prototype_has_no_stream_and_says_so():
    from kmap_amd import _ffi
    from tests import _stream_order as SO
    header = (ROOT / "include" / "kmap_hip.h").read_text()
    name = "kmap_erase_pwm_sites_dev"
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int " + name + r"\(([^;]*)\);", header, re.S)
    assert m, "the prototype with its comment in front"
    comment, params = " ".join(m.group(1).split()), " ".join(m.group(2).split())
    assert "stream" not in re.sub(r"/\*.*?\*/", "", params) and "void *" not in params
    assert "no stream argument" in comment and "null stream" in comment and "blocking" in comment
    assert name not in SO.stream_entries(header)
    assert [p.strip().split()[-1].lstrip("*") for p in re.sub(r"/\*.*?\*/", "", params).split(",")] == \
        ["codes_dev", "inval_eval_dev", "n", "n_mat", "widths", "weights", "thresholds", "revcom", "inval_out_dev", "n_hits",
         "n_covered", "n_new"]
    assert name in _ffi.exported_symbols()
    res, args = _ffi._SIGS[name]
    assert res is _ffi.i32 and len(args) == 12
    src = (ROOT / "kmap_amd" / "csrc" / "pwm_erase.hip").read_text()
    assert f"int {name}(" in src and "pwm_erase_kernel" in src and "erase_apply_kernel" in src
    for shared in ("build_table", "win_bits", "win_valid", "win_score", "load_grp<true>"):
        assert shared in src, shared                         # the scores are scan_pwm's by construction


# ---- 6. the command lines ---------------------------------------------------------------------------------------------------------
def test_cli_options_and_defaults(monkeypatch):
    from click.testing import CliRunner
    from kmap_amd import discover, erase
    from kmap_amd.cli import cli
    calls = []
    monkeypatch.setattr(discover, "_discover_pwms", lambda *a: calls.append(a))
    monkeypatch.setattr(erase, "_erase_pwm_sites", lambda *a: calls.append(a))
    runner = CliRunner()
    base = ["discover_pwms", "--res_dir", "D", "--control_fasta_file", "C.fa"]
    r = runner.invoke(cli, base + ["--erase_rounds", "3"])
    assert r.exit_code == 0, r.output
    assert calls[-1] == ("D", "C.fa", 8, 64, 1, 20, 2, 2, 1e-4, 1.0, None, 20, 5, 0.01, None, 3)
    r = runner.invoke(cli, base + ["--erase_rounds", "1"])
    assert r.exit_code == 0 and calls[-1] == ("D", "C.fa", 8, 64, 1, 20, 2, 2, 1e-4, 1.0, None, 20, 5, 0.01, None)
    assert runner.invoke(cli, base + ["--erase_rounds", "two"]).exit_code == 2
    assert "--erase_rounds" in runner.invoke(cli, ["discover_pwms", "--help"]).output
    r = runner.invoke(cli, ["erase_pwm_sites", "--res_dir", "D", "--library_file", "L.meme"])
    assert r.exit_code == 0, r.output
    assert calls[-1] == ("D", ["L.meme"], 1e-4, None, 1.0, 20, None, None)
    r = runner.invoke(cli, ["erase_pwm_sites", "--res_dir", "D", "--library_file", "L.meme", "--library_file", "M.csv", "--p_value", "1e-3",
                            "--min_score", "7.5", "--pseudocount", "0.5", "--nsites_default", "30", "--revcom_mode", "False",
                            "--output_file", "O.fa"])
    assert r.exit_code == 0, r.output
    assert calls[-1] == ("D", ["L.meme", "M.csv"], 1e-3, 7.5, 0.5, 30, False, "O.fa")
    for missing in (["--library_file", "L"], ["--res_dir", "D"]):
        assert runner.invoke(cli, ["erase_pwm_sites"] + missing).exit_code == 2
    r = runner.invoke(cli, ["erase_pwm_sites", "--help"])
    for opt in ("--res_dir", "--library_file", "--p_value", "--min_score", "--pseudocount", "--nsites_default", "--revcom_mode",
                "--output_file"):
        assert opt in r.output, opt
    assert "erase_pwm_sites" in runner.invoke(cli, ["--help"]).output
    import kmap_amd.cli as cli_module
    doc = cli_module.__doc__
    assert doc.index("A twelfth, `discover_pwms`") < doc.index("--erase_rounds") < doc.index("A thirteenth, `erase_pwm_sites`")
    readme = (ROOT / "README.md").read_text()
    assert "erase_pwm_sites" in readme and "--erase_rounds" in readme


def test_erase_info_file(tmp_path):
    from types import SimpleNamespace

    from kmap_amd import erase as E
    C = np.zeros((4, 6), np.int64)
    C[[0, 1, 2, 3, 0, 1], np.arange(6)] = 9
    motifs = [SimpleNamespace(name="m1", counts=C), SimpleNamespace(name="m2", counts=C[:, :5])]
    E.write_erase_info(tmp_path / E.INFO_FILE, motifs, [700, 650], np.array([3, 5]), np.array([17, 25]), 40)
    assert (tmp_path / E.INFO_FILE).read_text() == ("name,width,consensus,threshold,hits,covered\nm1,6,ACGTAC,700,3,17\nm2,5,ACGTA,650,5,25\n"
                                                    "total,,,,8,40\n")
