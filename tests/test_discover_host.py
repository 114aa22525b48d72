"""discover_pwms on the host (kmap_amd/discover.py): the seed matrix and its first threshold against an
explicit enumeration by Hamming distance, the lockstep refinement against refine.refine_matrix, the whole core on the numpy models
(tests/_discover_model.py) for tests/golden/test.fa, the MEME round trip, the argument checks, the registration of the new entry
and the command line.  No GPU."""
import re
from pathlib import Path

import numpy as np
import pytest

from tests import _discover_model as DM
from tests._refine_model import encode_fasta_np, model_count_fn, np_hits
from tests._shuffle_model import shuffle_array

ROOT = Path(__file__).resolve().parent.parent
COMPLEMENT = str.maketrans("ACGT", "TGCA")


def revcom_text(s):
    return s.translate(COMPLEMENT)[::-1]


# ---- 1. the seed matrix and the first threshold -----------------------------------------------------------------------------------
def seeded_reads(seed_kmer, rng):
    """~200 reads of 40 bases, a 255 behind each, a few invalid bases; the seed, its reverse complement and copies of either with one,
    two and three substitutions are planted, so that every distance around the threshold occurs on both strands"""
    n_reads, L = 200, 40
    seq = rng.integers(0, 4, n_reads * (L + 1)).astype(np.uint8)
    starts = np.arange(n_reads, dtype=np.int64) * (L + 1)
    code = {c: i for i, c in enumerate("ACGT")}
    for r in range(0, 160):
        word = [code[c] for c in (seed_kmer if r % 2 == 0 else revcom_text(seed_kmer))]
        for _ in range((r // 2) % 4):                          # 0 .. 3 substitutions
            word[int(rng.integers(0, len(word)))] = int(rng.integers(0, 4))
        at = starts[r] + int(rng.integers(0, L - len(word) + 1))
        seq[at:at + len(word)] = word
    seq[rng.random(len(seq)) < 0.01] = 255
    seq[starts + L] = 255
    return seq, np.stack([starts, starts + L], axis=1)


@pytest.mark.parametrize("revcom", [True, False])
@pytest.mark.parametrize("d", [0, 1, 2])
def test_first_threshold_selects_the_hamming_ball(d, revcom):
    from kmap_amd.discover import seed_matrix, seed_threshold
    from kmap_amd.pwm import pwm_weights
    from kmap_amd.refine import pad_matrix
    kmer, flank, n0 = "ACCTACGT", 2, 20
    seq, borders = seeded_reads(kmer, np.random.default_rng(2100 + d))
    C = seed_matrix(kmer, n0)
    assert C.shape == (4, 8) and (C.sum(axis=0) == n0).all() and "".join("ACGT"[b] for b in C.argmax(axis=0)) == kmer
    W = pwm_weights(pad_matrix(C, flank), 1.0)
    assert not W[:, :flank].any() and not W[:, -flank:].any()
    t1 = seed_threshold(kmer, n0, flank, d, 1.0)
    _, _, p, _, minus = np_hits(seq, borders, W, t1, revcom)
    # the enumeration: every window of 12 valid bases whose core is within d mismatches of the seed (or of its reverse complement)
    w, k = 8 + 2 * flank, 8
    fwd_word = np.array(["ACGT".index(c) for c in kmer])
    rc_word = np.array(["ACGT".index(c) for c in revcom_text(kmer)])
    want, want_minus = [], []
    for s in range(len(seq) - w + 1):
        win = seq[s:s + w]
        if (win == 255).any():
            continue
        df = int((win[flank:flank + k] != fwd_word).sum())
        dr = int((win[flank:flank + k] != rc_word).sum())
        if df <= d or (revcom and dr <= d):
            want.append(s)
            want_minus.append(revcom and dr < df)
    assert len(want) >= 10 and p.tolist() == want            # 20 exact forward copies were planted, invalid bases remove a few
    assert minus.tolist() == want_minus and (any(want_minus) if revcom else not any(want_minus))
    if d < 2:                                                # one more mismatch is outside: the threshold is not merely low
        far = seed_threshold(kmer, n0, flank, d + 1, 1.0)
        assert far < t1 and len(np_hits(seq, borders, W, far, revcom)[2]) > len(want)


def test_seed_rules():
    from kmap_amd.discover import seed_matrix, seed_threshold
    with pytest.raises(ValueError, match="seed 'ACGN"):
        seed_matrix("ACGNACGT", 20)
    with pytest.raises(ValueError, match="seed_count 0"):
        seed_matrix("ACGTACGT", 0)
    with pytest.raises(ValueError, match="seed_mismatches 8"):
        seed_threshold("ACGTACGT", 20, 2, 8, 1.0)
    with pytest.raises(ValueError, match="pseudocount"):
        seed_threshold("ACGTACGT", 20, 2, 1, 0.0)


# ---- 2. the lockstep refinement ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    seq, borders = encode_fasta_np(ROOT / "tests" / "golden" / "test.fa")
    cseq = shuffle_array(seq, 2, 0)
    for a in (seq, borders, cseq):
        a.setflags(write=False)
    return seq, borders, cseq


def test_refine_many_equals_refine_matrix(golden):
    from kmap_amd.discover import refine_many, seed_matrix
    from kmap_amd.refine import refine_matrix
    seq, borders, _ = golden
    # a sharp 4-mer with empty flanks: more than p 4^w windows tie at its best score, so the threshold lies above it -- no hit
    absent = seed_matrix("ACGT", 20)
    C0s = [seed_matrix("ACCTACGT", 20), seed_matrix("ATCGATAG", 20), seed_matrix("CGATAGCG", 20), absent, seed_matrix("AGTACGTA", 20)]
    for max_iter, flank in ((10, 2), (2, 1)):
        calls = []
        many = refine_many(C0s, DM.counts_fn(seq, borders, True, calls), flank, 1e-4, 1.0, max_iter)
        single = [refine_matrix(C0, model_count_fn(seq, borders, True, True), flank, 1e-4, 1.0, max_iter) for C0 in C0s]
        for (r1, s1, t1), (r2, s2, t2) in zip(many, single):
            np.testing.assert_array_equal(r1, r2)
            assert s1 == s2 and t1 == [row[:2] + row[3:] for row in t2]
        n_iter = [len(t) for _, _, t in many]
        statuses = [s for _, s, _ in many]
        # one call per round, with the matrices that were still running
        assert calls == [sum(n >= it for n in n_iter) for it in range(1, max(n_iter) + 1)]
        if max_iter == 10:
            assert statuses[3] == "no_hits" and statuses.count("converged") == 4 and len(set(n_iter)) >= 3, (statuses, n_iter)
        else:
            assert "max_iter" in statuses and statuses[3] == "no_hits" and max(n_iter) == 2, statuses
    with pytest.raises(ValueError, match="max_iter 0"):
        refine_many(C0s, None, 0, 1e-4, 1.0, 0)
    with pytest.raises(ValueError, match="5 matrices, 1 first thresholds"):
        refine_many(C0s, None, 0, 1e-4, 1.0, 3, [0])


# ---- 3. the core on the golden reads ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden_core(golden):
    from kmap_amd.discover import discover_core
    seq, borders, cseq = golden
    assert len(borders) == 1002
    seeds = DM.top_seeds(seq, borders, cseq, borders, 8, True, 2, 16)
    calls, matches = [], []

    def match_fn(*args):
        matches.append(len(args[0]))
        return DM.match_fn(*args)
    res = discover_core(seeds, DM.counts_fn(seq, borders, True, calls), DM.hist_fn(seq, borders, cseq, borders, True), match_fn, True,
                        flank=2, seed_mismatches=1)
    return seeds, res, calls, matches


def test_core_finds_the_two_planted_motifs(golden_core):
    from kmap_amd.pwm import pwm_consensus
    seeds, res, calls, matches = golden_core
    assert len(seeds) == len(res) == 16 and all(len(s[0]) == 8 and s[1] >= 2 and s[3] > 0 for s in seeds)
    assert [s[3] for s in seeds] == sorted((s[3] for s in seeds), reverse=True)
    assert matches == [16] and calls[0] == 16 and calls == sorted(calls, reverse=True)
    for st in res:
        assert st["status"] == "converged" and st["iterations"] <= 10 and st["iterations"] == len(st["trace"]), st["name"]
        assert st["mw_z"] > 5, (st["name"], st["mw_z"])
        assert st["counts"].shape == (4, 12) and (st["counts"].sum(axis=0) == st["n_selected"]).all()
        assert st["trace"][-1][-1] == 0 and st["trace"][-1][2:4] == (st["n_selected"], st["n_minus"])
    assert sorted(st["family"] for st in res if st["is_representative"]) == [0, 1]
    assert len({st["family"] for st in res}) == 2
    reps = sorted((st for st in res if st["is_representative"]), key=lambda st: st["rank"])
    texts = [pwm_consensus(st["counts"]) for st in reps]
    for word in ("CCTACGTA", "ATCGATAG"):
        assert sum(word in t or word in revcom_text(t) for t in texts) == 1, (word, texts)
    for st in res:                                           # the representative: the largest mw_z of its family
        mates = [o for o in res if o["family"] == st["family"]]
        assert st["family_size"] == len(mates)
        assert st["is_representative"] == (st["mw_z"] == max(o["mw_z"] for o in mates))
    assert sorted(st["rank"] for st in res) == list(range(16))
    by_rank = sorted(res, key=lambda st: st["rank"])
    assert [st["mw_z"] for st in by_rank] == sorted((st["mw_z"] for st in res), reverse=True)
    q = [st["q_bh"] for st in res]
    assert all(0 < x < 1e-10 for x in q)


def test_representative_rule_and_single_seed():
    from types import SimpleNamespace

    from kmap_amd.discover import group_families
    Cs = [np.full((4, 8), 5, np.int64)] * 4
    p = np.full((4, 4), 1e-12)
    p[3, :3] = p[:3, 3] = 1.0                                # 0, 1, 2 linked; 3 alone
    fam = group_families(Cs, [2.0, 7.0, 7.0, float("nan")], lambda *a: SimpleNamespace(p_best=p), True, 5, 1.0, 0.01)
    assert fam == ([0, 0, 0, 1], [3, 3, 3, 1], [False, True, False, True])
    fam = group_families(Cs, [float("nan"), float("nan"), 1.0, 0.0], lambda *a: SimpleNamespace(p_best=p), True, 5, 1.0, 0.01)
    assert fam[2] == [False, False, True, True]
    fam = group_families(Cs[:3], [float("nan")] * 3, lambda *a: SimpleNamespace(p_best=p[:3, :3]), True, 5, 1.0, 0.01)
    assert fam[2] == [True, False, False]

    def never(*a):
        raise AssertionError("match_fn was called for a single seed")
    assert group_families(Cs[:1], [1.0], never, True, 5, 1.0, 0.01) == ([0], [1], [True])


def test_no_seed_is_an_error():
    from kmap_amd.discover import discover_core
    with pytest.raises(ValueError, match="no seed"):
        discover_core([], None, None, None, True)


# ---- 4. the files -----------------------------------------------------------------------------------------------------------------
def test_files_and_meme_round_trip(golden_core, tmp_path):
    from kmap_amd import discover as D
    from kmap_amd.library import read_motif_library
    from kmap_amd.pwm import pwm_consensus, read_count_matrix
    _, res, _, _ = golden_core
    reps = D.write_discovery(tmp_path / "o", res, 1.0, True)
    assert [st["is_representative"] for st in reps] == [True, True] and reps[0]["rank"] < reps[1]["rank"]
    back = read_motif_library(tmp_path / "o" / D.MEME_FILE)
    assert [m.name for m in back] == [st["name"] for st in reps] and [m.altname for m in back] == [st["seed"] for st in reps]
    for m, st in zip(back, reps):
        assert m.skip is None
        np.testing.assert_array_equal(m.counts, st["counts"])
    assert f"nsites= {reps[0]['n_selected']} " in (tmp_path / "o" / D.MEME_FILE).read_text()
    lines = (tmp_path / "o" / D.RANK_FILE).read_text().split("\n")
    cols = lines[0].split(",")
    assert cols[:14] == ["rank", "name", "seed", "seed_fg", "seed_control", "seed_z", "status", "iterations", "n_selected", "n_minus",
                         "information_bits", "family", "family_size", "is_representative"]
    assert cols[14:16] == ["width", "consensus"] and cols[-2:] == ["log10_p", "q_bh"] and len(lines) == 18 and lines[-1] == ""
    rows = [dict(zip(cols, ln.split(","))) for ln in lines[1:-1]]
    assert all(len(ln.split(",")) == len(cols) for ln in lines[1:-1])
    assert [int(r["rank"]) for r in rows] == list(range(16)) and sum(int(r["is_representative"]) for r in rows) == 2
    z = [float(r["mw_z"]) for r in rows]
    assert z == sorted(z, reverse=True)
    for r in rows:
        st = res[int(r["name"].split("_")[0][4:])]
        assert r["name"] == f"seed{st['seed_rank']}_{r['consensus']}" and float(r["seed_z"]) == st["seed_z"] and r["width"] == "12"
        np.testing.assert_array_equal(read_count_matrix(tmp_path / "o" / D.MATRIX_DIR / f"{r['name']}.csv"), st["counts"])
        assert pwm_consensus(st["counts"]) == r["consensus"]
    trace = (tmp_path / "o" / D.TRACE_FILE).read_text().split("\n")
    assert trace[0] + "\n" == D.TRACE_HEADER and len(trace) == 2 + sum(st["iterations"] for st in res)
    assert trace[1].split(",")[:2] == ["0", "1"] and re.fullmatch(r"\d+,\d+,-?\d+,\d+,\d+,[ACGT]{12},\d+\.\d{3},\d+", trace[1])


def test_meme_text_refuses_unequal_columns():
    from kmap_amd.discover import meme_text
    C = np.full((4, 6), 3, np.int64)
    C[0, 2] = 4
    with pytest.raises(ValueError, match="common sum"):
        meme_text([("m", "", C)])
    assert "MOTIF a_b" in meme_text([("a,b", "", np.full((4, 6), 3, np.int64))])


# ---- 5. the verb's checks ---------------------------------------------------------------------------------------------------------
def test_argument_errors_come_first(tmp_path, monkeypatch):
    from kmap_amd import _ffi
    from kmap_amd import discover as D
    from tests._sites_model import write_planted
    monkeypatch.delenv("WORLD_SIZE", raising=False)

    def no_lib():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_ffi, "lib", no_lib)
    res, ctl, *_ = write_planted(tmp_path)
    out = tmp_path / "out"
    ok = dict(res_dir=str(res), control_fasta_file=str(ctl), output_dir=str(out))
    bad = [(dict(seed_len=28, flank=2), "seed_len 28 \\+ 2 x flank 2 = 32 is more than 31"),
           (dict(seed_len=3), "seed_len 3 outside 4..31"),
           (dict(seed_mismatches=8), "seed_mismatches 8 outside 0..7"),
           (dict(seed_mismatches=-1), "seed_mismatches -1"),
           (dict(pseudocount=0.0), "pseudocount 0.0 is not a finite number > 0"),
           (dict(control_fasta_file=str(tmp_path / "missing.fa")), "control FASTA file .*missing.fa is missing"),
           (dict(n_seeds=0), "n_seeds 0 outside 1..1024"),
           (dict(n_seeds=1025), "n_seeds 1025"),
           (dict(seed_count=0), "seed_count 0"),
           (dict(flank=-1), "flank -1"),
           (dict(min_count=0), "min_count 0"),
           (dict(max_iter=0), "max_iter 0"),
           (dict(min_overlap=0), "min_overlap 0"),
           (dict(p_value=float("nan")), "p_value"),
           (dict(family_e_value=-1.0), "family_e_value"),
           (dict(res_dir=str(tmp_path / "nowhere")), "not a result directory")]
    for change, word in bad:
        with pytest.raises(ValueError, match=word):
            D._discover_pwms(**{**ok, **change})
    assert not out.exists() and not (res / D.OUTPUT_DIR).exists()
    with pytest.raises(AssertionError, match="the library was loaded"):
        D._discover_pwms(**ok)
    assert not out.exists()


def test_other_ranks_do_nothing(monkeypatch):
    from kmap_amd.discover import _discover_pwms
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "1")
    assert _discover_pwms("nowhere", None, seed_len=99) is None


def test_library_counts_checks_come_before_the_library(monkeypatch):
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
        with pytest.raises(ValueError, match="library_counts: .*" + word):
            ds.library_counts(Ws, ts, True)


def test_symbol_registered():
    from kmap_amd import _ffi
    header = (ROOT / "include" / "kmap_hip.h").read_text()
    name = "kmap_readscore_counts_library_dev"
    assert name in _ffi.exported_symbols() and f"int {name}(" in header
    res, args = _ffi._SIGS[name]
    assert res is _ffi.i32 and len(args) == 14
    assert not name.startswith("kmap_pwm_")
    src = (ROOT / "kmap_amd" / "csrc" / "pwm_sites.hip").read_text()
    assert f"int {name}(" in src and "sites_count_kernel" in src


# ---- 6. the command line ----------------------------------------------------------------------------------------------------------
def test_cli_options_and_defaults(monkeypatch):
    from click.testing import CliRunner
    from kmap_amd import discover
    from kmap_amd.cli import cli
    calls = []
    monkeypatch.setattr(discover, "_discover_pwms", lambda *a: calls.append(a))
    runner = CliRunner()
    r = runner.invoke(cli, ["discover_pwms", "--res_dir", "D", "--control_fasta_file", "C.fa"])
    assert r.exit_code == 0, r.output
    assert calls[-1] == ("D", "C.fa", 8, 64, 1, 20, 2, 2, 1e-4, 1.0, None, 20, 5, 0.01, None)
    r = runner.invoke(cli, ["discover_pwms", "--res_dir", "D", "--control_fasta_file", "C.fa", "--seed_len", "10", "--n_seeds", "16",
                            "--seed_mismatches", "2", "--seed_count", "30", "--flank", "3", "--min_count", "5", "--p_value", "1e-3",
                            "--pseudocount", "0.5", "--revcom_mode", "False", "--max_iter", "7", "--min_overlap", "6",
                            "--family_e_value", "0.05", "--output_dir", "O"])
    assert r.exit_code == 0, r.output
    assert calls[-1] == ("D", "C.fa", 10, 16, 2, 30, 3, 5, 1e-3, 0.5, False, 7, 6, 0.05, "O")
    for missing in (["--control_fasta_file", "C.fa"], ["--res_dir", "D"]):
        assert runner.invoke(cli, ["discover_pwms"] + missing).exit_code == 2
    assert len(calls) == 2
    r = runner.invoke(cli, ["discover_pwms", "--help"])
    for opt in ("--res_dir", "--control_fasta_file", "--seed_len", "--n_seeds", "--seed_mismatches", "--seed_count", "--flank",
                "--min_count", "--p_value", "--pseudocount", "--revcom_mode", "--max_iter", "--min_overlap", "--family_e_value",
                "--output_dir"):
        assert opt in r.output, opt
    assert "discover_pwms" in runner.invoke(cli, ["--help"]).output
    import kmap_amd.cli as cli_module
    doc = cli_module.__doc__
    assert "ten verbs the reference does not have" in doc and "An eleventh, `motif_cooccurrence`" in doc
    assert doc.index("An eleventh,") < doc.index("A twelfth, `discover_pwms`")
    assert "discover_pwms" in (ROOT / "README.md").read_text()
