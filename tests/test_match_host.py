"""match_motifs without a GPU: the definitions as tests/_match_model.py restates them, and the host side of
kmap_amd/motif_match.py -- quantisation, the table layout, the batches, the pair statistics, the families, the file formats, the
argument checks -- held to that model or to hand-made cases."""
import itertools
import math
import re
from pathlib import Path

import numpy as np
import pytest

from tests import _match_model as M

ROOT = Path(__file__).resolve().parent.parent
LIB = ROOT / "tests" / "golden" / "library"
MATCH = ROOT / "tests" / "golden" / "match"


def one_pair(Cq, Ct, library, min_overlap=5, revcom=True):
    """the model's best configuration of one pair, the null built from `library` (count matrices)"""
    uq, ut = M.quantise(Cq), M.quantise(Ct)
    lib_u = [M.quantise(C) for C in library]
    H = M.null_hist(uq, M.library_columns(lib_u, revcom))
    tables = M.null_tables(H, sum(u.shape[1] for u in lib_u) * (2 if revcom else 1))
    return M.best_configuration(M.configurations(uq, ut, tables, min_overlap, revcom))


@pytest.fixture(scope="module")
def some_motifs():
    rng = np.random.default_rng(1700)
    return [M.random_counts(rng, w) for w in (8, 11, 6, 14, 9)]


# ---- 1. the definitions ---------------------------------------------------------------------------------------------------------------
def test_column_score_range():
    assert M.col_score([1024, 0, 0, 0], [1024, 0, 0, 0]) == 90 and M.col_score([1024, 0, 0, 0], [0, 1024, 0, 0]) == 0
    assert M.col_score([256, 256, 256, 256], [1024, 0, 0, 0]) == (1448 - math.isqrt(768 ** 2 + 3 * 256 ** 2)) // 16


def test_motif_against_itself_and_its_reverse_complement(some_motifs):
    C = some_motifs[1]
    w = C.shape[1]
    p, o, strand, L, x = one_pair(C, C, some_motifs)
    assert (o, strand, L, x) == (0, 0, w, 90 * w)
    rc = C[::-1, ::-1]
    assert not np.array_equal(rc, C)
    p2, o, strand, L, x = one_pair(C, rc, some_motifs)
    assert (o, strand, L, x) == (0, 1, w, 90 * w) and p2 == p
    assert one_pair(C, rc, some_motifs, revcom=False)[4] < 90 * w


def test_embedded_motif_is_found_at_its_offset(some_motifs):
    rng = np.random.default_rng(1701)
    short = some_motifs[0]                                   # 8 columns
    long = M.random_counts(rng, 15)
    long[:, 3:11] = short
    p, o, strand, L, x = one_pair(long, short, some_motifs + [long])   # target column j faces query column j + 3
    assert (o, strand, L, x) == (3, 0, 8, 720)
    p, o, strand, L, x = one_pair(short, long, some_motifs + [long])
    assert (o, strand, L, x) == (-3, 0, 8, 720)


def test_null_tables_against_brute_force():
    """a library of 6 columns, a query of 3: every tail probability of the range 0..2 against the 6^3 column triples"""
    rng = np.random.default_rng(1702)
    uq = M.quantise(M.random_counts(rng, 4))[:, :3]
    cols = M.quantise(M.random_counts(rng, 6, sharp=0.5)).T
    H = M.null_hist(uq, cols)
    assert H.dtype == np.uint32 and H.sum(axis=1).tolist() == [6, 6, 6]
    tables = M.null_tables(H, 6)
    assert sorted(tables) == [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]
    totals = [sum(M.col_score(uq[:, i], y[i]) for i in range(3)) for y in itertools.product(cols, repeat=3)]
    pmf, sf = tables[(0, 2)]
    assert len(pmf) == len(sf) == 271
    for x in range(271):
        want = sum(t >= x for t in totals) / 216.0
        assert sf[x] == pytest.approx(want, rel=1e-12, abs=0.0), x
    for pmf, sf in tables.values():
        assert pmf.sum() == pytest.approx(1.0, rel=1e-12) and sf[0] == pytest.approx(1.0, rel=1e-12)
        assert (pmf >= 0).all() and (np.diff(sf) <= 0).all()


# ---- 2. the host side of the package ----------------------------------------------------------------------------------------------------
def test_quantise_columns(some_motifs):
    from kmap_amd import motif_match as K
    from kmap_amd.pwm import pwm_weights
    for C, a in itertools.product(some_motifs, (1.0, 0.0, 0.37)):
        u = K.quantise_columns(C, a)
        assert u.dtype == np.uint16 and u.shape == (C.shape[1], 4) and u.flags.c_contiguous
        np.testing.assert_array_equal(u.T, M.quantise(C, a))
        assert int(u.max()) <= 1024
    C = some_motifs[0]
    f = (C + 0.25) / (C.sum(axis=0) + 1.0)                   # pwm_weights' frequencies
    np.testing.assert_array_equal(pwm_weights(C, 1.0), np.rint(np.log2(f / 0.25) * 100).astype(np.int32))
    np.testing.assert_array_equal(K.quantise_columns(C, 1.0).T, np.rint(1024 * f))
    empty = C.copy()
    empty[:, 2] = 0
    with pytest.raises(ValueError, match="pseudocount > 0"):
        K.quantise_columns(empty, 0.0)
    with pytest.raises(ValueError, match="pseudocount"):
        K.quantise_columns(C, -1.0)


def test_table_layout_and_batches():
    from kmap_amd import motif_match as K
    for w, ml in ((4, 1), (4, 4), (13, 5), (31, 1), (31, 5), (31, 31)):
        at = 0
        for a in range(w):
            for b in range(a + ml - 1, w):
                assert K.table_offset(a, b, w, ml) == at, (w, ml, a, b)
                at += 90 * (b - a + 1) + 1
        assert K.table_doubles(w, ml) == at
    sizes = [10, 20, 30, 5, 100, 1]
    assert K.plan_batches(sizes, 1 << 40) == [(0, 6)]
    assert K.plan_batches(sizes, 8 * 60) == [(0, 3), (3, 4), (4, 5), (5, 6)]   # 100 alone is over the budget: a batch of its own
    assert K.plan_batches(sizes, 1) == [(q, q + 1) for q in range(6)]
    assert K.plan_batches([], 1) == []
    many = K.plan_batches([1] * (K.MAX_QUERIES_PER_CALL + 2), 1 << 40)
    assert many == [(0, K.MAX_QUERIES_PER_CALL), (K.MAX_QUERIES_PER_CALL, K.MAX_QUERIES_PER_CALL + 2)]


def test_pair_statistics_against_the_model():
    from kmap_amd import library
    from kmap_amd import motif_match as K
    rng = np.random.default_rng(1703)
    qw, tw = [4, 9, 31, 12], [6, 31, 4, 17, 10]
    p = rng.random((4, 5)) ** 6
    p[0, 0], p[1, 2], p[2, 2] = 1.0, 0.0, 1e-300
    for mo, revcom in ((5, True), (1, False), (31, True)):
        pm, ev, qb = K.pair_statistics(p, qw, tw, mo, revcom)
        for q, t in itertools.product(range(4), range(5)):
            n = M.n_cfg(qw[q], tw[t], mo, revcom)
            assert n == K.n_configurations(qw[q], tw[t], mo, revcom)
            assert pm[q, t] == pytest.approx(M.p_match(p[q, t], n), rel=1e-14, abs=0.0)
            assert ev[q, t] == pm[q, t] * 5
        assert pm[0, 0] == 1.0 and pm[1, 2] == 0.0 and pm[2, 2] > 0.0
        for q in range(4):
            np.testing.assert_allclose(qb[q], M.bh(pm[q]), rtol=1e-14)
            np.testing.assert_array_equal(qb[q], library.bh_qvalues(pm[q]))          # reused unchanged
    # all against all: the diagonal is left out, T - 1 targets
    p = rng.random((5, 5)) ** 6
    pm, ev, qb = K.pair_statistics(p, tw, tw, 5, True, all_against_all=True)
    for q in range(5):
        others = [t for t in range(5) if t != q]
        assert math.isnan(pm[q, q]) and math.isnan(ev[q, q]) and math.isnan(qb[q, q])
        np.testing.assert_array_equal(ev[q, others], pm[q, others] * 4)
        np.testing.assert_allclose(qb[q, others], M.bh(pm[q, others]), rtol=1e-14)


def test_families_on_hand_made_links():
    from kmap_amd import motif_match as K
    # 0-3-5 a chain, 1-2 a pair, 4 alone, 6-7-8 a triangle with 9 hanging off 8
    links = [(3, 5), (0, 3), (2, 1), (6, 7), (7, 8), (6, 8), (8, 9), (8, 9)]
    family, size, rep, n_links = K.families(10, links)
    assert family == [0, 1, 1, 0, 2, 0, 3, 3, 3, 3]                     # numbered by the smallest member
    assert size == [3, 2, 2, 3, 1, 3, 4, 4, 4, 4]
    assert n_links == [1, 1, 1, 2, 0, 1, 2, 2, 3, 1]                    # the doubled link counts once
    assert [i for i in range(10) if rep[i]] == [1, 3, 4, 8]             # most links; the pair's tie goes to the smaller index
    assert K.families(3, []) == ([0, 1, 2], [1, 1, 1], [True, True, True], [0, 0, 0])
    family, _, rep, _ = K.families(4, [(0, 1), (1, 2), (2, 3), (3, 0)])     # a ring: all tie
    assert family == [0, 0, 0, 0] and rep == [True, False, False, False]
    with pytest.raises(ValueError, match="outside"):
        K.families(3, [(0, 3)])
    e = np.array([[np.nan, 1e-5, 0.5], [1e-3, np.nan, 1e-9], [1e-9, 0.5, np.nan]])
    assert K.family_links(e, 0.01) == [(0, 1)]                          # both directions must pass
    assert K.family_links(e, 1e-4) == []


def test_csv_formatting():
    from kmap_amd import motif_match as K
    from kmap_amd.library import LibraryMotif
    Cq = np.array([[9, 0, 0, 1], [0, 9, 1, 0], [1, 0, 9, 0], [0, 1, 0, 9]])         # ACGT
    Ct = np.array([[9, 9, 0, 1, 0], [0, 0, 9, 0, 0], [1, 0, 0, 9, 0], [0, 1, 1, 0, 10]])  # AACGT
    q, t = LibraryMotif("q,1", "", "a.csv", Cq), LibraryMotif("T1", "alt,name", "lib.meme", Ct)
    assert q.name == "q_1" and t.altname == "alt_name"
    line = K.match_line(q, t, -1, 0, 4, 352, 1.5e-7, 3e-7, 0.25)
    assert line == "q_1,T1,alt_name,lib.meme,4,5,-1,+,4,352,1.5e-07,3e-07,0.25,ACGT,AACGT\n"
    assert K.match_line(q, t, 0, 1, 4, 352, 1.0, 2.0, 1.0).endswith(",0,-,4,352,1.0,2.0,1.0,ACGT,ACGTT\n")
    assert len(line.split(",")) == len(K.MATCH_HEADER.split(",")) == 15
    assert K.MATCH_HEADER == ("query,target,altname,source,query_width,target_width,offset,strand,overlap,score,p_value,e_value,q_bh,"
                              "query_consensus,target_consensus\n")
    assert K.FAMILY_HEADER == "family,size,name,altname,source,width,consensus,is_representative,n_links\n"
    assert K.top_targets([0.5, 0.1, 0.1, 0.0], ["d", "c", "b", "a"], 3) == [3, 2, 1]
    assert K.top_targets([0.5, 0.1, 0.1, 0.0], ["d", "c", "b", "a"], 10, skip=3) == [2, 1, 0]


def test_value_errors_come_before_the_library(tmp_path, monkeypatch):
    from kmap_amd import _ffi
    from kmap_amd import motif_match as K

    def no_lib():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_ffi, "lib", no_lib)
    out = tmp_path / "out"
    queries = str(MATCH / "queries")
    only_wide = tmp_path / "wide.meme"
    only_wide.write_text("MEME version 4\n\nMOTIF W\nletter-probability matrix: alength= 4 w= 32\n" + "0.25 0.25 0.25 0.25\n" * 32)
    zero = tmp_path / "zero.csv"
    zero.write_text("0,2,3,0\n0,2,3,4\n0,2,3,4\n0,2,3,4\n")
    one = str(MATCH / "queries" / "q1_planted.csv")
    ok = dict(query_files=[queries], library_files=[str(LIB / "three.meme")], output_dir=out)
    bad = [(dict(query_files=[]), "no query file"),
           (dict(query_files=[str(tmp_path / "nowhere.csv")]), "nowhere.csv"),
           (dict(library_files=[str(tmp_path / "nowhere.meme")]), "nowhere.meme"),
           (dict(library_files=[str(LIB / "bad_alength.meme")]), "bad_alength.meme:11"),
           (dict(library_files=[str(only_wide)]), "none of the motifs of the library.*W: width 32"),
           (dict(query_files=[str(only_wide)]), "none of the motifs of the query.*W: width 32"),
           (dict(query_files=[str(zero)], pseudocount=0.0), "zero.csv: motif zero: .*pseudocount"),
           (dict(query_files=[one], library_files=[]), "nothing to match"),
           (dict(pseudocount=-1.0), "pseudocount"),
           (dict(pseudocount=float("nan")), "pseudocount"),
           (dict(min_overlap=0), "min_overlap"),
           (dict(nsites_default=0), "nsites_default"),
           (dict(top_n=0), "top_n"),
           (dict(family_e_value=-1.0), "family_e_value"),
           (dict(table_byte_budget=0), "table_byte_budget")]
    for change, word in bad:
        with pytest.raises(ValueError, match=word):
            K._match_motifs(**{**ok, **change})
    assert not out.exists()
    with pytest.raises(AssertionError, match="the library was loaded"):
        K._match_motifs(**ok)
    assert not out.exists()
    C = np.ones((4, 6), np.int64)
    for kw, word in ((dict(min_overlap=0), "min_overlap"), (dict(table_byte_budget=0), "table_byte_budget"), (dict(pseudocount=-1), "pseudocount")):
        with pytest.raises(ValueError, match=word):
            K.match_motifs([C], [C], **kw)
    with pytest.raises(ValueError, match="no query or no target"):
        K.match_motifs([], [C])
    with pytest.raises(ValueError, match="4 x w|width|shape"):
        K.match_motifs([np.ones((4, 32), np.int64)], [C])


def test_other_ranks_do_nothing(monkeypatch):
    from kmap_amd.motif_match import _match_motifs
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "1")
    assert _match_motifs(["nowhere"]) is None


# ---- 3. the entries, the command line, the documents -----------------------------------------------------------------------------------
def test_symbols_declared_and_bound():
    from kmap_amd import _ffi
    header = (ROOT / "include" / "kmap_hip.h").read_text()
    for name, n_args in (("kmap_match_hist_dev", 7), ("kmap_match_tables_dev", 11), ("kmap_match_pairs_dev", 19)):
        assert name in _ffi.exported_symbols() and f"int {name}(" in header
        res, args = _ffi._SIGS[name]
        assert res is _ffi.i32 and len(args) == n_args
        decl = re.search(rf"int {name}\((.*?)\);", header, re.S).group(1)
        assert len(re.sub(r"/\*.*?\*/", "", decl, flags=re.S).split(",")) == n_args
    src = (ROOT / "kmap_amd" / "csrc" / "motif_match.hip").read_text()
    from kmap_amd import motif_match as K
    assert int(re.search(r"constexpr int MM_BINS = (\d+);", src).group(1)) == K.N_BINS
    assert f"n_query <= {K.MAX_QUERIES_PER_CALL}" in src


def test_cli_options_and_defaults(monkeypatch):
    from click.testing import CliRunner
    from kmap_amd import motif_match
    from kmap_amd.cli import cli
    calls = []
    monkeypatch.setattr(motif_match, "_match_motifs", lambda *a: calls.append(a))
    r = CliRunner().invoke(cli, ["match_motifs", "--query_file", "a.csv", "--query_file", "d"])
    assert r.exit_code == 0, r.output
    assert calls[-1] == (["a.csv", "d"], [], True, 5, 1.0, 20, 10, 0.01, "./motif_matches")
    r = CliRunner().invoke(cli, ["match_motifs", "--query_file", "a.csv", "--library_file", "l.meme", "--library_file", "m", "--revcom_mode",
                                 "False", "--min_overlap", "7", "--pseudocount", "0.5", "--nsites_default", "30", "--top_n", "3",
                                 "--family_e_value", "1e-3", "--output_dir", "o"])
    assert r.exit_code == 0, r.output
    assert calls[-1] == (["a.csv"], ["l.meme", "m"], False, 7, 0.5, 30, 3, 1e-3, "o")
    assert CliRunner().invoke(cli, ["match_motifs"]).exit_code != 0            # --query_file is required
    assert "res_dir" not in cli.commands["match_motifs"].get_help(__import__("click").Context(cli.commands["match_motifs"]))


def test_documents_name_the_verb():
    readme = (ROOT / "README.md").read_text()
    assert "match_motifs" in readme.split("\n\n")[0] + readme.split("\n\n")[1] and "python -m kmap_amd match_motifs --query_file" in readme
    design = (ROOT / "DESIGN.md").read_text()
    assert "## 17." in design and "match_motifs" in design and "section 17" in design.split("## 17.")[0].split("## 16.")[1]
    assert "match_motifs" in (ROOT / "CHANGELOG.md").read_text()
    from kmap_amd import cli
    assert "match_motifs" in cli.__doc__
