"""match_motifs on the GPU (csrc/motif_match.hip).  The yardstick is tests/_match_model.py, never the kernels:
histograms and configurations as equal integers, tables and p-values to rtol 1e-9.

Why 1e-9 for the tables: every term is non-negative, so nothing cancels; an entry is at most 31 levels of sums of at most 91 products,
then a tail sum of at most 2 791 terms, each operation within 2^-53: a relative error below 31 * 92 * 2^-53 + 2791 * 2^-53 ~ 6e-13 in
either summation order.  1e-9 leaves three decades.  Zeros are exact on both sides: a sum of non-negative terms is zero only when
every term is, and no product of count fractions underflows ((1 / N)^31 > 1e-300 for every N the tests use)."""
import math
from pathlib import Path

import numpy as np
import pytest

from tests import _match_model as M

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
LIB = ROOT / "tests" / "golden" / "library"
QUERIES = ROOT / "tests" / "golden" / "match" / "queries"
RTOL = 1e-9
Q_WIDTHS = [4, 5, 16, 17, 31, 9, 12]
T_WIDTHS = [4, 5, 16, 17, 31, 31, 20, 4, 9, 12, 6, 7, 8, 25, 30, 13, 5, 11, 10, 14, 15, 18, 19, 21, 22, 23, 24, 26, 27, 28, 29, 6, 8, 10, 12, 16, 17]


class Motifs:
    """Q = 7 queries, T = 37 targets of mixed widths (fixed seed): random motifs, and among the targets relatives of the queries -- a
    copy, a reverse complement, a piece, a motif that contains the query -- so that there are clear matches on both strands and
    at offsets of both signs.  The model's score matrices of every pair are computed once."""

    def __init__(self):
        rng = np.random.default_rng(1710)
        self.queries = [M.random_counts(rng, w) for w in Q_WIDTHS]
        self.targets = [M.random_counts(rng, w) for w in T_WIDTHS]
        q16, q31, q9, q12 = self.queries[2], self.queries[4], self.queries[5], self.queries[6]
        self.targets[2] = q16.copy()                                  # the query itself
        self.targets[5] = q31[::-1, ::-1].copy()                      # its reverse complement, full width
        self.targets[8] = q31[:, 11:20].copy()                        # a piece of a wider query: w_q > w_t, o > 0
        self.targets[6][:, 5:14] = q9                                 # the query inside a wider target: w_q < w_t, o < 0
        self.targets[13][:, 10:22] = q12[::-1, ::-1]                  # the same on the other strand
        self.uq = [M.quantise(C) for C in self.queries]
        self.ut = [M.quantise(C) for C in self.targets]
        self.scores = [[(M.score_matrix(uq, ut), M.score_matrix(uq, M.revcomp(ut))) for ut in self.ut] for uq in self.uq]
        self._tables = {}

    def hist(self, revcom):
        cols = M.library_columns(self.ut, revcom)
        return [M.null_hist(uq, cols) for uq in self.uq], len(cols)

    def tables(self, revcom, min_len):
        """per query {(a, b): (pmf, sf)} for the ranges of at least min(min_len, w_q) columns"""
        key = (revcom, min_len)
        if key not in self._tables:
            H, n = self.hist(revcom)
            self._tables[key] = [M.null_tables(h, n, min(min_len, len(h))) for h in H]
        return self._tables[key]

    def configurations(self, q, t, min_overlap, revcom):
        tables = self.tables(revcom, min(min_overlap, min(T_WIDTHS)))
        return M.configurations(self.uq[q], self.ut[t], tables[q], min_overlap, revcom, self.scores[q][t])


@pytest.fixture(scope="module")
def motifs():
    return Motifs()


def check_pairs(res, configurations, n_q, n_t):
    """every pair of the device result against the model's configurations of that pair"""
    assert all(a.shape == (n_q, n_t) for a in res) and res.p_best.dtype == np.float64
    assert all(a.dtype == np.int32 for a in res[1:])
    for q in range(n_q):
        for t in range(n_t):
            cfgs = configurations(q, t)
            by_cfg = {(c[1], c[2]): c for c in cfgs}
            p_min = M.best_configuration(cfgs)[0]
            got = (int(res.o[q, t]), int(res.strand[q, t]))
            assert got in by_cfg, f"pair {q},{t}: (o, strand) = {got} is no configuration"
            p, o, strand, L, x = by_cfg[got]
            assert abs(p - p_min) <= RTOL * p_min, f"pair {q},{t}: {got} has model p {p}, the minimum is {p_min}"
            assert (int(res.L[q, t]), int(res.x[q, t])) == (L, x), f"pair {q},{t}"
            assert abs(res.p_best[q, t] - p_min) <= RTOL * p_min, f"pair {q},{t}: p_best {res.p_best[q, t]}, model {p_min}"


# ---- 1. histograms ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("revcom", [True, False])
def test_histograms(motifs, revcom):
    from kmap_amd import motif_match as K
    lcols = np.concatenate([K.quantise_columns(C) for C in motifs.targets])
    assert len(lcols) % 64 != 0 and len(lcols) > 2 * 256          # a block walks tiles of 256 library columns
    qcols = np.concatenate([K.quantise_columns(C) for C in motifs.queries])
    assert len(qcols) > 5 * 16 and len(qcols) % 16 != 0           # blocks of 16 query columns, the last one partial
    want, n = motifs.hist(revcom)
    got = K.column_histograms(qcols, lcols, revcom)
    assert got.dtype == np.uint32 and got.shape == (len(qcols), 91)
    np.testing.assert_array_equal(got, np.concatenate(want))
    assert (got.sum(axis=1) == n).all() and n == len(lcols) * (2 if revcom else 1)
    # the targets as queries (widths 4, 5, 16, 17, 31 among them) against a library of one motif, of each of these widths
    tq = np.concatenate([K.quantise_columns(C) for C in motifs.targets[:6]])
    for one in range(5):
        cols = M.library_columns([motifs.ut[one]], revcom)
        got = K.column_histograms(tq, K.quantise_columns(motifs.targets[one]), revcom)
        np.testing.assert_array_equal(got, np.concatenate([M.null_hist(u, cols) for u in motifs.ut[:6]]))


# ---- 2. null tables -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("revcom,min_len", [(True, 4), (False, 1), (True, 31)])
def test_null_tables(motifs, revcom, min_len):
    from kmap_amd import motif_match as K
    H, n = motifs.hist(revcom)
    widths = [len(h) for h in H]
    min_lens = [min(min_len, w) for w in widths]
    got, offsets = K.null_tables(np.concatenate(H), n, widths, min_lens)
    assert got.dtype == np.float64 and len(got) == offsets[-1] == sum(K.table_doubles(w, m) for w, m in zip(widths, min_lens))
    covered = 0
    for q, (w, ml) in enumerate(zip(widths, min_lens)):
        want = M.null_tables(H[q], n, ml)
        assert sorted(want) == [(a, b) for a in range(w) for b in range(a + ml - 1, w)]
        for (a, b), (_, sf) in want.items():
            at = int(offsets[q]) + K.table_offset(a, b, w, ml)
            dev = got[at:at + len(sf)]
            assert len(sf) == 90 * (b - a + 1) + 1
            np.testing.assert_array_equal(dev == 0.0, sf == 0.0, err_msg=f"zeros of query {q} range {a}..{b}")
            np.testing.assert_allclose(dev, sf, rtol=RTOL, atol=0.0, err_msg=f"query {q} range {a}..{b}")
            covered += len(sf)
    assert covered == len(got)                                    # no double of the array is left unchecked
    again, _ = K.null_tables(np.concatenate(H), n, widths, min_lens)
    assert again.tobytes() == got.tobytes()                       # fixed summation order: the same bits


# ---- 3. pairs -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("revcom", [True, False])
@pytest.mark.parametrize("min_overlap", [1, 5, 31])
def test_pairs(motifs, min_overlap, revcom):
    from kmap_amd import motif_match as K
    res = K.match_motifs(motifs.queries, motifs.targets, revcom, min_overlap)
    check_pairs(res, lambda q, t: motifs.configurations(q, t, min_overlap, revcom), len(Q_WIDTHS), len(T_WIDTHS))
    if min_overlap == 5 and revcom:                               # the planted relatives are what they were made to be
        assert (res.o[2, 2], res.strand[2, 2], res.L[2, 2], res.x[2, 2]) == (0, 0, 16, 1440)
        assert (res.o[4, 5], res.strand[4, 5], res.L[4, 5], res.x[4, 5]) == (0, 1, 31, 2790)
        assert (res.o[4, 8], res.strand[4, 8], res.L[4, 8], res.x[4, 8]) == (11, 0, 9, 810)
        assert (res.o[5, 6], res.strand[5, 6], res.L[5, 6], res.x[5, 6]) == (-5, 0, 9, 810)
        assert (res.o[6, 13], res.strand[6, 13], res.L[6, 13], res.x[6, 13]) == (-(25 - 22), 1, 12, 1080)


def test_exact_ties(motifs):
    """the same table entry reached by two configurations: bit-equal doubles, so the tie-break decides"""
    from kmap_amd import motif_match as K
    rng = np.random.default_rng(1711)
    half = M.random_counts(rng, 4, sharp=1.0)
    pal = np.concatenate([half, half[::-1, ::-1]], axis=1)        # its own reverse complement
    assert np.array_equal(pal, pal[::-1, ::-1])
    q6 = M.random_counts(rng, 6, sharp=1.0)
    twice = np.concatenate([q6, q6], axis=1)
    targets = [pal, twice] + motifs.targets[:10]
    ut = [M.quantise(C) for C in targets]
    res = K.match_motifs([pal, q6], targets, True, 5)
    lib_cols = M.library_columns(ut, True)

    def cfgs(q, t):
        uq = M.quantise([pal, q6][q])
        return M.configurations(uq, ut[t], M.null_tables(M.null_hist(uq, lib_cols), len(lib_cols), 4), 5, True)
    check_pairs(res, cfgs, 2, len(targets))
    both = [c for c in cfgs(0, 0) if c[1] == 0]
    assert len(both) == 2 and both[0][0] == both[1][0] and both[0][3:] == both[1][3:] == (8, 720)
    assert (res.o[0, 0], res.strand[0, 0], res.L[0, 0], res.x[0, 0]) == (0, 0, 8, 720)              # + before -
    full = [c for c in cfgs(1, 1) if c[2] == 0 and c[1] in (-6, 0)]
    assert len(full) == 2 and full[0][0] == full[1][0] == M.best_configuration(cfgs(1, 1))[0] and full[0][4] == 540
    assert (res.o[1, 1], res.strand[1, 1], res.L[1, 1], res.x[1, 1]) == (-6, 0, 6, 540)             # the smaller offset


# ---- 4. batches ---------------------------------------------------------------------------------------------------------------------
def test_batches_do_not_change_a_bit(motifs):
    from kmap_amd import motif_match as K
    info = {}
    one = K.match_motifs(motifs.queries, motifs.targets, True, 5, stage_ms=info)
    assert info["batches"] == 1 and all(info[s] >= 0.0 for s in ("histograms", "tables", "pairs"))
    wide = 8 * K.table_doubles(31, 4)                             # the ranges go down to the narrowest target's 4 columns
    # below the widest query's tables: it is a batch of its own, with its neighbours grouped / split / every query alone
    for budget, n_batches in ((wide - 8, 3), (8 * 80_000, 4), (1, 7)):
        info = {}
        res = K.match_motifs(motifs.queries, motifs.targets, True, 5, table_byte_budget=budget, stage_ms=info)
        assert info["batches"] == n_batches >= 3
        assert res.p_best.tobytes() == one.p_best.tobytes()
        for name in ("o", "strand", "L", "x"):
            np.testing.assert_array_equal(getattr(res, name), getattr(one, name), err_msg=name)


def test_entries_refuse_bad_arguments(motifs):
    from kmap_amd import _ffi
    from kmap_amd import motif_match as K
    lib = _ffi.lib()
    cols = K.quantise_columns(motifs.queries[2])
    d = _ffi.DeviceBuffer.from_numpy(cols)
    out = _ffi.DeviceBuffer(16 * 91 * 4 + 4096)
    w, c0, ml, off = (np.array([16], np.int32), np.array([0], np.int64), np.array([5], np.int32), np.array([0], np.int64))
    P = _ffi.ptr
    n_tab = K.table_doubles(16, 5)
    tab = _ffi.DeviceBuffer(n_tab * 8)
    try:
        assert lib.kmap_match_hist_dev(d.ptr, -1, d.ptr, 16, 1, out.ptr, None) == -1 and "match_hist" in _ffi.last_error()
        assert lib.kmap_match_hist_dev(None, 16, d.ptr, 16, 1, out.ptr, None) == -1
        for bad_w, bad_c0, bad_ml, bad_off, n, word in ((np.array([3], np.int32), c0, ml, off, n_tab, "width=3"),
                                                        (np.array([32], np.int32), c0, ml, off, n_tab, "width=32"),
                                                        (w, np.array([1], np.int64), ml, off, n_tab, "columns of query 0"),
                                                        (w, c0, np.array([17], np.int32), off, n_tab, "min_len=17"),
                                                        (w, c0, np.array([0], np.int32), off, n_tab, "min_len=0"),
                                                        (w, c0, ml, np.array([1], np.int64), n_tab, "tables of query 0"),
                                                        (w, c0, ml, off, n_tab - 1, "tables of query 0")):
            assert lib.kmap_match_tables_dev(out.ptr, 16, 32, 1, P(bad_w), P(bad_c0), P(bad_ml), P(bad_off), tab.ptr, n, None) == -1
            assert "match_tables" in _ffi.last_error() and word in _ffi.last_error()
        assert lib.kmap_match_tables_dev(out.ptr, 16, 0, 1, P(w), P(c0), P(ml), P(off), tab.ptr, n_tab, None) == -1
        tw, tc = np.array([4], np.int32), np.array([0], np.int64)
        p, cfg = _ffi.DeviceBuffer(8), _ffi.DeviceBuffer(16)
        args = (d.ptr, 16, 1, P(w), P(c0), P(ml), P(off), tab.ptr, n_tab, d.ptr, 16, 1)
        assert lib.kmap_match_pairs_dev(*args, P(tw), P(tc), 5, 1, p.ptr, cfg.ptr, None) == -1      # tables from 5 columns, overlaps of 4
        assert "min_len=5" in _ffi.last_error()
        assert lib.kmap_match_pairs_dev(*args, P(np.array([16], np.int32)), P(np.array([1], np.int64)), 5, 1, p.ptr, cfg.ptr, None) == -1
        assert "columns of target 0" in _ffi.last_error()
        assert lib.kmap_match_pairs_dev(*args, P(np.array([16], np.int32)), P(tc), 0, 1, p.ptr, cfg.ptr, None) == -1
        assert "min_overlap=0" in _ffi.last_error()
    finally:
        for b in (d, out, tab):
            b.free()


# ---- 5. the verb --------------------------------------------------------------------------------------------------------------------
FLOAT_FIELDS = ("p_value", "e_value", "q_bh")


def model_rows(queries, targets, min_overlap, revcom, all_against_all):
    """per query {target index: dict of the fields of motif_matches.csv}, from the model alone"""
    from kmap_amd.pwm import pwm_consensus
    ut = [M.quantise(m.counts) for m in targets]
    cols = M.library_columns(ut, revcom)
    rows = []
    for q, qm in enumerate(queries):
        uq = M.quantise(qm.counts)
        ml = min([min_overlap, uq.shape[1]] + [u.shape[1] for u in ut])
        tables = M.null_tables(M.null_hist(uq, cols), len(cols), ml)
        ts = [t for t in range(len(targets)) if not (all_against_all and t == q)]
        best = {t: M.best_configuration(M.configurations(uq, ut[t], tables, min_overlap, revcom)) for t in ts}
        pm = {t: M.p_match(best[t][0], M.n_cfg(uq.shape[1], ut[t].shape[1], min_overlap, revcom)) for t in ts}
        qb = dict(zip(ts, M.bh([pm[t] for t in ts])))
        rows.append({})
        for t in ts:
            p, o, strand, L, x = best[t]
            cons = pwm_consensus(targets[t].counts)
            rows[-1][t] = dict(query=qm.name, target=targets[t].name, altname=targets[t].altname, source=targets[t].source,
                               query_width=str(uq.shape[1]), target_width=str(ut[t].shape[1]), offset=str(o), strand="+-"[strand],
                               overlap=str(L), score=str(x), p_value=pm[t], e_value=pm[t] * len(ts), q_bh=qb[t],
                               query_consensus=pwm_consensus(qm.counts),
                               target_consensus=cons.translate(str.maketrans("ACGT", "TGCA"))[::-1] if strand else cons)
    return rows


def check_match_file(path, rows, queries, targets, top_n):
    from kmap_amd import motif_match as K
    lines = path.read_text().split("\n")
    assert lines[0] + "\n" == K.MATCH_HEADER and lines[-1] == ""
    cols, at = lines[0].split(","), 1
    for q, per_target in enumerate(rows):
        order = sorted(per_target, key=lambda t: (per_target[t]["p_value"], targets[t].name))[:top_n]
        for t in order:
            got = dict(zip(cols, lines[at].split(",")))
            assert len(lines[at].split(",")) == len(cols)
            for name, want in per_target[t].items():
                if name in FLOAT_FIELDS:
                    assert got[name] == repr(float(got[name])) and float(got[name]) == pytest.approx(want, rel=RTOL, abs=0.0), (q, t, name)
                else:
                    assert got[name] == want, (q, t, name)
            at += 1
    assert at == len(lines) - 1


def test_verb_against_a_library(tmp_path, capsys):
    from kmap_amd import library as L
    from kmap_amd import motif_match as K
    out = tmp_path / "out"
    info = K._match_motifs([str(QUERIES)], [str(LIB / "three.meme")], top_n=2, output_dir=out)
    printed = capsys.readouterr().out
    queries, targets = L.read_motif_library(str(QUERIES)), [m for m in L.read_meme(str(LIB / "three.meme")) if m.skip is None]
    assert [m.name for m in info["queries"]] == [m.name for m in queries] == ["q1_planted", "q2_revcom", "q3_other"]
    assert [m.name for m in info["targets"]] == ["M1_CAATCGATAGC", "M2_ACCTACGTA"]
    assert sorted(p.name for p in out.iterdir()) == ["motif_matches.csv", "skipped.csv"]
    rows = model_rows(queries, targets, 5, True, False)
    check_match_file(out / "motif_matches.csv", rows, queries, targets, 2)
    assert (out / "skipped.csv").read_text() == f"name,altname,source,reason\nM3_long,too_wide,{LIB / 'three.meme'},width 40 outside 4..31\n"
    table = [line.split(",") for line in (out / "motif_matches.csv").read_text().split("\n")[1:-1]]
    assert table[0][:9] == ["q1_planted", "M1_CAATCGATAGC", "planted_a", str(LIB / "three.meme"), "15", "11", "2", "+", "11"]
    assert table[2][:2] == ["q2_revcom", "M2_ACCTACGTA"] and table[2][6:9] == ["1", "-", "9"] and table[2][14] == "TACGTAGGT"
    assert float(table[0][11]) < 1e-3 and float(table[2][11]) < 1e-3          # the planted ones are found, far from chance
    assert printed.count("\n") == 4 and printed.startswith("q1_planted: M1_CAATCGATAGC planted_a, offset 2, strand +, 11 columns, p ")
    assert f"match_motifs: 3 queries against 2 library motifs, 1 skipped, both strands: {out}" in printed
    # the forward strand only, every target listed: the reverse complement is no longer found
    K._match_motifs([str(QUERIES)], [str(LIB / "three.meme")], revcom_mode=False, output_dir=tmp_path / "fwd")
    check_match_file(tmp_path / "fwd" / "motif_matches.csv", model_rows(queries, targets, 5, False, False), queries, targets, 10)


def test_verb_all_against_all_families(tmp_path, capsys):
    """twelve motifs: a family of four (a motif, a resampled copy, its reverse complement, a copy with flanks), a family of three
    (one of them reverse-complemented), five unrelated ones"""
    from kmap_amd import library as L
    from kmap_amd import motif_match as K
    rng = np.random.default_rng(1712)

    def resample(C, n=60):
        return np.stack([rng.multinomial(n, (c + 0.5) / (c + 0.5).sum()) for c in C.T]).T
    a, b = M.random_counts(rng, 10, sharp=1.0), M.random_counts(rng, 12, sharp=1.0)
    flanked = np.concatenate([M.random_counts(rng, 2, sharp=0.0), resample(a), M.random_counts(rng, 3, sharp=0.0)], axis=1)
    mats = {"m00_a": a, "m01_rand": M.random_counts(rng, 8), "m02_a_copy": resample(a), "m03_b": b, "m04_rand": M.random_counts(rng, 14),
            "m05_a_rc": resample(a)[::-1, ::-1], "m06_b_rc": resample(b)[::-1, ::-1], "m07_rand": M.random_counts(rng, 6),
            "m08_a_flanked": flanked, "m09_rand": M.random_counts(rng, 11), "m10_b_copy": resample(b), "m11_rand": M.random_counts(rng, 9)}
    src = tmp_path / "motifs"
    src.mkdir()
    for name, C in mats.items():
        np.savetxt(src / f"{name}.csv", C, delimiter=",", fmt="%d")
    out = tmp_path / "out"
    info = K._match_motifs([str(src)], top_n=3, output_dir=out)
    printed = capsys.readouterr().out
    motifs = L.read_motif_library(str(src))
    assert [m.name for m in motifs] == list(mats) and sorted(p.name for p in out.iterdir()) == ["motif_families.csv", "motif_matches.csv", "skipped.csv"]
    rows = model_rows(motifs, motifs, 5, True, True)
    check_match_file(out / "motif_matches.csv", rows, motifs, motifs, 3)
    # the families from the model's E-values
    e = np.full((12, 12), np.nan)
    for q, per_target in enumerate(rows):
        for t, r in per_target.items():
            e[q, t] = r["e_value"]
    links = [(i, j) for i in range(12) for j in range(i + 1, 12) if e[i, j] <= 0.01 and e[j, i] <= 0.01]
    assert all(min(abs(e[i, j] - 0.01), abs(e[j, i] - 0.01)) > 1e-6 for i in range(12) for j in range(12) if i != j)   # none at the edge
    fam_a, fam_b = [0, 2, 5, 8], [3, 6, 10]
    comp = {i: {i} for i in range(12)}
    for i, j in links:
        merged = comp[i] | comp[j]
        for k in merged:
            comp[k] = merged
    assert comp[0] == set(fam_a) and comp[3] == set(fam_b) and all(comp[i] == {i} for i in (1, 4, 7, 9, 11))
    deg = [sum(i in l for l in links) for i in range(12)]
    want = []
    for f, members in enumerate(sorted({tuple(sorted(c)) for c in comp.values()})):
        rep = max(members, key=lambda i: (deg[i], -i))
        for i in members:
            m = motifs[i]
            want.append(f"{f},{len(members)},{m.name},,{m.source},{m.counts.shape[1]},{K.pwm_consensus(m.counts)},{int(i == rep)},{deg[i]}")
    assert (out / "motif_families.csv").read_text() == K.FAMILY_HEADER + "\n".join(want) + "\n"
    assert [w.split(",")[0] for w in want] == ["0"] * 4 + ["1"] + ["2"] * 3 + [str(f) for f in range(3, 7)]
    assert info["families"][0] == [0, 1, 0, 2, 3, 0, 2, 4, 0, 5, 2, 6]
    assert printed.count("\n") == 13 and "12 queries against themselves, 0 skipped, both strands, 7 families" in printed
    assert math.isnan(info["p_match"][3, 3]) and not (out / "motif_matches.csv").read_text().count("m03_b,m03_b,")
