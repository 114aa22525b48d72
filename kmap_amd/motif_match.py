"""`kmap match_motifs`: which motif of a library is the one I found, and which motifs of a library are the same motif in variants?
(the reference's nearest tool, align_conseq, aligns consensus strings.)

Count matrices are compared column by column: every column becomes four integers rint(1024 f), two columns score
s = (1448 - floor(sqrt(sum_b (x_b - y_b)^2))) // 16 in 0..90, a query and a target are laid over one another at every offset and on
both strands, and an overlap's score sum is turned into a p-value by a null built from the library's own columns for that query and
that range of its columns (the Tomtom construction: the library's columns drawn independently), so that long and short overlaps
compare.  csrc/motif_match.hip does the three stages -- the per-column score histograms, the null tables, the pairs --; host code is
parsing, the pair statistics (p over the configurations tried, E-value, Benjamini-Hochberg q), the families of an all-against-all
run and the file formats.  The comparison has no CPU path."""
import math
from collections import namedtuple
from pathlib import Path

import numpy as np

from .pwm import MAX_WIDTH, MIN_WIDTH, _check_counts, pwm_consensus

OUTPUT_DIR, MATCH_FILE, FAMILY_FILE, SKIPPED_FILE = "motif_matches", "motif_matches.csv", "motif_families.csv", "skipped.csv"
MATCH_HEADER = ("query,target,altname,source,query_width,target_width,offset,strand,overlap,score,p_value,e_value,q_bh,"
                "query_consensus,target_consensus\n")
FAMILY_HEADER = "family,size,name,altname,source,width,consensus,is_representative,n_links\n"
QUANT, MAX_COL_SCORE, N_BINS = 1024, 90, 91
MAX_QUERIES_PER_CALL = 65535           # csrc/motif_match.hip: a query is a grid row of the pair kernel

MatchResult = namedtuple("MatchResult", "p_best o strand L x")


def _check_pseudocount(pseudocount):
    a = float(pseudocount)
    if not a >= 0 or math.isinf(a):
        raise ValueError(f"pseudocount {pseudocount} is not a finite number >= 0")
    return a


def quantise_columns(C, pseudocount=1.0):
    """uint16 [w, 4]: row j = rint(1024 f[:, j]) of the count matrix C [4, w] (rows A C G T), f = (C + a / 4) / (sum_b C + a) in
    float64 -- pwm_weights' frequencies --, a = pseudocount.  One row is one 8-byte column of the device arrays.  A column without
    counts needs a > 0: ValueError."""
    C = _check_counts(C)
    a = _check_pseudocount(pseudocount)
    total = C.sum(axis=0) + a
    if (total == 0).any():
        raise ValueError("a column without counts needs a pseudocount > 0 (it has no frequencies)")
    return np.ascontiguousarray(np.rint(QUANT * ((C + a / 4) / total)).astype(np.uint16).T)


# ---- the place of a range's table among a query's tables (the same arithmetic as csrc/motif_match.hip) ---------------------------------
def _len_offset(L, min_len):
    return 0 if L <= min_len else MAX_COL_SCORE * ((L - 1) * L // 2 - (min_len - 1) * min_len // 2) + (L - min_len)


def table_offset(a, b, w, min_len):
    """first double of sf_{a,b} among the tables of a query of width w that holds the ranges of at least min_len columns: by a, then
    by length, 90 L + 1 doubles each"""
    return sum(_len_offset(w - i + 1, min_len) for i in range(a)) + _len_offset(b - a + 1, min_len)


def table_doubles(w, min_len):
    return table_offset(w, w - 1, w, min_len)


def plan_batches(sizes, table_byte_budget):
    """[(first, end)] over the queries: consecutive queries whose tables (sizes, in doubles) fit the budget together; a batch holds
    at least one query, and at most MAX_QUERIES_PER_CALL"""
    batches, first, used = [], 0, 0
    for q, n in enumerate(sizes):
        if q > first and (8 * (used + n) > table_byte_budget or q - first >= MAX_QUERIES_PER_CALL):
            batches.append((first, q))
            first, used = q, 0
        used += n
    if len(sizes) > first:
        batches.append((first, len(sizes)))
    return batches


# ---- the device stages ------------------------------------------------------------------------------------------------------------------
def _columns(cols):
    cols = np.ascontiguousarray(cols, np.uint16)
    if cols.ndim != 2 or cols.shape[1] != 4 or (cols.size and int(cols.max()) > QUANT):
        raise ValueError(f"quantised columns are an [n, 4] array of integers 0..{QUANT}")
    return cols


def _query_arrays(widths, min_lens):
    widths, min_lens = np.ascontiguousarray(widths, np.int32), np.ascontiguousarray(min_lens, np.int32)
    if widths.shape != min_lens.shape or widths.ndim != 1:
        raise ValueError(f"{widths.shape} widths, {min_lens.shape} range lengths")
    if len(widths) and not (MIN_WIDTH <= int(widths.min()) and int(widths.max()) <= MAX_WIDTH):
        raise ValueError(f"a width outside {MIN_WIDTH}..{MAX_WIDTH}")
    if ((min_lens < 1) | (min_lens > widths)).any():
        raise ValueError("a range length outside 1..width")
    col0 = np.zeros(len(widths), np.int64)
    np.cumsum(widths[:-1], out=col0[1:])
    sizes = [table_doubles(int(w), int(m)) for w, m in zip(widths, min_lens)]
    return widths, min_lens, col0, sizes


def column_histograms(qcols, lcols, revcom):
    """uint32 [n_query_cols, 91]: per query column the library columns (with revcom also their reverse-complement twins) by column
    score; columns as quantise_columns writes them"""
    from . import _ffi
    qcols, lcols = _columns(qcols), _columns(lcols)
    if len(qcols) == 0:
        return np.zeros((0, N_BINS), np.uint32)
    qd, ld = _ffi.DeviceBuffer.from_numpy(qcols), _ffi.DeviceBuffer.from_numpy(lcols)
    hd = _ffi.DeviceBuffer(len(qcols) * N_BINS * 4)
    try:
        _ffi.check(_ffi.lib().kmap_match_hist_dev(qd.ptr, len(qcols), ld.ptr, len(lcols), int(bool(revcom)), hd.ptr, None))
        return hd.to_numpy(np.uint32, (len(qcols), N_BINS))
    finally:
        for b in (qd, ld, hd):
            b.free()


def null_tables(H, n_null, widths, min_lens):
    """(tables, offsets): the sf tables of every query from the histogram rows H [sum of widths, 91] and the number of library
    columns n_null behind every row; float64, flat, query q from offsets[q] (table_offset within it), offsets[-1] = the length"""
    from . import _ffi
    widths, min_lens, col0, sizes = _query_arrays(widths, min_lens)
    H = np.ascontiguousarray(H, np.uint32)
    if H.shape != (int(widths.sum()), N_BINS):
        raise ValueError(f"histograms of shape {H.shape}, the widths ask for {(int(widths.sum()), N_BINS)}")
    if int(n_null) < 1:
        raise ValueError(f"n_null {n_null} < 1")
    offsets = np.cumsum([0] + sizes, dtype=np.int64)
    if len(widths) == 0:
        return np.zeros(0, np.float64), offsets
    hd, td = _ffi.DeviceBuffer.from_numpy(H), _ffi.DeviceBuffer(int(offsets[-1]) * 8)
    try:
        for first, end in plan_batches(sizes, 1 << 62):
            _ffi.check(_ffi.lib().kmap_match_tables_dev(hd.ptr, len(H), int(n_null), end - first, _ffi.ptr(widths[first:end]),
                                                        _ffi.ptr(col0[first:end]), _ffi.ptr(min_lens[first:end]),
                                                        _ffi.ptr(np.ascontiguousarray(offsets[first:end])), td.ptr, int(offsets[-1]), None))
        return td.to_numpy(np.float64, (int(offsets[-1]),)), offsets
    finally:
        hd.free()
        td.free()


def _check_match_args(min_overlap, table_byte_budget):
    if int(min_overlap) != min_overlap or min_overlap < 1:
        raise ValueError(f"min_overlap {min_overlap} < 1")
    if int(table_byte_budget) != table_byte_budget or table_byte_budget < 1:
        raise ValueError(f"table_byte_budget {table_byte_budget} < 1")


def match_motifs(queries, targets, revcom=True, min_overlap=5, pseudocount=1.0, table_byte_budget=1 << 30, stage_ms=None):
    """Every query count matrix against every target count matrix ([4, w] each, 4 <= w <= 31).  Returns MatchResult(p_best float64,
    o, strand (0 '+', 1 '-'), L, x int32), each [Q, T]: per pair the configuration (strand, offset o: target column j faces query
    column j + o) with the smallest p = sf_{a,b}[x] of the query's null for the overlapping query columns a..b (L of them, score
    sum x); exactly equal p: the larger L, then '+', then the smaller o.  The null is built from `targets`: for all against all pass
    the same list twice.  The queries' tables are made and used in batches that fit table_byte_budget (at least one query per
    batch); the batches do not change any result.  stage_ms, a dict, receives the device times of the three stages in ms."""
    from . import _ffi
    _check_match_args(min_overlap, table_byte_budget)
    revcom = bool(revcom)
    if len(queries) == 0 or len(targets) == 0:
        raise ValueError("match_motifs: no query or no target")
    qcols = [quantise_columns(C, pseudocount) for C in queries]
    tcols = [quantise_columns(C, pseudocount) for C in targets]
    t_width = np.array([len(c) for c in tcols], np.int32)
    t_col0 = np.zeros(len(tcols), np.int64)
    np.cumsum(t_width[:-1], out=t_col0[1:])
    q_all, t_all = np.concatenate(qcols), np.concatenate(tcols)
    q_width = np.array([len(c) for c in qcols], np.int32)
    q_width, q_min_len, q_col0, sizes = _query_arrays(q_width, np.minimum(q_width, min(int(min_overlap), int(t_width.min()))))
    batches = plan_batches(sizes, int(table_byte_budget))
    n_q, n_t = len(qcols), len(tcols)
    n_null = len(t_all) * (2 if revcom else 1)
    n_table = max(sum(sizes[first:end]) for first, end in batches)

    lib = _ffi.lib()
    bufs = []

    def dev(x):
        bufs.append(_ffi.DeviceBuffer.from_numpy(x) if isinstance(x, np.ndarray) else _ffi.DeviceBuffer(x))
        return bufs[-1]
    ev = [_ffi.Event() for _ in range(4)] if stage_ms is not None else None
    ms = [0.0, 0.0, 0.0]

    def mark(i):
        if ev is not None:
            ev[i].record(None)
    try:
        qd, ld, hd = dev(q_all), dev(t_all), dev(len(q_all) * N_BINS * 4)
        td, pd, cd = dev(n_table * 8), dev(n_q * n_t * 8), dev(n_q * n_t * 16)
        mark(0)
        _ffi.check(lib.kmap_match_hist_dev(qd.ptr, len(q_all), ld.ptr, len(t_all), int(revcom), hd.ptr, None))
        mark(1)
        if ev is not None:
            _ffi.sync()
            ms[0] = ev[0].elapsed_ms(ev[1])
        for first, end in batches:
            toff = np.cumsum([0] + sizes[first:end - 1], dtype=np.int64)
            meta = (_ffi.ptr(np.ascontiguousarray(q_width[first:end])), _ffi.ptr(np.ascontiguousarray(q_col0[first:end])),
                    _ffi.ptr(np.ascontiguousarray(q_min_len[first:end])), _ffi.ptr(toff))
            mark(1)
            _ffi.check(lib.kmap_match_tables_dev(hd.ptr, len(q_all), n_null, end - first, *meta, td.ptr, n_table, None))
            mark(2)
            _ffi.check(lib.kmap_match_pairs_dev(qd.ptr, len(q_all), end - first, *meta, td.ptr, n_table, ld.ptr, len(t_all), n_t,
                                                _ffi.ptr(t_width), _ffi.ptr(t_col0), int(min_overlap), int(revcom),
                                                pd.ptr + first * n_t * 8, cd.ptr + first * n_t * 16, None))
            mark(3)
            if ev is not None:
                _ffi.sync()
                ms[1] += ev[1].elapsed_ms(ev[2])
                ms[2] += ev[2].elapsed_ms(ev[3])
        p = pd.to_numpy(np.float64, (n_q, n_t))
        cfg = cd.to_numpy(np.int32, (n_q, n_t, 4))
    finally:
        for b in bufs:
            b.free()
    if stage_ms is not None:
        stage_ms.update(histograms=ms[0], tables=ms[1], pairs=ms[2], batches=len(batches))
    return MatchResult(p, *(np.ascontiguousarray(cfg[:, :, i]) for i in range(4)))


# ---- pair statistics and families (host) --------------------------------------------------------------------------------------------
def n_configurations(w_q, w_t, min_overlap, revcom):
    m = min(int(min_overlap), int(w_q), int(w_t))
    return (int(w_q) + int(w_t) - 2 * m + 1) * (2 if revcom else 1)


def pair_statistics(p_best, q_widths, t_widths, min_overlap, revcom, all_against_all=False):
    """(p_match, e_value, q_bh), float64 [Q, T]: p_match = 1 - (1 - p_best)^n_cfg over the n_cfg configurations of the pair (as
    -expm1(n_cfg log1p(-p_best)); 1 at p_best = 1), e_value = p_match times the number of targets the query is reported against,
    q_bh = library.bh_qvalues over those targets.  all_against_all: target t is motif t of the queries; a motif is not reported
    against itself, the diagonal is nan and the number of targets is T - 1."""
    from .library import bh_qvalues
    p_best = np.asarray(p_best, np.float64)
    n_q, n_t = p_best.shape
    n_cfg = np.array([[n_configurations(wq, wt, min_overlap, revcom) for wt in t_widths] for wq in q_widths], np.float64)
    with np.errstate(divide="ignore"):
        p_match = np.where(p_best >= 1.0, 1.0, -np.expm1(n_cfg * np.log1p(-np.minimum(p_best, 1.0))))
    n_rep = n_t - 1 if all_against_all else n_t
    e_value, q_bh = p_match * n_rep, np.full((n_q, n_t), np.nan)
    for q in range(n_q):
        keep = np.arange(n_t) != q if all_against_all else np.ones(n_t, bool)
        if keep.any():
            q_bh[q, keep] = bh_qvalues(p_match[q, keep])
    if all_against_all:
        idx = np.arange(min(n_q, n_t))
        p_match[idx, idx] = e_value[idx, idx] = np.nan
    return p_match, e_value, q_bh


def family_links(e_value, family_e_value):
    """[(i, j)], i < j: e_value[i, j] and e_value[j, i] are both at most family_e_value"""
    e = np.asarray(e_value, np.float64)
    ok = (e <= family_e_value) & (e.T <= family_e_value)     # nan (the diagonal) compares False
    return [(int(i), int(j)) for i, j in zip(*np.nonzero(np.triu(ok, 1)))]


def families(n, links):
    """(family, size, is_representative, n_links), one entry per motif 0..n-1: the connected components of the links (union-find),
    numbered in the order of their smallest member; n_links = the motif's links (all of them lie inside its family); the
    representative of a family is its member with the most links, on a tie the smallest index."""
    parent = list(range(n))

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i
    n_links = [0] * n
    for i, j in sorted(set((min(int(i), int(j)), max(int(i), int(j))) for i, j in links)):
        if not (0 <= i < j < n):
            raise ValueError(f"link ({i}, {j}) outside the {n} motifs")
        n_links[i] += 1
        n_links[j] += 1
        a, b = find(i), find(j)
        if a != b:
            parent[max(a, b)] = min(a, b)                    # the root is the smallest member
    roots = [find(i) for i in range(n)]
    number = {r: f for f, r in enumerate(sorted(set(roots)))}
    family = [number[r] for r in roots]
    size, rep = [0] * len(number), [None] * len(number)
    for i, f in enumerate(family):
        size[f] += 1
        if rep[f] is None or n_links[i] > n_links[rep[f]]:
            rep[f] = i
    return family, [size[f] for f in family], [rep[f] == i for i, f in enumerate(family)], n_links


# ---- the verb ---------------------------------------------------------------------------------------------------------------------------
_COMPLEMENT = str.maketrans("ACGT", "TGCA")


def revcom_text(s):
    return s.translate(_COMPLEMENT)[::-1]


def match_line(q, t, o, strand, L, x, p_match, e_value, q_bh):
    """one line of motif_matches.csv (q, t: LibraryMotif)"""
    cons = pwm_consensus(t.counts)
    return (f"{q.name},{t.name},{t.altname},{t.source},{q.counts.shape[1]},{t.counts.shape[1]},{int(o)},{'-' if strand else '+'},{int(L)},"
            f"{int(x)},{float(p_match)!r},{float(e_value)!r},{float(q_bh)!r},{pwm_consensus(q.counts)},"
            f"{revcom_text(cons) if strand else cons}\n")


def top_targets(p_match_row, names, top_n, skip=None):
    """the top_n targets of one query: by p_match ascending, then by name; `skip` = the query's own index, left out"""
    order = sorted((t for t in range(len(names)) if t != skip), key=lambda t: (float(p_match_row[t]), names[t]))
    return order[:int(top_n)]


def _match_motifs(query_files, library_files=None, revcom_mode=True, min_overlap=5, pseudocount=1.0, nsites_default=20, top_n=10,
                  family_e_value=0.01, output_dir=None, table_byte_budget=1 << 30):
    """`kmap match_motifs`: query files (+ library files; without them the queries are matched against themselves) ->
    motif_matches.csv, skipped.csv and, all against all, motif_families.csv in output_dir (default ./motif_matches).  Every file is
    parsed and every argument checked before the device is touched or a file is written.  Under a torch.distributed launch rank 0
    works alone.  Returns a dict: queries, targets (LibraryMotif lists), skipped, result (MatchResult), p_match, e_value, q_bh and,
    all against all, families (families()' four lists)."""
    from .kmer_count import rank0_only
    from .library import SKIPPED_HEADER, _field, read_motif_library
    if not rank0_only():
        return None
    query_files, library_files = [str(f) for f in query_files], [str(f) for f in (library_files or [])]
    if not query_files:
        raise ValueError("match_motifs: no query file given")
    _check_match_args(min_overlap, table_byte_budget)
    a = _check_pseudocount(pseudocount)
    if int(nsites_default) != nsites_default or nsites_default < 1:
        raise ValueError(f"nsites_default {nsites_default} < 1")
    if int(top_n) != top_n or top_n < 1:
        raise ValueError(f"top_n {top_n} < 1")
    if not float(family_e_value) >= 0 or math.isinf(float(family_e_value)):
        raise ValueError(f"family_e_value {family_e_value} is not a finite number >= 0")
    revcom, all_against_all = bool(revcom_mode), not library_files

    skipped = []

    def load(files):
        kept = []
        for f in files:
            for m in read_motif_library(f, nsites_default):
                if m.skip is None:
                    try:
                        quantise_columns(m.counts, a)
                    except ValueError as exc:
                        raise ValueError(f"{m.source}: motif {m.name}: {exc}") from None
                (kept if m.skip is None else skipped).append(m)
        return kept
    queries = load(query_files)
    targets = queries if all_against_all else load(library_files)
    if not queries or not targets:
        raise ValueError(f"match_motifs: none of the motifs of the {'query' if not queries else 'library'} files can be used "
                         f"(the first: {skipped[0].name}: {skipped[0].skip})")
    if all_against_all and len(queries) < 2:
        raise ValueError("match_motifs: one motif and no library file: there is nothing to match it against")

    res = match_motifs([m.counts for m in queries], [m.counts for m in targets], revcom, min_overlap, a, table_byte_budget)
    q_w, t_w = [m.counts.shape[1] for m in queries], [m.counts.shape[1] for m in targets]
    p_match, e_value, q_bh = pair_statistics(res.p_best, q_w, t_w, min_overlap, revcom, all_against_all)
    out_info = dict(queries=queries, targets=targets, skipped=skipped, result=res, p_match=p_match, e_value=e_value, q_bh=q_bh)

    out = Path(OUTPUT_DIR if output_dir is None else output_dir)
    out.mkdir(parents=True, exist_ok=True)
    t_names = [m.name for m in targets]
    best_lines = []
    with open(out / MATCH_FILE, "w") as fh:
        fh.write(MATCH_HEADER)
        for q, qm in enumerate(queries):
            for rank, t in enumerate(top_targets(p_match[q], t_names, top_n, q if all_against_all else None)):
                fh.write(match_line(qm, targets[t], res.o[q, t], res.strand[q, t], res.L[q, t], res.x[q, t], p_match[q, t], e_value[q, t],
                                    q_bh[q, t]))
                if rank == 0:
                    tm = targets[t]
                    best_lines.append(f"{qm.name}: {tm.name}{' ' + tm.altname if tm.altname else ''}, offset {int(res.o[q, t])}, strand "
                                      f"{'-' if res.strand[q, t] else '+'}, {int(res.L[q, t])} columns, p {p_match[q, t]:.3g}, "
                                      f"E {e_value[q, t]:.3g}, q {q_bh[q, t]:.3g}")
    with open(out / SKIPPED_FILE, "w") as fh:
        fh.write(SKIPPED_HEADER)
        fh.write("".join(f"{m.name},{m.altname},{m.source},{_field(m.skip)}\n" for m in skipped))
    n_families = None
    if all_against_all:
        fam = families(len(queries), family_links(e_value, float(family_e_value)))
        out_info["families"] = fam
        n_families = len(set(fam[0]))
        with open(out / FAMILY_FILE, "w") as fh:
            fh.write(FAMILY_HEADER)
            for i in sorted(range(len(queries)), key=lambda i: (fam[0][i], i)):
                m = queries[i]
                fh.write(f"{fam[0][i]},{fam[1][i]},{m.name},{m.altname},{m.source},{m.counts.shape[1]},{pwm_consensus(m.counts)},"
                         f"{int(fam[2][i])},{fam[3][i]}\n")
    print("\n".join(best_lines))
    print(f"match_motifs: {len(queries)} {'query' if len(queries) == 1 else 'queries'} against "
          f"{'themselves' if all_against_all else str(len(targets)) + ' library motifs'}, {len(skipped)} skipped, "
          f"{'both strands' if revcom else 'forward strand'}" + (f", {n_families} families" if all_against_all else "") + f": {out}")
    return out_info
