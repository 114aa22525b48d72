"""`kmap discover_pwms`: count matrices found in the reads themselves, from the k-mers that are enriched against control reads
(the reference has no such verb).

enrich_kmers ranks k-mers, refine_pwm iterates one matrix, evaluate_pwm and rank_motif_library score matrices against a control and
match_motifs groups them; this module is the step that makes the matrices.  The best k-mers by enrich_z become seeds: a one-hot
count matrix, padded with empty flanks, whose first iteration selects the Hamming ball around the k-mer -- the project's own motif
definition -- and whose later iterations are refine_pwm's.  All seeds are refined in lockstep: one DeviceSeq.library_counts call
(csrc/pwm_sites.hip) per round for the matrices still running.  Every result is evaluated against the control as
rank_motif_library does it, the results are matched all against all as match_motifs does it, and every family is represented by its
member with the largest Mann-Whitney z.  The core takes its device work as callables, so it runs on any count, histogram and match
function; host code is the loops, small-matrix arithmetic and the file formats.  The matrices are evaluated on the reads they were
counted from, so mw_z is optimistic: a hold-out split is not made.  With --erase_rounds above 1 the sites
of what a round found are erased from reads and control (DeviceSeq.erase_sites, csrc/pwm_erase.hip) and the next round takes its
seeds and its counts from what is left, so that a weaker motif behind a dominant one gets seeds of its own; the evaluation stays
on the original reads in every round."""
import math
from pathlib import Path

import numpy as np

from .evaluate import EVAL_HEADER, MAX_BINS, eval_line, evaluate_histograms
from .library import _field, bh_qvalues, log10_p_of_z
from .pwm import MAX_WIDTH, MIN_WIDTH, pwm_consensus, pwm_threshold, pwm_weights
from .refine import information_bits, pad_matrix

OUTPUT_DIR, RANK_FILE, TRACE_FILE, MEME_FILE, MATRIX_DIR = "pwm_discovery", "discovered_rank.csv", "discover_trace.csv", "discovered.meme", "matrices"
MATRIX_FILE = "seed{i}_{consensus}.csv"
RANK_HEADER = ("rank,name,seed,seed_fg,seed_control,seed_z,status,iterations,n_selected,n_minus,information_bits,family,family_size,"
               "is_representative," + EVAL_HEADER.rstrip("\n").split(",", 1)[1] + ",log10_p,q_bh\n")
TRACE_HEADER = "seed,iteration,threshold,n_selected,n_minus,consensus,information_bits,cells_changed\n"
MAX_SEEDS = 1024


# ---- seeds ------------------------------------------------------------------------------------------------------------------------
def seed_matrix(kmer, n0=20):
    """the count matrix of a seed: 4 x k, n0 at the k-mer's base of every column, 0 elsewhere"""
    kmer = str(kmer)
    if not MIN_WIDTH <= len(kmer) <= MAX_WIDTH or set(kmer) - set("ACGT"):
        raise ValueError(f"seed {kmer!r} is not {MIN_WIDTH}..{MAX_WIDTH} letters of A, C, G, T")
    if int(n0) != n0 or n0 < 1:
        raise ValueError(f"seed_count {n0} < 1")
    C = np.zeros((4, len(kmer)), np.int64)
    C[["ACGT".index(c) for c in kmer], np.arange(len(kmer))] = int(n0)
    return C


def seed_threshold(kmer, n0, flank, mismatches, pseudocount):
    """t1 = (k - d) m + d x of the padded seed matrix's weights: every core column has the match weight m at the k-mer's base and the
    mismatch weight x at the three others, every flank column weighs 0, so the windows that score t1 or more are exactly the windows
    whose core lies within d mismatches of the k-mer.  Needs a pseudocount > 0 (pwm_weights' rule for the zero counts) and
    0 <= d < k."""
    k, d = len(kmer), int(mismatches)
    if d != mismatches or not 0 <= d < k:
        raise ValueError(f"seed_mismatches {mismatches} outside 0..{k - 1} (seed_len - 1)")
    W = pwm_weights(pad_matrix(seed_matrix(kmer, n0), flank), pseudocount)
    f = int(flank)
    m, x = int(W.max(axis=0)[f]), int(W.min(axis=0)[f])
    if not m > x:
        raise ValueError(f"seed_count {n0} with pseudocount {pseudocount}: the match weight {m} is not above the mismatch weight {x}")
    return (k - d) * m + d * x


# ---- the lockstep refinement ------------------------------------------------------------------------------------------------------
def refine_many(C0s, counts_fn, flank=0, p_value=1e-4, pseudocount=1.0, max_iter=20, first_thresholds=None):
    """refine.refine_matrix with `select best` for a list of matrices in lockstep: per round ONE call
    counts_fn(Ws, ts) -> (Cs, n_selected, n_minus) for the matrices that are still running, in their order.  Per matrix the rules are
    refine_matrix's: C = C0 padded; W = pwm_weights(C, a), t = pwm_threshold(W, p)[0] -- in the first round first_thresholds[i]
    where that list is given --, C' from counts_fn; `converged` when C' == C, `cycle` when C' equals an earlier matrix of the run
    (the padded input included), `no_hits` when nothing was selected, `max_iter` after max_iter rounds.  Returns [(result, status,
    trace)]: result = the last matrix built from at least one selected window, else the padded input; trace rows are
    (iteration, threshold, n_selected, n_minus, consensus of C', information_bits of C', cells_changed)."""
    if int(max_iter) != max_iter or max_iter < 1:
        raise ValueError(f"max_iter {max_iter} is not an integer >= 1")
    Cs = [pad_matrix(C0, flank) for C0 in C0s]
    if first_thresholds is not None and len(first_thresholds) != len(Cs):
        raise ValueError(f"{len(Cs)} matrices, {len(first_thresholds)} first thresholds")
    results, seen = list(Cs), [[C] for C in Cs]
    status, traces = ["max_iter"] * len(Cs), [[] for _ in Cs]
    running = list(range(len(Cs)))
    for it in range(1, int(max_iter) + 1):
        if not running:
            break
        Ws = [pwm_weights(Cs[i], pseudocount) for i in running]
        if it == 1 and first_thresholds is not None:
            ts = [int(first_thresholds[i]) for i in running]
        else:
            ts = [pwm_threshold(W, p_value)[0] for W in Ws]
        new, n_sel, n_minus = counts_fn(Ws, ts)
        if not len(new) == len(n_sel) == len(n_minus) == len(running):
            raise ValueError(f"counts_fn returned {len(new)} matrices for {len(running)}")
        still = []
        for i, t, Cn, ns, nm in zip(running, ts, new, n_sel, n_minus):
            C, Cn = Cs[i], np.asarray(Cn, np.int64)
            if Cn.shape != C.shape:
                raise ValueError(f"counts_fn returned shape {Cn.shape}, expected {C.shape}")
            traces[i].append((it, int(t), int(ns), int(nm), pwm_consensus(Cn), information_bits(Cn, pseudocount),
                              int(np.count_nonzero(Cn != C))))
            if ns == 0:
                status[i] = "no_hits"
                continue
            results[i] = Cn
            if np.array_equal(Cn, C):
                status[i] = "converged"
                continue
            if any(np.array_equal(Cn, S) for S in seen[i]):
                status[i] = "cycle"
                continue
            seen[i].append(Cn)
            Cs[i] = Cn
            still.append(i)
        running = still
    return [(results[i], status[i], traces[i]) for i in range(len(Cs))]


def trace_line(seed, row):
    return "%d,%d,%d,%d,%d,%s,%.3f,%d\n" % ((seed,) + tuple(row))


# ---- the core: seeds -> refined, evaluated and grouped matrices ---------------------------------------------------------------------
def _z_key(z, i):
    """mw_z descending, nan last, then the seed rank"""
    return (z != z, 0.0 if z != z else -z, i)


def group_families(Cs, mw_z, match_fn, revcom, min_overlap, pseudocount, family_e_value):
    """(family, family_size, is_representative) per matrix: match_motifs' all-against-all families (motif_match.pair_statistics,
    family_links, families: the connected components), but a family's representative is its member with the largest mw_z -- on a tie
    or with nan the smaller index.  A single matrix is its own family and match_fn is not called."""
    from .motif_match import families, family_links, pair_statistics
    n = len(Cs)
    if n == 1:
        return [0], [1], [True]
    res = match_fn(Cs, Cs, revcom, min_overlap, pseudocount)
    widths = [C.shape[1] for C in Cs]
    _, e_value, _ = pair_statistics(res.p_best, widths, widths, min_overlap, revcom, all_against_all=True)
    family, size, _, _ = families(n, family_links(e_value, float(family_e_value)))
    rep = {}
    for i, f in enumerate(family):
        if f not in rep or _z_key(mw_z[i], i) < _z_key(mw_z[rep[f]], rep[f]):
            rep[f] = i
    return family, size, [rep[f] == i for i, f in enumerate(family)]


def discover_core(seeds, counts_fn, hist_fn, match_fn, revcom, flank=2, seed_mismatches=1, seed_count=20, p_value=1e-4,
                  pseudocount=1.0, max_iter=20, min_overlap=5, family_e_value=0.01, min_reads=10):
    """Steps 2 - 7 of DESIGN.md section 21 on injected device work.
    seeds: [(kmer, fg_count, control_count, z)] in rank order;
    counts_fn(Ws, ts) -> (Cs, n_selected, n_minus): DeviceSeq.library_counts on the reads;
    hist_fn(Ws, los, n_bins) -> (Hf, fg_unscorable, Hc, control_unscorable): the best-score histograms of reads and control per
    matrix and the reads without a valid window (DeviceSeq.library_histograms on either set);
    match_fn(queries, targets, revcom, min_overlap, pseudocount) -> an object with p_best [Q, T]: motif_match.match_motifs.
    Returns one dict per seed, in seed order: evaluate_histograms' fields plus seed_rank, name, seed, seed_fg, seed_control, seed_z,
    counts, status, trace, iterations, n_selected, n_minus, information_bits, family, family_size, is_representative, lo,
    fg_unscorable, control_unscorable, log10_p, q_bh, rank (its line in discovered_rank.csv)."""
    out = refine_and_evaluate(seeds, counts_fn, hist_fn, flank, seed_mismatches, seed_count, p_value, pseudocount, max_iter, min_reads)
    return group_and_rank(out, match_fn, revcom, min_overlap, pseudocount, family_e_value)


def refine_and_evaluate(seeds, counts_fn, hist_fn, flank=2, seed_mismatches=1, seed_count=20, p_value=1e-4, pseudocount=1.0,
                        max_iter=20, min_reads=10, first_index=0):
    """discover_core's steps up to the evaluation for one list of seeds, numbered from first_index on: its dicts without q_bh, the
    family fields and rank (threshold_p is pwm_threshold(W, p_value)[0] of the result's weights)"""
    seeds = [(str(s[0]), int(s[1]), int(s[2]), float(s[3])) for s in seeds]
    if not seeds:
        raise ValueError("discover_pwms: no seed: no k-mer is enriched in the reads (z > 0) at this seed_len and min_count")
    firsts = [seed_threshold(s[0], seed_count, flank, seed_mismatches, pseudocount) for s in seeds]
    runs = refine_many([seed_matrix(s[0], seed_count) for s in seeds], counts_fn, flank, p_value, pseudocount, max_iter, firsts)

    plans = []
    for i, (C, _, _) in enumerate(runs):
        W = pwm_weights(C, pseudocount)
        t, lo, hi = pwm_threshold(W, p_value)
        if hi - lo + 1 > MAX_BINS:
            raise ValueError(f"discover_pwms: seed {first_index + i}: scores from {lo} to {hi}: more than 2^22 different scores")
        plans.append((W, t, lo, hi))
    Hf, fg_un, Hc, ctl_un = hist_fn([p[0] for p in plans], [p[2] for p in plans], [p[3] - p[2] + 1 for p in plans])
    out = []
    for i, (s, (C, status, trace), (W, t, lo, hi)) in enumerate(zip(seeds, runs, plans)):
        st = evaluate_histograms(Hf[i], Hc[i], lo, t, min_reads)
        last = trace[-1]
        built = [row for row in trace if row[2] > 0]             # the rounds with a selected window: the last one made the result
        idx = first_index + i
        st.update(seed_rank=idx, name=_field(f"seed{idx}_{pwm_consensus(C)}"), seed=s[0], seed_fg=s[1], seed_control=s[2], seed_z=s[3],
                  counts=C, status=status, trace=trace, iterations=len(trace), n_selected=built[-1][2] if built else last[2],
                  n_minus=built[-1][3] if built else last[3], information_bits=information_bits(C, pseudocount), lo=lo,
                  fg_unscorable=int(fg_un[i]), control_unscorable=int(ctl_un[i]), log10_p=log10_p_of_z(st["mw_z"]))
        out.append(st)
    return out


def group_and_rank(out, match_fn, revcom, min_overlap=5, pseudocount=1.0, family_e_value=0.01):
    """q_bh, the families with their representatives and rank over all of refine_and_evaluate's dicts, in place; returns them"""
    for st, q in zip(out, bh_qvalues([10.0 ** st["log10_p"] for st in out]).tolist()):
        st["q_bh"] = q
    fam = group_families([st["counts"] for st in out], [st["mw_z"] for st in out], match_fn, revcom, min_overlap, pseudocount,
                         family_e_value)
    for st, f, size, rep in zip(out, *fam):
        st.update(family=int(f), family_size=int(size), is_representative=bool(rep))
    for rank, i in enumerate(sorted(range(len(out)), key=lambda i: _z_key(out[i]["mw_z"], i))):
        out[i]["rank"] = rank
    return out


# ---- the rounds: discover, erase what was found, discover again ---------------------------------------------
MAX_ERASE_ROUNDS = 16


def check_erase_rounds(erase_rounds):
    return _check_int("erase_rounds", erase_rounds, 1, MAX_ERASE_ROUNDS)


def discover_rounds(seeds_fn, counts_fn, erase_fn, hist_fn, match_fn, revcom, erase_rounds=1, flank=2, seed_mismatches=1, seed_count=20,
                    p_value=1e-4, pseudocount=1.0, max_iter=20, min_overlap=5, family_e_value=0.01, min_reads=10):
    """discover_core in up to erase_rounds rounds with the found sites erased in between, on injected device work.
    seeds_fn(round) -> [(kmer, fg_count, control_count, z)]: round 1 from the original reads and control, later rounds from what
    the erasures left of both (select_seeds' use_work);
    counts_fn(Ws, ts) in round 1, counts_fn(Ws, ts, use_work=True) in the later rounds: DeviceSeq.library_counts on the reads;
    erase_fn(Ws, ts) -> (fg_hits[n], fg_covered[n], fg_new, control_hits[n], control_covered[n], control_new): DeviceSeq.erase_sites
    (use_work=True) on the reads and on the control;
    hist_fn and match_fn are discover_core's; hist_fn sees the original reads and the original control in every round, so mw_z is
    comparable between rounds.
    A round runs refine_and_evaluate on its seeds, numbered on from the round before.  After every round but the last the round's
    own representatives (group_families over the round's matrices alone) that were built from at least one selected window are
    erased: every hit at threshold_p.  The rounds end early when a later round has no seed, when a round has nothing to erase, or
    when an erasure takes no position from the reads (the next round would be this one again); round 1 without a seed is
    discover_core's ValueError.  q_bh, the families, their representatives and rank are group_and_rank's over the seeds of all
    rounds: one match_fn call over the union.  Returns (results: discover_core's dicts plus `round`, in seed order; erase_log: one
    dict per erasure: round, rows [(name, threshold, fg_hits, fg_covered, control_hits, control_covered)], fg_new, control_new).
    With erase_rounds 1 the results are discover_core's and the log is empty."""
    n_rounds = check_erase_rounds(erase_rounds)
    results, erase_log = [], []
    for r in range(1, n_rounds + 1):
        seeds = list(seeds_fn(r))
        if r > 1 and not seeds:
            break
        fn = counts_fn if r == 1 else (lambda Ws, ts: counts_fn(Ws, ts, use_work=True))
        out = refine_and_evaluate(seeds, fn, hist_fn, flank, seed_mismatches, seed_count, p_value, pseudocount, max_iter, min_reads,
                                  first_index=len(results))
        for st in out:
            st["round"] = r
        results += out
        if r == n_rounds:
            break
        _, _, is_rep = group_families([st["counts"] for st in out], [st["mw_z"] for st in out], match_fn, revcom, min_overlap,
                                      pseudocount, family_e_value)
        found = [st for st, rep in zip(out, is_rep) if rep and st["n_selected"] > 0]
        if not found:
            break
        ts = [int(st["threshold_p"]) for st in found]
        fh, fc, f_new, ch, cc, c_new = erase_fn([pwm_weights(st["counts"], pseudocount) for st in found], ts)
        erase_log.append(dict(round=r, fg_new=int(f_new), control_new=int(c_new),
                              rows=[(st["name"], t, int(a), int(b), int(c), int(d)) for st, t, a, b, c, d in zip(found, ts, fh, fc, ch, cc)]))
        if int(f_new) == 0:
            break
    return group_and_rank(results, match_fn, revcom, min_overlap, pseudocount, family_e_value), erase_log


# ---- files ------------------------------------------------------------------------------------------------------------------------
ERASE_FILE = "discover_erase.csv"
ERASE_HEADER = "round,name,threshold,fg_hits,fg_covered,control_hits,control_covered\n"
ERASE_TOTALS_HEADER = "round,fg_new,control_new\n"


def rank_line(st, pseudocount, revcom):
    """one line of discovered_rank.csv: pwm_eval.csv's columns from `width` on in eval_line's formatting, between the seed's own
    fields and its p and q"""
    C = st["counts"]
    tail = eval_line(0, C.shape[1], pwm_consensus(C), pseudocount, revcom, st["fg_unscorable"], st["control_unscorable"],
                     st).rstrip("\n").split(",", 1)[1]
    return (f"{st['rank']},{st['name']},{st['seed']},{st['seed_fg']},{st['seed_control']},{float(st['seed_z'])!r},{st['status']},"
            f"{st['iterations']},{st['n_selected']},{st['n_minus']},{st['information_bits']:.3f},{st['family']},{st['family_size']},"
            f"{int(st['is_representative'])},{tail},{float(st['log10_p'])!r},{float(st['q_bh'])!r}\n")


def meme_text(motifs, revcom=True):
    """MEME minimal text of [(name, altname, counts)] that library.read_motif_library reads back to the same counts: every motif's
    columns must have one common sum >= 1, written as nsites=; the probabilities count / nsites are written with repr, and
    rint(p nsites) is the count again"""
    lines = ["MEME version 4", "", "ALPHABET= ACGT", "", f"strands: {'+ -' if revcom else '+'}", "",
             "Background letter frequencies", "A 0.25 C 0.25 G 0.25 T 0.25", ""]
    for name, altname, C in motifs:
        C = np.asarray(C, np.int64)
        sums = C.sum(axis=0)
        n = int(sums[0])
        if n < 1 or (sums != n).any():
            raise ValueError(f"motif {name}: the columns do not have one common sum >= 1")
        lines.append(f"MOTIF {_field(name)} {_field(altname)}".rstrip())
        lines.append(f"letter-probability matrix: alength= 4 w= {C.shape[1]} nsites= {n} E= 0")
        lines += [" " + " ".join(repr(float(int(c) / n)) for c in C[:, j]) for j in range(C.shape[1])]
        lines.append("")
    return "\n".join(lines) + "\n"


def write_discovery(out_dir, results, pseudocount, revcom, erase_log=None):
    """the files of `kmap discover_pwms` from discover_core's results; returns the representatives in rank order.  erase_log
    (discover_rounds', for a run with --erase_rounds above 1; may be empty): discovered_rank.csv and discover_trace.csv get a last
    column `round`, and discover_erase.csv lists what every erasure took: a row per erased matrix, and under them the positions
    every erasure took from the reads and from the control."""
    out = Path(out_dir)
    (out / MATRIX_DIR).mkdir(parents=True, exist_ok=True)
    ranked = sorted(results, key=lambda st: st["rank"])

    def with_round(text, st):
        return text if erase_log is None else text[:-1] + f",{st['round']}\n"
    with open(out / RANK_FILE, "w") as fh:
        fh.write(RANK_HEADER if erase_log is None else RANK_HEADER[:-1] + ",round\n")
        fh.write("".join(with_round(rank_line(st, pseudocount, revcom), st) for st in ranked))
    with open(out / TRACE_FILE, "w") as fh:
        fh.write(TRACE_HEADER if erase_log is None else TRACE_HEADER[:-1] + ",round\n")
        for st in results:
            fh.write("".join(with_round(trace_line(st["seed_rank"], row), st) for row in st["trace"]))
    if erase_log is not None:
        with open(out / ERASE_FILE, "w") as fh:
            fh.write(ERASE_HEADER)
            for e in erase_log:
                fh.write("".join("%d,%s,%d,%d,%d,%d,%d\n" % ((e["round"],) + tuple(row)) for row in e["rows"]))
            fh.write(ERASE_TOTALS_HEADER)
            fh.write("".join(f"{e['round']},{e['fg_new']},{e['control_new']}\n" for e in erase_log))
    for st in results:
        np.savetxt(out / MATRIX_DIR / MATRIX_FILE.format(i=st["seed_rank"], consensus=pwm_consensus(st["counts"])), st["counts"],
                   delimiter=",", fmt="%d")
    reps = [st for st in ranked if st["is_representative"]]
    usable = [st for st in reps if st["n_selected"] > 0]         # a seed without a selected window is still its padded one-hot matrix
    with open(out / MEME_FILE, "w") as fh:
        fh.write(meme_text([(st["name"], st["seed"], st["counts"]) for st in usable], revcom))
    return reps


# ---- the verb ---------------------------------------------------------------------------------------------------------------------
def _check_int(name, value, lo, hi=None):
    if isinstance(value, bool) or int(value) != value or value < lo or (hi is not None and value > hi):
        raise ValueError(f"{name} {value} outside {lo}..{hi}" if hi is not None else f"{name} {value} < {lo}")
    return int(value)


def check_arguments(seed_len=8, n_seeds=64, seed_mismatches=1, seed_count=20, flank=2, min_count=2, p_value=1e-4, pseudocount=1.0,
                    max_iter=20, min_overlap=5, family_e_value=0.01, erase_rounds=1):
    """every ValueError of the verb's numbers, each with its own message"""
    k = _check_int("seed_len", seed_len, MIN_WIDTH, MAX_WIDTH)
    f = _check_int("flank", flank, 0)
    if k + 2 * f > MAX_WIDTH:
        raise ValueError(f"seed_len {k} + 2 x flank {f} = {k + 2 * f} is more than {MAX_WIDTH}")
    _check_int("n_seeds", n_seeds, 1, MAX_SEEDS)
    if isinstance(seed_mismatches, bool) or int(seed_mismatches) != seed_mismatches or not 0 <= seed_mismatches < k:
        raise ValueError(f"seed_mismatches {seed_mismatches} outside 0..{k - 1} (seed_len - 1)")
    _check_int("seed_count", seed_count, 1)
    _check_int("min_count", min_count, 1)
    _check_int("max_iter", max_iter, 1)
    _check_int("min_overlap", min_overlap, 1)
    check_erase_rounds(erase_rounds)
    a = float(pseudocount)
    if not a > 0 or math.isinf(a):
        raise ValueError(f"pseudocount {pseudocount} is not a finite number > 0: the seed's empty flanks and zero counts need one")
    if not float(p_value) >= 0:
        raise ValueError(f"p_value {p_value} is not a number >= 0")
    if not float(family_e_value) >= 0 or math.isinf(float(family_e_value)):
        raise ValueError(f"family_e_value {family_e_value} is not a finite number >= 0")
    seed_threshold("A" * k, seed_count, f, seed_mismatches, a)          # the match weight lies above the mismatch weight


def select_seeds(fg_seq, ctl_seq, k, dedupe, revcom, min_count, n_seeds, use_work=False):
    """[(kmer, fg_count, control_count, z)]: enrich_kmers' counting and exact selection at length k, the selected rows in rank order
    with z > 0, at most n_seeds; use_work: counted under the working masks of reads and control (what erase_sites left)"""
    from .enrichment import DeviceEnrich, count_both, select_enriched
    from .kmer_count import DeviceCounts, hash2kmer
    dc_f = dc_b = en = None
    try:
        dc_f, dc_b, en = DeviceCounts(), DeviceCounts(), DeviceEnrich()
        _, Nf, Nb = count_both(fg_seq, ctl_seq, dc_f, dc_b, k, dedupe, revcom, use_work=use_work)
        (_, kh, a, b, z), _ = select_enriched(ctl_seq, dc_f, dc_b, en, k, dedupe, revcom, Nf, Nb, min_count, n_seeds, use_work=use_work)
    finally:
        for h in (en, dc_f, dc_b):
            if h is not None:
                h.close()
    return [(hash2kmer(int(h), k), int(ai), int(bi), float(zi)) for h, ai, bi, zi in zip(kh, a, b, z) if zi > 0][:int(n_seeds)]


def _discover_pwms(res_dir, control_fasta_file, seed_len=8, n_seeds=64, seed_mismatches=1, seed_count=20, flank=2, min_count=2,
                   p_value=1e-4, pseudocount=1.0, revcom_mode=None, max_iter=20, min_overlap=5, family_e_value=0.01, output_dir=None,
                   erase_rounds=1):
    """`kmap discover_pwms`: config.toml + the encoded reads of a preproc result directory + a control FASTA -> discovered_rank.csv,
    discover_trace.csv, matrices/seed{i}_{consensus}.csv and discovered.meme (the representatives: a --library_file for the library
    verbs) in output_dir (default res_dir/pwm_discovery).  Every argument and file is checked before the device is touched or
    anything is written.  Under a torch.distributed launch rank 0 works alone.  Returns discover_core's results in seed order.
    erase_rounds above 1: discover_rounds -- after every round but the last the sites of the round's representatives are erased
    from reads and control (DeviceSeq.erase_sites) and the next round takes its seeds and its counts from what is left; the two
    tables get a `round` column and discover_erase.csv is written.  Every matrix is still evaluated on the original reads and the
    original control, so mw_z is comparable between rounds -- and optimistic in every round, as without erasure."""
    from .kmer_count import encode_fasta, load_array_pickle, load_config, rank0_only, result_paths
    if not rank0_only():
        return None
    check_arguments(seed_len, n_seeds, seed_mismatches, seed_count, flank, min_count, p_value, pseudocount, max_iter, min_overlap,
                    family_e_value, erase_rounds)
    erase_rounds = int(erase_rounds)
    res, cfg_path, seq_path, border_path = result_paths(res_dir, reads=True)
    if control_fasta_file is None or not Path(control_fasta_file).is_file():
        raise ValueError(f"control FASTA file {control_fasta_file} is missing")
    cfg, revcom = load_config(cfg_path, revcom_mode)
    dedupe = not bool(cfg["general"]["repetitive_mode"])

    from .motif_discovery import DeviceSeq
    from .motif_match import match_motifs
    fg_seq = DeviceSeq(load_array_pickle(seq_path), load_array_pickle(border_path))
    ctl_seq = None
    try:
        ctl_seq = DeviceSeq(*encode_fasta(str(control_fasta_file)))

        def seeds_fn(r):
            return select_seeds(fg_seq, ctl_seq, int(seed_len), dedupe, revcom, int(min_count), int(n_seeds), use_work=r > 1)

        def hist_fn(Ws, los, n_bins):
            per_set = []
            for ds in (fg_seq, ctl_seq):
                hists, outside, scored = ds.library_histograms(Ws, los, n_bins, revcom)
                if np.any(np.asarray(outside) != 0):
                    raise ValueError(f"discover_pwms: reads score outside the score range of seed {int(np.nonzero(outside)[0][0])}")
                per_set += [hists, [ds.n_seq - int(s) for s in scored]]
            return tuple(per_set)

        def erase_fn(Ws, ts):
            per_set = ()
            for ds in (fg_seq, ctl_seq):
                per_set += ds.erase_sites(Ws, ts, revcom, use_work=True)
            return per_set
        results, erase_log = discover_rounds(seeds_fn, lambda Ws, ts, use_work=False: fg_seq.library_counts(Ws, ts, revcom, use_work),
                                             erase_fn, hist_fn, match_motifs, revcom, erase_rounds, int(flank), int(seed_mismatches),
                                             int(seed_count), p_value, float(pseudocount), int(max_iter), int(min_overlap),
                                             float(family_e_value))
    finally:
        for h in (ctl_seq, fg_seq):
            if h is not None:
                h.close()

    out = res / OUTPUT_DIR if output_dir is None else Path(output_dir)
    reps = write_discovery(out, results, float(pseudocount), revcom, erase_log if erase_rounds > 1 else None)
    for e in erase_log:
        print(f"round {e['round']}: {len(e['rows'])} {'matrix' if len(e['rows']) == 1 else 'matrices'} erased, {e['fg_new']} positions of the "
              f"reads and {e['control_new']} of the control")
    for st in reps:
        print(f"{st['rank']} {st['name']} (seed {st['seed']}, family {st['family']} of {st['family_size']}): {st['status']} after "
              f"{st['iterations']} iteration{'s' if st['iterations'] != 1 else ''}, {st['n_selected']} sites ({st['n_minus']} on '-'), "
              f"{st['information_bits']:.3f} bits, auroc {st['auroc']:.4f}, mw_z {st['mw_z']:.6g}, q {st['q_bh']:.3g}")
    print(f"discover_pwms: {len(results)} {'seed' if len(results) == 1 else 'seeds'} of length {int(seed_len)}, {len(reps)} "
          f"{'family' if len(reps) == 1 else 'families'}, {'both strands' if revcom else 'forward strand'}: {out}")
    return results
