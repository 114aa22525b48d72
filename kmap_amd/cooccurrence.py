"""`kmap motif_cooccurrence`: which motifs of a library share reads?  (the reference's check_motif_co_occurence
compares two consensus strings, not a library.)

Co-binding partners share reads more often than their own frequencies predict, alternative factors less often.  This module reads
a library as motif_centrality does, has csrc/pwm_presence.hip score every read under every matrix in batched passes and keep one
bit per (motif, read) -- present: the read's best window reaches the motif's threshold -- and has csrc/bit_pairs.hip count the
reads every pair of motifs shares, C[i][j] = popcount(row i AND row j), for all pairs at once.  Behind the two kernels the
statistic is host arithmetic on that one integer matrix: given the margins n_i = C[i][i] and n_j, the shared count n_ij is
hypergeometric under independence; a normal-approximation z from its exact mean and variance, a two-sided p, Benjamini-Hochberg
over the pairs that were tested, and for the written rows the exact hypergeometric tail.  With a control read set the same counts
are taken there and the shared count is compared between the two sets.  Host code is parsing, that arithmetic and the file formats;
neither kernel has a CPU path.

Two motifs that match the same window -- a motif and its longer variant, two members of one family -- are "together" by
construction: the same sites make both present.  match_motifs' families tell which pairs those are; nothing is filtered here."""
import math
from pathlib import Path

import numpy as np

from .enrichment import enrich_z
from .library import bh_qvalues, load_library, open_read_sets, write_skipped
from .pwm import SCORE_UNIT, min_score_threshold, pwm_consensus

OUTPUT_DIR, PAIRS_FILE, PRESENCE_FILE, SKIPPED_FILE, MATRIX_FILE = ("motif_cooccurrence", "cooccurrence_pairs.csv", "motif_presence.csv",
                                                                    "skipped.csv", "pair_counts.tsv")
PAIRS_HEADER = ("rank,name_i,altname_i,width_i,name_j,altname_j,width_j,n_i,n_j,n_both,expected,z,direction,log10_p,log10_p_exact,"
                "n_tests,q_bh")
PAIRS_CONTROL_HEADER = ",control_i,control_j,control_both,z_vs_control"
PRESENCE_HEADER = "name,altname,source,width,consensus,threshold,threshold_bits,n_present,share"
PRESENCE_CONTROL_HEADER = ",control_present,control_share"
MAX_MOTIFS = 4096                                            # device_seq.BIT_PAIRS_MAX_ROWS
_TAIL_DECADES = 40.0


def _counts(C):
    C = np.asarray(C)
    if C.ndim != 2 or C.shape[0] != C.shape[1] or C.dtype.kind not in "iu":
        raise ValueError("a square matrix of integer pair counts is expected")
    C = C.astype(np.int64)
    if (C < 0).any() or not np.array_equal(C, C.T):
        raise ValueError("the pair counts are negative or not symmetric")
    return C


def pair_stats(C, N, min_expected=5.0):
    """The statistic of every pair i < j (row-major over the upper triangle) of the pair counts C [n_mat, n_mat] of N reads: a dict
    of arrays i, j, n_i, n_j, n_both (int64), expected E = n_i n_j / N and variance V = E (1 - n_i / N) (N - n_j) / (N - 1) of the
    hypergeometric n_both given the margins, tested (E, n_i - E and n_j - E all >= min_expected, so that both tails have room, and
    V > 0), z = (n_both - E) / sqrt(V), log10_p = the two-sided normal tail (log10 of the upper tail of |z| + log10 2, at most 0),
    q_bh = Benjamini-Hochberg over the tested pairs; z, log10_p and q_bh are nan where the pair is not tested.  n_tests = the
    number of tested pairs.  float64, in this order."""
    from scipy.special import log_ndtr
    C, N = _counts(C), int(N)
    if not min_expected >= 0:
        raise ValueError(f"min_expected {min_expected} < 0")
    n = np.diagonal(C)
    if N < 0 or (len(n) and (int(n.max()) > N or (C > np.minimum.outer(n, n)).any())):
        raise ValueError(f"pair counts above their margins, or margins above the {N} reads")
    i, j = np.triu_indices(len(n), 1)
    n_i, n_j, n_both = n[i], n[j], C[i, j]
    with np.errstate(divide="ignore", invalid="ignore"):
        fi, fj, fN = n_i.astype(np.float64), n_j.astype(np.float64), float(N)
        E = fi * fj / fN
        V = E * (1.0 - fi / fN) * (fN - fj) / (fN - 1.0)
        tested = (E >= min_expected) & (fi - E >= min_expected) & (fj - E >= min_expected) & (V > 0.0)
        z = np.where(tested, (n_both - E) / np.sqrt(V), np.nan)
    log10_p = np.full(len(z), np.nan)
    log10_p[tested] = np.minimum(log_ndtr(-np.abs(z[tested])) / math.log(10.0) + math.log10(2.0), 0.0)
    q = np.full(len(z), np.nan)
    q[tested] = bh_qvalues(10.0 ** log10_p[tested])
    return dict(i=i.astype(np.int64), j=j.astype(np.int64), n_i=n_i, n_j=n_j, n_both=n_both, expected=E, variance=V, tested=tested, z=z,
                log10_p=log10_p, q_bh=q, n_tests=int(tested.sum()))


def _log_comb(n, k):
    return math.lgamma(n + 1) - math.lgamma(k + 1) - math.lgamma(n - k + 1)


def log10_p_exact(n_both, n_i, n_j, N, upper):
    """log10 of twice the hypergeometric tail of n_both given the margins, at most 0: P(X >= n_both) when `upper`, else
    P(X <= n_both), X = the reads two sets of n_i and n_j among N share.  Summed in log space with math.lgamma from the observed
    count outwards until a term lies 40 decades under the largest."""
    n_both, n_i, n_j, N = int(n_both), int(n_i), int(n_j), int(N)
    lo, hi = max(0, n_i + n_j - N), min(n_i, n_j)
    if not (0 <= n_i <= N and 0 <= n_j <= N and lo <= n_both <= hi):
        raise ValueError(f"log10_p_exact: n_both={n_both} n_i={n_i} n_j={n_j} N={N}")
    base = _log_comb(N, n_j)
    terms, largest = [], -math.inf
    k, step = n_both, 1 if upper else -1
    while lo <= k <= hi:
        t = _log_comb(n_i, k) + _log_comb(N - n_i, n_j - k) - base
        if t < largest - _TAIL_DECADES * math.log(10.0):
            break
        terms.append(t)
        largest = max(largest, t)
        k += step
    total = largest + math.log(math.fsum(math.exp(t - largest) for t in terms))
    return min(0.0, total / math.log(10.0) + math.log10(2.0))


def select_rows(st, names, top_n):
    """the indices into pair_stats' arrays of the rows to write: the tested pairs by |z| descending, ties by the two names, the
    first top_n of them; top_n 0: all of them, then the pairs that were not tested, by the two names"""
    uniq = {name: r for r, name in enumerate(sorted(set(names)))}
    rank_of = np.array([uniq[name] for name in names], np.int64)
    ri, rj = rank_of[st["i"]], rank_of[st["j"]]
    tested = np.nonzero(st["tested"])[0]
    order = tested[np.lexsort((rj[tested], ri[tested], -np.abs(st["z"][tested])))]
    if top_n:
        return order[:int(top_n)]
    rest = np.nonzero(~st["tested"])[0]
    return np.concatenate([order, rest[np.lexsort((rj[rest], ri[rest]))]])


def direction_of(z):
    return "together" if z > 0 else "apart" if z < 0 else "none"


def pair_line(rank, mi, mj, row, control):
    """one line of cooccurrence_pairs.csv: integers as integers, floats repr; z, direction, both p and q are empty for a pair that
    was not tested"""
    line = (f"{int(rank)},{mi.name},{mi.altname},{mi.counts.shape[1]},{mj.name},{mj.altname},{mj.counts.shape[1]},{row['n_i']},"
            f"{row['n_j']},{row['n_both']},{float(row['expected'])!r},")
    if row["tested"]:
        line += (f"{float(row['z'])!r},{row['direction']},{float(row['log10_p'])!r},{float(row['log10_p_exact'])!r},{row['n_tests']},"
                 f"{float(row['q_bh'])!r}")
    else:
        line += f",,,,{row['n_tests']},"
    if control:
        line += f",{row['control_i']},{row['control_j']},{row['control_both']},{float(row['z_vs_control'])!r}"
    return line + "\n"


def pair_rows(C, N, names, min_expected=5.0, top_n=1000, C_control=None, N_control=None):
    """(rows, stats): pair_stats of C and the rows select_rows picks, each a dict with i, j, n_i, n_j, n_both, expected, tested,
    z, direction, log10_p, log10_p_exact (the exact tail on the side of z), n_tests, q_bh and, with the control's pair counts,
    control_i, control_j, control_both and z_vs_control = enrich_z(n_both, control_both, N, N_control)"""
    st = pair_stats(C, N, min_expected)
    Cc = None if C_control is None else _counts(C_control)
    if Cc is not None and Cc.shape != np.asarray(C).shape:
        raise ValueError("the control's pair counts have another shape")
    rows = []
    for p in select_rows(st, names, top_n).tolist():
        i, j, tested = int(st["i"][p]), int(st["j"][p]), bool(st["tested"][p])
        row = dict(i=i, j=j, n_i=int(st["n_i"][p]), n_j=int(st["n_j"][p]), n_both=int(st["n_both"][p]), expected=float(st["expected"][p]),
                   tested=tested, z=float(st["z"][p]), log10_p=float(st["log10_p"][p]), q_bh=float(st["q_bh"][p]), n_tests=st["n_tests"],
                   direction="", log10_p_exact=math.nan)
        if tested:
            row["direction"] = direction_of(row["z"])
            row["log10_p_exact"] = (0.0 if row["z"] == 0 else
                                    log10_p_exact(row["n_both"], row["n_i"], row["n_j"], N, row["z"] > 0))
        if Cc is not None:
            row.update(control_i=int(Cc[i, i]), control_j=int(Cc[j, j]), control_both=int(Cc[i, j]),
                       z_vs_control=enrich_z(row["n_both"], int(Cc[i, j]), N, N_control))
        rows.append(row)
    return rows, st


def write_tables(out, motifs, ts, rows, C, N, C_control=None, N_control=None, write_matrix=False):
    """cooccurrence_pairs.csv, motif_presence.csv and, with write_matrix, pair_counts.tsv in the directory `out`"""
    control = C_control is not None
    with open(out / PAIRS_FILE, "w") as fh:
        fh.write(PAIRS_HEADER + (PAIRS_CONTROL_HEADER if control else "") + "\n")
        for rank, row in enumerate(rows):
            fh.write(pair_line(rank, motifs[row["i"]], motifs[row["j"]], row, control))
    with open(out / PRESENCE_FILE, "w") as fh:
        fh.write(PRESENCE_HEADER + (PRESENCE_CONTROL_HEADER if control else "") + "\n")
        for i, (m, t) in enumerate(zip(motifs, ts)):
            n = int(C[i][i])
            line = (f"{m.name},{m.altname},{m.source},{m.counts.shape[1]},{pwm_consensus(m.counts)},{int(t)},{int(t) / SCORE_UNIT:.2f},{n},"
                    f"{(n / N if N else math.nan)!r}")
            if control:
                nc = int(C_control[i][i])
                line += f",{nc},{(nc / N_control if N_control else math.nan)!r}"
            fh.write(line + "\n")
    if write_matrix:
        with open(out / MATRIX_FILE, "w") as fh:
            fh.write("\t" + "\t".join(m.name for m in motifs) + "\n")
            for m, counts in zip(motifs, np.asarray(C).tolist()):
                fh.write(m.name + "\t" + "\t".join(str(int(c)) for c in counts) + "\n")


# ---- the verb -----------------------------------------------------------------------------------------------------------------
def _motif_cooccurrence(res_dir, library_files, control_fasta_file=None, p_value=1e-4, min_score=None, pseudocount=1.0,
                        nsites_default=20, revcom_mode=None, min_expected=5.0, top_n=1000, write_matrix=False, output_dir=None):
    """`kmap motif_cooccurrence`: config.toml + the encoded reads of a preproc result directory + library files (+ a control FASTA)
    -> cooccurrence_pairs.csv, motif_presence.csv, skipped.csv and, with write_matrix, pair_counts.tsv in output_dir (default
    res_dir/motif_cooccurrence).  Every file is parsed, every threshold found and every ValueError raised before the device is
    touched or a file is written; motifs whose width lies outside 4..31 are listed in skipped.csv.  Under a torch.distributed launch
    rank 0 works alone.  Returns a dict: motifs, thresholds, n_reads, pair_counts, rows (pair_rows', in rank order), n_tests and,
    with a control, control_reads and control_pair_counts."""
    from .kmer_count import load_config, rank0_only, result_paths
    if not rank0_only():
        return None
    res, cfg_path, seq_path, border_path = result_paths(res_dir, reads=True)
    if control_fasta_file is not None and not Path(control_fasta_file).is_file():
        raise ValueError(f"control FASTA file {control_fasta_file} is missing")
    library_files = [str(f) for f in library_files]
    if not library_files:
        raise ValueError("motif_cooccurrence: no library file given")
    if not min_expected >= 0:
        raise ValueError(f"min_expected {min_expected} < 0")
    if int(top_n) != top_n or top_n < 0:
        raise ValueError(f"top_n {top_n} < 0")
    t_fixed = None if min_score is None else min_score_threshold(min_score)
    _, revcom = load_config(cfg_path, revcom_mode)

    motifs, skipped, Ws, plans = load_library("motif_cooccurrence", library_files, nsites_default, pseudocount, p_value, t_fixed)
    ts = [p[0] for p in plans]
    if len(motifs) > MAX_MOTIFS:
        raise ValueError(f"motif_cooccurrence: {len(motifs)} motifs, more than {MAX_MOTIFS}")

    per_set = []
    with open_read_sets(seq_path, border_path, control_fasta_file) as read_sets:
        for ds in read_sets:
            if ds is not None:
                planes = ds.library_presence(Ws, ts, revcom)
                try:
                    C = planes.pair_counts()
                    if not np.array_equal(np.diagonal(C), planes.n_present):
                        raise RuntimeError("motif_cooccurrence: the diagonal of the pair counts is not the number of present reads")
                finally:
                    planes.close()
                per_set.append((C, int(ds.n_seq)))

    control = len(per_set) == 2
    (C, N), (Cc, Nc) = per_set[0], per_set[1] if control else (None, None)
    rows, st = pair_rows(C, N, [m.name for m in motifs], min_expected, top_n, Cc, Nc)
    out = res / OUTPUT_DIR if output_dir is None else Path(output_dir)
    out.mkdir(parents=True, exist_ok=True)
    write_tables(out, motifs, ts, rows, C, N, Cc, Nc, write_matrix)
    write_skipped(out, skipped)
    for rank, row in enumerate(rows[:10]):
        mi, mj = motifs[row["i"]], motifs[row["j"]]
        what = (f"z {row['z']:.6g} ({row['direction']}), log10 p {row['log10_p']:.2f}, exact {row['log10_p_exact']:.2f}, q {row['q_bh']:.3g}"
                if row["tested"] else "not tested")
        print(f"{rank} {mi.name} + {mj.name}: {row['n_both']} reads hold both ({row['n_i']} and {row['n_j']} of {N}), "
              f"{row['expected']:.1f} expected, {what}"
              + (f"; z against the control {row['z_vs_control']:.6g}" if control else ""))
    n_pairs = len(motifs) * (len(motifs) - 1) // 2
    print(f"motif_cooccurrence: {len(motifs)} {'motif' if len(motifs) == 1 else 'motifs'}, {st['n_tests']} of {n_pairs} pairs tested, "
          f"{len(skipped)} skipped, {'both strands' if revcom else 'forward strand'}: {out}")
    result = dict(motifs=motifs, thresholds=ts, n_reads=N, pair_counts=C, rows=rows, n_tests=st["n_tests"])
    if control:
        result.update(control_reads=Nc, control_pair_counts=Cc)
    return result
