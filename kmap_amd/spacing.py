"""`kmap motif_spacing`: which motifs sit at a fixed distance and orientation from the bound factor's site?  (DESIGN.md section 19;
the reference has no such verb.)

Composite elements, half-site spacings and co-factor grammars show as a secondary motif whose best site lies a fixed number of
bases up- or downstream of the primary motif's site, on a fixed strand relative to it (the SpaMo question).  This module reads one
primary motif and a library as rank_motif_library does, has csrc/pwm_readscore.hip find the primary's best site of every read and
csrc/pwm_spacing.hip, in batched passes, the best site of every library matrix *that does not overlap it*, reduced on the device to
two small integer histograms per motif: S[quadrant][gap], the pair reads by side, relative strand and gap, and R[u][d], the same
reads by how many window positions within max_gap each side of the primary site offers.  Behind the kernel the statistic is host
arithmetic on those two: the expected count of every bin when the secondary site is uniform over the free positions and its strand
a fair coin, a Poisson upper tail per bin, the bin with the smallest p, Bonferroni over the bins tried, Benjamini-Hochberg over the
motifs.  Host code is parsing, that arithmetic and the file formats; the scoring has no CPU path."""
import math
from pathlib import Path

import numpy as np

from .library import _field, _file_name, bh_qvalues, load_library, open_read_sets, rank_order, read_motif_library, write_skipped
from .pwm import SCORE_UNIT, min_score_threshold, pwm_consensus, pwm_threshold, pwm_weights

OUTPUT_DIR, RANK_FILE, SKIPPED_FILE, HIST_FILE = "motif_spacing", "spacing_rank.csv", "skipped.csv", "spacing_{rank}_{name}.csv"
RANK_HEADER = ("rank,name,altname,source,width,consensus,threshold,threshold_bits,n_primary,n_pairs,n_in_range,n_far,best_side,"
               "best_strand,best_gap,pairs_in_bin,expected_in_bin,log10_p,n_bins,log10_p_adj,q_bh")
HIST_HEADER = "side,strand,gap,pairs,expected"
SIDES, STRANDS = ("upstream", "downstream"), ("same", "opposite")      # quadrant = 2 downstream + opposite
MAX_GAP = 511                                                # device_seq.SPACING_MAX_GAP


def log10_poisson_sf(k, mu):
    """log10 P(X >= k) for X Poisson with mean mu, k an integer >= 0.  Above the mean a log-sum-exp of the terms j ln mu - mu -
    lgamma(j + 1) over j >= k, which fall from the first one on, until they no longer change a double; at or below the mean (the tail
    is then at least about a half) log1p of minus the lower tail, summed the same way, so that neither form cancels.  k = 0 gives 0,
    mu = 0 with k > 0 gives -inf; a tail far below the smallest double stays finite."""
    if isinstance(k, bool) or int(k) != k or k < 0 or not mu >= 0 or math.isinf(mu):
        raise ValueError(f"log10_poisson_sf: k={k}, mu={mu}")
    k, mu = int(k), float(mu)
    if k == 0:
        return 0.0
    if mu == 0.0:
        return -math.inf
    ln_mu = math.log(mu)

    def term(j):
        return j * ln_mu - mu - math.lgamma(j + 1.0)
    if k > mu:
        first, total, j = term(k), 1.0, k + 1
        while True:
            x = math.exp(term(j) - first)                    # below 1 and falling: mu / j < 1
            total += x
            if x < 1e-17 * total:
                break
            j += 1
        return (first + math.log(total)) / math.log(10.0)
    lower = math.fsum(math.exp(term(j)) for j in range(k))   # P(X < k): at most about a half at or below the mean
    return math.log1p(-lower) / math.log(10.0)


def rooms(L, p, wP, w, max_gap, minus):
    """(u, d): how many windows of width w a read of length L offers upstream and downstream of a primary window of width wP at loc
    p on strand `minus`, no further than max_gap bases from it -- the left room min(max(p - w + 1, 0), max_gap + 1) and the right
    room min(max(L - p - wP - w + 1, 0), max_gap + 1), the left one upstream of a '+' primary.  What csrc/pwm_spacing.hip counts
    in R."""
    if p < 0 or p + wP > L or w < 1 or max_gap < 0:
        raise ValueError(f"rooms: L={L} p={p} wP={wP} w={w} max_gap={max_gap}")
    left, right = min(max(p - w + 1, 0), max_gap + 1), min(max(L - p - wP - w + 1, 0), max_gap + 1)
    return (right, left) if minus else (left, right)


def _hists(S, R):
    S, R = np.asarray(S), np.asarray(R)
    if S.ndim != 2 or S.shape[0] != 4 or R.ndim != 2 or R.shape != (S.shape[1] + 1, S.shape[1] + 1) or S.dtype.kind not in "iu" \
            or R.dtype.kind not in "iu":
        raise ValueError("a gap histogram [4, G + 1] and a room histogram [G + 2, G + 2] of integer counts are expected")
    if (S.dtype.kind == "i" and (S < 0).any()) or (R.dtype.kind == "i" and (R < 0).any()):
        raise ValueError("a histogram count is negative")
    if R[0, 0]:
        raise ValueError("a pair read in range without room on either side")
    return S.astype(np.int64), R.astype(np.int64)


def expected_bins(R, revcom):
    """E float64[4, G + 1] from the room histogram R[u][d]: a read with rooms (u, d) puts 1 / (s (u + d)) on every bin (upstream,
    g < u) and (downstream, g < d) of each of its s strands -- s = 2 with revcom, else 1 and the `opposite` quadrants 1 and 3 stay
    0.  The sum of E is the sum of R."""
    R = np.asarray(R)
    G = R.shape[0] - 2
    s = 2 if revcom else 1
    rooms = np.arange(G + 2, dtype=np.float64)
    total = rooms[:, None] + rooms[None, :]
    total[0, 0] = 1.0                                        # R[0][0] is 0
    share = R.astype(np.float64) / (s * total)
    by_u, by_d = share.sum(axis=1), share.sum(axis=0)
    # bin g takes the reads with a room above g: suffix sums over the rooms g + 1 .. G + 1
    up, down = np.cumsum(by_u[::-1])[::-1][1:], np.cumsum(by_d[::-1])[::-1][1:]
    E = np.zeros((4, G + 1), np.float64)
    for opposite in range(s):
        E[opposite], E[2 + opposite] = up, down
    return E


def best_bin(S, R, revcom, min_pairs=10):
    """The bin (quadrant, gap) with the smallest Poisson upper tail P(X >= S[bin]) at mean E[bin], among the bins with E > 0; on a
    tie the smaller quadrant, then the smaller gap.  A dict with n_in_range (the sum of S), n_bins (the candidates), quadrant and gap
    (None without a candidate or with fewer than min_pairs pair reads in range), pairs_in_bin, expected_in_bin, log10_p and
    log10_p_adj = min(0, log10_p + log10 n_bins), Bonferroni over the bins tried, and E."""
    if int(min_pairs) != min_pairs or min_pairs < 1:
        raise ValueError(f"min_pairs {min_pairs} < 1")
    S, R = _hists(S, R)
    if int(S.sum()) != int(R.sum()):
        raise ValueError("the gap histogram and the room histogram count different reads")
    E = expected_bins(R, revcom)
    if (S[E <= 0] != 0).any():
        raise ValueError("a pair read in a bin that no read has room for")
    n, n_bins = int(S.sum()), int((E > 0).sum())
    out = dict(n_in_range=n, n_bins=n_bins, quadrant=None, gap=None, pairs_in_bin=None, expected_in_bin=math.nan, log10_p=0.0,
               log10_p_adj=0.0, E=E)
    if n_bins == 0 or n < min_pairs:
        return out
    best = None
    for q, g in zip(*np.nonzero(E > 0)):                     # by quadrant, then gap: the first of equal minima stays
        lp = log10_poisson_sf(int(S[q, g]), float(E[q, g])) if S[q, g] else 0.0
        if best is None or lp < best[0]:
            best = (lp, int(q), int(g))
    lp, q, g = best
    out.update(quadrant=q, gap=g, pairs_in_bin=int(S[q, g]), expected_in_bin=float(E[q, g]), log10_p=lp,
               log10_p_adj=min(0.0, lp + math.log10(n_bins)))
    return out


def rank_line(rank, motif, t, st):
    """one line of spacing_rank.csv: integers as integers, bits as %.2f, other floats repr; the five fields that describe the bin are
    empty when there is none"""
    q = st["quadrant"]
    where = f"{SIDES[q >> 1]},{STRANDS[q & 1]},{st['gap']},{st['pairs_in_bin']},{float(st['expected_in_bin'])!r}" if q is not None else ",,,,"
    return (f"{int(rank)},{motif.name},{motif.altname},{motif.source},{motif.counts.shape[1]},{pwm_consensus(motif.counts)},{int(t)},"
            f"{int(t) / SCORE_UNIT:.2f},{st['n_primary']},{st['n_pairs']},{st['n_in_range']},{st['n_far']},{where},"
            f"{float(st['log10_p'])!r},{st['n_bins']},{float(st['log10_p_adj'])!r},{float(st['q_bh'])!r}\n")


def write_gap_histogram(path, S, E):
    """spacing_{rank}_{name}.csv: the bins some pair read lies in, by quadrant, then gap"""
    with open(path, "w") as fh:
        fh.write(HIST_HEADER + "\n")
        for q, g in zip(*np.nonzero(S)):
            fh.write(f"{SIDES[q >> 1]},{STRANDS[q & 1]},{int(g)},{int(S[q, g])},{float(E[q, g])!r}\n")


def _one_primary(primary_file, primary_name, nsites_default):
    motifs = [m for m in read_motif_library(primary_file, nsites_default) if m.skip is None]
    if primary_name is not None:
        motifs = [m for m in motifs if m.name == _field(primary_name)]
    if len(motifs) != 1:
        raise ValueError(f"motif_spacing: {primary_file} holds {len(motifs)} motifs that can be scored"
                         + (f" and are named {primary_name}" if primary_name is not None else "")
                         + ": exactly one primary motif is expected (--primary_name selects one)")
    return motifs[0]


# ---- the verb -----------------------------------------------------------------------------------------------------------------
def _motif_spacing(res_dir, primary_file, library_files, primary_name=None, p_value=1e-4, primary_min_score=None, min_score=None,
                   pseudocount=1.0, nsites_default=20, revcom_mode=None, max_gap=150, min_pairs=10, top_hist=5, output_dir=None):
    """`kmap motif_spacing`: config.toml + the encoded reads of a preproc result directory + a primary motif + library files ->
    spacing_rank.csv, skipped.csv and spacing_{rank}_{name}.csv for the top_hist best in output_dir (default
    res_dir/motif_spacing).  Every file is parsed, every threshold found and every ValueError raised before the device is touched
    or a file is written; motifs whose width lies outside 4..31 are listed in skipped.csv.  Under a torch.distributed launch rank
    0 works alone.  Returns one dict per motif in rank order: best_bin's fields plus motif, rank, threshold, S, R, n_primary,
    n_pairs, n_far and q_bh."""
    from .kmer_count import load_config, rank0_only, result_paths
    if not rank0_only():
        return None
    res, cfg_path, seq_path, border_path = result_paths(res_dir, reads=True)
    library_files = [str(f) for f in library_files]
    if not library_files:
        raise ValueError("motif_spacing: no library file given")
    if isinstance(max_gap, bool) or int(max_gap) != max_gap or not 0 <= max_gap <= MAX_GAP:
        raise ValueError(f"max_gap {max_gap} outside 0 .. {MAX_GAP}")
    if int(min_pairs) != min_pairs or min_pairs < 1:
        raise ValueError(f"min_pairs {min_pairs} < 1")
    if int(top_hist) != top_hist or top_hist < 0:
        raise ValueError(f"top_hist {top_hist} < 0")
    if int(nsites_default) != nsites_default or nsites_default < 1:          # read_meme's check, also when every file is a CSV
        raise ValueError(f"nsites_default {nsites_default} < 1")
    t_fixed = None if min_score is None else min_score_threshold(min_score)
    tP_fixed = None if primary_min_score is None else min_score_threshold(primary_min_score)
    _, revcom = load_config(cfg_path, revcom_mode)

    primary = _one_primary(str(primary_file), primary_name, nsites_default)
    try:
        W_P = pwm_weights(primary.counts, pseudocount)
        tP = pwm_threshold(W_P, p_value)[0] if tP_fixed is None else tP_fixed
    except ValueError as exc:
        raise ValueError(f"{primary.source}: motif {primary.name}: {exc}") from None
    motifs, skipped, Ws, plans = load_library("motif_spacing", library_files, nsites_default, pseudocount, p_value, t_fixed)
    ts = [p[0] for p in plans]

    with open_read_sets(seq_path, border_path) as (seq, _):
        scores = seq.read_scores(W_P, revcom)
        try:
            S, R, n_primary, n_pair, n_far = seq.library_spacing(scores, W_P.shape[1], tP, Ws, ts, revcom, int(max_gap))
        finally:
            scores.close()

    results = []
    for i, (m, t) in enumerate(zip(motifs, ts)):
        st = best_bin(S[i], R[i], revcom, min_pairs)
        if st["n_in_range"] != int(n_pair[i]) - int(n_far[i]):
            raise ValueError(f"motif_spacing: the histograms of motif {m.name} hold {st['n_in_range']} reads, "
                             f"{int(n_pair[i]) - int(n_far[i])} pair reads are in range")
        st.update(motif=m, threshold=t, S=S[i], R=R[i], n_primary=int(n_primary), n_pairs=int(n_pair[i]), n_far=int(n_far[i]))
        results.append(st)
    for st, q in zip(results, bh_qvalues([10.0 ** st["log10_p_adj"] for st in results]).tolist()):
        st["q_bh"] = q
    results = [results[i] for i in rank_order([st["motif"].name for st in results],
                                              [math.nan if st["quadrant"] is None else -st["log10_p_adj"] for st in results])]

    out = res / OUTPUT_DIR if output_dir is None else Path(output_dir)
    out.mkdir(parents=True, exist_ok=True)
    with open(out / RANK_FILE, "w") as fh:
        fh.write(RANK_HEADER + "\n")
        for rank, st in enumerate(results):
            st["rank"] = rank
            fh.write(rank_line(rank, st["motif"], st["threshold"], st))
    write_skipped(out, skipped)
    for st in results[:int(top_hist)]:
        write_gap_histogram(out / HIST_FILE.format(rank=st["rank"], name=_file_name(st["motif"].name)), st["S"], st["E"])
    print(f"primary {primary.name}{' ' + primary.altname if primary.altname else ''}: at {tP / SCORE_UNIT:.2f} bits "
          f"{int(n_primary)} primary reads")
    for st in results[:10]:
        m, q = st["motif"], st["quadrant"]
        where = (f"no bin to test among {st['n_in_range']} pair reads within {int(max_gap)} bases" if q is None else
                 f"{st['pairs_in_bin']} of {st['n_in_range']} pair reads {st['gap']} bases {SIDES[q >> 1]} on the {STRANDS[q & 1]} strand, "
                 f"{st['expected_in_bin']:.1f} expected, log10 p adj {st['log10_p_adj']:.2f}, q {st['q_bh']:.3g}")
        print(f"{st['rank']} {m.name}{' ' + m.altname if m.altname else ''}: at {st['threshold'] / SCORE_UNIT:.2f} bits {where}")
    print(f"motif_spacing: {len(results)} {'motif' if len(results) == 1 else 'motifs'} ranked, {len(skipped)} skipped, "
          f"{'both strands' if revcom else 'forward strand'}: {out}")
    return results
