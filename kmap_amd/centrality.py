"""`kmap motif_centrality`: is the best site of a motif where the peak is?  (the reference has no such verb.)

For peak-centred reads the strongest evidence that a motif is the bound factor is that its best site sits at the reads' centre.
This module reads a library as rank_motif_library does, has csrc/pwm_sites.hip find the best window of every read under every
matrix in batched passes and reduce the site reads -- best score at or above the matrix's threshold -- on the device to two small
histograms per motif: the doubled centre offsets d = 2 loc + w - L and the read lengths L.  Behind the kernel the statistic is
host arithmetic on those two histograms: for every half-width a the number of sites with |d| <= a against the exact mean and
variance of that number when the site is uniform over each read's L - w + 1 windows (a Poisson-binomial over the lengths), a
normal-approximation z, the half-width with the largest z, Bonferroni over the half-widths tried, Benjamini-Hochberg over the
motifs.  No control is needed; with one, the share of sites inside the best region is compared between the two read sets.  Host
code is parsing, that arithmetic and the file formats; the scoring has no CPU path."""
import math
from pathlib import Path

import numpy as np

from .enrichment import enrich_z
from .library import _file_name, bh_qvalues, load_library, log10_p_of_z, open_read_sets, rank_order, write_skipped
from .pwm import SCORE_UNIT, min_score_threshold, pwm_consensus

OUTPUT_DIR, RANK_FILE, SKIPPED_FILE, OFFSETS_FILE = "motif_centrality", "centrality_rank.csv", "skipped.csv", "site_offsets_{rank}_{name}.csv"
RANK_HEADER = ("rank,name,altname,source,width,consensus,threshold,threshold_bits,n_sites,half_width_x2,half_width_bases,"
               "sites_in_region,expected_in_region,z,log10_p,n_regions,log10_p_adj,q_bh")
CONTROL_HEADER = ",control_sites,control_in_region,z_vs_control"


def windows_within(L, w, a):
    """c(L, w, a): how many of the L - w + 1 windows of a read of length L have a doubled centre offset |d| <= a.  The offsets are
    -m, -m + 2, .. m with m = L - w: with a' = min(a, m), a' + 1 of them when a' has m's parity, else a'."""
    m = int(L) - int(w)
    if m < 0 or a < 0:
        raise ValueError(f"windows_within: L={L} w={w} a={a}")
    a = min(int(a), m)
    return a + 1 if (a - m) % 2 == 0 else a


def _hists(D, Hlen):
    D, Hlen = np.asarray(D), np.asarray(Hlen)
    if D.ndim != 1 or Hlen.ndim != 1 or len(D) % 2 != 1 or D.dtype.kind not in "iu" or Hlen.dtype.kind not in "iu":
        raise ValueError("an offset histogram of 2 max_len + 1 and a length histogram of integer counts are expected")
    if (D.dtype.kind == "i" and (D < 0).any()) or (Hlen.dtype.kind == "i" and (Hlen < 0).any()):
        raise ValueError("a histogram count is negative")
    return D.astype(np.int64), Hlen.astype(np.int64)


def sites_within(D, a):
    """k(a): the site reads with |d| <= a of an offset histogram (bin d + (len(D) - 1) / 2)"""
    D = np.asarray(D)
    c = (len(D) - 1) // 2
    a = min(int(a), c)
    return int(D[c - a:c + a + 1].sum()) if a >= 0 else 0


def region_curve(D, Hlen, w):
    """(k, E, V) as arrays over the half-widths a = 0 .. A, A = the largest L - w of an occupied length (beyond it nothing
    changes): k(a) = sum_{|d| <= a} D[d] (int64), E(a) = sum_L Hlen[L] q_L(a), V(a) = sum_L Hlen[L] q_L(a) (1 - q_L(a)) with
    q_L(a) = c(L, w, a) / (L - w + 1), in float64, the lengths ascending.  Empty arrays when there is no site."""
    D, Hlen = _hists(D, Hlen)
    lengths = np.nonzero(Hlen)[0]
    if len(lengths) == 0:
        return np.zeros(0, np.int64), np.zeros(0), np.zeros(0)
    if lengths[0] < w:
        raise ValueError(f"a site read of length {int(lengths[0])} under a matrix of width {w}")
    A = int(lengths[-1]) - int(w)
    centre = (len(D) - 1) // 2
    if A > centre or D[:centre - A].any() or D[centre + A + 1:].any():
        raise ValueError("an offset lies outside the longest site read")
    k = np.cumsum(np.concatenate([[D[centre]], D[centre + 1:centre + A + 1] + D[centre - A:centre][::-1]]))
    a = np.arange(A + 1, dtype=np.int64)
    E, V = np.zeros(A + 1), np.zeros(A + 1)
    for L in lengths.tolist():
        m = L - int(w)
        ac = np.minimum(a, m)
        q = np.where((ac - m) % 2 == 0, ac + 1, ac) / float(m + 1)
        E += float(Hlen[L]) * q
        V += float(Hlen[L]) * (q * (1.0 - q))
    return k.astype(np.int64), E, V


def best_region(D, Hlen, w, min_half=0, min_sites=10):
    """The half-width with the largest z(a) = (k(a) - E(a)) / sqrt(V(a)) among the integers a >= min_half with V(a) > 0, on a tie
    the smallest: a dict with n_sites, n_regions (the candidates), half_width_x2 = a* (None without a candidate or with fewer
    than min_sites sites), sites_in_region, expected_in_region, variance, z, log10_p (the upper normal tail) and log10_p_adj =
    min(0, log10_p + log10 n_regions), Bonferroni over the half-widths tried."""
    if int(min_half) != min_half or min_half < 0:
        raise ValueError(f"min_half {min_half} < 0")
    if int(min_sites) != min_sites or min_sites < 1:
        raise ValueError(f"min_sites {min_sites} < 1")
    k, E, V = region_curve(D, Hlen, w)
    n = int(np.asarray(Hlen).sum())
    cand = np.nonzero(V > 0)[0]
    cand = cand[cand >= min_half]
    out = dict(n_sites=n, n_regions=len(cand), half_width_x2=None, sites_in_region=None, expected_in_region=math.nan,
               variance=math.nan, z=math.nan, log10_p=0.0, log10_p_adj=0.0)
    if len(cand) == 0 or n < min_sites:
        return out
    z = (k[cand] - E[cand]) / np.sqrt(V[cand])
    i = int(np.argmax(z))                                    # the first of equal maxima: the smallest a
    a = int(cand[i])
    log10_p = log10_p_of_z(float(z[i]))
    out.update(half_width_x2=a, sites_in_region=int(k[a]), expected_in_region=float(E[a]), variance=float(V[a]), z=float(z[i]),
               log10_p=log10_p, log10_p_adj=min(0.0, log10_p + math.log10(len(cand))))
    return out


def rank_line(rank, motif, t, st, control):
    """one line of centrality_rank.csv: integers as integers, bits as %.2f, half_width_bases as %.1f, other floats repr; the
    region's fields are empty when there is none"""
    a = st["half_width_x2"]
    region = f"{a},{a / 2:.1f},{st['sites_in_region']},{float(st['expected_in_region'])!r}" if a is not None else ",,,"
    line = (f"{int(rank)},{motif.name},{motif.altname},{motif.source},{motif.counts.shape[1]},{pwm_consensus(motif.counts)},{int(t)},"
            f"{int(t) / SCORE_UNIT:.2f},{st['n_sites']},{region},{float(st['z'])!r},{float(st['log10_p'])!r},{st['n_regions']},"
            f"{float(st['log10_p_adj'])!r},{float(st['q_bh'])!r}")
    if control:
        inside = "" if st["control_in_region"] is None else st["control_in_region"]
        line += f",{st['control_sites']},{inside},{float(st['z_vs_control'])!r}"
    return line + "\n"


def write_site_offsets(path, D, D_control=None):
    """site_offsets_{rank}_{name}.csv: the doubled offsets some site read has, ascending"""
    c = (len(D) - 1) // 2
    counts = {int(i) - c: [int(D[i]), 0] for i in np.nonzero(D)[0]}
    if D_control is not None:
        cc = (len(D_control) - 1) // 2
        for i in np.nonzero(D_control)[0]:
            counts.setdefault(int(i) - cc, [0, 0])[1] = int(D_control[i])
    with open(path, "w") as fh:
        fh.write("offset_x2,fg_sites" + (",control_sites\n" if D_control is not None else "\n"))
        for d in sorted(counts):
            fh.write(f"{d},{counts[d][0]}" + (f",{counts[d][1]}\n" if D_control is not None else "\n"))


# ---- the verb -----------------------------------------------------------------------------------------------------------------
def _motif_centrality(res_dir, library_files, control_fasta_file=None, p_value=1e-4, min_score=None, pseudocount=1.0,
                      nsites_default=20, revcom_mode=None, min_half=0, min_sites=10, top_hist=5, output_dir=None):
    """`kmap motif_centrality`: config.toml + the encoded reads of a preproc result directory + library files (+ a control FASTA)
    -> centrality_rank.csv, skipped.csv and site_offsets_{rank}_{name}.csv for the top_hist best in output_dir (default
    res_dir/motif_centrality).  Every file is parsed, every threshold found and every ValueError raised before the device is
    touched or a file is written; motifs whose width lies outside 4..31 are listed in skipped.csv.  Under a torch.distributed
    launch rank 0 works alone.  Returns one dict per motif in rank order: best_region's fields plus motif, rank, threshold, D,
    Hlen, q_bh and, with a control, D_control, control_sites, control_in_region, z_vs_control."""
    from .kmer_count import load_config, rank0_only, result_paths
    if not rank0_only():
        return None
    res, cfg_path, seq_path, border_path = result_paths(res_dir, reads=True)
    if control_fasta_file is not None and not Path(control_fasta_file).is_file():
        raise ValueError(f"control FASTA file {control_fasta_file} is missing")
    library_files = [str(f) for f in library_files]
    if not library_files:
        raise ValueError("motif_centrality: no library file given")
    if int(min_half) != min_half or min_half < 0:
        raise ValueError(f"min_half {min_half} < 0")
    if int(min_sites) != min_sites or min_sites < 1:
        raise ValueError(f"min_sites {min_sites} < 1")
    if int(top_hist) != top_hist or top_hist < 0:
        raise ValueError(f"top_hist {top_hist} < 0")
    t_fixed = None if min_score is None else min_score_threshold(min_score)
    _, revcom = load_config(cfg_path, revcom_mode)

    motifs, skipped, Ws, plans = load_library("motif_centrality", library_files, nsites_default, pseudocount, p_value, t_fixed)
    ts = [p[0] for p in plans]

    per_set = []
    with open_read_sets(seq_path, border_path, control_fasta_file) as read_sets:
        for ds in read_sets:
            if ds is not None:
                D, Hlen, _, too_long = ds.library_sites(Ws, ts, revcom)
                if np.any(np.asarray(too_long) != 0):
                    raise ValueError(f"motif_centrality: site reads of motif {motifs[int(np.nonzero(too_long)[0][0])].name} are longer "
                                     "than the longest read")
                per_set.append((D, Hlen))

    control = len(per_set) == 2
    results = []
    for i, (m, t) in enumerate(zip(motifs, ts)):
        st = best_region(per_set[0][0][i], per_set[0][1][i], m.counts.shape[1], min_half, min_sites)
        st.update(motif=m, threshold=t, D=per_set[0][0][i], Hlen=per_set[0][1][i])
        if control:
            Dc = per_set[1][0][i]
            a, nc = st["half_width_x2"], int(Dc.sum())
            kc = None if a is None else sites_within(Dc, a)
            st.update(D_control=Dc, control_sites=nc, control_in_region=kc,
                      z_vs_control=math.nan if a is None else enrich_z(st["sites_in_region"], kc, st["n_sites"], nc))
        results.append(st)
    for st, q in zip(results, bh_qvalues([10.0 ** st["log10_p_adj"] for st in results]).tolist()):
        st["q_bh"] = q
    results = [results[i] for i in rank_order([st["motif"].name for st in results], [st["z"] for st in results])]

    out = res / OUTPUT_DIR if output_dir is None else Path(output_dir)
    out.mkdir(parents=True, exist_ok=True)
    with open(out / RANK_FILE, "w") as fh:
        fh.write(RANK_HEADER + (CONTROL_HEADER if control else "") + "\n")
        for rank, st in enumerate(results):
            st["rank"] = rank
            fh.write(rank_line(rank, st["motif"], st["threshold"], st, control))
    write_skipped(out, skipped)
    for st in results[:int(top_hist)]:
        write_site_offsets(out / OFFSETS_FILE.format(rank=st["rank"], name=_file_name(st["motif"].name)), st["D"], st.get("D_control"))
    for st in results[:10]:
        m, a = st["motif"], st["half_width_x2"]
        where = (f"no region to test among {st['n_sites']} sites" if a is None else
                 f"{st['sites_in_region']} of {st['n_sites']} sites within {a / 2:.1f} bases of the centre, {st['expected_in_region']:.1f} "
                 f"expected, z {st['z']:.6g}, log10 p adj {st['log10_p_adj']:.2f}, q {st['q_bh']:.3g}")
        print(f"{st['rank']} {m.name}{' ' + m.altname if m.altname else ''}: at {st['threshold'] / SCORE_UNIT:.2f} bits {where}"
              + (f"; z against the control {st['z_vs_control']:.6g}" if control and a is not None else ""))
    print(f"motif_centrality: {len(results)} {'motif' if len(results) == 1 else 'motifs'} ranked, {len(skipped)} skipped, "
          f"{'both strands' if revcom else 'forward strand'}: {out}")
    return results
