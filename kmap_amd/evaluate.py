"""`kmap evaluate_pwm`: does a count matrix separate the reads of a result directory from control reads?  (the
reference has no such verb.)

scan_pwm and refine_pwm judge a matrix against the uniform 4^w null.  This module scores both read sets with the matrix -- per read
the best window, csrc/pwm_readscore.hip -- and compares the two distributions of best scores: a rank statistic (AUROC, Mann-Whitney
z with the tie correction) and the pooled two-proportion z of enrichment.py at every score threshold.  Scores are integers (0.01
bit), so everything behind the kernel is exact integer arithmetic on two histograms: no sort, no tolerance, two runs write the same
bytes.  Host code here is that arithmetic, argument checking and the file formats; the scoring has no CPU path."""
import math
from pathlib import Path

import numpy as np

from .enrichment import enrich_z, log2_fold
from .pwm import SCORE_UNIT, load_matrices

EVAL_FILE, HIST_FILE, READS_FILE = "pwm_eval.csv", "score_hist_motif{i}_{consensus}.csv", "read_scores_motif{i}_{consensus}.tsv"
OUTPUT_DIR = "pwm_eval"
EVAL_HEADER = ("motif,width,consensus,pseudocount,revcom,n_fg,n_control,fg_unscorable,control_unscorable,auroc,mw_z,"
               "threshold_p,threshold_p_bits,fg_reads_p,control_reads_p,log2_fold_p,z_p,"
               "threshold_best,threshold_best_bits,fg_reads_best,control_reads_best,z_best\n")
HIST_HEADER = "score,fg_reads,control_reads\n"
READS_HEADER = "seq_ind\tscore\tloc\tstrand\n"
MAX_BINS = 1 << 22


def _hist_pair(Hf, Hc):
    Hf, Hc = np.asarray(Hf), np.asarray(Hc)
    if Hf.ndim != 1 or Hf.shape != Hc.shape or Hf.dtype.kind not in "iu" or Hc.dtype.kind not in "iu":
        raise ValueError("two histograms of the same length with integer counts are expected")
    if (Hf.dtype.kind == "i" and (Hf < 0).any()) or (Hc.dtype.kind == "i" and (Hc < 0).any()):
        raise ValueError("a histogram count is negative")
    return Hf, Hc


def rank_stats(Hf, Hc):
    """(U2, auroc, mw_z) of two histograms over the same score bins, ascending.  U2 = sum_s Hf[s] (2 sum_{s' < s} Hc[s'] + Hc[s]) =
    twice the Mann-Whitney U of the foreground with a tie counting one half, a Python integer; auroc = U2 / (2 nf nc); mw_z =
    (U2 - nf nc) / 2 / sqrt(V), V = nf nc ((N + 1) N (N - 1) - sum_s (t_s^3 - t_s)) / (12 N (N - 1)), N = nf + nc, t_s = Hf[s] + Hc[s]:
    numerator and denominator of V are exact integers, divided once.  nf = 0, nc = 0 or V = 0 gives nan for both."""
    Hf, Hc = _hist_pair(Hf, Hc)
    f, c = [int(x) for x in Hf.tolist()], [int(x) for x in Hc.tolist()]
    nf, nc = sum(f), sum(c)
    U2 = below = ties = 0
    for x, y in zip(f, c):
        if x or y:
            U2 += x * (2 * below + y)
            below += y
            t = x + y
            ties += t * t * t - t
    N = nf + nc
    v_num = nf * nc * ((N + 1) * N * (N - 1) - ties)
    if nf == 0 or nc == 0 or v_num == 0:
        return U2, math.nan, math.nan
    return U2, U2 / (2 * nf * nc), float(U2 - nf * nc) / 2.0 / math.sqrt(v_num / (12 * N * (N - 1)))


def reads_at(Hf, Hc, lo, t):
    """(a, b): foreground and control reads whose best score is >= t (bin i holds the score lo + i)"""
    Hf, Hc = _hist_pair(Hf, Hc)
    i = min(max(int(t) - int(lo), 0), len(Hf))
    return int(Hf[i:].sum(dtype=np.uint64)), int(Hc[i:].sum(dtype=np.uint64))


def threshold_sweep(Hf, Hc, lo, min_reads=10):
    """The integer threshold t in [lo, lo + len(Hf)) with the largest z(t) = enrich_z(a(t), b(t), nf, nc) among those with
    a(t) + b(t) >= min_reads, on a tie the largest t: (t, a, b, z), or None when no threshold qualifies.  Between two occupied
    scores a and b do not change, so the largest t of every such stretch -- an occupied score -- is all that has to be evaluated."""
    Hf, Hc = _hist_pair(Hf, Hc)
    if int(min_reads) != min_reads or min_reads < 1:
        raise ValueError(f"min_reads {min_reads} < 1")
    occupied = np.nonzero((Hf != 0) | (Hc != 0))[0]
    a_at = np.cumsum(Hf[occupied][::-1].astype(np.uint64))[::-1].tolist()
    b_at = np.cumsum(Hc[occupied][::-1].astype(np.uint64))[::-1].tolist()
    nf, nc = (int(a_at[0]), int(b_at[0])) if len(occupied) else (0, 0)
    best = None
    for i, a, b in zip(occupied.tolist(), a_at, b_at):       # ascending t: a later equal z replaces an earlier one
        if a + b < min_reads:
            break
        z = enrich_z(a, b, nf, nc)
        if best is None or z >= best[3]:
            best = (int(lo) + i, int(a), int(b), z)
    return best


def evaluate_histograms(Hf, Hc, lo, t_p, min_reads=10):
    """every figure of a pwm_eval.csv row that comes from the two histograms: a dict with n_fg, n_control, U2, auroc, mw_z,
    threshold_p, fg_reads_p, control_reads_p, log2_fold_p, z_p and best = threshold_sweep's tuple or None"""
    Hf, Hc = _hist_pair(Hf, Hc)
    nf, nc = int(Hf.sum(dtype=np.uint64)), int(Hc.sum(dtype=np.uint64))
    U2, auroc, mw_z = rank_stats(Hf, Hc)
    a, b = reads_at(Hf, Hc, lo, t_p)
    return dict(n_fg=nf, n_control=nc, U2=U2, auroc=auroc, mw_z=mw_z, threshold_p=int(t_p), fg_reads_p=a, control_reads_p=b,
                log2_fold_p=log2_fold(a, b, nf, nc), z_p=enrich_z(a, b, nf, nc), best=threshold_sweep(Hf, Hc, lo, min_reads))


# ---- writers: floats as repr (the shortest text that reads back the same double), thresholds in bits as %.2f -------------------------
def eval_line(motif, width, consensus, pseudocount, revcom, fg_unscorable, control_unscorable, st):
    """one line of pwm_eval.csv from evaluate_histograms' dict"""
    best = st["best"]
    tail = (f"{best[0]},{best[0] / SCORE_UNIT:.2f},{best[1]},{best[2]},{float(best[3])!r}" if best is not None else ",,,,nan")
    return (f"{int(motif)},{int(width)},{consensus},{float(pseudocount)!r},{int(bool(revcom))},{st['n_fg']},{st['n_control']},"
            f"{int(fg_unscorable)},{int(control_unscorable)},{float(st['auroc'])!r},{float(st['mw_z'])!r},"
            f"{st['threshold_p']},{st['threshold_p'] / SCORE_UNIT:.2f},{st['fg_reads_p']},{st['control_reads_p']},"
            f"{float(st['log2_fold_p'])!r},{float(st['z_p'])!r},{tail}\n")


def write_eval_table(path, lines):
    with open(path, "w") as fh:
        fh.write(EVAL_HEADER)
        fh.write("".join(lines))


def write_score_hist(path, Hf, Hc, lo):
    """score_hist_motif{i}_{consensus}.csv: the scores some read has as its best, ascending"""
    Hf, Hc = _hist_pair(Hf, Hc)
    occupied = np.nonzero((Hf != 0) | (Hc != 0))[0]
    with open(path, "w") as fh:
        fh.write(HIST_HEADER)
        fh.write("".join(f"{int(lo) + i},{int(Hf[i])},{int(Hc[i])}\n" for i in occupied.tolist()))


def write_read_scores(path, score, loc, strand):
    """read_scores_motif{i}_{consensus}.tsv: one line per foreground read; NA for a read without a valid window"""
    with open(path, "w") as fh:
        fh.write(READS_HEADER)
        for a in range(0, len(score), 1 << 16):
            rows = []
            for r, (s, p, m) in enumerate(zip(score[a:a + (1 << 16)].tolist(), loc[a:a + (1 << 16)].tolist(),
                                              strand[a:a + (1 << 16)].tolist()), a):
                rows.append(f"{r}\tNA\tNA\tNA\n" if p < 0 else "%d\t%.2f\t%d\t%s\n" % (r, s / SCORE_UNIT, p, "-" if m else "+"))
            fh.write("".join(rows))


# ---- the verb -----------------------------------------------------------------------------------------------------------------
def _evaluate_pwm(res_dir, control_fasta_file, matrix_files, p_value=1e-4, min_score=None, pseudocount=1.0, revcom_mode=None,
                  min_reads=10, read_scores=False, output_dir=None):
    """`kmap evaluate_pwm`: config.toml + the encoded reads of a preproc result directory + a control FASTA + count matrix files ->
    pwm_eval.csv, score_hist_motif{i}_{consensus}.csv per matrix and (read_scores) read_scores_motif{i}_{consensus}.tsv in output_dir
    (default res_dir/pwm_eval).  Every matrix is read, its thresholds found and every ValueError raised before the device is touched
    or a file is written.  Under a torch.distributed launch rank 0 works alone.  Returns one dict per matrix: evaluate_histograms'
    fields plus Hf, Hc, lo, fg_unscorable, control_unscorable."""
    from .kmer_count import encode_fasta, load_array_pickle, load_config, rank0_only, result_paths
    if not rank0_only():
        return None
    res, cfg_path, seq_path, border_path = result_paths(res_dir, reads=True)
    if control_fasta_file is None or not Path(control_fasta_file).is_file():
        raise ValueError(f"control FASTA file {control_fasta_file} is missing")
    matrix_files = [str(f) for f in matrix_files]
    if not matrix_files:
        raise ValueError("evaluate_pwm: no matrix file given")
    if int(min_reads) != min_reads or min_reads < 1:
        raise ValueError(f"min_reads {min_reads} < 1")
    _, revcom = load_config(cfg_path, revcom_mode)

    def check_bins(lo, hi):
        if hi - lo + 1 > MAX_BINS:
            raise ValueError(f"scores from {lo} to {hi}: more than 2^22 different scores are not supported")
    motifs = load_matrices(matrix_files, pseudocount, p_value, min_score, check_bins)

    from .motif_discovery import DeviceSeq
    fg_seq = DeviceSeq(load_array_pickle(seq_path), load_array_pickle(border_path))
    ctl_seq, results, per_read = None, [], []
    try:
        ctl_seq = DeviceSeq(*encode_fasta(str(control_fasta_file)))
        for _, _, W, _, t, lo, hi in motifs:
            hists, unscorable = [], []
            for ds in (fg_seq, ctl_seq):
                rs = ds.read_scores(W, revcom)
                try:
                    hists.append(rs.histogram(lo, hi - lo + 1))
                    unscorable.append(ds.n_seq - rs.n_scored)
                    if read_scores and ds is fg_seq:
                        per_read.append(rs.fetch())
                finally:
                    rs.close()
            st = evaluate_histograms(hists[0], hists[1], lo, t, min_reads)
            st.update(Hf=hists[0], Hc=hists[1], lo=lo, fg_unscorable=unscorable[0], control_unscorable=unscorable[1])
            results.append(st)
    finally:
        for h in (ctl_seq, fg_seq):
            if h is not None:
                h.close()

    out = res / OUTPUT_DIR if output_dir is None else Path(output_dir)
    out.mkdir(parents=True, exist_ok=True)
    lines = []
    for i, ((f, C, W, cons, t, lo, hi), st) in enumerate(zip(motifs, results)):
        lines.append(eval_line(i, C.shape[1], cons, pseudocount, revcom, st["fg_unscorable"], st["control_unscorable"], st))
        write_score_hist(out / HIST_FILE.format(i=i, consensus=cons), st["Hf"], st["Hc"], lo)
        if read_scores:
            write_read_scores(out / READS_FILE.format(i=i, consensus=cons), *per_read[i])
        best = st["best"]
        note = (f"best threshold {best[0] / SCORE_UNIT:.2f} bits: {best[1]} / {best[2]} reads, z={best[3]:.6g}" if best is not None
                else f"no threshold leaves {min_reads} reads or more: no best threshold")
        print(f"motif {i} {cons}: auroc {st['auroc']:.4f}, mw_z {st['mw_z']:.6g}; at {t / SCORE_UNIT:.2f} bits {st['fg_reads_p']} of "
              f"{st['n_fg']} reads against {st['control_reads_p']} of {st['n_control']} control reads, z={st['z_p']:.6g}; {note}")
    write_eval_table(out / EVAL_FILE, lines)
    print(f"evaluate_pwm: {len(motifs)} {'matrix' if len(motifs) == 1 else 'matrices'}, {'both strands' if revcom else 'forward strand'}: {out}")
    return results
