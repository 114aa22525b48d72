"""`kmap scan_pwm`: score every read position against a base-count matrix (the reference has no such verb).

scan_motif and `ex_hamball --return_type matrix` write a 4 x w count matrix per motif (hamming_balls/cntmat_*.csv).  This module
reads such a file back, turns it into integer log-odds weights (unit 0.01 bit, uniform background, pseudocount), finds the score
threshold of a p-value exactly (integer DP over all 4^w sequences) and scans the packed reads with csrc/pwm_scan.hip.  The hits
leave in the occurrence-CSV contract, so extract_motif_locations and the co-occurrence / density functions read them unchanged.
Definitions: DESIGN.md section 11.  Host code here is small-matrix arithmetic only; the scan has no CPU path."""
import math
import re
from decimal import Decimal
from pathlib import Path

import numpy as np

MIN_WIDTH, MAX_WIDTH = 4, 31          # the package's k range: the scored window spans at most three code words
SCORE_UNIT = 100                      # weights and scores are integers in units of 1 / SCORE_UNIT bit
OCCURRENCE_FILE, CONSEQ_FILE, HITS_FILE, INFO_FILE = "pwm.motif_occurence.csv", "pwm_conseq.txt", "pwm_hits.tsv", "pwm_info.csv"
_ROW = re.compile(r"\d+(,\d+)*")


def read_count_matrix(path):
    """A count matrix file -> int64 [4, w], rows A C G T.  The file has exactly the form np.savetxt(..., delimiter=",", fmt="%d")
    writes for a 4 x w grid of non-negative integers with 4 <= w <= 31; anything else raises ValueError naming the file."""
    with open(path) as fh:
        lines = fh.read().split("\n")
    if lines and lines[-1] == "":
        lines.pop()
    if len(lines) != 4:
        raise ValueError(f"{path}: {len(lines)} rows, a count matrix has 4 (A, C, G, T)")
    rows = []
    for r, line in enumerate(lines, 1):
        if not _ROW.fullmatch(line):
            raise ValueError(f"{path}:{r}: not a comma-separated row of non-negative integers")
        rows.append([int(x) for x in line.split(",")])
    if len({len(r) for r in rows}) != 1:
        raise ValueError(f"{path}: rows of {[len(r) for r in rows]} entries, a count matrix has 4 rows of equal length")
    w = len(rows[0])
    if not MIN_WIDTH <= w <= MAX_WIDTH:
        raise ValueError(f"{path}: width {w} outside {MIN_WIDTH}..{MAX_WIDTH}")
    if max(max(r) for r in rows) >= 2 ** 60:
        raise ValueError(f"{path}: a count of 2^60 or more")
    return np.array(rows, np.int64)


def _check_counts(C):
    C = np.asarray(C)
    if C.ndim != 2 or C.shape[0] != 4 or not MIN_WIDTH <= C.shape[1] <= MAX_WIDTH or C.dtype.kind not in "iu" or (C < 0).any():
        raise ValueError(f"a count matrix is 4 x w non-negative integers, {MIN_WIDTH} <= w <= {MAX_WIDTH}")
    return C.astype(np.int64)


def pwm_weights(C, pseudocount=1.0):
    """W[b][j] = rint(100 log2(f[b][j] / 0.25)) as int32, f[b][j] = (C[b][j] + a / 4) / (sum_b C[b][j] + a), a = pseudocount,
    in float64.  A zero count with a = 0 has no finite weight: ValueError."""
    C = _check_counts(C)
    a = float(pseudocount)
    if not a >= 0 or math.isinf(a):
        raise ValueError(f"pseudocount {pseudocount} is not a finite number >= 0")
    if a == 0 and (C == 0).any():
        raise ValueError("a column with a zero count needs a pseudocount > 0 (its weight would be infinite)")
    f = (C + a / 4) / (C.sum(axis=0) + a)
    return np.rint(np.log2(f / 0.25) * SCORE_UNIT).astype(np.int32)


def pwm_consensus(C):
    """the most frequent base of every column; the first of A, C, G, T on ties"""
    C = _check_counts(C)
    return "".join("ACGT"[i] for i in np.argmax(C, axis=0))


def _check_weights(W):
    W = np.asarray(W)
    if W.ndim != 2 or W.shape[0] != 4 or not MIN_WIDTH <= W.shape[1] <= MAX_WIDTH or W.dtype.kind not in "iu":
        raise ValueError(f"a weight matrix is 4 x w integers, {MIN_WIDTH} <= w <= {MAX_WIDTH}")
    W = W.astype(np.int64)
    if np.abs(W).max() >= 2 ** 31 // MAX_WIDTH:
        raise ValueError("weights too large: a window's score must fit int32")
    return W


def score_counts(W):
    """(min_score, counts): counts[s - min_score] = how many of the 4^w sequences have the forward score s, int64 (4^31 < 2^63);
    column by column, every column adds its four weights to the distribution so far"""
    W = _check_weights(W)
    lo, hi = W.min(axis=0), W.max(axis=0)
    dist = np.ones(1, np.int64)
    for j in range(W.shape[1]):
        nxt = np.zeros(len(dist) + int(hi[j] - lo[j]), np.int64)
        for b in range(4):
            d = int(W[b, j] - lo[j])
            nxt[d:d + len(dist)] += dist
        dist = nxt
    return int(lo.sum()), dist


def pwm_threshold(W, p_value):
    """(t, min_score, max_score): t = the smallest integer score with N(t) <= p_value 4^w, N(s) = number of the 4^w sequences whose
    forward score is >= s (exact).  N(max_score) > p_value 4^w gives t = max_score + 1 (no window can hit); p_value >= 1 gives
    min_score.  The p-value is per strand and per position."""
    p = float(p_value)
    if not p >= 0:
        raise ValueError(f"p_value {p_value} is not a number >= 0")
    min_score, dist = score_counts(W)
    max_score = min_score + len(dist) - 1
    total = 4 ** np.asarray(W).shape[1]
    limit = total if p >= 1 else min(total, math.floor(p * float(total)))     # 4^w is a power of two: the product is exact
    n_ge = np.cumsum(dist[::-1])[::-1]                                          # N(min_score + i)
    ok = np.nonzero(n_ge <= limit)[0]
    t = min_score + int(ok[0]) if len(ok) else max_score + 1
    return t, min_score, max_score


def min_score_threshold(min_score_bits):
    """t = ceil(100 S) for --min_score S, S read as the decimal number written (10.62 gives 1062, not the 1063 of the nearest double)"""
    s = float(min_score_bits)
    if math.isnan(s) or math.isinf(s) or abs(s) * SCORE_UNIT >= 2 ** 31 - 1:
        raise ValueError(f"min_score {min_score_bits} is out of range")
    return int((Decimal(repr(s)) * SCORE_UNIT).to_integral_value(rounding="ROUND_CEILING"))


def load_matrices(matrix_files, pseudocount, p_value, min_score=None, check=None):
    """[(file, C, W, consensus, t, min_score, max_score)] of count matrix files: weights, the p-value's threshold (min_score given:
    that one instead) and the score range; check(lo, hi) may refuse a matrix.  A ValueError names the file."""
    motifs = []
    for f in matrix_files:
        C = read_count_matrix(f)
        try:
            W = pwm_weights(C, pseudocount)
            t, lo, hi = pwm_threshold(W, p_value)
            if check is not None:
                check(lo, hi)
        except ValueError as exc:
            raise ValueError(f"{f}: {exc}") from None
        if min_score is not None:
            t = min_score_threshold(min_score)
        motifs.append((f, C, W, pwm_consensus(C), t, lo, hi))
    return motifs


def _scan_pwm(res_dir, matrix_files, p_value=1e-4, min_score=None, pseudocount=1.0, revcom_mode=None, output_dir=None):
    """`kmap scan_pwm`: config.toml + the encoded reads of a preproc result directory + count matrix files -> pwm.motif_occurence.csv,
    pwm_conseq.txt, pwm_hits.tsv, pwm_info.csv in output_dir (default res_dir/pwm_scan).  Every matrix is read and its threshold
    found before the device is touched or a file is written.  Under a torch.distributed launch rank 0 scans alone.
    Returns [(hits_per_read, positions, scores, strand)] per matrix."""
    from .kmer_count import load_array_pickle, load_config, rank0_only, result_paths
    if not rank0_only():
        return None
    res, cfg_path, seq_path, border_path = result_paths(res_dir, reads=True)
    matrix_files = [str(f) for f in matrix_files]
    if not matrix_files:
        raise ValueError("scan_pwm: no matrix file given")
    _, revcom = load_config(cfg_path, revcom_mode)
    motifs = load_matrices(matrix_files, pseudocount, p_value, min_score)

    from .motif_discovery import DeviceSeq, write_occurence_file
    dev_seq = DeviceSeq(load_array_pickle(seq_path), load_array_pickle(border_path))
    try:
        per = [dev_seq.scan_pwm(W, t, revcom) for _, _, W, _, t, _, _ in motifs]
        out = res / "pwm_scan" if output_dir is None else Path(output_dir)
        out.mkdir(parents=True, exist_ok=True)
        conseqs = [m[3] for m in motifs]
        write_occurence_file([[h, p] for h, p, _, _ in per], conseqs, out / OCCURRENCE_FILE, dev_seq.out_n_seq, dev_seq.out_read_len)
    finally:
        dev_seq.close()
    with open(out / CONSEQ_FILE, "w") as fh:
        fh.write("".join(c + "\n" for c in conseqs))
    with open(out / HITS_FILE, "w") as fh:
        fh.write("motif\tseq_ind\tloc\tstrand\tscore\n")
        for i, (hits, pos, scores, strand) in enumerate(per):
            seq_ind = np.repeat(np.arange(len(hits), dtype=np.int64), hits)
            sign = np.where(strand == 0, "+", "-")
            for a in range(0, len(pos), 1 << 16):
                b = min(a + (1 << 16), len(pos))
                flat = np.empty((b - a, 5), object)
                flat[:, 0] = i
                flat[:, 1], flat[:, 2], flat[:, 3] = seq_ind[a:b].tolist(), pos[a:b].tolist(), sign[a:b].tolist()
                flat[:, 4] = (scores[a:b] / SCORE_UNIT).tolist()
                fh.write(("%d\t%d\t%d\t%s\t%.2f\n" * (b - a)) % tuple(flat.ravel().tolist()))
    with open(out / INFO_FILE, "w") as fh:
        fh.write("motif,matrix_file,width,consensus,pseudocount,p_value,threshold,threshold_bits,min_score,max_score,n_hits,n_reads_hit\n")
        for i, ((f, C, W, cons, t, lo, hi), (hits, pos, _, _)) in enumerate(zip(motifs, per)):
            fh.write(f"{i},{f},{C.shape[1]},{cons},{float(pseudocount)!r},{float(p_value)!r},{t},{t / SCORE_UNIT:.2f},{lo},{hi},"
                     f"{len(pos)},{int(np.count_nonzero(hits))}\n")
            note = "  (no window can reach the threshold: it lies above the matrix's best score)" if t > hi else ""
            print(f"motif {i} {cons}: threshold {t / SCORE_UNIT:.2f} bits, {len(pos)} hits in {int(np.count_nonzero(hits))} reads{note}")
    print(f"scan_pwm: {len(motifs)} {'matrix' if len(motifs) == 1 else 'matrices'}, {'both strands' if revcom else 'forward strand'}: {out}")
    return per
