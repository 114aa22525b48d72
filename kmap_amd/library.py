"""`kmap rank_motif_library`: which motifs of a library of known motifs are enriched in the reads of a result directory against
control reads?  (the reference has no such verb.)

evaluate_pwm answers the question for one matrix at a time, with a pass over the reads, three per-read arrays and a histogram call
per matrix.  This module reads a whole library -- MEME minimal text, or the count-matrix CSVs the other verbs write --, turns every
motif into pwm.py's integer weights and threshold, and has csrc/pwm_library.hip score reads and control against batches of matrices
in one pass each, straight to the histograms of the best scores.  Behind the kernel everything is evaluate.py's exact integer
arithmetic on two histograms per motif; added here are the one-sided p of the Mann-Whitney z, Benjamini-Hochberg q-values over the
library and the ranking.  Host code is parsing, that arithmetic and the file formats; the scoring has no CPU path."""
import contextlib
import math
import re
from pathlib import Path

import numpy as np

from .evaluate import EVAL_HEADER, MAX_BINS, eval_line, evaluate_histograms, write_score_hist
from .pwm import MAX_WIDTH, MIN_WIDTH, SCORE_UNIT, pwm_consensus, pwm_threshold, pwm_weights, read_count_matrix

OUTPUT_DIR, RANK_FILE, SKIPPED_FILE, HIST_FILE = "pwm_library", "library_rank.csv", "skipped.csv", "score_hist_{rank}_{name}.csv"
RANK_HEADER = "rank,name,altname,source," + EVAL_HEADER.rstrip("\n").split(",", 1)[1] + ",log10_p,q_bh\n"
SKIPPED_HEADER = "name,altname,source,reason\n"
_KEY_VALUE = re.compile(r"(\w+)=\s*(\S+)")
_SKIP_LINES = ("MEME version", "ALPHABET", "strands:", "URL")


class LibraryMotif:
    """one motif of a library: `counts` int64 [4, w] (rows A C G T), or None with `skip` = why it cannot be used"""

    def __init__(self, name, altname, source, counts=None, skip=None):
        self.name, self.altname, self.source, self.counts, self.skip = _field(name), _field(altname), str(source), counts, skip


def _field(text):
    return str(text).replace(",", "_")                       # the tables are comma-separated


def _number(text):
    try:
        x = float(text)
    except ValueError:
        return math.nan
    return x if math.isfinite(x) else math.nan


def _width_skip(w):
    return None if MIN_WIDTH <= w <= MAX_WIDTH else f"width {w} outside {MIN_WIDTH}..{MAX_WIDTH}"


def read_meme(path, nsites_default=20):
    """[LibraryMotif] of a MEME minimal text file.  `MOTIF id [altname]` starts a motif; `letter-probability matrix: alength= 4 w= W
    [nsites= N] ...` is followed by W rows of four probabilities in A C G T order (without w=: the rows up to the first line that is
    not four numbers); counts = round(p nsites), nsites = nsites_default when absent or below 1.  The version, ALPHABET, strands: and
    URL lines, the background block with its frequency row and anything else outside a matrix are passed over.  A motif whose width
    lies outside 4..31 or that has no matrix is returned with `skip` set.  ValueError naming file and line: another alphabet, a row
    that is not four numbers or does not sum to 1 within 0.01, a matrix before the first MOTIF line."""
    if int(nsites_default) != nsites_default or nsites_default < 1:
        raise ValueError(f"nsites_default {nsites_default} < 1")
    with open(path, newline=None) as fh:                      # universal newlines: a file with Windows line ends reads the same
        lines = fh.read().split("\n")
    motifs, cur, i = [], None, 0

    def close(m):
        if m is not None:
            motifs.append(m if m.counts is not None or m.skip else LibraryMotif(m.name, m.altname, path, skip="no letter-probability matrix"))
    while i < len(lines):
        line, at = lines[i].strip(), i + 1
        i += 1
        if not line or line.startswith(_SKIP_LINES):
            continue
        if line.startswith("Background letter frequencies"):
            while i < len(lines) and not lines[i].strip():
                i += 1
            i += 1                                           # its frequency row
            continue
        if line.startswith("MOTIF"):
            close(cur)
            words = line.split()
            if len(words) < 2:
                raise ValueError(f"{path}:{at}: a MOTIF line without an identifier")
            cur = LibraryMotif(words[1], words[2] if len(words) > 2 else "", path)
            continue
        if not line.startswith("letter-probability matrix"):
            continue
        if cur is None:
            raise ValueError(f"{path}:{at}: a letter-probability matrix in front of the first MOTIF line")
        if cur.counts is not None or cur.skip:
            raise ValueError(f"{path}:{at}: a second letter-probability matrix for motif {cur.name}")
        keys = dict(_KEY_VALUE.findall(line))
        if keys.get("alength", "4") != "4":
            raise ValueError(f"{path}:{at}: alength= {keys['alength']}: only the DNA alphabet (alength= 4, A C G T) is supported")
        w = _number(keys["w"]) if "w" in keys else None
        if w is not None and (w != w or w < 1 or int(w) != w):
            raise ValueError(f"{path}:{at}: w= {keys['w']} is not a positive integer")
        nsites = _number(keys.get("nsites", "nan"))
        nsites = int(round(nsites)) if nsites >= 1 else int(nsites_default)
        rows = []
        while i < len(lines) and (w is None or len(rows) < w):
            row, row_at = lines[i].split(), i + 1
            p = [_number(x) for x in row]
            bad = len(p) != 4 or any(x != x or x < 0 for x in p)
            if bad and (w is None or not row):               # the end of the rows: a line of something else; with w=, a blank one
                break
            i += 1
            if bad:
                raise ValueError(f"{path}:{row_at}: row {len(rows) + 1} of motif {cur.name} is not four probabilities (A C G T)")
            if abs(sum(p) - 1.0) > 0.01:
                raise ValueError(f"{path}:{row_at}: row {len(rows) + 1} of motif {cur.name} sums to {sum(p):.4f}, not to 1 within 0.01")
            rows.append(p)
        if w is not None and len(rows) < w:
            raise ValueError(f"{path}:{at}: motif {cur.name} announces w= {int(w)}, {len(rows)} rows follow")
        cur.skip = _width_skip(len(rows))
        if cur.skip is None:
            cur.counts = np.rint(np.array(rows, np.float64).T * nsites).astype(np.int64)
    close(cur)
    if not motifs:
        raise ValueError(f"{path}: no MOTIF line")
    return motifs


def _is_meme(path):
    with open(path, errors="replace") as fh:
        return any(line.startswith(("MEME version", "MOTIF")) for line in fh)


def read_motif_library(path, nsites_default=20):
    """[LibraryMotif] of a library file, its format detected by content: MEME minimal text (read_meme), else a count-matrix CSV
    (pwm.read_count_matrix, the motif named by the file stem).  A directory stands for every *.csv and *.meme in it, in sorted order."""
    p = Path(path)
    if p.is_dir():
        files = sorted(f for f in p.iterdir() if f.suffix in (".csv", ".meme") and f.is_file())
        if not files:
            raise ValueError(f"{path}: no *.csv or *.meme file in this directory")
        return [m for f in files for m in read_motif_library(f, nsites_default)]
    if not p.is_file():
        raise ValueError(f"library file {path} is missing")
    if _is_meme(p):
        return read_meme(str(path), nsites_default)
    return [LibraryMotif(p.stem, "", path, read_count_matrix(str(path)))]


def load_library(who, library_files, nsites_default, pseudocount, p_value, t_fixed=None, veto=None):
    """What the library verbs score: every motif of library_files (read_motif_library, in file order) as pwm.py's integer weights
    and threshold.  Returns (motifs, skipped, Ws, plans): the motifs kept, those left out with `skip` set (a width outside 4..31,
    or veto(W, t, lo, hi) gave the reason), and per motif kept W and plan = pwm_threshold(W, p_value)'s (t, lo, hi) -- with t_fixed
    in t's place when one is given.  ValueError: a file that cannot be read, `{source}: motif {name}: ...` for a matrix without
    weights or threshold, and under `who` a library none of whose motifs is kept."""
    motifs, skipped, Ws, plans = [], [], [], []
    for f in library_files:
        for m in read_motif_library(f, nsites_default):
            if m.skip is None:
                try:
                    W = pwm_weights(m.counts, pseudocount)
                    t, lo, hi = pwm_threshold(W, p_value)
                except ValueError as exc:
                    raise ValueError(f"{m.source}: motif {m.name}: {exc}") from None
                if veto is not None:
                    m.skip = veto(W, t, lo, hi)
            if m.skip is None:
                motifs.append(m)
                Ws.append(W)
                plans.append((t if t_fixed is None else t_fixed, lo, hi))
            else:
                skipped.append(m)
    if not motifs:
        raise ValueError(f"{who}: none of the {len(skipped)} motifs of the library can be scored "
                         f"(the first: {skipped[0].name}: {skipped[0].skip})")
    return motifs, skipped, Ws, plans


@contextlib.contextmanager
def open_read_sets(seq_path, border_path, control_fasta_file=None):
    """(fg_seq, ctl_seq): the encoded reads of a result directory and, with a control FASTA, the control reads (else None) as
    DeviceSeq, the foreground opened first; both are closed on the way out"""
    from .kmer_count import encode_fasta, load_array_pickle
    from .motif_discovery import DeviceSeq
    fg_seq = DeviceSeq(load_array_pickle(seq_path), load_array_pickle(border_path))
    ctl_seq = None
    try:
        if control_fasta_file is not None:
            ctl_seq = DeviceSeq(*encode_fasta(str(control_fasta_file)))
        yield fg_seq, ctl_seq
    finally:
        for h in (ctl_seq, fg_seq):
            if h is not None:
                h.close()


def write_skipped(out, skipped):
    """skipped.csv in the directory `out`: the motifs that were not scored and why"""
    with open(out / SKIPPED_FILE, "w") as fh:
        fh.write(SKIPPED_HEADER)
        fh.write("".join(f"{m.name},{m.altname},{m.source},{_field(m.skip)}\n" for m in skipped))


def bh_qvalues(p):
    """Benjamini-Hochberg q-values of the p-values (nan counts as 1): the step-up procedure, q of the i-th smallest of n = the
    minimum over j >= i of p_(j) n / j, at most 1.  The sort is stable (ties keep the input order; they get the same q)."""
    p = np.asarray(p, np.float64).reshape(-1)
    p = np.where(np.isnan(p), 1.0, p)
    n = len(p)
    order = np.argsort(p, kind="stable")
    scaled = p[order] * n / np.arange(1, n + 1)
    q = np.empty(n, np.float64)
    q[order] = np.minimum(np.minimum.accumulate(scaled[::-1])[::-1], 1.0)
    return q


def log10_p_of_z(z):
    """log10 of the upper normal tail of z (one-sided: enriched in the reads); a nan z has p = 1"""
    from .kmer_count import norm_logsf
    return 0.0 if z != z else float(norm_logsf(z, 0.0, 1.0)) / math.log(10.0)


def rank_order(names, mw_z):
    """indices by mw_z descending, then name, nan last"""
    return sorted(range(len(names)), key=lambda i: (mw_z[i] != mw_z[i], 0.0 if mw_z[i] != mw_z[i] else -mw_z[i], names[i]))


def rank_line(rank, motif, pseudocount, revcom, st):
    """one line of library_rank.csv: pwm_eval.csv's columns from `width` on in eval_line's formatting, between the motif's names and
    its p and q"""
    tail = eval_line(0, motif.counts.shape[1], pwm_consensus(motif.counts), pseudocount, revcom, st["fg_unscorable"],
                     st["control_unscorable"], st).rstrip("\n").split(",", 1)[1]
    return f"{int(rank)},{motif.name},{motif.altname},{motif.source},{tail},{float(st['log10_p'])!r},{float(st['q_bh'])!r}\n"


def _file_name(name):
    return re.sub(r"[^A-Za-z0-9._+-]", "_", name)


# ---- the verb -----------------------------------------------------------------------------------------------------------------
def _rank_motif_library(res_dir, control_fasta_file, library_files, p_value=1e-4, pseudocount=1.0, nsites_default=20, revcom_mode=None,
                        min_reads=10, top_hist=0, output_dir=None):
    """`kmap rank_motif_library`: config.toml + the encoded reads of a preproc result directory + a control FASTA + library files ->
    library_rank.csv, skipped.csv and score_hist_{rank}_{name}.csv for the top_hist best in output_dir (default
    res_dir/pwm_library).  Every file is parsed, every threshold found and every ValueError raised before the device is touched or
    a file is written; motifs that cannot be scored (width outside 4..31, more than 2^22 different scores) are listed in skipped.csv.
    Under a torch.distributed launch rank 0 works alone.  Returns one dict per evaluated motif in rank order: evaluate_histograms'
    fields plus motif, rank, Hf, Hc, lo, fg_unscorable, control_unscorable, log10_p, q_bh."""
    from .kmer_count import load_config, rank0_only, result_paths
    if not rank0_only():
        return None
    res, cfg_path, seq_path, border_path = result_paths(res_dir, reads=True)
    if control_fasta_file is None or not Path(control_fasta_file).is_file():
        raise ValueError(f"control FASTA file {control_fasta_file} is missing")
    library_files = [str(f) for f in library_files]
    if not library_files:
        raise ValueError("rank_motif_library: no library file given")
    if int(min_reads) != min_reads or min_reads < 1:
        raise ValueError(f"min_reads {min_reads} < 1")
    if int(top_hist) != top_hist or top_hist < 0:
        raise ValueError(f"top_hist {top_hist} < 0")
    _, revcom = load_config(cfg_path, revcom_mode)

    motifs, skipped, Ws, plans = load_library(
        "rank_motif_library", library_files, nsites_default, pseudocount, p_value,
        veto=lambda W, t, lo, hi: f"scores from {lo} to {hi}: more than 2^22 different scores" if hi - lo + 1 > MAX_BINS else None)

    los, nbs = [p[1] for p in plans], [p[2] - p[1] + 1 for p in plans]
    per_set = []
    with open_read_sets(seq_path, border_path, control_fasta_file) as read_sets:
        for ds in read_sets:
            hists, outside, scored = ds.library_histograms(Ws, los, nbs, revcom)
            if np.any(np.asarray(outside) != 0):
                raise ValueError(f"rank_motif_library: reads score outside the score range of motif {motifs[int(np.nonzero(outside)[0][0])].name}")
            per_set.append((hists, [ds.n_seq - int(s) for s in scored]))

    results = []
    for i, (m, (t, lo, hi)) in enumerate(zip(motifs, plans)):
        Hf, Hc = per_set[0][0][i], per_set[1][0][i]
        st = evaluate_histograms(Hf, Hc, lo, t, min_reads)
        st.update(motif=m, Hf=Hf, Hc=Hc, lo=lo, fg_unscorable=per_set[0][1][i], control_unscorable=per_set[1][1][i],
                  log10_p=log10_p_of_z(st["mw_z"]))
        results.append(st)
    for st, q in zip(results, bh_qvalues([10.0 ** st["log10_p"] for st in results]).tolist()):
        st["q_bh"] = q
    results = [results[i] for i in rank_order([st["motif"].name for st in results], [st["mw_z"] for st in results])]

    out = res / OUTPUT_DIR if output_dir is None else Path(output_dir)
    out.mkdir(parents=True, exist_ok=True)
    with open(out / RANK_FILE, "w") as fh:
        fh.write(RANK_HEADER)
        for rank, st in enumerate(results):
            st["rank"] = rank
            fh.write(rank_line(rank, st["motif"], pseudocount, revcom, st))
    write_skipped(out, skipped)
    for st in results[:int(top_hist)]:
        write_score_hist(out / HIST_FILE.format(rank=st["rank"], name=_file_name(st["motif"].name)), st["Hf"], st["Hc"], st["lo"])
    for st in results[:10]:
        m = st["motif"]
        print(f"{st['rank']} {m.name}{' ' + m.altname if m.altname else ''}: auroc {st['auroc']:.4f}, mw_z {st['mw_z']:.6g}, "
              f"log10 p {st['log10_p']:.2f}, q {st['q_bh']:.3g}; at {st['threshold_p'] / SCORE_UNIT:.2f} bits {st['fg_reads_p']} of "
              f"{st['n_fg']} reads against {st['control_reads_p']} of {st['n_control']} control reads")
    print(f"rank_motif_library: {len(results)} {'motif' if len(results) == 1 else 'motifs'} ranked, {len(skipped)} skipped, "
          f"{'both strands' if revcom else 'forward strand'}: {out}")
    return results
