"""`kmap enrich_kmers`: k-mers and motifs enriched in the reads of a result directory over a set of control reads (DESIGN.md section
12; the reference has no such verb).

find_motif and scan_pwm measure against a uniform null.  This module counts the control reads (input DNA, flanks, round 0, a
shuffled set) on the device like the foreground, joins the two tables where they lie in HBM (csrc/enrich.hip), scores every
foreground k-mer with the pooled two-proportion z and selects the best rows exactly, ties by table index.  The motif table needs no
kernel of its own: the Hamming-ball mass of every consensus over both tables.  Host code here is argument checking, the few written
rows and the file formats; the join, the scores and the selection have no CPU path."""
import ctypes as C
import math
from pathlib import Path

import numpy as np

from . import _ffi
from ._ffi import check, ptr

KMER_FILE, INFO_FILE, MOTIF_FILE = "enriched_kmers_k{k}.tsv", "enrichment_info.csv", "motif_enrichment.csv"
OUTPUT_DIR = "kmer_enrichment"
KMER_HEADER = "rank\tkmer\trevcom_kmer\tfg_count\tcontrol_count\tfg_share\tcontrol_share\tlog2_fold\tz\n"
INFO_HEADER = "k,dedupe,revcom,n_fg_uniq,n_control_uniq,Nf,Nb,min_count,n_eligible,n_written\n"
MOTIF_HEADER = ("conseq,k,max_ham_dist,fg_mass,control_mass,Nf,Nb,fg_share,control_share,fg_ratio,control_ratio,log2_fold,z\n")
MAX_TOTAL = 2 ** 52 - 1


# ---- the statistic on the host (the motif table; the k-mer table's z comes from the device) -------------------------------------
def enrich_z(a, b, Nf, Nb):
    """pooled two-proportion z of a of Nf against b of Nb: D = a Nb - b Nf as a Python integer, converted to float once;
    s = ((a + b)(Nf + Nb - a - b)) ((Nf Nb) / (Nf + Nb)) in float64 in this order; D / sqrt(s), 0.0 unless s > 0.  The device
    kernel evaluates the same expression."""
    a, b, Nf, Nb = int(a), int(b), int(Nf), int(Nb)
    if Nf + Nb == 0:
        return 0.0
    s = (float(a + b) * float(Nf + Nb - a - b)) * ((float(Nf) * float(Nb)) / float(Nf + Nb))
    return float(a * Nb - b * Nf) / math.sqrt(s) if s > 0.0 else 0.0


def _log2(x):
    return math.log2(x) if x > 0 else -math.inf


def log2_fold(a, b, Nf, Nb, pseudocount=1.0):
    """log2((a + pc) / (Nf + pc)) - log2((b + pc) / (Nb + pc))"""
    pc = float(pseudocount)
    if Nf + pc <= 0 or Nb + pc <= 0:          # an empty read set and no pseudocount: no share to compare
        return math.nan
    return _log2((a + pc) / (Nf + pc)) - _log2((b + pc) / (Nb + pc))


def _share(x, n):
    return x / n if n else 0.0


# ---- writers ------------------------------------------------------------------------------------------------------------------
def write_kmer_table(path, k, kh, a, b, z, Nf, Nb, pseudocount=1.0):
    """enriched_kmers_k{k}.tsv: the given rows in the given (rank) order"""
    from .kmer_count import hash2kmer, reverse_complement
    with open(path, "w") as fh:
        fh.write(KMER_HEADER)
        for r, (h, ai, bi, zi) in enumerate(zip(kh, a, b, z), 1):
            kmer = hash2kmer(int(h), k)
            ai, bi = int(ai), int(bi)
            fh.write(f"{r}\t{kmer}\t{reverse_complement(kmer)}\t{ai}\t{bi}\t{_share(ai, Nf):.6e}\t{_share(bi, Nb):.6e}\t"
                     f"{log2_fold(ai, bi, Nf, Nb, pseudocount):.6g}\t{float(zi):.6g}\n")


def write_info_table(path, rows):
    """enrichment_info.csv: one row per k, each a dict with the header's fields"""
    names = INFO_HEADER.strip().split(",")
    with open(path, "w") as fh:
        fh.write(INFO_HEADER)
        for row in rows:
            fh.write(",".join(str(int(row[n])) for n in names) + "\n")


def motif_row(conseq, d, fg_mass, control_mass, Nf, Nb, pseudocount=1.0):
    """one line of motif_enrichment.csv; d: the MotifDef of the consensus' length, None -> empty value fields"""
    if d is None:
        return f"{conseq},{len(conseq)}" + "," * (MOTIF_HEADER.count(",") - 1) + "\n"
    fa, fb = int(fg_mass), int(control_mass)
    sa, sb = _share(fa, Nf), _share(fb, Nb)
    return (f"{conseq},{len(conseq)},{int(d.max_ham_dist)},{fa},{fb},{int(Nf)},{int(Nb)},{sa:.6e},{sb:.6e},{sa / d.p_uniform:.6g},"
            f"{sb / d.p_uniform:.6g},{log2_fold(fa, fb, Nf, Nb, pseudocount):.6g},{enrich_z(fa, fb, Nf, Nb):.6g}\n")


def write_motif_table(path, lines):
    with open(path, "w") as fh:
        fh.write(MOTIF_HEADER)
        fh.write("".join(lines))


# ---- device handle ------------------------------------------------------------------------------------------------------------
class DeviceEnrich:
    """Owns a kmap_enrich handle (csrc/enrich.hip): set_control(control DeviceCounts, revcom) -> run(foreground DeviceCounts, Nf, Nb,
    min_count) -> select(top_n) -> fetch().  The tables are borrowed: neither may be counted again before fetch()."""

    def __init__(self):
        h = _ffi.vp()
        check(_ffi.lib().kmap_enrich_create(C.byref(h)))
        self._h = h.value
        self.n = self.n_sel = self.n_eligible = 0

    def set_control(self, dc, revcom, stream=None):
        check(_ffi.lib().kmap_enrich_set_control(self._h, dc._h, int(bool(revcom)), stream))

    def run(self, dc, Nf, Nb, min_count=1, stream=None):
        check(_ffi.lib().kmap_enrich_run(self._h, dc._h, int(Nf), int(Nb), int(min_count), stream))
        self.n = dc.n_uniq

    def result_dev(self):
        """(device address of b uint64[n], of z float64[n], n)"""
        b, z, n = _ffi.vp(), _ffi.vp(), _ffi.i64(0)
        check(_ffi.lib().kmap_enrich_result_dev(self._h, C.byref(b), C.byref(z), C.byref(n)))
        return b.value, z.value, n.value

    def result(self):
        """(b uint64[n], z float64[n]) of every foreground entry, fetched"""
        b_dev, z_dev, n = self.result_dev()
        b, z = np.empty(n, np.uint64), np.empty(n, np.float64)
        if n:
            check(_ffi.lib().kmap_memcpy_d2h(ptr(b), b_dev, n * 8, None))
            check(_ffi.lib().kmap_memcpy_d2h(ptr(z), z_dev, n * 8, None))
            _ffi.sync()
        return b, z

    def select(self, top_n, stream=None):
        m, el = _ffi.i64(0), _ffi.i64(0)
        check(_ffi.lib().kmap_enrich_select(self._h, int(top_n), C.byref(m), C.byref(el), stream))
        self.n_sel, self.n_eligible = m.value, el.value
        return self.n_sel

    def fetch(self):
        """(table index int64, key uint64, a int64, b int64, z float64) of the selected rows in rank order"""
        m = self.n_sel
        idx, kh, a, b, z = np.empty(m, np.int64), np.empty(m, np.uint64), np.empty(m, np.int64), np.empty(m, np.int64), np.empty(m, np.float64)
        check(_ffi.lib().kmap_enrich_fetch(self._h, ptr(idx), ptr(kh), ptr(a), ptr(b), ptr(z)))
        return idx, kh, a, b, z

    def close(self):
        if self._h:
            _ffi.lib().kmap_enrich_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- counting and selection of one k-mer length (enrich_kmers and discover_pwms) --------------------------------------------------
def count_both(fg_seq, ctl_seq, dc_f, dc_b, k, dedupe, revcom, use_work=False):
    """reads and control counted at length k into dc_f / dc_b, both merged with revcom: (n_fg_uniq, Nf, Nb); use_work: under the
    working masks of both sets instead of the original ones"""
    n_fg = fg_seq.count(dc_f, k, dedupe, revcom, use_work=use_work)
    Nf = dc_f.total()
    ctl_seq.count(dc_b, k, dedupe, revcom, use_work=use_work)    # merged like the foreground: the total and the ball masses
    Nb = dc_b.total()
    if max(Nf, Nb) > MAX_TOTAL or min(Nf, Nb) < 0:
        raise ValueError(f"k={k}: totals {Nf} / {Nb} outside 0..2^52 - 1")
    return n_fg, Nf, Nb


def select_enriched(ctl_seq, dc_f, dc_b, en, k, dedupe, revcom, Nf, Nb, min_count, top_n, use_work=False):
    """behind count_both: the device join, the z of every foreground k-mer with a count >= min_count and the exact selection of
    the top_n best: (fetch()'s rows in rank order, n_control_uniq).  dc_b is counted again without the merge when revcom is set
    (use_work: under the control's working mask, as count_both counted it)."""
    n_ctl = ctl_seq.count(dc_b, k, dedupe, False, use_work=use_work) if revcom else dc_b.n_uniq  # B: unmerged, ascending
    en.set_control(dc_b, revcom)
    en.run(dc_f, Nf, Nb, min_count)
    en.select(top_n)
    return en.fetch(), n_ctl


# ---- the verb -----------------------------------------------------------------------------------------------------------------
def _enrich_kmers(res_dir, control_fasta_file, kmer_len=(), top_n=1000, min_count=2, pseudocount=1.0, conseq_file=None,
                  output_dir=None):
    """`kmap enrich_kmers`: config.toml + the encoded reads of a preproc result directory + a control FASTA -> enriched_kmers_k{k}.tsv
    per --kmer_len, enrichment_info.csv and (with a consensus file) motif_enrichment.csv in output_dir (default
    res_dir/kmer_enrichment).  Every argument and file is checked before the device is touched or anything is written.  Under a
    torch.distributed launch rank 0 works alone.  Returns {"kmers": {k: (idx, kh, a, b, z)}, "info": [...], "motifs": [...]}."""
    from .kmer_count import (DeviceCounts, FileNameDict, encode_fasta, gen_motif_def_dict, hash2kmer, kmer2hash, load_array_pickle,
                             load_config, rank0_only, result_paths)
    if not rank0_only():
        return None
    res, cfg_path, seq_path, border_path = result_paths(res_dir, reads=True)
    if control_fasta_file is None or not Path(control_fasta_file).is_file():
        raise ValueError(f"control FASTA file {control_fasta_file} is missing")
    kmer_lens = []
    for k in ([kmer_len] if isinstance(kmer_len, (int, np.integer)) else list(kmer_len or ())):
        if int(k) != k or not 1 <= int(k) <= 31:
            raise ValueError(f"kmer_len {k} outside 1..31")
        if int(k) not in kmer_lens:
            kmer_lens.append(int(k))
    if int(top_n) != top_n or top_n < 1:
        raise ValueError(f"top_n {top_n} < 1")
    if int(min_count) != min_count or min_count < 1:
        raise ValueError(f"min_count {min_count} < 1")
    pc = float(pseudocount)
    if not pc >= 0 or math.isinf(pc):
        raise ValueError(f"pseudocount {pseudocount} is not a finite number >= 0")
    if conseq_file is None:
        default = res / FileNameDict["final_conseq_file"]
        conseq_path = default if default.exists() else None
    else:
        conseq_path = Path(conseq_file)
        if not conseq_path.is_file():
            raise ValueError(f"consensus file {conseq_file} is missing")
    conseqs = []
    if conseq_path is not None:
        conseqs = [ln.strip() for ln in conseq_path.read_text().splitlines() if ln.strip()]
        for c in conseqs:
            if set(c) - set("ACGT"):
                raise ValueError(f"{conseq_path}: consensus {c!r} has letters other than A, C, G, T")
    if not kmer_lens and not conseqs:
        raise ValueError("enrich_kmers: nothing to do: no --kmer_len given and no consensus file found")
    cfg, revcom = load_config(cfg_path)
    dedupe = not bool(cfg["general"]["repetitive_mode"])
    motif_def = gen_motif_def_dict(cfg) if conseqs else {}
    by_len = {}
    for c in conseqs:
        if len(c) in motif_def and 1 <= len(c) <= 31:
            by_len.setdefault(len(c), []).append(c)
        else:
            print(f"enrich_kmers: consensus {c} of length {len(c)} has no row in the motif definition table: listed without values")

    from .motif_discovery import DeviceSeq
    fg_seq = DeviceSeq(load_array_pickle(seq_path), load_array_pickle(border_path))
    ctl_seq = dc_f = dc_b = en = None
    kmers, info, masses = {}, [], {}
    try:
        ctl_seq = DeviceSeq(*encode_fasta(str(control_fasta_file)))
        dc_f, dc_b, en = DeviceCounts(), DeviceCounts(), DeviceEnrich()
        for k in sorted(set(kmer_lens) | set(by_len)):          # both read sets are counted once per distinct length
            n_fg, Nf, Nb = count_both(fg_seq, ctl_seq, dc_f, dc_b, k, dedupe, revcom)
            if k in by_len:
                d = motif_def[k]
                cands = np.array([kmer2hash(c) for c in by_len[k]], np.uint64)
                ma, mb = dc_f.hamball_mass(cands, d.max_ham_dist, revcom), dc_b.hamball_mass(cands, d.max_ham_dist, revcom)
                for c, x, y in zip(by_len[k], ma, mb):
                    masses[c] = (d, int(x), int(y), Nf, Nb)
            if k in kmer_lens:
                kmers[k], n_ctl = select_enriched(ctl_seq, dc_f, dc_b, en, k, dedupe, revcom, Nf, Nb, min_count, top_n)
                info.append(dict(k=k, dedupe=dedupe, revcom=revcom, n_fg_uniq=n_fg, n_control_uniq=n_ctl, Nf=Nf, Nb=Nb,
                                 min_count=min_count, n_eligible=en.n_eligible, n_written=en.n_sel))
    finally:
        for h in (en, dc_f, dc_b, ctl_seq, fg_seq):
            if h is not None:
                h.close()

    out = res / OUTPUT_DIR if output_dir is None else Path(output_dir)
    out.mkdir(parents=True, exist_ok=True)
    by_k = {row["k"]: row for row in info}
    for k in kmer_lens:
        _, kh, a, b, z = kmers[k]
        write_kmer_table(out / KMER_FILE.format(k=k), k, kh, a, b, z, by_k[k]["Nf"], by_k[k]["Nb"], pc)
        print(f"k={k}: {by_k[k]['n_eligible']} of {by_k[k]['n_fg_uniq']} k-mers with a count >= {min_count}, {by_k[k]['n_written']} written"
              + (f", best {hash2kmer(int(kh[0]), k)} z={z[0]:.6g}" if len(kh) else ""))
    if kmer_lens:
        write_info_table(out / INFO_FILE, [by_k[k] for k in kmer_lens])
    lines = []
    if conseqs:
        for c in conseqs:
            lines.append(motif_row(c, *masses[c], pc) if c in masses else motif_row(c, None, 0, 0, 0, 0))
        write_motif_table(out / MOTIF_FILE, lines)
    print(f"enrich_kmers: {len(kmer_lens)} k-mer length{'' if len(kmer_lens) == 1 else 's'}, {len(conseqs)} consensus sequence"
          f"{'' if len(conseqs) == 1 else 's'}, {'both strands' if revcom else 'forward strand'}: {out}")
    return {"kmers": kmers, "info": info, "motifs": lines}
