"""numpy restatement of DESIGN.md section 22 for tests/test_erase_host.py and tests/test_gpu_erase.py: the erasure of the sites of a list
of weight matrices, built from tests/_refine_model.py's np_hits (section 11's hits), and the device work of discover_pwms
--erase_rounds on the models (the callables kmap_amd.discover.discover_rounds takes).  Integers only; it is the only witness."""
import numpy as np

from tests import _discover_model as DM
from tests._refine_model import np_counts, np_hits


def np_erase(seq, borders, Ws, ts, revcom, out=None):
    """(erased uint8 array, n_hits int64[n_mat], n_covered int64[n_mat], n_new): every matrix's hits on `seq` as it is given (255 =
    invalid), cover_m = the positions inside a hit of m, and `out` (default: seq; an array with more 255s for a run that evaluates
    on one mask and writes another) with 255 at the union of the covers; n_new = the positions of the union that were not 255 in
    `out`"""
    seq = np.asarray(seq, np.uint8)
    union = np.zeros(len(seq), bool)
    n_hits, n_cov = np.zeros(len(Ws), np.int64), np.zeros(len(Ws), np.int64)
    for m, (W, t) in enumerate(zip(Ws, ts)):
        w = np.asarray(W).shape[1]
        p = np_hits(seq, borders, W, t, revcom)[2]
        cover = np.zeros(len(seq), bool)
        for j in range(w):                                   # a hit at p covers p .. p + w - 1
            cover[p + j] = True
        n_hits[m], n_cov[m] = len(p), int(cover.sum())
        union |= cover
    erased = np.array(seq if out is None else out, np.uint8)
    n_new = int((union & (erased != 255)).sum())
    erased[union] = 255
    return erased, n_hits, n_cov, n_new


def mask_words(seq):
    """the invalid mask of a uint8 array as the packed layout holds it: uint16 per group of 16 positions, position 0 in bit 15, the
    positions behind the array invalid"""
    seq = np.asarray(seq, np.uint8)
    n_data = (len(seq) + 15) // 16
    bad = np.ones(n_data * 16, bool)
    bad[:len(seq)] = seq == 255
    return (bad.reshape(n_data, 16) * (1 << np.arange(15, -1, -1))).sum(axis=1).astype(np.uint16)


def rc_hash(h, k):
    """the hash of the reverse complement of the k-mer with hash h (base 4, the first base the most significant digit)"""
    digits = [(h >> (2 * j)) & 3 for j in range(k)]          # the last base first
    out = 0
    for d in digits:
        out = out * 4 + (3 - d)
    return out


def merged_kmer_table(seq, borders, k):
    """{lower hash: count} as the counting kernels merge the strands (tests/test_gpu_enrich.py's restate_counts): every k-mer once
    per read, then count[min(x, rc x)] = count[x] + count[rc x] -- a palindrome counts twice, and so does a read that holds a
    k-mer and its reverse complement.  tests/_discover_model.py's kmer_table takes the lower hash BEFORE the reads are counted, so
    it differs from the device at exactly those k-mers; without the merge the two are the same."""
    plain = DM.kmer_table(seq, borders, k, False)
    merged = {}
    for x, c in plain.items():
        rx = rc_hash(x, k)
        merged[min(x, rx)] = c + plain.get(rx, 0)
    return merged


def top_seeds_merged(seq, borders, cseq, cborders, k, min_count, n_seeds):
    """tests/_discover_model.py's top_seeds on merged_kmer_table: the seeds as the device's counts give them on both strands"""
    from kmap_amd.enrichment import enrich_z
    from kmap_amd.kmer_count import hash2kmer
    fg, ctl = merged_kmer_table(seq, borders, k), merged_kmer_table(cseq, cborders, k)
    Nf, Nb = sum(fg.values()), sum(ctl.values())
    rows = [(h, a, ctl.get(h, 0), enrich_z(a, ctl.get(h, 0), Nf, Nb)) for h, a in fg.items() if a >= min_count]
    rows.sort(key=lambda r: (-r[3], r[0]))
    return [(hash2kmer(h, k), a, b, z) for h, a, b, z in rows if z > 0][:n_seeds]


class ModelReads:
    """reads and control with their working copies: what two DeviceSeq hold for discover_rounds.  merged: the seeds come from
    merged_kmer_table (the device's strand merge) instead of tests/_discover_model.py's kmer_table"""

    def __init__(self, seq, borders, cseq, cborders, revcom, merged=False):
        self.seq, self.borders, self.cseq, self.cborders, self.revcom, self.merged = seq, borders, cseq, cborders, revcom, merged
        self.work, self.cwork = np.array(seq, np.uint8), np.array(cseq, np.uint8)
        self.seed_calls, self.erase_calls = [], []

    def seeds_fn(self, k, min_count, n_seeds):
        def fn(r):
            self.seed_calls.append(r)
            a, b = (self.seq, self.cseq) if r == 1 else (self.work, self.cwork)
            if self.merged:
                return top_seeds_merged(a, self.borders, b, self.cborders, k, min_count, n_seeds)
            return DM.top_seeds(a, self.borders, b, self.cborders, k, self.revcom, min_count, n_seeds)
        return fn

    def counts_fn(self, Ws, ts, use_work=False):
        s = self.work if use_work else self.seq
        got = [np_counts(s, self.borders, W, t, self.revcom, True) for W, t in zip(Ws, ts)]
        return [g[0] for g in got], np.array([g[2] for g in got], np.int64), np.array([g[3] for g in got], np.int64)

    def erase_fn(self, Ws, ts):
        self.erase_calls.append(len(Ws))
        self.work, fh, fc, f_new = np_erase(self.work, self.borders, Ws, ts, self.revcom)
        self.cwork, ch, cc, c_new = np_erase(self.cwork, self.cborders, Ws, ts, self.revcom)
        return fh, fc, f_new, ch, cc, c_new

    def hist_fn(self):
        return DM.hist_fn(self.seq, self.borders, self.cseq, self.cborders, self.revcom)


def planted_reads(seed=2201, n_reads=400, length=40, words=("ACCTACGTAC", "TTGCATCAGG"), shares=(0.5, 0.2), p_sub=0.3):
    """the reads of the issue's experiment: n_reads of `length` bases, a 255 behind each; words[0] planted in the first shares[0] of
    the reads, words[1] in the next shares[1], every copy with one random substitution with probability p_sub"""
    rng = np.random.default_rng(seed)
    starts = np.arange(n_reads, dtype=np.int64) * (length + 1)
    seq = rng.integers(0, 4, n_reads * (length + 1)).astype(np.uint8)
    seq[starts + length] = 255
    first = 0
    for word, share in zip(words, shares):
        code = ["ACGT".index(c) for c in word]
        for r in range(first, first + int(round(share * n_reads))):
            wd = list(code)
            if rng.random() < p_sub:
                wd[int(rng.integers(0, len(wd)))] = int(rng.integers(0, 4))
            at = starts[r] + int(rng.integers(0, length - len(wd) + 1))
            seq[at:at + len(wd)] = wd
        first += int(round(share * n_reads))
    return seq, np.stack([starts, starts + length], axis=1)
