"""numpy / plain Python restatement of motif_cooccurrence, for tests/test_cooccurrence_host.py,
tests/test_gpu_bit_pairs.py and tests/test_gpu_cooccurrence.py: section 14's best score of every read from
tests/_readscore_model.py thresholded to presence flags, the flags packed 64 per word, the pair counts as a matrix product of the
unpacked bits, and the statistic of section 20 written pair by pair.  Never the kernels under test, never kmap_amd.cooccurrence."""
import math

import numpy as np

from tests import _readscore_model as M


def np_presence(seq, borders, Ws, ts, revcom, scored=None):
    """bool [n_mat, n_seq]: read r has a valid window under matrix m and its best score is ts[m] or more"""
    borders = np.asarray(borders, np.int64).reshape(-1, 2)
    out = np.zeros((len(Ws), len(borders)), bool)
    for m, (W, t) in enumerate(zip(Ws, ts)):
        score, loc, _ = M.np_read_scores(seq, borders, W, revcom, None if scored is None else scored[m])
        out[m] = (np.asarray(loc) >= 0) & (np.asarray(score, np.int64) >= int(t))
    return out


def np_pack(bits):
    """uint64 [n_rows, (n_bits + 63) // 64]: bit r & 63 (least significant first) of word r >> 6 = bits[row][r]; the tail is 0"""
    bits = np.asarray(bits, bool)
    n_rows, n_bits = bits.shape
    n_words = (n_bits + 63) // 64
    padded = np.zeros((n_rows, n_words * 64), np.uint8)
    padded[:, :n_bits] = bits
    weights = np.uint64(1) << np.arange(64, dtype=np.uint64)
    return (padded.reshape(n_rows, n_words, 64).astype(np.uint64) * weights).sum(axis=2, dtype=np.uint64).reshape(n_rows, n_words)


def np_unpack(planes, n_bits=None):
    """bool [n_rows, n_bits] of packed words (n_bits None: all 64 of every word)"""
    planes = np.asarray(planes, np.uint64)
    n_rows, n_words = planes.shape
    shifts = np.arange(64, dtype=np.uint64)
    bits = ((planes[:, :, None] >> shifts) & np.uint64(1)).astype(bool).reshape(n_rows, n_words * 64)
    if n_bits is not None:
        assert not bits[:, n_bits:].any()
        bits = bits[:, :n_bits]
    return bits


def np_pair_counts(bits):
    """int64 [n_rows, n_rows]: the matrix product of the bits with their transpose.  Computed in float64, where it is exact (every
    count is an integer of at most n_bits < 2^53), because numpy multiplies integer matrices a hundred times more slowly;
    tests/test_cooccurrence_host.py holds the two against each other."""
    b = np.asarray(bits, bool).astype(np.float64)
    assert b.shape[1] < 2 ** 53
    C = b @ b.T
    assert (C == np.rint(C)).all()
    return C.astype(np.int64)


def comb_moments(N, n_i, n_j):
    """(mean, variance) of the hypergeometric count by exhaustive enumeration with math.comb, as exact fractions turned to float"""
    from fractions import Fraction
    lo, hi = max(0, n_i + n_j - N), min(n_i, n_j)
    total = math.comb(N, n_j)
    pmf = {k: Fraction(math.comb(n_i, k) * math.comb(N - n_i, n_j - k), total) for k in range(lo, hi + 1)}
    assert sum(pmf.values()) == 1
    mean = sum(k * p for k, p in pmf.items())
    var = sum((k - mean) ** 2 * p for k, p in pmf.items())
    return float(mean), float(var)


def comb_log10_p_exact(n_both, n_i, n_j, N, upper):
    """log10 of min(1, twice the hypergeometric tail), the tail summed directly as a fraction of integers"""
    from fractions import Fraction
    lo, hi = max(0, n_i + n_j - N), min(n_i, n_j)
    ks = range(n_both, hi + 1) if upper else range(lo, n_both + 1)
    tail = Fraction(sum(math.comb(n_i, k) * math.comb(N - n_i, n_j - k) for k in ks), math.comb(N, n_j))
    two = 2 * tail
    if two >= 1:
        return 0.0
    return (math.log(two.numerator) - math.log(two.denominator)) / math.log(10.0)


def bh_loop(p):
    """Benjamini-Hochberg by its definition: q of the i-th smallest p of n = min over j >= i of p_(j) n / j, at most 1"""
    n = len(p)
    order = sorted(range(n), key=lambda a: (p[a], a))
    q = [0.0] * n
    for pos, a in enumerate(order):
        q[a] = min([1.0] + [p[order[b]] * n / (b + 1) for b in range(pos, n)])
    return q


def np_pair_stats(C, N, min_expected=5.0):
    """one dict per pair i < j, in row-major order: i, j, n_i, n_j, n_both, expected, variance, tested, z, direction, log10_p, q_bh,
    n_tests -- section 20's formulas, pair by pair; z, log10_p and q_bh are None for a pair that is not tested"""
    from kmap_amd.library import log10_p_of_z
    C = np.asarray(C, np.int64)
    N = int(N)
    pairs = []
    for i in range(len(C)):
        for j in range(i + 1, len(C)):
            n_i, n_j, n_both = int(C[i][i]), int(C[j][j]), int(C[i][j])
            E = float(n_i) * float(n_j) / float(N) if N else math.nan
            V = E * (1.0 - float(n_i) / float(N)) * (float(N) - float(n_j)) / (float(N) - 1.0) if N > 1 else math.nan
            tested = bool(E >= min_expected and n_i - E >= min_expected and n_j - E >= min_expected and V > 0.0)
            row = dict(i=i, j=j, n_i=n_i, n_j=n_j, n_both=n_both, expected=E, variance=V, tested=tested, z=None, direction="",
                       log10_p=None, q_bh=None)
            if tested:
                row["z"] = (n_both - E) / math.sqrt(V)
                row["direction"] = "together" if row["z"] > 0 else "apart" if row["z"] < 0 else "none"
                row["log10_p"] = min(0.0, log10_p_of_z(abs(row["z"])) + math.log10(2.0))
            pairs.append(row)
    tested = [r for r in pairs if r["tested"]]
    for r, q in zip(tested, bh_loop([10.0 ** r["log10_p"] for r in tested])):
        r["q_bh"] = q
    for r in pairs:
        r["n_tests"] = len(tested)
    return pairs


def model_order(pairs, names, top_n):
    """the written rows of np_pair_stats' pairs: tested by |z| descending, then the two names; top_n 0: all, the untested behind"""
    tested = sorted((r for r in pairs if r["tested"]), key=lambda r: (-abs(r["z"]), names[r["i"]], names[r["j"]]))
    if top_n:
        return tested[:top_n]
    return tested + sorted((r for r in pairs if not r["tested"]), key=lambda r: (names[r["i"]], names[r["j"]]))


class ModelPlanes:
    """PresencePlanes' part in motif_cooccurrence, on the host"""

    def __init__(self, bits):
        self.bits = bits
        self.n_mat, self.n_seq = bits.shape
        self.n_words = (self.n_seq + 63) // 64
        self.n_present = bits.sum(axis=1).astype(np.int64)

    def pair_counts(self):
        return np_pair_counts(self.bits)

    def fetch(self):
        return np_pack(self.bits)

    def close(self):
        pass


class ModelSeq:
    """DeviceSeq's part in motif_cooccurrence, on the host: library_presence is the model"""

    def __init__(self, seq, borders):
        self.seq, self.borders = np.asarray(seq, np.uint8), np.asarray(borders, np.int64).reshape(-1, 2)
        self.n_seq = len(self.borders)

    def library_presence(self, Ws, thresholds, revcom):
        return ModelPlanes(np_presence(self.seq, self.borders, Ws, thresholds, revcom))

    def close(self):
        pass


PLANT_A, PLANT_B = "CAATCGATAGC", "ACCTACGTA"                # the consensus of M1 and M2 of tests/golden/library/three.meme


def planted_pair_reads(seed=2001):
    """(seq, borders): 2000 reads of 60 bases, a 255 behind each; PLANT_A in 400 of them at loc 5 .. 15, PLANT_B at loc 35 .. 45 in
    300 of those 400 and in no other read (what chance adds aside)"""
    rng = np.random.default_rng(seed)
    code = {c: i for i, c in enumerate("ACGT")}
    seq = rng.integers(0, 4, 2000 * 61).astype(np.uint8)
    starts = np.arange(2000, dtype=np.int64) * 61
    seq[starts + 60] = 255
    perm = rng.permutation(2000)
    for r in perm[:400]:
        at = starts[r] + 5 + int(rng.integers(0, 11))
        seq[at:at + len(PLANT_A)] = [code[c] for c in PLANT_A]
    for r in perm[:300]:
        at = starts[r] + 35 + int(rng.integers(0, 11))
        seq[at:at + len(PLANT_B)] = [code[c] for c in PLANT_B]
    return seq, np.stack([starts, starts + 60], axis=1)
