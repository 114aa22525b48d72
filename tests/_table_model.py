"""numpy restatement of what is read off a finished (uniq, cnt) table, for tests/test_table_model_host.py (which holds it to the
oracle on any CPU) and tests/test_gpu_table_queries.py (which holds the device to it): the total, the top entries and the
Hamming-ball mass that find_motif asks for (csrc/counts_stats.hip), the labelling of sample_disp_kmer with its per-label sums,
member lists and inverse-CDF search, and the Hamming-ball extraction with its count matrix (csrc/reports.hip).  No project code;
keys are int64 (k <= 31: 62 bits), sums are Python ints.

The signedness rule of the counts: a count is the reference's int32 for k < 16 -- bit 31 makes it negative
-- and the unsigned 32-bit value for k >= 16, on every path."""
import numpy as np

M5 = 0x5555555555555555


def as_keys(uniq):
    """int64 keys of a uint32 / uint64 hash array (k <= 31: they fit)"""
    u = np.asarray(uniq)
    assert u.size == 0 or int(u.max()) < 1 << 62
    return u.astype(np.int64)


def popc2(x):
    """number of non-zero 2-bit groups of x >= 0 (< 2^62): the Hamming distance of two k-mer hashes from their XOR"""
    y = (np.asarray(x, np.int64) | (np.asarray(x, np.int64) >> 1)) & M5
    y = (y & 0x3333333333333333) + ((y >> 2) & 0x3333333333333333)
    y = (y + (y >> 4)) & 0x0F0F0F0F0F0F0F0F
    y = y + (y >> 8)
    y = y + (y >> 16)
    y = y + (y >> 32)
    return y & 0x7F


def revcom(h, k):
    """reverse complement of k-base hashes: every base b -> 3 - b, order of the bases reversed"""
    com = ((1 << (2 * k)) - 1) - np.asarray(h, np.int64)
    out = np.zeros_like(com)
    for p in range(k):
        out = (out << 2) | ((com >> (2 * p)) & 3)
    return out


def count_values(cnt, k):
    """the counts as the numbers they stand for: the low 32 bits, read as int32 for k < 16 and unsigned otherwise"""
    v = np.asarray(cnt).astype(np.int64) & 0xFFFFFFFF
    return np.where(v >= 1 << 31, v - (1 << 32), v) if k < 16 else v


def isum(v):
    """exact sum of int64 values below 2^32 in size (fewer than 2^31 of them: it stays inside int64) as a Python int"""
    assert len(v) < 1 << 31 and (len(v) == 0 or int(np.abs(v).max()) < 1 << 32)
    return int(np.sum(v, dtype=np.int64))


def table_total(cnt, k):
    return isum(count_values(cnt, k))


def table_topk(cnt, k, top_k):
    """(indices, counts) of the top_k largest positive counts, largest first, equal counts by the lowest index"""
    v = count_values(cnt, k)
    pos = np.flatnonzero(v > 0)
    order = pos[np.lexsort((pos, -v[pos]))][:top_k]
    return order, v[order]


def ball_dist(u, c, k, revcom_mode):
    """(distance of every key to the k-base consensus c -- with revcom_mode to the nearer of c and rc(c) --, rc strictly nearer)"""
    m = (1 << (2 * k)) - 1
    d = popc2((u ^ int(c)) & m)
    if not revcom_mode:
        return d, np.zeros(len(u), bool)
    d2 = popc2((u ^ int(revcom(int(c), k))) & m)
    return np.minimum(d, d2), d2 < d


def ball_mass(uniq, cnt, k, cands, r, revcom_mode):
    """per candidate: the sum of the counts of the keys within distance r (Python ints)"""
    u, v = as_keys(uniq), count_values(cnt, k)
    return [isum(v[ball_dist(u, c, k, revcom_mode)[0] <= r]) for c in cands]


def label_table(uniq, k, cons, lens, radii, radius_k, revcom_mode):
    """(labels int64[n], re-oriented keys int64[n]).  Distance of a key to consensus c: its first lens[c] bases against cons[c], or
    -- revcom_mode -- its last lens[c] bases against rc(cons[c]) if that is strictly smaller; a distance above radii[c] counts as
    k; label = the first consensus at the minimum, or len(cons) (noise) when the minimum exceeds radius_k; the members that matched
    through the reverse complement are reverse-complemented."""
    u = as_keys(uniq)
    n, nc = len(u), len(cons)
    dist, through_rc = np.empty((nc, n), np.int64), np.zeros((nc, n), bool)
    for c in range(nc):
        cl, m = int(lens[c]), (1 << (2 * int(lens[c]))) - 1
        d = popc2(((u >> (2 * (k - cl))) ^ int(cons[c])) & m)
        if revcom_mode:
            d2 = popc2((u ^ int(revcom(int(cons[c]) & m, cl))) & m)
            through_rc[c] = d2 < d
            d = np.minimum(d, d2)
        dist[c] = np.where(d > int(radii[c]), k, d)
    lab = np.argmin(dist, axis=0)                                   # first minimum
    at = np.arange(n)
    lab = np.where(dist[lab, at] > radius_k, nc, lab)
    flip = (lab < nc) & through_rc[np.minimum(lab, nc - 1), at]
    return lab.astype(np.int64), np.where(flip, revcom(u, k), u)


def label_sums(labels, cnt, k, n_labels):
    """(sum of the counts, number of members) per label: lists of Python ints"""
    v = count_values(cnt, k)
    return ([isum(v[labels == c]) for c in range(n_labels)],
            [int(np.count_nonzero(labels == c)) for c in range(n_labels)])


def members_of(labels, c):
    return np.flatnonzero(np.asarray(labels) == c).astype(np.int64)


def cdf_hits(weights, targets):
    """index of the entry whose cumulative-weight interval [cdf[i-1], cdf[i]) holds each target; len(weights) past the total.
    The weights are unsigned 32-bit values; their sum stays below 2^63."""
    w = np.asarray(weights).astype(np.int64) & 0xFFFFFFFF
    assert isum(w) < 1 << 63
    return np.searchsorted(np.cumsum(w.astype(np.uint64), dtype=np.uint64), np.asarray(targets).astype(np.uint64), side="right")


def ball_members(uniq, cnt, k, cons, r, revcom_mode):
    """(re-oriented keys, counts as count_values) of the keys inside the ball, in table order: the labelling with one k-base
    consensus whose radius is also the radius of k"""
    lab, u2 = label_table(uniq, k, [cons], [k], [r], r, revcom_mode)
    return u2[lab == 0], count_values(cnt, k)[lab == 0]


def cnt_mat(uniq, cnt, k):
    """4 x k Python-int matrix: the summed counts of the keys with base b at position p (first base most significant)"""
    u, v = as_keys(uniq), count_values(cnt, k)
    return [[isum(v[((u >> (2 * (k - 1 - p))) & 3) == b]) for p in range(k)] for b in range(4)]
