"""Restatement of DESIGN.md section 15 (the k-let-preserving shuffle of csrc/shuffle.hip) on the uint8 array, independent of the
library: segments, the random draws and the tree enumeration.

Two forms of the same definition: `shuffle_segment`, one segment in plain Python integers, the text of section 15 line by line; and
`shuffle_array`, all segments of an array in lock step with numpy (uint64 arithmetic wraps like the device's; the high half of a 64 x 64
bit product from 32-bit halves), which hands segments longer than LONG to the scalar form.  tests/test_shuffle_host.py holds one
against the other."""
import itertools

import numpy as np

MASK64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15
M1, M2 = 0xBF58476D1CE4E5B9, 0x94D049BB133111EB
MAX_SEGMENT = (1 << 21) - 1
LONG = 512                       # shuffle_array: longer segments go through shuffle_segment


# ---- the draws -------------------------------------------------------------------------------------------------------------------
def mix64(x):
    x = (x + GOLDEN) & MASK64
    x = ((x ^ (x >> 30)) * M1) & MASK64
    x = ((x ^ (x >> 27)) * M2) & MASK64
    return x ^ (x >> 31)


def copy_seed(seed, copy):
    return mix64((seed + copy * GOLDEN) & MASK64)


def segment_key(seed, start):
    return mix64(seed ^ mix64(start))


def draw(key, i, bound):
    """draw i of a segment, below bound: floor(h bound / 2^64) of h = mix64(key + i GOLDEN)"""
    return (mix64((key + i * GOLDEN) & MASK64) * bound) >> 64


# ---- segments and trees ------------------------------------------------------------------------------------------------------------
def segments(seq):
    """(starts, lengths) of the maximal runs of values 0..3"""
    valid = np.asarray(seq) < 4
    edge = np.diff(np.concatenate([[False], valid, [False]]).astype(np.int8))
    starts = np.nonzero(edge == 1)[0].astype(np.int64)
    return starts, np.nonzero(edge == -1)[0].astype(np.int64) - starts


def others(z):
    return [v for v in range(4) if v != z]


def is_tree(z, succ):
    """succ: {vertex: successor} for the three vertices other than z; True when every one reaches z"""
    for v in succ:
        x = v
        for _ in range(3):
            x = succ.get(x, z)
        if x != z:
            return False
    return True


def tree_table(z):
    """the assignments (t0, t1, t2) of a successor to others(z) that are arborescences rooted at z, in lexicographic order"""
    return [t for t in itertools.product(range(4), repeat=3) if is_tree(z, dict(zip(others(z), t)))]


TREES = [tree_table(z) for z in range(4)]
assert all(len(t) == 16 for t in TREES)


def last_exit_weight(m, z, v, t):
    """the weight of `v is left for t the last time`: the multiplicity of the edge, never a self-loop; a vertex the segment does
    not leave (it does not hold it) has one choice of weight 1, written as z"""
    if sum(m[v]) == 0:
        return 1 if t == z else 0
    return 0 if t == v else m[v][t]


# ---- one segment, Python integers --------------------------------------------------------------------------------------------------
def pick(counts, r):
    """the first index whose running sum exceeds r"""
    cum = 0
    for b, c in enumerate(counts):
        cum += c
        if r < cum:
            return b
    raise AssertionError("draw outside the counts")


def shuffle_segment(x, start, klet, seed):
    x = [int(b) for b in x]
    L = len(x)
    assert L <= MAX_SEGMENT
    key = segment_key(seed, start)
    if klet == 1:
        if L <= 1:
            return x
        left = [x.count(b) for b in range(4)]
        out = []
        for j in range(L):
            b = pick(left, draw(key, j, sum(left)))
            left[b] -= 1
            out.append(b)
        return out
    assert klet == 2
    if L <= 3:
        return x
    m = [[0] * 4 for _ in range(4)]
    for a, b in zip(x, x[1:]):
        m[a][b] += 1
    z = x[-1]
    vs = others(z)
    weights = []
    for t in TREES[z]:
        w = 1
        for v, tv in zip(vs, t):
            w *= last_exit_weight(m, z, v, tv)
        weights.append(w)
    assert 0 < sum(weights) < 1 << 63
    tree = TREES[z][pick(weights, draw(key, 0, sum(weights)))]
    reserved = {}
    for v, tv in zip(vs, tree):
        if sum(m[v]):
            reserved[v] = tv
            m[v][tv] -= 1
    out, a = [x[0]], x[0]
    for j in range(1, L):
        left = sum(m[a])
        if left:
            b = pick(m[a], draw(key, j, left))
            m[a][b] -= 1
        else:
            b = reserved.pop(a)
        out.append(b)
        a = b
    assert not reserved and not any(any(r) for r in m) and a == z
    return out


# ---- all segments in lock step, numpy ----------------------------------------------------------------------------------------------
def np_mix64(x):
    with np.errstate(over="ignore"):
        x = x + np.uint64(GOLDEN)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(M1)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(M2)
        return x ^ (x >> np.uint64(31))


def np_mulhi(h, b):
    """floor(h b / 2^64), uint64 arrays"""
    lo32, s = np.uint64(0xFFFFFFFF), np.uint64(32)
    h0, h1, b0, b1 = h & lo32, h >> s, b & lo32, b >> s
    u = h1 * b0 + ((h0 * b0) >> s)
    v = h0 * b1 + (u & lo32)
    return h1 * b1 + (u >> s) + (v >> s)


def np_pick(counts, r):
    """per row the first index whose running sum exceeds r (counts.shape[1] when none does)"""
    return (np.cumsum(counts, axis=1, dtype=np.uint64) <= r[:, None]).sum(axis=1)


VALID = np.zeros((4, 64), np.uint64)
for _z in range(4):
    for _t in TREES[_z]:
        VALID[_z, _t[0] << 4 | _t[1] << 2 | _t[2]] = 1


def _shuffle_bucket(seq, starts, lens, klet, seed, out):
    """segments of similar lengths, all at once"""
    ns, width = len(starts), int(lens.max())
    idx = np.minimum(starts[:, None] + np.arange(width)[None, :], len(seq) - 1)
    X = seq[idx].astype(np.int64)
    rows = np.arange(ns)
    key = np_mix64(np.full(ns, seed, np.uint64) ^ np_mix64(starts.astype(np.uint64)))
    m = np.zeros((ns, 4, 4), np.int64)                       # klet 1: row 0 only
    res = np.zeros((ns, width), np.int64)
    reserved = np.zeros((ns, 4), np.int64)
    if klet == 1:
        for j in range(width):
            on = rows[lens > j]
            np.add.at(m, (on, 0, X[on, j]), 1)
        first = 0
    else:
        for j in range(width - 1):
            on = rows[lens > j + 1]
            np.add.at(m, (on, X[on, j], X[on, j + 1]), 1)
        z = X[rows, lens - 1]
        W = np.zeros((ns, 3, 4), np.uint64)
        vk = np.stack([k + (k >= z) for k in range(3)], axis=1)              # others(z), per segment
        present = m[rows[:, None], vk].sum(axis=2) > 0
        for k in range(3):
            for t in range(4):
                W[:, k, t] = np.where(present[:, k], np.where(vk[:, k] == t, 0, m[rows, vk[:, k], t]), z == t)
        c = np.arange(64)
        weights = W[:, 0, c >> 4] * W[:, 1, (c >> 2) & 3] * W[:, 2, c & 3] * VALID[z]
        total = weights.sum(axis=1, dtype=np.uint64)
        assert (total > 0).all()
        sel = np_pick(weights, np_mulhi(np_mix64(key), total))
        for k in range(3):
            tk = (sel >> (4 - 2 * k)) & 3
            on = rows[present[:, k]]
            reserved[on, vk[on, k]] = tk[on]
            m[on, vk[on, k], tk[on]] -= 1
        res[:, 0] = X[:, 0]
        first = 1
    a = X[:, 0].copy() if klet == 2 else np.zeros(ns, np.int64)
    for j in range(first, width):
        on = rows[lens > j]
        row = m[on, a[on]]
        left = row.sum(axis=1).astype(np.uint64)
        with np.errstate(over="ignore"):
            h = np_mix64(key[on] + np.uint64(j) * np.uint64(GOLDEN))
        b = np_pick(row, np_mulhi(h, left))
        b = np.where(left == 0, reserved[on, a[on]], b)
        m[on, a[on], b] -= (left > 0).astype(np.int64)
        res[on, j] = b
        if klet == 2:
            a[on] = b
    assert not m.any()
    for i in range(ns):
        out[starts[i]:starts[i] + lens[i]] = res[i, :lens[i]]


def shuffle_array(seq, klet, seed):
    """the shuffled array: every value above 3 where it was, every segment shuffled with (seed, its start)"""
    assert klet in (1, 2)
    seq = np.ascontiguousarray(seq, np.uint8)
    out = seq.copy()
    starts, lens = segments(seq)
    moved = lens > (3 if klet == 2 else 1)
    for i in np.nonzero(moved & (lens > LONG))[0]:
        s, n = int(starts[i]), int(lens[i])
        out[s:s + n] = shuffle_segment(seq[s:s + n], s, klet, seed)
    short = moved & (lens <= LONG)
    bucket = np.ceil(np.log2(np.maximum(lens, 1))).astype(np.int64)
    for b in np.unique(bucket[short]):
        on = short & (bucket == b)
        _shuffle_bucket(seq, starts[on], lens[on], klet, int(seed), out)
    return out


# ---- what a shuffle must keep (the tests' invariants; no draw is involved) ---------------------------------------------------------
def base_counts(seq):
    """(segments, 4): the bases of every segment"""
    starts, lens = segments(seq)
    seg = np.repeat(np.arange(len(starts)), lens)
    out = np.zeros((len(starts), 4), np.int64)
    np.add.at(out, (seg, seq[seq < 4]), 1)
    return out


def pair_counts(seq):
    """(segments, 16) dinucleotide counts, and the first and the last base of every segment"""
    seq = np.asarray(seq)
    starts, lens = segments(seq)
    seg_of = np.full(len(seq), -1, np.int64)
    seg_of[seq < 4] = np.repeat(np.arange(len(starts)), lens)
    both = (seq[:-1] < 4) & (seq[1:] < 4)
    out = np.zeros((len(starts), 16), np.int64)
    np.add.at(out, (seg_of[:-1][both], seq[:-1][both].astype(np.int64) * 4 + seq[1:][both]), 1)
    return out, seq[starts], seq[starts + lens - 1]


def all_arrangements(x, klet):
    """every sequence a klet shuffle of x may return, by exhaustive search: klet 1 every arrangement of the bases, klet 2 every walk
    from the first base that uses every dinucleotide of x as often as x does; sorted tuples"""
    x = tuple(int(b) for b in x)
    found = []
    if klet == 1:
        left = [x.count(b) for b in range(4)]

        def grow(prefix):
            if len(prefix) == len(x):
                found.append(tuple(prefix))
            for b in range(4):
                if left[b]:
                    left[b] -= 1
                    grow(prefix + [b])
                    left[b] += 1
        grow([])
    else:
        m = [[0] * 4 for _ in range(4)]
        for a, b in zip(x, x[1:]):
            m[a][b] += 1

        def walk(prefix):
            if len(prefix) == len(x):
                found.append(tuple(prefix))
            for b in range(4):
                if m[prefix[-1]][b]:
                    m[prefix[-1]][b] -= 1
                    walk(prefix + [b])
                    m[prefix[-1]][b] += 1
        walk([x[0]])
    assert len(set(found)) == len(found)
    return sorted(found)
