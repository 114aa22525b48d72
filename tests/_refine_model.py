"""numpy restatement of DESIGN.md sections 11 and 13 and the read sets the PWM tests share (tests/test_gpu_pwm.py,
tests/test_gpu_refine.py, tests/test_gpu_evaluate.py, tests/test_refine_host.py): section 11's scores and hits (sliding windows over
the uint8 array, W[x, arange(w)].sum(1), the reversed-complemented matrix for the other strand, the borders only to attribute hits to
reads), scan_pwm's four arrays, then refine_pwm's selection and the count of the selected windows' oriented bases.  Integers only."""
import functools

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view


def encode_fasta_np(path):
    """(uint8 array, borders [n_seq, 2]): A C G T (either case) = 0 1 2 3, anything else 255, a 255 behind every read"""
    lut = np.full(256, 255, np.uint8)
    for i, c in enumerate("ACGT"):
        lut[ord(c)] = lut[ord(c.lower())] = i
    reads, cur = [], None
    with open(path, "rb") as fh:
        for line in fh.read().split(b"\n"):
            if line.startswith(b">"):
                if cur is not None:
                    reads.append(b"".join(cur))
                cur = []
            elif cur is not None:
                cur.append(line.strip())
    if cur is not None:
        reads.append(b"".join(cur))
    lengths = np.array([len(r) for r in reads], np.int64)
    starts = np.concatenate([[0], np.cumsum(lengths + 1)[:-1]]).astype(np.int64)
    seq = np.full(int((lengths + 1).sum()), 255, np.uint8)
    for s, r in zip(starts, reads):
        seq[s:s + len(r)] = lut[np.frombuffer(r, np.uint8)]
    return seq, np.stack([starts, starts + lengths], axis=1)


def window_scores(seq, W):
    """(valid, fwd, rc) of every window start 0 .. n - w of the uint8 array"""
    W = np.asarray(W, np.int64)
    w = W.shape[1]
    if len(seq) < w:
        z = np.zeros(0, np.int64)
        return np.zeros(0, bool), z, z
    win = sliding_window_view(np.asarray(seq, np.uint8), w)
    valid = (win != 255).all(axis=1)
    x = np.where(win == 255, 0, win).astype(np.int64)
    cols = np.arange(w)
    fwd = W[x, cols].sum(axis=1)
    Wrc = W[::-1, ::-1]                                      # Wrc[b][j] = W[3 - b][w - 1 - j]
    rc = Wrc[x, cols].sum(axis=1)
    return valid, fwd, rc


def np_hits(seq, borders, W, t, revcom, scored=None):
    """(read, loc, array position, score, minus) of every hit of section 11, in array order"""
    valid, fwd, rc = window_scores(seq, W) if scored is None else scored
    if revcom:
        score, minus = np.maximum(fwd, rc), rc > fwd        # a tie is '+'
    else:
        score, minus = fwd, np.zeros(len(fwd), bool)
    p = np.nonzero(valid & (score >= t))[0]
    borders = np.asarray(borders, np.int64).reshape(-1, 2)
    r = np.searchsorted(borders[:, 0], p, side="right") - 1  # the last read that starts at or before the window
    assert (p + np.asarray(W).shape[1] <= borders[r, 1]).all()  # a valid window lies inside its read: the 255 behind every read
    return r, p - borders[r, 0], p, score[p], minus[p]


def np_scan(seq, borders, W, t, revcom, scored=None):
    """(hits_per_read, loc, score, strand) as section 11 defines them: what DeviceSeq.scan_pwm returns"""
    r, loc, _, score, minus = np_hits(seq, borders, W, t, revcom, scored)
    hits = np.bincount(r, minlength=len(np.asarray(borders).reshape(-1, 2))).astype(np.int32)
    return hits, loc.astype(np.int32), score.astype(np.int32), minus.astype(np.uint8)


def np_counts(seq, borders, W, t, revcom, select_best, scored=None):
    """(C' int64[4, w], n_hits, n_selected, n_minus): the selection -- every hit, or per read the largest score and on a tie the
    smallest loc -- and C'[b][j] = selected windows whose oriented base j is b"""
    w = np.asarray(W).shape[1]
    r, loc, p, score, minus = np_hits(seq, borders, W, t, revcom, scored)
    n_hits = len(p)
    if select_best and n_hits:
        order = np.lexsort((loc, -score, r))                 # by read, then score descending, then loc ascending
        first = np.concatenate([[True], r[order][1:] != r[order][:-1]])
        keep = order[first]
        p, minus = p[keep], minus[keep]
    C = np.zeros((4, w), np.int64)
    if len(p):
        win = np.asarray(seq, np.uint8)[p[:, None] + np.arange(w)[None, :]].astype(np.int64)
        oriented = np.where(minus[:, None], 3 - win[:, ::-1], win)
        for b in range(4):
            C[b] = (oriented == b).sum(axis=0)
    return C, n_hits, len(p), int(minus.sum())


def model_count_fn(seq, borders, revcom, select_best):
    return lambda W, t: np_counts(seq, borders, W, t, revcom, select_best)


# ---- read sets ------------------------------------------------------------------------------------------------------------------
def make_reads(lengths, rng, frac_invalid=0.02, last_separator=True):
    """reads of the given lengths, a 255 behind each (behind the last one only with last_separator); frac_invalid of the bases are
    255, among them first and last bases of reads"""
    lengths = np.asarray(lengths, np.int64)
    starts = np.concatenate([[0], np.cumsum(lengths + 1)[:-1]])
    borders = np.stack([starts, starts + lengths], axis=1)
    n = int((lengths + 1).sum())
    seq = rng.integers(0, 4, n).astype(np.uint8)
    seq[rng.random(n) < frac_invalid] = 255
    nonempty = np.nonzero(lengths > 0)[0]
    seq[borders[nonempty[::7], 0]] = 255                     # a read's first base
    seq[borders[nonempty[3::11], 1] - 1] = 255               # a read's last base
    seq[borders[:, 1]] = 255
    return (seq, borders) if last_separator else (seq[:-1].copy(), borders)


def asym_matrix(w, rng):
    """random weights whose first column strongly wants A and whose last strongly wants C: a wrong column reversal or a wrong
    complement changes nearly every score"""
    W = rng.integers(-300, 201, size=(4, w)).astype(np.int32)
    W[:, 0] = [200, -400, -410, -420]
    W[:, -1] = [-430, 200, -440, -450]
    return W


EDGE_STARTS = (16, 1024, 2048, 4096, 5136)      # a group edge, a wave-tile edge, the next tile, a block edge, that + a tile + a group
EDGE_SIZES = {(-1, 9): (5196, 4045), (0, 9): (5197, 4064), (1, 9): (5198, 4029),       # (shift, w): (n, valid windows)
              (-1, 31): (5240, 2839), (0, 31): (5241, 2932), (1, 31): (5242, 2839)}


@functools.lru_cache(maxsize=None)
def edge_reads(shift, w):
    """(seq, borders, W, (valid, fwd, rc), edge read indices): reads that start exactly at EDGE_STARTS + shift between short filler
    reads, two more reads behind them; a 255 behind every read but the last and no other invalid base, so n is no multiple of 16,
    the last read ends where the array ends and every window inside a read is valid.  Shared and not to be written to."""
    rng = np.random.default_rng(50 + shift)
    short, long, aim = (20, 60, 90) if w == 9 else (40, 90, 180)
    lengths, at = [], 0
    for target in (e + shift for e in EDGE_STARTS):
        while target - at > aim:
            lengths.append(int(rng.integers(short, long)))
            at += lengths[-1] + 1
        lengths.append(target - at - 1)                      # the next read starts at the target
        at = target
    lengths = np.array(lengths + [w + 28, w + 14], np.int64)
    starts = np.concatenate([[0], np.cumsum(lengths + 1)[:-1]])
    borders = np.stack([starts, starts + lengths], axis=1)
    seq = rng.integers(0, 4, int(borders[-1, 1])).astype(np.uint8)
    seq[borders[:-1, 1]] = 255
    W = asym_matrix(w, rng)
    edges = np.searchsorted(borders[:, 0], np.array(EDGE_STARTS) + shift)
    for a in (seq, borders, W):
        a.setflags(write=False)
    return seq, borders, W, window_scores(seq, W), edges


def check_edge_hits(shift, w, t_lo_hits, revcom):
    """what the read set of edge_reads must show at the all-hits threshold, on np_hits' output: these hold for the model alone"""
    seq, borders, W, scored, edges = edge_reads(shift, w)
    r, loc, p, _, minus = t_lo_hits
    n, length = len(seq), borders[:, 1] - borders[:, 0]
    assert (n, len(p)) == EDGE_SIZES[shift, w] and n % 16 != 0 and borders[-1, 1] == n
    assert borders[edges, 0].tolist() == [e + shift for e in EDGE_STARTS]
    for e in edges:
        assert ((r == e) & (loc == 0)).any()                                # the edge read's first window
        last = length[e - 1] - w                                            # the last window of the read in front of it
        assert ((r == e - 1) & (loc == last)).any() if last >= 0 else not (r == e - 1).any()
    assert length[edges[0] - 1] == 15 + shift and p[-1] == n - w            # (too short for w = 31); the array's last window
    assert 0 < minus.sum() < len(p) if revcom else not minus.any()
