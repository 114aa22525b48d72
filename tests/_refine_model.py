"""numpy restatement of one refine_pwm iteration, for tests/test_refine_host.py and tests/test_gpu_refine.py:
section 11's scores and hits as tests/test_gpu_pwm.py states them (sliding windows over the uint8 array, W[x, arange(w)].sum(1), the
reversed-complemented matrix for the other strand, the borders only to attribute hits to reads), then the selection and the count of
the selected windows' oriented bases.  Integers only."""
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
    assert (p + np.asarray(W).shape[1] <= borders[r, 1]).all()
    return r, p - borders[r, 0], p, score[p], minus[p]


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
