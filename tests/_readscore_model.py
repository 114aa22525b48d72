"""numpy restatement of evaluate_pwm's device side, for tests/test_gpu_evaluate.py: section 11's scores of
every window as tests/_refine_model.py states them, then per read the valid window with the largest score, on a tie the smallest
loc, and the histogram of those scores.  Integers only."""
import numpy as np

from tests._refine_model import encode_fasta_np, window_scores  # noqa: F401  (encode_fasta_np: re-exported for the tests)

INT32_MIN = -2 ** 31


def np_read_scores(seq, borders, W, revcom, scored=None):
    """(score int32[n_seq], loc int32[n_seq], strand uint8[n_seq]) of definition 1: a read without a valid window has
    INT32_MIN, -1, 0"""
    valid, fwd, rc = window_scores(seq, W) if scored is None else scored
    borders = np.asarray(borders, np.int64).reshape(-1, 2)
    n_seq = len(borders)
    if revcom:
        score, minus = np.maximum(fwd, rc), rc > fwd         # a tie is '+'
    else:
        score, minus = fwd, np.zeros(len(fwd), bool)
    out_score, out_loc, out_strand = np.full(n_seq, INT32_MIN, np.int32), np.full(n_seq, -1, np.int32), np.zeros(n_seq, np.uint8)
    p = np.nonzero(valid)[0]
    if len(p) == 0 or n_seq == 0:
        return out_score, out_loc, out_strand
    read = np.searchsorted(borders[:, 0], p, side="right") - 1   # the last read that starts at or before the window
    assert (read >= 0).all() and (p + np.asarray(W).shape[1] <= borders[read, 1]).all()
    loc, s = p - borders[read, 0], score[p]
    order = np.lexsort((loc, -s, read))                       # by read, then score descending, then loc ascending
    first = np.concatenate([[True], read[order][1:] != read[order][:-1]])
    keep = order[first]
    out_score[read[keep]], out_loc[read[keep]], out_strand[read[keep]] = s[keep], loc[keep], minus[p[keep]]
    return out_score, out_loc, out_strand


def np_histogram(score, loc, lo, n_bins):
    """(uint64[n_bins] histogram of the scorable reads' scores over [lo, lo + n_bins), number of scorable reads outside)"""
    s = np.asarray(score, np.int64)[np.asarray(loc) >= 0] - int(lo)
    inside = (s >= 0) & (s < n_bins)
    return np.bincount(s[inside], minlength=n_bins).astype(np.uint64), int((~inside).sum())


def score_range(W):
    """(lo, hi): every score of either strand lies in between"""
    W = np.asarray(W, np.int64)
    return int(W.min(axis=0).sum()), int(W.max(axis=0).sum())
