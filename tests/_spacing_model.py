"""numpy restatement of motif_spacing's device side, for tests/test_gpu_spacing.py and
tests/test_spacing_host.py: section 14's best window of every read under the primary matrix from tests/_readscore_model.py, section
11's hits of every other matrix from tests/_refine_model.py, then per primary read the best hit that does not overlap the primary
window, and the pair reads reduced to the gap histogram S[quadrant][gap] and the room histogram R[u][d].  Integers only."""
import numpy as np

from tests import _readscore_model as M
from tests._refine_model import np_hits

PLANTED_SEED = 1900
PRIMARY, FIXED, UNIFORM = "CAATCGATAGC", "ACCTACGTA", "GGTCAAGTTC"
FIXED_GAP = 3                                                # FIXED lies this many bases downstream of PRIMARY, on its strand


def reduce_pairs(read, loc, score, minus, ploc, pstrand, borders, w, wP, G):
    """(S int64[4, G + 1], R int64[G + 2, G + 2], n_pair, n_far) of definitions 2 - 4 from the hits (read, loc, score, minus) of one
    matrix of width w, in any order: those in reads without a primary site (ploc < 0) or overlapping it are dropped, of the rest the
    best per read -- the largest score, then the smallest loc -- is the secondary site.  What the model and the second witness,
    DeviceSeq.scan_pwm's hit list, are reduced with."""
    borders = np.asarray(borders, np.int64).reshape(-1, 2)
    read, loc, score = np.asarray(read, np.int64), np.asarray(loc, np.int64), np.asarray(score, np.int64)
    minus, ploc, pstrand = np.asarray(minus).astype(bool), np.asarray(ploc, np.int64), np.asarray(pstrand).astype(bool)
    S, R = np.zeros((4, G + 1), np.int64), np.zeros((G + 2, G + 2), np.int64)
    p = ploc[read]
    keep = (p >= 0) & ((loc + w <= p) | (loc >= p + wP))
    read, loc, score, minus, p = read[keep], loc[keep], score[keep], minus[keep], p[keep]
    if len(read) == 0:
        return S, R, 0, 0
    order = np.lexsort((loc, -score, read))                  # by read, then score descending, then loc ascending
    first = np.concatenate([[True], read[order][1:] != read[order][:-1]])
    best = order[first]
    read, loc, minus, p = read[best], loc[best], minus[best], p[best]
    L, sP = borders[read, 1] - borders[read, 0], pstrand[read]
    assert (loc + w <= L).all() and (p + wP <= L).all()
    left = loc + w <= p
    g = np.where(left, p - loc - w, loc - p - wP)
    assert (g >= 0).all()
    near = g <= G
    left_room = np.minimum(np.maximum(p - w + 1, 0), G + 1)
    right_room = np.minimum(np.maximum(L - p - wP - w + 1, 0), G + 1)
    assert (g[near] < np.where(left, left_room, right_room)[near]).all()
    downstream = ~left ^ sP                                  # right of a '+' primary, left of a '-' one
    quadrant = 2 * downstream.astype(np.int64) + (minus != sP)
    u, d = np.where(sP, right_room, left_room), np.where(sP, left_room, right_room)
    np.add.at(S, (quadrant[near], g[near]), 1)
    np.add.at(R, (u[near], d[near]), 1)
    return S, R, len(read), int((~near).sum())


def primary_sites(score, loc, strand, tP):
    """(ploc int64[n_seq]: the primary site's loc or -1, strand as bool, n_primary) from per-read best (score, loc, strand)"""
    score, loc = np.asarray(score, np.int64), np.asarray(loc, np.int64)
    prim = (loc >= 0) & (score >= int(tP))
    return np.where(prim, loc, -1), np.asarray(strand).astype(bool), int(prim.sum())


def reduce_library(seq, borders, ploc, pstrand, n_primary, wP, Ws, ts, revcom, G, scored=None):
    """reduce_pairs for every matrix of a library, stacked as DeviceSeq.library_spacing returns them"""
    rows = []
    for i, (W, t) in enumerate(zip(Ws, ts)):
        read, loc, _, score, minus = np_hits(seq, borders, W, t, revcom, None if scored is None else scored[i])
        rows.append(reduce_pairs(read, loc, score, minus, ploc, pstrand, borders, np.asarray(W).shape[1], wP, G))
    S = np.array([r[0] for r in rows], np.int64).reshape(len(rows), 4, G + 1)
    R = np.array([r[1] for r in rows], np.int64).reshape(len(rows), G + 2, G + 2)
    return S, R, n_primary, np.array([r[2] for r in rows], np.int64), np.array([r[3] for r in rows], np.int64)


def np_library_spacing(seq, borders, W_P, tP, Ws, ts, revcom, G, scored_P=None, scored=None):
    """DeviceSeq.library_spacing on the host: (S [n_mat, 4, G + 1], R [n_mat, G + 2, G + 2], n_primary, n_pair [n_mat], n_far
    [n_mat]); scored_P / scored[i]: window_scores of the primary / of matrix i, when the caller has them"""
    borders = np.asarray(borders, np.int64).reshape(-1, 2)
    primary = primary_sites(*M.np_read_scores(seq, borders, W_P, revcom, scored_P), tP)
    return reduce_library(seq, borders, *primary, np.asarray(W_P).shape[1], Ws, ts, revcom, G, scored)


# ---- the planted reads of the verb's tests ------------------------------------------------------------------------------------------
_CODE = {c: i for i, c in enumerate("ACGT")}


def _codes(word, minus):
    x = np.array([_CODE[c] for c in word], np.uint8)
    return (3 - x)[::-1] if minus else x


def planted_reads(seed=PLANTED_SEED):
    """(seq, borders): 600 reads of 100 random bases, a 255 behind each.  PRIMARY is planted in 400 of them at loc 40 .. 48 on a
    random strand.  In 200 of those FIXED lies FIXED_GAP bases downstream of it on its strand -- left of a '-' primary and
    reverse-complemented; in the other 200 UNIFORM lies at a window drawn uniformly from those that do not overlap the primary, on
    a random strand."""
    rng = np.random.default_rng(seed)
    seq = rng.integers(0, 4, 600 * 101).astype(np.uint8)
    starts = np.arange(600, dtype=np.int64) * 101
    seq[starts + 100] = 255
    wP, wF, wU = len(PRIMARY), len(FIXED), len(UNIFORM)
    perm = rng.permutation(600)
    for n, r in enumerate(perm[:400]):
        p, minus = 40 + int(rng.integers(0, 9)), bool(rng.integers(0, 2))
        seq[starts[r] + p:starts[r] + p + wP] = _codes(PRIMARY, minus)
        if n < 200:
            at = p - FIXED_GAP - wF if minus else p + wP + FIXED_GAP
            seq[starts[r] + at:starts[r] + at + wF] = _codes(FIXED, minus)
        else:
            free = [x for x in range(100 - wU + 1) if x + wU <= p or x >= p + wP]
            at = free[int(rng.integers(0, len(free)))]
            seq[starts[r] + at:starts[r] + at + wU] = _codes(UNIFORM, bool(rng.integers(0, 2)))
    return seq, np.stack([starts, starts + 100], axis=1)


def consensus_counts(word):
    """44 of 50 sites on the consensus base, 2 on each other base"""
    C = np.full((4, len(word)), 2, np.int64)
    C[[_CODE[c] for c in word], np.arange(len(word))] = 44
    return C


def write_planted(tmp_path, seed=PLANTED_SEED):
    """(res_dir, primary CSV, [library CSVs], seq, borders): planted_reads as a preproc result directory with the default config,
    and the three motifs as count-matrix CSV files under tmp_path (named by their consensus)"""
    import pickle
    from pathlib import Path

    import kmap_amd.kmer_count as K
    seq, borders = planted_reads(seed)
    res = tmp_path / "res"
    res.mkdir()
    (res / K.FileNameDict["config_file"]).write_text((Path(K.__file__).parent / "default_config.toml").read_text())
    with open(res / K.FileNameDict["processed_fasta_file"], "wb") as fh:
        pickle.dump(seq, fh)
    with open(res / K.FileNameDict["processed_fasta_seqboarder_file"], "wb") as fh:
        pickle.dump(borders, fh)
    lib = tmp_path / "motifs"
    lib.mkdir()
    files = []
    for word in (PRIMARY, FIXED, UNIFORM):
        files.append(lib / f"{word}.csv")
        files[-1].write_text("".join(",".join(str(int(x)) for x in row) + "\n" for row in consensus_counts(word)))
    return res, files[0], files, seq, borders


class ModelScores:
    """ReadScores' part in motif_spacing, on the host"""

    def __init__(self, score, loc, strand):
        self.score, self.loc, self.strand, self.closed = score, loc, strand, False

    def close(self):
        self.closed = True


class ModelSeq:
    """DeviceSeq's part in motif_spacing, on the host: read_scores and library_spacing are the model"""
    calls = []

    def __init__(self, seq, borders):
        self.seq, self.borders = np.asarray(seq, np.uint8), np.asarray(borders, np.int64).reshape(-1, 2)
        self.n_seq = len(self.borders)

    def read_scores(self, W, revcom):
        ModelSeq.calls.append(("read_scores", np.asarray(W).shape[1], bool(revcom)))
        return ModelScores(*M.np_read_scores(self.seq, self.borders, W, revcom))

    def library_spacing(self, primary, prim_width, prim_threshold, Ws, thresholds, revcom, max_gap=150):
        ModelSeq.calls.append(("library_spacing", prim_width, len(Ws), bool(revcom), max_gap))
        assert isinstance(primary, ModelScores) and not primary.closed
        primary_reads = primary_sites(primary.score, primary.loc, primary.strand, prim_threshold)
        return reduce_library(self.seq, self.borders, *primary_reads, prim_width, Ws, thresholds, revcom, max_gap)

    def close(self):
        pass
