"""numpy restatement of motif_centrality's device side, for tests/test_gpu_sites.py and
tests/test_centrality_host.py: section 14's best window of every read from tests/_readscore_model.py, then over the site reads
(best score >= t) the histogram of the doubled centre offsets d = 2 loc + w - L and the histogram of the lengths L.  Integers only."""
import numpy as np

from tests import _readscore_model as M


PLANTED_SEED = 1800
CENTRED, UNIFORM = "CAATCGATAGC", "ACCTACGTA"               # the consensus of M1 and M2 of tests/golden/library/three.meme


def planted_reads(seed=PLANTED_SEED):
    """(seq, borders, control_seq, control_borders): 600 reads of 100 bases, a 255 behind each.  CENTRED is planted in 300 of them
    within 3 bases of the centre (loc 44 or 45 is central: d = 2 loc + 11 - 100), UNIFORM in the other 300 at a loc drawn uniformly
    from its 92 windows; the control is 600 random reads of the same length."""
    rng = np.random.default_rng(seed)
    code = {c: i for i, c in enumerate("ACGT")}
    sets = []
    for planted in (True, False):
        seq = rng.integers(0, 4, 600 * 101).astype(np.uint8)
        starts = np.arange(600, dtype=np.int64) * 101
        seq[starts + 100] = 255
        if planted:
            perm = rng.permutation(600)
            for r in perm[:300]:
                at = starts[r] + 42 + int(rng.integers(0, 6))                   # loc 42 .. 47: d = 2 loc - 89 = -5 .. 5
                seq[at:at + len(CENTRED)] = [code[c] for c in CENTRED]
            for r in perm[300:]:                                                # the other 300 reads
                at = starts[r] + int(rng.integers(0, 100 - len(UNIFORM) + 1))
                seq[at:at + len(UNIFORM)] = [code[c] for c in UNIFORM]
        sets += [seq, np.stack([starts, starts + 100], axis=1)]
    return tuple(sets)


def write_planted(tmp_path, seed=PLANTED_SEED):
    """(res_dir, control FASTA, seq, borders, control_seq, control_borders): planted_reads as a preproc result directory with the
    default config and a control FASTA file under tmp_path"""
    import pickle
    from pathlib import Path

    import kmap_amd.kmer_count as K
    seq, borders, cseq, cborders = planted_reads(seed)
    res = tmp_path / "res"
    res.mkdir()
    (res / K.FileNameDict["config_file"]).write_text((Path(K.__file__).parent / "default_config.toml").read_text())
    with open(res / K.FileNameDict["processed_fasta_file"], "wb") as fh:
        pickle.dump(seq, fh)
    with open(res / K.FileNameDict["processed_fasta_seqboarder_file"], "wb") as fh:
        pickle.dump(borders, fh)
    ctl = tmp_path / "control.fa"
    with open(ctl, "w") as fh:
        for i, (s, e) in enumerate(cborders.tolist()):
            fh.write(f">c{i}\n" + "".join("ACGT"[b] for b in cseq[s:e]) + "\n")
    return res, ctl, seq, borders, cseq, cborders


class ModelSeq:
    """DeviceSeq's part in motif_centrality, on the host: library_sites is the model"""
    calls = []

    def __init__(self, seq, borders):
        self.seq, self.borders = np.asarray(seq, np.uint8), np.asarray(borders, np.int64).reshape(-1, 2)
        self.n_seq = len(self.borders)

    def library_sites(self, Ws, thresholds, revcom, max_len=None):
        ModelSeq.calls.append((len(Ws), bool(revcom), max_len))
        return np_library_sites(self.seq, self.borders, Ws, thresholds, revcom, max_len)

    def close(self):
        pass


def sites_from_scores(score, loc, borders, w, t, max_len):
    """(D int64[2 max_len + 1], Hlen int64[max_len + 1], n_sites, n_too_long) from per-read best (score, loc): what the model and
    the second witness, DeviceSeq.read_scores(...).fetch(), are reduced with"""
    borders = np.asarray(borders, np.int64).reshape(-1, 2)
    score, loc = np.asarray(score, np.int64), np.asarray(loc, np.int64)
    L = borders[:, 1] - borders[:, 0]
    site = (loc >= 0) & (score >= int(t))
    assert (L[site] >= w).all() and (loc[site] + w <= L[site]).all()
    inside = site & (L <= max_len)
    d = 2 * loc[inside] + w - L[inside]
    assert (np.abs(d) <= L[inside] - w).all() and ((d - (L[inside] - w)) % 2 == 0).all()
    D = np.bincount(d + max_len, minlength=2 * max_len + 1).astype(np.int64)
    Hlen = np.bincount(L[inside], minlength=max_len + 1).astype(np.int64)
    return D, Hlen, int(inside.sum()), int((site & ~inside).sum())


def np_sites(seq, borders, W, t, revcom, max_len, scored=None):
    score, loc, _ = M.np_read_scores(seq, borders, W, revcom, scored)
    return sites_from_scores(score, loc, borders, np.asarray(W).shape[1], t, max_len)


def np_library_sites(seq, borders, Ws, thresholds, revcom, max_len=None, scored=None):
    """DeviceSeq.library_sites on the host: (D [n_mat, 2 max_len + 1], Hlen [n_mat, max_len + 1], n_sites, n_too_long)"""
    borders = np.asarray(borders, np.int64).reshape(-1, 2)
    if max_len is None:
        max_len = int((borders[:, 1] - borders[:, 0]).max()) if len(borders) else 0
    rows = [np_sites(seq, borders, W, t, revcom, max_len, None if scored is None else scored[i])
            for i, (W, t) in enumerate(zip(Ws, thresholds))]
    D = np.array([r[0] for r in rows], np.int64).reshape(len(rows), 2 * max_len + 1)
    Hlen = np.array([r[1] for r in rows], np.int64).reshape(len(rows), max_len + 1)
    return D, Hlen, np.array([r[2] for r in rows], np.int64), np.array([r[3] for r in rows], np.int64)
