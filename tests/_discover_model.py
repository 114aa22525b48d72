"""The device work of discover_pwms on the numpy models, for tests/test_discover_host.py and
tests/test_gpu_discover.py: the callables kmap_amd.discover.discover_core takes -- the batched counting step from
tests/_refine_model.py, the best-score histograms from tests/_readscore_model.py, the all-against-all match from
tests/_match_model.py -- and the seed k-mers by enrich_z, counted with numpy."""
from types import SimpleNamespace

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

from tests import _match_model as MM
from tests import _readscore_model as M
from tests._refine_model import np_counts


def counts_fn(seq, borders, revcom, calls=None):
    """DeviceSeq.library_counts on the model: (Cs, n_selected, n_minus); `calls`, a list, receives the number of matrices per call"""
    def fn(Ws, ts):
        if calls is not None:
            calls.append(len(Ws))
        got = [np_counts(seq, borders, W, t, revcom, True) for W, t in zip(Ws, ts)]
        return [g[0] for g in got], np.array([g[2] for g in got], np.int64), np.array([g[3] for g in got], np.int64)
    return fn


def hist_fn(seq, borders, cseq, cborders, revcom):
    """(Hf, fg_unscorable, Hc, control_unscorable) per matrix, as two DeviceSeq.library_histograms calls give them"""
    def fn(Ws, los, n_bins):
        out = []
        for s, b in ((seq, borders), (cseq, cborders)):
            hists, unscorable = [], []
            for W, lo, nb in zip(Ws, los, n_bins):
                score, loc, _ = M.np_read_scores(s, b, W, revcom)
                H, outside = M.np_histogram(score, loc, lo, nb)
                assert outside == 0
                hists.append(H)
                unscorable.append(int((loc < 0).sum()))
            out += [hists, unscorable]
        return tuple(out)
    return fn


def match_fn(queries, targets, revcom, min_overlap, pseudocount):
    """motif_match.match_motifs' p_best [Q, T] from the model's plain loops"""
    uq, ut = [MM.quantise(C, pseudocount) for C in queries], [MM.quantise(C, pseudocount) for C in targets]
    lib = MM.library_columns(ut, revcom)
    m_all = min(int(min_overlap), min(u.shape[1] for u in ut))
    p = np.ones((len(uq), len(ut)), np.float64)
    for q, u in enumerate(uq):
        tables = MM.null_tables(MM.null_hist(u, lib), len(lib), min(u.shape[1], m_all))
        for t, v in enumerate(ut):
            p[q, t] = MM.best_configuration(MM.configurations(u, v, tables, min_overlap, revcom))[0]
    return SimpleNamespace(p_best=p)


def kmer_table(seq, borders, k, revcom):
    """{canonical hash: the number of reads that hold the k-mer}: every valid window of every read, with revcom the smaller of the
    k-mer's hash and its reverse complement's, each k-mer once per read"""
    seq = np.asarray(seq, np.uint8)
    win = sliding_window_view(seq, k)
    valid = (win != 255).all(axis=1)
    x = np.where(win == 255, 0, win).astype(np.uint64)
    pw = (np.uint64(4) ** np.arange(k - 1, -1, -1, dtype=np.uint64))
    h = (x * pw).sum(axis=1)
    if revcom:
        h = np.minimum(h, ((np.uint64(3) - x[:, ::-1]) * pw).sum(axis=1))
    p = np.nonzero(valid)[0]
    read = np.searchsorted(np.asarray(borders)[:, 0], p, side="right") - 1
    pairs = np.unique(np.stack([read.astype(np.uint64), h[p]], axis=1), axis=0)
    keys, counts = np.unique(pairs[:, 1], return_counts=True)
    return dict(zip(keys.tolist(), counts.tolist()))


def top_seeds(seq, borders, cseq, cborders, k, revcom, min_count, n_seeds):
    """[(kmer, fg_count, control_count, z)]: the n_seeds k-mers with the largest enrich_z > 0 among those with a foreground count
    of at least min_count; ties by the hash"""
    from kmap_amd.enrichment import enrich_z
    from kmap_amd.kmer_count import hash2kmer
    fg, ctl = kmer_table(seq, borders, k, revcom), kmer_table(cseq, cborders, k, revcom)
    Nf, Nb = sum(fg.values()), sum(ctl.values())
    rows = [(h, a, ctl.get(h, 0), enrich_z(a, ctl.get(h, 0), Nf, Nb)) for h, a in fg.items() if a >= min_count]
    rows.sort(key=lambda r: (-r[3], r[0]))
    return [(hash2kmer(h, k), a, b, z) for h, a, b, z in rows if z > 0][:n_seeds]
