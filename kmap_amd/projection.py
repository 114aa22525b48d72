"""project_kmers: place new k-mers on an existing 2-D k-mer map without moving its points (DESIGN.md "Projection").

A `visualize_kmers` run embeds the N sampled k-mers of `sample_kmers.pkl`; this module takes that map as fixed anchors and puts M
query k-mers on it: orientation and nearest references (csrc/project.hip, a counting select on the Hamming distances), the
query's smoothed distances as the sum of its neighbours' neighbour-sum rows, the same sigmoid / exp chain as the map's own
probabilities, a start at the probability-weighted mean of the neighbours' anchors and `n_iter` gradient steps of the map's loss
for the one free point.  Single GPU; no CPU fallback.
"""
import pickle
from pathlib import Path

import numpy as np

from . import _ffi
from ._ffi import check
from .kmer_count import FileNameDict, get_hash_dtype, load_config, rank0_only, result_paths
from .visualization import dedupe_sums_rows, sigmoid, sums_rows_from_kmers

MAX_NEIGHBOURS = 64               # csrc/project.hip PJ_MAX_NB: one lane per neighbour in the in-wave ordering
DEFAULT_BYTE_BUDGET = 1 << 30     # bytes of float32 p rows held on the device at a time
_MAX_ROWS_PER_CALL = 65535        # kmap_project_prob_dev: one grid row per query
OUTPUT_FILE = "projected_kmers.tsv"


def hd_prob_lut_projected(kmer_len, n_neighbour):
    """LUT3[s] = p of a query whose summed neighbour rows give s, s = 0 .. n_nb^3 k: the chain of `hd_prob_lut` with one more float32
    division (the query's row is the mean of n_nb smoothed rows, each sums / n_nb / n_nb), evaluated by host numpy."""
    nn = np.float32(n_neighbour)
    s = np.arange(n_neighbour ** 3 * kmer_len + 1, dtype=np.float32)
    S = ((s / nn) / nn) / nn
    T = sigmoid(S, 16.0, change_point=kmer_len / 2, scale_factor=0.2 * kmer_len - 0.2)
    return np.exp(-T / 0.5).astype("float32")


class Projection:
    """xy: float32 [2, M]; nb: int32 [M, n_nb] reference indices by (distance, index); nb_dist: uint8 [M, n_nb]; flipped: bool [M];
    kh: the oriented query hashes.  Q (uint32 [M, N]) only when asked for (keep_q); block_rows: query rows per device block."""

    def __init__(self, xy, nb, nb_dist, flipped, kh, Q=None, block_rows=0):
        self.xy, self.nb, self.nb_dist, self.flipped, self.kh, self.Q, self.block_rows = xy, nb, nb_dist, flipped, kh, Q, block_rows


def _check_neighbours(n, n_neighbour):
    if n_neighbour < 1 or n_neighbour > MAX_NEIGHBOURS:
        raise ValueError(f"project_kmers: n_neighbour={n_neighbour} outside 1..{MAX_NEIGHBOURS}")
    if n < n_neighbour:
        raise ValueError(f"project_kmers: {n} reference k-mers for n_neighbour={n_neighbour}")


def project_knn(query_kh, ref_kh, kmer_len, n_neighbour=20, revcom_mode=True):
    """Orientation and nearest references of every query -> (kh oriented, nb int32 [M, n_nb], nb_dist uint8 [M, n_nb], flipped bool [M])."""
    dt = get_hash_dtype(kmer_len)
    q = np.ascontiguousarray(query_kh, dt).copy()
    ref = np.ascontiguousarray(ref_kh, dt)
    m, n = len(q), len(ref)
    _check_neighbours(n, n_neighbour)
    nb, dist, flipped = np.zeros((m, n_neighbour), np.int32), np.zeros((m, n_neighbour), np.uint8), np.zeros(m, np.uint8)
    if m == 0:
        return q, nb, dist, flipped.astype(bool)
    fn = _ffi.lib().kmap_project_knn_u32_dev if dt == np.uint32 else _ffi.lib().kmap_project_knn_u64_dev
    bufs = [_ffi.DeviceBuffer.from_numpy(q), _ffi.DeviceBuffer.from_numpy(ref), _ffi.DeviceBuffer(nb.nbytes),
            _ffi.DeviceBuffer(dist.nbytes), _ffi.DeviceBuffer(m)]
    try:
        q_d, ref_d, nb_d, dist_d, flip_d = bufs
        check(fn(q_d.ptr, m, ref_d.ptr, n, kmer_len, 1 if revcom_mode else 0, n_neighbour, nb_d.ptr, dist_d.ptr, flip_d.ptr, None))
        _ffi.sync()
        q = q_d.to_numpy(dt, (m,))
        nb = nb_d.to_numpy(np.int32, nb.shape)
        dist = dist_d.to_numpy(np.uint8, dist.shape)
        flipped = flip_d.to_numpy(np.uint8, (m,))
    finally:
        for b in bufs:
            b.free()
    return q, nb, dist, flipped.astype(bool)


def project_rows(nb, sums_d, lds, n, lut, ref_xy, n_iter, learning_rate, rowmap_d=None, src_rows=None,
                 byte_budget=DEFAULT_BYTE_BUDGET, keep_q=False, keep_p=False):
    """Query sums, probabilities, start and descent for the neighbour table nb [M, n_nb] over the device sums rows (uint16, pitch
    lds, through rowmap_d when they are stored de-duplicated: src_rows of them).  The queries go through the device in blocks of
    `rows * n * 4 <= byte_budget` bytes of p rows (at least one row).  -> (xy float32 [2, M], Q or None, p or None, block_rows)"""
    nb = np.ascontiguousarray(nb, np.int32)
    m, n_nb = nb.shape
    ref_xy = np.ascontiguousarray(ref_xy, np.float32)
    if ref_xy.shape != (2, n):
        raise ValueError(f"project_kmers: reference coordinates of shape {ref_xy.shape}, expected (2, {n})")
    lut = np.ascontiguousarray(lut, np.float32)
    src_rows = n if src_rows is None else int(src_rows)
    rows = int(max(1, min(_MAX_ROWS_PER_CALL, int(byte_budget) // (4 * n), max(m, 1))))
    xy = np.zeros((2, m), np.float32)
    Q = np.zeros((m, n), np.uint32) if keep_q else None
    P = np.zeros((m, n), np.float32) if keep_p else None
    if m == 0:
        return xy, Q, P, rows
    ldp = (n + 63) & ~63
    lib = _ffi.lib()
    bufs = [_ffi.DeviceBuffer.from_numpy(nb), _ffi.DeviceBuffer.from_numpy(lut), _ffi.DeviceBuffer.from_numpy(ref_xy),
            _ffi.DeviceBuffer(xy.nbytes), _ffi.DeviceBuffer(rows * ldp * 4)]
    if keep_q:
        bufs.append(_ffi.DeviceBuffer(rows * ldp * 4))
    try:
        nb_d, lut_d, ref_d, xy_d, p_d = bufs[:5]
        q_d = bufs[5] if keep_q else None
        for r0 in range(0, m, rows):
            nr = min(rows, m - r0)
            check(lib.kmap_project_prob_dev(nb_d.ptr, m, n_nb, sums_d.ptr, lds, None if rowmap_d is None else rowmap_d.ptr, src_rows, n,
                                            lut_d.ptr, len(lut), r0, nr, p_d.ptr, ldp, None if q_d is None else q_d.ptr, None))
            check(lib.kmap_project_descend_dev(p_d.ptr, ldp, nb_d.ptr, m, n_nb, ref_d.ptr, n, r0, nr, int(n_iter), float(learning_rate),
                                               xy_d.ptr, None))
            _ffi.sync()                               # the next block rewrites the p rows
            if keep_q:
                Q[r0:r0 + nr] = q_d.to_numpy(np.uint32, (nr, ldp))[:, :n]
            if keep_p:
                P[r0:r0 + nr] = p_d.to_numpy(np.float32, (nr, ldp))[:, :n]
        xy = xy_d.to_numpy(np.float32, (2, m))
    finally:
        for b in bufs:
            b.free()
    return xy, Q, P, rows


def project_kmers(query_kh, ref_kh, ref_label, conseq_lens, ref_xy, kmer_len, n_neighbour=20, n_iter=100, learning_rate=0.01,
                  revcom_mode=True, ref_neighbours=None, byte_budget=DEFAULT_BYTE_BUDGET, keep_q=False):
    """Place the queries (hashes of k-mers of kmer_len bases) on the map ref_xy (float32 [2, N]) of the reference set (ref_kh,
    ref_label: the expanded order `np.repeat(samp_kh, samp_cnts)` of `kmap_from_kmers`; conseq_lens[l] = length of consensus l).
    ref_neighbours: optional (N, n_neighbour) neighbour table of the reference set replacing the selection `kmap_from_kmers` would
    make.  -> Projection."""
    dt = get_hash_dtype(kmer_len)
    ref = np.ascontiguousarray(ref_kh, dt)
    lab = np.ascontiguousarray(ref_label, np.int32)
    n = len(ref)
    if len(lab) != n:
        raise ValueError(f"project_kmers: {n} reference k-mers with {len(lab)} labels")
    if n_iter < 0:
        raise ValueError(f"project_kmers: n_iter={n_iter}")
    kh, nb, nb_dist, flipped = project_knn(query_kh, ref, kmer_len, n_neighbour, revcom_mode)
    m = len(kh)
    if m == 0:
        return Projection(np.zeros((2, 0), np.float32), nb, nb_dist, flipped, kh, np.zeros((0, n), np.uint32) if keep_q else None, 0)
    lens = [int(c) for c in conseq_lens]
    sums_d, lds = sums_rows_from_kmers(ref, lab, kmer_len, lens, n_neighbour, ref_neighbours, natural_diag=True, matrix_fallback=False)
    rowmap_d = None
    try:
        sums_d, rowmap_d, stored = dedupe_sums_rows(sums_d, n, lds, n=n)
        xy, Q, _, rows = project_rows(nb, sums_d, lds, n, hd_prob_lut_projected(kmer_len, n_neighbour), ref_xy, n_iter, learning_rate,
                                      rowmap_d, stored, byte_budget, keep_q)
    finally:
        sums_d.free()
        if rowmap_d is not None:
            rowmap_d.free()
    return Projection(xy, nb, nb_dist, flipped, kh, Q, rows)


# ---- `kmap project_kmers` ----------------------------------------------------------------------------
_BASE_CODE = np.full(256, 255, np.uint8)
_BASE_CODE[[ord(c) for c in "ACGT"]] = [0, 1, 2, 3]


def read_kmer_file(kmer_file, kmer_len):
    """One k-mer per line -> (lines as given, hashes).  Blank lines are skipped and case is folded; a line of another length or
    with a letter outside ACGT raises ValueError naming the line."""
    given, codes = [], []
    with open(kmer_file) as fh:
        for lineno, line in enumerate(fh, 1):
            text = line.strip()
            if not text:
                continue
            if len(text) != kmer_len:
                raise ValueError(f"{kmer_file}:{lineno}: {text!r} has {len(text)} bases, the map's k-mers have {kmer_len}")
            try:
                c = _BASE_CODE[np.frombuffer(text.upper().encode("ascii"), np.uint8)]
            except UnicodeEncodeError:
                c = np.array([255], np.uint8)
            if len(c) != kmer_len or (c == 255).any():
                raise ValueError(f"{kmer_file}:{lineno}: {text!r} has a letter outside ACGT")
            given.append(text)
            codes.append(c)
    kh = np.zeros(len(given), np.uint64)
    if given:
        for col in np.stack(codes).T:
            kh = (kh << np.uint64(2)) | col.astype(np.uint64)
    return given, kh.astype(get_hash_dtype(kmer_len))


def read_anchors(res_dir, n_expected, labels_expected):
    """low_dim_data.tsv -> float32 [2, N]: the 3-decimal coordinates the user plotted, row i = point i of the expanded order."""
    path = Path(res_dir) / FileNameDict["ld_data_file"]
    with open(path) as fh:
        rows = fh.read().splitlines()
    if not rows or rows[0].split("\t") != ["x", "y", "label"]:
        raise ValueError(f"{path}: header is not x<TAB>y<TAB>label")
    body = [r for r in rows[1:] if r]
    if len(body) != n_expected:
        raise ValueError(f"{path}: {len(body)} points, {FileNameDict['sample_kmer_pkl_file']} has {n_expected}")
    try:
        cols = [r.split("\t") for r in body]
        xy = np.array([[float(c[0]) for c in cols], [float(c[1]) for c in cols]], np.float32).reshape(2, len(body))
        labels = np.array([int(c[2]) for c in cols], np.int64)
    except (ValueError, IndexError) as exc:
        raise ValueError(f"{path}: malformed row ({exc})") from None
    if not np.array_equal(labels, np.asarray(labels_expected, np.int64)):
        raise ValueError(f"{path}: labels differ from {FileNameDict['sample_kmer_pkl_file']} (another run's map?)")
    return xy


def _project_kmers(res_dir, kmer_file, output_file=None, n_iter=100):
    """`kmap project_kmers`: config.toml + sample_kmers.pkl + low_dim_data.tsv + a file of k-mers -> projected_kmers.tsv.
    Under a torch.distributed launch rank 0 projects alone."""
    if not rank0_only():
        return None
    res, cfg_path = result_paths(res_dir, made_by="preproc / scan_motif")
    cfg, _ = load_config(cfg_path)
    vz = cfg["visualization"]
    with open(res / FileNameDict["sample_kmer_pkl_file"], "rb") as fh:
        samp_kh, samp_cnts, samp_label, conseq_list = pickle.load(fh)
    kmer_len = max(len(c) for c in conseq_list)
    ref_kh = np.repeat(np.asarray(samp_kh), samp_cnts)
    ref_label = np.repeat(np.asarray(samp_label), samp_cnts).astype(np.int32)
    ref_xy = read_anchors(res, int(np.sum(samp_cnts)), ref_label)
    given, query_kh = read_kmer_file(kmer_file, kmer_len)
    pr = project_kmers(query_kh, ref_kh, ref_label, [len(c) for c in conseq_list], ref_xy, kmer_len, n_neighbour=vz["n_neighbour"],
                       n_iter=n_iter, learning_rate=vz["learning_rate"], revcom_mode=cfg["kmer_count"]["revcom_mode"])
    out_path = res / OUTPUT_FILE if output_file is None else Path(output_file)
    m = len(given)
    flat = np.empty((m, 6), object)
    flat[:, 0] = given
    flat[:, 1] = pr.xy[0].tolist()
    flat[:, 2] = pr.xy[1].tolist()
    flat[:, 3] = ref_label[pr.nb[:, 0]].tolist() if m else []
    flat[:, 4] = pr.nb_dist[:, 0].tolist() if m else []
    flat[:, 5] = pr.flipped.astype(int).tolist()
    with open(out_path, "w") as fh:
        fh.write("kmer\tx\ty\tnearest_label\tmin_ham_dist\tflipped\n" + ("%s\t%3.3f\t%3.3f\t%d\t%d\t%d\n" * m) % tuple(flat.ravel().tolist()))
    print(f"{m} k-mers projected onto the map of {len(ref_kh)} points: {out_path}")
    return pr
