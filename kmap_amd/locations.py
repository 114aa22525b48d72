"""Motif hits back onto the genome, and the co-occurrence of two user motifs: `extract_motif_locations` (reference util.py:292-352)
and `check_motif_co_occurence` (reference motif_discovery.py:111-177).

extract_motif_locations: every hit p of consensus i in the row of read `seq_ind` becomes the window [bed.start + p, bed.start + p +
len(conseq)] of BED row `seq_ind` (by position, like iloc); the windows of one (row, consensus) are merged in start order -- a new
interval starts only when prev_end < start, so touching windows merge -- and written as `chrom, start, end, motif_{i}_{seq_ind}, 0,
strand` to `motif_{i}_{conseq}_locations.bed`, sorted like Python sorts those lists (chrom, start, end, then the name AS A STRING).
The reference walks the rows with pandas iterrows; here the occurrence CSV and the BED file are parsed by native host threads
(csrc/host_bed.hip), merging, keying and sorting of all consensuses run as one GPU pipeline (csrc/locations.hip), and the lines are
formatted by native host threads.  Where the reference crashes: a 3-column BED gets strand "."; a column
without a comma (pandas parses it as numbers) is read as single positions; a seq_ind outside the BED file or more consensuses than
occurrence columns raise ValueError before any file is written.  There is no CPU fallback.
"""
import ctypes as C
from pathlib import Path

import numpy as np

from . import _ffi
from ._ffi import check, ptr
from .reports import Occurrence


def read_occurrence(path) -> Occurrence:
    """Occurrence.from_file's result, parsed by native host threads (csrc/host_bed.hip)"""
    h, n_rows, n_cols = _ffi.vp(), _ffi.i64(0), _ffi.i32(0)
    check(_ffi.lib().kmap_occ_open(str(path).encode(), C.byref(h), C.byref(n_rows), C.byref(n_cols)))
    try:
        n, nc = n_rows.value, n_cols.value
        n_pos = np.zeros(max(nc, 1), np.int64)
        check(_ffi.lib().kmap_occ_sizes(h, ptr(n_pos)))
        seq_ind, seq_len = np.empty(n, np.int64), np.empty(n, np.int64)
        hits = [np.empty(n, np.int32) for _ in range(nc)]
        pos = [np.empty(int(n_pos[c]), np.int32) for c in range(nc)]
        hp = (C.c_void_p * max(nc, 1))(*[a.ctypes.data for a in hits])
        pp = (C.c_void_p * max(nc, 1))(*[a.ctypes.data for a in pos])
        check(_ffi.lib().kmap_occ_read(h, ptr(seq_ind), ptr(seq_len), hp, pp))
    finally:
        _ffi.lib().kmap_occ_close(h)
    return Occurrence(hits, pos, seq_len, seq_ind)


class BedFile:
    """A BED file parsed by native host threads: `start` (int64 per row), `chrom_rank` (int32 per row, the chrom's place in the output
    order), `chroms` (names by rank, as written), `int_chrom` (every chrom an integer literal), `n_cols` (3 or 6)."""

    def __init__(self, path):
        h, n, nc, nchr, ic = _ffi.vp(), _ffi.i64(0), _ffi.i32(0), _ffi.i32(0), _ffi.i32(0)
        check(_ffi.lib().kmap_bed_open(str(path).encode(), C.byref(h), C.byref(n), C.byref(nc), C.byref(nchr), C.byref(ic)))
        self._h = h.value
        self.n_rows, self.n_cols, self.n_chrom, self.int_chrom = n.value, nc.value, nchr.value, bool(ic.value)
        self.start, self.chrom_rank = np.empty(self.n_rows, np.int64), np.empty(self.n_rows, np.int32)
        check(_ffi.lib().kmap_bed_rows(self._h, ptr(self.start), ptr(self.chrom_rank)))

    @property
    def chroms(self):
        out = []
        for r in range(self.n_chrom):
            cap = 256
            while True:
                buf = C.create_string_buffer(cap)
                rc = _ffi.lib().kmap_bed_chrom(self._h, r, buf, cap)
                if rc >= 0:
                    break
                cap *= 16
                if cap > 1 << 24:
                    check(rc)
            out.append(buf.raw[:rc].decode(errors="surrogateescape"))
        return out

    def write_locations(self, path, cons_index, row, start, end):
        """the BED output of one consensus (native threaded formatter); returns the bytes written"""
        row, start, end = (np.ascontiguousarray(a, np.int64) for a in (row, start, end))
        assert len(row) == len(start) == len(end)
        nb = _ffi.i64(0)
        check(_ffi.lib().kmap_bed_write_locations(self._h, str(path).encode(), int(cons_index), len(row), ptr(row), ptr(start), ptr(end),
                                                  C.byref(nb)))
        return nb.value

    def close(self):
        if getattr(self, "_h", None):
            _ffi.lib().kmap_bed_close(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:     # noqa: BLE001 -- interpreter shutdown
            pass


def _occurrence_input(occ):
    """(Occurrence, every row counts as a CSV row): a path is parsed natively (every row of the file is a row of the reference's
    iterrows); an in-memory Occurrence or scan_motif_occurence hit list only has the rows with a hit (the rows its CSV would hold)"""
    if isinstance(occ, Occurrence):
        return occ, False
    if isinstance(occ, (str, Path)):
        return read_occurrence(occ), True
    per = [tuple(r) for r in occ]                  # entries unpack to (hits_per_read, positions), ScanHits included
    return Occurrence([h for h, _ in per], [p for _, p in per], np.zeros(len(per[0][0]) if per else 0, np.int64)), False


def locate(bed: BedFile, occ: Occurrence, conseq_list, all_rows=True, timing=None):
    """the GPU pipeline: per consensus i (row, start, end) of the merged intervals in output order.  timing (dict, optional):
    'device_ms' from HIP events (upload to download)"""
    n_cons = len(conseq_list)
    if n_cons > occ.n_conseq:
        raise ValueError(f"the consensus file lists {n_cons} consensus sequences, the occurrence file has {occ.n_conseq} motif columns")
    n_rows = len(occ.seq_ind)
    if n_cons and n_rows:
        rows = np.ones(n_rows, bool) if all_rows else np.logical_or.reduce([h > 0 for h in occ.hits])
        s = occ.seq_ind[rows]
        bad = (s < 0) | (s >= bed.n_rows)
        if bad.any():
            raise ValueError(f"seq_ind {int(s[bad][0])} of the occurrence file is outside the BED file ({bed.n_rows} rows)")
    hits = [np.ascontiguousarray(occ.hits[c], np.int32) for c in range(n_cons)]
    pos = [np.ascontiguousarray(occ.pos[c], np.int32) for c in range(n_cons)]
    n_pos = np.array([len(p) for p in pos] or [0], np.int64)
    total = int(n_pos[:n_cons].sum())
    lens = np.array([len(s) for s in conseq_list] or [0], np.int32)
    out_row, out_start, out_end = (np.empty(max(total, 1), np.int64) for _ in range(3))
    n_per = np.zeros(max(n_cons, 1), np.int64)
    hp = (C.c_void_p * max(n_cons, 1))(*[a.ctypes.data for a in hits])
    pp = (C.c_void_p * max(n_cons, 1))(*[a.ctypes.data for a in pos])
    ms = _ffi.f32(0)
    seq_ind = np.ascontiguousarray(occ.seq_ind, np.int64)
    check(_ffi.lib().kmap_locations_sort(n_rows, n_cons, hp, pp, ptr(n_pos), ptr(lens), ptr(seq_ind), bed.n_rows, ptr(bed.start),
                                         ptr(bed.chrom_rank), bed.n_chrom, len(out_row), ptr(out_row), ptr(out_start), ptr(out_end),
                                         ptr(n_per), C.byref(ms)))
    if timing is not None:
        timing["device_ms"] = ms.value
    at = np.concatenate([[0], np.cumsum(n_per[:n_cons])]).astype(np.int64)
    return [(out_row[at[i]:at[i + 1]], out_start[at[i]:at[i + 1]], out_end[at[i]:at[i + 1]]) for i in range(n_cons)]


def _extract_motif_locations(bed_file, conseq_file, motif_occurrence_file, output_dir, timing=None):
    """`kmap extract_motif_locations` (reference util.py:292-352).  motif_occurrence_file: a path, an in-memory Occurrence or the hit
    list of scan_motif_occurence.  timing (dict, optional): seconds of 'parse', 'device', 'format' and the HIP-event 'device_ms'"""
    import time
    t0 = time.perf_counter()
    conseq_list = Path(conseq_file).read_text().splitlines()
    occ, all_rows = _occurrence_input(motif_occurrence_file)
    bed = BedFile(bed_file)
    try:
        t1 = time.perf_counter()
        res = locate(bed, occ, conseq_list, all_rows, timing)       # raises before any file or directory is made
        t2 = time.perf_counter()
        output_path = Path(output_dir)
        output_path.mkdir(parents=True, exist_ok=True)
        for i, (conseq, (row, start, end)) in enumerate(zip(conseq_list, res)):
            bed.write_locations(output_path / f"motif_{i}_{conseq}_locations.bed", i, row, start, end)
        t3 = time.perf_counter()
    finally:
        bed.close()
    if timing is not None:
        timing.update(parse=t1 - t0, device=t2 - t1, format=t3 - t2)
    print(f"Motif location extraction complete. Results saved in {output_path}")


def check_motif_co_occurence(input_fasta_file, motif1: str, motif2: str, max_ham_dist1: int, max_ham_dist2: int, output_dir,
                             revcom_mode=True):
    """`kmap check_motif_co_occurence` (reference motif_discovery.py:111-177): the occurrence scan of the two motifs on the GPU
    (user_motif_occurence.csv; when both have the same length the second radius wins, as in the reference), the co-occurrence
    matrices from the in-memory hit list, the reference's `co_occur_freq=XX.XX%` line when any pair co-occurs, and the four
    co-occurrence data files of scan_motif (the m0-m1 distance distribution is drawn from the distance data file).  No figures."""
    from .motif_discovery import _write_co_occurrence_files, get_user_motif_occurence_file
    from .reports import _as_occurrence, get_motif_co_occurence_mat
    input_fasta_path = Path(input_fasta_file)
    assert input_fasta_path.exists()
    output_dir_path = Path(output_dir)
    output_dir_path.mkdir(parents=True, exist_ok=True)
    conseq_list = [motif1, motif2]
    per = get_user_motif_occurence_file(input_fasta_path, conseq_list, [max_ham_dist1, max_ham_dist2],
                                        output_dir_path / "user_motif_occurence.csv", revcom_mode)
    occ = _as_occurrence(per)
    co_occur_mat, _, _ = get_motif_co_occurence_mat(occ, len(conseq_list))
    info_str = ""
    if np.any(co_occur_mat):
        co_occur_freq = co_occur_mat[0][1] * 2 / (co_occur_mat[0][0] + co_occur_mat[1][1])
        info_str = f"co_occur_freq={co_occur_freq*100:.2f}%"
        print(info_str)
    _write_co_occurrence_files(output_dir_path, occ, conseq_list)
    return info_str
