"""The resident read set: DeviceSeq (the encoded reads in HBM as 2-bit codes + invalid bitmask, with every verb that runs on
them: counting, masking, the occurrence and weight-matrix scans, shuffling) and the results that stay in HBM until someone asks
for them (ScanHits, ReadScores).  motif_discovery re-exports the names; distributed.py subclasses DeviceSeq and ScanHits.
"""
import ctypes as C
import threading

import numpy as np

from . import _ffi
from ._ffi import check, ptr


def _as_weights(W, who):
    """a weight matrix as the C ABI takes it: contiguous int32 [4, width]"""
    W = np.ascontiguousarray(W, dtype=np.int32)
    if W.ndim != 2 or W.shape[0] != 4:
        raise ValueError(f"{who}: weights of shape {W.shape}, expected (4, width) with rows A, C, G, T")
    return W


LIBRARY_BATCH, LIBRARY_BATCH_CHUNKS = 8, 24    # csrc/pwm_batch.h: a batch is at most this many matrices and chunks of 4 columns
LIBRARY_LDS_BINS, LIBRARY_MAX_BINS = 32768, 1 << 22      # ranges up to the first are counted in block-private bins; the second is the limit
SITES_MAX_LEN = 1 << 20                        # csrc/pwm_sites.hip: the longest read library_sites makes histograms for
SPACING_MAX_GAP = 511                          # csrc/pwm_spacing.hip: the largest gap library_spacing makes histograms for
# csrc/bit_pairs.hip: the words of a staging step, the fewest words of a block's slice, the most rows pair_counts takes
BIT_PAIRS_K, BIT_PAIRS_MIN_SLICE, BIT_PAIRS_MAX_ROWS = 32, 128, 4096


def _as_threshold(t, who):
    if not -2 ** 31 <= int(t) < 2 ** 31:
        raise ValueError(f"{who}: threshold {t} does not fit int32")
    return int(t)


def _pack_library(who, Ws, thresholds=None):
    """the matrices of a library as the batched entry points take them (csrc/pwm_batch.h): (n_mat, widths int32[n_mat], weights
    int32[n_mat, 4, 32] with zeros behind every width, thr int32[n_mat] or None without thresholds); ValueError under `who`"""
    Ws = [_as_weights(W, who) for W in Ws]
    n_mat, thr = len(Ws), None
    if thresholds is not None:
        thresholds = [_as_threshold(t, who) for t in thresholds]
        if n_mat != len(thresholds):
            raise ValueError(f"{who}: {n_mat} matrices, {len(thresholds)} thresholds")
        thr = np.array(thresholds, np.int32).reshape(n_mat)
    widths, weights = np.zeros(n_mat, np.int32), np.zeros((n_mat, 4, 32), np.int32)
    for m, W in enumerate(Ws):
        if not 4 <= W.shape[1] <= 31:
            raise ValueError(f"{who}: matrix {m} has width {W.shape[1]}, outside 4..31")
        widths[m] = W.shape[1]
        weights[m, :, :W.shape[1]] = W
    return n_mat, widths, weights, thr


class DeviceSeq:
    """The encoded reads resident in HBM as 2-bit codes + invalid bitmask (layout: packed.hip), plus the (n_seq, 2) borders.
    `inval_orig` is the pristine mask, `inval_work` the one find_motif masks; the codes are shared."""

    def __init__(self, seq_np_arr, boarder_mat, _device_arrays=None):
        if _device_arrays is not None:           # from_device(): the uint8 array and the borders already lie in HBM
            raw, self.n, self.borders, self.n_seq, fixed_len = _device_arrays
            self.borders_host = None
            self.read_len = np.full(self.n_seq, fixed_len, np.int64) if fixed_len is not None else None
        else:
            seq = np.ascontiguousarray(seq_np_arr, dtype=np.uint8)
            self.n = len(seq)
            self.borders_host = np.ascontiguousarray(boarder_mat, dtype=np.int64).reshape(-1, 2)
            self.n_seq = len(self.borders_host)
            self.borders = _ffi.DeviceBuffer.from_numpy(self.borders_host)
            self.read_len = (self.borders_host[:, 1] - self.borders_host[:, 0]).astype(np.int64)
            raw = _ffi.DeviceBuffer.from_numpy(seq) if self.n else _ffi.DeviceBuffer(16)
        self.groups = int(_ffi.lib().kmap_packed_groups(self.n))
        self.codes = _ffi.DeviceBuffer(self.groups * 4)
        self.inval_orig = _ffi.DeviceBuffer(self.groups * 2)
        self.inval_work = _ffi.DeviceBuffer(self.groups * 2)
        check(_ffi.lib().kmap_pack_reads_dev(raw.ptr, self.n, self.codes.ptr, self.inval_orig.ptr, None))
        # bit planes of the codes (0.25 B / position more): the scans and the masking test all windows bit-sliced on them
        self.planes = _ffi.DeviceBuffer(self.groups * 4)
        check(_ffi.lib().kmap_pack_planes_dev(self.codes.ptr, self.n, self.planes.ptr, None))
        _ffi.sync()
        raw.free()                      # the uint8 array does not stay on the device
        self._layout = False            # not looked at yet (_uniform_layout)
        self.reset()
        self._scan = None
        dev = _ffi.i32(0)
        check(_ffi.lib().kmap_get_device(C.byref(dev)))
        self.device = dev.value         # HIP's current device is per thread: worker threads that fetch hit lists select it
        self._lazy_lock, self._lazy_free, self._lazy_all = threading.Lock(), [], []     # scan handles of scan_lazy()

    @classmethod
    def from_device(cls, raw_u8, n, borders_dev, n_seq, fixed_read_len=None):
        """the reads already in HBM (raw_u8: DeviceBuffer with the uint8 array contract, consumed -- freed once packed;
        borders_dev: DeviceBuffer int64[n_seq][2]), e.g. from synth.synth_reads_dev; fixed_read_len: every read's length, if
        the caller knows it (the occurrence CSV needs the lengths on the host)"""
        return cls(None, None, _device_arrays=(raw_u8, int(n), borders_dev, int(n_seq), fixed_read_len))

    # the reads scan() results cover: these reads here; ALL reads for a read-sharded DistDeviceSeq (distributed.py)
    out_n_seq = property(lambda self: self.n_seq)
    out_read_len = property(lambda self: self.read_len)

    def reset(self):
        """restore the unmasked reads (reference motif_discovery.py:263): n/8 bytes"""
        check(_ffi.lib().kmap_memcpy_d2d(self.inval_work.ptr, self.inval_orig.ptr, self.groups * 2, None))

    def count(self, dc, k, dedupe, merge_revcom, use_work=True, gather_full=False):
        inval = self.inval_work if use_work else self.inval_orig
        nu = _ffi.i64(0)
        dc._unshard()
        check(_ffi.lib().kmap_counts_run_packed_dev(dc._h, self.codes.ptr, inval.ptr, self.n, self.borders.ptr, self.n_seq, k,
                                                    int(dedupe), int(merge_revcom), C.byref(nu), None))
        dc.k, dc.n_uniq = k, nu.value
        return dc.n_uniq

    def count_range(self, dc, k, dedupe, merge_revcom, first_bin, n_bins, use_work=True):
        """positions [first_bin, first_bin + n_bins) -- in key order -- of the table count() would produce, from the windows that
        decide them alone (kmap_counts_run_packed_range_dev, 11 <= k <= 16): a rank's share of a key-space-sharded count"""
        inval = self.inval_work if use_work else self.inval_orig
        nu = _ffi.i64(0)
        dc._unshard()
        check(_ffi.lib().kmap_counts_run_packed_range_dev(dc._h, self.codes.ptr, inval.ptr, self.n, self.borders.ptr, self.n_seq, k,
                                                          int(dedupe), int(merge_revcom), int(first_bin), int(n_bins), C.byref(nu), None))
        dc.k, dc.n_uniq = k, nu.value
        return dc.n_uniq

    def mask(self, k, consensus_kh_arr, max_ham_dist_arr):
        cons = np.ascontiguousarray(consensus_kh_arr, dtype=np.uint64)
        rad = np.ascontiguousarray(max_ham_dist_arr, dtype=np.int32)
        check(_ffi.lib().kmap_mask_hamball_packed_dev(self.codes.ptr, self.inval_work.ptr, self.n, k, ptr(cons), ptr(rad),
                                                      len(cons), self.planes.ptr, None))

    def download(self):
        """the working reads as the reference's uint8 array (masked positions = 255)"""
        out_d = _ffi.DeviceBuffer(max(self.n, 1))
        check(_ffi.lib().kmap_unpack_reads_dev(self.codes.ptr, self.inval_work.ptr, self.n, out_d.ptr, None))
        out = out_d.to_numpy(np.uint8, (self.n,))
        out_d.free()
        return out

    def _uniform_layout(self):
        """(read_len, stride) when read s is [s * stride, s * stride + read_len) -- fixed-length reads -- else None; from the host
        borders (one vectorised comparison, once), or the caller's fixed length for reads that only exist in HBM"""
        if self._layout is False:
            self._layout = None
            bh = self.borders_host
            if bh is not None and len(bh) >= 1 and bh[0, 0] == 0:
                ln = int(bh[0, 1] - bh[0, 0])
                stride = int(bh[1, 0] - bh[0, 0]) if len(bh) > 1 else ln + 1
                if stride >= max(ln, 1):
                    idx = np.arange(len(bh), dtype=np.int64) * stride
                    if np.array_equal(bh[:, 0], idx) and np.array_equal(bh[:, 1], idx + ln):
                        self._layout = (ln, stride)
            elif bh is None and self.read_len is not None and self.n_seq >= 1:
                ln = int(self.read_len[0])
                self._layout = (ln, ln + 1)         # synth_reads_dev: a separator behind every read (verified on the device below)
        return self._layout

    def declare_layout(self, handle):
        """tell a scan handle that these reads are laid out uniformly (kmap_scan_declare_uniform verifies it on the device): its runs on
        these borders then derive them from the read index instead of loading 16 bytes per read"""
        lay = self._uniform_layout()
        if lay is None:
            return False
        ok = _ffi.i32(0)
        check(_ffi.lib().kmap_scan_declare_uniform(handle, self.borders.ptr, self.n_seq, lay[0], lay[1], C.byref(ok), None))
        return bool(ok.value)

    def _new_scan_handle(self):
        h = _ffi.vp()
        check(_ffi.lib().kmap_scan_create(C.byref(h)))
        self.declare_layout(h.value)
        return h.value

    def _own_scan_handle(self):
        """the handle of scan() and scan_pwm(), created on first use"""
        if self._scan is None:
            self._scan = self._new_scan_handle()
        return self._scan

    def _take_lazy_handle(self):
        """a free handle of the lazy rotation, or a new one; it goes back through _lazy_release"""
        with self._lazy_lock:
            h = self._lazy_free.pop() if self._lazy_free else None
        if h is None:
            h = self._new_scan_handle()
            self._lazy_all.append(h)
        return h

    def scan(self, k, consensus_kh, radius, revcom):
        """positions at each read's minimum hit distance (original, unmasked reads):
        returns (hits_per_read int32[n_seq], positions int32[total])."""
        tot = _ffi.i64(0)
        check(_ffi.lib().kmap_scan_run_packed_dev(self._own_scan_handle(), self.codes.ptr, self.inval_orig.ptr, self.n, self.borders.ptr,
                                                  self.n_seq, k, int(consensus_kh), int(radius), int(revcom), C.byref(tot),
                                                  self.planes.ptr, None))
        hits = np.empty(self.n_seq, np.int32)
        pos = np.empty(tot.value, np.int32)
        check(_ffi.lib().kmap_scan_fetch(self._scan, ptr(hits), None, ptr(pos)))   # per-read minimum distances stay on the device
        return hits, pos

    def scan_lazy(self, k, consensus_kh, radius, revcom):
        """scan() whose hit list stays in HBM, inside its scan handle, until someone asks for it: `ScanHits.n_reads_hit / .total /
        .max_hits` are known at once (what scan_motif's candidate table needs), the two arrays are fetched on first use -- by the
        background CSV writer in scan_motif, off the critical path.  Handles rotate: a fetched (or dropped) ScanHits hands its
        handle back, so a run allocates a handful of result buffers once instead of one set per consensus."""
        h = self._take_lazy_handle()
        tot, nhit, mx = _ffi.i64(0), _ffi.i64(0), _ffi.i32(0)
        check(_ffi.lib().kmap_scan_run_packed_dev(h, self.codes.ptr, self.inval_orig.ptr, self.n, self.borders.ptr,
                                                  self.n_seq, k, int(consensus_kh), int(radius), int(revcom), C.byref(tot),
                                                  self.planes.ptr, None))
        check(_ffi.lib().kmap_scan_summary(h, C.byref(nhit), C.byref(mx), None))    # returns once the lists are complete
        return ScanHits(self, h, self.n_seq, tot.value, nhit.value, mx.value)

    def _pwm_run(self, h, W, t, revcom):
        W, t = _as_weights(W, "scan_pwm"), _as_threshold(t, "scan_pwm")
        tot = _ffi.i64(0)
        check(_ffi.lib().kmap_pwm_scan_packed_dev(h, self.codes.ptr, self.inval_orig.ptr, self.n, self.borders.ptr, self.n_seq,
                                                  W.shape[1], ptr(W), t, int(bool(revcom)), C.byref(tot), None))
        return tot.value

    def scan_pwm(self, W, t, revcom):
        """every window of the original reads whose weight-matrix score (W: int32 [4, width], rows A C G T; with revcom the larger
        of the two strands' scores) is >= t and that touches no invalid position (csrc/pwm_scan.hip):
        returns (hits_per_read int32[n_seq], positions int32[total], scores int32[total], strand uint8[total]: 0 '+', 1 '-')."""
        total = self._pwm_run(self._own_scan_handle(), W, t, revcom)
        hits, pos = np.empty(self.n_seq, np.int32), np.empty(total, np.int32)
        scores, strand = np.empty(total, np.int32), np.empty(total, np.uint8)
        check(_ffi.lib().kmap_pwm_scan_fetch(self._scan, ptr(hits), ptr(pos), ptr(scores), ptr(strand)))
        return hits, pos, scores, strand

    def scan_pwm_lazy(self, W, t, revcom):
        """scan_pwm() whose (hits_per_read, positions) stay in HBM like scan_lazy()'s: a ScanHits (scores and strands are not kept)"""
        h = self._take_lazy_handle()
        nhit, mx = _ffi.i64(0), _ffi.i32(0)
        try:
            total = self._pwm_run(h, W, t, revcom)
            check(_ffi.lib().kmap_scan_summary(h, C.byref(nhit), C.byref(mx), None))
        except BaseException:
            self._lazy_release(h)
            raise
        return ScanHits(self, h, self.n_seq, total, nhit.value, mx.value)

    def pwm_counts(self, W, t, revcom, select_best=True):
        """one refinement step (csrc/pwm_refine.hip): of scan_pwm(W, t, revcom)'s hits on the original reads,
        every one (select_best False) or per read the one with the largest score, the smallest loc on a tie; returns
        (C' int64[4, width]: C'[b][j] = selected windows whose oriented base j is b, n_hits, n_selected, n_minus).  Needs no scan handle."""
        W, t = _as_weights(W, "pwm_counts"), _as_threshold(t, "pwm_counts")
        counts = np.zeros((4, W.shape[1]), np.int64)
        n_hits, n_sel, n_minus = _ffi.i64(0), _ffi.i64(0), _ffi.i64(0)
        check(_ffi.lib().kmap_refine_counts_packed_dev(self.codes.ptr, self.inval_orig.ptr, self.n, self.borders.ptr, self.n_seq,
                                                       W.shape[1], ptr(W), t, int(bool(revcom)), int(bool(select_best)), ptr(counts),
                                                       C.byref(n_hits), C.byref(n_sel), C.byref(n_minus), None))
        return counts, n_hits.value, n_sel.value, n_minus.value

    def read_scores(self, W, revcom):
        """per read the valid window with the largest score, on a tie the smallest loc (csrc/pwm_readscore.hip, DESIGN.md section
        14; scores and strands are scan_pwm's, there is no threshold): a ReadScores whose three arrays stay in HBM until fetch().
        Needs no scan handle."""
        W = _as_weights(W, "read_scores")
        out = ReadScores(self.n_seq)
        try:
            n_scored = _ffi.i64(0)
            check(_ffi.lib().kmap_readscore_packed_dev(self.codes.ptr, self.inval_orig.ptr, self.n, self.borders.ptr, self.n_seq,
                                                       W.shape[1], ptr(W), int(bool(revcom)), out.score.ptr, out.loc.ptr, out.strand.ptr,
                                                       C.byref(n_scored), None))
        except BaseException:
            out.close()
            raise
        out.n_scored = n_scored.value
        return out

    def library_histograms(self, Ws, los, n_bins, revcom):
        """For every weight matrix of Ws (int32 [4, width], widths may differ) the histogram of the reads' best scores over
        [los[m], los[m] + n_bins[m]), as read_scores(W, revcom).histogram(lo, n_bins) gives it, from one pass over the original
        reads per batch of matrices and without the per-read arrays (csrc/pwm_library.hip): returns
        (list of uint64[n_bins[m]], n_outside int64[n_mat]: scorable reads whose best score lies outside the range -- they are in no
        bin --, n_scored int64[n_mat]: reads with a valid window).  Needs no scan handle."""
        n_mat, widths, weights, _ = _pack_library("library_histograms", Ws)
        los, n_bins = [int(x) for x in los], [int(x) for x in n_bins]
        if not n_mat == len(los) == len(n_bins):
            raise ValueError(f"library_histograms: {n_mat} matrices, {len(los)} range starts, {len(n_bins)} bin counts")
        for m, (lo, nb) in enumerate(zip(los, n_bins)):
            if not 0 <= nb <= LIBRARY_MAX_BINS or not -2 ** 31 <= lo < 2 ** 31:
                raise ValueError(f"library_histograms: matrix {m}: {nb} bins from {lo}, at most 2^22 bins of int32 scores are supported")
        lo_arr, nb_arr = np.array(los, np.int32).reshape(n_mat), np.array(n_bins, np.int64).reshape(n_mat)
        flat = np.zeros(int(nb_arr.sum()), np.uint64)
        outside, scored = np.zeros(n_mat, np.int64), np.zeros(n_mat, np.int64)
        check(_ffi.lib().kmap_readscore_library_dev(self.codes.ptr, self.inval_orig.ptr, self.n, self.borders.ptr, self.n_seq, n_mat,
                                                    ptr(widths), ptr(weights), ptr(lo_arr), ptr(nb_arr), int(bool(revcom)), ptr(flat),
                                                    ptr(outside), ptr(scored), None))
        ends = np.cumsum(nb_arr)
        return [flat[e - nb:e] for e, nb in zip(ends.tolist(), nb_arr.tolist())], outside, scored

    def max_read_len(self):
        """the largest read length: from the host's lengths, or for reads that only exist in HBM from the borders, fetched once"""
        if self.read_len is None:
            b = self.borders.to_numpy(np.int64, (self.n_seq, 2))
            _ffi.sync()
            self.read_len = (b[:, 1] - b[:, 0]).astype(np.int64)
        return int(self.read_len.max()) if self.n_seq else 0

    def library_sites(self, Ws, thresholds, revcom, max_len=None):
        """For every weight matrix of Ws (int32 [4, width], widths may differ) where the best window of its site reads lies
        (csrc/pwm_sites.hip).  A site read is a read whose best window (read_scores': the largest score, the
        smallest loc on a tie) scores thresholds[m] or more; with L its length, d = 2 loc + width - L is the window's doubled
        centre offset.  Returns (D int64[n_mat][2 max_len + 1]: D[m][d + max_len] = site reads with offset d, Hlen
        int64[n_mat][max_len + 1]: site reads of length L, n_sites int64[n_mat]: the sum of either, n_too_long int64[n_mat]: site
        reads longer than max_len, which are in neither histogram).  max_len None: the largest read length.  One pass over the
        original reads per batch of matrices, nothing per read leaves the device.  Needs no scan handle."""
        n_mat, widths, weights, thr = _pack_library("library_sites", Ws, thresholds)
        if max_len is not None and (isinstance(max_len, bool) or int(max_len) != max_len or not 0 <= max_len <= SITES_MAX_LEN):
            raise ValueError(f"library_sites: max_len {max_len} outside 0 .. 2^20")
        max_len = self.max_read_len() if max_len is None else int(max_len)
        if max_len > SITES_MAX_LEN:
            raise ValueError(f"library_sites: the longest read has {max_len} bases, more than 2^20")
        D, Hlen = np.zeros((n_mat, 2 * max_len + 1), np.uint64), np.zeros((n_mat, max_len + 1), np.uint64)
        sites, too_long = np.zeros(n_mat, np.int64), np.zeros(n_mat, np.int64)
        check(_ffi.lib().kmap_readscore_sites_library_dev(self.codes.ptr, self.inval_orig.ptr, self.n, self.borders.ptr, self.n_seq, n_mat,
                                                          ptr(widths), ptr(weights), ptr(thr), int(bool(revcom)), max_len, ptr(D),
                                                          ptr(Hlen), ptr(sites), ptr(too_long), None))
        return D.astype(np.int64), Hlen.astype(np.int64), sites, too_long

    def library_counts(self, Ws, thresholds, revcom, use_work=False):
        """One refinement step for every weight matrix of Ws (int32 [4, width], widths may differ): the count matrix of the site
        reads' best windows (csrc/pwm_sites.hip).  Per matrix what pwm_counts(W, t, revcom,
        select_best=True) returns without n_hits, from library_sites' one pass over the original reads per batch of matrices:
        returns (list of int64[4, w_m]: C'[b][j] = selected windows whose oriented base j is b, n_selected int64[n_mat]: the site
        reads, n_minus int64[n_mat]: those on '-').  Nothing per read leaves the device.  Needs no scan handle.  use_work: the
        windows are those that are valid under the working mask (what mask() and erase_sites() left) instead of the original one."""
        n_mat, widths, weights, thr = _pack_library("library_counts", Ws, thresholds)
        counts = np.zeros((n_mat, 4, 32), np.uint64)
        n_sel, n_minus = np.zeros(n_mat, np.int64), np.zeros(n_mat, np.int64)
        inval = self.inval_work if use_work else self.inval_orig
        check(_ffi.lib().kmap_readscore_counts_library_dev(self.codes.ptr, inval.ptr, self.n, self.borders.ptr, self.n_seq, n_mat,
                                                           ptr(widths), ptr(weights), ptr(thr), int(bool(revcom)), ptr(counts),
                                                           ptr(n_sel), ptr(n_minus), None))
        return [counts[m, :, :int(widths[m])].astype(np.int64) for m in range(n_mat)], n_sel, n_minus

    def erase_sites(self, Ws, thresholds, revcom, use_work=True):
        """Every position inside a hit of a weight matrix of Ws (int32 [4, width], widths may differ) becomes invalid in the working
        mask (csrc/pwm_erase.hip).  A hit of matrix m is scan_pwm's: a window that scores thresholds[m] or
        more (with revcom the larger of the two strands' scores) and touches no invalid position -- of the working mask as it is
        on entry (use_work) or of the original one; every matrix sees that same mask.  Returns (n_hits int64[n_mat], n_covered
        int64[n_mat]: the positions inside at least one hit of the matrix, n_new: the positions that were valid in the working mask
        and are not any more).  Always writes inval_work, never the codes or inval_orig; reset() undoes it as it undoes mask().
        Runs on the null stream and blocks.  Needs no scan handle."""
        n_mat, widths, weights, thr = _pack_library("erase_sites", Ws, thresholds)
        n_hits, n_cov, n_new = np.zeros(n_mat, np.int64), np.zeros(n_mat, np.int64), _ffi.i64(0)
        inval = self.inval_work if use_work else self.inval_orig
        check(_ffi.lib().kmap_erase_pwm_sites_dev(self.codes.ptr, inval.ptr, self.n, n_mat, ptr(widths), ptr(weights), ptr(thr),
                                                  int(bool(revcom)), self.inval_work.ptr, ptr(n_hits), ptr(n_cov), C.byref(n_new)))
        return n_hits, n_cov, n_new.value

    def library_spacing(self, primary, prim_width, prim_threshold, Ws, thresholds, revcom, max_gap=150):
        """For every weight matrix of Ws (int32 [4, width], widths may differ) at which distance and in which orientation its best
        site lies from the primary matrix's site (csrc/pwm_spacing.hip).  `primary` is the ReadScores of the
        primary matrix (read_scores(W_P, revcom), still in HBM) of prim_width columns: a read whose best window scores
        prim_threshold or more is a primary read, p that window's loc and sP its strand.  The secondary site of matrix m is the
        best window (read_scores' order) among the valid windows that score thresholds[m] or more and do not overlap the primary
        window; its gap g counts the bases between the two windows.  Returns (S int64[n_mat, 4, max_gap + 1]: S[m][2 downstream
        + opposite][g] = pair reads, the side told in the primary's orientation, R int64[n_mat, max_gap + 2, max_gap + 2]:
        R[m][u][d] = the same reads by their upstream and downstream rooms, the window positions on each side with a gap of at
        most max_gap, n_primary, n_pair int64[n_mat]: primary reads with a secondary site, n_far int64[n_mat]: those with
        g > max_gap, which are in neither histogram).  One pass over the original reads per batch of matrices, nothing per read
        leaves the device.  Needs no scan handle."""
        n_mat, widths, weights, thr = _pack_library("library_spacing", Ws, thresholds)
        prim_threshold = _as_threshold(prim_threshold, "library_spacing")
        if isinstance(prim_width, bool) or int(prim_width) != prim_width or not 4 <= prim_width <= 31:
            raise ValueError(f"library_spacing: the primary matrix has width {prim_width}, outside 4..31")
        if isinstance(max_gap, bool) or int(max_gap) != max_gap or not 0 <= max_gap <= SPACING_MAX_GAP:
            raise ValueError(f"library_spacing: max_gap {max_gap} outside 0 .. {SPACING_MAX_GAP}")
        if not isinstance(primary, ReadScores) or primary.n_seq != self.n_seq:
            raise ValueError(f"library_spacing: the primary must be the ReadScores of these {self.n_seq} reads")
        G = int(max_gap)
        S, R = np.zeros((n_mat, 4, G + 1), np.uint64), np.zeros((n_mat, G + 2, G + 2), np.uint64)
        pair, far, n_primary = np.zeros(n_mat, np.int64), np.zeros(n_mat, np.int64), _ffi.i64(0)
        check(_ffi.lib().kmap_readscore_spacing_library_dev(self.codes.ptr, self.inval_orig.ptr, self.n, self.borders.ptr, self.n_seq,
                                                            primary.score.ptr, primary.loc.ptr, primary.strand.ptr, int(prim_width),
                                                            prim_threshold, n_mat, ptr(widths), ptr(weights), ptr(thr), int(bool(revcom)),
                                                            G, ptr(S), ptr(R), C.byref(n_primary), ptr(pair), ptr(far), None))
        return S.astype(np.int64), R.astype(np.int64), n_primary.value, pair, far

    def library_presence(self, Ws, thresholds, revcom):
        """For every weight matrix of Ws (int32 [4, width], widths may differ) which reads hold a site: read r is present under
        matrix m when its best window (read_scores') scores thresholds[m] or more; a read without a valid window never is
        (csrc/pwm_presence.hip).  Returns a PresencePlanes: one bit per (matrix, read) in HBM and n_present
        int64[n_mat].  One pass over the original reads per batch of matrices, nothing per read leaves the device.  Needs no scan
        handle."""
        n_mat, widths, weights, thr = _pack_library("library_presence", Ws, thresholds)
        out = PresencePlanes(n_mat, self.n_seq)
        try:
            check(_ffi.lib().kmap_presence_library_dev(self.codes.ptr, self.inval_orig.ptr, self.n, self.borders.ptr, self.n_seq, n_mat,
                                                       ptr(widths), ptr(weights), ptr(thr), int(bool(revcom)), out.planes.ptr,
                                                       out.n_words, ptr(out.n_present), None))
        except BaseException:
            out.close()
            raise
        return out

    def shuffled(self, klet=2, seed=0):
        """a new resident read set: every maximal run of valid bases of the ORIGINAL reads (inval_orig; a mask() before does not
        count) shuffled so that its base counts (klet 1) or its first base and dinucleotide counts (klet 2) stay (csrc/shuffle.hip,
        DESIGN.md section 15).  The result has its own copy of the borders; this object is not touched.  `shuffle_stats` of the
        result = (segments, valid bases)."""
        if isinstance(klet, bool) or int(klet) != klet or int(klet) not in (1, 2):
            raise ValueError(f"shuffled: klet {klet}: 1 (base counts) or 2 (dinucleotide counts) expected")
        if isinstance(seed, bool) or int(seed) != seed or not 0 <= seed < 2 ** 64:
            raise ValueError(f"shuffled: seed {seed} outside 0 .. 2^64 - 1")
        raw = _ffi.DeviceBuffer(max(self.n, 16))
        borders = None
        try:
            stats = (_ffi.i64 * 2)()
            check(_ffi.lib().kmap_shuffle_packed_dev(self.codes.ptr, self.inval_orig.ptr, self.n, int(klet), int(seed), raw.ptr, stats, None))
            borders = _ffi.DeviceBuffer(max(self.n_seq, 1) * 16)
            if self.n_seq:
                check(_ffi.lib().kmap_memcpy_d2d(borders.ptr, self.borders.ptr, self.n_seq * 16, None))
            out = DeviceSeq.from_device(raw, self.n, borders, self.n_seq)
        except BaseException:
            # no DeviceSeq owns the two buffers unless from_device returned.  It frees raw itself once packed and never borders;
            # DeviceBuffer.free is a no-op the second time, so freeing both here is right wherever the failure came from.
            raw.free()
            if borders is not None:
                borders.free()
            raise
        out.borders_host = None if self.borders_host is None else self.borders_host.copy()
        out.read_len = None if self.read_len is None else self.read_len.copy()
        out.shuffle_stats = (int(stats[0]), int(stats[1]))
        return out

    def _lazy_release(self, h):
        with self._lazy_lock:
            if self._lazy_all is not None:
                self._lazy_free.append(h)

    def close(self):
        if self._scan:
            _ffi.lib().kmap_scan_destroy(self._scan)
            self._scan = None
        with self._lazy_lock:
            handles, self._lazy_all, self._lazy_free = self._lazy_all or [], None, []
        for h in handles:                 # a ScanHits not fetched by now reports that its sequence is closed
            _ffi.lib().kmap_scan_destroy(h)
        for b in (self.codes, self.planes, self.inval_orig, self.inval_work, self.borders):
            b.free()


class ReadScores:
    """DeviceSeq.read_scores' result in HBM: score int32[n_seq] (unit 0.01 bit), loc int32[n_seq], strand uint8[n_seq] (0 '+', 1 '-');
    a read without a valid window has INT32_MIN, -1, 0.  `n_scored` = reads with a valid window."""
    MAX_BINS = 1 << 22

    def __init__(self, n_seq):
        self.n_seq, self.n_scored = int(n_seq), 0
        self.score, self.loc = _ffi.DeviceBuffer(max(self.n_seq, 1) * 4), _ffi.DeviceBuffer(max(self.n_seq, 1) * 4)
        self.strand = _ffi.DeviceBuffer(max(self.n_seq, 1))

    def fetch(self):
        """(score, loc, strand) as numpy arrays"""
        out = (self.score.to_numpy(np.int32, (self.n_seq,)), self.loc.to_numpy(np.int32, (self.n_seq,)),
               self.strand.to_numpy(np.uint8, (self.n_seq,)))
        _ffi.sync()
        return out

    def histogram(self, lo, n_bins):
        """uint64[n_bins]: the number of scorable reads with best score lo + i; ValueError when n_bins is more than 2^22 or a
        scorable read's score lies outside [lo, lo + n_bins)"""
        lo, n_bins = int(lo), int(n_bins)
        if not 0 <= n_bins <= self.MAX_BINS or not -2 ** 31 <= lo < 2 ** 31:
            raise ValueError(f"read score histogram: {n_bins} bins from {lo}, at most 2^22 bins of int32 scores are supported")
        hist, outside = np.zeros(n_bins, np.uint64), _ffi.i64(0)
        check(_ffi.lib().kmap_readscore_hist_dev(self.score.ptr, self.loc.ptr, self.n_seq, lo, n_bins, ptr(hist), C.byref(outside), None))
        if outside.value:
            raise ValueError(f"read score histogram: {outside.value} reads score outside [{lo}, {lo + n_bins})")
        return hist

    def close(self):
        for b in (self.score, self.loc, self.strand):
            b.free()


def bitrows_pair_counts(planes, n_mat, n_words):
    """int64 [n_mat, n_mat]: C[i][j] = the bits that rows i and j of the bit matrix `planes` (a DeviceBuffer of uint64 [n_mat,
    n_words]) share; symmetric, the diagonal holds the row popcounts (csrc/bit_pairs.hip)"""
    n_mat, n_words = int(n_mat), int(n_words)
    if not 0 <= n_mat <= BIT_PAIRS_MAX_ROWS or n_words < 0:
        raise ValueError(f"pair_counts: {n_mat} rows of {n_words} words, 0 .. {BIT_PAIRS_MAX_ROWS} rows are supported")
    pairs = np.zeros((n_mat, n_mat), np.uint64)
    check(_ffi.lib().kmap_bitrows_pair_counts_dev(planes.ptr, n_mat, n_words, ptr(pairs), None))
    return pairs.astype(np.int64)


class PresencePlanes:
    """DeviceSeq.library_presence's result: planes uint64 [n_mat, n_words] in HBM, bit r & 63 (least significant first) of word
    r >> 6 of row m = read r is present under matrix m, the bits behind n_seq are 0; n_present int64[n_mat] = the row popcounts."""

    def __init__(self, n_mat, n_seq):
        self.n_mat, self.n_seq, self.n_words = int(n_mat), int(n_seq), (int(n_seq) + 63) // 64
        self.planes = _ffi.DeviceBuffer(max(self.n_mat * self.n_words, 1) * 8)
        self.n_present = np.zeros(self.n_mat, np.int64)

    def pair_counts(self):
        """int64 [n_mat, n_mat]: C[i][j] = reads present under both matrix i and matrix j; C[i][i] = n_present[i]"""
        return bitrows_pair_counts(self.planes, self.n_mat, self.n_words)

    def fetch(self):
        """the planes as a uint64 [n_mat, n_words] numpy array"""
        out = self.planes.to_numpy(np.uint64, (self.n_mat, self.n_words))
        _ffi.sync()
        return out

    def close(self):
        self.planes.free()


class ScanHits:
    """One consensus' hit list, resident in HBM (in its scan handle) until first use.  Unpacks like the (hits_per_read, positions)
    pair scan() returns (`hits, pos = scan_hits` fetches); the summary numbers need no fetch."""

    def __init__(self, owner, handle, n_seq, total, n_reads_hit, max_hits):
        self._owner, self._handle = owner, handle
        self.n_seq, self.total, self.n_reads_hit, self.max_hits = n_seq, total, n_reads_hit, max_hits
        self._host = None
        self._lock = threading.Lock()

    def _fetch(self, fetch, hits_dtype):
        """(hits, positions) on a private stream; the handle goes back to its sequence.  The caller holds the lock."""
        if self._owner._lazy_all is None:
            raise RuntimeError("ScanHits: the DeviceSeq was closed before the hit list was fetched")
        hits, pos = np.empty(self.n_seq, hits_dtype), np.empty(self.total, np.int32)
        check(_ffi.lib().kmap_set_device(self._owner.device))  # this may be a CSV writer thread (fresh threads start on device 0)
        st = _ffi.vp()
        check(_ffi.lib().kmap_stream_create(C.byref(st)))      # own stream: neither waits for nor blocks the launching thread
        try:
            check(fetch(self._handle, ptr(hits), ptr(pos), st.value))
        finally:
            _ffi.lib().kmap_stream_destroy(st.value)
        self._owner._lazy_release(self._handle)
        self._owner, self._handle = None, None
        return hits, pos

    def host(self):
        with self._lock:
            if self._host is None:
                if self._handle is None:
                    raise RuntimeError("ScanHits: the list was already handed to a CSV writer (host_u8)")
                self._host = list(self._fetch(_ffi.lib().kmap_scan_fetch_stream, np.int32))
            return self._host

    @property
    def unfetched(self):
        return self._host is None and self._handle is not None

    def host_u8(self):
        """(hits as uint8, positions) for a list with max_hits <= 255, fetched without keeping the int32 pair; the handle goes
        back to its sequence, so this is the list's last use"""
        with self._lock:
            assert self._host is None and self._handle is not None and self.max_hits <= 255
            return self._fetch(_ffi.lib().kmap_scan_fetch_stream_u8, np.uint8)

    def release(self):
        """hand the scan handle back to its sequence without a fetch: the list is dropped, the summary numbers stay"""
        with self._lock:
            if self._handle is not None:
                self._owner._lazy_release(self._handle)
                self._owner, self._handle = None, None

    def __del__(self):
        try:
            self.release()
        except Exception:     # noqa: BLE001 -- interpreter shutdown
            pass

    def __iter__(self):
        return iter(self.host())

    def __getitem__(self, i):
        return self.host()[i]

    def __len__(self):
        return 2
