"""GPU parity of the tiled Hamming kernel at the edges of its 1024-column wave quarters (byte-exact vs the oracle's
ko_hamdist_rows).

A tile-kernel wave owns one quarter.  For a row of a short consensus it decides once, for all its 1024 columns, whether they lie
entirely inside the row's label group, entirely outside it, or across a group boundary, and only in the last case selects per
column.  Labels here put group boundaries on, next to and away from quarter edges, into the partial last quarter, and nowhere;
single invalid labels break otherwise uniform quarters.  Every case pre-fills the output with 0xA5 and checks
that the kernel wrote every byte it owes (rows [row0, row0 + nrows) x columns [0, n)) and nothing else (pad bytes, guard rows),
as test_gpu_hamdist_tail.py does.  All shapes have n >= 4096 and the odd-4-KiB pitch, so all of them take the tile kernel."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
GUARD_BEFORE, GUARD_AFTER = 8, 300
N = 4096 + 1024 + 17             # one full column block, one full quarter and a partial quarter of the tail block
ROWS = (1000, 60)                # rows 1000 .. 1059: in "edges" the rows of labels 1, 2 (row 1023), 0 (row 1024) and 1 again


def _lens(k):
    """label 0 full length, label 1 a (k - 1)-base consensus, label 2 a 3-base one"""
    return np.array([k, k - 1, 3], np.int32)


def _segments(n, edges, labs):
    lab = np.empty(n, np.int32)
    for lo, hi, l in zip([0] + edges, edges + [n], labs):
        lab[lo:hi] = l
    return lab


def _labels(n, mode):
    i = np.arange(n)
    if mode == "edges":                # boundaries at columns 1023, 1024, 1025, 2048 and 5120 (the last full quarter edge)
        return _segments(n, [1023, 1024, 1025, 2048, 5120], [1, 2, 0, 1, 2, 1])
    if mode == "partial_boundary":     # a boundary inside the partial last quarter (columns 5120 .. n - 1)
        return _segments(n, [1030, n - 9], [2, 1, 2])
    if mode == "partial_uniform":      # the partial last quarter carries one id; the boundary lies in the quarter in front of it
        return _segments(n, [1030, 5000], [1, 2, 1])
    if mode == "interleaved":          # every quarter mixed: every wave selects per column
        return (i % 3).astype(np.int32)
    if mode == "all_short":            # every quarter uniform with a non-zero group id
        return np.ones(n, np.int32)
    if mode == "all_full":             # no short consensus anywhere
        return np.zeros(n, np.int32)
    if mode == "invalid":              # -1 and labels >= n_lab act as id 0 and make their otherwise uniform quarters mixed
        lab = np.ones(n, np.int32)
        lab[[100, 1010]] = -1
        lab[3000] = 3
        lab[n - 5] = 1 << 20
        return lab
    raise AssertionError(mode)


def _check(n, k, lab, lens, row0, nrows, seed):
    from kmap_amd import _ffi
    from kmap_amd.hamdist import hamdist_matrix_dev, pitch_for
    from kmap_amd.kmer_count import get_hash_dtype
    from oracle import oracle as O
    rng = np.random.default_rng(seed)
    kh = rng.integers(0, 4 ** k, size=n, dtype=np.uint64)
    lab = np.ascontiguousarray(lab, np.int32)
    ld = pitch_for(n)
    assert n >= 4096 and ld % 4096 == 0 and (ld // 4096) % 2 == 1 and ld >= n
    before, after = min(GUARD_BEFORE, row0), min(GUARD_AFTER, n - row0 - nrows)
    rows_buf = before + nrows + after
    kh_d, lab_d = _ffi.DeviceBuffer.from_numpy(kh.astype(get_hash_dtype(k))), _ffi.DeviceBuffer.from_numpy(lab)
    out_d = _ffi.DeviceBuffer(rows_buf * ld)
    _ffi.check(_ffi.lib().kmap_memset(out_d.ptr, SENTINEL, rows_buf * ld, None))
    hamdist_matrix_dev(kh_d.ptr, lab_d.ptr, n, k, lens, out_d.ptr + before * ld, ld, row0=row0, nrows=nrows)
    got = out_d.to_numpy(np.uint8, (rows_buf, ld))
    for b in (out_d, kh_d, lab_d):
        b.free()
    want = np.empty((nrows, n), np.uint8)
    O.lib().ko_hamdist_rows(kh, lab, n, k, np.ascontiguousarray(lens, np.int32), len(lens), row0, nrows, want)
    mine = got[before:before + nrows]
    np.testing.assert_array_equal(mine[:, :n], want)
    assert np.all(mine[:, n:] == SENTINEL), "pad bytes [n, ld) of a written row were overwritten"
    assert np.all(got[:before] == SENTINEL), "a row in front of the range was written"
    assert np.all(got[before + nrows:] == SENTINEL), "a row behind the range was written"


MODES = ["edges", "partial_boundary", "partial_uniform", "interleaved", "all_short", "all_full", "invalid"]


@pytest.mark.parametrize("k", [8, 12, 16])           # <1,4>, <0,8>, <2,8> (k = 16 through the u64 entry)
@pytest.mark.parametrize("mode", MODES)
def test_label_layouts(mode, k):
    _check(N, k, _labels(N, mode), _lens(k), *ROWS, seed=100 * k + MODES.index(mode))


@pytest.mark.parametrize("k", [8, 12, 16])
def test_no_labels(k):
    """n_lab = 0: whatever the label array holds, every column has id 0"""
    _check(N, k, _labels(N, "interleaved"), np.zeros(0, np.int32), *ROWS, seed=k)


@pytest.mark.parametrize("k", [8, 12, 16])
@pytest.mark.parametrize("row0,nrows", [(0, 1), (5, 37)])
def test_row_ranges(row0, nrows, k):
    """rows of the (k - 1)-base label across all the quarter-edge boundaries"""
    _check(N, k, _labels(N, "edges"), _lens(k), row0, nrows, seed=31 * k + nrows)


def test_full_height():
    """n = 5137, all rows, k = 8: every row of every label against every quarter"""
    _check(N, 8, _labels(N, "edges"), _lens(8), 0, N, seed=5137)


def test_scratch_reuse():
    """calls with different n on one stream share the cached scratch buffers: nothing the first call left there (eight quarters
    of one short group id) may show in the later ones (five quarters, all mixed; then no short consensus at all)"""
    _check(8192, 8, _labels(8192, "all_short"), _lens(8), 0, 64, seed=1)
    _check(4100, 8, _labels(4100, "interleaved"), _lens(8), 0, 64, seed=2)
    _check(4100, 8, _labels(4100, "all_full"), _lens(8), 0, 64, seed=3)
