"""GPU parity of the tiled Hamming kernel's last column block (byte-exact vs the oracle's ko_hamdist_rows).

When the last 4-KiB column block holds at most 2048 valid columns (tw = 1 or 2 wave quarters) it is written by packed tail
workgroups that cover 4 / tw row sets each; otherwise by the normal tiles.  Every case pre-fills the output with 0xA5 and checks
that the kernel wrote every byte it owes (rows [row0, row0 + nrows) x columns [0, n)) and nothing else: not the pad bytes
[n, ld) of a written row, not a row outside the range (guard rows in front of and behind the range; 300 behind it, more than
the 256 rows a tail workgroup of the 8-row instantiations spans)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
GUARD_BEFORE, GUARD_AFTER = 8, 300
COL0 = 4096                      # cb = 2: the tail block starts here


def _labels(n, mode):
    """lens = [k, k - 3]: label 0 full length, label 1 a consensus shorter than k, label 2 noise.
    full: no row takes the prefix compare.  handover: the sample's shape, grouped labels with ONE short label whose rows start
    in front of the tail column block and end inside it (in the middle of a lane's 16 columns where the block is wide enough), so
    a group boundary falls inside a tail wave's columns; the same label on rows 3 .. 19 puts prefix-compare rows into the row
    ranges at the top of the matrix."""
    lab = np.zeros(n, np.int32)
    if mode == "full":
        lab[n // 2:] = 2
        return lab
    tail = n - COL0
    end = COL0 + max(1, tail // 2 + 5 if tail > 16 else tail // 2)
    lab[3:20] = 1
    lab[COL0 - 1000:end] = 1
    lab[end:] = 2
    return lab


def _check(n, k, mode, row0, nrows, seed):
    from kmap_amd import _ffi
    from kmap_amd.hamdist import hamdist_matrix_dev, pitch_for
    from kmap_amd.kmer_count import get_hash_dtype
    from oracle import oracle as O
    rng = np.random.default_rng(seed)
    kh = rng.integers(0, 4 ** k, size=n, dtype=np.uint64)
    lab = _labels(n, mode)
    lens = np.array([k, k - 3], np.int32)
    ld = pitch_for(n)
    assert ld % 4096 == 0 and (ld // 4096) % 2 == 1 and ld >= n
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
    O.lib().ko_hamdist_rows(kh, lab, n, k, lens, len(lens), row0, nrows, want)
    mine = got[before:before + nrows]
    np.testing.assert_array_equal(mine[:, :n], want)
    assert np.all(mine[:, n:] == SENTINEL), "pad bytes [n, ld) of a written row were overwritten"
    assert np.all(got[:before] == SENTINEL), "a row in front of the range was written"
    assert np.all(got[before + nrows:] == SENTINEL), "a row behind the range was written"


# tail widths at cb = 2: tw = 1 (1, the benchmark's 848, exactly one wave), tw = 2, tw = 3 (normal tiles), no partial block
WIDTHS = [1, 848, 1024, 1025, 2048, 2049, 4096]


@pytest.mark.parametrize("mode", ["full", "handover"])
@pytest.mark.parametrize("k", [8, 12, 16])          # <1,4>, <0,8>, <2,8> (k = 16 through the u64 entry)
@pytest.mark.parametrize("tail", WIDTHS)
def test_tail_widths(tail, k, mode):
    # rows 3090 .. 3289: full-length rows, then (handover) the short label's rows; 200 rows fill no tail workgroup evenly
    _check(COL0 + tail, k, mode, 3090, 200, seed=1000 * k + tail)


@pytest.mark.parametrize("k", [8, 12, 16])
@pytest.mark.parametrize("tail", [848, 2048])       # m = 4 and m = 2 row sets per tail workgroup
@pytest.mark.parametrize("row0", [0, 5])
@pytest.mark.parametrize("nrows", [1, 31, 33, 127, 130])
def test_row_ranges(nrows, row0, tail, k):
    """the last tail workgroup has fewer than m row sets, and the last row set fewer than R rows"""
    _check(COL0 + tail, k, "handover", row0, nrows, seed=7 * nrows + row0 + tail + k)


def test_full_height():
    """n = 3 full column blocks + the benchmark's tail, all rows, k = 8: 64 seeded rows against the oracle"""
    from kmap_amd import _ffi
    from kmap_amd.hamdist import hamdist_matrix_dev, pitch_for
    from oracle import oracle as O
    n, k = 12_288 + 848, 8
    rng = np.random.default_rng(13136)
    kh = rng.integers(0, 4 ** k, size=n, dtype=np.uint64)
    lab = np.sort(rng.integers(0, 3, size=n)).astype(np.int32)
    lens = np.array([8, 7], np.int32)
    ld = pitch_for(n)
    kh_d, lab_d = _ffi.DeviceBuffer.from_numpy(kh.astype(np.uint32)), _ffi.DeviceBuffer.from_numpy(lab)
    out_d = _ffi.DeviceBuffer(n * ld)
    _ffi.check(_ffi.lib().kmap_memset(out_d.ptr, SENTINEL, n * ld, None))
    hamdist_matrix_dev(kh_d.ptr, lab_d.ptr, n, k, lens, out_d.ptr, ld)
    rows = np.unique(np.concatenate([[0, 7, 8, n - 1], rng.integers(0, n, size=60)]))
    while len(rows) < 64:
        rows = np.unique(np.concatenate([rows, rng.integers(0, n, size=64 - len(rows))]))
    want = np.empty((1, n), np.uint8)
    for r in rows:
        got = out_d.to_numpy(np.uint8, (ld,), offset=int(r) * ld)
        O.lib().ko_hamdist_rows(kh, lab, n, k, lens, len(lens), int(r), 1, want)
        np.testing.assert_array_equal(got[:n], want[0], err_msg=f"row {r}")
        assert np.all(got[n:] == SENTINEL), f"pad bytes of row {r} were overwritten"
    for b in (out_d, kh_d, lab_d):
        b.free()
