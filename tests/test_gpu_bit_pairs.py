"""kmap_bitrows_pair_counts_dev alone (csrc/bit_pairs.hip): any bit matrix is a legal input, so its edges are
tested without reads.  The planes go up from numpy through _ffi.DeviceBuffer; the result must equal the matrix product of the
unpacked bits (tests/_cooccurrence_model.py) as integers, be symmetric and hold the row popcounts on its diagonal."""
import numpy as np
import pytest

from kmap_amd.device_seq import BIT_PAIRS_K as K, BIT_PAIRS_MIN_SLICE as SLICE
from tests import _cooccurrence_model as CM

pytestmark = pytest.mark.gpu

# 625 words = 4 slices of 128 words and a remainder of 113 = 3 staging steps and 17 words: the split of csrc/bit_pairs.hip asks for
# about 16 blocks per CU, far more than these sizes give, so a slice is the smallest one
LONG = 4 * SLICE + 3 * K + 17
ROWS = (1, 2, 63, 64, 65, 130)
WORDS = (1, K - 1, K, K + 1, LONG)


def pair_counts(planes):
    from kmap_amd import _ffi
    from kmap_amd.device_seq import bitrows_pair_counts
    planes = np.ascontiguousarray(planes, np.uint64)
    buf = _ffi.DeviceBuffer.from_numpy(planes) if planes.size else _ffi.DeviceBuffer(8)
    try:
        return bitrows_pair_counts(buf, planes.shape[0], planes.shape[1])
    finally:
        buf.free()


def check(planes):
    planes = np.ascontiguousarray(planes, np.uint64)
    got = pair_counts(planes)
    bits = CM.np_unpack(planes)
    assert got.dtype == np.int64 and got.shape == (len(planes),) * 2
    np.testing.assert_array_equal(got, CM.np_pair_counts(bits))
    np.testing.assert_array_equal(got, got.T)
    np.testing.assert_array_equal(np.diagonal(got), bits.sum(axis=1))
    return got


def random_planes(rng, n_mat, n_words, density):
    return CM.np_pack(rng.random((n_mat, n_words * 64)) < density)


def test_geometry_of_the_cases():
    assert LONG == 625 and (LONG + SLICE - 1) // SLICE >= 3 and LONG % SLICE != 0 and LONG % K != 0
    assert 130 * LONG * 64 < 130 * 41_000


@pytest.mark.parametrize("n_words", WORDS)
@pytest.mark.parametrize("n_mat", ROWS)
def test_random_bits(n_mat, n_words):
    rng = np.random.default_rng(2100 + 1000 * n_mat + n_words)
    dense = check(random_planes(rng, n_mat, n_words, 0.5))
    assert dense.max() > 0
    check(random_planes(rng, n_mat, n_words, 0.02))


@pytest.mark.parametrize("n_mat,n_words", [(130, LONG), (65, K + 1), (2, 1)])
def test_special_contents(n_mat, n_words):
    rng = np.random.default_rng(2101)
    ones = np.full((n_mat, n_words), 2 ** 64 - 1, np.uint64)
    assert (check(ones) == n_words * 64).all()                                  # every count is the bit length
    assert not check(np.zeros((n_mat, n_words), np.uint64)).any()
    sparse = random_planes(rng, n_mat, n_words, 0.02)
    sparse[n_mat // 2] = 2 ** 64 - 1                                            # one row of all ones among sparse rows
    got = check(sparse)
    np.testing.assert_array_equal(got[n_mat // 2], np.where(np.arange(n_mat) == n_mat // 2, n_words * 64, np.diagonal(got)))
    if n_mat >= 2:
        twin = random_planes(rng, n_mat, n_words, 0.3)
        twin[n_mat - 1] = twin[0]                                               # row i equal to row j, in different tiles when n_mat > 64
        got = check(twin)
        assert got[0, n_mat - 1] == got[0, 0] == got[n_mat - 1, n_mat - 1]
        np.testing.assert_array_equal(got[0], got[n_mat - 1])


def test_single_bits_at_the_ends_of_rows_and_slices():
    """rows whose only set bits sit in the first word, the last word, and the last word of a slice and the first of the next"""
    n_mat = 130
    places = [(0, 0), (0, 63), (LONG - 1, 0), (LONG - 1, 63), (SLICE - 1, 63), (SLICE, 0), (2 * SLICE - 1, 5), (K - 1, 63), (K, 0),
              (4 * SLICE + 3 * K - 1, 63), (4 * SLICE + 3 * K, 0)]
    planes = np.zeros((n_mat, LONG), np.uint64)
    for r in range(n_mat):
        w, b = places[r % len(places)]
        planes[r, w] = np.uint64(1) << np.uint64(b)
    got = check(planes)
    assert (np.diagonal(got) == 1).all() and got[0, len(places)] == 1 and got[0, 1] == 0 and got[64, 64 + len(places)] == 1
    both = planes.copy()
    both[7] |= both[129]                                                        # two bits, in different slices
    assert check(both)[7, 129] == 1


def test_two_calls_give_the_same_matrix():
    rng = np.random.default_rng(2102)
    planes = random_planes(rng, 130, LONG, 0.03)
    np.testing.assert_array_equal(pair_counts(planes), pair_counts(planes))


def test_degenerate_sizes_and_errors():
    from kmap_amd import _ffi
    lib = _ffi.lib()
    assert pair_counts(np.zeros((0, 5), np.uint64)).shape == (0, 0)
    got = pair_counts(np.zeros((3, 0), np.uint64))
    assert got.shape == (3, 3) and not got.any()
    buf = _ffi.DeviceBuffer(8 * 4)
    try:
        out = np.full((2, 2), 7, np.uint64)
        assert lib.kmap_bitrows_pair_counts_dev(buf.ptr, 0, 2, _ffi.ptr(out), None) == 0 and (out == 7).all()      # n_mat == 0 writes nothing
        assert lib.kmap_bitrows_pair_counts_dev(buf.ptr, 2, 0, _ffi.ptr(out), None) == 0 and not out.any()         # n_words == 0: zeros
        out[:] = 7
        # more than 4096 rows: refused before anything is read (the buffer holds four words) or launched
        assert lib.kmap_bitrows_pair_counts_dev(buf.ptr, 4097, 1, _ffi.ptr(out), None) == -4 and "4096" in _ffi.last_error()
        assert lib.kmap_bitrows_pair_counts_dev(buf.ptr, 4097, 1, None, None) == -4
        for args in ((None, 2, 2, _ffi.ptr(out)), (buf.ptr, 2, 2, None), (buf.ptr, -1, 2, _ffi.ptr(out)), (buf.ptr, 2, -1, _ffi.ptr(out))):
            assert lib.kmap_bitrows_pair_counts_dev(*args, None) == -1 and "bitrows_pair_counts" in _ffi.last_error()
        assert (out == 7).all()
        with pytest.raises(ValueError, match="4097 rows"):
            from kmap_amd.device_seq import bitrows_pair_counts
            bitrows_pair_counts(buf, 4097, 1)
    finally:
        buf.free()
    # and the next call is as good as the first
    check(random_planes(np.random.default_rng(2103), 5, 3, 0.5))
