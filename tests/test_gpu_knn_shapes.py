"""The smoothing stage at its edges: neighbour selection (knn_select_kernel), the matrix-based neighbour sums (csrc/knn_smooth.hip)
and the profile / MFMA / v_dot4 sums (csrc/knn_profile.hip) against a CPU reference that shares nothing with a device kernel.

    sums[i, j] = sum_{a in nb[i], b in nb[j]} D[a, b]           exact integers: every comparison here is assert_array_equal

Reference (int64): M[i] = sum_a D[nb[i, a], :], want[i] = M[i][nb].sum(axis=1) -- the factored form of A[rows] @ D @ A.T with
A[i, nb[i, a]] += 1 (`test_reference_forms_agree` ties the two).  Small n compares whole outputs, with D from the oracle
(`oracle.hamdist_matrix_u8`) or built on the host; large n compares sampled rows, the rows of D they need coming from the oracle's
`ko_hamdist_rows` while the device builds its own matrix from the k-mers (`hamdist_matrix_dev`, pinned by its own tests).

Neighbour tables are random (indices repeat).  Every case plants rows whose neighbours are all one index: a pair of rows whose
sum is n_nb^2 * max(D), the largest value every accumulator of that case can hold, and a pair whose sum is 0.

`knn_sums_path` / `profile_form` restate the dispatch arithmetic of the two entry points, and every case asserts the path it is
meant to take: a later change of those constants then shows up as a failing expectation here, not as silently lost coverage.
Outputs are written into sentinel-filled buffers: pad columns [n, lds) and rows outside the requested range must stay untouched."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5                                                        # every byte of an output buffer before the launch
SENT16 = 0xA5A5


@pytest.fixture(scope="module")
def V():
    import kmap_amd.visualization as vz
    return vz


# ---- dispatch mirrors -----------------------------------------------------------------------------------------------------------
def knn_sums_path(n, n_nb, dmax):
    """kmap_knn_sums_u8_dev: (kernel, rows per block, LDS sum type, index type, column chunks)."""
    m8 = dmax * n_nb <= 255
    pitch = (n + 15) // 16 * 16
    rows = min(4, (150 * 1024) // (pitch * (1 if m8 else 2)))
    if rows >= 2:
        return "rows", rows, "u8" if m8 else "u16", "u16" if n <= 65536 else "i32", 1
    chunk = min(pitch, 65536)
    return "one_row", 1, "u16", "i32", -(-n // chunk)


def profile_form(n_nb, k, lens):
    """kmap_knn_sums_kmers_*_dev: None (refused), else (kernel, short-consensus groups, profile dwords per k-mer)."""
    short = [c for c in lens if c < k]
    if k < 1 or k > 16 or n_nb > 255 or n_nb * n_nb * k > 65535 or len(short) > 4:
        return None
    mfma = n_nb <= 127 and all(k - c <= 4 * c for c in short)
    return "mfma" if mfma else "dot4", len(short), 8 if k <= 8 else 16


# ---- reference --------------------------------------------------------------------------------------------------------------------
def ref_sums(D, nb, rows):
    """int64 sums of `rows` (natural diagonal) from a host matrix D [n, n] and the neighbour table nb [n, n_nb]."""
    rows = np.asarray(rows)
    out = np.empty((len(rows), len(D)), np.int64)
    for a in range(0, len(rows), 64):
        M = D[nb[rows[a:a + 64]]].sum(axis=1, dtype=np.int64)         # [rows, n]
        out[a:a + 64] = M[:, nb].sum(axis=2)
    return out


def zero_diag(want, rows):
    want = want.copy()
    want[np.arange(len(rows)), np.asarray(rows)] = 0
    return want


def ref_sums_row_from_kmers(kh64, lab, k, cl, nb, i):
    """One row (natural diagonal) without a host matrix: the rows of D come from the oracle one at a time."""
    from oracle import oracle as O
    n = len(kh64)
    buf = np.empty((1, n), np.uint8)
    M = np.zeros(n, np.int64)
    for r, cnt in zip(*np.unique(nb[i], return_counts=True)):
        O.lib().ko_hamdist_rows(kh64, lab, n, k, cl, len(cl), int(r), 1, buf)
        M += int(cnt) * buf[0].astype(np.int64)
    return M[nb].sum(axis=1)


def test_reference_forms_agree():
    rng = np.random.default_rng(1)
    n, n_nb = 100, 7
    D = rng.integers(0, 256, size=(n, n), dtype=np.uint8)
    nb = rng.integers(0, n, size=(n, n_nb)).astype(np.int32)
    A = np.zeros((n, n), np.int64)
    np.add.at(A, (np.repeat(np.arange(n), n_nb), nb.ravel()), 1)
    np.testing.assert_array_equal(ref_sums(D, nb, np.arange(n)), A @ D.astype(np.int64) @ A.T)


# ---- device helpers ---------------------------------------------------------------------------------------------------------------
def _filled(nbytes):
    from kmap_amd import _ffi
    buf = _ffi.DeviceBuffer(nbytes)
    _ffi.check(_ffi.lib().kmap_memset(buf.ptr, SENTINEL, nbytes, None))
    return buf


def _read_rows(launch, n, nrows, lds):
    """launch(dst) fills [nrows x lds] uint16 at dst; -> the rows' n columns, after checking that the pad columns and one guard row
    in front of and behind the block still hold the sentinel.  launch may return None (request refused): passed on."""
    out_d = _filled((nrows + 2) * lds * 2)
    res = launch(out_d.ptr + lds * 2)
    if res is None:
        out_d.free()
        return None
    got = out_d.to_numpy(np.uint16, (nrows + 2, lds))
    out_d.free()
    assert np.all(got[0] == SENT16) and np.all(got[-1] == SENT16), "a row outside the requested range was written"
    assert np.all(got[1:-1, n:] == SENT16), "pad columns [n, lds) were written"
    return got[1:-1, :n]


def matrix_sums(V, D_d, ldd, nb_d, n, n_nb, row0, nrows):
    lds = (n + 127) & ~127
    return _read_rows(lambda dst: V.knn_sums_dev(D_d.ptr, ldd, nb_d, n, n_nb, row0=row0, nrows=nrows, out=dst), n, nrows, lds)


def profile_sums(V, kh_d, lab_d, n, k, lens, nb_d, n_nb, row0, nrows, natural):
    lds = (n + 127) & ~127
    return _read_rows(lambda dst: V.knn_sums_kmers_dev(kh_d.ptr, lab_d.ptr, n, k, lens, nb_d, n_nb, row0=row0, nrows=nrows, out=dst,
                                                       natural_diag=natural), n, nrows, lds)


def _upload_matrix(D):
    from kmap_amd import _ffi
    from kmap_amd.hamdist import pitch_for
    n = len(D)
    ldd = pitch_for(n)
    Dp = np.full((n, ldd), 0xEE, np.uint8)                             # pitch padding holds garbage
    Dp[:, :n] = D
    return _ffi.DeviceBuffer.from_numpy(Dp), ldd


def _row_ranges(n, wanted):
    return [(0, n)] + [(r0, nr) for r0, nr in wanted if r0 >= 0 and r0 + nr <= n and (r0, nr) != (0, n)]


# =====================================================================================================================================
# 1. matrix-based sums
# =====================================================================================================================================
@pytest.mark.parametrize("n,n_nb,hi,path", [
    (1, 1, 200, ("rows", 4, "u8", "u16", 1)),                          # the smallest matrix
    (15, 7, 36, ("rows", 4, "u8", "u16", 1)),                          # one lane, ragged edge only
    (16, 7, 36, ("rows", 4, "u8", "u16", 1)),                          # one lane, one 16-byte load
    (17, 7, 36, ("rows", 4, "u8", "u16", 1)),                          # a vector lane and a ragged one
    (100, 17, 15, ("rows", 4, "u8", "u16", 1)),                        # dmax * n_nb = 255: the last byte-sum case, planted byte 255
    (100, 16, 16, ("rows", 4, "u16", "u16", 1)),                       # dmax * n_nb = 256: the first 16-bit case
    (257, 51, 5, ("rows", 4, "u8", "u16", 1)),                         # byte sums with n_nb well above 20
    (600, 255, 1, ("rows", 4, "u8", "u16", 1)),                        # byte sum 255, final sum 65 025
    (600, 16, 255, ("rows", 4, "u16", "u16", 1)),                      # 16-bit fields at 16 * 255, final sum 65 280
])
def test_matrix_sums_small(V, n, n_nb, hi, path):
    """Host-built byte matrices (not symmetric, diagonal not zero: the kernel may assume neither), whole output and the row
    ranges (3, 5) and (n - 1, 1), whose last group holds fewer rows than the kernel's R."""
    from kmap_amd import _ffi
    rng = np.random.default_rng(1000 * n + n_nb)
    D = rng.integers(0, hi + 1, size=(n, n), dtype=np.uint8)
    nb = rng.integers(0, n, size=(n, n_nb)).astype(np.int32)
    if n >= 8:
        a, b, c = n - 1, n - 2, n - 3
        D[a, b], D[c, c] = hi, 0
        nb[3], nb[n - 1], nb[4], nb[0] = a, b, c, c                    # rows 3 and 4 lie in every checked range but the last
    D[0, 0] = hi                                                       # max(D) is hi in every case
    assert knn_sums_path(n, n_nb, int(D.max())) == path
    want = ref_sums(D, nb, np.arange(n))
    if n >= 8:
        assert want[3, n - 1] == n_nb * n_nb * hi and want[4, 0] == 0
    want = zero_diag(want, np.arange(n))
    assert want.max() <= 65535
    D_d, ldd = _upload_matrix(D)
    nb_d = _ffi.DeviceBuffer.from_numpy(nb)
    for r0, nr in _row_ranges(n, ((3, 5), (n - 1, 1))):
        got = matrix_sums(V, D_d, ldd, nb_d, n, n_nb, r0, nr)
        np.testing.assert_array_equal(got, want[r0:r0 + nr], err_msg=f"rows [{r0}, {r0 + nr})")
    D_d.free()
    nb_d.free()


def _kmers(rng, n, k, lens, shuffle=False, stray_labels=False):
    """-> kh (hash dtype of k), lab int32, nb-ready planted indices (a, b, c): kh[a] and kh[b] differ in all k bases and are noise
    (D[a, b] = k, the matrix maximum); c carries the first short consensus' label where there is one."""
    from kmap_amd.kmer_count import get_hash_dtype
    n_lab = len(lens)
    kh = rng.integers(0, 4 ** k, size=n, dtype=np.uint64)
    kh[::9] = kh[0]                                                    # duplicates, as in expanded samples
    lab = rng.integers(0, n_lab + 1, size=n).astype(np.int32)          # n_lab: noise
    if not shuffle:
        lab.sort()
    a = b = c = None
    if n >= 8:
        a, b = n - 1, n - 2
        kh[a], kh[b] = 0, 4 ** k - 1
        lab[a] = lab[b] = n_lab
        short = [g for g, cl in enumerate(lens) if cl < k]
        cand = np.flatnonzero(lab[:n - 2] == short[0]) if short else []
        c = int(cand[len(cand) // 2]) if len(cand) else n // 2
    if stray_labels:                                                   # labels outside [0, n_lab) count as noise
        noise = np.flatnonzero(lab == n_lab)
        lab[noise[0::3]] = -1
        lab[noise[1::3]] = n_lab + 7
    return kh.astype(get_hash_dtype(k)), lab, (a, b, c)


@pytest.mark.parametrize("n,k,lens,path,ranges", [
    (19_261, 20, [20, 13], ("rows", 3, "u16", "u16", 1), ((0, 3), (9_630, 2), (19_258, 3))),
    (25_661, 20, [20], ("rows", 2, "u16", "u16", 1), ((0, 3), (12_830, 2), (25_658, 3))),
    (38_461, 20, [20, 6], ("one_row", 1, "u16", "i32", 1), ((0, 2), (19_230, 2), (38_459, 2))),
    (65_603, 20, [20], ("one_row", 1, "u16", "i32", 2), ((0, 2), (65_535, 2), (65_601, 2))),     # accumulation across c0 > 0
    (40_013, 8, [8], ("rows", 3, "u8", "u16", 1), ((0, 3), (20_006, 2), (40_010, 3))),
    (65_603, 8, [8, 5], ("rows", 2, "u8", "i32", 1), ((0, 2), (65_535, 2), (65_600, 3))),         # int32 indices in the rows kernel
    (76_819, 8, [8], ("one_row", 1, "u16", "i32", 2), ((0, 2), (65_535, 2), (76_817, 2))),        # one-row kernel from byte-sized inputs
])
def test_matrix_sums_large_sampled_rows(V, n, k, lens, path, ranges):
    """The 16-bit-sum instantiations, R = 2 and 3, int32 indices and the one-row chunked kernel, none of which a small matrix
    reaches: the device builds D from the k-mers, a few short row ranges (first, middle, last; rows 65 535 and 65 536 where n
    allows) are requested and every row of them is compared."""
    from kmap_amd import _ffi
    from kmap_amd.hamdist import hamdist_matrix_dev, pitch_for
    n_nb = 20
    rng = np.random.default_rng(n + k)
    kh, lab, (a, b, c) = _kmers(rng, n, k, lens)
    nb = rng.integers(0, n, size=(n, n_nb)).astype(np.int32)
    nb[0], nb[n // 2], nb[1], nb[7] = a, b, c, c
    assert knn_sums_path(n, n_nb, k) == path                           # max(D) = k: kh[a] and kh[b] differ everywhere
    kh_d, lab_d, nb_d = (_ffi.DeviceBuffer.from_numpy(x) for x in (kh, lab, nb))
    ldd = pitch_for(n)
    D_d = _ffi.DeviceBuffer(n * ldd)
    hamdist_matrix_dev(kh_d.ptr, lab_d.ptr, n, k, lens, D_d.ptr, ldd)
    got = {r0: matrix_sums(V, D_d, ldd, nb_d, n, n_nb, r0, nr) for r0, nr in ranges}
    for buf in (D_d, kh_d, lab_d, nb_d):
        buf.free()
    kh64, cl = np.ascontiguousarray(kh, np.uint64), np.asarray(lens, np.int32)
    for r0, nr in ranges:
        for i in range(r0, r0 + nr):
            want = ref_sums_row_from_kmers(kh64, lab, k, cl, nb, i)
            if i == 0:
                assert want[n // 2] == n_nb * n_nb * k
            if i == 1:
                assert want[7] == 0
            want[i] = 0
            np.testing.assert_array_equal(got[r0][i - r0], want, err_msg=f"row {i}")


def test_matrix_sums_second_trip_of_the_group_loop(V):
    """nrows = n = 8300 > 2048 blocks * 4 rows: groups 2048.. are a block's second trip through its loop (rows 8192..)."""
    from kmap_amd import _ffi
    from kmap_amd.hamdist import hamdist_matrix_dev, pitch_for
    n, k, lens, n_nb = 8300, 12, [12, 7], 20
    rng = np.random.default_rng(n)
    kh, lab, (a, b, c) = _kmers(rng, n, k, lens)
    nb = rng.integers(0, n, size=(n, n_nb)).astype(np.int32)
    nb[8192], nb[0], nb[8191], nb[8299] = a, b, c, c
    assert knn_sums_path(n, n_nb, k) == ("rows", 4, "u8", "u16", 1) and -(-n // 4) > 2048
    kh_d, lab_d, nb_d = (_ffi.DeviceBuffer.from_numpy(x) for x in (kh, lab, nb))
    ldd, lds = pitch_for(n), (n + 127) & ~127
    D_d = _ffi.DeviceBuffer(n * ldd)
    hamdist_matrix_dev(kh_d.ptr, lab_d.ptr, n, k, lens, D_d.ptr, ldd)
    out_d = _filled(n * lds * 2)
    V.knn_sums_dev(D_d.ptr, ldd, nb_d, n, n_nb, out=out_d.ptr)
    kh64, cl = np.ascontiguousarray(kh, np.uint64), np.asarray(lens, np.int32)
    for i in (0, 8191, 8192, 8299):
        got = out_d.to_numpy(np.uint16, (lds,), offset=i * lds * 2)
        want = ref_sums_row_from_kmers(kh64, lab, k, cl, nb, i)
        if i == 8192:
            assert want[0] == n_nb * n_nb * k
        if i == 8191:
            assert want[8299] == 0
        want[i] = 0
        np.testing.assert_array_equal(got[:n], want, err_msg=f"row {i}")
        assert np.all(got[n:] == SENT16)
    for buf in (D_d, kh_d, lab_d, nb_d, out_d):
        buf.free()


# =====================================================================================================================================
# 2. profile sums
# =====================================================================================================================================
def _check_profile(V, n, k, lens, n_nb, form, seed, shuffle=False, stray_labels=False, ranges=((5, 1), (31, 33))):
    """Whole output and row ranges whose row0 / nrows are no multiples of 32, with the reference's zero diagonal and with the
    natural one, against the int64 reference on the oracle's matrix."""
    from kmap_amd import _ffi
    from oracle import oracle as O
    assert profile_form(n_nb, k, lens) == form
    rng = np.random.default_rng(seed)
    kh, lab, (a, b, c) = _kmers(rng, n, k, lens, shuffle=shuffle, stray_labels=stray_labels)
    nb = rng.integers(0, n, size=(n, n_nb)).astype(np.int32)
    if n >= 8:
        nb[5], nb[1], nb[6], nb[2] = a, b, c, c
    D = O.hamdist_matrix_u8(kh, lab, k, lens)
    natural = ref_sums(D, nb, np.arange(n))
    if n >= 8:
        assert natural[5, 1] == n_nb * n_nb * k and natural[6, 2] == 0
    want = {True: natural, False: zero_diag(natural, np.arange(n))}
    kh_d, lab_d, nb_d = (_ffi.DeviceBuffer.from_numpy(x) for x in (kh, lab, nb))
    for r0, nr in _row_ranges(n, ranges):
        for nat in (False, True):
            got = profile_sums(V, kh_d, lab_d, n, k, lens, nb_d, n_nb, r0, nr, nat)
            assert got is not None, _ffi.last_error()
            np.testing.assert_array_equal(got, want[nat][r0:r0 + nr], err_msg=f"rows [{r0}, {r0 + nr}), natural_diag={nat}")
    for buf in (kh_d, lab_d, nb_d):
        buf.free()


@pytest.mark.parametrize("short", [0, 1], ids=["plain", "short"])     # without / with a consensus three bases shorter than k
@pytest.mark.parametrize("k", [8, 12])                                 # one MFMA per tile, two
@pytest.mark.parametrize("n", [1, 31, 32, 33, 255, 256, 257, 1023, 1024, 1025, 2049])
def test_profile_sums_sizes(V, n, k, short):
    """n below one 32 x 32 tile, at the 256-column strip and the 1024-column block edges, and in a second block."""
    _check_profile(V, n, k, [k, k - 3][:1 + short], 20, ("mfma", short, 8 if k == 8 else 16), seed=10 * n + k + short,
                   ranges=((5, 1), (31, 33), (n - 1, 1)))


@pytest.mark.parametrize("k", [1, 4, 8, 9, 15, 16])                    # 9: sixteen profile dwords, seven of them padding
def test_profile_sums_k(V, k):
    _check_profile(V, 300, k, [k], 20, ("mfma", 0, 8 if k <= 8 else 16), seed=k)


@pytest.mark.parametrize("n_nb,k,form", [
    (1, 8, "mfma"), (20, 8, "mfma"),
    (63, 16, "mfma"),                                                  # n_nb^2 k = 63 504, just inside the limit
    (127, 4, "mfma"),                                                  # planted rows: counters of 127, negated to -127 in a group
    (128, 3, "dot4"), (181, 2, "dot4"),
    (255, 1, "dot4"),                                                  # planted rows: a byte counter of 255
])
def test_profile_sums_n_nb(V, n_nb, k, form):
    _check_profile(V, 300, k, [k], n_nb, (form, 0, 8 if k <= 8 else 16), seed=100 * n_nb + k)
    if k > 1:                                                          # and with a short consensus that keeps the form
        _check_profile(V, 290, k, [k, (k + 1) // 2], n_nb, (form, 1, 8 if k <= 8 else 16), seed=100 * n_nb + k + 1)


@pytest.mark.parametrize("n_nb,k", [(256, 1), (64, 16), (20, 17)])
def test_profile_sums_refuses(V, n_nb, k):
    """Outside the profile kernel's range the wrapper returns None (the caller then takes the matrix) and writes nothing."""
    from kmap_amd import _ffi
    from kmap_amd.kmer_count import get_hash_dtype
    n = 300
    assert profile_form(n_nb, k, [k]) is None
    rng = np.random.default_rng(k)
    kh = rng.integers(0, 4 ** k, size=n, dtype=np.uint64).astype(get_hash_dtype(k))
    nb = rng.integers(0, n, size=(n, n_nb)).astype(np.int32)
    kh_d, lab_d, nb_d = (_ffi.DeviceBuffer.from_numpy(x) for x in (kh, np.zeros(n, np.int32), nb))
    lds = (n + 127) & ~127
    out_d = _filled(n * lds * 2)
    assert V.knn_sums_kmers_dev(kh_d.ptr, lab_d.ptr, n, k, [k], nb_d, n_nb, out=out_d.ptr) is None
    assert np.all(out_d.to_numpy(np.uint8, (n * lds * 2,)) == SENTINEL)
    for buf in (kh_d, lab_d, nb_d, out_d):
        buf.free()


@pytest.mark.parametrize("shuffle", [False, True], ids=["sorted", "shuffled"])
@pytest.mark.parametrize("k,lens,form", [
    (15, [15, 3], ("mfma", 1, 16)),                                    # tail 12 = 4 * 3: the last MFMA case
    (16, [16, 3], ("dot4", 1, 16)),                                    # tail 13 > 4 * 3
    (5, [5, 1], ("mfma", 1, 8)),                                       # the tail fills all four byte slots of the single position
    (12, [12, 9, 7, 5, 3], ("mfma", 4, 16)),                           # four groups: four more MFMA pairs per tile
    (8, [8, 1, 1, 1, 1], ("dot4", 4, 8)),                              # four groups on v_dot4: 64 KiB of dynamic LDS, 8 columns per lane
    (16, [16, 3, 3, 3, 3], ("dot4", 4, 16)),                           # the same 64 KiB with 4 columns per lane
])
def test_profile_sums_short_consensuses(V, k, lens, form, shuffle):
    """The short-consensus rule at its limits; shuffled labels also carry values outside [0, n_lab), which count as noise."""
    _check_profile(V, 523, k, lens, 20, form, seed=sum(lens) + 2 * k, shuffle=shuffle, stray_labels=shuffle)


@pytest.mark.parametrize("k,lens,form", [(8, [8, 5], ("mfma", 1, 8)), (8, [8, 1], ("dot4", 1, 8))])
def test_profile_sums_unaligned_output(k, lens, form):
    """Raw entry point with lds = n odd and the output one uint16 behind a 16-byte boundary: the scalar store path of both forms
    (and 4 columns per lane on v_dot4 at k <= 8).  Nothing but rows x [0, n) may be written."""
    from kmap_amd import _ffi
    from oracle import oracle as O
    n, n_nb, r0, nr = 301, 20, 5, 70
    assert profile_form(n_nb, k, lens) == form
    rng = np.random.default_rng(k + len(form[0]))
    kh, lab, (a, b, c) = _kmers(rng, n, k, lens)
    nb = rng.integers(0, n, size=(n, n_nb)).astype(np.int32)
    nb[5], nb[1], nb[6], nb[2] = a, b, c, c
    want = zero_diag(ref_sums(O.hamdist_matrix_u8(kh, lab, k, lens), nb, np.arange(r0, r0 + nr)), np.arange(r0, r0 + nr))
    assert want[0, 1] == n_nb * n_nb * k and want[1, 2] == 0
    kh_d, lab_d, nb_d = (_ffi.DeviceBuffer.from_numpy(x) for x in (kh, lab, nb))
    total = 1 + nr * n + 2 * n                                         # one uint16 in front, two guard rows behind
    out_d = _filled(total * 2)
    assert out_d.ptr % 16 == 0
    clen = np.asarray(lens, np.int32)
    _ffi.check(_ffi.lib().kmap_knn_sums_kmers_u32_dev(kh_d.ptr, lab_d.ptr, n, k, _ffi.ptr(clen), len(clen), nb_d.ptr, n_nb, r0, nr,
                                                      out_d.ptr + 2, n, None))
    _ffi.sync()
    got = out_d.to_numpy(np.uint16, (total,))
    for buf in (kh_d, lab_d, nb_d, out_d):
        buf.free()
    np.testing.assert_array_equal(got[1:1 + nr * n].reshape(nr, n), want)
    assert got[0] == SENT16 and np.all(got[1 + nr * n:] == SENT16), "written outside rows x [0, n)"


# =====================================================================================================================================
# 3. selection
# =====================================================================================================================================
def _select(V, D, n_nb, row0=0, nrows=None):
    from kmap_amd import _ffi
    n = len(D)
    nrows = n - row0 if nrows is None else nrows
    D_d, ldd = _upload_matrix(D)
    out_d = _filled((nrows + 1) * n_nb * 4)
    _ffi.check(_ffi.lib().kmap_knn_select_u8_dev(D_d.ptr, ldd, n, n_nb, row0, nrows, out_d.ptr, None))
    _ffi.sync()
    got = out_d.to_numpy(np.int32, (nrows + 1, n_nb))
    D_d.free()
    out_d.free()
    assert np.all(got[-1].view(np.uint8) == SENTINEL), "written behind the requested rows"
    return np.sort(got[:-1], axis=1)


@pytest.mark.parametrize("hi", [9, 256], ids=["lt32", "bytes"])        # lane-private counters / the generic histogram path
@pytest.mark.parametrize("n,n_nb,row0,nrows", [(100, 1, 0, 100), (5, 5, 0, 5), (63, 20, 0, 63), (64, 20, 0, 64), (65, 20, 0, 65),
                                               (65, 20, 2, 5)])       # (2, 5): a second block with one live wave
def test_select_small(V, n, n_nb, row0, nrows, hi):
    from oracle import oracle as O
    rng = np.random.default_rng(n + n_nb + hi)
    D = rng.integers(0, hi, size=(n, n), dtype=np.uint8)
    np.testing.assert_array_equal(_select(V, D, n_nb, row0, nrows), np.sort(O.knn_select_stable(D, n_nb)[row0:row0 + nrows], axis=1))


@pytest.mark.parametrize("base", [9, 200], ids=["lt32", "bytes"])
@pytest.mark.parametrize("n", [1024, 1031])                            # the last column in a full 1024-entry step / in the ragged one
def test_select_ties_and_last_column(V, n, base):
    """Constant rows (all ties: the quota is filled from index order alone) and rows whose n_nb-th entry is the very last column."""
    from oracle import oracle as O
    n_nb = 20
    rng = np.random.default_rng(n + base)
    D = np.full((n, n), base, np.uint8)
    D[1] = 0
    for r in (2, 3, 4):                                                # n_nb - 1 small entries somewhere, the n_nb-th in the last column
        D[r, rng.choice(n - 2, size=n_nb - 1, replace=False)] = base - 2
        D[r, n - 1] = base - 1
    D[4, n - 2] = base - 1                                             # a tie for the last place: the lower index wins, not the last column
    got = _select(V, D, n_nb)
    want = np.sort(O.knn_select_stable(D, n_nb), axis=1)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(got[0], np.arange(n_nb))
    assert got[2, -1] == n - 1 and got[3, -1] == n - 1 and got[4, -1] == n - 2


# =====================================================================================================================================
# 4. sums beyond uint16
# =====================================================================================================================================
def test_knn_smooth_sums_beyond_uint16(V):
    """n_nb^2 * max(D) > 65535: the integer path's uint16 sums cannot hold the result; knn_smooth() must give the reference's
    answer (the float operator) and kmap() must run on it.  Sums of 400 values <= 255 are exact in float32 in any order."""
    from oracle import oracle as O
    rng = np.random.default_rng(64)
    n, n_nb, k = 64, 20, 8
    D = rng.integers(200, 256, size=(n, n)).astype(np.int64)
    D = np.triu(D, 1)
    D = D + D.T
    nb = rng.integers(0, n, size=(n, n_nb)).astype(np.int32)
    exact = zero_diag(ref_sums(D, nb, np.arange(n)), np.arange(n))
    assert exact.max() > 65535
    S = V.knn_smooth(D, n_nb, neighbor_inds_mat=nb)
    assert S.dtype == np.float32
    np.testing.assert_array_equal(S, O.knn_smooth(D, n_nb, nb=nb))
    np.testing.assert_array_equal(S, (exact.astype(np.float32) / np.float32(n_nb)) / np.float32(n_nb))
    T = V.sigmoid(S, 16.0, change_point=k / 2, scale_factor=0.2 * k - 0.2)
    a = V.umap(T, n_max_iter=1, random_seed=5, debug=False, mode=V.EMBED_SEQ)
    b = V.kmap(D, k, n_neighbour=n_nb, n_max_iter=1, random_seed=5, debug=False, mode=V.EMBED_SEQ, neighbor_inds_mat=nb)
    assert b.shape == (2, n) and np.all(np.isfinite(b))
    np.testing.assert_array_equal(a, b)
