"""Both sides of every branch a kernel takes on the alignment of a CALLER's pointer or pitch (`grep -n uintptr_t kmap_amd/csrc`),
against the plain reference, bit for bit.

The Python wrappers only ever hand hipMalloc'ed (256-byte aligned) arrays and padded pitches to the library, so the rest of the
suite runs the vector side of these branches alone.  The C entry points take raw pointers: slices of torch tensors, row blocks
`ptr + row0 * ld`, dense n x n outputs.  Every case here calls the `_ffi.lib()` entry itself with `tests/_footprint.Guarded`
pointers whose `lead` is the misalignment, runs twice (output fill 0xA5 / 0x5A, input guard fill 0x00 / 0xFF, see _footprint),
compares with the reference and checks the guard bands of every array, inputs included.  Shapes are the smallest that reach a
full vector unit, a ragged tail and a second workgroup."""
import ctypes as C

import numpy as np
import pytest

from tests import _footprint as F
from tests._footprint import free, guards, ok
from tests._packed_model import packed_groups, ref_pack

pytestmark = pytest.mark.gpu

KMAP_E_INVAL = -1


@pytest.fixture(scope="module")
def L():
    from kmap_amd import _ffi
    return _ffi.lib()


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


# =====================================================================================================================================
# packed reads: pack_kernel (seq_dev % 16), unpack_kernel, hash_packed_kernel (out % 16; u32, u64, u64 wide)
# =====================================================================================================================================
PACK_N = [1, 15, 16, 17, 33, 4095, 4096, 4097]           # a block is 256 groups of 16: 4096 fills one, 4097 starts a second


def reads_bytes(rng, n, others=True):
    """bases with ~10 % separators (255) and, with `others`, ~5 % bytes from 4..254 (not a base either)"""
    seq = rng.integers(0, 4, size=n, dtype=np.uint8)
    seq[rng.random(n) < 0.10] = 255
    if others:
        m = rng.random(n) < 0.05
        seq[m] = rng.integers(4, 255, size=int(m.sum()), dtype=np.uint8)
        if n >= 4:
            seq[n - 1], seq[n // 2] = 4, 254              # the two ends of the non-base range, one of them in the last position
    return seq


@pytest.mark.parametrize("n", PACK_N)
def test_pack_reads_seq_alignment(L, n):
    """seq_dev lead 0: 16-byte loads for whole groups; leads 1, 4, 15: byte loads.  All kmap_packed_groups(n) groups are compared,
    the halo included, and nothing behind them is written.  The code bits of invalid positions are outside the contract, so the
    reference compares the valid ones; all four leads must give the same words bit for bit."""
    rng = np.random.default_rng(n)
    seq = reads_bytes(rng, n)
    want_c, want_i, valid = ref_pack(seq)
    ng = packed_groups(n)
    assert L.kmap_packed_groups(n) == ng
    words = {}
    for lead in (0, 1, 4, 15):
        def case(out_fill, in_fill):
            s = F.Guarded.of(seq, lead=lead, fill=in_fill, name="seq")
            c, i = F.Guarded(ng * 4, fill=out_fill, name="codes"), F.Guarded(ng * 2, fill=out_fill, name="inval")
            ok(L.kmap_pack_reads_dev(s.ptr, n, c.ptr, i.ptr, None))
            np.testing.assert_array_equal(i.payload(np.uint16), want_i, err_msg=f"inval, lead {lead}")
            np.testing.assert_array_equal(c.payload(np.uint32) & valid, want_c, err_msg=f"codes, lead {lead}")
            words[lead] = c.payload(np.uint32)
            guards(s, c, i)
            free(s)
            return [c, i]
        F.run_twice(case)
        np.testing.assert_array_equal(words[lead], words[0], err_msg=f"codes of lead {lead} differ from the aligned form's")


@pytest.mark.parametrize("lead", [0, 1, 3])
@pytest.mark.parametrize("n", PACK_N)
def test_unpack_reads_out_alignment(L, n, lead):
    """round trip: the input with every non-base byte read back as 255; exactly n bytes written"""
    rng = np.random.default_rng(100 + n)
    seq = reads_bytes(rng, n)
    codes, inval, _ = ref_pack(seq, rng)
    want = np.where(seq > 3, 255, seq).astype(np.uint8)

    def case(out_fill, in_fill):
        c, i = F.Guarded.of(codes, fill=in_fill, name="codes"), F.Guarded.of(inval, fill=in_fill, name="inval")
        out = F.Guarded(n, lead=lead, fill=out_fill, name="seq_out")
        ok(L.kmap_unpack_reads_dev(c.ptr, i.ptr, n, out.ptr, None))
        np.testing.assert_array_equal(out.payload(np.uint8), want)
        guards(c, i, out)
        free(c, i)
        return [out]
    F.run_twice(case)


@pytest.mark.parametrize("k,lead", [(15, 0), (15, 4), (15, 8), (15, 12), (16, 0), (16, 8), (17, 0), (17, 8)])
@pytest.mark.parametrize("n", PACK_N)
def test_hash_kmers_packed_out_alignment(L, O, n, k, lead):
    """out_dev % 16 of the three instantiations (k = 15: uint32, 16: uint64, 17: uint64 with the wide window).  The declared
    input is kmap_packed_groups(n) groups of codes and inval, halo included; the code bits of invalid positions are noise."""
    rng = np.random.default_rng(1000 * k + n)
    seq = reads_bytes(rng, n, others=False)
    if n >= 64:
        seq[20:20 + 2 * k] = 3                            # poly-T windows: at k = 16 the hash is 2^32 - 1, a valid uint64 value
    codes, inval, _ = ref_pack(seq, rng)
    want = O.comp_kmer_hash(seq, k)
    dt = want.dtype

    def case(out_fill, in_fill):
        c, i = F.Guarded.of(codes, fill=in_fill, name="codes"), F.Guarded.of(inval, fill=in_fill, name="inval")
        out = F.Guarded(n * dt.itemsize, lead=lead, fill=out_fill, name="out")
        ok(L.kmap_hash_kmers_packed_dev(c.ptr, i.ptr, n, k, out.ptr, None))
        np.testing.assert_array_equal(out.payload(dt), want)
        guards(c, i, out)
        free(c, i)
        return [out]
    F.run_twice(case)


@pytest.mark.parametrize("k", [1, 15, 16, 31])
@pytest.mark.parametrize("n", [1, 15, 16, 17, 4095, 4096, 4097])      # a block is 256 threads x 16 positions
def test_hash_kmers_unaligned_seq(L, O, n, k):
    """no alignment branch: an odd seq_dev, the tail bound and the footprint of the rolling-window kernel"""
    rng = np.random.default_rng(31 * n + k)
    seq = reads_bytes(rng, n, others=False)
    want = O.comp_kmer_hash(seq, k)
    dt = want.dtype
    fn = L.kmap_hash_kmers_u32_dev if k < 16 else L.kmap_hash_kmers_u64_dev

    def case(out_fill, in_fill):
        s = F.Guarded.of(seq, lead=1, fill=in_fill, name="seq")
        out = F.Guarded(n * dt.itemsize, fill=out_fill, name="out")
        ok(fn(s.ptr, n, k, out.ptr, None))
        np.testing.assert_array_equal(out.payload(dt), want)
        guards(s, out)
        free(s)
        return [out]
    F.run_twice(case)


# =====================================================================================================================================
# Hamming 1-vs-N: ham1vN_kernel (out & 3)
# =====================================================================================================================================
@pytest.mark.parametrize("form", ["full", "head", "tail"])
@pytest.mark.parametrize("k", [11, 21])                                # the uint32 / the uint64 entry
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 1024, 1025])          # a thread owns 4 outputs, a block 1024
def test_hamdist_1vN_out_alignment(L, O, n, k, form):
    """out_dev lead 0: one 32-bit store per thread; leads 1, 2, 3: four byte stores.  Invalid hashes included."""
    rng = np.random.default_rng(97 * n + k)
    dt = O.get_hash_dtype(k)
    h = rng.integers(0, 4 ** k, size=n, dtype=np.uint64).astype(dt)
    h[::5] = O.get_invalid_hash(dt)
    clen = k if form == "full" else k - 4
    cons = int(rng.integers(0, 4 ** clen, dtype=np.uint64))
    if form == "full":
        want, shift = O.cal_hamming_dist(h, cons, k), 0
    elif form == "head":
        want, shift = O.cal_hamming_dist_head(h, cons, k, clen), 2 * (k - clen)
    else:
        want, shift = O.cal_hamming_dist_tail(h, cons, k, clen), 0
    fn =L.kmap_hamdist_1vN_u32_dev if dt == np.uint32 else L.kmap_hamdist_1vN_u64_dev
    for lead in (0, 1, 2, 3):
        def case(out_fill, in_fill):
            hd = F.Guarded.of(h, fill=in_fill, name="h")
            out = F.Guarded(n, lead=lead, fill=out_fill, name="out")
            ok(fn(hd.ptr, n, cons, shift, clen, out.ptr, None))
            np.testing.assert_array_equal(out.payload(np.uint8), want, err_msg=f"lead {lead}")
            guards(hd, out)
            free(hd)
            return [out]
        F.run_twice(case)


# =====================================================================================================================================
# Hamming matrix: launch_matrix's vec_ok (kh_dev % 16, out_dev % 16, ld % 16) and the fall-through from the tile kernel
# =====================================================================================================================================
def matrix_inputs(rng, n, k):
    """labels: 0 full length, 1 a consensus three bases shorter than k (its pairs compare k - 3 bases), 2 noise"""
    from kmap_amd.kmer_count import get_hash_dtype
    kh = rng.integers(0, 4 ** k, size=n, dtype=np.uint64)
    lab = rng.integers(0, 3, size=n).astype(np.int32)
    if n >= 8:
        lab[:8] = [1, 1, 0, 2, 1, 0, 1, 2]
    return kh, kh.astype(get_hash_dtype(k)), lab, np.array([k, k - 3], np.int32)


def oracle_rows(O, kh64, lab, k, lens, row0, nrows):
    want = np.empty((nrows, len(kh64)), np.uint8)
    O.lib().ko_hamdist_rows(kh64, lab, len(kh64), k, lens, len(lens), row0, nrows, want)
    return want


def run_matrix(L, kh, lab, k, lens, row0, nrows, ld, out_lead=0, kh_lead=0):
    """-> the owed bytes (nrows x n) after both runs passed the guard, pad and written checks"""
    n = len(kh)
    fn = L.kmap_hamdist_matrix_u32_dev if kh.dtype == np.uint32 else L.kmap_hamdist_matrix_u64_dev
    got = []

    def case(out_fill, in_fill):
        kd = F.Guarded.of(kh, lead=kh_lead, fill=in_fill, name="kh")
        ld_ = F.Guarded.of(lab, fill=in_fill, name="label")
        out = F.Guarded.pitched(nrows, n, ld, lead=out_lead, fill=out_fill, name="out")
        ok(fn(kd.ptr, ld_.ptr, n, k, lens.ctypes.data_as(C.c_void_p), len(lens), row0, nrows, out.ptr, ld, None))
        got.append(out.rows())
        guards(kd, ld_, out)
        free(kd, ld_)
        return [out]
    F.run_twice(case)
    np.testing.assert_array_equal(got[0], got[1])
    return got[0]


@pytest.mark.parametrize("k", [8, 16, 20])                             # uint32; uint64 at the widest k <= 16; k > 16
@pytest.mark.parametrize("n", [1, 17, 1023, 1024, 1025, 2049])         # a wave owns 1024 columns, a lane 16
def test_hamdist_matrix_general_vec_and_scalar(L, O, n, k):
    """run_rows<H, true> next to each way to lose vec_ok: out_dev lead 1, a dense output with odd ld = n, kh_dev one element
    behind a 16-byte boundary.  Whole matrix and the row range (5, min(37, n - 5)); all forms give the oracle's bytes."""
    rng = np.random.default_rng(1000 * n + k)
    kh64, kh, lab, lens = matrix_inputs(rng, n, k)
    pitch = L.kmap_hamdist_pitch(n)
    assert pitch % 16 == 0 and pitch >= n
    ranges = [(0, n)] + ([(5, min(37, n - 5))] if n > 5 else [])
    for row0, nrows in ranges:
        want = oracle_rows(O, kh64, lab, k, lens, row0, nrows)
        forms = {"aligned": dict(ld=pitch), "out lead 1": dict(ld=pitch, out_lead=1), "kh lead": dict(ld=pitch, kh_lead=kh.itemsize)}
        if n % 2:
            forms["dense odd ld"] = dict(ld=n)
        for name, kw in forms.items():
            got = run_matrix(L, kh, lab, k, lens, row0, nrows, **kw)
            np.testing.assert_array_equal(got, want, err_msg=f"{name}, rows [{row0}, {row0 + nrows})")


@pytest.mark.parametrize("k", [8, 16])
def test_hamdist_matrix_fall_through_from_tile_kernel(L, O, k):
    """n = 4097 >= 4096: ld = 12288 at a 4096-aligned out_dev takes the tile kernel; an even chunk count (ld = 8192) or an out_dev
    16 bytes behind a 4096-byte boundary falls through to the general kernel.  All three equal the oracle (and so each other)."""
    n, row0, nrows = 4097, 4000, 40
    rng = np.random.default_rng(k)
    kh64, kh, lab, lens = matrix_inputs(rng, n, k)
    want = oracle_rows(O, kh64, lab, k, lens, row0, nrows)
    tile = run_matrix(L, kh, lab, k, lens, row0, nrows, ld=12288)
    np.testing.assert_array_equal(tile, want, err_msg="tile kernel")
    for name, kw in {"ld 8192": dict(ld=8192), "ld 12288, out lead 16": dict(ld=12288, out_lead=16)}.items():
        got = run_matrix(L, kh, lab, k, lens, row0, nrows, **kw)
        np.testing.assert_array_equal(got, tile, err_msg=f"{name} vs the tile kernel")
        np.testing.assert_array_equal(got, want, err_msg=name)


# =====================================================================================================================================
# rows_fresh_kernel / gather_rows_kernel ((a | b) & 15 per row pair), knn_select_kernel (`aligned`)
# =====================================================================================================================================
def repeated_rows(rng, n):
    """8 rows: 1 repeats 0; 2 differs from 1 in its last byte only; 3 repeats 2; 4 differs from 3 only in byte 16 * (n // 16), the
    first one behind the last whole 16-byte unit (where n has such a byte, else in the first byte of the last unit); 5 repeats 4;
    6 is new; 7 repeats 6"""
    D = np.empty((8, n), np.uint8)
    D[0] = rng.integers(0, 256, n)
    D[1] = D[0]
    D[2] = D[1]
    D[2, n - 1] ^= 0x40
    D[3] = D[2]
    D[4] = D[3]
    D[4, 16 * (n // 16) if n % 16 else max(n - 16, 0)] ^= 0x01
    D[5] = D[4]
    D[6] = rng.integers(0, 256, n)
    D[7] = D[6]
    return D


def pitched_input(A, ld, lead, fill, name="D"):
    g = F.Guarded.pitched(A.shape[0], A.shape[1] * A.itemsize, ld * A.itemsize, lead=lead, fill=fill, name=name)
    g.upload_rows(A)
    return g


@pytest.mark.parametrize("dense", [False, True], ids=["pitch", "ldd=n"])
@pytest.mark.parametrize("lead", [0, 1])
@pytest.mark.parametrize("n", [1, 15, 16, 17, 4097])
def test_rows_fresh_alignment(L, n, lead, dense):
    rng = np.random.default_rng(n)
    D = repeated_rows(rng, n)
    ldd = n if dense else int(L.kmap_hamdist_pitch(n))
    for row0 in (0, 3):
        nrows = len(D) - row0
        want = np.ones(nrows, np.uint8)
        want[1:] = (D[row0 + 1:] != D[row0:-1]).any(axis=1)

        def case(out_fill, in_fill):
            Dd = pitched_input(D, ldd, lead, in_fill)
            out = F.Guarded(nrows, fill=out_fill, name="fresh")
            ok(L.kmap_rows_fresh_u8_dev(Dd.ptr, ldd, n, row0, nrows, out.ptr, None))
            np.testing.assert_array_equal(out.payload(np.uint8), want, err_msg=f"row0 {row0}")
            guards(Dd, out)
            free(Dd)
            return [out]
        F.run_twice(case)


@pytest.mark.parametrize("dense", [False, True], ids=["pitch", "ldd=n"])
@pytest.mark.parametrize("lead", [0, 1])
@pytest.mark.parametrize("n", [1, 15, 16, 17, 4097])
def test_gather_rows_alignment(L, n, lead, dense):
    rng = np.random.default_rng(n + 1)
    D = repeated_rows(rng, n)
    ldd = n if dense else int(L.kmap_hamdist_pitch(n))
    idx = np.array([7, 0, 0, 3, 5, 2], np.int32)
    for out_lead in (0, 1):
        for ldo in (n, n + 3):
            def case(out_fill, in_fill):
                Dd, ix = pitched_input(D, ldd, lead, in_fill), F.Guarded.of(idx, fill=in_fill, name="idx")
                out = F.Guarded.pitched(len(idx), n, ldo, lead=out_lead, fill=out_fill, name="out")
                ok(L.kmap_gather_rows_u8_dev(Dd.ptr, ldd, n, ix.ptr, len(idx), out.ptr, ldo, None))
                np.testing.assert_array_equal(out.rows(), D[idx], err_msg=f"out lead {out_lead}, ldo {ldo}")
                guards(Dd, ix, out)
                free(Dd, ix)
                return [out]
            F.run_twice(case)


@pytest.mark.parametrize("hi", [9, 256], ids=["lt32", "bytes"])        # the lane-private counters / a value >= 32 in the row
@pytest.mark.parametrize("n_nb", [1, 20])
@pytest.mark.parametrize("n", [5, 65, 1031])                           # n % 16 != 0: a dense matrix has an unaligned pitch
def test_knn_select_alignment(L, O, n, n_nb, hi):
    """16-byte row loads (padded pitch, aligned D_dev) next to the generic row walk (ldd = n; D_dev lead 1).  Ties go to the lowest
    index: constant rows, and rows whose n_nb-th entry is the last column or ties with it (test_select_ties_and_last_column)."""
    n_nb = min(n_nb, n)
    rng = np.random.default_rng(n + n_nb + hi)
    D = rng.integers(0, hi, size=(n, n), dtype=np.uint8)
    base = hi - 1
    D[1] = base                                                        # all ties: index order alone
    if n > n_nb + 2:
        for r in (2, 3):                                               # n_nb - 1 small entries somewhere, the n_nb-th in the last column
            D[r] = base
            D[r, rng.choice(n - 2, size=n_nb - 1, replace=False)] = base - 2
            D[r, n - 1] = base - 1
        D[3, n - 2] = base - 1                                         # a tie for the last place: the lower index wins
    want = np.sort(O.knn_select_stable(D, n_nb), axis=1)
    pitch = int(L.kmap_hamdist_pitch(n))
    ranges = [(0, n)] + ([(2, 5)] if n >= 7 else [])
    for name, ldd, lead in (("aligned", pitch, 0), ("ldd = n", n, 0), ("D lead 1", pitch, 1)):
        for row0, nrows in ranges:
            def case(out_fill, in_fill):
                Dd = pitched_input(D, ldd, lead, in_fill)
                out = F.Guarded(nrows * n_nb * 4, fill=out_fill, name="nb_out")
                ok(L.kmap_knn_select_u8_dev(Dd.ptr, ldd, n, n_nb, row0, nrows, out.ptr, None))
                got = np.sort(out.payload(np.int32, (nrows, n_nb)), axis=1)
                np.testing.assert_array_equal(got, want[row0:row0 + nrows], err_msg=f"{name}, rows [{row0}, {row0 + nrows})")
                guards(Dd, out)
                free(Dd)
                return [out]
            F.run_twice(case)


# =====================================================================================================================================
# shuffle: aligned16 (fill kernel) and aligned4 (ByteWriter)
# =====================================================================================================================================
_PACKED = {}


def packed_shuffle_input(name):
    if name not in _PACKED:
        from tests import test_gpu_shuffle as S
        seq = S.array(name)
        codes, inval, _ = ref_pack(seq, np.random.default_rng(len(seq)))
        _PACKED[name] = (seq, codes, inval)
    return _PACKED[name]


@pytest.mark.parametrize("klet", [1, 2])
@pytest.mark.parametrize("name", ["edges", "short"])
def test_shuffle_out_alignment(L, name, klet):
    """seq_out_dev lead 0: 16-byte fill stores and word stores of the walk; 4: words but no 16-byte stores; 1, 2, 15: bytes only.
    The same seed gives the model's bytes for every lead."""
    from tests import test_gpu_shuffle as S
    seq, codes, inval = packed_shuffle_input(name)
    n, seed = len(seq), S.SEEDS[0]
    want = S.model_shuffle(name, klet, seed)
    for lead in (0, 1, 2, 4, 15):
        def case(out_fill, in_fill):
            c, i = F.Guarded.of(codes, fill=in_fill, name="codes"), F.Guarded.of(inval, fill=in_fill, name="inval")
            out = F.Guarded(n, lead=lead, fill=out_fill, name="seq_out")
            ok(L.kmap_shuffle_packed_dev(c.ptr, i.ptr, n, klet, seed, out.ptr, None, None))
            np.testing.assert_array_equal(out.payload(np.uint8), want, err_msg=f"lead {lead}")
            guards(c, i, out)
            free(c, i)
            return [out]
        F.run_twice(case)


# =====================================================================================================================================
# project_prob_kernel's `vec` (lds & 3, sums_dev & 7)
# =====================================================================================================================================
def test_project_prob_sums_alignment(L):
    """tests/test_gpu_project.py reaches vec = 1 alone (the wrapper's pitch is a multiple of 128 on an aligned allocation).  Here:
    vec = 1 (lds = n = 300, lead 0) next to the three ways to vec = 0 (lds = 301; sums_dev one uint16 behind an 8-byte boundary;
    both), on a row range inside m.  Q is exact and p is LUT3[Q] bit for bit, as in test_sums_and_p_exact."""
    from kmap_amd.projection import hd_prob_lut_projected
    from tests import test_gpu_project as P
    c = P.case("k8n300")
    n, k, m = c["n"], c["k"], len(c["nb"])
    lut3 = np.ascontiguousarray(hd_prob_lut_projected(k, P.N_NB), np.float32)
    assert c["Sref"].max() <= 65535 and c["Q"].max() < len(lut3)
    row0, nrows, ldp = 3, m - 5, n + 1
    want_q, want_p = c["Q"][row0:row0 + nrows], c["p"][row0:row0 + nrows]
    rng = np.random.default_rng(300)
    bits = {}
    for lds in (n, n + 1):
        sums = rng.integers(0, 65536, size=(n, lds)).astype(np.uint16)                 # pad columns hold noise
        sums[:, :n] = c["Sref"]
        for lead in (0, 2):
            def case(out_fill, in_fill):
                nb, s = F.Guarded.of(c["nb"], fill=in_fill, name="nb"), F.Guarded.of(sums, lead=lead, fill=in_fill, name="sums")
                lut = F.Guarded.of(lut3, fill=in_fill, name="lut")
                p = F.Guarded.pitched(nrows, n * 4, ldp * 4, fill=out_fill, name="p")
                q = F.Guarded.pitched(nrows, n * 4, ldp * 4, fill=out_fill, name="qsum")
                ok(L.kmap_project_prob_dev(nb.ptr, m, P.N_NB, s.ptr, lds, None, n, n, lut.ptr, len(lut3), row0, nrows, p.ptr, ldp, q.ptr,
                                           None))
                np.testing.assert_array_equal(q.rows(np.uint32), want_q, err_msg=f"Q, lds {lds}, lead {lead}")
                np.testing.assert_array_equal(p.rows(np.uint32), want_p.view(np.uint32), err_msg=f"p, lds {lds}, lead {lead}")
                bits[lds, lead] = p.rows(np.uint32)
                guards(nb, s, lut, p, q)
                free(nb, s, lut)
                return [p, q]
            F.run_twice(case)
    for key, got in bits.items():
        np.testing.assert_array_equal(got, bits[n, 0], err_msg=f"{key} vs the vector form")


# =====================================================================================================================================
# counts: hist_hashes (hash_dev % 16 together with n >= 2^20)
# =====================================================================================================================================
@pytest.mark.parametrize("k", [8, 10])
def test_counts_run_hashes_alignment(L, O, k):
    """n = 2^20 + 3 uint32 hashes (the suite's one 4-MB case).  k = 8: hash_dev lead 0 takes hist_lds_kernel (16-byte loads and a
    3-element tail), lead 4 hist_kernel.  k = 10 at this n is counted by the partitioned histogram whatever the pointer; it runs
    the same two leads.  Tables equal each other and oracle.count_uniq_hash."""
    from kmap_amd import _ffi
    n = (1 << 20) + 3
    rng = np.random.default_rng(k)
    h = rng.integers(0, 4 ** k, size=n, dtype=np.uint64).astype(np.uint32)
    h[rng.random(n) < 0.05] = 0xFFFFFFFF
    h[-3:] = [5, 0xFFFFFFFF, 4 ** k - 1]                              # the tail behind the last 16-byte unit
    want_u, want_c = O.count_uniq_hash(h, k)
    for lead, in_fill in ((0, 0x00), (0, 0xFF), (4, 0x00), (4, 0xFF)):
        hd = F.Guarded.of(h, lead=lead, fill=in_fill, name="hash")
        c = _ffi.vp()
        _ffi.check(L.kmap_counts_create(C.byref(c)))
        try:
            nu = C.c_int64(-1)
            ok(L.kmap_counts_run_hashes_dev(c.value, hd.ptr, n, k, 0, C.byref(nu), None))
            assert nu.value == len(want_u)
            uniq, cnt = np.empty(nu.value, np.uint32), np.empty(nu.value, np.int32)
            _ffi.check(L.kmap_counts_fetch(c.value, _ffi.ptr(uniq), _ffi.ptr(cnt)))
        finally:
            L.kmap_counts_destroy(c.value)
        np.testing.assert_array_equal(uniq, want_u, err_msg=f"lead {lead}")
        np.testing.assert_array_equal(cnt, want_c, err_msg=f"lead {lead}")
        np.testing.assert_array_equal(hd.payload(np.uint32), h)        # the input is left alone
        guards(hd)
        free(hd)


# =====================================================================================================================================
# entries that state an alignment requirement refuse a misaligned pointer (kmap_pack_planes_dev: tests/test_gpu_errors.py)
# =====================================================================================================================================
def assert_untouched(*bufs):
    for g in bufs:
        assert np.all(g.payload(np.uint8) == g.fill), f"{g.name} was written by a refused call"
        g.check_guards()


@pytest.mark.parametrize("lead", [1, 8])
def test_synth_reads_refuses_misaligned_seq(L, lead):
    from kmap_amd import _ffi
    n_reads, read_len = 37, 30
    seq, borders = F.Guarded(n_reads * (read_len + 1), lead=lead, name="seq"), F.Guarded(n_reads * 16, name="borders")
    rc = L.kmap_synth_reads_dev(seq.ptr, borders.ptr, n_reads, read_len, 7, None, None, None, 0, 0.0, None)
    assert rc == KMAP_E_INVAL and "seq_dev" in _ffi.last_error() and "aligned" in _ffi.last_error()
    _ffi.sync()
    assert_untouched(seq, borders)
    free(seq, borders)


@pytest.mark.parametrize("lead,dense", [(1, False), (0, True)], ids=["D lead 1", "ldd = n odd"])
def test_knn_sums_refuses_misaligned_matrix(L, lead, dense):
    from kmap_amd import _ffi
    n, n_nb = 33, 4
    rng = np.random.default_rng(33)
    D = rng.integers(0, 9, size=(n, n), dtype=np.uint8)
    ldd = n if dense else int(L.kmap_hamdist_pitch(n))
    Dd = pitched_input(D, ldd, lead, 0x00)
    nb = F.Guarded.of(rng.integers(0, n, size=(n, n_nb)).astype(np.int32), name="nb")
    sums = F.Guarded.pitched(n, n * 2, 2 * (n + 7), name="sums")
    rc = L.kmap_knn_sums_u8_dev(Dd.ptr, ldd, nb.ptr, n, n_nb, 0, n, sums.ptr, n + 7, None)
    assert rc == KMAP_E_INVAL and "knn_sums: D must be 16-byte aligned" in _ffi.last_error() and "ldd" in _ffi.last_error()
    _ffi.sync()
    assert_untouched(sums)
    guards(Dd, nb)
    free(Dd, nb, sums)
