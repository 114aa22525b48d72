"""Every device entry against stale scratch and stale handle state (tests/_stale.py has the choreography, DESIGN.md the audit).

All verbs borrow their temporary device memory from one cached arena that is never cleared, and the handles keep buffers that
only grow.  Every other test of the suite sees the arena in whatever state the fixed file order left it -- and fresh device
memory is zero, so a forgotten memset, a clear that is a few words short, a read beyond the carved size or a scan that takes a
live slot gives right answers there.  Here every case runs cold (arena released), and three times behind a LARGER instance of
its own family with the whole arena set to 0x00, 0x5A and 0xFF; the four results must be bit for bit the case's reference: the
oracle or the host model that the entry's own test uses, never another run of the entry.  The helper also requires that the case
took scratch at all.  The handle cases run a small input on a handle that has just run a large one.

The control comes first: if a fill does not reach the arena, nothing below can discriminate."""
import ctypes as C

import numpy as np
import pytest

from tests import _stale as ST
from tests._stale import covers

pytestmark = pytest.mark.gpu

COMBOS = [(0, 0), (0, 1), (1, 0), (1, 1)]                  # (dedupe per read, reverse-complement merge)


@pytest.fixture(scope="module")
def env():
    from kmap_amd import _ffi
    from kmap_amd.kmer_count import DeviceCounts
    from kmap_amd.motif_discovery import DeviceSeq
    from oracle import oracle as O
    return _ffi, DeviceCounts, DeviceSeq, O


_KEPT = {}                                                  # name -> object with close(), built once and shared by the cases


@pytest.fixture(scope="module", autouse=True)
def _close_kept():
    yield
    for v in _KEPT.values():
        for x in (v if isinstance(v, tuple) else (v,)):
            if hasattr(x, "close"):
                x.close()
    _KEPT.clear()


def kept(name, make):
    if name not in _KEPT:
        _KEPT[name] = make()
    return _KEPT[name]


def synth(rng, n_reads, lo, hi, p_n=0.02):
    """tests/test_gpu_packed.synth: reads of lo .. hi bases, a 255 behind every read, p_n of the bases invalid"""
    lens = rng.integers(lo, hi + 1, size=n_reads)
    starts = np.concatenate([[0], np.cumsum(lens + 1)[:-1]])
    borders = np.ascontiguousarray(np.stack([starts, starts + lens], axis=1), np.int64)
    seq = rng.integers(0, 4, size=int((lens + 1).sum())).astype(np.uint8)
    seq[rng.random(len(seq)) < p_n] = 255
    seq[borders[:, 1]] = 255
    return seq, borders


def reads_exact(seed, n_total, lo=20, hi=160):
    """synth with exactly n_total array positions"""
    rng = np.random.default_rng(seed)
    lens, left = [], n_total
    while left > 0:
        ln = int(rng.integers(lo, hi + 1))
        if left - (ln + 1) < lo + 1:
            ln = left - 1
        lens.append(ln)
        left -= ln + 1
    lens = np.array(lens, np.int64)
    starts = np.concatenate([[0], np.cumsum(lens + 1)[:-1]])
    borders = np.ascontiguousarray(np.stack([starts, starts + lens], axis=1), np.int64)
    seq = rng.integers(0, 4, n_total).astype(np.uint8)
    seq[rng.random(n_total) < 0.02] = 255
    seq[borders[:, 1]] = 255
    assert len(seq) == n_total and borders[-1, 1] == n_total - 1
    return seq, borders


# ---- the control: the fill reaches the arena -----------------------------------------------------------------------------------------
@covers("kmap_scratch_fill", "kmap_scratch_acquired")
def test_control_the_fill_reaches_the_arena(env):
    """After a count at k = 8 the shared table (kmap_counts_bins) lies in the arena: kmap_scratch_fill(0xA5) must report it, the
    table read back must be all 0xA5, and the handle must then refuse kmap_counts_finish with the error that says the arena was
    released or overwritten."""
    _ffi, DeviceCounts, DeviceSeq, O = env
    L = _ffi.lib()
    A = ST.arena()
    seq, borders = synth(np.random.default_rng(1), 200, 30, 90)
    ds, dc = DeviceSeq(seq, borders), DeviceCounts()
    try:
        before = A.acquired()
        _ffi.check(L.kmap_counts_hist_packed_dev(dc._h, ds.codes.ptr, ds.inval_orig.ptr, ds.n, ds.borders.ptr, ds.n_seq, 8, 0, None))
        assert A.acquired() > before, "kmap_scratch_acquired did not advance during a count"
        p, nb = C.c_void_p(), C.c_int64(0)
        _ffi.check(L.kmap_counts_bins(dc._h, C.byref(p), C.byref(nb)))
        assert nb.value == 4 ** 8
        table = np.empty(nb.value, np.uint32)
        _ffi.check(L.kmap_memcpy_d2h(_ffi.ptr(table), p, table.nbytes, None))
        assert int(table.sum()) == int((O.comp_kmer_hash(seq, 8) != O.get_invalid_hash(np.uint32)).sum())
        n_buffers, n_bytes = A.fill(0xA5)
        why = "the cases of this file cannot discriminate: kmap_scratch_fill does not reach the arena's buffers"
        assert n_buffers >= 1 and n_bytes >= table.nbytes, f"{why} (it reports {n_buffers} buffers, {n_bytes} bytes)"
        _ffi.check(L.kmap_memcpy_d2h(_ffi.ptr(table), p, table.nbytes, None))
        assert (table.view(np.uint8) == 0xA5).all(), f"{why} (the shared table does not hold the fill byte)"
        nu = C.c_int64(-1)
        rc = L.kmap_counts_finish(dc._h, 8, 1, C.byref(nu), None)
        err = L.kmap_last_error()
        assert rc == -5 and b"shared histogram" in err and b"released" in err, f"{why} (finish on the overwritten table: rc {rc}, {err!r})"
    finally:
        dc.close()
        ds.close()


# ---- counting ---------------------------------------------------------------------------------------------------------------------------
N_PART = (1 << 20) + 32768 + 17
COUNT_CASES = {                                             # name -> (k, positions of the case, positions of the primer)
    "k8_lds": (8, 65553, 90000), "k12_fine": (12, N_PART, 1400000), "k14_fine": (14, N_PART, 1400000),
    "k14_one_kmer": (14, 0, 0), "k16_two_level": (16, N_PART, 1400000), "k19_sort": (19, 70001, 100003),
}


def one_kmer_reads(n_reads):
    """the one-k-mer input of tests/test_gpu_packed.test_fine_partition_edge_inputs: poly-A reads of 160 bases"""
    L = 160
    seq = np.zeros(n_reads * (L + 1), np.uint8)
    seq.reshape(n_reads, L + 1)[:, L] = 255
    starts = np.arange(n_reads, dtype=np.int64) * (L + 1)
    return seq, np.ascontiguousarray(np.stack([starts, starts + L], axis=1))


def count_reads(name, which):
    k, n_case, n_prime = COUNT_CASES[name]
    if name == "k14_one_kmer":
        return one_kmer_reads(7000 if which == "case" else 9000)
    return reads_exact(len(name) + (0 if which == "case" else 50), n_case if which == "case" else n_prime)


def count_pair(env, name):
    """(reads, borders, DeviceSeq of the case, DeviceSeq of the primer, one DeviceCounts), shared by the four combinations"""
    _ffi, DeviceCounts, DeviceSeq, O = env

    def make():
        seq, borders = count_reads(name, "case")
        pseq, pborders = count_reads(name, "primer")
        assert len(pseq) > len(seq) + len(seq) // 8        # beyond the head-room: every slot grows for the primer
        return _Host(seq, borders), DeviceSeq(seq, borders), DeviceSeq(pseq, pborders), DeviceCounts()
    return kept("count " + name, make)


class _Host:
    def __init__(self, seq, borders):
        self.seq, self.borders = seq, borders


def counted(ds, dc, k, dedupe, merge):
    ds.count(dc, k, dedupe=bool(dedupe), merge_revcom=bool(merge))
    u, c = dc.fetch()
    return {"uniq": u, "cnt": c}


@covers("kmap_counts_run_packed_dev", "kmap_counts_hist_packed_dev", "kmap_counts_finish", "kmap_counts_fetch")
@pytest.mark.parametrize("dedupe,merge", COMBOS)
@pytest.mark.parametrize("name", list(COUNT_CASES))
def test_counts(env, name, dedupe, merge):
    """Reference: oracle.count_kmers.  k8_lds: the 16-bit LDS histograms at 65 553 positions; k12_fine / k14_fine: the fine
    partition at 2^20 + 32 768 + 17; k14_one_kmer: every key in one bucket, the 16-bit spill list in slot B; k16_two_level: the
    re-sorted keys in the dead hash slot, a scan of 131 072 counts; k19_sort: 70 001 positions, radix_sort.h scans 256 x 69 tile
    counts in its tiled form (slots C and D)."""
    _ffi, DeviceCounts, DeviceSeq, O = env
    k = COUNT_CASES[name][0]
    host, ds, prime, dc = count_pair(env, name)
    u, c = O.count_kmers(host.seq, host.borders, k, not dedupe, bool(merge))
    if name == "k19_sort":
        assert 256 * ((int((O.comp_kmer_hash(host.seq, k) != O.get_invalid_hash(np.uint64)).sum()) + 1023) // 1024) > 4096
    # k = 8 without dedupe takes no slot that grows with the reads (the table and two minimum-size slots): its primer counts at
    # k = 9, the same 16-bit LDS form on a table four times as large
    k_prime = 9 if k == 8 else k
    ST.states(f"count {name} dedupe={dedupe} merge={merge}", lambda: counted(ds, dc, k, dedupe, merge),
              lambda: counted(prime, dc, k_prime, dedupe, merge), {"uniq": u, "cnt": c})


def range_slice(O, seq, borders, k, dedupe, merge, first_bin, n_bins):
    """oracle.count_kmers' table sliced by POSITION, as tests/test_gpu_packed.py restates it: an entry's position is its own key,
    but an unpaired higher member of a reverse-complement pair stays at its position with its key replaced by the partner's"""
    if not merge:
        u, c = O.count_kmers(seq, borders, k, not dedupe, False)
        keep = (u.astype(np.uint64) >= first_bin) & (u.astype(np.uint64) < first_bin + n_bins)
        return u[keep], c[keep]
    u0, _ = O.count_kmers(seq, borders, k, not dedupe, False)
    p0 = u0.astype(np.uint64)
    r0 = O.get_revcom_hash_arr(u0, k).astype(np.uint64)
    gone = np.isin(r0, p0) & (p0 > r0)
    pos = p0[~gone]
    u, c = O.count_kmers(seq, borders, k, not dedupe, True)
    assert len(u) == len(pos) and (u.astype(np.uint64) == np.minimum(p0, r0)[~gone]).all()
    keep = (pos >= first_bin) & (pos < first_bin + n_bins)
    return u[keep], c[keep]


@covers("kmap_counts_run_packed_range_dev")
@pytest.mark.parametrize("dedupe,merge", [(1, 1), (0, 0)])
@pytest.mark.parametrize("first_bin,n_bins", [(4 ** 14 // 4, 4 ** 14 // 4), (8 * 12345, 777777)], ids=["masked", "plain"])
def test_count_range(env, first_bin, n_bins, dedupe, merge):
    """k = 14, one range with a common key prefix (the masked form of the stage kernel) and one without (the plain form).
    Reference: oracle.count_kmers sliced by position."""
    _ffi, DeviceCounts, DeviceSeq, O = env
    host, ds, prime, dc = count_pair(env, "k14_fine")

    def run(d):
        d.count_range(dc, 14, bool(dedupe), bool(merge), first_bin, n_bins)
        u, c = dc.fetch()
        return {"uniq": u, "cnt": c}
    u, c = range_slice(O, host.seq, host.borders, 14, dedupe, merge, first_bin, n_bins)
    assert len(u) > 100
    ST.states(f"count_range [{first_bin}, +{n_bins}) dedupe={dedupe} merge={merge}", lambda: run(ds), lambda: run(prime), {"uniq": u, "cnt": c})


# ---- scan and mask on the packed reads -------------------------------------------------------------------------------------------------
def oracle_scan(O, seq, borders, k, cons, r, revcom):
    """ko_scan_read read by read, as tests/test_gpu_packed.py: (hits int32[n_seq], positions int32[total])"""
    buf, md = np.empty(max(int((borders[:, 1] - borders[:, 0]).max()), 1) + 1, np.int32), C.c_int(0)
    hits, pos = np.zeros(len(borders), np.int32), []
    fn = O.lib().ko_scan_read
    for i, (a, b) in enumerate(borders.tolist()):
        m = fn(np.ascontiguousarray(seq[a:b]), b - a, k, cons, r, int(revcom), buf, C.byref(md))
        hits[i] = m
        pos.append(buf[:m].copy())
    return hits, (np.concatenate(pos) if pos else np.zeros(0, np.int32)).astype(np.int32)


def tiny_reads(seed, total):
    rng = np.random.default_rng(seed)
    parts, borders, st = [], [], 0
    while st < total:
        L = int(rng.integers(1, 90))
        parts += [rng.integers(0, 4, size=L).astype(np.uint8), np.array([255], np.uint8)]
        borders.append((st, st + L))
        st += L + 1
    return np.concatenate(parts), np.array(borders, np.int64)


def scanned(ds, k, cons, r, revcom=True):
    hits, pos = ds.scan(k, cons, r, revcom)
    return {"hits": hits, "pos": pos}


def first_kmer(O, seq, borders, k):
    a = next(a for a, b in borders.tolist() if b - a >= k and seq[a:a + k].max() < 4)
    return int(O.comp_kmer_hash(seq[a:a + k], k)[0])


@covers("kmap_scan_run_packed_dev", "kmap_scan_fetch")
@pytest.mark.parametrize("total,k,r", [(330, 8, 3), (1500, 14, 6)], ids=["two_pass_330", "fused_1500"])
def test_scan_short_inputs(env, total, k, r):
    """330 positions: fewer than one row of code words, the two-pass form; 1500: the fused pass with its reservation cursors in
    slot PART.  Reference: ko_scan_read."""
    _ffi, DeviceCounts, DeviceSeq, O = env
    seq, borders = tiny_reads(77 + total, total)
    pseq, pborders = synth(np.random.default_rng(78), 3000, 20, 120)
    cons = first_kmer(O, seq, borders, k)
    ds, prime = DeviceSeq(seq, borders), DeviceSeq(pseq, pborders)
    try:
        hits, pos = oracle_scan(O, seq, borders, k, cons, r, True)
        assert hits.sum() > 0
        ST.states(f"scan {total} positions", lambda: scanned(ds, k, cons, r), lambda: scanned(prime, k, cons, r), {"hits": hits, "pos": pos})
    finally:
        ds.close()
        prime.close()


def overfull_reads(n_reads, L=150, seed=99):
    """tests/test_gpu_packed.test_packed_scan_more_hits_than_the_one_pass_buffer: every other read poly-A, a quarter poly-T"""
    rng = np.random.default_rng(seed)
    seq = rng.integers(0, 4, size=n_reads * (L + 1)).astype(np.uint8).reshape(n_reads, L + 1)
    seq[::2, :] = 0
    seq[1::4, :] = 3
    seq[:, L] = 255
    borders = np.stack([np.arange(n_reads) * (L + 1), np.arange(n_reads) * (L + 1) + L], axis=1).astype(np.int64)
    return np.ascontiguousarray(seq.reshape(-1)), borders


@covers("kmap_scan_run_packed_dev")
def test_scan_more_hits_than_the_one_pass_buffer(env):
    """30 000 reads, a 3-mer at radius 1: the one-pass buffer overflows and the count / scan / write form runs on block sums the
    fused kernel left behind.  Reference: ko_scan_read on every read."""
    _ffi, DeviceCounts, DeviceSeq, O = env
    seq, borders = overfull_reads(30_000)
    pseq, pborders = overfull_reads(36_000, seed=100)
    cons = int(O.kmer2hash("AAA"))
    ds, prime = DeviceSeq(seq, borders), DeviceSeq(pseq, pborders)
    try:
        hits, pos = oracle_scan(O, seq, borders, 3, cons, 1, True)
        assert len(pos) > max(2 * len(borders), 1 << 20)
        ST.states("scan beyond the one-pass buffer", lambda: scanned(ds, 3, cons, 1), lambda: scanned(prime, 3, cons, 1),
                  {"hits": hits, "pos": pos})
    finally:
        ds.close()
        prime.close()


@covers("kmap_scan_run_packed_dev")
@pytest.mark.parametrize("r", [8, 15], ids=["nibbles_r8", "wave_per_read_r15"])
def test_scan_wide(env, r):
    """k = 20 (csrc/scan_wide.hip) on 4097 short reads: the scan of the per-read hit counts takes its tiled form with slots C and
    D.  Reference: ko_scan_read."""
    _ffi, DeviceCounts, DeviceSeq, O = env
    k = 20
    seq, borders = synth(np.random.default_rng(20 + r), 4097, 18, 60)
    pseq, pborders = synth(np.random.default_rng(21 + r), 6000, 18, 80)
    cons = first_kmer(O, seq, borders, k)
    ds, prime = DeviceSeq(seq, borders), DeviceSeq(pseq, pborders)
    try:
        hits, pos = oracle_scan(O, seq, borders, k, cons, r, True)
        assert hits.sum() > 0 and len(borders) > 4096
        ST.states(f"wide scan r={r}", lambda: scanned(ds, k, cons, r), lambda: scanned(prime, k, cons, r), {"hits": hits, "pos": pos})
    finally:
        ds.close()
        prime.close()


@covers("kmap_mask_hamball_packed_dev")
@pytest.mark.parametrize("k,n_cons", [(7, 17), (18, 33)], ids=["bitsliced_two_passes", "wide_two_batches"])
def test_mask(env, k, n_cons):
    """17 consensuses at k = 7: two flag passes of the bit-sliced form, their hit arrays side by side in slot A; 33 at k = 18: two
    batches of csrc/scan_wide.hip's.  Reference: oracle.mask_input."""
    _ffi, DeviceCounts, DeviceSeq, O = env
    rng = np.random.default_rng(13 + k)
    seq, borders = synth(rng, 300, 30, 100)
    pseq, pborders = synth(rng, 900, 30, 100)
    cons = rng.integers(0, 4 ** k, size=n_cons, dtype=np.uint64)
    cons[0] = int(O.kmer2hash("T" * k))
    cons[1] = first_kmer(O, seq, borders, k)
    rad = rng.integers(0, 2 if k == 7 else 5, size=n_cons)
    ds, prime = DeviceSeq(seq, borders), DeviceSeq(pseq, pborders)

    def run(d):
        d.reset()
        d.mask(k, cons, rad)
        return d.download()
    try:
        want = O.mask_input(seq.copy(), k, cons, rad)
        assert (want != seq).any()
        ST.states(f"mask k={k}", lambda: run(ds), lambda: run(prime), want)
    finally:
        ds.close()
        prime.close()


@covers("kmap_scan_declare_uniform")
@pytest.mark.parametrize("declared", [True, False], ids=["accepted", "refused"])
def test_scan_declare_uniform(env, declared):
    """uniform reads, the declaration accepted (the borders come from the read index) and refused (a wrong length; the flag word
    in slot D must have been cleared either way).  Reference: ko_scan_read."""
    _ffi, DeviceCounts, DeviceSeq, O = env
    L = _ffi.lib()
    seq, borders = synth(np.random.default_rng(9), 700, 60, 60, p_n=0.004)
    pseq, pborders = synth(np.random.default_rng(10), 2000, 60, 60, p_n=0.004)
    cons = first_kmer(O, seq, borders, 8)

    def run(d):
        h = _ffi.vp()
        _ffi.check(L.kmap_scan_create(C.byref(h)))
        try:
            ok, tot = _ffi.i32(7), _ffi.i64(0)
            _ffi.check(L.kmap_scan_declare_uniform(h.value, d.borders.ptr, d.n_seq, 60 if declared else 61, 61, C.byref(ok), None))
            _ffi.check(L.kmap_scan_run_packed_dev(h.value, d.codes.ptr, d.inval_orig.ptr, d.n, d.borders.ptr, d.n_seq, 8, cons, 2, 1,
                                                  C.byref(tot), d.planes.ptr, None))
            hits, pos = np.empty(d.n_seq, np.int32), np.empty(tot.value, np.int32)
            _ffi.check(L.kmap_scan_fetch(h.value, _ffi.ptr(hits), None, _ffi.ptr(pos)))
            return {"accepted": np.array([ok.value]), "hits": hits, "pos": pos}
        finally:
            L.kmap_scan_destroy(h.value)
    ds, prime = DeviceSeq(seq, borders), DeviceSeq(pseq, pborders)
    try:
        hits, pos = oracle_scan(O, seq, borders, 8, cons, 2, True)
        ST.states(f"declare_uniform declared={declared}", lambda: run(ds), lambda: run(prime),
                  {"accepted": np.array([int(declared)]), "hits": hits, "pos": pos})
    finally:
        ds.close()
        prime.close()


# ---- hash-array verbs -----------------------------------------------------------------------------------------------------------------
@covers("kmap_dedupe_per_read_u32", "kmap_dedupe_per_read_u64", "kmap_dedupe_per_read_u32_dev", "kmap_dedupe_per_read_u64_dev")
@pytest.mark.parametrize("k", [6, 20])
def test_dedupe_with_a_long_read(env, k):
    """per-read dedupe of a hash array with one read of 513 positions among short ones: the long reads' ids and their counter lie
    in slot C.  Reference: oracle.remove_duplicate_hash_per_seq."""
    _ffi, DeviceCounts, DeviceSeq, O = env
    from kmap_amd import kmer_count as kc
    rng = np.random.default_rng(600 + k)

    def reads(lengths):
        parts, borders, at = [], [], 0
        for ln in lengths:
            parts += [np.resize(rng.integers(0, 4, 11), ln).astype(np.uint8), np.array([255], np.uint8)]   # period 11: duplicates
            borders.append((at, at + ln))
            at += ln + 1
        return np.concatenate(parts), np.array(borders, np.int64)
    seq, borders = reads([40, 513, 70, 512, 90])
    pseq, pborders = reads([600] * 3 + [50] * 400)
    h, ph = O.comp_kmer_hash(seq, k), O.comp_kmer_hash(pseq, k)
    want = O.remove_duplicate_hash_per_seq(h.copy(), borders)
    assert (want != h).any()
    ST.states(f"dedupe k={k}", lambda: kc.remove_duplicate_hash_per_seq(h.copy(), borders),
              lambda: kc.remove_duplicate_hash_per_seq(ph.copy(), pborders), want)


@covers("kmap_hamdist_matrix_u8", "kmap_hamdist_matrix_u32_dev", "kmap_hamdist_matrix_u64_dev")
@pytest.mark.parametrize("k", [8, 16])
def test_hamdist_matrix(env, k):
    """n = 300 with two short consensuses (the general kernel; the group ids lie in slot A).  Reference: oracle.hamdist_matrix_u8."""
    _ffi, DeviceCounts, DeviceSeq, O = env
    from kmap_amd.hamdist import hamdist_matrix_u8
    rng = np.random.default_rng(3 + k)
    lens = [k, 5, k - 2]

    def data(n):
        return rng.integers(0, 4 ** k, size=n, dtype=np.uint64).astype(O.get_hash_dtype(k)), np.sort(rng.integers(0, 3, n)).astype(np.int32)
    kh, lab = data(300)
    pkh, plab = data(1000)
    ST.states(f"hamdist_matrix k={k}", lambda: hamdist_matrix_u8(kh, lab, k, lens), lambda: hamdist_matrix_u8(pkh, plab, k, lens),
              O.hamdist_matrix_u8(kh, lab, k, lens))


@covers("kmap_hamdist_matrix_u32_dev", "kmap_hamdist_matrix_u64_dev", "kmap_knn_select_u8_dev", "kmap_knn_sums_u8_dev",
        "kmap_knn_sums_kmers_u32_dev", "kmap_knn_sums_kmers_u64_dev")
@pytest.mark.parametrize("k", [8, 16])
def test_knn_chain(env, k):
    """matrix -> selection -> sums from the matrix -> sums from the k-mers at n = 257, 20 neighbours (two workgroups of every
    kernel; the transposed neighbour lists, the maximum word and the profile vectors lie in slots C and D).  Reference: the
    oracle's matrix, oracle.knn_select_stable and the neighbour sums A D A^T of the oracle's matrix."""
    _ffi, DeviceCounts, DeviceSeq, O = env
    L = _ffi.lib()
    n_nb = 20
    rng = np.random.default_rng(340 + k)
    clen = np.array([k], np.int32)
    mat = L.kmap_hamdist_matrix_u32_dev if k < 16 else L.kmap_hamdist_matrix_u64_dev
    sums_k = L.kmap_knn_sums_kmers_u32_dev if k < 16 else L.kmap_knn_sums_kmers_u64_dev

    def run(n, kh):
        ldd, lds = (n + 15) & ~15, (n + 127) & ~127
        bufs = [_ffi.DeviceBuffer.from_numpy(kh), _ffi.DeviceBuffer.from_numpy(np.zeros(n, np.int32)), _ffi.DeviceBuffer(n * ldd),
                _ffi.DeviceBuffer(n * n_nb * 4), _ffi.DeviceBuffer(n * lds * 2), _ffi.DeviceBuffer(n * lds * 2)]
        kh_d, lab_d, D_d, nb_d, s_d, sk_d = bufs
        try:
            _ffi.check(mat(kh_d.ptr, lab_d.ptr, n, k, _ffi.ptr(clen), 1, 0, n, D_d.ptr, ldd, None))
            _ffi.check(L.kmap_knn_select_u8_dev(D_d.ptr, ldd, n, n_nb, 0, n, nb_d.ptr, None))
            _ffi.check(L.kmap_knn_sums_u8_dev(D_d.ptr, ldd, nb_d.ptr, n, n_nb, 0, n, s_d.ptr, lds, None))
            _ffi.check(sums_k(kh_d.ptr, lab_d.ptr, n, k, _ffi.ptr(clen), 1, nb_d.ptr, n_nb, 0, n, sk_d.ptr, lds, None))
            _ffi.sync()
            return {"nb": np.sort(nb_d.to_numpy(np.int32, (n, n_nb)), axis=1),                 # the rule fixes the set, not its order
                    "sums": np.ascontiguousarray(s_d.to_numpy(np.uint16, (n, lds))[:, :n]),
                    "sums_k": np.ascontiguousarray(sk_d.to_numpy(np.uint16, (n, lds))[:, :n])}
        finally:
            for b in bufs:
                b.free()
    kh = rng.integers(0, 4 ** k, size=257, dtype=np.uint64).astype(O.get_hash_dtype(k))
    pkh = rng.integers(0, 4 ** k, size=700, dtype=np.uint64).astype(O.get_hash_dtype(k))
    D = O.hamdist_matrix_u8(kh, np.zeros(257, np.int32), k, clen).astype(np.int64)
    nb = O.knn_select_stable(D, n_nb)
    A = np.zeros((257, 257), np.int64)
    A[np.arange(257)[:, None], nb] = 1
    want = A @ D @ A.T
    np.fill_diagonal(want, 0)
    want = want.astype(np.uint16)
    ST.states(f"knn chain k={k}", lambda: run(257, kh), lambda: run(700, pkh),
              {"nb": np.sort(nb, axis=1).astype(np.int32), "sums": want, "sums_k": want})


# ---- the weight-matrix verbs -----------------------------------------------------------------------------------------------------------
PWM_WIDTHS = (4, 5, 6, 7, 8, 9, 11, 16, 31)                # nine matrices: eight fill a batch, the 31-column one is the second


def pwm_set(env):
    """the read set of tests/test_gpu_pwm_library.edge_set (edge_reads, on a DeviceSeq of its own), a larger primer set, nine matrices and their
    window scores, computed once"""
    _ffi, DeviceCounts, DeviceSeq, O = env

    def make():
        from tests import test_gpu_pwm_library as TL
        from tests._refine_model import asym_matrix, make_reads, window_scores
        seq, borders, _ = TL.edge_reads()
        rng = np.random.default_rng(1700)
        Ws = [asym_matrix(w, rng) for w in PWM_WIDTHS]
        pseq, pborders = make_reads(rng.integers(0, 201, 1500), rng)
        assert len(pseq) > 2 * len(seq) and len(pborders) > 2 * len(borders)
        return _PwmSet(DeviceSeq(seq, borders), DeviceSeq(pseq, pborders), seq, borders, Ws, [window_scores(seq, W) for W in Ws])
    return kept("pwm", make)


class _PwmSet:
    def __init__(self, ds, prime, seq, borders, Ws, scored):
        self.ds, self.prime, self.seq, self.borders, self.Ws, self.scored = ds, prime, seq, borders, Ws, scored
        from tests import _readscore_model as RM
        self.best = [RM.np_read_scores(seq, borders, W, True, sc) for W, sc in zip(Ws, scored)]
        # per matrix the median best score of the scorable reads: about half of them are site reads
        self.thr = [int(np.median(s[loc >= 0])) for s, loc, _ in self.best]

    def close(self):
        self.ds.close()
        self.prime.close()


@covers("kmap_readscore_packed_dev", "kmap_readscore_hist_dev")
def test_read_scores_and_histogram(env):
    """Reference: tests/_readscore_model.np_read_scores and np_histogram (the 31-column matrix)."""
    from tests import _readscore_model as RM
    _ffi = env[0]
    p = pwm_set(env)
    W = p.Ws[-1]
    lo, hi = RM.score_range(W)
    lo, nb = lo + (hi - lo) // 3, (hi - lo) // 3

    def run(d):
        rs = d.read_scores(W, True)
        try:
            score, loc, strand = rs.fetch()
            hist, outside = np.full(nb, 0xEEEE, np.uint64), _ffi.i64(-1)       # the entry itself: the method refuses reads outside the range
            _ffi.check(_ffi.lib().kmap_readscore_hist_dev(rs.score.ptr, rs.loc.ptr, rs.n_seq, lo, nb, _ffi.ptr(hist), C.byref(outside), None))
            return {"score": score, "loc": loc, "strand": strand, "hist": hist, "n": np.array([rs.n_scored, outside.value], np.int64)}
        finally:
            rs.close()
    score, loc, strand = p.best[-1]
    hist, outside = RM.np_histogram(score, loc, lo, nb)
    ST.states("read_scores + histogram", lambda: run(p.ds), lambda: run(p.prime),
              {"score": score, "loc": loc, "strand": strand, "hist": hist, "n": np.array([(loc >= 0).sum(), outside], np.int64)})


@covers("kmap_readscore_library_dev")
def test_library_histograms(env):
    """Reference: tests/_readscore_model.py per matrix (a range that leaves reads outside)."""
    from tests import _readscore_model as RM
    p = pwm_set(env)
    rng = [RM.score_range(W) for W in p.Ws]
    los, nbs = [a + (b - a) // 3 for a, b in rng], [(b - a) // 3 for a, b in rng]

    def run(d):
        hists, outside, scored = d.library_histograms(p.Ws, los, nbs, True)
        return {"hist": np.concatenate(hists), "outside": outside, "scored": scored}
    want = [RM.np_histogram(s, loc, lo, nb) for (s, loc, _), lo, nb in zip(p.best, los, nbs)]
    ST.states("library_histograms", lambda: run(p.ds), lambda: run(p.prime),
              {"hist": np.concatenate([h for h, _ in want]), "outside": np.array([o for _, o in want], np.int64),
               "scored": np.array([(loc >= 0).sum() for _, loc, _ in p.best], np.int64)})


@covers("kmap_readscore_sites_library_dev")
def test_library_sites(env):
    """Reference: tests/_sites_model.np_library_sites (max_len below the longest read, so that n_too_long counts)."""
    from tests._sites_model import np_library_sites
    p = pwm_set(env)
    max_len = 200

    def run(d):
        return d.library_sites(p.Ws, p.thr, True, max_len)
    want = np_library_sites(p.seq, p.borders, p.Ws, p.thr, True, max_len, p.scored)
    assert want[2].min() > 0
    ST.states("library_sites", lambda: run(p.ds), lambda: run(p.prime), want)


@covers("kmap_presence_library_dev", "kmap_bitrows_pair_counts_dev")
def test_presence_and_pair_counts(env):
    """Reference: tests/_cooccurrence_model.np_presence, np_pack and np_pair_counts."""
    from tests import _cooccurrence_model as CM
    p = pwm_set(env)

    def run(d):
        planes = d.library_presence(p.Ws, p.thr, True)
        try:
            return {"pairs": planes.pair_counts(), "planes": planes.fetch(), "present": planes.n_present.copy()}
        finally:
            planes.close()
    bits = CM.np_presence(p.seq, p.borders, p.Ws, p.thr, True, p.scored)
    want = {"planes": np.asarray(CM.np_pack(bits), np.uint64).reshape(len(p.Ws), -1), "present": bits.sum(axis=1).astype(np.int64),
            "pairs": np.asarray(CM.np_pair_counts(bits)).astype(np.int64)}
    ST.states("presence + pair counts", lambda: run(p.ds), lambda: run(p.prime), want)


@covers("kmap_readscore_spacing_library_dev")
def test_library_spacing(env):
    """Reference: tests/_spacing_model.np_library_spacing (the primary sites' locs and their counter lie in slot D, the weights
    in slot C, through both batches)."""
    from tests._refine_model import asym_matrix, window_scores
    from tests._spacing_model import np_library_spacing
    from tests import _readscore_model as RM
    p = pwm_set(env)
    WP = asym_matrix(8, np.random.default_rng(27))
    scored_P = window_scores(p.seq, WP)
    sP, locP, _ = RM.np_read_scores(p.seq, p.borders, WP, True, scored_P)
    tP = int(np.median(sP[locP >= 0]))
    thr = [t - 300 for t in p.thr]                           # secondary sites away from the best window need lower bars
    G = 40

    def run(d):
        prim = d.read_scores(WP, True)
        try:
            S, R, n_primary, pair, far = d.library_spacing(prim, 8, tP, p.Ws, thr, True, G)
            return {"S": S, "R": R, "n": np.concatenate([[n_primary], pair, far]).astype(np.int64)}
        finally:
            prim.close()
    S, R, n_primary, pair, far = np_library_spacing(p.seq, p.borders, WP, tP, p.Ws, thr, True, G, scored_P, p.scored)
    assert n_primary > 10 and pair.max() > 0
    ST.states("library_spacing", lambda: run(p.ds), lambda: run(p.prime),
              {"S": S, "R": R, "n": np.concatenate([[n_primary], pair, far]).astype(np.int64)})


@covers("kmap_refine_counts_packed_dev", "kmap_readscore_counts_library_dev")
@pytest.mark.parametrize("select_best", [True, False])
def test_refine_and_library_counts(env, select_best):
    """Reference: tests/_refine_model.np_counts per matrix; select_best also through the batched entry."""
    from tests._refine_model import np_counts
    p = pwm_set(env)

    def run(d):
        out = {}
        for m in (0, 8):
            Cm, n_hits, n_sel, n_minus = d.pwm_counts(p.Ws[m], p.thr[m], True, select_best)
            out[f"counts{m}"], out[f"n{m}"] = Cm, np.array([n_hits, n_sel, n_minus], np.int64)
        if select_best:
            mats, sel, minus = d.library_counts(p.Ws, p.thr, True)
            out.update({f"lib{m}": c for m, c in enumerate(mats)}, sel=sel, minus=minus)
        return out
    want, models = {}, [np_counts(p.seq, p.borders, W, t, True, select_best, sc) for W, t, sc in zip(p.Ws, p.thr, p.scored)]
    for m in (0, 8):
        want[f"counts{m}"], want[f"n{m}"] = models[m][0].astype(np.int64), np.array(models[m][1:], np.int64)
    if select_best:
        want.update({f"lib{m}": r[0].astype(np.int64) for m, r in enumerate(models)}, sel=np.array([r[2] for r in models], np.int64),
                    minus=np.array([r[3] for r in models], np.int64))
    ST.states(f"refine counts best={select_best}", lambda: run(p.ds), lambda: run(p.prime), want)


@covers("kmap_erase_pwm_sites_dev")
def test_erase_sites(env):
    """Reference: tests/_erase_model.np_erase (the working mask is restored before every run)."""
    from tests._erase_model import np_erase
    p = pwm_set(env)
    thr = [t + 200 for t in p.thr]

    def run(d):
        d.reset()
        n_hits, n_cov, n_new = d.erase_sites(p.Ws, thr, True)
        out = d.download()
        d.reset()
        return {"seq": out, "hits": n_hits, "covered": n_cov, "new": np.array([n_new], np.int64)}
    erased, n_hits, n_cov, n_new = np_erase(p.seq, p.borders, p.Ws, thr, True)
    assert n_hits.sum() > 0 and n_new > 0
    ST.states("erase_sites", lambda: run(p.ds), lambda: run(p.prime),
              {"seq": erased, "hits": n_hits.astype(np.int64), "covered": n_cov.astype(np.int64), "new": np.array([n_new], np.int64)})


@covers("kmap_pwm_scan_packed_dev", "kmap_pwm_scan_fetch")
def test_pwm_scan(env):
    """Reference: tests/_refine_model.np_scan."""
    from tests._refine_model import np_scan
    p = pwm_set(env)
    W, t = p.Ws[5], p.thr[5]

    def run(d):
        hits, pos, scores, strand = d.scan_pwm(W, t, True)
        return {"hits": hits, "pos": pos}
    hits, loc, _, _ = np_scan(p.seq, p.borders, W, t, True, p.scored[5])
    ST.states("scan_pwm", lambda: run(p.ds), lambda: run(p.prime), {"hits": hits.astype(np.int32), "pos": loc.astype(np.int32)})


@covers("kmap_refine_counts_packed_dev")
def test_pass_a_beyond_4096_tiles(env):
    """pwm_pass_a on 4100 wave tiles of 1024 positions: the scan of its tile counts takes the tiled form with slots C and D while
    the hit bits, tile counts and offsets lie in HASH, B and PART and the accumulators in A.  Reference: the vectorised
    tests/_refine_model.np_counts."""
    _ffi, DeviceCounts, DeviceSeq, O = env
    from tests._refine_model import asym_matrix, np_counts
    rng = np.random.default_rng(4096)
    W = asym_matrix(6, rng)

    def reads(n_reads):
        seq = rng.integers(0, 4, size=n_reads * 128).astype(np.uint8)
        seq[127::128] = 255
        seq[rng.random(len(seq)) < 0.001] = 255
        starts = np.arange(n_reads, dtype=np.int64) * 128
        return seq, np.ascontiguousarray(np.stack([starts, starts + 127], axis=1))
    seq, borders = reads(4100 * 8)
    pseq, pborders = reads(4700 * 8)
    assert (len(seq) + 1023) // 1024 > 4096
    t = int(np.asarray(W).max(axis=0).sum()) - 150           # near the top score: few hits
    ds, prime = DeviceSeq(seq, borders), DeviceSeq(pseq, pborders)

    def run(d):
        Cm, n_hits, n_sel, n_minus = d.pwm_counts(W, t, True, True)
        return {"counts": Cm, "n": np.array([n_hits, n_sel, n_minus], np.int64)}
    try:
        Cm, n_hits, n_sel, n_minus = np_counts(seq, borders, W, t, True, True)
        assert n_hits > 100
        ST.states("pass A, 4100 tiles", lambda: run(ds), lambda: run(prime),
                  {"counts": Cm.astype(np.int64), "n": np.array([n_hits, n_sel, n_minus], np.int64)})
    finally:
        ds.close()
        prime.close()


# ---- the rest -----------------------------------------------------------------------------------------------------------------------------
@covers("kmap_shuffle_packed_dev")
@pytest.mark.parametrize("klet", [1, 2])
def test_shuffle(env, klet):
    """Reference: tests/_shuffle_model.shuffle_array (the segment starts and lengths lie in slots B and C, the counters in A)."""
    _ffi, DeviceCounts, DeviceSeq, O = env
    from tests._shuffle_model import shuffle_array
    seq, borders = synth(np.random.default_rng(320 + klet), 120, 20, 160)
    pseq, pborders = synth(np.random.default_rng(330 + klet), 500, 20, 160)
    ds, prime = DeviceSeq(seq, borders), DeviceSeq(pseq, pborders)

    def run(d):
        out = d.shuffled(klet, 77)
        try:
            return {"seq": out.download(), "valid": np.array([out.shuffle_stats[1]], np.int64)}
        finally:
            out.close()
    try:
        want = shuffle_array(seq, klet, 77)
        ST.states(f"shuffle klet={klet}", lambda: run(ds), lambda: run(prime), {"seq": want, "valid": np.array([(seq != 255).sum()], np.int64)})
    finally:
        ds.close()
        prime.close()


@covers("kmap_hamball_extract")
@pytest.mark.parametrize("k", [12, 17])
def test_hamball_extract(env, k):
    """3000 table entries (three blocks of the count and write kernels; their block counts and offsets lie in slots A and B).
    Reference: oracle.ex_hamball and oracle.cal_cnt_mat."""
    _ffi, DeviceCounts, DeviceSeq, O = env
    from kmap_amd import reports as R
    rng = np.random.default_rng(1000 + k)
    cons = int(rng.integers(0, 4 ** k))

    def table(n):
        near = np.full(n // 2, cons, np.uint64)
        for _ in range(2):
            near = near ^ (rng.integers(1, 4, len(near)).astype(np.uint64) << (2 * rng.integers(0, k, len(near))).astype(np.uint64))
        u = np.unique(np.concatenate([near, rng.integers(0, 4 ** k, n, dtype=np.uint64)]))[:n]
        return u.astype(O.get_hash_dtype(k)), rng.integers(1, 1000, len(u)).astype(O.get_cnt_dtype(k))
    u, c = table(3000)
    pu, pc = table(12000)

    def run(u, c):
        ou, oc, mat = R._hamball_extract(u, c, k, cons, 2, True)
        return {"uniq": ou, "cnt": oc, "mat": mat}
    wu, wc = O.ex_hamball(u, c, k, cons, 2, True)
    assert len(wu) > 100
    ST.states(f"hamball_extract k={k}", lambda: run(u, c), lambda: run(pu, pc),
              {"uniq": wu, "cnt": wc, "mat": np.asarray(O.cal_cnt_mat(wu, wc, k)).astype(np.int64)})


@covers("kmap_label_prefix_dev", "kmap_label_members_dev", "kmap_prefix_search_dev", "kmap_label_sums_dev")
def test_label_prefix_members_and_search(env):
    """5000 labelled keys: the prefix sums take the tiled scan (more than 4096 items, slots C and D; kmap_label_sums_dev,
    _members_dev and _prefix_search_dev take no scratch themselves and read what it wrote).  Reference: numpy, as
    tests/_table_model.py states it (label_sums, members_of, cdf_hits)."""
    _ffi, DeviceCounts, DeviceSeq, O = env
    from tests import _table_model as TM
    L = _ffi.lib()
    rng = np.random.default_rng(310)

    def data(n):
        return rng.integers(0, 4, n).astype(np.uint8), rng.integers(1, 1000, n).astype(np.int32)

    def run(lab, cnt):
        n = len(lab)
        bufs = [_ffi.DeviceBuffer.from_numpy(lab), _ffi.DeviceBuffer.from_numpy(cnt), _ffi.DeviceBuffer(n * 4), _ffi.DeviceBuffer((n + 1) * 8),
                _ffi.DeviceBuffer((n + 1) * 8)]
        lab_d, cnt_d, w_d, excl_d, excl1_d = bufs
        try:
            wsum, members = np.zeros(4, np.int64), np.zeros(4, np.int64)
            _ffi.check(L.kmap_label_sums_dev(lab_d.ptr, cnt_d.ptr, 0, n, 4, _ffi.ptr(wsum), _ffi.ptr(members)))
            _ffi.check(L.kmap_label_prefix_dev(lab_d.ptr, cnt_d.ptr, 0, n, 1, w_d.ptr, excl_d.ptr, None))
            _ffi.check(L.kmap_label_prefix_dev(lab_d.ptr, None, 0, n, 1, w_d.ptr, excl1_d.ptr, None))
            _ffi.sync()
            targets = np.ascontiguousarray(np.arange(50, dtype=np.int64) * int(wsum[1]) // 50)
            hit, mem = np.full(50, -1, np.int64), np.full(int(members[1]), -1, np.int64)
            _ffi.check(L.kmap_prefix_search_dev(excl_d.ptr, n, _ffi.ptr(targets), 50, _ffi.ptr(hit)))
            _ffi.check(L.kmap_label_members_dev(lab_d.ptr, excl1_d.ptr, n, 1, len(mem), _ffi.ptr(mem)))
            return {"sums": np.concatenate([wsum, members]), "excl": excl_d.to_numpy(np.uint64, (n + 1,)), "hit": hit, "members": mem}
        finally:
            for b in bufs:
                b.free()
    lab, cnt = data(5000)
    plab, pcnt = data(40000)
    wsum, members = TM.label_sums(lab.astype(np.int64), cnt, 12, 4)
    w = np.where(lab == 1, cnt, 0)
    targets = np.arange(50, dtype=np.int64) * int(wsum[1]) // 50
    ST.states("label prefix / members / search", lambda: run(lab, cnt), lambda: run(plab, pcnt),
              {"sums": np.array(list(wsum) + list(members), np.int64), "excl": np.concatenate([[0], np.cumsum(w)]).astype(np.uint64),
               "hit": np.asarray(TM.cdf_hits(w, targets)).astype(np.int64), "members": TM.members_of(lab, 1)})

@covers("kmap_locations_sort")
def test_locations_sort(env):
    """tests/test_gpu_locations.test_sort_at_tile_edges at 4097 keys (one consensus, one hit per row, a key wider than 64 bits):
    both scans of csrc/locations.hip and the digit scans of the radix sort pass 4096 items and take slots C and D.  The primer has
    20 001 keys.  Reference: that file's _numpy_expected."""
    from kmap_amd.locations import locate
    from kmap_amd.reports import Occurrence
    from tests.test_gpu_locations import _key_bits, _numpy_expected
    rng = np.random.default_rng(77)
    n_bed, L = 2_500_000, 12

    class Bed:
        pass
    bed = Bed()
    bed.n_rows, bed.n_chrom = n_bed, 25
    bed.start = rng.integers(2 ** 32, 2 ** 33, n_bed).astype(np.int64)
    bed.chrom_rank = rng.integers(0, 25, n_bed).astype(np.int32)

    def rows(M):
        seq_ind = (1_000_000 + rng.choice(1_500_000, M, replace=False)).astype(np.int64)
        pos = rng.integers(0, 200, M).astype(np.int32)
        seq_ind[-1], pos[-1] = seq_ind[0], pos[0]            # two keys equal in every field, far apart in the input
        return seq_ind, pos, np.ones(M, np.int32)

    def run(seq_ind, pos, hits):
        row, start, end = locate(bed, Occurrence([hits], [pos], np.full(len(hits), 200), seq_ind), ["A" * L], all_rows=True)[0]
        return {"row": row, "start": start, "end": end}
    case, prime = rows(4097), rows(20001)
    assert _key_bits(bed, case[0], case[1], L) > 64
    row, start, end = _numpy_expected(bed.start, bed.chrom_rank, case[0], case[2], case[1], L)
    ST.states("locations sort, 4097 keys", lambda: run(*case), lambda: run(*prime), {"row": row, "start": start, "end": end})


@covers("kmap_match_tables_dev", "kmap_match_pairs_dev", "kmap_match_hist_dev")
@pytest.mark.parametrize("revcom", [True, False])
def test_match(env, revcom):
    """the 7 queries and 37 targets of tests/test_gpu_match.py (null tables, then all pairs; the packed query and target records
    lie in slots A and B) behind a primer of 37 queries on 74 targets.  That file holds the tables to tests/_match_model.py within
    rtol 1e-9 and the pairs to the model's configurations, not bit for bit (the model sums in another order); so here the cold
    result gets exactly those checks, and the three warm results must be the cold one bit for bit."""
    from kmap_amd import motif_match as K
    from tests import _match_model as M
    from tests import test_gpu_match as TM
    motifs = kept("motifs", TM.Motifs)
    H, n = motifs.hist(revcom)
    widths = [len(h) for h in H]
    min_lens = [min(4, w) for w in widths]
    pH = np.concatenate([M.null_hist(u, M.library_columns(motifs.ut, revcom)) for u in motifs.ut])
    p_widths = list(TM.T_WIDTHS)
    assert len(pH) == sum(p_widths)

    def run(queries, targets, hist, w, ml):
        tables, offsets = K.null_tables(hist, n, w, ml)
        res = K.match_motifs(queries, targets, revcom, 5)
        return {"tables": tables, "offsets": np.asarray(offsets, np.int64), "p": res.p_best, "o": res.o, "strand": res.strand, "L": res.L, "x": res.x}

    def check(got):
        covered = 0
        for q, (w, ml) in enumerate(zip(widths, min_lens)):
            for (a, b), (_, sf) in M.null_tables(H[q], n, ml).items():
                at = int(got["offsets"][q]) + K.table_offset(a, b, w, ml)
                dev = got["tables"][at:at + len(sf)]
                np.testing.assert_array_equal(dev == 0.0, sf == 0.0, err_msg=f"zeros of query {q} range {a}..{b}")
                np.testing.assert_allclose(dev, sf, rtol=TM.RTOL, atol=0.0, err_msg=f"query {q} range {a}..{b}")
                covered += len(sf)
        assert covered == len(got["tables"])
        res = K.MatchResult(got["p"], got["o"], got["strand"], got["L"], got["x"])
        TM.check_pairs(res, lambda q, t: motifs.configurations(q, t, 5, revcom), len(TM.Q_WIDTHS), len(TM.T_WIDTHS))
    ST.states(f"match revcom={revcom}", lambda: run(motifs.queries, motifs.targets, np.concatenate(H), widths, min_lens),
              lambda: run(motifs.targets, motifs.targets + motifs.targets, pH, p_widths, [min(4, w) for w in p_widths]), check=check)


# ---- handles ----------------------------------------------------------------------------------------------------------------------------
class _Scan:
    """a kmap_scan handle of its own on a DeviceSeq's arrays"""

    def __init__(self, _ffi):
        self._ffi, self.L = _ffi, _ffi.lib()
        h = _ffi.vp()
        _ffi.check(self.L.kmap_scan_create(C.byref(h)))
        self.h = h.value

    def run(self, d, k, cons, r):
        tot = self._ffi.i64(0)
        self._ffi.check(self.L.kmap_scan_run_packed_dev(self.h, d.codes.ptr, d.inval_orig.ptr, d.n, d.borders.ptr, d.n_seq, k, cons, r, 1,
                                                        C.byref(tot), d.planes.ptr if k <= 16 else None, None))
        self.n_seq, self.total = d.n_seq, tot.value

    def summary(self):
        nhit, mx = self._ffi.i64(-1), self._ffi.i32(-1)
        self._ffi.check(self.L.kmap_scan_summary(self.h, C.byref(nhit), C.byref(mx), None))
        return np.array([nhit.value, mx.value], np.int64)

    def fetch(self):
        hits, pos = np.full(self.n_seq, -1, np.int32), np.full(self.total, -1, np.int32)
        self._ffi.check(self.L.kmap_scan_fetch_stream(self.h, self._ffi.ptr(hits), self._ffi.ptr(pos), None))
        return hits, pos

    def fetch_u8(self):
        hits, pos = np.full(self.n_seq, 0xEE, np.uint8), np.full(self.total, -1, np.int32)
        self._ffi.check(self.L.kmap_scan_fetch_stream_u8(self.h, self._ffi.ptr(hits), self._ffi.ptr(pos), None))
        return hits, pos

    def close(self):
        self.L.kmap_scan_destroy(self.h)


def scan_lists(s):
    summary = s.summary()
    hits, pos = s.fetch()
    hits8, pos8 = s.fetch_u8()
    return {"summary": summary, "hits": hits, "pos": pos, "hits_u8": hits8, "pos_u8": pos8, "summary_again": s.summary()}


def scan_lists_reference(hits, pos):
    summary = np.array([np.count_nonzero(hits), hits.max(initial=0)], np.int64)
    return {"summary": summary, "hits": hits, "pos": pos, "hits_u8": np.minimum(hits, 255).astype(np.uint8), "pos_u8": pos, "summary_again": summary}


@covers("kmap_scan_run_packed_dev", "kmap_scan_summary", "kmap_scan_fetch_stream", "kmap_scan_fetch_stream_u8")
@pytest.mark.parametrize("k,r", [(8, 2), (20, 8)], ids=["bitsliced", "wide"])
def test_scan_handle_after_a_larger_run(env, k, r):
    """a 30 000-read scan, then a 7-read scan on the same handle: hits, positions, summary and the byte counts staged in the
    handle's offset array.  Reference: ko_scan_read."""
    _ffi, DeviceCounts, DeviceSeq, O = env
    big_seq, big_borders = synth(np.random.default_rng(30 + k), 30_000, 25, 60)
    seq, borders = synth(np.random.default_rng(31 + k), 7, 25, 60)
    cons = first_kmer(O, seq, borders, k)
    big, small = DeviceSeq(big_seq, big_borders), DeviceSeq(seq, borders)

    def run_small(s):
        s.run(small, k, cons, r)
        return scan_lists(s)
    try:
        hits, pos = oracle_scan(O, seq, borders, k, cons, r, True)
        assert hits.sum() > 0
        ST.reused(f"scan handle k={k}", lambda: _Scan(_ffi), lambda s: (s.run(big, k, cons, r), scan_lists(s)), run_small,
                  scan_lists_reference(hits, pos))
    finally:
        big.close()
        small.close()


FETCH_ORDERS = ["summary u8 summary i32", "i32 summary u8", "u8 u8", "u8 summary i32", "summary u8 i32 summary"]


@covers("kmap_scan_summary", "kmap_scan_fetch_stream", "kmap_scan_fetch_stream_u8")
def test_scan_fetch_orders(env):
    """kmap_scan_summary keeps its statistics in the first 16 bytes of the handle's dead offset array and kmap_scan_fetch_stream_u8
    stages the byte counts 64 bytes into it: on one result, five orders of the three entries must give the same lists and
    statistics every time.  Reference: ko_scan_read."""
    _ffi, DeviceCounts, DeviceSeq, O = env
    seq, borders = synth(np.random.default_rng(40), 1200, 25, 90)
    cons = first_kmer(O, seq, borders, 8)
    ds = DeviceSeq(seq, borders)
    hits, pos = oracle_scan(O, seq, borders, 8, cons, 2, True)
    want = {"summary": np.array([np.count_nonzero(hits), hits.max()], np.int64), "i32": (hits, pos),
            "u8": (np.minimum(hits, 255).astype(np.uint8), pos)}
    s = _Scan(_ffi)
    try:
        s.run(ds, 8, cons, 2)
        for order in FETCH_ORDERS:
            for step, what in enumerate(order.split()):
                got = {"summary": s.summary, "i32": s.fetch, "u8": s.fetch_u8}[what]()
                d = ST.first_difference(got, want[what])
                assert d is None, f"order '{order}', step {step} ({what}): {d[1]}"
    finally:
        s.close()
        ds.close()


@covers("kmap_counts_run_packed_dev", "kmap_counts_fetch")
def test_counts_handle_through_four_k(env):
    """k = 16, then 8, then 19, then 12 on ONE handle (two-level partition, LDS histograms, sort path, fine partition: the
    handle's table arrays shrink and change their key width), each equal to the oracle -- which the same k on fresh handles equals
    in test_counts."""
    _ffi, DeviceCounts, DeviceSeq, O = env
    host, ds, _, _ = count_pair(env, "k12_fine")
    dc = DeviceCounts()
    try:
        for k in (16, 8, 19, 12):
            got = counted(ds, dc, k, 1, 1)
            fresh = DeviceCounts()
            try:
                alone = counted(ds, fresh, k, 1, 1)
            finally:
                fresh.close()
            u, c = O.count_kmers(host.seq, host.borders, k, False, True)
            for name, res in (("fresh handle", alone), ("reused handle", got)):
                d = ST.first_difference(res, {"uniq": u, "cnt": c})
                assert d is None, f"k={k}, {name}: {d[1]}"
    finally:
        dc.close()


@covers("kmap_mask_hamball_packed_dev", "kmap_counts_run_packed_dev", "kmap_scan_run_packed_dev")
def test_device_seq_mask_count_scan_restore_count(env):
    """DeviceSeq: mask, count (working mask), scan (original mask), restore the working mask, count again.  Reference:
    oracle.mask_input, oracle.count_kmers on the masked and on the original reads, ko_scan_read."""
    _ffi, DeviceCounts, DeviceSeq, O = env
    k = 8
    seq, borders = synth(np.random.default_rng(50), 2000, 25, 120)
    cons = np.array([first_kmer(O, seq, borders, k), int(O.kmer2hash("T" * k))], np.uint64)
    rad = np.array([1, 0])
    masked = O.mask_input(seq.copy(), k, cons, rad)
    ds, dc = DeviceSeq(seq, borders), DeviceCounts()
    try:
        ds.mask(k, cons, rad)
        steps = [("masked reads", ds.download(), masked)]
        u, c = O.count_kmers(masked, borders, k, False, True)
        steps.append(("count after the mask", counted(ds, dc, k, 1, 1), {"uniq": u, "cnt": c}))
        hits, pos = oracle_scan(O, seq, borders, k, int(cons[0]), 2, True)
        steps.append(("scan", scanned(ds, k, int(cons[0]), 2), {"hits": hits, "pos": pos}))
        ds.reset()
        steps.append(("restored reads", ds.download(), seq))
        u, c = O.count_kmers(seq, borders, k, False, True)
        steps.append(("count after the restore", counted(ds, dc, k, 1, 1), {"uniq": u, "cnt": c}))
        for name, got, want in steps:
            d = ST.first_difference(got, want)
            assert d is None, f"{name}: {d[1]}"
    finally:
        dc.close()
        ds.close()


@covers("kmap_enrich_set_control", "kmap_enrich_run")
@pytest.mark.parametrize("revcom", [0, 1])
def test_enrich_handle_after_a_larger_control(env, revcom):
    """the enrich handle: a control table of 65 537 keys, then one of 999 keys on the same handle (its directory and control arrays
    only grow); b of 1000 foreground keys.  Reference: tests/test_gpu_enrich.expected_b (exact integers) for b; z within that
    file's bound of exact arithmetic (check_scores), and bit for bit what a fresh handle gives."""
    _ffi, DeviceCounts, DeviceSeq, O = env
    from kmap_amd.enrichment import DeviceEnrich
    from tests import test_gpu_enrich as TE
    k = 12
    rng = np.random.default_rng(1200 + revcom)

    def table(n):
        return TE.sample_keys(rng, 4 ** k, n), rng.integers(1, 1000, n).astype(np.uint64)
    big_keys, big_cnt = table(65537)
    bkeys, bcnt = table(999)
    fkeys = np.concatenate([bkeys[::3], TE.rc_keys(bkeys[1::3], k), big_keys[::97]])
    fkeys = rng.permutation(np.unique(fkeys))[:1000]
    a = rng.integers(1, 1000, len(fkeys)).astype(np.uint64)
    Nf, Nb = int(a.sum()), int(bcnt.sum()) * (2 if revcom else 1)
    tables = [DeviceCounts() for _ in range(3)]
    dc_f, dc_b, dc_big = tables
    TE.load_table(dc_f, fkeys, a, k)
    TE.load_table(dc_b, bkeys, bcnt, k)
    TE.load_table(dc_big, big_keys, big_cnt, k)
    z_seen = []

    def small(en):
        en.set_control(dc_b, revcom)
        en.run(dc_f, Nf, Nb, 1)
        b, z = en.result()
        z_seen.append(z)
        return {"b": b}

    def big(en):
        en.set_control(dc_big, revcom)
        en.run(dc_f, Nf, int(big_cnt.sum()) * (2 if revcom else 1), 1)
    try:
        want = TE.expected_b(fkeys, bkeys, bcnt, k, revcom)
        assert (want > 0).sum() > 200
        ST.reused(f"enrich handle revcom={revcom}", DeviceEnrich, big, small, {"b": want.astype(np.uint64)})
        fresh, again = z_seen
        TE.check_scores(want.astype(np.uint64), again, a.astype(object), want, Nf, Nb, "reused handle")
        assert ST.same(fresh, again), "z on the reused handle differs from z on a fresh handle"
    finally:
        for t in tables:
            t.close()
