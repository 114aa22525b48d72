"""What the device entry points write outside what they owe, and what they read outside what they were given.

tests/test_gpu_alignment.py guards the entries that branch on a caller's pointer; this file gives the same check to the other
entries that write a caller-owned device array.  Every array, input or output, lies in a `tests/_footprint.Guarded` buffer; a
case runs twice (output fill 0xA5 / 0x5A, input guard fill 0x00 / 0xFF): every owed byte must be written, the two runs must
agree with each other and with the reference, and every guard band must be intact.  Inputs and shapes are those of each entry's
own test, at the smallest size that still spans two workgroups."""
import ctypes as C

import numpy as np
import pytest

from tests import _footprint as F
from tests._footprint import free, guards, host, ok
from tests._packed_model import packed_groups, ref_pack, ref_planes
from tests.test_gpu_kmer_ops import synth_reads

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    from kmap_amd import _ffi
    return _ffi.lib()


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


# ---- reverse complement -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [11, 16, 31])
@pytest.mark.parametrize("n", [1, 255, 256, 257])                      # a block is 256 hashes
def test_revcom_footprint(L, O, n, k):
    rng = np.random.default_rng(n + k)
    dt = np.dtype(O.get_hash_dtype(k))
    h = rng.integers(0, 4 ** k, size=n, dtype=np.uint64).astype(dt)
    want = O.get_revcom_hash_arr(h, k)
    fn = L.kmap_revcom_u32_dev if dt == np.uint32 else L.kmap_revcom_u64_dev

    def case(out_fill, in_fill):
        hd = F.Guarded.of(h, fill=in_fill, name="in")
        out = F.Guarded(n * dt.itemsize, fill=out_fill, name="out")
        ok(fn(hd.ptr, n, k, out.ptr, None))
        np.testing.assert_array_equal(out.payload(dt), want)
        guards(hd, out)
        free(hd)
        return [out]
    F.run_twice(case)


# ---- per-read de-duplication (in place) -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [4, 16])                                 # the uint32 / the uint64 entry
def test_dedupe_per_read_footprint(L, O, k):
    """Low-complexity reads of ragged lengths, one of 513 positions (the long-read path, 512 is the LDS kernel's longest), more than
    four reads (a second block).  The borders skip every other separator-delimited stretch: hashes outside every border pair --
    duplicates of each other -- and the guard bands stay as they were."""
    rng = np.random.default_rng(k)
    lens = [0, 1, 2, 63, 64, 65, 513, 3, 0, 77, 40, 40]
    parts, borders, st = [], [], 0
    for i, n_ in enumerate(lens):
        read = np.tile(rng.integers(0, 4, size=11), n_ // 11 + 1)[:n_]   # period 11: duplicates at every k from 27 positions on
        read[n_ // 2:n_ // 2 + 1] ^= 1                                 # ... but for the windows over one changed base
        parts += [read.astype(np.uint8), np.array([255], np.uint8)]
        if i % 4 != 3:                                                 # reads 3, 7 and 11 belong to no border pair
            borders.append((st, st + n_))
        st += n_ + 1
    seq, borders = np.concatenate(parts), np.array(borders, np.int64)
    h = O.comp_kmer_hash(seq, k)
    dt = h.dtype
    outside = np.ones(len(h), bool)
    for s, e in borders:
        outside[s:e] = False
    h[outside] = 5                                                     # the same valid hash at every position no read owns
    want = O.remove_duplicate_hash_per_seq(h.copy(), borders)
    assert (want != h).any() and np.all(want[outside] == 5)
    fn = L.kmap_dedupe_per_read_u32_dev if dt == np.uint32 else L.kmap_dedupe_per_read_u64_dev

    def case(out_fill, in_fill):
        hd = F.Guarded.of(h, fill=out_fill, name="hash")
        bd = F.Guarded.of(borders, fill=in_fill, name="borders")
        ok(fn(hd.ptr, len(h), bd.ptr, len(borders), None))
        np.testing.assert_array_equal(hd.payload(dt), want)
        guards(hd, bd)
        free(bd)
        return [hd]
    F.run_twice(case)


# ---- Hamming-ball mask (in place) ---------------------------------------------------------------------------------------------------
def mask_case(O, k, r):
    """reads of tests/test_gpu_kmer_ops.test_mask_vs_oracle_random without the last separator: the array ends inside a read, whose
    last k - 1 windows pass the end, hash as invalid and so match the poly-T consensus"""
    rng = np.random.default_rng(11 + k)
    seq, _ = synth_reads(rng, 40, 30, 150)
    seq = seq[:-1].copy()
    seq[-k:] = rng.integers(0, 4, k)
    cons = rng.integers(0, 4 ** k, size=3, dtype=np.uint64)
    cons[0] = int(O.kmer2hash("T" * k))
    cons[1] = int(O.comp_kmer_hash(seq[100:100 + k], k)[0]) if seq[100:100 + k].max() < 4 else cons[1]
    rad = np.array([r, r, 0], np.int32)
    want = O.mask_input(seq.copy(), k, cons, rad)
    assert len(seq) > 512 and np.all(want[-(k - 1):] == 255) and (want != seq).sum() > k
    return seq, cons, rad, want


@pytest.mark.parametrize("k,r", [(6, 1), (8, 2), (17, 7)])
def test_mask_hamball_footprint(L, O, k, r):
    seq, cons, rad, want = mask_case(O, k, r)

    def case(out_fill, in_fill):
        s = F.Guarded.of(seq, fill=out_fill, name="seq")
        ok(L.kmap_mask_hamball_dev(s.ptr, len(seq), k, host(cons), host(rad), len(cons), None))
        np.testing.assert_array_equal(s.payload(np.uint8), want)
        guards(s)
        return [s]
    F.run_twice(case)


@pytest.mark.parametrize("with_planes", [False, True], ids=["windows", "planes"])
@pytest.mark.parametrize("k,r", [(6, 1), (8, 2), (17, 7)])
def test_mask_hamball_packed_footprint(L, O, k, r, with_planes):
    """in place on inval: kmap_packed_groups(n) words, the masked positions' bits ORed in; the codes (an input) stay as they are.
    Without planes_dev: k > 16 masks window by window, k <= 16 is refused and writes nothing (include/kmap_hip.h)."""
    from kmap_amd import _ffi
    seq, cons, rad, want = mask_case(O, k, r)
    n = len(seq)
    codes, inval, _ = ref_pack(seq, np.random.default_rng(k))
    refused = k <= 16 and not with_planes
    want_inval = inval if refused else ref_pack(want)[1]
    planes = ref_planes(codes)

    def case(out_fill, in_fill):
        c, i = F.Guarded.of(codes, fill=in_fill, name="codes"), F.Guarded.of(inval, fill=out_fill, name="inval")
        p = F.Guarded.of(planes, fill=in_fill, name="planes")
        rc = L.kmap_mask_hamball_packed_dev(c.ptr, i.ptr, n, k, host(cons), host(rad), len(cons), p.ptr if with_planes else None, None)
        if refused:
            assert rc == -1 and "planes" in _ffi.last_error()
            rc = 0
        ok(rc)
        np.testing.assert_array_equal(i.payload(np.uint16), want_inval)
        np.testing.assert_array_equal(c.payload(np.uint32), codes)
        guards(c, i, p)
        free(c, p)
        return [i]
    F.run_twice(case)


@pytest.mark.parametrize("m", [0, 1, 15, 16, 17, 1025])                # a block is 64 groups = 1024 positions
def test_inval_set_prefix_footprint(L, m):
    """positions [0, m) become invalid: bits ORed into ceil(m / 16) words, every other word and bit as it was"""
    n = 2000
    rng = np.random.default_rng(m)
    inval = rng.integers(0, 65536, size=packed_groups(n)).astype(np.uint16)
    inval[:3] = 0
    want = inval.copy()
    bits = (np.arange(len(want) * 16) < m).reshape(-1, 16)
    want |= np.bitwise_or.reduce(bits.astype(np.uint16) << (15 - np.arange(16)).astype(np.uint16), axis=1)
    assert m == 0 or (want != inval).any()

    def case(out_fill, in_fill):
        i = F.Guarded.of(inval, fill=out_fill, name="inval")
        ok(L.kmap_inval_set_prefix_dev(i.ptr, m, None))
        np.testing.assert_array_equal(i.payload(np.uint16), want)
        guards(i)
        return [i]
    F.run_twice(case)


@pytest.mark.parametrize("n", [1, 16, 17, 8161, 8192, 8193])           # a block is 256 group pairs = 8192 positions (+ the halo)
def test_pack_planes_footprint(L, n):
    """exactly kmap_packed_groups(n) words written, the halo's included"""
    rng = np.random.default_rng(n)
    ng = packed_groups(n)
    codes = rng.integers(0, 2 ** 32, size=ng, dtype=np.uint64).astype(np.uint32)
    want = ref_planes(codes)

    def case(out_fill, in_fill):
        c = F.Guarded.of(codes, fill=in_fill, name="codes")
        p = F.Guarded(ng * 4, fill=out_fill, name="planes")
        ok(L.kmap_pack_planes_dev(c.ptr, n, p.ptr, None))
        np.testing.assert_array_equal(p.payload(np.uint32), want)
        guards(c, p)
        free(c)
        return [p]
    F.run_twice(case)


# ---- synthetic reads ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_reads,read_len", [(1, 5), (37, 30), (300, 40)])   # 6, 1147 and 12 300 bytes: none a multiple of 16
def test_synth_reads_footprint(L, n_reads, read_len):
    """n_reads * (read_len + 1) bytes, the last thread's 16-byte store cut short: separators are 255, all else 0..3, the borders
    are exact, the planted motif is there, and nothing lies behind the last separator"""
    n_bytes = n_reads * (read_len + 1)
    assert n_bytes % 16
    motif = np.array([0, 2, 2, 0, 1], np.uint8)
    want_b = np.arange(n_reads, dtype=np.int64)[:, None] * (read_len + 1) + np.array([0, read_len], np.int64)
    seen = []

    def case(out_fill, in_fill):
        seq, borders = F.Guarded(n_bytes, fill=out_fill, name="seq"), F.Guarded(n_reads * 16, fill=out_fill, name="borders")
        ok(L.kmap_synth_reads_dev(seq.ptr, borders.ptr, n_reads, read_len, 7, host(motif), host(np.array([5], np.int32)),
                                  host(np.array([1.0])), 1, 0.0, None))
        got = seq.payload(np.uint8).reshape(n_reads, read_len + 1)
        assert np.all(got[:, read_len] == 255) and got[:, :read_len].max() <= 3
        win = np.lib.stride_tricks.sliding_window_view(got[:, :read_len], 5, axis=1)
        assert (win == motif).all(axis=2).any(axis=1).all(), "mutation_rate 0, fraction 1: every read carries the motif"
        np.testing.assert_array_equal(borders.payload(np.int64, (n_reads, 2)), want_b)
        seen.append(got)
        guards(seq, borders)
        return [seq, borders]
    F.run_twice(case)
    np.testing.assert_array_equal(seen[0], seen[1])


# ---- labelled sampling: label / prefix / search / members / gather -------------------------------------------------------------------
HOST_SENT = -0x5A5A5A5A5A5A5A5B


def host_out(m, dtype=np.int64):
    """a host output of m elements with one sentinel element in front of and behind it -> (whole array, pointer to element 1)"""
    a = np.full(m + 2, HOST_SENT, np.int64).view(np.uint8)[:(m + 2) * np.dtype(dtype).itemsize].view(dtype).copy()
    return a, C.c_void_p(a.ctypes.data + a.itemsize)


def host_ok(a, m):
    fill = np.full(1, HOST_SENT, np.int64).view(np.uint8)[:a.itemsize].view(a.dtype)[0]
    assert len(a) == m + 2 and a[0] == fill and a[-1] == fill, "written outside the host output"
    return a[1:-1]


@pytest.mark.parametrize("name", ["n_1", "n_4097"])                    # one block; the tile scan's second tile (4096 per tile)
def test_label_path_footprint(L, name):
    """tests/test_gpu_table_queries.test_cdf_prefix_and_search's tables through the raw entries: kmap_label_kmers_dev re-orients
    uniq_dev in place (n keys) and writes n labels; kmap_label_prefix_dev writes n + 1 prefix sums (and at most n scratch words);
    kmap_prefix_search_dev, kmap_label_members_dev and kmap_gather_dev write m host elements."""
    from tests import test_gpu_table_queries as T
    k, n, raw, cons, radius_of_len = T._cdf_case(name)
    rng = np.random.default_rng(n)
    u = T._keys(rng, k, n)
    cnt = T._counts(raw, k)
    wlab, wu = T._model_labels(u, cons, k, radius_of_len, True)
    wlab = np.asarray(wlab)
    cons_kh = np.array([T._hash(s) for s in cons], np.uint64)
    lens = np.array([len(s) for s in cons], np.int32)
    rads = np.array([radius_of_len[len(s)] for s in cons], np.int32)
    c = int(np.bincount(wlab, minlength=len(cons) + 1).argmax())       # the label with most members
    mem = T.M.members_of(wlab, c)
    w = np.where(wlab == c, raw, 0)
    excl_w = np.concatenate([[0], np.cumsum(w, dtype=np.int64)]).astype(np.uint64)
    excl_1 = np.concatenate([[0], np.cumsum(wlab == c, dtype=np.int64)]).astype(np.uint64)
    targets = np.unique(np.clip(np.concatenate([[0], excl_w.astype(np.int64) - 1, excl_w.astype(np.int64)]), 0, int(excl_w[-1]) - 1))
    targets = np.ascontiguousarray(targets[:: max(1, len(targets) // 300)], np.int64)
    idx = np.ascontiguousarray(rng.integers(0, n, size=257), np.int64)

    def case(out_fill, in_fill):
        ud, lab = F.Guarded.of(u, fill=out_fill, name="uniq"), F.Guarded(n, fill=out_fill, name="label")
        ok(L.kmap_label_kmers_dev(ud.ptr, n, k, len(cons), host(cons_kh), host(lens), host(rads), radius_of_len[k], 1, lab.ptr, None))
        np.testing.assert_array_equal(lab.payload(np.uint8), wlab)
        np.testing.assert_array_equal(ud.payload(u.dtype), np.asarray(wu).astype(u.dtype))
        cd = F.Guarded.of(cnt, fill=in_fill, name="cnt")
        scratch, excl = F.Guarded(n * 4, fill=out_fill, name="scratch"), F.Guarded((n + 1) * 8, fill=out_fill, name="excl")
        ok(L.kmap_label_prefix_dev(lab.ptr, cd.ptr, int(cnt.dtype == np.int64), n, c, scratch.ptr, excl.ptr, None))
        np.testing.assert_array_equal(excl.payload(np.uint64), excl_w)
        hit, hit_p = host_out(len(targets))
        ok(L.kmap_prefix_search_dev(excl.ptr, n, host(targets), len(targets), hit_p))
        np.testing.assert_array_equal(host_ok(hit, len(targets)), T.M.cdf_hits(w, targets))
        excl1 = F.Guarded((n + 1) * 8, fill=out_fill, name="excl (members)")
        ok(L.kmap_label_prefix_dev(lab.ptr, None, 0, n, c, scratch.ptr, excl1.ptr, None))
        np.testing.assert_array_equal(excl1.payload(np.uint64), excl_1)
        got_mem, mem_p = host_out(len(mem))
        ok(L.kmap_label_members_dev(lab.ptr, excl1.ptr, n, c, len(mem), mem_p))
        np.testing.assert_array_equal(host_ok(got_mem, len(mem)), mem)
        for src, arr in ((ud, np.asarray(wu).astype(u.dtype)), (lab, wlab.astype(np.uint8))):
            got, got_p = host_out(len(idx), arr.dtype)
            ok(L.kmap_gather_dev(src.ptr, arr.itemsize, host(idx), len(idx), got_p))
            np.testing.assert_array_equal(host_ok(got, len(idx)), arr[idx])
        guards(ud, lab, cd, scratch, excl, excl1)
        free(cd, scratch)
        return [ud, lab, excl, excl1]
    F.run_twice(case)


# ---- best window per read, presence bit rows ------------------------------------------------------------------------------------------
def scored_reads(n_seq, seed):
    """n_seq reads of 0 .. 30 bases (tests/_refine_model.make_reads: 2 % invalid bases, first and last bases among them), packed"""
    from tests._refine_model import make_reads
    rng = np.random.default_rng(seed)
    lengths = rng.integers(0, 31, n_seq)
    lengths[0] = 20
    seq, borders = make_reads(lengths, rng)
    codes, inval, _ = ref_pack(seq, rng)
    return seq, np.ascontiguousarray(borders, np.int64), codes, inval


@pytest.mark.parametrize("n_seq", [1, 255, 256, 257])
def test_readscore_packed_footprint(L, n_seq):
    """score_dev, loc_dev and strand_dev hold n_seq elements each; reads shorter than the width are unscorable (INT32_MIN, -1, 0)"""
    from tests import _readscore_model as RM
    from tests._refine_model import asym_matrix, window_scores
    seq, borders, codes, inval = scored_reads(n_seq, 500 + n_seq)
    W = asym_matrix(9, np.random.default_rng(9))
    want = RM.np_read_scores(seq, borders, W, True, window_scores(seq, W))
    n_unscorable = int((np.asarray(want[1]) < 0).sum())
    assert n_seq == 1 or 0 < n_unscorable < n_seq

    def case(out_fill, in_fill):
        c, i = F.Guarded.of(codes, fill=in_fill, name="codes"), F.Guarded.of(inval, fill=in_fill, name="inval")
        b = F.Guarded.of(borders, fill=in_fill, name="borders")
        score, loc = F.Guarded(n_seq * 4, fill=out_fill, name="score"), F.Guarded(n_seq * 4, fill=out_fill, name="loc")
        strand = F.Guarded(n_seq, fill=out_fill, name="strand")
        n_scored = C.c_int64(-1)
        ok(L.kmap_readscore_packed_dev(c.ptr, i.ptr, len(seq), b.ptr, n_seq, 9, host(W), 1, score.ptr, loc.ptr, strand.ptr,
                                       C.byref(n_scored), None))
        np.testing.assert_array_equal(loc.payload(np.int32), want[1])
        np.testing.assert_array_equal(score.payload(np.int32), want[0])
        np.testing.assert_array_equal(strand.payload(np.uint8), want[2])
        assert n_scored.value == n_seq - n_unscorable
        guards(c, i, b, score, loc, strand)
        free(c, i, b)
        return [score, loc, strand]
    F.run_twice(case)


@pytest.mark.parametrize("n_mat", [1, 3])
@pytest.mark.parametrize("n_seq", [1, 63, 64, 65, 4097])
def test_presence_library_footprint(L, n_seq, n_mat):
    """every word of planes_dev (n_mat x (n_seq + 63) / 64) is written, the bits behind n_seq are 0, n_present holds n_mat counts"""
    from tests import _cooccurrence_model as CM
    from tests import _readscore_model as RM
    from tests._refine_model import asym_matrix, window_scores
    seq, borders, codes, inval = scored_reads(n_seq, 700 + n_seq)
    rng = np.random.default_rng(n_mat)
    mats = [asym_matrix(w, rng) for w in (4, 9, 16)[:n_mat]]
    scored = [window_scores(seq, W) for W in mats]
    ts = []
    for W, sc in zip(mats, scored):                                    # the median best score: about half of the scorable reads
        score, loc, _ = RM.np_read_scores(seq, borders, W, True, sc)
        best = np.asarray(score)[np.asarray(loc) >= 0]
        ts.append(int(np.median(best)) if len(best) else 0)
    bits = CM.np_presence(seq, borders, mats, ts, True, scored)
    assert n_seq < 63 or (bits.any(axis=1).all() and not bits.all(axis=1).any())
    n_words = (n_seq + 63) // 64
    widths, weights = np.zeros(n_mat, np.int32), np.zeros((n_mat, 4, 32), np.int32)
    for m, W in enumerate(mats):
        widths[m] = W.shape[1]
        weights[m, :, :W.shape[1]] = W
    thr = np.array(ts, np.int32)

    def case(out_fill, in_fill):
        c, i = F.Guarded.of(codes, fill=in_fill, name="codes"), F.Guarded.of(inval, fill=in_fill, name="inval")
        b = F.Guarded.of(borders, fill=in_fill, name="borders")
        planes = F.Guarded(n_mat * n_words * 8, fill=out_fill, name="planes")
        n_present, n_present_p = host_out(n_mat)
        ok(L.kmap_presence_library_dev(c.ptr, i.ptr, len(seq), b.ptr, n_seq, n_mat, host(widths), host(weights), host(thr), 1, planes.ptr,
                                       n_words, n_present_p, None))
        got = planes.payload(np.uint64, (n_mat, n_words))
        np.testing.assert_array_equal(got, CM.np_pack(bits))
        if n_seq % 64:
            assert not (got[:, -1] >> np.uint64(n_seq % 64)).any()
        np.testing.assert_array_equal(host_ok(n_present, n_mat), bits.sum(axis=1))
        guards(c, i, b, planes)
        free(c, i, b)
        return [planes]
    F.run_twice(case)


# ---- projection ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["k8n300", "k16n300"])                 # the uint32 / the uint64 entry
def test_project_knn_footprint(L, tag):
    """q_dev in place (m hashes), nb_dev and nb_dist_dev m x n_nb, flipped_dev m: 70 queries, more than one block"""
    from tests import test_gpu_project as P
    c = P.case(tag)
    m, n, k = len(c["q"]), c["n"], c["k"]
    fn = L.kmap_project_knn_u32_dev if c["q"].dtype == np.uint32 else L.kmap_project_knn_u64_dev

    def case(out_fill, in_fill):
        q, ref = F.Guarded.of(c["q"], fill=out_fill, name="q"), F.Guarded.of(c["ref"], fill=in_fill, name="ref")
        nb, dist = F.Guarded(m * P.N_NB * 4, fill=out_fill, name="nb"), F.Guarded(m * P.N_NB, fill=out_fill, name="nb_dist")
        flipped = F.Guarded(m, fill=out_fill, name="flipped")
        ok(fn(q.ptr, m, ref.ptr, n, k, 1, P.N_NB, nb.ptr, dist.ptr, flipped.ptr, None))
        np.testing.assert_array_equal(q.payload(c["q"].dtype), c["kh"])
        np.testing.assert_array_equal(nb.payload(np.int32, (m, P.N_NB)), c["nb"])
        np.testing.assert_array_equal(dist.payload(np.uint8, (m, P.N_NB)), c["nb_dist"])
        np.testing.assert_array_equal(flipped.payload(np.uint8), c["flip"].astype(np.uint8))
        guards(q, ref, nb, dist, flipped)
        free(ref)
        return [q, nb, dist, flipped]
    F.run_twice(case)


def test_project_prob_and_descend_row_range(L):
    """Queries [3, 3 + m - 5) of m = 70: p and Q rows are local to the range; of xy (2 x m) only entries [row0, row0 + nrows) of both
    planes are written.  The range's coordinates equal the whole run's bit for bit (a query's arithmetic is its own), and the whole
    run is held to the float64 oracle by the rule of test_start_and_descent_against_float64 at n_iter = 1."""
    from kmap_amd.projection import hd_prob_lut_projected
    from tests import test_gpu_project as P
    tag, n_iter = "k8n300", 1
    c = P.case(tag)
    n, k, m = c["n"], c["k"], len(c["nb"])
    lut3 = np.ascontiguousarray(hd_prob_lut_projected(k, P.N_NB), np.float32)
    lds = ldp = n + 4
    sums = np.full((n, lds), 0xEEEE, np.uint16)
    sums[:, :n] = c["Sref"]
    xy_of = {}
    for row0, nrows in ((0, m), (3, m - 5)):
        runs = []
        for out_fill, in_fill in F.FILLS:
            nb, s = F.Guarded.of(c["nb"], fill=in_fill, name="nb"), F.Guarded.of(sums, fill=in_fill, name="sums")
            lut, ref_xy = F.Guarded.of(lut3, fill=in_fill, name="lut"), F.Guarded.of(c["xy"].astype(np.float32), fill=in_fill, name="ref_xy")
            p = F.Guarded.pitched(nrows, n * 4, ldp * 4, fill=out_fill, name="p")
            xy = F.Guarded(2 * m * 4, fill=out_fill, name="xy")
            ok(L.kmap_project_prob_dev(nb.ptr, m, P.N_NB, s.ptr, lds, None, n, n, lut.ptr, len(lut3), row0, nrows, p.ptr, ldp, None, None))
            np.testing.assert_array_equal(p.rows(np.uint32), c["p"][row0:row0 + nrows].view(np.uint32))
            ok(L.kmap_project_descend_dev(p.ptr, ldp, nb.ptr, m, P.N_NB, ref_xy.ptr, n, row0, nrows, n_iter, P.LR, xy.ptr, None))
            raw = xy.payload(np.uint8).reshape(2, m, 4)
            owed = np.zeros(m, bool)
            owed[row0:row0 + nrows] = True
            assert np.all(raw[:, ~owed] == out_fill), "xy entries outside [row0, row0 + nrows) were written"
            runs.append(xy.payload(np.float32, (2, m))[:, owed])
            guards(nb, s, lut, ref_xy, p, xy)
            free(nb, s, lut, ref_xy, p, xy)
        np.testing.assert_array_equal(runs[0].view(np.uint32), runs[1].view(np.uint32))
        assert np.isfinite(runs[0]).all()
        xy_of[row0] = runs[0]
    np.testing.assert_array_equal(xy_of[3].view(np.uint32), xy_of[0][:, 3:m - 2].view(np.uint32))
    want, e32, _ = P.descent_oracle(tag, n_iter)
    err = np.abs(xy_of[0].astype(np.float64) - want)
    tol = np.maximum(4 * e32, 4 * np.spacing(np.abs(want).astype(np.float32)).astype(np.float64))
    assert (err <= tol).all(), (float(err.max()), e32)


# ---- count matrices against a library of count matrices: histograms, null tables, pairs ------------------------------------------------
_MATCH = {}


def match_case():
    """tests/test_gpu_match.Motifs (7 queries on 94 columns, 37 targets on 599: six blocks of 16 query columns, three tiles of 256
    library columns) with the reverse complement and min_overlap 5, built once: the quantised columns, the model's histograms, the
    host arrays of the queries and the model's sf tables laid out as kmap_match_tables_dev lays them out -- n_table doubles exactly"""
    if not _MATCH:
        from kmap_amd import motif_match as K
        from tests import test_gpu_match as T
        mo = T.Motifs()
        min_overlap = 5
        qcols = np.concatenate([K.quantise_columns(c) for c in mo.queries])
        lcols = np.concatenate([K.quantise_columns(c) for c in mo.targets])
        H, n_null = mo.hist(True)
        q_width = np.array(T.Q_WIDTHS, np.int32)
        t_width = np.array(T.T_WIDTHS, np.int32)
        min_len = min(min_overlap, int(t_width.min()))
        q_min_len = np.minimum(q_width, min_len).astype(np.int32)
        q_col0 = np.concatenate([[0], np.cumsum(q_width[:-1])]).astype(np.int64)
        t_col0 = np.concatenate([[0], np.cumsum(t_width[:-1])]).astype(np.int64)
        sizes = [K.table_doubles(int(w), int(m)) for w, m in zip(q_width, q_min_len)]
        q_toff = np.concatenate([[0], np.cumsum(sizes[:-1])]).astype(np.int64)
        n_table = int(sum(sizes))
        tables = np.full(n_table, np.nan)
        for q, per_range in enumerate(mo.tables(True, min_len)):
            for (a, b), (_, sf) in per_range.items():
                at = int(q_toff[q]) + K.table_offset(a, b, int(q_width[q]), int(q_min_len[q]))
                assert np.isnan(tables[at:at + len(sf)]).all()
                tables[at:at + len(sf)] = sf
        assert not np.isnan(tables).any()                              # the ranges tile the n_table doubles exactly
        assert len(qcols) == q_width.sum() > 5 * 16 and len(lcols) == t_width.sum() > 2 * 256
        _MATCH.update(mo=mo, qcols=qcols, lcols=lcols, H=np.concatenate(H).astype(np.uint32), n_null=n_null, q_width=q_width,
                      q_min_len=q_min_len, q_col0=q_col0, q_toff=q_toff, t_width=t_width, t_col0=t_col0, n_table=n_table,
                      tables=tables, min_overlap=min_overlap, rtol=T.RTOL, check_pairs=T.check_pairs, result=K.MatchResult)
    return _MATCH


def test_match_hist_footprint(L):
    """hist_dev: n_qcols x 91 uint32, every word written (the entry clears what its blocks add into)"""
    m = match_case()
    n_q, n_l = len(m["qcols"]), len(m["lcols"])

    def case(out_fill, in_fill):
        q, l_ = F.Guarded.of(m["qcols"], fill=in_fill, name="qcols"), F.Guarded.of(m["lcols"], fill=in_fill, name="lcols")
        hist = F.Guarded(n_q * 91 * 4, fill=out_fill, name="hist")
        ok(L.kmap_match_hist_dev(q.ptr, n_q, l_.ptr, n_l, 1, hist.ptr, None))
        got = hist.payload(np.uint32, (n_q, 91))
        np.testing.assert_array_equal(got, m["H"])
        assert (got.sum(axis=1) == m["n_null"]).all() and m["n_null"] == 2 * n_l
        guards(q, l_, hist)
        free(q, l_)
        return [hist]
    F.run_twice(case)


def test_match_tables_footprint(L):
    """tables_dev: exactly n_table doubles, every one written, the same bits in both runs; against the model's tables by the rule
    of tests/test_gpu_match.test_null_tables (the zeros where the model has zeros, rtol 1e-9 elsewhere)"""
    m = match_case()
    n_q, n_query, n_table = len(m["qcols"]), len(m["q_width"]), m["n_table"]

    def case(out_fill, in_fill):
        hist = F.Guarded.of(m["H"], fill=in_fill, name="hist")
        tab = F.Guarded(n_table * 8, fill=out_fill, name="tables")
        ok(L.kmap_match_tables_dev(hist.ptr, n_q, m["n_null"], n_query, host(m["q_width"]), host(m["q_col0"]), host(m["q_min_len"]),
                                   host(m["q_toff"]), tab.ptr, n_table, None))
        got = tab.payload(np.float64)
        np.testing.assert_array_equal(got == 0.0, m["tables"] == 0.0)
        np.testing.assert_allclose(got, m["tables"], rtol=m["rtol"], atol=0.0)
        guards(hist, tab)
        free(hist)
        return [tab]
    F.run_twice(case)


def test_match_pairs_footprint(L):
    """p_dev: n_query x n_target doubles, cfg_dev: four int32 per pair; the tables are the model's, so every p is a table entry"""
    m = match_case()
    mo = m["mo"]
    n_q, n_l, n_query, n_target, n_table = len(m["qcols"]), len(m["lcols"]), len(m["q_width"]), len(m["t_width"]), m["n_table"]

    def case(out_fill, in_fill):
        q, l_ = F.Guarded.of(m["qcols"], fill=in_fill, name="qcols"), F.Guarded.of(m["lcols"], fill=in_fill, name="lcols")
        tab = F.Guarded.of(m["tables"], fill=in_fill, name="tables")
        p, cfg = F.Guarded(n_query * n_target * 8, fill=out_fill, name="p"), F.Guarded(n_query * n_target * 16, fill=out_fill, name="cfg")
        ok(L.kmap_match_pairs_dev(q.ptr, n_q, n_query, host(m["q_width"]), host(m["q_col0"]), host(m["q_min_len"]), host(m["q_toff"]),
                                  tab.ptr, n_table, l_.ptr, n_l, n_target, host(m["t_width"]), host(m["t_col0"]), m["min_overlap"], 1,
                                  p.ptr, cfg.ptr, None))
        c = cfg.payload(np.int32, (n_query, n_target, 4))
        res = m["result"](p.payload(np.float64, (n_query, n_target)), *(np.ascontiguousarray(c[:, :, i]) for i in range(4)))
        if out_fill == F.FILLS[0][0]:                                  # the second run must equal the first bit for bit (run_twice)
            m["check_pairs"](res, lambda qi, ti: mo.configurations(qi, ti, m["min_overlap"], True), n_query, n_target)
        guards(q, l_, tab, p, cfg)
        free(q, l_, tab)
        return [p, cfg]
    F.run_twice(case)
