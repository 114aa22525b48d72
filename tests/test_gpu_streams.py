"""Every device entry point on a caller's own stream (tests/_stream_order.py has the choreography).

No other test passes a stream other than NULL, so none can see a launch, memset or copy inside an entry that forgot its stream, a
host read-back that waits for the wrong stream, or scratch that two streams share.  Here every entry with a `void *stream`
parameter runs on a stream of kmap_stream_create behind a delay, with its device inputs holding a decoy until the truth arrives
on that stream; its results must be the truth's.  `drive` runs one case:

  * the entry (or chain of entries) is issued by `issue(p, S, S2)`: p maps buffer names to device pointers, S is the stream under
    test, S2 a second stream for the fetches the product issues from other streams; it returns the host outputs as arrays;
  * the expected results come from `model(inputs)` where an existing test has a cheap model of the operation, and otherwise from the
    same `issue` on the null stream with full synchronisation (S = S2 = NULL) -- the existing tests hold that to their references.
    Every test's docstring says which of the two it uses.  Comparisons are bit for bit.

The three control cases give the entry stream NULL on purpose and must see the decoy's result: that proves that the delay is long
enough and that the two streams are unordered on this runtime.  If a control sees the truth, the cases of this file cannot
discriminate, and test_control_sees_the_decoy fails with that message.

The last test parses include/kmap_hip.h: an entry with a stream parameter must have a case here or a reason in NOT_COVERED."""
import ctypes as C
import os
import threading
from pathlib import Path

import numpy as np
import pytest

from tests import _footprint as F
from tests import _stream_order as SO
from tests._packed_model import packed_groups, ref_pack, ref_planes
from tests._stream_order import covers

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]


@pytest.fixture(scope="module")
def L():
    from kmap_amd import _ffi
    return _ffi.lib()


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


def chk(rc):
    from kmap_amd import _ffi
    _ffi.check(rc)


def sync(stream=None):
    from kmap_amd import _ffi
    _ffi.sync(stream)


def host(a):
    return F.host(a)


def i64():
    return C.c_int64(-1)


# ---- the driver -------------------------------------------------------------------------------------------------------------------
def _call(issue, p, S, S2, ctx):
    return dict((issue(p, S, S2) if ctx is None else issue(p, S, S2, ctx)) or {})


def _null_run(ins, inout, outs, issue, which, setup=None, teardown=None):
    """`issue` on the null stream, everything drained before and after: {name: array} of device outputs, in-place inputs and host
    outputs.  The buffers are laid out like the stream run's (same alignment, same guard bands)."""
    bufs = {}
    for name, pair in ins.items():
        bufs[name] = F.Guarded.of(pair[which], fill=SO.SENTINEL, name=name)
    for name, (dtype, shape) in outs.items():
        bufs[name] = F.Guarded(int(np.prod(shape)) * np.dtype(dtype).itemsize, fill=SO.SENTINEL, name=name)
    p = {name: b.ptr for name, b in bufs.items()}
    ctx = setup(p) if setup else None
    try:
        sync()
        res = _call(issue, p, None, None, ctx)
        sync()
    finally:
        if teardown:
            teardown(ctx)
    for name in inout:
        res[name] = bufs[name].payload(ins[name][which].dtype, ins[name][which].shape)
    for name, (dtype, shape) in outs.items():
        res[name] = bufs[name].payload(dtype, shape)
    for b in bufs.values():
        b.check_guards()
        b.free()
    return {k: np.asarray(v) for k, v in res.items()}


def expectations(name, ins, outs, issue, inout=(), model=None, twice=False, setup=None, teardown=None):
    """[expected results of the truth, of the decoy]: the null-stream reference, overridden by model(which) where it has a name"""
    want = [_null_run(ins, inout, outs, issue, w, setup, teardown) for w in (0, 1)]
    if twice:
        again = _null_run(ins, inout, outs, issue, 0, setup, teardown)
        for k in want[0]:
            assert SO.same(want[0][k], again[k]), f"{name}: {k}: two null-stream evaluations differ"
    if model is not None:
        for w in (0, 1):
            want[w].update({k: np.asarray(v) for k, v in model(w).items()})
    return want


def open_case(name, ins, outs, inout=(), delay_ms=None, stream=0):
    """the buffers of a stream run: (Case, {name: device pointer})"""
    c = SO.Case(name, delay_ms=SO.DELAY_MS if delay_ms is None else delay_ms, stream=stream)
    p = {}
    for k, (t, d) in ins.items():
        p[k] = (c.inout if k in inout else c.input)(k, t, d).ptr
    for k, (dtype, shape) in outs.items():
        p[k] = c.output(k, int(np.prod(shape)) * np.dtype(dtype).itemsize).ptr
    return c, p


def collect(c, got, ins, outs, inout=()):
    """the host outputs of a stream run plus the snapshots of its device outputs and in-place inputs"""
    got = {k: np.asarray(v) for k, v in got.items()}
    for k in inout:
        got[k] = c.snapshot(k, ins[k][0].dtype, ins[k][0].shape)
    for k, (dtype, shape) in outs.items():
        got[k] = c.snapshot(k, dtype, shape)
    return got


def compare(c, got, want, skip=(), escape=False):
    assert set(got) == set(want[0]) == set(want[1]), (sorted(got), sorted(want[0]))
    seen = {}
    for k in sorted(got):
        if k in skip:
            continue
        if escape:
            seen[k] = c.observed(k, want[0][k], want[1][k], got[k])
        else:
            c.expect(k, want[0][k], want[1][k], got[k])
    return seen


def _contig(ins):
    return {k: (np.ascontiguousarray(t), np.ascontiguousarray(d)) for k, (t, d) in ins.items()}


def drive(name, ins, outs, issue, inout=(), model=None, escape=False, delay_ms=None, stream=0, skip=(), twice=False, setup=None,
          teardown=None):
    """One case.  ins: {name: (truth, decoy)} device inputs; inout: the names among them that the entry changes in place;
    outs: {name: (dtype, shape)} device outputs; issue(p, S, S2) -> {name: host output}; model(which) -> {name: expected array} for
    which = 0 (truth) / 1 (decoy), overriding the null-stream reference for the names it returns; skip: names compared by the
    caller.  setup(p) -> ctx runs before the streams are drained (handles that allocate; issue then gets ctx as a fourth argument),
    teardown(ctx) after the run.  escape: the control -- returns {name: 'truth' / 'decoy' / 'other'} instead of asserting.  twice:
    require two null-stream evaluations of the truth to agree bit for bit first.  Returns the stream run's results."""
    ins = _contig(ins)
    want = expectations(name, ins, outs, issue, inout, model, twice, setup, teardown)
    S2 = SO.device().stream(stream + 1)
    c, p = open_case(name, ins, outs, inout, delay_ms, stream)
    ctx = None
    try:
        ctx = setup(p) if setup else None
        got = collect(c, c.run(lambda S: _call(issue, p, S, None if S is None else S2, ctx), escape=escape), ins, outs, inout)
        seen = compare(c, got, want, skip, escape)
    finally:
        if teardown and ctx is not None:
            teardown(ctx)
        c.finish()
    return seen if escape else got


# ---- read sets ----------------------------------------------------------------------------------------------------------------------
def read_pair(seed, n_reads=120, lo=20, hi=160, p_n=0.02):
    """(truth, decoy, borders): two read sets with the same borders -- 255 behind every read, p_n of the bases invalid -- and
    independent bases"""
    rng = np.random.default_rng(seed)
    lens = rng.integers(lo, hi + 1, size=n_reads)
    starts = np.concatenate([[0], np.cumsum(lens + 1)[:-1]])
    borders = np.ascontiguousarray(np.stack([starts, starts + lens], axis=1), np.int64)
    n = int((lens + 1).sum())
    out = []
    for _ in range(2):
        s = rng.integers(0, 4, n).astype(np.uint8)
        s[rng.random(n) < p_n] = 255
        s[borders[:, 1]] = 255
        out.append(s)
    return out[0], out[1], borders


def packed_pair(seq_t, seq_d, seed=0):
    """codes, inval and planes of both read sets: ((codes_t, codes_d), (inval_t, inval_d), (planes_t, planes_d))"""
    rng = np.random.default_rng(seed)
    ct, it, _ = ref_pack(seq_t, rng)
    cd, id_, _ = ref_pack(seq_d, rng)
    return (ct, cd), (it, id_), (ref_planes(ct), ref_planes(cd))


def hashes_pair(k, n, seed):
    rng = np.random.default_rng(seed)
    dt = np.uint32 if k < 16 else np.uint64
    return [rng.integers(0, 4 ** k, size=n, dtype=np.uint64).astype(dt) for _ in range(2)]


# ---- the control: the method can fail ---------------------------------------------------------------------------------------------
def _revcom_case(L, O, k=11, n=1000):
    h = hashes_pair(k, n, 1)
    dt = h[0].dtype
    fn = L.kmap_revcom_u32_dev if dt == np.uint32 else L.kmap_revcom_u64_dev
    return dict(ins={"in": (h[0], h[1])}, outs={"out": (dt, (n,))},
                issue=lambda p, S, S2: chk(fn(p["in"], n, k, p["out"], S)),
                model=lambda w: {"out": O.get_revcom_hash_arr(h[w], k)})


def _hash_packed_case(L, O, k=8):
    st, sd, _ = read_pair(2)
    n = len(st)
    codes, inval, _ = packed_pair(st, sd)
    return dict(ins={"codes": codes, "inval": inval}, outs={"out": (np.uint32, (n,))},
                issue=lambda p, S, S2: chk(L.kmap_hash_kmers_packed_dev(p["codes"], p["inval"], n, k, p["out"], S)),
                model=lambda w: {"out": O.comp_kmer_hash((st, sd)[w], k)})


def _matrix_case(L, O, n=300, k=8):
    """the general kernel: n below 4096, a pitch that is no multiple of 4 KiB; one label with a short consensus"""
    kh = hashes_pair(k, n, 3)
    rng = np.random.default_rng(4)
    lab = [rng.integers(0, 2, n).astype(np.int32) for _ in range(2)]
    clen = np.array([k, 5], np.int32)
    ld = n + 4
    return dict(ins={"kh": (kh[0], kh[1]), "label": (lab[0], lab[1])}, outs={"D": (np.uint8, (n, ld))},
                issue=lambda p, S, S2: chk(L.kmap_hamdist_matrix_u32_dev(p["kh"], p["label"], n, k, host(clen), 2, 0, n, p["D"], ld, S)),
                model=lambda w: {"D": np.pad(O.hamdist_matrix_u8(kh[w], lab[w], k, clen), ((0, 0), (0, ld - n)),
                                             constant_values=SO.SENTINEL)})


CONTROLS = {"kmap_revcom_u32_dev": _revcom_case, "kmap_hash_kmers_packed_dev": _hash_packed_case,
            "kmap_hamdist_matrix_u32_dev": _matrix_case}


def control_observations(L, O, delay_ms, reps=1):
    """what the three escaped entries show: {entry: ['decoy' | 'truth' | 'other', ...]}"""
    return {name: [next(iter(drive("control " + name, escape=True, delay_ms=delay_ms, **make(L, O)).values())) for _ in range(reps)]
            for name, make in CONTROLS.items()}


def test_control_sees_the_decoy(L, O):
    """Expected values: the oracle (get_revcom_hash_arr, comp_kmer_hash, hamdist_matrix_u8).  Three entries without any host
    synchronisation get stream NULL while the truth arrives on S behind the delay: they must compute the decoy's result."""
    seen = control_observations(L, O, SO.DELAY_MS)
    blind = {k: v for k, v in seen.items() if v != ["decoy"]}
    assert not blind, (f"the stream-order cases of this file cannot discriminate: an entry on the null stream saw {blind} although the "
                       f"truth only arrives behind a {SO.DELAY_MS} ms delay on another stream")


# ---- element-wise entries -----------------------------------------------------------------------------------------------------------
@covers("kmap_revcom_u32_dev", "kmap_revcom_u64_dev")
@pytest.mark.parametrize("k", [11, 20])
def test_revcom(L, O, k):
    """Expected values: oracle.get_revcom_hash_arr."""
    drive(f"revcom k={k}", **_revcom_case(L, O, k))


@covers("kmap_hash_kmers_u32_dev", "kmap_hash_kmers_u64_dev")
@pytest.mark.parametrize("k", [8, 20])
def test_hash_kmers(L, O, k):
    """Expected values: oracle.comp_kmer_hash."""
    st, sd, _ = read_pair(10 + k)
    n = len(st)
    dt = O.get_hash_dtype(k)
    fn = L.kmap_hash_kmers_u32_dev if np.dtype(dt) == np.uint32 else L.kmap_hash_kmers_u64_dev
    drive(f"hash_kmers k={k}", {"seq": (st, sd)}, {"out": (dt, (n,))}, lambda p, S, S2: chk(fn(p["seq"], n, k, p["out"], S)),
          model=lambda w: {"out": O.comp_kmer_hash((st, sd)[w], k)})


@covers("kmap_hamdist_1vN_u32_dev", "kmap_hamdist_1vN_u64_dev")
@pytest.mark.parametrize("k", [11, 20])
def test_hamdist_1vN(L, O, k):
    """Expected values: oracle.cal_hamming_dist_head (the head form: shift 2 (k - clen), clen bases)."""
    n, clen = 1000, k - 3
    h = hashes_pair(k, n, 20 + k)
    cons = int(np.random.default_rng(k).integers(0, 4 ** clen))
    fn = L.kmap_hamdist_1vN_u32_dev if k < 16 else L.kmap_hamdist_1vN_u64_dev
    drive(f"hamdist_1vN k={k}", {"h": (h[0], h[1])}, {"out": (np.uint8, (n,))},
          lambda p, S, S2: chk(fn(p["h"], n, cons, 2 * (k - clen), clen, p["out"], S)),
          model=lambda w: {"out": np.asarray(O.cal_hamming_dist_head(h[w], cons, k, clen)).astype(np.uint8)})


def _low_complexity_pair(seed, n_reads=80):
    """reads with a period of 11 bases (duplicates at every k), one base changed per read"""
    rng = np.random.default_rng(seed)
    lens = rng.integers(20, 161, size=n_reads)
    starts = np.concatenate([[0], np.cumsum(lens + 1)[:-1]])
    borders = np.ascontiguousarray(np.stack([starts, starts + lens], axis=1), np.int64)
    out = []
    for _ in range(2):
        s = np.full(int((lens + 1).sum()), 255, np.uint8)
        for a, n_ in zip(starts, lens):
            r = np.tile(rng.integers(0, 4, size=11), n_ // 11 + 1)[:n_]
            r[n_ // 2] ^= 1
            s[a:a + n_] = r
        out.append(s)
    return out[0], out[1], borders


@covers("kmap_dedupe_per_read_u32_dev", "kmap_dedupe_per_read_u64_dev")
@pytest.mark.parametrize("k", [4, 16])
def test_dedupe_per_read(L, O, k):
    """Expected values: oracle.remove_duplicate_hash_per_seq.  In place on the hash array; the borders are the truth's in both."""
    st, sd, borders = _low_complexity_pair(30 + k)
    h = [O.comp_kmer_hash(s, k) for s in (st, sd)]
    fn = L.kmap_dedupe_per_read_u32_dev if h[0].dtype == np.uint32 else L.kmap_dedupe_per_read_u64_dev
    want = [O.remove_duplicate_hash_per_seq(x.copy(), borders) for x in h]
    assert (want[0] != h[0]).any()
    drive(f"dedupe k={k}", {"hash": (h[0], h[1]), "borders": (borders, borders)}, {},
          lambda p, S, S2: chk(fn(p["hash"], len(h[0]), p["borders"], len(borders), S)), inout=("hash",),
          model=lambda w: {"hash": want[w]})


def _mask_inputs(O, k, seed):
    """both read sets, consensuses taken from windows of each (so each is masked somewhere) and the radii"""
    st, sd, borders = read_pair(seed)
    cons = []
    for s in (st, sd):
        at = next(a for a in range(50, len(s)) if s[a:a + k].max() < 4)
        cons.append(int(O.comp_kmer_hash(s[at:at + k], k)[0]))
    cons = np.array(cons + [int(O.kmer2hash("T" * k))], np.uint64)
    rad = np.array([1, 1, 0], np.int32)
    want = [O.mask_input(s.copy(), k, cons, rad) for s in (st, sd)]
    assert (want[0] != st).any() and (want[1] != sd).any()
    return st, sd, borders, cons, rad, want


@covers("kmap_mask_hamball_dev")
def test_mask_hamball(L, O):
    """Expected values: oracle.mask_input.  In place on the uint8 array."""
    k = 8
    st, sd, _, cons, rad, want = _mask_inputs(O, k, 40)
    drive("mask_hamball", {"seq": (st, sd)}, {},
          lambda p, S, S2: chk(L.kmap_mask_hamball_dev(p["seq"], len(st), k, host(cons), host(rad), len(cons), S)), inout=("seq",),
          model=lambda w: {"seq": want[w]})


@covers("kmap_mask_hamball_packed_dev")
@pytest.mark.parametrize("k", [8, 18])
def test_mask_hamball_packed(L, O, k):
    """Expected values: oracle.mask_input, packed by tests/_packed_model.ref_pack.  k = 8 runs bit-sliced on the planes, k = 18
    window by window without them."""
    st, sd, _, cons, rad, want = _mask_inputs(O, k, 41 + k)
    n = len(st)
    codes, inval, planes = packed_pair(st, sd)
    drive(f"mask_hamball_packed k={k}", {"codes": codes, "inval": inval, "planes": planes}, {},
          lambda p, S, S2: chk(L.kmap_mask_hamball_packed_dev(p["codes"], p["inval"], n, k, host(cons), host(rad), len(cons),
                                                             p["planes"] if k <= 16 else None, S)), inout=("inval",),
          model=lambda w: {"inval": ref_pack(want[w])[1]})


@covers("kmap_inval_set_prefix_dev")
def test_inval_set_prefix(L):
    """Expected values: numpy (bits of positions [0, m) ORed into the mask words)."""
    n, m = 2000, 1025
    rng = np.random.default_rng(50)
    inval = [rng.integers(0, 65536, size=packed_groups(n)).astype(np.uint16) for _ in range(2)]
    bits = (np.arange(packed_groups(n) * 16) < m).reshape(-1, 16)
    add = np.bitwise_or.reduce(bits.astype(np.uint16) << (15 - np.arange(16)).astype(np.uint16), axis=1)
    drive("inval_set_prefix", {"inval": (inval[0], inval[1])}, {}, lambda p, S, S2: chk(L.kmap_inval_set_prefix_dev(p["inval"], m, S)),
          inout=("inval",), model=lambda w: {"inval": inval[w] | add})


@covers("kmap_pack_reads_dev", "kmap_pack_planes_dev", "kmap_hash_kmers_packed_dev", "kmap_unpack_reads_dev")
def test_packed_chain(L, O):
    """pack -> planes -> hash -> unpack chained on S with no synchronisation in between.  Expected values: ref_pack's invalid mask,
    oracle.comp_kmer_hash, and the reads themselves (they hold 0..3 and 255 only); the codes are compared on the valid positions
    (the code bits of an invalid position are not part of the contract) and the planes with ref_planes of the codes found."""
    k = 8
    st, sd, _ = read_pair(60)
    n, ng = len(st), packed_groups(len(st))
    packed = [ref_pack(s) for s in (st, sd)]

    def issue(p, S, S2):
        chk(L.kmap_pack_reads_dev(p["seq"], n, p["codes"], p["inval"], S))
        chk(L.kmap_pack_planes_dev(p["codes"], n, p["planes"], S))
        chk(L.kmap_hash_kmers_packed_dev(p["codes"], p["inval"], n, k, p["hash"], S))
        chk(L.kmap_unpack_reads_dev(p["codes"], p["inval"], n, p["back"], S))
    got = drive("packed chain", {"seq": (st, sd)},
                {"codes": (np.uint32, (ng,)), "inval": (np.uint16, (ng,)), "planes": (np.uint32, (ng,)), "hash": (np.uint32, (n,)),
                 "back": (np.uint8, (n,))}, issue, skip=("codes", "planes"),
                model=lambda w: {"inval": packed[w][1], "hash": O.comp_kmer_hash((st, sd)[w], k), "back": (st, sd)[w]})
    np.testing.assert_array_equal(got["codes"] & packed[0][2], packed[0][0])
    assert (packed[0][0] != (packed[1][0] & packed[0][2])).any()
    np.testing.assert_array_equal(got["planes"], ref_planes(got["codes"]))


# ---- counting ---------------------------------------------------------------------------------------------------------------------
def read_pair_exact(seed, n_total):
    """read_pair with exactly n_total array positions"""
    rng = np.random.default_rng(seed)
    lens = []
    left = n_total
    while left > 0:
        ln = int(rng.integers(20, 161))
        if left - (ln + 1) < 21:                                       # the last read takes what is left
            ln = left - 1
        lens.append(ln)
        left -= ln + 1
    lens = np.array(lens, np.int64)
    starts = np.concatenate([[0], np.cumsum(lens + 1)[:-1]])
    borders = np.ascontiguousarray(np.stack([starts, starts + lens], axis=1), np.int64)
    out = []
    for _ in range(2):
        s = rng.integers(0, 4, n_total).astype(np.uint8)
        s[rng.random(n_total) < 0.02] = 255
        s[borders[:, 1]] = 255
        out.append(s)
    assert len(out[0]) == n_total
    return out[0], out[1], borders


def rc_pair(seed, n_base=12, length=70, copies=3):
    """about 5000 positions: n_base reads, each `copies` times and as often reverse-complemented: repeated k-mers with their
    reverse-complement partners present at any k"""
    rng = np.random.default_rng(seed)
    n_reads = n_base * copies * 2
    starts = np.arange(n_reads, dtype=np.int64) * (length + 1)
    borders = np.ascontiguousarray(np.stack([starts, starts + length], axis=1), np.int64)
    out = []
    for _ in range(2):
        base = rng.integers(0, 4, size=(n_base, length)).astype(np.uint8)
        rows = np.concatenate([base] * copies + [3 - base[:, ::-1]] * copies)
        rows = rows[rng.permutation(n_reads)]
        s = np.full(n_reads * (length + 1), 255, np.uint8)
        s.reshape(n_reads, length + 1)[:, :length] = rows
        s[rng.integers(0, len(s), 40)] = 255
        out.append(s)
    return out[0], out[1], borders


_COUNT_DATA = {}


def count_data(O, k):
    """the read pair of a k and its expected tables, built once: k = 8 the LDS pass, 12 and 15 the partitioned passes on 2^20 + 17
    positions, 19 the sort path on repeated k-mers with reverse-complement partners"""
    if k not in _COUNT_DATA:
        st, sd, borders = rc_pair(100 + k) if k >= 17 else read_pair_exact(100 + k, (1 << 20) + 17) if k >= 12 else read_pair(100 + k)
        _COUNT_DATA[k] = dict(seq=(st, sd), borders=borders, tables={})
    return _COUNT_DATA[k]


def count_tables(O, k, dedupe, merge, with_borders=True):
    d = count_data(O, k)
    key = (dedupe, merge, with_borders)
    if key not in d["tables"]:
        d["tables"][key] = [O.count_kmers(s, d["borders"] if with_borders else None, k, not dedupe, merge) for s in d["seq"]]
    return d["tables"][key]


def table_results(L, O, h, k, n_uniq, S, S2, merge):
    """what the product reads of a finished table.  The counting entries return the number of entries while the kernel that writes
    the table may still be in flight on S, so S is drained first, as include/kmap_hip.h demands of every reader on another stream
    (the product's background saver does the same).  Then both arrays through kmap_counts_fetch_stream and kmap_counts_write_range on
    S2 (kmap_counts_fetch without a stream), and the stream-less kmap_counts_total, _topk and _hamball_mass."""
    from kmap_amd import _ffi
    sync(S)
    u, c = np.empty(n_uniq, O.get_hash_dtype(k)), np.empty(n_uniq, O.get_cnt_dtype(k))
    if S2 is None:
        chk(L.kmap_counts_fetch(h, _ffi.ptr(u), _ffi.ptr(c)))
    else:
        chk(L.kmap_counts_fetch_stream(h, _ffi.ptr(u), _ffi.ptr(c), S2))
    first, count = n_uniq // 3, n_uniq - n_uniq // 3 - 1
    fd = os.memfd_create("kmap_write_range")
    try:
        chk(L.kmap_counts_write_range(h, 0, first, count, fd, 16, S2))
        chk(L.kmap_counts_write_range(h, 1, first, count, fd, 16 + count * u.itemsize, S2))
        raw = os.pread(fd, 16 + count * (u.itemsize + c.itemsize) + 1, 0)
    finally:
        os.close(fd)
    total, n_found = i64(), C.c_int(-1)
    chk(L.kmap_counts_total(h, C.byref(total)))
    idx, kh, cnt = np.full(5, -1, np.int64), np.zeros(5, np.uint64), np.full(5, -1, np.int64)
    chk(L.kmap_counts_topk(h, 5, _ffi.ptr(idx), _ffi.ptr(kh), _ffi.ptr(cnt), C.byref(n_found)))
    cands = np.ascontiguousarray(u[:3], np.uint64)
    mass = np.zeros(3, np.float64)
    chk(L.kmap_counts_hamball_mass(h, _ffi.ptr(cands), 3, 1, int(merge), _ffi.ptr(mass)))
    assert (mass == np.rint(mass)).all()
    return {"uniq": u, "cnt": c, "file": np.frombuffer(raw, np.uint8),
            "stats": np.concatenate([[n_uniq, total.value, n_found.value], idx, cnt, mass]).astype(np.int64)}


def table_model(O, k, table, merge):
    from tests import _table_model as TM
    u, c = table
    first, count = len(u) // 3, len(u) - len(u) // 3 - 1
    idx, cnt = TM.table_topk(c, k, 5)
    raw = np.concatenate([np.zeros(16, np.uint8), u[first:first + count].view(np.uint8), c[first:first + count].view(np.uint8)])
    return {"uniq": u, "cnt": c, "file": raw,
            "stats": np.concatenate([[len(u), TM.table_total(c, k), len(idx)], idx, cnt, TM.ball_mass(u, c, k, u[:3], 1, merge)]).astype(np.int64)}


def counted(L, run):
    """issue(p, S, S2) of a counting case: a fresh handle, `run(h, p, S)` -> (n_uniq, what to read of the table)"""
    def issue(p, S, S2):
        h = C.c_void_p()
        chk(L.kmap_counts_create(C.byref(h)))
        try:
            return run(h, p, S, S2)
        finally:
            chk(L.kmap_counts_destroy(h))
    return issue


@covers("kmap_counts_run_seq_dev", "kmap_counts_run_hashes_dev", "kmap_counts_run_packed_dev", "kmap_counts_fetch_stream",
        "kmap_counts_write_range")
@pytest.mark.parametrize("k", [8, 12, 15, 19])
@pytest.mark.parametrize("entry", ["seq", "hashes", "packed"])
def test_counts_run(L, O, entry, k):
    """Expected values: oracle.count_kmers for the table, tests/_table_model.py for total, top-k and Hamming-ball mass.  The table
    is fetched and written into a file on a second stream S2; kmap_counts_total / _topk / _hamball_mass follow kmap_stream_sync(S)."""
    d = count_data(O, k)
    (st, sd), borders = d["seq"], d["borders"]
    n, n_seq, merge, dedupe = len(st), len(borders), 1, int(entry != "hashes")
    tables = count_tables(O, k, dedupe, merge, entry != "hashes")
    if k == 19:
        rc = O.get_revcom_hash_arr(tables[0][0], k)
        assert tables[0][1].max() > 1 and len(tables[0][0]) < (O.comp_kmer_hash(st, k) != O.get_invalid_hash(O.get_hash_dtype(k))).sum() / 2
        assert not np.isin(rc[rc != tables[0][0]], tables[0][0]).any()           # the partners were merged away
    if entry == "seq":
        ins = {"seq": (st, sd), "borders": (borders, borders)}

        def run(h, p, S, S2):
            nu = i64()
            chk(L.kmap_counts_run_seq_dev(h, p["seq"], n, p["borders"], n_seq, k, dedupe, merge, C.byref(nu), S))
            return table_results(L, O, h, k, nu.value, S, S2, merge)
    elif entry == "hashes":
        ins = {"hash": tuple(O.comp_kmer_hash(s, k) for s in (st, sd))}

        def run(h, p, S, S2):
            nu = i64()
            chk(L.kmap_counts_run_hashes_dev(h, p["hash"], n, k, merge, C.byref(nu), S))
            return table_results(L, O, h, k, nu.value, S, S2, merge)
    else:
        codes, inval, _ = packed_pair(st, sd)
        ins = {"codes": codes, "inval": inval, "borders": (borders, borders)}

        def run(h, p, S, S2):
            nu = i64()
            chk(L.kmap_counts_run_packed_dev(h, p["codes"], p["inval"], n, p["borders"], n_seq, k, dedupe, merge, C.byref(nu), S))
            return table_results(L, O, h, k, nu.value, S, S2, merge)
    drive(f"counts_run_{entry} k={k}", ins, {}, counted(L, run), model=lambda w: table_model(O, k, tables[w], merge))


@covers("kmap_counts_hist_packed_dev", "kmap_counts_finish")
def test_counts_hist_and_finish(L, O):
    """Expected values: oracle.count_kmers / tests/_table_model.py.  The two halves of the all-reduce form, chained on S."""
    k, merge = 11, 1
    d = count_data(O, 8)
    (st, sd), borders = d["seq"], d["borders"]
    codes, inval, _ = packed_pair(st, sd)
    tables = [O.count_kmers(s, borders, k, False, True) for s in (st, sd)]

    def run(h, p, S, S2):
        nu = i64()
        chk(L.kmap_counts_hist_packed_dev(h, p["codes"], p["inval"], len(st), p["borders"], len(borders), k, 1, S))
        chk(L.kmap_counts_finish(h, k, merge, C.byref(nu), S))
        return table_results(L, O, h, k, nu.value, S, S2, merge)
    drive("counts hist + finish", {"codes": codes, "inval": inval, "borders": (borders, borders)}, {}, counted(L, run),
          model=lambda w: table_model(O, k, tables[w], merge))


@covers("kmap_counts_presence_dev", "kmap_counts_merge_presence_dev", "kmap_counts_finish_range")
def test_counts_presence_path(L, O):
    """Expected values: oracle.count_kmers / tests/_table_model.py for the table (one rank: the whole key range is its slice); the
    nibble array from numpy (bin x present -> nibble x of byte x / 2, low nibble for even x)."""
    k = 11
    d = count_data(O, 8)
    (st, sd), borders = d["seq"], d["borders"]
    codes, inval, _ = packed_pair(st, sd)
    tables = [O.count_kmers(s, borders, k, False, True) for s in (st, sd)]
    plain = [O.count_kmers(s, borders, k, False, False) for s in (st, sd)]
    n_bins = 4 ** k

    def nibbles(u):
        nib = np.zeros(n_bins // 2, np.uint8)
        u = u.astype(np.int64)
        np.bitwise_or.at(nib, u >> 1, np.where(u & 1, 16, 1).astype(np.uint8))
        return nib

    def run(h, p, S, S2):
        nu = i64()
        chk(L.kmap_counts_hist_packed_dev(h, p["codes"], p["inval"], len(st), p["borders"], len(borders), k, 1, S))
        chk(L.kmap_counts_presence_dev(h, k, p["nib"], S))
        chk(L.kmap_counts_merge_presence_dev(h, k, p["nib"], S))
        chk(L.kmap_counts_finish_range(h, k, 1, 0, n_bins, C.byref(nu), S))
        return table_results(L, O, h, k, nu.value, S, S2, 1)

    def model(w):
        out = table_model(O, k, tables[w], 1)
        out["nib"] = nibbles(plain[w][0])
        return out
    drive("counts presence path", {"codes": codes, "inval": inval, "borders": (borders, borders)}, {"nib": (np.uint8, (n_bins // 2,))},
          counted(L, run), model=model)


@covers("kmap_counts_run_packed_range_dev")
@pytest.mark.parametrize("first_bin,n_bins", [(4 ** 11 // 4, 4 ** 11 // 4), (8 * 12345, 777777)], ids=["prefix", "odd"])
def test_counts_run_packed_range(L, O, first_bin, n_bins):
    """Expected values: oracle.count_kmers' merged table, sliced by POSITION as tests/test_gpu_packed.py restates it: the position of
    an entry is its own key, but an unpaired higher member of a reverse-complement pair stays at its position with its key replaced
    by the partner's, so the positions come from the table without the merge."""
    k, merge = 11, 1
    d = count_data(O, 8)
    (st, sd), borders = d["seq"], d["borders"]
    codes, inval, _ = packed_pair(st, sd)
    tables = []
    for s in (st, sd):
        u0, _ = O.count_kmers(s, borders, k, False, False)
        p0 = u0.astype(np.uint64)
        r0 = O.get_revcom_hash_arr(u0, k).astype(np.uint64)
        present = np.isin(r0, p0)
        pos = p0[~(present & (p0 > r0))]
        u, c = O.count_kmers(s, borders, k, False, True)
        assert len(u) == len(pos) and (u.astype(np.uint64) == np.minimum(p0, r0)[~(present & (p0 > r0))]).all()
        keep = (pos >= first_bin) & (pos < first_bin + n_bins)
        tables.append((u[keep], c[keep]))
    assert len(tables[0][0]) > 10

    def run(h, p, S, S2):
        nu = i64()
        chk(L.kmap_counts_run_packed_range_dev(h, p["codes"], p["inval"], len(st), p["borders"], len(borders), k, 1, merge, first_bin,
                                               n_bins, C.byref(nu), S))
        return table_results(L, O, h, k, nu.value, S, S2, merge)
    drive("counts_run_packed_range", {"codes": codes, "inval": inval, "borders": (borders, borders)}, {}, counted(L, run),
          model=lambda w: table_model(O, k, tables[w], merge))


# ---- scans --------------------------------------------------------------------------------------------------------------------------
def scan_results(L, h, n_seq, total, S, S2, with_u8=True):
    """the protocol csrc/scan.hip documents: kmap_scan_summary on the stream of the run, then the fetches on another stream"""
    from kmap_amd import _ffi
    nhit, mx = i64(), C.c_int32(-1)
    chk(L.kmap_scan_summary(h, C.byref(nhit), C.byref(mx), S))
    hits, pos = np.full(n_seq, -1, np.int32), np.full(total, -1, np.int32)
    chk(L.kmap_scan_fetch_stream(h, _ffi.ptr(hits), _ffi.ptr(pos), S2))
    out = {"hits": hits, "pos": pos, "summary": np.array([total, nhit.value, mx.value], np.int64)}
    if with_u8:
        hits8, pos8 = np.full(n_seq, 0xEE, np.uint8), np.full(total, -1, np.int32)
        chk(L.kmap_scan_fetch_stream_u8(h, _ffi.ptr(hits8), _ffi.ptr(pos8), S2))
        out.update(hits_u8=hits8, pos_u8=pos8)
    return out


def scanned(L, run):
    def issue(p, S, S2):
        h = C.c_void_p()
        chk(L.kmap_scan_create(C.byref(h)))
        try:
            return run(h, p, S, S2)
        finally:
            chk(L.kmap_scan_destroy(h))
    return issue


def _consensus_of(O, seq, k, at=50):
    a = next(a for a in range(at, len(seq)) if seq[a:a + k].max() < 4)
    return int(O.comp_kmer_hash(seq[a:a + k], k)[0])


@covers("kmap_scan_run_packed_dev", "kmap_scan_summary", "kmap_scan_fetch_stream", "kmap_scan_fetch_stream_u8")
@pytest.mark.parametrize("k,r,n_reads", [(8, 2, 120), (8, 2, 6), (18, 6, 120)], ids=["k8", "short", "wide"])
def test_scan_run(L, O, k, r, n_reads):
    """Expected values: the same entries on the null stream with full synchronisation.  k8: the one-pass form; short: fewer than
    400 positions, the two-pass form; wide: csrc/scan_wide.hip.  Run and summary on S, both fetches on S2."""
    st, sd, borders = read_pair(200 + k + n_reads, n_reads=n_reads, hi=160 if n_reads > 6 else 60)
    n, n_seq = len(st), len(borders)
    assert n_reads > 6 or n < 400
    cons = _consensus_of(O, st, k, at=5)
    codes, inval, planes = packed_pair(st, sd)

    def run(h, p, S, S2):
        tot = i64()
        chk(L.kmap_scan_run_packed_dev(h, p["codes"], p["inval"], n, p["borders"], n_seq, k, cons, r, 1, C.byref(tot), p["planes"], S))
        return scan_results(L, h, n_seq, tot.value, S, S2)
    got = drive(f"scan k={k} n={n}", {"codes": codes, "inval": inval, "planes": planes, "borders": (borders, borders)}, {},
                scanned(L, run))
    assert got["summary"][0] > 0 and got["hits"].sum() == got["summary"][0]
    np.testing.assert_array_equal(got["hits_u8"], np.minimum(got["hits"], 255).astype(np.uint8))
    np.testing.assert_array_equal(got["pos_u8"], got["pos"])


@covers("kmap_scan_declare_uniform")
def test_scan_declare_uniform(L, O):
    """Expected values: the same entries on the null stream with full synchronisation.  Here the borders are the input under
    test: the truth's are uniform (read s = [41 s, 41 s + 40)), the decoy's end one base early in every third read -- still inside
    the reads, so a step that read them by mistake stays in bounds -- and the declaration is refused for them."""
    k, r, n_seq, ln = 8, 2, 150, 40
    rng = np.random.default_rng(210)
    st = rng.integers(0, 4, n_seq * (ln + 1)).astype(np.uint8)
    st[rng.random(len(st)) < 0.02] = 255
    st.reshape(n_seq, ln + 1)[:, ln] = 255
    sd = st.copy()
    bt = np.arange(n_seq, dtype=np.int64)[:, None] * (ln + 1) + np.array([0, ln], np.int64)
    bd = bt.copy()
    bd[::3, 1] -= 1
    cons = _consensus_of(O, st, k, at=ln - k)                          # the last window of read 0: outside the decoy's read 0
    codes, inval, planes = packed_pair(st, sd)
    n = len(st)

    def run(h, p, S, S2):
        ok, tot = C.c_int(-1), i64()
        chk(L.kmap_scan_declare_uniform(h, p["borders"], n_seq, ln, ln + 1, C.byref(ok), S))
        chk(L.kmap_scan_run_packed_dev(h, p["codes"], p["inval"], n, p["borders"], n_seq, k, cons, r, 1, C.byref(tot), p["planes"], S))
        out = scan_results(L, h, n_seq, tot.value, S, S2, with_u8=False)
        out["accepted"] = np.array([ok.value], np.int64)
        return out
    got = drive("scan_declare_uniform", {"codes": codes, "inval": inval, "planes": planes, "borders": (bt, bd)}, {}, scanned(L, run))
    assert got["accepted"][0] == 1


def pwm_reads(seed, n_seq=150):
    """two read sets of 0 .. 160 bases on the same borders (tests/_refine_model.make_reads: 2 % invalid, first and last bases too)"""
    from tests._refine_model import make_reads
    rng = np.random.default_rng(seed)
    lengths = rng.integers(20, 161, n_seq)
    lengths[:4] = [0, 3, 8, 9]
    st, borders = make_reads(lengths, rng)
    sd, _ = make_reads(lengths, rng)
    return st, sd, np.ascontiguousarray(borders, np.int64)


@covers("kmap_pwm_scan_packed_dev")
def test_pwm_scan(L):
    """Expected values: tests/_refine_model.np_scan.  Scan on S, summary on S, fetches on S2."""
    from tests._refine_model import asym_matrix, np_scan
    st, sd, borders = pwm_reads(220)
    W = asym_matrix(9, np.random.default_rng(9))
    t = 0
    n, n_seq = len(st), len(borders)
    codes, inval, _ = packed_pair(st, sd)

    def run(h, p, S, S2):
        tot = i64()
        chk(L.kmap_pwm_scan_packed_dev(h, p["codes"], p["inval"], n, p["borders"], n_seq, 9, host(W), t, 1, C.byref(tot), S))
        return scan_results(L, h, n_seq, tot.value, S, S2)

    def model(w):
        hits, loc, _, _ = np_scan((st, sd)[w], borders, W, t, True)
        return {"hits": hits, "pos": loc, "pos_u8": loc, "hits_u8": np.minimum(hits, 255).astype(np.uint8),
                "summary": np.array([len(loc), (hits > 0).sum(), hits.max()], np.int64)}
    got = drive("pwm_scan", {"codes": codes, "inval": inval, "borders": (borders, borders)}, {}, scanned(L, run), model=model)
    assert got["summary"][0] > 20


@covers("kmap_refine_counts_packed_dev")
@pytest.mark.parametrize("select_best", [0, 1])
def test_refine_counts(L, select_best):
    """Expected values: tests/_refine_model.np_counts.  Blocking: the host outputs are complete on return."""
    from kmap_amd import _ffi
    from tests._refine_model import asym_matrix, np_counts
    st, sd, borders = pwm_reads(230)
    W = asym_matrix(9, np.random.default_rng(9))
    n, n_seq = len(st), len(borders)
    codes, inval, _ = packed_pair(st, sd)

    def issue(p, S, S2):
        counts = np.full((4, 9), -1, np.int64)
        a, b, c = i64(), i64(), i64()
        chk(L.kmap_refine_counts_packed_dev(p["codes"], p["inval"], n, p["borders"], n_seq, 9, host(W), 0, 1, select_best, _ffi.ptr(counts),
                                            C.byref(a), C.byref(b), C.byref(c), S))
        return {"counts": counts, "n": np.array([a.value, b.value, c.value], np.int64)}

    def model(w):
        Cm, n_hits, n_sel, n_minus = np_counts((st, sd)[w], borders, W, 0, True, bool(select_best))
        return {"counts": Cm.astype(np.int64), "n": np.array([n_hits, n_sel, n_minus], np.int64)}
    drive(f"refine_counts best={select_best}", {"codes": codes, "inval": inval, "borders": (borders, borders)}, {}, issue, model=model)


@covers("kmap_readscore_packed_dev", "kmap_readscore_hist_dev")
def test_readscore_and_hist(L):
    """Expected values: tests/_readscore_model.np_read_scores and np_histogram.  The histogram reads the three arrays the first
    entry wrote on S, with no synchronisation in between."""
    from kmap_amd import _ffi
    from tests import _readscore_model as RM
    from tests._refine_model import asym_matrix
    st, sd, borders = pwm_reads(240)
    W = asym_matrix(9, np.random.default_rng(9))
    lo, hi = RM.score_range(W)
    lo, n_bins = lo + (hi - lo) // 3, (hi - lo) // 3                   # a range that leaves reads outside
    n, n_seq = len(st), len(borders)
    codes, inval, _ = packed_pair(st, sd)

    def issue(p, S, S2):
        n_scored, outside = i64(), i64()
        hist = np.full(n_bins, 0xEEEE, np.uint64)
        chk(L.kmap_readscore_packed_dev(p["codes"], p["inval"], n, p["borders"], n_seq, 9, host(W), 1, p["score"], p["loc"], p["strand"],
                                        C.byref(n_scored), S))
        chk(L.kmap_readscore_hist_dev(p["score"], p["loc"], n_seq, lo, n_bins, _ffi.ptr(hist), C.byref(outside), S))
        return {"hist": hist, "n": np.array([n_scored.value, outside.value], np.int64)}

    def model(w):
        score, loc, strand = RM.np_read_scores((st, sd)[w], borders, W, True)
        hist, outside = RM.np_histogram(score, loc, lo, n_bins)
        return {"score": score, "loc": loc, "strand": strand, "hist": hist, "n": np.array([(loc >= 0).sum(), outside], np.int64)}
    got = drive("readscore + hist", {"codes": codes, "inval": inval, "borders": (borders, borders)},
                {"score": (np.int32, (n_seq,)), "loc": (np.int32, (n_seq,)), "strand": (np.uint8, (n_seq,))}, issue, model=model)
    assert 0 < got["n"][1] < got["n"][0] < n_seq


# ---- the batched library entries ----------------------------------------------------------------------------------------------------
LIB_WIDTHS = (4, 5, 6, 7, 4, 5, 6, 7, 31, 31, 31, 31)


def library(seed=16):
    """twelve matrices: eight narrow ones close a batch by the matrix limit, three of the four 31-column ones by the chunk limit
    (nine matrices cannot do both: eight fill a batch, the ninth alone ends the list)"""
    from kmap_amd.device_seq import _pack_library
    from tests._batch_model import batches
    from tests._refine_model import asym_matrix
    rng = np.random.default_rng(seed)
    Ws = [asym_matrix(w, rng) for w in LIB_WIDTHS]
    assert [why for _, why in batches(LIB_WIDTHS)] == ["matrices", "chunks", "end"]
    return (Ws,) + _pack_library("library", Ws)


def lib_thresholds(seq, borders, Ws):
    """per matrix the median best score of the truth's scorable reads: about half of them are site reads"""
    from tests import _readscore_model as RM
    out = []
    for W in Ws:
        score, loc, _ = RM.np_read_scores(seq, borders, W, True)
        best = score[loc >= 0]
        out.append(int(np.median(best)) if len(best) else 0)
    return np.array(out, np.int32)


def lib_issue(L, name, n, n_seq, *rest):
    """issue(p, S, S2) of one batched entry: blocking per batch, host outputs complete on return"""
    from kmap_amd import _ffi
    n_mat, widths, weights, thr = rest[:4]

    def issue(p, S, S2):
        head = (p["codes"], p["inval"], n, p["borders"], n_seq)
        mats = (n_mat, host(widths), host(weights))
        if name == "readscore":
            lo, nb = rest[4], rest[5]
            hist, outside, scored = np.full(int(nb.sum()), 0xEEEE, np.uint64), np.full(n_mat, -1, np.int64), np.full(n_mat, -1, np.int64)
            chk(L.kmap_readscore_library_dev(*head, *mats, host(lo), host(nb), 1, _ffi.ptr(hist), _ffi.ptr(outside), _ffi.ptr(scored), S))
            return {"hist": hist, "n": np.concatenate([outside, scored])}
        if name == "sites":
            max_len = rest[4]
            D, H = np.full((n_mat, 2 * max_len + 1), 0xEEEE, np.uint64), np.full((n_mat, max_len + 1), 0xEEEE, np.uint64)
            sites, too_long = np.full(n_mat, -1, np.int64), np.full(n_mat, -1, np.int64)
            chk(L.kmap_readscore_sites_library_dev(*head, *mats, host(thr), 1, max_len, _ffi.ptr(D), _ffi.ptr(H), _ffi.ptr(sites),
                                                   _ffi.ptr(too_long), S))
            return {"pos_hist": D, "len_hist": H, "n": np.concatenate([sites, too_long])}
        if name == "counts":
            counts, sel, minus = np.full((n_mat, 4, 32), 0xEEEE, np.uint64), np.full(n_mat, -1, np.int64), np.full(n_mat, -1, np.int64)
            chk(L.kmap_readscore_counts_library_dev(*head, *mats, host(thr), 1, _ffi.ptr(counts), _ffi.ptr(sel), _ffi.ptr(minus), S))
            return {"counts": counts, "n": np.concatenate([sel, minus])}
        if name == "spacing":
            wP, tP, G = rest[4:7]
            gap, room = np.full((n_mat, 4, G + 1), 0xEEEE, np.uint64), np.full((n_mat, G + 2, G + 2), 0xEEEE, np.uint64)
            n_primary, pair, far = i64(), np.full(n_mat, -1, np.int64), np.full(n_mat, -1, np.int64)
            chk(L.kmap_readscore_spacing_library_dev(*head, p["score"], p["loc"], p["strand"], wP, tP, *mats, host(thr), 1, G,
                                                     _ffi.ptr(gap), _ffi.ptr(room), C.byref(n_primary), _ffi.ptr(pair), _ffi.ptr(far), S))
            return {"gap": gap, "room": room, "n": np.concatenate([[n_primary.value], pair, far])}
        n_words = (n_seq + 63) // 64
        present = np.full(n_mat, -1, np.int64)
        chk(L.kmap_presence_library_dev(*head, *mats, host(thr), 1, p["planes"], n_words, _ffi.ptr(present), S))
        return {"present": present}
    return issue


def lib_case(L, seed):
    st, sd, borders = pwm_reads(seed)
    Ws, n_mat, widths, weights, _ = library()
    thr = lib_thresholds(st, borders, Ws)
    codes, inval, _ = packed_pair(st, sd)
    ins = {"codes": codes, "inval": inval, "borders": (borders, borders)}
    return st, sd, borders, Ws, (n_mat, widths, weights, thr), ins


@covers("kmap_readscore_library_dev")
def test_readscore_library(L):
    """Expected values: tests/_readscore_model.py per matrix.  Documented as blocking per batch: the host outputs must be the
    truth's although the truth only arrives behind the delay."""
    from tests import _readscore_model as RM
    st, sd, borders, Ws, mats, ins = lib_case(L, 250)
    rng = [RM.score_range(W) for W in Ws]
    lo = np.array([a + (b - a) // 3 for a, b in rng], np.int32)
    nb = np.array([(b - a) // 3 for a, b in rng], np.int64)

    def model(w):
        hists, outside, scored = [], [], []
        for W, lo_, nb_ in zip(Ws, lo, nb):
            score, loc, _ = RM.np_read_scores((st, sd)[w], borders, W, True)
            h, o = RM.np_histogram(score, loc, int(lo_), int(nb_))
            hists.append(h), outside.append(o), scored.append(int((loc >= 0).sum()))
        return {"hist": np.concatenate(hists), "n": np.array(outside + scored, np.int64)}
    drive("readscore_library", ins, {}, lib_issue(L, "readscore", len(st), len(borders), *mats, lo, nb), model=model)


@covers("kmap_readscore_sites_library_dev", "kmap_readscore_counts_library_dev")
@pytest.mark.parametrize("name", ["sites", "counts"])
def test_sites_and_counts_library(L, name):
    """Expected values: the same entry on the null stream with full synchronisation (tests/test_gpu_sites.py and
    tests/test_gpu_discover.py hold it to tests/_sites_model.py and _refine_model.py).  Blocking per batch."""
    st, sd, borders, Ws, mats, ins = lib_case(L, 260)
    rest = (int((borders[:, 1] - borders[:, 0]).max()) - 5,) if name == "sites" else ()
    got = drive(f"{name}_library", ins, {}, lib_issue(L, name, len(st), len(borders), *mats, *rest))
    assert got["n"][:mats[0]].min() > 0                                # every matrix has site reads
    assert name != "sites" or got["n"][mats[0]:].max() > 0             # ... and some read is longer than max_len


@covers("kmap_readscore_spacing_library_dev")
def test_spacing_library(L):
    """Expected values: the same entry on the null stream with full synchronisation (tests/test_gpu_spacing.py holds it to
    tests/_spacing_model.py).  The primary matrix's three arrays are device inputs with their own decoy: tests/_readscore_model.py's
    arrays of the decoy reads."""
    from tests import _readscore_model as RM
    from tests._refine_model import asym_matrix
    st, sd, borders, Ws, mats, ins = lib_case(L, 270)
    WP = asym_matrix(8, np.random.default_rng(27))
    prim = [RM.np_read_scores(s, borders, WP, True) for s in (st, sd)]
    tP = int(np.median(prim[0][0][prim[0][1] >= 0]))
    for i, key in enumerate(("score", "loc", "strand")):
        ins[key] = (prim[0][i], prim[1][i])
    thr = (mats[3] - 300).astype(np.int32)                             # secondary sites away from the best window need lower bars
    got = drive("spacing_library", ins, {}, lib_issue(L, "spacing", len(st), len(borders), *mats[:3], thr, 8, tP, 40))
    n_mat = mats[0]
    assert got["n"][0] > 10 and got["n"][1:1 + n_mat].max() > 0


@covers("kmap_presence_library_dev", "kmap_bitrows_pair_counts_dev")
def test_presence_library_and_pair_counts(L):
    """Expected values: tests/_cooccurrence_model.np_presence, np_pack and np_pair_counts.  The pair counts read the planes the
    first entry wrote on S."""
    from kmap_amd import _ffi
    from tests import _cooccurrence_model as CM
    st, sd, borders, Ws, mats, ins = lib_case(L, 280)
    n_mat, n_seq = mats[0], len(borders)
    n_words = (n_seq + 63) // 64
    presence = lib_issue(L, "presence", len(st), n_seq, *mats)

    def issue(p, S, S2):
        out = presence(p, S, S2)
        pairs = np.full((n_mat, n_mat), 0xEEEE, np.uint64)
        chk(L.kmap_bitrows_pair_counts_dev(p["planes"], n_mat, n_words, _ffi.ptr(pairs), S))
        out["pairs"] = pairs
        return out

    def model(w):
        bits = CM.np_presence((st, sd)[w], borders, Ws, [int(t) for t in mats[3]], True)
        return {"planes": CM.np_pack(bits), "present": bits.sum(axis=1).astype(np.int64), "pairs": np.asarray(CM.np_pair_counts(bits)).astype(np.uint64)}
    drive("presence_library + pair_counts", ins, {"planes": (np.uint64, (n_mat, n_words))}, issue, model=model)


# ---- count matrices against a library -----------------------------------------------------------------------------------------------
@covers("kmap_match_hist_dev", "kmap_match_tables_dev", "kmap_match_pairs_dev")
def test_match_chain(L):
    """hist -> tables -> pairs chained on S (each packs host arrays first, one synchronisation of S per call).  Expected values:
    the same chain on the null stream with full synchronisation (integer histograms, gathers in a fixed order and exact double
    comparisons: the same bits in every run); the truth's histograms also against tests/test_gpu_match.Motifs.  The decoy's
    columns are the truth's rolled by five columns: valid motif columns, other motifs."""
    from tests.test_gpu_footprint import match_case
    m = match_case()
    q, l_ = np.asarray(m["qcols"]), np.asarray(m["lcols"])
    n_q, n_l, n_query, n_target, n_table = len(q), len(l_), len(m["q_width"]), len(m["t_width"]), m["n_table"]
    assert q.shape == (n_q, 4) and l_.shape == (n_l, 4) and q.dtype == np.uint16
    ins = {"qcols": (q, np.roll(q, 5, axis=0)), "lcols": (l_, np.roll(l_, 5, axis=0))}

    def issue(p, S, S2):
        chk(L.kmap_match_hist_dev(p["qcols"], n_q, p["lcols"], n_l, 1, p["hist"], S))
        chk(L.kmap_match_tables_dev(p["hist"], n_q, m["n_null"], n_query, host(m["q_width"]), host(m["q_col0"]), host(m["q_min_len"]),
                                    host(m["q_toff"]), p["tables"], n_table, S))
        chk(L.kmap_match_pairs_dev(p["qcols"], n_q, n_query, host(m["q_width"]), host(m["q_col0"]), host(m["q_min_len"]),
                                   host(m["q_toff"]), p["tables"], n_table, p["lcols"], n_l, n_target, host(m["t_width"]),
                                   host(m["t_col0"]), m["min_overlap"], 1, p["p"], p["cfg"], S))
    got = drive("match chain", ins, {"hist": (np.uint32, (n_q, 91)), "tables": (np.float64, (n_table,)),
                                     "p": (np.float64, (n_query, n_target)), "cfg": (np.int32, (n_query, n_target, 4))}, issue)
    np.testing.assert_array_equal(got["hist"], m["H"])


# ---- enrichment ---------------------------------------------------------------------------------------------------------------------
@covers("kmap_enrich_set_control", "kmap_enrich_run", "kmap_enrich_select")
def test_enrich(L):
    """set_control, run, select and fetch on S over two tables loaded with kmap_counts_load beforehand: 1000 foreground and 999 control
    keys at k = 12.  The handles hold the DECOY tables when the streams are drained; the truth reaches the tables' device arrays
    (kmap_counts_table_dev) on S.  Expected values: the same entries on the null stream with full synchronisation
    (tests/test_gpu_enrich.py holds them to its model).  Both decoys are valid tables: keys ascending and unique, the truth's
    counts in another order (the same totals)."""
    from kmap_amd import _ffi
    k, n_fg, n_bg = 12, 1000, 999
    rng = np.random.default_rng(300)

    def table(n):
        keys = np.sort(rng.choice(4 ** k, size=n, replace=False)).astype(np.uint32)
        return keys, rng.integers(1, 200, n).astype(np.int32)
    fg, bg = table(n_fg), table(n_bg)
    common = rng.choice(n_bg, 400, replace=False)                       # shared keys, so that b is not 0 everywhere
    fg_u = np.unique(np.concatenate([fg[0][:600], bg[0][common]]))[:n_fg]
    fg_u = np.sort(np.concatenate([fg_u, np.setdiff1d(fg[0], fg_u)[:n_fg - len(fg_u)]])).astype(np.uint32)
    assert len(fg_u) == n_fg and len(np.unique(fg_u)) == n_fg
    fg_d, bg_d = table(n_fg), table(n_bg)
    tabs = {"fg_u": (fg_u, fg_d[0]), "fg_c": (fg[1].view(np.uint32), rng.permutation(fg[1]).view(np.uint32)),
            "bg_u": (bg[0], bg_d[0]), "bg_c": (bg[1].view(np.uint32), rng.permutation(bg[1]).view(np.uint32))}
    Nf, Nb = int(fg[1].sum()), int(bg[1].sum())

    def setup(p):
        hs = [C.c_void_p() for _ in range(3)]
        chk(L.kmap_counts_create(C.byref(hs[0])))
        chk(L.kmap_counts_create(C.byref(hs[1])))
        chk(L.kmap_enrich_create(C.byref(hs[2])))
        dev = []
        for h, u, c in ((hs[0], "fg_u", "fg_c"), (hs[1], "bg_u", "bg_c")):
            chk(L.kmap_counts_load(h, host(tabs[u][1]), host(tabs[c][1].view(np.int32)), len(tabs[u][1]), k))
            pu, pc, n = C.c_void_p(), C.c_void_p(), i64()
            chk(L.kmap_counts_table_dev(h, C.byref(pu), C.byref(pc), C.byref(n)))
            dev += [(pu.value, u), (pc.value, c)]
        return hs, dev

    def teardown(ctx):
        hs, _ = ctx
        chk(L.kmap_enrich_destroy(hs[2]))
        chk(L.kmap_counts_destroy(hs[0]))
        chk(L.kmap_counts_destroy(hs[1]))

    def issue(p, S, S2, ctx):
        (fgh, bgh, e), dev = ctx
        for ptr_, name in dev:
            chk(L.kmap_memcpy_d2d(ptr_, p[name], tabs[name][0].nbytes, S))
        chk(L.kmap_enrich_set_control(e, bgh, 1, S))
        chk(L.kmap_enrich_run(e, fgh, Nf, Nb, 2, S))
        n_sel, n_el = i64(), i64()
        chk(L.kmap_enrich_select(e, 50, C.byref(n_sel), C.byref(n_el), S))
        m = n_sel.value
        idx, kh, a, b, z = np.empty(m, np.int64), np.empty(m, np.uint64), np.empty(m, np.int64), np.empty(m, np.int64), np.empty(m, np.float64)
        chk(L.kmap_enrich_fetch(e, _ffi.ptr(idx), _ffi.ptr(kh), _ffi.ptr(a), _ffi.ptr(b), _ffi.ptr(z)))
        pb, pz, n_all = C.c_void_p(), C.c_void_p(), i64()
        chk(L.kmap_enrich_result_dev(e, C.byref(pb), C.byref(pz), C.byref(n_all)))
        b_all, z_all = np.full(n_all.value, 0xEEEE, np.uint64), np.full(n_all.value, np.nan)
        chk(L.kmap_memcpy_d2h(_ffi.ptr(b_all), pb, b_all.nbytes, S))
        chk(L.kmap_memcpy_d2h(_ffi.ptr(z_all), pz, z_all.nbytes, S))
        # the most enriched keys are those the control lacks: the selected b may be 0 in truth and decoy alike, so a and b are one array
        # ... and the two counts ride behind the indices (the decoy's counts are the truth's in another order: as many are eligible)
        return {"idx": np.concatenate([idx, [m, n_el.value]]), "kh": kh, "ab": np.stack([a, b]), "z": z, "b_all": b_all, "z_all": z_all}
    got = drive("enrich", tabs, {}, issue, setup=setup, teardown=teardown)
    assert got["idx"][-2] == 50 and (got["b_all"] > 0).sum() > 100 and len(got["b_all"]) == n_fg


# ---- labels -------------------------------------------------------------------------------------------------------------------------
@covers("kmap_label_kmers_dev", "kmap_label_prefix_dev")
def test_labels(L):
    """kmap_label_kmers_dev and two kmap_label_prefix_dev (weights, members) on S; after kmap_stream_sync(S) the stream-less
    kmap_label_sums_dev, kmap_prefix_search_dev, kmap_label_members_dev and kmap_gather_dev, as their rule in include/kmap_hip.h
    demands.  n = 3000 keys, three consensuses.  Expected values: the same entries on the null stream with full synchronisation
    (tests/test_gpu_table_queries.py holds them to tests/_table_model.py)."""
    from kmap_amd import _ffi
    k, n = 12, 3000
    rng = np.random.default_rng(310)
    cons = rng.integers(0, 4 ** k, 3, dtype=np.uint64)
    lens, rads = np.array([12, 9, 7], np.int32), np.array([3, 2, 1], np.int32)
    cons_kh = np.array([int(c) >> (2 * (k - int(ln))) for c, ln in zip(cons, lens)], np.uint64)

    def keys():
        near = np.repeat(cons, 500)                                    # two substitutions per key: inside the first consensus' radius
        for _ in range(2):
            near = near ^ (rng.integers(1, 4, 1500).astype(np.uint64) << (2 * rng.integers(0, k, 1500)).astype(np.uint64))
        u = np.unique(np.concatenate([near, rng.integers(0, 4 ** k, 4000, dtype=np.uint64)]))
        return np.sort(rng.choice(u, n, replace=False)).astype(np.uint32)
    uniq = (keys(), keys())
    cnt = (rng.integers(1, 1000, n).astype(np.int32), rng.integers(1, 1000, n).astype(np.int32))

    def issue(p, S, S2):
        chk(L.kmap_label_kmers_dev(p["uniq"], n, k, 3, host(cons_kh), host(lens), host(rads), 3, 1, p["label"], S))
        chk(L.kmap_label_prefix_dev(p["label"], p["cnt"], 0, n, 0, p["scratch"], p["excl"], S))
        chk(L.kmap_label_prefix_dev(p["label"], None, 0, n, 0, p["scratch"], p["excl1"], S))
        sync(S)
        wsum, members = np.full(4, -1, np.int64), np.full(4, -1, np.int64)
        chk(L.kmap_label_sums_dev(p["label"], p["cnt"], 0, n, 4, _ffi.ptr(wsum), _ffi.ptr(members)))
        targets = np.ascontiguousarray(np.arange(50, dtype=np.int64) * max(int(wsum[0]), 1) // 50)
        hit = np.full(50, -1, np.int64)
        if wsum[0] > 0:
            chk(L.kmap_prefix_search_dev(p["excl"], n, _ffi.ptr(targets), 50, _ffi.ptr(hit)))
        m = int(members[0])
        mem = np.full(m, -1, np.int64)
        chk(L.kmap_label_members_dev(p["label"], p["excl1"], n, 0, m, _ffi.ptr(mem)))
        picked = np.full(m, 0xEEEEEEEE, np.uint32)
        chk(L.kmap_gather_dev(p["uniq"], 4, _ffi.ptr(mem), m, _ffi.ptr(picked)))
        return {"sums": np.concatenate([wsum, members]), "hit": hit, "members": mem, "picked": picked}
    got = drive("labels", {"uniq": uniq, "cnt": cnt},
                {"label": (np.uint8, (n,)), "scratch": (np.uint32, (n,)), "excl": (np.uint64, (n + 1,)), "excl1": (np.uint64, (n + 1,))},
                issue, inout=("uniq",), skip=("scratch",))
    assert got["sums"][4] > 50 and got["sums"][5] > 0 and got["sums"][6] > 0           # every consensus has members
    lab = got["label"]
    np.testing.assert_array_equal(got["members"], np.flatnonzero(lab == 0))
    np.testing.assert_array_equal(got["excl1"], np.concatenate([[0], np.cumsum(lab == 0)]).astype(np.uint64))
    np.testing.assert_array_equal(got["excl"], np.concatenate([[0], np.cumsum(np.where(lab == 0, cnt[0], 0))]).astype(np.uint64))
    np.testing.assert_array_equal(got["picked"], got["uniq"][got["members"]])


# ---- generators ---------------------------------------------------------------------------------------------------------------------
@covers("kmap_synth_reads_dev")
def test_synth_reads(L):
    """The generator has no device input, so nothing can hold a decoy.  Instead both outputs are overwritten on S just before the
    entry: they are registered as in-place inputs whose 'truth' is a fill of 0x33 bytes.  A launch that escaped to the null
    stream writes while S sits in the delay, and the fill then wipes its work: the decoy's expected result is the fill.  Expected
    values of the truth: the same entry on the null stream with full synchronisation."""
    n_reads, read_len = 300, 40
    n_bytes = n_reads * (read_len + 1)
    motif = np.array([0, 2, 2, 0, 1], np.uint8)
    wiped = {"seq": np.full(n_bytes, 0x33, np.uint8), "borders": np.full((n_reads, 2), 0x3333333333333333, np.int64)}
    ins = {k: (v, np.full_like(v, 0x44)) for k, v in wiped.items()}

    def issue(p, S, S2):
        chk(L.kmap_synth_reads_dev(p["seq"], p["borders"], n_reads, read_len, 7, host(motif), host(np.array([5], np.int32)),
                                   host(np.array([0.5])), 1, 0.05, S))
    got = drive("synth_reads", ins, {}, issue, inout=("seq", "borders"), model=lambda w: wiped if w else {})
    assert np.all(got["seq"].reshape(n_reads, read_len + 1)[:, read_len] == 255) and got["seq"].reshape(n_reads, -1)[:, :read_len].max() <= 3
    np.testing.assert_array_equal(got["borders"], np.arange(n_reads, dtype=np.int64)[:, None] * (read_len + 1) + np.array([0, read_len]))


@covers("kmap_shuffle_packed_dev")
@pytest.mark.parametrize("klet", [1, 2])
def test_shuffle(L, klet):
    """Expected values: tests/_shuffle_model.shuffle_array.  The call blocks until the segment list is built; the kernels that
    write the output are asynchronous on S."""
    from tests._shuffle_model import shuffle_array
    st, sd, _ = read_pair(320 + klet)
    n = len(st)
    codes, inval, _ = packed_pair(st, sd)

    def issue(p, S, S2):
        stats = (C.c_int64 * 2)(-1, -1)
        chk(L.kmap_shuffle_packed_dev(p["codes"], p["inval"], n, klet, 77, p["out"], stats, S))
        return {"stats": np.array([stats[0], stats[1]], np.int64)}
    got = drive(f"shuffle klet={klet}", {"codes": codes, "inval": inval}, {"out": (np.uint8, (n,))}, issue,
                model=lambda w: {"out": shuffle_array((st, sd)[w], klet, 77)})
    assert got["stats"][1] == (st != 255).sum() and (got["out"] != st).any()


# ---- the matrix stage ---------------------------------------------------------------------------------------------------------------
@covers("kmap_hamdist_matrix_u32_dev", "kmap_hamdist_matrix_u64_dev")
@pytest.mark.parametrize("k,n", [(8, 300), (8, 4100), (16, 4100)], ids=["general", "tile_u32", "tile_u64"])
def test_hamdist_matrix(L, O, k, n):
    """Expected values: oracle.hamdist_matrix_u8 on the n payload columns; the whole pitched buffer (pad columns included) against
    the same entry on the null stream.  n = 300: the general kernel; n = 4100 at the pitch of kmap_hamdist_pitch: the tile kernel
    with its packed tail, one label with a short consensus."""
    if n == 300:
        drive("hamdist_matrix general", **_matrix_case(L, O, n, k))
        return
    kh = hashes_pair(k, n, 330 + k)
    rng = np.random.default_rng(331)
    lab = [rng.integers(0, 2, n).astype(np.int32) for _ in range(2)]
    clen = np.array([k, k - 3], np.int32)
    ld = int(L.kmap_hamdist_pitch(n))
    fn = L.kmap_hamdist_matrix_u32_dev if k < 16 else L.kmap_hamdist_matrix_u64_dev
    got = drive(f"hamdist_matrix k={k} n={n}", {"kh": (kh[0], kh[1]), "label": (lab[0], lab[1])}, {"D": (np.uint8, (n, ld))},
                lambda p, S, S2: chk(fn(p["kh"], p["label"], n, k, host(clen), 2, 0, n, p["D"], ld, S)))
    np.testing.assert_array_equal(got["D"][:, :n], O.hamdist_matrix_u8(kh[0], lab[0], k, clen))


@covers("kmap_knn_select_u8_dev", "kmap_knn_sums_u8_dev", "kmap_knn_sums_kmers_u32_dev", "kmap_knn_sums_kmers_u64_dev")
@pytest.mark.parametrize("k", [8, 16])
def test_knn_chain(L, O, k):
    """matrix -> selection -> sums from the matrix -> sums from the k-mers, chained on S: n = 257, 20 neighbours.  Expected values:
    the same chain on the null stream; the truth's selection also against oracle.knn_select_stable and its sums against the
    neighbour sums of the oracle's matrix (both sums entries: they are documented as identical)."""
    n, n_nb = 257, 20
    kh = hashes_pair(k, n, 340 + k)
    lab = (np.zeros(n, np.int32), np.zeros(n, np.int32))
    clen = np.array([k], np.int32)
    ldd, lds = 272, 384
    mat = L.kmap_hamdist_matrix_u32_dev if k < 16 else L.kmap_hamdist_matrix_u64_dev
    sums_k = L.kmap_knn_sums_kmers_u32_dev if k < 16 else L.kmap_knn_sums_kmers_u64_dev

    def issue(p, S, S2):
        chk(mat(p["kh"], p["label"], n, k, host(clen), 1, 0, n, p["D"], ldd, S))
        chk(L.kmap_knn_select_u8_dev(p["D"], ldd, n, n_nb, 0, n, p["nb"], S))
        chk(L.kmap_knn_sums_u8_dev(p["D"], ldd, p["nb"], n, n_nb, 0, n, p["sums"], lds, S))
        chk(sums_k(p["kh"], p["label"], n, k, host(clen), 1, p["nb"], n_nb, 0, n, p["sums_k"], lds, S))
    # nb is an index array that later steps of the chain follow: it starts out holding valid indices, not the sentinel, so that
    # even a step that ran too early would stay in bounds
    nb0 = np.tile(np.arange(n_nb, dtype=np.int32), (n, 1))
    got = drive(f"knn chain k={k}", {"kh": (kh[0], kh[1]), "label": lab, "nb": (nb0, nb0[:, ::-1].copy())},
                {"D": (np.uint8, (n, ldd)), "sums": (np.uint16, (n, lds)), "sums_k": (np.uint16, (n, lds))}, issue, inout=("nb",))
    D = O.hamdist_matrix_u8(kh[0], lab[0], k, clen).astype(np.int64)
    nb = O.knn_select_stable(D, n_nb)
    np.testing.assert_array_equal(np.sort(got["nb"], axis=1), np.sort(nb, axis=1))   # the rule fixes the set, not its order
    A = np.zeros((n, n), np.int64)
    A[np.arange(n)[:, None], nb] = 1
    want = A @ D @ A.T
    np.fill_diagonal(want, 0)
    np.testing.assert_array_equal(got["sums"][:, :n], want)
    np.testing.assert_array_equal(got["sums_k"][:, :n], want)


@covers("kmap_rows_fresh_u8_dev", "kmap_gather_rows_u8_dev")
def test_rows_fresh_and_gather(L):
    """Expected values: numpy (row r differs from the row above; out row o = row idx[o]).  The decoy's indices are in range."""
    n, nrows, ldd, ldo, n_idx = 200, 150, 208, 224, 60
    rng = np.random.default_rng(350)

    def matrix():
        rows = rng.integers(0, 9, size=(nrows // 3, ldd)).astype(np.uint8)
        return np.ascontiguousarray(rows[np.sort(rng.integers(0, nrows // 3, nrows))])
    D = (matrix(), matrix())
    idx = tuple(rng.integers(0, nrows, n_idx).astype(np.int32) for _ in range(2))

    def issue(p, S, S2):
        chk(L.kmap_rows_fresh_u8_dev(p["D"], ldd, n, 0, nrows, p["fresh"], S))
        chk(L.kmap_gather_rows_u8_dev(p["D"], ldd, n, p["idx"], n_idx, p["out"], ldo, S))

    def model(w):
        fresh = np.concatenate([[1], (D[w][1:, :n] != D[w][:-1, :n]).any(axis=1)]).astype(np.uint8)
        out = np.full((n_idx, ldo), SO.SENTINEL, np.uint8)
        out[:, :n] = D[w][idx[w]][:, :n]
        return {"fresh": fresh, "out": out}
    got = drive("rows_fresh + gather_rows", {"D": D, "idx": idx}, {"fresh": (np.uint8, (nrows,)), "out": (np.uint8, (n_idx, ldo))},
                issue, model=model)
    assert 0 < got["fresh"].sum() < nrows


# ---- projection ---------------------------------------------------------------------------------------------------------------------
@covers("kmap_project_knn_u32_dev", "kmap_project_knn_u64_dev", "kmap_project_prob_dev", "kmap_project_descend_dev")
@pytest.mark.parametrize("tag", ["k8n300", "k16n300"])
def test_projection_chain(L, tag):
    """selection -> probabilities -> descent chained on S: 50 queries on 300 references.  Expected values: the same chain on the
    null stream with full synchronisation, after two such evaluations agreed bit for bit; the truth's selection also against
    tests/test_gpu_project.case.  The decoys are valid inputs: other queries and references, the sums' rows, the table and the
    coordinates in another order."""
    from kmap_amd.projection import hd_prob_lut_projected
    from tests import test_gpu_project as P
    c = P.case(tag)
    m, n, k, n_nb = 50, c["n"], c["k"], P.N_NB
    rng = np.random.default_rng(360)
    lut = np.ascontiguousarray(hd_prob_lut_projected(k, n_nb), np.float32)
    lds = ldp = n + 4
    sums = np.zeros((n, lds), np.uint16)
    sums[:, :n] = c["Sref"]
    q, ref, xy = c["q"][:m], c["ref"], c["xy"].astype(np.float32)
    ins = {"q": (q, rng.permutation(c["q"])[:m]), "ref": (ref, ref[::-1].copy()), "sums": (sums, sums[::-1].copy()),
           "lut": (lut, lut[::-1].copy()), "ref_xy": (xy, np.ascontiguousarray(-xy[:, ::-1]))}
    fn = L.kmap_project_knn_u32_dev if q.dtype == np.uint32 else L.kmap_project_knn_u64_dev

    def issue(p, S, S2):
        chk(fn(p["q"], m, p["ref"], n, k, 1, n_nb, p["nb"], p["dist"], p["flipped"], S))
        chk(L.kmap_project_prob_dev(p["nb"], m, n_nb, p["sums"], lds, None, n, n, p["lut"], len(lut), 0, m, p["p"], ldp, p["qsum"], S))
        chk(L.kmap_project_descend_dev(p["p"], ldp, p["nb"], m, n_nb, p["ref_xy"], n, 0, m, 5, P.LR, p["xy"], S))
    # nb is an index array that the next two steps follow: it starts out holding valid indices, not the sentinel
    nb0 = np.tile(np.arange(n_nb, dtype=np.int32), (m, 1))
    ins["nb"] = (nb0, nb0[:, ::-1].copy())
    got = drive(f"projection {tag}", ins,
                {"dist": (np.uint8, (m, n_nb)), "flipped": (np.uint8, (m,)), "p": (np.float32, (m, ldp)),
                 "qsum": (np.uint32, (m, ldp)), "xy": (np.float32, (2, m))}, issue, inout=("q", "nb"), twice=True)
    np.testing.assert_array_equal(got["nb"], c["nb"][:m])
    np.testing.assert_array_equal(got["q"], c["kh"][:m])
    assert np.isfinite(got["xy"]).all()


# ---- embedding ----------------------------------------------------------------------------------------------------------------------
def embed_case(L, mode, variant):
    """n = 300 points, sums and table as tests/test_gpu_embed.py draws them.  The decoy is a different start-coordinate array: the
    session is given it with kmap_embed_set_coords before the streams are drained, and the truth reaches the session's device
    coordinates (kmap_embed_coords_dev) on S.  The sums are the same in both (kmap_embed_set_prob_lut may read them when called)."""
    from kmap_amd import _ffi
    from kmap_amd import visualization as V
    n, n_best = 300, 3
    lds = (n + 127) & ~127
    rng = np.random.default_rng(370)
    sums = rng.integers(0, 3201, size=(n, lds), dtype=np.uint16)
    sums[:, :n] = np.triu(sums[:, :n], 1) + np.triu(sums[:, :n], 1).T
    lut = np.ascontiguousarray(V.hd_prob_lut(8, 20, 3200), np.float32)
    coords = ((rng.standard_normal((2, n)) * 3).astype(np.float32), (rng.standard_normal((2, n)) * 3).astype(np.float32))
    normals = np.ascontiguousarray(rng.normal(0, 0.01, 64))
    placeholders = np.zeros((n_best, 2, n), np.float32)
    n_iter = 10 if variant == "step" else 4                            # more than n_best: the best list holds no placeholder at the end
    n_msg = int(L.kmap_embed_msg_floats(n))
    ins = {"sums": (sums, sums), "coords": coords}
    inout = ()
    if variant == "forces":
        ins.update(grad=(np.zeros((2, n), np.float32), rng.standard_normal((2, n)).astype(np.float32)),
                   loss=(np.zeros(1, np.float64), np.array([123.0])))
        inout = ("grad", "loss")
    elif variant == "msg":
        noise = np.zeros(n_msg, np.float32)
        noise[:2 * n] = rng.standard_normal(2 * n)                    # the decoy's limbs and flag stay zero: a legal message
        ins.update(msg=(np.zeros(n_msg, np.float32), noise))
        inout = ("msg",)

    def setup(p):
        e = C.c_void_p()
        chk(L.kmap_embed_create(C.byref(e), n, 0, n, n_best, 0.01, mode))
        chk(L.kmap_embed_set_prob_lut(e, p["sums"], lds, host(lut), len(lut)))
        chk(L.kmap_embed_set_coords(e, host(coords[1]), host(placeholders)))
        chk(L.kmap_embed_set_jitter(e, host(normals), len(normals)))
        return e

    def teardown(e):
        chk(L.kmap_embed_destroy(e))

    def issue(p, S, S2, e):
        chk(L.kmap_memcpy_d2d(L.kmap_embed_coords_dev(e), p["coords"], 2 * n * 4, S))
        if variant == "step":
            chk(L.kmap_embed_step(e, n_iter, S))
        elif variant == "forces":
            for it in range(n_iter):
                if it:
                    chk(L.kmap_memset(p["grad"], 0, 2 * n * 4, S))
                    chk(L.kmap_memset(p["loss"], 0, 8, S))
                chk(L.kmap_embed_forces(e, p["grad"], p["loss"], S))
                chk(L.kmap_embed_apply(e, p["grad"], p["loss"], S))
        else:
            for _ in range(n_iter):
                chk(L.kmap_embed_forces_msg(e, p["msg"], S))
                chk(L.kmap_embed_apply_msg(e, p["msg"], S))
        iters, stopped, last, best, used = i64(), C.c_int(-1), C.c_float(-1), C.c_float(-1), C.c_int(-1)
        chk(L.kmap_embed_state(e, C.byref(iters), C.byref(stopped), C.byref(last), C.byref(best), C.byref(used), S))
        xy, xy_best = np.full((2, n), np.nan, np.float32), np.full((2, n), np.nan, np.float32)
        chk(L.kmap_embed_get_coords(e, _ffi.ptr(xy), S))
        chk(L.kmap_embed_get_best(e, _ffi.ptr(xy_best), S))
        snaps, snap_losses = np.full((n_best, 2, n), np.nan, np.float32), np.full(n_best, np.nan, np.float32)
        chk(L.kmap_embed_get_best_list(e, _ffi.ptr(snaps), _ffi.ptr(snap_losses), S))
        losses, n_loss = np.full(16, np.nan, np.float32), i64()
        chk(L.kmap_embed_get_losses(e, _ffi.ptr(losses), 16, C.byref(n_loss), S))
        return {"state": np.array([last.value, best.value], np.float32), "xy": xy, "xy_best": xy_best, "snaps": snaps,
                "snap_losses": snap_losses, "losses": losses[:n_loss.value].copy(),
                "counters": np.array([iters.value, stopped.value, used.value, n_loss.value], np.int64)}
    return dict(ins=ins, outs={}, issue=issue, inout=inout, setup=setup, teardown=teardown, twice=True, skip=("counters", "sums"))


@covers("kmap_embed_step", "kmap_embed_state", "kmap_embed_get_coords", "kmap_embed_get_best", "kmap_embed_get_best_list",
        "kmap_embed_get_losses", "kmap_embed_forces", "kmap_embed_apply", "kmap_embed_forces_msg", "kmap_embed_apply_msg")
@pytest.mark.parametrize("variant", ["step", "forces", "msg"])
@pytest.mark.parametrize("mode", [1, 0], ids=["SEQ", "FAST"])
def test_embed(L, mode, variant):
    """Expected values: the same entries on the null stream with full synchronisation, bit for bit, after two such evaluations
    agreed bit for bit (SEQ is pinned to the reference bit for bit by tests/test_gpu_embed.py; FAST at this size runs the row
    kernel, whose order is fixed).  step: kmap_embed_step(e, 10, S); forces / msg: four iterations as kmap_embed_forces +
    kmap_embed_apply on the caller's gradient and loss buffers, or as kmap_embed_forces_msg + kmap_embed_apply_msg on the caller's
    message buffer, which get the decoy/truth treatment too.  State, coordinates, best list and losses are read with S."""
    spec = embed_case(L, mode, variant)
    got = drive(f"embed mode={mode} {variant}", **spec)
    assert got["counters"][0] == (10 if variant == "step" else 4) and np.isfinite(got["xy"]).all()


# ---- two streams at once ------------------------------------------------------------------------------------------------------------
def dual(specs, threaded):
    """Two cases with different data, the first on one stream behind the delay, the second on another without a delay.  One
    thread: both streams are primed (delay and truth copies), then the entries are issued back to back.  threaded: every case from
    its own Python thread (for entries that block).  Both results must be the truth's."""
    specs = [dict(s, ins=_contig(s["ins"])) for s in specs]
    wants = [expectations(s["name"], s["ins"], s["outs"], s["issue"], s.get("inout", ()), s.get("model")) for s in specs]
    dev = SO.device()
    opened = [open_case(s["name"], s["ins"], s["outs"], s.get("inout", ()), None if i == 0 else 0, stream=2 * i) for i, s in enumerate(specs)]
    gots, errors = [None, None], []
    try:
        def go(i):
            try:
                c, p = opened[i]
                gots[i] = _call(specs[i]["issue"], p, c.S, dev.stream(2 * i + 1), None)
            except BaseException as e:                                  # reported by the main thread
                errors.append(e)
        for c, _ in opened:
            c.begin()
        if threaded:
            threads = [threading.Thread(target=go, args=(i,)) for i in range(2)]
            for t in threads:
                t.start()
            for t in threads:
                t.join()
        else:
            go(0), go(1)
        for c, _ in opened:
            c.end()
        assert not errors, errors
        for i, s in enumerate(specs):
            compare(opened[i][0], collect(opened[i][0], gots[i], s["ins"], s["outs"], s.get("inout", ())), wants[i])
    finally:
        for c, _ in opened:
            c.finish()


def test_two_streams_counting(L, O):
    """k = 19 (the sort path: arena slots C and D of the stream it is given).  Expected values: oracle.count_kmers / _table_model."""
    specs = []
    for i in range(2):
        st, sd, borders = rc_pair(400 + i)
        codes, inval, _ = packed_pair(st, sd)
        tables = [O.count_kmers(s, borders, 19, False, True) for s in (st, sd)]

        def run(h, p, S, S2, n=len(st), n_seq=len(borders)):
            nu = i64()
            chk(L.kmap_counts_run_packed_dev(h, p["codes"], p["inval"], n, p["borders"], n_seq, 19, 1, 1, C.byref(nu), S))
            return table_results(L, O, h, 19, nu.value, S, S2, 1)
        specs.append(dict(name=f"two streams: counts {i}", ins={"codes": codes, "inval": inval, "borders": (borders, borders)}, outs={},
                          issue=counted(L, run), model=lambda w, t=tables: table_model(O, 19, t[w], 1)))
    dual(specs, threaded=False)


def test_two_streams_scan(L, O):
    """the occurrence scan at k = 8.  Expected values: the same entries on the null stream with full synchronisation."""
    specs = []
    for i in range(2):
        st, sd, borders = read_pair(410 + i)
        codes, inval, planes = packed_pair(st, sd)
        cons = _consensus_of(O, st, 8)

        def run(h, p, S, S2, n=len(st), n_seq=len(borders), cons=cons):
            tot = i64()
            chk(L.kmap_scan_run_packed_dev(h, p["codes"], p["inval"], n, p["borders"], n_seq, 8, cons, 2, 1, C.byref(tot), p["planes"], S))
            return scan_results(L, h, n_seq, tot.value, S, S2)
        specs.append(dict(name=f"two streams: scan {i}", ins={"codes": codes, "inval": inval, "planes": planes, "borders": (borders, borders)},
                          outs={}, issue=scanned(L, run)))
    dual(specs, threaded=False)


def test_two_streams_readscore_library(L):
    """kmap_readscore_library_dev blocks, so each case is issued from its own Python thread with its own stream: the weights of the
    two libraries lie in arena slot C of their streams.  Expected values: the same entry on the null stream."""
    specs = []
    for i in range(2):
        st, sd, borders = pwm_reads(420 + i)
        Ws, n_mat, widths, weights, _ = library(seed=16 + i)
        from tests import _readscore_model as RM
        rng = [RM.score_range(W) for W in Ws]
        lo = np.array([a + (b - a) // 3 for a, b in rng], np.int32)
        nb = np.array([(b - a) // 3 for a, b in rng], np.int64)
        codes, inval, _ = packed_pair(st, sd)
        specs.append(dict(name=f"two streams: library {i}", ins={"codes": codes, "inval": inval, "borders": (borders, borders)}, outs={},
                          issue=lib_issue(L, "readscore", len(st), len(borders), n_mat, widths, weights, None, lo, nb)))
    dual(specs, threaded=True)


# ---- the product's background pattern -------------------------------------------------------------------------------------------------
def test_background_fetch_while_counting(L, O):
    """Handle A counted at k = 12 and finished; kmap_counts_fetch_stream(A, S) is enqueued behind the delay from a worker thread
    while the main thread counts other reads into handle B at the same k on the null stream (one per-device table, stamped with a
    generation).  A's arrays must be what they were.  Expected values: oracle.count_kmers."""
    from kmap_amd import _ffi
    k = 12
    dev = SO.device()
    S = dev.stream(0)
    tables, handles, bufs = [], [], []
    for i in range(2):
        st, _, borders = read_pair(430 + i, n_reads=300)
        tables.append(O.count_kmers(st, borders, k, False, True))
        codes, inval, _ = ref_pack(st)
        handles.append(C.c_void_p())
        chk(L.kmap_counts_create(C.byref(handles[i])))
        bufs.append((F.Guarded.of(codes, name="codes"), F.Guarded.of(inval, name="inval"), F.Guarded.of(borders, name="borders"),
                     len(st), len(borders)))

    def count(i):
        c, iv, b, n, n_seq = bufs[i]
        nu = i64()
        chk(L.kmap_counts_run_packed_dev(handles[i], c.ptr, iv.ptr, n, b.ptr, n_seq, k, 1, 1, C.byref(nu), None))
        return nu.value
    try:
        n_a = count(0)
        assert n_a == len(tables[0][0])
        u, c = np.zeros(n_a, np.uint32), np.zeros(n_a, np.int32)
        errors = []

        def worker():
            try:
                dev.delay(SO.DELAY_MS, S)
                chk(L.kmap_counts_fetch_stream(handles[0], _ffi.ptr(u), _ffi.ptr(c), S))
            except BaseException as e:
                errors.append(e)
        sync()
        t = threading.Thread(target=worker)
        t.start()
        n_b = count(1)
        t.join()
        assert not errors, errors
        np.testing.assert_array_equal(u, tables[0][0])
        np.testing.assert_array_equal(c, tables[0][1])
        ub, cb = np.zeros(n_b, np.uint32), np.zeros(n_b, np.int32)
        chk(L.kmap_counts_fetch(handles[1], _ffi.ptr(ub), _ffi.ptr(cb)))
        np.testing.assert_array_equal(ub, tables[1][0])
        np.testing.assert_array_equal(cb, tables[1][1])
        assert not SO.same(u, ub)
    finally:
        for h in handles:
            chk(L.kmap_counts_destroy(h))
        for g in bufs:
            F.guards(*g[:3])
            F.free(*g[:3])


# ---- stream lifetime: after all of the above ----------------------------------------------------------------------------------------------
@covers("kmap_stream_destroy")
def test_streams_end_and_the_arena_survives(L, O):
    """kmap_stream_destroy of every stream of this file, kmap_scratch_release(0), then one null-stream count (k = 19: arena slots
    and DevBufs) gives the oracle's table: the arena survives the loss of its streams."""
    from kmap_amd import _ffi
    dev = SO.device()
    dev.stream(0)
    sync()
    assert dev.destroy_streams() >= 1
    chk(L.kmap_scratch_release(0))
    st, _, borders = rc_pair(440)
    want = O.count_kmers(st, borders, 19, False, True)
    codes, inval, _ = ref_pack(st)
    bufs = [F.Guarded.of(a, name=nm) for a, nm in ((codes, "codes"), (inval, "inval"), (borders, "borders"))]
    h, nu = C.c_void_p(), i64()
    chk(L.kmap_counts_create(C.byref(h)))
    try:
        chk(L.kmap_counts_run_packed_dev(h, bufs[0].ptr, bufs[1].ptr, len(st), bufs[2].ptr, len(borders), 19, 1, 1, C.byref(nu), None))
        u, c = np.zeros(nu.value, np.uint64), np.zeros(nu.value, np.int64)
        chk(L.kmap_counts_fetch(h, _ffi.ptr(u), _ffi.ptr(c)))
    finally:
        chk(L.kmap_counts_destroy(h))
    np.testing.assert_array_equal(u, want[0])
    np.testing.assert_array_equal(c, want[1])
    F.guards(*bufs)
    F.free(*bufs)


# ---- the list of entries ----------------------------------------------------------------------------------------------------------------
NOT_COVERED = {
    "kmap_memset": "the choreography's own tool (buffer fills)",
    "kmap_memcpy_h2d": "the choreography's own tool (uploads); blocking",
    "kmap_memcpy_d2h": "the choreography's own tool (read-backs); blocking",
    "kmap_memcpy_d2d": "the choreography's own tool: it carries the truth and the snapshots on the stream under test",
    "kmap_memcpy2d_d2h": "blocking pitched read-back, a one-line wrapper of hipMemcpy2DAsync + synchronise like kmap_memcpy_d2h",
    "kmap_stream_sync": "the choreography's own tool",
    "kmap_event_record": "timing helper of bench.py; records, launches nothing",
    "kmap_embed_step_peer": "needs more than one GPU (the kmap_peer_* exchange); tests/test_gpu_distributed.py runs it",
    "kmap_selftest_delay_dev": "the delay itself: the control shows that it holds its stream for the chosen time",
}


def test_every_stream_entry_has_a_case():
    """every prototype of include/kmap_hip.h with a `void *stream` parameter is named by a case of this file (@covers) or in
    NOT_COVERED with a reason; a new stream-taking entry fails here until it gets a case"""
    names = SO.stream_entries((ROOT / "include" / "kmap_hip.h").read_text())
    assert len(names) > 80
    here = {e for e, tests in SO.REGISTERED.items() if all(t in globals() for t in tests)}
    both = sorted(here & set(NOT_COVERED))
    assert not both, f"listed as not covered although a case names them: {both}"
    gone = sorted((here | set(NOT_COVERED)) - set(names))
    assert not gone, f"not in the header (any more), or without a stream parameter: {gone}"
    missing = [n for n in names if n not in here and n not in NOT_COVERED]
    assert not missing, f"entries with a stream parameter and no case in tests/test_gpu_streams.py: {missing}"
    assert all(len(r) > 10 for r in NOT_COVERED.values())
