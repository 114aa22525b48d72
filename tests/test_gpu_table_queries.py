"""The integer queries on a finished (uniq, cnt) table at the edges of their launch geometry, bit for bit against
tests/_table_model.py (held to the oracle by tests/test_table_model_host.py) and against the oracle where it has the function:
kmap_counts_total / _topk / _hamball_mass (csrc/counts_stats.hip), the Hamming-ball extraction from host arrays and from the resident
table, the label path of sample_disp_kmer through _LabelledTable (csrc/reports.hip) and the position density.

Launch geometry the shapes come from: 256-thread blocks; grids capped at 4096 (sum, label sums), 1024 (top-k) and 2048 (mass) blocks,
i.e. grid strides of 1 048 576, 262 144 and 524 288 entries; 16 top entries per thread; 16 candidates per mass launch; 1024 entries
per extraction block, whose counts are scanned by one block up to 4096 of them and tile by tile (2048 a tile) beyond.

Counts are the reference's int32 for k < 16 (bit 31 makes them negative) and unsigned 32-bit values for k >= 16, on every path."""
import ctypes as C
from contextlib import contextmanager
from types import SimpleNamespace

import numpy as np
import pytest

from tests import _table_model as M

pytestmark = pytest.mark.gpu

BIT31 = 1 << 31
TOPK_STRIDE = 1024 * 256
MASS_STRIDE = 2048 * 256
SUM_STRIDE = 4096 * 256


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


@pytest.fixture(scope="module")
def R():
    from kmap_amd import reports
    return reports


# ---- building tables -------------------------------------------------------------------------------------------------------------
def _hd(k):
    return np.uint32 if k < 16 else np.uint64


def _cd(k):
    return np.int32 if k < 16 else np.int64


def _counts(raw, k):
    """32-bit count values as the reference's count array: int32 with the same bits for k < 16, int64 otherwise"""
    raw = np.asarray(raw, np.int64)
    assert len(raw) == 0 or (0 <= int(raw.min()) and int(raw.max()) < 1 << 32)
    return raw.astype(np.uint32).view(np.int32) if k < 16 else raw.copy()


def _load(u, c, k):
    """a DeviceCounts handle holding (u, c), loaded as test_device_topk_tie_rule does"""
    from kmap_amd import _ffi
    from kmap_amd.kmer_count import DeviceCounts
    assert u.dtype == _hd(k) and c.dtype == _cd(k) and len(u) == len(c)
    dc = DeviceCounts()
    try:
        _ffi.check(_ffi.lib().kmap_counts_load(dc._h, _ffi.ptr(u), _ffi.ptr(c), len(u), k))
    except BaseException:
        dc.close()
        raise
    dc.k, dc.n_uniq = k, len(u)
    return dc


def _keys(rng, k, n, plant=(), avoid=None):
    """n sorted unique keys below 4^k: the first of `plant` that fit, the rest drawn; avoid(keys) -> mask of keys to leave out"""
    plant = np.unique(np.asarray(list(plant), np.int64))[:max(n // 2, 1 if n else 0)]
    s = plant
    while True:
        draw = rng.integers(0, 4 ** k, size=2 * n + 64, dtype=np.int64)
        if avoid is not None:
            draw = draw[~avoid(draw)]
        s = np.union1d(s, draw)
        if len(s) >= n:
            break
    extra = np.setdiff1d(s, plant)
    keep = rng.choice(extra, size=n - len(plant), replace=False)
    out = np.sort(np.concatenate([plant, keep]))
    assert len(out) == n and (n < 2 or (np.diff(out) > 0).all())
    return out.astype(_hd(k))


def _hash(s):
    h = 0
    for b in s:
        h = h * 4 + "ACGT".index(b)
    return h


def _kmer(h, k):
    return "".join("ACGT"[(int(h) >> (2 * (k - 1 - p))) & 3] for p in range(k))


def _rc(s):
    return "".join("TGCA"["ACGT".index(b)] for b in reversed(s))


def _canon(s):
    """the orientation with the smaller hash: how consensuses are stored in reverse-complement mode"""
    return s if _hash(s) <= _hash(_rc(s)) else _rc(s)


def _rand_kmer(rng, n):
    return "".join("ACGT"[b] for b in rng.integers(0, 4, size=n))


def _mutate(rng, s, n_mut, lo=0, hi=None):
    """s with n_mut distinct positions of [lo, hi) changed to another base"""
    s = list(s)
    for p in rng.choice(np.arange(lo, len(s) if hi is None else hi), size=n_mut, replace=False):
        s[p] = "ACGT"[("ACGT".index(s[p]) + int(rng.integers(1, 4))) % 4]
    return "".join(s)


# ---- total -----------------------------------------------------------------------------------------------------------------------
TOTAL_N = [0, 1, 63, 64, 65, 255, 256, 257, SUM_STRIDE, SUM_STRIDE + 1 + 300]


@pytest.mark.parametrize("k", [15, 16, 21])
def test_total(k):
    """k = 15: bit-31 counts, the signed sum; k = 16, 21: counts in [2^31, 2^32), the unsigned sum; the empty table; one entry up
    to one more than the grid stride of the sum"""
    rng = np.random.default_rng(k)
    if k < 16:
        big = rng.integers(0, 1 << 32, size=TOTAL_N[-1], dtype=np.int64)
        big[::2] |= BIT31
    else:
        big = rng.integers(BIT31, 1 << 32, size=TOTAL_N[-1], dtype=np.int64)
    for n in TOTAL_N:
        raw = big[:n]
        dc = _load(np.arange(n, dtype=_hd(k)), _counts(raw, k), k)
        try:
            got = dc.total()
        finally:
            dc.close()
        want = M.table_total(raw, k)
        print(f"total k={k} n={n}: device {got} model {want}")
        assert got == want, n
        assert n < 2 or (want > 1 << 32 if k >= 16 else want < int(raw.sum()) - (1 << 32))


# ---- top-k -----------------------------------------------------------------------------------------------------------------------
N_SLICE = 15 * TOPK_STRIDE + 1000      # a thread of the first 1000 owns the 16 entries i0 + j * TOPK_STRIDE, j = 0..15


def _topk_case(name):
    """(k, raw counts, top_k values) of one named table"""
    rng = np.random.default_rng(sum(map(ord, name)))
    ks = (1, 2, 15, 16)
    own = 700 + TOPK_STRIDE * np.arange(16)
    if name == "winners_in_one_thread":
        raw = rng.integers(1, 6, size=N_SLICE)
        raw[own] = 1000 + rng.permutation(16)
        return 12, raw, ks
    if name == "winners_in_one_block":
        raw = rng.integers(1, 6, size=5000)
        raw[:16] = 1000 + rng.permutation(16)
        return 9, raw, ks
    if name == "winners_in_last_partial_block":
        raw = rng.integers(1, 6, size=5000)                      # the last block starts at 4864
        raw[-16:] = 1000 + rng.permutation(16)
        return 9, raw, ks
    if name in ("plateau_across_blocks", "plateau_across_blocks_at_the_top"):
        raw = rng.integers(1, 6, size=5000)
        raw[[40, 41, 255, 256, 700, 1200, 1279, 1280, 2500, 2501, 3900, 4095, 4096, 4863, 4864, 4998, 4999, 3000, 3001, 3002]] = 7
        if name == "plateau_across_blocks":
            raw[[1234, 77]] = 9
        return 9, raw, ks
    if name in ("plateau_in_one_block", "plateau_in_one_block_at_the_top"):
        raw = rng.integers(1, 6, size=5000)
        raw[300:321] = 7
        if name == "plateau_in_one_block":
            raw[[4000, 310 + 256]] = 9
        return 9, raw, ks
    if name in ("plateau_in_one_thread", "plateau_in_one_thread_at_the_top"):
        raw = rng.integers(1, 6, size=N_SLICE)
        raw[own] = 7
        raw[own[:4] + 1] = 7                                     # and four more in the next thread
        if name == "plateau_in_one_thread":
            raw[[5, 99_999]] = 9
        return 12, raw, ks
    if name == "three_positive_entries":
        raw = np.zeros(5000, np.int64)
        raw[[4000, 17, 2600]] = [4, 9, 4]
        return 9, raw, (5, 1, 2, 3, 4, 16)
    if name == "one_entry":
        return 9, np.array([3]), ks
    if name == "k15_bit31_never_candidates":
        raw = rng.integers(BIT31, 1 << 32, size=5000)            # negative as int32 ...
        raw[rng.choice(5000, size=400, replace=False)] = 0
        raw[[4999, 0, 256, 2222, 2223, 255, 3000, 1, 4864, 1024]] = [3, 8, 8, BIT31 - 1, 5, 5, 5, 2, 1, 8]   # ... but for these ten
        return 15, raw, ks
    if name == "k16_bit31_ranks_first":
        raw = rng.integers(1, BIT31, size=5000)
        raw[[4321, 12, 2047, 2048, 3333]] = [(1 << 32) - 1, BIT31, BIT31 + 5, BIT31 + 5, (1 << 32) - 2]
        return 16, raw, ks
    raise KeyError(name)


@pytest.mark.parametrize("name", ["winners_in_one_thread", "winners_in_one_block", "winners_in_last_partial_block",
                                  "plateau_across_blocks", "plateau_across_blocks_at_the_top", "plateau_in_one_block",
                                  "plateau_in_one_block_at_the_top", "plateau_in_one_thread", "plateau_in_one_thread_at_the_top",
                                  "three_positive_entries", "one_entry", "k15_bit31_never_candidates", "k16_bit31_ranks_first"])
def test_topk(name):
    """largest count first, equal counts by the lowest index, positive counts only (signed for k < 16), n_found = min(top_k,
    positive entries)"""
    k, raw, top_ks = _topk_case(name)
    n = len(raw)
    u = (np.arange(n, dtype=np.int64) * 3 + 1).astype(_hd(k))
    assert int(u[-1]) < 4 ** k
    dc = _load(u, _counts(raw, k), k)
    try:
        all_idx, all_cnt = M.table_topk(raw, k, max(top_ks))          # one sort: a smaller top_k is a prefix of it
        for top_k in top_ks:
            idx, kh, cnt = dc.topk(top_k)
            widx, wcnt = all_idx[:top_k], all_cnt[:top_k]
            print(f"topk {name} top_k={top_k}: device {list(idx)} {list(cnt)} model {list(widx)} {list(wcnt)}")
            assert len(widx) == min(top_k, int(np.count_nonzero(M.count_values(raw, k) > 0)))
            np.testing.assert_array_equal(idx, widx)
            np.testing.assert_array_equal(cnt, wcnt)
            np.testing.assert_array_equal(kh, u[widx])
            assert kh.dtype == _hd(k)
    finally:
        dc.close()


# ---- Hamming-ball mass -------------------------------------------------------------------------------------------------------------
def _self_rc_like(rng, k):
    """a k-mer as close to its own reverse complement as k allows: equal to it (even k), one mismatch -- the middle base -- (odd k)"""
    half = _rand_kmer(rng, k // 2)
    return half + ("" if k % 2 == 0 else "G") + _rc(half)


def _mass_raw(rng, k, n):
    if k == 15:
        raw = rng.integers(0, 1 << 32, size=n, dtype=np.int64)
        raw[::2] |= BIT31
        return raw
    if k == 16:
        return rng.integers(BIT31, 1 << 32, size=n, dtype=np.int64)
    return rng.integers(1, 1000, size=n, dtype=np.int64)


def _mass_table(k, n, seed):
    """(keys, raw counts, 33 candidates): the candidates' own neighbourhoods are planted in the table"""
    rng = np.random.default_rng(seed)
    special = _self_rc_like(rng, k)
    assert M.popc2(_hash(special) ^ _hash(_rc(special))) == k % 2
    seeds = [special, _mutate(rng, special, 1), _rc(_mutate(rng, special, 2))] + [_rand_kmer(rng, k) for _ in range(8)]
    plant = [_hash(s) for s in seeds] + [_hash(_rc(s)) for s in seeds[3:7]]
    plant += [_hash(_mutate(rng, s, int(rng.integers(1, 4)))) for s in seeds for _ in range(6)]
    if k == 16:
        plant = [0xFFFFFFFF] + plant                       # the all-T 16-mer: the key that is the invalid marker of the 32-bit hashes
    u = _keys(rng, k, n, plant)
    cands = [_hash(s) for s in seeds] + [int(x) for x in u[rng.integers(0, n, size=10)]]
    cands += [_hash(_mutate(rng, _kmer(x, k), 1)) for x in u[rng.integers(0, n, size=33 - len(cands))]]
    if k == 16:
        cands[5] = 0xFFFFFFFF
    cands[7], cands[16], cands[20] = cands[2], cands[0], cands[19]    # duplicates inside a launch and across launches
    assert len(cands) == 33
    return u, _mass_raw(rng, k, n), cands


@pytest.mark.parametrize("k", [8, 15, 16, 17, 31])
def test_hamball_mass_candidates(O, k):
    """0 to 33 candidates (a second and a third launch from 17 on) with duplicates, a palindrome (even k) or a candidate one
    mismatch from its own reverse complement (odd k); radius 0, 1, k / 2, k, k + 1 and -1; reverse complement off and on"""
    u, raw, cands = _mass_table(k, 257, 40 + k)
    c = _counts(raw, k)
    if k == 16:
        assert 0xFFFFFFFF in u
    dc = _load(u, c, k)
    try:
        for n_cand in (0, 1, 15, 16, 17, 33):
            cd = np.array(cands[:n_cand], np.uint64)
            for r in (0, 1, k // 2, k, k + 1, -1):
                for rc in (False, True):
                    got = [int(x) for x in dc.hamball_mass(cd, r, rc)]
                    want = M.ball_mass(u, raw, k, cands[:n_cand], r, rc)
                    assert got == want, (n_cand, r, rc)
                    assert [int(x) for x in O.hamball_mass(u, c, k, cd, r, rc)] == want, (n_cand, r, rc)
        full = M.ball_mass(u, raw, k, cands[:1], k, True)[0]
        assert full == M.table_total(raw, k) and M.ball_mass(u, raw, k, cands[:1], 0, True)[0] != 0
        if k % 2 == 0:   # the palindrome's ball is counted once: reverse complement on and off agree
            assert M.ball_mass(u, raw, k, cands[:1], 1, True) == M.ball_mass(u, raw, k, cands[:1], 1, False)
    finally:
        dc.close()


MASS_N = [1, 255, 256, 257, MASS_STRIDE, MASS_STRIDE + 1 + 700]


@pytest.mark.parametrize("k", [8, 15, 16, 17, 31])
def test_hamball_mass_table_sizes(O, k):
    """one entry up to one more than the grid stride of the mass kernel (k = 8 has 4^8 keys: the sizes below that), 17 candidates"""
    sizes = [n for n in MASS_N if n <= 4 ** k // 4]
    u_all, raw_all, cands = _mass_table(k, sizes[-1], 60 + k)
    cands = cands[:17]
    cd = np.array(cands, np.uint64)
    dist = {rc: [M.ball_dist(M.as_keys(u_all), x, k, rc)[0] for x in cands] for rc in (False, True)}   # once for every size
    val = M.count_values(raw_all, k)
    for n in sizes:
        u, raw = u_all[:n].copy(), raw_all[:n]
        c = _counts(raw, k)
        dc = _load(u, c, k)
        try:
            for r, rc in ((1, True), (3 * k // 4, True), (3 * k // 4, False)):
                got = [int(x) for x in dc.hamball_mass(cd, r, rc)]
                want = [M.isum(val[:n][d[:n] <= r]) for d in dist[rc]]
                print(f"mass k={k} n={n} r={r} rc={rc}: device {got[:3]}.. model {want[:3]}..")
                assert got == want, (n, r, rc)
                n_o = 17 if n < MASS_STRIDE else 4      # the oracle walks the bases one by one: a few candidates at the large sizes
                assert [int(x) for x in O.hamball_mass(u, c, k, cd[:n_o], r, rc)] == want[:n_o], (n, r, rc)
        finally:
            dc.close()
    assert any(w != 0 for w in want)


# ---- Hamming-ball extraction -------------------------------------------------------------------------------------------------------
def _resident_extract(dc, k, cons, r, rc, cap, fill=None):
    """one call of kmap_counts_hamball_extract with a count matrix -> (n_out, keys[cap], counts[cap], matrix); the output arrays
    are pre-filled with `fill`"""
    from kmap_amd import _ffi
    ou, oc = np.empty(max(cap, 1), _hd(k)), np.empty(max(cap, 1), _cd(k))
    mat = np.full((4, k), -1, np.int64)
    if fill is not None:
        ou[:], oc[:] = fill, fill
    n_out = _ffi.i64(-1)
    _ffi.check(_ffi.lib().kmap_counts_hamball_extract(dc._h, int(cons), int(r), int(rc), cap, _ffi.ptr(ou), _ffi.ptr(oc),
                                                      C.byref(n_out), _ffi.ptr(mat)))
    return n_out.value, ou, oc, mat


def _check_ball(R, O, u, raw, k, cons, r, rc, dc=None):
    """host-array and resident extraction == oracle == model: keys, counts, dtypes, count matrix; returns the member indices"""
    c = _counts(raw, k)
    wu, wc = O.ex_hamball(u, c, k, cons, r, rc)
    wmat = O.cal_cnt_mat(wu, wc, k)
    mu, mc = M.ball_members(u, raw, k, cons, r, rc)
    np.testing.assert_array_equal(wu.astype(np.int64), mu)
    np.testing.assert_array_equal(wc, mc)
    hu, hc, hmat = R._hamball_extract(u, c, k, cons, r, rc)
    assert hu.dtype == _hd(k) and hc.dtype == _cd(k)
    np.testing.assert_array_equal(hu, wu)
    np.testing.assert_array_equal(hc, wc)
    np.testing.assert_array_equal(hmat, wmat)
    own = dc is None
    dc = _load(u, c, k) if own else dc
    try:
        du, dcnt = R._hamball_extract_resident(dc, k, cons, r, rc)
        assert du.dtype == _hd(k) and dcnt.dtype == _cd(k)
        np.testing.assert_array_equal(du, wu)
        np.testing.assert_array_equal(dcnt, wc)
        n_out, du, dcnt, dmat = _resident_extract(dc, k, cons, r, rc, len(wu))
        assert n_out == len(wu)
        np.testing.assert_array_equal(du[:n_out], wu)
        np.testing.assert_array_equal(dcnt[:n_out], wc)
        np.testing.assert_array_equal(dmat, wmat)
    finally:
        if own:
            dc.close()
    return np.flatnonzero(M.ball_dist(M.as_keys(u), cons, k, rc)[0] <= r)


def _edge_slot_table(rng, k, n, cons, r):
    """n sorted keys whose members of the ball (cons, r) -- with or without the reverse complement -- sit exactly in the first and
    the last slot of every 1024-entry block: the members are cons itself and single-base changes among its first six bases (4^(k-6)
    or more apart), the slots in between are filled with the non-members just below the next member"""
    slots = sorted({b * 1024 + s for b in range((n + 1023) // 1024) for s in (0, 1023) if b * 1024 + s < n})
    mem = sorted({_hash(cons)} | {_hash(cons[:p] + b + cons[p + 1:]) for p in range(6) for b in "ACGT"})[-len(slots):]

    def fillers(start, step, count):
        out, x = [], start
        while len(out) < count:
            if M.ball_dist(np.array([x], np.int64), _hash(cons), k, True)[0][0] > r:
                out.append(x)
            x += step
        return out
    keys, prev = [], -1
    for s, m in zip(slots, mem):
        keys += fillers(m - 1, -1, s - prev - 1) + [m]
        prev = s
    keys += fillers(mem[-1] + 1, 1, n - 1 - prev)
    keys = np.array(sorted(keys), np.int64)
    assert len(keys) == n and (np.diff(keys) > 0).all() and keys[0] >= 0 and keys[-1] < 4 ** k
    return keys.astype(_hd(k)), slots


EXTRACT_N = [1, 3, 4, 5, 1023, 1024, 1025, 2048, 2049]


@pytest.mark.parametrize("k", [12, 17])
@pytest.mark.parametrize("pattern", ["no_members", "all_members", "first_and_last_slot", "reoriented"])
def test_hamball_extract_block_edges(R, O, k, pattern):
    """one entry, the four items of a thread, the 1024 entries of a block and two blocks, each +-1; host arrays and resident table"""
    rng = np.random.default_rng(1000 * k + len(pattern))
    cons = "C" + _rand_kmer(rng, k - 2) + "A"                     # canonical: its reverse complement starts with T
    near = [_mutate(rng, cons, int(rng.integers(0, 3))) for _ in range(40)]
    for n in EXTRACT_N:
        raw = rng.integers(1, 1000, size=n)
        if k >= 16:
            raw[::3] += BIT31                                      # unsigned on both entry points
        if pattern == "no_members":
            u = _keys(rng, k, n, avoid=lambda x: M.ball_dist(x, _hash(cons), k, True)[0] <= 1)
            assert len(_check_ball(R, O, u, raw, k, _hash(cons), 1, True)) == 0
            assert len(_check_ball(R, O, u, raw, k, _hash(cons), -1, True)) == 0
        elif pattern == "all_members":
            u = _keys(rng, k, n, [_hash(s) for s in near] + [_hash(_rc(s)) for s in near])
            assert len(_check_ball(R, O, u, raw, k, _hash(cons), k, True)) == n
            assert len(_check_ball(R, O, u, raw, k, _hash(cons), k, False)) == n
        elif pattern == "first_and_last_slot":
            u, slots = _edge_slot_table(rng, k, n, cons, 1)
            for rc in (False, True):
                assert list(_check_ball(R, O, u, raw, k, _hash(cons), 1, rc)) == slots
        else:
            u = _keys(rng, k, n, [_hash(_rc(s)) for s in near] + [_hash(s) for s in near[:10]])
            idx = _check_ball(R, O, u, raw, k, _hash(cons), 2, True)
            assert len(idx) >= min(n, 20) // 2
            wu, _ = O.ex_hamball(u, _counts(raw, k), k, _hash(cons), 2, True)
            assert (wu != u[idx]).any()                            # members that came through the reverse complement


BIG_N = 4096 * 1024 + 1025       # 4098 blocks: the scan of the block counts goes tile by tile


@pytest.mark.parametrize("pattern", ["no_members", "all_members", "some_reoriented"])
def test_hamball_extract_past_4096_blocks(R, O, pattern):
    k = 12
    rng = np.random.default_rng(len(pattern))
    u = np.arange(BIG_N, dtype=np.uint32)                          # every 12-mer that starts with A, and 1025 that start with C
    raw = rng.integers(1, 1000, size=BIG_N)
    cons = "AAAAAACCCCCT"                                          # its reverse complement AGGGGGTTTTTT starts with A too
    if pattern == "no_members":
        assert len(_check_ball(R, O, u, raw, k, _hash("GGGGGGGGGGGT"), 0, False)) == 0       # no key starts with G
    elif pattern == "all_members":
        assert len(_check_ball(R, O, u, raw, k, _hash(cons), k, True)) == BIG_N
    else:
        idx = _check_ball(R, O, u, raw, k, _hash(cons), 3, True)
        wu, _ = O.ex_hamball(u, _counts(raw, k), k, _hash(cons), 3, True)
        assert (wu != u[idx]).any() and idx[0] < 1024 and idx[-1] >= 4096 * 1024     # first block ... past block 4096


@pytest.mark.parametrize("k", [12, 17])
def test_hamball_extract_resident_cap_and_signedness(R, O, k):
    """cap below the member count: nothing is written and n_out says how many there are; the count matrix of the resident table
    follows the signedness rule (bit-31 counts: negative for k = 12, unsigned for k = 17)"""
    rng = np.random.default_rng(k)
    cons = "C" + _rand_kmer(rng, k - 2) + "A"
    near = [_mutate(rng, cons, int(rng.integers(0, 3))) for _ in range(40)]
    u = _keys(rng, k, 1500, [_hash(s) for s in near] + [_hash(_rc(s)) for s in near])
    raw = rng.integers(1, 1000, size=len(u))
    dc = _load(u, _counts(raw, k), k)
    try:
        members = len(_check_ball(R, O, u, raw, k, _hash(cons), 2, True, dc=dc))
        assert members > 20
        for cap in (0, 1, members - 1):
            n_out, du, dcnt, _ = _resident_extract(dc, k, _hash(cons), 2, True, cap, fill=77)
            assert n_out == members and (du == 77).all() and (dcnt == 77).all(), cap
    finally:
        dc.close()
    raw[::2] += BIT31
    _check_ball(R, O, u, raw, k, _hash(cons), 2, True)


# ---- the label path of sample_disp_kmer ------------------------------------------------------------------------------------------
@contextmanager
def _labelled(u, c, cons, k, radius_of_len, revcom, resident):
    """a _LabelledTable over host arrays, or over the table of a DeviceCounts handle loaded with them"""
    from kmap_amd.motif_discovery import _LabelledTable
    md = {n: SimpleNamespace(max_ham_dist=r) for n, r in radius_of_len.items()}
    dc = tab = None
    try:
        if resident:
            dc = _load(u, c, k)
            tab = _LabelledTable(None, None, cons, k, md, revcom, resident=dc)
        else:
            tab = _LabelledTable(u, c, cons, k, md, revcom)
        yield tab
    finally:
        if tab is not None:
            tab.close()
        if dc is not None:
            dc.close()


def _model_labels(u, cons, k, radius_of_len, revcom):
    return M.label_table(u, k, [_hash(s) for s in cons], [len(s) for s in cons], [radius_of_len[len(s)] for s in cons],
                         radius_of_len[k], revcom)


def _label_seeds(rng, k):
    """consensuses with planted neighbourhoods: two k-long ones two bases apart and a k-mer one base from both, a (k-2)-long one, a
    palindrome"""
    c1 = "A" + _rand_kmer(rng, k - 2) + "A"                       # canonical whatever lies between: the reverse complement starts with T
    c2 = c1[0] + "ACGT"[("ACGT".index(c1[1]) + 1) % 4] + "ACGT"[("ACGT".index(c1[2]) + 2) % 4] + c1[3:]
    mid = c1[0] + c2[1] + c1[2:]                                  # one base from c1 and from c2
    short = "A" + _rand_kmer(rng, k - 4) + "C"
    pal = _self_rc_like(rng, k if k % 2 == 0 else 6)
    plant = [c1, c2, mid, _rc(mid), _rc(c1)] + [_mutate(rng, x, int(rng.integers(1, 4))) for x in (c1, c2, mid) for _ in range(8)]
    for _ in range(40):
        s = _mutate(rng, short, int(rng.integers(0, 5))) + _rand_kmer(rng, 2)
        plant += [s, _rc(s)]
    for _ in range(12):
        s = _mutate(rng, pal, int(rng.integers(0, 3)))
        plant.append(s + _rand_kmer(rng, k - len(s)))
    return dict(c1=c1, c2=c2, mid=mid, short=short, pal=pal), [_hash(s) for s in plant]


def _three_mers(revcom):
    """32 consensuses of length 3: with the reverse complement the 32 canonical ones (no 3-mer is its own), else the first 32"""
    all3 = [_kmer(h, 3) for h in range(64)]
    return [s for s in all3 if _canon(s) == s] if revcom else all3[:32]


def _label_configs(rng, k, u, seeds, revcom):
    """name -> (consensus list, longest first; radius by consensus length)"""
    fix = _canon if revcom else (lambda s: s)
    table_kmers = [fix(_kmer(h, k)) for h in u[rng.choice(len(u), size=min(29, len(u)), replace=False)]]
    k_long = ([seeds["c1"], seeds["c2"]] + table_kmers * 31)[:31]
    base = {n: n // 4 for n in range(1, 32)}
    return {
        "63_consensuses": (k_long + _three_mers(revcom), {**base, 3: 0}),
        "one_k_long": ([table_kmers[0]], {**base, k: k // 3}),
        "one_of_length_3": ([fix("ACG")], {**base, 3: 1, k: 1}),
        "tie_first_wins": ([seeds["c1"], seeds["c2"]], {**base, k: 2}),
        "tie_first_wins_swapped": ([seeds["c2"], seeds["c1"]], {**base, k: 2}),
        "radius_0": ([seeds["c1"], seeds["short"]], {**base, k: 0, k - 2: 0}),
        "radius_k_below_own_radius": ([seeds["short"]], {**base, k - 2: 4, k: 1}),
        "palindrome": ([seeds["pal"], fix("ACG")] if len(seeds["pal"]) == k else [seeds["short"], seeds["pal"]],
                       {**base, k: 2, k - 2: 2, 6: 1, 3: 0}),
    }


LABEL_N = [1, 255, 256, 257, 2048, 2049, 4096, 4097, 6145]


@pytest.mark.parametrize("resident", [False, True], ids=["host_arrays", "resident"])
@pytest.mark.parametrize("k", [8, 15, 16, 21, 31])
def test_labels_and_reoriented_keys(k, resident):
    """labels and re-oriented keys of every entry: 63 consensuses (lengths k and 3) at every n, the other configurations at 6145"""
    rng = np.random.default_rng(7 * k + resident)
    seeds, plant = _label_seeds(rng, k)
    seen_labels, flipped = set(), 0
    for n in LABEL_N:
        u = _keys(rng, k, n, plant)
        raw = rng.integers(1, 1000, size=n)
        for revcom in (True, False):
            configs = _label_configs(rng, k, u, seeds, revcom)
            for name in (configs if n == LABEL_N[-1] else ["63_consensuses"]):
                cons, radius_of_len = configs[name]
                wlab, wu = _model_labels(u, cons, k, radius_of_len, revcom)
                with _labelled(u, _counts(raw, k), cons, k, radius_of_len, revcom, resident) as tab:
                    gu, glab = tab.whole_table()
                assert gu.dtype == _hd(k)
                np.testing.assert_array_equal(glab, wlab, err_msg=f"{name} n={n} revcom={revcom}")
                np.testing.assert_array_equal(gu, wu.astype(_hd(k)), err_msg=f"{name} n={n} revcom={revcom}")
                if name.startswith("tie") and revcom:
                    at = int(np.searchsorted(u, _hash(seeds["mid"])))
                    assert u[at] == _hash(seeds["mid"]) and wlab[at] == 0       # one base from both: the first listed wins
                if name == "63_consensuses":
                    seen_labels |= set(wlab.tolist())
                    flipped += int((wu != M.as_keys(u)).sum())
    assert len(seen_labels) > 32 and 0 in seen_labels and flipped > 100      # the tables exercise what they are meant to


def _totals_table(k, n, seed):
    """keys, raw counts (k = 15: bit 31 set in half of them; k = 16: all in [2^31, 2^32)) and three consensuses, the middle one
    without members"""
    rng = np.random.default_rng(seed)
    c1 = "A" + _rand_kmer(rng, k - 2) + "A"
    empty = "A" * (k - 1)                                         # no key starts with it, none ends in its reverse complement
    plant = [_hash(_mutate(rng, x, int(rng.integers(0, 2)))) for x in (c1, _rc(c1)) for _ in range(30)]
    u = _keys(rng, k, n, plant, avoid=lambda x: ((x >> 2) == 0) | ((x & (4 ** (k - 1) - 1)) == 4 ** (k - 1) - 1))
    return u, _mass_raw(rng, k, n), [c1, empty, "ACG"], {**{m: 0 for m in range(1, 32)}, k: 1, 3: 1}


@pytest.mark.parametrize("resident", [False, True], ids=["host_arrays", "resident"])
@pytest.mark.parametrize("n", [6145, SUM_STRIDE + 300])
@pytest.mark.parametrize("k", [15, 16])
def test_label_totals_and_members(k, n, resident):
    """per-label count sums and member counts, then the member indices of every label.  k = 15: bit-31 counts are negative on both
    paths.  k = 16: counts in [2^31, 2^32) are unsigned on both paths -- the resident table holds them as uint32 bins and must not
    sign-extend them."""
    u, raw, cons, radius_of_len = _totals_table(k, n, 100 * k + (n & 1))
    wlab, _ = _model_labels(u, cons, k, radius_of_len, True)
    ww, wm = M.label_sums(wlab, raw, k, len(cons) + 1)
    assert wm[1] == 0 and wm[0] > 10 and wm[2] > n // 100 and wm[3] > n // 100
    with _labelled(u, _counts(raw, k), cons, k, radius_of_len, True, resident) as tab:
        gw, gm = tab.label_totals()
        print(f"label_totals k={k} n={n} resident={resident}: device {gw.tolist()} model {ww}")
        assert gm.tolist() == wm
        assert gw.tolist() == ww
        for c in range(len(cons) + 1):
            np.testing.assert_array_equal(tab.member_indices(c, wm[c]), M.members_of(wlab, c), err_msg=f"label {c}")


@pytest.mark.parametrize("resident", [False, True], ids=["host_arrays", "resident"])
@pytest.mark.parametrize("k", [15, 16])
def test_label_totals_all_noise(k, resident):
    u, raw, cons, radius_of_len = _totals_table(k, 6145, k)
    with _labelled(u, _counts(raw, k), cons[1:2], k, radius_of_len, True, resident) as tab:
        gw, gm = tab.label_totals()
        assert gm.tolist() == [0, 6145] and gw.tolist() == [0, M.table_total(raw, k)]
        assert len(tab.member_indices(0, 0)) == 0
        np.testing.assert_array_equal(tab.member_indices(1, 6145), np.arange(6145))


def _cdf_case(name):
    """(k, n, raw counts, consensuses, radius by length): one label with a few hundred members or more where n allows"""
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "big_counts_6145_members":     # every 2048-entry tile of the scan sums to more than 2^32
        k, n = 16, 6145
        raw = rng.integers(2_900_000_000, 3_100_000_000, size=n)
        return k, n, raw, ["ACG"], {**{m: m for m in range(1, 32)}}           # radius 3 of 3, radius k of k: every entry is a member
    k, n = {"n_1": (8, 1), "n_4096": (15, 4096), "n_4097": (15, 4097), "n_4097_k21": (21, 4097)}[name]
    raw = rng.integers(1, 1000, size=n)
    raw[rng.choice(n, size=n // 5, replace=False)] = 1              # width-1 intervals: boundary +-1 lands in the neighbours
    return k, n, raw, ["ACG"], {**{m: 1 for m in range(1, 32)}}


@pytest.mark.parametrize("resident", [False, True], ids=["host_arrays", "resident"])
@pytest.mark.parametrize("name", ["n_1", "n_4096", "n_4097", "n_4097_k21", "big_counts_6145_members"])
def test_cdf_prefix_and_search(name, resident):
    """the two calls of cdf_pick -- kmap_label_prefix_dev over a label's counts, then kmap_prefix_search_dev -- with targets at 0, at
    every boundary +-1 of the cumulative counts of up to 300 members, and at the total -1 / +0 / +1; the prefix itself is compared
    too.  The single-block scan serves n <= 4096, the tile scan n > 4096; a tile of counts may sum past 2^32."""
    from kmap_amd import _ffi
    k, n, raw, cons, radius_of_len = _cdf_case(name)
    rng = np.random.default_rng(n)
    u = _keys(rng, k, n)
    wlab, _ = _model_labels(u, cons, k, radius_of_len, True)
    lib = _ffi.lib()
    with _labelled(u, _counts(raw, k), cons, k, radius_of_len, True, resident) as tab:
        for c in range(len(cons) + 1):
            w = np.where(wlab == c, raw, 0)
            excl = np.concatenate([[0], np.cumsum(w, dtype=np.int64)])
            total = int(excl[-1])
            if total == 0:
                continue
            mem = M.members_of(wlab, c)
            mem = mem[np.unique(np.linspace(0, len(mem) - 1, 300).astype(np.int64))]
            edges = np.concatenate([excl[mem], excl[mem + 1], [total]])
            targets = np.unique(np.clip(np.concatenate([[0], edges - 1, edges, edges + 1]), 0, total + 1)).astype(np.int64)
            _ffi.check(lib.kmap_label_prefix_dev(tab.lab_d.ptr, tab.c_d.ptr, tab.cnt64, tab.n, c, tab.w32_d.ptr, tab.excl_d.ptr, None))
            hit = np.full(len(targets), -1, np.int64)
            _ffi.check(lib.kmap_prefix_search_dev(tab.excl_d.ptr, tab.n, _ffi.ptr(targets), len(targets), _ffi.ptr(hit)))
            got_excl = tab.excl_d.to_numpy(np.uint64, (n + 1,))
            want = M.cdf_hits(w, targets)
            bad = np.flatnonzero(hit != want)
            print(f"cdf {name} resident={resident} label {c}: total {total}, device total {int(got_excl[-1])}, "
                  f"{len(bad)} of {len(targets)} targets differ")
            np.testing.assert_array_equal(got_excl, excl.astype(np.uint64))
            np.testing.assert_array_equal(hit, want)
            assert want[-1] == n and want[-3] < n and (name == "n_1" or len(np.unique(want)) > min(len(mem), 100))
    if name.startswith("big"):
        assert all(int(raw[t:t + 2048].sum()) > 1 << 32 for t in range(0, n - 1, 2048)) and (wlab == 0).all()


@pytest.mark.parametrize("resident", [False, True], ids=["host_arrays", "resident"])
@pytest.mark.parametrize("k", [8, 16])
def test_gather_at_indices(k, resident):
    """kmers_at / counts_at / labels_at: 0, 1 and a block +-1 of unsorted, repeated indices"""
    rng = np.random.default_rng(k)
    seeds, plant = _label_seeds(rng, k)
    n = 6145
    u, raw = _keys(rng, k, n, plant), _mass_raw(rng, k, n)
    cons, radius_of_len = _label_configs(rng, k, u, seeds, True)["63_consensuses"]
    wlab, wu = _model_labels(u, cons, k, radius_of_len, True)
    c = _counts(raw, k)
    with _labelled(u, c, cons, k, radius_of_len, True, resident) as tab:
        for m in (0, 1, 255, 256, 257):
            idx = rng.integers(0, n, size=m)
            if m > 2:
                idx[-1], idx[m // 2] = idx[0], n - 1
                assert (np.diff(idx) < 0).any()
            got_u, got_c, got_l = tab.kmers_at(idx), tab.counts_at(idx), tab.labels_at(idx)
            assert got_u.dtype == _hd(k) and got_c.dtype == _cd(k) and len(got_u) == len(got_c) == len(got_l) == m
            np.testing.assert_array_equal(got_u, wu[idx].astype(_hd(k)))
            np.testing.assert_array_equal(got_c, c[idx])
            np.testing.assert_array_equal(got_l, wlab[idx])


# ---- position density ------------------------------------------------------------------------------------------------------------
def _density_rows(rng, n_seq, kmer_len, first):
    """hits / positions / read lengths: read 0 is `first` -- a single hit at position 0, a single hit in the last window, or a read
    as long as the k-mer --, reads 1 and 2 are the other two where there are that many, the reads on both sides of every 256-read
    block edge have no hit"""
    seq_len = rng.integers(kmer_len + 1, 300, size=n_seq).astype(np.int64)
    hits = np.where(rng.random(n_seq) < 0.7, rng.integers(1, 6, size=n_seq), 0).astype(np.int32)
    kinds = [first] + [x for x in ("at_0", "last_window", "read_is_one_window") if x != first]
    for r, kind in enumerate(kinds[:n_seq]):
        hits[r] = 1
        if kind == "read_is_one_window":
            seq_len[r] = kmer_len
    for r in (255, 256, 511, 512):
        if r < n_seq:
            hits[r] = 0
    pos = [np.sort(rng.integers(0, seq_len[r] - kmer_len + 1, size=hits[r])) for r in range(n_seq)]
    for r, kind in enumerate(kinds[:n_seq]):
        pos[r] = np.array([seq_len[r] - kmer_len if kind == "last_window" else 0])
    return hits, np.concatenate(pos).astype(np.int32), seq_len


@pytest.mark.parametrize("n_seq", [1, 255, 256, 257, 513])
def test_pos_density_block_and_grid_edges(R, O, n_seq):
    """reads at the 256-read block edges of pos_density_kernel, grids at the 128-thread edge; f64 against the oracle's sequential
    sum at the tolerance of test_gpu_reports.py.  The bandwidth keeps every term a normal float64 (|z| <= 20)."""
    kmer_len, bandwidth = 9, 0.05
    for first in ("at_0", "last_window", "read_is_one_window"):
        rng = np.random.default_rng(n_seq)
        hits, pos, seq_len = _density_rows(rng, n_seq, kmer_len, first)
        occ = R.Occurrence([hits], [pos], seq_len)
        offs = occ.offs(0)
        rows = [(pos[offs[r]:offs[r + 1]].tolist(), seq_len[r]) for r in range(n_seq) if hits[r]]
        for nx in (1, 127, 128, 129):
            x_arr = np.linspace(0.0, 1.0, nx) if nx > 1 else np.array([0.5])
            n, m, d = R.get_motif_pos_density(occ, 0, kmer_len, x_step=bandwidth, x_arr=x_arr)
            want = O.motif_pos_density(rows, kmer_len, x_arr, bandwidth)
            assert n == len(rows) and m == int(hits.sum()) and d.shape == (nx,)
            np.testing.assert_allclose(d, want, rtol=1e-12, atol=1e-300)
            assert (want > 0).all()
        if n_seq > 3:
            break            # the three special reads are all in one table
