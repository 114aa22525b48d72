"""enrich_kmers on the GPU (csrc/enrich.hip) against exact integer arithmetic, against the counting kernels that exist, against
np.lexsort for the selection, and the verb end to end against a numpy restatement.  Definitions: DESIGN.md section 12.

z bound: |z - z_ref| <= 16 * 2^-53 * |z_ref|.  At most six roundings of 2^-53 reach z: one to two in converting D, three in s (halved by
the root), one in the root and one in the division; 16 leaves a margin of about 2.7 and covers a square root that is 1 ulp off.
z_ref itself is evaluated from the exact integer D in 64-bit-mantissa long doubles (five roundings of 2^-64: 0.003 of one of those
2^-53), or with 60-digit decimals where long double is no wider than double."""
import ctypes as C
from decimal import Decimal, getcontext
from pathlib import Path

import numpy as np
import pytest
from numpy.lib.stride_tricks import sliding_window_view

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
GOLD = ROOT / "tests" / "golden"
U32MAX = 2 ** 32 - 1
TMAX = 2 ** 52 - 1
Z_TOL = 16 * 2.0 ** -53
LD = np.longdouble
WIDE = np.finfo(LD).nmant >= 63
KMAP_E_INVAL, KMAP_E_UNSUP, KMAP_E_STATE = -1, -4, -5


# ---- helpers ----------------------------------------------------------------------------------------------------------------
def key_dtype(k):
    return np.uint32 if k < 16 else np.uint64


def rc_keys(x, k):
    """reverse complement of every key (uint64 in, uint64 out)"""
    x = np.asarray(x, np.uint64)
    com = np.uint64(4 ** k - 1) - x
    out = np.zeros_like(com)
    for _ in range(k):
        out = (out << np.uint64(2)) | (com & np.uint64(3))
        com = com >> np.uint64(2)
    return out


def load_table(dc, keys, cnt, k):
    """a (keys, counts) table into a DeviceCounts; counts up to 2^32 - 1 (the device keeps them as uint32)"""
    from kmap_amd import _ffi
    u = np.ascontiguousarray(np.asarray(keys, np.uint64).astype(key_dtype(k)))
    c = np.asarray(cnt, np.uint64)
    c = np.ascontiguousarray(c.astype(np.uint32).view(np.int32) if k < 16 else c.astype(np.int64))
    dc._unshard()
    _ffi.check(_ffi.lib().kmap_counts_load(dc._h, _ffi.ptr(u), _ffi.ptr(c), len(u), k))
    dc.k, dc.n_uniq = k, len(u)


def expected_b(fkeys, bkeys, bcnt, k, revcom):
    """b_i = B[x_i] + (revcom ? B[rc x_i] : 0) as Python integers (object array); bkeys ascending"""
    def look(x):
        if len(bkeys) == 0:
            return np.zeros(len(x), object)
        pos = np.minimum(np.searchsorted(bkeys, x), len(bkeys) - 1)
        return np.where(bkeys[pos] == x, bcnt[pos].astype(object), 0)
    b = look(fkeys)
    if revcom:
        b = b + look(rc_keys(fkeys, k))
    return b.astype(object)


def z_reference(a, b, Nf, Nb):
    """(D as Python integers, z_ref as long double) of every entry; a, b object arrays of Python integers"""
    n = len(a)
    D = a * Nb - b * Nf if n else np.zeros(0, object)
    if Nf + Nb == 0:
        return D, np.zeros(n, LD)
    if WIDE:
        mag = np.abs(D)
        hi = (mag >> 40).astype(np.float64).astype(LD)            # |D| < 2^85: both halves are exact
        lo = (mag & (2 ** 40 - 1)).astype(np.float64).astype(LD)
        Dl = (hi * LD(2.0 ** 40) + lo) * np.where(D < 0, -1.0, 1.0).astype(LD)
        ab = (a + b).astype(np.float64).astype(LD)                # < 2^34, and Nf + Nb - a - b < 2^53: exact
        rest = (Nf + Nb - a - b).astype(np.float64).astype(LD)
        s = ab * rest * LD(Nf) * LD(Nb) / LD(Nf + Nb)
        with np.errstate(divide="ignore", invalid="ignore"):
            z = np.where(s > 0, Dl / np.sqrt(np.where(s > 0, s, LD(1))), LD(0))
        return D, z
    getcontext().prec = 60
    z = np.zeros(n, LD)
    for i in range(n):
        s = Decimal(int(a[i] + b[i]) * int(Nf + Nb - a[i] - b[i]) * Nf * Nb) / Decimal(Nf + Nb)
        z[i] = LD(float(Decimal(int(D[i])) / s.sqrt())) if s > 0 else LD(0)
    return D, z


def check_scores(b_got, z_got, a, b, Nf, Nb, where=""):
    np.testing.assert_array_equal(b_got, b.astype(np.uint64), err_msg=f"b {where}")
    assert not np.isnan(z_got).any(), where
    D, z_ref = z_reference(a, b, Nf, Nb)
    err = np.abs(z_got.astype(LD) - z_ref)
    bad = np.nonzero(err > LD(Z_TOL) * np.abs(z_ref))[0]
    assert len(bad) == 0, (where, len(bad), int(bad[0]), float(z_got[bad[0]]), float(z_ref[bad[0]]), int(a[bad[0]]), int(b[bad[0]]), Nf, Nb)
    zero = np.nonzero(D == 0)[0]
    assert not np.signbit(z_got[zero]).any() and (z_got[zero] == 0).all(), where      # a Nb == b Nf: +0.0
    return D


@pytest.fixture(scope="module")
def env():
    from kmap_amd import _ffi
    from kmap_amd.enrichment import DeviceEnrich
    from kmap_amd.kmer_count import DeviceCounts
    return _ffi, DeviceCounts, DeviceEnrich


# ---- 1. every entry against exact arithmetic -----------------------------------------------------------------------------------
def palindrome(u, k):
    """the even-length k-mer u + rc(u)"""
    h = k // 2
    return (int(u) << (2 * h)) | int(rc_keys(np.array([u], np.uint64), h)[0])


def sample_keys(rng, nkeys, n):
    """n distinct keys below nkeys, ascending"""
    if nkeys <= 1 << 22:
        return np.sort(rng.choice(nkeys, size=n, replace=False)).astype(np.uint64)
    got = np.unique(rng.integers(0, nkeys, size=2 * n + 64, dtype=np.uint64))
    return np.sort(rng.permutation(got)[:n])


def make_case(k, n_fg, n_bg, revcom, rng):
    """(fkeys shuffled, a, bkeys ascending, bcnt, plan).  Planted in F: key 0 and the largest key, B's first and last key, a key below
    B's first and one above its last, the first and the last key of a directory bucket and a key of an empty bucket, for even k a
    palindrome present in B and one absent, a pair whose two partners both count 2^32 - 1, an entry with a == b, and a = 2^32 - 1 --
    the bucket, pair and palindrome plants wherever the key space has room for them (`roomy`)"""
    nkeys, top = 4 ** k, 4 ** k - 1
    ends = n_bg in (2, 65537)                                  # B holds key 0 and the largest key: both ends of B in one entry
    n_bg, n_fg = min(n_bg, nkeys), min(n_fg, nkeys)
    d = min(2 * k, 20)
    shift = 2 * k - d
    roomy = nkeys >= 4096 and n_bg >= 999
    table, plan = {}, {}
    if n_bg == 2:
        table = {0: 5, top: 7}
    elif n_bg:
        for x in sample_keys(rng, nkeys, n_bg).tolist():
            table[x] = int(rng.integers(1, 1000))
    if roomy:
        rc1 = lambda x: int(rc_keys(np.array([x], np.uint64), k)[0])   # noqa: E731
        j, j_empty = 3, 5
        first, last = j << shift, ((j + 1) << shift) - 1       # first and last key of directory bucket j
        banned = set() if ends else {0, 1, top, top - 1}       # without them a key below B's first and one above its last exist
        fixed = {first: 17, last: 19}
        if ends:
            fixed.update({0: 11, top: 13})
        plan["bucket"] = [first, last, (j_empty << shift) + (1 if shift else 0)]
        p = int(rng.integers(nkeys // 4, nkeys // 2))          # a pair with both partners at 2^32 - 1
        q = int(rng.integers(nkeys // 2, 3 * nkeys // 4))      # an entry with a == b, so a Nb == b Nf when Nf == Nb
        if len({p, rc1(p), q, rc1(q)} | set(fixed)) == 4 + len(fixed) and not any((x >> shift) == j_empty for x in (p, rc1(p), q, rc1(q))):
            fixed.update({p: U32MAX, rc1(p): U32MAX, q: 77})
            banned.add(rc1(q))
            plan["both_max"], plan["balanced"] = p, q
        if k % 2 == 0:
            pal_in, pal_out = palindrome(int(rng.integers(0, 2 ** k)), k), palindrome(int(rng.integers(0, 2 ** k)), k)
            if pal_in != pal_out and not ({pal_in, pal_out} & (set(fixed) | banned)) and (pal_in >> shift) != j_empty:
                fixed[pal_in] = 23                             # a palindrome present in B (expect 2 B[x]) and one absent
                banned.add(pal_out)
                plan["palindromes"] = [pal_in, pal_out]
        for x in [y for y in table if y in banned or (y >> shift) == j_empty]:
            del table[x]
        table.update(fixed)
        spare = [x for x in table if x not in fixed]
        while len(table) > n_bg and spare:
            del table[spare.pop()]
        if nkeys > 8 * n_bg:                                   # back to n_bg entries
            while len(table) < n_bg:
                x = int(rng.integers(0, nkeys))
                if x not in table and x not in banned and (x >> shift) != j_empty:
                    table[x] = int(rng.integers(1, 1000))
    bkeys = np.array(sorted(table), np.uint64)
    bcnt = np.array([table[x] for x in bkeys.tolist()], np.uint64)
    # foreground: the planted keys first, then keys of B, reverse complements of keys of B and random keys
    planted = [0, top]
    if len(bkeys):
        planted += [int(bkeys[0]), int(bkeys[-1])]
        if bkeys[0] > 0:
            planted.append(int(bkeys[0]) - 1)                  # below B's first
        if bkeys[-1] < top:
            planted.append(int(bkeys[-1]) + 1)                 # above B's last
    planted += plan.get("bucket", []) + plan.get("palindromes", [])
    planted += [plan[x] for x in ("both_max", "balanced") if x in plan]
    if n_fg < len(planted):
        r = (k + n_bg) % len(planted)
        planted = planted[r:] + planted[:r]
    pool = [np.array(planted, np.uint64)]
    if len(bkeys):
        some = bkeys[rng.permutation(len(bkeys))[:max(n_fg // 3, 1)]]
        pool += [some, rc_keys(some[: len(some) // 2 + 1], k)]
    pool.append(sample_keys(rng, nkeys, min(n_fg, nkeys)))
    allk = np.concatenate(pool)
    _, firsts = np.unique(allk, return_index=True)
    fkeys = allk[np.sort(firsts)][:n_fg]                       # distinct, the planted ones kept
    fkeys = fkeys[rng.permutation(len(fkeys))]                 # the foreground table is NOT ascending
    a = rng.integers(1, 1000, size=len(fkeys)).astype(np.uint64)
    for name, val in (("both_max", U32MAX), ("balanced", 77)):
        if name in plan:
            a[fkeys == np.uint64(plan[name])] = val
    free = np.nonzero(~np.isin(fkeys, np.array([plan.get("both_max", 0), plan.get("balanced", 0)], np.uint64)))[0]
    if len(free):
        a[free[int(rng.integers(0, len(free)))]] = U32MAX          # a = 2^32 - 1 on an ordinary entry
    return fkeys, a, bkeys, bcnt, plan


N_FG = [1, 63, 64, 65, 1000, 70001]
N_BG = [0, 1, 2, 999, 65537]


@pytest.mark.parametrize("revcom", [0, 1])
@pytest.mark.parametrize("k", [1, 4, 8, 10, 11, 15, 16, 17, 31])
def test_every_entry_against_exact_arithmetic(env, k, revcom):
    _ffi, DeviceCounts, DeviceEnrich = env
    rng = np.random.default_rng(1000 * k + revcom)
    dc_f, dc_b, en = DeviceCounts(), DeviceCounts(), DeviceEnrich()
    seen = {"negative": 0, "balanced": 0, "both_max": 0, "pal": 0, "a_max": 0}
    try:
        for n_bg in N_BG:
            for n_fg in N_FG:
                fkeys, a, bkeys, bcnt, plan = make_case(k, n_fg, n_bg, revcom, rng)
                if k == 16 and n_fg >= 63:
                    assert np.uint64(U32MAX) in fkeys          # the all-T 16-mer, 0xFFFFFFFF held as uint64
                load_table(dc_b, bkeys, bcnt, k)
                load_table(dc_f, fkeys, a, k)
                en.set_control(dc_b, revcom)
                ao = a.astype(object)
                bo = expected_b(fkeys, bkeys, bcnt, k, revcom)
                if "palindromes" in plan and revcom:
                    for pal, want in zip(plan["palindromes"], (2 * 23, 0)):
                        hit = np.nonzero(fkeys == np.uint64(pal))[0]
                        if len(hit):
                            assert bo[hit[0]] == want
                            seen["pal"] += 1
                if "both_max" in plan and revcom:
                    hit = np.nonzero(fkeys == np.uint64(plan["both_max"]))[0]
                    if len(hit):
                        assert bo[hit[0]] == 2 * U32MAX and ao[hit[0]] == U32MAX
                        seen["both_max"] += 1
                seen["a_max"] += int(np.any(a == U32MAX))
                sum_b = int(bcnt.astype(object).sum()) if len(bcnt) else 0
                own = (int(ao.sum()), 2 * sum_b if revcom else sum_b)       # Nb = 0 with an empty B
                for Nf, Nb in (own, (TMAX, TMAX)):
                    en.run(dc_f, Nf, Nb, 1)
                    b_got, z_got = en.result()
                    D = check_scores(b_got, z_got, ao, bo, Nf, Nb, f"k={k} revcom={revcom} n_fg={n_fg} n_bg={n_bg} Nf={Nf} Nb={Nb}")
                    if Nb == 0:
                        assert (z_got == 0).all() and not np.signbit(z_got).any()
                    seen["negative"] += int((z_got < 0).sum())
                    if Nf == Nb and "balanced" in plan and np.any(fkeys == np.uint64(plan["balanced"])):
                        i = int(np.nonzero(fkeys == np.uint64(plan["balanced"]))[0][0])
                        assert D[i] == 0 and z_got[i] == 0 and not np.signbit(z_got[i])
                        seen["balanced"] += 1
                    if Nf == TMAX and len(D):
                        assert max(abs(int(d)) for d in D[:64]) < 2 ** 85
        assert seen["negative"] > 0 and seen["a_max"] > 0
        if 4 ** k >= 4096:
            assert seen["balanced"] > 0 and (not revcom or seen["both_max"] > 0)
            assert k % 2 or not revcom or seen["pal"] > 0
    finally:
        for h in (en, dc_f, dc_b):
            h.close()


def test_totals_near_the_limit_reach_2_pow_84(env):
    """a = 2^32 - 1 against an empty control at Nf = Nb = 2^52 - 1: |D| = a Nb, just below 2^84, converted to double once"""
    _ffi, DeviceCounts, DeviceEnrich = env
    dc_f, dc_b, en = DeviceCounts(), DeviceCounts(), DeviceEnrich()
    try:
        load_table(dc_b, np.array([5], np.uint64), np.array([U32MAX], np.uint64), 12)
        load_table(dc_f, np.array([9, 5], np.uint64), np.array([U32MAX, 1], np.uint64), 12)
        en.set_control(dc_b, 0)
        en.run(dc_f, TMAX, TMAX, 1)
        b, z = en.result()
        a_o, b_o = np.array([U32MAX, 1], object), np.array([0, U32MAX], object)
        D = check_scores(b, z, a_o, b_o, TMAX, TMAX)
        assert D[0] == U32MAX * TMAX and D[0] > 2 ** 83 and D[1] == TMAX - U32MAX * TMAX and z[0] > 0 > z[1]
    finally:
        for h in (en, dc_f, dc_b):
            h.close()


# ---- 2. against the kernels that exist -----------------------------------------------------------------------------------------
def _reads_of(seq, borders):
    return [seq[s:e] for s, e in np.asarray(borders, np.int64).reshape(-1, 2)]


def _join(reads):
    parts, borders, at = [], [], 0
    for r in reads:
        parts += [r, np.array([255], np.uint8)]
        borders.append((at, at + len(r)))
        at += len(r) + 1
    return np.concatenate(parts) if parts else np.zeros(0, np.uint8), np.array(borders, np.int64).reshape(-1, 2)


def _revcom_read(r):
    return np.where(r[::-1] == 255, 255, 3 - r[::-1]).astype(np.uint8)


_TESTFA = {}


def _testfa_sets():
    """(foreground DeviceSeq, control: the same reads permuted, each reverse-complemented with probability 1/2, control without every
    third read), built once"""
    if not _TESTFA:
        from kmap_amd.kmer_count import encode_fasta
        from kmap_amd.motif_discovery import DeviceSeq
        seq, borders = encode_fasta(str(GOLD / "test.fa"))
        reads = _reads_of(seq, borders)
        rng = np.random.default_rng(2024)
        perm = rng.permutation(len(reads))
        flip = rng.random(len(reads)) < 0.5
        ctl = [_revcom_read(reads[i]) if f else reads[i] for i, f in zip(perm, flip)]
        _TESTFA["sets"] = (DeviceSeq(seq, borders), DeviceSeq(*_join(ctl)), DeviceSeq(*_join([r for i, r in enumerate(ctl) if i % 3 != 2])))
    return _TESTFA["sets"]


@pytest.mark.parametrize("dedupe", [True, False])
@pytest.mark.parametrize("k", [6, 9, 12, 14, 16, 17])
def test_against_the_counting_kernels(env, k, dedupe):
    _ffi, DeviceCounts, DeviceEnrich = env
    fg, same, thinned = _testfa_sets()
    dc_f, dc_b, dc_m, en = DeviceCounts(), DeviceCounts(), DeviceCounts(), DeviceEnrich()
    try:
        fg.count(dc_f, k, dedupe, True, use_work=False)
        uf, cf = dc_f.fetch()
        Nf = dc_f.total()
        assert len(uf) > 1000
        for ctl, identical in ((same, True), (thinned, False)):
            ctl.count(dc_m, k, dedupe, True, use_work=False)        # the control counted WITH the merge by the existing kernels
            um, cm = dc_m.fetch()
            Nb = dc_m.total()
            ctl.count(dc_b, k, dedupe, False, use_work=False)
            ub, _ = dc_b.fetch()
            assert (ub[1:] > ub[:-1]).all()                         # B ascends and is unique
            en.set_control(dc_b, 1)
            en.run(dc_f, Nf, Nb, 1)
            b, z = en.result()
            merged = dict(zip(um.tolist(), cm.tolist()))
            want = np.array([merged.get(x, 0) for x in uf.tolist()], np.uint64)
            np.testing.assert_array_equal(b, want)
            if identical:                                          # the same multiset of reads up to strand
                assert Nb == Nf
                np.testing.assert_array_equal(b, cf.astype(np.uint64))
                assert (z == 0).all() and not np.signbit(z).any()
            else:
                assert Nb < Nf and (b <= cf.astype(np.uint64)).all() and (b < cf.astype(np.uint64)).any()
                check_scores(b, z, cf.astype(object), want.astype(object), Nf, Nb, f"k={k} thinned")
                assert (z > 0).any()
    finally:
        for h in (en, dc_f, dc_b, dc_m):
            h.close()


# ---- 3. selection --------------------------------------------------------------------------------------------------------------
SEL_K = 12


def selection_input(kind, n, rng):
    """(a, b, extra top_n values, min_count values)"""
    if kind == "random":
        return rng.integers(1, 400, n), rng.integers(0, 400, n), [], [1]
    if kind == "mixed_signs":
        a = rng.integers(1, 50, n)
        return a, np.where(rng.random(n) < 0.5, a * 3, a // 3), [], [1]
    if kind == "one_tie_group":
        return np.full(n, 7), np.full(n, 3), [], [1]
    if kind == "two_tie_groups":
        high = rng.random(n) < 0.3
        return np.where(high, 9, 4), np.where(high, 1, 6), [int(high.sum()) + max((n - int(high.sum())) // 2, 1)], [1]
    assert kind == "min_count"
    a = rng.integers(2, 50, n)
    if n > 1:
        a[int(rng.integers(0, n))] = 1
    a[int(np.nonzero(a > 1)[0][0]) if (a > 1).any() else 0] = 100
    return a, rng.integers(0, 60, n), [], [101, 100, 2]           # 0, 1 and n - 1 eligible entries


@pytest.mark.parametrize("n", [1, 255, 256, 257, 100003])
@pytest.mark.parametrize("kind", ["random", "one_tie_group", "two_tie_groups", "mixed_signs", "min_count"])
def test_selection_against_lexsort(env, kind, n):
    _ffi, DeviceCounts, DeviceEnrich = env
    rng = np.random.default_rng(n + len(kind))
    a, b, extra, min_counts = selection_input(kind, n, rng)
    a, b = a.astype(np.uint64), b.astype(np.uint64)
    keys = sample_keys(rng, 4 ** SEL_K, n)
    order = rng.permutation(n)
    dc_f, dc_b, en = DeviceCounts(), DeviceCounts(), DeviceEnrich()
    try:
        load_table(dc_f, keys[order], a, SEL_K)                       # shuffled foreground; b travels through the control table
        inv = np.argsort(order)
        load_table(dc_b, keys, b[inv], SEL_K)
        en.set_control(dc_b, 0)
        Nf, Nb = int(a.sum()), max(int(b.sum()), 1)
        for min_count in min_counts:
            en.run(dc_f, Nf, Nb, min_count)
            b_got, z = en.result()
            np.testing.assert_array_equal(b_got, b)
            if kind == "mixed_signs" and n > 1:
                assert (z > 0).any() and (z < 0).any()
            elig = np.nonzero(a >= min_count)[0]
            if kind == "min_count" and n >= 255:
                assert len(elig) == {101: 0, 100: 1, 2: n - 1}[min_count]
            ranked = elig[np.lexsort((elig, -z[elig]))]
            for top_n in sorted({t for t in [1, 2, n - 1, n, n + 5] + extra if t >= 1}):
                m = en.select(top_n)
                assert m == min(top_n, len(elig)) and en.n_eligible == len(elig), (kind, n, top_n, min_count)
                got = en.fetch()
                idx, kh, a_s, b_s, z_s = got
                np.testing.assert_array_equal(idx, ranked[:m], err_msg=f"{kind} n={n} top_n={top_n} min_count={min_count}")
                np.testing.assert_array_equal(kh, keys[order][idx])
                np.testing.assert_array_equal(a_s, a[idx].astype(np.int64))
                np.testing.assert_array_equal(b_s, b[idx].astype(np.int64))
                assert z_s.tobytes() == z[idx].tobytes()
                assert en.select(top_n) == m
                again = en.fetch()
                assert all(x.tobytes() == y.tobytes() for x, y in zip(got, again))
            if kind == "two_tie_groups" and n >= 255:
                assert 0 < int((a == 9).sum()) < extra[0] < n         # the cut lies inside the second group
    finally:
        for h in (en, dc_f, dc_b):
            h.close()


# ---- 4. errors -----------------------------------------------------------------------------------------------------------------
def test_errors(env):
    _ffi, DeviceCounts, DeviceEnrich = env
    lib = _ffi.lib()
    dc_f, dc_b, dc_other, en = DeviceCounts(), DeviceCounts(), DeviceCounts(), DeviceEnrich()
    try:
        load_table(dc_f, np.array([3, 1], np.uint64), np.array([5, 6], np.uint64), 8)
        load_table(dc_b, np.array([1, 2], np.uint64), np.array([5, 6], np.uint64), 8)
        load_table(dc_other, np.array([1, 2], np.uint64), np.array([5, 6], np.uint64), 9)
        m, el = _ffi.i64(0), _ffi.i64(0)
        assert lib.kmap_enrich_run(en._h, dc_f._h, 11, 11, 1, None) == KMAP_E_STATE         # run before set_control
        assert "set_control" in _ffi.last_error()
        assert lib.kmap_enrich_select(en._h, 1, C.byref(m), C.byref(el), None) == KMAP_E_STATE
        assert lib.kmap_enrich_set_control(en._h, dc_b._h, 1, None) == 0
        assert lib.kmap_enrich_run(en._h, dc_other._h, 11, 11, 1, None) == KMAP_E_INVAL     # different k
        assert lib.kmap_enrich_run(en._h, dc_f._h, 11, 11, 0, None) == KMAP_E_INVAL         # min_count < 1
        assert lib.kmap_enrich_run(en._h, dc_f._h, 2 ** 52, 11, 1, None) == KMAP_E_UNSUP    # a total of 2^52
        assert lib.kmap_enrich_run(en._h, dc_f._h, 11, 2 ** 52, 1, None) == KMAP_E_UNSUP
        assert lib.kmap_enrich_run(en._h, dc_f._h, TMAX, TMAX, 1, None) == 0
        assert lib.kmap_enrich_fetch(en._h, None, None, None, None, None) == KMAP_E_STATE   # fetch before select
        assert lib.kmap_enrich_select(en._h, 0, C.byref(m), C.byref(el), None) == KMAP_E_INVAL
        assert lib.kmap_enrich_select(en._h, 5, C.byref(m), C.byref(el), None) == 0 and m.value == 2 and el.value == 2
        assert lib.kmap_enrich_fetch(en._h, None, None, None, None, None) == 0
        load_table(dc_f, np.array([3, 1, 2], np.uint64), np.array([5, 6, 7], np.uint64), 8)   # the foreground changed under the handle
        assert lib.kmap_enrich_select(en._h, 5, C.byref(m), C.byref(el), None) == KMAP_E_STATE
    finally:
        for h in (en, dc_f, dc_b, dc_other):
            h.close()


# ---- 5. the verb end to end ----------------------------------------------------------------------------------------------------
MOTIF = "ATCGGATT"


def verb_reads():
    """the issue's recipe: draw order foreground codes, control codes, mask, positions"""
    rng = np.random.default_rng(11)
    fg = rng.integers(0, 4, size=(2000, 60)).astype(np.uint8)
    ctl = rng.integers(0, 4, size=(2000, 60)).astype(np.uint8)
    mask = rng.random(2000) < 0.3
    pos = rng.integers(0, 53, size=int(mask.sum()))
    codes = np.array(["ACGT".index(c) for c in MOTIF], np.uint8)
    for r, p in zip(np.nonzero(mask)[0], pos):
        fg[r, p:p + 8] = codes
    return fg, ctl


def restate_counts(reads, k):
    """per-read de-duplicated k-mer counts: (unmerged {key: count}, merged {lower key: count}, palindromes doubled)"""
    w = 4 ** np.arange(k - 1, -1, -1, dtype=np.int64)
    keys = sliding_window_view(reads.astype(np.int64), k, axis=1) @ w
    per_read = np.concatenate([np.unique(row) for row in keys])
    u, c = np.unique(per_read, return_counts=True)
    plain = dict(zip(u.tolist(), c.tolist()))
    merged = {}
    for x, rx in zip(u.tolist(), rc_keys(u.astype(np.uint64), k).tolist()):
        merged[min(x, rx)] = plain[x] + plain.get(rx, 0)
    return plain, merged


def write_fasta(path, reads):
    lut = np.frombuffer(b"ACGT", np.uint8)
    with open(path, "w") as fh:
        for i, r in enumerate(reads):
            fh.write(f">r{i}\n{lut[r].tobytes().decode()}\n")


def ball_mass(merged, cons, k, radius):
    keys = np.array(list(merged), np.uint64)
    cnt = np.array(list(merged.values()), np.int64)

    def dist(c):
        x = keys ^ np.uint64(c)
        return sum(((x >> np.uint64(2 * j)) & np.uint64(3)) != 0 for j in range(k))
    rc = int(rc_keys(np.array([cons], np.uint64), k)[0])
    return int(cnt[np.minimum(dist(cons), dist(rc)) <= radius].sum())


def test_verb_end_to_end(tmp_path):
    from click.testing import CliRunner
    from kmap_amd.cli import cli
    from kmap_amd.enrichment import enrich_z
    from kmap_amd.kmer_count import _preproc, gen_motif_def_dict, kmer2hash, read_default_config_file
    fg, ctl = verb_reads()
    write_fasta(tmp_path / "fg.fa", fg)
    write_fasta(tmp_path / "ctl.fa", ctl)
    res = tmp_path / "res"
    _preproc(str(tmp_path / "fg.fa"), str(res))
    long_one = "ACGT" * 10
    (res / "final_conseq.txt").write_text(f"{MOTIF}\n{long_one}\n")
    r = CliRunner().invoke(cli, ["enrich_kmers", "--res_dir", str(res), "--control_fasta_file", str(tmp_path / "ctl.fa"), "--kmer_len", "8",
                                 "--top_n", "50", "--min_count", "2"], catch_exceptions=False)
    assert r.exit_code == 0, r.output
    plain_f, merged_f = restate_counts(fg, 8)
    plain_b, merged_b = restate_counts(ctl, 8)
    Nf, Nb = sum(merged_f.values()), sum(merged_b.values())
    assert (Nf, Nb, len(merged_f), len(plain_b)) == (106335, 106407, 31323, 52591)      # the figures of the CPU run of this recipe
    out = res / "kmer_enrichment"
    rows = [ln.split("\t") for ln in (out / "enriched_kmers_k8.tsv").read_text().splitlines()]
    assert rows[0] == "rank kmer revcom_kmer fg_count control_count fg_share control_share log2_fold z".split() and len(rows) == 51
    # row 1: the planted motif under its lower strand, key 3427 = AATCCGAT = rc(ATCGGATT)
    key = 3427
    assert int(kmer2hash(MOTIF)) == 13967 and int(rc_keys(np.array([13967], np.uint64), 8)[0]) == key
    assert rows[1][:5] == ["1", "AATCCGAT", MOTIF, "579", "4"]
    assert abs(float(rows[1][8]) - 23.85) < 0.005 and abs(float(rows[2][8]) - 12.19) < 0.005
    zs = []
    for rank, row in enumerate(rows[1:], 1):
        x = int(kmer2hash(row[1]))
        a, b = merged_f[x], merged_b.get(x, 0)
        assert int(row[0]) == rank and (int(row[3]), int(row[4])) == (a, b) and a >= 2
        want = enrich_z(a, b, Nf, Nb)
        assert abs(float(row[8]) - want) <= 1e-5 * abs(want) + 1e-12
        zs.append(want)
    assert all(x >= y for x, y in zip(zs, zs[1:]))
    best = sorted((enrich_z(a, merged_b.get(x, 0), Nf, Nb) for x, a in merged_f.items() if a >= 2), reverse=True)
    np.testing.assert_allclose(zs, best[:50], rtol=1e-12)
    info = (out / "enrichment_info.csv").read_text().splitlines()
    n_elig = sum(1 for a in merged_f.values() if a >= 2)
    assert info[1] == f"8,1,1,31323,52591,106335,106407,2,{n_elig},50"
    # the motif table: ball masses over both merged tables, an unknown length listed with empty fields
    d = gen_motif_def_dict(read_default_config_file())[8]
    motif = (out / "motif_enrichment.csv").read_text().splitlines()
    f = motif[1].split(",")
    ma, mb = ball_mass(merged_f, 13967, 8, d.max_ham_dist), ball_mass(merged_b, 13967, 8, d.max_ham_dist)
    assert f[:7] == [MOTIF, "8", str(d.max_ham_dist), str(ma), str(mb), "106335", "106407"] and ma > mb
    assert abs(float(f[12]) - enrich_z(ma, mb, Nf, Nb)) <= 1e-5 * abs(enrich_z(ma, mb, Nf, Nb))
    assert motif[2] == f"{long_one},40" + "," * 11 and len(motif) == 3
    assert "no row in the motif definition table" in r.output
