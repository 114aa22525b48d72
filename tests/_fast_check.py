"""Per-element check of the FAST force kernels (kmap_amd/csrc/embed_fast.hip) against the float64 oracle.

For every checked coordinate c of row i:   |g_dev - g64| <= kappa * u * M + FLOOR,   u = 2^-24,
with g64 = sum_{j != i} t (y_i - y_j)_c in float64 and M = sum_j |q / (1 - q)| (|p| + q) |y_i - y_j|_c
(oracle.embed_forces_rows_f64).  M has no cancellation, so the bound is what a summation of that many terms
can lose, whatever the sign pattern of the terms.

kappa, per kernel family: the worst case follows from the summation structure (kappa_worst below); the constant used
is about 4x the largest err / (u M) observed on an MI355X over every shape and input of tests/test_gpu_fast_forces.py
and the full-size checks, capped by that worst case (kappa()).  Planted pairs (Planted) show that the check has power: each
planted term |t (y_i - y_j)_c| is at least POWER x the bound at both of its rows, so losing, doubling or negating one
pair cannot pass.
"""
import math

import numpy as np

U = 2.0 ** -24
FLOOR = 1e-30     # below every nonzero |term| the kernels can produce; keeps exact zeros (M = 0) comparable
POWER = 100.0     # planted term / bound at both rows of the pair

# Per pair, all families: dx, dy and dy^2 round once each, the FMA of d2 once -> d2 within 4u; the clamp to
# [1/999, 999] keeps relative errors; 1 + d2, d2 (1 + d2), v_rcp_f32 (1 ulp) and the multiplies for q and q/(1-q)
# add one u each -> q and q/(1-q) within ~8u, p - q within u |p - q| + 8u q, times dx one more u:
# a pair's term is within ~12u of |q/(1-q)| (|p| + q) |dx|, the summand of M.
KAPPA_PAIR = 12
# Worst case of the sums (Higham: a sum of depth D is within D u sum|terms|):
#   rows   (forces_fast_kernel): a lane chains F_CPL = 8 FMAs per 512-column step, ceil(n / 512) steps, then 6 shuffle levels.
#   sym    (forces_sym2_kernel + sym_reduce_kernel): per tile the row side is <= 8 FMAs + 6 DPP / transpose levels, the column
#          side 64 FMAs (a wave's rows) + 3 LDS adds (4 waves); sym_reduce_kernel's lane adds ceil(nJ / 8) row partials and
#          ceil(nI / 8) column partials in one chain, then 3 butterfly levels.
#   cyclic: the sym depth of a shard plus the f32 sum of the world messages (world - 1 adds).
# Measured on an MI355X (largest err / (u M) over tests/test_gpu_fast_forces.py and the C3 / C4 full-size checks): rows 6.6
# (n = 16 383 and n = 1000 at scale 30: 6.4), sym 6.7 (C4, N = 200 000, planted), cyclic 4.4 (n = 17 229, world 2 .. 8).
# Round-off of sums this long grows like sqrt(depth), not like depth: the constants are ~4x the maxima, and kappa() never
# exceeds the worst case.
KAPPA_ROWS = 28.0
KAPPA_SYM = 28.0
KAPPA_CYCLIC = 18.0
# the f32 oracle (kb_embed_forces_rows, the reference's arithmetic): a sequential sum of n - 1 terms, and per pair the f32
# 1 - q, whose rounding is amplified by q / (1 - q) <= 999 -> up to ~1000 u of the pair's summand
KAPPA_REF32_PAIR = 1010


def kappa_worst(family, n, world=1):
    """the worst-case kappa of a family at size n (see above); the constants in use must stay below it"""
    if family == "rows":
        return KAPPA_PAIR + 8 * math.ceil(n / 512) + 6
    nJ, nI = math.ceil(n / 512), math.ceil(n / 256)
    d = KAPPA_PAIR + 64 + 3 + math.ceil(nJ / 8) + math.ceil(math.ceil(nI / world) / 8) + 3
    if family == "sym":
        return d
    if family == "cyclic":
        return d + world - 1
    if family == "ref32":
        return KAPPA_REF32_PAIR + n
    raise ValueError(family)


def kappa(family, n, world=1):
    """kappa of a family at size n: the measured constant, capped by the worst case"""
    const = {"rows": KAPPA_ROWS, "sym": KAPPA_SYM, "cyclic": KAPPA_CYCLIC}[family]
    return min(const, float(kappa_worst(family, n, world)))


def ratio(g_dev, g64, M):
    """err / (u M) per element (0 where M = 0 and the values agree)"""
    err = np.abs(np.asarray(g_dev, np.float64) - g64)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(M > 0, err / (U * M), np.where(err > FLOOR, np.inf, 0.0))
    return r


def failing_rows(g_dev, g64, M, kappa):
    """indices (into the checked rows) where some coordinate exceeds the bound"""
    err = np.abs(np.asarray(g_dev, np.float64) - g64)
    return np.nonzero((err > kappa * U * M + FLOOR).any(axis=0))[0]


def assert_forces_close(g_dev, g64, M, kappa, rows, what=""):
    """the per-element bound on every checked row; returns the largest err / (u M) seen"""
    g_dev = np.asarray(g_dev)
    assert g_dev.shape == g64.shape == M.shape == (2, len(rows))
    assert np.all(np.isfinite(g_dev)), f"{what}: non-finite gradient"
    bad = failing_rows(g_dev, g64, M, kappa)
    r = ratio(g_dev, g64, M)
    assert len(bad) == 0, (f"{what}: {len(bad)} rows beyond {kappa} u M, first rows {np.asarray(rows)[bad][:8].tolist()}: "
                           f"got {g_dev[:, bad[:3]].tolist()} want {g64[:, bad[:3]].tolist()} err/(u M) {r[:, bad[:3]].tolist()}")
    return float(r.max()) if r.size else 0.0


# ---- planted pairs ------------------------------------------------------------------------------------------------------------
BG_P = (0.0, 0.0, 0.0, 0.0, 1e-11, 1e-6, 1e-5, 1e-4)   # background probabilities: sums (a_i + a_j) % 8; 0 and 1e-11 take the eps branch
PL_P = (0.25, 0.0, 1.0, 0.6)                             # planted pairs' probabilities (LUT codes 8 ..)
PL_D2 = (0.25, 0.01, 1.0, 0.1, 0.5, 0.04)                # planted pairs' squared distances
SPACING = 64.0                                           # background grid: every non-partner pair has d >= 32, d2 >= 999


def select_pairs(n, candidates):
    """the candidates (i, j) that exist at size n, greedily made disjoint (each point in at most one pair), i < j"""
    used, out = set(), []
    for i, j in candidates:
        i, j = (i + n if i < 0 else i), (j + n if j < 0 else j)
        i, j = min(i, j), max(i, j)
        if 0 <= i < j < n and i not in used and j not in used:
            used |= {i, j}
            out.append((i, j))
    return out


def structural_pairs(n, extra=()):
    """planted positions where the kernels' structure can drop or double a pair (embed_fast.hip)"""
    c = list(extra)
    c += [(255, 256), (511, 512), (1023, 1024), (63, 64), (64, 65)]          # j = i + 1 across row-block / column-tile edges
    c += [(600, 601), (700, 1022), (1030, 1031), (1100, 1535)]              # first and last j > i of diagonal tiles
    c += [(100, n - 1), (n - 3, n - 2), (0, n - 4)]                          # right-edge tile, ragged bottom block (i = n - 1)
    c += [(3000, 9000), (5000, 15000), (40, 16000), (2000, 16383)]          # interior tiles
    for b in range(9):                                                       # rows of every rank of a cyclic split (world <= 8)
        c += [(256 * b + 10, 256 * b + 11), (256 * b + 130, 256 * (b + 17) + 200)]
    c += [(n // 2, n // 2 + 1), (n - 520, n - 7)]
    return select_pairs(n, c)


class Planted:
    """n points on a grid of spacing SPACING (every background pair clamped at d2 >= 999), the partner j of each pair
    (i, j) moved next to i (d2 from PL_D2, both coordinates nonzero).  Sums: (a_i + a_j) % 8 in the background, codes 8 ..
    for the planted pairs; the LUT maps them to BG_P / PL_P.  `coords` may be replaced (natural inputs) -- the sums stay."""

    def __init__(self, n, pairs, seed=0):
        rng = np.random.default_rng(seed)
        self.n, self.pairs = n, list(pairs)
        side = max(1, math.ceil(math.sqrt(n)))
        k = np.arange(n)
        y = np.stack([SPACING * (k % side), SPACING * (k // side)]).astype(np.float64)
        self.code = {}
        for t, (i, j) in enumerate(self.pairs):
            d = math.sqrt(PL_D2[t % len(PL_D2)] / 2.0)
            s = rng.choice([-1.0, 1.0], size=2)
            y[:, j] = y[:, i] + d * s
            self.code[(i, j)] = len(BG_P) + t % len(PL_P)
        self.coords = y.astype(np.float32)
        self.a = rng.integers(0, len(BG_P), size=n).astype(np.int64)
        self.lut = np.array(BG_P + PL_P, np.float32)
        self._pi = np.array([p[0] for p in self.pairs], np.int64)
        self._pj = np.array([p[1] for p in self.pairs], np.int64)
        self._pc = np.array([self.code[p] for p in self.pairs], np.int64)

    def sums_rows(self, rows):
        rows = np.asarray(rows, np.int64)
        S = ((self.a[rows, None] + self.a[None, :]) % len(BG_P)).astype(np.uint16)
        pos = {int(r): t for t, r in enumerate(rows)}
        for i, j, c in zip(self._pi, self._pj, self._pc):
            if int(i) in pos:
                S[pos[int(i)], j] = c
            if int(j) in pos:
                S[pos[int(j)], i] = c
        return S

    def p_rows(self, rows):
        return self.lut[self.sums_rows(rows)]

    def planted_rows(self):
        return np.unique(np.concatenate([self._pi, self._pj])) if self.pairs else np.zeros(0, np.int64)

    def pair_terms(self):
        """t (y_i - y_j)_c of every planted pair in float64 (row i's term; row j's is its negative): [n_pairs, 2]"""
        return pair_terms(self.coords, self.pairs, self.lut[self._pc])

    def pair_ce(self):
        y = self.coords.astype(np.float64)
        d = y[:, self._pi] - y[:, self._pj]
        q = np.clip(1.0 / (1.0 + (d * d).sum(0)), 1e-3, 1 - 1e-3)
        p = self.lut[self._pc].astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(p < 1e-10, -np.log(1 - q), -p * np.log(q) - (1 - p) * np.log(1 - q))

    def assert_visible(self, rows, M, kappa, power=POWER):
        """every planted term is >= power x the bound at both of its rows; returns the smallest term / bound"""
        return assert_pairs_visible(self.pairs, self.pair_terms(), rows, M, kappa, power)


def pair_terms(coords, pairs, p):
    """t (y_i - y_j)_c in float64 of pairs (i, j) with probabilities p: [n_pairs, 2] (row i's term; row j's is its negative)"""
    y = np.asarray(coords, np.float64)
    pi, pj = np.array([a for a, _ in pairs]), np.array([b for _, b in pairs])
    d = y[:, pi] - y[:, pj]
    q = np.clip(1.0 / (1.0 + (d * d).sum(0)), 1e-3, 1 - 1e-3)
    return ((q / (1 - q) * (np.asarray(p, np.float64) - q)) * d).T


def assert_pairs_visible(pairs, terms, rows, M, kappa, power=POWER):
    """|term| >= power x the bound at both rows of every pair; returns the smallest |term| / bound"""
    pos = {int(r): t for t, r in enumerate(rows)}
    worst = np.inf
    for (i, j), tm in zip(pairs, np.abs(terms)):
        for r in (i, j):
            assert r in pos, f"planted row {r} not checked"
            worst = min(worst, float((tm / (kappa * U * M[:, pos[r]] + FLOOR)).min()))
    assert worst >= power, f"a planted pair stands only {worst:.1f} x above the bound"
    return worst


def plant_far(coords, pairs, d2=1.0 / 1998, x0=200.0):
    """natural coordinates with the pairs moved out of the cloud: pair k at (x0 + 64 k, x0) and (x0 + 64 k, x0) + (d, d),
    d2 = 2 d^2 (default inside the q clip); every other pair of those rows is far (d2 >= 999)"""
    y = np.array(coords, np.float32, copy=True)
    d = np.sqrt(d2 / 2)
    for k, (i, j) in enumerate(pairs):
        y[:, i] = (x0 + 64 * k, x0)
        y[:, j] = (x0 + 64 * k + d, x0 + d)
    return y


def check_rows(n, rows_extra=(), rng_rows=64, seed=1, planted=None):
    """rows to check at size n: every row up to 1024, else edges of blocks / tiles, the planted rows and a random fill"""
    if n <= 1024:
        return np.arange(n, dtype=np.int64)
    rng = np.random.default_rng(seed)
    e = [0, 1, 62, 63, 64, 65, 127, 128, 254, 255, 256, 257, 510, 511, 512, 513, 1023, 1024, n // 2, n - 257, n - 256,
         n - 255, n - 65, n - 64, n - 2, n - 1]
    e += [(n // 256) * 256 - 1, (n // 256) * 256, (n // 512) * 512 - 1, (n // 512) * 512]
    rows = set(r for r in e if 0 <= r < n) | set(int(r) for r in rows_extra if 0 <= r < n)
    rows |= set(rng.integers(0, n, rng_rows).tolist())
    if planted is not None:
        rows |= set(planted.planted_rows().tolist())
    return np.array(sorted(rows), np.int64)


def reference(P_or_planted, rows, coords):
    """(g64, M, loss) of the rows: P_or_planted is a Planted or a callable rows -> f32 probability slab"""
    from oracle import oracle as O
    p_rows = P_or_planted.p_rows if isinstance(P_or_planted, Planted) else P_or_planted
    return O.embed_forces_rows_f64(p_rows(rows), rows, coords)


def total_loss64(p_rows, n, coords, chunk=1024):
    """sum_{i<j} CE in float64 over all rows (chunks of rows: no n x n matrix on the host)"""
    from oracle import oracle as O
    s = 0.0
    for r0 in range(0, n, chunk):
        rows = np.arange(r0, min(n, r0 + chunk), dtype=np.int64)
        s += float(O.embed_forces_rows_f64(p_rows(rows), rows, coords)[2].sum())
    return s
