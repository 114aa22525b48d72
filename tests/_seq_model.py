"""Host model of the reference's SEQ force arithmetic (taichi_core.py:252-270, 305-326 with T of visualization.py:131-145), in
plain numpy float32 and for a SUBSET of rows: the yardstick tests/test_gpu_seq_forms.py holds every form of the SEQ force kernel to,
row by row.  No project code: tests/test_seq_model_host.py ties it to the oracle bit for bit.

    dx = x[i] - x[j], dy likewise, d2 = dx*dx + dy*dy          every product and sum rounded on its own
    q  = clip(1 / (1 + d2), 1e-3, 1 - 1e-3)
    T  = (q / (1 - q)) * (p - q);  g[i] = sum over j != i, j ascending, of T*dx (T*dy)

np.cumsum in float32 is a strictly sequential, index-ascending sum.  The skipped diagonal is added as +0.0, which changes no bit:
an accumulator that starts at +0.0 never becomes -0.0 under round-to-nearest.
"""
import numpy as np

F = np.float32
Q_LO, Q_HI = F(1e-3), F(1 - 1e-3)
_CHUNK = 64            # rows evaluated at once (64 x 60 000 floats per temporary)


def p_rows_lut(lut, sums, rows, n, rowmap=None):
    """probabilities of the session rows `rows` (local indices) from u16 sums + LUT: lut[sums[rowmap[rows]]]"""
    rows = np.asarray(rows, np.int64)
    stored = rows if rowmap is None else np.asarray(rowmap, np.int64)[rows]
    return np.asarray(lut, F)[sums[stored, :n]]


def _q_block(ld, rows):
    x, y = ld[0].astype(F, copy=False), ld[1].astype(F, copy=False)
    dx = x[rows, None] - x[None, :]
    dy = y[rows, None] - y[None, :]
    d2 = dx * dx + dy * dy
    with np.errstate(over="ignore"):
        q = F(1) / (F(1) + d2)
    q = np.maximum(np.minimum(q, Q_HI), Q_LO)
    assert dx.dtype == F and q.dtype == F
    return dx, dy, q


def q_rows(ld, rows):
    """rows of the low-dimensional probability matrix (cal_ld_prob_mat; a diagonal entry is 1 clipped to 1 - 1e-3)"""
    rows = np.asarray(rows, np.int64)
    if len(rows) == 0:
        return np.zeros((0, ld.shape[1]), F)
    return np.concatenate([_q_block(ld, rows[a:a + _CHUNK])[2] for a in range(0, len(rows), _CHUNK)])


def grad_rows(ld, rows, p_rows):
    """-> float32 [2, len(rows)]: the SEQ gradient (gradient_loss / 4) of the global rows `rows`; p_rows[k] = probabilities of
    row rows[k] against all n columns (float32)"""
    rows = np.asarray(rows, np.int64)
    n = ld.shape[1]
    assert p_rows.dtype == F and p_rows.shape == (len(rows), n)
    g = np.zeros((2, len(rows)), F)
    for a in range(0, len(rows), _CHUNK):
        r = rows[a:a + _CHUNK]
        dx, dy, q = _q_block(ld, r)
        with np.errstate(over="ignore", invalid="ignore"):
            t = (q / (F(1) - q)) * (p_rows[a:a + _CHUNK] - q)
            tx, ty = t * dx, t * dy
        k = np.arange(len(r))
        tx[k, r] = 0.0
        ty[k, r] = 0.0
        with np.errstate(over="ignore", invalid="ignore"):
            g[0, a:a + _CHUNK] = np.cumsum(tx, axis=1, dtype=F)[:, -1]
            g[1, a:a + _CHUNK] = np.cumsum(ty, axis=1, dtype=F)[:, -1]
    return g


def loss_rows(ld, rows, p_rows):
    """sum over i in rows, i < j < n, of -(p ln q + (1 - p) ln(1 - q)) in float64 from the float32 q, 1 - q and p: the partial
    kmap_embed_forces hands out (no eps branches; the reference's factor 2 is applied by the iteration's apply step)"""
    rows = np.asarray(rows, np.int64)
    n = ld.shape[1]
    total = 0.0
    for a in range(0, len(rows), _CHUNK):
        r = rows[a:a + _CHUNK]
        q = _q_block(ld, r)[2]
        p = p_rows[a:a + _CHUNK].astype(np.float64)
        ce = -(p * np.log(q.astype(np.float64)) + (1.0 - p) * np.log((F(1) - q).astype(np.float64)))
        ce[np.arange(n)[None, :] <= r[:, None]] = 0.0
        total += float(ce.sum())
    return total


def clustered(n, seed):
    """2 x n float32 coordinates with every kind of batch the kernels tell apart: point j belongs to cluster (j // 200) % 7, the
    centres lie on a circle of radius 100 (pairs of different clusters are far: d2 >= 1000), unit normal noise; a coincident
    pair (4, 5); a pair 1e-4 apart (16, 17); three points of magnitude 1e16 (squared distances beyond 1e30: generic division).
    A term against such a point is ~1e13 and would absorb every other term of the row sum -- unless its probability is the clipped
    q = 1e-3 itself, which makes the term a signed zero: give the columns `huge_points` that probability (the batch still takes the
    generic division, for all its columns)"""
    rng = np.random.default_rng(seed)
    c = (np.arange(n) // 200) % 7
    ang = 2 * np.pi * c / 7
    ld = (np.stack([100 * np.cos(ang), 100 * np.sin(ang)]) + rng.standard_normal((2, n))).astype(F)
    if n > 5:
        ld[:, 5] = ld[:, 4]
    if n > 17:
        ld[:, 17] = ld[:, 16] + F(1e-4)
    if n >= 64:
        for j, (sx, sy) in zip((n // 3 + 1, n // 2 + 3, n - 7), ((1, 1), (-1, 0.5), (0.25, -1))):
            ld[:, j] = (F(sx * 1e16), F(sy * 1e16))
    return ld


def huge_points(ld):
    """columns whose coordinates exceed 1e15 (see `clustered`)"""
    return np.nonzero(np.abs(ld).max(axis=0) >= 1e15)[0]


def uniform(n, seed, scale):
    """standard normal coordinates times `scale`, with the coincident and the 1e-4-apart pair of `clustered`"""
    ld = (np.random.default_rng(seed).standard_normal((2, n)) * scale).astype(F)
    if n > 5:
        ld[:, 5] = ld[:, 4]
    if n > 17:
        ld[:, 17] = ld[:, 16] + F(1e-4 * scale)
    return ld


def far_share(ld, rows_per_wave, cols_per_batch):
    """share of the tiles (rows_per_wave consecutive rows x cols_per_batch consecutive columns, both from 0) whose pairs ALL have
    d2 >= 1000: the tiles a wave evaluates as `far`"""
    n = ld.shape[1]
    cuts = np.arange(0, n, cols_per_batch)
    mins = []
    for a in range(0, n, rows_per_wave * 64):
        rows = np.arange(a, min(n, a + rows_per_wave * 64))
        x, y = ld[0], ld[1]
        dx, dy = x[rows, None] - x[None, :], y[rows, None] - y[None, :]
        with np.errstate(over="ignore"):
            d2 = dx * dx + dy * dy
        m = np.minimum.reduceat(d2, cuts, axis=1)
        mins.append(np.minimum.reduceat(m, np.arange(0, len(rows), rows_per_wave), axis=0))
    mins = np.concatenate(mins)
    return float((mins >= 1000).mean())
