"""Host model of the record one iteration of the reference's embedding loop keeps (reference visualization.py:293-317 and
add_jitter, :179-196), restated from the rule in numpy f32 scalars, plus the scripts that drive it and the device side by side
(tests/test_loop_model_host.py, tests/test_gpu_loop_record.py).  No test lives here.

The loop, per iteration, given the loss of the current iterate and its gradient:

    loss = f32(2 * total)                               np.sum(ce) * 2
    if loss < best[-1].loss:                            false for NaN
        best[-1] <- (loss, copy of the iterate); best = best[:-1]; bisect.insort_right(best, entry, key=loss)
    if |prev - loss| < f32(1e-7) * |loss|: stop         the loss is logged and counted, the insert done; no update, no jitter
    prev = loss
    y += -(f32(4) * g_raw) * f32(lr)                    three roundings
    add_jitter(y, 0.1)

add_jitter walks the 2 x N array as N x 2, so its two passes see the two-element columns (x_0, y_0) and (x_1, y_1) and nothing
else: per column the stable order of the two, their f32 difference, and if that is < f32(0.1) the smaller element becomes
f32(f64(v) + normal) with the next draw of np.random.normal(0, 0.01); column 0 before column 1.

ONE rule here is the project's own, not the reference's: the draws are handed over as a pool, and once `jitter_used` has reached
the pool's length a due draw adds 0.0 and the count still advances (the product refills the pool before that can happen).
The cap of the loss log (`log_cap`, 65 536 entries; iterations beyond it are counted but not logged) is the project's as well.
"""
import bisect
from fractions import Fraction

import numpy as np

F32 = np.float32
MSG_EXTRA = 8
LOG_CAP = 1 << 16
TWO48 = 1 << 48
M48 = TWO48 - 1
STOP_FLIP = 1611392          # mantissa field of the loss at which prev = loss +- 1 ulp does not stop yet; + 1: it stops


class LoopModel:
    def __init__(self, n, n_best, lr, coords_2xn, placeholders=None, normals=(), log_cap=LOG_CAP):
        self.n, self.n_best, self.lr, self.log_cap = int(n), int(n_best), F32(lr), int(log_cap)
        self.coords = np.array(coords_2xn, np.float32).reshape(2, self.n).copy()
        ph = np.zeros((self.n_best, 2, self.n), np.float32) if placeholders is None else np.asarray(placeholders, np.float32)
        assert ph.shape == (self.n_best, 2, self.n)
        # [loss, snapshot, iteration that produced it (-1: a placeholder)]
        self.best = [[F32(np.inf), ph[b].copy(), -1] for b in range(self.n_best)]
        self.normals = np.array(normals, np.float64).reshape(-1)
        self.iters, self.stopped, self.jitter_used = 0, False, 0
        self.prev_loss = F32(np.inf)
        self.last_loss = F32(np.inf)
        self.log = []

    def set_jitter(self, normals):
        """a new pool; the running count keeps indexing into it"""
        self.normals = np.array(normals, np.float64).reshape(-1)

    def apply(self, g_raw_2xn, loss_total_f64):
        if self.stopped:
            return
        g_raw = np.asarray(g_raw_2xn, np.float32).reshape(2, self.n)
        with np.errstate(all="ignore"):
            loss = F32(2.0 * float(loss_total_f64))
            if self.iters < self.log_cap:
                self.log.append(loss)
            self.iters += 1
            self.last_loss = loss
            if loss < self.best[-1][0]:
                entry = self.best[-1]
                entry[0], entry[1], entry[2] = loss, self.coords.copy(), self.iters - 1
                self.best = self.best[:-1]
                bisect.insort_right(self.best, entry, key=lambda b: b[0])
            if abs(self.prev_loss - loss) < F32(1e-7) * abs(loss):
                self.stopped = True
                return
            self.prev_loss = loss
            g = F32(4) * g_raw
            self.coords = self.coords + (-g * self.lr)
            assert self.coords.dtype == np.float32
            for p in (0, 1):
                if p >= self.n:
                    break
                pair = self.coords[:, p]
                idx = np.argsort(pair, kind="stable")
                diff = pair[idx[1]] - pair[idx[0]]
                if diff < F32(0.1):
                    nrm = self.normals[self.jitter_used] if self.jitter_used < len(self.normals) else 0.0
                    self.jitter_used += 1
                    self.coords[idx[0], p] = F32(np.float64(pair[idx[0]]) + np.float64(nrm))

    def apply_msg(self, msg):
        """msg: the summed message [gradient 2 N | six loss limbs, flag, pad]"""
        from kmap_amd.distributed import loss_from_limbs
        msg = np.asarray(msg, np.float32)
        assert msg.shape == (2 * self.n + MSG_EXTRA,)
        self.apply(msg[:2 * self.n].reshape(2, self.n), loss_from_limbs(msg[2 * self.n:]))

    # ---- what the session's getters return ----
    def best_losses(self):
        return np.array([b[0] for b in self.best], np.float32)

    def best_snaps(self):
        return np.stack([b[1] for b in self.best])

    def best_iters(self):
        return [b[2] for b in self.best]


# ---- f32 values by their bits ----------------------------------------------------------------------------------------------------
def f32_from_fields(binade, mantissa):
    """the positive normal f32 2^binade * (1 + mantissa / 2^23)"""
    assert -126 <= binade <= 127 and 0 <= mantissa < (1 << 23)
    return np.array([((binade + 127) << 23) | mantissa], np.uint32).view(np.float32)[0]


def ulps(x, k):
    """the f32 k ulps above (k < 0: below) the positive f32 x"""
    b = int(np.array([x], np.float32).view(np.uint32)[0]) + k
    assert 0 < b < 0x7F800000
    return np.array([b], np.uint32).view(np.float32)[0]


def total_of(loss_f32):
    """the f64 total that makes the loop see exactly this f32 loss (loss = f32(2 * total))"""
    return float(loss_f32) / 2


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def stop_pairs(binade):
    """(name, prev, loss) around the stop rule in one binade; the model decides what each does"""
    out = []
    for m in (STOP_FLIP, STOP_FLIP + 1):
        loss = f32_from_fields(binade, m)
        for k in (-2, -1, 1, 2):
            out.append((f"m{m}{k:+d}ulp", ulps(loss, k), loss))
    loss = f32_from_fields(binade, STOP_FLIP + 1)
    out.append(("equal", loss, loss))
    edge = f32_from_fields(binade + 1, 0)
    out.append(("edge_from_below", ulps(edge, -1), edge))         # one (small) ulp apart across the binade edge
    out.append(("edge_from_above", edge, ulps(edge, -1)))
    out.append(("edge_upper_ulp", ulps(edge, 1), edge))
    out.append(("edge_both_sides", ulps(edge, -1), ulps(edge, 1)))
    return out


# ---- scripts -----------------------------------------------------------------------------------------------------------------
def distinct_coords(n, rng, scale=3.0):
    """2 x n f32 with a distinct value per index; points 0 and 1 start as close pairs, so add_jitter has work"""
    while True:
        c = (rng.standard_normal((2, n)) * scale).astype(np.float32)
        for p, d in ((0, 0.03), (1, -0.05)):
            if p < n:
                c[1, p] = c[0, p] + F32(d)
        if len(np.unique(c)) == 2 * n:
            return c


def distinct_grad(n, rng):
    while True:
        g = rng.standard_normal((2, n)).astype(np.float32)
        if len(np.unique(g)) == 2 * n and not (g == 0).any():
            return g


def placeholders_for(n, n_best, rng):
    return rng.standard_normal((n_best, 2, n)).astype(np.float32)


def no_repeat(losses):
    """the premise of a script that is not about the stop rule: no two consecutive losses equal"""
    ls = np.asarray(losses, np.float32)
    assert not (ls[1:] == ls[:-1]).any()
    return [F32(v) for v in ls]


def random_losses(steps, rng):
    """falling on the whole, with repeats of earlier values (ties in the best list) but never of the one before"""
    out = []
    for i in range(steps):
        while True:
            v = F32(out[rng.integers(len(out))]) if out and rng.random() < 0.3 else F32(100.0 * (1.0 - i / (2.0 * steps)) + rng.random())
            if not out or v != out[-1]:
                break
        out.append(v)
    return no_repeat(out)


def falling_losses(steps):
    return no_repeat([F32(1000.0) - F32(i) for i in range(steps)])


def rising_losses(steps):
    return no_repeat([F32(10.0) + F32(i) for i in range(steps)])


def pooled_losses(steps, rng, pool=(3.5, 1.25, 7.0, 2.0, 5.75, 4.5)):
    """drawn from six distinct values, no two consecutive equal: ties at every position of the best list"""
    out = []
    for _ in range(steps):
        while True:
            v = F32(pool[rng.integers(len(pool))])
            if not out or v != out[-1]:
                break
        out.append(v)
    return no_repeat(out)


def worst_and_best_tie_losses(n_best):
    """fill the list with falling losses, then (after a loss the list refuses) one equal to the current worst, then (after another
    refused one) one equal to the current best.  The first must be refused; the second must land behind the best entry -- with
    n_best = 1 the best is the worst and it is refused as well."""
    fill = [F32(100.0) - F32(i) for i in range(n_best)]
    return no_repeat(fill + [F32(500.0), fill[0], F32(501.0), fill[-1], F32(502.0)])


def make_msg(g_raw_2xn, tail):
    g = np.asarray(g_raw_2xn, np.float32).reshape(-1)
    tail = np.asarray(tail, np.float32)
    assert tail.shape == (MSG_EXTRA,)
    return np.concatenate([g, tail])


def tail_of_loss(loss_f32):
    """the limbs of one rank that make the loop see exactly this f32 loss"""
    from kmap_amd.distributed import loss_to_limbs
    return loss_to_limbs(total_of(loss_f32))


# ---- limbs of W ranks --------------------------------------------------------------------------------------------------------
def split_fixed(q, world, rng):
    """the exact 48.48 fixed-point total q (an integer: total * 2^48) as `world` non-negative partials, each of them a float64
    (what a rank's loss_to_limbs is given): ranks 0 .. world - 2 carry random 48-bit fractions, whose sum may carry into the integer
    part, and less than 32 of the integer part each (5 + 48 bits = one f64 mantissa); the last rank carries the integer rest"""
    assert q >= 0 and world >= 1
    if world == 1:
        return [q]
    H, F = q >> 48, q & M48
    m = world - 1
    fr = [int(rng.integers(0, TWO48)) for _ in range(m - 1)]
    fr.append((F - sum(fr)) & M48)
    carry = (sum(fr) - F) >> 48
    if carry > H:                                   # the integer part cannot pay for the carries: one rank brings the fraction
        fr, carry = [F] + [0] * (m - 1), 0
    assert (sum(fr) - F) == carry << 48
    left = H - carry
    parts = []
    for f in fr:
        h = int(rng.integers(0, min(31, left) + 1))
        left -= h
        parts.append((h << 48) + f)
    parts.append(left << 48)
    assert sum(parts) == q
    return parts


def sum_tails(parts, rng):
    """every partial (an integer of 2^-48) encoded with loss_to_limbs as the f64 it must be, and the tails added in float32 in a
    shuffled order, as a float32 SUM all-reduce may"""
    from kmap_amd.distributed import loss_to_limbs
    acc = np.zeros(MSG_EXTRA, np.float32)
    for i in rng.permutation(len(parts)):
        v = parts[i] / TWO48
        assert Fraction(v) == Fraction(parts[i], TWO48), "a rank's partial must be a float64"
        acc = (acc + loss_to_limbs(v)).astype(np.float32)
    return acc


def fixed_from_tail(tail):
    """the summed limbs back to the exact integer of 2^-48 (None: flagged)"""
    if float(tail[6]) != 0.0:
        return None
    return sum(int(tail[i]) << (16 * i) for i in range(6))


def limb_cases(rng):
    """(name, world, parts): random splits for every world size, and the edges: all-0xFFFF fraction limbs on 256 ranks (every
    fraction limb sums to 16 776 960, just below 2^24), fractions that carry into the integer part, the largest integer part"""
    cases = []
    for world in (1, 2, 3, 8, 256):
        q = (int(rng.integers(1, 1 << 20)) << 48) + int(rng.integers(0, TWO48))
        if world == 1:
            q = (int(rng.integers(1, 32)) << 48) + int(rng.integers(0, TWO48))
        cases.append((f"random_w{world}", world, split_fixed(q, world, rng)))
    cases.append(("all_ffff_w256", 256, [(31 << 48) + M48] * 256))
    cases.append(("int_ffff_w256", 256, [((1 << 47) - 1) << 48] * 256))
    cases.append(("carry_w3", 3, [3 * (TWO48 >> 2)] * 3))                        # 0.75 x 3 = 2.25
    cases.append(("carry_w8", 8, [(1 << 48) + M48] * 7 + [7]))                   # 1.FF..F x 7 + 7 x 2^-48 = 14: every fraction limb carries
    cases.append(("zero_w2", 2, [0, 0]))
    return cases
