"""The loop record of the embedding (csrc/embed.hip: step_decide, step_element, step_leader behind apply_kernel<false> and
apply_msg_kernel<true / false>) against tests/_loop_model.py, bit for bit after EVERY step of a scripted (gradient, loss)
sequence: kmap_embed_apply / kmap_embed_apply_msg take the caller's gradient and loss, so no probabilities and no force kernel
are involved and the record can be walked through the cases a natural trajectory never reaches -- ties in the best list, the
stop rule one ulp either side of its threshold, NaN and flagged losses, n_best other than 10, N of 1 to 3, the leader's indices at
a block edge, a dry or replaced jitter pool, limb sums of many ranks, applies on a stopped session.

Every comparison is exact: floats as their uint32 bits (a NaN by its position only); there is no tolerance in this file.
The caller's gradient, loss and message always live in guarded buffers (tests/_footprint.py), checked after every step.
"""
from fractions import Fraction

import numpy as np
import pytest

from tests import _footprint as F
from tests import _loop_model as M

pytestmark = pytest.mark.gpu

F32 = np.float32
LR = 0.01
_BUF = None                     # buffer class of the guarded buffers (None: device memory)


def _session(n, n_best, lr, kind):
    """apply: full rows, driven through kmap_embed_apply (apply_kernel<false>); msg: full rows through kmap_embed_apply_msg
    (apply_msg_kernel<false>); shard: a row-sharded SEQ session through apply_msg (apply_msg_kernel<true>, which zeroes the
    gradient entries of the message); cyclic: rank 0 of 2 of the cyclic layout through apply_msg (nothing zeroed)"""
    from kmap_amd.visualization import EMBED_FAST, EMBED_SEQ, EmbedSession
    if kind == "shard":
        return EmbedSession(n, n_best, lr, EMBED_SEQ, row0=n // 3, nrows=n // 3)
    if kind == "cyclic":
        return EmbedSession(n, n_best, lr, cyclic=(2, 0))
    return EmbedSession(n, n_best, lr, EMBED_FAST if kind == "apply" else EMBED_SEQ)


def _same(got, want, ctx):
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    assert got.shape == want.shape, (ctx, got.shape, want.shape)
    gn, wn = np.isnan(got), np.isnan(want)
    np.testing.assert_array_equal(gn, wn, err_msg=f"{ctx}: NaN positions")
    np.testing.assert_array_equal(np.where(gn, 0, got.view(np.uint32)), np.where(wn, 0, want.view(np.uint32)), err_msg=ctx)


class Driver:
    """one session and its model side by side; every step is compared in full"""

    def __init__(self, n, kind="apply", n_best=10, lr=LR, seed=0, coords=None, pool=None, fill=0xA5):
        self.rng = rng = np.random.default_rng([seed, n, n_best])
        self.n, self.kind, self.steps = n, kind, 0
        coords = M.distinct_coords(n, rng) if coords is None else np.array(coords, np.float32).reshape(2, n)
        ph = M.placeholders_for(n, n_best, rng)
        pool = rng.normal(0, 0.01, 64) if pool is None else np.asarray(pool, np.float64)
        self.bufs = []
        self.sess = _session(n, n_best, lr, kind)
        try:
            self.sess.set_coords(coords, ph)
            self.sess.set_jitter(pool)
            self.model = M.LoopModel(n, n_best, lr, coords, ph, pool)
            self.g = self._guarded(2 * n * 4, fill, "gradient")
            self.l = self._guarded(8, fill, "loss")
            self.m = self._guarded((2 * n + M.MSG_EXTRA) * 4, fill, "message")
            self.check("after set_coords")
        except BaseException:
            self.close()
            raise

    def _guarded(self, nbytes, fill, name):
        g = F.Guarded(nbytes, fill=fill, buffer_cls=_BUF, name=name)
        self.bufs.append(g)
        return g

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def close(self):
        self.sess.close()
        F.free(*self.bufs)
        self.bufs = []

    def grad(self, zero_points=False):
        """a gradient with a distinct value per index (zero_points: points 0 and 1 stay where they are)"""
        g = M.distinct_grad(self.n, self.rng)
        if zero_points:
            g[:, :2] = 0
        return g

    def set_jitter(self, pool):
        self.sess.set_jitter(pool)
        self.model.set_jitter(pool)

    # ---- one iteration ----
    def apply(self, g_raw, total):
        g_raw = np.ascontiguousarray(g_raw, np.float32).reshape(2, self.n)
        tot = np.array([total], np.float64)
        self.g.upload(g_raw)
        self.l.upload(tot)
        self.sess.apply(self.g.ptr, self.l.ptr)
        self.model.apply(g_raw, total)
        self.steps += 1
        self.check("apply")
        np.testing.assert_array_equal(self.g.payload(np.uint32), g_raw.reshape(-1).view(np.uint32), err_msg="the caller's gradient changed")
        np.testing.assert_array_equal(self.l.payload(np.uint64), tot.view(np.uint64), err_msg="the caller's loss changed")

    def apply_msg(self, g_raw, tail):
        msg = M.make_msg(g_raw, tail)
        self.m.upload(msg)
        self.sess.apply_msg(self.m.ptr)
        self.model.apply_msg(msg)
        self.steps += 1
        want = msg.copy()
        if self.kind == "shard":
            want[:2 * self.n] = 0                       # read, then zeroed -- on a stopped session too; the tail is left alone
        np.testing.assert_array_equal(self.m.payload(np.uint32), want.view(np.uint32), err_msg=f"{self.kind}: the message after apply_msg")
        self.check("apply_msg")

    def step(self, g_raw, loss_f32):
        """an exact f32 loss through whichever entry the session is driven by"""
        if self.kind == "apply":
            self.apply(g_raw, M.total_of(loss_f32))
        else:
            self.apply_msg(g_raw, M.tail_of_loss(loss_f32))

    def run(self, losses, zero_points=False):
        for v in losses:
            self.step(self.grad(zero_points), v)

    # ---- the whole record ----
    def check(self, what):
        s, m = self.sess, self.model
        ctx = f"{self.kind} n={self.n} n_best={m.n_best} step {self.steps} ({what})"
        st = s.state()
        assert (st["iters"], st["stopped"], st["jitter_used"]) == (m.iters, m.stopped, m.jitter_used), (ctx, st)
        _same(st["last_loss"], m.last_loss, ctx + ": last_loss")
        _same(st["best_loss"], m.best[0][0], ctx + ": best_loss")
        _same(s.coords(), m.coords, ctx + ": coords")
        snaps, losses = s.best_list()
        _same(losses, m.best_losses(), ctx + ": best-list losses")
        _same(snaps, m.best_snaps(), ctx + ": best-list snapshots")
        _same(s.best(), m.best[0][1], ctx + ": best()")
        _same(s.losses(), np.array(m.log, np.float32), ctx + ": loss log")
        F.guards(*self.bufs)


# ---- shapes ------------------------------------------------------------------------------------------------------------------
NS = [1, 2, 3, 127, 128, 129, 255, 256, 257, 701]
SHAPES = [(n, kind) for n in NS for kind in ("apply", "msg", "shard") if kind != "shard" or n >= 3] + [(257, "cyclic"), (701, "cyclic")]


@pytest.mark.parametrize("n,kind", SHAPES)
def test_twelve_random_steps(n, kind):
    """2 N at, below and above one 256-thread block; the leader's indices n, n + 1 at the last thread of block 0 (n = 255), on both
    sides of the edge (n = 255, 256: 255 | 256, 256 | 257) and further in; N too small for point 1 or for any other point"""
    with Driver(n, kind, seed=1) as d:
        d.run(M.random_losses(12, d.rng))
        assert d.model.iters == 12 and not d.model.stopped
        assert d.model.jitter_used > 0 and -1 not in d.model.best_iters()


# ---- best list ---------------------------------------------------------------------------------------------------------------
N_BEST = [1, 2, 10, 64]


@pytest.mark.parametrize("n_best", N_BEST)
@pytest.mark.parametrize("script", ["falling", "rising", "worst_and_best_tie"])
def test_best_list_scripts(n_best, script):
    losses = {"falling": lambda: M.falling_losses(n_best + 3), "rising": lambda: M.rising_losses(n_best + 3),
              "worst_and_best_tie": lambda: M.worst_and_best_tie_losses(n_best)}[script]()
    with Driver(129, "apply", n_best=n_best, seed=2) as d:
        d.run(losses)
        m = d.model
        assert not m.stopped and m.iters == len(losses)
        if script == "falling":                                   # every loss enters at the front
            assert m.best_iters() == list(range(n_best + 2, 2, -1))
        elif script == "rising":                                  # only the first n_best enter
            assert m.best_iters() == list(range(n_best))
        elif n_best == 1:                                         # equal to the worst = the best: refused twice
            assert m.best_iters() == [0]
        else:                                                     # worst refused; the best's equal lands behind it
            assert m.best_iters()[:2] == [n_best - 1, n_best + 3] and n_best + 1 not in m.best_iters()


@pytest.mark.parametrize("n_best", N_BEST)
@pytest.mark.parametrize("kind", ["apply", "shard"])
def test_best_list_ties_everywhere(n_best, kind):
    """200 losses from a pool of six values, no two consecutive equal: ties at every position of the list"""
    with Driver(129, kind, n_best=n_best, seed=3) as d:
        d.run(M.pooled_losses(200, d.rng))
        assert not d.model.stopped and d.model.iters == 200
        if n_best >= 2:
            bl = d.model.best_losses()
            assert (bl[1:] == bl[:-1]).any()
            pairs = list(zip(bl.tolist(), d.model.best_iters()))
            assert pairs == sorted(pairs)                         # among equals the earlier iteration stands in front


# ---- stop rule ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("binade", [-8, 0, 5, 12, 23, 40])
@pytest.mark.parametrize("kind", ["apply", "shard"])
def test_stop_rule_at_its_threshold(binade, kind):
    """prev = loss +- 1 ulp at the two mantissas either side of the flip, +- 2 ulp, prev == loss, a pair across a binade edge, a
    repeated zero; the first iteration (prev = inf) never stops.  Then three more applies with new gradients and lower losses:
    a stopped session keeps its record, and a sharded one still zeroes the message."""
    known = {f"m{M.STOP_FLIP}-1ulp": False, f"m{M.STOP_FLIP}+1ulp": False, f"m{M.STOP_FLIP + 1}-1ulp": True,
             f"m{M.STOP_FLIP + 1}+1ulp": True, f"m{M.STOP_FLIP + 1}-2ulp": False, f"m{M.STOP_FLIP + 1}+2ulp": False,
             "equal": True, "zero_twice": False}
    for name, prev, loss in M.stop_pairs(binade) + [("zero_twice", F32(0), F32(0))]:
        with Driver(5, kind, n_best=3, seed=4) as d:
            d.step(d.grad(), prev)
            assert not d.model.stopped, name
            d.step(d.grad(), loss)
            if name in known:
                assert d.model.stopped == known[name], name
            stopped, coords, iters = d.model.stopped, d.model.coords.copy(), d.model.iters
            for j in range(3):
                d.step(d.grad(), loss * F32(0.5 ** (j + 1)))
            if stopped:
                assert d.model.iters == iters == 2 and len(d.model.log) == 2
                np.testing.assert_array_equal(d.model.coords, coords)
            else:
                assert d.model.iters == 5


# ---- NaN, flags, signs -------------------------------------------------------------------------------------------------------
def _assert_nan_step(d, step):
    """the iteration was logged as NaN, not inserted, no stop, and the update was applied"""
    m = d.model
    assert np.isnan(m.log[step]) and step not in m.best_iters() and not m.stopped and m.iters == step + 1


def test_nan_negative_and_infinite_losses_through_apply():
    with Driver(129, "apply", n_best=4, seed=5) as d:
        d.step(d.grad(), F32(50))
        before = d.model.coords.copy()
        d.apply(d.grad(), float("nan"))
        _assert_nan_step(d, 1)
        assert (d.model.coords != before).all()
        d.step(d.grad(), F32(50))                        # prev is NaN now: the repeated 50 is no stop
        assert not d.model.stopped and 2 in d.model.best_iters()
        d.apply(d.grad(), -3.0)                          # a negative loss is the best one
        assert d.model.best_iters()[0] == 3 and d.model.best[0][0] == F32(-6)
        d.step(d.grad(), F32(44))
        d.apply(d.grad(), float("inf"))                  # +inf: not below an inf placeholder or anything else; |44 - inf| is no stop
        assert 5 not in d.model.best_iters() and not d.model.stopped
        d.step(d.grad(), F32(43))                        # |inf - 43| < 1e-7 * 43 is false
        d.apply(d.grad(), float("-inf"))
        assert d.model.best_iters()[0] == 7
        d.apply(d.grad(), 1e300)                         # f32(2 * total) overflows to +inf
        d.step(d.grad(), F32(42))
        assert not d.model.stopped and d.model.iters == 10


@pytest.mark.parametrize("kind", ["msg", "shard"])
def test_flagged_losses_through_apply_msg(kind):
    from kmap_amd.distributed import loss_to_limbs
    one_rank = loss_to_limbs(float("nan")) + loss_to_limbs(3.25) + loss_to_limbs(7.0)
    two_ranks = loss_to_limbs(-1.0) + loss_to_limbs(float("inf")) + loss_to_limbs(2.5)
    too_large = loss_to_limbs(2.0 ** 47)
    assert (one_rank[6], two_ranks[6], too_large[6]) == (1.0, 2.0, 1.0)
    with Driver(129, kind, n_best=4, seed=6) as d:
        d.step(d.grad(), F32(50))
        for i, tail in enumerate((one_rank, two_ranks, too_large)):
            before = d.model.coords.copy()
            d.apply_msg(d.grad(), tail)
            _assert_nan_step(d, 1 + 2 * i)
            assert (d.model.coords != before).all()
            d.step(d.grad(), F32(50))                    # prev is NaN: the repeated 50 is no stop
            assert not d.model.stopped and 2 + 2 * i in d.model.best_iters()
        d.apply_msg(d.grad(), loss_to_limbs(2.0 ** 47 - 1))         # the largest partial a rank can send
        assert d.model.log[-1] == F32(2.0 ** 48) and not d.model.stopped


# ---- limbs of many ranks -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["msg", "shard"])
def test_limb_sums_of_many_ranks(kind):
    """W ranks' limbs added in float32 in a shuffled order, with all-0xFFFF limbs and carries out of every fraction limb: the
    logged loss is f32(2 * exact sum)"""
    with Driver(5, kind, n_best=3, seed=7) as d:
        for name, world, parts in M.limb_cases(d.rng):
            q = sum(parts)
            d.apply_msg(d.grad(), M.sum_tails(parts, d.rng))
            assert not d.model.stopped, name
            assert M.bits(d.model.log[-1]) == M.bits(F32(2.0 * float(Fraction(q, M.TWO48)))), name
            d.step(d.grad(), F32(77))                    # something else in between: no two equal sums in a row


# ---- jitter ------------------------------------------------------------------------------------------------------------------
FAR = [(10.0, 20.0), (-30.0, 40.0)]                 # a point whose pair is no jitter candidate
TENTH = F32(0.1)
JITTER_CASES = {
    # name: (n, pair of point 0, pair of point 1, pool, draws of step 1, [(coordinate, point) that took them])
    "exactly_a_tenth": (4, (0.0, TENTH), FAR[1], [0.5, 0.25], 0, []),
    "one_ulp_below_a_tenth": (4, (0.0, M.ulps(TENTH, -1)), FAR[1], [0.5, 0.25], 1, [(0, 0)]),
    "equal_values_x_takes_it": (4, (2.5, 2.5), FAR[1], [0.01, 0.02], 1, [(0, 0)]),
    "y_below_x_y_takes_it": (4, (2.5, 2.45), FAR[1], [0.01, 0.02], 1, [(1, 0)]),
    "point_1_only": (4, FAR[0], (-3.0, -3.02), [0.01, 0.02], 1, [(1, 1)]),
    "both_points_in_order": (4, (1.0, 1.05), (-3.0, -3.02), [0.015, -0.02, 0.01, 0.01], 2, [(0, 0), (1, 1)]),
    "one_point_only_exists": (1, (0.5, 0.5), None, [0.01, 0.02, 0.03], 1, [(0, 0)]),
    "two_points_exist": (2, (0.5, 0.5), (0.25, 0.3), [0.01, 0.02, 0.03, 0.04, 0.05, 0.06], 2, [(0, 0), (0, 1)]),
    "normal_below_half_an_ulp": (4, (1024.0, 1024.05), FAR[1], [1e-5, 2e-5, 3e-5], 1, []),
}


def _jitter_coords(n, p0, p1, rng):
    c = M.distinct_coords(n, rng)
    for p, pair in ((0, p0), (1, p1)):
        if p < n:
            c[0, p], c[1, p] = pair
    return c


@pytest.mark.parametrize("kind", ["apply", "shard"])
@pytest.mark.parametrize("case", list(JITTER_CASES))
def test_jitter_cases(case, kind):
    """points 0 and 1 get a zero gradient, so the pair add_jitter sees in step 1 is the pair that was set"""
    n, p0, p1, pool, draws, took = JITTER_CASES[case]
    if kind == "shard" and n < 3:
        kind = "msg"
    rng = np.random.default_rng(8)
    coords = _jitter_coords(n, p0, p1, rng)
    with Driver(n, kind, n_best=2, seed=8, coords=coords, pool=pool) as d:
        d.step(d.grad(zero_points=True), F32(90))
        assert d.model.jitter_used == draws
        changed = {(int(c), int(p)) for c, p in zip(*np.nonzero(d.model.coords[:, :2] != coords[:, :2]))}
        assert changed == set(took)
        for k, (c, p) in enumerate(took):
            assert d.model.coords[c, p] == F32(np.float64(coords[c, p]) + pool[k])
        d.run([F32(80), F32(70)], zero_points=True)
        assert d.model.iters == 3


@pytest.mark.parametrize("kind", ["apply", "shard"])
def test_jitter_pool_runs_dry_and_is_replaced(kind):
    """three normals for a script that wants two per iteration: the fourth draw adds 0.0 and the count still advances (the
    project's rule).  Then a longer pool with other leading values: the running count indexes into it."""
    rng = np.random.default_rng(9)
    coords = _jitter_coords(4, (2.5, 2.5), (7.0, 7.0), rng)
    with Driver(4, kind, n_best=2, seed=9, coords=coords, pool=[1e-3, -1e-3, 2e-3]) as d:
        d.run([F32(90), F32(80)], zero_points=True)
        assert d.model.jitter_used == 4
        at_dry = d.model.coords.copy()
        d.step(d.grad(zero_points=True), F32(70))
        assert d.model.jitter_used == 6
        np.testing.assert_array_equal(d.model.coords[:, :2], at_dry[:, :2])            # + 0.0 twice
        longer = np.array([9.0, 9.0, 9.0, 9.0, 9.0, 9.0, 3e-3, -2e-3, 1e-3, 4e-3])
        d.set_jitter(longer)
        d.step(d.grad(zero_points=True), F32(60))
        assert d.model.jitter_used == 8
        assert not (np.abs(d.model.coords[:, :2] - at_dry[:, :2]) > 0.1).any()         # none of the 9.0 in front was taken
        assert (d.model.coords[:, :2] != at_dry[:, :2]).sum() == 2
        d.step(d.grad(zero_points=True), F32(50))
        assert d.model.jitter_used == 10
        d.step(d.grad(zero_points=True), F32(40))                                      # dry again
        assert d.model.jitter_used == 12


# ---- footprint ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fill", [0x00, 0xFF])
@pytest.mark.parametrize("n", [1, 129, 257])
def test_footprint_of_the_callers_buffers(n, fill):
    """gradient, loss and message in guarded buffers whose bands hold 0x00 in one run and 0xFF (NaN as floats) in the other: the
    bands stay intact, gradient and loss are unchanged, the message is unchanged -- but for [0, 2 N) of a sharded session, which is
    zeroed while its 8 tail floats stay -- and the record does not depend on a byte outside them (all inside Driver.apply /
    apply_msg / check)"""
    kinds = ["apply", "msg"] + (["shard"] if n >= 3 else []) + (["cyclic"] if n >= 257 else [])
    for kind in kinds:
        with Driver(n, kind, n_best=3, seed=10, fill=fill) as d:
            d.run(M.random_losses(3, d.rng))
            d.step(d.grad(), d.model.log[-1])                    # a stop, then an apply on the stopped session
            assert d.model.stopped
            d.step(d.grad(), F32(1))
            assert d.model.iters == 4
            if kind != "apply":
                tail = d.m.payload(np.float32)[2 * n:]
                np.testing.assert_array_equal(tail, M.tail_of_loss(F32(1)))
                assert d.m.payload(np.float32)[:2 * n].any() == (kind != "shard")


# ---- log cap -----------------------------------------------------------------------------------------------------------------
def test_loss_log_cap():
    """65 541 applies at N = 3, the losses 1e6 - i resident as one device array of doubles addressed by offset and one resident
    gradient: every iteration is counted, the first 65 536 are logged, and the record at the end is the model's"""
    n, steps = 3, M.LOG_CAP + 5
    losses = (1e6 - np.arange(steps)).astype(np.float32)
    assert (losses.astype(np.float64) == 1e6 - np.arange(steps)).all()
    with Driver(n, "apply", n_best=10, seed=11) as d:
        totals = d._guarded(steps * 8, 0xA5, "losses")
        totals.upload(losses.astype(np.float64) / 2)
        g = d.grad()
        d.g.upload(g)
        for i in range(steps):
            d.sess.apply(d.g.ptr, totals.ptr + 8 * i)
            d.model.apply(g, float(losses[i]) / 2)
        d.steps = steps
        d.check("after the last apply")
        st = d.sess.state()
        assert st["iters"] == steps == d.model.iters and not st["stopped"]
        got = d.sess.losses()
        assert len(got) == M.LOG_CAP == len(d.model.log)
        np.testing.assert_array_equal(got, losses[:M.LOG_CAP])
        assert d.model.best_iters() == list(range(steps - 1, steps - 11, -1))
        np.testing.assert_array_equal(totals.payload(np.float64), losses.astype(np.float64) / 2)
