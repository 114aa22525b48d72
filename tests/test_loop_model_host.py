"""tests/_loop_model.py against the reference's own recorded runs, on any CPU: the model has to say what the reference did --
which iterations its best list kept, where it stopped, where its coordinates went and when add_jitter drew -- before
tests/test_gpu_loop_record.py holds the device's loop record to it bit for bit.  If a test here fails the model is wrong, never
the fixture."""
from fractions import Fraction

import numpy as np
import pytest

from tests import _loop_model as M

F32 = np.float32


def _feed_losses(losses, n_best=10):
    """a loss trace through the model on two far-apart points with a zero gradient: the record alone"""
    m = M.LoopModel(2, n_best, 0.01, [[0.0, 1.0], [5.0, 7.0]])
    stopped_at = None
    for i, v in enumerate(losses):
        m.apply(np.zeros((2, 2), np.float32), M.total_of(v))
        if m.stopped and stopped_at is None:
            stopped_at = i
    return m, stopped_at


@pytest.mark.parametrize("tag", ["s15", "n128"])
def test_best_list_of_recorded_long_runs(golden, tag):
    """(a) the 2500 recorded losses of a default-horizon run: the model's best list names the reference's iterations"""
    u = golden("umap_long.npz")
    losses = u[f"{tag}_losses"]
    m, stopped_at = _feed_losses(losses)
    assert stopped_at is None and m.iters == len(losses)
    assert m.best_iters() == [int(i) for i in u[f"{tag}_best_iters"]]
    np.testing.assert_array_equal(M.bits(m.best_losses()), M.bits(losses[m.best_iters()]))
    np.testing.assert_array_equal(M.bits(m.log), M.bits(losses))


@pytest.mark.parametrize("tag", ["a", "b"])
def test_early_stop_of_recorded_runs(golden, tag):
    """(b) the recorded early stops: `stopped` rises on the last loss of the trace and not before"""
    u = golden("umap_earlystop.npz")
    losses = u[f"{tag}_losses"]
    assert len(losses) < int(u[f"{tag}_n_max_iter"])
    m, stopped_at = _feed_losses(losses)
    assert stopped_at == len(losses) - 1
    assert m.iters == len(losses) and len(m.log) == len(losses)
    before = (m.iters, list(m.log), m.coords.copy(), m.best_iters())
    m.apply(np.ones((2, 2), np.float32), 0.25)                         # every later apply changes nothing
    assert (m.iters, m.log, m.best_iters()) == (before[0], before[1], before[3])
    np.testing.assert_array_equal(m.coords, before[2])


def test_coordinate_trace_of_recorded_run(golden):
    """(c) 200 recorded iterations at N = 96: the CPU oracle's gradient / 4 of the model's own iterate, the fixture's losses and
    the normals the fixture's seed yields after the init and placeholder draws -> the recorded coordinates within the 1e-5 abs of
    the existing CPU test (tests/test_distributed_cpu.py), the jitter draws per iteration exactly"""
    from oracle import oracle as O
    u = golden("umap_n96.npz")
    n, k, n_iter = 96, int(u["kmer_len"]), int(u["n_iter"])
    p = O.hd_prob_from_smooth(O.knn_smooth(u["D"].astype(np.int64), 20, nb=u["nb"]), k)
    np.random.seed(int(u["seed"]))
    init = np.random.randn(2, n).astype("float32")
    ph = np.stack([np.random.randn(2, n).astype("float32") for _ in range(10)])
    normals = np.random.normal(0, 0.01, int(u["jitter_hits"].sum()))
    np.testing.assert_array_equal(init, u["init"])
    m = M.LoopModel(n, 10, 0.01, init, ph, normals)
    hits = []
    for i in range(n_iter):
        g_raw = O.gradient_loss(p, O.cal_ld_prob_mat(m.coords), m.coords) / 4.0          # kernel output before the x4
        assert g_raw.dtype == np.float32
        used = m.jitter_used
        m.apply(g_raw, M.total_of(u["losses"][i]))
        hits.append(m.jitter_used - used)
        np.testing.assert_allclose(m.coords, u["coords"][i], rtol=0, atol=1e-5, err_msg=f"coordinates after iteration {i}")
    assert hits == [int(h) for h in u["jitter_hits"]]
    assert not m.stopped and m.jitter_used == len(normals)
    best = m.best[0]
    np.testing.assert_allclose(best[1], u["final"], rtol=0, atol=1e-5)


@pytest.mark.parametrize("binade", range(-8, 41))
def test_stop_rule_flips_at_one_mantissa(binade):
    """(d) prev and loss one ulp apart: no stop up to mantissa field 1 611 392 of the loss, a stop from 1 611 393 on, in every
    binade and whichever side prev lies on; the right-hand side evaluated in float64 decides the same (numpy < 2 promoted the
    reference's `1e-7 * abs(curr_loss)` to float64), here and on the 40 floats either side of the flip"""
    def rule32(prev, loss):
        return bool(abs(prev - loss) < F32(1e-7) * abs(loss))

    def rule64(prev, loss):
        return bool(np.float64(abs(prev - loss)) < 1e-7 * np.float64(abs(loss)))

    for m in range(M.STOP_FLIP - 40, M.STOP_FLIP + 42):
        loss = M.f32_from_fields(binade, m)
        for k in (-1, 1):
            prev = M.ulps(loss, k)
            assert rule32(prev, loss) == (m > M.STOP_FLIP), (binade, m, k)
            assert rule64(prev, loss) == (m > M.STOP_FLIP), (binade, m, k)
    # and the model is that rule
    for name, prev, loss in M.stop_pairs(binade):
        lm = M.LoopModel(1, 1, 0.01, [[0.0], [5.0]])
        lm.apply(np.zeros((2, 1), np.float32), M.total_of(prev))
        assert not lm.stopped and lm.log[-1] == prev                   # prev = inf: the first iteration never stops
        lm.apply(np.zeros((2, 1), np.float32), M.total_of(loss))
        assert lm.stopped == rule32(prev, loss) and lm.log[-1] == loss, name
    want = {f"m{M.STOP_FLIP}-1ulp": False, f"m{M.STOP_FLIP}+1ulp": False, f"m{M.STOP_FLIP + 1}-1ulp": True,
            f"m{M.STOP_FLIP + 1}+1ulp": True, "equal": True, f"m{M.STOP_FLIP + 1}+2ulp": False, f"m{M.STOP_FLIP + 1}-2ulp": False}
    got = {name: rule32(prev, loss) for name, prev, loss in M.stop_pairs(binade)}
    assert {k: got[k] for k in want} == want


def test_limb_helper_sums_are_exact():
    """(e) W ranks' limbs, added in float32 in a shuffled order, decode to the exact integer sum: W in {1, 2, 3, 8, 256}, all-0xFFFF
    limbs on 256 ranks, fractions that carry into the integer part"""
    from kmap_amd.distributed import loss_from_limbs
    rng = np.random.default_rng(5)
    cases = M.limb_cases(rng)
    assert {w for _, w, _ in cases} == {1, 2, 3, 8, 256}
    carried = 0
    for name, world, parts in cases:
        assert len(parts) == world
        q = sum(parts)
        tail = M.sum_tails(parts, rng)
        assert tail.dtype == np.float32 and tail[:6].max() < (1 << 24) and tail[6] == 0 and tail[7] == 0
        assert M.fixed_from_tail(tail) == q, name
        np.testing.assert_array_equal(tail, M.sum_tails(parts, rng), err_msg=name)      # another order, the same floats
        assert int(float(q >> 48)) == q >> 48                                           # float(hi) is exact, so the decoder
        assert loss_from_limbs(tail) == float(Fraction(q, M.TWO48)), name               #   rounds once
        carried += sum(p & M.M48 for p in parts) >> 48 > 0
    by_name = {name: parts for name, _, parts in cases}
    t = M.sum_tails(by_name["all_ffff_w256"], rng)
    assert list(t[:3]) == [16776960.0] * 3 and t[3] == 31 * 256
    t = M.sum_tails(by_name["int_ffff_w256"], rng)
    assert list(t[3:5]) == [16776960.0] * 2
    assert loss_from_limbs(M.sum_tails(by_name["carry_w3"], rng)) == 2.25
    assert loss_from_limbs(M.sum_tails(by_name["carry_w8"], rng)) == 14.0
    assert carried >= 5                                                                 # the random splits carry too
    # the split itself: every partial a float64, the sum exact, for totals that need the whole 48.48 range
    for world in (2, 3, 8, 256):
        for q in (0, 1, M.M48, M.TWO48, (12345 << 48) + 1, (((1 << 40) + 3) << 48) + M.M48):
            parts = M.split_fixed(q, world, rng)
            assert len(parts) == world and sum(parts) == q and min(parts) >= 0
            assert M.fixed_from_tail(M.sum_tails(parts, rng)) == q
    flagged = M.sum_tails([3 << 48, 5 << 48], rng)
    flagged[6] = 1.0
    assert M.fixed_from_tail(flagged) is None and np.isnan(loss_from_limbs(flagged))


def test_model_rules_on_hand_made_steps():
    """the rules a recorded run does not reach: NaN is logged but neither inserted nor a stop, a tie lands behind its equals, a
    loss equal to the worst is refused, an exhausted pool adds 0.0 and still counts, a refilled pool is indexed by the running
    count"""
    z = np.zeros((2, 2), np.float32)
    m = M.LoopModel(2, 3, 0.01, [[0.0, 1.0], [5.0, 7.0]])
    for v in (4.0, float("nan"), 2.0, 4.0, 9.0, 2.0, 9.0, 4.0):
        m.apply(z, v / 2)
    assert not m.stopped and m.iters == 8 and np.isnan(m.log[1])
    assert m.best_iters() == [2, 5, 0]                                  # 2.0 (it 2), 2.0 (it 5) behind it, 4.0 (it 0); 4.0 = worst refused
    # jitter: equal pair -> x takes the draw; y < x -> y takes it; the pool runs dry; a longer pool continues at the count
    m = M.LoopModel(2, 1, 0.01, [[1.0, 3.0], [1.0, 2.95]], normals=[0.25])
    m.apply(z, 10.0)
    assert m.jitter_used == 2 and m.coords[0, 0] == F32(1.25) and m.coords[1, 1] == F32(2.95) and m.coords[0, 1] == F32(3.0)
    m.set_jitter([9.0, 9.0, 0.5, -0.5])
    m.coords[:] = [[1.0, 3.0], [1.0, 2.95]]
    m.apply(z, 9.0)
    assert m.jitter_used == 4 and m.coords[0, 0] == F32(1.5) and m.coords[1, 1] == F32(2.45)
    # a difference of exactly f32(0.1) does not draw, one ulp less does
    m = M.LoopModel(1, 1, 0.01, [[0.0], [F32(0.1)]], normals=[0.5])
    m.apply(np.zeros((2, 1), np.float32), 10.0)
    assert m.jitter_used == 0
    m = M.LoopModel(1, 1, 0.01, [[0.0], [M.ulps(F32(0.1), -1)]], normals=[0.5])
    m.apply(np.zeros((2, 1), np.float32), 10.0)
    assert m.jitter_used == 1 and m.coords[0, 0] == F32(0.5)
    # the update: three roundings, in this order
    g, y, lr = F32(0.3333333), F32(1.7), F32(0.01)
    m = M.LoopModel(1, 1, 0.01, [[y], [50.0]])
    m.apply(np.array([[g], [0.0]], np.float32), 10.0)
    assert m.coords[0, 0] == F32(y + F32(-F32(F32(4) * g) * lr))
