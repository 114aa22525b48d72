"""Helpers of the default-horizon embedding tests (tests/test_gpu_embed.py, tests/test_gpu_fullsize.py): a loop driver that
stops the device loop on checkpoints, the reference's best-list rule replayed on a loss trace, and the comparison of a device run
with a run of the reference / the CPU oracle.  No test lives here."""
import numpy as np


def spy_run_loop(V, monkeypatch, ckpts, rec):
    """Replace visualization._run_loop by a driver that stops the device loop on every checkpoint (coordinates after i updates and
    jitters; 0 = the init) and records them, the loop state, the loss log and the whole best list before the session closes."""
    real = V._run_loop
    want = sorted(set(int(c) for c in ckpts))

    def spy(sess, n_max_iter, step_fn=None, debug=False, trace=None):
        got, done = {}, [0]
        if 0 in want:
            got[0] = sess.coords()

        def stepper(seg):
            end = done[0] + seg
            while done[0] < end:
                nxt = min([c for c in want if c > done[0]] + [end])
                sess.step(nxt - done[0])
                done[0] = nxt
                if nxt in want:
                    got[nxt] = sess.coords()

        info = real(sess, n_max_iter, step_fn=stepper, debug=debug, trace=trace)
        rec.update(coords=got, info=info, losses=sess.losses(), best_list=sess.best_list(), best=sess.best())
        return info

    monkeypatch.setattr(V, "_run_loop", spy)


def replay_best_list(losses, n_best=10):
    """the loss indices of visualization.py:304-308's best list after the run (insort_right; -1: a placeholder)"""
    import bisect
    best = [(np.inf, -1)] * n_best
    for j, v in enumerate(np.asarray(losses, np.float64)):
        if v < best[-1][0]:
            best = best[:-1]
            best.insert(bisect.bisect_right([b[0] for b in best], float(v)), (float(v), j))
    return [b[1] for b in best]


def assert_same_run(rec, want_coords, want_best_iters, want_final, want_hits, want_losses, loss_rtol=2e-6):
    """rec (from spy_run_loop) against a run of the reference / the oracle (want_coords: at least the device's checkpoints and the
    iterations of the best list): every checkpoint and the returned array bit for bit, the
    same best list (each device snapshot is the checkpoint of the iteration the list names), the same number of jitter draws, the
    losses to loss_rtol.  Returns the largest relative loss difference."""
    assert rec["info"]["iters"] == len(want_losses) and not rec["info"]["stopped"]
    assert rec["coords"]
    for i, c in sorted(rec["coords"].items()):
        np.testing.assert_array_equal(c, want_coords[i], err_msg=f"coordinates after {i} iterations")
    np.testing.assert_array_equal(rec["best"], want_final)
    assert rec["info"]["jitter_used"] == want_hits
    dl = np.asarray(rec["losses"], np.float64)
    wl = np.asarray(want_losses, np.float64)
    assert len(dl) == len(wl)
    rel = float(np.max(np.abs(dl / wl - 1)))
    assert rel <= loss_rtol, rel
    # the device's best list: its own losses decide it exactly as the reference's rule would ...
    got_iters = replay_best_list(dl, len(want_best_iters))
    if got_iters != list(want_best_iters):          # only entries whose losses are closer than the loss tolerance may trade places
        assert sorted(got_iters) == sorted(want_best_iters), (got_iters, list(want_best_iters))
        for a, b in zip(got_iters, want_best_iters):
            assert a == b or abs(wl[a] / wl[b] - 1) <= 2 * loss_rtol, (got_iters, list(want_best_iters))
    # ... and every snapshot it holds is the checkpoint of the iteration it names, its loss that iteration's logged loss
    snaps, bl = rec["best_list"]
    for pos, it in enumerate(got_iters):
        np.testing.assert_array_equal(snaps[pos], want_coords[it], err_msg=f"best-list entry {pos} (iteration {it})")
        assert bl[pos] == np.float32(dl[it])
    return rel


def assert_margins(losses, n_best=10, margin=1e-5):
    """the premise that makes the decisions above a test of the device: the n_best + 1 lowest losses are more than `margin` apart
    (relative) and no two consecutive losses come near the stop rule's 1e-7"""
    ls = np.asarray(losses, np.float64)
    lo = np.sort(ls)[:n_best + 1]
    assert (np.diff(lo) / lo[1:]).min() > margin, np.diff(lo) / lo[1:]
    assert (np.abs(np.diff(ls)) / ls[1:]).min() > 100 * 1e-7
