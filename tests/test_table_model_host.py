"""tests/_table_model.py against the oracle, on any CPU: the model has to say what the reference says before
tests/test_gpu_table_queries.py holds the device to it.  Small random tables (a few hundred entries) at k = 5, 8, 15, 16, 21, 31."""
import warnings

import numpy as np
import pytest

from tests import _table_model as M

KS = [5, 8, 15, 16, 21, 31]


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


def _table(O, k, seed, n=400):
    rng = np.random.default_rng(seed)
    u = np.unique(rng.integers(0, 4 ** k, size=n, dtype=np.uint64)).astype(O.get_hash_dtype(k))
    c = rng.integers(1, 1000, size=len(u)).astype(O.get_cnt_dtype(k))
    return rng, u, c


def _canon(O, h, k):
    """the smaller of a hash and its reverse complement (how consensuses are stored in reverse-complement mode)"""
    return min(int(h), int(O.revcom_hash(int(h), k)))


def test_popc2_and_revcom(O):
    rng = np.random.default_rng(1)
    for k in KS + [1, 2, 30]:
        x = rng.integers(0, 4 ** k, size=300, dtype=np.uint64).astype(np.int64)
        naive = sum((((x >> (2 * p)) & 3) != 0).astype(np.int64) for p in range(k))
        np.testing.assert_array_equal(M.popc2(x), naive)
        rc = O.get_revcom_hash_arr(x.astype(O.get_hash_dtype(k)), k)
        np.testing.assert_array_equal(M.revcom(x, k), rc.astype(np.int64))
        np.testing.assert_array_equal(M.revcom(M.revcom(x, k), k), x)
    assert int(M.popc2(0)) == 0 and int(M.popc2((1 << 62) - 1)) == 31 and int(M.popc2(0b100001)) == 2


def test_count_values_total_topk():
    raw = np.array([5, 0, 2 ** 31, 2 ** 32 - 1, 7, 7, 2 ** 31 - 1], np.int64)
    np.testing.assert_array_equal(M.count_values(raw, 15), [5, 0, -2 ** 31, -1, 7, 7, 2 ** 31 - 1])
    np.testing.assert_array_equal(M.count_values(raw.astype(np.uint32).view(np.int32), 15), M.count_values(raw, 15))
    np.testing.assert_array_equal(M.count_values(raw, 16), raw)
    assert M.table_total(raw, 15) == 5 - 2 ** 31 - 1 + 14 + 2 ** 31 - 1 and M.table_total(raw, 16) == int(raw.sum())
    assert M.table_total(raw[:0], 16) == 0
    idx, cnt = M.table_topk(raw, 15, 3)
    assert list(idx) == [6, 4, 5] and list(cnt) == [2 ** 31 - 1, 7, 7]
    idx, cnt = M.table_topk(raw, 16, 16)
    assert list(idx) == [3, 2, 6, 4, 5, 0] and list(cnt) == [2 ** 32 - 1, 2 ** 31, 2 ** 31 - 1, 7, 7, 5]
    rng = np.random.default_rng(2)
    c = rng.integers(0, 6, size=500)
    idx, cnt = M.table_topk(c, 9, 16)                      # against a stable sort: equal counts keep the table order
    want = np.argsort(-c, kind="stable")[:16]
    np.testing.assert_array_equal(idx, want)
    np.testing.assert_array_equal(cnt, c[want])


@pytest.mark.parametrize("k", KS)
def test_ball_mass_vs_oracle(O, k):
    rng, u, c = _table(O, k, 10 + k)
    cands = [int(u[3]), int(O.revcom_hash(int(u[7]), k)), int(u[3]), int(rng.integers(0, 4 ** k)), 0, 4 ** k - 1]
    if k % 2 == 0:
        cands.append(int(O.kmer2hash(("ACGT" * 8)[:k // 2] + O.reverse_complement(("ACGT" * 8)[:k // 2]))))   # a palindrome
    for r in (-1, 0, 1, k // 2, k, k + 1):
        for rc in (False, True):
            want = O.hamball_mass(u, c, k, np.array(cands, np.uint64), r, rc)
            assert M.ball_mass(u, c, k, cands, r, rc) == [int(x) for x in want], (r, rc)


def _consensus_sets(O, k, u, rng, revcom_mode):
    """lists of consensus strings, longest first: one full-length one; short ones sharing planted heads; a palindrome"""
    kmers = [O.hash2kmer(int(h), k) for h in u[rng.choice(len(u), size=6, replace=False)]]

    def ok(s):
        return s if not revcom_mode or int(O.kmer2hash(s)) <= int(O.revcom_hash(O.kmer2hash(s), len(s))) else O.reverse_complement(s)
    sets = [[ok(kmers[0])],
            [ok(kmers[1]), ok(kmers[2][:max(3, k - 2)]), ok(kmers[3][:3]), ok(kmers[4][:3])],
            [ok(kmers[5][:max(3, k // 2)]), ok(kmers[5][:max(3, k // 2)]), ok("ACGT"[:4] if k >= 4 else "ACG")]]
    if k >= 6:
        sets.append([ok("AACGTT"), ok(kmers[0][:4])])       # AACGTT is its own reverse complement
    return sets


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("revcom_mode", [True, False])
def test_label_table_vs_oracle(O, k, revcom_mode):
    rng, u, c = _table(O, k, 20 + k)
    for cons in _consensus_sets(O, k, u, rng, revcom_mode):
        for radius_of_len in ({n: min(n, 1 + n // 4) for n in range(1, 32)}, {n: 0 for n in range(1, 32)},
                              {n: (0 if n == k else 2) for n in range(1, 32)}, {n: n for n in range(1, 32)}):
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                ou, oc, olab, _ = O.sample_disp_kmer(cons, k, radius_of_len, u, c, n_total_sample=10 ** 12, revcom_mode=revcom_mode)
            lab, u2 = M.label_table(u, k, [int(O.kmer2hash(s)) for s in cons], [len(s) for s in cons],
                                    [radius_of_len[len(s)] for s in cons], radius_of_len[k], revcom_mode)
            np.testing.assert_array_equal(lab, olab)
            np.testing.assert_array_equal(u2, ou.astype(np.int64))
            w, m = M.label_sums(lab, c, k, len(cons) + 1)
            assert w == [int(x) for x in np.bincount(olab, weights=c, minlength=len(cons) + 1)]
            assert m == [int(x) for x in np.bincount(olab, minlength=len(cons) + 1)]
            for l in range(len(cons) + 1):
                np.testing.assert_array_equal(M.members_of(lab, l), np.where(olab == l)[0])


@pytest.mark.parametrize("k", KS)
def test_ball_members_and_cnt_mat_vs_oracle(O, k):
    rng, u, c = _table(O, k, 30 + k)
    cons = _canon(O, u[len(u) // 3], k)
    for r, rc in ((-1, True), (0, True), (1, True), (k // 2, False), (k // 2, True), (k, True), (k + 1, False)):
        ou, oc = O.ex_hamball(u, c, k, cons, r, rc)
        mu, mc = M.ball_members(u, c, k, cons, r, rc)
        np.testing.assert_array_equal(mu, ou.astype(np.int64))
        np.testing.assert_array_equal(mc, oc)
        assert M.cnt_mat(mu, mc, k) == O.cal_cnt_mat(ou, oc, k).tolist()
    assert M.cnt_mat(u, c, k) == O.cal_cnt_mat(u, c, k).tolist()


def test_cdf_hits():
    w = np.array([3, 0, 1, 0, 0, 5, 2 ** 32 - 1, 3 * 10 ** 9, 1], np.int64)
    cdf = [int(x) for x in np.cumsum(w)]
    t = sorted({max(0, b + d) for b in [0] + cdf for d in (-1, 0, 1)})
    want = [next((i for i, e in enumerate(cdf) if e > x), len(w)) for x in t]     # first entry whose inclusive prefix exceeds x
    np.testing.assert_array_equal(M.cdf_hits(w, t), want)
    np.testing.assert_array_equal(M.cdf_hits(w.astype(np.uint32), t), want)
    assert list(M.cdf_hits(w, [cdf[-1] - 1, cdf[-1]])) == [len(w) - 1, len(w)]
