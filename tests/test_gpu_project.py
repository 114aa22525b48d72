"""project_kmers on the GPU against a numpy oracle written out here: np.lexsort for the selection, integer numpy for the query
sums (Sref built from the distance matrix and an injected neighbour table, natural diagonal and label rule included), float64 for
the start and the descent.  Reference sets and their maps: tests/golden/project_maps.npz (gen_golden_project.py)."""
import functools
import hashlib
import pickle
import shutil
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
GOLD = Path(__file__).resolve().parent / "golden"
N_NB, M, LR = 20, 70, 0.01
TAGS = ["k8n300", "k16n300", "k8n1100", "k16n1100"]
# special queries (rows of every case's query set)
Q_EQUAL, Q_REVCOM, Q_PALINDROME, Q_TIE, Q_CROWDED = 0, 1, 2, 3, 4


# ---- the oracle ----------------------------------------------------------------------------------------
def _rc(kh, k):
    kh = np.asarray(kh, np.uint64)
    out = np.zeros_like(kh)
    for p in range(k):
        out = (out << np.uint64(2)) | (np.uint64(3) - ((kh >> np.uint64(2 * p)) & np.uint64(3)))
    return out


def _ham(a, b, k, first=None):
    """mismatching bases of every pair, over all k bases or the first `first` ones -> int64 [len(a), len(b)]"""
    x = np.asarray(a, np.uint64)[:, None] ^ np.asarray(b, np.uint64)[None, :]
    d = np.zeros(x.shape, np.int64)
    for p in range(k if first is None else first):
        d += ((x >> np.uint64(2 * (k - 1 - p))) & np.uint64(3)) != 0
    return d


def oracle_knn(q, ref, k, n_nb, revcom_mode=True):
    """steps 1 - 2 -> (oriented hashes, nb, nb_dist, flipped, the distance rows of the chosen strand)"""
    q = np.asarray(q, np.uint64)
    qr = _rc(q, k)
    Df, Dr = _ham(q, ref, k), _ham(qr, ref, k)
    flip = (Dr.min(axis=1) < Df.min(axis=1)) if revcom_mode else np.zeros(len(q), bool)
    D = np.where(flip[:, None], Dr, Df)
    idx = np.broadcast_to(np.arange(len(ref)), D.shape)
    nb = np.lexsort((idx, D), axis=1)[:, :n_nb]                   # smallest (distance, index) pairs, in that order
    return np.where(flip, qr, q), nb.astype(np.int32), np.take_along_axis(D, nb, 1).astype(np.uint8), flip, D


def oracle_ref_matrix(ref, lab, clens, k):
    """the Hamming matrix of the reference set: pairs that share a label whose consensus is shorter than k are compared on its
    first clen bases only"""
    D = _ham(ref, ref, k)
    for l, clen in enumerate(clens):
        if clen < k:
            both = (lab[:, None] == l) & (lab[None, :] == l)
            D = np.where(both, _ham(ref, ref, k, first=int(clen)), D)
    return D


def oracle_sref(Dref, nbr):
    """Sref[i][j] = sum_ii sum_jj D[nbr[i][ii], nbr[j][jj]], diagonal included (the natural diagonal)"""
    n = len(Dref)
    W = np.zeros((n, n), np.float64)                               # small integers: the float64 products and sums are exact
    np.add.at(W, (np.repeat(np.arange(n), nbr.shape[1]), nbr.ravel()), 1)
    S = W @ Dref.astype(np.float64) @ W.T
    assert S.max() < 2 ** 53 and (S == np.rint(S)).all()
    return S.astype(np.int64)


def oracle_descend(p, nb, xy, n_iter, lr, dt):
    """steps 5 - 6 in dtype dt.  float64: the oracle.  float32: the restatement, every sum a j-ascending cumsum."""
    def total(a):
        return np.cumsum(a, axis=1, dtype=dt)[:, -1] if dt is np.float32 else a.sum(axis=1)
    p, xy, lr, one = p.astype(dt), xy.astype(dt), dt(lr), dt(1)
    lo, hi = dt(1e-3), one - dt(1e-3)
    w = np.take_along_axis(p, nb.astype(np.int64), 1)
    sw = total(w)
    yx, yy = total(w * xy[0][nb]) / sw, total(w * xy[1][nb]) / sw
    for _ in range(n_iter):
        dx, dy = yx[:, None] - xy[0][None, :], yy[:, None] - xy[1][None, :]
        q = one / (one + (dx * dx + dy * dy))
        q = np.clip(q, lo, hi)
        T = q / (one - q) * (p - q)
        yx = yx - lr * (dt(4) * total(T * dx))
        yy = yy - lr * (dt(4) * total(T * dy))
        assert yx.dtype == dt and T.dtype == dt
    return np.stack([yx, yy])


# ---- the cases -------------------------------------------------------------------------------------------
def _hash_of(bases):
    h = 0
    for b in bases:
        h = (h << 2) | int(b)
    return h


@functools.lru_cache(maxsize=None)
def case(tag):
    """reference set, map, queries and every oracle quantity of a case; computed once, shared, never modified"""
    from kmap_amd.kmer_count import get_hash_dtype
    from kmap_amd.projection import hd_prob_lut_projected
    g = np.load(GOLD / "project_maps.npz")
    k = int(tag[1:tag.index("n")])
    ref = np.repeat(g[f"{tag}_kh"], g[f"{tag}_cnts"])
    lab = np.repeat(g[f"{tag}_label"], g[f"{tag}_cnts"]).astype(np.int32)
    clens, xy = g[f"{tag}_clens"], g[f"{tag}_xy"]
    n = len(ref)
    assert n == int(tag[tag.index("n") + 1:]) and xy.shape == (2, n) and (g[f"{tag}_cnts"] > 1).any() and clens[1] < k
    rng = np.random.default_rng(1000 + n + k)
    rand = lambda: int(rng.integers(0, 4 ** k))                    # noqa: E731
    once = np.flatnonzero(np.repeat(g[f"{tag}_cnts"], g[f"{tag}_cnts"]) == 1)
    noise_once = [int(i) for i in once if lab[i] == 2]
    q = [0] * 5
    q[Q_EQUAL] = int(ref[noise_once[0]])                           # replaced below by a k-mer whose float64 projection is at home
    # the reverse complement of a reference whose own strand is absent from the set: d_r = 0 < d_f
    i_rc = next(i for i in noise_once[1:] if _ham(_rc(ref[i:i + 1], k), ref, k).min() > 0)
    q[Q_REVCOM] = int(_rc(ref[i_rc:i_rc + 1], k)[0])
    half = rng.integers(0, 4, size=k // 2)
    q[Q_PALINDROME] = _hash_of(list(half) + [3 - b for b in half[::-1]])
    while True:                                                    # forward and reverse minima tie, not a palindrome
        c = np.array([rand()], np.uint64)
        if _rc(c, k)[0] != c[0] and _ham(c, ref, k).min() == _ham(_rc(c, k), ref, k).min():
            q[Q_TIE] = int(c[0])
            break
    while True:                                                    # more references at the threshold distance than places left
        c = np.array([rand()], np.uint64)
        d = np.sort(oracle_knn(c, ref, k, N_NB)[4][0])
        if d[N_NB] == d[N_NB - 1] and d[0] < d[N_NB - 1]:
            q[Q_CROWDED] = int(c[0])
            break
    for i in rng.choice(np.flatnonzero(lab < 2), size=25, replace=False):   # near the motif clusters: one base changed
        q.append(int(ref[i]) ^ (int(rng.integers(1, 4)) << (2 * int(rng.integers(0, k)))))
    for i in rng.choice(n, size=10, replace=False):                          # reverse strands of references
        q.append(int(_rc(ref[i:i + 1], k)[0]))
    q += [rand() for _ in range(M - len(q))]
    q = np.array(q, np.uint64)
    assert len(q) == M
    Dref = oracle_ref_matrix(ref, lab, clens, k)
    nbr = np.argsort(Dref, axis=1, kind="stable")[:, :N_NB].astype(np.int32)   # the injected reference neighbour table
    Sref = oracle_sref(Dref, nbr)
    lut3 = hd_prob_lut_projected(k, N_NB)
    # Q_EQUAL: a k-mer that is on the map once.  The float64 oracle decides which one: the first (in index order) that it places
    # within 0.25 map units of its own point after 50 iterations, on a trajectory the float32 restatement follows to 1e-3 -- a noise
    # k-mer's neighbours are scattered over the map, and so is their weighted mean
    cand = np.array([int(i) for i in once if lab[i] < 2])
    _, c_nb, _, c_flip, _ = oracle_knn(ref[cand], ref, k, N_NB)
    c_p = lut3[Sref[c_nb].sum(axis=1)]
    y64, y32 = (oracle_descend(c_p, c_nb, xy, 50, LR, dt) for dt in (np.float64, np.float32))
    home = np.hypot(*(y64 - xy[:, cand].astype(np.float64)))
    ok = (home < 0.25) & (np.abs(y32 - y64).max(axis=0) < 1e-3) & ~c_flip & (c_nb[:, 0] == cand)
    i_equal = int(cand[np.flatnonzero(ok)[0]]) if ok.any() else int(cand[0])     # the property is asserted at N = 300 only
    q[Q_EQUAL] = int(ref[i_equal])
    kh, nb, nb_dist, flip, Drows = oracle_knn(q, ref, k, N_NB)
    Q = Sref[nb].sum(axis=1)
    dt = get_hash_dtype(k)
    out = dict(k=k, n=n, ref=ref.astype(dt), lab=lab, clens=clens, xy=xy, q=q.astype(dt), kh=kh.astype(dt), nb=nb, nb_dist=nb_dist,
               flip=flip, Drows=Drows, nbr=nbr, Sref=Sref, Q=Q.astype(np.uint32), p=lut3[Q], i_equal=i_equal)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def _project(c, **kw):
    from kmap_amd.projection import project_kmers
    return project_kmers(c["q"], c["ref"], c["lab"], c["clens"], c["xy"], c["k"], n_neighbour=N_NB, learning_rate=LR,
                         ref_neighbours=c["nbr"], **kw)


# ---- selection ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", TAGS)
def test_selection_exact(tag):
    from kmap_amd.projection import project_knn
    c = case(tag)
    k, flip, D = c["k"], c["flip"], c["Drows"]
    # the inputs are the ones the issue names
    assert c["nb_dist"][Q_EQUAL, 0] == 0 and not flip[Q_EQUAL]
    assert flip[Q_REVCOM] and c["nb_dist"][Q_REVCOM, 0] == 0
    assert _rc(c["q"][Q_PALINDROME:Q_PALINDROME + 1], k)[0] == c["q"][Q_PALINDROME] and not flip[Q_PALINDROME]
    assert not flip[Q_TIE] and _ham(_rc(c["q"][Q_TIE:Q_TIE + 1], k), c["ref"], k).min() == D[Q_TIE].min()
    t = c["nb_dist"][Q_CROWDED, -1]
    assert (D[Q_CROWDED] == t).sum() > (c["nb_dist"][Q_CROWDED] == t).sum()
    assert flip.sum() >= 5 and (~flip).sum() >= 5
    kh, nb, nb_dist, flipped = project_knn(c["q"], c["ref"], k, N_NB, revcom_mode=True)
    assert nb.dtype == np.int32 and nb_dist.dtype == np.uint8 and kh.dtype == c["q"].dtype
    np.testing.assert_array_equal(flipped, flip)
    np.testing.assert_array_equal(kh, c["kh"])
    np.testing.assert_array_equal(nb_dist, c["nb_dist"])
    np.testing.assert_array_equal(nb, c["nb"])


@pytest.mark.parametrize("tag", ["k8n300", "k16n1100"])
def test_selection_without_revcom_never_flips(tag):
    from kmap_amd.projection import project_knn
    c = case(tag)
    want_kh, want_nb, want_dist, want_flip, _ = oracle_knn(c["q"], c["ref"], c["k"], N_NB, revcom_mode=False)
    kh, nb, nb_dist, flipped = project_knn(c["q"], c["ref"], c["k"], N_NB, revcom_mode=False)
    assert not flipped.any() and not want_flip.any()
    np.testing.assert_array_equal(kh, c["q"])
    np.testing.assert_array_equal(nb, want_nb)
    np.testing.assert_array_equal(nb_dist, want_dist)


@pytest.mark.parametrize("tag", ["k8n300", "k16n300"])
def test_selection_edges(tag):
    from kmap_amd.projection import project_knn
    c = case(tag)
    k, ref = c["k"], c["ref"]
    # N == n_nb: every reference is a neighbour, in (distance, index) order
    want = oracle_knn(c["q"], ref[:N_NB], k, N_NB)
    kh, nb, nb_dist, flipped = project_knn(c["q"], ref[:N_NB], k, N_NB)
    np.testing.assert_array_equal(nb, want[1])
    np.testing.assert_array_equal(nb_dist, want[2])
    np.testing.assert_array_equal(flipped, want[3])
    assert (np.sort(nb, axis=1) == np.arange(N_NB)).all()
    with pytest.raises(ValueError):
        project_knn(c["q"], ref[:N_NB - 1], k, N_NB)
    with pytest.raises(ValueError):
        project_knn(c["q"], ref, k, 65)
    with pytest.raises(ValueError):
        _project(dict(c, ref=ref[:N_NB - 1], lab=c["lab"][:N_NB - 1], xy=c["xy"][:, :N_NB - 1], nbr=c["nbr"][:N_NB - 1]), n_iter=0)
    # the library itself refuses what the Python layer refuses (bad arguments are status codes, never faults)
    from kmap_amd import _ffi
    fn = _ffi.lib().kmap_project_knn_u32_dev if ref.dtype == np.uint32 else _ffi.lib().kmap_project_knn_u64_dev
    for m_, n_, k_, nn_ in ((1, 19, k, 20), (1, 300, k, 65), (1, 300, 0, 20), (1, 300, 32, 20), (-1, 300, k, 20), (1, 0, k, 20)):
        assert fn(None, m_, None, n_, k_, 1, nn_, None, None, None, None) == -1, (m_, n_, k_, nn_)
        assert _ffi.last_error()
    assert fn(None, 0, None, 300, k, 1, 20, None, None, None, None) == 0            # M = 0: a no-op
    # M = 0 returns empty arrays
    kh, nb, nb_dist, flipped = project_knn(c["q"][:0], ref, k, N_NB)
    assert kh.shape == (0,) and nb.shape == (0, N_NB) and nb_dist.shape == (0, N_NB) and flipped.shape == (0,)
    pr = _project(dict(c, q=c["q"][:0]), n_iter=5)
    assert pr.xy.shape == (2, 0) and pr.xy.dtype == np.float32 and pr.nb.shape == (0, N_NB)


# ---- sums and probabilities -----------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["k8n300", "k16n300", "k16n1100"])
def test_sums_and_p_exact(tag):
    """Q against the integer oracle and p bit for bit against LUT3[Q], over plain and over de-duplicated sums rows"""
    from kmap_amd.projection import hd_prob_lut_projected, project_rows
    from kmap_amd.visualization import dedupe_sums_rows, sums_rows_from_kmers
    c = case(tag)
    k, n = c["k"], c["n"]
    lut3 = hd_prob_lut_projected(k, N_NB)
    assert c["Sref"].max() <= N_NB * N_NB * k and c["Q"].max() < len(lut3)
    assert (np.diag(c["Sref"]) > 0).any()                          # the natural diagonal, not the reference's zero
    if k == 16:
        assert c["Q"].max() > 65535                                # indices that a uint16 sum could not hold
    sums_d, lds = sums_rows_from_kmers(c["ref"], c["lab"], k, [int(v) for v in c["clens"]], N_NB, c["nbr"], natural_diag=True,
                                       matrix_fallback=False)
    rowmap_d = None
    try:
        got = sums_d.to_numpy(np.uint16, (n, lds))[:, :n]
        np.testing.assert_array_equal(got, c["Sref"])              # the rows the projection adds up
        xy, Q, P, _ = project_rows(c["nb"], sums_d, lds, n, lut3, c["xy"], 0, LR, keep_q=True, keep_p=True)
        np.testing.assert_array_equal(Q, c["Q"])
        np.testing.assert_array_equal(P.view(np.uint32), c["p"].view(np.uint32))
        sums_d, rowmap_d, stored = dedupe_sums_rows(sums_d, n, lds, n=n)
        assert rowmap_d is not None and stored < n                 # the repeated k-mers' rows are stored once
        xy2, Q2, P2, _ = project_rows(c["nb"], sums_d, lds, n, lut3, c["xy"], 0, LR, rowmap_d=rowmap_d, src_rows=stored, keep_q=True,
                                      keep_p=True)
        np.testing.assert_array_equal(Q2, c["Q"])
        np.testing.assert_array_equal(P2.view(np.uint32), c["p"].view(np.uint32))
        np.testing.assert_array_equal(xy2.view(np.uint32), xy.view(np.uint32))
    finally:
        sums_d.free()
        if rowmap_d is not None:
            rowmap_d.free()
    pr = _project(c, n_iter=0, keep_q=True)                        # the public entry point takes the same route
    np.testing.assert_array_equal(pr.Q, c["Q"])
    np.testing.assert_array_equal(pr.nb, c["nb"])


def test_unsupported_reference_set_is_refused():
    """where the profile kernel does not build Sref (k > 16) the projection says so instead of using the zero-diagonal sums"""
    from kmap_amd.projection import project_kmers
    rng = np.random.default_rng(3)
    ref = rng.integers(0, 4 ** 17, size=64).astype(np.uint64)
    with pytest.raises(ValueError, match="k <= 16"):
        project_kmers(ref[:3], ref, np.zeros(64, np.int32), [17], np.zeros((2, 64), np.float32), 17, n_neighbour=N_NB, n_iter=1,
                      ref_neighbours=np.tile(np.arange(N_NB, dtype=np.int32), (64, 1)))


# ---- start and descent --------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def descent_oracle(tag, n_iter):
    c = case(tag)
    want = oracle_descend(c["p"], c["nb"], c["xy"], n_iter, LR, np.float64)
    f32 = oracle_descend(c["p"], c["nb"], c["xy"], n_iter, LR, np.float32)
    e32 = np.abs(f32.astype(np.float64) - want).max(axis=0)        # per query
    for a in (want, e32):
        a.setflags(write=False)
    return want, float(e32.max()), e32


@pytest.mark.parametrize("n_iter", [0, 1, 50])
@pytest.mark.parametrize("tag", ["k8n300", "k16n1100"])
def test_start_and_descent_against_float64(tag, n_iter):
    """Allowed device error per coordinate: 4 x the largest |float32 restatement - float64| of the case (the factor is for the freer
    summation order), at least 4 ulp of the coordinate.  At n_iter = 50 some trajectories are not contractive (a query that comes
    within a few hundredths of an anchor it is not drawn to is thrown out again by q / (1 - q) = 999, in a direction the last bits
    decide) and the restatement itself leaves the oracle by whole map units, which makes the case-wide bound wide; the queries
    whose restatement follows the oracle to 1e-4 (a tenth of the 3-decimal file format) are therefore held to the same rule among
    themselves.  Measured on an MI355X (restatement error / device error): DESIGN.md section 10."""
    c = case(tag)
    want, e32, e32_q = descent_oracle(tag, n_iter)
    got = _project(c, n_iter=n_iter).xy
    assert got.dtype == np.float32 and got.shape == (2, M)
    err = np.abs(got.astype(np.float64) - want)
    tol = np.maximum(4 * e32, 4 * np.spacing(np.abs(want).astype(np.float32)).astype(np.float64))
    print(f"project descent {tag} n_iter={n_iter}: restatement error {e32:.3e}, device error {err.max():.3e}, "
          f"allowed {tol.min():.3e} .. {tol.max():.3e}, |y| <= {np.abs(want).max():.3f}")
    follows = e32_q <= 1e-4                                        # queries whose restatement follows the oracle
    print(f"    queries the restatement follows to 1e-4: {follows.sum()} of {M}: restatement error {e32_q[follows].max():.3e}, "
          f"device error {err[:, follows].max():.3e}; the others: restatement {e32_q[~follows].max() if (~follows).any() else 0:.3e}, "
          f"device {err[:, ~follows].max() if (~follows).any() else 0:.3e}")
    assert np.isfinite(got).all()
    assert (err <= tol).all(), (float(err.max()), e32)
    assert follows.sum() >= M // 3
    tol_f = np.maximum(4 * e32_q[follows].max(), 4 * np.spacing(np.abs(want[:, follows]).astype(np.float32)).astype(np.float64))
    assert (err[:, follows] <= tol_f).all(), (float(err[:, follows].max()), float(e32_q[follows].max()))


def test_query_equal_to_a_reference_lands_on_its_anchor():
    """a k-mer that is on the map once is placed within 0.5 map units of its own point (N = 300)"""
    c = case("k8n300")
    anchor = c["xy"][:, c["i_equal"]].astype(np.float64)
    assert c["nb"][Q_EQUAL, 0] == c["i_equal"] and c["nb_dist"][Q_EQUAL, 0] == 0
    want = descent_oracle("k8n300", 50)[0]
    assert np.hypot(*(want[:, Q_EQUAL] - anchor)) < 0.5            # the oracle itself: the input is a fair one
    got = _project(c, n_iter=50).xy
    assert np.hypot(*(got[:, Q_EQUAL].astype(np.float64) - anchor)) < 0.5


def test_row_blocks_do_not_change_a_bit():
    c = case("k8n1100")
    one = _project(c, n_iter=50, keep_q=True)
    blocked = _project(c, n_iter=50, keep_q=True, byte_budget=32 * c["n"] * 4)
    assert blocked.block_rows == 32 and one.block_rows >= M
    np.testing.assert_array_equal(blocked.nb, one.nb)
    np.testing.assert_array_equal(blocked.Q, one.Q)
    np.testing.assert_array_equal(blocked.xy.view(np.uint32), one.xy.view(np.uint32))
    np.testing.assert_array_equal(one.Q, c["Q"])


# ---- end to end ---------------------------------------------------------------------------------------------------
def _digest(root):
    return {str(p.relative_to(root)): hashlib.sha256(p.read_bytes()).hexdigest() for p in sorted(root.rglob("*")) if p.is_file()}


def test_project_kmers_on_the_testfa_pipeline(tmp_path, golden):
    """preproc -> scan_motif -> visualize_kmers of tests/test.fa with the reference run's config (60 iterations, the neighbour table
    of that run injected), then 12 k-mers projected onto the map through the verb's entry point"""
    from kmap_amd._toml import dump_toml, load_toml
    from kmap_amd.kmer_count import _preproc, hashes2kmers
    from kmap_amd.motif_discovery import _scan_motif
    from kmap_amd.projection import _project_kmers
    from kmap_amd.visualization import _visualize_kmers
    u = golden("umap_n300.npz")
    fa = tmp_path / "test.fa"
    shutil.copyfile(GOLD / "test.fa", fa)
    res = tmp_path / "res"
    res.mkdir()
    cfg = load_toml(GOLD / "scan_testfa" / "config.toml")
    cfg["general"]["input_fasta_file"] = str(fa)
    cfg["general"]["res_dir"] = str(res)
    assert cfg["visualization"]["n_max_iter"] == 60
    dump_toml(cfg, res / "config.toml")
    _preproc(str(fa), str(res))
    np.random.seed(123)
    _scan_motif(str(res))
    _visualize_kmers(str(res), neighbor_inds_mat=u["nb"])
    with open(res / "sample_kmers.pkl", "rb") as fh:
        samp_kh, samp_cnts, samp_label, conseqs = pickle.load(fh)
    k = max(len(s) for s in conseqs)
    ref = np.repeat(np.asarray(samp_kh), samp_cnts)
    lab = np.repeat(np.asarray(samp_label), samp_cnts)
    kmers = hashes2kmers(np.asarray(samp_kh), k).tolist()
    rng = np.random.default_rng(12)
    rc = {"A": "T", "C": "G", "G": "C", "T": "A"}
    mutate = lambda s, p: s[:p] + rc[s[p]] + s[p + 1:]             # noqa: E731
    given = [kmers[0], kmers[5].lower(), "".join(rc[b] for b in reversed(kmers[9])), mutate(kmers[20], 3), mutate(kmers[-1], k - 1),
             "".join(rc[b] for b in reversed(mutate(kmers[40], 0))), conseqs[0]]
    given += ["".join("ACGT"[b] for b in rng.integers(0, 4, size=k)) for _ in range(12 - len(given))]
    qfile = tmp_path / "queries.txt"
    qfile.write_text("\n".join(given[:6]) + "\n\n" + "\n".join(given[6:]) + "\n")
    before = _digest(res)
    pr = _project_kmers(str(res), str(qfile), None, 20)
    after = _digest(res)
    assert set(after) - set(before) == {"projected_kmers.tsv"}
    assert {f: h for f, h in after.items() if f != "projected_kmers.tsv"} == before   # low_dim_data.tsv and everything else untouched
    rows = (res / "projected_kmers.tsv").read_text().splitlines()
    assert rows[0] == "kmer\tx\ty\tnearest_label\tmin_ham_dist\tflipped" and len(rows) == 13
    from kmap_amd.kmer_count import kmer2hash
    q = np.array([int(kmer2hash(s.upper())) for s in given], np.uint64)
    _, nb, nb_dist, flip, _ = oracle_knn(q, ref, k, cfg["visualization"]["n_neighbour"], revcom_mode=cfg["kmer_count"]["revcom_mode"])
    assert flip[2] and not flip[0] and nb_dist[0, 0] == 0 and nb_dist[3, 0] <= 1
    np.testing.assert_array_equal(pr.nb, nb)
    for i, row in enumerate(rows[1:]):
        f = row.split("\t")
        assert len(f) == 6 and f[0] == given[i]
        for v, want in ((f[1], pr.xy[0, i]), (f[2], pr.xy[1, i])):
            assert v == f"{want:3.3f}" and np.isfinite(float(v))
        assert (int(f[3]), int(f[4]), int(f[5])) == (int(lab[nb[i, 0]]), int(nb_dist[i, 0]), int(flip[i]))
    out2 = tmp_path / "elsewhere.tsv"                               # --output_file
    _project_kmers(str(res), str(qfile), str(out2), 20)
    assert out2.read_text().splitlines() == rows and _digest(res) == after
