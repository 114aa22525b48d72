"""motif_cooccurrence on the GPU (csrc/pwm_presence.hip, csrc/bit_pairs.hip).  The yardstick is never the
new kernels: it is tests/_cooccurrence_model.py (per read the best score of tests/_readscore_model.py, thresholded, packed 64 per
word; the pair counts as a matrix product of the bits; the statistic pair by pair), and as a second witness the per-matrix device
path DeviceSeq.read_scores(...).fetch() thresholded and packed on the host.  Planes and counts are compared as equal integers; the
verb's tables field by field with the run on the model."""
from pathlib import Path

import numpy as np
import pytest

from tests import _cooccurrence_model as CM
from tests import _readscore_model as M
from tests import _sites_model as S
from tests._batch_model import batches
from tests._refine_model import asym_matrix, make_reads, window_scores

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
LIB = ROOT / "tests" / "golden" / "library"

# eleven random matrices and an all-zero one.  By width the eight narrow ones fill a batch (the 8-matrix limit cuts), three of the
# four 31-column ones fill the next (the 24-chunk limit cuts), the fourth is alone.
WIDTHS = (4, 9, 16, 31, 31, 31, 31, 5, 6, 7, 12)


@pytest.fixture(scope="module")
def geometry():
    """tests/test_gpu_sites.py's read geometry, built anew: ~3000 reads on under 40 000 positions (fixed seed), lengths 0 .. 30 at
    random and w - 1, w, w + 1 of every width used, one read of 2100 bases that spans a wave tile, 1200 reads of one base in a run,
    2 % invalid bases, n no multiple of 16 -- and n_seq no multiple of 64, so the last word of a row is partial.  The model's
    window scores per matrix are computed once."""
    from kmap_amd.motif_discovery import DeviceSeq
    rng = np.random.default_rng(2010)
    lengths = [int(x) for x in rng.integers(0, 31, 600)] + [0, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 15, 16, 17, 30, 31, 32, 0]
    i_long = len(lengths)
    lengths += [2100] + [1] * 1200 + [int(x) for x in rng.integers(0, 31, 1150)] + [31] * 8 + [7, 8, 9, 33]
    if len(lengths) % 64 == 0:
        lengths.append(5)
    if (sum(lengths) + len(lengths) - 1) % 16 == 0:
        lengths[-1] += 1
    seq, borders = make_reads(lengths, rng, frac_invalid=0.02, last_separator=False)
    n = len(seq)
    assert 2900 < len(borders) < 3100 and n < 40_000 and n % 16 != 0 and len(borders) % 64 != 0
    first_tile, last_tile = borders[i_long, 0] // 1024 + 1, (borders[i_long, 1] - 1) // 1024 - 1
    assert last_tile >= first_tile and not ((borders[:, 0] >= first_tile * 1024) & (borders[:, 0] < (first_tile + 1) * 1024)).any()
    closed = batches(WIDTHS + (8,))
    assert [c[1] for c in closed] == ["matrices", "chunks", "end"] and [c[0] for c in closed] == [8, 3, 1]
    mats = [asym_matrix(w, rng) for w in WIDTHS] + [np.zeros((4, 8), np.int32)]
    scored = [window_scores(seq, W) for W in mats]
    ds = DeviceSeq(seq, borders)
    yield ds, seq, borders, mats, scored
    ds.close()


def fetch_and_close(planes):
    try:
        return planes.fetch(), planes.n_present.copy(), planes.pair_counts()
    finally:
        planes.close()


def check_planes(got, n_present, bits):
    n_seq = bits.shape[1]
    assert got.dtype == np.uint64 and got.shape == (len(bits), (n_seq + 63) // 64)
    np.testing.assert_array_equal(got, CM.np_pack(bits))
    assert n_present.dtype == np.int64
    np.testing.assert_array_equal(n_present, bits.sum(axis=1))
    np.testing.assert_array_equal(n_present, CM.np_unpack(got).sum(axis=1))       # the row popcounts, tail included
    if n_seq % 64 and len(bits):
        assert not (got[:, -1] >> np.uint64(n_seq % 64)).any()                     # the bits behind n_seq are zero


@pytest.mark.parametrize("revcom", [True, False])
def test_presence_planes_and_pair_counts(geometry, revcom):
    from kmap_amd.pwm import pwm_threshold
    ds, seq, borders, mats, scored = geometry
    ts = [pwm_threshold(W, 1e-2)[0] for W in mats[:-1]] + [0]
    bits = CM.np_presence(seq, borders, mats, ts, revcom, scored)
    planes = ds.library_presence(mats, ts, revcom)
    assert (planes.n_mat, planes.n_seq, planes.n_words) == (12, len(borders), (len(borders) + 63) // 64)
    got, n_present, pairs = fetch_and_close(planes)
    check_planes(got, n_present, bits)
    assert n_present[0] > 100 and n_present[-1] > 100 and 0 < n_present[3] < n_present[0]
    assert pairs.dtype == np.int64
    np.testing.assert_array_equal(pairs, CM.np_pair_counts(bits))
    np.testing.assert_array_equal(np.diagonal(pairs), n_present)
    # the caller's order does not matter: a permutation permutes the rows
    perm = np.random.default_rng(2011).permutation(12)
    got_p, n_p, pairs_p = fetch_and_close(ds.library_presence([mats[i] for i in perm], [ts[i] for i in perm], revcom))
    np.testing.assert_array_equal(got_p, got[perm])
    np.testing.assert_array_equal(pairs_p, pairs[np.ix_(perm, perm)])
    # and two calls give the same bits
    np.testing.assert_array_equal(fetch_and_close(ds.library_presence(mats, ts, revcom))[0], got)


@pytest.mark.parametrize("revcom", [True, False])
def test_threshold_edges(geometry, revcom):
    """per matrix: the smallest score (present = scorable), a read's best score exactly (inclusive) and one above it, the largest
    score + 1 (an empty row), and the lowest threshold there is (a read without a valid window stays absent)"""
    ds, seq, borders, mats, scored = geometry
    Ws, ts, pick = [], [], []
    for W, sc in zip(mats, scored):
        lo, hi = M.score_range(W)
        score, loc, _ = M.np_read_scores(seq, borders, W, revcom, sc)
        scorable = np.nonzero(loc >= 0)[0]
        r = int(scorable[np.argsort(score[scorable], kind="stable")[len(scorable) // 2]])      # a read with the median best score
        pick.append((r, int(score[r])))
        Ws += [W] * 5
        ts += [lo, int(score[r]), int(score[r]) + 1, hi + 1, -2 ** 31]
    bits = CM.np_presence(seq, borders, Ws, ts, revcom, [sc for sc in scored for _ in range(5)])
    got, n_present, _ = fetch_and_close(ds.library_presence(Ws, ts, revcom))
    check_planes(got, n_present, bits)
    _, _, n_scored = ds.library_histograms(mats, [M.score_range(W)[0] for W in mats], [1] * len(mats), revcom)
    np.testing.assert_array_equal(n_present[0::5], n_scored)
    np.testing.assert_array_equal(n_present[4::5], n_scored)
    np.testing.assert_array_equal(got[0::5], got[4::5])
    assert not n_present[3::5].any() and not got[3::5].any()
    unpacked = CM.np_unpack(got, len(borders))
    for m, (r, s) in enumerate(pick):
        assert unpacked[5 * m + 1, r] and not unpacked[5 * m + 2, r]
        assert n_present[5 * m + 2] < n_present[5 * m + 1] <= n_present[5 * m]
    assert (n_scored < len(borders)).all() and n_scored[0] > n_scored[3]         # unscorable reads exist under every matrix


def test_against_the_per_matrix_device_path(geometry):
    from kmap_amd.pwm import pwm_threshold
    ds, seq, borders, mats, _ = geometry
    idx = (0, 2, 3, 11)
    ts = {0: pwm_threshold(mats[0], 1e-2)[0], 2: M.score_range(mats[2])[0], 3: pwm_threshold(mats[3], 1e-2)[0], 11: 0}
    got, n_present, _ = fetch_and_close(ds.library_presence([mats[m] for m in idx], [ts[m] for m in idx], True))
    for row, m in enumerate(idx):
        rs = ds.read_scores(mats[m], True)
        try:
            score, loc, _ = rs.fetch()
        finally:
            rs.close()
        flags = (loc >= 0) & (score.astype(np.int64) >= ts[m])
        np.testing.assert_array_equal(got[row], CM.np_pack(flags[None, :])[0])
        assert n_present[row] == flags.sum() > 0


def test_degenerate_sizes_and_errors(geometry):
    from kmap_amd import _ffi
    from kmap_amd.motif_discovery import DeviceSeq
    ds, seq, borders, mats, scored = geometry
    lib = _ffi.lib()
    W = mats[1]
    t = M.score_range(W)[0]
    empty = ds.library_presence([], [], True)
    assert (empty.n_mat, empty.n_words) == (0, (ds.n_seq + 63) // 64) and empty.n_present.shape == (0,)
    assert empty.fetch().shape == (0, empty.n_words) and empty.pair_counts().shape == (0, 0)
    empty.close()
    n_words = (ds.n_seq + 63) // 64
    buf = _ffi.DeviceBuffer(2 * n_words * 8)

    def call(widths, weights, n=ds.n, n_seq=ds.n_seq, words=n_words, codes=ds.codes.ptr, planes=buf.ptr, n_mat=None):
        wd, thr = np.array(widths, np.int32), np.array([t, t], np.int32)
        present = np.full(2, -5, np.int64)
        rc = lib.kmap_presence_library_dev(codes, ds.inval_orig.ptr, n, ds.borders.ptr, n_seq, len(widths) if n_mat is None else n_mat,
                                           _ffi.ptr(wd), weights, _ffi.ptr(thr), 1, planes, words, _ffi.ptr(present), None)
        return rc, present
    grid = np.zeros((2, 4, 32), np.int32)
    grid[:, :, :9] = W
    try:
        rc, present = call([9, 9], _ffi.ptr(grid))
        want = CM.np_presence(seq, borders, [W, W], [t, t], True, [scored[1]] * 2)
        assert rc == 0
        check_planes(buf.to_numpy(np.uint64, (2, n_words)), present, want)
        # no matrix: nothing is written; no read: rows without words; no position: zero rows
        buf.zero()
        _ffi.sync()
        rc, present = call([9, 9], _ffi.ptr(grid), n_mat=0)
        assert rc == 0 and (present == -5).all()
        rc, present = call([9, 9], _ffi.ptr(grid), n_seq=0, words=0)
        assert rc == 0 and not present.any()
        check_planes(buf.to_numpy(np.uint64, (2, n_words)), np.zeros(2, np.int64), np.zeros_like(want))
        rc, present = call([9, 9], _ffi.ptr(grid))
        assert rc == 0 and present.all()
        rc, present = call([9, 9], _ffi.ptr(grid), n=0)
        assert rc == 0 and not present.any() and not buf.to_numpy(np.uint64, (2, n_words)).any()
        # n_words other than (n_seq + 63) / 64, width 3 and 32, a weight behind the width or too large, null arrays, negative sizes
        for words in (n_words - 1, n_words + 1, 0):
            rc, present = call([9, 9], _ffi.ptr(grid), words=words)
            assert rc == -1 and "presence_library" in _ffi.last_error() and "words" in _ffi.last_error() and (present == -5).all()
        for widths in ([3, 9], [9, 32]):
            rc, present = call(widths, _ffi.ptr(grid))
            assert rc == -1 and "presence_library" in _ffi.last_error() and f"width={3 if 3 in widths else 32}" in _ffi.last_error()
            assert (present == -5).all()
            with pytest.raises(ValueError, match="library_presence: .*width (3|32)"):
                ds.library_presence([np.zeros((4, w), np.int32) for w in widths], [0, 0], True)
        rc, present = call([8, 9], _ffi.ptr(grid))
        assert rc == -1 and "behind its width" in _ffi.last_error() and (present == -5).all()
        huge = grid.copy()
        huge[1, 2, 3] = 2 ** 31 // 31
        rc, present = call([9, 9], _ffi.ptr(huge))
        assert rc == -1 and "int32" in _ffi.last_error() and (present == -5).all()
        assert call([9, 9], None)[0] == -1 and call([9, 9], _ffi.ptr(grid), n=-1)[0] == -1
        assert call([9, 9], _ffi.ptr(grid), n_seq=-1)[0] == -1 and call([9, 9], _ffi.ptr(grid), words=-1)[0] == -1
        assert call([9, 9], _ffi.ptr(grid), codes=None)[0] == -1 and call([9, 9], _ffi.ptr(grid), planes=None)[0] == -1
    finally:
        buf.free()
    # a read set without reads, and the next call on the full one is as good as the first
    none = DeviceSeq(np.zeros(0, np.uint8), np.zeros((0, 2), np.int64))
    try:
        p = none.library_presence([W], [t], True)
        assert p.n_words == 0 and p.n_present.tolist() == [0] and p.fetch().shape == (1, 0) and p.pair_counts().tolist() == [[0]]
        p.close()
    finally:
        none.close()
    got, n_present, _ = fetch_and_close(ds.library_presence([W], [t], True))
    check_planes(got, n_present, want[:1])


# ---- the verb end to end --------------------------------------------------------------------------------------------------------------
def fields_equal(path_a, path_b, n_cols, sep=","):
    a, b = path_a.read_text().split("\n"), path_b.read_text().split("\n")
    cols = a[0].split(sep)
    assert len(a) == len(b) and len(cols) == n_cols and a[0] == b[0]
    for line_a, line_b in zip(a[1:], b[1:]):
        for name, x, y in zip(cols, line_a.split(sep), line_b.split(sep)):
            assert x == y, name
        assert len(line_a.split(sep)) == len(line_b.split(sep))
    return a


@pytest.mark.parametrize("control,top_n", [(False, 1000), (True, 1000), (True, 0)])
def test_verb_end_to_end(tmp_path, monkeypatch, capsys, control, top_n):
    """the seeded reads of tests/test_cooccurrence_host.py and the library of tests/golden/library: every file of the run on the
    device equals, field by field, the one the host statistics give on the model's counts"""
    import kmap_amd.kmer_count as K
    import kmap_amd.motif_discovery as D
    from kmap_amd import cooccurrence as C
    from kmap_amd.pwm import pwm_weights
    res, ctl, seq, borders, *_ = S.write_planted(tmp_path)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    lib = [str(LIB / "three.meme"), str(LIB / "mixed")]
    ctl = str(ctl) if control else None
    real = C._motif_cooccurrence(str(res), lib, ctl, top_n=top_n, write_matrix=True, output_dir=str(tmp_path / "device"))
    monkeypatch.setattr(D, "DeviceSeq", CM.ModelSeq)
    monkeypatch.setattr(K, "encode_fasta", lambda path: M.encode_fasta_np(path))
    model = C._motif_cooccurrence(str(res), lib, ctl, top_n=top_n, write_matrix=True, output_dir=str(tmp_path / "model"))
    capsys.readouterr()
    np.testing.assert_array_equal(real["pair_counts"], model["pair_counts"])
    assert real["pair_counts"].dtype == np.int64 and real["n_reads"] == 600
    if control:
        np.testing.assert_array_equal(real["control_pair_counts"], model["control_pair_counts"])
    a = fields_equal(tmp_path / "device" / "cooccurrence_pairs.csv", tmp_path / "model" / "cooccurrence_pairs.csv", 21 if control else 17)
    assert len(a) == (8 if top_n == 0 else 5)
    assert a[1].split(",")[1:13:3][:2] == ["M2_ACCTACGTA", "a_counts"] and a[1].split(",")[12] == "together"
    assert a[2].split(",")[1] == "M1_CAATCGATAGC" and a[2].split(",")[12] == "apart"
    fields_equal(tmp_path / "device" / "motif_presence.csv", tmp_path / "model" / "motif_presence.csv", 11 if control else 9)
    mat = fields_equal(tmp_path / "device" / "pair_counts.tsv", tmp_path / "model" / "pair_counts.tsv", 5, sep="\t")
    want = CM.np_pair_counts(CM.np_presence(seq, borders, [pwm_weights(m.counts, 1.0) for m in real["motifs"]], real["thresholds"], True))
    assert [[int(x) for x in line.split("\t")[1:]] for line in mat[1:5]] == want.tolist()
    assert sorted(p.name for p in (tmp_path / "device").iterdir()) == sorted(p.name for p in (tmp_path / "model").iterdir())
    for p in (tmp_path / "device").iterdir():
        assert p.read_bytes() == (tmp_path / "model" / p.name).read_bytes(), p.name


def test_planted_pair_ranks_first(tmp_path, monkeypatch, capsys):
    """2000 reads of 60 bases; motif A planted in 400 of them, motif B in 300 of those and in no other; an unrelated matrix C that
    a few percent of the reads hold.  The model says that all three pairs pass the min_expected rule; then (A, B) must rank
    first, as `together`, with the model's counts."""
    import pickle

    import kmap_amd.kmer_count as K
    from kmap_amd import cooccurrence as C
    from kmap_amd.library import read_motif_library
    from kmap_amd.pwm import pwm_threshold, pwm_weights
    seq, borders = CM.planted_pair_reads()
    res = tmp_path / "res"
    res.mkdir()
    (res / K.FileNameDict["config_file"]).write_text((Path(K.__file__).parent / "default_config.toml").read_text())
    with open(res / K.FileNameDict["processed_fasta_file"], "wb") as fh:
        pickle.dump(seq, fh)
    with open(res / K.FileNameDict["processed_fasta_seqboarder_file"], "wb") as fh:
        pickle.dump(borders, fh)
    unrelated = tmp_path / "unrelated.csv"
    unrelated.write_text("2,2,2,2,2,2\n2,2,2,2,2,2\n18,18,2,2,18,18\n2,2,18,18,2,2\n")           # GGTTGG: in neither planted word
    lib = [str(LIB / "three.meme"), str(unrelated)]
    motifs = [m for f in lib for m in read_motif_library(f) if m.skip is None]
    assert [m.name for m in motifs] == ["M1_CAATCGATAGC", "M2_ACCTACGTA", "unrelated"]
    Ws = [pwm_weights(m.counts, 1.0) for m in motifs]
    ts = [pwm_threshold(W, 1e-3)[0] for W in Ws]                 # A and B where planted and a little by chance, C in 3 % of all reads
    bits = CM.np_presence(seq, borders, Ws, ts, True)
    want = CM.np_pair_counts(bits)
    stats = CM.np_pair_stats(want, 2000)                         # the default min_expected
    assert all(r["tested"] for r in stats), [(r["expected"], r["n_i"], r["n_j"]) for r in stats]
    assert 400 <= want[0, 0] < 440 and 300 <= want[1, 1] < 330 and want[0, 1] >= 300 and 30 < want[2, 2] < 200
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    real = C._motif_cooccurrence(str(res), lib, p_value=1e-3)
    capsys.readouterr()
    np.testing.assert_array_equal(real["pair_counts"], want)
    first = real["rows"][0]
    assert (first["i"], first["j"], first["direction"]) == (0, 1, "together") and first["n_both"] == want[0, 1]
    assert first["z"] == stats[0]["z"] > 20 and first["q_bh"] < 1e-50 and real["n_tests"] == 3
    line = (res / "motif_cooccurrence" / "cooccurrence_pairs.csv").read_text().split("\n")[1].split(",")
    assert line[:2] == ["0", "M1_CAATCGATAGC"] and line[4] == "M2_ACCTACGTA" and line[12] == "together"
    assert [int(x) for x in line[7:10]] == [int(want[0, 0]), int(want[1, 1]), int(want[0, 1])]
