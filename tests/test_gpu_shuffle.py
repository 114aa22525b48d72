"""shuffle_reads on the GPU (csrc/shuffle.hip) against the restatement of DESIGN.md section 15 in tests/_shuffle_model.py: the whole
output array byte for byte, what a shuffle must keep (checked without the model's draws), uniformity over everything a shuffle may
return, seeds, the source left alone, the verb's file, errors."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

from tests import _shuffle_model as M

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
GOLD = ROOT / "tests" / "golden"
MOTIF0, MOTIF1 = GOLD / "report_testfa" / "cntmat_motif0_CAATCGATAGC.csv", GOLD / "report_testfa" / "cntmat_motif1_ACCTACGTA.csv"
CODE = {c: i for i, c in enumerate("ACGT")}
LENGTHS = [0, 1, 2, 3, 4, 15, 16, 17, 31, 32, 33, 63, 64, 65]
SEEDS = (15, 2 ** 64 - 3)
KLETS = (1, 2)
EDGES = (16, 64, 1024, 4096, 16384)          # positions of a group; of a thread, a wave and a block of the kernels (edges_array)
SLOT = 16384


@pytest.fixture(autouse=True)
def model_draws_are_the_package_s():
    """the model stands for the package only while its draws are the package's; without kmap_amd.shuffle no test here says anything"""
    from kmap_amd import shuffle
    assert (M.GOLDEN, M.mix64(15), M.copy_seed(15, 1)) == (shuffle.GOLDEN, shuffle.mix64(15), shuffle.copy_seed(15, 1))


def encode(text):
    return np.array([CODE.get(c, 255) for c in text], np.uint8)


# ---- the arrays ---------------------------------------------------------------------------------------------------------------------
def edges_array():
    """every length of LENGTHS starting at, and ending in front of, the tile edges of the kernels - 1, + 0, + 1, alone in a stretch of
    255 (more than 256 segments: two blocks of the shuffle): EDGES are a 16-position group of the mask, and the positions of a thread
    (64 = 4 groups), a wave (4096) and a block (16384) of the start search and of a wave (1024) and a block (4096) of the fill
    kernel, each at a multiple of itself in the array (SLOT is a multiple of them all); then the same lengths with ONE 255 between
    neighbours, so that segments share code words and groups; reads with N inside, at both ends and in runs; one-letter and
    two-letter reads and a read whose last base occurs once; the array ends in the middle of a group, inside a segment"""
    rng = np.random.default_rng(1501)
    slot = SLOT
    places = [(b, sh, L, at_start) for b in EDGES for sh in (-1, 0, 1) for L in LENGTHS for at_start in (True, False)]
    seq = np.full((len(places) + 1) * slot, 255, np.uint8)
    for i, (b, sh, L, at_start) in enumerate(places):
        s = i * slot + b + sh - (0 if at_start else L)
        seq[s:s + L] = rng.integers(0, 4, L)
    parts = [seq]
    for L in LENGTHS * 6:                                     # 14 x 6 segments, one separator each: starts at every offset of a group
        parts += [rng.integers(0, 4, L).astype(np.uint8), np.array([255], np.uint8)]
    parts.append(encode("NACGTTGCANNNNACGGTNNTTGACCAGTGNANCNGNTN" + "NNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNN" + "A" * 40 + "N" + "AC" * 23 + "N" + "C" * 17
                        + "N" + "CA" * 9 + "C" + "N" + "T" * 30 + "G" + "N" + "GGGGGGGGGGA" + "N" + "ACGTACGTTTGACA" * 3 + "G" + "N"))
    parts.append(rng.integers(0, 4, 41).astype(np.uint8))     # the last segment ends with the array
    seq = np.concatenate(parts)
    if len(seq) % 16 == 0:
        seq = np.concatenate([seq, rng.integers(0, 4, 5).astype(np.uint8)])
    return seq


def short_reads_array():
    """70 000 reads of 0 .. 12 bases over one to four letters: 274 blocks of the shuffle kernel"""
    rng = np.random.default_rng(1502)
    lens = rng.integers(0, 13, 70_000)
    seq = rng.integers(0, 4, int(lens.sum()) + len(lens)).astype(np.uint8)
    seq %= np.repeat(rng.integers(1, 5, len(lens)), lens + 1).astype(np.uint8)
    seq[np.cumsum(lens + 1) - 1] = 255
    return seq


def long_read_array():
    rng = np.random.default_rng(1503)
    return np.concatenate([rng.integers(0, 4, 40), [255], rng.integers(0, 4, 200_000), [255, 255], rng.integers(0, 4, 35)]).astype(np.uint8)


def golden_reads_array():
    from kmap_amd.kmer_count import encode_fasta
    return np.asarray(encode_fasta(str(GOLD / "test.fa"))[0], np.uint8)


ARRAYS = {"edges": edges_array, "short": short_reads_array, "long": long_read_array, "testfa": golden_reads_array}
_SEQ, _DEV, _OUT, _WANT = {}, {}, {}, {}


def array(name):
    if name not in _SEQ:
        _SEQ[name] = ARRAYS[name]()
    return _SEQ[name]


def device_seq(name):
    """the array as one resident read set (its borders play no part in a shuffle)"""
    if name not in _DEV:
        from kmap_amd.motif_discovery import DeviceSeq
        seq = array(name)
        _DEV[name] = DeviceSeq(seq, np.array([[0, len(seq)]], np.int64))
    return _DEV[name]


def device_shuffle(name, klet, seed):
    """DeviceSeq.shuffled(...).download(), once per case"""
    if (name, klet, seed) not in _OUT:
        sh = device_seq(name).shuffled(klet, seed)
        try:
            starts, lens = M.segments(array(name))
            assert sh.shuffle_stats == (len(starts), int(lens.sum()))
            _OUT[name, klet, seed] = sh.download()
        finally:
            sh.close()
    return _OUT[name, klet, seed]


def model_shuffle(name, klet, seed):
    if (name, klet, seed) not in _WANT:
        _WANT[name, klet, seed] = M.shuffle_array(array(name), klet, seed)
    return _WANT[name, klet, seed]


# ---- 1. the whole array against the model -------------------------------------------------------------------------------------------
def test_edges_array_is_what_it_says():
    seq = array("edges")
    starts, lens = M.segments(seq)
    assert len(seq) % 16 != 0 and seq[-1] < 4 and seq[0] == 255
    assert set(LENGTHS[1:]) <= set(lens.tolist())
    assert all(SLOT % b == 0 for b in EDGES) and SLOT == 16 * 4 * 256          # a block of the start search: SH_GPT groups a thread
    for b in EDGES:
        for sh in (-1, 0, 1):
            assert {(b + sh) % SLOT} <= set((starts % SLOT).tolist()) and {(b + sh) % SLOT} <= set(((starts + lens) % SLOT).tolist())
    assert set(range(16)) <= set((starts % 16).tolist()) and len(starts) > 256
    assert (np.diff(starts) == lens[:-1] + 1).sum() > 80      # neighbours one 255 apart


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("klet", KLETS)
@pytest.mark.parametrize("name", ["edges", "short", "testfa"])
def test_equals_the_model(name, klet, seed):
    got, want = device_shuffle(name, klet, seed), model_shuffle(name, klet, seed)
    assert got.dtype == np.uint8 and got.shape == want.shape
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, f"{len(bad)} positions differ, the first at {bad[:5]}: {got[bad[:5]]} for {want[bad[:5]]}"


@pytest.mark.parametrize("klet", KLETS)
def test_a_read_of_200_000_bases_equals_the_model(klet):
    for seed in SEEDS:
        np.testing.assert_array_equal(device_shuffle("long", klet, seed), model_shuffle("long", klet, seed))


# ---- 2. what a shuffle keeps, without the model's draws -----------------------------------------------------------------------------
@pytest.mark.parametrize("klet", KLETS)
@pytest.mark.parametrize("name", ["edges", "short", "long", "testfa"])
def test_invariants(name, klet):
    seq = array(name)
    starts, lens = M.segments(seq)
    for seed in SEEDS:
        out = device_shuffle(name, klet, seed)
        np.testing.assert_array_equal(out == 255, seq == 255)
        assert (out[seq != 255] < 4).all()
        np.testing.assert_array_equal(M.base_counts(out), M.base_counts(seq))
        if klet == 2:
            for got, want in zip(M.pair_counts(out), M.pair_counts(seq)):
                np.testing.assert_array_equal(got, want)
            for s, n in zip(starts[lens <= 3], lens[lens <= 3]):
                np.testing.assert_array_equal(out[s:s + n], seq[s:s + n])


def test_golden_reads_do_move():
    """an identity `shuffle` keeps every invariant: at klet 2 fewer than half of the reads of 20 bases or more come back as they were"""
    seq = array("testfa")
    starts, lens = M.segments(seq)
    out = device_shuffle("testfa", 2, SEEDS[0])
    long_enough = np.nonzero(lens >= 20)[0]
    same = sum(np.array_equal(out[starts[i]:starts[i] + lens[i]], seq[starts[i]:starts[i] + lens[i]]) for i in long_enough)
    assert len(long_enough) > 900 and same < len(long_enough) / 2, (same, len(long_enough))


# ---- 3. uniformity --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("text,klet,n_arrangements", [("GATTACAGATTC", 2, 36), ("AAACCAGTCAGA", 2, 120), ("AACGT", 1, 60)])
def test_uniform(text, klet, n_arrangements):
    """2000 M copies of one read as separate reads: the draws are keyed by position, so every copy gets its own shuffle.  Every one
    of the M possible results occurs, and Pearson's chi-square against the uniform distribution stays below its 1 - 1e-9 quantile
    (110.3 at M = 36, 235.9 at M = 120, 148.9 at M = 60)."""
    from kmap_amd.motif_discovery import DeviceSeq
    from scipy.stats import chi2
    x = encode(text)
    every = M.all_arrangements(x, klet)
    assert len(every) == n_arrangements
    n = 2000 * n_arrangements
    seq = np.tile(np.concatenate([x, [255]]).astype(np.uint8), n)
    ds = DeviceSeq(seq, np.stack([np.arange(n) * (len(x) + 1), np.arange(n) * (len(x) + 1) + len(x)], axis=1))
    try:
        sh = ds.shuffled(klet, 15)
        out = sh.download().reshape(n, len(x) + 1)
        sh.close()
    finally:
        ds.close()
    assert (out[:, -1] == 255).all()
    seen, counts = np.unique(out[:, :-1], axis=0, return_counts=True)
    assert [tuple(r) for r in seen.tolist()] == every
    stat = float(((counts - 2000.0) ** 2 / 2000.0).sum())
    print(f"{text} klet {klet}: chi2 {stat:.1f} at {n_arrangements - 1} degrees of freedom")
    assert stat < chi2.ppf(1 - 1e-9, n_arrangements - 1)


# ---- 4. seeds, and the source is left alone -------------------------------------------------------------------------------------------
def count6(ds, use_work):
    from kmap_amd.kmer_count import DeviceCounts
    dc = DeviceCounts()
    try:
        ds.count(dc, 6, True, True, use_work=use_work)
        return dc.fetch()
    finally:
        dc.close()


def test_seeds_and_the_source():
    from kmap_amd.kmer_count import encode_fasta, kmer2hash
    from kmap_amd.motif_discovery import DeviceSeq
    seq, borders = encode_fasta(str(GOLD / "test.fa"))
    seq, borders = np.asarray(seq, np.uint8), np.asarray(borders, np.int64).reshape(-1, 2)
    ds = DeviceSeq(seq, borders)
    try:
        before = count6(ds, True)
        a = ds.shuffled(2, 5)
        b = ds.shuffled(2, 5)
        c = ds.shuffled(2, 6)
        try:
            out_a, out_b, out_c = a.download(), b.download(), c.download()
            np.testing.assert_array_equal(out_a, out_b)
            assert (out_a != out_c).mean() > 0.2
            np.testing.assert_array_equal(out_a, device_shuffle("testfa", 2, 5))            # whatever the borders say
            # the result is a read set of its own
            assert a.n == ds.n and a.n_seq == ds.n_seq and a.borders.ptr != ds.borders.ptr and a.codes.ptr != ds.codes.ptr
            np.testing.assert_array_equal(a.borders_host, borders)
            assert a.borders_host is not ds.borders_host
            np.testing.assert_array_equal(a.read_len, borders[:, 1] - borders[:, 0])
            np.testing.assert_array_equal(a.borders.to_numpy(np.int64, (a.n_seq, 2)), borders)
            # 1-mer counts stay, 6-mer counts do not
            kh, cnt = count6(a, True)
            assert not (len(kh) == len(before[0]) and np.array_equal(cnt, before[1]))
        finally:
            for h in (a, b, c):
                h.close()
        # the source: codes, both masks and its counts
        np.testing.assert_array_equal(ds.download(), seq)
        after = count6(ds, True)
        for x, y in zip(before, after):
            np.testing.assert_array_equal(x, y)
        # a mask() before does not count: the shuffle reads the original reads
        ds.mask(9, np.array([kmer2hash("ACCTACGTA")], np.uint64), np.array([2], np.int32))
        masked = ds.download()
        assert (masked != seq).sum() > 1000
        d = ds.shuffled(2, 5)
        try:
            np.testing.assert_array_equal(d.download(), out_a)
        finally:
            d.close()
        np.testing.assert_array_equal(ds.download(), masked)
        for x, y in zip(before, count6(ds, False)):
            np.testing.assert_array_equal(x, y)
    finally:
        ds.close()


# ---- 5. the verb end to end -----------------------------------------------------------------------------------------------------------
def test_verb_end_to_end(tmp_path, capsys):
    from kmap_amd import shuffle as S
    from kmap_amd.enrichment import _enrich_kmers
    from kmap_amd.evaluate import _evaluate_pwm
    from kmap_amd.kmer_count import _preproc, encode_fasta
    from kmap_amd.motif_discovery import DeviceSeq
    res = tmp_path / "res"
    _preproc(str(GOLD / "test.fa"), str(res))
    seq, borders = encode_fasta(str(GOLD / "test.fa"))
    seq, borders = np.asarray(seq, np.uint8), np.asarray(borders, np.int64).reshape(-1, 2)
    capsys.readouterr()
    assert S._shuffle_reads(str(res), seed=5, n_copies=2) == (len(borders),) + S.unchanged_by_definition(seq, 2)
    printed = capsys.readouterr().out
    assert "klet 2, seed 5, 2 copies of 1002 reads" in printed and "1002 segments" in printed
    out = res / S.OUTPUT_FILE
    names = [line for line in out.read_text().splitlines()[::2]]
    assert names == [f">shuffled_{c}_{i}" for c in range(2) for i in range(len(borders))]
    got_seq, got_borders = encode_fasta(str(out))
    ds = DeviceSeq(seq, borders)
    try:
        want = []
        for c in range(2):
            sh = ds.shuffled(2, S.copy_seed(5, c))
            want.append(sh.download())
            sh.close()
    finally:
        ds.close()
    assert not np.array_equal(want[0], want[1])
    np.testing.assert_array_equal(np.asarray(got_seq), np.concatenate(want))
    np.testing.assert_array_equal(np.asarray(got_borders).reshape(-1, 2), np.concatenate([borders, borders + len(seq)]))
    np.testing.assert_array_equal(want[0], M.shuffle_array(seq, 2, M.copy_seed(5, 0)))
    # the same arguments write the same file; klet 1 and another file name
    first = out.read_bytes()
    S._shuffle_reads(str(res), seed=5, n_copies=2)
    assert out.read_bytes() == first
    other = tmp_path / "sub" / "k1.fa"
    S._shuffle_reads(str(res), klet=1, seed=5, output_file=str(other))
    k1_seq, k1_borders = encode_fasta(str(other))
    np.testing.assert_array_equal(np.asarray(k1_seq), M.shuffle_array(seq, 1, M.copy_seed(5, 0)))
    # the file is a control for the two verbs that need one
    results = _evaluate_pwm(str(res), str(out), [str(MOTIF0), str(MOTIF1)], output_dir=str(tmp_path / "eval"))
    for name, st in zip(("CAATCGATAGC", "ACCTACGTA"), results):
        print(f"auroc of {name} against the klet-2 shuffle: {st['auroc']:.4f}, mw_z {st['mw_z']:.2f}")
        assert st["auroc"] > 0.5 and st["n_control"] + st["control_unscorable"] == 2 * len(borders)
    _enrich_kmers(str(res), str(out), [8], output_dir=str(tmp_path / "enrich"))
    rows = (tmp_path / "enrich" / "enriched_kmers_k8.tsv").read_text().splitlines()
    assert len(rows) > 10


# ---- 6. errors ------------------------------------------------------------------------------------------------------------------------
def packed(seq):
    from kmap_amd import _ffi
    lib = _ffi.lib()
    groups = int(lib.kmap_packed_groups(len(seq)))
    raw = _ffi.DeviceBuffer.from_numpy(seq) if len(seq) else _ffi.DeviceBuffer(16)
    codes, inval = _ffi.DeviceBuffer(groups * 4), _ffi.DeviceBuffer(groups * 2)
    assert lib.kmap_pack_reads_dev(raw.ptr, len(seq), codes.ptr, inval.ptr, None) == 0
    _ffi.sync()
    raw.free()
    return codes, inval


def test_errors_and_the_longest_segment():
    from kmap_amd import _ffi
    from kmap_amd.motif_discovery import DeviceSeq
    lib = _ffi.lib()
    rng = np.random.default_rng(1506)
    limit = 2 ** 21 - 1
    seq = np.concatenate([rng.integers(0, 4, 30), [255], rng.integers(0, 4, limit + 1), [255], rng.integers(0, 4, 9)]).astype(np.uint8)
    codes, inval = packed(seq)
    out = _ffi.DeviceBuffer(len(seq))
    stats = (_ffi.i64 * 2)(-7, -7)

    def call(klet, n=len(seq), c=codes.ptr, m=inval.ptr, o=out.ptr, st=stats):
        return lib.kmap_shuffle_packed_dev(c, m, n, klet, 15, o, st, None)

    def untouched():
        _ffi.sync()
        return bool((out.to_numpy(np.uint8, (len(seq),)) == 0xA5).all())
    assert lib.kmap_memset(out.ptr, 0xA5, len(seq), None) == 0
    for klet in (0, 3, -1):
        assert call(klet) == -1 and "klet" in _ffi.last_error()
    assert stats[0] == -7 and untouched()
    assert call(2, n=-1) == -1 and call(2, c=None) == -1 and call(2, m=None) == -1 and call(2, o=None) == -1 and untouched()
    # a segment of 2^21 bases: KMAP_E_UNSUP, nothing written
    for klet in KLETS:
        assert call(klet) == -4 and "2^21" in _ffi.last_error()
    assert untouched()
    ds = DeviceSeq(seq[:100], np.array([[0, 100]]))
    try:
        for klet in (0, 3):
            with pytest.raises(ValueError, match="klet"):
                ds.shuffled(klet, 1)
        with pytest.raises(ValueError, match="seed"):
            ds.shuffled(2, -1)
        with pytest.raises(ValueError, match="seed"):
            ds.shuffled(2, 2 ** 64)
    finally:
        ds.close()
    # n = 0: accepted, nothing written, with and without stats
    assert call(2, n=0) == 0 and (stats[0], stats[1]) == (0, 0) and call(1, n=0, st=None) == 0 and call(2, n=0, c=None, m=None, o=None) == 0
    assert untouched()
    # one base fewer is served: 2^21 - 1 bases, through the entry itself
    seq[31 + limit] = 255
    for b in (codes, inval):
        b.free()
    codes, inval = packed(seq)
    for klet in KLETS:
        assert call(klet, c=codes.ptr, m=inval.ptr) == 0 and (stats[0], stats[1]) == (3, 30 + limit + 9)
        _ffi.sync()
        got = out.to_numpy(np.uint8, (len(seq),))
        np.testing.assert_array_equal(got == 255, seq == 255)
        np.testing.assert_array_equal(M.base_counts(got), M.base_counts(seq))
        if klet == 2:
            for x, y in zip(M.pair_counts(got), M.pair_counts(seq)):
                np.testing.assert_array_equal(x, y)
        assert (got[31:31 + limit] != seq[31:31 + limit]).mean() > 0.5
        for s, n in ((0, 30), (33 + limit, 9)):
            assert got[s:s + n].tolist() == M.shuffle_segment(seq[s:s + n], s, klet, 15)
    # all segments invalid: the output is the input
    blank = np.full(100, 255, np.uint8)
    bc, bm = packed(blank)
    assert call(2, n=100, c=bc.ptr, m=bm.ptr) == 0 and (stats[0], stats[1]) == (0, 0)
    _ffi.sync()
    assert (out.to_numpy(np.uint8, (100,)) == 255).all()
    for b in (codes, inval, out, bc, bm):
        b.free()
