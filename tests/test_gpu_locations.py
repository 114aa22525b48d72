"""GPU: extract_motif_locations against the reference's outputs (tests/golden/locations/, written by gen_golden_locations.py), against a
Python restatement of the reference's loop on crafted and random inputs (including the documented deviations), against a numpy
restatement at ~2e6 rows, and check_motif_co_occurence against the reference's tables on tests/test.fa."""
import json
import shutil
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
GOLD = ROOT / "tests" / "golden"
LGOLD = GOLD / "locations"
HEADER = "chrom\tstart\tend\tname\tscore\tstrand\n"


def _int_lit(s):
    try:
        int(s)
        return s.strip() == s and s.lstrip("+-").isdigit()
    except ValueError:
        return False


def model(bed_lines, occ_rows, conseqs):
    """the reference's loop restated (util.py:292-352): bed_lines = [[chrom, start, ...(, strand)]], occ_rows = [(seq_ind, [cells])]
    with positions; returns {file name: text}"""
    ints = all(_int_lit(b[0]) for b in bed_lines)
    out = {}
    for i, cs in enumerate(conseqs):
        rows = []
        for s, cells in occ_rows:
            b = bed_lines[s]
            chrom = int(b[0]) if ints else b[0]
            strand = b[5] if len(b) == 6 else "."
            merged = []
            for st, en in sorted([int(b[1]) + p, int(b[1]) + p + len(cs)] for p in cells[i]):
                if not merged or merged[-1][1] < st:
                    merged.append([st, en])
                else:
                    merged[-1][1] = max(merged[-1][1], en)
            rows += [[chrom, st, en, f"motif_{i}_{s}", 0, strand] for st, en in merged]
        rows.sort()
        out[f"motif_{i}_{cs}_locations.bed"] = HEADER + "".join("\t".join(map(str, r)) + "\n" for r in rows)
    return out


def _run(tmp_path, bed_text, occ_text, conseqs, tag="x"):
    from kmap_amd.locations import _extract_motif_locations
    d = tmp_path / tag
    d.mkdir()
    (d / "in.bed").write_text(bed_text)
    (d / "occ.csv").write_text(occ_text)
    (d / "conseq.txt").write_text("\n".join(conseqs) + "\n")
    _extract_motif_locations(d / "in.bed", d / "conseq.txt", d / "occ.csv", d / "out")
    return {f.name: f.read_text() for f in sorted((d / "out").iterdir())}


def _occ_text(occ_rows, n_cols):
    return ";".join(["seq_ind"] + [f"motif_{c}" for c in range(n_cols)] + ["seq_len"]) + "\n" + "".join(
        f"{s};" + ";".join(",".join(map(str, c)) for c in cells) + ";100\n" for s, cells in occ_rows)


@pytest.mark.parametrize("bed", ["bed6_chr", "bed6_int"])
@pytest.mark.parametrize("occ", ["synth", "testfa"])
def test_golden_outputs_byte_identical(tmp_path, capsys, bed, occ):
    from kmap_amd.locations import _extract_motif_locations
    src = {"synth": (LGOLD / "synth.motif_occurence.csv", LGOLD / "synth_conseq.txt"),
           "testfa": (GOLD / "scan_testfa" / "final.motif_occurence.csv", GOLD / "scan_testfa" / "final_conseq.txt")}[occ]
    out = tmp_path / "out"
    _extract_motif_locations(str(LGOLD / f"{bed}.bed"), str(src[1]), str(src[0]), str(out))
    assert capsys.readouterr().out.strip().endswith(f"Motif location extraction complete. Results saved in {out}")
    want = sorted((LGOLD / f"out_{bed}_{occ}").iterdir())
    assert [f.name for f in sorted(out.iterdir())] == [f.name for f in want]
    for f in want:
        assert (out / f.name).read_bytes() == f.read_bytes(), f.name


def test_tie_break_and_merge_rules(tmp_path):
    """touching windows merge, a gap of one does not, overlapping / duplicate / unsorted hits merge; at equal coordinates the names
    sort as strings (motif_0_10 < motif_0_100 < motif_0_2); a chain of touching windows is one interval; an empty consensus line is a
    consensus of length 0"""
    bed = [["chr1", "1000", "1100", "n", "0", s] for s in "+-.+"] * 30
    L = 6
    occ_rows = [(2, [[0, 40], [5, 5 + L, 5 + 2 * L + 1]]), (10, [[0, 40], [30, 32, 31, 30]]), (100, [[0, 40], []]),
                (3, [[7, 7 + L, 7 + 2 * L, 7 + 3 * L], [1, 1]]), (21, [[], [9, 9 + L + 1]])]
    conseqs = ["ACGTAC", "GGGTTT", ""]
    occ_rows = [(s, cells + [[4, 4, 5]]) for s, cells in occ_rows]
    got = _run(tmp_path, "".join("\t".join(b) + "\n" for b in bed), _occ_text(occ_rows, 3), conseqs)
    assert got == model(bed, occ_rows, conseqs)
    lines = got["motif_0_ACGTAC_locations.bed"].splitlines()
    assert [ln.split("\t")[3] for ln in lines[1:4]] == ["motif_0_10", "motif_0_100", "motif_0_2"]
    assert "chr1\t1007\t1031\tmotif_0_3\t0\t+" in lines                      # four touching windows: one interval


def test_deviations_three_columns_and_single_position_columns(tmp_path):
    """where the reference raises: a 3-column BED gets strand "."; columns without a comma (pandas would parse them as numbers) are
    single positions"""
    rng = np.random.default_rng(5)
    bed = [[rng.choice(["7", "12", "3"]), str(int(rng.integers(0, 10 ** 6))), "0"] for _ in range(50)]
    occ_rows = [(int(s), [[int(rng.integers(0, 90))], [int(rng.integers(0, 90))]]) for s in rng.choice(50, 20, replace=False)]
    got = _run(tmp_path, "".join("\t".join(b) + "\n" for b in bed), _occ_text(occ_rows, 2), ["ACGT", "TTTTTTT"])
    assert got == model(bed, occ_rows, ["ACGT", "TTTTTTT"])
    assert all(ln.endswith("\t0\t.") for t in got.values() for ln in t.splitlines()[1:])
    assert got["motif_0_ACGT_locations.bed"].splitlines()[1].split("\t")[0].isdigit()      # integer chroms stay integers


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_random_against_python_model(tmp_path, seed):
    rng = np.random.default_rng(100 + seed)
    n_bed = int(rng.integers(1, 400))
    names = [["chr1", "chr2", "chr10", "chrX", "chrUn_1"], ["1", "2", "10", "010", "-3"], ["only"]][seed % 3]
    bed = [[str(rng.choice(names)), str(int(rng.integers(0, 2 ** 34))), "0", "n", "0", str(rng.choice(["+", "-", "."]))] for _ in range(n_bed)]
    conseqs = ["".join(rng.choice(list("ACGT"), int(rng.integers(1, 15)))) for _ in range(int(rng.integers(1, 5)))]
    n_cols = len(conseqs) + int(rng.integers(0, 2))                          # extra columns are ignored
    occ_rows = []
    for s in rng.choice(n_bed, min(n_bed, 300), replace=False):
        cells = [sorted(int(x) for x in rng.integers(0, 60, int(rng.integers(0, 6)))) for _ in range(n_cols)]
        cells[0] = cells[0] + [int(rng.integers(0, 60))]                      # every column holds commas somewhere
        occ_rows.append((int(s), [sorted(c) for c in cells]))
    got = _run(tmp_path, "".join("\t".join(b) + "\n" for b in bed), _occ_text(occ_rows, n_cols), conseqs)
    assert got == model(bed, occ_rows, conseqs)


def _numpy_expected(bed_start, bed_rank, seq_ind, hits, pos, L):
    """per consensus: (row, start, end) in output order, by np.lexsort over (name string rank, end, start, chrom rank)"""
    n = len(seq_ind)
    r = np.repeat(np.arange(n), hits)
    if len(pos) == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.int64)
    new_cell = np.ones(len(pos), bool)
    new_cell[1:] = r[1:] != r[:-1]
    flag = new_cell.copy()
    flag[1:] |= pos[:-1].astype(np.int64) + L < pos[1:]
    first = np.flatnonzero(flag)
    last = np.append(first[1:], len(pos)) - 1
    s = seq_ind[r[first]]
    st = bed_start[s] + pos[first]
    en = bed_start[s] + pos[last] + L
    u = np.unique(s)
    name_rank = np.empty(u.max() + 1, np.int64)
    name_rank[u[np.argsort(u.astype(str), kind="stable")]] = np.arange(len(u))
    o = np.lexsort((name_rank[s], en, st, bed_rank[s]))
    return s[o], st[o], en[o]


@pytest.mark.parametrize("single_chrom", [False, True])
def test_two_million_rows_against_numpy(single_chrom):
    """~2e6 occurrence rows x 3 consensuses through the device pipeline (locate) == a numpy restatement; starts above 2^31; the
    single-chrom input has a constant chrom field (its radix passes are skipped)"""
    from kmap_amd.locations import locate
    from kmap_amd.reports import Occurrence
    rng = np.random.default_rng(9 + single_chrom)
    n, n_bed = 2_000_000, 2_500_000

    class Bed:
        pass
    bed = Bed()
    bed.n_rows = n_bed
    bed.n_chrom = 1 if single_chrom else 25
    bed.start = rng.integers(0, 2 ** 33, n_bed).astype(np.int64)
    bed.chrom_rank = rng.integers(0, bed.n_chrom, n_bed).astype(np.int32)
    seq_ind = rng.choice(n_bed, n, replace=False).astype(np.int64)
    lens = [8, 12, 21]
    hits, pos = [], []
    for c in range(3):
        h = rng.choice([0, 0, 1, 2, 3, 5], n).astype(np.int32)
        p = np.sort(rng.integers(0, 200, (n, 5)).astype(np.int32), axis=1)
        keep = np.arange(5)[None, :] < h[:, None]
        hits.append(h)
        pos.append(np.ascontiguousarray(p[keep]))
    occ = Occurrence(hits, pos, np.full(n, 200), seq_ind)
    timing = {}
    res = locate(bed, occ, ["A" * L for L in lens], all_rows=True, timing=timing)
    assert timing["device_ms"] > 0
    for c in range(3):
        want = _numpy_expected(bed.start, bed.chrom_rank, seq_ind, hits[c], pos[c], lens[c])
        for g, w in zip(res[c], want):
            np.testing.assert_array_equal(g, w)


SORT_EDGES = (1, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 16384, 16385, 20001)


def _key_bits(bed, seq_ind, pos, L):
    """the width of the sort key as locations_impl lays it out: name nibbles, end - start, start, chrom rank (one consensus: no bits)"""
    bits = lambda v: int(v).bit_length()
    return (4 * len(str(int(seq_ind.max()))) + bits(int(pos.max()) + L) + bits(int(bed.start[seq_ind].max()) + int(pos.max()))
            + bits(bed.n_chrom - 1))


def test_sort_at_tile_edges():
    """one consensus with one hit in each of M rows, so exactly M sort keys, at the radix sort's own edges (64 keys are a wave, 1024 a
    wave's tile, 4096 a block's four tiles, past 16384 keys the pass's scan changes kernel).  BED starts from 2^32 up to 2^33,
    seven-digit seq_ind and 25 chromosomes: the key is wider than 64 bits (asserted), so passes run in its second word.  Once more at
    4097 keys with one chromosome and one position: whole digits are constant and skipped.  From M = 2 on the last row repeats the
    first row's seq_ind and position: two keys equal in every field, far apart in the input, whose (equal) triples must come out next
    to each other, where the numpy model puts them."""
    from kmap_amd.locations import locate
    from kmap_amd.reports import Occurrence
    rng = np.random.default_rng(77)
    n_bed, L = 2_500_000, 12

    class Bed:
        pass
    bed = Bed()
    bed.n_rows = n_bed
    bed.start = rng.integers(2 ** 32, 2 ** 33, n_bed).astype(np.int64)
    ranks = rng.integers(0, 25, n_bed).astype(np.int32)
    for M, single in [(M, False) for M in SORT_EDGES] + [(4097, True)]:
        bed.n_chrom = 1 if single else 25
        bed.chrom_rank = np.zeros(n_bed, np.int32) if single else ranks
        seq_ind = (1_000_000 + rng.choice(1_500_000, M, replace=False)).astype(np.int64)
        pos = np.full(M, 57, np.int32) if single else rng.integers(0, 200, M).astype(np.int32)
        if M > 1:
            seq_ind[-1], pos[-1] = seq_ind[0], pos[0]
        assert _key_bits(bed, seq_ind, pos, L) > 64
        hits = np.ones(M, np.int32)
        res = locate(bed, Occurrence([hits], [pos], np.full(M, 200), seq_ind), ["A" * L], all_rows=True)
        want = _numpy_expected(bed.start, bed.chrom_rank, seq_ind, hits, pos, L)
        assert len(res[0][0]) == M
        for g, w in zip(res[0], want):
            np.testing.assert_array_equal(g, w)
        if M > 1:
            at = np.flatnonzero(res[0][0] == seq_ind[0])
            assert len(at) == 2 and at[1] == at[0] + 1


def test_in_memory_occurrence_equals_path(tmp_path):
    """an Occurrence, or a scan_motif_occurence-style hit list, in place of the file path: the same files"""
    from kmap_amd.locations import _extract_motif_locations
    from kmap_amd.reports import Occurrence
    occ_file = GOLD / "scan_testfa" / "final.motif_occurence.csv"
    cons = GOLD / "scan_testfa" / "final_conseq.txt"
    bed = LGOLD / "bed6_chr.bed"
    _extract_motif_locations(bed, cons, occ_file, tmp_path / "a")
    occ = Occurrence.from_file(occ_file)
    _extract_motif_locations(bed, cons, occ, tmp_path / "b")
    full = [(np.zeros(1002, np.int32), np.zeros(0, np.int32)) for _ in range(occ.n_conseq)]       # one row per read, like the scan
    for c in range(occ.n_conseq):
        h = np.zeros(1002, np.int32)
        h[occ.seq_ind] = occ.hits[c]
        full[c] = (h, np.concatenate([occ.pos[c][occ.offs(c)[i]:occ.offs(c)[i + 1]] for i in np.argsort(occ.seq_ind)]).astype(np.int32))
    _extract_motif_locations(bed, cons, full, tmp_path / "c")
    for f in sorted((tmp_path / "a").iterdir()):
        assert (tmp_path / "b" / f.name).read_bytes() == f.read_bytes() == (tmp_path / "c" / f.name).read_bytes()


def test_errors_raise_before_any_file(tmp_path):
    from kmap_amd.locations import _extract_motif_locations
    (tmp_path / "small.bed").write_text("chr1\t0\t10\tn\t0\t+\nchr1\t5\t10\tn\t0\t+\n")
    (tmp_path / "four.bed").write_text("chr1\t0\t10\tn\n")
    (tmp_path / "occ.csv").write_text("seq_ind;m0;m1;seq_len\n0;1,2;3;10\n1;;4,5;10\n")
    (tmp_path / "past.csv").write_text("seq_ind;m0;m1;seq_len\n0;1,2;3;10\n2;;4,5;10\n")
    (tmp_path / "two.txt").write_text("ACGT\nTTTT\n")
    (tmp_path / "three.txt").write_text("ACGT\nTTTT\nGGGG\n")
    cases = [("small.bed", "two.txt", "past.csv", "outside the BED"), ("small.bed", "three.txt", "occ.csv", "3 consensus"),
             ("four.bed", "two.txt", "occ.csv", "3 or 6 columns")]
    for bed, cons, occ, msg in cases:
        out = tmp_path / "out"
        with pytest.raises(ValueError, match=msg):
            _extract_motif_locations(tmp_path / bed, tmp_path / cons, tmp_path / occ, out)
        assert not out.exists()
    _extract_motif_locations(tmp_path / "small.bed", tmp_path / "two.txt", tmp_path / "occ.csv", tmp_path / "ok")
    assert (tmp_path / "ok" / "motif_1_TTTT_locations.bed").read_text() == HEADER + "chr1\t3\t7\tmotif_1_0\t0\t+\nchr1\t9\t14\tmotif_1_1\t0\t+\n"


@pytest.mark.parametrize("case", ["readme", "samelen"])
def test_check_motif_co_occurence_matches_reference(tmp_path, capsys, case):
    from kmap_amd.locations import check_motif_co_occurence
    d = LGOLD / f"co_{case}"
    a = json.loads((d / "args.json").read_text())
    np.random.seed(a["seed"])
    info = check_motif_co_occurence(GOLD / "test.fa", a["motif1"], a["motif2"], a["max_ham_dist1"], a["max_ham_dist2"], tmp_path / "o")
    want_info = (d / "info.txt").read_text().strip()
    assert info == want_info
    if want_info:
        assert want_info in capsys.readouterr().out
    for f in ("user_motif_occurence.csv", "co_occurence_mat.tsv", "co_occurence_mat.norm.tsv", "co_occurence_motif_dist_mat.tsv",
              "co_occurence_motif_dist_data.txt"):
        assert (tmp_path / "o" / f).read_bytes() == (d / f).read_bytes(), f


def test_cli_readme_command_lines(tmp_path):
    """the reference README's two command lines through `python -m kmap_amd` (default --conseq_file / --motif_occurrence_file /
    --output_dir in the result directory)"""
    res = tmp_path / "res"
    res.mkdir()
    shutil.copyfile(GOLD / "scan_testfa" / "final_conseq.txt", res / "final_conseq.txt")
    shutil.copyfile(GOLD / "scan_testfa" / "final.motif_occurence.csv", res / "final.motif_occurence.csv")
    shutil.copyfile(LGOLD / "bed6_int.bed", res / "your_bed_file.bed")
    env_py = [sys.executable, "-m", "kmap_amd"]
    r = subprocess.run(env_py + ["extract_motif_locations", "--bed_file", "your_bed_file.bed"], cwd=res, capture_output=True,
                       text=True, timeout=600, env={**__import__("os").environ, "PYTHONPATH": str(ROOT)})
    assert r.returncode == 0, r.stderr[-3000:]
    assert "Motif location extraction complete. Results saved in motif_locations" in r.stdout
    for f in sorted((LGOLD / "out_bed6_int_testfa").iterdir()):
        assert (res / "motif_locations" / f.name).read_bytes() == f.read_bytes()
    shutil.copyfile(GOLD / "test.fa", res / "test.fa")
    r = subprocess.run(env_py + ["check_motif_co_occurence", "--input_fasta_file", "./test.fa", "--motif1", "GTACGTAGGTCCTA",
                                 "--motif2", "AATCGATAGCGA", "--max_ham_dist1", "6", "--max_ham_dist2", "5", "--output_dir", "./results"],
                       cwd=res, capture_output=True, text=True, timeout=600, env={**__import__("os").environ, "PYTHONPATH": str(ROOT)})
    assert r.returncode == 0, r.stderr[-3000:]
    assert "co_occur_freq=" in r.stdout
    assert (res / "results" / "co_occurence_mat.tsv").read_bytes() == (LGOLD / "co_readme" / "co_occurence_mat.tsv").read_bytes()
