#!/usr/bin/env python3
"""Generate the fixtures of tests/golden/locations/ by RUNNING THE REFERENCE ITSELF (same import scheme as gen_golden.py: the
reference's src/ with the stand-ins of tests/golden/refshim/ ahead of it on sys.path).  Authoring-container only; only inputs and the
outputs the reference computed are stored.

    python tests/golden/gen_golden_locations.py

Writes
  bed6_chr.bed / bed6_int.bed      seeded 6-column BED files, one row per read of test.fa (chr1/chr2/chr10/chrX names; integer
                                   names); rows 2, 3, 10, 20, 100 share chrom and start (the name-string tie-break decides)
  synth.motif_occurence.csv        synthetic occurrence rows: touching (p + L) / gapped (p + L + 1) / overlapping / duplicate
  synth_conseq.txt                 positions, reads 2, 10, 100 at equal coordinates
  out_<bed>_<occ>/*.bed            the reference's extract_motif_locations outputs for both BED files x (synth, scan_testfa final)
  co_<name>/                       check_motif_co_occurence on test.fa: user_motif_occurence.csv, the four co-occurrence files,
                                   info.txt (the co_occur_freq string) and args.json
  cli_options.json                 option names / defaults / required / types of the reference's two click commands
"""
import json
import os
import shutil
import sys
import warnings
from pathlib import Path

HERE = Path(__file__).resolve().parent
REF = Path("/root/reference")
os.environ.setdefault("MPLBACKEND", "Agg")
sys.dont_write_bytecode = True
sys.path.insert(0, str(REF / "src"))
sys.path.insert(0, str(HERE / "refshim"))

import numpy as np  # noqa: E402

warnings.filterwarnings("ignore", category=RuntimeWarning)

import kmap.kmer_count as kc  # noqa: E402
import kmap.motif_discovery as md  # noqa: E402
import kmap.util as ref_util  # noqa: E402

# the reference's hash kernels read up to k-1 bytes past the array under plain Python: the padded call of gen_golden.py
for _name in ("kmer2hash_kernel_uint32", "kmer2hash_kernel_uint64"):
    _orig = getattr(kc, _name)

    def _padded(arr, arr_size, k, hash_arr, inv, miss, _orig=_orig):
        pad = np.concatenate([np.asarray(arr), np.full(k, 255, dtype=np.uint8)])
        return _orig(pad, arr_size, k, hash_arr, inv, miss)

    setattr(kc, _name, _padded)
md.comp_kmer_hash_taichi = kc.comp_kmer_hash_taichi

DST = HERE / "locations"
N_READS = 1002          # reads of tests/golden/test.fa
TIE_ROWS = (2, 3, 10, 20, 100)
CO_CASES = {"readme": ("GTACGTAGGTCCTA", "AATCGATAGCGA", 6, 5, 11),
            "samelen": ("AATCGATAGC", "CCTACGTAGG", 3, 1, 12)}


def write_bed(path, chroms, rng):
    starts = rng.integers(0, 3_000_000, size=N_READS)
    names = rng.choice(chroms, size=N_READS)
    strands = rng.choice(["+", "-", "."], size=N_READS)
    for r in TIE_ROWS:
        names[r], starts[r] = chroms[0], 5000
    with open(path, "w") as fh:
        for i in range(N_READS):
            fh.write(f"{names[i]}\t{starts[i]}\t{starts[i] + 150}\tpeak{i}\t{rng.integers(0, 1000)}\t{strands[i]}\n")


def write_synth_occ(path, lens, rng):
    """two motif columns; every column holds at least one comma (pandas keeps it as text)"""
    rows = {}
    L0, L1 = lens
    rows[0] = ([5, 5 + L0, 5 + 2 * L0 + 1], [7, 7 + L1 + 1])           # touching then gapped; gapped
    rows[1] = ([30, 32, 31, 30], [])                                    # overlapping, duplicate, unsorted
    for r in (2, 10, 100):                                              # equal coordinates (shared BED start), names decide
        rows[r] = ([12, 40], [12])
    rows[3] = ([], [3, 3 + L1, 3 + 2 * L1, 50])                         # a chain of touching windows
    rows[20] = ([12], [])
    for r in rng.choice(np.arange(4, N_READS), size=300, replace=False):
        r = int(r)
        if r in rows:
            continue
        cells = []
        for _ in range(2):
            k = int(rng.integers(0, 4))
            cells.append(sorted(int(x) for x in rng.integers(0, 120, size=k)))
        rows[r] = tuple(cells)
    with open(path, "w") as fh:
        fh.write(f"seq_ind;motif_0_A;motif_1_B;seq_len\n")
        for r in sorted(rows):
            a, b = rows[r]
            if not a and not b:
                continue
            fh.write(f"{r};{','.join(map(str, a))};{','.join(map(str, b))};150\n")


def gen_extract():
    rng = np.random.default_rng(20261016)
    write_bed(DST / "bed6_chr.bed", ["chr1", "chr2", "chr10", "chrX"], rng)
    write_bed(DST / "bed6_int.bed", ["1", "2", "10", "3"], rng)
    conseqs = ["ACGTACGT", "TTGACAGGCA"]
    (DST / "synth_conseq.txt").write_text("\n".join(conseqs) + "\n")
    write_synth_occ(DST / "synth.motif_occurence.csv", [len(c) for c in conseqs], rng)
    occs = {"synth": (DST / "synth.motif_occurence.csv", DST / "synth_conseq.txt"),
            "testfa": (HERE / "scan_testfa" / "final.motif_occurence.csv", HERE / "scan_testfa" / "final_conseq.txt")}
    for bed in ("bed6_chr", "bed6_int"):
        for name, (occ, cons) in occs.items():
            out = DST / f"out_{bed}_{name}"
            shutil.rmtree(out, ignore_errors=True)
            ref_util._extract_motif_locations(str(DST / f"{bed}.bed"), str(cons), str(occ), str(out))


def gen_co():
    for name, (m1, m2, d1, d2, seed) in CO_CASES.items():
        out = DST / f"co_{name}"
        shutil.rmtree(out, ignore_errors=True)
        out.mkdir(parents=True)
        np.random.seed(seed)
        occ_file = out / "user_motif_occurence.csv"
        md.get_user_motif_occurence_file(HERE / "test.fa", [m1, m2], [d1, d2], occ_file, True)
        co, dist, dd = md.get_motif_co_occurence_mat(occ_file, 2)
        info = ""
        if np.any(co):
            freq = co[0][1] * 2 / (co[0][0] + co[1][1])
            info = f"co_occur_freq={freq*100:.2f}%"
        (out / "info.txt").write_text(info + "\n")
        co_sum = np.diag(co) + np.diag(co).reshape((-1, 1))
        names = [m1, m2]
        md.write_co_occurence_mat(out / "co_occurence_mat.tsv", co + 0.0, names)
        md.write_co_occurence_mat(out / "co_occurence_mat.norm.tsv", 2 * co / co_sum, names)
        md.write_co_occurence_mat(out / "co_occurence_motif_dist_mat.tsv", dist, names)
        md.write_co_occurence_dist_arr(out / "co_occurence_motif_dist_data.txt", dd, names)
        (out / "args.json").write_text(json.dumps({"motif1": m1, "motif2": m2, "max_ham_dist1": d1, "max_ham_dist2": d2, "seed": seed}) + "\n")


def _plain(v):
    return v if isinstance(v, (str, int, float, bool)) else None      # click's "no default" sentinel -> null


def gen_cli():
    table = {}
    for cmd in (ref_util.extract_motif_locations, md.check_motif_co_occurence):
        table[cmd.name] = [{"name": p.name, "opts": list(p.opts), "default": _plain(p.default), "required": p.required, "type": p.type.name}
                           for p in cmd.params]
    (DST / "cli_options.json").write_text(json.dumps(table, indent=1) + "\n")


if __name__ == "__main__":
    DST.mkdir(exist_ok=True)
    gen_extract()
    gen_co()
    gen_cli()
