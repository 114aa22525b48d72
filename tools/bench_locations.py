#!/usr/bin/env python3
"""Times `extract_motif_locations` on a seeded synthetic input: N occurrence rows x C consensuses (0-3 hits per cell, locations
< 200) and an N-line 6-column BED file, split into parse (native host threads), device (upload, merge, key, radix sort, gather,
download; HIP events and wall) and format (native host threads, C BED files).  Prints one JSON line.

    python tools/bench_locations.py                    # 10 M rows x 5 consensuses
    python tools/bench_locations.py --rows 1000000 --conseqs 3
"""
import argparse
import ctypes as C
import json
import shutil
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def write_bed(path, n, rng):
    """fixed-width lines `chrNN\\tSSSSSSSSSS\\tEEEEEEEEEE\\tp\\t0\\t+` built as a byte matrix (zero-padded integers parse as integers)"""
    start = rng.integers(0, 3_000_000_000, n)
    chrom = rng.integers(1, 25, n)
    tmpl = np.frombuffer(b"chr00\t0000000000\t0000000000\tp\t0\t+\n", np.uint8)
    m = np.tile(tmpl, (n, 1))
    m[:, 3] = 48 + chrom // 10
    m[:, 4] = 48 + chrom % 10
    for col0, v in ((6, start), (17, start + 300)):
        for k in range(10):
            m[:, col0 + k] = 48 + (v // 10 ** (9 - k)) % 10
    m[:, 32] = np.frombuffer(b"+-.", np.uint8)[rng.integers(0, 3, n)]
    m.tofile(path)


def write_occ(path, n, n_cons, rng):
    from kmap_amd import _ffi
    from kmap_amd._ffi import check, ptr
    hits, pos = [], []
    for _ in range(n_cons):
        h = rng.choice(np.array([0, 0, 0, 1, 1, 2, 3], np.int32), n)
        p = np.sort(rng.integers(0, 200, (n, 3)).astype(np.int32), axis=1)
        hits.append(h)
        pos.append(np.ascontiguousarray(p[np.arange(3)[None, :] < h[:, None]]))
    header = "seq_ind;" + ";".join(f"motif_{i}_M{i}" for i in range(n_cons)) + ";seq_len"
    hp = (C.c_void_p * n_cons)(*[h.ctypes.data for h in hits])
    pp = (C.c_void_p * n_cons)(*[p.ctypes.data for p in pos])
    rows = _ffi.i64(0)
    read_len = np.full(n, 200, np.int64)
    check(_ffi.lib().kmap_write_occurrence_csv(str(path).encode(), header.encode(), n, n_cons, hp, pp, ptr(read_len), C.byref(rows)))
    return rows.value, int(sum(len(p) for p in pos))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--conseqs", type=int, default=5)
    ap.add_argument("--repeat", type=int, default=2)
    ap.add_argument("--workdir", default=None)
    a = ap.parse_args()
    from kmap_amd.locations import _extract_motif_locations
    rng = np.random.default_rng(2026)
    work = Path(a.workdir or tempfile.mkdtemp(prefix="bench_loc_"))
    work.mkdir(parents=True, exist_ok=True)
    try:
        t0 = time.perf_counter()
        write_bed(work / "in.bed", a.rows, rng)
        csv_rows, n_hits = write_occ(work / "occ.csv", a.rows, a.conseqs, rng)
        (work / "conseq.txt").write_text("\n".join("ACGTACGTAC"[: 6 + i % 5] for i in range(a.conseqs)) + "\n")
        gen_s = time.perf_counter() - t0
        _extract_motif_locations(work / "in.bed", work / "conseq.txt", work / "occ.csv", work / "warm")   # warm-up (HIP context, page cache)
        runs = []
        for _ in range(a.repeat):
            shutil.rmtree(work / "out", ignore_errors=True)
            t = {}
            t1 = time.perf_counter()
            _extract_motif_locations(work / "in.bed", work / "conseq.txt", work / "occ.csv", work / "out", timing=t)
            t["total"] = time.perf_counter() - t1
            runs.append(t)
        best = min(runs, key=lambda t: t["total"])
        out_bytes = sum(f.stat().st_size for f in (work / "out").iterdir())
        print(json.dumps({"bench": "extract_motif_locations", "rows": a.rows, "csv_rows": csv_rows, "conseqs": a.conseqs, "hits": n_hits,
                          "bed_mb": round((work / "in.bed").stat().st_size / 1e6, 1),
                          "csv_mb": round((work / "occ.csv").stat().st_size / 1e6, 1), "out_mb": round(out_bytes / 1e6, 1),
                          "total_s": round(best["total"], 3), "parse_s": round(best["parse"], 3), "device_s": round(best["device"], 3),
                          "device_events_ms": round(best["device_ms"], 1), "format_s": round(best["format"], 3),
                          "all_totals_s": [round(t["total"], 3) for t in runs], "generate_s": round(gen_s, 1)}))
    finally:
        if a.workdir is None:
            shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    main()
