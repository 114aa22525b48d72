#!/usr/bin/env python3
"""First numbers of the enrichment kernels (csrc/enrich.hip) at the C3 shape: foreground and control reads of 10 M x 150 bp generated
in HBM (the control without planted motifs), per-read dedupe, both strands.  For k = 8, 12, 16: HIP-event times of the directory
build (kmap_enrich_set_control), of lookup + score (kmap_enrich_run) and of the selection at top_n = 1000 (kmap_enrich_select, which
reads six small histograms and the selected rows back), median of --reps runs after a warm-up of each.  Beside them the host path
the verb replaces: fetch of both tables, np.searchsorted join of both strands, float64 z and np.argpartition, wall clock, one run;
skipped above --host_max table entries (at k = 16 the two tables are ~40 GB of host arrays).  Prints one JSON object."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def np_revcom(x, k):
    com = np.uint64(4 ** k - 1) - x.astype(np.uint64)
    out = np.zeros_like(com)
    for _ in range(k):
        out = (out << np.uint64(2)) | (com & np.uint64(3))
        com >>= np.uint64(2)
    return out


def host_path(dc_f, dc_b, k, Nf, Nb, top_n):
    t0 = time.perf_counter()
    uf, cf = dc_f.fetch()
    ub, cb = dc_b.fetch()
    t1 = time.perf_counter()

    def look(x):
        pos = np.minimum(np.searchsorted(ub, x), len(ub) - 1)
        return np.where(ub[pos] == x, cb[pos], 0).astype(np.float64)
    b = look(uf) + look(np_revcom(uf, k).astype(uf.dtype))
    a = cf.astype(np.float64)
    s = (a + b) * (Nf + Nb - a - b) * (float(Nf) * float(Nb) / float(Nf + Nb))
    z = np.where(s > 0, (a * Nb - b * Nf) / np.sqrt(np.where(s > 0, s, 1.0)), 0.0)
    z[cf < 2] = -np.inf
    top = np.argpartition(-z, min(top_n, len(z) - 1))[:top_n]
    top = top[np.lexsort((top, -z[top]))]
    t2 = time.perf_counter()
    return {"fetch_s": t1 - t0, "join_score_select_s": t2 - t1, "total_s": t2 - t0, "best_z": float(z[top[0]])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--read_len", type=int, default=150)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--top_n", type=int, default=1000)
    ap.add_argument("--host_max", type=int, default=200_000_000, help="largest number of table entries (both tables) for the host path")
    ap.add_argument("--kmer_len", type=int, action="append")
    args = ap.parse_args()
    from kmap_amd import _ffi, synth
    from kmap_amd.enrichment import DeviceEnrich
    from kmap_amd.kmer_count import DeviceCounts
    assert _ffi.device_count() >= 1, "no HIP device"
    fg = synth.synth_reads_dev(args.reads, args.read_len, 3)
    ctl = synth.synth_reads_dev(args.reads, args.read_len, 4, fractions=(0.0, 0.0))
    out = {"device": _ffi.device_arch(), "reads": args.reads, "read_len": args.read_len, "reps": args.reps, "top_n": args.top_n}
    ev0, ev1 = _ffi.Event(), _ffi.Event()

    def timed(call):
        call()
        _ffi.sync()
        ms = []
        for _ in range(args.reps):
            ev0.record()
            call()
            ev1.record()
            _ffi.sync()
            ms.append(ev0.elapsed_ms(ev1))
        return {"ms_median": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms)}

    dc_f, dc_b, en = DeviceCounts(), DeviceCounts(), DeviceEnrich()
    for k in args.kmer_len or [8, 12, 16]:
        n_fg = fg.count(dc_f, k, True, True, use_work=False)
        Nf = dc_f.total()
        ctl.count(dc_b, k, True, True, use_work=False)
        Nb = dc_b.total()
        n_ctl = ctl.count(dc_b, k, True, False, use_work=False)
        row = {"n_fg_uniq": n_fg, "n_control_uniq": n_ctl, "Nf": Nf, "Nb": Nb}
        row["directory"] = timed(lambda: en.set_control(dc_b, True))
        row["lookup_score"] = timed(lambda: en.run(dc_f, Nf, Nb, 2))
        row["lookup_score"]["entries_per_s"] = n_fg / (row["lookup_score"]["ms_median"] * 1e-3)
        row["select"] = timed(lambda: en.select(args.top_n))
        row["n_eligible"], row["n_selected"] = en.n_eligible, en.n_sel
        sel = en.fetch()
        row["best_z"] = float(sel[4][0]) if en.n_sel else None
        row["host"] = host_path(dc_f, dc_b, k, Nf, Nb, args.top_n) if n_fg + n_ctl <= args.host_max else "skipped: tables above --host_max entries"
        out[f"k{k}"] = row
        print(json.dumps({f"k{k}": row}), file=sys.stderr, flush=True)
    for h in (en, dc_f, dc_b, fg, ctl):
        h.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
