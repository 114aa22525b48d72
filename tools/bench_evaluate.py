#!/usr/bin/env python3
"""Time of evaluate_pwm's device pass (csrc/pwm_readscore.hip: the dense best-window-per-read kernel, the unpack kernel and the
8-byte read-back) over resident reads at the C3 shape (10 M x 150 bp, generated in HBM): a w = 11 and a w = 31 matrix on both
strands, and beside each, in the same process, one scan_pwm run (csrc/pwm_scan.hip: pass A + B) of the same matrix at p = 1e-4 --
both evaluate every window of the reads, the scan keeps the hits above a threshold, read_scores keeps one maximum per read.  Times
are HIP-event times around one call, median of --reps runs after a warm-up call of each shape.  Prints one JSON object."""
import argparse
import ctypes as C
import json
import statistics
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def consensus_matrix(consensus, rng):
    """counts of a planted motif as scan_motif would tabulate them: ~90 % consensus base, the rest spread (tools/bench_pwm.py)"""
    C4 = rng.integers(2, 6, size=(4, len(consensus)))
    for j, c in enumerate(consensus):
        C4["ACGT".index(c), j] = 90
    return C4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--read_len", type=int, default=150)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--p_value", type=float, default=1e-4)
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps must be at least 5")
    from kmap_amd import _ffi, synth
    from kmap_amd.kmer_count import kmer2hash
    from kmap_amd.motif_discovery import ReadScores
    from kmap_amd.pwm import pwm_threshold, pwm_weights
    assert _ffi.device_count() >= 1, "no HIP device"
    ds = synth.synth_reads_dev(args.reads, args.read_len, 3)
    out = {"device": _ffi.device_arch(), "reads": args.reads, "read_len": args.read_len, "positions": ds.n, "p_value": args.p_value,
           "reps": args.reps}
    lib = _ffi.lib()
    ds.scan(11, kmer2hash(synth.MOTIF_A + "A"), 2, True)          # creates the handle scan_pwm runs on
    ev0, ev1 = _ffi.Event(), _ffi.Event()

    def timed(call):
        call()                                                     # warm-up of this shape
        _ffi.sync()
        ms = []
        for _ in range(args.reps):
            ev0.record()
            call()
            ev1.record()
            _ffi.sync()
            ms.append(ev0.elapsed_ms(ev1))
        return {"ms_median": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms)}

    rng = np.random.default_rng(7)
    tot, n_scored = _ffi.i64(0), _ffi.i64(0)
    rs = ReadScores(ds.n_seq)
    for name, consensus in (("w11", synth.MOTIF_A + "A"), ("w31", (synth.MOTIF_A + synth.MOTIF_B) + "ACGTTGCA")):
        W = np.ascontiguousarray(pwm_weights(consensus_matrix(consensus, rng)), np.int32)
        t, lo, hi = pwm_threshold(W, args.p_value)

        def scan():
            _ffi.check(lib.kmap_pwm_scan_packed_dev(ds._scan, ds.codes.ptr, ds.inval_orig.ptr, ds.n, ds.borders.ptr, ds.n_seq, W.shape[1],
                                                    _ffi.ptr(W), t, 1, C.byref(tot), None))

        def read_scores():
            _ffi.check(lib.kmap_readscore_packed_dev(ds.codes.ptr, ds.inval_orig.ptr, ds.n, ds.borders.ptr, ds.n_seq, W.shape[1],
                                                     _ffi.ptr(W), 1, rs.score.ptr, rs.loc.ptr, rs.strand.ptr, C.byref(n_scored), None))
        row = {"width": int(W.shape[1]), "threshold": t, "scan_pwm": timed(scan)}
        r = timed(read_scores)
        rs.n_scored = n_scored.value
        r.update(n_scored=n_scored.value, positions_per_s=ds.n / (r["ms_median"] * 1e-3), ratio_to_scan=r["ms_median"] / row["scan_pwm"]["ms_median"])
        row["read_scores"] = r
        row["histogram"] = timed(lambda: rs.histogram(lo, hi - lo + 1))
        out[name] = row
    rs.close()
    ds.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
