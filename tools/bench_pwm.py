#!/usr/bin/env python3
"""Throughput of the weight-matrix scan (csrc/pwm_scan.hip) over resident reads at the C3 shape (10 M x 150 bp, generated in HBM):
a w = 11 and a w = 31 matrix at p = 1e-4 on both strands, and in the same process the Hamming-ball scan of a k = 11 consensus
on the same reads.  Times are HIP-event times around one call (its kernels, the scan of the tile counts and the 8-byte read-back of
the total between its two passes), median of --reps runs after a warm-up call of each shape.  The byte floor is the 0.375 B per
position of the packed reads (codes + invalid mask) at 8 TB/s.  Prints one JSON object."""
import argparse
import ctypes as C
import json
import statistics
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

HBM_PEAK = 8.0e12
BYTES_PER_POSITION = 0.375


def consensus_matrix(consensus, rng):
    """counts of a planted motif as scan_motif would tabulate them: ~90 % consensus base, the rest spread"""
    C4 = rng.integers(2, 6, size=(4, len(consensus)))
    for j, c in enumerate(consensus):
        C4["ACGT".index(c), j] = 90
    return C4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--read_len", type=int, default=150)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--p_value", type=float, default=1e-4)
    args = ap.parse_args()
    if args.reps < 10:
        ap.error("--reps must be at least 10")
    from kmap_amd import _ffi, synth
    from kmap_amd.kmer_count import kmer2hash
    from kmap_amd.pwm import pwm_threshold, pwm_weights
    assert _ffi.device_count() >= 1, "no HIP device"
    ds = synth.synth_reads_dev(args.reads, args.read_len, 3)
    n = ds.n
    floor_ms = n * BYTES_PER_POSITION / HBM_PEAK * 1e3
    out = {"device": _ffi.device_arch(), "reads": args.reads, "read_len": args.read_len, "positions": n, "p_value": args.p_value,
           "reps": args.reps, "byte_floor_ms": floor_ms}
    lib = _ffi.lib()
    ds.scan(11, kmer2hash(synth.MOTIF_A + "A"), 2, True)          # creates the handle
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
        return statistics.median(ms), min(ms), max(ms)

    rng = np.random.default_rng(7)
    tot = _ffi.i64(0)
    for name, consensus in (("pwm_w11", synth.MOTIF_A + "A"), ("pwm_w31", (synth.MOTIF_A + synth.MOTIF_B) + "ACGTTGCA")):
        W = pwm_weights(consensus_matrix(consensus, rng))
        t, lo, hi = pwm_threshold(W, args.p_value)
        Wc = np.ascontiguousarray(W, np.int32)

        def call():
            _ffi.check(lib.kmap_pwm_scan_packed_dev(ds._scan, ds.codes.ptr, ds.inval_orig.ptr, ds.n, ds.borders.ptr, ds.n_seq, Wc.shape[1],
                                                    _ffi.ptr(Wc), t, 1, C.byref(tot), None))
        med, mn, mx = timed(call)
        out[name] = {"width": int(Wc.shape[1]), "threshold": t, "max_score": hi, "total_hits": tot.value, "ms_median": med, "ms_min": mn,
                     "ms_max": mx, "positions_per_s": n / (med * 1e-3), "share_of_byte_floor": floor_ms / med}
    cons = int(kmer2hash(synth.MOTIF_A + "A"))

    def hamming():
        _ffi.check(lib.kmap_scan_run_packed_dev(ds._scan, ds.codes.ptr, ds.inval_orig.ptr, ds.n, ds.borders.ptr, ds.n_seq, 11, cons, 2, 1,
                                                C.byref(tot), ds.planes.ptr, None))
    med, mn, mx = timed(hamming)
    out["hamming_k11_r2"] = {"total_hits": tot.value, "ms_median": med, "ms_min": mn, "ms_max": mx, "positions_per_s": n / (med * 1e-3)}
    ds.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
