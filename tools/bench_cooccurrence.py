#!/usr/bin/env python3
"""Times of motif_cooccurrence's two device passes.
(a) Presence: csrc/pwm_presence.hip (pwm_library.hip's batched scoring pass + the ballot kernel) over resident reads at the C3 shape
    (10 M x 150 bp, generated in HBM) for the M = 16 matrices of tools/bench_library.py on both strands at their p = 10^-4
    thresholds, into planes allocated once.  Beside it, in the same process and on the same inputs: library_histograms, the pass it
    shares the scoring with.
(b) Pairs: csrc/bit_pairs.hip on seeded synthetic planes of --rows x --reads bits (every word the AND of five random words: a
    density of 1/32) and on the 16 real rows of (a).  Beside it the path it replaces, on the first --host_rows synthetic rows: fetch,
    np.unpackbits, integer matrix product (in chunks of 2^20 bits); its one run is scaled by the number of row pairs to the full
    matrix, which is an extrapolation and is marked as one.  The device result for those rows must equal the host's, which is checked.
Times are HIP-event times, median of --reps runs after a warm-up.  Prints one JSON object."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from bench_library import library_matrices  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--read_len", type=int, default=150)
    ap.add_argument("--matrices", type=int, default=16)
    ap.add_argument("--rows", type=int, default=2048)
    ap.add_argument("--host_rows", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps must be at least 5")
    from kmap_amd import _ffi, synth
    from kmap_amd.device_seq import PresencePlanes, bitrows_pair_counts
    from kmap_amd.pwm import pwm_threshold, pwm_weights
    assert _ffi.device_count() >= 1, "no HIP device"
    ds = synth.synth_reads_dev(args.reads, args.read_len, 3)
    rng = np.random.default_rng(7)
    Ws = [np.ascontiguousarray(pwm_weights(C4), np.int32) for C4 in library_matrices(args.matrices, rng)]
    plans = [pwm_threshold(W, 1e-4) for W in Ws]
    ts, los, nbs = [p[0] for p in plans], [p[1] for p in plans], [p[2] - p[1] + 1 for p in plans]
    out = {"device": _ffi.device_arch(), "reads": args.reads, "read_len": args.read_len, "positions": ds.n, "reps": args.reps,
           "matrices": args.matrices, "widths": [int(W.shape[1]) for W in Ws], "thresholds": ts}
    ev0, ev1 = _ffi.Event(), _ffi.Event()
    kept = {}

    def timed(call, reps=args.reps):
        call()                                                     # warm-up of this path
        _ffi.sync()
        ms = []
        for _ in range(reps):
            ev0.record()
            call()
            ev1.record()
            _ffi.sync()
            ms.append(ev0.elapsed_ms(ev1))
        return {"ms_median": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms)}

    # ---- (a) presence ---------------------------------------------------------------------------------------------------------
    n_mat = len(Ws)
    widths, weights = np.array([W.shape[1] for W in Ws], np.int32), np.zeros((n_mat, 4, 32), np.int32)
    for m, W in enumerate(Ws):
        weights[m, :, :W.shape[1]] = W
    thr = np.array(ts, np.int32)
    real = PresencePlanes(n_mat, ds.n_seq)                         # allocated once: the calls are timed, not hipMalloc

    def presence():
        _ffi.check(_ffi.lib().kmap_presence_library_dev(ds.codes.ptr, ds.inval_orig.ptr, ds.n, ds.borders.ptr, ds.n_seq, n_mat,
                                                        _ffi.ptr(widths), _ffi.ptr(weights), _ffi.ptr(thr), 1, real.planes.ptr,
                                                        real.n_words, _ffi.ptr(real.n_present), None))

    def histograms():
        kept["histograms"] = ds.library_histograms(Ws, los, nbs, True)

    out["library_histograms"] = timed(histograms)
    out["library_presence"] = timed(presence)
    out["ratio_presence_to_histograms"] = out["library_presence"]["ms_median"] / out["library_histograms"]["ms_median"]
    out["n_present"] = real.n_present.tolist()
    hists = kept["histograms"][0]
    for m, (t, lo) in enumerate(zip(ts, los)):                     # the reads at or above the threshold, from the score histogram
        assert int(hists[m][t - lo:].sum()) == int(real.n_present[m]), m

    # ---- (b) pairs ------------------------------------------------------------------------------------------------------------
    def pairs_of(planes, rows, words):
        return lambda: kept.__setitem__("pairs", bitrows_pair_counts(planes, rows, words))

    out["pairs_real"] = timed(pairs_of(real.planes, n_mat, real.n_words))
    assert np.array_equal(np.diagonal(kept["pairs"]), real.n_present)
    out["pairs_real"]["word_pairs"] = n_mat * (n_mat + 1) // 2 * real.n_words

    rows, n_words = args.rows, (args.reads + 63) // 64
    synth_planes = _ffi.DeviceBuffer(rows * n_words * 8)
    host_rows = min(args.host_rows, rows)
    head = None
    t0 = time.perf_counter()
    for r0 in range(0, rows, 64):                                  # 64 rows at a time: the host never holds the whole matrix
        n = min(64, rows - r0)
        block = rng.integers(0, 2 ** 64, (n, n_words), dtype=np.uint64)
        for _ in range(4):
            block &= rng.integers(0, 2 ** 64, (n, n_words), dtype=np.uint64)
        if args.reads % 64:
            block[:, -1] &= np.uint64((1 << (args.reads % 64)) - 1)
        _ffi.check(_ffi.lib().kmap_memcpy_h2d(synth_planes.ptr + r0 * n_words * 8, _ffi.ptr(block), block.nbytes, None))
        _ffi.sync()
        if r0 == 0:
            head = block[:host_rows].copy()
    out["synthetic"] = {"rows": rows, "bits": args.reads, "words": n_words, "density": 1 / 32, "host_seconds_to_make": time.perf_counter() - t0}
    out["pairs_synthetic"] = timed(pairs_of(synth_planes, rows, n_words))
    device_pairs = kept["pairs"]
    word_pairs = rows * (rows + 1) // 2 * n_words
    tiles = (rows + 63) // 64
    computed = tiles * (tiles + 1) // 2 * 4096 * n_words           # what the kernel works on: whole 64 x 64 tiles, the diagonal ones too
    sec = out["pairs_synthetic"]["ms_median"] / 1e3
    out["pairs_synthetic"].update(word_pairs=word_pairs, word_pairs_per_s=word_pairs / sec, computed_word_pairs=computed,
                                  computed_word_pairs_per_s=computed / sec)
    out["pairs_real"]["word_pairs_per_s"] = out["pairs_real"]["word_pairs"] / (out["pairs_real"]["ms_median"] / 1e3)

    if host_rows == 0:                                             # --host_rows 0: the device passes alone (for a profiler run)
        real.close()
        synth_planes.free()
        ds.close()
        print(json.dumps(out))
        return
    # the path it replaces, once, on the first host_rows rows
    t0 = time.perf_counter()
    fetched = synth_planes.to_numpy(np.uint64, (host_rows, n_words))
    _ffi.sync()
    host_pairs = np.zeros((host_rows, host_rows), np.int64)
    step = (1 << 20) // 64
    for w0 in range(0, n_words, step):
        bits = np.unpackbits(fetched[:, w0:w0 + step].view(np.uint8), axis=1, bitorder="little").astype(np.int32)
        host_pairs += bits @ bits.T
    host_s = time.perf_counter() - t0
    assert np.array_equal(fetched, head)
    np.testing.assert_array_equal(device_pairs[:host_rows, :host_rows], host_pairs)
    scale = (rows * (rows + 1) / 2) / (host_rows * (host_rows + 1) / 2)
    out["host_path"] = {"rows": host_rows, "seconds": host_s, "runs": 1, "extrapolated_seconds_all_rows": host_s * scale,
                        "extrapolation": "the sampled rows' time multiplied by the ratio of the numbers of row pairs; not a measurement"}
    real.close()
    synth_planes.free()
    ds.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
