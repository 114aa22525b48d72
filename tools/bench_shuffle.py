#!/usr/bin/env python3
"""Time of shuffle_reads' device pass (csrc/shuffle.hip: the two passes over the invalid mask that list the segments, the length
pass with its read-back, the fill and the per-segment shuffle kernel) over resident reads at the C3 shape (10 M x 150 bp, generated
in HBM), klet 1 and klet 2, and beside them, in the same process, an unpack + pack of the same reads (kmap_unpack_reads_dev +
kmap_pack_reads_dev): what it costs to move the bytes a shuffle has to move, with no shuffle in between.  Times are HIP-event times
around one call, median of --reps runs after a warm-up call of each shape.  First numbers of a new kernel: there is nothing to compare
them with but that floor.  Prints one JSON object."""
import argparse
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--read_len", type=int, default=150)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=15)
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps must be at least 5")
    from kmap_amd import _ffi, synth
    assert _ffi.device_count() >= 1, "no HIP device"
    ds = synth.synth_reads_dev(args.reads, args.read_len, 3)
    out = {"device": _ffi.device_arch(), "reads": args.reads, "read_len": args.read_len, "positions": ds.n, "reps": args.reps}
    lib = _ffi.lib()
    raw = _ffi.DeviceBuffer(max(ds.n, 16))
    codes2, inval2 = _ffi.DeviceBuffer(ds.groups * 4), _ffi.DeviceBuffer(ds.groups * 2)
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

    def floor():
        _ffi.check(lib.kmap_unpack_reads_dev(ds.codes.ptr, ds.inval_orig.ptr, ds.n, raw.ptr, None))
        _ffi.check(lib.kmap_pack_reads_dev(raw.ptr, ds.n, codes2.ptr, inval2.ptr, None))
    out["unpack_pack"] = timed(floor)
    stats = (_ffi.i64 * 2)()
    for klet in (1, 2):
        def shuffle():
            _ffi.check(lib.kmap_shuffle_packed_dev(ds.codes.ptr, ds.inval_orig.ptr, ds.n, klet, args.seed, raw.ptr, stats, None))
        r = timed(shuffle)
        r.update(segments=int(stats[0]), bases=int(stats[1]), bases_per_s=int(stats[1]) / (r["ms_median"] * 1e-3),
                 ratio_to_unpack_pack=r["ms_median"] / out["unpack_pack"]["ms_median"])
        out[f"klet{klet}"] = r
    for b in (raw, codes2, inval2):
        b.free()
    ds.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
