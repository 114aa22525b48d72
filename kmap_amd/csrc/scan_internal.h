// scan_internal.h -- the occurrence-scan handle shared by scan.hip (lists, fetch, the Hamming verbs' entry points), bitslice.hip
// (hit bits of every window, k <= 16), scan_reads.hip (the per-read passes on them), scan_wide.hip (Hamming scan, k > 16) and
// pwm_scan.hip (PWM scan); and the read geometry that every per-read kernel of the Hamming scan starts with
#pragma once
#include "common.h"

struct kmap_scan {
    int64_t n_seq = 0, total = 0, cap_seq = 0, cap_pos = 0;
    int32_t *hits = nullptr;
    int8_t *mind = nullptr;
    uint64_t *offs = nullptr;           // exclusive scan of hits (run); afterwards scratch: summary words, byte-narrowed hits
    int32_t *pos = nullptr;
    // a PWM run (pwm_scan.hip) fills hits / pos like a Hamming run, plus a score and a strand per position; it has no per-read minimum distance
    int pwm = 0;                        // the last run was a PWM scan
    int32_t *score = nullptr;
    uint8_t *strand = nullptr;
    int64_t cap_score = 0;
    // the caller's declaration (kmap_scan_declare_uniform, verified on the device) that read s of these borders is
    // [s * stride, s * stride + len): the per-read kernels then take the borders from s instead of loading 16 bytes per read (scan_reads.hip)
    const void *geo_borders = nullptr;
    int64_t geo_n_seq = -1, geo_len = 0, geo_stride = 0;   // stride 0: not uniform
};
int kmap_scan_reserve(kmap_scan *s, int64_t n_seq);
int kmap_scan_reserve_pos(kmap_scan *s, uint64_t total);

// Read s of a Hamming scan over n positions: its borders clamped to [0, n) -> first position st and length L; the windows the
// reference looks at are the python slice [0 : L - k + 1] (motif_discovery.py:1443), i.e. positions [0, stop) of the read.  A
// read shorter than k - 1 has a NEGATIVE slice stop, which python counts from the read's end (quirk): its windows all run off
// the read and have the all-ones hash.  uni_stride > 0: read s is [s * uni_stride, s * uni_stride + uni_len) and the borders are
// not loaded (a declared and verified layout); the k > 16 kernels pass 0.
struct ReadSlice {
    int64_t st, L, stop;
    bool quirk;
};
__device__ __forceinline__ ReadSlice read_slice(const int64_t *__restrict__ borders, int64_t uni_len, int64_t uni_stride, int64_t s, int64_t n,
                                                int k) {
    int64_t st, en;
    if (uni_stride > 0) {                                                // wave-uniform
        st = s * uni_stride;
        en = st + uni_len;
    } else {
        st = borders[2 * s];
        en = borders[2 * s + 1];
    }
    if (st < 0) st = 0;
    if (en > n) en = n;
    const int64_t L = en > st ? en - st : 0;
    int64_t stop = L - k + 1;
    const bool quirk = stop < 0;
    if (quirk) {
        stop += L;
        if (stop < 0) stop = 0;
    }
    return {st, L, stop > L ? L : stop, quirk};
}

// bitslice.hip: hit bits of every window (k <= 16) from the bit planes of the reads (words: one uint32 per 32 windows for the
// scan; else uint16 per group for the mask's coverage pass)
int kmap_bitslice_hits(const uint32_t *planes, const uint16_t *inval, int64_t n, int k, const uint64_t *cons, const int32_t *radius,
                       int n_cons, int revcom_pairs, uint16_t *hit16, bool words, hipStream_t st);
// scan_reads.hip: the whole per-read part of the scan on those hit words in one call: one pass + a copy of the blocks' segments
// into read order (two passes when the hits do not fit the temporary buffer)
int kmap_bitslice_scan_reads_all(const uint32_t *hit32, const uint32_t *codes, const uint16_t *inval, int64_t n, const int64_t *borders,
                                 int64_t n_seq, int k, uint64_t cons, int revcom, int radius, kmap_scan *s, uint64_t *total_out,
                                 hipStream_t st);
int kmap_bitslice_declare_uniform(kmap_scan *s, const int64_t *borders, int64_t n_seq, int64_t len, int64_t stride, int *accepted, hipStream_t st);

// scan_wide.hip (k > 16, window by window): the mask's flag passes, 32 consensuses each, on the mask as it is on entry -- pass b's hit
// bits (uint16 per group) at *hit_out + b * *stride_out (KMAP_SLOT_A), *passes_out passes -- and the whole scan into s (hits, offsets, positions, total)
int kmap_wide_mask_flags(const uint32_t *codes_dev, const uint16_t *inval_dev, int64_t n, int k, const uint64_t *cons, const int32_t *radius,
                         int n_cons, uint16_t **hit_out, int64_t *stride_out, int *passes_out, hipStream_t st);
int kmap_wide_scan_run(kmap_scan *s, const uint32_t *codes_dev, const uint16_t *inval_dev, int64_t n, const int64_t *borders_dev,
                       int64_t n_seq, int k, uint64_t c, uint64_t rcc, int radius, int revcom, int64_t *total_hits, hipStream_t st);
