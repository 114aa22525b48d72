// packed_keys.h -- the ONE place that knows how a k-mer window leaves the 2-bit packed reads (layout: packed.hip).
//   * k <= 16, a 16-position group at a time: the 16 uint32 window keys and which of them are dropped -- the pieces (smear of the
//     invalid flags, per-read-dedupe skip bits, array tail) and the keys function built from them.  Users: the hash-free partitioned
//     histograms (counts_part.hip, counts_fine.hip), the LDS histograms (counts_packed.hip) and the key-range stage
//     (counts_range.hip); the last two keep their own per-window bodies and take only the drop bits from here.
//   * any k < 32, a window at a time: Win / load_win / win_hash (hash materialisation and the generic histogram of packed.hip /
//     counts_packed.hip, the k > 16 kernels of scan_wide.hip).
#pragma once
#include "common.h"

// ---- the drop bits of a group (window i of the group in bit 15 - i) ----------------------------------------------------------------
// bad: the 48 invalid flags of groups g, g + 1, g + 2, position 0 in bit 47.  Out: bit 47 - p = OR of bad[p .. p + k - 1] = "the window
// at p touches an invalid position", by doubling; windows 0 .. 15 of the group are bits 47 .. 32 (bits above 47 hold leftovers).
__device__ __forceinline__ uint64_t smear_invalid(uint64_t bad, int k) {
    for (int have = 1; have < k;) {
        const int step = (have <= k - have) ? have : k - have;
        bad |= bad << step;
        have += step;
    }
    return bad;
}
// skip bits of per-read de-duplication (dedupe_bitmap_packed_kernel): word w covers positions 32w .. 32w+31, position 32w+j in bit
// 31-j; a set bit = "the k-mer starting here already occurred in its read".  Group g's 16 bits out of its word skip[g >> 1]:
__device__ __forceinline__ uint32_t skip16_in(uint32_t word, int64_t g) { return (word >> ((g & 1) ? 0 : 16)) & 0xFFFFu; }
__device__ __forceinline__ uint32_t skip16_of(const uint32_t *__restrict__ skip, int64_t g) {
    return skip ? skip16_in(skip[g >> 1], g) : 0u;
}
// windows that start at / behind position n: left = n - 16 g windows of the group start inside the array
__device__ __forceinline__ uint32_t tail_drop16(int64_t left) {
    return left < 16 ? (left <= 0 ? 0xFFFFu : ((1u << (16 - (int)left)) - 1u)) : 0u;
}
__device__ __forceinline__ uint32_t group_drop16(uint64_t bad, uint32_t skip16, int64_t left, int k) {
    return ((uint32_t)(smear_invalid(bad, k) >> 32) & 0xFFFFu) | skip16 | tail_drop16(left);
}

// ---- the 16 keys of a group ------------------------------------------------------------------------------------------------------
// keys[i] = hash of the window starting at position 16 g + i (hi / lo: codes of groups g, g + 1), or 0xFFFFFFFF when the window is
// dropped.  32-bit windows: v_alignbit + shift.  ONES (k = 16 can occur): the all-T 16-mer's hash IS 0xFFFFFFFF -- its valid windows
// are reported in n_ones (and leave as invalid keys); without it n_ones is left alone.
template <bool ONES>
__device__ __forceinline__ void group_keys(uint32_t hi, uint32_t lo, uint64_t bad, uint32_t skip16, int64_t left, int k,
                                           uint32_t keys[16], uint32_t &n_ones) {
    const uint32_t drop16 = group_drop16(bad, skip16, left, k);
    const int sh = 32 - 2 * k;
    if (ONES) n_ones = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const uint32_t top = (i == 0) ? hi : __builtin_amdgcn_alignbit(hi, lo, 32 - 2 * i);
        const uint32_t h = top >> sh;
        const uint32_t d = (uint32_t)__builtin_amdgcn_sbfe((int)drop16, 15 - i, 1);   // all ones when dropped
        if (ONES) n_ones += (~d & (uint32_t)(h == 0xFFFFFFFFu));
        keys[i] = h | d;
    }
}
// the same from the arrays; a group behind the array (last tile of a scatter pass) costs no loads
__device__ __forceinline__ void packed_group_keys(const uint32_t *__restrict__ codes, const uint16_t *__restrict__ inval,
                                                  const uint32_t *__restrict__ skip, int64_t n, int k, int64_t g, uint32_t keys[16],
                                                  uint32_t &n_ones) {
    if (16 * g >= n) {
#pragma unroll
        for (int i = 0; i < 16; ++i) keys[i] = 0xFFFFFFFFu;
        n_ones = 0;
        return;
    }
    const uint32_t hi = codes[g], lo = codes[g + 1];
    const uint64_t bad = ((uint64_t)inval[g] << 32) | ((uint64_t)inval[g + 1] << 16) | inval[g + 2];
    group_keys<true>(hi, lo, bad, skip16_of(skip, g), n - 16 * g, k, keys, n_ones);
}

// ---- single windows, any k < 32 ----------------------------------------------------------------------------------------------------
struct Win {
    uint64_t t0;    // bases 0..31 of the 48-base stream (group g and g+1), base 0 in bits 63:62
    uint32_t c2;    // bases 32..47 (group g+2)
    uint64_t m;     // 48 invalid flags, position 0 in bit 47
};
__device__ __forceinline__ Win load_win(const uint32_t *__restrict__ codes, const uint16_t *__restrict__ inval, int64_t g) {
    Win w;
    const uint32_t c0 = codes[g], c1 = codes[g + 1];
    w.t0 = ((uint64_t)c0 << 32) | c1;
    w.c2 = codes[g + 2];
    w.m = ((uint64_t)inval[g] << 32) | ((uint64_t)inval[g + 1] << 16) | inval[g + 2];
    return w;
}
// hash of the k bases starting at offset i (0..15) of the stream; invalid windows return all ones in the low 2k bits
// (the value the reference's invalid hash has under its "compare like any value" rule); `bad` reports invalidity.
template <bool WIDE>   // WIDE: k may exceed 16 (needs the third group)
__device__ __forceinline__ uint64_t win_hash(const Win &w, int i, int k, uint64_t kmask, bool &bad) {
    uint64_t v = w.t0 << (2 * i);
    if (WIDE && i > 0) v |= (uint64_t)w.c2 >> (32 - 2 * i);
    const uint64_t h = v >> (64 - 2 * k);
    bad = ((w.m >> (48 - i - k)) & ((1ull << k) - 1ull)) != 0;
    return bad ? kmask : h;
}
