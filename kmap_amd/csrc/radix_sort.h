// radix_sort.h -- the library's one stable LSD radix sort, 8-bit digits: keys of WORDS uint64 words (word 0 the least significant),
// optionally a uint32 payload that moves with its key.  counts_sort.hip sorts one-word k-mer hashes with it, locations.hip two-word
// composite keys with the interval index as payload.
//
// A pass over one digit: (1) every wave histograms its tile of 1024 keys (64 lanes x 16, striped) into 256 LDS counters ->
// counts[digit][tile]; (2) exclusive scan of the digit-major counts; (3) every wave ranks its tile's keys again -- lanes holding the
// same digit find each other with eight ballots (one per digit bit), a lane's rank is the digit's running count + the lanes of its
// group in front of it, the group's first lane bumps the count: stable, no atomics -- and stores key i at offset[digit][tile] + rank.
#pragma once
#include <utility>

#include "scan_util.h"

namespace {
constexpr int RS_ITEMS = 16, RS_TILE = KMAP_WAVE * RS_ITEMS, RS_WAVES = 4;   // 1024 keys per wave; four independent waves per block

// one set of key buffers, passed to the kernels by value: the key words, and with them the payload
template <int WORDS>
struct RsWords {
    uint64_t *w[WORDS];
};
template <int WORDS, bool VAL>
struct RsBufs : RsWords<WORDS> {
    uint32_t *val;                                                        // null unless VAL
};

// reads only the word that holds the digit
template <int WORDS>
__global__ __launch_bounds__(KMAP_WAVE *RS_WAVES) void rs_hist_kernel(RsWords<WORDS> in, int64_t n, int shift, int64_t n_tiles,
                                                                      uint32_t *__restrict__ counts) {
    __shared__ uint32_t cnt[RS_WAVES][256];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t tile = (int64_t)blockIdx.x * RS_WAVES + wave;
    const uint64_t *__restrict__ kw = in.w[WORDS == 1 ? 0 : shift >> 6];
    const int sh = shift & 63;
    for (int d = lane; d < 256; d += 64) cnt[wave][d] = 0;
    __builtin_amdgcn_wave_barrier();
    if (tile < n_tiles) {
#pragma unroll
        for (int i = 0; i < RS_ITEMS; ++i) {
            const int64_t idx = tile * RS_TILE + (int64_t)i * KMAP_WAVE + lane;
            if (idx < n) atomicAdd(&cnt[wave][(kw[idx] >> sh) & 255u], 1u);
        }
    }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_s_waitcnt(0xC07F);
    if (tile < n_tiles)
        for (int d = lane; d < 256; d += 64) counts[(int64_t)d * n_tiles + tile] = cnt[wave][d];
}

template <int WORDS, bool VAL>
__global__ __launch_bounds__(KMAP_WAVE *RS_WAVES) void rs_scatter_kernel(RsBufs<WORDS, VAL> in, int64_t n, int shift, int64_t n_tiles,
                                                                         const uint64_t *__restrict__ offs, RsBufs<WORDS, VAL> out) {
    __shared__ uint32_t cnt[RS_WAVES][256];
    __shared__ uint64_t base[RS_WAVES][256];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t tile = (int64_t)blockIdx.x * RS_WAVES + wave;
    if (tile >= n_tiles) return;                                          // wave-uniform; no block-wide barrier below
    for (int d = lane; d < 256; d += 64) {
        cnt[wave][d] = 0;
        base[wave][d] = offs[(int64_t)d * n_tiles + tile];
    }
    __builtin_amdgcn_wave_barrier();
    const unsigned long long lt = (1ull << lane) - 1ull;
    const int word = WORDS == 1 ? 0 : shift >> 6, sh = shift & 63;
#pragma unroll 4
    for (int i = 0; i < RS_ITEMS; ++i) {
        const int64_t idx = tile * RS_TILE + (int64_t)i * KMAP_WAVE + lane;
        const bool live = idx < n;
        uint64_t key[WORDS];
#pragma unroll
        for (int w = 0; w < WORDS; ++w) key[w] = live ? in.w[w][idx] : 0ull;
        const uint32_t dg = (uint32_t)(key[word] >> sh) & 255u;
        unsigned long long same = __ballot(live);                         // lanes with this lane's digit (and a key)
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const unsigned long long bal = __ballot((dg >> b) & 1u);
            same &= ((dg >> b) & 1u) ? bal : ~bal;
        }
        if (live) {
            const uint32_t old = cnt[wave][dg];                           // the group's lanes all read the count before its leader bumps it
            const uint32_t rank = old + (uint32_t)__popcll(same & lt);
            if ((same & lt) == 0ull) cnt[wave][dg] = old + (uint32_t)__popcll(same);
            const uint64_t to = base[wave][dg] + rank;
#pragma unroll
            for (int w = 0; w < WORDS; ++w) out.w[w][to] = key[w];
            if (VAL) out.val[to] = in.val[idx];
        }
        __builtin_amdgcn_wave_barrier();                                  // LDS operations of a wave execute in order: item i + 1 sees the bump
    }
}

// Sorts the n keys of `a` by the bits set in mask (mask[w]: word w), ascending, stable; `b` is the ping-pong partner.  One pass for
// every 8-bit digit whose mask bits are not all zero, the sets swapped after each: on return `a` names the buffers that hold the
// result and `b` the others.  Queues on st and does not synchronise it.
template <int WORDS, bool VAL>
int radix_sort(RsBufs<WORDS, VAL> &a, RsBufs<WORDS, VAL> &b, int64_t n, const uint64_t (&mask)[WORDS], hipStream_t st) {
    const int64_t n_tiles = (n + RS_TILE - 1) / RS_TILE;
    const unsigned grid = (unsigned)((n_tiles + RS_WAVES - 1) / RS_WAVES);
    DevBuf counts, offs;
    KMAP_TRY(counts.alloc((size_t)256 * n_tiles * 4));
    KMAP_TRY(offs.alloc(((size_t)256 * n_tiles + 1) * 8));
    for (int shift = 0; shift < 64 * WORDS; shift += 8) {
        if (((mask[shift >> 6] >> (shift & 63)) & 255u) == 0) continue;
        rs_hist_kernel<WORDS><<<grid, KMAP_WAVE * RS_WAVES, 0, st>>>(a, n, shift, n_tiles, counts.as<uint32_t>());
        KMAP_TRY(exclusive_scan_u32(counts.as<uint32_t>(), 256 * n_tiles, offs.as<uint64_t>(), st));
        rs_scatter_kernel<WORDS, VAL><<<grid, KMAP_WAVE * RS_WAVES, 0, st>>>(a, n, shift, n_tiles, offs.as<uint64_t>(), b);
        std::swap(a, b);
    }
    KMAP_CHECK_HIP(hipGetLastError());
    return KMAP_OK;
}
}  // namespace
