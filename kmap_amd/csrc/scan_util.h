// scan_util.h -- small shared device utilities: the scans and sums inside a wave / a block, and the exclusive scan of an array of
// uint32 counts (counts*.hip, scan_wide.hip, scan_reads.hip, ...)
#pragma once
#include "common.h"

namespace {
// ---- inside a wave / a block (1-D blocks of whole waves) ---------------------------------------------------------------------------
// inclusive prefix sum over the 64 lanes
template <typename T>
__device__ __forceinline__ T wave_inclusive_scan(T v) {
    const int lane = threadIdx.x & 63;
    for (int o = 1; o < 64; o <<= 1) {
        const T t = __shfl_up(v, o);
        if (lane >= o) v += t;
    }
    return v;
}
// sum over the 64 lanes: lane 0 holds it
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    return v;
}
// exclusive prefix sum of v over the block's WAVES * 64 threads.  wsum: WAVES words of the caller's LDS, the waves' sums after the ONE
// barrier inside (a caller that scans again through the same words puts a barrier in between); *total: the block's sum, on request.
// The lower waves are summed by the loop each caller had: to `wave` without a total, a fixed-count predicated one with it (one
// fixed-count loop for both costs part_scatter_kernel three to five VGPRs)
template <int WAVES, typename T>
__device__ __forceinline__ T block_exclusive_scan(T v, T *wsum, T *total = nullptr) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const T inc = wave_inclusive_scan(v);
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    T off = 0;
    if (total) {
        T all = 0;
        for (int w = 0; w < WAVES; ++w) {
            if (w < wave) off += wsum[w];
            all += wsum[w];
        }
        *total = all;
    } else {
        for (int w = 0; w < wave; ++w) off += wsum[w];
    }
    return off + (inc - v);
}

// exclusive scan of n uint32 (IN: or uint64) values into uint64 offsets by ONE block (n up to a few million);
// total written to *total
template <typename IN>
__global__ __launch_bounds__(1024) void scan_single_block_kernel(const IN *__restrict__ in, int64_t n,
                                                                 uint64_t *__restrict__ out,
                                                                 uint64_t *__restrict__ total) {
    __shared__ uint64_t part[1024];
    const int t = threadIdx.x;
    const int64_t chunk = (n + 1023) / 1024;
    const int64_t lo = (int64_t)t * chunk, hi = (lo + chunk < n) ? lo + chunk : n;
    uint64_t s = 0;
    for (int64_t i = lo; i < hi; ++i) s += in[i];
    part[t] = s;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {   // Hillis-Steele inclusive scan
        uint64_t v = (t >= o) ? part[t - o] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    uint64_t run = (t == 0) ? 0 : part[t - 1];
    for (int64_t i = lo; i < hi; ++i) {
        out[i] = run;
        run += in[i];
    }
    if (t == 1023) *total = part[1023];
}


// ---- multi-block exclusive scan: uint32 in -> uint64 out (+ total) -------------------------------------------
// phase 1: per-tile sums; phase 2: single-block scan of the tile sums; phase 3: per-tile scan + tile offset.
// ACC is the type a tile of SCAN_TILE values is summed in.  The contract of uint32_t: every tile sums to less than 2^32 -- flags,
// per-block and per-bucket counts, whose tile sum is bounded by the number of items behind the tile.  A caller that cannot promise
// that (k-mer counts: kmap_label_prefix_dev) asks for uint64_t.
constexpr int SCAN_TPB = 256;
constexpr int SCAN_ITEMS = 8;
constexpr int SCAN_TILE = SCAN_TPB * SCAN_ITEMS;

template <typename ACC>
__global__ __launch_bounds__(SCAN_TPB) void scan_tile_sums_kernel(const uint32_t *__restrict__ in, int64_t n,
                                                                  ACC *__restrict__ tile_sums) {
    __shared__ ACC ws[SCAN_TPB / 64];
    const int64_t base = (int64_t)blockIdx.x * SCAN_TILE + (int64_t)threadIdx.x * SCAN_ITEMS;
    ACC s = 0;
#pragma unroll
    for (int i = 0; i < SCAN_ITEMS; ++i)
        if (base + i < n) s += in[base + i];
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) tile_sums[blockIdx.x] = ws[0] + ws[1] + ws[2] + ws[3];   // ACC = uint32_t: < 2^32 per tile is the caller's promise
}

template <typename ACC>
__global__ __launch_bounds__(SCAN_TPB) void scan_tiles_kernel(const uint32_t *__restrict__ in, int64_t n,
                                                              const uint64_t *__restrict__ tile_off,
                                                              uint64_t *__restrict__ out) {
    __shared__ ACC ws[SCAN_TPB / 64];
    const int64_t base = (int64_t)blockIdx.x * SCAN_TILE + (int64_t)threadIdx.x * SCAN_ITEMS;
    uint32_t v[SCAN_ITEMS];
    ACC s = 0;
#pragma unroll
    for (int i = 0; i < SCAN_ITEMS; ++i) {
        v[i] = (base + i < n) ? in[base + i] : 0u;
        s += v[i];
    }
    uint64_t run = tile_off[blockIdx.x] + block_exclusive_scan<SCAN_TPB / 64>(s, ws);
#pragma unroll
    for (int i = 0; i < SCAN_ITEMS; ++i) {
        if (base + i < n) out[base + i] = run;
        run += v[i];
    }
}

// out[0..n) = exclusive prefix sums of in, out[n] = total.  tile scratch from the arena (slots C and D).  ACC: see above -- with the
// default every SCAN_TILE-aligned tile of `in` must sum to less than 2^32 (n <= 4096 is summed in 64 bits either way).
template <typename ACC = uint32_t>
inline int exclusive_scan_u32(const uint32_t *in, int64_t n, uint64_t *out, hipStream_t st) {
    if (n <= 4096) {
        scan_single_block_kernel<uint32_t><<<1, 1024, 0, st>>>(in, n, out, out + n);
        return KMAP_OK;
    }
    const int64_t tiles = (n + SCAN_TILE - 1) / SCAN_TILE;
    ACC *tsum = nullptr;
    uint64_t *toff = nullptr;
    KMAP_TRY(kmap_scratch((void **)&tsum, (size_t)tiles * sizeof(ACC), st, KMAP_SLOT_C));
    KMAP_TRY(kmap_scratch((void **)&toff, ((size_t)tiles + 1) * 8, st, KMAP_SLOT_D));
    scan_tile_sums_kernel<ACC><<<(unsigned)tiles, SCAN_TPB, 0, st>>>(in, n, tsum);
    scan_single_block_kernel<ACC><<<1, 1024, 0, st>>>(tsum, tiles, toff, out + n);   // total lands in out[n]
    scan_tiles_kernel<ACC><<<(unsigned)tiles, SCAN_TPB, 0, st>>>(in, n, toff, out);
    return KMAP_OK;
}
// the same, then *total = out[n] on the host: returns after st has been synchronised
inline int exclusive_scan_total(const uint32_t *in, int64_t n, uint64_t *out, uint64_t *total, hipStream_t st) {
    KMAP_TRY(exclusive_scan_u32(in, n, out, st));
    KMAP_CHECK_HIP(hipMemcpyAsync(total, out + n, 8, hipMemcpyDeviceToHost, st));
    KMAP_CHECK_HIP(hipStreamSynchronize(st));
    return KMAP_OK;
}
}  // namespace
