// pwm_internal.h -- the device side shared by pwm_scan.hip (scan_pwm) and pwm_refine.hip (refine_pwm): the chunk tables, the group
// loads, the window helpers and pass A (hit bit per position + hit count per wave tile); DESIGN.md sections 11 and 13
#pragma once
#include "common.h"

namespace {

constexpr int PW_TPB = 256;
constexpr int PW_WAVES = PW_TPB / KMAP_WAVE;
constexpr int PW_MAX_BLOCKS = 2048;      // 8 blocks of 4 waves on each of 256 CUs: the blocks are persistent, the table is built once each
constexpr int PW_MAX_CHUNKS = 8;
constexpr int PW_TILE_GROUPS = KMAP_WAVE;   // a wave's tile: 64 groups = 1024 positions

struct PwmWeights {
    int32_t w[4][32];   // rows A C G T; columns >= width are 0
};

// chunk tables in LDS: entry [c][b0 b1 b2 b3] = (sum_j W[b_j][4c + j], sum_j W[3 - b_j][width - 1 - (4c + j)]) over the columns 4c + j < width
__device__ __forceinline__ void build_table(int2 *tab, int32_t *wl, const PwmWeights &wt, int width, int nch) {
    if (threadIdx.x < 128) wl[threadIdx.x] = wt.w[threadIdx.x >> 5][threadIdx.x & 31];
    __syncthreads();
    for (int e = threadIdx.x; e < nch * 256; e += PW_TPB) {
        const int c = e >> 8, idx = e & 255;
        int f = 0, r = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int col = 4 * c + j, b = (idx >> (6 - 2 * j)) & 3;
            if (col < width) {
                f += wl[b * 32 + col];
                r += wl[(3 - b) * 32 + (width - 1 - col)];
            }
        }
        tab[e] = make_int2(f, r);
    }
    __syncthreads();
}

struct Grp {
    uint64_t t0;    // bases 0..31 of the 48-base stream (groups g, g + 1), base 0 in bits 63:62
    uint32_t c2;    // bases 32..47 (group g + 2)
    uint64_t m;     // 48 invalid flags, position 0 in bit 47
};
// groups at or behind n_data read as the halo does (all invalid); g + 1 and g + 2 of a data group lie inside the arrays (two halo groups)
__device__ __forceinline__ Grp load_grp(const uint32_t *__restrict__ codes, const uint16_t *__restrict__ inval, int64_t g, int64_t n_data,
                                        int lane) {
    const bool in = g < n_data;
    const uint32_t c0 = in ? codes[g] : 0u, m0 = in ? (uint32_t)inval[g] : 0xFFFFu;
    uint32_t c1 = __shfl_down(c0, 1), c2 = __shfl_down(c0, 2), m1 = __shfl_down(m0, 1), m2 = __shfl_down(m0, 2);
    if (lane >= KMAP_WAVE - 2) {           // the neighbours belong to the next wave's tile
        if (lane == KMAP_WAVE - 1) {
            c1 = in ? codes[g + 1] : 0u;
            m1 = in ? (uint32_t)inval[g + 1] : 0xFFFFu;
        }
        c2 = in ? codes[g + 2] : 0u;
        m2 = in ? (uint32_t)inval[g + 2] : 0xFFFFu;
    }
    Grp w;
    w.t0 = ((uint64_t)c0 << 32) | c1;
    w.c2 = c2;
    w.m = ((uint64_t)m0 << 32) | ((uint64_t)m1 << 16) | m2;
    return w;
}
// the 32 bases from offset i (0..15) of the stream, first base in bits 63:62
__device__ __forceinline__ uint64_t win_bits(const Grp &w, int i) {
    uint64_t v = w.t0 << (2 * i);
    if (i > 0) v |= (uint64_t)w.c2 >> (32 - 2 * i);
    return v;
}
__device__ __forceinline__ bool win_valid(const Grp &w, int i, int width, uint64_t wmask) {
    return ((w.m >> (48 - i - width)) & wmask) == 0;
}
template <bool RC>
__device__ __forceinline__ void win_score(const int2 *tab, uint64_t v, int nch, int &fwd, int &rc) {
    fwd = 0;
    rc = 0;
#pragma unroll
    for (int c = 0; c < PW_MAX_CHUNKS; ++c)
        if (c < nch) {                     // uniform
            const uint32_t idx = (uint32_t)(v >> (56 - 8 * c)) & 255u;
            if (RC) {
                const int2 e = tab[c * 256 + idx];
                fwd += e.x;
                rc += e.y;
            } else {
                fwd += tab[c * 256 + idx].x;
            }
        }
}

// pass A: hit bits of every group + hit count of every wave tile
template <bool RC>
__global__ __launch_bounds__(PW_TPB) void pwm_hits_kernel(const uint32_t *__restrict__ codes, const uint16_t *__restrict__ inval,
                                                          int64_t n_data, int64_t n_tiles, PwmWeights wt, int width, int nch,
                                                          int32_t thr, uint16_t *__restrict__ hit16, uint32_t *__restrict__ tile_cnt) {
    __shared__ int2 tab[PW_MAX_CHUNKS * 256];
    __shared__ int32_t wl[128];
    build_table(tab, wl, wt, width, nch);
    const int lane = threadIdx.x & (KMAP_WAVE - 1), wave = threadIdx.x >> 6;
    const uint64_t wmask = (1ull << width) - 1ull;
    for (int64_t t = (int64_t)blockIdx.x * PW_WAVES + wave; t < n_tiles; t += (int64_t)gridDim.x * PW_WAVES) {
        const int64_t g = t * PW_TILE_GROUPS + lane;
        const Grp w = load_grp(codes, inval, g, n_data, lane);
        uint32_t bits = 0;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            int fwd, rc;
            win_score<RC>(tab, win_bits(w, i), nch, fwd, rc);
            const int s = RC ? (rc > fwd ? rc : fwd) : fwd;
            if (win_valid(w, i, width, wmask) && s >= thr) bits |= 0x8000u >> i;
        }
        if (g < n_data) hit16[g] = (uint16_t)bits;
        uint32_t cnt = (uint32_t)__builtin_popcount(bits);
        for (int o = 32; o; o >>= 1) cnt += __shfl_down(cnt, o);
        if (lane == 0) tile_cnt[t] = cnt;
    }
}

}  // namespace
