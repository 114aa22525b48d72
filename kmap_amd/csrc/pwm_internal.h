// pwm_internal.h -- what pwm_scan.hip (scan_pwm), pwm_refine.hip (refine_pwm), pwm_readscore.hip (evaluate_pwm) and pwm_library.hip
// (rank_motif_library) share; DESIGN.md sections 11, 13, 14 and 16.
//   device: the chunk tables, the group loads, the window helpers, pass A (pwm_hits_kernel: hit bit per position + hit count per wave
//           tile), for_each_hit, the ONE sparse traversal of pass A's hits that every later pass of scan and refine is a call of,
//           and tile_read_starts, the reads of a wave tile for the two dense per-read passes
//   host:   PwmPlan (an entry point's checks, the weights as a kernel argument, the launch geometry), pwm_pass_a (scratch, launch,
//           exclusive scan of the tile counts, total), with_bool (a run-time flag as a template argument)
// pwm_batch.h holds the batched dense pass of the library verbs (DESIGN.md sections 16, 18 to 20).
#pragma once
#include <algorithm>
#include <type_traits>

#include "common.h"
#include "scan_util.h"

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
// groups at or behind n_data read as the halo does (all invalid); g + 1 and g + 2 of a data group lie inside the arrays (two halo groups).
// SIGNED: the wave's first lanes may stand in front of the array (pwm_erase.hip: lanes 0 and 1 of the first tile hold groups -2 and -1);
// a group in front of 0 reads as the halo does too
template <bool SIGNED = false>
__device__ __forceinline__ Grp load_grp(const uint32_t *__restrict__ codes, const uint16_t *__restrict__ inval, int64_t g, int64_t n_data,
                                        int lane) {
    const bool in = (!SIGNED || g >= 0) && g < n_data;
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
        cnt = wave_sum(cnt);
        if (lane == 0) tile_cnt[t] = cnt;
    }
}

// the read of array position p: the last one that starts at or before it (a valid window cannot cross the 255 behind a read)
__device__ __forceinline__ int64_t find_read(const int64_t *__restrict__ borders, int64_t n_seq, int64_t p) {
    int64_t lo = 0, hi = n_seq;            // borders[2 lo] <= p (or lo == 0), borders[2 hi] > p (or hi == n_seq)
    while (hi - lo > 1) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (borders[2 * mid] <= p) lo = mid; else hi = mid;
    }
    return lo;
}

// ---- the reads of a wave tile: what the dense per-read passes share (pwm_readscore.hip, pwm_batch.h) -----------------------------
constexpr int RS_TILE_POS = PW_TILE_GROUPS * 16;      // 1024 positions per wave tile

// the wave's own LDS words: what its lanes wrote (stores, atomics) before is what they read after; no block barrier -- the waves of
// a block run different numbers of tiles
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// the number of reads that start before array position p (the borders ascend); the whole wave calls it with the same p and gets
// the same answer
__device__ __forceinline__ int64_t reads_before(const int64_t *__restrict__ borders, int64_t n_seq, int64_t p, int lane) {
    int64_t lo = 0, hi = n_seq;            // reads below lo start before p, reads from hi on do not
    while (lo < hi) {
        const int64_t step = (hi - lo + KMAP_WAVE - 1) / KMAP_WAVE, idx = lo + lane * step;
        const bool before = idx < hi && borders[2 * idx] < p;
        const int c = __builtin_popcountll(__ballot(before));      // the answers are 1 .. 1 0 .. 0
        if (c == 0) break;
        if (lo + c * step < hi) hi = lo + c * step;
        lo = lo + (c - 1) * step + 1;
    }
    return lo;
}

// The read starts of the wave tile that begins at array position tile0, found once per tile by the whole wave: `base` reads start
// before the tile, those from base on are marked where they start in the wave's 64 LDS words bits / cnt (per group of the tile: one
// bit per position, position 0 in bit 15, and how many reads start there -- reads may share a start).  The lane gets its group's
// words (sb, sc) and returns the last read that starts before its group's first position (-1: none).
__device__ __forceinline__ int64_t tile_read_starts(const int64_t *__restrict__ borders, int64_t n_seq, int64_t tile0, int lane,
                                                    uint32_t *bits, uint32_t *cnt, uint32_t &sb, uint32_t &sc) {
    const int64_t base = reads_before(borders, n_seq, tile0, lane);
    bits[lane] = 0;
    cnt[lane] = 0;
    wave_lds_sync();
    for (int64_t r = base + lane;; r += KMAP_WAVE) {
        const int64_t rel = r < n_seq ? borders[2 * r] - tile0 : (int64_t)RS_TILE_POS;
        const bool in = rel >= 0 && rel < RS_TILE_POS;
        if (in) {
            atomicOr(&bits[rel >> 4], 0x8000u >> (rel & 15));
            atomicAdd(&cnt[rel >> 4], 1u);
        }
        if (__ballot(in) != ~0ull) break;          // uniform: the starts ascend
    }
    wave_lds_sync();
    sb = bits[lane];
    sc = cnt[lane];
    uint32_t before = sc;                          // reads that start in the tile before this lane's group
    for (int o = 1; o < KMAP_WAVE; o <<= 1) {
        const uint32_t up = __shfl_up(before, o);
        if (lane >= o) before += up;
    }
    before -= sc;
    return base + (int64_t)before - 1;
}
// a read starts at position i of the lane's group: r moves to the last read that starts there
__device__ __forceinline__ void step_read(const int64_t *__restrict__ borders, int64_t n_seq, int64_t p, bool shared_starts, int64_t &r) {
    if (r + 1 < n_seq) ++r;
    while (shared_starts && r + 1 < n_seq && borders[2 * (r + 1)] <= p) ++r;
}

// The sparse traversal of pass A's hits, in array order per lane: the block's waves stride over the tiles with hits, a lane takes the
// hit bits of its group, scores each hit again and hands it to on_hit(i, p, r, start, v, fwd, rc): window i of the group, array
// position p, read r that starts at `start`, the window's bits (win_bits) and its scores (rc only with RC).
//   on_tile(t, bits, lane)  the whole wave, once per tile with hits, before its hits are visited: the place for wave-wide shuffles
//   READS                   the callbacks need the hit's read.  A binary search of the borders places the lane's first hit, the
//                           following ones step forward (hits ascend).  on_read(left, entered) follows the lane from read to read:
//                           (-1, r) in front of its first hit, (r, r + 1) for every border it steps over, (r, -1) behind its last
//                           hit.  What a caller gathers per read it hands in at `left` and starts anew, so at (-1, r) it holds
//                           nothing.  Without READS the borders are never touched, r = start = 0 and on_read is not called.
template <bool RC, bool READS, class OnTile, class OnHit, class OnRead>
__device__ __forceinline__ void for_each_hit(const int2 *tab, const uint32_t *__restrict__ codes, const uint16_t *__restrict__ inval,
                                             int64_t n_data, int64_t n_tiles, int nch, const uint16_t *__restrict__ hit16,
                                             const uint32_t *__restrict__ tile_cnt, const int64_t *__restrict__ borders, int64_t n_seq,
                                             OnTile on_tile, OnHit on_hit, OnRead on_read) {
    const int lane = threadIdx.x & (KMAP_WAVE - 1), wave = threadIdx.x >> 6;
    for (int64_t t = (int64_t)blockIdx.x * PW_WAVES + wave; t < n_tiles; t += (int64_t)gridDim.x * PW_WAVES) {
        if (tile_cnt[t] == 0) continue;    // uniform
        const int64_t g = t * PW_TILE_GROUPS + lane;
        const Grp w = load_grp(codes, inval, g, n_data, lane);
        uint32_t bits = g < n_data ? (uint32_t)hit16[g] : 0u;
        on_tile(t, bits, lane);
        if (bits) {        // (no `continue`: the wave meets again at the next tile's shuffles)
            int64_t r = 0, start = 0;
            if (READS) {
                r = find_read(borders, n_seq, g * 16 + (__builtin_clz(bits) - 16));
                start = borders[2 * r];
                on_read((int64_t)-1, r);
            }
            while (bits) {
                const int i = __builtin_clz(bits) - 16;
                bits &= ~(0x8000u >> i);
                const int64_t p = g * 16 + i;
                while (READS && r + 1 < n_seq) {       // hits ascend: step to the hit's read
                    const int64_t nx = borders[2 * (r + 1)];
                    if (nx > p) break;
                    on_read(r, r + 1);
                    ++r;
                    start = nx;
                }
                const uint64_t v = win_bits(w, i);
                int fwd, rc;
                win_score<RC>(tab, v, nch, fwd, rc);
                on_hit(i, p, r, start, v, fwd, rc);
            }
            if (READS) on_read(r, (int64_t)-1);
        }
    }
}
template <bool RC, bool READS, class OnHit, class OnRead>
__device__ __forceinline__ void for_each_hit(const int2 *tab, const uint32_t *__restrict__ codes, const uint16_t *__restrict__ inval,
                                             int64_t n_data, int64_t n_tiles, int nch, const uint16_t *__restrict__ hit16,
                                             const uint32_t *__restrict__ tile_cnt, const int64_t *__restrict__ borders, int64_t n_seq,
                                             OnHit on_hit, OnRead on_read) {
    for_each_hit<RC, READS>(tab, codes, inval, n_data, n_tiles, nch, hit16, tile_cnt, borders, n_seq, [](int64_t, uint32_t, int) {},
                            on_hit, on_read);
}

// ---- host ----------------------------------------------------------------------------------------------------

// f(std::true_type) or f(std::false_type): a run-time flag as a template argument, `decltype(flag)::value` inside a generic lambda
template <class F>
inline void with_bool(bool b, F f) {
    if (b) f(std::true_type{}); else f(std::false_type{});
}

struct PwmPlan {
    PwmWeights wt;
    int width, nch;
    int64_t n_data, n_tiles;   // groups of 16 positions; wave tiles of 64 groups
    unsigned grid;             // 0 when n == 0
};
// the checks of a PWM entry point (`who` = its prefix in the messages), the weights and the geometry of n positions
inline int pwm_plan(PwmPlan &pl, const char *who, int64_t n, int64_t n_seq, int width, const int32_t *weights) {
    KMAP_REQUIRE(width >= 4 && width <= 31, "%s: width=%d outside 4..31", who, width);
    KMAP_REQUIRE(weights, "%s: null weights", who);
    KMAP_REQUIRE(n >= 0 && n_seq >= 0, "%s: negative size", who);
    memset(&pl.wt, 0, sizeof pl.wt);
    for (int b = 0; b < 4; ++b)
        for (int j = 0; j < width; ++j) pl.wt.w[b][j] = weights[b * width + j];
    pl.width = width;
    pl.nch = (width + 3) / 4;
    pl.n_data = (n + 15) >> 4;
    pl.n_tiles = (pl.n_data + PW_TILE_GROUPS - 1) / PW_TILE_GROUPS;
    pl.grid = (unsigned)std::min<int64_t>((pl.n_tiles + PW_WAVES - 1) / PW_WAVES, PW_MAX_BLOCKS);
    return KMAP_OK;
}

// pass A on `st` (n_tiles > 0): hit16[n_data], tile_cnt[n_tiles] and its exclusive scan tile_off[n_tiles + 1] in the scratch slots
// HASH, B and PART; returns once *total = tile_off[n_tiles], the number of hits, has arrived
inline int pwm_pass_a(const PwmPlan &pl, const uint32_t *codes, const uint16_t *inval, int32_t threshold, int revcom, hipStream_t st,
                      uint16_t **hit16, uint32_t **tile_cnt, uint64_t **tile_off, uint64_t *total) {
    KMAP_TRY(kmap_scratch((void **)hit16, (size_t)pl.n_data * 2, st, KMAP_SLOT_HASH));
    KMAP_TRY(kmap_scratch((void **)tile_cnt, (size_t)pl.n_tiles * 4, st, KMAP_SLOT_B));
    KMAP_TRY(kmap_scratch((void **)tile_off, ((size_t)pl.n_tiles + 1) * 8, st, KMAP_SLOT_PART));
    with_bool(revcom, [&](auto rc) {
        pwm_hits_kernel<decltype(rc)::value><<<pl.grid, PW_TPB, 0, st>>>(codes, inval, pl.n_data, pl.n_tiles, pl.wt, pl.width, pl.nch,
                                                                         threshold, *hit16, *tile_cnt);
    });
    KMAP_CHECK_HIP(hipGetLastError());
    KMAP_TRY(exclusive_scan_u32(*tile_cnt, pl.n_tiles, *tile_off, st));
    *total = 0;
    KMAP_CHECK_HIP(hipMemcpyAsync(total, *tile_off + pl.n_tiles, 8, hipMemcpyDeviceToHost, st));
    KMAP_CHECK_HIP(hipStreamSynchronize(st));
    return KMAP_OK;
}

}  // namespace
