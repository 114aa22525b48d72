// pwm_batch.h -- the batched best-window-per-read pass (DESIGN.md sections 16, 18, 19): the best window of every read under every
// matrix of a BATCH of matrices in one pass over the reads.  What pwm_readscore.hip does for one matrix -- load the packed reads,
// find the reads of the tile, reduce the windows of every read to one maximum -- is done once per tile for the whole batch: the
// loads, the border search and the read segmentation do not depend on the matrix.  pwm_library.hip, pwm_presence.hip, pwm_sites.hip
// and pwm_spacing.hip include it; each instantiates the key policies it launches and keeps the reduction behind the keys.
//
//   * A key policy names what a read keeps of its best window (zero = "none": the matrix check refuses weights of 2^31 / 31 or more
//     in magnitude, pwm._check_weights' bound, so |score| <= 31 (2^31 / 31 - 1) < 2^31 - 1, the score is never INT32_MIN and a real
//     key never 0), largest key wins:
//         ScoreKey  u32  the score with the sign bit flipped; every valid window is a candidate
//         SiteKey   u64  score << 32 | (0x7FFFFFFF - loc): on a tie the smallest loc; windows below the matrix's threshold are dropped
//                        (the best window of a site read is itself at or above it; at p = 10^-4 that removes almost every atomic)
//         PairKey   u64  score << 32 | (0x7FFFFFFF - loc) << 1 | minus: pwm_readscore.hip's key, so forward and reverse scores are
//                        kept apart; thresholds as SiteKey, and a window that overlaps the read's primary site ploc[r] (or lies in a
//                        read without one, ploc[r] < 0) is never a candidate
//   * pwm_batch_kernel<RC, Policy>: persistent blocks over wave tiles of 64 groups x 16 positions like readscore_kernel.  The chunk
//     tables of the batch's matrices lie behind one another in LDS (2 KB per chunk with RC, 1 KB without: the forward sums alone);
//     every matrix has its own width, hence its own chunk count, window mask and valid test.  Per tile: load_grp and
//     tile_read_starts ONCE, then per matrix the 16 windows of the lane, reduced to segments per read exactly as readscore_kernel
//     does: a read that begins and ends inside the lane goes to its key at once, head and tail are combined by a segmented max scan
//     across the lanes, ONE atomicMax per (wave, read, matrix).  A maximum is order-free: deterministic.
//   * LDS budget: static LDS, 24 chunk tables and 8 matrices per batch -- 48 KB of tables with RC, 50.5 KB in all, so three blocks
//     share a CU's 160 KB, and __launch_bounds__(PW_TPB, 3) holds the kernel to the 168 VGPRs of three waves per SIMD (DESIGN.md
//     section 18 has the resource table of every instantiation).  Unmeasured against the alternative (dynamic LDS, up to ~70 chunks,
//     one block per CU).
//   * pwm_key_batches<Policy>: the host side -- the grid, the matrices sorted by width, the greedy batches, the scoring launch -- as a
//     function that hands every batch's keys to a callback.
#pragma once
#include <numeric>
#include <vector>

#include "common.h"
#include "pwm_internal.h"

namespace {

constexpr int PB_MAX_MAT = 8;            // matrices per batch (kmap_amd/device_seq.py: LIBRARY_BATCH)
constexpr int PB_MAX_CHUNKS = 24;        // chunk tables per batch (LIBRARY_BATCH_CHUNKS): 8 matrices of w <= 12, 3 of w >= 29
constexpr int32_t PB_MAX_WEIGHT = (int32_t)((1ll << 31) / 31);      // pwm._check_weights: |w| below this

template <bool RC> struct PwmEntry { using T = int; };              // forward sum of a chunk
template <> struct PwmEntry<true> { using T = int2; };              // (forward, reverse complement)

struct PwmBatchMats {
    int n_mat;
    int src[PB_MAX_MAT];        // the matrix's row in the weights array
    int width[PB_MAX_MAT];
    int chunk0[PB_MAX_MAT];     // its first chunk table
};
template <bool THR> struct PwmBatch : PwmBatchMats {};
template <> struct PwmBatch<true> : PwmBatchMats {
    int32_t thr[PB_MAX_MAT];    // windows below it are dropped
};

struct ScoreKey {
    using Key = unsigned int;
    static constexpr bool THR = false, LOC = false, PRIM = false;
    static __device__ __forceinline__ Key pack(int score, uint32_t, bool) { return (uint32_t)score ^ 0x80000000u; }
};
struct SiteKey {
    using Key = unsigned long long;
    static constexpr bool THR = true, LOC = true, PRIM = false;
    static __device__ __forceinline__ Key pack(int score, uint32_t loc, bool) {
        return ((uint64_t)((uint32_t)score ^ 0x80000000u) << 32) | (uint64_t)(0x7FFFFFFFu - loc);
    }
};
struct PairKey {
    using Key = unsigned long long;
    static constexpr bool THR = true, LOC = true, PRIM = true;
    static __device__ __forceinline__ Key pack(int score, uint32_t loc, bool minus) {
        return ((uint64_t)((uint32_t)score ^ 0x80000000u) << 32) | ((uint64_t)(0x7FFFFFFFu - loc) << 1) | (minus ? 1u : 0u);
    }
};

// the window's score and strand: with RC the larger of the two strands' sums, a tie is '+'
template <bool RC>
__device__ __forceinline__ int pwm_chunk_score(const typename PwmEntry<RC>::T *tab, uint64_t v, int nch, bool &minus) {
    int fwd = 0, rc = 0;
#pragma unroll
    for (int c = 0; c < PW_MAX_CHUNKS; ++c)
        if (c < nch) {                     // uniform
            const uint32_t idx = (uint32_t)(v >> (56 - 8 * c)) & 255u;
            if constexpr (RC) {
                const int2 e = tab[c * 256 + idx];
                fwd += e.x;
                rc += e.y;
            } else {
                fwd += tab[c * 256 + idx];
            }
        }
    minus = RC && rc > fwd;
    return minus ? rc : fwd;
}

// P's flags are the places where the passes differ: THR drops windows below the matrix's threshold, LOC tracks the window's loc in its
// read for the key, PRIM carries the read's primary site and drops what overlaps it: ploc[r] = the loc of read r's primary site of
// prim_width columns, or -1 (unused arguments otherwise).  Every instantiation compiles to the instructions of the separate kernel
// it replaced; three things in the lane loop keep it so and are marked there.
template <bool RC, class P>
__global__ __launch_bounds__(PW_TPB, 3) void pwm_batch_kernel(const uint32_t *__restrict__ codes, const uint16_t *__restrict__ inval,
                                                              int64_t n_data, int64_t n_tiles, const int32_t *__restrict__ weights,
                                                              PwmBatch<P::THR> bt, const int64_t *__restrict__ borders, int64_t n_seq,
                                                              const int32_t *__restrict__ ploc, int prim_width,
                                                              typename P::Key *__restrict__ key) {
    using Entry = typename PwmEntry<RC>::T;
    using Key = typename P::Key;
    __shared__ Entry tab[PB_MAX_CHUNKS * 256];
    __shared__ int32_t wl[128];
    __shared__ int s_width[PB_MAX_MAT], s_chunk0[PB_MAX_MAT], s_thr[P::THR ? PB_MAX_MAT : 1];
    __shared__ uint32_t start_bits[PW_WAVES][KMAP_WAVE];
    __shared__ uint32_t start_cnt[PW_WAVES][KMAP_WAVE];
    // build_table's entries, matrix after matrix through the one staging row (columns >= width are 0 in the weights array)
#pragma unroll
    for (int m = 0; m < PB_MAX_MAT; ++m) {
        if (m < bt.n_mat) {                // uniform
            const int width = bt.width[m], nch = (width + 3) >> 2;
            if (threadIdx.x < 128) wl[threadIdx.x] = weights[(int64_t)bt.src[m] * 128 + threadIdx.x];
            if (threadIdx.x == 0) {
                s_width[m] = width;
                s_chunk0[m] = bt.chunk0[m];
                if constexpr (P::THR) s_thr[m] = bt.thr[m];
            }
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
                if constexpr (RC) tab[bt.chunk0[m] * 256 + e] = make_int2(f, r); else tab[bt.chunk0[m] * 256 + e] = f;
            }
            __syncthreads();
        }
    }
    const int lane = threadIdx.x & (KMAP_WAVE - 1), wave = threadIdx.x >> 6;
    const int n_mat = bt.n_mat;
    for (int64_t t = (int64_t)blockIdx.x * PW_WAVES + wave; t < n_tiles; t += (int64_t)gridDim.x * PW_WAVES) {
        const int64_t g = t * PW_TILE_GROUPS + lane, tile0 = t * RS_TILE_POS;
        const Grp w = load_grp(codes, inval, g, n_data, lane);
        uint32_t sb, sc;
        const int64_t r0 = tile_read_starts(borders, n_seq, tile0, lane, start_bits[wave], start_cnt[wave], sb, sc);
        const bool shared_starts = sc != (uint32_t)__builtin_popcount(sb);
        const bool split = sb != 0;                    // a read starts in this group
        uint32_t loc_first = 0;                        // loc of the group's first position (an int32 in a read)
        if constexpr (P::LOC) loc_first = (uint32_t)(g * 16 - (r0 >= 0 ? borders[2 * r0] : 0));
        int32_t pl_first = 0;                          // the primary site of the read that reaches the group from the left
        if constexpr (P::PRIM) pl_first = r0 >= 0 ? ploc[r0] : -1;
        for (int m = 0; m < n_mat; ++m) {
            const int width = __builtin_amdgcn_readfirstlane(s_width[m]), nch = (width + 3) >> 2;
            int thr = 0;
            if constexpr (P::THR) thr = __builtin_amdgcn_readfirstlane(s_thr[m]);
            const Entry *tb = tab + __builtin_amdgcn_readfirstlane(s_chunk0[m]) * 256;
            const uint64_t wmask = (1ull << width) - 1ull;
            uint32_t span = 0;                         // loc - pl + width - 1 of a window that overlaps the primary site lies below it
            if constexpr (P::PRIM) span = (uint32_t)(prim_width + width - 1);
            Key *km = key + (int64_t)m * n_seq;
            Key cur = 0, head = 0;                     // the running segment; the one that reached the lane from the left
            int64_t r = r0;
            uint32_t loc0 = loc_first;
            int32_t pl = pl_first;
            bool seen = false;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                if (sb & (0x8000u >> i)) {
                    if (!seen) {
                        head = cur;
                        seen = true;
                    } else if (cur) {
                        atomicMax(&km[r], cur);        // a read that began and ends in this group
                    }
                    cur = 0;
                    step_read(borders, n_seq, g * 16 + i, shared_starts, r);
                    if constexpr (P::LOC) loc0 = (uint32_t)-i;
                    if constexpr (P::PRIM) pl = ploc[r];   // a read start was marked, so n_seq >= 1 and 0 <= r < n_seq
                }
                bool minus;
                const int s = pwm_chunk_score<RC>(tb, win_bits(w, i), nch, minus);
                // kept: at or above the threshold; PRIM: in a read with a primary site, and ends at or before that window's first base
                // or begins at or behind its last; valid; in a read.  On purpose (1) one short-circuit condition: gathered in a bool
                // first, the same test moves the 32-bit kernel's spills (10 and 14 for 12 and 12); (2) loc0 + i written where it is
                // used: named in front of the test, the 64-bit site kernel packs its key with selects instead of a branch; (3) ploc a
                // __restrict__ argument of the kernel, not the member of a struct: the pair kernel schedules its loads otherwise.
                if ((!P::THR || s >= thr) && (!P::PRIM || (pl >= 0 && loc0 + i - (uint32_t)pl + (uint32_t)(width - 1) >= span)) &&
                    win_valid(w, i, width, wmask) && (P::PRIM || r >= 0)) {
                    const Key k = P::pack(s, loc0 + i, minus);
                    cur = k > cur ? k : cur;
                }
            }
            // lanes of one read: inclusive segmented maximum of the tails, a lane with a read start opens a segment
            Key seg = cur;
            int open = split ? 1 : 0;
            for (int o = 1; o < KMAP_WAVE; o <<= 1) {
                const Key up = __shfl_up(seg, o);
                const int up_open = __shfl_up(open, o);
                if (lane >= o && !open) {
                    seg = up > seg ? up : seg;
                    open = up_open;
                }
            }
            Key left = __shfl_up(seg, 1);              // what the lanes to the left hold of this lane's first read
            if (lane == 0) left = 0;
            if (split && r0 >= 0) {
                const Key best = head > left ? head : left;
                if (best) atomicMax(&km[r0], best);
            }
            if (lane == KMAP_WAVE - 1 && seg && r >= 0) atomicMax(&km[r], seg);     // the read that leaves the tile
        }
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------

// the argument rules of a batched entry point's matrices (`who` = its prefix in the messages): KMAP_E_INVAL for a width outside 4..31,
// a weight of 2^31 / 31 or more in magnitude or behind the width, a NULL array
inline int pwm_library_check(const char *who, int n_mat, const int32_t *widths, const int32_t *weights) {
    KMAP_REQUIRE(widths && weights, "%s: null pointer", who);
    for (int m = 0; m < n_mat; ++m) {
        KMAP_REQUIRE(widths[m] >= 4 && widths[m] <= 31, "%s: width=%d of matrix %d outside 4..31", who, widths[m], m);
        for (int e = 0; e < 128; ++e) {
            const int32_t v = weights[(size_t)m * 128 + e];
            KMAP_REQUIRE(v > -PB_MAX_WEIGHT && v < PB_MAX_WEIGHT, "%s: a weight of matrix %d is 2^31 / 31 or more: a window's score must fit int32", who, m);
            KMAP_REQUIRE((e & 31) < widths[m] || v == 0, "%s: matrix %d has a weight behind its width %d", who, m, widths[m]);
        }
    }
    return KMAP_OK;
}

// Checked matrices, n > 0, n_seq > 0, n_mat > 0: sorts them by width, batches them (8 matrices, 24 chunk tables), scores a batch on
// `st` and calls on_batch(bt, key, weights_dev) with its keys in scratch slot A: key[j n_seq + r] of the batch's matrix j = the
// caller's matrix bt.src[j], 0 = none; they are valid on the stream until on_batch returns.  on_batch enqueues its own work on `st`
// behind the scoring kernel; there is no synchronisation here.  The weights lie in slot C; slot B is the caller's.  `thresholds` is
// NULL for a policy without THR; ploc_dev and prim_width are PairKey's (NULL and 0 otherwise).
template <class P, class OnBatch>
int pwm_key_batches(const char *who, const uint32_t *codes_dev, const uint16_t *inval_dev, int64_t n, const int64_t *borders_dev,
                    int64_t n_seq, int n_mat, const int32_t *widths, const int32_t *weights, const int32_t *thresholds, int revcom,
                    const int32_t *ploc_dev, int prim_width, hipStream_t st, OnBatch on_batch) {
    using Key = typename P::Key;
    const int64_t n_data = (n + 15) >> 4, n_tiles = (n_data + PW_TILE_GROUPS - 1) / PW_TILE_GROUPS;   // groups of 16 positions; wave tiles
    // persistent blocks: as many as are resident at once (registers and LDS decide; the tables are built once per block)
    int dev = 0, cus = 0, per_cu = 0;
    KMAP_CHECK_HIP(hipGetDevice(&dev));
    KMAP_CHECK_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    if (revcom) KMAP_CHECK_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, pwm_batch_kernel<true, P>, PW_TPB, 0));
    else KMAP_CHECK_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, pwm_batch_kernel<false, P>, PW_TPB, 0));
    KMAP_REQUIRE(cus > 0 && per_cu > 0, "%s: no block of the scoring kernel fits a compute unit", who);
    const unsigned grid = (unsigned)std::min<int64_t>((n_tiles + PW_WAVES - 1) / PW_WAVES, (int64_t)cus * per_cu);

    // by width (ties: the caller's order), so that a batch holds matrices of similar chunk counts
    std::vector<int> order(n_mat);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return widths[a] < widths[b]; });

    int32_t *weights_dev = nullptr;
    KMAP_TRY(kmap_scratch((void **)&weights_dev, (size_t)n_mat * 512, st, KMAP_SLOT_C));
    KMAP_CHECK_HIP(hipMemcpyAsync(weights_dev, weights, (size_t)n_mat * 512, hipMemcpyHostToDevice, st));
    Key *key = nullptr;
    KMAP_TRY(kmap_scratch((void **)&key, (size_t)std::min(n_mat, PB_MAX_MAT) * (size_t)n_seq * sizeof(Key), st, KMAP_SLOT_A));

    for (int first = 0; first < n_mat;) {
        PwmBatch<P::THR> bt = {};
        int chunks = 0;
        while (first + bt.n_mat < n_mat && bt.n_mat < PB_MAX_MAT) {
            const int m = order[first + bt.n_mat], nch = (widths[m] + 3) / 4, j = bt.n_mat;
            if (chunks + nch > PB_MAX_CHUNKS) break;
            bt.src[j] = m;
            bt.width[j] = widths[m];
            bt.chunk0[j] = chunks;
            if constexpr (P::THR) bt.thr[j] = thresholds[m];
            chunks += nch;
            ++bt.n_mat;
        }                                              // n_mat >= 1: one matrix has 8 chunks at the most
        KMAP_CHECK_HIP(hipMemsetAsync(key, 0, (size_t)bt.n_mat * (size_t)n_seq * sizeof(Key), st));
        with_bool(revcom, [&](auto rc) {
            pwm_batch_kernel<decltype(rc)::value, P><<<grid, PW_TPB, 0, st>>>(codes_dev, inval_dev, n_data, n_tiles, weights_dev, bt,
                                                                              borders_dev, n_seq, ploc_dev, prim_width, key);
        });
        KMAP_CHECK_HIP(hipGetLastError());
        KMAP_TRY(on_batch(bt, (const Key *)key, (const int32_t *)weights_dev));
        first += bt.n_mat;
    }
    return KMAP_OK;
}

}  // namespace
