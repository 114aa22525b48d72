// pwm_refine.hip -- one iteration of refine_pwm on the device: the hits of a weight matrix on the packed
// reads (section 11's hits, pass A of pwm_scan.hip as it is), a selection among them, and the 4 x width count matrix of the selected
// windows' oriented bases.  Nothing but 126 integers leaves the device.
//
//   * pass A (pwm_hits_kernel, pwm_internal.h): hit bit per position, hit count per wave tile, exclusive scan, total = n_hits.
//   * pwm_best_kernel (select_best only): every hit is evaluated again (the sparse traversal of pwm_scan.hip's pass B: tiles with
//     hits, groups with hit bits, binary search of the borders for a lane's first hit, a step forward for the following ones) and
//     takes part in an unsigned 64-bit atomicMax on key[read], key = (score with the sign bit flipped) << 32 | (0xFFFFFFFF - loc):
//     the largest score wins, on a tie the smallest loc.  A maximum does not depend on the order of its operands, so the result is
//     deterministic.  Zero = "no hit" (a real key's low half is >= 2^31: loc is an int32).
//   * pwm_accum_kernel: the same traversal; a hit counts when its key equals key[read] (select_best) or always.  Its width oriented
//     bases -- window base j on '+', 3 - (window base width - 1 - j) on '-' -- go into a per-block LDS histogram [31][4] (+ the
//     selected / minus counters); after the grid-stride loop at most 126 threads of a block add its non-zero cells to the global
//     uint64 array, one integer atomic each (order-free).
// It uses scratch slots only: no kmap_scan handle is needed or touched.
#include <algorithm>

#include "common.h"
#include "pwm_internal.h"
#include "scan_util.h"

namespace {

constexpr int PR_CELLS = 31 * 4;          // histogram cells [column][base]
constexpr int PR_SELECTED = PR_CELLS;     // + the number of selected windows
constexpr int PR_MINUS = PR_CELLS + 1;    // + those on '-'
constexpr int PR_SLOTS = PR_CELLS + 2;    // 126

__device__ __forceinline__ uint64_t pack_key(int score, int64_t loc) {
    return ((uint64_t)((uint32_t)score ^ 0x80000000u) << 32) | (uint64_t)(0xFFFFFFFFu - (uint32_t)loc);
}

// the read of array position p: the last one that starts at or before it (pwm_write_kernel's search)
__device__ __forceinline__ int64_t find_read(const int64_t *__restrict__ borders, int64_t n_seq, int64_t p) {
    int64_t lo = 0, hi = n_seq;            // borders[2 lo] <= p (or lo == 0), borders[2 hi] > p (or hi == n_seq)
    while (hi - lo > 1) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (borders[2 * mid] <= p) lo = mid; else hi = mid;
    }
    return lo;
}

// the best hit of every read: key[read] = max over its hits
template <bool RC>
__global__ __launch_bounds__(PW_TPB) void pwm_best_kernel(const uint32_t *__restrict__ codes, const uint16_t *__restrict__ inval,
                                                          int64_t n_data, int64_t n_tiles, PwmWeights wt, int width, int nch,
                                                          const uint16_t *__restrict__ hit16, const uint32_t *__restrict__ tile_cnt,
                                                          const int64_t *__restrict__ borders, int64_t n_seq,
                                                          unsigned long long *__restrict__ key) {
    __shared__ int2 tab[PW_MAX_CHUNKS * 256];
    __shared__ int32_t wl[128];
    build_table(tab, wl, wt, width, nch);
    const int lane = threadIdx.x & (KMAP_WAVE - 1), wave = threadIdx.x >> 6;
    for (int64_t t = (int64_t)blockIdx.x * PW_WAVES + wave; t < n_tiles; t += (int64_t)gridDim.x * PW_WAVES) {
        if (tile_cnt[t] == 0) continue;    // uniform
        const int64_t g = t * PW_TILE_GROUPS + lane;
        const Grp w = load_grp(codes, inval, g, n_data, lane);
        uint32_t bits = g < n_data ? (uint32_t)hit16[g] : 0u;
        if (bits) {
            int64_t r = find_read(borders, n_seq, g * 16 + (__builtin_clz(bits) - 16)), start = borders[2 * r];
            uint64_t best = 0;             // of the lane's hits in read r
            while (bits) {
                const int i = __builtin_clz(bits) - 16;
                bits &= ~(0x8000u >> i);
                const int64_t p = g * 16 + i;
                while (r + 1 < n_seq) {    // hits ascend: step to the hit's read, handing in what the last one got
                    const int64_t nx = borders[2 * (r + 1)];
                    if (nx > p) break;
                    if (best) atomicMax(&key[r], (unsigned long long)best);
                    best = 0;
                    ++r;
                    start = nx;
                }
                int fwd, rc;
                win_score<RC>(tab, win_bits(w, i), nch, fwd, rc);
                const uint64_t k = pack_key(RC && rc > fwd ? rc : fwd, p - start);
                best = k > best ? k : best;
            }
            if (best) atomicMax(&key[r], (unsigned long long)best);
        }
    }
}

// the oriented bases of the selected hits: per-block histogram in LDS, one global integer atomic per non-zero cell and block
template <bool RC, bool BEST>
__global__ __launch_bounds__(PW_TPB) void pwm_accum_kernel(const uint32_t *__restrict__ codes, const uint16_t *__restrict__ inval,
                                                           int64_t n_data, int64_t n_tiles, PwmWeights wt, int width, int nch,
                                                           const uint16_t *__restrict__ hit16, const uint32_t *__restrict__ tile_cnt,
                                                           const int64_t *__restrict__ borders, int64_t n_seq,
                                                           const unsigned long long *__restrict__ key,
                                                           unsigned long long *__restrict__ acc) {
    __shared__ int2 tab[PW_MAX_CHUNKS * 256];
    __shared__ int32_t wl[128];
    __shared__ uint32_t hist[PR_SLOTS];    // a block sees fewer than 2^32 positions (checked by the caller)
    if (threadIdx.x < PR_SLOTS) hist[threadIdx.x] = 0;
    build_table(tab, wl, wt, width, nch);  // its barriers publish the zeroes too
    const int lane = threadIdx.x & (KMAP_WAVE - 1), wave = threadIdx.x >> 6;
    for (int64_t t = (int64_t)blockIdx.x * PW_WAVES + wave; t < n_tiles; t += (int64_t)gridDim.x * PW_WAVES) {
        if (tile_cnt[t] == 0) continue;    // uniform
        const int64_t g = t * PW_TILE_GROUPS + lane;
        const Grp w = load_grp(codes, inval, g, n_data, lane);
        uint32_t bits = g < n_data ? (uint32_t)hit16[g] : 0u;
        if (bits) {
            int64_t r = 0, start = 0;
            uint64_t want = 0;             // key[r]
            if (BEST) {
                r = find_read(borders, n_seq, g * 16 + (__builtin_clz(bits) - 16));
                start = borders[2 * r];
                want = key[r];
            }
            while (bits) {
                const int i = __builtin_clz(bits) - 16;
                bits &= ~(0x8000u >> i);
                const uint64_t v = win_bits(w, i);
                int fwd = 0, rc = 0;
                if (RC || BEST) win_score<RC>(tab, v, nch, fwd, rc);
                const bool minus = RC && rc > fwd;
                if (BEST) {
                    const int64_t p = g * 16 + i;
                    while (r + 1 < n_seq) {
                        const int64_t nx = borders[2 * (r + 1)];
                        if (nx > p) break;
                        ++r;
                        start = nx;
                        want = key[r];
                    }
                    if (pack_key(minus ? rc : fwd, p - start) != want) continue;
                }
                for (int j = 0; j < width; ++j) {
                    const int b = (int)(v >> (62 - 2 * j)) & 3;
                    atomicAdd(&hist[minus ? (width - 1 - j) * 4 + (3 - b) : j * 4 + b], 1u);
                }
                atomicAdd(&hist[PR_SELECTED], 1u);
                if (minus) atomicAdd(&hist[PR_MINUS], 1u);
            }
        }
    }
    __syncthreads();
    if (threadIdx.x < PR_SLOTS) {
        const uint32_t c = hist[threadIdx.x];
        if (c) atomicAdd(&acc[threadIdx.x], (unsigned long long)c);
    }
}

}  // namespace

extern "C" {

int kmap_refine_counts_packed_dev(const uint32_t *codes_dev, const uint16_t *inval_dev, int64_t n, const int64_t *borders_dev,
                                  int64_t n_seq, int width, const int32_t *weights, int32_t threshold, int revcom, int select_best,
                                  int64_t *counts, int64_t *n_hits, int64_t *n_selected, int64_t *n_minus, void *stream) {
    KMAP_REQUIRE(width >= 4 && width <= 31, "refine_counts: width=%d outside 4..31", width);
    KMAP_REQUIRE(weights, "refine_counts: null weights");
    KMAP_REQUIRE(n >= 0 && n_seq >= 0, "refine_counts: negative size");
    KMAP_REQUIRE(select_best == 0 || select_best == 1, "refine_counts: select_best=%d is neither 0 nor 1", select_best);
    KMAP_REQUIRE(counts, "refine_counts: null counts");
    memset(counts, 0, (size_t)4 * width * sizeof(int64_t));
    if (n_hits) *n_hits = 0;
    if (n_selected) *n_selected = 0;
    if (n_minus) *n_minus = 0;
    if (n_seq == 0 || n == 0) return KMAP_OK;
    KMAP_REQUIRE(codes_dev && inval_dev && borders_dev, "refine_counts: null pointer");
    hipStream_t st = as_stream(stream);
    const int64_t n_data = (n + 15) >> 4, n_tiles = (n_data + PW_TILE_GROUPS - 1) / PW_TILE_GROUPS;
    const unsigned grid = (unsigned)std::min<int64_t>((n_tiles + PW_WAVES - 1) / PW_WAVES, PW_MAX_BLOCKS);
    // a block's uint32 histogram cell counts at most the positions the block visits
    const int64_t sweeps = (n_tiles + (int64_t)grid * PW_WAVES - 1) / ((int64_t)grid * PW_WAVES);
    KMAP_REQUIRE(sweeps * PW_WAVES * PW_TILE_GROUPS * 16 < (1ll << 32), "refine_counts: n=%lld gives a block 2^32 positions or more",
                 (long long)n);
    PwmWeights wt;
    memset(&wt, 0, sizeof wt);
    for (int b = 0; b < 4; ++b)
        for (int j = 0; j < width; ++j) wt.w[b][j] = weights[b * width + j];
    const int nch = (width + 3) / 4;
    uint16_t *hit16 = nullptr;
    uint32_t *tile_cnt = nullptr;
    uint64_t *tile_off = nullptr;
    unsigned long long *acc = nullptr;     // PR_SLOTS accumulators, then (select_best) one key per read
    const size_t acc_words = (size_t)PR_SLOTS + 2 + (select_best ? (size_t)n_seq : 0);
    KMAP_TRY(kmap_scratch((void **)&hit16, (size_t)n_data * 2, st, KMAP_SLOT_HASH));
    KMAP_TRY(kmap_scratch((void **)&tile_cnt, (size_t)n_tiles * 4, st, KMAP_SLOT_B));
    KMAP_TRY(kmap_scratch((void **)&tile_off, ((size_t)n_tiles + 1) * 8, st, KMAP_SLOT_PART));
    KMAP_TRY(kmap_scratch((void **)&acc, acc_words * 8, st, KMAP_SLOT_A));
    unsigned long long *key = acc + PR_SLOTS + 2;
    if (revcom)
        pwm_hits_kernel<true><<<grid, PW_TPB, 0, st>>>(codes_dev, inval_dev, n_data, n_tiles, wt, width, nch, threshold, hit16, tile_cnt);
    else
        pwm_hits_kernel<false><<<grid, PW_TPB, 0, st>>>(codes_dev, inval_dev, n_data, n_tiles, wt, width, nch, threshold, hit16, tile_cnt);
    KMAP_CHECK_HIP(hipGetLastError());
    KMAP_TRY(exclusive_scan_u32(tile_cnt, n_tiles, tile_off, st));
    uint64_t total = 0;
    KMAP_CHECK_HIP(hipMemcpyAsync(&total, tile_off + n_tiles, 8, hipMemcpyDeviceToHost, st));
    KMAP_CHECK_HIP(hipMemsetAsync(acc, 0, acc_words * 8, st));
    KMAP_CHECK_HIP(hipStreamSynchronize(st));
    if (n_hits) *n_hits = (int64_t)total;
    if (total == 0) return KMAP_OK;
    if (select_best) {
        if (revcom)
            pwm_best_kernel<true><<<grid, PW_TPB, 0, st>>>(codes_dev, inval_dev, n_data, n_tiles, wt, width, nch, hit16, tile_cnt, borders_dev,
                                                          n_seq, key);
        else
            pwm_best_kernel<false><<<grid, PW_TPB, 0, st>>>(codes_dev, inval_dev, n_data, n_tiles, wt, width, nch, hit16, tile_cnt, borders_dev,
                                                           n_seq, key);
        KMAP_CHECK_HIP(hipGetLastError());
    }
#define KMAP_ACCUM(RC, BEST)                                                                                                      \
    pwm_accum_kernel<RC, BEST><<<grid, PW_TPB, 0, st>>>(codes_dev, inval_dev, n_data, n_tiles, wt, width, nch, hit16, tile_cnt, borders_dev, \
                                                        n_seq, key, acc)
    if (revcom) {
        if (select_best) KMAP_ACCUM(true, true); else KMAP_ACCUM(true, false);
    } else {
        if (select_best) KMAP_ACCUM(false, true); else KMAP_ACCUM(false, false);
    }
#undef KMAP_ACCUM
    KMAP_CHECK_HIP(hipGetLastError());
    unsigned long long host[PR_SLOTS];
    KMAP_CHECK_HIP(hipMemcpyAsync(host, acc, sizeof host, hipMemcpyDeviceToHost, st));
    KMAP_CHECK_HIP(hipStreamSynchronize(st));
    for (int b = 0; b < 4; ++b)
        for (int j = 0; j < width; ++j) counts[b * width + j] = (int64_t)host[j * 4 + b];
    if (n_selected) *n_selected = (int64_t)host[PR_SELECTED];
    if (n_minus) *n_minus = (int64_t)host[PR_MINUS];
    return KMAP_OK;
}

}  // extern "C"
