// pwm_refine.hip -- one iteration of refine_pwm on the device: the hits of a weight matrix on the packed
// reads (section 11's hits, pass A of pwm_scan.hip as it is), a selection among them, and the 4 x width count matrix of the selected
// windows' oriented bases.  Nothing but 126 integers leaves the device.
//
//   * pass A (pwm_pass_a, pwm_internal.h): hit bit per position, hit count per wave tile, exclusive scan, total = n_hits.
//   * pwm_best_kernel (select_best only): every hit is evaluated again (for_each_hit, the sparse traversal of pwm_internal.h) and
//     takes part in an unsigned 64-bit atomicMax on key[read], key = (score with the sign bit flipped) << 32 | (0xFFFFFFFF - loc):
//     the largest score wins, on a tie the smallest loc.  A maximum does not depend on the order of its operands, so the result is
//     deterministic.  Zero = "no hit" (a real key's low half is >= 2^31: loc is an int32).
//   * pwm_accum_kernel: the same traversal -- without select_best it asks for no reads and the borders are never loaded; a hit
//     counts when its key equals key[read] (select_best) or always.  Its width oriented
//     bases -- window base j on '+', 3 - (window base width - 1 - j) on '-' -- go into a per-block LDS histogram [31][4] (+ the
//     selected / minus counters); after the grid-stride loop at most 126 threads of a block add its non-zero cells to the global
//     uint64 array, one integer atomic each (order-free).
// It uses scratch slots only: no kmap_scan handle is needed or touched.
#include "common.h"
#include "pwm_internal.h"

namespace {

constexpr int PR_CELLS = 31 * 4;          // histogram cells [column][base]
constexpr int PR_SELECTED = PR_CELLS;     // + the number of selected windows
constexpr int PR_MINUS = PR_CELLS + 1;    // + those on '-'
constexpr int PR_SLOTS = PR_CELLS + 2;    // 126

__device__ __forceinline__ uint64_t pack_key(int score, int64_t loc) {
    return ((uint64_t)((uint32_t)score ^ 0x80000000u) << 32) | (uint64_t)(0xFFFFFFFFu - (uint32_t)loc);
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
    uint64_t best = 0;     // of the lane's hits in the read it is in
    for_each_hit<RC, true>(
        tab, codes, inval, n_data, n_tiles, nch, hit16, tile_cnt, borders, n_seq,
        [&](int, int64_t p, int64_t, int64_t start, uint64_t, int fwd, int rc) {
            const uint64_t k = pack_key(RC && rc > fwd ? rc : fwd, p - start);
            best = k > best ? k : best;
        },
        [&](int64_t left, int64_t) {                   // handing in what the read the lane leaves got
            if (best) atomicMax(&key[left], (unsigned long long)best);
            best = 0;
        });
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
    uint64_t want = 0;     // key[the read the lane is in]
    for_each_hit<RC, BEST>(
        tab, codes, inval, n_data, n_tiles, nch, hit16, tile_cnt, borders, n_seq,
        [&](int, int64_t p, int64_t, int64_t start, uint64_t v, int fwd, int rc) {
            const bool minus = RC && rc > fwd;
            if (BEST && pack_key(minus ? rc : fwd, p - start) != want) return;
            for (int j = 0; j < width; ++j) {
                const int b = (int)(v >> (62 - 2 * j)) & 3;
                atomicAdd(&hist[minus ? (width - 1 - j) * 4 + (3 - b) : j * 4 + b], 1u);
            }
            atomicAdd(&hist[PR_SELECTED], 1u);
            if (minus) atomicAdd(&hist[PR_MINUS], 1u);
        },
        [&](int64_t, int64_t entered) {
            if (entered >= 0) want = key[entered];
        });
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
    PwmPlan pl;
    KMAP_TRY(pwm_plan(pl, "refine_counts", n, n_seq, width, weights));
    KMAP_REQUIRE(select_best == 0 || select_best == 1, "refine_counts: select_best=%d is neither 0 nor 1", select_best);
    KMAP_REQUIRE(counts, "refine_counts: null counts");
    memset(counts, 0, (size_t)4 * width * sizeof(int64_t));
    if (n_hits) *n_hits = 0;
    if (n_selected) *n_selected = 0;
    if (n_minus) *n_minus = 0;
    if (n_seq == 0 || n == 0) return KMAP_OK;
    KMAP_REQUIRE(codes_dev && inval_dev && borders_dev, "refine_counts: null pointer");
    hipStream_t st = as_stream(stream);
    // a block's uint32 histogram cell counts at most the positions the block visits
    const int64_t sweeps = (pl.n_tiles + (int64_t)pl.grid * PW_WAVES - 1) / ((int64_t)pl.grid * PW_WAVES);
    KMAP_REQUIRE(sweeps * PW_WAVES * PW_TILE_GROUPS * 16 < (1ll << 32), "refine_counts: n=%lld gives a block 2^32 positions or more",
                 (long long)n);
    uint16_t *hit16 = nullptr;
    uint32_t *tile_cnt = nullptr;
    uint64_t *tile_off = nullptr;
    unsigned long long *acc = nullptr;     // PR_SLOTS accumulators, then (select_best) one key per read
    const size_t acc_words = (size_t)PR_SLOTS + 2 + (select_best ? (size_t)n_seq : 0);
    KMAP_TRY(kmap_scratch((void **)&acc, acc_words * 8, st, KMAP_SLOT_A));
    unsigned long long *key = acc + PR_SLOTS + 2;
    KMAP_CHECK_HIP(hipMemsetAsync(acc, 0, acc_words * 8, st));
    uint64_t total = 0;
    KMAP_TRY(pwm_pass_a(pl, codes_dev, inval_dev, threshold, revcom, st, &hit16, &tile_cnt, &tile_off, &total));
    if (n_hits) *n_hits = (int64_t)total;
    if (total == 0) return KMAP_OK;
    with_bool(revcom, [&](auto rc) {
        if (select_best)
            pwm_best_kernel<decltype(rc)::value><<<pl.grid, PW_TPB, 0, st>>>(codes_dev, inval_dev, pl.n_data, pl.n_tiles, pl.wt, width, pl.nch,
                                                                             hit16, tile_cnt, borders_dev, n_seq, key);
        with_bool(select_best, [&](auto best) {
            pwm_accum_kernel<decltype(rc)::value, decltype(best)::value><<<pl.grid, PW_TPB, 0, st>>>(
                codes_dev, inval_dev, pl.n_data, pl.n_tiles, pl.wt, width, pl.nch, hit16, tile_cnt, borders_dev, n_seq, key, acc);
        });
    });
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
