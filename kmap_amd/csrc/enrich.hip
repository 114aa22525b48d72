// enrich.hip -- k-mer enrichment of a foreground table against a control table (enrich_kmers).  Both tables
// are counts handles resident in HBM.  The foreground F stands in the reference's order (after the reverse-complement merge NOT
// ascending); the control B is counted without the merge, so its keys ascend and are unique.
//
//   * directory (dir_kernel): offsets of B's keys per leading d = min(2k, 20) bits, 2^d + 1 entries; entry j is the lower bound of
//     key j << (2k - d), found by ONE thread with a binary search over B -- no atomics.  For k <= 10 a bucket is one key.
//   * lookup + score (score_kernel): one foreground entry per lane, grid-stride.  b = B[x] + (revcom ? B[rc x] : 0): one directory
//     read and a binary search inside the bucket per key, the two searches of a lane advanced together so that two chains of
//     dependent loads are in flight.  D = a Nb - b Nf exactly in 128-bit integers, converted to double once;
//     s = ((a + b)(Nf + Nb - a - b)) ((Nf Nb) / (Nf + Nb)) in double in this order; z = D / sqrt(s), 0 unless s > 0.
//   * selection (kmap_enrich_select): z -> order-preserving uint64 key; radix select of the N-th largest key among the eligible
//     entries (a >= min_count), EN_BITS bits per pass: LDS histogram per block, one integer atomic add per non-empty bin and block
//     into a global table, the host picks the bin.  Then a compaction in table order keeps every eligible entry above the
//     threshold and the FIRST r entries equal to it (per-tile counts of both, exclusive scans, a write pass): a tie group, however
//     large, is never materialised.  The N survivors are ordered (z descending, index ascending) on the host.
//   * EVERY search loop has a compile-time bound on its trip count (EN_SEARCH_STEPS): a wrong bound ends with a wrong answer.
#include <algorithm>
#include <numeric>
#include <vector>

#include "common.h"
#include "counts_internal.h"
#include "scan_util.h"

struct kmap_enrich {
    // control
    kmap_counts *bg = nullptr;
    const void *bg_keys = nullptr;   // borrowed from bg until its next count / load
    const uint32_t *bg_cnt = nullptr;
    int64_t n_bg = 0;
    int k = 0, narrow = 1, revcom = 0, d = 0;
    uint32_t *dir = nullptr;         // 2^d + 1 offsets into B
    size_t dir_cap = 0;
    // scores of the last run
    kmap_counts *fg = nullptr;
    const void *fg_keys = nullptr;   // borrowed from fg until its next count / load
    const uint32_t *fg_cnt = nullptr;
    int64_t n = 0;
    uint32_t min_count = 1;
    uint64_t *b = nullptr;
    double *z = nullptr;
    size_t res_cap = 0;
    int has_control = 0, has_run = 0, has_sel = 0;
    int none_eligible = 0;           // min_count above every uint32 count
    // selection scratch and result
    unsigned long long *bins = nullptr;
    uint32_t *tile_g = nullptr, *tile_e = nullptr;
    uint64_t *off_g = nullptr, *off_e = nullptr;
    size_t tile_cap = 0;
    std::vector<int64_t> s_idx, s_a, s_b;
    std::vector<uint64_t> s_kh;
    std::vector<double> s_z;
};

namespace {

constexpr int EN_TPB = 256;
constexpr int EN_MAX_BLOCKS = 2048;
constexpr int EN_SEARCH_STEPS = 64;      // a bucket holds < 2^32 keys: 33 halvings at most
constexpr int EN_ITEMS = 8;
constexpr int EN_TILE = EN_TPB * EN_ITEMS;
// 11 bits per pass, 6 passes: a block's 2048 uint32 bins are 8 KiB of LDS (the 65 536 bins of a 16-bit digit would be 256 KiB)
constexpr int EN_BITS = 11;
constexpr int EN_BINS = 1 << EN_BITS;
constexpr int EN_PASSES = (64 + EN_BITS - 1) / EN_BITS;
constexpr uint64_t EN_MAX_TOTAL = ((uint64_t)1 << 52) - 1;

// ---- directory ------------------------------------------------------------------------------------------------------------
template <typename H>
__global__ __launch_bounds__(EN_TPB) void dir_kernel(const H *__restrict__ keys, int64_t n_bg, int d, int shift, uint32_t *__restrict__ dir) {
    const int64_t j = (int64_t)blockIdx.x * EN_TPB + threadIdx.x, n_buckets = (int64_t)1 << d;
    if (j > n_buckets) return;
    int64_t lo = 0, hi = n_bg;           // first index whose key is >= j << shift
    if (j == n_buckets) lo = hi;
    const H target = (H)((uint64_t)j << shift);
    for (int s = 0; s < EN_SEARCH_STEPS && lo < hi; ++s) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (keys[mid] < target) lo = mid + 1; else hi = mid;
    }
    dir[j] = (uint32_t)lo;
}

// ---- lookup + score -------------------------------------------------------------------------------------------------------
struct Range {
    int64_t lo, hi;
};
template <typename H>
__device__ __forceinline__ Range bucket_of(const uint32_t *__restrict__ dir, H x, int d, int shift, bool on) {
    const uint64_t bk = (uint64_t)x >> shift;
    Range r = {0, 0};
    if (on && bk < ((uint64_t)1 << d)) {     // a key at or above 4^k is in no bucket
        r.lo = dir[bk];
        r.hi = dir[bk + 1];
    }
    return r;
}

__device__ __forceinline__ double score_z(uint32_t a, uint64_t b, uint64_t Nf, uint64_t Nb, double pre) {
    const __int128 D = (__int128)((unsigned __int128)a * Nb) - (__int128)((unsigned __int128)b * Nf);
    const uint64_t ab = (uint64_t)a + b;
    const double s = ((double)ab * (double)(int64_t)(Nf + Nb - ab)) * pre;
    return s > 0.0 ? (double)D / sqrt(s) : 0.0;      // s == 0, or NaN from Nf + Nb == 0: no evidence either way
}

template <typename H, bool RC>
__global__ __launch_bounds__(EN_TPB) void score_kernel(const H *__restrict__ fkeys, const uint32_t *__restrict__ fcnt, int64_t n,
                                                       const H *__restrict__ bkeys, const uint32_t *__restrict__ bcnt,
                                                       const uint32_t *__restrict__ dir, int k, int d, int shift, uint64_t Nf,
                                                       uint64_t Nb, double pre, uint64_t *__restrict__ b_out, double *__restrict__ z_out) {
    const int64_t stride = (int64_t)gridDim.x * EN_TPB;
    for (int64_t i = (int64_t)blockIdx.x * EN_TPB + threadIdx.x; i < n; i += stride) {
        const H x = fkeys[i], y = RC ? revcom_hash(x, k) : x;
        Range r1 = bucket_of<H>(dir, x, d, shift, true), r2 = bucket_of<H>(dir, y, d, shift, RC);
        int64_t f1 = -1, f2 = -1;
        for (int s = 0; s < EN_SEARCH_STEPS && (r1.lo < r1.hi || r2.lo < r2.hi); ++s) {
            const bool on1 = r1.lo < r1.hi, on2 = r2.lo < r2.hi;
            const int64_t m1 = r1.lo + ((r1.hi - r1.lo) >> 1), m2 = r2.lo + ((r2.hi - r2.lo) >> 1);
            const H k1 = on1 ? bkeys[m1] : (H)0, k2 = on2 ? bkeys[m2] : (H)0;      // both loads issue before either is used
            if (on1) {
                if (k1 == x) { f1 = m1; r1.lo = r1.hi; }
                else if (k1 < x) r1.lo = m1 + 1;
                else r1.hi = m1;
            }
            if (on2) {
                if (k2 == y) { f2 = m2; r2.lo = r2.hi; }
                else if (k2 < y) r2.lo = m2 + 1;
                else r2.hi = m2;
            }
        }
        uint64_t b = 0;
        if (f1 >= 0) b += bcnt[f1];
        if (f2 >= 0) b += bcnt[f2];       // a palindrome finds itself twice: the doubling of the reference's merge
        b_out[i] = b;
        z_out[i] = score_z(fcnt[i], b, Nf, Nb, pre);
    }
}

// ---- selection ------------------------------------------------------------------------------------------------------------
// order-preserving map double -> uint64 (no NaN reaches it; -0.0 is not produced by score_z)
__device__ __forceinline__ uint64_t order_key(double z) {
    const uint64_t u = (uint64_t)__double_as_longlong(z);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

// pass p looks at the digit below the 11 p bits already fixed (`prefix`); the last pass has 64 - 55 = 9 bits left
__global__ __launch_bounds__(EN_TPB) void hist_kernel(const double *__restrict__ z, const uint32_t *__restrict__ a, int64_t n,
                                                      uint32_t min_count, int done_bits, int width, uint64_t prefix,
                                                      unsigned long long *__restrict__ bins) {
    __shared__ uint32_t h[EN_BINS];
    for (int j = threadIdx.x; j < EN_BINS; j += EN_TPB) h[j] = 0;
    __syncthreads();
    const int low = 64 - done_bits - width;
    const int64_t stride = (int64_t)gridDim.x * EN_TPB;
    for (int64_t i = (int64_t)blockIdx.x * EN_TPB + threadIdx.x; i < n; i += stride) {
        if (a[i] < min_count) continue;
        const uint64_t key = order_key(z[i]);
        if (done_bits && (key >> (64 - done_bits)) != prefix) continue;
        atomicAdd(&h[(uint32_t)(key >> low) & ((1u << width) - 1u)], 1u);
    }
    __syncthreads();
    for (int j = threadIdx.x; j < EN_BINS; j += EN_TPB)
        if (h[j]) atomicAdd(&bins[j], (unsigned long long)h[j]);
}

// the entries of a tile in table order, EN_ITEMS consecutive ones per thread: flags "above the threshold" (bits 0..7) / "equal to
// it" (bits 8..15)
__device__ __forceinline__ uint32_t tile_flags(const double *__restrict__ z, const uint32_t *__restrict__ a, int64_t n, uint32_t min_count,
                                               uint64_t thr, int64_t base) {
    uint32_t f = 0;
#pragma unroll
    for (int j = 0; j < EN_ITEMS; ++j) {
        const int64_t i = base + j;
        const bool in = i < n;
        const uint32_t ai = in ? a[i] : 0u;
        const uint64_t key = order_key(in ? z[i] : 0.0);
        const bool el = in && ai >= min_count;
        f |= (uint32_t)(el && key > thr) << j;
        f |= (uint32_t)(el && key == thr) << (8 + j);
    }
    return f;
}

__global__ __launch_bounds__(EN_TPB) void tile_count_kernel(const double *__restrict__ z, const uint32_t *__restrict__ a, int64_t n,
                                                            uint32_t min_count, uint64_t thr, uint32_t *__restrict__ tile_g,
                                                            uint32_t *__restrict__ tile_e) {
    __shared__ uint32_t wg[EN_TPB / KMAP_WAVE], we[EN_TPB / KMAP_WAVE];
    const uint32_t f = tile_flags(z, a, n, min_count, thr, (int64_t)blockIdx.x * EN_TILE + (int64_t)threadIdx.x * EN_ITEMS);
    const uint32_t gt = f & 0xFFu, eq = f >> 8;
    uint32_t g = (uint32_t)__builtin_popcount(gt), e = (uint32_t)__builtin_popcount(eq);
    for (int o = 32; o > 0; o >>= 1) {
        g += __shfl_down(g, o);
        e += __shfl_down(e, o);
    }
    if ((threadIdx.x & 63) == 0) {
        wg[threadIdx.x >> 6] = g;
        we[threadIdx.x >> 6] = e;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        tile_g[blockIdx.x] = wg[0] + wg[1] + wg[2] + wg[3];
        tile_e[blockIdx.x] = we[0] + we[1] + we[2] + we[3];
    }
}

// sel[0 .. n_gt) = the entries above the threshold, sel[n_gt .. n_gt + r) = the first r entries equal to it, both in table order
__global__ __launch_bounds__(EN_TPB) void tile_write_kernel(const double *__restrict__ z, const uint32_t *__restrict__ a, int64_t n,
                                                            uint32_t min_count, uint64_t thr, const uint64_t *__restrict__ off_g,
                                                            const uint64_t *__restrict__ off_e, uint64_t n_gt, uint64_t r,
                                                            int64_t *__restrict__ sel) {
    __shared__ uint32_t wg[EN_TPB / KMAP_WAVE], we[EN_TPB / KMAP_WAVE];
    const int64_t base = (int64_t)blockIdx.x * EN_TILE + (int64_t)threadIdx.x * EN_ITEMS;
    const uint32_t f = tile_flags(z, a, n, min_count, thr, base);
    const uint32_t gt = f & 0xFFu, eq = f >> 8;
    const uint32_t g = (uint32_t)__builtin_popcount(gt), e = (uint32_t)__builtin_popcount(eq);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t ig = g, ie = e;
    for (int o = 1; o < KMAP_WAVE; o <<= 1) {
        const uint32_t tg = __shfl_up(ig, o), te = __shfl_up(ie, o);
        if (lane >= o) {
            ig += tg;
            ie += te;
        }
    }
    if (lane == KMAP_WAVE - 1) {
        wg[wave] = ig;
        we[wave] = ie;
    }
    __syncthreads();
    uint64_t pg = off_g[blockIdx.x] + (ig - g), pe = off_e[blockIdx.x] + (ie - e);
    for (int w = 0; w < wave; ++w) {
        pg += wg[w];
        pe += we[w];
    }
#pragma unroll
    for (int j = 0; j < EN_ITEMS; ++j) {
        if (gt >> j & 1u) {
            if (pg < n_gt) sel[pg] = base + j;          // (always true: n_gt is the scan's total)
            ++pg;
        } else if (eq >> j & 1u) {
            if (pe < r) sel[n_gt + pe] = base + j;
            ++pe;
        }
    }
}

template <typename H>
__global__ __launch_bounds__(EN_TPB) void gather_kernel(const int64_t *__restrict__ sel, int64_t m, int64_t n, const H *__restrict__ keys,
                                                        const uint32_t *__restrict__ a, const uint64_t *__restrict__ b,
                                                        const double *__restrict__ z, uint64_t *__restrict__ kh_out,
                                                        int64_t *__restrict__ a_out, int64_t *__restrict__ b_out, double *__restrict__ z_out) {
    const int64_t j = (int64_t)blockIdx.x * EN_TPB + threadIdx.x;
    if (j >= m) return;
    const int64_t i = sel[j];
    if (i < 0 || i >= n) return;
    kh_out[j] = (uint64_t)keys[i];
    a_out[j] = (int64_t)a[i];
    b_out[j] = (int64_t)b[i];
    z_out[j] = z[i];
}

template <typename T>
int regrow(T **p, size_t *cap, size_t want) {
    if (*p && *cap >= want) return KMAP_OK;
    if (*p) KMAP_CHECK_HIP(hipFree(*p));
    *p = nullptr;
    *cap = 0;
    KMAP_CHECK_HIP(hipMalloc((void **)p, (want ? want : 1) * sizeof(T)));
    *cap = want ? want : 1;
    return KMAP_OK;
}

int state_error(const char *msg) {
    kmap_set_error("%s", msg);
    return KMAP_E_STATE;
}

// the borrowed arrays are still the ones the handle saw (the table was not counted or loaded anew)
bool same_table(const kmap_counts *c, const void *keys, const uint32_t *cnt, int64_t n, int k) {
    return c && c->k == k && c->n_uniq == n && c->uniq == keys && c->cnt == cnt;
}

}  // namespace

extern "C" {

int kmap_enrich_create(kmap_enrich **e) {
    KMAP_REQUIRE(e, "enrich_create: null");
    *e = new kmap_enrich();
    return KMAP_OK;
}

int kmap_enrich_destroy(kmap_enrich *e) {
    if (!e) return KMAP_OK;
    void *bufs[] = {e->dir, e->b, e->z, e->bins, e->tile_g, e->tile_e, e->off_g, e->off_e};
    for (void *p : bufs)
        if (p) (void)hipFree(p);
    delete e;
    return KMAP_OK;
}

int kmap_enrich_set_control(kmap_enrich *e, kmap_counts *bg, int revcom, void *stream) {
    KMAP_REQUIRE(e && bg, "enrich_set_control: null handle");
    KMAP_REQUIRE(bg->k > 0 && bg->k < 32, "enrich_set_control: the control table holds no count yet");
    if (bg->n_uniq >= ((int64_t)1 << 32)) {
        kmap_set_error("enrich_set_control: %lld control k-mers, the directory holds 32-bit offsets", (long long)bg->n_uniq);
        return KMAP_E_UNSUP;
    }
    hipStream_t st = as_stream(stream);
    e->has_control = 0;
    e->has_run = e->has_sel = 0;
    const int k = bg->k, d = 2 * k < 20 ? 2 * k : 20;
    const size_t entries = ((size_t)1 << d) + 1;
    size_t cap = e->dir_cap;
    KMAP_TRY(regrow(&e->dir, &cap, entries));
    e->dir_cap = cap;
    const unsigned grid = grid_for((int64_t)entries, EN_TPB);
    if (bg->narrow)
        dir_kernel<uint32_t><<<grid, EN_TPB, 0, st>>>((const uint32_t *)bg->uniq, bg->n_uniq, d, 2 * k - d, e->dir);
    else
        dir_kernel<uint64_t><<<grid, EN_TPB, 0, st>>>((const uint64_t *)bg->uniq, bg->n_uniq, d, 2 * k - d, e->dir);
    KMAP_CHECK_HIP(hipGetLastError());
    e->bg = bg;
    e->bg_keys = bg->uniq;
    e->bg_cnt = bg->cnt;
    e->n_bg = bg->n_uniq;
    e->k = k;
    e->narrow = bg->narrow;
    e->revcom = revcom ? 1 : 0;
    e->d = d;
    e->has_control = 1;
    return KMAP_OK;
}

int kmap_enrich_run(kmap_enrich *e, kmap_counts *fg, int64_t n_fg_total, int64_t n_bg_total, int64_t min_count, void *stream) {
    KMAP_REQUIRE(e && fg, "enrich_run: null handle");
    if (!e->has_control) return state_error("enrich_run: no control table set (kmap_enrich_set_control comes first)");
    if (!same_table(e->bg, e->bg_keys, e->bg_cnt, e->n_bg, e->k))
        return state_error("enrich_run: the control table was counted or loaded again since kmap_enrich_set_control");
    KMAP_REQUIRE(fg->k > 0, "enrich_run: the foreground table holds no count yet");
    KMAP_REQUIRE(fg->k == e->k, "enrich_run: foreground k=%d, control k=%d", fg->k, e->k);
    KMAP_REQUIRE(min_count >= 1, "enrich_run: min_count=%lld < 1", (long long)min_count);
    KMAP_REQUIRE(n_fg_total >= 0 && n_bg_total >= 0, "enrich_run: negative total");
    if ((uint64_t)n_fg_total > EN_MAX_TOTAL || (uint64_t)n_bg_total > EN_MAX_TOTAL) {
        kmap_set_error("enrich_run: totals %lld / %lld, at most 2^52 - 1 is supported", (long long)n_fg_total, (long long)n_bg_total);
        return KMAP_E_UNSUP;
    }
    hipStream_t st = as_stream(stream);
    e->has_run = e->has_sel = 0;
    const int64_t n = fg->n_uniq;
    size_t cap_b = e->res_cap, cap_z = e->res_cap;
    e->res_cap = 0;
    KMAP_TRY(regrow(&e->b, &cap_b, (size_t)n));
    KMAP_TRY(regrow(&e->z, &cap_z, (size_t)n));
    e->res_cap = std::min(cap_b, cap_z);
    if (n) {
        const uint64_t Nf = (uint64_t)n_fg_total, Nb = (uint64_t)n_bg_total;
        const double pre = ((double)Nf * (double)Nb) / (double)(Nf + Nb);
        const unsigned grid = (unsigned)std::min<int64_t>(grid_for(n, EN_TPB), EN_MAX_BLOCKS);
        const int shift = 2 * e->k - e->d;
#define KMAP_ENRICH_LAUNCH(H, RC)                                                                                                  \
    score_kernel<H, RC><<<grid, EN_TPB, 0, st>>>((const H *)fg->uniq, fg->cnt, n, (const H *)e->bg_keys, e->bg_cnt, e->dir, e->k, \
                                                 e->d, shift, Nf, Nb, pre, e->b, e->z)
        if (e->narrow) {
            if (e->revcom) KMAP_ENRICH_LAUNCH(uint32_t, true); else KMAP_ENRICH_LAUNCH(uint32_t, false);
        } else {
            if (e->revcom) KMAP_ENRICH_LAUNCH(uint64_t, true); else KMAP_ENRICH_LAUNCH(uint64_t, false);
        }
#undef KMAP_ENRICH_LAUNCH
        KMAP_CHECK_HIP(hipGetLastError());
    }
    e->fg = fg;
    e->fg_keys = fg->uniq;
    e->fg_cnt = fg->cnt;
    e->n = n;
    e->min_count = (uint32_t)std::min<int64_t>(min_count, 0xFFFFFFFFll);
    e->none_eligible = min_count > 0xFFFFFFFFll;
    e->has_run = 1;
    return KMAP_OK;
}

int kmap_enrich_result_dev(kmap_enrich *e, void **b_dev, void **z_dev, int64_t *n) {
    KMAP_REQUIRE(e && b_dev && z_dev && n, "enrich_result_dev: null");
    if (!e->has_run) return state_error("enrich_result_dev: no run yet");
    *b_dev = e->b;
    *z_dev = e->z;
    *n = e->n;
    return KMAP_OK;
}

int kmap_enrich_select(kmap_enrich *e, int64_t top_n, int64_t *n_sel, int64_t *n_eligible, void *stream) {
    KMAP_REQUIRE(e && n_sel, "enrich_select: null");
    KMAP_REQUIRE(top_n >= 1, "enrich_select: top_n=%lld < 1", (long long)top_n);
    if (!e->has_run) return state_error("enrich_select: no run yet (kmap_enrich_run comes first)");
    if (!same_table(e->fg, e->fg_keys, e->fg_cnt, e->n, e->k))
        return state_error("enrich_select: the foreground table was counted or loaded again since kmap_enrich_run");
    hipStream_t st = as_stream(stream);
    e->has_sel = 0;
    *n_sel = 0;
    if (n_eligible) *n_eligible = 0;
    e->s_idx.clear(); e->s_kh.clear(); e->s_a.clear(); e->s_b.clear(); e->s_z.clear();
    const int64_t n = e->n;
    if (n == 0 || e->none_eligible) {
        e->has_sel = 1;
        return KMAP_OK;
    }
    size_t cap = e->bins ? (size_t)EN_BINS : 0;
    KMAP_TRY(regrow(&e->bins, &cap, (size_t)EN_BINS));
    const unsigned hgrid = (unsigned)std::min<int64_t>(grid_for(n, EN_TILE), EN_MAX_BLOCKS);
    std::vector<unsigned long long> host(EN_BINS);
    uint64_t prefix = 0, want = 0, n_gt = 0;
    int done = 0;
    for (int p = 0; p < EN_PASSES; ++p) {
        const int width = std::min(EN_BITS, 64 - done);
        KMAP_CHECK_HIP(hipMemsetAsync(e->bins, 0, EN_BINS * sizeof(unsigned long long), st));
        hist_kernel<<<hgrid, EN_TPB, 0, st>>>(e->z, e->fg_cnt, n, e->min_count, done, width, prefix, e->bins);
        KMAP_CHECK_HIP(hipGetLastError());
        KMAP_CHECK_HIP(hipMemcpyAsync(host.data(), e->bins, EN_BINS * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
        KMAP_CHECK_HIP(hipStreamSynchronize(st));
        if (p == 0) {
            const uint64_t eligible = std::accumulate(host.begin(), host.end(), (uint64_t)0);
            if (n_eligible) *n_eligible = (int64_t)eligible;
            want = std::min<uint64_t>((uint64_t)top_n, eligible);
            if (want == 0) {
                e->has_sel = 1;
                return KMAP_OK;
            }
        }
        // the bin that holds the want-th largest key among those that share the prefix
        uint64_t above = 0;
        int bin = (1 << width) - 1;
        for (; bin > 0 && above + host[(size_t)bin] < want; --bin) above += host[(size_t)bin];
        n_gt += above;
        want -= above;
        prefix = (prefix << width) | (uint64_t)bin;
        done += width;
    }
    // prefix = the threshold key; n_gt entries lie above it, the first `want` (>= 1) of those equal to it complete the selection
    const uint64_t thr = prefix, r = want, m = n_gt + r;
    const int64_t tiles = (n + EN_TILE - 1) / EN_TILE;
    if (e->tile_cap < (size_t)tiles + 1) {       // all four arrays share one capacity
        size_t c1 = e->tile_cap, c2 = e->tile_cap, c3 = e->tile_cap, c4 = e->tile_cap;
        e->tile_cap = 0;
        KMAP_TRY(regrow(&e->tile_g, &c1, (size_t)tiles + 1));
        KMAP_TRY(regrow(&e->tile_e, &c2, (size_t)tiles + 1));
        KMAP_TRY(regrow(&e->off_g, &c3, (size_t)tiles + 1));
        KMAP_TRY(regrow(&e->off_e, &c4, (size_t)tiles + 1));
        e->tile_cap = (size_t)tiles + 1;
    }
    tile_count_kernel<<<(unsigned)tiles, EN_TPB, 0, st>>>(e->z, e->fg_cnt, n, e->min_count, thr, e->tile_g, e->tile_e);
    KMAP_CHECK_HIP(hipGetLastError());
    KMAP_TRY(exclusive_scan_u32(e->tile_g, tiles, e->off_g, st));
    KMAP_TRY(exclusive_scan_u32(e->tile_e, tiles, e->off_e, st));
    KMAP_CHECK_HIP(hipGetLastError());
    uint64_t tot_g = 0, tot_e = 0;
    KMAP_CHECK_HIP(hipMemcpyAsync(&tot_g, e->off_g + tiles, 8, hipMemcpyDeviceToHost, st));
    KMAP_CHECK_HIP(hipMemcpyAsync(&tot_e, e->off_e + tiles, 8, hipMemcpyDeviceToHost, st));
    KMAP_CHECK_HIP(hipStreamSynchronize(st));
    if (tot_g != n_gt || tot_e < r) {
        kmap_set_error("enrich_select: the compaction counted %llu above / %llu at the threshold, the radix passes %llu / >= %llu",
                       (unsigned long long)tot_g, (unsigned long long)tot_e, (unsigned long long)n_gt, (unsigned long long)r);
        return KMAP_E_STATE;
    }
    DevBuf sel, kh, a, b, z;
    KMAP_TRY(sel.alloc((size_t)m * 8));
    KMAP_TRY(kh.alloc((size_t)m * 8));
    KMAP_TRY(a.alloc((size_t)m * 8));
    KMAP_TRY(b.alloc((size_t)m * 8));
    KMAP_TRY(z.alloc((size_t)m * 8));
    KMAP_CHECK_HIP(hipMemsetAsync(sel.p, 0xFF, (size_t)m * 8, st));
    tile_write_kernel<<<(unsigned)tiles, EN_TPB, 0, st>>>(e->z, e->fg_cnt, n, e->min_count, thr, e->off_g, e->off_e, n_gt, r, sel.as<int64_t>());
    KMAP_CHECK_HIP(hipGetLastError());
    const unsigned ggrid = grid_for((int64_t)m, EN_TPB);
    if (e->narrow)
        gather_kernel<uint32_t><<<ggrid, EN_TPB, 0, st>>>(sel.as<int64_t>(), (int64_t)m, n, (const uint32_t *)e->fg_keys, e->fg_cnt, e->b, e->z,
                                                          kh.as<uint64_t>(), a.as<int64_t>(), b.as<int64_t>(), z.as<double>());
    else
        gather_kernel<uint64_t><<<ggrid, EN_TPB, 0, st>>>(sel.as<int64_t>(), (int64_t)m, n, (const uint64_t *)e->fg_keys, e->fg_cnt, e->b, e->z,
                                                          kh.as<uint64_t>(), a.as<int64_t>(), b.as<int64_t>(), z.as<double>());
    KMAP_CHECK_HIP(hipGetLastError());
    std::vector<int64_t> idx(m), va(m), vb(m);
    std::vector<uint64_t> vk(m);
    std::vector<double> vz(m);
    KMAP_CHECK_HIP(hipMemcpyAsync(idx.data(), sel.p, (size_t)m * 8, hipMemcpyDeviceToHost, st));
    KMAP_CHECK_HIP(hipMemcpyAsync(vk.data(), kh.p, (size_t)m * 8, hipMemcpyDeviceToHost, st));
    KMAP_CHECK_HIP(hipMemcpyAsync(va.data(), a.p, (size_t)m * 8, hipMemcpyDeviceToHost, st));
    KMAP_CHECK_HIP(hipMemcpyAsync(vb.data(), b.p, (size_t)m * 8, hipMemcpyDeviceToHost, st));
    KMAP_CHECK_HIP(hipMemcpyAsync(vz.data(), z.p, (size_t)m * 8, hipMemcpyDeviceToHost, st));
    KMAP_CHECK_HIP(hipStreamSynchronize(st));
    std::vector<int64_t> order(m);
    std::iota(order.begin(), order.end(), (int64_t)0);
    std::sort(order.begin(), order.end(), [&](int64_t p, int64_t q) {      // z descending, ties by the lower table index
        if (vz[(size_t)p] != vz[(size_t)q]) return vz[(size_t)p] > vz[(size_t)q];
        return idx[(size_t)p] < idx[(size_t)q];
    });
    e->s_idx.resize(m); e->s_kh.resize(m); e->s_a.resize(m); e->s_b.resize(m); e->s_z.resize(m);
    for (size_t j = 0; j < (size_t)m; ++j) {
        const size_t o = (size_t)order[j];
        e->s_idx[j] = idx[o];
        e->s_kh[j] = vk[o];
        e->s_a[j] = va[o];
        e->s_b[j] = vb[o];
        e->s_z[j] = vz[o];
    }
    *n_sel = (int64_t)m;
    e->has_sel = 1;
    return KMAP_OK;
}

int kmap_enrich_fetch(kmap_enrich *e, int64_t *idx_out, uint64_t *kh_out, int64_t *a_out, int64_t *b_out, double *z_out) {
    KMAP_REQUIRE(e, "enrich_fetch: null handle");
    if (!e->has_sel) return state_error("enrich_fetch: no selection yet (kmap_enrich_select comes first)");
    const size_t m = e->s_idx.size();
    if (m == 0) return KMAP_OK;
    if (idx_out) memcpy(idx_out, e->s_idx.data(), m * 8);
    if (kh_out) memcpy(kh_out, e->s_kh.data(), m * 8);
    if (a_out) memcpy(a_out, e->s_a.data(), m * 8);
    if (b_out) memcpy(b_out, e->s_b.data(), m * 8);
    if (z_out) memcpy(z_out, e->s_z.data(), m * 8);
    return KMAP_OK;
}

}  // extern "C"
