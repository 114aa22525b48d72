// pwm_sites.hip -- where in the reads the best site of every matrix of a library lies (motif_centrality).
// The scoring is pwm_batch.h's batched pass with section 14's (score, loc) key (SiteKey: the largest score wins, on a tie the smallest
// loc; only site reads -- best score >= the matrix's threshold -- get a key), and behind it a reduction of the keys to two small
// histograms per matrix, so that nothing per read leaves the device.
//
//   * sites_hist_kernel: blockIdx.y = the matrix, blockIdx.x strides over its keys.  A non-zero key gives loc; the read's two
//     borders give its length L; the doubled centre offset d = 2 loc + width - L lies in [-(L - width), L - width].  Per matrix, in one
//     flat uint64 array: sites, too_long, D[2 max_len + 1] (bin d + max_len), Hlen[max_len + 1].  A site read longer than max_len
//     is in neither histogram but in too_long.  Block-private uint32 bins in dynamic LDS when both histograms fit 32 768 words,
//     flushed with one global integer atomic per non-zero bin and block; global integer atomics otherwise.  Integer counts either
//     way: exact and order-free.
//   * sites_count_kernel<RC> (discover_pwms): the same keys reduced to the count matrix of the site reads' best
//     windows instead -- one refinement step (pwm_refine.hip's select_best) for a batch of matrices.  The two entry points differ in
//     what they enqueue behind the scoring kernel.
#include <vector>

#include "common.h"
#include "pwm_batch.h"

namespace {

constexpr int ST_HIST_TPB = 1024;
constexpr int ST_HIST_BLOCKS = 512;      // blocks of one histogram launch, over all matrices of the batch
constexpr int64_t ST_HIST_LDS_WORDS = 32768;     // 128 KB of block-private uint32 bins (pwm_library.hip: LB_HIST_LDS_BINS)
constexpr int64_t ST_MAX_LEN = 1ll << 20;
constexpr int ST_HEAD = 2;               // words in front of a matrix's histograms: sites, too_long

using SiteBatch = PwmBatch<true>;

struct SiteHist {
    int width[PB_MAX_MAT];
    int64_t off[PB_MAX_MAT];    // acc[off] = sites, acc[off + 1] = too_long, then D[2 max_len + 1], then Hlen[max_len + 1]
};

// LDS: the histograms of the block's matrix in block-private bins, D then Hlen (the entry point decides: they fit)
template <bool LDS>
__global__ __launch_bounds__(ST_HIST_TPB) void sites_hist_kernel(const unsigned long long *__restrict__ key, int64_t n_seq,
                                                                 const int64_t *__restrict__ borders, SiteHist h, int max_len,
                                                                 unsigned long long *__restrict__ acc) {
    extern __shared__ uint32_t site_bins[];
    const int m = blockIdx.y;
    int width = 0;
    int64_t off = 0;
#pragma unroll
    for (int j = 0; j < PB_MAX_MAT; ++j)
        if (j == m) {                      // uniform
            width = h.width[j];
            off = h.off[j];
        }
    unsigned long long *a = acc + off;
    const int n_bins = 3 * max_len + 2, len0 = 2 * max_len + 1;      // Hlen's first bin
    if (LDS) {
        for (int b = threadIdx.x; b < n_bins; b += ST_HIST_TPB) site_bins[b] = 0;
        __syncthreads();
    }
    const unsigned long long *km = key + (int64_t)m * n_seq;
    unsigned long long sites = 0, too_long = 0;
    for (int64_t r = (int64_t)blockIdx.x * ST_HIST_TPB + threadIdx.x; r < n_seq; r += (int64_t)gridDim.x * ST_HIST_TPB) {
        const unsigned long long k = km[r];
        if (k == 0) continue;
        const int64_t loc = (int64_t)(0x7FFFFFFFu - (uint32_t)k), L = borders[2 * r + 1] - borders[2 * r];
        // the best window lies in its read (the borders' contract), so |d| <= L - width <= max_len; borders that break it must not
        // move a count out of the bins
        if (L > max_len || loc + width > L) {
            ++too_long;
            continue;
        }
        ++sites;
        const int d = (int)(2 * loc + width - L) + max_len, l = len0 + (int)L;
        if (LDS) {
            atomicAdd(&site_bins[d], 1u);
            atomicAdd(&site_bins[l], 1u);
        } else {
            atomicAdd(&a[ST_HEAD + d], 1ull);
            atomicAdd(&a[ST_HEAD + l], 1ull);
        }
    }
    sites = wave_sum(sites);
    too_long = wave_sum(too_long);
    if ((threadIdx.x & (KMAP_WAVE - 1)) == 0) {
        if (sites) atomicAdd(&a[0], sites);
        if (too_long) atomicAdd(&a[1], too_long);
    }
    if (LDS) {
        __syncthreads();
        for (int b = threadIdx.x; b < n_bins; b += ST_HIST_TPB) {
            const uint32_t c = site_bins[b];
            if (c) atomicAdd(&a[ST_HEAD + b], (unsigned long long)c);
        }
    }
}

// ---- sites_count_kernel: the count matrices of the site reads' best windows (discover_pwms) -------------------
constexpr int SC_TPB = 256;
constexpr int SC_BLOCKS = 2048;           // blocks of one counting launch, over all matrices of the batch: 8 waves per SIMD of 256 CUs
constexpr int SC_CELLS = 31 * 4;          // histogram cells [column][base], as pwm_refine.hip's
constexpr int SC_SELECTED = SC_CELLS;     // + the number of selected windows
constexpr int SC_MINUS = SC_CELLS + 1;    // + those on '-'
constexpr int SC_SLOTS = SC_CELLS + 2;    // 126

// blockIdx.y = the matrix, blockIdx.x strides over its keys.  A non-zero key gives loc, the window starts at borders[r][0] + loc and
// its width <= 31 codes lie in at most three code words; a word behind the window's last one is not read.  With RC the one window is
// scored again on both strands from the matrix's weights (the strand is not in the key); without RC nothing is scored.
template <bool RC>
__global__ __launch_bounds__(SC_TPB) void sites_count_kernel(const unsigned long long *__restrict__ key, int64_t n_seq,
                                                             const int64_t *__restrict__ borders, const uint32_t *__restrict__ codes,
                                                             int64_t n_data, const int32_t *__restrict__ weights, SiteBatch bt,
                                                             unsigned long long *__restrict__ acc) {
    __shared__ uint32_t hist[SC_SLOTS];    // a block sees fewer than 2^32 reads (checked by the caller)
    __shared__ int32_t wl[128];
    const int m = blockIdx.y;
    int width = 0, src = 0;
#pragma unroll
    for (int j = 0; j < PB_MAX_MAT; ++j)
        if (j == m) {                      // uniform
            width = bt.width[j];
            src = bt.src[j];
        }
    if (threadIdx.x < SC_SLOTS) hist[threadIdx.x] = 0;
    if (RC && threadIdx.x < 128) wl[threadIdx.x] = weights[(int64_t)src * 128 + threadIdx.x];
    __syncthreads();
    const unsigned long long *km = key + (int64_t)m * n_seq;
    for (int64_t r = (int64_t)blockIdx.x * SC_TPB + threadIdx.x; r < n_seq; r += (int64_t)gridDim.x * SC_TPB) {
        const unsigned long long k = km[r];
        if (k == 0) continue;
        const int64_t p = borders[2 * r] + (int64_t)(0x7FFFFFFFu - (uint32_t)k);
        const int64_t g = p >> 4, last = (p + width - 1) >> 4;
        // a selected window is valid and lies in its read, so last < n_data; borders that break that must not move a load out of the array
        if (p < 0 || last >= n_data) continue;
        const int off = (int)(p & 15);
        const uint32_t c0 = codes[g], c1 = last > g ? codes[g + 1] : 0u, c2 = last > g + 1 ? codes[g + 2] : 0u;
        uint64_t v = (((uint64_t)c0 << 32) | c1) << (2 * off);        // win_bits: the 32 bases from the window's first, in bits 63:62
        if (off > 0) v |= (uint64_t)c2 >> (32 - 2 * off);
        bool minus = false;
        if constexpr (RC) {
            int fwd = 0, rc = 0;
            for (int j = 0; j < width; ++j) {
                const int b = (int)(v >> (62 - 2 * j)) & 3;
                fwd += wl[b * 32 + j];
                rc += wl[(3 - b) * 32 + (width - 1 - j)];
            }
            minus = rc > fwd;              // a tie is '+'
        }
        for (int j = 0; j < width; ++j) {
            const int b = (int)(v >> (62 - 2 * j)) & 3;
            atomicAdd(&hist[minus ? (width - 1 - j) * 4 + (3 - b) : j * 4 + b], 1u);
        }
        atomicAdd(&hist[SC_SELECTED], 1u);
        if (minus) atomicAdd(&hist[SC_MINUS], 1u);
    }
    __syncthreads();
    if (threadIdx.x < SC_SLOTS) {
        const uint32_t c = hist[threadIdx.x];
        if (c) atomicAdd(&acc[(int64_t)m * SC_SLOTS + threadIdx.x], (unsigned long long)c);
    }
}

}  // namespace

extern "C" {

int kmap_readscore_sites_library_dev(const uint32_t *codes_dev, const uint16_t *inval_dev, int64_t n, const int64_t *borders_dev,
                                     int64_t n_seq, int n_mat, const int32_t *widths, const int32_t *weights, const int32_t *thresholds,
                                     int revcom, int64_t max_len, uint64_t *pos_hist_host, uint64_t *len_hist_host, int64_t *n_sites,
                                     int64_t *n_too_long, void *stream) {
    KMAP_REQUIRE(n_mat >= 0 && n >= 0 && n_seq >= 0, "readscore_sites_library: negative size");
    KMAP_REQUIRE(max_len >= 0, "readscore_sites_library: max_len=%lld is negative", (long long)max_len);
    if (max_len > ST_MAX_LEN) {
        kmap_set_error("readscore_sites_library: max_len=%lld, more than 2^20", (long long)max_len);
        return KMAP_E_UNSUP;
    }
    if (n_mat == 0) return KMAP_OK;
    KMAP_REQUIRE(widths && weights && thresholds && pos_hist_host && len_hist_host && n_sites && n_too_long,
                 "readscore_sites_library: null pointer");
    KMAP_TRY(pwm_library_check("readscore_sites_library", n_mat, widths, weights));
    const size_t pos_bins = 2 * (size_t)max_len + 1, len_bins = (size_t)max_len + 1, words = ST_HEAD + pos_bins + len_bins;
    memset(pos_hist_host, 0, (size_t)n_mat * pos_bins * 8);
    memset(len_hist_host, 0, (size_t)n_mat * len_bins * 8);
    memset(n_sites, 0, (size_t)n_mat * 8);
    memset(n_too_long, 0, (size_t)n_mat * 8);
    if (n_seq == 0 || n == 0) return KMAP_OK;          // no read, or no position: no site
    KMAP_REQUIRE(codes_dev && inval_dev && borders_dev, "readscore_sites_library: null pointer");
    hipStream_t st = as_stream(stream);

    const bool lds = (int64_t)(pos_bins + len_bins) <= ST_HIST_LDS_WORDS;
    unsigned long long *acc = nullptr;
    KMAP_TRY(kmap_scratch((void **)&acc, (size_t)std::min(n_mat, PB_MAX_MAT) * words * 8, st, KMAP_SLOT_B));
    if (lds) KMAP_TRY(kmap_allow_lds((const void *)sites_hist_kernel<true>, (int)(ST_HIST_LDS_WORDS * 4)));

    std::vector<unsigned long long> back;
    return pwm_key_batches<SiteKey>(
        "readscore_sites_library", codes_dev, inval_dev, n, borders_dev, n_seq, n_mat, widths, weights, thresholds, revcom, nullptr, 0, st,
        [&](const SiteBatch &bt, const unsigned long long *key, const int32_t *) -> int {
            SiteHist hs = {};
            for (int j = 0; j < bt.n_mat; ++j) {
                hs.width[j] = bt.width[j];
                hs.off[j] = (int64_t)((size_t)j * words);
            }
            const size_t batch_words = (size_t)bt.n_mat * words;
            KMAP_CHECK_HIP(hipMemsetAsync(acc, 0, batch_words * 8, st));
            const unsigned gx = (unsigned)std::max<int64_t>(1, std::min<int64_t>(grid_for(n_seq, ST_HIST_TPB), ST_HIST_BLOCKS / bt.n_mat));
            const dim3 hist_grid(gx, (unsigned)bt.n_mat);
            if (lds)
                sites_hist_kernel<true><<<hist_grid, ST_HIST_TPB, (pos_bins + len_bins) * 4, st>>>(key, n_seq, borders_dev, hs, (int)max_len, acc);
            else
                sites_hist_kernel<false><<<hist_grid, ST_HIST_TPB, 0, st>>>(key, n_seq, borders_dev, hs, (int)max_len, acc);
            KMAP_CHECK_HIP(hipGetLastError());
            back.resize(batch_words);
            KMAP_CHECK_HIP(hipMemcpyAsync(back.data(), acc, batch_words * 8, hipMemcpyDeviceToHost, st));
            KMAP_CHECK_HIP(hipStreamSynchronize(st));      // once per batch
            for (int j = 0; j < bt.n_mat; ++j) {
                const int m = bt.src[j];
                const unsigned long long *a = back.data() + hs.off[j];
                n_sites[m] = (int64_t)a[0];
                n_too_long[m] = (int64_t)a[1];
                memcpy(pos_hist_host + (size_t)m * pos_bins, a + ST_HEAD, pos_bins * 8);
                memcpy(len_hist_host + (size_t)m * len_bins, a + ST_HEAD + pos_bins, len_bins * 8);
            }
            return KMAP_OK;
        });
}

int kmap_readscore_counts_library_dev(const uint32_t *codes_dev, const uint16_t *inval_dev, int64_t n, const int64_t *borders_dev,
                                      int64_t n_seq, int n_mat, const int32_t *widths, const int32_t *weights, const int32_t *thresholds,
                                      int revcom, uint64_t *counts_host, int64_t *n_selected, int64_t *n_minus, void *stream) {
    KMAP_REQUIRE(n_mat >= 0 && n >= 0 && n_seq >= 0, "readscore_counts_library: negative size");
    KMAP_REQUIRE(n_seq < (1ll << 32), "readscore_counts_library: n_seq=%lld is 2^32 or more: a block-private cell is uint32",
                 (long long)n_seq);
    if (n_mat == 0) return KMAP_OK;
    KMAP_REQUIRE(widths && weights && thresholds && counts_host && n_selected && n_minus, "readscore_counts_library: null pointer");
    KMAP_TRY(pwm_library_check("readscore_counts_library", n_mat, widths, weights));
    memset(counts_host, 0, (size_t)n_mat * 128 * 8);
    memset(n_selected, 0, (size_t)n_mat * 8);
    memset(n_minus, 0, (size_t)n_mat * 8);
    if (n_seq == 0 || n == 0) return KMAP_OK;          // no read, or no position: no site
    KMAP_REQUIRE(codes_dev && inval_dev && borders_dev, "readscore_counts_library: null pointer");
    hipStream_t st = as_stream(stream);

    const int64_t n_data = (n + 15) >> 4;
    unsigned long long *acc = nullptr;
    KMAP_TRY(kmap_scratch((void **)&acc, (size_t)PB_MAX_MAT * SC_SLOTS * 8, st, KMAP_SLOT_B));
    unsigned long long back[PB_MAX_MAT * SC_SLOTS];
    return pwm_key_batches<SiteKey>(
        "readscore_counts_library", codes_dev, inval_dev, n, borders_dev, n_seq, n_mat, widths, weights, thresholds, revcom, nullptr, 0, st,
        [&](const SiteBatch &bt, const unsigned long long *key, const int32_t *weights_dev) -> int {
            const size_t batch_words = (size_t)bt.n_mat * SC_SLOTS;
            KMAP_CHECK_HIP(hipMemsetAsync(acc, 0, batch_words * 8, st));
            const unsigned gx = (unsigned)std::max<int64_t>(1, std::min<int64_t>(grid_for(n_seq, SC_TPB), SC_BLOCKS / bt.n_mat));
            const dim3 count_grid(gx, (unsigned)bt.n_mat);
            with_bool(revcom, [&](auto rc) {
                sites_count_kernel<decltype(rc)::value><<<count_grid, SC_TPB, 0, st>>>(key, n_seq, borders_dev, codes_dev, n_data,
                                                                                      weights_dev, bt, acc);
            });
            KMAP_CHECK_HIP(hipGetLastError());
            KMAP_CHECK_HIP(hipMemcpyAsync(back, acc, batch_words * 8, hipMemcpyDeviceToHost, st));
            KMAP_CHECK_HIP(hipStreamSynchronize(st));      // once per batch
            for (int j = 0; j < bt.n_mat; ++j) {
                const int m = bt.src[j];
                const unsigned long long *a = back + (size_t)j * SC_SLOTS;
                uint64_t *c = counts_host + (size_t)m * 128;
                for (int b = 0; b < 4; ++b)
                    for (int col = 0; col < bt.width[j]; ++col) c[b * 32 + col] = a[col * 4 + b];
                n_selected[m] = (int64_t)a[SC_SELECTED];
                n_minus[m] = (int64_t)a[SC_MINUS];
            }
            return KMAP_OK;
        });
}

}  // extern "C"
