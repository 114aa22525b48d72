// pwm_library.hip -- the histograms of the best score of every read under every matrix of a library (rank_motif_library, DESIGN.md
// section 16).  The scoring is pwm_batch.h's batched pass with the score alone as the key (ScoreKey: no loc, no strand, no per-read
// arrays leave the device), so a key is 32 bits and the histogram reads the keys directly.
//
//   * library_hist_kernel: blockIdx.y = the matrix, blockIdx.x strides over its keys.  uint64 bins of all matrices of the batch in
//     one flat array (per matrix: outside, unscorable, then its n_bins bins).  A matrix whose range fits is counted in block-private
//     uint32 bins in dynamic LDS and flushed with one global integer atomic per non-zero bin and block; wider ranges go to global
//     integer atomics directly.  Integer counts either way: exact and order-free.
#include <vector>

#include "common.h"
#include "pwm_batch.h"

namespace {

constexpr int LB_HIST_TPB = 1024;
constexpr int LB_HIST_BLOCKS = 512;      // blocks of one histogram launch, over all matrices of the batch
// Ranges up to this many bins are privatised per block: 128 KB of uint32 counters in dynamic LDS, the size counts_fine.hip's
// fine_hist_kernel already runs with; one such block fills a CU's LDS (160 KB), a larger array would leave no room for a second
// kernel's blocks beside it.  A 31-column matrix at pseudocount 1 spans about 20 000 scores, so libraries fit as a rule.  A block
// counts at most n_seq / 64 reads (the launch has 64 blocks or more per matrix once n_seq >= 65 536): a uint32 bin would need
// 2^38 reads, a terabyte of keys, to overflow.
constexpr int64_t LB_HIST_LDS_BINS = 32768;
constexpr int64_t LB_MAX_BINS = 1ll << 22;

struct LibHist {
    int n_mat;
    int lds[PB_MAX_MAT];        // the range fits the block-private bins
    int32_t lo[PB_MAX_MAT];
    int64_t n_bins[PB_MAX_MAT];
    int64_t off[PB_MAX_MAT];    // acc[off] = outside, acc[off + 1] = unscorable, acc[off + 2 ..] = the bins
};

__global__ __launch_bounds__(LB_HIST_TPB) void library_hist_kernel(const unsigned int *__restrict__ key, int64_t n_seq, LibHist h,
                                                                   unsigned long long *__restrict__ acc) {
    extern __shared__ uint32_t lib_bins[];
    const int m = blockIdx.y;
    int lds = 0;
    int32_t lo = 0;
    int64_t n_bins = 0, off = 0;
#pragma unroll
    for (int j = 0; j < PB_MAX_MAT; ++j)
        if (j == m) {                      // uniform
            lds = h.lds[j];
            lo = h.lo[j];
            n_bins = h.n_bins[j];
            off = h.off[j];
        }
    unsigned long long *a = acc + off;
    if (lds) {
        for (int b = threadIdx.x; b < n_bins; b += LB_HIST_TPB) lib_bins[b] = 0;
        __syncthreads();
    }
    const unsigned int *km = key + (int64_t)m * n_seq;
    unsigned long long outside = 0, unscorable = 0;
    for (int64_t r = (int64_t)blockIdx.x * LB_HIST_TPB + threadIdx.x; r < n_seq; r += (int64_t)gridDim.x * LB_HIST_TPB) {
        const uint32_t k = km[r];
        if (k == 0) {
            ++unscorable;
            continue;
        }
        const int64_t b = (int64_t)(int32_t)(k ^ 0x80000000u) - lo;
        if (b < 0 || b >= n_bins) ++outside;
        else if (lds) atomicAdd(&lib_bins[b], 1u);
        else atomicAdd(&a[2 + b], 1ull);
    }
    outside = wave_sum(outside);
    unscorable = wave_sum(unscorable);
    if ((threadIdx.x & (KMAP_WAVE - 1)) == 0) {
        if (outside) atomicAdd(&a[0], outside);
        if (unscorable) atomicAdd(&a[1], unscorable);
    }
    if (lds) {
        __syncthreads();
        for (int b = threadIdx.x; b < n_bins; b += LB_HIST_TPB) {
            const uint32_t c = lib_bins[b];
            if (c) atomicAdd(&a[2 + b], (unsigned long long)c);
        }
    }
}

}  // namespace

extern "C" {

int kmap_readscore_library_dev(const uint32_t *codes_dev, const uint16_t *inval_dev, int64_t n, const int64_t *borders_dev,
                               int64_t n_seq, int n_mat, const int32_t *widths, const int32_t *weights, const int32_t *lo,
                               const int64_t *n_bins, int revcom, uint64_t *hist_host, int64_t *n_outside, int64_t *n_scored,
                               void *stream) {
    KMAP_REQUIRE(n_mat >= 0 && n >= 0 && n_seq >= 0, "readscore_library: negative size");
    if (n_mat == 0) return KMAP_OK;
    KMAP_REQUIRE(widths && weights && lo && n_bins && n_outside && n_scored, "readscore_library: null pointer");
    size_t total_bins = 0;
    for (int m = 0; m < n_mat; ++m) {
        KMAP_REQUIRE(widths[m] >= 4 && widths[m] <= 31, "readscore_library: width=%d of matrix %d outside 4..31", widths[m], m);
        KMAP_REQUIRE(n_bins[m] >= 0, "readscore_library: negative size");
        if (n_bins[m] > LB_MAX_BINS) {
            kmap_set_error("readscore_library: %lld bins for matrix %d, more than 2^22", (long long)n_bins[m], m);
            return KMAP_E_UNSUP;
        }
        KMAP_TRY(pwm_library_check("readscore_library", 1, widths + m, weights + (size_t)m * 128));
        total_bins += (size_t)n_bins[m];
    }
    KMAP_REQUIRE(hist_host || total_bins == 0, "readscore_library: null histogram");
    if (total_bins) memset(hist_host, 0, total_bins * 8);
    memset(n_outside, 0, (size_t)n_mat * 8);
    memset(n_scored, 0, (size_t)n_mat * 8);
    if (n_seq == 0 || n == 0) return KMAP_OK;          // no read, or no position: nothing is scorable
    KMAP_REQUIRE(codes_dev && inval_dev && borders_dev, "readscore_library: null pointer");
    hipStream_t st = as_stream(stream);

    std::vector<size_t> host_off(n_mat);               // the matrix's first bin in hist_host
    for (size_t m = 0, at = 0; m < (size_t)n_mat; at += (size_t)n_bins[m], ++m) host_off[m] = at;
    KMAP_TRY(kmap_allow_lds((const void *)library_hist_kernel, (int)(LB_HIST_LDS_BINS * 4)));

    std::vector<unsigned long long> back;
    return pwm_key_batches<ScoreKey>(
        "readscore_library", codes_dev, inval_dev, n, borders_dev, n_seq, n_mat, widths, weights, nullptr, revcom, nullptr, 0, st,
        [&](const PwmBatch<false> &bt, const unsigned int *key, const int32_t *) -> int {
        LibHist hs = {};
        int64_t words = 0, lds_bins = 1;
        for (int j = 0; j < bt.n_mat; ++j) {
            const int m = bt.src[j];
            hs.lds[j] = n_bins[m] <= LB_HIST_LDS_BINS;
            hs.lo[j] = lo[m];
            hs.n_bins[j] = n_bins[m];
            hs.off[j] = words;
            words += 2 + n_bins[m];
            if (hs.lds[j]) lds_bins = std::max(lds_bins, n_bins[m]);
        }
        hs.n_mat = bt.n_mat;
        unsigned long long *acc = nullptr;
        KMAP_TRY(kmap_scratch((void **)&acc, (size_t)words * 8, st, KMAP_SLOT_B));
        KMAP_CHECK_HIP(hipMemsetAsync(acc, 0, (size_t)words * 8, st));
        const unsigned gx = (unsigned)std::max<int64_t>(1, std::min<int64_t>(grid_for(n_seq, LB_HIST_TPB), LB_HIST_BLOCKS / bt.n_mat));
        library_hist_kernel<<<dim3(gx, (unsigned)bt.n_mat), LB_HIST_TPB, (size_t)lds_bins * 4, st>>>(key, n_seq, hs, acc);
        KMAP_CHECK_HIP(hipGetLastError());
        back.resize((size_t)words);
        KMAP_CHECK_HIP(hipMemcpyAsync(back.data(), acc, (size_t)words * 8, hipMemcpyDeviceToHost, st));
        KMAP_CHECK_HIP(hipStreamSynchronize(st));      // once per batch
        for (int j = 0; j < bt.n_mat; ++j) {
            const int m = bt.src[j];
            const unsigned long long *a = back.data() + hs.off[j];
            n_outside[m] = (int64_t)a[0];
            n_scored[m] = n_seq - (int64_t)a[1];
            if (n_bins[m]) memcpy(hist_host + host_off[m], a + 2, (size_t)n_bins[m] * 8);
        }
        return KMAP_OK;
    });
}

}  // extern "C"
