// pwm_spacing.hip -- at which distance and in which orientation the best site of every matrix of a library lies from the primary
// matrix's site (motif_spacing).  The scoring is pwm_batch.h's batched pass with the key that carries the
// strand (PairKey), under which a window that overlaps the read's primary site (or lies in a read without one) is never a
// candidate, and behind it a reduction of the keys to two small integer histograms per matrix, so that nothing per read leaves the
// device.
//
//   * spacing_primary_kernel: ploc[r] = the primary's best loc of read r when that window scores prim_threshold or more, else -1,
//     from a ReadScores' score and loc arrays; the number of primary reads.
//   * spacing_hist_kernel: blockIdx.y = the matrix, blockIdx.x strides over its keys.  A non-zero key gives loc and strand of the
//     secondary site; ploc[r], prim_strand[r] and the read's two borders give p, sP and L; then the gap g, the quadrant
//     2 downstream + opposite and the two rooms (u, d) go into one flat uint64 array per matrix: n_pair, n_far, S[4][G + 1],
//     R[G + 2][G + 2], with global integer atomics (pair reads are a small share of the reads).  Integer counts: exact and order-free.
#include <vector>

#include "common.h"
#include "pwm_batch.h"

namespace {

constexpr int SP_MAX_GAP = 511;          // device_seq.py: SPACING_MAX_GAP; R alone is then 2 MB per matrix
constexpr int SP_HIST_TPB = 1024;
constexpr int SP_HIST_BLOCKS = 512;      // blocks of one histogram launch, over all matrices of the batch
constexpr int SP_HEAD = 2;               // words in front of a matrix's histograms: n_pair, n_far

// n_primary = acc[0]
__global__ __launch_bounds__(256) void spacing_primary_kernel(const int32_t *__restrict__ score, const int32_t *__restrict__ loc,
                                                              int64_t n_seq, int32_t thr, int32_t *__restrict__ ploc,
                                                              unsigned long long *__restrict__ acc) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool prim = false;
    if (r < n_seq) {
        const int32_t l = loc[r];
        prim = l >= 0 && score[r] >= thr;
        ploc[r] = prim ? l : -1;
    }
    const int c = __builtin_popcountll(__ballot(prim));
    if ((threadIdx.x & (KMAP_WAVE - 1)) == 0 && c) atomicAdd(acc, (unsigned long long)c);
}

struct SpacingHist {
    int width[PB_MAX_MAT];
    int64_t off[PB_MAX_MAT];    // acc[off] = n_pair, acc[off + 1] = n_far, then S[4][G + 1], then R[G + 2][G + 2]
};

__global__ __launch_bounds__(SP_HIST_TPB) void spacing_hist_kernel(const unsigned long long *__restrict__ key, int64_t n_seq,
                                                                   const int64_t *__restrict__ borders, const int32_t *__restrict__ ploc,
                                                                   const uint8_t *__restrict__ prim_strand, int prim_width, SpacingHist h,
                                                                   int max_gap, unsigned long long *__restrict__ acc) {
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
    unsigned long long *S = a + SP_HEAD, *R = S + 4 * (max_gap + 1);
    const unsigned long long *km = key + (int64_t)m * n_seq;
    unsigned long long pairs = 0, far = 0;
    for (int64_t r = (int64_t)blockIdx.x * SP_HIST_TPB + threadIdx.x; r < n_seq; r += (int64_t)gridDim.x * SP_HIST_TPB) {
        const unsigned long long k = km[r];
        if (k == 0) continue;
        ++pairs;
        const uint32_t low = (uint32_t)k;
        const int64_t loc = (int64_t)(0x7FFFFFFFu - (low >> 1)), p = ploc[r], L = borders[2 * r + 1] - borders[2 * r];
        const bool minus = low & 1u, prim_minus = prim_strand[r] != 0;
        const bool is_left = loc + width <= p, is_right = loc >= p + prim_width;
        const int64_t gap = is_left ? p - loc - width : loc - p - prim_width;
        // both windows lie in their read and do not overlap (the borders' contract and the scoring kernel's test), so in range
        // 0 <= gap < the room of its side; borders or a ploc that break it must not move a count out of the bins
        if (p < 0 || !(is_left || is_right) || p + prim_width > L || loc + width > L || gap > max_gap) {
            ++far;
            continue;
        }
        // the window positions on each side with a gap of at most max_gap
        const int64_t cap = (int64_t)max_gap + 1, lr = p - width + 1, rr = L - p - prim_width - width + 1;
        const int64_t left_room = lr < 0 ? 0 : lr > cap ? cap : lr, right_room = rr < 0 ? 0 : rr > cap ? cap : rr;
        const int downstream = is_right != prim_minus, opposite = minus != prim_minus;
        const int64_t u = prim_minus ? right_room : left_room, d = prim_minus ? left_room : right_room;
        atomicAdd(&S[(2 * downstream + opposite) * (max_gap + 1) + (int)gap], 1ull);
        atomicAdd(&R[u * (max_gap + 2) + d], 1ull);
    }
    pairs = wave_sum(pairs);
    far = wave_sum(far);
    if ((threadIdx.x & (KMAP_WAVE - 1)) == 0) {
        if (pairs) atomicAdd(&a[0], pairs);
        if (far) atomicAdd(&a[1], far);
    }
}

}  // namespace

extern "C" {

int kmap_readscore_spacing_library_dev(const uint32_t *codes_dev, const uint16_t *inval_dev, int64_t n, const int64_t *borders_dev,
                                       int64_t n_seq, const int32_t *prim_score_dev, const int32_t *prim_loc_dev,
                                       const uint8_t *prim_strand_dev, int prim_width, int32_t prim_threshold, int n_mat,
                                       const int32_t *widths, const int32_t *weights, const int32_t *thresholds, int revcom, int max_gap,
                                       uint64_t *gap_hist_host, uint64_t *room_hist_host, int64_t *n_primary, int64_t *n_pair,
                                       int64_t *n_far, void *stream) {
    KMAP_REQUIRE(n_mat >= 0 && n >= 0 && n_seq >= 0, "readscore_spacing_library: negative size");
    KMAP_REQUIRE(max_gap >= 0, "readscore_spacing_library: max_gap=%d is negative", max_gap);
    if (max_gap > SP_MAX_GAP) {
        kmap_set_error("readscore_spacing_library: max_gap=%d, more than %d", max_gap, SP_MAX_GAP);
        return KMAP_E_UNSUP;
    }
    KMAP_REQUIRE(prim_width >= 4 && prim_width <= 31, "readscore_spacing_library: prim_width=%d outside 4..31", prim_width);
    KMAP_REQUIRE(n_primary, "readscore_spacing_library: null pointer");
    KMAP_REQUIRE(n_mat == 0 || (widths && weights && thresholds && gap_hist_host && room_hist_host && n_pair && n_far),
                 "readscore_spacing_library: null pointer");
    if (n_mat) KMAP_TRY(pwm_library_check("readscore_spacing_library", n_mat, widths, weights));
    KMAP_REQUIRE(n_seq == 0 || (prim_score_dev && prim_loc_dev && prim_strand_dev && borders_dev),
                 "readscore_spacing_library: null pointer");
    KMAP_REQUIRE(n_seq == 0 || n == 0 || n_mat == 0 || (codes_dev && inval_dev), "readscore_spacing_library: null pointer");
    const size_t gap_bins = 4 * ((size_t)max_gap + 1), room_bins = ((size_t)max_gap + 2) * ((size_t)max_gap + 2);
    const size_t words = SP_HEAD + gap_bins + room_bins;
    *n_primary = 0;
    if (n_mat) {
        memset(gap_hist_host, 0, (size_t)n_mat * gap_bins * 8);
        memset(room_hist_host, 0, (size_t)n_mat * room_bins * 8);
        memset(n_pair, 0, (size_t)n_mat * 8);
        memset(n_far, 0, (size_t)n_mat * 8);
    }
    if (n_seq == 0) return KMAP_OK;                    // no read: no primary read
    hipStream_t st = as_stream(stream);

    // the primary reads: a counter, then ploc[n_seq]
    unsigned long long *prim = nullptr;
    KMAP_TRY(kmap_scratch((void **)&prim, 8 + (size_t)n_seq * 4, st, KMAP_SLOT_D));
    int32_t *ploc = (int32_t *)(prim + 1);
    KMAP_CHECK_HIP(hipMemsetAsync(prim, 0, 8, st));
    spacing_primary_kernel<<<grid_for(n_seq, 256), 256, 0, st>>>(prim_score_dev, prim_loc_dev, n_seq, prim_threshold, ploc, prim);
    KMAP_CHECK_HIP(hipGetLastError());
    unsigned long long primary = 0;
    if (n_mat == 0 || n == 0) {                        // no matrix, or no position: no pair
        KMAP_CHECK_HIP(hipMemcpyAsync(&primary, prim, 8, hipMemcpyDeviceToHost, st));
        KMAP_CHECK_HIP(hipStreamSynchronize(st));
        *n_primary = (int64_t)primary;
        return KMAP_OK;
    }

    unsigned long long *acc = nullptr;
    KMAP_TRY(kmap_scratch((void **)&acc, (size_t)std::min(n_mat, PB_MAX_MAT) * words * 8, st, KMAP_SLOT_B));
    std::vector<unsigned long long> back;
    bool first = true;                                 // the first batch's synchronisation brings n_primary along
    KMAP_TRY(pwm_key_batches<PairKey>(
        "readscore_spacing_library", codes_dev, inval_dev, n, borders_dev, n_seq, n_mat, widths, weights, thresholds, revcom,
        ploc, prim_width, st, [&](const PwmBatch<true> &bt, const unsigned long long *key, const int32_t *) -> int {
            SpacingHist hs = {};
            for (int j = 0; j < bt.n_mat; ++j) {
                hs.width[j] = bt.width[j];
                hs.off[j] = (int64_t)((size_t)j * words);
            }
            const size_t batch_words = (size_t)bt.n_mat * words;
            KMAP_CHECK_HIP(hipMemsetAsync(acc, 0, batch_words * 8, st));
            const unsigned gx = (unsigned)std::max<int64_t>(1, std::min<int64_t>(grid_for(n_seq, SP_HIST_TPB), SP_HIST_BLOCKS / bt.n_mat));
            spacing_hist_kernel<<<dim3(gx, (unsigned)bt.n_mat), SP_HIST_TPB, 0, st>>>(key, n_seq, borders_dev, ploc, prim_strand_dev,
                                                                                      prim_width, hs, max_gap, acc);
            KMAP_CHECK_HIP(hipGetLastError());
            back.resize(batch_words);
            if (first) KMAP_CHECK_HIP(hipMemcpyAsync(&primary, prim, 8, hipMemcpyDeviceToHost, st));
            first = false;
            KMAP_CHECK_HIP(hipMemcpyAsync(back.data(), acc, batch_words * 8, hipMemcpyDeviceToHost, st));
            KMAP_CHECK_HIP(hipStreamSynchronize(st));      // once per batch
            for (int j = 0; j < bt.n_mat; ++j) {
                const int m = bt.src[j];
                const unsigned long long *a = back.data() + hs.off[j];
                n_pair[m] = (int64_t)a[0];
                n_far[m] = (int64_t)a[1];
                memcpy(gap_hist_host + (size_t)m * gap_bins, a + SP_HEAD, gap_bins * 8);
                memcpy(room_hist_host + (size_t)m * room_bins, a + SP_HEAD + gap_bins, room_bins * 8);
            }
            return KMAP_OK;
        }));
    *n_primary = (int64_t)primary;
    return KMAP_OK;
}

}  // extern "C"
