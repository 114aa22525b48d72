// pwm_presence.hip -- which reads hold a site of which matrix of a library, one bit per (matrix, read) (motif_cooccurrence, DESIGN.md
// section 20).  The scoring is pwm_batch.h's batched pass with the score alone as the key (ScoreKey), as pwm_library.hip runs it: it
// leaves the 32-bit keys of a batch -- the best score of every read with the sign bit flipped, 0 = no valid window -- in scratch.
// Behind it:
//   * presence_kernel: blockIdx.y = the matrix of the batch, the waves stride over the 64-read words of its row.  A lane reads one
//     key, compares it with the flipped threshold (unsigned order of flipped keys = signed order of scores; key 0 is never present,
//     whatever the threshold), the wave ballots, lane 0 writes the word with a plain vector store -- every word of the row is
//     written, the lanes behind n_seq vote 0, so the tail bits are zero and the planes need no memset.  The ballot's popcount is the
//     wave's sum already; a wave adds its running count to n_present with one integer atomic at the end.  Integers only: two calls
//     give the same bits and counts.
// The batches are queued on the stream without a synchronisation in between; the entry point synchronises once, for the counts.
#include <vector>

#include "common.h"
#include "pwm_batch.h"

namespace {

constexpr int PR_TPB = 256;
constexpr int PR_WAVES = PR_TPB / KMAP_WAVE;
constexpr int PR_BLOCKS = 2048;          // blocks of one launch, over all matrices of the batch

struct PresBatch {
    uint32_t tkey[PB_MAX_MAT];           // the threshold with the sign bit flipped
    int src[PB_MAX_MAT];                 // the matrix's row in the planes and in n_present
};

__global__ __launch_bounds__(PR_TPB) void presence_kernel(const unsigned int *__restrict__ key, int64_t n_seq, int64_t n_words, PresBatch pb,
                                                          unsigned long long *__restrict__ planes, unsigned long long *__restrict__ n_present) {
    const int j = blockIdx.y, lane = threadIdx.x & (KMAP_WAVE - 1);
    uint32_t tkey = 0;
    int src = 0;
#pragma unroll
    for (int i = 0; i < PB_MAX_MAT; ++i)
        if (i == j) {                      // uniform
            tkey = pb.tkey[i];
            src = pb.src[i];
        }
    const unsigned int *km = key + (int64_t)j * n_seq;
    unsigned long long *row = planes + (int64_t)src * n_words;
    unsigned long long cnt = 0;            // the same in every lane
    for (int64_t w = (int64_t)blockIdx.x * PR_WAVES + (threadIdx.x >> 6); w < n_words; w += (int64_t)gridDim.x * PR_WAVES) {
        const int64_t r = w * KMAP_WAVE + lane;
        const uint32_t k = r < n_seq ? km[r] : 0u;
        const unsigned long long bits = __ballot(k != 0 && k >= tkey);
        if (lane == 0) row[w] = bits;
        cnt += (unsigned long long)__builtin_popcountll(bits);
    }
    if (lane == 0 && cnt) atomicAdd(&n_present[src], cnt);
}

}  // namespace

extern "C" {

int kmap_presence_library_dev(const uint32_t *codes_dev, const uint16_t *inval_dev, int64_t n, const int64_t *borders_dev, int64_t n_seq,
                              int n_mat, const int32_t *widths, const int32_t *weights, const int32_t *thresholds, int revcom,
                              uint64_t *planes_dev, int64_t n_words, int64_t *n_present, void *stream) {
    KMAP_REQUIRE(n_mat >= 0 && n >= 0 && n_seq >= 0 && n_words >= 0, "presence_library: negative size");
    KMAP_REQUIRE(n_words == (n_seq + 63) / 64, "presence_library: %lld words per row for %lld reads, (n_seq + 63) / 64 expected",
                 (long long)n_words, (long long)n_seq);
    if (n_mat == 0) return KMAP_OK;
    KMAP_REQUIRE(widths && weights && thresholds && n_present, "presence_library: null pointer");
    KMAP_TRY(pwm_library_check("presence_library", n_mat, widths, weights));
    memset(n_present, 0, (size_t)n_mat * 8);
    if (n_seq == 0) return KMAP_OK;                    // no read: the rows have no word
    KMAP_REQUIRE(planes_dev, "presence_library: null pointer");
    hipStream_t st = as_stream(stream);
    if (n == 0) {                                      // no position: nothing is scorable
        KMAP_CHECK_HIP(hipMemsetAsync(planes_dev, 0, (size_t)n_mat * (size_t)n_words * 8, st));
        KMAP_CHECK_HIP(hipStreamSynchronize(st));
        return KMAP_OK;
    }
    KMAP_REQUIRE(codes_dev && inval_dev && borders_dev, "presence_library: null pointer");

    unsigned long long *cnt_dev = nullptr;
    KMAP_TRY(kmap_scratch((void **)&cnt_dev, (size_t)n_mat * 8, st, KMAP_SLOT_B));
    KMAP_CHECK_HIP(hipMemsetAsync(cnt_dev, 0, (size_t)n_mat * 8, st));
    KMAP_TRY(pwm_key_batches<ScoreKey>(
        "presence_library", codes_dev, inval_dev, n, borders_dev, n_seq, n_mat, widths, weights, nullptr, revcom, nullptr, 0, st,
        [&](const PwmBatch<false> &bt, const unsigned int *key, const int32_t *) -> int {
        PresBatch pb = {};
        for (int j = 0; j < bt.n_mat; ++j) {
            pb.src[j] = bt.src[j];
            pb.tkey[j] = (uint32_t)thresholds[bt.src[j]] ^ 0x80000000u;
        }
        const unsigned gx = (unsigned)std::max<int64_t>(1, std::min<int64_t>(grid_for(n_words, PR_WAVES), PR_BLOCKS / bt.n_mat));
        presence_kernel<<<dim3(gx, (unsigned)bt.n_mat), PR_TPB, 0, st>>>(key, n_seq, n_words, pb,
                                                                           (unsigned long long *)planes_dev, cnt_dev);
        KMAP_CHECK_HIP(hipGetLastError());
        return KMAP_OK;
    }));
    std::vector<unsigned long long> back((size_t)n_mat);
    KMAP_CHECK_HIP(hipMemcpyAsync(back.data(), cnt_dev, (size_t)n_mat * 8, hipMemcpyDeviceToHost, st));
    KMAP_CHECK_HIP(hipStreamSynchronize(st));
    for (int m = 0; m < n_mat; ++m) n_present[m] = (int64_t)back[m];
    return KMAP_OK;
}

}  // extern "C"
