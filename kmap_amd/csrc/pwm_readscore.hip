// pwm_readscore.hip -- the best window of every read under a weight matrix (evaluate_pwm): a dense pass over
// the packed reads that reduces section 11's score of every valid window to one (score, loc, strand) per read, and the histogram
// of those scores.  No threshold, no hit list, no scan handle: scratch slots only.
//
//   * readscore_kernel<RC>: persistent blocks over wave tiles of 64 groups x 16 positions, the tables, loads and window helpers of
//     pwm_internal.h.  Per tile the wave finds ONCE how many reads start before the tile (a 64-ary search of the borders: the 64
//     lanes probe 64 borders per step, a ballot narrows the range 64-fold -- 4 steps at 10^7 reads), then marks the read starts
//     that fall inside the tile in a per-wave LDS bitmap (one bit per position) and a per-group count.  A prefix sum of the counts
//     gives every lane the read of its first position; a set bit moves the lane to the next read.
//   * A lane reduces its 16 windows into segments, one per read, with the key
//         (score with the sign bit flipped) << 32 | (0x7FFFFFFF - loc) << 1 | strand
//     so the largest score wins and on a tie the smallest loc; equal (score, loc) means the same window, hence the same strand:
//     the strand bit rides below everything that orders.  A read that begins and ends inside the lane's 16 positions is complete
//     there and goes to key[read] at once; the segment that reaches the lane from the left (head) and the one that leaves it to
//     the right (tail) are combined across lanes by a segmented max scan (shuffles), and ONE unsigned 64-bit atomicMax per
//     (wave, read) reaches key[read].  A maximum does not depend on the order of its operands: the result is deterministic.
//     Zero = "no valid window" (a real key would need loc = 2^31 - 1, past any int32 read length).
//   * readscore_unpack_kernel: key -> score / loc / strand (INT32_MIN / -1 / 0 for a zero key) + the number of scorable reads.
//   * readscore_hist_kernel<LDS>: uint64 histogram of the scorable reads' scores; block-private uint32 bins in LDS when the range
//     fits (then one global integer atomic per non-zero bin and block), global integer atomics otherwise.  Order-free either way.
#include "common.h"
#include "pwm_internal.h"

namespace {

constexpr int RS_LDS_BINS = 4096;                     // histogram ranges up to this many bins are privatised per block
constexpr int RS_HIST_BLOCKS = 1024;
constexpr int64_t RS_MAX_BINS = 1ll << 22;

__device__ __forceinline__ uint64_t pack_read_key(int score, uint32_t loc, bool minus) {
    return ((uint64_t)((uint32_t)score ^ 0x80000000u) << 32) | ((uint64_t)(0x7FFFFFFFu - loc) << 1) | (minus ? 1u : 0u);
}

template <bool RC>
__global__ __launch_bounds__(PW_TPB) void readscore_kernel(const uint32_t *__restrict__ codes, const uint16_t *__restrict__ inval,
                                                           int64_t n_data, int64_t n_tiles, PwmWeights wt, int width, int nch,
                                                           const int64_t *__restrict__ borders, int64_t n_seq,
                                                           unsigned long long *__restrict__ key) {
    __shared__ int2 tab[PW_MAX_CHUNKS * 256];
    __shared__ int32_t wl[128];
    __shared__ uint32_t start_bits[PW_WAVES][KMAP_WAVE];   // per group of the wave's tile: read starts, position 0 in bit 15
    __shared__ uint32_t start_cnt[PW_WAVES][KMAP_WAVE];    // and how many reads start there (reads may share a start)
    build_table(tab, wl, wt, width, nch);
    const int lane = threadIdx.x & (KMAP_WAVE - 1), wave = threadIdx.x >> 6;
    const uint64_t wmask = (1ull << width) - 1ull;
    for (int64_t t = (int64_t)blockIdx.x * PW_WAVES + wave; t < n_tiles; t += (int64_t)gridDim.x * PW_WAVES) {
        const int64_t g = t * PW_TILE_GROUPS + lane, tile0 = t * RS_TILE_POS;
        const Grp w = load_grp(codes, inval, g, n_data, lane);
        // the reads of the tile (tile_read_starts, pwm_internal.h): r = the last read that starts before the group's first position
        uint32_t sb, sc;
        int64_t r = tile_read_starts(borders, n_seq, tile0, lane, start_bits[wave], start_cnt[wave], sb, sc);
        uint32_t loc0 = (uint32_t)(g * 16 - (r >= 0 ? borders[2 * r] : 0));    // loc of the group's first position (an int32 in a read)
        const bool shared_starts = sc != (uint32_t)__builtin_popcount(sb);
        uint64_t cur = 0, head = 0;                    // the running segment; the one that reached the lane from the left
        int64_t r_head = r;
        bool split = false;                            // a read starts in this group
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            if (sb & (0x8000u >> i)) {
                if (!split) {
                    head = cur;
                    split = true;
                } else if (cur) {
                    atomicMax(&key[r], (unsigned long long)cur);   // a read that began and ends in this group
                }
                cur = 0;
                step_read(borders, n_seq, g * 16 + i, shared_starts, r);   // the last read that starts here
                loc0 = (uint32_t)-i;
            }
            int fwd, rc;
            win_score<RC>(tab, win_bits(w, i), nch, fwd, rc);
            if (win_valid(w, i, width, wmask) && r >= 0) {
                const bool minus = RC && rc > fwd;
                const uint64_t k = pack_read_key(minus ? rc : fwd, loc0 + i, minus);
                cur = k > cur ? k : cur;
            }
        }
        // lanes of one read: inclusive segmented maximum of the tails, a lane with a read start opens a segment
        uint64_t seg = cur;
        int open = split ? 1 : 0;
        for (int o = 1; o < KMAP_WAVE; o <<= 1) {
            const uint64_t up = __shfl_up((unsigned long long)seg, o);
            const int up_open = __shfl_up(open, o);
            if (lane >= o && !open) {
                seg = up > seg ? up : seg;
                open = up_open;
            }
        }
        uint64_t left = __shfl_up((unsigned long long)seg, 1);      // what the lanes to the left hold of this lane's first read
        if (lane == 0) left = 0;
        if (split && r_head >= 0) {
            const uint64_t m = head > left ? head : left;
            if (m) atomicMax(&key[r_head], (unsigned long long)m);
        }
        if (lane == KMAP_WAVE - 1 && seg && r >= 0) atomicMax(&key[r], (unsigned long long)seg);   // the read that leaves the tile
    }
}

__global__ __launch_bounds__(256) void readscore_unpack_kernel(const unsigned long long *__restrict__ key, int64_t n_seq,
                                                               int32_t *__restrict__ score, int32_t *__restrict__ loc,
                                                               uint8_t *__restrict__ strand, unsigned long long *__restrict__ n_scored) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const unsigned long long k = r < n_seq ? key[r] : 0ull;
    if (r < n_seq) {
        const uint32_t low = (uint32_t)k;
        score[r] = k ? (int32_t)((uint32_t)(k >> 32) ^ 0x80000000u) : INT32_MIN;
        loc[r] = k ? (int32_t)(0x7FFFFFFFu - (low >> 1)) : -1;
        strand[r] = k ? (uint8_t)(low & 1u) : (uint8_t)0;
    }
    const int c = __builtin_popcountll(__ballot(k != 0));
    if ((threadIdx.x & (KMAP_WAVE - 1)) == 0 && c) atomicAdd(n_scored, (unsigned long long)c);
}

// acc[0 .. n_bins) = the histogram, acc[n_bins] = scorable reads outside the range
template <bool LDS>
__global__ __launch_bounds__(256) void readscore_hist_kernel(const int32_t *__restrict__ score, const int32_t *__restrict__ loc,
                                                             int64_t n_seq, int32_t lo, int64_t n_bins,
                                                             unsigned long long *__restrict__ acc) {
    __shared__ uint32_t bins[LDS ? RS_LDS_BINS + 1 : 1];   // a block sees n_seq / gridDim reads: 2^32 of them would be 32 GiB of scores and locs
    if (LDS) {
        for (int b = threadIdx.x; b <= n_bins; b += blockDim.x) bins[b] = 0;
        __syncthreads();
    }
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n_seq; r += (int64_t)gridDim.x * blockDim.x) {
        if (loc[r] < 0) continue;
        int64_t b = (int64_t)score[r] - lo;
        if (b < 0 || b >= n_bins) b = n_bins;
        if (LDS) atomicAdd(&bins[b], 1u); else atomicAdd(&acc[b], 1ull);
    }
    if (LDS) {
        __syncthreads();
        for (int b = threadIdx.x; b <= n_bins; b += blockDim.x) {
            const uint32_t c = bins[b];
            if (c) atomicAdd(&acc[b], (unsigned long long)c);
        }
    }
}

}  // namespace

extern "C" {

int kmap_readscore_packed_dev(const uint32_t *codes_dev, const uint16_t *inval_dev, int64_t n, const int64_t *borders_dev,
                              int64_t n_seq, int width, const int32_t *weights, int revcom, int32_t *score_dev, int32_t *loc_dev,
                              uint8_t *strand_dev, int64_t *n_scored, void *stream) {
    PwmPlan pl;
    KMAP_TRY(pwm_plan(pl, "readscore", n, n_seq, width, weights));
    if (n_scored) *n_scored = 0;
    if (n_seq == 0) return KMAP_OK;
    KMAP_REQUIRE(score_dev && loc_dev && strand_dev, "readscore: null result pointer");
    hipStream_t st = as_stream(stream);
    unsigned long long *acc = nullptr;     // the number of scorable reads (+ a spare word), then one key per read
    KMAP_TRY(kmap_scratch((void **)&acc, ((size_t)n_seq + 2) * 8, st, KMAP_SLOT_A));
    unsigned long long *key = acc + 2;
    KMAP_CHECK_HIP(hipMemsetAsync(acc, 0, ((size_t)n_seq + 2) * 8, st));
    if (n > 0) {
        KMAP_REQUIRE(codes_dev && inval_dev && borders_dev, "readscore: null pointer");
        with_bool(revcom, [&](auto rc) {
            readscore_kernel<decltype(rc)::value><<<pl.grid, PW_TPB, 0, st>>>(codes_dev, inval_dev, pl.n_data, pl.n_tiles, pl.wt, width, pl.nch,
                                                                              borders_dev, n_seq, key);
        });
        KMAP_CHECK_HIP(hipGetLastError());
    }
    readscore_unpack_kernel<<<grid_for(n_seq, 256), 256, 0, st>>>(key, n_seq, score_dev, loc_dev, strand_dev, acc);
    KMAP_CHECK_HIP(hipGetLastError());
    unsigned long long scored = 0;
    KMAP_CHECK_HIP(hipMemcpyAsync(&scored, acc, 8, hipMemcpyDeviceToHost, st));
    KMAP_CHECK_HIP(hipStreamSynchronize(st));
    if (n_scored) *n_scored = (int64_t)scored;
    return KMAP_OK;
}

int kmap_readscore_hist_dev(const int32_t *score_dev, const int32_t *loc_dev, int64_t n_seq, int32_t lo, int64_t n_bins,
                            uint64_t *hist_host, int64_t *n_outside, void *stream) {
    KMAP_REQUIRE(n_seq >= 0 && n_bins >= 0, "readscore_hist: negative size");
    if (n_bins > RS_MAX_BINS) {
        kmap_set_error("readscore_hist: %lld bins, more than 2^22", (long long)n_bins);
        return KMAP_E_UNSUP;
    }
    KMAP_REQUIRE(hist_host || n_bins == 0, "readscore_hist: null histogram");
    if (n_outside) *n_outside = 0;
    if (n_bins) memset(hist_host, 0, (size_t)n_bins * 8);
    if (n_seq == 0) return KMAP_OK;
    KMAP_REQUIRE(score_dev && loc_dev, "readscore_hist: null pointer");
    hipStream_t st = as_stream(stream);
    unsigned long long *acc = nullptr;
    const size_t words = (size_t)n_bins + 1;
    KMAP_TRY(kmap_scratch((void **)&acc, words * 8, st, KMAP_SLOT_B));
    KMAP_CHECK_HIP(hipMemsetAsync(acc, 0, words * 8, st));
    const unsigned grid = (unsigned)std::min<int64_t>(grid_for(n_seq, 256), RS_HIST_BLOCKS);
    if (n_bins <= RS_LDS_BINS)
        readscore_hist_kernel<true><<<grid, 256, 0, st>>>(score_dev, loc_dev, n_seq, lo, n_bins, acc);
    else
        readscore_hist_kernel<false><<<grid, 256, 0, st>>>(score_dev, loc_dev, n_seq, lo, n_bins, acc);
    KMAP_CHECK_HIP(hipGetLastError());
    unsigned long long outside = 0;
    if (n_bins) KMAP_CHECK_HIP(hipMemcpyAsync(hist_host, acc, (size_t)n_bins * 8, hipMemcpyDeviceToHost, st));
    KMAP_CHECK_HIP(hipMemcpyAsync(&outside, acc + n_bins, 8, hipMemcpyDeviceToHost, st));
    KMAP_CHECK_HIP(hipStreamSynchronize(st));
    if (n_outside) *n_outside = (int64_t)outside;
    return KMAP_OK;
}

}  // extern "C"
