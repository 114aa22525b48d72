// pwm_library.hip -- the best score of every read under every matrix of a library, and the histograms of those scores
// (rank_motif_library).  What pwm_readscore.hip does for one matrix -- load the packed reads, find the reads of
// the tile, reduce the windows of every read to one maximum -- is done here for a BATCH of matrices in one pass over the reads: the
// loads, the border search and the read segmentation do not depend on the matrix and are done once per tile.  Only the score is kept
// (no loc, no strand, no per-read arrays leave the device), so a key is 32 bits and the histogram reads the keys directly.
//
//   * readscore_multi_kernel<RC>: persistent blocks over wave tiles of 64 groups x 16 positions like readscore_kernel.  The chunk
//     tables of the batch's matrices lie behind one another in LDS (2 KB per chunk with RC, 1 KB without: the forward sums alone);
//     every matrix has its own width, hence its own chunk count, window mask and valid test.  Per tile: load_grp and
//     tile_read_starts ONCE, then per matrix the 16 windows of the lane, reduced to segments per read exactly as readscore_kernel
//     does: a read that begins and ends inside the lane goes to its key at once, head and tail are combined by a segmented max scan
//     across the lanes, ONE atomicMax per (wave, read, matrix).  key[m][read] = score with the sign bit flipped; 0 = "no valid
//     window": the entry point refuses weights of 2^31 / 31 or more in magnitude (pwm._check_weights' bound), so |score| <= 31
//     (2^31 / 31 - 1) < 2^31 - 1, the score is never INT32_MIN and a real key never 0.  A maximum is order-free: deterministic.
//   * library_hist_kernel: blockIdx.y = the matrix, blockIdx.x strides over its keys.  uint64 bins of all matrices of the batch in
//     one flat array (per matrix: outside, unscorable, then its n_bins bins).  A matrix whose range fits is counted in block-private
//     uint32 bins in dynamic LDS and flushed with one global integer atomic per non-zero bin and block; wider ranges go to global
//     integer atomics directly.  Integer counts either way: exact and order-free.
//   * LDS budget: static LDS, 24 chunk tables and 8 matrices per batch -- 48 KB of tables with RC, 50.5 KB
//     in all, so three blocks share a CU's 160 KB.  Unmeasured against the alternative (dynamic LDS, up to ~70 chunks, one block
//     per CU).
//   * pwm_library_key_batches (pwm_internal.h): the batching and the scoring launch as a host function that hands every batch's
//     keys to a callback; the histogram entry point below and pwm_presence.hip's presence planes are its two callers.
#include <numeric>
#include <vector>

#include "common.h"
#include "pwm_internal.h"

namespace {

constexpr int LB_MAX_MAT = 8;            // matrices per batch (kmap_amd/device_seq.py: LIBRARY_BATCH)
constexpr int LB_MAX_CHUNKS = 24;        // chunk tables per batch (LIBRARY_BATCH_CHUNKS): 8 matrices of w <= 12, 3 of w >= 29
constexpr int LB_HIST_TPB = 1024;
constexpr int LB_HIST_BLOCKS = 512;      // blocks of one histogram launch, over all matrices of the batch
// Ranges up to this many bins are privatised per block: 128 KB of uint32 counters in dynamic LDS, the size counts_fine.hip's
// fine_hist_kernel already runs with; one such block fills a CU's LDS (160 KB), a larger array would leave no room for a second
// kernel's blocks beside it.  A 31-column matrix at pseudocount 1 spans about 20 000 scores, so libraries fit as a rule.  A block
// counts at most n_seq / 64 reads (the launch has 64 blocks or more per matrix once n_seq >= 65 536): a uint32 bin would need
// 2^38 reads, a terabyte of keys, to overflow.
constexpr int64_t LB_HIST_LDS_BINS = 32768;
constexpr int64_t LB_MAX_BINS = 1ll << 22;
constexpr int32_t LB_MAX_WEIGHT = (int32_t)((1ll << 31) / 31);      // pwm._check_weights: |w| below this

template <bool RC> struct LibEntry { using T = int; };              // forward sum of a chunk
template <> struct LibEntry<true> { using T = int2; };              // (forward, reverse complement)

struct LibBatch {
    int n_mat;
    int src[LB_MAX_MAT];        // the matrix's row in the weights array
    int width[LB_MAX_MAT];
    int chunk0[LB_MAX_MAT];     // its first chunk table
};

struct LibHist {
    int n_mat;
    int lds[LB_MAX_MAT];        // the range fits the block-private bins
    int32_t lo[LB_MAX_MAT];
    int64_t n_bins[LB_MAX_MAT];
    int64_t off[LB_MAX_MAT];    // acc[off] = outside, acc[off + 1] = unscorable, acc[off + 2 ..] = the bins
};

template <bool RC>
__device__ __forceinline__ int lib_score(const typename LibEntry<RC>::T *tab, uint64_t v, int nch) {
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
    return RC && rc > fwd ? rc : fwd;
}

// Three waves per SIMD (168 VGPRs, a dozen spilled) -- the three blocks per CU the LDS admits -- instead of the two the compiler's own
// allocation (181 VGPRs) leaves: measured 50.6 ms against 67.4 ms for the 16 matrices of tools/bench_library.py.
template <bool RC>
__global__ __launch_bounds__(PW_TPB, 3) void readscore_multi_kernel(const uint32_t *__restrict__ codes, const uint16_t *__restrict__ inval,
                                                                 int64_t n_data, int64_t n_tiles, const int32_t *__restrict__ weights,
                                                                 LibBatch bt, const int64_t *__restrict__ borders, int64_t n_seq,
                                                                 unsigned int *__restrict__ key) {
    using Entry = typename LibEntry<RC>::T;
    __shared__ Entry tab[LB_MAX_CHUNKS * 256];
    __shared__ int32_t wl[128];
    __shared__ int s_width[LB_MAX_MAT], s_chunk0[LB_MAX_MAT];
    __shared__ uint32_t start_bits[PW_WAVES][KMAP_WAVE];
    __shared__ uint32_t start_cnt[PW_WAVES][KMAP_WAVE];
    // build_table's entries, matrix after matrix through the one staging row (columns >= width are 0 in the weights array)
#pragma unroll
    for (int m = 0; m < LB_MAX_MAT; ++m) {
        if (m < bt.n_mat) {                // uniform
            const int width = bt.width[m], nch = (width + 3) >> 2;
            if (threadIdx.x < 128) wl[threadIdx.x] = weights[(int64_t)bt.src[m] * 128 + threadIdx.x];
            if (threadIdx.x == 0) {
                s_width[m] = width;
                s_chunk0[m] = bt.chunk0[m];
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
        for (int m = 0; m < n_mat; ++m) {
            const int width = __builtin_amdgcn_readfirstlane(s_width[m]), nch = (width + 3) >> 2;
            const Entry *tb = tab + __builtin_amdgcn_readfirstlane(s_chunk0[m]) * 256;
            const uint64_t wmask = (1ull << width) - 1ull;
            unsigned int *km = key + (int64_t)m * n_seq;
            uint32_t cur = 0, head = 0;                // the running segment; the one that reached the lane from the left
            int64_t r = r0;
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
                }
                const int s = lib_score<RC>(tb, win_bits(w, i), nch);
                if (win_valid(w, i, width, wmask) && r >= 0) {
                    const uint32_t k = (uint32_t)s ^ 0x80000000u;
                    cur = k > cur ? k : cur;
                }
            }
            // lanes of one read: inclusive segmented maximum of the tails, a lane with a read start opens a segment
            uint32_t seg = cur;
            int open = split ? 1 : 0;
            for (int o = 1; o < KMAP_WAVE; o <<= 1) {
                const uint32_t up = __shfl_up(seg, o);
                const int up_open = __shfl_up(open, o);
                if (lane >= o && !open) {
                    seg = up > seg ? up : seg;
                    open = up_open;
                }
            }
            uint32_t left = __shfl_up(seg, 1);         // what the lanes to the left hold of this lane's first read
            if (lane == 0) left = 0;
            if (split && r0 >= 0) {
                const uint32_t best = head > left ? head : left;
                if (best) atomicMax(&km[r0], best);
            }
            if (lane == KMAP_WAVE - 1 && seg && r >= 0) atomicMax(&km[r], seg);     // the read that leaves the tile
        }
    }
}

__global__ __launch_bounds__(LB_HIST_TPB) void library_hist_kernel(const unsigned int *__restrict__ key, int64_t n_seq, LibHist h,
                                                                   unsigned long long *__restrict__ acc) {
    extern __shared__ uint32_t lib_bins[];
    const int m = blockIdx.y;
    int lds = 0;
    int32_t lo = 0;
    int64_t n_bins = 0, off = 0;
#pragma unroll
    for (int j = 0; j < LB_MAX_MAT; ++j)
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

// ---- the batch pass as other files reach it (pwm_internal.h) -----------------------------------------------------------------------

int pwm_library_check(const char *who, int n_mat, const int32_t *widths, const int32_t *weights) {
    KMAP_REQUIRE(widths && weights, "%s: null pointer", who);
    for (int m = 0; m < n_mat; ++m) {
        KMAP_REQUIRE(widths[m] >= 4 && widths[m] <= 31, "%s: width=%d of matrix %d outside 4..31", who, widths[m], m);
        for (int e = 0; e < 128; ++e) {
            const int32_t v = weights[(size_t)m * 128 + e];
            KMAP_REQUIRE(v > -LB_MAX_WEIGHT && v < LB_MAX_WEIGHT, "%s: a weight of matrix %d is 2^31 / 31 or more: a window's score must fit int32", who, m);
            KMAP_REQUIRE((e & 31) < widths[m] || v == 0, "%s: matrix %d has a weight behind its width %d", who, m, widths[m]);
        }
    }
    return KMAP_OK;
}

int pwm_library_key_batches(const char *who, const uint32_t *codes_dev, const uint16_t *inval_dev, int64_t n, const int64_t *borders_dev,
                            int64_t n_seq, int n_mat, const int32_t *widths, const int32_t *weights, int revcom, hipStream_t st,
                            const std::function<int(const LibKeys &)> &on_batch) {
    const int64_t n_data = (n + 15) >> 4, n_tiles = (n_data + PW_TILE_GROUPS - 1) / PW_TILE_GROUPS;   // groups of 16 positions; wave tiles
    // persistent blocks: as many as are resident at once (registers and LDS decide; the tables are built once per block)
    int dev = 0, cus = 0, per_cu = 0;
    KMAP_CHECK_HIP(hipGetDevice(&dev));
    KMAP_CHECK_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    if (revcom) KMAP_CHECK_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, readscore_multi_kernel<true>, PW_TPB, 0));
    else KMAP_CHECK_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, readscore_multi_kernel<false>, PW_TPB, 0));
    KMAP_REQUIRE(cus > 0 && per_cu > 0, "%s: no block of the scoring kernel fits a compute unit", who);
    const unsigned grid = (unsigned)std::min<int64_t>((n_tiles + PW_WAVES - 1) / PW_WAVES, (int64_t)cus * per_cu);

    // by width (ties: the caller's order), so that a batch holds matrices of similar chunk counts
    std::vector<int> order(n_mat);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return widths[a] < widths[b]; });

    int32_t *weights_dev = nullptr;
    KMAP_TRY(kmap_scratch((void **)&weights_dev, (size_t)n_mat * 512, st, KMAP_SLOT_C));
    KMAP_CHECK_HIP(hipMemcpyAsync(weights_dev, weights, (size_t)n_mat * 512, hipMemcpyHostToDevice, st));
    unsigned int *key = nullptr;
    KMAP_TRY(kmap_scratch((void **)&key, (size_t)std::min(n_mat, LB_MAX_MAT) * (size_t)n_seq * 4, st, KMAP_SLOT_A));

    for (int first = 0; first < n_mat;) {
        LibBatch bt = {};
        int chunks = 0;
        while (first + bt.n_mat < n_mat && bt.n_mat < LB_MAX_MAT) {
            const int m = order[first + bt.n_mat], nch = (widths[m] + 3) / 4, j = bt.n_mat;
            if (chunks + nch > LB_MAX_CHUNKS) break;
            bt.src[j] = m;
            bt.width[j] = widths[m];
            bt.chunk0[j] = chunks;
            chunks += nch;
            ++bt.n_mat;
        }                                              // n_mat >= 1: one matrix has 8 chunks at the most
        KMAP_CHECK_HIP(hipMemsetAsync(key, 0, (size_t)bt.n_mat * (size_t)n_seq * 4, st));
        with_bool(revcom, [&](auto rc) {
            readscore_multi_kernel<decltype(rc)::value><<<grid, PW_TPB, 0, st>>>(codes_dev, inval_dev, n_data, n_tiles, weights_dev,
                                                                                 bt, borders_dev, n_seq, key);
        });
        KMAP_CHECK_HIP(hipGetLastError());
        const LibKeys keys = {bt.n_mat, bt.src, key};
        KMAP_TRY(on_batch(keys));
        first += bt.n_mat;
    }
    return KMAP_OK;
}

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
    return pwm_library_key_batches("readscore_library", codes_dev, inval_dev, n, borders_dev, n_seq, n_mat, widths, weights, revcom, st,
                                   [&](const LibKeys &keys) -> int {
        LibHist hs = {};
        int64_t words = 0, lds_bins = 1;
        for (int j = 0; j < keys.n_mat; ++j) {
            const int m = keys.src[j];
            hs.lds[j] = n_bins[m] <= LB_HIST_LDS_BINS;
            hs.lo[j] = lo[m];
            hs.n_bins[j] = n_bins[m];
            hs.off[j] = words;
            words += 2 + n_bins[m];
            if (hs.lds[j]) lds_bins = std::max(lds_bins, n_bins[m]);
        }
        hs.n_mat = keys.n_mat;
        unsigned long long *acc = nullptr;
        KMAP_TRY(kmap_scratch((void **)&acc, (size_t)words * 8, st, KMAP_SLOT_B));
        KMAP_CHECK_HIP(hipMemsetAsync(acc, 0, (size_t)words * 8, st));
        const unsigned gx = (unsigned)std::max<int64_t>(1, std::min<int64_t>(grid_for(n_seq, LB_HIST_TPB), LB_HIST_BLOCKS / keys.n_mat));
        library_hist_kernel<<<dim3(gx, (unsigned)keys.n_mat), LB_HIST_TPB, (size_t)lds_bins * 4, st>>>(keys.key, n_seq, hs, acc);
        KMAP_CHECK_HIP(hipGetLastError());
        back.resize((size_t)words);
        KMAP_CHECK_HIP(hipMemcpyAsync(back.data(), acc, (size_t)words * 8, hipMemcpyDeviceToHost, st));
        KMAP_CHECK_HIP(hipStreamSynchronize(st));      // once per batch
        for (int j = 0; j < keys.n_mat; ++j) {
            const int m = keys.src[j];
            const unsigned long long *a = back.data() + hs.off[j];
            n_outside[m] = (int64_t)a[0];
            n_scored[m] = n_seq - (int64_t)a[1];
            if (n_bins[m]) memcpy(hist_host + host_off[m], a + 2, (size_t)n_bins[m] * 8);
        }
        return KMAP_OK;
    });
}

}  // extern "C"
