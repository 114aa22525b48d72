// pwm_spacing.hip -- at which distance and in which orientation the best site of every matrix of a library lies from the primary
// matrix's site (motif_spacing).  pwm_sites.hip's batched dense pass with two changes -- the key carries the
// strand, and a window that overlaps the read's primary site (or lies in a read without one) is never a candidate -- and behind it a
// reduction of the keys to two small integer histograms per matrix, so that nothing per read leaves the device.
//
//   * spacing_primary_kernel: ploc[r] = the primary's best loc of read r when that window scores prim_threshold or more, else -1,
//     from a ReadScores' score and loc arrays; the number of primary reads.
//   * spacing_multi_kernel<RC>: sites_multi_kernel's pass -- persistent blocks over wave tiles, the chunk tables of the batch's
//     matrices behind one another in LDS, load_grp and tile_read_starts once per tile, per matrix the lane's 16 windows reduced to
//     segments per read, a segmented maximum across the lanes and ONE atomicMax per (wave, read, matrix) -- with pwm_readscore.hip's
//     key
//         (score with the sign bit flipped) << 32 | (0x7FFFFFFF - loc) << 1 | minus
//     (zero = none), so forward and reverse scores are kept apart until minus = rc > fwd is known.  Every lane carries pl, the ploc
//     of the read its current window belongs to: loaded once per tile for the read that reaches the group from the left, again after
//     every step_read.  With pl >= 0 a window at read-local loc is kept iff (uint32)(loc - pl + w - 1) >= (uint32)(wP + w - 1): it
//     ends at or before the primary window's first base or begins at or behind its last.  The new state (pl, the strand) lives in
//     registers: the LDS of three blocks per CU leaves no room (DESIGN.md section 19 has the resource table).
//   * spacing_hist_kernel: blockIdx.y = the matrix, blockIdx.x strides over its keys.  A non-zero key gives loc and strand of the
//     secondary site; ploc[r], prim_strand[r] and the read's two borders give p, sP and L; then the gap g, the quadrant
//     2 downstream + opposite and the two rooms (u, d) go into one flat uint64 array per matrix: n_pair, n_far, S[4][G + 1],
//     R[G + 2][G + 2], with global integer atomics (pair reads are a small share of the reads).  Integer counts: exact and order-free.
#include <numeric>
#include <vector>

#include "common.h"
#include "pwm_internal.h"

namespace {

constexpr int SP_MAX_MAT = 8;            // a batch is pwm_library.hip's: at most this many matrices (device_seq.py: LIBRARY_BATCH)
constexpr int SP_MAX_CHUNKS = 24;        // and this many chunk tables (LIBRARY_BATCH_CHUNKS)
constexpr int SP_MAX_GAP = 511;          // device_seq.py: SPACING_MAX_GAP; R alone is then 2 MB per matrix
constexpr int SP_HIST_TPB = 1024;
constexpr int SP_HIST_BLOCKS = 512;      // blocks of one histogram launch, over all matrices of the batch
constexpr int32_t SP_MAX_WEIGHT = (int32_t)((1ll << 31) / 31);      // pwm._check_weights: |w| below this
constexpr int SP_HEAD = 2;               // words in front of a matrix's histograms: n_pair, n_far

template <bool RC> struct SpacingEntry { using T = int; };          // forward sum of a chunk
template <> struct SpacingEntry<true> { using T = int2; };          // (forward, reverse complement)

struct SpacingBatch {
    int n_mat;
    int src[SP_MAX_MAT];        // the matrix's row in the weights array
    int width[SP_MAX_MAT];
    int chunk0[SP_MAX_MAT];     // its first chunk table
    int32_t thr[SP_MAX_MAT];    // windows below it are dropped
};

// the window's score and strand: with RC the larger of the two strands' sums, a tie is '+'
template <bool RC>
__device__ __forceinline__ int spacing_score(const typename SpacingEntry<RC>::T *tab, uint64_t v, int nch, bool &minus) {
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

__device__ __forceinline__ uint64_t pack_pair_key(int score, uint32_t loc, bool minus) {
    return ((uint64_t)((uint32_t)score ^ 0x80000000u) << 32) | ((uint64_t)(0x7FFFFFFFu - loc) << 1) | (minus ? 1u : 0u);
}

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

// Three blocks per CU as sites_multi_kernel (the LDS admits no more): DESIGN.md section 19 has the register table.
template <bool RC>
__global__ __launch_bounds__(PW_TPB, 3) void spacing_multi_kernel(const uint32_t *__restrict__ codes, const uint16_t *__restrict__ inval,
                                                                  int64_t n_data, int64_t n_tiles, const int32_t *__restrict__ weights,
                                                                  SpacingBatch bt, const int64_t *__restrict__ borders, int64_t n_seq,
                                                                  const int32_t *__restrict__ ploc, int prim_width,
                                                                  unsigned long long *__restrict__ key) {
    using Entry = typename SpacingEntry<RC>::T;
    __shared__ Entry tab[SP_MAX_CHUNKS * 256];
    __shared__ int32_t wl[128];
    __shared__ int s_width[SP_MAX_MAT], s_chunk0[SP_MAX_MAT], s_thr[SP_MAX_MAT];
    __shared__ uint32_t start_bits[PW_WAVES][KMAP_WAVE];
    __shared__ uint32_t start_cnt[PW_WAVES][KMAP_WAVE];
    // build_table's entries, matrix after matrix through the one staging row (columns >= width are 0 in the weights array)
#pragma unroll
    for (int m = 0; m < SP_MAX_MAT; ++m) {
        if (m < bt.n_mat) {                // uniform
            const int width = bt.width[m], nch = (width + 3) >> 2;
            if (threadIdx.x < 128) wl[threadIdx.x] = weights[(int64_t)bt.src[m] * 128 + threadIdx.x];
            if (threadIdx.x == 0) {
                s_width[m] = width;
                s_chunk0[m] = bt.chunk0[m];
                s_thr[m] = bt.thr[m];
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
        const uint32_t loc_first = (uint32_t)(g * 16 - (r0 >= 0 ? borders[2 * r0] : 0));   // loc of the group's first position (an int32 in a read)
        const int32_t pl_first = r0 >= 0 ? ploc[r0] : -1;          // the primary site of the read that reaches the group from the left
        for (int m = 0; m < n_mat; ++m) {
            const int width = __builtin_amdgcn_readfirstlane(s_width[m]), nch = (width + 3) >> 2;
            const int thr = __builtin_amdgcn_readfirstlane(s_thr[m]);
            const Entry *tb = tab + __builtin_amdgcn_readfirstlane(s_chunk0[m]) * 256;
            const uint64_t wmask = (1ull << width) - 1ull;
            const uint32_t span = (uint32_t)(prim_width + width - 1);      // loc - pl + width - 1 of an overlapping window lies below it
            unsigned long long *km = key + (int64_t)m * n_seq;
            uint64_t cur = 0, head = 0;                // the running segment; the one that reached the lane from the left
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
                        atomicMax(&km[r], (unsigned long long)cur);     // a read that began and ends in this group
                    }
                    cur = 0;
                    step_read(borders, n_seq, g * 16 + i, shared_starts, r);
                    loc0 = (uint32_t)-i;
                    pl = ploc[r];                      // a read start was marked, so n_seq >= 1 and 0 <= r < n_seq
                }
                bool minus;
                const int s = spacing_score<RC>(tb, win_bits(w, i), nch, minus);
                const uint32_t loc = loc0 + i;
                if (s >= thr && pl >= 0 && loc - (uint32_t)pl + (uint32_t)(width - 1) >= span && win_valid(w, i, width, wmask)) {
                    const uint64_t k = pack_pair_key(s, loc, minus);
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
            uint64_t left = __shfl_up((unsigned long long)seg, 1);     // what the lanes to the left hold of this lane's first read
            if (lane == 0) left = 0;
            if (split && r0 >= 0) {
                const uint64_t best = head > left ? head : left;
                if (best) atomicMax(&km[r0], (unsigned long long)best);
            }
            if (lane == KMAP_WAVE - 1 && seg && r >= 0) atomicMax(&km[r], (unsigned long long)seg);   // the read that leaves the tile
        }
    }
}

struct SpacingHist {
    int width[SP_MAX_MAT];
    int64_t off[SP_MAX_MAT];    // acc[off] = n_pair, acc[off + 1] = n_far, then S[4][G + 1], then R[G + 2][G + 2]
};

__global__ __launch_bounds__(SP_HIST_TPB) void spacing_hist_kernel(const unsigned long long *__restrict__ key, int64_t n_seq,
                                                                   const int64_t *__restrict__ borders, const int32_t *__restrict__ ploc,
                                                                   const uint8_t *__restrict__ prim_strand, int prim_width, SpacingHist h,
                                                                   int max_gap, unsigned long long *__restrict__ acc) {
    const int m = blockIdx.y;
    int width = 0;
    int64_t off = 0;
#pragma unroll
    for (int j = 0; j < SP_MAX_MAT; ++j)
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
    for (int m = 0; m < n_mat; ++m) {
        KMAP_REQUIRE(widths[m] >= 4 && widths[m] <= 31, "readscore_spacing_library: width=%d of matrix %d outside 4..31", widths[m], m);
        for (int e = 0; e < 128; ++e) {
            const int32_t v = weights[(size_t)m * 128 + e];
            KMAP_REQUIRE(v > -SP_MAX_WEIGHT && v < SP_MAX_WEIGHT, "readscore_spacing_library: a weight of matrix %d is 2^31 / 31 or more: a window's score must fit int32", m);
            KMAP_REQUIRE((e & 31) < widths[m] || v == 0, "readscore_spacing_library: matrix %d has a weight behind its width %d", m, widths[m]);
        }
    }
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

    const int64_t n_data = (n + 15) >> 4, n_tiles = (n_data + PW_TILE_GROUPS - 1) / PW_TILE_GROUPS;   // groups of 16 positions; wave tiles
    // persistent blocks: as many as are resident at once (registers and LDS decide; the tables are built once per block)
    int dev = 0, cus = 0, per_cu = 0;
    KMAP_CHECK_HIP(hipGetDevice(&dev));
    KMAP_CHECK_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    if (revcom) KMAP_CHECK_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, spacing_multi_kernel<true>, PW_TPB, 0));
    else KMAP_CHECK_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, spacing_multi_kernel<false>, PW_TPB, 0));
    KMAP_REQUIRE(cus > 0 && per_cu > 0, "readscore_spacing_library: no block of the scoring kernel fits a compute unit");
    const unsigned grid = (unsigned)std::min<int64_t>((n_tiles + PW_WAVES - 1) / PW_WAVES, (int64_t)cus * per_cu);

    // by width (ties: the caller's order), so that a batch holds matrices of similar chunk counts
    std::vector<int> order(n_mat);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return widths[a] < widths[b]; });

    const int per_batch = std::min(n_mat, SP_MAX_MAT);
    int32_t *weights_dev = nullptr;
    KMAP_TRY(kmap_scratch((void **)&weights_dev, (size_t)n_mat * 512, st, KMAP_SLOT_C));
    KMAP_CHECK_HIP(hipMemcpyAsync(weights_dev, weights, (size_t)n_mat * 512, hipMemcpyHostToDevice, st));
    unsigned long long *key = nullptr, *acc = nullptr;
    KMAP_TRY(kmap_scratch((void **)&key, (size_t)per_batch * (size_t)n_seq * 8, st, KMAP_SLOT_A));
    KMAP_TRY(kmap_scratch((void **)&acc, (size_t)per_batch * words * 8, st, KMAP_SLOT_B));

    std::vector<unsigned long long> back;
    for (int first = 0; first < n_mat;) {
        SpacingBatch bt = {};
        SpacingHist hs = {};
        int chunks = 0;
        while (first + bt.n_mat < n_mat && bt.n_mat < SP_MAX_MAT) {
            const int m = order[first + bt.n_mat], nch = (widths[m] + 3) / 4, j = bt.n_mat;
            if (chunks + nch > SP_MAX_CHUNKS) break;
            bt.src[j] = m;
            bt.width[j] = hs.width[j] = widths[m];
            bt.chunk0[j] = chunks;
            bt.thr[j] = thresholds[m];
            chunks += nch;
            hs.off[j] = (int64_t)((size_t)j * words);
            ++bt.n_mat;
        }
        const size_t batch_words = (size_t)bt.n_mat * words;       // n_mat >= 1: one matrix has 8 chunks at the most
        KMAP_CHECK_HIP(hipMemsetAsync(acc, 0, batch_words * 8, st));
        KMAP_CHECK_HIP(hipMemsetAsync(key, 0, (size_t)bt.n_mat * (size_t)n_seq * 8, st));
        with_bool(revcom, [&](auto rc) {
            spacing_multi_kernel<decltype(rc)::value><<<grid, PW_TPB, 0, st>>>(codes_dev, inval_dev, n_data, n_tiles, weights_dev, bt,
                                                                               borders_dev, n_seq, ploc, prim_width, key);
        });
        KMAP_CHECK_HIP(hipGetLastError());
        const unsigned gx = (unsigned)std::max<int64_t>(1, std::min<int64_t>(grid_for(n_seq, SP_HIST_TPB), SP_HIST_BLOCKS / bt.n_mat));
        spacing_hist_kernel<<<dim3(gx, (unsigned)bt.n_mat), SP_HIST_TPB, 0, st>>>(key, n_seq, borders_dev, ploc, prim_strand_dev, prim_width,
                                                                                  hs, max_gap, acc);
        KMAP_CHECK_HIP(hipGetLastError());
        back.resize(batch_words);
        if (first == 0) KMAP_CHECK_HIP(hipMemcpyAsync(&primary, prim, 8, hipMemcpyDeviceToHost, st));
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
        first += bt.n_mat;
    }
    *n_primary = (int64_t)primary;
    return KMAP_OK;
}

}  // extern "C"
