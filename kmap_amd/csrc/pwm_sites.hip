// pwm_sites.hip -- where in the reads the best site of every matrix of a library lies (motif_centrality).
// pwm_library.hip's batched dense pass with section 14's (score, loc) key instead of the score alone, and behind it a reduction of
// the keys to two small histograms per matrix, so that nothing per read leaves the device.
//
//   * sites_multi_kernel<RC>: readscore_multi_kernel's pass -- persistent blocks over wave tiles, the chunk tables of the batch's
//     matrices behind one another in LDS, load_grp and tile_read_starts once per tile, then per matrix the lane's 16 windows reduced
//     to segments per read, a segmented maximum across the lanes and ONE atomicMax per (wave, read, matrix) -- with the key
//         (score with the sign bit flipped) << 32 | (0x7FFFFFFF - loc)
//     so the largest score wins and on a tie the smallest loc.  Zero = "none" (a real key would need the score INT32_MIN, which the
//     weight bound of the entry point excludes).  Only site reads -- best score >= the matrix's threshold -- are wanted, and the best
//     window of a site read is itself at or above the threshold: a window below it never becomes a key.  At p = 10^-4 that removes
//     almost every atomic.  A kernel of its own and not a template argument of readscore_multi_kernel: that one sits at a tuned
//     register count (pwm_library.hip) which a 64-bit key would move.
//   * sites_hist_kernel: blockIdx.y = the matrix, blockIdx.x strides over its keys.  A non-zero key gives loc; the read's two
//     borders give its length L; the doubled centre offset d = 2 loc + width - L lies in [-(L - width), L - width].  Per matrix, in one
//     flat uint64 array: sites, too_long, D[2 max_len + 1] (bin d + max_len), Hlen[max_len + 1].  A site read longer than max_len
//     is in neither histogram but in too_long.  Block-private uint32 bins in dynamic LDS when both histograms fit 32 768 words,
//     flushed with one global integer atomic per non-zero bin and block; global integer atomics otherwise.  Integer counts either
//     way: exact and order-free.
//   * sites_count_kernel<RC> (discover_pwms): the same keys reduced to the count matrix of the site reads' best
//     windows instead -- one refinement step (pwm_refine.hip's select_best) for a batch of matrices.  The two entry points share the
//     batch loop (sites_key_batches; the matrix checks are pwm_library.hip's) and differ in what they enqueue behind the scoring kernel.
#include <numeric>
#include <vector>

#include "common.h"
#include "pwm_internal.h"

namespace {

constexpr int ST_MAX_MAT = 8;            // a batch is pwm_library.hip's: at most this many matrices (device_seq.py: LIBRARY_BATCH)
constexpr int ST_MAX_CHUNKS = 24;        // and this many chunk tables (LIBRARY_BATCH_CHUNKS)
constexpr int ST_HIST_TPB = 1024;
constexpr int ST_HIST_BLOCKS = 512;      // blocks of one histogram launch, over all matrices of the batch
constexpr int64_t ST_HIST_LDS_WORDS = 32768;     // 128 KB of block-private uint32 bins (pwm_library.hip: LB_HIST_LDS_BINS)
constexpr int64_t ST_MAX_LEN = 1ll << 20;
constexpr int ST_HEAD = 2;               // words in front of a matrix's histograms: sites, too_long

template <bool RC> struct SiteEntry { using T = int; };             // forward sum of a chunk
template <> struct SiteEntry<true> { using T = int2; };             // (forward, reverse complement)

struct SiteBatch {
    int n_mat;
    int src[ST_MAX_MAT];        // the matrix's row in the weights array
    int width[ST_MAX_MAT];
    int chunk0[ST_MAX_MAT];     // its first chunk table
    int32_t thr[ST_MAX_MAT];    // windows below it are dropped
};

template <bool RC>
__device__ __forceinline__ int site_score(const typename SiteEntry<RC>::T *tab, uint64_t v, int nch) {
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

__device__ __forceinline__ uint64_t pack_site_key(int score, uint32_t loc) {
    return ((uint64_t)((uint32_t)score ^ 0x80000000u) << 32) | (uint64_t)(0x7FFFFFFFu - loc);
}

// Three blocks per CU as readscore_multi_kernel (the LDS admits no more): DESIGN.md section 18 has the register table.
template <bool RC>
__global__ __launch_bounds__(PW_TPB, 3) void sites_multi_kernel(const uint32_t *__restrict__ codes, const uint16_t *__restrict__ inval,
                                                                int64_t n_data, int64_t n_tiles, const int32_t *__restrict__ weights,
                                                                SiteBatch bt, const int64_t *__restrict__ borders, int64_t n_seq,
                                                                unsigned long long *__restrict__ key) {
    using Entry = typename SiteEntry<RC>::T;
    __shared__ Entry tab[ST_MAX_CHUNKS * 256];
    __shared__ int32_t wl[128];
    __shared__ int s_width[ST_MAX_MAT], s_chunk0[ST_MAX_MAT], s_thr[ST_MAX_MAT];
    __shared__ uint32_t start_bits[PW_WAVES][KMAP_WAVE];
    __shared__ uint32_t start_cnt[PW_WAVES][KMAP_WAVE];
    // build_table's entries, matrix after matrix through the one staging row (columns >= width are 0 in the weights array)
#pragma unroll
    for (int m = 0; m < ST_MAX_MAT; ++m) {
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
        for (int m = 0; m < n_mat; ++m) {
            const int width = __builtin_amdgcn_readfirstlane(s_width[m]), nch = (width + 3) >> 2;
            const int thr = __builtin_amdgcn_readfirstlane(s_thr[m]);
            const Entry *tb = tab + __builtin_amdgcn_readfirstlane(s_chunk0[m]) * 256;
            const uint64_t wmask = (1ull << width) - 1ull;
            unsigned long long *km = key + (int64_t)m * n_seq;
            uint64_t cur = 0, head = 0;                // the running segment; the one that reached the lane from the left
            int64_t r = r0;
            uint32_t loc0 = loc_first;
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
                }
                const int s = site_score<RC>(tb, win_bits(w, i), nch);
                if (s >= thr && win_valid(w, i, width, wmask) && r >= 0) {
                    const uint64_t k = pack_site_key(s, loc0 + i);
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

struct SiteHist {
    int width[ST_MAX_MAT];
    int64_t off[ST_MAX_MAT];    // acc[off] = sites, acc[off + 1] = too_long, then D[2 max_len + 1], then Hlen[max_len + 1]
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
    for (int j = 0; j < ST_MAX_MAT; ++j)
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
    for (int j = 0; j < ST_MAX_MAT; ++j)
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

// ---- host: what the two entry points share --------------------------------------------------------------------------------------------
// Checked matrices, n > 0, n_seq > 0, n_mat > 0: sorts them by width, batches them (8 matrices, 24 chunk tables), leaves a batch's
// (score, loc) keys in scratch slot A (key[j n_seq + r] of the batch's matrix j = the caller's matrix bt.src[j], 0 = no site) and
// calls on_batch(bt, key, weights_dev): it enqueues its own work on `st` behind the scoring kernel and synchronises once before it
// returns.  The weights lie in slot C; slot B is the caller's.
template <class OnBatch>
int sites_key_batches(const char *who, const uint32_t *codes_dev, const uint16_t *inval_dev, int64_t n, const int64_t *borders_dev,
                      int64_t n_seq, int n_mat, const int32_t *widths, const int32_t *weights, const int32_t *thresholds, int revcom,
                      hipStream_t st, OnBatch on_batch) {
    const int64_t n_data = (n + 15) >> 4, n_tiles = (n_data + PW_TILE_GROUPS - 1) / PW_TILE_GROUPS;   // groups of 16 positions; wave tiles
    // persistent blocks: as many as are resident at once (registers and LDS decide; the tables are built once per block)
    int dev = 0, cus = 0, per_cu = 0;
    KMAP_CHECK_HIP(hipGetDevice(&dev));
    KMAP_CHECK_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    if (revcom) KMAP_CHECK_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, sites_multi_kernel<true>, PW_TPB, 0));
    else KMAP_CHECK_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, sites_multi_kernel<false>, PW_TPB, 0));
    KMAP_REQUIRE(cus > 0 && per_cu > 0, "%s: no block of the scoring kernel fits a compute unit", who);
    const unsigned grid = (unsigned)std::min<int64_t>((n_tiles + PW_WAVES - 1) / PW_WAVES, (int64_t)cus * per_cu);

    // by width (ties: the caller's order), so that a batch holds matrices of similar chunk counts
    std::vector<int> order(n_mat);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return widths[a] < widths[b]; });

    const int per_batch = std::min(n_mat, ST_MAX_MAT);
    int32_t *weights_dev = nullptr;
    KMAP_TRY(kmap_scratch((void **)&weights_dev, (size_t)n_mat * 512, st, KMAP_SLOT_C));
    KMAP_CHECK_HIP(hipMemcpyAsync(weights_dev, weights, (size_t)n_mat * 512, hipMemcpyHostToDevice, st));
    unsigned long long *key = nullptr;
    KMAP_TRY(kmap_scratch((void **)&key, (size_t)per_batch * (size_t)n_seq * 8, st, KMAP_SLOT_A));

    for (int first = 0; first < n_mat;) {
        SiteBatch bt = {};
        int chunks = 0;
        while (first + bt.n_mat < n_mat && bt.n_mat < ST_MAX_MAT) {
            const int m = order[first + bt.n_mat], nch = (widths[m] + 3) / 4, j = bt.n_mat;
            if (chunks + nch > ST_MAX_CHUNKS) break;
            bt.src[j] = m;
            bt.width[j] = widths[m];
            bt.chunk0[j] = chunks;
            bt.thr[j] = thresholds[m];
            chunks += nch;
            ++bt.n_mat;
        }
        // n_mat >= 1: one matrix has 8 chunks at the most
        KMAP_CHECK_HIP(hipMemsetAsync(key, 0, (size_t)bt.n_mat * (size_t)n_seq * 8, st));
        with_bool(revcom, [&](auto rc) {
            sites_multi_kernel<decltype(rc)::value><<<grid, PW_TPB, 0, st>>>(codes_dev, inval_dev, n_data, n_tiles, weights_dev, bt,
                                                                             borders_dev, n_seq, key);
        });
        KMAP_CHECK_HIP(hipGetLastError());
        KMAP_TRY(on_batch(bt, (const unsigned long long *)key, (const int32_t *)weights_dev));
        first += bt.n_mat;
    }
    return KMAP_OK;
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
    KMAP_TRY(kmap_scratch((void **)&acc, (size_t)std::min(n_mat, ST_MAX_MAT) * words * 8, st, KMAP_SLOT_B));
    if (lds) KMAP_TRY(kmap_allow_lds((const void *)sites_hist_kernel<true>, (int)(ST_HIST_LDS_WORDS * 4)));

    std::vector<unsigned long long> back;
    return sites_key_batches(
        "readscore_sites_library", codes_dev, inval_dev, n, borders_dev, n_seq, n_mat, widths, weights, thresholds, revcom, st,
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
    KMAP_TRY(kmap_scratch((void **)&acc, (size_t)ST_MAX_MAT * SC_SLOTS * 8, st, KMAP_SLOT_B));
    unsigned long long back[ST_MAX_MAT * SC_SLOTS];
    return sites_key_batches(
        "readscore_counts_library", codes_dev, inval_dev, n, borders_dev, n_seq, n_mat, widths, weights, thresholds, revcom, st,
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
