// pwm_scan.hip -- position weight matrix scan of the packed reads (scan_pwm).  Every window of `width`
// positions gets an integer log-odds score from a 4 x width weight matrix, on the forward strand and -- with revcom -- on the
// reverse complement; a hit is a window without an invalid position whose score reaches the threshold.  The reads are used as
// they lie in HBM (2-bit codes + invalid mask, packed.hip: 0.375 B per position), nothing is unpacked.
//
//   * A window's score is a sum of table lookups, one per chunk of 4 columns: the chunk's 4 bases are 8 bits of the code stream
//     and index a 256-entry table whose entry holds the chunk's forward partial and its reverse-complement partial, so ONE 8-byte
//     LDS read serves both strands.  ceil(width / 4) <= 8 chunks, at most 16 KiB per block, built once per block from the weights
//     (a kernel argument) by persistent blocks; the padding columns of width % 4 != 0 weigh 0 for every base.
//   * lane = one group of 16 window starts; it needs the group's code word and the next two (16 + 30 positions) and takes those
//     from the two lanes above it (the last two lanes of a wave load them: the halo groups make that legal for every data group).
//   * pass A (pwm_hits_kernel): hit bit per position (uint16 per group, window i in bit 15 - i) + hit count per wave tile of 1024
//     positions; exclusive scan of the tile counts; pass B (pwm_write_kernel): the tiles with hits evaluate their (sparse) hits
//     again and write loc / score / strand at the tile's offset.  Array order IS read order, ascending inside a read, so the lists
//     need no sort.  A hit's read is the last read that starts at or before it (a valid window cannot cross the 255 behind a read):
//     binary search of the borders for a lane's first hit, a step forward for the following ones; the per-read counts are integer
//     atomic adds of run lengths (order-free, so the result is deterministic).  Nothing depends on the reads' lengths: empty reads,
//     a read that spans thousands of tiles, more than 65 535 reads and any number of hits per read take the same path.
#include <algorithm>

#include "common.h"
#include "pwm_internal.h"
#include "scan_internal.h"
#include "scan_util.h"

namespace {

// pass B: loc / score / strand of every hit, in array order, and the per-read counts
template <bool RC>
__global__ __launch_bounds__(PW_TPB) void pwm_write_kernel(const uint32_t *__restrict__ codes, const uint16_t *__restrict__ inval,
                                                           int64_t n_data, int64_t n_tiles, PwmWeights wt, int width, int nch,
                                                           const uint16_t *__restrict__ hit16, const uint32_t *__restrict__ tile_cnt,
                                                           const uint64_t *__restrict__ tile_off, const int64_t *__restrict__ borders,
                                                           int64_t n_seq, int32_t *__restrict__ hits, int32_t *__restrict__ pos,
                                                           int32_t *__restrict__ score, uint8_t *__restrict__ strand) {
    __shared__ int2 tab[PW_MAX_CHUNKS * 256];
    __shared__ int32_t wl[128];
    build_table(tab, wl, wt, width, nch);
    const int lane = threadIdx.x & (KMAP_WAVE - 1), wave = threadIdx.x >> 6;
    for (int64_t t = (int64_t)blockIdx.x * PW_WAVES + wave; t < n_tiles; t += (int64_t)gridDim.x * PW_WAVES) {
        if (tile_cnt[t] == 0) continue;    // uniform
        const int64_t g = t * PW_TILE_GROUPS + lane;
        const Grp w = load_grp(codes, inval, g, n_data, lane);
        uint32_t bits = g < n_data ? (uint32_t)hit16[g] : 0u;
        const uint32_t cnt = (uint32_t)__builtin_popcount(bits);
        uint32_t inc = cnt;
        for (int o = 1; o < KMAP_WAVE; o <<= 1) {
            const uint32_t u = __shfl_up(inc, o);
            if (lane >= o) inc += u;
        }
        if (bits) {        // (no `continue`: the wave meets again at the next tile's shuffles)
            uint64_t out = tile_off[t] + (inc - cnt);
            // the read of the lane's first hit: the last one that starts at or before it
            int64_t p = g * 16 + (__builtin_clz(bits) - 16);
            int64_t lo = 0, hi = n_seq;        // borders[2 lo] <= p (or lo == 0), borders[2 hi] > p (or hi == n_seq)
            while (hi - lo > 1) {
                const int64_t mid = lo + ((hi - lo) >> 1);
                if (borders[2 * mid] <= p) lo = mid; else hi = mid;
            }
            int64_t r = lo, start = borders[2 * r];
            int32_t run = 0;
            while (bits) {
                const int i = __builtin_clz(bits) - 16;
                bits &= ~(0x8000u >> i);
                p = g * 16 + i;
                while (r + 1 < n_seq) {        // hits ascend: step to the hit's read, counting what the last one got
                    const int64_t nx = borders[2 * (r + 1)];
                    if (nx > p) break;
                    if (run) atomicAdd(&hits[r], run);
                    run = 0;
                    ++r;
                    start = nx;
                }
                int fwd, rc;
                win_score<RC>(tab, win_bits(w, i), nch, fwd, rc);
                const bool minus = RC && rc > fwd;
                pos[out] = (int32_t)(p - start);
                score[out] = minus ? rc : fwd;
                strand[out] = minus ? 1 : 0;
                ++out;
                ++run;
            }
            if (run) atomicAdd(&hits[r], run);
        }
    }
}

int reserve_scores(kmap_scan *s, uint64_t total) {
    if (s->cap_score < (int64_t)total || !s->score) {
        if (s->score) KMAP_CHECK_HIP(hipFree(s->score));
        if (s->strand) KMAP_CHECK_HIP(hipFree(s->strand));
        s->score = nullptr; s->strand = nullptr; s->cap_score = 0;
        const size_t cap = total ? (size_t)total + (size_t)total / 8 : 1;
        KMAP_CHECK_HIP(hipMalloc((void **)&s->score, cap * 4));
        KMAP_CHECK_HIP(hipMalloc((void **)&s->strand, cap));
        s->cap_score = (int64_t)cap;
    }
    return KMAP_OK;
}

}  // namespace

extern "C" {

int kmap_pwm_scan_packed_dev(kmap_scan *s, const uint32_t *codes_dev, const uint16_t *inval_dev, int64_t n, const int64_t *borders_dev,
                             int64_t n_seq, int width, const int32_t *weights, int32_t threshold, int revcom, int64_t *total_hits,
                             void *stream) {
    KMAP_REQUIRE(s, "pwm_scan: null handle");
    KMAP_REQUIRE(width >= 4 && width <= 31, "pwm_scan: width=%d outside 4..31", width);
    KMAP_REQUIRE(weights, "pwm_scan: null weights");
    KMAP_REQUIRE(n >= 0 && n_seq >= 0, "pwm_scan: negative size");
    s->n_seq = n_seq;
    s->total = 0;
    s->pwm = 1;
    if (total_hits) *total_hits = 0;
    if (n_seq == 0) return KMAP_OK;
    KMAP_REQUIRE(codes_dev && inval_dev && borders_dev, "pwm_scan: null pointer");
    hipStream_t st = as_stream(stream);
    KMAP_TRY(kmap_scan_reserve(s, n_seq));
    KMAP_CHECK_HIP(hipMemsetAsync(s->hits, 0, (size_t)n_seq * 4, st));
    const int64_t n_data = (n + 15) >> 4, n_tiles = (n_data + PW_TILE_GROUPS - 1) / PW_TILE_GROUPS;
    if (n_tiles == 0) return KMAP_OK;
    PwmWeights wt;
    memset(&wt, 0, sizeof wt);
    for (int b = 0; b < 4; ++b)
        for (int j = 0; j < width; ++j) wt.w[b][j] = weights[b * width + j];
    const int nch = (width + 3) / 4;
    uint16_t *hit16 = nullptr;
    uint32_t *tile_cnt = nullptr;
    uint64_t *tile_off = nullptr;
    KMAP_TRY(kmap_scratch((void **)&hit16, (size_t)n_data * 2, st, KMAP_SLOT_HASH));
    KMAP_TRY(kmap_scratch((void **)&tile_cnt, (size_t)n_tiles * 4, st, KMAP_SLOT_B));
    KMAP_TRY(kmap_scratch((void **)&tile_off, ((size_t)n_tiles + 1) * 8, st, KMAP_SLOT_PART));
    const unsigned grid = (unsigned)std::min<int64_t>((n_tiles + PW_WAVES - 1) / PW_WAVES, PW_MAX_BLOCKS);
    if (revcom)
        pwm_hits_kernel<true><<<grid, PW_TPB, 0, st>>>(codes_dev, inval_dev, n_data, n_tiles, wt, width, nch, threshold, hit16, tile_cnt);
    else
        pwm_hits_kernel<false><<<grid, PW_TPB, 0, st>>>(codes_dev, inval_dev, n_data, n_tiles, wt, width, nch, threshold, hit16, tile_cnt);
    KMAP_CHECK_HIP(hipGetLastError());
    KMAP_TRY(exclusive_scan_u32(tile_cnt, n_tiles, tile_off, st));
    uint64_t total = 0;
    KMAP_CHECK_HIP(hipMemcpyAsync(&total, tile_off + n_tiles, 8, hipMemcpyDeviceToHost, st));
    KMAP_CHECK_HIP(hipStreamSynchronize(st));
    KMAP_TRY(kmap_scan_reserve_pos(s, total));
    KMAP_TRY(reserve_scores(s, total));
    if (total) {
        if (revcom)
            pwm_write_kernel<true><<<grid, PW_TPB, 0, st>>>(codes_dev, inval_dev, n_data, n_tiles, wt, width, nch, hit16, tile_cnt, tile_off,
                                                           borders_dev, n_seq, s->hits, s->pos, s->score, s->strand);
        else
            pwm_write_kernel<false><<<grid, PW_TPB, 0, st>>>(codes_dev, inval_dev, n_data, n_tiles, wt, width, nch, hit16, tile_cnt, tile_off,
                                                            borders_dev, n_seq, s->hits, s->pos, s->score, s->strand);
        KMAP_CHECK_HIP(hipGetLastError());
    }
    s->total = (int64_t)total;
    if (total_hits) *total_hits = (int64_t)total;
    return KMAP_OK;
}

int kmap_pwm_scan_fetch(kmap_scan *s, int32_t *hits_per_read, int32_t *positions, int32_t *scores, uint8_t *strand) {
    KMAP_REQUIRE(s, "pwm_scan_fetch: null handle");
    if (!s->pwm) {
        kmap_set_error("pwm_scan_fetch: the handle's last run was not a PWM scan");
        return KMAP_E_STATE;
    }
    KMAP_CHECK_HIP(hipDeviceSynchronize());
    if (s->n_seq && hits_per_read) KMAP_CHECK_HIP(hipMemcpy(hits_per_read, s->hits, (size_t)s->n_seq * 4, hipMemcpyDeviceToHost));
    if (s->total) {
        if (positions) KMAP_CHECK_HIP(hipMemcpy(positions, s->pos, (size_t)s->total * 4, hipMemcpyDeviceToHost));
        if (scores) KMAP_CHECK_HIP(hipMemcpy(scores, s->score, (size_t)s->total * 4, hipMemcpyDeviceToHost));
        if (strand) KMAP_CHECK_HIP(hipMemcpy(strand, s->strand, (size_t)s->total, hipMemcpyDeviceToHost));
    }
    return KMAP_OK;
}

}  // extern "C"
