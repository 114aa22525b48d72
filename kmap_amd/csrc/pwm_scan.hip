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
//     positions; exclusive scan of the tile counts (pwm_pass_a, pwm_internal.h); pass B (pwm_write_kernel): the sparse traversal
//     of pwm_internal.h (for_each_hit: the tiles with hits evaluate their hits again, each with the read it lies in) writes loc /
//     score / strand at the tile's offset.  Array order IS read order, ascending inside a read, so the lists need no sort.  The
//     per-read counts are integer atomic adds of run lengths (order-free, so the result is deterministic).  Nothing depends on the
//     reads' lengths: empty reads, a read that spans thousands of tiles, more than 65 535 reads and any number of hits per read
//     take the same path.
#include "common.h"
#include "pwm_internal.h"
#include "scan_internal.h"

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
    uint64_t out = 0;      // where the lane's next hit goes
    int32_t run = 0;       // the lane's hits in the read it is in
    for_each_hit<RC, true>(
        tab, codes, inval, n_data, n_tiles, nch, hit16, tile_cnt, borders, n_seq,
        [&](int64_t t, uint32_t bits, int lane) {      // wave-uniform: the lanes' offsets inside the tile, before any hit is visited
            const uint32_t cnt = (uint32_t)__builtin_popcount(bits);
            out = tile_off[t] + (wave_inclusive_scan(cnt) - cnt);
        },
        [&](int, int64_t p, int64_t, int64_t start, uint64_t, int fwd, int rc) {
            const bool minus = RC && rc > fwd;
            pos[out] = (int32_t)(p - start);
            score[out] = minus ? rc : fwd;
            strand[out] = minus ? 1 : 0;
            ++out;
            ++run;
        },
        [&](int64_t left, int64_t) {                   // counting what the read the lane leaves got
            if (run) atomicAdd(&hits[left], run);
            run = 0;
        });
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
    PwmPlan pl;
    KMAP_TRY(pwm_plan(pl, "pwm_scan", n, n_seq, width, weights));
    s->n_seq = n_seq;
    s->total = 0;
    s->pwm = 1;
    if (total_hits) *total_hits = 0;
    if (n_seq == 0) return KMAP_OK;
    KMAP_REQUIRE(codes_dev && inval_dev && borders_dev, "pwm_scan: null pointer");
    hipStream_t st = as_stream(stream);
    KMAP_TRY(kmap_scan_reserve(s, n_seq));
    KMAP_CHECK_HIP(hipMemsetAsync(s->hits, 0, (size_t)n_seq * 4, st));
    if (pl.n_tiles == 0) return KMAP_OK;
    uint16_t *hit16 = nullptr;
    uint32_t *tile_cnt = nullptr;
    uint64_t *tile_off = nullptr;
    uint64_t total = 0;
    KMAP_TRY(pwm_pass_a(pl, codes_dev, inval_dev, threshold, revcom, st, &hit16, &tile_cnt, &tile_off, &total));
    KMAP_TRY(kmap_scan_reserve_pos(s, total));
    KMAP_TRY(reserve_scores(s, total));
    if (total) {
        with_bool(revcom, [&](auto rc) {
            pwm_write_kernel<decltype(rc)::value><<<pl.grid, PW_TPB, 0, st>>>(codes_dev, inval_dev, pl.n_data, pl.n_tiles, pl.wt, width,
                                                                              pl.nch, hit16, tile_cnt, tile_off, borders_dev, n_seq,
                                                                              s->hits, s->pos, s->score, s->strand);
        });
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
