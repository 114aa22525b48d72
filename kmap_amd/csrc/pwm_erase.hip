// pwm_erase.hip -- the sites of a library of weight matrices erased from an invalid mask (discover_pwms --erase_rounds,
// erase_pwm_sites).  A hit is scan_pwm's (section 11): the tables, the group loads and the window helpers are
// pwm_internal.h's, so the scores are pwm_hits_kernel's by construction.  What is new is the cover: every position inside a hit.
//
//   * pwm_erase_kernel<RC>: one launch per matrix, nothing on the host in between.  A wave's tile is 62 OUTPUT groups: its 64 lanes
//     score the groups g0 - 2 .. g0 + 61, a lane takes the hit bits of the two groups in front of its own from its neighbours
//     (__shfl_up), smears the 48 hit bits right by the width and keeps the low 16: the cover of its own group -- a hit three groups
//     back ends at most 45 positions later, in front of it.  Lanes 2 .. 63 own their group: exactly one lane of one launch does, and
//     the launches follow each other on the stream, so the cover is ORed into accum16[g] with a plain read-modify-write.  The owned
//     hit bits and cover bits are counted (popcount, wave_sum, one integer atomic per wave and counter).  The two groups scored
//     twice (3 %) replace a hit16 round trip, a scan and a synchronisation per matrix.
//   * erase_apply_kernel: out[g] |= accum16[g], and the bits that are new in out are counted.
//
// The mask the matrices are evaluated against is only read until the apply kernel runs, so out may be that mask itself.
#include "common.h"
#include "pwm_batch.h"

namespace {

constexpr int ER_TILE_GROUPS = KMAP_WAVE - 2;     // groups a wave tile owns
constexpr int ER_APPLY_TPB = 256;
constexpr int ER_APPLY_BLOCKS = 2048;

// the cover of a hit word: bit b set = a window starts there; it covers the bits b .. b - (width - 1)
__device__ __forceinline__ uint64_t smear_right(uint64_t h, int width) {
    int done = 1;                          // every set bit stands for `done` covered positions
    while (2 * done <= width) {            // uniform
        h |= h >> done;
        done *= 2;
    }
    if (done < width) h |= h >> (width - done);
    return h;
}

// counters[0] += hits, counters[1] += covered positions of this matrix
template <bool RC>
__global__ __launch_bounds__(PW_TPB) void pwm_erase_kernel(const uint32_t *__restrict__ codes, const uint16_t *__restrict__ inval,
                                                           int64_t n_data, int64_t n_tiles, PwmWeights wt, int width, int nch,
                                                           int32_t thr, uint16_t *__restrict__ accum16,
                                                           unsigned long long *__restrict__ counters) {
    __shared__ int2 tab[PW_MAX_CHUNKS * 256];
    __shared__ int32_t wl[128];
    build_table(tab, wl, wt, width, nch);
    const int lane = threadIdx.x & (KMAP_WAVE - 1), wave = threadIdx.x >> 6;
    const uint64_t wmask = (1ull << width) - 1ull;
    unsigned long long hits = 0, covered = 0;
    for (int64_t t = (int64_t)blockIdx.x * PW_WAVES + wave; t < n_tiles; t += (int64_t)gridDim.x * PW_WAVES) {
        const int64_t g = t * ER_TILE_GROUPS - 2 + lane;
        const Grp w = load_grp<true>(codes, inval, g, n_data, lane);
        uint32_t bits = 0;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            int fwd, rc;
            win_score<RC>(tab, win_bits(w, i), nch, fwd, rc);
            const int s = RC ? (rc > fwd ? rc : fwd) : fwd;
            if (win_valid(w, i, width, wmask) && s >= thr) bits |= 0x8000u >> i;
        }
        const uint32_t h1 = __shfl_up(bits, 1), h2 = __shfl_up(bits, 2);      // groups g - 1 and g - 2 (lanes 0 and 1 own nothing)
        if (lane >= 2 && g < n_data) {
            const uint64_t word = ((uint64_t)h2 << 32) | ((uint64_t)h1 << 16) | bits;
            const uint32_t cover = (uint32_t)smear_right(word, width) & 0xFFFFu;
            if (cover) accum16[g] = (uint16_t)(accum16[g] | cover);
            hits += (unsigned)__builtin_popcount(bits);
            covered += (unsigned)__builtin_popcount(cover);
        }
    }
    hits = wave_sum(hits);
    covered = wave_sum(covered);
    if (lane == 0) {
        if (hits) atomicAdd(&counters[0], hits);
        if (covered) atomicAdd(&counters[1], covered);
    }
}

// out may be the mask the matrices were evaluated against: nothing reads that any more
__global__ __launch_bounds__(ER_APPLY_TPB) void erase_apply_kernel(const uint16_t *__restrict__ accum16, int64_t n_data, uint16_t *out,
                                                                   unsigned long long *__restrict__ n_new) {
    unsigned long long fresh = 0;
    for (int64_t g = (int64_t)blockIdx.x * ER_APPLY_TPB + threadIdx.x; g < n_data; g += (int64_t)gridDim.x * ER_APPLY_TPB) {
        const uint32_t a = accum16[g];
        if (a) {
            const uint32_t old = out[g];
            out[g] = (uint16_t)(old | a);
            fresh += (unsigned)__builtin_popcount(a & ~old);
        }
    }
    fresh = wave_sum(fresh);
    if ((threadIdx.x & (KMAP_WAVE - 1)) == 0 && fresh) atomicAdd(n_new, fresh);
}

}  // namespace

extern "C" {

int kmap_erase_pwm_sites_dev(const uint32_t *codes_dev, const uint16_t *inval_eval_dev, int64_t n, int n_mat, const int32_t *widths,
                             const int32_t *weights, const int32_t *thresholds, int revcom, uint16_t *inval_out_dev, int64_t *n_hits,
                             int64_t *n_covered, int64_t *n_new) {
    KMAP_REQUIRE(n_mat >= 0 && n >= 0, "erase_pwm_sites_dev: negative size");
    KMAP_REQUIRE(n_new, "erase_pwm_sites_dev: null pointer");
    if (n_mat > 0) {
        KMAP_REQUIRE(widths && weights && thresholds && n_hits && n_covered, "erase_pwm_sites_dev: null pointer");
        KMAP_TRY(pwm_library_check("erase_pwm_sites_dev", n_mat, widths, weights));
    }
    const bool work = n_mat > 0 && n > 0;              // no matrix, or no position: no hit, the mask stays
    KMAP_REQUIRE(!work || (codes_dev && inval_eval_dev && inval_out_dev), "erase_pwm_sites_dev: null pointer");
    if (n_mat > 0) {
        memset(n_hits, 0, (size_t)n_mat * 8);
        memset(n_covered, 0, (size_t)n_mat * 8);
    }
    *n_new = 0;
    if (!work) return KMAP_OK;
    hipStream_t st = nullptr;                          // the null stream: this entry has no stream argument

    const int64_t n_data = (n + 15) >> 4, n_tiles = (n_data + ER_TILE_GROUPS - 1) / ER_TILE_GROUPS;
    const unsigned grid = (unsigned)std::min<int64_t>((n_tiles + PW_WAVES - 1) / PW_WAVES, PW_MAX_BLOCKS);
    uint16_t *accum16 = nullptr;
    unsigned long long *counters = nullptr;            // [2 m] hits, [2 m + 1] covered, [2 n_mat] new bits
    const size_t n_counters = 2 * (size_t)n_mat + 1;
    KMAP_TRY(kmap_scratch((void **)&accum16, (size_t)n_data * 2, st, KMAP_SLOT_HASH));
    KMAP_TRY(kmap_scratch((void **)&counters, n_counters * 8, st, KMAP_SLOT_B));
    KMAP_CHECK_HIP(hipMemsetAsync(accum16, 0, (size_t)n_data * 2, st));
    KMAP_CHECK_HIP(hipMemsetAsync(counters, 0, n_counters * 8, st));

    for (int m = 0; m < n_mat; ++m) {
        PwmWeights wt;
        memcpy(wt.w, weights + (size_t)m * 128, sizeof wt.w);      // [4][32], zeros behind the width (checked)
        const int width = widths[m], nch = (width + 3) / 4;
        with_bool(revcom, [&](auto rc) {
            pwm_erase_kernel<decltype(rc)::value><<<grid, PW_TPB, 0, st>>>(codes_dev, inval_eval_dev, n_data, n_tiles, wt, width, nch,
                                                                           thresholds[m], accum16, counters + 2 * (size_t)m);
        });
        KMAP_CHECK_HIP(hipGetLastError());
    }
    erase_apply_kernel<<<(unsigned)std::min<int64_t>(grid_for(n_data, ER_APPLY_TPB), ER_APPLY_BLOCKS), ER_APPLY_TPB, 0, st>>>(
        accum16, n_data, inval_out_dev, counters + 2 * (size_t)n_mat);
    KMAP_CHECK_HIP(hipGetLastError());

    std::vector<unsigned long long> back(n_counters);
    KMAP_CHECK_HIP(hipMemcpyAsync(back.data(), counters, n_counters * 8, hipMemcpyDeviceToHost, st));
    KMAP_CHECK_HIP(hipStreamSynchronize(st));          // the only one
    for (int m = 0; m < n_mat; ++m) {
        n_hits[m] = (int64_t)back[2 * (size_t)m];
        n_covered[m] = (int64_t)back[2 * (size_t)m + 1];
    }
    *n_new = (int64_t)back[2 * (size_t)n_mat];
    return KMAP_OK;
}

}  // extern "C"
