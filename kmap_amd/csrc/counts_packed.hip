// counts_packed.hip -- k-mer counting straight from the 2-bit packed reads (layout: packed.hip): the LDS-privatised histograms for
// k <= 9 (32-bit counters for k <= 7, 16-bit counters for k = 8, 9; device atomics below 2^16 positions) and the C entry points of the
// whole packed counting path, the key-space front door included.  They choose between these kernels, the partitioned histograms
// (counts_part.hip / counts_fine.hip, 10 <= k <= 16), the key-range stage (counts_range.hip) and, for k > 16 or reads too long for
// the skip-bit dedupe (dedupe_packed.hip), a materialised hash array (packed.hip) that counts.hip / counts_sort.hip count.
#include "common.h"
#include "counts_internal.h"
#include "packed_keys.h"

namespace {

constexpr int BLK = 256;

// ---- histogram straight from the packed stream (no per-read dedupe) ---------------------------------------------
constexpr int HP_BINS = 32768;   // uint32 LDS bins per block (128 KiB)
constexpr int HP_TPB = 1024;
template <bool WIDE, bool LDSMODE>
__global__ __launch_bounds__(LDSMODE ? HP_TPB : BLK) void hist_packed_kernel(const uint32_t *__restrict__ codes,
                                                                             const uint16_t *__restrict__ inval, int64_t n,
                                                                             int k, uint64_t bin0, uint32_t *__restrict__ bins,
                                                                             const uint32_t *__restrict__ skip) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lb[];
    if (LDSMODE) {
        for (int b = threadIdx.x; b < HP_BINS; b += blockDim.x) lb[b] = 0;
        __syncthreads();
    }
    const uint64_t kmask = low_mask<uint64_t>(k);
    const int64_t n_groups = (n + 15) >> 4;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    // software pipeline: the loads of the thread's NEXT group are issued before the 16 windows of the current one are counted
    // (raw registers, nothing derived from them before their turn, the same number of loads on every path -- otherwise the
    // compiler waits for them where they are issued).  Without it every iteration exposed one memory round trip: 360
    // iterations x ~1.6 us = the 0.59 ms a pass took, at 50 % VALU utilisation and 75 % of the wave-cycles waiting (PMC).
    const int64_t g_first = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t g_last = n_groups - 1;
    uint32_t nc0 = 0, nc1 = 0, nc2 = 0, nsk = 0;
    uint16_t nf0 = 0, nf1 = 0, nf2 = 0;
    const uint32_t *skp = skip ? skip : codes;    // the skip word travels with the windows; without skip bits: any valid word, ignored
    if (n_groups > 0) {
        const int64_t gl = g_first < n_groups ? g_first : g_last;
        nc0 = codes[gl]; nc1 = codes[gl + 1]; nc2 = codes[gl + 2];
        nf0 = inval[gl]; nf1 = inval[gl + 1]; nf2 = inval[gl + 2];
        nsk = skp[gl >> 1];
    }
    const uint32_t dummy = (uint32_t)HP_BINS + (threadIdx.x & 63u);   // LDSMODE: this lane's private bin behind the table
    for (int64_t g = g_first; g < n_groups; g += stride) {
        Win w;
        w.t0 = ((uint64_t)nc0 << 32) | nc1;
        w.c2 = nc2;
        w.m = ((uint64_t)nf0 << 32) | ((uint64_t)nf1 << 16) | nf2;
        const uint32_t sk16 = skip ? skip16_in(nsk, g) : 0u;
        {
            const int64_t gn = g + stride < n_groups ? g + stride : g_last;      // clamped: the last round re-reads a valid group
            nc0 = codes[gn]; nc1 = codes[gn + 1]; nc2 = codes[gn + 2];
            nf0 = inval[gn]; nf1 = inval[gn + 1]; nf2 = inval[gn + 2];
            nsk = skp[gn >> 1];
        }
        if ((w.m >> 32) == 0xFFFFull) continue;   // group entirely invalid (cheap skip of masked regions)
        if constexpr (LDSMODE && !WIDE) {
            // 32-bit fast path (k <= 16): window i = bits [63-2i, 64-2i-2k) of t0 -> one v_alignbit + one shift; the 16
            // "window touches an invalid position" flags come from one doubling pass over the 48-bit invalid stream
            // (bit 47-p of `bad` = OR of m[p .. p+k-1]) instead of a 64-bit shift-and-mask per window
            const uint32_t bad16 = (uint32_t)(smear_invalid(w.m, k) >> 32) | sk16;   // windows 0..15 in bits 15..0 (+ per-read duplicates)
            const uint32_t hi = (uint32_t)(w.t0 >> 32), lo = (uint32_t)w.t0;
            const uint32_t b0 = (uint32_t)bin0;
            const int sh = 32 - 2 * k;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const uint32_t top = (i == 0) ? hi : __builtin_amdgcn_alignbit(hi, lo, 32 - 2 * i);
                // no branch, no exec mask per window (a pass was bound by instruction issue: ~10 instructions per window, two of
                // them scalar): a window that is invalid (sign-extended flag bit ORed in) or belongs to another pass's bin range
                // lands, by one unsigned min, in the lane's private bin behind the table
                // (key ^ b0) | flag in one v_bitop3: b0 is a multiple of the 32 768 bins of a pass, so inside the pass's range the
                // XOR is the subtraction, and outside it leaves a high bit set
                uint32_t a = __builtin_amdgcn_bitop3_b32(top >> sh, b0, (uint32_t)__builtin_amdgcn_sbfe((int)bad16, 15 - i, 1), 0xBE);
                a = a < dummy ? a : dummy;
                atomicAdd(&lb[a], 1u);
            }
            continue;
        }
        const uint32_t sk = sk16;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            bool bad;
            const uint64_t h = win_hash<WIDE>(w, i, k, kmask, bad);
            if (bad || ((sk >> (15 - i)) & 1u)) continue;
            if (LDSMODE) {
                const uint64_t a = h - bin0;
                if (a < (uint64_t)HP_BINS) atomicAdd(&lb[a], 1u);
            } else {
                atomicAdd(&bins[h], 1u);
            }
        }
    }
    if (LDSMODE) {
        __syncthreads();
        for (int b = threadIdx.x; b < HP_BINS; b += blockDim.x) {
            const uint32_t c = lb[b];
            if (c) atomicAdd(&bins[bin0 + b], c);
        }
    }
}

// ---- the same with 16-bit LDS counters: 65 536 bins per pass (k = 8 in ONE pass instead of two, k = 9 in four instead of eight) ----
// Two counters per LDS word, plain (non-returning) adds of 1 or 1 << 16.  A block adds at most 1024 x 16 = 16 384 windows per round of its
// loop; every HP16_ROUNDS = 3 rounds the block meets at a barrier and sweeps the table (32 words per thread): a word with a half at or
// above 0x4000 is emptied (atomic exchange) into the global bins.  A second barrier BEHIND the sweep keeps the waves that finish it early
// from adding the next interval's windows before a slower wave has looked at its words: between two looks at a word exactly one
// interval's adds (at most 49 152) can land on it, so a half stays below 0x4000 + 49 152 = 65 536 and no carry ever reaches the
// neighbour -- also when ONE k-mer takes every window of a block (poly-A: tests/test_gpu_packed.py::test_hist16_single_kmer_no_carry).
// (The returning form of the add with a check of the
// returned word was measured first: 0.97 against 0.94 ms for the two 32-bit passes -- the returned data costs what the second pass did.)
constexpr int HP16_BINS = 65536;
constexpr int HP16_ROUNDS = 3;
__global__ __launch_bounds__(HP_TPB) void hist_packed16_kernel(const uint32_t *__restrict__ codes, const uint16_t *__restrict__ inval,
                                                               int64_t n, int k, uint32_t bin0, uint32_t *__restrict__ bins,
                                                               const uint32_t *__restrict__ skip) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lb[];      // HP16_BINS / 2 words + 64 lane-private words for dropped windows
    for (int b = threadIdx.x; b < HP16_BINS / 2 + 64; b += blockDim.x) lb[b] = 0;
    __syncthreads();
    const int64_t n_groups = (n + 15) >> 4;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t g_first = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t g_last = n_groups - 1;
    uint32_t nc0 = 0, nc1 = 0, nsk = 0;
    uint16_t nf0 = 0, nf1 = 0, nf2 = 0;
    const uint32_t *skp = skip ? skip : codes;                            // the same software pipeline as hist_packed_kernel's, without the third code word
    if (n_groups > 0) {
        const int64_t gl = g_first < n_groups ? g_first : g_last;
        nc0 = codes[gl]; nc1 = codes[gl + 1];
        nf0 = inval[gl]; nf1 = inval[gl + 1]; nf2 = inval[gl + 2];
        nsk = skp[gl >> 1];
    }
    const uint32_t dummy = (uint32_t)HP16_BINS + 2u * (threadIdx.x & 63u);   // bin index of the lane's private word (low half)
    const int sh = 32 - 2 * k;
    // every thread of the block runs the same number of rounds (the barriers): a thread behind the last group counts nothing
    const int64_t rounds = (n_groups - (int64_t)blockIdx.x * blockDim.x + stride - 1) / stride;      // of thread 0 = the block's maximum
    auto sweep = [&]() {
        typedef uint32_t u32x4v __attribute__((ext_vector_type(4)));
        for (int q = threadIdx.x; q < HP16_BINS / 8; q += HP_TPB) {        // 4 words = 8 bins per step
            const u32x4v v = *reinterpret_cast<const u32x4v *>(lb + 4 * q);
            if (((v.x | v.y | v.z | v.w) & 0xC000C000u) == 0u) continue;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t w0 = j == 0 ? v.x : j == 1 ? v.y : j == 2 ? v.z : v.w;
                if ((w0 & 0xC000C000u) == 0u) continue;
                const uint32_t w = atomicExch(&lb[4 * q + j], 0u);
                const uint32_t b = (uint32_t)(8 * q + 2 * j);
                if (w & 0xFFFFu) atomicAdd(&bins[bin0 + b], w & 0xFFFFu);
                if (w >> 16) atomicAdd(&bins[bin0 + b + 1], w >> 16);
            }
        }
        if (threadIdx.x < 64) lb[HP16_BINS / 2 + threadIdx.x] = 0;          // the private words only absorb: nobody reads them
    };
    int64_t g = g_first;
    for (int64_t r = 0; r < rounds; ++r, g += stride) {
        if (r && r % HP16_ROUNDS == 0) {
            __syncthreads();
            sweep();
            __syncthreads();    // no wave adds for the next interval before every word has been looked at (see above)
        }
        const uint32_t hi = nc0, lo = nc1;
        const uint64_t bad = ((uint64_t)nf0 << 32) | ((uint64_t)nf1 << 16) | nf2;
        const uint32_t sk16 = skip ? skip16_in(nsk, g) : 0u;
        {
            const int64_t gn = g + stride < n_groups ? g + stride : g_last;      // clamped: the last round re-reads a valid group
            nc0 = codes[gn]; nc1 = codes[gn + 1];
            nf0 = inval[gn]; nf1 = inval[gn + 1]; nf2 = inval[gn + 2];
            nsk = skp[gn >> 1];
        }
        if (g >= n_groups || (bad >> 32) == 0xFFFFull) continue;   // behind the array / group entirely invalid
        const uint32_t bad16 = (uint32_t)(smear_invalid(bad, k) >> 32) | sk16;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const uint32_t top = (i == 0) ? hi : __builtin_amdgcn_alignbit(hi, lo, 32 - 2 * i);
            // (key ^ bin0) | flag: inside the pass's range the XOR is the subtraction, outside it (or dropped) a high bit is set
            uint32_t a = __builtin_amdgcn_bitop3_b32(top >> sh, bin0, (uint32_t)__builtin_amdgcn_sbfe((int)bad16, 15 - i, 1), 0xBE);
            a = a < dummy ? a : dummy;
            atomicAdd(lb + (a >> 1), 1u << ((a & 1u) << 4));
        }
    }
    __syncthreads();
    for (int b = threadIdx.x; b < HP16_BINS / 2; b += blockDim.x) {
        const uint32_t w = lb[b];
        if (w & 0xFFFFu) atomicAdd(&bins[bin0 + 2 * b], w & 0xFFFFu);
        if (w >> 16) atomicAdd(&bins[bin0 + 2 * b + 1], w >> 16);
    }
}

// the hash array of the packed reads (uint32 for k < 16, else uint64; the stream's KMAP_SLOT_HASH scratch), de-duplicated per read
// on request: the way to the counts for reads longer than the LDS set of dedupe_skip_bits allows, and for k > 16
int hash_and_dedupe(const uint32_t *codes_dev, const uint16_t *inval_dev, int64_t n, const int64_t *borders_dev, int64_t n_seq, int k,
                    int dedupe_per_read, void *stream, void **hash_out) {
    void *hash = nullptr;
    KMAP_TRY(kmap_scratch(&hash, (size_t)(n ? n : 1) * (k < 16 ? 4 : 8), as_stream(stream), KMAP_SLOT_HASH));
    KMAP_TRY(kmap_hash_kmers_packed_dev(codes_dev, inval_dev, n, k, hash, stream));
    if (dedupe_per_read) {
        if (k < 16) KMAP_TRY(kmap_dedupe_per_read_u32_dev((uint32_t *)hash, n, borders_dev, n_seq, stream));
        else KMAP_TRY(kmap_dedupe_per_read_u64_dev((uint64_t *)hash, n, borders_dev, n_seq, stream));
    }
    *hash_out = hash;
    return KMAP_OK;
}
}  // namespace

extern "C" {

// fills c->bins (zeroed first) with the k-mer histogram of the packed reads; k <= 16
int kmap_counts_hist_packed_dev(kmap_counts *c, const uint32_t *codes_dev, const uint16_t *inval_dev, int64_t n,
                                const int64_t *borders_dev, int64_t n_seq, int k, int dedupe_per_read, void *stream) {
    KMAP_REQUIRE(c, "counts_hist_packed: null handle");
    KMAP_REQUIRE(k > 0 && k <= 16, "counts_hist_packed: k=%d needs the sort path (no histogram)", k);
    KMAP_REQUIRE(n >= 0 && codes_dev && inval_dev, "counts_hist_packed: bad input");
    hipStream_t st = as_stream(stream);
    uint32_t *skip = nullptr;   // per-read duplicates as one bit per position (first find_motif round), or null
    if (dedupe_per_read) {
        KMAP_REQUIRE(n_seq == 0 || borders_dev, "counts_hist_packed: dedupe needs borders");
        KMAP_TRY(dedupe_skip_bits(codes_dev, inval_dev, n, borders_dev, n_seq, k, st, &skip));
    }
    if (dedupe_per_read && !skip) {
        // reads longer than the LDS set allows: per-read dedupe on a materialised hash array (any length)
        void *hash = nullptr;
        KMAP_TRY(hash_and_dedupe(codes_dev, inval_dev, n, borders_dev, n_seq, k, 1, stream, &hash));
        return kmap_counts_hist_hashes(c, hash, n, k, st);
    }
    if (kmap_counts_part_applies(k, n)) {
        // 10 <= k <= 16: bucket-partitioned histogram, keys hashed from the packed reads inside its count and scatter passes (no
        // 4 B / position hash array written and read back)
        return kmap_counts_part_hist_packed(c, codes_dev, inval_dev, skip, n, k, st);
    }
    KMAP_TRY(kmap_counts_prepare_bins(c, k, st));
    if (n > 0) {
        const size_t n_bins = (size_t)1 << (2 * k);
        if (n_bins >= (size_t)HP16_BINS && n_bins / HP16_BINS <= 16 && n >= (1 << 16)) {
            // k = 8, 9: 16-bit LDS counters, 65 536 bins per pass
            KMAP_TRY(kmap_allow_lds((const void *)hist_packed16_kernel, (HP16_BINS / 2 + 64) * 4));
            for (size_t p = 0; p < n_bins / HP16_BINS; ++p)
                hist_packed16_kernel<<<256, HP_TPB, (HP16_BINS / 2 + 64) * 4, st>>>(codes_dev, inval_dev, n, k, (uint32_t)(p * HP16_BINS), c->bins, skip);
        } else if (n_bins <= (size_t)HP_BINS && n >= (1 << 16)) {   // k <= 7: the whole table in one block's 32-bit LDS counters
            KMAP_TRY(kmap_allow_lds((const void *)hist_packed_kernel<false, true>, (HP_BINS + 64) * 4));
            hist_packed_kernel<false, true><<<256, HP_TPB, (HP_BINS + 64) * 4, st>>>(codes_dev, inval_dev, n, k, 0, c->bins, skip);
        } else {
            int64_t g = ((n + 15) / 16 + BLK - 1) / BLK;
            if (g > 256 * 16) g = 256 * 16;
            hist_packed_kernel<false, false><<<(unsigned)g, BLK, 16, st>>>(codes_dev, inval_dev, n, k, 0, c->bins, skip);
        }
        KMAP_CHECK_HIP(hipGetLastError());
    }
    return KMAP_OK;
}

int kmap_counts_bins(kmap_counts *c, void **bins_dev, int64_t *n_bins) {
    KMAP_REQUIRE(c && bins_dev && n_bins, "counts_bins: null");
    KMAP_TRY(kmap_counts_bins_check(c, "counts_bins"));
    *bins_dev = c->bins;
    *n_bins = (int64_t)c->bins_cap;
    return KMAP_OK;
}

int kmap_counts_finish(kmap_counts *c, int k, int merge_revcom, int64_t *n_uniq, void *stream) {
    KMAP_REQUIRE(c && c->bins && k > 0 && k <= 16 && c->bins_cap >= ((size_t)1 << (2 * k)), "counts_finish: no histogram for k=%d", k);
    KMAP_TRY(kmap_counts_bins_check(c, "counts_finish"));
    return kmap_counts_finish_hist(c, k, merge_revcom, n_uniq, as_stream(stream));
}

int kmap_counts_run_packed_dev(kmap_counts *c, const uint32_t *codes_dev, const uint16_t *inval_dev, int64_t n,
                               const int64_t *borders_dev, int64_t n_seq, int k, int dedupe_per_read, int merge_revcom,
                               int64_t *n_uniq, void *stream) {
    KMAP_REQUIRE(c, "counts_run_packed: null handle");
    KMAP_REQUIRE(k > 0 && k < 32, "counts_run_packed: k=%d out of range", k);
    KMAP_REQUIRE(n >= 0 && codes_dev && inval_dev, "counts_run_packed: bad input");
    hipStream_t st = as_stream(stream);
    if (k > 16) {   // sort path on a materialised hash array
        KMAP_REQUIRE(!dedupe_per_read || n_seq == 0 || borders_dev, "counts_run_packed: dedupe needs borders");
        void *hash = nullptr;
        KMAP_TRY(hash_and_dedupe(codes_dev, inval_dev, n, borders_dev, n_seq, k, dedupe_per_read, stream, &hash));
        return kmap_counts_run_hashes_dev(c, hash, n, k, merge_revcom, n_uniq, stream);
    }
    KMAP_TRY(kmap_counts_hist_packed_dev(c, codes_dev, inval_dev, n, borders_dev, n_seq, k, dedupe_per_read, stream));
    return kmap_counts_finish_hist(c, k, merge_revcom, n_uniq, st);
}

/* Key-space-sharded counting (include/kmap_hip.h; counts_internal.h: kmap_key_range): the slice [first_bin, first_bin + n_bins) -- by
 * POSITION in key order -- of the table kmap_counts_run_packed_dev would produce from the same reads, computed from the windows that
 * decide it alone.  Every rank of a multi-GPU run holds all reads and calls this with its own range; the shards, concatenated in rank
 * order, are the single-GPU table, and no table bytes are exchanged.  The histogram passes are those of a table of 2 n_bins (with
 * merge) or n_bins (without) entries over the windows that fall into it: they shrink with the number of ranks. */
int kmap_counts_run_packed_range_dev(kmap_counts *c, const uint32_t *codes_dev, const uint16_t *inval_dev, int64_t n,
                                     const int64_t *borders_dev, int64_t n_seq, int k, int dedupe_per_read, int merge_revcom,
                                     uint64_t first_bin, uint64_t n_bins, int64_t *n_uniq, void *stream) {
    KMAP_REQUIRE(c, "counts_run_packed_range: null handle");
    KMAP_REQUIRE(k >= 11 && k <= 16, "counts_run_packed_range: key ranges serve 11 <= k <= 16 (k=%d)", k);
    KMAP_REQUIRE(n >= 0 && codes_dev && inval_dev, "counts_run_packed_range: bad input");
    const uint64_t table = (uint64_t)1 << (2 * k);
    KMAP_REQUIRE(n_bins > 0 && first_bin < table && n_bins <= table - first_bin && first_bin % 8 == 0,
                 "counts_run_packed_range: range [%llu, +%llu) outside the 4^%d table or not 8-aligned", (unsigned long long)first_bin,
                 (unsigned long long)n_bins, k);
    hipStream_t st = as_stream(stream);
    // the virtual table: 4^vk bins with half = 4^vk / 2 >= n_bins (merge), or 4^vk >= n_bins (no merge); at least 4^10
    int vk = 10;
    while ((merge_revcom ? ((uint64_t)1 << (2 * vk - 1)) : ((uint64_t)1 << (2 * vk))) < n_bins) ++vk;
    uint32_t *skip = nullptr;
    if (dedupe_per_read) {
        KMAP_REQUIRE(n_seq == 0 || borders_dev, "counts_run_packed_range: dedupe needs borders");
        KMAP_TRY(dedupe_skip_bits(codes_dev, inval_dev, n, borders_dev, n_seq, k, st, &skip));
    }
    // no gain, or no room: the whole table by the usual passes, then the slice.  (vk > k: the range is more than half of the table;
    // vk == 16 with a range that reaches virtual key 0xFFFFFFFF = the invalid marker; small inputs; reads beyond the LDS dedupe's length.)
    const bool ranged = kmap_counts_part_applies(k, n) && vk <= k && !(dedupe_per_read && !skip) && n_bins <= 0xFFFFFFF0ull &&
                        !(vk == 16 && merge_revcom && n_bins > ((uint64_t)1 << 31) - 8);
    if (!ranged) {
        KMAP_TRY(kmap_counts_hist_packed_dev(c, codes_dev, inval_dev, n, borders_dev, n_seq, k, dedupe_per_read, stream));
        return kmap_counts_finish_hist_slice(c, k, merge_revcom, first_bin, n_bins, n_uniq, st);
    }
    kmap_key_range kr;
    kr.lo = (uint32_t)first_bin;
    kr.len = (uint32_t)n_bins;
    kr.half = merge_revcom ? (uint32_t)((uint64_t)1 << (2 * vk - 1)) : 0u;
    kr.sh = 32 - 2 * k;
    uint32_t *keys = nullptr;
    int64_t n_keys = 0;
    KMAP_TRY(kmap_counts_range_stage(codes_dev, inval_dev, skip, n, k, kr, &keys, &n_keys, st));
    KMAP_TRY(kmap_counts_part_hist_u32(c, keys, n_keys, vk, st));      // the table of the virtual keys: 4^vk bins, every bin written
    return kmap_counts_finish_key_range(c, k, kr, n_uniq, st);
}

}  // extern "C"
