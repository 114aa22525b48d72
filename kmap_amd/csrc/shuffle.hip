// shuffle.hip -- k-let-preserving shuffle of the packed reads (shuffle_reads): control reads for enrich_kmers
// and evaluate_pwm that keep every read's length, composition and (klet = 2) dinucleotide counts.
//
// A segment is a maximal run of valid positions of the array; invalid positions (N, separators) never move.  Every segment is
// shuffled on its own, by ONE lane, from a counter-based random stream keyed by (seed, array position of its first base): the
// output is a function of the input and the seed alone, whatever the launch shape.
//
//   * shuffle_starts_kernel<WRITE>: thread = four 16-position groups of the invalid mask.  The starts of a group are the valid bits
//     whose left neighbour is clear; a block counts them (prefix sum by shuffles, the waves' totals through LDS), takes its range
//     of the list with ONE atomic and writes the positions.  Run twice: once to size the list (and to count the valid bases), once
//     to fill it.  The list's order across blocks is whatever the atomics give; nothing depends on it.
//   * shuffle_lengths_kernel: lane = one segment, walks the mask from its start to the first invalid bit (the halo groups behind the
//     array end every walk), at most 2^21 positions.  Leaves the lengths and a flag "a segment is too long".
//   * shuffle_fill_kernel: thread = 16 bytes of the output = the unpacked input.  Invalid positions and the segments that come back
//     unchanged by definition are final here.
//   * shuffle_kernel<KLET>: lane = one segment.  Pass A streams the segment's bases from the packed codes and counts its bases
//     (klet 1) or its 16 dinucleotides (klet 2).  The counters are indexed by data, so they live in LDS -- word i of lane t at
//     [i][t]: a lane's words are all on bank t % 32, the 32 lanes of an access on 32 banks, no conflict whatever the data -- and
//     are updated by non-returning LDS adds.  klet 2 then draws the last-exit edges of the vertices other than the last base z:
//     one draw over the arborescences rooted at z, each weighted by the product of its edges' multiplicities (at most 16 of the 64
//     assignments of a successor to the three other bases are arborescences; which, depends on z alone: four constant masks).
//     Pass B walks: at base a the next base is drawn in proportion to what is left of a's row, the reserved edge goes last.
//     klet 1 is the same walk on one vertex.  The output is streamed: bytes up to the first 4-byte boundary inside the segment,
//     whole words, bytes again at the end -- no word is shared with a neighbouring segment's lane.
//     No loop's trip count depends on a draw: pass A and pass B take one step per base, the tree choice is straight-line code.
#include <algorithm>

#include "common.h"
#include "scan_util.h"

namespace {

constexpr int SH_TPB = 256;
constexpr int64_t SH_MAX_SEG = (1ll << 21) - 1;     // three counters' product and the sum of all tree weights stay below 2^63
constexpr uint64_t SH_GOLDEN = 0x9E3779B97F4A7C15ull;

__device__ __forceinline__ uint64_t mix64(uint64_t x) {      // splitmix64 finaliser (synth.hip's)
    x += SH_GOLDEN;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
// floor(h * bound / 2^64) for bound < 2^32
__device__ __forceinline__ uint32_t draw32(uint64_t h, uint32_t bound) {
    const uint64_t lo = (h & 0xFFFFFFFFull) * bound, hi = (h >> 32) * bound;
    return (uint32_t)((hi + (lo >> 32)) >> 32);
}

// bit c = t0 << 4 | t1 << 2 | t2 set when "the k-th base other than z (ascending) is followed by t_k" sends all three to z
constexpr uint64_t tree_mask(int z) {
    uint64_t m = 0;
    for (int c = 0; c < 64; ++c) {
        const int t[3] = {c >> 4, (c >> 2) & 3, c & 3};
        int nxt[4] = {0, 0, 0, 0};
        nxt[z] = z;
        for (int k = 0; k < 3; ++k) nxt[k + (k >= z ? 1 : 0)] = t[k];
        bool ok = true;
        for (int k = 0; k < 3; ++k) {
            int x = k + (k >= z ? 1 : 0);
            for (int hop = 0; hop < 3; ++hop) x = nxt[x];
            ok = ok && x == z;
        }
        if (ok) m |= 1ull << c;
    }
    return m;
}
constexpr int popcount64(uint64_t x) {
    int c = 0;
    for (; x; x &= x - 1) ++c;
    return c;
}
constexpr uint64_t SH_TREES[4] = {tree_mask(0), tree_mask(1), tree_mask(2), tree_mask(3)};
static_assert(popcount64(SH_TREES[0]) == 16 && popcount64(SH_TREES[1]) == 16 && popcount64(SH_TREES[2]) == 16 &&
                  popcount64(SH_TREES[3]) == 16, "4^(4-2) spanning trees per root");

// ---- pass 1: the segment starts ----------------------------------------------------------------------------------------------
// thread = SH_GPT consecutive groups; a block adds its count to counter[0] with ONE atomic, so that the single counter takes one
// atomic per 16384 positions (9.2 10^4 per pass at 10 M reads of 150 bases).  !WRITE also sums the valid bases into counter[1].
constexpr int SH_GPT = 4;
constexpr int SH_WAVES = SH_TPB / KMAP_WAVE;
template <bool WRITE>
__global__ __launch_bounds__(SH_TPB) void shuffle_starts_kernel(const uint16_t *__restrict__ inval, int64_t n_groups,
                                                                unsigned long long *__restrict__ counter, int64_t *__restrict__ starts) {
    __shared__ uint32_t wave_starts[SH_WAVES], wave_valid[SH_WAVES];
    __shared__ unsigned long long wave_base[SH_WAVES];
    const int64_t g0 = ((int64_t)blockIdx.x * SH_TPB + threadIdx.x) * SH_GPT;
    const int lane = threadIdx.x & (KMAP_WAVE - 1), wave = threadIdx.x >> 6;
    uint32_t s[SH_GPT];                               // starts of the groups, position i in bit 15 - i
    uint32_t c = 0, nv = 0;
    uint32_t prev = (g0 > 0 && g0 <= n_groups) ? (~(uint32_t)inval[g0 - 1] & 1u) : 0u;       // the position before the group
#pragma unroll
    for (int j = 0; j < SH_GPT; ++j) {
        s[j] = 0;
        if (g0 + j < n_groups) {
            const uint32_t v = ~(uint32_t)inval[g0 + j] & 0xFFFFu;
            s[j] = v & ~(((prev << 16) | v) >> 1);
            prev = v & 1u;
            nv += (uint32_t)__builtin_popcount(v);
        }
        c += (uint32_t)__builtin_popcount(s[j]);
    }
    const uint32_t incl = wave_inclusive_scan(c);
    if (!WRITE) nv = wave_sum(nv);
    if (lane == KMAP_WAVE - 1) wave_starts[wave] = incl;
    if (lane == 0) wave_valid[wave] = nv;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t total = 0, valid = 0;
        for (int w = 0; w < SH_WAVES; ++w) {
            total += wave_starts[w];
            valid += wave_valid[w];
        }
        unsigned long long base = total ? atomicAdd(&counter[0], (unsigned long long)total) : 0ull;
        if (!WRITE && valid) atomicAdd(&counter[1], (unsigned long long)valid);
        for (int w = 0; w < SH_WAVES; ++w) {
            wave_base[w] = base;
            base += wave_starts[w];
        }
    }
    if (!WRITE) return;
    __syncthreads();
    int64_t o = (int64_t)wave_base[wave] + (incl - c);
#pragma unroll
    for (int j = 0; j < SH_GPT; ++j) {
        uint32_t sj = s[j];
        while (sj) {                                  // at most 8 starts in 16 positions
            const int i = __builtin_clz(sj) - 16;
            starts[o++] = (g0 + j) * 16 + i;
            sj &= ~(0x8000u >> i);
        }
    }
}

// acc[2] |= 1 when a segment is longer than SH_MAX_SEG
__global__ __launch_bounds__(SH_TPB) void shuffle_lengths_kernel(const uint16_t *__restrict__ inval, const int64_t *__restrict__ starts,
                                                                 int64_t n_seg, int32_t *__restrict__ lens,
                                                                 unsigned long long *__restrict__ acc) {
    const int64_t s = (int64_t)blockIdx.x * SH_TPB + threadIdx.x;
    if (s >= n_seg) return;
    int64_t len = 0;
    {
        const int64_t p = starts[s];
        int64_t g = p >> 4;
        const int i = (int)(p & 15);
        uint32_t m = (uint32_t)inval[g] & (0xFFFFu >> i);            // invalid positions of the group from i on
        if (m) {
            len = __builtin_clz(m) - 16 - i;
        } else {
            len = 16 - i;
            while (len <= SH_MAX_SEG) {                              // ends at the halo groups at the latest
                m = inval[++g];
                if (m) {
                    len += __builtin_clz(m) - 16;
                    break;
                }
                len += 16;
            }
        }
        if (len > SH_MAX_SEG) {
            len = SH_MAX_SEG + 1;
            atomicOr(&acc[2], 1ull);
        }
        lens[s] = (int32_t)len;
    }
}

// ---- the output as the unpacked input ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SH_TPB) void shuffle_fill_kernel(const uint32_t *__restrict__ codes, const uint16_t *__restrict__ inval,
                                                              int64_t n, uint8_t *__restrict__ seq, int aligned) {
    const int64_t g = (int64_t)blockIdx.x * SH_TPB + threadIdx.x;
    const int64_t p0 = g * 16;
    if (p0 >= n) return;
    const uint32_t c = codes[g], m = inval[g];
    uint32_t w[4];
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        uint32_t x = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int i = 4 * d + b;
            const uint32_t v = ((m >> (15 - i)) & 1u) ? 255u : ((c >> (30 - 2 * i)) & 3u);
            x |= v << (8 * b);
        }
        w[d] = x;
    }
    if (p0 + 16 <= n && aligned) {
        *reinterpret_cast<uint4 *>(seq + p0) = make_uint4(w[0], w[1], w[2], w[3]);
    } else {
        for (int b = 0; b < 16 && p0 + b < n; ++b) seq[p0 + b] = (uint8_t)(w[b >> 2] >> (8 * (b & 3)));
    }
}

// ---- pass 2: lane = segment ------------------------------------------------------------------------------------------------------
struct BaseReader {                                    // the bases from array position p on, one at a time
    const uint32_t *__restrict__ codes;
    int64_t g;
    uint32_t w;
    int i;
    __device__ __forceinline__ BaseReader(const uint32_t *__restrict__ c, int64_t p) : codes(c), g(p >> 4), i((int)(p & 15)) {
        w = codes[g] << (2 * i);
    }
    __device__ __forceinline__ uint32_t next() {
        const uint32_t b = w >> 30;
        w <<= 2;
        if (++i == 16) {
            i = 0;
            w = codes[++g];                            // behind the segment's last group: a data or halo group, never used
        }
        return b;
    }
};
struct ByteWriter {                                    // the bytes from array position p on; words only inside [p, ...)
    uint8_t *__restrict__ out;
    int64_t p, word0;                                  // word0: first 4-byte boundary at or behind the start (never: byte stores only)
    uint32_t acc;
    __device__ __forceinline__ ByteWriter(uint8_t *__restrict__ o, int64_t start, bool words)
        : out(o), p(start), word0(words ? (start + 3) & ~(int64_t)3 : INT64_MAX), acc(0) {}
    __device__ __forceinline__ void put(uint32_t b) {
        if (p < word0) {
            out[p] = (uint8_t)b;
        } else {
            acc |= b << (8 * (int)(p & 3));
            if ((p & 3) == 3) {
                *reinterpret_cast<uint32_t *>(out + p - 3) = acc;
                acc = 0;
            }
        }
        ++p;
    }
    __device__ __forceinline__ void finish() {
        if (p < word0) return;
        const int r = (int)(p & 3);
        for (int k = 0; k < r; ++k) out[p - r + k] = (uint8_t)(acc >> (8 * k));
    }
};

typedef __attribute__((address_space(3))) uint32_t *sh_lds;
__device__ __forceinline__ void lds_add(uint32_t *w, uint32_t v) {
    (void)__hip_atomic_fetch_add(w, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);      // result unused: a non-returning ds_add
}
__device__ __forceinline__ uint32_t lds_get(uint32_t *w) {
    return __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

template <int KLET>
__global__ __launch_bounds__(SH_TPB) void shuffle_kernel(const uint32_t *__restrict__ codes, const int64_t *__restrict__ starts,
                                                         const int32_t *__restrict__ lens, int64_t n_seg, uint64_t seed,
                                                         uint8_t *__restrict__ out, int words) {
    constexpr int NC = KLET == 2 ? 16 : 4;
    __shared__ uint32_t cnt[NC * SH_TPB];              // counter i of thread t at [i][t]
    const int64_t s = (int64_t)blockIdx.x * SH_TPB + threadIdx.x;
    if (s >= n_seg) return;                            // nothing below talks to another lane
    const int64_t start = starts[s];
    const int len = lens[s];
    if (len <= (KLET == 2 ? 3 : 1)) return;            // unchanged by definition: the fill kernel wrote it
    uint32_t *my = cnt + threadIdx.x;
#pragma unroll
    for (int i = 0; i < NC; ++i) my[i * SH_TPB] = 0;
    // pass A: the counts
    BaseReader rd(codes, start);
    uint32_t first = rd.next(), z = first;
    if constexpr (KLET == 1) lds_add(&my[first * SH_TPB], 1u);
    for (int j = 1; j < len; ++j) {
        const uint32_t b = rd.next();
        lds_add(&my[(KLET == 2 ? z * 4 + b : b) * SH_TPB], 1u);
        z = b;
    }
    const uint64_t key = mix64(seed ^ mix64((uint64_t)start));       // draw i of the segment = mix64(key + i * SH_GOLDEN)
    uint32_t reserved = 0;                                            // klet 2: the last-exit successor of base v in bits 2v+1 : 2v
    if constexpr (KLET == 2) {
        uint32_t m[4][4];
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) m[a][b] = lds_get(&my[(a * 4 + b) * SH_TPB]);
        // W[k][t]: the weight of "v_k, the k-th base other than z, is followed last by t"; a base the segment does not hold points at z
        uint32_t W[3][4];
        bool present[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            uint32_t row[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) row[t] = (uint32_t)k >= z ? m[k + 1][t] : m[k][t];
            const uint32_t vk = (uint32_t)k + ((uint32_t)k >= z ? 1u : 0u);
            present[k] = (row[0] + row[1] + row[2] + row[3]) != 0;
#pragma unroll
            for (int t = 0; t < 4; ++t) W[k][t] = present[k] ? ((uint32_t)t == vk ? 0u : row[t]) : ((uint32_t)t == z ? 1u : 0u);
        }
        const uint64_t valid = z == 0 ? SH_TREES[0] : z == 1 ? SH_TREES[1] : z == 2 ? SH_TREES[2] : SH_TREES[3];
        // The trees in the order of (t0, t1, t2), t0 slowest, and ONE draw r below their total weight: the tree is the first whose
        // running sum exceeds r.  The sums nest -- S2[t0][t1] = sum over t2 of W2, P1[t0] = W0[t0] sum over t1 of W1[t1] S2[t0][t1] --
        // so t0, then t1, then t2 are found with the same r, lowered by what was passed: 28 products instead of 2 x 80.
        uint32_t S2[4][4];
#pragma unroll
        for (int t0 = 0; t0 < 4; ++t0)
#pragma unroll
            for (int t1 = 0; t1 < 4; ++t1) {
                uint32_t sum = 0;
#pragma unroll
                for (int t2 = 0; t2 < 4; ++t2) sum += ((valid >> (t0 << 4 | t1 << 2 | t2)) & 1ull) ? W[2][t2] : 0u;
                S2[t0][t1] = sum;
            }
        uint64_t P1[4];
#pragma unroll
        for (int t0 = 0; t0 < 4; ++t0) {
            uint64_t s1 = 0;
#pragma unroll
            for (int t1 = 0; t1 < 4; ++t1) s1 += (uint64_t)W[1][t1] * (uint64_t)S2[t0][t1];
            P1[t0] = s1 * (uint64_t)W[0][t0];
        }
        const uint64_t total = P1[0] + P1[1] + P1[2] + P1[3];        // > 0: the segment's own last exits are a tree
        uint64_t r = __umul64hi(mix64(key), total);                   // draw 0
        auto pick = [&r](uint64_t q0, uint64_t q1, uint64_t q2) -> uint32_t {      // r < q0 + q1 + q2 + q3
            const uint32_t t = (r >= q0 ? 1u : 0u) + (r >= q0 + q1 ? 1u : 0u) + (r >= q0 + q1 + q2 ? 1u : 0u);
            r -= t == 0 ? 0ull : t == 1 ? q0 : t == 2 ? q0 + q1 : q0 + q1 + q2;
            return t;
        };
        auto at = [](const uint32_t *x, uint32_t t) -> uint32_t { return t == 0 ? x[0] : t == 1 ? x[1] : t == 2 ? x[2] : x[3]; };
        const uint32_t s0 = pick(P1[0], P1[1], P1[2]);
        const uint32_t w0 = at(W[0], s0);
        uint64_t q[4];
#pragma unroll
        for (int t1 = 0; t1 < 4; ++t1) {
            const uint32_t col[4] = {S2[0][t1], S2[1][t1], S2[2][t1], S2[3][t1]};
            q[t1] = (uint64_t)w0 * (uint64_t)W[1][t1] * (uint64_t)at(col, s0);
        }
        const uint32_t s1 = pick(q[0], q[1], q[2]);
        const uint64_t w01 = (uint64_t)w0 * (uint64_t)at(W[1], s1);
#pragma unroll
        for (int t2 = 0; t2 < 4; ++t2) q[t2] = ((valid >> (s0 << 4 | s1 << 2 | (uint32_t)t2)) & 1ull) ? w01 * (uint64_t)W[2][t2] : 0ull;
        const uint32_t s2 = pick(q[0], q[1], q[2]);
        const uint32_t sel = s0 << 4 | s1 << 2 | s2;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const uint32_t vk = (uint32_t)k + ((uint32_t)k >= z ? 1u : 0u);
            const uint32_t tk = (sel >> (4 - 2 * k)) & 3u;
            if (present[k]) {
                reserved |= tk << (2 * vk);
                lds_add(&my[(vk * 4 + tk) * SH_TPB], 0xFFFFFFFFu);    // the reserved edge leaves its row
            }
        }
    }
    // pass B: the walk
    ByteWriter wr(out, start, words != 0);
    uint32_t a = 0;
    uint64_t ctr = key;
    int j = 0;
    if constexpr (KLET == 2) {
        wr.put(first);
        a = first;
        ctr += SH_GOLDEN;
        j = 1;
    }
    for (; j < len; ++j, ctr += SH_GOLDEN) {
        uint32_t *row = my + (KLET == 2 ? a * 4 * SH_TPB : 0);
        const uint32_t c0 = lds_get(row), c1 = lds_get(row + SH_TPB), c2 = lds_get(row + 2 * SH_TPB), c3 = lds_get(row + 3 * SH_TPB);
        const uint32_t left = c0 + c1 + c2 + c3;
        const uint32_t r = draw32(mix64(ctr), left);                  // draw j
        uint32_t b = (r >= c0 ? 1u : 0u) + (r >= c0 + c1 ? 1u : 0u) + (r >= c0 + c1 + c2 ? 1u : 0u);
        if (left) lds_add(row + b * SH_TPB, 0xFFFFFFFFu);
        else b = (reserved >> (2 * a)) & 3u;                          // klet 2 only: the row is empty, the reserved edge goes
        wr.put(b);
        if (KLET == 2) a = b;
    }
    wr.finish();
}

}  // namespace

extern "C" {

int kmap_shuffle_packed_dev(const uint32_t *codes_dev, const uint16_t *inval_dev, int64_t n, int klet, uint64_t seed,
                            uint8_t *seq_out_dev, int64_t *stats, void *stream) {
    KMAP_REQUIRE(klet == 1 || klet == 2, "shuffle: klet=%d, 1 or 2 expected", klet);
    KMAP_REQUIRE(n >= 0, "shuffle: negative size");
    if (stats) stats[0] = stats[1] = 0;
    if (n == 0) return KMAP_OK;
    KMAP_REQUIRE(codes_dev && inval_dev && seq_out_dev, "shuffle: null pointer");
    hipStream_t st = as_stream(stream);
    const int64_t n_groups = (n + 15) >> 4;
    unsigned long long *acc = nullptr;                 // segments, valid bases, "a segment is too long"
    KMAP_TRY(kmap_scratch((void **)&acc, 4 * 8, st, KMAP_SLOT_A));
    KMAP_CHECK_HIP(hipMemsetAsync(acc, 0, 4 * 8, st));
    shuffle_starts_kernel<false><<<grid_for(n_groups, SH_TPB * SH_GPT), SH_TPB, 0, st>>>(inval_dev, n_groups, acc, nullptr);
    KMAP_CHECK_HIP(hipGetLastError());
    unsigned long long host[4] = {0, 0, 0, 0};
    KMAP_CHECK_HIP(hipMemcpyAsync(host, acc, 16, hipMemcpyDeviceToHost, st));
    KMAP_CHECK_HIP(hipStreamSynchronize(st));
    const int64_t n_seg = (int64_t)host[0], n_valid = (int64_t)host[1];
    int64_t *starts = nullptr;
    int32_t *lens = nullptr;
    if (n_seg) {
        KMAP_TRY(kmap_scratch((void **)&starts, (size_t)n_seg * 8, st, KMAP_SLOT_B));
        KMAP_TRY(kmap_scratch((void **)&lens, (size_t)n_seg * 4, st, KMAP_SLOT_C));
        KMAP_CHECK_HIP(hipMemsetAsync(acc, 0, 4 * 8, st));
        shuffle_starts_kernel<true><<<grid_for(n_groups, SH_TPB * SH_GPT), SH_TPB, 0, st>>>(inval_dev, n_groups, acc, starts);
        shuffle_lengths_kernel<<<grid_for(n_seg, SH_TPB), SH_TPB, 0, st>>>(inval_dev, starts, n_seg, lens, acc);
        KMAP_CHECK_HIP(hipGetLastError());
        KMAP_CHECK_HIP(hipMemcpyAsync(host, acc, 4 * 8, hipMemcpyDeviceToHost, st));
        KMAP_CHECK_HIP(hipStreamSynchronize(st));
        if (host[2]) {
            kmap_set_error("shuffle: a run of more than 2^21 - 1 valid bases is not supported");
            return KMAP_E_UNSUP;
        }
    }
    const int aligned16 = ((uintptr_t)seq_out_dev % 16) == 0, aligned4 = ((uintptr_t)seq_out_dev % 4) == 0;
    shuffle_fill_kernel<<<grid_for(n_groups, SH_TPB), SH_TPB, 0, st>>>(codes_dev, inval_dev, n, seq_out_dev, aligned16);
    if (n_seg) {
        if (klet == 2)
            shuffle_kernel<2><<<grid_for(n_seg, SH_TPB), SH_TPB, 0, st>>>(codes_dev, starts, lens, n_seg, seed, seq_out_dev, aligned4);
        else
            shuffle_kernel<1><<<grid_for(n_seg, SH_TPB), SH_TPB, 0, st>>>(codes_dev, starts, lens, n_seg, seed, seq_out_dev, aligned4);
    }
    KMAP_CHECK_HIP(hipGetLastError());
    if (stats) {
        stats[0] = n_seg;
        stats[1] = n_valid;
    }
    return KMAP_OK;
}

}  // extern "C"
