// scan_reads.hip -- the per-read passes of the occurrence scan (get_motif_occurence, motif_discovery.py:1422-1477) for k <= 16, on
// the hit words of bitslice.hip (one bit per window: "within the radius on either strand").  Per read: the exact distance of its few
// hit windows -> the minimum, the number of hits at the minimum and their positions in read order.  One pass + a copy of the blocks'
// segments (scan_hits_reads_fused_kernel, scan_reorder_kernel) when the hits fit a temporary buffer, else count / scan / write
// (scan_hits_reads_kernel).  The read geometry (borders, slice stop) is scan_internal.h's, shared with the k > 16 kernels of
// scan_wide.hip; the dispatching entry point is in scan.hip.
#include <algorithm>

#include "common.h"
#include "scan_internal.h"
#include "scan_util.h"

namespace {

constexpr int HR_TPB = 256;
constexpr int HR_LONG = 1024;
// The per-read work in two phases.  COUNT: the exact distance of every hit window of the read -> minimum, number of hits at
// the minimum, and whether the hits lie at more than one distance ("mixed").  WRITE: the positions at the minimum, ascending,
// to pos_out[base ...] -- for a read that is not mixed simply the set bits of its range; only mixed reads evaluate distances
// again.  (Clearing the losing bits in place instead would break reads whose borders overlap -- the API allows them.)
// Reads longer than HR_LONG positions are walked by their whole wave, 64 hit words per step, in both phases.
constexpr int HR_CHUNK = 6;              // hit words fetched together (a 150-bp read spans 5 - 6, a 300-bp read 10 - 11)
constexpr int HR_MIXED = 0x40;           // flag bit in the min_dist byte between the two kernels of the two-pass form
struct HrCtx {
    const uint32_t *__restrict__ hit32;
    const uint32_t *__restrict__ codes;
    const uint16_t *__restrict__ inval;
    int64_t n;
    int64_t n_alloc;                     // groups the code / flag arrays hold (kmap_packed_groups(n))
    int k, revcom, d_inv, radius;
    uint32_t km, cons, rcc;
    int64_t uni_len = 0, uni_stride = 0;  // stride > 0: read s = [s * stride, s * stride + len) -- the borders need not be loaded
};
struct HrRead {
    int64_t st = 0, stop = 0;
    bool quirk = false;                  // negative slice stop: every window runs off the read (all-ones hash)
    int best = 127, count = 0;
    bool mixed = false;
};
__device__ __forceinline__ void hr_setup(const HrCtx &c, const int64_t *__restrict__ borders, int64_t s, int64_t n_seq, HrRead &r) {
    if (s < n_seq) {
        const ReadSlice rs = read_slice(borders, c.uni_len, c.uni_stride, s, c.n, c.k);   // uniform layout: verified on the device
        r.st = rs.st;
        r.stop = rs.stop;
        r.quirk = rs.quirk;
    }
}

// exact min(fwd, rc) distance of the window that starts i positions into the group of code word hi (lo: the next group's);
// fl: the invalid flags of that group and the two behind it.  CHECK_INVALID: a hit may be a window that touches an invalid
// position (only when the all-ones hash itself lies within the radius, d_inv <= r) -- it then has distance d_inv; otherwise
// every hit window is valid and the invalid mask need not be read.
template <bool CHECK_INVALID>
__device__ __forceinline__ int window_dist(const HrCtx &c, uint32_t hi, uint32_t lo, int i, const uint16_t *__restrict__ fl) {
    const uint32_t top = i ? __builtin_amdgcn_alignbit(hi, lo, 32 - 2 * i) : hi;
    uint32_t h = (top >> (32 - 2 * c.k)) & c.km;
    if (CHECK_INVALID) {
        const uint64_t m = ((uint64_t)fl[0] << 32) | ((uint64_t)fl[1] << 16) | fl[2];
        if (((m >> (48 - i - c.k)) & ((1ull << c.k) - 1ull)) != 0) h = c.km;
    }
    int d = popc2(h ^ c.cons);
    if (c.revcom) {
        const int d2 = popc2(h ^ c.rcc);
        d = d2 < d ? d2 : d;
    }
    return d;
}
// the window at absolute position p, code words from global memory
template <bool CHECK_INVALID>
__device__ __forceinline__ int hr_dist(const HrCtx &c, int64_t p) {
    const int64_t g = p >> 4;
    return window_dist<CHECK_INVALID>(c, c.codes[g], c.codes[g + 1], (int)(p & 15), c.inval + g);
}
// Word j of a hit-word stream (position p in bit 31 - (p & 31) of word p >> 5) restricted to the stream's bits [a_off, end):
// a_off < 32, the range ends in word nw - 1.  I: int relative to a short read's first word, int64_t for absolute words.
template <typename I>
__device__ __forceinline__ uint32_t edge_mask(I j, I nw, int a_off, I end) {
    uint32_t m = j < nw ? ~0u : 0u;
    if (j == 0) m &= ~0u >> a_off;
    if (j == nw - 1) m &= ~0u << (int)(32 * nw - end);
    return m;
}
// hit word wi (positions 32 wi .. 32 wi + 31, position i in bit 31 - i) restricted to absolute positions [a, b)
__device__ __forceinline__ uint32_t hr_mask(int64_t wi, int64_t a, int64_t b) {
    const int64_t w0 = a >> 5;
    return edge_mask<int64_t>(wi - w0, ((b - 1) >> 5) - w0 + 1, (int)(a & 31), b - (w0 << 5));
}

template <bool CHECK_INVALID>
__device__ __forceinline__ void hr_count(const HrCtx &c, HrRead &r) {
    const int lane = threadIdx.x & 63;
    int64_t stop = r.stop;
    if (r.quirk) {
        r.best = c.d_inv <= c.radius ? c.d_inv : 127;
        r.count = c.d_inv <= c.radius ? (int)stop : 0;
        stop = 0;
    }
    const bool is_long = stop > HR_LONG;
    if (stop > 0 && !is_long) {
        // 32-bit arithmetic relative to the read's first hit word (a short read spans at most 33 words).  This walk stands twice,
        // here and in hr_write: as ONE walker that takes the per-hit body as a callable (or hands out one hit per call) the
        // compiler kept more lane masks across the divergent loop, and the overflow fallback took 0.9 % longer (measured).
        const uint32_t *hw = c.hit32 + (r.st >> 5);
        const int a_off = (int)(r.st & 31), end = a_off + (int)stop;       // bit range [a_off, end) of the word stream
        const int nw = (end + 31) >> 5;
        const int64_t word0 = (r.st >> 5) << 5;                           // absolute position of bit 0 of the stream
        for (int j0 = 0; j0 < nw; j0 += HR_CHUNK) {
            uint32_t xs[HR_CHUNK];                                          // the chunk's words in ONE round trip, not one per word
#pragma unroll
            for (int t = 0; t < HR_CHUNK; ++t) xs[t] = hw[min(j0 + t, nw - 1)];
            // ONE loop over the chunk's hits (three 64-bit words, earliest position in the top bit): a wave runs it as often as its
            // busiest read has hits.  One loop per 32-bit word ran each of the six as often as ITS busiest lane had hits -- about
            // twice the divergent iterations, each with the round trip of hr_dist's code loads inside.
            uint64_t q[HR_CHUNK / 2];
#pragma unroll
            for (int t = 0; t < HR_CHUNK; ++t) {
                const uint32_t x = xs[t] & edge_mask(j0 + t, nw, a_off, end);
                if (t & 1) q[t >> 1] |= x;
                else q[t >> 1] = (uint64_t)x << 32;
            }
            static_assert(HR_CHUNK == 6, "three 64-bit words");
            for (;;) {
                const int sel = q[0] ? 0 : (q[1] ? 1 : 2);
                const uint64_t cur = q[0] ? q[0] : (q[1] ? q[1] : q[2]);
                if (!cur) break;
                const int tb = 63 - __builtin_clzll(cur);
                const uint64_t clr = ~(1ull << tb);
                q[0] &= sel == 0 ? clr : ~0ull;
                q[1] &= sel == 1 ? clr : ~0ull;
                q[2] &= sel == 2 ? clr : ~0ull;
                const int rel = 32 * j0 + 64 * sel + 63 - tb;
                const int d = hr_dist<CHECK_INVALID>(c, word0 + rel);
                if (d < r.best) { r.mixed = r.mixed || r.count > 0; r.best = d; r.count = 1; }
                else if (d == r.best) ++r.count;
                else r.mixed = true;
            }
        }
    }
    unsigned long long todo = __ballot(is_long);
    while (todo) {
        const int src = __builtin_ctzll(todo);
        todo &= todo - 1;
        const int64_t a = __shfl(r.st, src), b = a + __shfl(stop, src);
        const int64_t w0 = a >> 5, w1 = (b - 1) >> 5;
        int m = 127, cc = 0, total_c = 0;
        for (int64_t wi = w0 + lane; wi <= w1; wi += 64) {
            uint32_t x = c.hit32[wi] & hr_mask(wi, a, b);
            total_c += __builtin_popcount(x);
            while (x) {
                const int tb = 31 - __builtin_clz(x);
                x &= ~(1u << tb);
                const int d = hr_dist<CHECK_INVALID>(c, (wi << 5) + (31 - tb));
                if (d < m) { m = d; cc = 1; }
                else if (d == m) ++cc;
            }
        }
        int gm = m;
        for (int o = 32; o > 0; o >>= 1) {
            const int v = __shfl_xor(gm, o);
            gm = v < gm ? v : gm;
        }
        cc = (m == gm) ? cc : 0;
        for (int o = 32; o > 0; o >>= 1) {
            cc += __shfl_xor(cc, o);
            total_c += __shfl_xor(total_c, o);
        }
        if (lane == src) {
            r.best = gm;
            r.count = cc;
            r.mixed = total_c != cc;             // some hit of the read lies above its minimum
        }
    }
}
// cap: capacity of pos_out (writes beyond it are dropped; the caller re-runs with a larger buffer)
template <bool CHECK_INVALID>
__device__ __forceinline__ void hr_write(const HrCtx &c, const HrRead &r, uint64_t base, int32_t *__restrict__ pos_out, uint64_t cap) {
    const int lane = threadIdx.x & 63;
    int64_t stop = r.count ? r.stop : 0;                                   // nothing to write for a read without hits
    if (r.quirk) {
        for (int64_t p = 0; p < stop; ++p)
            if (base + p < cap) pos_out[base + p] = (int32_t)p;
        stop = 0;
    }
    const bool is_long = stop > HR_LONG;
    if (stop > 0 && !is_long) {
        const uint32_t *hw = c.hit32 + (r.st >> 5);
        const int a_off = (int)(r.st & 31), end = a_off + (int)stop;
        const int nw = (end + 31) >> 5;
        const int64_t word0 = (r.st >> 5) << 5;
        for (int j0 = 0; j0 < nw; j0 += HR_CHUNK) {
            uint32_t xs[HR_CHUNK];
#pragma unroll
            for (int t = 0; t < HR_CHUNK; ++t) xs[t] = hw[min(j0 + t, nw - 1)];
            uint64_t q[HR_CHUNK / 2];                                       // one loop over the chunk's hits, as in hr_count
#pragma unroll
            for (int t = 0; t < HR_CHUNK; ++t) {
                const uint32_t x = xs[t] & edge_mask(j0 + t, nw, a_off, end);
                if (t & 1) q[t >> 1] |= x;
                else q[t >> 1] = (uint64_t)x << 32;
            }
            for (;;) {                           // ascending positions: most significant bit first
                const int sel = q[0] ? 0 : (q[1] ? 1 : 2);
                const uint64_t cur = q[0] ? q[0] : (q[1] ? q[1] : q[2]);
                if (!cur) break;
                const int tb = 63 - __builtin_clzll(cur);
                const uint64_t clr = ~(1ull << tb);
                q[0] &= sel == 0 ? clr : ~0ull;
                q[1] &= sel == 1 ? clr : ~0ull;
                q[2] &= sel == 2 ? clr : ~0ull;
                const int rel = 32 * j0 + 64 * sel + 63 - tb;              // position relative to the stream's bit 0
                if (r.mixed && hr_dist<CHECK_INVALID>(c, word0 + rel) != r.best) continue;
                if (base < cap) pos_out[base] = (int32_t)(rel - a_off);
                ++base;
            }
        }
    }
    unsigned long long todo = __ballot(is_long);
    while (todo) {
        const int src = __builtin_ctzll(todo);
        todo &= todo - 1;
        const int64_t a = __shfl(r.st, src), b = a + __shfl(stop, src);
        const int64_t w0 = a >> 5, w1 = (b - 1) >> 5;
        uint64_t wbase = __shfl(base, src);
        const bool mx = __shfl((int)r.mixed, src) != 0;
        const int bst = __shfl(r.best, src);
        for (int64_t c0 = w0; c0 <= w1; c0 += 64) {
            const int64_t wi = c0 + lane;
            uint32_t keep = (wi <= w1) ? (c.hit32[wi] & hr_mask(wi, a, b)) : 0u;
            if (mx) {                            // drop the hits above the read's minimum
                uint32_t x = keep;
                while (x) {
                    const int tb = 31 - __builtin_clz(x);
                    x &= ~(1u << tb);
                    if (hr_dist<CHECK_INVALID>(c, (wi << 5) + (31 - tb)) != bst) keep &= ~(1u << tb);
                }
            }
            const int cnt = __builtin_popcount(keep);
            const int inc = wave_inclusive_scan(cnt);
            uint64_t at = wbase + (uint64_t)(inc - cnt);
            while (keep) {
                const int tb = 31 - __builtin_clz(keep);
                keep &= ~(1u << tb);
                if (at < cap) pos_out[at] = (int32_t)((wi << 5) + (31 - tb) - a);
                ++at;
            }
            wbase += (uint64_t)__shfl(inc, 63);
        }
    }
}

// two-pass form: count kernel (also: the block's hit total) -> exclusive scan of the 1 / 256 as many block totals (caller) ->
// write kernel (the read's offset = its block's offset + the prefix of the counts inside the block, recomputed from hits[])
template <bool WRITE, bool CHECK_INVALID>
__global__ __launch_bounds__(HR_TPB) void scan_hits_reads_kernel(HrCtx c, const int64_t *__restrict__ borders, int64_t n_seq,
                                                                 int32_t *__restrict__ hits, int8_t *__restrict__ min_dist,
                                                                 uint32_t *__restrict__ block_sums, const uint64_t *__restrict__ block_offs,
                                                                 int32_t *__restrict__ pos_out) {
    __shared__ unsigned int s_wave[HR_TPB / 64];
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    HrRead r;
    hr_setup(c, borders, s, n_seq, r);
    if (!WRITE) {
        hr_count<CHECK_INVALID>(c, r);
        if (s < n_seq) {
            hits[s] = r.count;
            min_dist[s] = (int8_t)(r.best <= c.radius ? (r.best | (r.mixed ? HR_MIXED : 0)) : -1);
        }
        unsigned int total;
        (void)block_exclusive_scan<HR_TPB / 64>((unsigned int)r.count, s_wave, &total);
        if (threadIdx.x == 0) block_sums[blockIdx.x] = total;
    } else {
        if (s < n_seq) {
            r.count = hits[s];
            if (r.count) {
                const int md = min_dist[s];
                r.mixed = (md & HR_MIXED) != 0;
                r.best = md & (HR_MIXED - 1);
                if (r.mixed) min_dist[s] = (int8_t)r.best;
            }
        }
        unsigned int total;                          // unused: asked for because the form with a total sums the lower waves in a fixed-count loop
        const unsigned int in_block = block_exclusive_scan<HR_TPB / 64>((unsigned int)r.count, s_wave, &total);
        hr_write<CHECK_INVALID>(c, r, block_offs[blockIdx.x] + in_block, pos_out, ~0ull);
    }
}

// One-pass form (the default): the per-read work is done ONCE.  A block counts its 256 reads, reserves room for all their positions
// with one fetch-add on a global cursor -- blocks therefore land in the buffer in the order they happen to finish -- and writes the
// positions right away (the hit words are still in L1; reads that are not "mixed" need no second distance evaluation).  What is
// left for after the scan of the block totals is a copy of every block's contiguous segment to its place in read order: 4 B per
// HIT instead of a second walk over every read's borders, hit words and codes (C5: 1.3 ms of 6.2).
// (A decoupled look-back over published block aggregates, which would keep read order in a single kernel, was built and measured
// in r03: 5.1 ms at C3 against 0.7 ms for the three launches -- on a part with eight L2s every agent-scope release / acquire of
// the status words is an L2 write-back / invalidate, paid once per block.  The unordered reservation needs no such hand-over.)
// Short reads in the one-pass form: all hit words of the read (up to HF_WORDS = 12: 352 positions) arrive in ONE round trip of six
// 8-byte loads, the masked words stay in registers for the write phase, and the first HF_KEEP positions at the running minimum are
// kept in registers while counting -- a read whose hits all lie at one distance (nearly all: one planted hit) is written from
// them without a second walk.  (r04 counters on the general form at the C5 shape: 1213 vector + 365 scalar instructions per 64
// reads at 57 % issue utilisation -- instruction-bound as much as latency-bound: two chunks of six word loads, mask building and
// the hit loop ran once for the counts and again for the positions.)
constexpr int HF_WORDS = 12, HF_KEEP = 4, HF_CURSORS = 64;
// (r04, second pass: 1010 vector + 490 scalar instructions per wave at C3, issue utilisation 0.85.  The hit loop popped "the earliest
// hit of six 64-bit words" through a chain of compares and selects per iteration -- and the compiler turned that loop, divergent
// through its `continue`s, into three nested ones glued together by dozens of mask operations.  Now: one plain loop per 64-bit
// word (ascending order as before), the distance from a per-read code pointer + 32-bit offsets, and the wave takes the form with
// NQ = 3 words (192 positions) when all its reads fit: half the loads, masks and loops for 150-bp reads.)
typedef uint32_t hf_u32x2 __attribute__((ext_vector_type(2), aligned(4)));
template <int NQ>
struct HfRead {
    uint64_t q[NQ];                      // the read's hit bits, position p of the word stream in bit 63 - (p & 63) of q[p >> 6]
    int keep[HF_KEEP];                   // first positions (relative to the read) at the minimum, ascending
    int a_off;                           // bit offset of the read's first position in the word stream
    uint32_t row;                        // index (dwords) into the block's code rows of the group holding the stream's bit 0
    const uint16_t *ib;                  // invalid flags of that group
};
template <int NQ>
constexpr int hf_row_words() { return 4 * NQ + 1; }   // code words of 64 NQ positions + the next group (a window runs into it)
__device__ __forceinline__ int hf_words(const HrRead &r) { return (int)(((r.st & 31) + r.stop + 31) >> 5); }
__device__ __forceinline__ bool hf_applies(const HrRead &r) {
    return !r.quirk && r.stop > 0 && r.stop <= 32 * HF_WORDS && hf_words(r) <= HF_WORDS;
}
// distance of the window `rel` positions into the word stream, on the read's code words in LDS.  (From global memory every
// iteration of the divergent hit loops began with a dependent load of two code words -- ~5 exposed round trips per wave, 75 % of
// the wave-cycles waiting.  The read's 13 / 25 code words now arrive in the same round trip as its hit words and are parked in a
// per-lane LDS row: odd row length, no bank conflicts between the lanes' rows.)
template <bool CHECK_INVALID>
__device__ __forceinline__ int hf_dist(const HrCtx &c, const uint32_t *code_rows, uint32_t row, const uint16_t *__restrict__ ib, int rel) {
    const uint32_t g = (uint32_t)rel >> 4;
    return window_dist<CHECK_INVALID>(c, code_rows[row + g], code_rows[row + g + 1], rel & 15, ib + g);
}
template <int NQ, bool CHECK_INVALID>
__device__ __forceinline__ void hf_count(const HrCtx &c, HrRead &r, HfRead<NQ> &f, bool active, uint32_t *code_rows) {
    constexpr int NG = hf_row_words<NQ>();
    f.a_off = (int)(r.st & 31);
    f.ib = c.inval + ((r.st >> 5) << 1);
    const int end = f.a_off + (int)r.stop;
    const int nw = active ? (end + 31) >> 5 : 0;
    const uint32_t *hw = c.hit32 + (r.st >> 5);
    uint32_t x[2 * NQ];
#pragma unroll
    for (int t = 0; t < NQ; ++t) {          // word pairs behind the read's last word repeat its last pair (inside the array)
        const int at = (2 * t < nw) ? 2 * t : (nw > 0 ? (nw - 1) & ~1 : 0);
        const hf_u32x2 v = *reinterpret_cast<const hf_u32x2 *>(hw + at);
        x[2 * t] = v.x;
        x[2 * t + 1] = v.y;
    }
    {   // the read's code words: NG consecutive groups from the one of the stream's bit 0, moved back where they would pass the end
        // of the array (the caller guarantees n_alloc >= NG); same round trip as the hit words above
        const int64_t g0 = active ? (r.st >> 5) << 1 : 0;
        const int64_t gb = g0 + NG <= c.n_alloc ? g0 : c.n_alloc - NG;
        typedef uint32_t hf_u32x4 __attribute__((ext_vector_type(4), aligned(4)));
        // a wave's rows start at the wave's share of the block's array (the waves of a block may run different NQ)
        const uint32_t row0 = (threadIdx.x >> 6) * (64u * hf_row_words<HF_WORDS / 2>()) + (threadIdx.x & 63u) * (uint32_t)NG;
        uint32_t *my = code_rows + row0;
        hf_u32x4 v[NQ];
#pragma unroll
        for (int t = 0; t < NQ; ++t) v[t] = *reinterpret_cast<const hf_u32x4 *>(c.codes + gb + 4 * t);
        const uint32_t last = c.codes[gb + 4 * NQ];
#pragma unroll
        for (int t = 0; t < NQ; ++t) {
            my[4 * t] = v[t].x; my[4 * t + 1] = v[t].y; my[4 * t + 2] = v[t].z; my[4 * t + 3] = v[t].w;
        }
        my[4 * NQ] = last;
        f.row = row0 + (uint32_t)(g0 - gb);
    }
#pragma unroll
    for (int j = 0; j < 2 * NQ; ++j) x[j] &= edge_mask(j, nw, f.a_off, end);
#pragma unroll
    for (int t = 0; t < NQ; ++t) f.q[t] = ((uint64_t)x[2 * t] << 32) | x[2 * t + 1];
#pragma unroll
    for (int t = 0; t < HF_KEEP; ++t) f.keep[t] = 0;
#pragma unroll
    for (int t = 0; t < NQ; ++t) {
        uint64_t w = f.q[t];
        while (w) {                         // a wave runs this as often as its busiest read has hits in this word
            const int lz = __builtin_clzll(w);
            w &= ~(0x8000000000000000ull >> lz);
            const int rel = 64 * t + lz;
            const int d = hf_dist<CHECK_INVALID>(c, code_rows, f.row, f.ib, rel);
            const int p = rel - f.a_off;
            if (d < r.best) {
                r.mixed = r.mixed || r.count > 0;
                r.best = d;
                r.count = 1;
                f.keep[0] = p;
            } else if (d == r.best) {
#pragma unroll
                for (int u = 1; u < HF_KEEP; ++u)
                    if (r.count == u) f.keep[u] = p;
                ++r.count;
            } else {
                r.mixed = true;
            }
        }
    }
}
template <int NQ, bool CHECK_INVALID>
__device__ __forceinline__ void hf_write(const HrCtx &c, const HrRead &r, const HfRead<NQ> &f, uint64_t base, int32_t *__restrict__ pos_out, uint64_t cap,
                                         const uint32_t *code_rows) {
    if (r.count == 0) return;
    if (r.count <= HF_KEEP) {               // the positions are in registers
#pragma unroll
        for (int t = 0; t < HF_KEEP; ++t)
            if (t < r.count && base + t < cap) pos_out[base + t] = f.keep[t];
        return;
    }
#pragma unroll
    for (int t = 0; t < NQ; ++t) {          // many hits (or several distances): walk the saved words again
        uint64_t w = f.q[t];
        while (w) {
            const int lz = __builtin_clzll(w);
            w &= ~(0x8000000000000000ull >> lz);
            const int rel = 64 * t + lz;
            if (r.mixed && hf_dist<CHECK_INVALID>(c, code_rows, f.row, f.ib, rel) != r.best) continue;
            if (base < cap) pos_out[base] = rel - f.a_off;
            ++base;
        }
    }
}

template <bool CHECK_INVALID>
__global__ __launch_bounds__(HR_TPB) void scan_hits_reads_fused_kernel(HrCtx c, const int64_t *__restrict__ borders, int64_t n_seq,
                                                                       int32_t *__restrict__ hits, int8_t *__restrict__ min_dist,
                                                                       uint32_t *__restrict__ block_sums, uint64_t *__restrict__ block_ubase,
                                                                       unsigned long long *__restrict__ cursor, int32_t *__restrict__ tmp_pos,
                                                                       uint64_t cap) {
    __shared__ unsigned int s_wave[HR_TPB / 64];
    __shared__ unsigned long long s_base;
    __shared__ uint32_t s_codes[HR_TPB * hf_row_words<HF_WORDS / 2>()];     // a row of code words per thread (25.6 KB)
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    HrRead r;
    hr_setup(c, borders, s, n_seq, r);
    const bool fast = hf_applies(r);
    const bool general = !fast && (r.stop > 0 || r.quirk);                  // long reads, the negative-slice quirk
    const bool narrow = __all(!fast || hf_words(r) <= 6);                   // wave-uniform: every short read of the wave fits three 64-bit words
    HfRead<3> f3;
    HfRead<HF_WORDS / 2> f6;
    if (narrow) hf_count<3, CHECK_INVALID>(c, r, f3, fast, s_codes);
    else hf_count<HF_WORDS / 2, CHECK_INVALID>(c, r, f6, fast, s_codes);
    if (__any(general)) {                                                   // wave-uniform: the general form for the lanes that need it
        HrRead g = r;
        if (!general) { g.stop = 0; g.quirk = false; }
        hr_count<CHECK_INVALID>(c, g);
        if (general) r = g;
    }
    if (s < n_seq) {
        hits[s] = r.count;
        min_dist[s] = (int8_t)(r.best <= c.radius ? r.best : -1);
    }
    unsigned int total;
    const unsigned int in_block = block_exclusive_scan<HR_TPB / 64>((unsigned int)r.count, s_wave, &total);
    if (threadIdx.x == 0) {
        // HF_CURSORS reservation counters, each with its own region of the buffer (a block takes counter blockIdx mod HF_CURSORS):
        // tens of thousands of device-scope fetch-adds on ONE address serialise at the memory side
        const unsigned cu = blockIdx.x % HF_CURSORS;
        const unsigned long long region = cap / HF_CURSORS;
        unsigned long long base = 0;
        if (total) {
            const unsigned long long at = atomicAdd(&cursor[cu], (unsigned long long)total);
            base = at + total <= region ? (unsigned long long)cu * region + at : cap;     // region full: dropped, and *overflow says so
            if (at + total > region) atomicMax(&cursor[HF_CURSORS], 1ull);
        }
        s_base = base;
        block_sums[blockIdx.x] = total;
        block_ubase[blockIdx.x] = base;
    }
    __syncthreads();
    const uint64_t base = s_base + in_block;
    if (fast) {                                                             // writes behind `cap` are dropped (the caller falls back)
        if (narrow) hf_write<3, CHECK_INVALID>(c, r, f3, base, tmp_pos, cap, s_codes);
        else hf_write<HF_WORDS / 2, CHECK_INVALID>(c, r, f6, base, tmp_pos, cap, s_codes);
    }
    if (__any(general)) {
        HrRead g = r;
        if (!general) { g.count = 0; g.stop = 0; g.quirk = false; }
        hr_write<CHECK_INVALID>(c, g, base, tmp_pos, cap);
    }
}
// segment of block b: tmp[ubase[b] .. + sums[b]) -> pos[offs[b] ..]; one wave per segment
__global__ __launch_bounds__(256) void scan_reorder_kernel(const int32_t *__restrict__ tmp, const uint64_t *__restrict__ ubase,
                                                           const uint64_t *__restrict__ offs, const uint32_t *__restrict__ sums, int64_t n_blocks,
                                                           int32_t *__restrict__ pos) {
    const int lane = threadIdx.x & 63;
    for (int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); b < n_blocks; b += (int64_t)gridDim.x * 4) {
        const uint32_t m = sums[b];
        const int32_t *src = tmp + ubase[b];
        int32_t *dst = pos + offs[b];
        for (uint32_t i = lane; i < m; i += 64) dst[i] = src[i];
    }
}

// flag[0] |= 1 when some read s is not [s * stride, s * stride + len)
__global__ __launch_bounds__(256) void borders_uniform_kernel(const int64_t *__restrict__ borders, int64_t n_seq, int64_t len, int64_t stride,
                                                              unsigned int *__restrict__ flag) {
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= n_seq) return;
    const bool bad = borders[2 * s] != s * stride || borders[2 * s + 1] != s * stride + len;
    if (bad && *reinterpret_cast<volatile unsigned int *>(flag) == 0u) atomicOr(flag, 1u);
}

// The two-pass form on s: count kernel (hits[], min_dist[] with the mixed flags, block totals) -> exclusive scan of the block
// totals -> write kernel.  s->offs doubles as [block offsets uint64 (nblk + 1) | block sums uint32 (nblk)]: n_seq + 1 uint64 are
// allocated.  total_out: read the total back and reserve s->pos for it in between (null: the caller has done both already).
int two_pass(const HrCtx &c, const int64_t *borders, int64_t n_seq, kmap_scan *s, uint64_t *total_out, hipStream_t st) {
    const unsigned grid = grid_for(n_seq, HR_TPB);
    const bool chk = c.d_inv <= c.radius;          // only then can a hit be a window that touches an invalid position
    uint32_t *bsums = reinterpret_cast<uint32_t *>(s->offs + (size_t)grid + 1);
    if (chk) scan_hits_reads_kernel<false, true><<<grid, HR_TPB, 0, st>>>(c, borders, n_seq, s->hits, s->mind, bsums, s->offs, nullptr);
    else scan_hits_reads_kernel<false, false><<<grid, HR_TPB, 0, st>>>(c, borders, n_seq, s->hits, s->mind, bsums, s->offs, nullptr);
    KMAP_CHECK_HIP(hipGetLastError());
    KMAP_TRY(exclusive_scan_u32(bsums, grid, s->offs, st));
    if (total_out) {
        KMAP_CHECK_HIP(hipMemcpyAsync(total_out, s->offs + grid, 8, hipMemcpyDeviceToHost, st));
        KMAP_CHECK_HIP(hipStreamSynchronize(st));
        KMAP_TRY(kmap_scan_reserve_pos(s, *total_out));
        if (*total_out == 0) return KMAP_OK;
    }
    if (chk) scan_hits_reads_kernel<true, true><<<grid, HR_TPB, 0, st>>>(c, borders, n_seq, s->hits, s->mind, bsums, s->offs, s->pos);
    else scan_hits_reads_kernel<true, false><<<grid, HR_TPB, 0, st>>>(c, borders, n_seq, s->hits, s->mind, bsums, s->offs, s->pos);
    KMAP_CHECK_HIP(hipGetLastError());
    return KMAP_OK;
}

}  // namespace

// The caller DECLARES that read s of `borders` is [s * stride, s * stride + len) (fixed-length reads: every BASELINE configuration);
// the declaration is verified on the device (one pass over the borders + a 4-byte read-back) and, if true, kept in the handle: the
// per-read kernels of later runs on the same border array take the borders from s instead of loading 16 bytes per read (0.8 GB of the
// pass's 6.7 GB at C5).  It holds until the handle sees other borders -- and must be renewed by the caller if the CONTENT of the array
// at that address changes (kmap_hip.h).  No automatic detection: a cache keyed by a device address could outlive the array it described.
int kmap_bitslice_declare_uniform(kmap_scan *s, const int64_t *borders, int64_t n_seq, int64_t len, int64_t stride, int *accepted, hipStream_t st) {
    s->geo_borders = nullptr; s->geo_n_seq = -1; s->geo_len = 0; s->geo_stride = 0;
    if (accepted) *accepted = 0;
    static const bool off = [] { const char *v = getenv("KMAP_SCAN_UNIFORM"); return v && v[0] == '0'; }();   // A/B switch: always load the borders
    if (off || n_seq < 1 || len < 0 || stride <= 0 || stride < len) return KMAP_OK;
    unsigned int *flag = nullptr;
    KMAP_TRY(kmap_scratch((void **)&flag, 64, st, KMAP_SLOT_D));
    KMAP_CHECK_HIP(hipMemsetAsync(flag, 0, 4, st));
    borders_uniform_kernel<<<(unsigned)((n_seq + 255) / 256), 256, 0, st>>>(borders, n_seq, len, stride, flag);
    unsigned int h = 1;
    KMAP_CHECK_HIP(hipMemcpyAsync(&h, flag, 4, hipMemcpyDeviceToHost, st));
    KMAP_CHECK_HIP(hipStreamSynchronize(st));
    if (h == 0) {
        s->geo_borders = borders; s->geo_n_seq = n_seq; s->geo_len = len; s->geo_stride = stride;
        if (accepted) *accepted = 1;
    }
    return KMAP_OK;
}
// the declared layout applies to this run's borders?
static void scan_geometry(const kmap_scan *s, const int64_t *borders, int64_t n_seq, HrCtx &c) {
    const bool same = s->geo_stride > 0 && s->geo_borders == borders && s->geo_n_seq == n_seq;
    c.uni_len = same ? s->geo_len : 0;
    c.uni_stride = same ? s->geo_stride : 0;
}

static HrCtx make_ctx(const uint32_t *hit32, const uint32_t *codes, const uint16_t *inval, int64_t n, int k, uint64_t cons, int revcom,
                      int radius) {
    HrCtx c;
    c.hit32 = hit32; c.codes = codes; c.inval = inval; c.n = n; c.n_alloc = kmap_packed_groups(n); c.k = k; c.revcom = revcom; c.radius = radius;
    c.km = low_mask<uint32_t>(k);
    c.cons = (uint32_t)cons & c.km;
    c.rcc = (uint32_t)host_revcom(c.cons, k, k < 16);
    c.d_inv = host_invalid_dist(c.cons, c.rcc, k, revcom);
    return c;
}

// The whole per-read part of the scan: hits[] / min_dist[] per read, positions in read order in s->pos, *total_out hits.
// One pass + a segment copy when the hits fit the temporary buffer (2 n_seq entries, at least 2^20), else the two-pass form.
int kmap_bitslice_scan_reads_all(const uint32_t *hit32, const uint32_t *codes, const uint16_t *inval, int64_t n, const int64_t *borders,
                                 int64_t n_seq, int k, uint64_t cons, int revcom, int radius, kmap_scan *s, uint64_t *total_out,
                                 hipStream_t st) {
    HrCtx c = make_ctx(hit32, codes, inval, n, k, cons, revcom, radius);
    scan_geometry(s, borders, n_seq, c);
    const int64_t nblk = (n_seq + HR_TPB - 1) / HR_TPB;
    // an input shorter than one row of code words: the two-pass form
    if (c.n_alloc < hf_row_words<HF_WORDS / 2>()) return two_pass(c, borders, n_seq, s, total_out, st);
    // s->offs ((n_seq + 1) uint64 + 128 B) holds: block offsets uint64[nblk + 1] | block sums uint32[nblk] (padded to 8 B) |
    // unordered block bases uint64[nblk] | cursor uint64
    uint64_t *boffs = s->offs;
    uint32_t *bsums = reinterpret_cast<uint32_t *>(s->offs + nblk + 1);
    uint64_t *ubase = s->offs + nblk + 1 + (nblk + 1) / 2;
    // the reservation counters (+ overflow flag) live in the scratch arena behind the temporary positions
    const size_t book = (size_t)(nblk + 1 + (nblk + 1) / 2 + nblk) * 8;
    KMAP_REQUIRE(book <= ((size_t)n_seq + 1) * 8 + 128, "scan: block bookkeeping does not fit");
    const uint64_t cap = ((uint64_t)std::max<int64_t>(2 * n_seq, (int64_t)1 << 20) + 2 * HF_CURSORS - 1) / (2 * HF_CURSORS) * (2 * HF_CURSORS);   // HF_CURSORS even regions
    int32_t *tmp = nullptr;
    KMAP_TRY(kmap_scratch((void **)&tmp, cap * 4 + (HF_CURSORS + 1) * 8, st, KMAP_SLOT_PART));
    unsigned long long *cursor = reinterpret_cast<unsigned long long *>(tmp + cap);       // cap is even: 8-byte aligned
    KMAP_CHECK_HIP(hipMemsetAsync(cursor, 0, (HF_CURSORS + 1) * 8, st));
    if (c.d_inv <= radius) scan_hits_reads_fused_kernel<true><<<(unsigned)nblk, HR_TPB, 0, st>>>(c, borders, n_seq, s->hits, s->mind, bsums, ubase, cursor, tmp, cap);
    else scan_hits_reads_fused_kernel<false><<<(unsigned)nblk, HR_TPB, 0, st>>>(c, borders, n_seq, s->hits, s->mind, bsums, ubase, cursor, tmp, cap);
    KMAP_CHECK_HIP(hipGetLastError());
    KMAP_TRY(exclusive_scan_u32(bsums, nblk, boffs, st));
    uint64_t total = 0;
    unsigned long long overflow = 0;
    KMAP_CHECK_HIP(hipMemcpyAsync(&total, boffs + nblk, 8, hipMemcpyDeviceToHost, st));
    KMAP_CHECK_HIP(hipMemcpyAsync(&overflow, cursor + HF_CURSORS, 8, hipMemcpyDeviceToHost, st));
    KMAP_CHECK_HIP(hipStreamSynchronize(st));
    KMAP_TRY(kmap_scan_reserve_pos(s, total));
    *total_out = total;
    if (total == 0) return KMAP_OK;
    if (!overflow) {
        const unsigned grid = (unsigned)std::min<int64_t>((nblk + 3) / 4, 8192);
        scan_reorder_kernel<<<grid, 256, 0, st>>>(tmp, ubase, boffs, bsums, nblk, s->pos);
        KMAP_CHECK_HIP(hipGetLastError());
        return KMAP_OK;
    }
    // more hits than a region of the temporary buffer holds (> 2 per read on average): count again with the mixed flags kept, then
    // write in order (s->pos is reserved and the total known)
    return two_pass(c, borders, n_seq, s, nullptr, st);
}
