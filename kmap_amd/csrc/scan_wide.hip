// scan_wide.hip -- the Hamming-ball mask's flag pass and the occurrence scan for k > 16, window by window on the 2-bit packed reads
// (layout: packed.hip; windows: packed_keys.h).  Nothing at k <= 16 runs these kernels: there both verbs are bit-sliced
// (bitslice.hip, the scan's per-read passes: scan_reads.hip).  The read geometry of the scan is scan_internal.h's, shared with
// those passes.  The dispatching entry points are in scan.hip.
#include "common.h"
#include "packed_keys.h"
#include "scan_internal.h"
#include "scan_util.h"

namespace {

constexpr int BLK = 256;

// ---- Hamming-ball mask on the packed stream (mask_input, kmer_count.py:580-610) ---------------------------------------
struct ConsTabP {
    uint64_t cons[32];
    int32_t radius[32];
    int n;
};
// hit16[g]: bit (15-i) set when the window at position 16g+i (invalid = all ones, compared as is) is within radius of
// any consensus.  Reads the CURRENT invalid mask; the coverage pass below writes it.
// k > 16 only: k <= 16 is tested bit-sliced on the reads' bit planes (bitslice.hip)
__global__ __launch_bounds__(BLK) void mask_flag_packed_kernel(const uint32_t *__restrict__ codes,
                                                               const uint16_t *__restrict__ inval, int64_t n, int k,
                                                               ConsTabP t, uint16_t *__restrict__ hit16) {
    const int64_t g = (int64_t)blockIdx.x * BLK + threadIdx.x;
    const int64_t n_groups = (n + 15) >> 4;
    if (g >= n_groups) return;
    const Win w = load_win(codes, inval, g);
    const uint64_t kmask = low_mask<uint64_t>(k);
    uint32_t hits = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        bool bad;
        const uint64_t h = win_hash<true>(w, i, k, kmask, bad);
        bool f = false;
        for (int c = 0; c < t.n; ++c) f |= (popc2((h ^ t.cons[c]) & kmask) <= t.radius[c]);
        if (16 * g + i >= n) f = false;           // positions past the end do not exist
        hits |= (uint32_t)f << (15 - i);
    }
    hit16[g] = (uint16_t)hits;
}

// ---- occurrence scan on the packed stream (get_motif_occurence, motif_discovery.py:1422-1477) ------------------------
constexpr int SC_WAVES = 4;
__device__ __forceinline__ int pos_dist(const uint32_t *__restrict__ codes, const uint16_t *__restrict__ inval, int64_t p,
                                        int k, uint64_t kmask, uint64_t cons, uint64_t rcc, int revcom) {
    const Win w = load_win(codes, inval, p >> 4);
    bool bad;
    const uint64_t h = win_hash<true>(w, (int)(p & 15), k, kmask, bad);
    int d = popc2((h ^ cons) & kmask);
    if (revcom) {
        const int d2 = popc2((h ^ rcc) & kmask);
        d = d2 < d ? d2 : d;
    }
    return d;
}
template <bool WRITE>
__global__ __launch_bounds__(KMAP_WAVE *SC_WAVES) void scan_packed_kernel(const uint32_t *__restrict__ codes,
                                                                           const uint16_t *__restrict__ inval, int64_t n,
                                                                           const int64_t *__restrict__ borders, int64_t n_seq,
                                                                           int k, uint64_t cons, uint64_t rcc, int radius,
                                                                           int revcom, int32_t *__restrict__ hits,
                                                                           int8_t *__restrict__ min_dist,
                                                                           const uint64_t *__restrict__ offs,
                                                                           int32_t *__restrict__ pos_out) {
    const int lane = threadIdx.x & 63;
    const int64_t s = (int64_t)blockIdx.x * SC_WAVES + (threadIdx.x >> 6);
    if (s >= n_seq) return;
    const ReadSlice rs = read_slice(borders, 0, 0, s, n, k);
    const int64_t st = rs.st, L = rs.L, stop = rs.stop;
    const uint64_t kmask = low_mask<uint64_t>(k);
    // the read's own end acts like a separator even if the caller's border does not sit on one
    constexpr int REG = 4;                       // distances kept in registers for reads up to 256 positions
    int dreg[REG];
    int best = 1 << 30;
#pragma unroll
    for (int r = 0; r < REG; ++r) {
        const int64_t p = (int64_t)r * 64 + lane;
        int d = 1 << 29;
        if (p < stop) {
            d = (p + k > L) ? popc2((kmask ^ cons) & kmask) : pos_dist(codes, inval, st + p, k, kmask, cons, rcc, revcom);
            if (p + k > L && revcom) { const int d2 = popc2((kmask ^ rcc) & kmask); d = d2 < d ? d2 : d; }
        }
        dreg[r] = d;
        if (d <= radius && d < best) best = d;
    }
    for (int64_t p = (int64_t)REG * 64 + lane; p < stop; p += 64) {
        int d = (p + k > L) ? popc2((kmask ^ cons) & kmask) : pos_dist(codes, inval, st + p, k, kmask, cons, rcc, revcom);
        if (p + k > L && revcom) { const int d2 = popc2((kmask ^ rcc) & kmask); d = d2 < d ? d2 : d; }
        if (d <= radius && d < best) best = d;
    }
    for (int o = 32; o > 0; o >>= 1) {
        const int v = __shfl_xor(best, o);
        best = v < best ? v : best;
    }
    int count = 0;
    uint64_t base = WRITE ? offs[s] : 0;
    if (best <= radius) {
        for (int64_t p0 = 0; p0 < stop; p0 += 64) {
            const int64_t p = p0 + lane;
            int d;
            if (p0 < (int64_t)REG * 64) d = dreg[p0 >> 6];
            else {
                d = 1 << 29;
                if (p < stop) {
                    d = (p + k > L) ? popc2((kmask ^ cons) & kmask) : pos_dist(codes, inval, st + p, k, kmask, cons, rcc, revcom);
                    if (p + k > L && revcom) { const int d2 = popc2((kmask ^ rcc) & kmask); d = d2 < d ? d2 : d; }
                }
            }
            const bool hit = (p < stop) && (d == best);
            const unsigned long long mask = __ballot(hit);
            if (WRITE && hit) pos_out[base + __popcll(mask & ((1ull << lane) - 1ull))] = (int32_t)p;
            const int c = __popcll(mask);
            count += c;
            base += c;
        }
    }
    if (!WRITE && lane == 0) {
        hits[s] = count;
        min_dist[s] = (int8_t)((best <= radius) ? best : -1);
    }
}


// ---- occurrence scan, flat formulation ---------------------------------------------------------------------------
// The wave-per-read kernel above spends its time on per-read latency chains (borders -> codes -> reduce -> ballot): 10^7
// waves of ~3 positions per lane.  Split instead into
// (k > 16 only: k <= 16 scans the bit-sliced hit words of bitslice.hip in scan_reads.hip.)
//   (1) a flat pass, thread per 16-position group, that stores the capped distance of EVERY window as a nibble
//       (d <= radius ? d : 15; 8 B per group = 0.5 B per position) -- independent of read borders because a window that
//       the scan may use (p < L-k+1) lies entirely inside its read;
//       plus the smallest nibble of every group as one byte;
//   (2) a thread-per-read pass: minimum over the read = its two boundary words (masked) and the group minima of the words
//       in between (consecutive threads read consecutive bytes); then the number of positions at that minimum, decoding
//       only the words whose group minimum equals it;
//   (3) after the scan of the counts, a thread-per-read pass that writes those positions in ascending order.
// Reads longer than FL_LONG positions are handled by their whole wave (64 words per step) inside (2) and (3).
// Needs radius <= 14; larger radii take the wave-per-read kernel.
constexpr int FL_TPB = 256;
constexpr int FL_LONG = 1024;
constexpr uint64_t NIB_ONES = 0x1111111111111111ull;

__device__ __forceinline__ int nib_min(uint64_t x) {
    // pairwise minimum of the 16 nibbles (SWAR: compare 8 nibble pairs held in separate bytes, then fold)
    int m = 15;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int v = (int)((x >> (4 * i)) & 15);
        m = v < m ? v : m;
    }
    return m;
}
__global__ __launch_bounds__(BLK) void scan_nibble_kernel(const uint32_t *__restrict__ codes, const uint16_t *__restrict__ inval,
                                                          int64_t n, int k, uint64_t cons, uint64_t rcc, int radius, int revcom,
                                                          uint64_t *__restrict__ nib, uint8_t *__restrict__ wmin) {
    const int64_t g = (int64_t)blockIdx.x * BLK + threadIdx.x;
    if (g >= ((n + 15) >> 4)) return;
    const Win w = load_win(codes, inval, g);
    const uint64_t kmask = low_mask<uint64_t>(k);
    uint64_t out = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        bool bad;
        const uint64_t h = win_hash<true>(w, i, k, kmask, bad);
        int d = popc2((h ^ cons) & kmask);
        if (revcom) {
            const int d2 = popc2((h ^ rcc) & kmask);
            d = d2 < d ? d2 : d;
        }
        out |= (uint64_t)(d <= radius ? d : 15) << (4 * i);
    }
    nib[g] = out;
    wmin[g] = (uint8_t)nib_min(out);   // smallest nibble of the word: the per-read passes skip words that cannot matter
}

// nibbles of word wi restricted to absolute positions [a, b): everything else reads as 15.  `src` is the nibble array
// shifted so that src[wi - wsh] is word wi (global array: wsh = 0; block-staged LDS copy: wsh = first staged word).
__device__ __forceinline__ uint64_t nib_load(const uint64_t *src, int64_t wsh, int64_t wi, int64_t a, int64_t b) {
    uint64_t x = src[wi - wsh];
    const int64_t w0 = wi << 4;
    if (a > w0) x |= (1ull << (4 * (int)(a - w0))) - 1ull;
    if (b < w0 + 16) x |= ~0ull << (4 * (int)(b - w0));
    return x;
}
// 16-bit mask (bit i = position i of the word) of the nibbles equal to v
__device__ __forceinline__ uint32_t nib_eq_mask(uint64_t x, int v) {
    uint64_t y = x ^ (NIB_ONES * (uint64_t)v);         // zero nibble <=> equal
    y |= y >> 1;
    y |= y >> 2;
    y = ~y & NIB_ONES;                                 // bit 4i set <=> nibble i equal
    y = (y | (y >> 3)) & 0x0303030303030303ull;        // gather: 2 bits per byte
    y = (y | (y >> 6)) & 0x000F000F000F000Full;        // 4 bits per 16
    y = (y | (y >> 12)) & 0x000000FF000000FFull;       // 8 bits per 32
    return (uint32_t)((y | (y >> 24)) & 0xFFFFull);
}

template <bool WRITE>
__global__ __launch_bounds__(FL_TPB) void scan_reads_kernel(const uint64_t *__restrict__ nib, int64_t n,
                                                            const int64_t *__restrict__ borders, int64_t n_seq, int k, int d_inv,
                                                            int radius, int32_t *__restrict__ hits, int8_t *__restrict__ min_dist,
                                                            const uint64_t *__restrict__ offs, int32_t *__restrict__ pos_out,
                                                            const uint8_t *__restrict__ wmin) {
    const int lane = threadIdx.x & 63;
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t st = 0, stop = 0;
    bool quirk = false;
    if (s < n_seq) {
        const ReadSlice rs = read_slice(borders, 0, 0, s, n, k);
        st = rs.st;
        stop = rs.stop;
        quirk = rs.quirk;                        // negative slice stop: every window runs off the read
    }
    int best = 15, count = 0;
    uint64_t base = 0;
    if (WRITE && s < n_seq) {
        count = hits[s];
        best = min_dist[s];
        base = offs[s];
        if (count == 0) stop = 0;                // nothing to write for this read
    }
    if (quirk) {
        if (!WRITE) {
            best = d_inv <= radius ? d_inv : 15;
            count = d_inv <= radius ? (int)stop : 0;
        } else {
            for (int64_t p = 0; p < stop; ++p) pos_out[base + p] = (int32_t)p;
        }
        stop = 0;
    }
    const bool is_long = stop > FL_LONG;
    if (stop > 0 && !is_long) {
        const int64_t a = st, b = st + stop;
        const int64_t w0 = a >> 4, w1 = (b - 1) >> 4;
        auto edge = [&](int64_t wi) -> uint64_t {            // boundary word: nibbles outside [a, b) read as 15
            uint64_t x = nib[wi];
            const int64_t p0 = wi << 4;
            if (a > p0) x |= (1ull << (4 * (int)(a - p0))) - 1ull;
            if (b < p0 + 16) x |= ~0ull << (4 * (int)(b - p0));
            return x;
        };
        // interior words are judged by their precomputed minimum (1 byte, consecutive threads read consecutive bytes);
        // only the two boundary words and the words that hold the read's minimum are decoded
        const uint64_t xa = edge(w0), xb = (w1 > w0) ? edge(w1) : ~0ull;
        if (!WRITE) {
            best = min(nib_min(xa), nib_min(xb));
            for (int64_t wi = w0 + 1; wi < w1; ++wi) best = min(best, (int)wmin[wi]);
            if (best < 15) {
                count = __builtin_popcount(nib_eq_mask(xa, best)) + __builtin_popcount(nib_eq_mask(xb, best));
                for (int64_t wi = w0 + 1; wi < w1; ++wi)
                    if (wmin[wi] == best) count += __builtin_popcount(nib_eq_mask(nib[wi], best));
            }
        } else {
            auto emit = [&](uint64_t x, int64_t wi) {
                uint32_t m = nib_eq_mask(x, best);
                while (m) {
                    const int i = __builtin_ctz(m);
                    m &= m - 1;
                    pos_out[base++] = (int32_t)((wi << 4) + i - st);
                }
            };
            emit(xa, w0);
            for (int64_t wi = w0 + 1; wi < w1; ++wi)
                if (wmin[wi] == best) emit(nib[wi], wi);
            if (w1 > w0) emit(xb, w1);
        }
    }
    // long reads: the whole wave works on one read at a time, 64 words per step
    unsigned long long todo = __ballot(is_long);
    while (todo) {
        const int src = __builtin_ctzll(todo);
        todo &= todo - 1;
        const int64_t a = __shfl(st, src), b = a + __shfl(stop, src);
        const int64_t w0 = a >> 4, w1 = (b - 1) >> 4;
        if (!WRITE) {
            int m = 15;
            for (int64_t wi = w0 + lane; wi <= w1; wi += 64) {
                const int v = nib_min(nib_load(nib, 0, wi, a, b));
                m = v < m ? v : m;
            }
            for (int o = 32; o > 0; o >>= 1) {
                const int v = __shfl_xor(m, o);
                m = v < m ? v : m;
            }
            int c = 0;
            if (m < 15)
                for (int64_t wi = w0 + lane; wi <= w1; wi += 64) c += __builtin_popcount(nib_eq_mask(nib_load(nib, 0, wi, a, b), m));
            for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
            if (lane == src) {
                best = m;
                count = c;
            }
        } else {
            const int bst = __shfl(best, src);
            uint64_t wbase = __shfl(base, src);
            for (int64_t c0 = w0; c0 <= w1; c0 += 64) {
                const int64_t wi = c0 + lane;
                uint32_t m = (wi <= w1) ? nib_eq_mask(nib_load(nib, 0, wi, a, b), bst) : 0u;
                const int c = __builtin_popcount(m);
                const int inc = wave_inclusive_scan(c);
                uint64_t at = wbase + (uint64_t)(inc - c);
                while (m) {
                    const int i = __builtin_ctz(m);
                    m &= m - 1;
                    pos_out[at++] = (int32_t)((wi << 4) + i - a);
                }
                wbase += (uint64_t)__shfl(inc, 63);
            }
        }
    }
    if (!WRITE && s < n_seq) {
        hits[s] = count;
        min_dist[s] = (int8_t)(best < 15 ? best : -1);
    }
}

}  // namespace

// all flag passes read the mask as it is on entry (the reference hashes once, kmer_count.py:605-607)
int kmap_wide_mask_flags(const uint32_t *codes_dev, const uint16_t *inval_dev, int64_t n, int k, const uint64_t *cons, const int32_t *radius,
                         int n_cons, uint16_t **hit_out, int64_t *stride_out, int *passes_out, hipStream_t st) {
    const int64_t ng = (n + 15) >> 4;
    const int batches = (n_cons + 31) / 32;
    uint16_t *hit = nullptr;
    const int64_t ngp = (ng + 7) & ~(int64_t)7;                   // per-batch stride: every batch's hit array 16-byte aligned
    KMAP_TRY(kmap_scratch((void **)&hit, (size_t)ngp * 2 * batches, st, KMAP_SLOT_A));
    for (int b = 0; b < batches; ++b) {
        ConsTabP t;
        t.n = (n_cons - 32 * b < 32) ? n_cons - 32 * b : 32;
        for (int c = 0; c < t.n; ++c) {
            t.cons[c] = cons[32 * b + c] & low_mask<uint64_t>(k);
            t.radius[c] = radius[32 * b + c];
        }
        mask_flag_packed_kernel<<<grid_for(ng, BLK), BLK, 0, st>>>(codes_dev, inval_dev, n, k, t, hit + (size_t)b * ngp);
    }
    *hit_out = hit;
    *stride_out = ngp;
    *passes_out = batches;
    return KMAP_OK;
}

int kmap_wide_scan_run(kmap_scan *s, const uint32_t *codes_dev, const uint16_t *inval_dev, int64_t n, const int64_t *borders_dev,
                       int64_t n_seq, int k, uint64_t c, uint64_t rcc, int radius, int revcom, int64_t *total_hits, hipStream_t st) {
    const bool flat = radius <= 14;                 // k > 16: nibble pass + thread-per-read passes; larger radii: wave per read
    const unsigned grid = (unsigned)((n_seq + SC_WAVES - 1) / SC_WAVES);
    const unsigned fgrid = (unsigned)((n_seq + FL_TPB - 1) / FL_TPB);
    uint64_t *nib = nullptr;
    uint8_t *wmin = nullptr;
    int d_inv = 0;
    if (flat) {
        const int64_t ng = (n + 15) >> 4;
        const size_t ngp = ((size_t)(ng ? ng : 1) + 15) & ~(size_t)15;
        KMAP_TRY(kmap_scratch((void **)&nib, ngp * 9, st, KMAP_SLOT_HASH));   // 8 B of nibbles + 1 B minimum per group
        wmin = reinterpret_cast<uint8_t *>(nib + ngp);
        if (ng) {
            scan_nibble_kernel<<<grid_for(ng, BLK), BLK, 0, st>>>(codes_dev, inval_dev, n, k, c, rcc, radius, revcom, nib, wmin);
        }
        d_inv = host_invalid_dist(c, rcc, k, revcom);
        scan_reads_kernel<false><<<fgrid, FL_TPB, 0, st>>>(nib, n, borders_dev, n_seq, k, d_inv, radius, s->hits, s->mind, nullptr, nullptr, wmin);
    } else {
        scan_packed_kernel<false><<<grid, KMAP_WAVE * SC_WAVES, 0, st>>>(codes_dev, inval_dev, n, borders_dev, n_seq, k, c, rcc,
                                                                         radius, revcom, s->hits, s->mind, nullptr, nullptr);
    }
    KMAP_TRY(exclusive_scan_u32(reinterpret_cast<const uint32_t *>(s->hits), n_seq, s->offs, st));
    uint64_t total = 0;
    KMAP_CHECK_HIP(hipMemcpyAsync(&total, s->offs + n_seq, 8, hipMemcpyDeviceToHost, st));
    KMAP_CHECK_HIP(hipStreamSynchronize(st));
    KMAP_TRY(kmap_scan_reserve_pos(s, total));
    if (total) {
        if (flat)
            scan_reads_kernel<true><<<fgrid, FL_TPB, 0, st>>>(nib, n, borders_dev, n_seq, k, d_inv, radius, s->hits, s->mind, s->offs, s->pos, wmin);
        else
            scan_packed_kernel<true><<<grid, KMAP_WAVE * SC_WAVES, 0, st>>>(codes_dev, inval_dev, n, borders_dev, n_seq, k, c, rcc,
                                                                            radius, revcom, s->hits, s->mind, s->offs, s->pos);
    }
    KMAP_CHECK_HIP(hipGetLastError());
    s->total = (int64_t)total;
    if (total_hits) *total_hits = (int64_t)total;
    return KMAP_OK;
}
