// scan.hip -- the handle of the per-read motif occurrence scan ("Hamming-ball scan over reads", BASELINE config 5; replaces
// get_motif_occurence, reference motif_discovery.py:1422-1477): its result lists (reserve), their summary and the ways out of
// the device (fetch) -- and, because they fill that handle, the two dispatching entry points of the verbs that run on the packed
// reads: kmap_scan_run_packed_dev and kmap_mask_hamball_packed_dev check the arguments and hand over to bitslice.hip (k <= 16: the hit
// bits of every window; the scan's per-read passes on them are scan_reads.hip) or scan_wide.hip (k > 16); the mask's coverage pass, which both branches end with, is here too.
#include <algorithm>
#include <vector>

#include "common.h"

namespace {

constexpr int BLK = 256;

// ---- Hamming-ball mask (mask_input, kmer_count.py:580-610): hits -> invalid positions ------------------------------------------------
// position q becomes invalid when a hit starts in [q-k+1, q]; k <= 31 reaches at most two groups back
__device__ __forceinline__ uint32_t cover16(uint64_t h2, uint64_t h1, uint64_t h0, int k) {
    // 48-bit stream of hits: groups g-2, g-1, g (position 0 of g-2 in bit 47); cover = OR_{j=0}^{k-1} (s >> j) by doubling
    uint64_t cover = (h2 << 32) | (h1 << 16) | h0;
    int have = 1;
    while (have < k) {
        const int step = (have <= k - have) ? have : k - have;
        cover |= cover >> step;
        have += step;
    }
    return (uint32_t)(cover & 0xFFFFull);
}
// thread = four groups (one 8-byte load of hits, one of the mask, one store); the hit array of a consensus batch starts 8-byte
// aligned.  (One group per thread moved two bytes per lane and access: 0.42 ms for 0.57 GB at C3.)
__global__ __launch_bounds__(BLK) void mask_cover_packed_kernel(const uint16_t *__restrict__ hit16, int64_t n, int k,
                                                                uint16_t *__restrict__ inval) {
    const int64_t g0 = ((int64_t)blockIdx.x * BLK + threadIdx.x) * 4;
    const int64_t n_groups = (n + 15) >> 4;
    if (g0 >= n_groups) return;
    if (g0 + 4 <= n_groups) {
        const uint64_t hq = *reinterpret_cast<const uint64_t *>(hit16 + g0);
        const uint32_t hp = g0 ? *reinterpret_cast<const uint32_t *>(hit16 + g0 - 2) : 0u;   // groups g0 - 2 (low half), g0 - 1
        const uint64_t h[6] = {hp & 0xFFFFu, hp >> 16, hq & 0xFFFFull, (hq >> 16) & 0xFFFFull, (hq >> 32) & 0xFFFFull, hq >> 48};
        uint64_t add = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) add |= (uint64_t)cover16(h[j], h[j + 1], h[j + 2], k) << (16 * j);
        if (add) {
            uint64_t *p = reinterpret_cast<uint64_t *>(inval + g0);
            *p |= add;
        }
        return;
    }
    for (int64_t g = g0; g < n_groups; ++g) {
        const uint64_t h2 = (g >= 2) ? hit16[g - 2] : 0, h1 = (g >= 1) ? hit16[g - 1] : 0, h0 = hit16[g];
        const uint16_t add = (uint16_t)cover16(h2, h1, h0, k);
        if (add) inval[g] = (uint16_t)(inval[g] | add);
    }
}

// ---- the handle's lists ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void scan_summary_kernel(const int32_t *__restrict__ hits, int64_t n_seq,
                                                           unsigned long long *__restrict__ stat) {
    unsigned long long cnt = 0, mx = 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n_seq; i += (int64_t)gridDim.x * 256) {
        const int32_t h = hits[i];
        cnt += h > 0;
        mx = (unsigned long long)h > mx && h > 0 ? (unsigned long long)h : mx;
    }
    for (int o = 32; o; o >>= 1) {
        cnt += __shfl_down(cnt, o);
        const unsigned long long m2 = __shfl_down(mx, o);
        mx = m2 > mx ? m2 : mx;
    }
    __shared__ unsigned long long wc[4], wm[4];                          // one pair of global atomics per block: thousands of
    if ((threadIdx.x & 63) == 0) {                                        // same-address 64-bit atomics cost 200 us, not 20
        wc[threadIdx.x >> 6] = cnt;
        wm[threadIdx.x >> 6] = mx;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned long long c = (wc[0] + wc[1]) + (wc[2] + wc[3]);
        unsigned long long m = wm[0] > wm[1] ? wm[0] : wm[1];
        m = wm[2] > m ? wm[2] : m;
        m = wm[3] > m ? wm[3] : m;
        if (c) atomicAdd(&stat[0], c);
        if (m) atomicMax(&stat[1], m);
    }
}

// thread = 4 reads: int32 hit counts -> bytes (saturating)
__global__ __launch_bounds__(256) void narrow_hits_kernel(const int32_t *__restrict__ hits, int64_t n_seq, uint8_t *__restrict__ out) {
    const int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    for (int j = 0; j < 4; ++j)
        if (i + j < n_seq) {
            const int32_t h = hits[i + j];
            out[i + j] = (uint8_t)(h < 0 ? 0 : h > 255 ? 255 : h);
        }
}

}  // namespace

#include "scan_internal.h"

int kmap_scan_reserve(kmap_scan *s, int64_t n_seq) {
    if (s->cap_seq < n_seq) {
        void *ptrs[] = {s->hits, s->mind, s->offs};
        for (void *p : ptrs)
            if (p) KMAP_CHECK_HIP(hipFree(p));
        s->hits = nullptr; s->mind = nullptr; s->offs = nullptr; s->cap_seq = 0;
        KMAP_CHECK_HIP(hipMalloc((void **)&s->hits, (size_t)n_seq * 4));
        KMAP_CHECK_HIP(hipMalloc((void **)&s->mind, (size_t)n_seq));
        KMAP_CHECK_HIP(hipMalloc((void **)&s->offs, ((size_t)n_seq + 1) * 8 + 128));   // + slack: doubles as scratch of kmap_scan_summary / _fetch_stream_u8 (64 B header + n_seq bytes)
        s->cap_seq = n_seq;
    }
    return KMAP_OK;
}
int kmap_scan_reserve_pos(kmap_scan *s, uint64_t total) {
    if (s->cap_pos < (int64_t)total || !s->pos) {
        if (s->pos) KMAP_CHECK_HIP(hipFree(s->pos));
        s->pos = nullptr;
        s->cap_pos = 0;
        const size_t cap = total ? (size_t)total + (size_t)total / 8 : 1;
        KMAP_CHECK_HIP(hipMalloc((void **)&s->pos, cap * 4));
        s->cap_pos = (int64_t)cap;
    }
    return KMAP_OK;
}

extern "C" {

int kmap_scan_create(kmap_scan **s) {
    KMAP_REQUIRE(s, "scan_create: null");
    *s = new kmap_scan();
    return KMAP_OK;
}
int kmap_scan_destroy(kmap_scan *s) {
    if (!s) return KMAP_OK;
    void *ptrs[] = {s->hits, s->mind, s->offs, s->pos, s->score, s->strand};
    for (void *p : ptrs)
        if (p) (void)hipFree(p);
    delete s;
    return KMAP_OK;
}

// fetch of the last run's lists on a stream of the caller's (a worker thread's own non-blocking stream: the copies then neither
// wait for nor hold up the launching thread's null-stream work).  The lists must be complete: call kmap_scan_summary first
// (it synchronises behind the kernels that write them); the handle must not run again before this returns.
int kmap_scan_fetch_stream(kmap_scan *s, int32_t *hits_per_read, int32_t *positions, void *stream) {
    KMAP_REQUIRE(s, "scan_fetch_stream: null handle");
    hipStream_t st = as_stream(stream);
    if (s->n_seq && hits_per_read)
        KMAP_CHECK_HIP(hipMemcpyAsync(hits_per_read, s->hits, (size_t)s->n_seq * 4, hipMemcpyDeviceToHost, st));
    if (s->total && positions)
        KMAP_CHECK_HIP(hipMemcpyAsync(positions, s->pos, (size_t)s->total * 4, hipMemcpyDeviceToHost, st));
    KMAP_CHECK_HIP(hipStreamSynchronize(st));
    return KMAP_OK;
}

// device addresses of the last run's lists (valid until the handle's next run): a multi-GPU caller gathers them with a
// device collective instead of fetching, exchanging and re-uploading them
int kmap_scan_result_dev(kmap_scan *s, void **hits_dev, void **pos_dev, int64_t *n_seq, int64_t *total) {
    KMAP_REQUIRE(s && hits_dev && pos_dev, "scan_result_dev: null");
    *hits_dev = s->n_seq ? (void *)s->hits : nullptr;
    *pos_dev = s->total ? (void *)s->pos : nullptr;
    if (n_seq) *n_seq = s->n_seq;
    if (total) *total = s->total;
    return KMAP_OK;
}

// what gen_motif_occurence_file's caller needs of a hit list without fetching it: reads with >= 1 hit, largest hit count
int kmap_scan_summary(kmap_scan *s, int64_t *reads_with_hits, int32_t *max_hits, void *stream) {
    KMAP_REQUIRE(s && reads_with_hits && max_hits, "scan_summary: null");
    *reads_with_hits = 0;
    *max_hits = 0;
    if (s->n_seq == 0) return KMAP_OK;
    hipStream_t st = as_stream(stream);
    unsigned long long *stat = reinterpret_cast<unsigned long long *>(s->offs);   // offs is dead once the positions are written
    KMAP_CHECK_HIP(hipMemsetAsync(stat, 0, 16, st));
    scan_summary_kernel<<<(unsigned)std::min<int64_t>((s->n_seq + 2047) / 2048, 512), 256, 0, st>>>(s->hits, s->n_seq, stat);
    KMAP_CHECK_HIP(hipGetLastError());
    unsigned long long host[2] = {0, 0};
    KMAP_CHECK_HIP(hipMemcpyAsync(host, stat, 16, hipMemcpyDeviceToHost, st));
    KMAP_CHECK_HIP(hipStreamSynchronize(st));
    *reads_with_hits = (int64_t)host[0];
    *max_hits = (int32_t)host[1];
    return KMAP_OK;
}

// the same with the hit counts narrowed to bytes on the device first (staged in the handle's dead offset array): for lists
// whose kmap_scan_summary max_hits is <= 255 -- larger counts would saturate at 255
int kmap_scan_fetch_stream_u8(kmap_scan *s, uint8_t *hits_u8, int32_t *positions, void *stream) {
    KMAP_REQUIRE(s, "scan_fetch_stream_u8: null handle");
    hipStream_t st = as_stream(stream);
    if (s->n_seq && hits_u8) {
        uint8_t *stage = reinterpret_cast<uint8_t *>(s->offs) + 64;
        narrow_hits_kernel<<<(unsigned)((s->n_seq + 1023) / 1024), 256, 0, st>>>(s->hits, s->n_seq, stage);
        KMAP_CHECK_HIP(hipGetLastError());
        KMAP_CHECK_HIP(hipMemcpyAsync(hits_u8, stage, (size_t)s->n_seq, hipMemcpyDeviceToHost, st));
    }
    if (s->total && positions)
        KMAP_CHECK_HIP(hipMemcpyAsync(positions, s->pos, (size_t)s->total * 4, hipMemcpyDeviceToHost, st));
    KMAP_CHECK_HIP(hipStreamSynchronize(st));
    return KMAP_OK;
}

int kmap_scan_fetch(kmap_scan *s, int32_t *hits_per_read, int8_t *min_dist, int32_t *positions) {
    KMAP_REQUIRE(s, "scan_fetch: null handle");
    if (s->pwm && min_dist) {
        kmap_set_error("scan_fetch: a PWM scan has no per-read minimum distance");
        return KMAP_E_STATE;
    }
    KMAP_CHECK_HIP(hipDeviceSynchronize());
    if (s->n_seq) {
        if (hits_per_read) KMAP_CHECK_HIP(hipMemcpy(hits_per_read, s->hits, (size_t)s->n_seq * 4, hipMemcpyDeviceToHost));
        if (min_dist) KMAP_CHECK_HIP(hipMemcpy(min_dist, s->mind, (size_t)s->n_seq, hipMemcpyDeviceToHost));
    }
    if (s->total && positions) KMAP_CHECK_HIP(hipMemcpy(positions, s->pos, (size_t)s->total * 4, hipMemcpyDeviceToHost));
    return KMAP_OK;
}

// ---- the verbs on the packed reads ------------------------------------------------------------------------------------------------
// k <= 16: the bit-sliced formulation (bitslice.hip, scan_reads.hip) on the reads' bit planes; the per-window kernels of scan_wide.hip serve k > 16
static bool bitslice_on(int k) { return k <= 16; }

int kmap_mask_hamball_packed_dev(const uint32_t *codes_dev, uint16_t *inval_dev, int64_t n, int k, const uint64_t *cons,
                                 const int32_t *radius, int n_cons, const uint32_t *planes_dev, void *stream) {
    KMAP_REQUIRE(k > 0 && k < 32, "mask_hamball_packed: k=%d out of range", k);
    KMAP_REQUIRE(n_cons >= 0 && (n_cons == 0 || (cons && radius)), "mask_hamball_packed: null consensus list");
    if (n <= 0 || n_cons == 0) return KMAP_OK;
    KMAP_REQUIRE(codes_dev && inval_dev, "mask_hamball_packed: null pointer");
    KMAP_REQUIRE(k > 16 || planes_dev, "mask_hamball_packed: k <= 16 needs the bit planes (kmap_pack_planes_dev)");
    // a negative radius matches nothing (the reference's `ham_dist <= r`, kmer_count.py:594-603): such entries are dropped here --
    // the bit-sliced "count > r" test is built for r >= 0
    std::vector<uint64_t> cons_v;
    std::vector<int32_t> rad_v;
    for (int c = 0; c < n_cons; ++c)
        if (radius[c] >= 0) {
            cons_v.push_back(cons[c]);
            rad_v.push_back(radius[c]);
        }
    if (cons_v.empty()) return KMAP_OK;
    cons = cons_v.data();
    radius = rad_v.data();
    n_cons = (int)cons_v.size();
    hipStream_t st = as_stream(stream);
    const int64_t ng = (n + 15) >> 4;
    uint16_t *hit = nullptr;                                         // the flag passes' hit arrays, `stride` entries apart
    int64_t stride = 0;
    int passes = 0;
    if (bitslice_on(k)) {
        // 16 consensuses per flag pass, all passes on the mask as it is on entry
        passes = (n_cons + 15) / 16;
        stride = (ng + 9) & ~(int64_t)7;                            // even (the kernel stores group pairs) and 16-byte aligned batches
        KMAP_TRY(kmap_scratch((void **)&hit, (size_t)stride * 2 * passes, st, KMAP_SLOT_A));
        for (int b = 0; b < passes; ++b) {
            const int m = (n_cons - 16 * b < 16) ? n_cons - 16 * b : 16;
            KMAP_TRY(kmap_bitslice_hits(planes_dev, inval_dev, n, k, cons + 16 * b, radius + 16 * b, m, 0, hit + (size_t)b * stride, false, st));
        }
    } else {
        KMAP_TRY(kmap_wide_mask_flags(codes_dev, inval_dev, n, k, cons, radius, n_cons, &hit, &stride, &passes, st));
    }
    // every flag pass has read the mask as it was on entry (the reference hashes once, kmer_count.py:605-607); now the coverage
    // passes OR into it
    for (int b = 0; b < passes; ++b)
        mask_cover_packed_kernel<<<grid_for((ng + 3) / 4, BLK), BLK, 0, st>>>(hit + (size_t)b * stride, n, k, inval_dev);
    KMAP_CHECK_HIP(hipGetLastError());
    return KMAP_OK;
}

int kmap_scan_declare_uniform(kmap_scan *s, const int64_t *borders_dev, int64_t n_seq, int64_t read_len, int64_t stride, int *accepted, void *stream) {
    KMAP_REQUIRE(s && (n_seq == 0 || borders_dev), "scan_declare_uniform: null");
    return kmap_bitslice_declare_uniform(s, borders_dev, n_seq, read_len, stride, accepted, as_stream(stream));
}

int kmap_scan_run_packed_dev(kmap_scan *s, const uint32_t *codes_dev, const uint16_t *inval_dev, int64_t n,
                             const int64_t *borders_dev, int64_t n_seq, int k, uint64_t cons, int radius, int revcom,
                             int64_t *total_hits, const uint32_t *planes_dev, void *stream) {
    KMAP_REQUIRE(s, "scan_run_packed: null handle");
    KMAP_REQUIRE(k > 0 && k < 32, "scan_run_packed: k=%d out of range", k);
    KMAP_REQUIRE(n >= 0 && n_seq >= 0 && radius >= 0, "scan_run_packed: negative size");
    s->n_seq = n_seq;
    s->total = 0;
    s->pwm = 0;
    if (total_hits) *total_hits = 0;
    if (n_seq == 0) return KMAP_OK;
    KMAP_REQUIRE(codes_dev && inval_dev && borders_dev, "scan_run_packed: null pointer");
    KMAP_REQUIRE(k > 16 || planes_dev, "scan_run_packed: k <= 16 needs the bit planes (kmap_pack_planes_dev)");
    hipStream_t st = as_stream(stream);
    KMAP_TRY(kmap_scan_reserve(s, n_seq));
    const uint64_t c = cons & low_mask<uint64_t>(k);
    const uint64_t rcc = host_revcom(c, k, k < 16);
    if (bitslice_on(k)) {
        // hit bit per window (bit-sliced, 0.125 B per position written), then the per-read passes evaluate the few hits exactly
        const int64_t ng = (n + 15) >> 4;
        uint16_t *hit16 = nullptr;
        KMAP_TRY(kmap_scratch((void **)&hit16, (size_t)((ng + 9) & ~(int64_t)7) * 2, st, KMAP_SLOT_HASH));
        if (n > 0) KMAP_TRY(kmap_bitslice_hits(planes_dev, inval_dev, n, k, &c, &radius, 1, revcom, hit16, true, st));
        uint32_t *hit32 = reinterpret_cast<uint32_t *>(hit16);
        uint64_t total = 0;
        KMAP_TRY(kmap_bitslice_scan_reads_all(hit32, codes_dev, inval_dev, n, borders_dev, n_seq, k, c, revcom, radius, s, &total, st));
        s->total = (int64_t)total;
        if (total_hits) *total_hits = (int64_t)total;
        return KMAP_OK;
    }
    return kmap_wide_scan_run(s, codes_dev, inval_dev, n, borders_dev, n_seq, k, c, rcc, radius, revcom, total_hits, st);
}

}  // extern "C"
