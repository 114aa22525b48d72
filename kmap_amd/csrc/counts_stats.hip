// counts_stats.hip -- what find_motif reads off a finished (uniq, cnt) table of a counts handle (counts.hip): the total count, the
// top-k entries by count and the Hamming-ball mass of candidate consensuses (motif_discovery.py:648, :666-673).
#include <algorithm>
#include <vector>

#include "common.h"
#include "counts_internal.h"
#include "scan_util.h"

namespace {

constexpr int BLK = 256;

__global__ __launch_bounds__(BLK) void sum_counts_kernel(const uint32_t *__restrict__ cnt, int64_t n, int as_signed,
                                                         unsigned long long *__restrict__ total) {
    // the reference sums int32 counts as Python ints (find_motif :648): sign-extend for k < 16
    long long s = 0;
    const int64_t stride = (int64_t)gridDim.x * BLK;
    for (int64_t i = (int64_t)blockIdx.x * BLK + threadIdx.x; i < n; i += stride)
        s += as_signed ? (long long)(int32_t)cnt[i] : (long long)cnt[i];
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) atomicAdd(total, (unsigned long long)s);
}

// ---- top-k by count ---------------------------------------------------------------------------
// key = (count << 32) | ~index : the maximum key is the largest count, lowest index.  Every thread keeps its own top
// TK of a grid-strided slice, the block merges them by TK rounds of a block-wide max, the host merges the blocks.
constexpr int TK = 16;
__global__ __launch_bounds__(BLK) void topk_kernel(const uint32_t *__restrict__ cnt, int64_t n, int as_signed, int top_k,
                                                   unsigned long long *__restrict__ out) {
    __shared__ unsigned long long red[BLK];
    unsigned long long best[TK];
#pragma unroll
    for (int t = 0; t < TK; ++t) best[t] = 0;
    const int64_t stride = (int64_t)gridDim.x * BLK;
    for (int64_t i = (int64_t)blockIdx.x * BLK + threadIdx.x; i < n; i += stride) {
        const long long cv = as_signed ? (long long)(int32_t)cnt[i] : (long long)cnt[i];
        if (cv <= 0) continue;
        unsigned long long key = ((unsigned long long)cv << 32) | (0xFFFFFFFFull - (unsigned long long)i);
        if (key > best[top_k - 1]) {   // insertion into the descending list
#pragma unroll
            for (int t = 0; t < TK; ++t) {
                if (t < top_k && key > best[t]) {
                    const unsigned long long tmp = best[t];
                    best[t] = key;
                    key = tmp;
                }
            }
        }
    }
    int head = 0;
    for (int round = 0; round < top_k; ++round) {
        unsigned long long mine = 0;
#pragma unroll
        for (int t = 0; t < TK; ++t)
            if (t == head) mine = best[t];
        red[threadIdx.x] = (head < top_k) ? mine : 0;
        __syncthreads();
        for (int o = BLK / 2; o > 0; o >>= 1) {
            if ((int)threadIdx.x < o && red[threadIdx.x + o] > red[threadIdx.x]) red[threadIdx.x] = red[threadIdx.x + o];
            __syncthreads();
        }
        const unsigned long long win = red[0];
        __syncthreads();
        if (threadIdx.x == 0) out[(size_t)blockIdx.x * top_k + round] = win;
        if (win != 0 && mine == win) ++head;   // keys are unique (they embed the index)
    }
}

// ---- Hamming-ball mass -----------------------------------------------------------------------
struct CandTab {
    uint64_t fwd[16];
    uint64_t rc[16];
    int n;
};
template <typename H>
__global__ __launch_bounds__(BLK) void mass_kernel(const H *__restrict__ uniq, const uint32_t *__restrict__ cnt, int64_t n,
                                                   int k, CandTab t, int radius, int revcom, int as_signed,
                                                   unsigned long long *__restrict__ mass) {
    long long acc[16];
#pragma unroll
    for (int c = 0; c < 16; ++c) acc[c] = 0;
    const uint64_t m = low_mask<uint64_t>(k);
    const int64_t stride = (int64_t)gridDim.x * BLK;
    for (int64_t i = (int64_t)blockIdx.x * BLK + threadIdx.x; i < n; i += stride) {
        const uint64_t u = (uint64_t)uniq[i];
        const long long w = as_signed ? (long long)(int32_t)cnt[i] : (long long)cnt[i];
#pragma unroll
        for (int c = 0; c < 16; ++c) {
            if (c < t.n) {
                int d = popc2((u ^ t.fwd[c]) & m);
                if (revcom) {
                    int d2 = popc2((u ^ t.rc[c]) & m);
                    d = d2 < d ? d2 : d;
                }
                if (d <= radius) acc[c] += w;
            }
        }
    }
#pragma unroll
    for (int c = 0; c < 16; ++c) {
        if (c < t.n) {   // wave-uniform
            long long s = acc[c];
            for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o);
            if ((threadIdx.x & 63) == 0 && s != 0) atomicAdd(&mass[c], (unsigned long long)s);
        }
    }
}

}  // namespace

extern "C" {

int kmap_counts_total(kmap_counts *c, int64_t *total) {
    KMAP_REQUIRE(c && c->k > 0 && total, "counts_total: nothing counted yet");
    *total = 0;
    if (c->n_uniq == 0) return KMAP_OK;
    DevBuf t;
    KMAP_TRY(t.alloc(8));
    KMAP_CHECK_HIP(hipMemset(t.p, 0, 8));
    int64_t g = (c->n_uniq + BLK - 1) / BLK;
    if (g > 4096) g = 4096;
    sum_counts_kernel<<<(unsigned)g, BLK>>>(c->cnt, c->n_uniq, c->narrow, t.as<unsigned long long>());
    KMAP_CHECK_HIP(hipMemcpy(total, t.p, 8, hipMemcpyDeviceToHost));
    return KMAP_OK;
}

int kmap_counts_topk(kmap_counts *c, int top_k, int64_t *idx_out, uint64_t *kh_out, int64_t *cnt_out, int *n_found) {
    KMAP_REQUIRE(c && c->k > 0, "counts_topk: nothing counted yet");
    KMAP_REQUIRE(top_k > 0 && top_k <= TK && idx_out && kh_out && cnt_out && n_found, "counts_topk: bad arguments (top_k <= %d)", TK);
    KMAP_REQUIRE(c->n_uniq < ((int64_t)1 << 32), "counts_topk: more than 2^32 unique k-mers");
    *n_found = 0;
    if (c->n_uniq == 0) return KMAP_OK;
    int64_t g = (c->n_uniq + BLK - 1) / BLK;
    if (g > 1024) g = 1024;
    DevBuf out;
    KMAP_TRY(out.alloc((size_t)g * top_k * 8));
    topk_kernel<<<(unsigned)g, BLK>>>(c->cnt, c->n_uniq, c->narrow, top_k, out.as<unsigned long long>());
    KMAP_CHECK_HIP(hipGetLastError());
    std::vector<unsigned long long> keys((size_t)g * top_k);
    KMAP_CHECK_HIP(hipMemcpy(keys.data(), out.p, keys.size() * 8, hipMemcpyDeviceToHost));
    std::sort(keys.begin(), keys.end(), [](unsigned long long a, unsigned long long b) { return a > b; });
    int m = 0;
    for (; m < top_k && m < (int)keys.size() && keys[(size_t)m] != 0; ++m) {
        const int64_t idx = (int64_t)(0xFFFFFFFFull - (keys[(size_t)m] & 0xFFFFFFFFull));
        idx_out[m] = idx;
        cnt_out[m] = (int64_t)(keys[(size_t)m] >> 32);
        if (c->narrow) {
            uint32_t h = 0;
            KMAP_CHECK_HIP(hipMemcpy(&h, (const uint32_t *)c->uniq + idx, 4, hipMemcpyDeviceToHost));
            kh_out[m] = h;
        } else {
            KMAP_CHECK_HIP(hipMemcpy(&kh_out[m], (const uint64_t *)c->uniq + idx, 8, hipMemcpyDeviceToHost));
        }
    }
    *n_found = m;
    return KMAP_OK;
}

int kmap_counts_hamball_mass(kmap_counts *c, const uint64_t *cands, int n_cand, int radius, int revcom, double *mass_out) {
    KMAP_REQUIRE(c && c->k > 0, "hamball_mass: nothing counted yet");
    KMAP_REQUIRE(n_cand >= 0 && (n_cand == 0 || (cands && mass_out)), "hamball_mass: null pointer");
    DevBuf m;
    KMAP_TRY(m.alloc(16 * 8));
    for (int c0 = 0; c0 < n_cand; c0 += 16) {
        CandTab t;
        t.n = (n_cand - c0 < 16) ? n_cand - c0 : 16;
        for (int i = 0; i < t.n; ++i) {
            t.fwd[i] = cands[c0 + i];
            t.rc[i] = host_revcom(cands[c0 + i], c->k, c->narrow);
        }
        KMAP_CHECK_HIP(hipMemset(m.p, 0, 16 * 8));
        if (c->n_uniq > 0) {
            int64_t g = (c->n_uniq + BLK - 1) / BLK;
            if (g > 2048) g = 2048;
            if (c->narrow)
                mass_kernel<uint32_t><<<(unsigned)g, BLK>>>((const uint32_t *)c->uniq, c->cnt, c->n_uniq, c->k, t, radius,
                                                            revcom, 1, m.as<unsigned long long>());
            else
                mass_kernel<uint64_t><<<(unsigned)g, BLK>>>((const uint64_t *)c->uniq, c->cnt, c->n_uniq, c->k, t, radius,
                                                            revcom, 0, m.as<unsigned long long>());
            KMAP_CHECK_HIP(hipGetLastError());
        }
        long long host[16];
        KMAP_CHECK_HIP(hipMemcpy(host, m.p, 16 * 8, hipMemcpyDeviceToHost));
        for (int i = 0; i < t.n; ++i) mass_out[c0 + i] = (double)host[i];
    }
    return KMAP_OK;
}

}  // extern "C"
