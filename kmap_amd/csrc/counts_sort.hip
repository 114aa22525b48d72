// counts_sort.hip -- k-mer counting for 17 <= k < 32, where a direct 4^k histogram is impossible: the counterpart of
// np.unique(return_counts=True) in count_uniq_hash (kmer_count.py:476-491) as an LSD radix sort of the valid uint64 hashes (the
// library's one sort, radix_sort.h) + run-length encoding, then the reverse-complement merge (kmer_count.py:643-685) by binary search
// in the sorted unique keys and an order-preserving compaction.  Off the headline path (the reference's default k range is 6..16).
//
// Invalid hashes (all ones) are dropped first (flag, scan, scatter); the sort then runs ceil(2k / 8) passes, one for every 8-bit digit
// of the 2k significant bits.
#include "counts_internal.h"
#include "radix_sort.h"

namespace {
constexpr int BLK = 256;

__device__ __forceinline__ int64_t lower_bound(const uint64_t *__restrict__ a, int64_t n, uint64_t v) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t m = (lo + hi) >> 1;
        if (a[m] < v) lo = m + 1;
        else hi = m;
    }
    return lo;
}

// flag[i] = 1 if entry i is emitted; okey/ocnt hold the emitted values (see bin_entry in counts.hip)
__global__ __launch_bounds__(BLK) void merge_decide_kernel(const uint64_t *__restrict__ uniq, const uint32_t *__restrict__ cnt,
                                                           int64_t n, int k, int merge, uint32_t *__restrict__ flag,
                                                           uint64_t *__restrict__ okey, uint32_t *__restrict__ ocnt) {
    const int64_t i = (int64_t)blockIdx.x * BLK + threadIdx.x;
    if (i >= n) return;
    const uint64_t x = uniq[i];
    uint32_t c = cnt[i];
    uint64_t key = x;
    uint32_t keep = 1;
    if (merge) {
        const uint64_t r = revcom_hash(x, k);
        if (r == x) {
            c = c + c;
        } else {
            const int64_t j = lower_bound(uniq, n, r);
            const bool present = (j < n && uniq[j] == r);
            if (present && x > r) keep = 0;
            else {
                key = x > r ? r : x;
                if (present) c += cnt[j];
            }
        }
    }
    flag[i] = keep;
    okey[i] = key;
    ocnt[i] = c;
}

// invalid hashes (all ones) out: flag, then compaction by the scanned flags
__global__ __launch_bounds__(BLK) void rs_flag_valid_kernel(const uint64_t *__restrict__ h, int64_t n, uint32_t *__restrict__ flag) {
    const int64_t i = (int64_t)blockIdx.x * BLK + threadIdx.x;
    if (i < n) flag[i] = h[i] != ~0ull;
}
__global__ __launch_bounds__(BLK) void rs_compact_kernel(const uint64_t *__restrict__ h, const uint32_t *__restrict__ flag,
                                                         const uint64_t *__restrict__ off, int64_t n, uint64_t *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * BLK + threadIdx.x;
    if (i < n && flag[i]) out[off[i]] = h[i];
}
// run-length encoding of sorted keys: flag = first of its run; start[run] = index of the run's first key
__global__ __launch_bounds__(BLK) void rle_flag_kernel(const uint64_t *__restrict__ keys, int64_t n, uint32_t *__restrict__ flag) {
    const int64_t i = (int64_t)blockIdx.x * BLK + threadIdx.x;
    if (i < n) flag[i] = (i == 0 || keys[i] != keys[i - 1]);
}
__global__ __launch_bounds__(BLK) void rle_emit_kernel(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ flag,
                                                       const uint64_t *__restrict__ off, int64_t n, uint64_t *__restrict__ uniq,
                                                       uint64_t *__restrict__ start) {
    const int64_t i = (int64_t)blockIdx.x * BLK + threadIdx.x;
    if (i < n && flag[i]) {
        uniq[off[i]] = keys[i];
        start[off[i]] = (uint64_t)i;
    }
}
__global__ __launch_bounds__(BLK) void rle_count_kernel(const uint64_t *__restrict__ start, int64_t runs, int64_t n, uint32_t *__restrict__ cnt) {
    const int64_t r = (int64_t)blockIdx.x * BLK + threadIdx.x;
    if (r < runs) cnt[r] = (uint32_t)((r + 1 < runs ? start[r + 1] : (uint64_t)n) - start[r]);
}

__global__ __launch_bounds__(BLK) void scatter_kernel(const uint32_t *__restrict__ flag, const uint64_t *__restrict__ off,
                                                      const uint64_t *__restrict__ key, const uint32_t *__restrict__ cnt,
                                                      int64_t n, uint64_t *__restrict__ okey, uint32_t *__restrict__ ocnt) {
    const int64_t i = (int64_t)blockIdx.x * BLK + threadIdx.x;
    if (i >= n || !flag[i]) return;
    okey[off[i]] = key[i];
    ocnt[off[i]] = cnt[i];
}
}  // namespace

int kmap_counts_sort_path(kmap_counts *c, const uint64_t *hash_dev, int64_t n, int k, int merge, int64_t *n_uniq,
                          hipStream_t st) {
    c->k = k;
    c->narrow = 0;
    c->n_uniq = 0;
    if (n_uniq) *n_uniq = 0;
    if (n == 0) return KMAP_OK;
    KMAP_REQUIRE(n < (int64_t)1 << 32, "counts (k >= 17): more than 2^32 positions per call are not supported");
    // ---- valid hashes only (np.unique result minus invalid, kmer_count.py:485-487)
    const unsigned gridn = (unsigned)((n + BLK - 1) / BLK);
    DevBuf flag, off, keys_a, keys_b, run_cnt, run_start, mkey, mcnt;
    KMAP_TRY(flag.alloc((size_t)n * 4));
    KMAP_TRY(off.alloc(((size_t)n + 1) * 8));
    rs_flag_valid_kernel<<<gridn, BLK, 0, st>>>(hash_dev, n, flag.as<uint32_t>());
    uint64_t n_valid = 0;
    KMAP_TRY(exclusive_scan_total(flag.as<uint32_t>(), n, off.as<uint64_t>(), &n_valid, st));
    if (n_valid == 0) return KMAP_OK;
    const int64_t nv = (int64_t)n_valid;
    KMAP_TRY(keys_a.alloc((size_t)nv * 8));
    KMAP_TRY(keys_b.alloc((size_t)nv * 8));
    rs_compact_kernel<<<gridn, BLK, 0, st>>>(hash_dev, flag.as<uint32_t>(), off.as<uint64_t>(), n, keys_a.as<uint64_t>());
    // ---- LSD radix sort over the 2 k significant bits
    RsBufs<1, false> ping{{keys_a.as<uint64_t>()}, nullptr}, pong{{keys_b.as<uint64_t>()}, nullptr};
    KMAP_TRY(radix_sort(ping, pong, nv, {low_mask<uint64_t>(k)}, st));
    KMAP_CHECK_HIP(hipStreamSynchronize(st));
    const uint64_t *sorted = ping.w[0];
    uint64_t *uniq = pong.w[0];                                           // the sort's other buffer, from here on the unique keys
    // ---- run-length encoding: unique keys (uniq) + counts (run_cnt)
    const unsigned gridv = (unsigned)((nv + BLK - 1) / BLK);
    rle_flag_kernel<<<gridv, BLK, 0, st>>>(sorted, nv, flag.as<uint32_t>());
    uint64_t runs64 = 0;
    KMAP_TRY(exclusive_scan_total(flag.as<uint32_t>(), nv, off.as<uint64_t>(), &runs64, st));
    const int64_t m = (int64_t)runs64;
    KMAP_TRY(run_cnt.alloc((size_t)m * 4));
    KMAP_TRY(run_start.alloc(((size_t)m + 1) * 8));
    rle_emit_kernel<<<gridv, BLK, 0, st>>>(sorted, flag.as<uint32_t>(), off.as<uint64_t>(), nv, uniq, run_start.as<uint64_t>());
    rle_count_kernel<<<(unsigned)((m + BLK - 1) / BLK), BLK, 0, st>>>(run_start.as<uint64_t>(), m, nv, run_cnt.as<uint32_t>());
    KMAP_CHECK_HIP(hipGetLastError());
    KMAP_CHECK_HIP(hipStreamSynchronize(st));
    flag.release();                                                       // sized for n; the merge needs m
    off.release();
    if (m == 0) return KMAP_OK;
    KMAP_TRY(flag.alloc((size_t)m * 4));
    KMAP_TRY(mkey.alloc((size_t)m * 8));
    KMAP_TRY(mcnt.alloc((size_t)m * 4));
    KMAP_TRY(off.alloc(((size_t)m + 1) * 8));
    const unsigned grid = (unsigned)((m + BLK - 1) / BLK);
    merge_decide_kernel<<<grid, BLK, 0, st>>>(uniq, run_cnt.as<uint32_t>(), m, k, merge, flag.as<uint32_t>(), mkey.as<uint64_t>(),
                                              mcnt.as<uint32_t>());
    uint64_t total = 0;
    KMAP_TRY(exclusive_scan_total(flag.as<uint32_t>(), m, off.as<uint64_t>(), &total, st));
    KMAP_TRY(kmap_counts_reserve_table(c, (size_t)total));
    scatter_kernel<<<grid, BLK, 0, st>>>(flag.as<uint32_t>(), off.as<uint64_t>(), mkey.as<uint64_t>(), mcnt.as<uint32_t>(), m,
                                         (uint64_t *)c->uniq, c->cnt);
    KMAP_CHECK_HIP(hipGetLastError());
    KMAP_CHECK_HIP(hipStreamSynchronize(st));
    c->n_uniq = (int64_t)total;
    if (n_uniq) *n_uniq = (int64_t)total;
    return KMAP_OK;
}
