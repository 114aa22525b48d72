// locations.hip -- the device part of `extract_motif_locations` (reference util.py:292-352): every consensus' hit windows merged per
// read, given a composite sort key and sorted, in one pipeline over all consensuses.
//
//   1. flags: position j of a cell (consensus c, row r) opens a merged interval iff it is the first of its cell or
//      pos[j-1] + len(c) < pos[j] (positions ascend inside a cell; windows that touch merge, like merge_intervals' prev_end < start)
//   2. exclusive scan of the flags + compaction: first[m] = index of the first position of interval m; its last position is
//      first[m + 1] - 1 (a new cell always opens an interval)
//   3. key kernel: (consensus, chrom rank, start, end - start, name key) packed LSB-first into 128 bits with widths the host chose;
//      the name key holds the decimal digits of seq_ind as (digit + 1) nibbles, most significant first, zero-padded, so that the
//      integer order of the keys is the string order of "motif_{i}_{seq_ind}".  The same pass ORs / ANDs all keys.
//   4. stable LSD radix sort of (key, interval index), 8-bit digits (radix_sort.h, two key words + payload); a digit that is the same
//      in every key (its bits of OR ^ AND are zero) is skipped
//   5. gather of the sorted (seq_ind, start, end) triples
#include <string.h>

#include <algorithm>
#include <vector>

#include "radix_sort.h"

namespace {
constexpr int BLK = 256;

__device__ __forceinline__ int find_cons(const int64_t *__restrict__ cb, int n_cons, int64_t j) {   // cb[c] <= j < cb[c + 1]
    int lo = 0, hi = n_cons;
    while (hi - lo > 1) {
        const int m = (lo + hi) >> 1;
        if (cb[m] <= j) lo = m;
        else hi = m;
    }
    return lo;
}

__global__ __launch_bounds__(BLK) void loc_flag_kernel(const int32_t *__restrict__ pos, int64_t n, const int64_t *__restrict__ cb, int n_cons,
                                                       const int32_t *__restrict__ clen, uint32_t *__restrict__ flag) {
    const int64_t j = (int64_t)blockIdx.x * BLK + threadIdx.x;
    if (j >= n) return;
    const int c = find_cons(cb, n_cons, j);
    flag[j] = (j == cb[c]) ? 1u : (uint32_t)((int64_t)pos[j - 1] + clen[c] < (int64_t)pos[j]);
}
// the first position of every non-empty cell opens an interval (runs after loc_flag_kernel on the same stream)
__global__ __launch_bounds__(BLK) void loc_head_kernel(const uint32_t *__restrict__ hits, const uint64_t *__restrict__ offs, int64_t n_cells,
                                                       uint32_t *__restrict__ flag) {
    const int64_t i = (int64_t)blockIdx.x * BLK + threadIdx.x;
    if (i < n_cells && hits[i]) flag[offs[i]] = 1u;
}
__global__ __launch_bounds__(BLK) void loc_first_kernel(const uint32_t *__restrict__ flag, const uint64_t *__restrict__ ioff, int64_t n,
                                                        uint32_t *__restrict__ first) {
    const int64_t j = (int64_t)blockIdx.x * BLK + threadIdx.x;
    if (j < n && flag[j]) first[ioff[j]] = (uint32_t)j;
}

struct KeyLayout {
    int name_digits;                       // nibbles of the name key
    int sh_len, sh_start, sh_chrom, sh_cons;   // bit offsets (the name key sits at bit 0)
};
__device__ __forceinline__ void put_field(uint64_t &lo, uint64_t &hi, uint64_t v, int sh) {   // v < 2^64, fits below bit 128
    if (sh < 64) {
        lo |= v << sh;
        if (sh > 0) hi |= v >> (64 - sh);
    } else {
        hi |= v << (sh - 64);
    }
}
__global__ __launch_bounds__(BLK) void loc_key_kernel(const uint32_t *__restrict__ first, int64_t m_total, int64_t n_pos,
                                                      const uint64_t *__restrict__ offs, int64_t n_cells, int64_t n_rows,
                                                      const int32_t *__restrict__ pos, const int32_t *__restrict__ clen,
                                                      const int64_t *__restrict__ seq_ind, const int64_t *__restrict__ bed_start,
                                                      const int32_t *__restrict__ chrom_rank, KeyLayout L, uint64_t *__restrict__ klo,
                                                      uint64_t *__restrict__ khi, uint32_t *__restrict__ idx, int64_t *__restrict__ v_row,
                                                      int64_t *__restrict__ v_start, int64_t *__restrict__ v_end,
                                                      unsigned long long *__restrict__ orand) {
    __shared__ uint64_t red[4][BLK / KMAP_WAVE];
    uint64_t o_lo = 0, o_hi = 0, a_lo = ~0ull, a_hi = ~0ull;
    for (int64_t m = (int64_t)blockIdx.x * BLK + threadIdx.x; m < m_total; m += (int64_t)gridDim.x * BLK) {
        const int64_t j0 = first[m], j1 = (m + 1 < m_total ? (int64_t)first[m + 1] : n_pos) - 1;
        int64_t lo = 0, hi = n_cells;                                  // the cell: last i with offs[i] <= j0 (it is non-empty)
        while (hi - lo > 1) {
            const int64_t mid = (lo + hi) >> 1;
            if ((int64_t)offs[mid] <= j0) lo = mid;
            else hi = mid;
        }
        const int c = (int)(lo / n_rows);
        const int64_t r = lo - (int64_t)c * n_rows;
        const int64_t s = seq_ind[r];
        const int64_t b = bed_start[s];
        const int64_t st = b + pos[j0], en = b + pos[j1] + clen[c];
        uint64_t name = 0;
        {
            uint64_t t = (uint64_t)s;
            int nd = 0;
            uint64_t rev = 0;                                          // digits, least significant first
            do {
                rev = (rev << 4) | (t % 10 + 1);
                t /= 10;
                ++nd;
            } while (t);
            for (int d = 0; d < nd; ++d) {                             // most significant digit into the highest nibble
                name |= (rev & 15ull) << (4 * (L.name_digits - 1 - d));
                rev >>= 4;
            }
        }
        uint64_t k_lo = 0, k_hi = 0;
        put_field(k_lo, k_hi, name, 0);
        put_field(k_lo, k_hi, (uint64_t)(en - st), L.sh_len);
        put_field(k_lo, k_hi, (uint64_t)st, L.sh_start);
        put_field(k_lo, k_hi, (uint64_t)chrom_rank[s], L.sh_chrom);
        put_field(k_lo, k_hi, (uint64_t)c, L.sh_cons);
        klo[m] = k_lo;
        khi[m] = k_hi;
        idx[m] = (uint32_t)m;
        v_row[m] = s;
        v_start[m] = st;
        v_end[m] = en;
        o_lo |= k_lo;
        o_hi |= k_hi;
        a_lo &= k_lo;
        a_hi &= k_hi;
    }
    for (int o = 32; o > 0; o >>= 1) {
        o_lo |= __shfl_xor(o_lo, o);
        o_hi |= __shfl_xor(o_hi, o);
        a_lo &= __shfl_xor(a_lo, o);
        a_hi &= __shfl_xor(a_hi, o);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        red[0][wave] = o_lo;
        red[1][wave] = o_hi;
        red[2][wave] = a_lo;
        red[3][wave] = a_hi;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < BLK / KMAP_WAVE; ++w) {
            red[0][0] |= red[0][w];
            red[1][0] |= red[1][w];
            red[2][0] &= red[2][w];
            red[3][0] &= red[3][w];
        }
        atomicOr(&orand[0], (unsigned long long)red[0][0]);
        atomicOr(&orand[1], (unsigned long long)red[1][0]);
        atomicAnd(&orand[2], (unsigned long long)red[2][0]);
        atomicAnd(&orand[3], (unsigned long long)red[3][0]);
    }
}

__global__ __launch_bounds__(BLK) void loc_gather_kernel(const uint32_t *__restrict__ idx, int64_t m_total, const int64_t *__restrict__ v_row,
                                                         const int64_t *__restrict__ v_start, const int64_t *__restrict__ v_end,
                                                         int64_t *__restrict__ o_row, int64_t *__restrict__ o_start, int64_t *__restrict__ o_end) {
    const int64_t t = (int64_t)blockIdx.x * BLK + threadIdx.x;
    if (t >= m_total) return;
    const uint32_t m = idx[t];
    o_row[t] = v_row[m];
    o_start[t] = v_start[m];
    o_end[t] = v_end[m];
}
__global__ void loc_bounds_kernel(const uint64_t *__restrict__ ioff, const int64_t *__restrict__ cb, int n, uint64_t *__restrict__ out) {
    const int c = (int)threadIdx.x + (int)blockIdx.x * (int)blockDim.x;
    if (c <= n) out[c] = ioff[cb[c]];
}

int bits_of(uint64_t v) { return v ? 64 - __builtin_clzll(v) : 0; }
}  // namespace

static int locations_impl(int64_t n_rows, int n_cons, const int32_t *const *hits, const int32_t *const *pos, const int64_t *n_pos,
                          const int32_t *cons_len, const int64_t *seq_ind, int64_t n_bed, const int64_t *bed_start,
                          const int32_t *chrom_rank, int n_chrom, int64_t cap, int64_t *out_row, int64_t *out_start, int64_t *out_end,
                          int64_t *n_per_cons, float *device_ms) {
    KMAP_REQUIRE(n_rows >= 0 && n_cons >= 0 && n_bed >= 0 && n_chrom >= 0 && cap >= 0, "locations: bad sizes");
    KMAP_REQUIRE(n_cons == 0 || (hits && pos && n_pos && cons_len && n_per_cons), "locations: null arrays");
    if (device_ms) *device_ms = 0.f;
    for (int c = 0; c < n_cons; ++c) n_per_cons[c] = 0;
    if (n_cons == 0 || n_rows == 0) return KMAP_OK;
    KMAP_REQUIRE(seq_ind && (n_bed == 0 || (bed_start && chrom_rank)), "locations: null arrays");
    // ---- host checks: everything the device indexes is in bounds, and the key fits in 128 bits
    std::vector<int64_t> cb((size_t)n_cons + 1, 0);
    int64_t max_pos = 0, max_s = 0, max_b = 0;
    int max_len = 0;
    for (int c = 0; c < n_cons; ++c) {
        KMAP_REQUIRE(hits[c] && (n_pos[c] == 0 || pos[c]) && n_pos[c] >= 0 && cons_len[c] >= 0, "locations: consensus %d: bad arrays", c);
        int64_t sum = 0;
        for (int64_t r = 0; r < n_rows; ++r) {
            KMAP_REQUIRE(hits[c][r] >= 0, "locations: negative hit count");
            sum += hits[c][r];
        }
        KMAP_REQUIRE(sum == n_pos[c], "locations: consensus %d: %lld hits, %lld positions", c, (long long)sum, (long long)n_pos[c]);
        for (int64_t j = 0; j < n_pos[c]; ++j) {
            KMAP_REQUIRE(pos[c][j] >= 0, "locations: negative location %d", pos[c][j]);
            max_pos = std::max<int64_t>(max_pos, pos[c][j]);
        }
        cb[(size_t)c + 1] = cb[(size_t)c] + n_pos[c];
        max_len = std::max(max_len, cons_len[c]);
    }
    const int64_t P = cb[(size_t)n_cons];
    if (P == 0) return KMAP_OK;
    KMAP_REQUIRE(P < ((int64_t)1 << 32), "locations: more than 2^32 - 1 hits are not supported");
    KMAP_REQUIRE(cap >= P && out_row && out_start && out_end, "locations: output capacity %lld < %lld hits", (long long)cap, (long long)P);
    for (int64_t r = 0; r < n_rows; ++r) {
        bool any = false;
        for (int c = 0; c < n_cons && !any; ++c) any = hits[c][r] > 0;
        if (!any) continue;
        const int64_t s = seq_ind[r];
        KMAP_REQUIRE(s >= 0 && s < n_bed, "locations: seq_ind %lld is outside the BED file (%lld rows)", (long long)s, (long long)n_bed);
        KMAP_REQUIRE(bed_start[s] >= 0, "locations: negative BED start %lld", (long long)bed_start[s]);
        KMAP_REQUIRE(chrom_rank[s] >= 0 && chrom_rank[s] < std::max(n_chrom, 1), "locations: bad chrom rank");
        max_s = std::max(max_s, s);
        max_b = std::max(max_b, bed_start[s]);
    }
    KMAP_REQUIRE(max_s < 10000000000ll, "locations: seq_ind %lld has more than 10 digits", (long long)max_s);
    KMAP_REQUIRE(max_b <= (INT64_MAX >> 2) - max_pos - max_len, "locations: coordinates too large");
    KeyLayout L;
    L.name_digits = std::max(1, (int)std::to_string(max_s).size());
    L.sh_len = 4 * L.name_digits;
    L.sh_start = L.sh_len + bits_of((uint64_t)(max_pos + max_len));
    L.sh_chrom = L.sh_start + bits_of((uint64_t)(max_b + max_pos));
    L.sh_cons = L.sh_chrom + bits_of((uint64_t)std::max(n_chrom - 1, 0));
    const int key_bits = L.sh_cons + bits_of((uint64_t)(n_cons - 1));
    if (key_bits > 128) {
        kmap_set_error("locations: the sort key needs %d bits (at most 128)", key_bits);
        return KMAP_E_UNSUP;
    }
    const int64_t n_cells = (int64_t)n_cons * n_rows;
    KMAP_REQUIRE(n_cells < ((int64_t)1 << 40), "locations: too many cells");

    // ---- device buffers
    hipStream_t st = nullptr;
    DevEvent ev0, ev1;
    KMAP_CHECK_HIP(ev0.create());
    KMAP_CHECK_HIP(ev1.create());
    KMAP_CHECK_HIP(hipEventRecord(ev0.e, st));
    DevBuf hits_d, offs, pos_d, flag, ioff, cb_d, bounds_d, clen_d, seq_d, bstart_d, crank_d;
    KMAP_TRY(hits_d.alloc((size_t)n_cells * 4));
    KMAP_TRY(offs.alloc(((size_t)n_cells + 1) * 8));
    KMAP_TRY(pos_d.alloc((size_t)P * 4));
    KMAP_TRY(flag.alloc((size_t)P * 4));
    KMAP_TRY(ioff.alloc(((size_t)P + 1) * 8));
    KMAP_TRY(cb_d.alloc(((size_t)n_cons + 1) * 8));
    KMAP_TRY(bounds_d.alloc(((size_t)n_cons + 1) * 8));
    KMAP_TRY(clen_d.alloc((size_t)n_cons * 4));
    KMAP_TRY(seq_d.alloc((size_t)n_rows * 8));
    KMAP_TRY(bstart_d.alloc((size_t)n_bed * 8));
    KMAP_TRY(crank_d.alloc((size_t)n_bed * 4));
    for (int c = 0; c < n_cons; ++c) {
        KMAP_CHECK_HIP(hipMemcpyAsync(hits_d.as<uint32_t>() + (size_t)c * n_rows, hits[c], (size_t)n_rows * 4, hipMemcpyHostToDevice, st));
        if (n_pos[c])
            KMAP_CHECK_HIP(hipMemcpyAsync(pos_d.as<int32_t>() + cb[(size_t)c], pos[c], (size_t)n_pos[c] * 4, hipMemcpyHostToDevice, st));
    }
    KMAP_CHECK_HIP(hipMemcpyAsync(cb_d.p, cb.data(), ((size_t)n_cons + 1) * 8, hipMemcpyHostToDevice, st));
    KMAP_CHECK_HIP(hipMemcpyAsync(clen_d.p, cons_len, (size_t)n_cons * 4, hipMemcpyHostToDevice, st));
    KMAP_CHECK_HIP(hipMemcpyAsync(seq_d.p, seq_ind, (size_t)n_rows * 8, hipMemcpyHostToDevice, st));
    if (n_bed) {
        KMAP_CHECK_HIP(hipMemcpyAsync(bstart_d.p, bed_start, (size_t)n_bed * 8, hipMemcpyHostToDevice, st));
        KMAP_CHECK_HIP(hipMemcpyAsync(crank_d.p, chrom_rank, (size_t)n_bed * 4, hipMemcpyHostToDevice, st));
    }
    // ---- 1-2: interval starts
    KMAP_TRY(exclusive_scan_u32(hits_d.as<uint32_t>(), n_cells, offs.as<uint64_t>(), st));
    const unsigned gp = (unsigned)((P + BLK - 1) / BLK);
    loc_flag_kernel<<<gp, BLK, 0, st>>>(pos_d.as<int32_t>(), P, cb_d.as<int64_t>(), n_cons, clen_d.as<int32_t>(), flag.as<uint32_t>());
    loc_head_kernel<<<(unsigned)((n_cells + BLK - 1) / BLK), BLK, 0, st>>>(hits_d.as<uint32_t>(), offs.as<uint64_t>(), n_cells,
                                                                           flag.as<uint32_t>());
    KMAP_TRY(exclusive_scan_u32(flag.as<uint32_t>(), P, ioff.as<uint64_t>(), st));
    loc_bounds_kernel<<<(unsigned)((n_cons + 1 + 63) / 64), 64, 0, st>>>(ioff.as<uint64_t>(), cb_d.as<int64_t>(), n_cons,
                                                                         bounds_d.as<uint64_t>());
    std::vector<uint64_t> bounds((size_t)n_cons + 1);
    KMAP_CHECK_HIP(hipMemcpyAsync(bounds.data(), bounds_d.p, ((size_t)n_cons + 1) * 8, hipMemcpyDeviceToHost, st));
    KMAP_CHECK_HIP(hipStreamSynchronize(st));
    KMAP_CHECK_HIP(hipGetLastError());
    const int64_t M = (int64_t)bounds[(size_t)n_cons];
    DevBuf first;
    KMAP_TRY(first.alloc((size_t)M * 4));
    loc_first_kernel<<<gp, BLK, 0, st>>>(flag.as<uint32_t>(), ioff.as<uint64_t>(), P, first.as<uint32_t>());
    // ---- 3: keys
    DevBuf klo, khi, klo2, khi2, idx, idx2, v_row, v_start, v_end, orand;
    KMAP_TRY(klo.alloc((size_t)M * 8));
    KMAP_TRY(khi.alloc((size_t)M * 8));
    KMAP_TRY(klo2.alloc((size_t)M * 8));
    KMAP_TRY(khi2.alloc((size_t)M * 8));
    KMAP_TRY(idx.alloc((size_t)M * 4));
    KMAP_TRY(idx2.alloc((size_t)M * 4));
    KMAP_TRY(v_row.alloc((size_t)M * 8));
    KMAP_TRY(v_start.alloc((size_t)M * 8));
    KMAP_TRY(v_end.alloc((size_t)M * 8));
    KMAP_TRY(orand.alloc(32));
    KMAP_CHECK_HIP(hipMemsetAsync(orand.p, 0, 16, st));
    KMAP_CHECK_HIP(hipMemsetAsync(orand.as<unsigned long long>() + 2, 0xff, 16, st));
    const unsigned gk = (unsigned)std::min<int64_t>((M + BLK - 1) / BLK, 4096);
    loc_key_kernel<<<gk, BLK, 0, st>>>(first.as<uint32_t>(), M, P, offs.as<uint64_t>(), n_cells, n_rows, pos_d.as<int32_t>(),
                                       clen_d.as<int32_t>(), seq_d.as<int64_t>(), bstart_d.as<int64_t>(), crank_d.as<int32_t>(), L,
                                       klo.as<uint64_t>(), khi.as<uint64_t>(), idx.as<uint32_t>(), v_row.as<int64_t>(),
                                       v_start.as<int64_t>(), v_end.as<int64_t>(), orand.as<unsigned long long>());
    unsigned long long oa[4];
    KMAP_CHECK_HIP(hipMemcpyAsync(oa, orand.p, 32, hipMemcpyDeviceToHost, st));
    KMAP_CHECK_HIP(hipStreamSynchronize(st));
    KMAP_CHECK_HIP(hipGetLastError());
    // ---- 4: radix passes over the digits that differ between keys
    RsBufs<2, true> ping{{klo.as<uint64_t>(), khi.as<uint64_t>()}, idx.as<uint32_t>()};
    RsBufs<2, true> pong{{klo2.as<uint64_t>(), khi2.as<uint64_t>()}, idx2.as<uint32_t>()};
    const uint64_t diff[2] = {(uint64_t)(oa[0] ^ oa[2]), (uint64_t)(oa[1] ^ oa[3])};
    KMAP_TRY(radix_sort(ping, pong, M, diff, st));
    // ---- 5: gather the sorted triples.  Only ping's payload is read from here on, so the rows and starts go into pong's two key
    // words -- the set that does not hold the result, whichever pair of allocations that is after the swaps -- and need no buffers
    // of their own
    int64_t *o_row = (int64_t *)pong.w[0], *o_start = (int64_t *)pong.w[1];
    DevBuf o_end;
    KMAP_TRY(o_end.alloc((size_t)M * 8));
    loc_gather_kernel<<<(unsigned)((M + BLK - 1) / BLK), BLK, 0, st>>>(ping.val, M, v_row.as<int64_t>(), v_start.as<int64_t>(),
                                                                       v_end.as<int64_t>(), o_row, o_start, o_end.as<int64_t>());
    KMAP_CHECK_HIP(hipGetLastError());
    KMAP_CHECK_HIP(hipMemcpyAsync(out_row, o_row, (size_t)M * 8, hipMemcpyDeviceToHost, st));
    KMAP_CHECK_HIP(hipMemcpyAsync(out_start, o_start, (size_t)M * 8, hipMemcpyDeviceToHost, st));
    KMAP_CHECK_HIP(hipMemcpyAsync(out_end, o_end.p, (size_t)M * 8, hipMemcpyDeviceToHost, st));
    KMAP_CHECK_HIP(hipEventRecord(ev1.e, st));
    KMAP_CHECK_HIP(hipStreamSynchronize(st));
    for (int c = 0; c < n_cons; ++c) n_per_cons[c] = (int64_t)(bounds[(size_t)c + 1] - bounds[(size_t)c]);
    if (device_ms) KMAP_CHECK_HIP(hipEventElapsedTime(device_ms, ev0.e, ev1.e));
    return KMAP_OK;
}

extern "C" int kmap_locations_sort(int64_t n_rows, int n_cons, const int32_t *const *hits, const int32_t *const *pos, const int64_t *n_pos,
                                   const int32_t *cons_len, const int64_t *seq_ind, int64_t n_bed, const int64_t *bed_start,
                                   const int32_t *chrom_rank, int n_chrom, int64_t cap, int64_t *out_row, int64_t *out_start,
                                   int64_t *out_end, int64_t *n_per_cons, float *device_ms) {
    try {
        return locations_impl(n_rows, n_cons, hits, pos, n_pos, cons_len, seq_ind, n_bed, bed_start, chrom_rank, n_chrom, cap, out_row,
                              out_start, out_end, n_per_cons, device_ms);
    } catch (const std::bad_alloc &) {
        kmap_set_error("locations: out of memory");
        return KMAP_E_NOMEM;
    }
}
