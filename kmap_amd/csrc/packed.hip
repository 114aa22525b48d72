// packed.hip -- 2-bit-packed reads resident in HBM and the kernels that work on them.
//
// Packed layout (one "group" = 16 consecutive positions of the reference's uint8 array, kmer_count.py:244-347):
//   codes[g] : uint32, base i of the group in bits [31-2i, 30-2i]   (first base most significant, like the hash)
//   inval[g] : uint16, bit (15-i) set when byte i is not A/C/G/T (255: N or read separator) or lies past the end
// plus two all-invalid halo groups, so every kernel may read groups g, g+1, g+2 unguarded.  0.375 B per position
// instead of 1 B, and a k-mer window is a funnel shift instead of a k-step byte loop.  Masking (mask_input,
// kmer_count.py:580-610) only ever turns positions into 255, i.e. it ORs bits into `inval`: the codes are immutable
// and "restore the unmasked array" (motif_discovery.py:263) is a copy of n/8 bytes.
//
// Here: the layout itself -- pack / unpack, the hash materialisation and the prefix invalidation.  What works ON the layout lives by job:
// the window-key front end in packed_keys.h, counting in counts_packed.hip (+ the per-read dedupe of dedupe_packed.hip, the partitioned
// histograms of counts_part.hip / counts_fine.hip), the Hamming-ball mask and the occurrence scan in scan.hip (dispatch, k <= 16 ->
// bitslice.hip, scan_reads.hip) and scan_wide.hip (k > 16).
#include "common.h"
#include "packed_keys.h"

namespace {

constexpr int BLK = 256;
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// ---- pack / unpack -------------------------------------------------------------------------------------------
__device__ __forceinline__ void pack4(uint32_t wd, uint32_t &code, uint32_t &flags) {
    const uint32_t t = wd & 0x03030303u;
    code = ((t << 6) | (t >> 4) | (t >> 14) | (t >> 24)) & 0xFFu;
    uint32_t f = wd & 0xFCFCFCFCu;                 // any of bits 7:2 set -> not a base
    f |= f >> 1; f |= f >> 2; f |= f >> 4;         // smear into bit 0 of every byte (cross-byte smear only goes downward
    f &= 0x01010101u;                              //  from a byte that is itself non-zero, so bit 0 of byte j stays exact)
    flags = ((f << 3) | (f >> 6) | (f >> 15) | (f >> 24)) & 0xFu;
}
__global__ __launch_bounds__(BLK) void pack_kernel(const uint8_t *__restrict__ seq, int64_t n, uint32_t *__restrict__ codes,
                                                   uint16_t *__restrict__ inval, int64_t n_groups, int aligned) {
    const int64_t g = (int64_t)blockIdx.x * BLK + threadIdx.x;
    if (g >= n_groups) return;
    const int64_t p0 = g * 16;
    uint32_t wd[4];
    if (p0 + 16 <= n && aligned) {
        const u32x4 v = *reinterpret_cast<const u32x4 *>(seq + p0);
        wd[0] = v.x; wd[1] = v.y; wd[2] = v.z; wd[3] = v.w;
    } else {
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            uint32_t x = 0;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const int64_t p = p0 + 4 * d + b;
                x |= (uint32_t)((p < n) ? seq[p] : 255u) << (8 * b);
            }
            wd[d] = x;
        }
    }
    uint32_t c = 0, m = 0;
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        uint32_t cd, fd;
        pack4(wd[d], cd, fd);
        c |= cd << (24 - 8 * d);
        m |= fd << (12 - 4 * d);
    }
    codes[g] = c;
    inval[g] = (uint16_t)m;
}
__global__ __launch_bounds__(BLK) void unpack_kernel(const uint32_t *__restrict__ codes, const uint16_t *__restrict__ inval,
                                                     int64_t n, uint8_t *__restrict__ seq) {
    const int64_t p = (int64_t)blockIdx.x * BLK + threadIdx.x;
    if (p >= n) return;
    const int64_t g = p >> 4;
    const int i = (int)(p & 15);
    const bool bad = (inval[g] >> (15 - i)) & 1;
    seq[p] = bad ? 255 : (uint8_t)((codes[g] >> (30 - 2 * i)) & 3u);
}

// ---- hash materialisation (one thread per group, 16 hashes, 64/128 contiguous bytes out) -------------------------
template <typename H, bool WIDE>
__global__ __launch_bounds__(BLK) void hash_packed_kernel(const uint32_t *__restrict__ codes, const uint16_t *__restrict__ inval,
                                                          int64_t n, int k, H *__restrict__ out, const uint32_t *__restrict__ skip,
                                                          unsigned long long *__restrict__ all_ones) {
    const int64_t g = (int64_t)blockIdx.x * BLK + threadIdx.x;
    const int64_t p0 = g * 16;
    if (p0 >= n) return;
    const Win w = load_win(codes, inval, g);
    const uint64_t kmask = low_mask<uint64_t>(k);
    const uint32_t sk = skip16_of(skip, g);
    H hs[16];
    uint32_t n_ones = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        bool bad;
        const uint64_t h = win_hash<WIDE>(w, i, k, kmask, bad);
        const bool drop = bad || ((sk >> (15 - i)) & 1u);
        hs[i] = drop ? (H)~(H)0 : (H)h;
        // 16-mers as uint32 (partitioned counting): the all-T k-mer's hash IS the invalid marker -- its valid windows are counted
        // aside (all_ones) and leave the array as invalid
        if (all_ones && !drop && (H)h == (H)~(H)0) ++n_ones;
    }
    if (n_ones) atomicAdd(all_ones, (unsigned long long)n_ones);
    if (p0 + 16 <= n && ((uintptr_t)out % 16) == 0) {
        u32x4 *o = reinterpret_cast<u32x4 *>(out + p0);
        if constexpr (sizeof(H) == 4) {
#pragma unroll
            for (int v = 0; v < 4; ++v) o[v] = u32x4{(uint32_t)hs[4 * v], (uint32_t)hs[4 * v + 1], (uint32_t)hs[4 * v + 2], (uint32_t)hs[4 * v + 3]};
        } else {
#pragma unroll
            for (int v = 0; v < 8; ++v)
                o[v] = u32x4{(uint32_t)hs[2 * v], (uint32_t)((uint64_t)hs[2 * v] >> 32), (uint32_t)hs[2 * v + 1],
                             (uint32_t)((uint64_t)hs[2 * v + 1] >> 32)};
        }
    } else {
        for (int i = 0; i < 16 && p0 + i < n; ++i) out[p0 + i] = hs[i];
    }
}
}  // namespace

extern "C" {

// data groups + two all-invalid halo groups, rounded up to an EVEN number of groups: kernels that take group pairs (bitslice.hip:
// thread = groups 2t .. 2t + 3) read whole aligned pairs without a bounds test
int64_t kmap_packed_groups(int64_t n) { return ((((n + 15) >> 4) + 2) + 1) & ~(int64_t)1; }

int kmap_pack_reads_dev(const uint8_t *seq_dev, int64_t n, uint32_t *codes_dev, uint16_t *inval_dev, void *stream) {
    KMAP_REQUIRE(n >= 0 && (n == 0 || seq_dev) && codes_dev && inval_dev, "pack_reads: bad arguments");
    const int64_t ng = kmap_packed_groups(n);
    pack_kernel<<<grid_for(ng, BLK), BLK, 0, as_stream(stream)>>>(seq_dev, n, codes_dev, inval_dev, ng,
                                                                   ((uintptr_t)seq_dev % 16) == 0);
    KMAP_CHECK_HIP(hipGetLastError());
    return KMAP_OK;
}

int kmap_unpack_reads_dev(const uint32_t *codes_dev, const uint16_t *inval_dev, int64_t n, uint8_t *seq_out_dev, void *stream) {
    KMAP_REQUIRE(n >= 0 && codes_dev && inval_dev && (n == 0 || seq_out_dev), "unpack_reads: bad arguments");
    if (n == 0) return KMAP_OK;
    unpack_kernel<<<grid_for(n, BLK), BLK, 0, as_stream(stream)>>>(codes_dev, inval_dev, n, seq_out_dev);
    KMAP_CHECK_HIP(hipGetLastError());
    return KMAP_OK;
}

int kmap_hash_kmers_packed_dev(const uint32_t *codes_dev, const uint16_t *inval_dev, int64_t n, int k, void *out_dev,
                               void *stream) {
    KMAP_REQUIRE(k > 0 && k < 32, "hash_kmers_packed: k=%d out of range", k);
    KMAP_REQUIRE(n >= 0 && codes_dev && inval_dev && (n == 0 || out_dev), "hash_kmers_packed: bad arguments");
    if (n == 0) return KMAP_OK;
    const unsigned g = grid_for((n + 15) >> 4, BLK);
    hipStream_t st = as_stream(stream);
    if (k < 16) hash_packed_kernel<uint32_t, false><<<g, BLK, 0, st>>>(codes_dev, inval_dev, n, k, (uint32_t *)out_dev, nullptr, nullptr);
    else if (k == 16) hash_packed_kernel<uint64_t, false><<<g, BLK, 0, st>>>(codes_dev, inval_dev, n, k, (uint64_t *)out_dev, nullptr, nullptr);
    else hash_packed_kernel<uint64_t, true><<<g, BLK, 0, st>>>(codes_dev, inval_dev, n, k, (uint64_t *)out_dev, nullptr, nullptr);
    KMAP_CHECK_HIP(hipGetLastError());
    return KMAP_OK;
}

namespace {
__global__ void inval_prefix_kernel(uint16_t *__restrict__ inval, int64_t m) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t left = m - 16 * g;                           // positions of this group inside the prefix
    if (left <= 0) return;
    inval[g] |= left >= 16 ? (uint16_t)0xFFFFu : (uint16_t)(0xFFFFu << (16 - (int)left));
}
}  // namespace

int kmap_inval_set_prefix_dev(uint16_t *inval_dev, int64_t m, void *stream) {
    if (m <= 0) return KMAP_OK;
    KMAP_REQUIRE(inval_dev, "inval_set_prefix: null pointer");
    const int64_t ng = (m + 15) >> 4;
    inval_prefix_kernel<<<(unsigned)((ng + 63) / 64), 64, 0, as_stream(stream)>>>(inval_dev, m);
    KMAP_CHECK_HIP(hipGetLastError());
    return KMAP_OK;
}

}  // extern "C"
