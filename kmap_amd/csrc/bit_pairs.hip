// bit_pairs.hip -- pairs[i][j] = sum_w popcount(planes[i][w] & planes[j][w]) for all pairs of rows of a bit matrix: an integer matrix
// product on bits (motif_cooccurrence).  It knows nothing of reads or motifs.
//   * bit_pairs_kernel: one block = one 64 x 64 tile of pairs (tile row <= tile column; blockIdx.x numbers those) over one slice of
//     the words (blockIdx.y).  The two row panels go through LDS in steps of BP_K = 32 words: 256 threads load 64 rows x 32 words
//     of each panel, 32 consecutive lanes one row's 256 contiguous bytes; rows behind n_mat and words behind the slice read as 0.
//     The next step's words are loaded into registers before the current step is computed.
//   * LDS rows have a stride of BP_K + 2 = 34 words = 68 dwords: a 16-byte read at row r starts at bank 4 r mod 64, so the 16
//     different rows of a panel that the lanes of one ds_read_b128 lane group ask for cover all 64 banks once; the stride is even so
//     that two words are read at once.  2 x 64 x 34 x 8 B = 34 816 B per block: four blocks per CU, four waves per SIMD.
//   * A thread holds a 4 x 4 micro-tile, rows ty + 16 a against rows tx + 16 b, in uint32 registers; per word and pair two ANDs
//     and two popcounts, the second adding the first (v_bcnt_u32_b32 adds its third operand), and one three-operand add per two
//     words: 4.5 vector instructions per word pair as compiled, 4 were the ideal.  A register gains at most 64 per word, and a slice has
//     at most BP_MAX_SLICE = 2^25 words: 2^31 < 2^32, no overflow.  The entry point checks the slice against that bound.
//   * The block adds its non-zero sums to a zeroed uint64 matrix with integer atomics: exact and order-free, so the result does not
//     depend on the split.  A diagonal tile holds both of its triangles; a tile above the diagonal adds every sum a second time at
//     the mirrored place, so the lower triangle is made on the device and the host only copies the matrix back.
//   * The split: the words are cut into slices so that about 64 blocks per CU exist (sixteen rounds of the four a CU holds: with 16
//     per CU a library of 2048 rows ran 4.1 rounds, the last one nearly empty.  That split and five instructions per word pair
//     took 47.3 ms for 2048 rows x 10 M bits, this one and 4.5 take 40.7 ms; the two changes were not measured apart) whatever the
//     number of tiles -- 16 rows are one tile, the grid then comes from the slices alone; a slice is a multiple of BP_K words
//     and at least BP_MIN_SLICE = 128 words, so that a block's up to 8192 atomics stand against 128 words x 4096 pairs of work.
//   * No zero-panel skip: a staged panel is 64 rows x 32 words = 131 072 bits, at a density of 2 - 3 % it is never all zero.
#include <vector>

#include "common.h"

namespace {

constexpr int BP_TILE = 64;
constexpr int BP_K = 32;                         // words per staging step (kmap_amd/device_seq.py: BIT_PAIRS_K)
constexpr int BP_STRIDE = BP_K + 2;              // words per LDS row
constexpr int BP_TPB = 256;
constexpr int BP_MAX_ROWS = 4096;
constexpr int64_t BP_MIN_SLICE = 128;            // (BIT_PAIRS_MIN_SLICE)
constexpr int64_t BP_MAX_SLICE = 1ll << 25;      // 64 bits x 2^25 words = 2^31: a uint32 sum cannot overflow
constexpr int BP_BLOCKS_PER_CU = 64;

struct alignas(16) Word2 {
    unsigned long long x, y;
};

__device__ __forceinline__ void bp_add(uint32_t &acc, unsigned long long a, unsigned long long b) {
    acc += (uint32_t)__popcll(a & b);
}

// Four blocks per CU, as the LDS admits: 127 VGPRs with a dozen spilled (load addresses, touched once per staging step) against the
// 180 of the compiler's own allocation, which leaves two waves per SIMD.  Unmeasured against that alternative.
__global__ __launch_bounds__(BP_TPB, 4) void bit_pairs_kernel(const unsigned long long *__restrict__ planes, int n_mat, int64_t n_words,
                                                              int n_tiles, int64_t slice_words, unsigned long long *__restrict__ out) {
    __shared__ __align__(16) unsigned long long sa[BP_TILE * BP_STRIDE], sb[BP_TILE * BP_STRIDE];
    int tr = 0, rem = (int)blockIdx.x;                 // the blockIdx.x-th tile pair with tr <= tc
    while (rem >= n_tiles - tr) {
        rem -= n_tiles - tr;
        ++tr;
    }
    const int tc = tr + rem;
    const int64_t w0 = (int64_t)blockIdx.y * slice_words, w1 = w0 + slice_words < n_words ? w0 + slice_words : n_words;
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    uint32_t acc[4][4] = {};
    unsigned long long pa[8], pb[8];
    auto fetch = [&](int64_t k0) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int idx = j * BP_TPB + tid, row = idx >> 5, col = idx & 31;
            const int64_t w = k0 + col;
            const int ra = tr * BP_TILE + row, rb = tc * BP_TILE + row;
            pa[j] = ra < n_mat && w < w1 ? planes[(int64_t)ra * n_words + w] : 0ull;
            pb[j] = rb < n_mat && w < w1 ? planes[(int64_t)rb * n_words + w] : 0ull;
        }
    };
    fetch(w0);
    for (int64_t k0 = w0; k0 < w1; k0 += BP_K) {
        __syncthreads();                               // the step before has been read
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int idx = j * BP_TPB + tid, row = idx >> 5, col = idx & 31;
            sa[row * BP_STRIDE + col] = pa[j];
            sb[row * BP_STRIDE + col] = pb[j];
        }
        __syncthreads();
        if (k0 + BP_K < w1) fetch(k0 + BP_K);
#pragma unroll 2
        for (int k = 0; k < BP_K; k += 2) {
            Word2 a[4], b[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                a[i] = *reinterpret_cast<const Word2 *>(&sa[(ty + 16 * i) * BP_STRIDE + k]);
                b[i] = *reinterpret_cast<const Word2 *>(&sb[(tx + 16 * i) * BP_STRIDE + k]);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    bp_add(acc[i][j], a[i].x, b[j].x);
                    bp_add(acc[i][j], a[i].y, b[j].y);
                }
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int r = tr * BP_TILE + ty + 16 * i, c = tc * BP_TILE + tx + 16 * j;
            if (r < n_mat && c < n_mat && acc[i][j]) {
                atomicAdd(&out[(int64_t)r * n_mat + c], (unsigned long long)acc[i][j]);
                if (tr != tc) atomicAdd(&out[(int64_t)c * n_mat + r], (unsigned long long)acc[i][j]);      // the tile under the diagonal
            }
        }
}

}  // namespace

extern "C" {

int kmap_bitrows_pair_counts_dev(const uint64_t *planes_dev, int n_mat, int64_t n_words, uint64_t *pairs_host, void *stream) {
    KMAP_REQUIRE(n_mat >= 0 && n_words >= 0, "bitrows_pair_counts: negative size");
    if (n_mat > BP_MAX_ROWS) {
        kmap_set_error("bitrows_pair_counts: %d rows, more than %d", n_mat, BP_MAX_ROWS);
        return KMAP_E_UNSUP;
    }
    if (n_mat == 0) return KMAP_OK;
    KMAP_REQUIRE(pairs_host, "bitrows_pair_counts: null pointer");
    const size_t cells = (size_t)n_mat * (size_t)n_mat;
    if (n_words == 0) {
        memset(pairs_host, 0, cells * 8);
        return KMAP_OK;
    }
    KMAP_REQUIRE(planes_dev, "bitrows_pair_counts: null pointer");
    hipStream_t st = as_stream(stream);
    int dev = 0, cus = 0;
    KMAP_CHECK_HIP(hipGetDevice(&dev));
    KMAP_CHECK_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    KMAP_REQUIRE(cus > 0, "bitrows_pair_counts: the device reports no compute unit");

    const int n_tiles = (n_mat + BP_TILE - 1) / BP_TILE, n_pairs = n_tiles * (n_tiles + 1) / 2;
    const int64_t want = std::max<int64_t>(1, ((int64_t)cus * BP_BLOCKS_PER_CU + n_pairs - 1) / n_pairs);     // slices asked for
    int64_t slice = std::max<int64_t>((n_words + want - 1) / want, BP_MIN_SLICE);
    slice = std::min<int64_t>((slice + BP_K - 1) / BP_K * BP_K, BP_MAX_SLICE);
    const int64_t n_slices = (n_words + slice - 1) / slice;
    // a register sums 64 bits per word of its slice at the most
    KMAP_REQUIRE(slice <= BP_MAX_SLICE && slice * 64 < (1ll << 32), "bitrows_pair_counts: a slice of %lld words overflows a 32-bit sum", (long long)slice);
    if (n_slices > 65535) {
        kmap_set_error("bitrows_pair_counts: %lld words per row need more than 65535 slices", (long long)n_words);
        return KMAP_E_UNSUP;
    }

    unsigned long long *out = nullptr;
    KMAP_TRY(kmap_scratch((void **)&out, cells * 8, st, KMAP_SLOT_A));
    KMAP_CHECK_HIP(hipMemsetAsync(out, 0, cells * 8, st));
    bit_pairs_kernel<<<dim3((unsigned)n_pairs, (unsigned)n_slices), BP_TPB, 0, st>>>((const unsigned long long *)planes_dev, n_mat, n_words,
                                                                                     n_tiles, slice, out);
    KMAP_CHECK_HIP(hipGetLastError());
    KMAP_CHECK_HIP(hipMemcpyAsync(pairs_host, out, cells * 8, hipMemcpyDeviceToHost, st));
    KMAP_CHECK_HIP(hipStreamSynchronize(st));
    return KMAP_OK;
}

}  // extern "C"
