// project.hip -- project_kmers: place M new k-mers on an existing 2-D map of N reference k-mers (DESIGN.md "Projection").
//
//   1. project_knn_kernel     orientation + the n_nb nearest references of every query: a counting select on the k + 1 possible
//                             Hamming distances, one wavefront per query, no M x N matrix.
//   2. project_prob_kernel    Q[m][j] = sum of the n_nb neighbour-sum rows of the query's neighbours (uint16 -> uint32), p = LUT3[Q].
//   3. project_descend_kernel start (p-weighted mean of the neighbours' anchors) + the whole n_iter gradient loop of a query
//                             inside one launch: the queries are independent of each other, the anchors never move.
#include "common.h"

namespace {
constexpr int PJ_MAX_NB = 64;     // neighbours per query: one lane each in the in-wave ordering

template <typename H>
struct PjKnn {
    static constexpr int bins = sizeof(H) == 4 ? 16 : 32;   // histogram bins: distances 0..k, k <= 15 for uint32 hashes, <= 31 for uint64
    static constexpr int waves = sizeof(H) == 4 ? 4 : 2;    // queries per block: 8 KiB (16 KiB) of per-lane histograms each
};

// One wavefront per query.  The wave walks the reference hashes in ascending 64-wide chunks (lane l reads ref[c * 64 + l]:
// coalesced), so "lowest index first" is the order of the chunks and, inside a chunk, of the lanes: ballot / popcount prefixes.
//   pass 1  per-lane histograms of the distance to q and to rc(q) in LDS ([orientation][distance][lane]: a lane only ever touches
//           its own column, so the adds are conflict-free and need no ordering); summed over the lanes they give both minima (the
//           flip decision), the threshold distance t of the chosen strand and how many entries at d == t are needed.
//   pass 2  collects every index with d < t and the first `need` with d == t, stops once n_nb are found.
//   order   the <= 64 collected (distance, index) keys are distinct: the rank of a key is the number of smaller keys.
template <typename H>
__global__ __launch_bounds__(KMAP_WAVE *PjKnn<H>::waves) void project_knn_kernel(H *__restrict__ q, int64_t m, const H *__restrict__ ref,
                                                                                int64_t n, int k, int revcom, int n_nb,
                                                                                int32_t *__restrict__ nb, uint8_t *__restrict__ nb_dist,
                                                                                uint8_t *__restrict__ flipped) {
    constexpr int NB = PjKnn<H>::bins, PJ_KNN_WAVES = PjKnn<H>::waves;
    __shared__ uint32_t hist_all[PJ_KNN_WAVES][2][NB][KMAP_WAVE];
    __shared__ uint32_t tot_all[PJ_KNN_WAVES][2][NB];
    __shared__ unsigned long long key_all[PJ_KNN_WAVES][PJ_MAX_NB];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t qi = (int64_t)blockIdx.x * PJ_KNN_WAVES + wave;
    if (qi >= m) return;                                        // wave-uniform; everything below is wave-local (no block barrier)
    uint32_t(*hist)[NB][KMAP_WAVE] = hist_all[wave];
    uint32_t(*tot)[NB] = tot_all[wave];
    unsigned long long *keys = key_all[wave];
    const H mask = low_mask<H>(k);
    const H qf = q[qi] & mask;
    const H qr = revcom_hash(qf, k);
    for (int o = 0; o < 2; ++o)
        for (int d = 0; d < NB; ++d) hist[o][d][lane] = 0;
    const int64_t n_chunks = (n + 63) / 64;
    for (int64_t c = 0; c < n_chunks; ++c) {
        const int64_t j = c * 64 + lane;
        if (j < n) {
            const H r = ref[j] & mask;
            atomicAdd(&hist[0][popc2((H)(qf ^ r))][lane], 1u);  // distance <= k < NB; the lane's own column: one LDS add, no conflict
            if (revcom) atomicAdd(&hist[1][popc2((H)(qr ^ r))][lane], 1u);
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    for (int t = lane; t < 2 * NB; t += 64) {                   // lane t sums bin t over the 64 lanes' columns
        const int o = t / NB, d = t % NB;
        uint32_t s = 0;
        for (int l = 0; l < 64; ++l) s += hist[o][d][(l + lane) & 63];
        tot[o][d] = s;
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    int min_f = NB, min_r = NB;
    for (int d = NB - 1; d >= 0; --d) {
        if (tot[0][d]) min_f = d;
        if (tot[1][d]) min_r = d;
    }
    const int flip = (revcom && min_r < min_f) ? 1 : 0;         // strictly closer on the reverse strand; a tie keeps the forward one
    const H qo = flip ? qr : qf;
    int thr = 0;
    uint32_t below = 0;                                         // entries with d < thr
    for (; thr < NB - 1; ++thr) {
        const uint32_t h = tot[flip][thr];
        if (below + h >= (uint32_t)n_nb) break;
        below += h;
    }
    const uint32_t need = (uint32_t)n_nb - below;               // entries to take at d == thr, lowest indices first
    uint32_t got = 0, got_eq = 0;
    for (int64_t c = 0; c < n_chunks && got < (uint32_t)n_nb; ++c) {
        const int64_t j = c * 64 + lane;
        int d = NB;
        if (j < n) d = popc2((H)(qo ^ (ref[j] & mask)));
        const unsigned long long lower = (1ull << lane) - 1ull;
        const unsigned long long b_eq = __ballot(d == thr);
        const uint32_t eq_rank = got_eq + (uint32_t)__builtin_popcountll(b_eq & lower);
        const bool take = d < thr || (d == thr && eq_rank < need);
        const unsigned long long b_take = __ballot(take);
        if (take) {
            const uint32_t slot = got + (uint32_t)__builtin_popcountll(b_take & lower);
            if (slot < (uint32_t)PJ_MAX_NB) keys[slot] = ((unsigned long long)d << 32) | (unsigned long long)(uint32_t)j;
        }
        got += (uint32_t)__builtin_popcountll(b_take);
        got_eq += (uint32_t)__builtin_popcountll(b_eq);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (lane < n_nb) {
        const unsigned long long key = keys[lane];
        int rank = 0;
        for (int l = 0; l < n_nb; ++l) rank += keys[l] < key ? 1 : 0;
        nb[qi * n_nb + rank] = (int32_t)(uint32_t)key;
        nb_dist[qi * n_nb + rank] = (uint8_t)(key >> 32);
    }
    if (lane == 0) {
        q[qi] = qo;
        flipped[qi] = (uint8_t)flip;
    }
}

// Q and p rows of queries [row0, row0 + nrows): block = 256 threads x 4 columns, blockIdx.y = the query.  The query's neighbour rows
// (through the row map where the sums are stored de-duplicated) are resolved once per block into LDS; a thread then adds 8 bytes
// (4 uint16 sums) of each of the n_nb rows.  LUT3 (n_nb^3 k + 1 floats: 128 001 at k = 16) is read from global memory.
// Indices are clamped to the rows / table the caller declared, so a corrupt neighbour table cannot make the kernel read outside them.
constexpr int PJ_PROB_CPT = 4;
__global__ __launch_bounds__(256) void project_prob_kernel(const int32_t *__restrict__ nb, int n_nb, const uint16_t *__restrict__ sums,
                                                           int64_t lds, const int32_t *__restrict__ rowmap, int64_t map_rows,
                                                           int64_t src_rows, int64_t n, const float *__restrict__ lut, int64_t lut_len,
                                                           int64_t row0, float *__restrict__ p, int64_t ldp, uint32_t *__restrict__ qsum,
                                                           int vec) {
    __shared__ int64_t rows[PJ_MAX_NB];
    const int64_t lr = blockIdx.y;
    if ((int)threadIdx.x < n_nb) {
        int64_t r = nb[(row0 + lr) * n_nb + threadIdx.x];
        if (rowmap) {
            r = r < 0 ? 0 : (r >= map_rows ? map_rows - 1 : r);
            r = rowmap[r];
        }
        rows[threadIdx.x] = r < 0 ? 0 : (r >= src_rows ? src_rows - 1 : r);
    }
    __syncthreads();
    const int64_t j0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * PJ_PROB_CPT;
    if (j0 >= n) return;
    uint32_t s[PJ_PROB_CPT] = {0, 0, 0, 0};
    if (vec && j0 + PJ_PROB_CPT <= n) {
        for (int a = 0; a < n_nb; ++a) {
            const uint2 v = *reinterpret_cast<const uint2 *>(sums + rows[a] * lds + j0);
            s[0] += v.x & 0xFFFFu;
            s[1] += v.x >> 16;
            s[2] += v.y & 0xFFFFu;
            s[3] += v.y >> 16;
        }
    } else {
        for (int a = 0; a < n_nb; ++a)
            for (int c = 0; c < PJ_PROB_CPT; ++c)
                if (j0 + c < n) s[c] += sums[rows[a] * lds + j0 + c];
    }
    for (int c = 0; c < PJ_PROB_CPT; ++c) {
        if (j0 + c >= n) break;
        const int64_t li = (int64_t)s[c] < lut_len ? (int64_t)s[c] : lut_len - 1;
        p[lr * ldp + j0 + c] = lut[li];
        if (qsum) qsum[lr * ldp + j0 + c] = s[c];
    }
}

// Block = 256 threads and PJ_QB queries; thread t owns the reference points j = tile + t + 256 u of every tile, for all of the block's
// queries.  The anchors are staged through LDS in tiles of PJ_TILE points (x and y planes: consecutive lanes, consecutive banks) and
// each staged pair serves the PJ_QB queries; when all N anchors fit one tile they are staged once and stay for the whole loop.  The p
// row of a query is re-read from global memory every iteration (coalesced; see DESIGN.md for why it is not kept in LDS).
// Per query and iteration: partial sums per thread in ascending j, a __shfl_xor butterfly inside the wave, then the four waves'
// partials through LDS, added in wave order by every thread -- each thread holds the same y_m.  A query's arithmetic depends only
// on its own row and on N, never on its position in the block or on the other queries, so row blocking does not change a bit.
constexpr int PJ_QB = 4, PJ_TILE = 2048, PJ_THREADS = 256;
__global__ __launch_bounds__(PJ_THREADS) void project_descend_kernel(const float *__restrict__ p, int64_t ldp, const int32_t *__restrict__ nb,
                                                                    int n_nb, const float *__restrict__ ref_x, const float *__restrict__ ref_y,
                                                                    int64_t n, int64_t row0, int64_t nrows, int n_iter, float lr,
                                                                    float *__restrict__ out_x, float *__restrict__ out_y) {
    __shared__ float tx[PJ_TILE], ty[PJ_TILE];
    __shared__ float red[PJ_THREADS / 64][PJ_QB][2];
    __shared__ float start[PJ_QB][2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t q0 = (int64_t)blockIdx.x * PJ_QB;             // first local row of the block
    // start: wave w places query w at the p-weighted mean of its neighbours' anchors
    {
        static_assert(PJ_THREADS / 64 == PJ_QB, "one wave per query in the start step");
        const int64_t lr_ = q0 + wave;
        float w = 0.f, wx = 0.f, wy = 0.f;
        if (lr_ < nrows && lane < n_nb) {
            int64_t j = nb[(row0 + lr_) * n_nb + lane];
            j = j < 0 ? 0 : (j >= n ? n - 1 : j);
            w = p[lr_ * ldp + j];
            wx = w * ref_x[j];
            wy = w * ref_y[j];
        }
        for (int o = 32; o > 0; o >>= 1) {
            w += __shfl_xor(w, o);
            wx += __shfl_xor(wx, o);
            wy += __shfl_xor(wy, o);
        }
        if (lane == 0) {
            start[wave][0] = wx / w;
            start[wave][1] = wy / w;
        }
    }
    __syncthreads();
    float yx[PJ_QB], yy[PJ_QB];
    const float *prow[PJ_QB];
    for (int qq = 0; qq < PJ_QB; ++qq) {
        yx[qq] = start[qq][0];
        yy[qq] = start[qq][1];
        const int64_t lr_ = q0 + qq < nrows ? q0 + qq : nrows - 1;   // a block's spare slots repeat its last query; never stored
        prow[qq] = p + lr_ * ldp;
    }
    const float q_lo = 1e-3f, q_hi = 1.0f - 1e-3f;
    const bool resident = n <= PJ_TILE;
    for (int it = 0; it < n_iter; ++it) {
        float gx[PJ_QB], gy[PJ_QB];
        for (int qq = 0; qq < PJ_QB; ++qq) gx[qq] = gy[qq] = 0.f;
        for (int64_t t0 = 0; t0 < n; t0 += PJ_TILE) {
            if (!resident || it == 0) {
                __syncthreads();                                // the previous tile has been consumed by every thread
                for (int u = tid; u < PJ_TILE; u += PJ_THREADS) {
                    const int64_t j = t0 + u;
                    tx[u] = j < n ? ref_x[j] : 0.f;
                    ty[u] = j < n ? ref_y[j] : 0.f;
                }
                __syncthreads();
            }
            for (int u = tid; u < PJ_TILE; u += PJ_THREADS) {
                const int64_t j = t0 + u;
                if (j >= n) break;
                const float ax = tx[u], ay = ty[u];
#pragma unroll
                for (int qq = 0; qq < PJ_QB; ++qq) {
                    const float pj = prow[qq][j];
                    const float dx = yx[qq] - ax, dy = yy[qq] - ay;
                    float qv = 1.0f / (1.0f + (dx * dx + dy * dy));
                    qv = fminf(qv, q_hi);
                    qv = fmaxf(qv, q_lo);
                    const float T = qv / (1.0f - qv) * (pj - qv);
                    gx[qq] += T * dx;
                    gy[qq] += T * dy;
                }
            }
        }
#pragma unroll
        for (int qq = 0; qq < PJ_QB; ++qq) {
            for (int o = 32; o > 0; o >>= 1) {
                gx[qq] += __shfl_xor(gx[qq], o);
                gy[qq] += __shfl_xor(gy[qq], o);
            }
            if (lane == 0) {
                red[wave][qq][0] = gx[qq];
                red[wave][qq][1] = gy[qq];
            }
        }
        __syncthreads();
#pragma unroll
        for (int qq = 0; qq < PJ_QB; ++qq) {
            const float sx = ((red[0][qq][0] + red[1][qq][0]) + red[2][qq][0]) + red[3][qq][0];
            const float sy = ((red[0][qq][1] + red[1][qq][1]) + red[2][qq][1]) + red[3][qq][1];
            yx[qq] = yx[qq] - lr * (4.0f * sx);
            yy[qq] = yy[qq] - lr * (4.0f * sy);
        }
        __syncthreads();                                        // red is rewritten by the next iteration
    }
    if (tid < PJ_QB && q0 + tid < nrows) {
        float vx = yx[0], vy = yy[0];
#pragma unroll
        for (int qq = 1; qq < PJ_QB; ++qq)
            if (tid == qq) {
                vx = yx[qq];
                vy = yy[qq];
            }
        out_x[row0 + q0 + tid] = vx;
        out_y[row0 + q0 + tid] = vy;
    }
}

template <typename H>
int project_knn(H *q_dev, int64_t m, const H *ref_dev, int64_t n, int k, int revcom, int n_nb, int32_t *nb_dev, uint8_t *nb_dist_dev,
                uint8_t *flipped_dev, void *stream) {
    const int kmax = sizeof(H) == 4 ? 15 : 31;
    KMAP_REQUIRE(k >= 1 && k <= kmax, "project_knn: k=%d outside 1..%d for %d-bit hashes", k, kmax, (int)(8 * sizeof(H)));
    KMAP_REQUIRE(m >= 0, "project_knn: m=%lld queries", (long long)m);
    KMAP_REQUIRE(n > 0 && n <= 0x7fffffffLL, "project_knn: n=%lld reference k-mers (1 .. 2^31 - 1)", (long long)n);
    KMAP_REQUIRE(n_nb >= 1 && n_nb <= PJ_MAX_NB, "project_knn: n_nb=%d outside 1..%d", n_nb, PJ_MAX_NB);
    KMAP_REQUIRE(n_nb <= n, "project_knn: n_nb=%d neighbours among n=%lld reference k-mers", n_nb, (long long)n);
    if (m == 0) return KMAP_OK;
    KMAP_REQUIRE(q_dev && ref_dev && nb_dev && nb_dist_dev && flipped_dev, "project_knn: null pointer");
    constexpr int waves = PjKnn<H>::waves;
    const int64_t blocks = (m + waves - 1) / waves;
    KMAP_REQUIRE(blocks <= 0x7fffffffLL, "project_knn: m=%lld too large for one launch", (long long)m);
    project_knn_kernel<H><<<(unsigned)blocks, KMAP_WAVE * waves, 0, as_stream(stream)>>>(q_dev, m, ref_dev, n, k, revcom ? 1 : 0, n_nb,
                                                                                                nb_dev, nb_dist_dev, flipped_dev);
    KMAP_CHECK_HIP(hipGetLastError());
    return KMAP_OK;
}
}  // namespace

extern "C" {
int kmap_project_knn_u32_dev(uint32_t *q_dev, int64_t m, const uint32_t *ref_dev, int64_t n, int k, int revcom, int n_nb,
                             int32_t *nb_dev, uint8_t *nb_dist_dev, uint8_t *flipped_dev, void *stream) {
    return project_knn<uint32_t>(q_dev, m, ref_dev, n, k, revcom, n_nb, nb_dev, nb_dist_dev, flipped_dev, stream);
}
int kmap_project_knn_u64_dev(uint64_t *q_dev, int64_t m, const uint64_t *ref_dev, int64_t n, int k, int revcom, int n_nb,
                             int32_t *nb_dev, uint8_t *nb_dist_dev, uint8_t *flipped_dev, void *stream) {
    return project_knn<uint64_t>(q_dev, m, ref_dev, n, k, revcom, n_nb, nb_dev, nb_dist_dev, flipped_dev, stream);
}

int kmap_project_prob_dev(const int32_t *nb_dev, int64_t m, int n_nb, const uint16_t *sums_dev, int64_t lds, const int32_t *rowmap_dev,
                          int64_t src_rows, int64_t n, const float *lut_dev, int64_t lut_len, int64_t row0, int64_t nrows, float *p_dev,
                          int64_t ldp, uint32_t *qsum_dev, void *stream) {
    KMAP_REQUIRE(m >= 0 && row0 >= 0 && nrows >= 0 && row0 + nrows <= m, "project_prob: rows [%lld, +%lld) of m=%lld queries",
                 (long long)row0, (long long)nrows, (long long)m);
    KMAP_REQUIRE(n_nb >= 1 && n_nb <= PJ_MAX_NB, "project_prob: n_nb=%d outside 1..%d", n_nb, PJ_MAX_NB);
    if (nrows == 0) return KMAP_OK;
    KMAP_REQUIRE(n > 0 && n <= 0x7fffffffLL && lds >= n && ldp >= n, "project_prob: n=%lld, lds=%lld, ldp=%lld", (long long)n,
                 (long long)lds, (long long)ldp);
    KMAP_REQUIRE(src_rows > 0 && (rowmap_dev || src_rows == n), "project_prob: %lld stored rows for n=%lld without a row map",
                 (long long)src_rows, (long long)n);
    KMAP_REQUIRE(lut_len > 0, "project_prob: empty LUT");
    KMAP_REQUIRE(nrows <= 65535, "project_prob: nrows=%lld too large for one launch (65535)", (long long)nrows);
    KMAP_REQUIRE(nb_dev && sums_dev && lut_dev && p_dev, "project_prob: null pointer");
    const int vec = ((lds & 3) == 0 && (reinterpret_cast<uintptr_t>(sums_dev) & 7) == 0) ? 1 : 0;
    const dim3 grid((unsigned)((n + 256 * PJ_PROB_CPT - 1) / (256 * PJ_PROB_CPT)), (unsigned)nrows);
    project_prob_kernel<<<grid, 256, 0, as_stream(stream)>>>(nb_dev, n_nb, sums_dev, lds, rowmap_dev, n, src_rows, n, lut_dev, lut_len, row0,
                                                             p_dev, ldp, qsum_dev, vec);
    KMAP_CHECK_HIP(hipGetLastError());
    return KMAP_OK;
}

int kmap_project_descend_dev(const float *p_dev, int64_t ldp, const int32_t *nb_dev, int64_t m, int n_nb, const float *ref_xy_dev,
                             int64_t n, int64_t row0, int64_t nrows, int n_iter, float learning_rate, float *xy_dev, void *stream) {
    KMAP_REQUIRE(m >= 0 && row0 >= 0 && nrows >= 0 && row0 + nrows <= m, "project_descend: rows [%lld, +%lld) of m=%lld queries",
                 (long long)row0, (long long)nrows, (long long)m);
    KMAP_REQUIRE(n_nb >= 1 && n_nb <= PJ_MAX_NB, "project_descend: n_nb=%d outside 1..%d", n_nb, PJ_MAX_NB);
    KMAP_REQUIRE(n_iter >= 0, "project_descend: n_iter=%d", n_iter);
    if (nrows == 0) return KMAP_OK;
    KMAP_REQUIRE(n > 0 && n <= 0x7fffffffLL && ldp >= n, "project_descend: n=%lld, ldp=%lld", (long long)n, (long long)ldp);
    KMAP_REQUIRE(p_dev && nb_dev && ref_xy_dev && xy_dev, "project_descend: null pointer");
    const int64_t blocks = (nrows + PJ_QB - 1) / PJ_QB;
    KMAP_REQUIRE(blocks <= 0x7fffffffLL, "project_descend: nrows=%lld too large for one launch", (long long)nrows);
    project_descend_kernel<<<(unsigned)blocks, PJ_THREADS, 0, as_stream(stream)>>>(p_dev, ldp, nb_dev, n_nb, ref_xy_dev, ref_xy_dev + n, n, row0,
                                                                                   nrows, n_iter, learning_rate, xy_dev, xy_dev + m);
    KMAP_CHECK_HIP(hipGetLastError());
    return KMAP_OK;
}
}
