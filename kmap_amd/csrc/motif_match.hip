// motif_match.hip -- count matrices compared with a library of count matrices (match_motifs).  A motif is a run
// of quantised columns, 4 x uint16 (A C G T, each 0..1024) = 8 bytes; the columns of all motifs of a set stand behind one another.
// The reverse complement of a motif needs no second array: its column j is column w - 1 - j with the four bases in reverse order.
//
//   * column score: d2 = sum_b (x_b - y_b)^2, e = floor(sqrt(d2)) exactly (a float root, then the integer correction
//     e^2 <= d2 < (e + 1)^2), s = (1448 - e) / 16 in 0..90.  The score is clamped to 0..90, so columns that are no quantised
//     frequencies (d2 > 2^21) cannot leave a bin array or a table; for quantised frequencies the clamp changes nothing.
//   * histograms (hist_kernel): a block owns MM_QB query columns and walks tiles of MM_TPB library columns, one column (one 8-byte
//     load) per thread and step; its MM_QB x 91 uint32 bins are in LDS; the flush is one integer atomic add per non-empty bin.
//   * null tables (tables_kernel): one block per query.  For every first column a the pmf of the range a..b grows column by column,
//     pmf'[x] = sum_k h_b[k] pmf[x - k] as a gather with k ascending (no floating atomics), between two LDS buffers; every range of
//     at least min_len columns has its tail sums written: per thread a chunk of consecutive scores, the chunks' sums added from the
//     top in a fixed order.  Every run gives the same bits.
//   * pairs (pairs_kernel): a wave per (query, target) pair, MM_WAVES pairs of one query per block.  The two w_q x w_t score
//     matrices (target forward / reverse-complemented) are computed once into LDS as bytes; a lane then owns configurations
//     (strand, offset): the diagonal sum, one table read, and a butterfly over the wave picks the best (p, then the longer overlap,
//     then + before -, then the smaller offset).  Column scores never reach HBM.
#include <algorithm>
#include <vector>

#include "common.h"

namespace {

constexpr int MM_TPB = 256;
constexpr int MM_WAVES = MM_TPB / KMAP_WAVE;
constexpr int MM_BINS = 91;              // column scores 0..90
constexpr int MM_MAX_W = 31, MM_MIN_W = 4;
constexpr int MM_QB = 16;                // query columns of a histogram block
constexpr int MM_HIST_TILES = 16;        // blocks that share the library columns of a group of query columns
constexpr int MM_PMF = 90 * MM_MAX_W + 1;                // 2791: the scores of a range of 31 columns
constexpr int MM_CHUNK = (MM_PMF + MM_TPB - 1) / MM_TPB; // 11 scores per thread in the tail sums
constexpr int MM_TABLE_LDS = (MM_MAX_W * MM_BINS + 2 * MM_PMF + MM_TPB) * 8;
constexpr int MM_ROW = 32;               // row pitch of a pair's score matrix in LDS

struct QueryMeta {
    int64_t col0;    // first column (row of the histogram array) of the query
    int64_t toff;    // first double of the query's tables
    int32_t w, min_len;
};
struct TargetMeta {
    int64_t col0;
    int32_t w, pad;
};

// doubles of the tables of lengths min_len .. L - 1 (the tables of one first column stand by length)
__host__ __device__ __forceinline__ int64_t len_offset(int L, int min_len) {
    if (L <= min_len) return 0;
    return 90 * ((int64_t)(L - 1) * L / 2 - (int64_t)(min_len - 1) * min_len / 2) + (L - min_len);
}
// doubles in front of the tables of first column a of a query of width w (a == w: all of the query's tables)
__host__ __device__ __forceinline__ int64_t row_offset(int a, int w, int min_len) {
    int64_t s = 0;
    for (int i = 0; i < a; ++i) s += len_offset(w - i + 1, min_len);
    return s;
}

__device__ __forceinline__ int col_score(uint2 x, uint2 y) {
    // 11 bits per entry hold 0..1024; whatever else the arrays hold, every square stays below 2^22 and q is exact as a float
    const int d0 = (int)(x.x & 0x7FFu) - (int)(y.x & 0x7FFu), d1 = (int)(x.x >> 16 & 0x7FFu) - (int)(y.x >> 16 & 0x7FFu);
    const int d2 = (int)(x.y & 0x7FFu) - (int)(y.y & 0x7FFu), d3 = (int)(x.y >> 16 & 0x7FFu) - (int)(y.y >> 16 & 0x7FFu);
    const uint32_t q = (uint32_t)(d0 * d0 + d1 * d1 + d2 * d2 + d3 * d3);
    uint32_t e = (uint32_t)sqrtf((float)q);
    if ((uint64_t)e * e > q) --e;
    if ((uint64_t)(e + 1) * (e + 1) <= q) ++e;
    const int s = (1448 - (int)e) >> 4;
    return s < 0 ? 0 : (s > 90 ? 90 : s);
}
// the column with its bases in reverse order: A C G T -> T G C A
__device__ __forceinline__ uint2 col_reverse(uint2 y) {
    return make_uint2((y.y >> 16) | (y.y << 16), (y.x >> 16) | (y.x << 16));
}

// ---- histograms -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MM_TPB) void hist_kernel(const uint2 *__restrict__ qcols, int64_t n_q, const uint2 *__restrict__ lcols,
                                                      int64_t n_l, int revcom, uint32_t *__restrict__ hist) {
    __shared__ uint32_t bins[MM_QB * MM_BINS];
    __shared__ uint2 q[MM_QB];
    const int64_t q0 = (int64_t)blockIdx.x * MM_QB;
    const int nq = (int)(n_q - q0 < MM_QB ? n_q - q0 : MM_QB);
    for (int j = threadIdx.x; j < MM_QB * MM_BINS; j += MM_TPB) bins[j] = 0;
    if ((int)threadIdx.x < nq) q[threadIdx.x] = qcols[q0 + threadIdx.x];
    __syncthreads();
    for (int64_t i = (int64_t)blockIdx.y * MM_TPB + threadIdx.x; i < n_l; i += (int64_t)gridDim.y * MM_TPB) {
        const uint2 y = lcols[i], yr = col_reverse(y);
        for (int j = 0; j < nq; ++j) {
            atomicAdd(&bins[j * MM_BINS + col_score(q[j], y)], 1u);
            if (revcom) atomicAdd(&bins[j * MM_BINS + col_score(q[j], yr)], 1u);
        }
    }
    __syncthreads();
    for (int j = threadIdx.x; j < nq * MM_BINS; j += MM_TPB)
        if (bins[j]) atomicAdd(&hist[q0 * MM_BINS + j], bins[j]);
}

// ---- null tables ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MM_TPB) void tables_kernel(const uint32_t *__restrict__ hist, double n_null, const QueryMeta *__restrict__ meta,
                                                        double *__restrict__ tables) {
    extern __shared__ double lds[];
    double *h = lds;                                 // [w][91]
    double *buf0 = h + MM_MAX_W * MM_BINS, *buf1 = buf0 + MM_PMF, *part = buf1 + MM_PMF;
    const QueryMeta m = meta[blockIdx.x];
    const int w = m.w, tid = threadIdx.x;
    for (int j = tid; j < w * MM_BINS; j += MM_TPB) h[j] = (double)hist[m.col0 * MM_BINS + j] / n_null;
    __syncthreads();
    double *out = tables + m.toff;
    for (int a = 0; a < w; ++a) {
        double *cur = buf0, *nxt = buf1;
        for (int j = tid; j < MM_BINS; j += MM_TPB) cur[j] = h[a * MM_BINS + j];
        __syncthreads();
        for (int L = 1; a + L <= w; ++L) {
            const int n = 90 * L + 1;
            if (L >= m.min_len) {                    // tail sums of cur[0 .. n)
                const int lo = tid * MM_CHUNK, hi = lo + MM_CHUNK < n ? lo + MM_CHUNK : n;
                double s = 0.0;
                for (int j = hi - 1; j >= lo; --j) s += cur[j];
                part[tid] = s;
                __syncthreads();
                double acc = 0.0;
                for (int c = MM_TPB - 1; c > tid; --c) acc += part[c];
                for (int j = hi - 1; j >= lo; --j) {
                    acc += cur[j];
                    out[j] = acc;
                }
                out += n;
            }
            if (a + L < w) {                         // the next column joins the range
                const double *hb = h + (a + L) * MM_BINS;
                for (int x = tid; x < n + 90; x += MM_TPB) {
                    const int k0 = x - (n - 1) > 0 ? x - (n - 1) : 0, k1 = x < 90 ? x : 90;
                    double s = 0.0;
                    for (int k = k0; k <= k1; ++k) s += hb[k] * cur[x - k];
                    nxt[x] = s;
                }
                double *t = cur;
                cur = nxt;
                nxt = t;
            }
            __syncthreads();
        }
    }
}

// ---- pairs ----------------------------------------------------------------------------------------------------------------------
struct Best {
    double p;
    int o, strand, L, x;
};
__device__ __forceinline__ bool better(const Best &a, const Best &b) {
    if (a.p != b.p) return a.p < b.p;
    if (a.L != b.L) return a.L > b.L;
    if (a.strand != b.strand) return a.strand < b.strand;
    return a.o < b.o;
}

__global__ __launch_bounds__(MM_TPB) void pairs_kernel(const uint2 *__restrict__ qcols, const QueryMeta *__restrict__ qmeta,
                                                       const double *__restrict__ tables, const uint2 *__restrict__ lcols,
                                                       const TargetMeta *__restrict__ tmeta, int n_target, int min_overlap, int revcom,
                                                       double *__restrict__ p_out, int4 *__restrict__ cfg_out) {
    __shared__ uint8_t S[MM_WAVES][2][MM_MAX_W * MM_ROW];
    __shared__ uint2 qc[MM_MAX_W];
    __shared__ int64_t row0[MM_MAX_W];
    const QueryMeta qm = qmeta[blockIdx.y];
    const int wq = qm.w, lane = threadIdx.x & (KMAP_WAVE - 1), wave = threadIdx.x / KMAP_WAVE;
    if ((int)threadIdx.x < wq) {
        qc[threadIdx.x] = qcols[qm.col0 + threadIdx.x];
        row0[threadIdx.x] = row_offset((int)threadIdx.x, wq, qm.min_len);
    }
    __syncthreads();
    const int t = (int)blockIdx.x * MM_WAVES + wave;
    const bool on = t < n_target;
    TargetMeta tm = {0, MM_MIN_W, 0};
    if (on) tm = tmeta[t];
    const int wt = tm.w;
    if (on)
        for (int e = lane; e < wq * wt; e += KMAP_WAVE) {
            const int i = e / wt, j = e - i * wt;
            const uint2 y = lcols[tm.col0 + j], x = qc[i];
            S[wave][0][i * MM_ROW + j] = (uint8_t)col_score(x, y);
            S[wave][1][i * MM_ROW + (wt - 1 - j)] = (uint8_t)col_score(x, col_reverse(y));
        }
    __syncthreads();
    if (!on) return;
    const int m = min(min_overlap, min(wq, wt)), n_off = wq + wt - 2 * m + 1, n_cfg = n_off * (revcom ? 2 : 1);
    Best best = {2.0, 0, 0, 0, 0};                   // above every p: lanes without a configuration lose
    for (int c = lane; c < n_cfg; c += KMAP_WAVE) {
        const int strand = c >= n_off, o = c - strand * n_off - (wt - m);
        const int a = o > 0 ? o : 0, b = (wq < wt + o ? wq : wt + o) - 1, L = b - a + 1;
        const uint8_t *s = S[wave][strand];
        int x = 0;
        for (int i = a; i <= b; ++i) x += s[i * MM_ROW + (i - o)];
        const Best cand = {tables[qm.toff + row0[a] + len_offset(L, qm.min_len) + x], o, strand, L, x};
        if (better(cand, best)) best = cand;
    }
    for (int d = KMAP_WAVE / 2; d > 0; d >>= 1) {
        Best other;
        other.p = __shfl_xor(best.p, d);
        other.o = __shfl_xor(best.o, d);
        other.strand = __shfl_xor(best.strand, d);
        other.L = __shfl_xor(best.L, d);
        other.x = __shfl_xor(best.x, d);
        if (better(other, best)) best = other;
    }
    if (lane == 0) {
        const int64_t at = (int64_t)blockIdx.y * n_target + t;
        p_out[at] = best.p;
        cfg_out[at] = make_int4(best.o, best.strand, best.L, best.x);
    }
}

// the queries' widths, columns, range lengths and table places: checked on the host, so that no kernel reads or writes outside the
// arrays it was given, then packed for the device
int pack_queries(const char *who, int n_query, const int32_t *q_width, const int64_t *q_col0, const int32_t *q_min_len,
                 const int64_t *q_toff, int64_t n_qcols, int64_t n_table, std::vector<QueryMeta> *out) {
    KMAP_REQUIRE(q_width && q_col0 && q_min_len && q_toff, "%s: null pointer", who);
    out->resize((size_t)n_query);
    for (int q = 0; q < n_query; ++q) {
        const int w = q_width[q], ml = q_min_len[q];
        KMAP_REQUIRE(w >= MM_MIN_W && w <= MM_MAX_W, "%s: width=%d of query %d outside 4..31", who, w, q);
        KMAP_REQUIRE(ml >= 1 && ml <= w, "%s: min_len=%d of query %d outside 1..%d", who, ml, q, w);
        KMAP_REQUIRE(q_col0[q] >= 0 && q_col0[q] + w <= n_qcols, "%s: the columns of query %d lie outside the %lld query columns", who, q,
                     (long long)n_qcols);
        KMAP_REQUIRE(q_toff[q] >= 0 && q_toff[q] <= n_table && row_offset(w, w, ml) <= n_table - q_toff[q],
                     "%s: the tables of query %d lie outside the %lld doubles of the table array", who, q, (long long)n_table);
        (*out)[(size_t)q] = {q_col0[q], q_toff[q], w, ml};
    }
    return KMAP_OK;
}

}  // namespace

extern "C" {

int kmap_match_hist_dev(const uint16_t *qcols_dev, int64_t n_qcols, const uint16_t *lcols_dev, int64_t n_lcols, int revcom,
                        uint32_t *hist_dev, void *stream) {
    KMAP_REQUIRE(n_qcols >= 0 && n_lcols >= 0, "match_hist: negative size");
    if (n_qcols == 0) return KMAP_OK;
    KMAP_REQUIRE(qcols_dev && hist_dev && (lcols_dev || n_lcols == 0), "match_hist: null pointer");
    KMAP_REQUIRE(n_lcols < ((int64_t)1 << 31), "match_hist: %lld library columns, a bin holds 32 bits", (long long)n_lcols);
    KMAP_REQUIRE((n_qcols + MM_QB - 1) / MM_QB < ((int64_t)1 << 31), "match_hist: %lld query columns", (long long)n_qcols);
    hipStream_t st = as_stream(stream);
    KMAP_CHECK_HIP(hipMemsetAsync(hist_dev, 0, (size_t)n_qcols * MM_BINS * 4, st));
    if (n_lcols == 0) return KMAP_OK;
    const dim3 grid(grid_for(n_qcols, MM_QB), (unsigned)std::min<int64_t>(grid_for(n_lcols, MM_TPB), MM_HIST_TILES));
    hist_kernel<<<grid, MM_TPB, 0, st>>>((const uint2 *)qcols_dev, n_qcols, (const uint2 *)lcols_dev, n_lcols, revcom ? 1 : 0, hist_dev);
    KMAP_CHECK_HIP(hipGetLastError());
    return KMAP_OK;
}

int kmap_match_tables_dev(const uint32_t *hist_dev, int64_t n_qcols, int64_t n_null, int n_query, const int32_t *q_width,
                          const int64_t *q_col0, const int32_t *q_min_len, const int64_t *q_toff, double *tables_dev, int64_t n_table,
                          void *stream) {
    KMAP_REQUIRE(n_query >= 0 && n_qcols >= 0 && n_table >= 0, "match_tables: negative size");
    if (n_query == 0) return KMAP_OK;
    KMAP_REQUIRE(hist_dev && tables_dev, "match_tables: null pointer");
    KMAP_REQUIRE(n_null >= 1, "match_tables: n_null=%lld < 1", (long long)n_null);
    std::vector<QueryMeta> meta;
    KMAP_TRY(pack_queries("match_tables", n_query, q_width, q_col0, q_min_len, q_toff, n_qcols, n_table, &meta));
    hipStream_t st = as_stream(stream);
    QueryMeta *meta_dev = nullptr;
    KMAP_TRY(kmap_scratch((void **)&meta_dev, meta.size() * sizeof(QueryMeta), st, KMAP_SLOT_A));
    KMAP_CHECK_HIP(hipMemcpyAsync(meta_dev, meta.data(), meta.size() * sizeof(QueryMeta), hipMemcpyHostToDevice, st));
    KMAP_CHECK_HIP(hipStreamSynchronize(st));        // `meta` is pageable and ends with this call
    KMAP_TRY(kmap_allow_lds((const void *)tables_kernel, MM_TABLE_LDS));
    tables_kernel<<<(unsigned)n_query, MM_TPB, MM_TABLE_LDS, st>>>(hist_dev, (double)n_null, meta_dev, tables_dev);
    KMAP_CHECK_HIP(hipGetLastError());
    return KMAP_OK;
}

int kmap_match_pairs_dev(const uint16_t *qcols_dev, int64_t n_qcols, int n_query, const int32_t *q_width, const int64_t *q_col0,
                         const int32_t *q_min_len, const int64_t *q_toff, const double *tables_dev, int64_t n_table,
                         const uint16_t *lcols_dev, int64_t n_lcols, int n_target, const int32_t *t_width, const int64_t *t_col0,
                         int min_overlap, int revcom, double *p_dev, int32_t *cfg_dev, void *stream) {
    KMAP_REQUIRE(n_query >= 0 && n_target >= 0 && n_qcols >= 0 && n_lcols >= 0 && n_table >= 0, "match_pairs: negative size");
    KMAP_REQUIRE(min_overlap >= 1, "match_pairs: min_overlap=%d < 1", min_overlap);
    if (n_query == 0 || n_target == 0) return KMAP_OK;
    KMAP_REQUIRE(qcols_dev && lcols_dev && tables_dev && p_dev && cfg_dev && t_width && t_col0, "match_pairs: null pointer");
    KMAP_REQUIRE(n_query <= 65535, "match_pairs: %d queries in one call, at most 65535", n_query);
    std::vector<QueryMeta> qmeta;
    KMAP_TRY(pack_queries("match_pairs", n_query, q_width, q_col0, q_min_len, q_toff, n_qcols, n_table, &qmeta));
    std::vector<TargetMeta> tmeta((size_t)n_target);
    int min_tw = MM_MAX_W;
    for (int t = 0; t < n_target; ++t) {
        const int w = t_width[t];
        KMAP_REQUIRE(w >= MM_MIN_W && w <= MM_MAX_W, "match_pairs: width=%d of target %d outside 4..31", w, t);
        KMAP_REQUIRE(t_col0[t] >= 0 && t_col0[t] + w <= n_lcols, "match_pairs: the columns of target %d lie outside the %lld library columns",
                     t, (long long)n_lcols);
        tmeta[(size_t)t] = {t_col0[t], w, 0};
        min_tw = std::min(min_tw, w);
    }
    for (int q = 0; q < n_query; ++q)                // every overlap the pairs can ask for has its table
        KMAP_REQUIRE(q_min_len[q] <= std::min(min_overlap, min_tw), "match_pairs: min_len=%d of query %d, but overlaps go down to %d columns",
                     q_min_len[q], q, std::min(min_overlap, std::min(min_tw, q_width[q])));
    hipStream_t st = as_stream(stream);
    QueryMeta *q_dev = nullptr;
    TargetMeta *t_dev = nullptr;
    KMAP_TRY(kmap_scratch((void **)&q_dev, qmeta.size() * sizeof(QueryMeta), st, KMAP_SLOT_A));
    KMAP_TRY(kmap_scratch((void **)&t_dev, tmeta.size() * sizeof(TargetMeta), st, KMAP_SLOT_B));
    KMAP_CHECK_HIP(hipMemcpyAsync(q_dev, qmeta.data(), qmeta.size() * sizeof(QueryMeta), hipMemcpyHostToDevice, st));
    KMAP_CHECK_HIP(hipMemcpyAsync(t_dev, tmeta.data(), tmeta.size() * sizeof(TargetMeta), hipMemcpyHostToDevice, st));
    KMAP_CHECK_HIP(hipStreamSynchronize(st));        // the two vectors are pageable and end with this call
    const dim3 grid(grid_for(n_target, MM_WAVES), (unsigned)n_query);
    pairs_kernel<<<grid, MM_TPB, 0, st>>>((const uint2 *)qcols_dev, q_dev, tables_dev, (const uint2 *)lcols_dev, t_dev, n_target, min_overlap,
                                          revcom ? 1 : 0, p_dev, (int4 *)cfg_dev);
    KMAP_CHECK_HIP(hipGetLastError());
    return KMAP_OK;
}

}  // extern "C"
