// counts_io.hip -- the counted table's way out of the device: blocking and stream-ordered fetches into host arrays (pinned staging,
// conversion to the reference's dtypes on host threads), ranges written straight into a file, and the table's device addresses.
#include <errno.h>
#include <string.h>
#include <unistd.h>

#include <algorithm>
#include <mutex>
#include <type_traits>
#include <vector>

#include "common.h"
#include "counts_internal.h"
#include "host_pool.h"

extern "C" {

int kmap_counts_fetch(kmap_counts *c, void *uniq_out, void *cnt_out) {
    KMAP_REQUIRE(c && c->k > 0, "counts_fetch: nothing counted yet");
    if (c->n_uniq == 0) return KMAP_OK;
    KMAP_REQUIRE(uniq_out && cnt_out, "counts_fetch: null output");
    const size_t n = (size_t)c->n_uniq;
    KMAP_CHECK_HIP(hipMemcpy(uniq_out, c->uniq, n * (c->narrow ? 4 : 8), hipMemcpyDeviceToHost));
    if (c->narrow) {
        KMAP_CHECK_HIP(hipMemcpy(cnt_out, c->cnt, n * 4, hipMemcpyDeviceToHost));   // uint32 bits == int32 wrap
    } else {
        uint32_t *tmp = (uint32_t *)malloc(n * 4);
        KMAP_REQUIRE(tmp, "counts_fetch: host malloc");
        hipError_t e = hipMemcpy(tmp, c->cnt, n * 4, hipMemcpyDeviceToHost);
        if (e == hipSuccess)   // widen uint32 -> int64 on several host threads (10^9 entries at k = 16)
            kmap_convert_pool<uint32_t, int64_t>((int64_t *)cnt_out, tmp, n, kmap_io_threads());
        free(tmp);
        KMAP_CHECK_HIP(e);
    }
    return KMAP_OK;
}

}  // extern "C"

namespace {
// device -> host copy of n elements through two pinned staging buffers on `st`, converted on host threads while the next chunk is
// in flight: SRC (device element) -> DST (host element), e.g. uint32 -> int64.  A plain hipMemcpy into pageable numpy memory runs
// at ~16 GB/s and, on the null stream, would also serialise with the kernels of the trials that follow; this path keeps the
// transfer on its own stream (SDMA next to the kernels) and reaches the host-side memory bandwidth.
// pinned staging buffers are kept in a process-wide free list (hipHostMalloc costs ~75 ms per 256 MiB: more than the whole copy
// of a 1-GB table); concurrent fetches (two TableSaver threads) each take their own pair
constexpr size_t STAGE_BYTES = (size_t)256 << 20;
std::mutex g_stage_mu;
std::vector<void *> g_stage_free;
struct StagePair {
    void *buf[2] = {nullptr, nullptr};
    StagePair() {
        std::lock_guard<std::mutex> lk(g_stage_mu);
        for (int b = 0; b < 2; ++b) {
            if (!g_stage_free.empty()) {
                buf[b] = g_stage_free.back();
                g_stage_free.pop_back();
            } else if (hipHostMalloc(&buf[b], STAGE_BYTES, hipHostMallocDefault) != hipSuccess) {
                buf[b] = nullptr;
            }
        }
    }
    bool ok() const { return buf[0] && buf[1]; }
    ~StagePair() {
        std::lock_guard<std::mutex> lk(g_stage_mu);
        for (int b = 0; b < 2; ++b)
            if (buf[b]) g_stage_free.push_back(buf[b]);
    }
};

template <typename SRC, typename DST>
int staged_fetch(DST *dst, const SRC *src_dev, size_t n, hipStream_t st) {
    if (n == 0) return KMAP_OK;
    StagePair sp;                                                 // two pinned 256-MiB buffers from the process-wide pool
    if (!sp.ok()) {
        kmap_set_error("counts_fetch: pinned staging allocation failed");
        return KMAP_E_NOMEM;
    }
    const size_t chunk = STAGE_BYTES / sizeof(SRC);               // elements per chunk
    SRC *stage[2] = {(SRC *)sp.buf[0], (SRC *)sp.buf[1]};
    const unsigned nt = kmap_io_threads();
    hipError_t err = hipSuccess;
    size_t off = 0;
    int b = 0;
    size_t len = std::min(chunk, n);
    err = hipMemcpyAsync(stage[0], src_dev, len * sizeof(SRC), hipMemcpyDeviceToHost, st);
    while (err == hipSuccess && off < n) {
        err = hipStreamSynchronize(st);                           // chunk `b` has landed
        if (err != hipSuccess) break;
        const size_t next_off = off + len, next_len = next_off < n ? std::min(chunk, n - next_off) : 0;
        if (next_len) err = hipMemcpyAsync(stage[b ^ 1], src_dev + next_off, next_len * sizeof(SRC), hipMemcpyDeviceToHost, st);
        kmap_convert_pool<SRC, DST>(dst + off, stage[b], len, nt);  // the destination may be an unaligned view into a memory-mapped pickle file (TableSaver)
        off = next_off;
        len = next_len;
        b ^= 1;
    }
    if (err != hipSuccess) (void)hipStreamSynchronize(st);
    KMAP_CHECK_HIP(err);
    return KMAP_OK;
}

// counts widened to the reference's int64 on the device (k >= 16): the bytes that cross PCIe are the bytes of the file
__global__ __launch_bounds__(256) void widen_counts_kernel(const uint32_t *__restrict__ in, int64_t n, int64_t *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = (int64_t)in[i];
}

// `n` elements of a device array -> file bytes at `file_off`, in the file's dtype DST: chunk i + 1 crosses PCIe into one pinned
// staging buffer while chunk i is written from the other -- no pageable copy, no conversion pass on the host (WIDEN: the uint32
// counts become int64 on the device, in a scratch buffer the size of a chunk)
template <typename SRC, typename DST>
int staged_write(int fd, int64_t file_off, const SRC *src_dev, size_t n, hipStream_t st) {
    if (n == 0) return KMAP_OK;
    constexpr bool WIDEN = !std::is_same<SRC, DST>::value;
    StagePair sp;
    if (!sp.ok()) {
        kmap_set_error("counts_write: pinned staging allocation failed");
        return KMAP_E_NOMEM;
    }
    const size_t chunk = STAGE_BYTES / sizeof(DST);
    DevBuf wide[2];
    if (WIDEN) {
        KMAP_TRY(wide[0].alloc(std::min(chunk, n) * sizeof(DST)));
        KMAP_TRY(wide[1].alloc(std::min(chunk, n) * sizeof(DST)));
    }
    auto issue = [&](int b, size_t off, size_t len) -> hipError_t {
        const void *from = src_dev + off;
        if (WIDEN) {
            widen_counts_kernel<<<(unsigned)((len + 255) / 256), 256, 0, st>>>((const uint32_t *)(src_dev + off), (int64_t)len, wide[b].as<int64_t>());
            from = wide[b].p;
        }
        return hipMemcpyAsync(sp.buf[b], from, len * sizeof(DST), hipMemcpyDeviceToHost, st);
    };
    size_t off = 0, len = std::min(chunk, n);
    int b = 0;
    hipError_t err = issue(0, 0, len);
    while (err == hipSuccess && off < n) {
        err = hipStreamSynchronize(st);                           // chunk `b` has landed
        if (err != hipSuccess) break;
        const size_t next_off = off + len, next_len = next_off < n ? std::min(chunk, n - next_off) : 0;
        if (next_len) err = issue(b ^ 1, next_off, next_len);
        if (!kmap_pwrite_all(fd, (const char *)sp.buf[b], len * sizeof(DST), file_off + (int64_t)(off * sizeof(DST)))) {
            const int en = errno;
            (void)hipStreamSynchronize(st);
            kmap_set_error("counts_write: pwrite failed: %s", strerror(en));
            return KMAP_E_IO;
        }
        off = next_off;
        len = next_len;
        b ^= 1;
    }
    if (err != hipSuccess) (void)hipStreamSynchronize(st);
    KMAP_CHECK_HIP(err);
    return KMAP_OK;
}

// uint64 keys that fit 32 bits (k = 16): narrowed on the device so that half the bytes cross PCIe
__global__ __launch_bounds__(256) void narrow_keys_kernel(const uint64_t *__restrict__ in, int64_t n, uint32_t *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = (uint32_t)in[i];
}
}  // namespace

extern "C" {

/* device addresses of the resident table (uniq: uint32 for k < 16 else uint64; cnt: uint32 whatever k), valid until the next
 * count / load / destroy on this handle */
int kmap_counts_table_dev(kmap_counts *c, void **uniq_dev, void **cnt_dev, int64_t *n_uniq) {
    KMAP_REQUIRE(c && c->k > 0 && uniq_dev && cnt_dev && n_uniq, "counts_table_dev: nothing counted yet / null output");
    *uniq_dev = c->uniq;
    *cnt_dev = (void *)c->cnt;
    *n_uniq = c->n_uniq;
    return KMAP_OK;
}

/* kmap_counts_fetch on a caller-chosen stream (so that a background host thread can drain a finished table while the null
 * stream keeps counting into ANOTHER handle): pinned staging, conversion on host threads.  Blocks until the arrays are complete. */
int kmap_counts_fetch_stream(kmap_counts *c, void *uniq_out, void *cnt_out, void *stream) {
    KMAP_REQUIRE(c && c->k > 0, "counts_fetch: nothing counted yet");
    if (c->n_uniq == 0) return KMAP_OK;
    KMAP_REQUIRE(uniq_out && cnt_out, "counts_fetch: null output");
    hipStream_t st = as_stream(stream);
    const size_t n = (size_t)c->n_uniq;
    if (c->narrow) {
        KMAP_TRY((staged_fetch<uint32_t, uint32_t>((uint32_t *)uniq_out, (const uint32_t *)c->uniq, n, st)));
        KMAP_TRY((staged_fetch<uint32_t, uint32_t>((uint32_t *)cnt_out, c->cnt, n, st)));   // uint32 bits == int32 wrap
    } else {
        if (c->k <= 16) {
            DevBuf k32;
            KMAP_TRY(k32.alloc(n * 4));
            narrow_keys_kernel<<<(unsigned)((n + 255) / 256), 256, 0, st>>>((const uint64_t *)c->uniq, (int64_t)n, k32.as<uint32_t>());
            KMAP_CHECK_HIP(hipGetLastError());
            KMAP_TRY((staged_fetch<uint32_t, uint64_t>((uint64_t *)uniq_out, k32.as<uint32_t>(), n, st)));
        } else {
            KMAP_TRY((staged_fetch<uint64_t, uint64_t>((uint64_t *)uniq_out, (const uint64_t *)c->uniq, n, st)));
        }
        KMAP_TRY((staged_fetch<uint32_t, int64_t>((int64_t *)cnt_out, c->cnt, n, st)));
    }
    return KMAP_OK;
}

/* a range of one array of the table straight into a file: which = 0 the unique hashes (uint32 for k < 16, uint64 otherwise), which = 1
 * the counts (int32 / int64).  The range's bytes, in the reference's dtype, are written at `file_offset` of the open descriptor `fd`
 * (pwrite: the descriptor's position is not used) from pinned staging buffers on `stream`, the next chunk in flight while the
 * current one is written: a multi-GB table reaches its file without being held in host memory.  The k{k}.pkl writers place the array payloads of a pickle whose layout they know this way. */
int kmap_counts_write_range(kmap_counts *c, int which, int64_t first, int64_t count, int fd, int64_t file_offset, void *stream) {
    KMAP_REQUIRE(c && c->k > 0 && (which == 0 || which == 1), "counts_write_range: nothing counted yet / bad selector");
    KMAP_REQUIRE(first >= 0 && count >= 0 && first + count <= c->n_uniq, "counts_write_range: range outside the table");
    KMAP_REQUIRE(fd >= 0 && file_offset >= 0, "counts_write_range: bad file descriptor / offset");
    if (count == 0) return KMAP_OK;
    hipStream_t st = as_stream(stream);
    const size_t n = (size_t)count;
    if (which == 0) {
        if (c->narrow) return staged_write<uint32_t, uint32_t>(fd, file_offset, (const uint32_t *)c->uniq + first, n, st);
        return staged_write<uint64_t, uint64_t>(fd, file_offset, (const uint64_t *)c->uniq + first, n, st);
    }
    if (c->narrow) return staged_write<uint32_t, uint32_t>(fd, file_offset, c->cnt + first, n, st);   // uint32 bits == int32 wrap
    return staged_write<uint32_t, int64_t>(fd, file_offset, c->cnt + first, n, st);
}

}  // extern "C"
