// host_pool.h -- the building blocks of the native host I/O (host_io.hip, host_bed.hip, the fetch and write paths of counts_io.hip):
// thread count, parallel loop, conversion pool, line cutter, pwrite in full, chunk buffers and their writer, decimal text of an
// integer, read-only file mapping.  Plain host C++17, no HIP types and no common.h: the CPU sanitizer harnesses (tests/host_san,
// tests/host_san_bed) compile it with -fsanitize=address,undefined and -fsanitize=thread, and a free-standing program can include it
// alone.
#pragma once
#include <errno.h>
#include <fcntl.h>
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <exception>
#include <memory>
#include <thread>
#include <type_traits>
#include <vector>

// Host threads of one I/O call: min(max(1, hardware_concurrency()), cap), cap = KMAP_IO_THREADS (at least 1), else 16 (several
// writers run at once in scan_motif).  The environment is read on every call, so a process may change the switch between calls.
// getenv is safe against concurrent getenv, not against a concurrent setenv: the package's only writes of os.environ are e2e.py's
// (KMAP_EMBED_MODE, before and after a whole run), and _scan_motif joins or closes every background writer before it returns, so
// no native I/O thread is alive when they happen.
inline unsigned kmap_io_threads() {
    const char *v = getenv("KMAP_IO_THREADS");
    const int cap = v ? std::max(1, atoi(v)) : 16;
    return (unsigned)std::min<int>((int)std::max(1u, std::thread::hardware_concurrency()), cap);
}

// fn(i) for i in [0, n) on up to `nt` threads, handed out by an atomic counter.  The calling thread takes its share; threads that
// cannot be started are not missed.  An exception of fn is caught on the thread that threw, the indices not yet handed out are
// abandoned, every thread is joined, and the first exception is re-thrown here: nothing propagates out of a std::thread.
template <typename F>
void kmap_parallel_for(size_t n, unsigned nt, F fn) {
    std::atomic<size_t> next{0};
    std::atomic<bool> failed{false};
    std::exception_ptr first;                                         // written by the one thread that sets `failed`, read after the joins
    auto worker = [&]() {
        try {
            for (size_t i; (i = next.fetch_add(1)) < n;) fn(i);
        } catch (...) {
            if (!failed.exchange(true)) first = std::current_exception();
            next.store(n);
        }
    };
    std::vector<std::thread> pool;
    try {
        for (unsigned t = 1; t < nt && t < n; ++t) pool.emplace_back(worker);
    } catch (...) {
    }
    worker();
    for (auto &th : pool) th.join();
    if (first) std::rethrow_exception(first);
}

// dst[i] = (DST)src[i] for i in [0, n) in `nt` equal shares on up to `nt` threads (n < 65536: one).  `dst` may be unaligned (a view
// into a memory-mapped pickle file: byte-wise typed stores).  Never throws across the caller (a C ABI function).
template <typename SRC, typename DST>
inline void kmap_convert_pool(DST *dst, const SRC *src, size_t n, unsigned nt) {
    typedef DST __attribute__((aligned(1))) DSTu;
    if (nt < 1) nt = 1;
    if (n < ((size_t)1 << 16)) nt = 1;                                // not worth a thread
    kmap_parallel_for(nt, nt, [=](size_t t) {
        const size_t lo = n * t / nt, hi = n * (t + 1) / nt;
        if (std::is_same<SRC, DST>::value) {
            memcpy((void *)((char *)dst + lo * sizeof(DST)), (const void *)(src + lo), (hi - lo) * sizeof(SRC));
        } else {
            DSTu *du = (DSTu *)dst;
            for (size_t i = lo; i < hi; ++i) du[i] = (DST)src[i];
        }
    });
}

// [lo, n) of the text `p` cut behind newlines into ranges of >= min_chunk (>= 1) bytes, at most 4 per thread: the cuts, ascending
// from lo to n.  An empty [lo, n) has no range: {lo}.
inline std::vector<size_t> kmap_cut_lines(const char *p, size_t lo, size_t n, unsigned threads, size_t min_chunk) {
    std::vector<size_t> cut{lo};
    if (lo >= n) return cut;
    const size_t len = n - lo;
    const size_t want = std::max<size_t>(1, std::min<size_t>((size_t)threads * 4, len / min_chunk));
    for (size_t t = 1; t < want; ++t) {
        const size_t from = std::max(cut.back(), lo + (len / want) * t);
        if (from >= n) break;
        const char *nl = (const char *)memchr(p + from, '\n', n - from);
        if (!nl || (size_t)(nl - p) + 1 >= n) break;
        const size_t at = (size_t)(nl - p) + 1;
        if (at > cut.back()) cut.push_back(at);
    }
    cut.push_back(n);
    return cut;
}

// pwrite() in full (short writes, EINTR); false + errno on failure (a write of nothing: EIO)
inline bool kmap_pwrite_all(int fd, const char *buf, size_t len, int64_t off) {
    while (len) {
        const ssize_t w = pwrite(fd, buf, len, (off_t)off);
        if (w < 0 && errno == EINTR) continue;
        if (w <= 0) {
            if (w == 0) errno = EIO;
            return false;
        }
        buf += w;
        off += w;
        len -= (size_t)w;
    }
    return true;
}

// a descriptor that is closed on every way out
struct KmapFd {
    int fd;
    explicit KmapFd(int f = -1) : fd(f) {}
    KmapFd(const KmapFd &) = delete;
    KmapFd &operator=(const KmapFd &) = delete;
    ~KmapFd() { (void)close(); }
    int close() {
        const int rc = fd >= 0 ? ::close(fd) : 0;
        fd = -1;
        return rc;
    }
};

// One formatted piece of an output file.  Uninitialised memory: a vector<char>::resize would zero-fill (and page-fault) every byte
// before it is formatted over.
struct KmapChunk {
    std::unique_ptr<char[]> mem;
    size_t len = 0;
};
// The chunks go back to back to their final offsets behind base_off with parallel pwrite()s (one memcpy into the page cache per
// thread instead of one serial stream: 185 MB per occurrence file at C3) on at most 2 threads: there is one inode lock, more
// threads only wait (measured with 4..64: 21-27 ms).  Returns the offset behind the last chunk, or -1 + errno.
inline int64_t kmap_write_chunks(int fd, int64_t base_off, const std::vector<KmapChunk> &chunks, unsigned nt) {
    std::vector<int64_t> off(chunks.size() + 1, base_off);
    for (size_t i = 0; i < chunks.size(); ++i) off[i + 1] = off[i] + (int64_t)chunks[i].len;
    std::atomic<int> err{0};
    kmap_parallel_for(chunks.size(), std::min(nt, 2u), [&](size_t i) {
        if (!err.load() && !kmap_pwrite_all(fd, chunks[i].mem.get(), chunks[i].len, off[i])) err.store(errno);
    });
    if (err.load()) {
        errno = err.load();
        return -1;
    }
    return off.back();
}

// decimal text of 0..9999: four characters (left-aligned, and zero-padded) + the length of the unpadded form.  The CSV rows
// are nothing but small integers -- read index, positions < read length, read length -- so one lookup and one 4-byte store
// per number replaces the digit loop (8 M rows per file at C3: 50 -> ~15 ns per row and core)
struct KmapDec4 {
    char plain[10000][4];
    char padded[10000][4];
    unsigned char len[10000];
    KmapDec4() {
        for (int v = 0; v < 10000; ++v) {
            const char d[4] = {(char)('0' + v / 1000), (char)('0' + v / 100 % 10), (char)('0' + v / 10 % 10), (char)('0' + v % 10)};
            const int skip = v >= 1000 ? 0 : v >= 100 ? 1 : v >= 10 ? 2 : 3;
            for (int i = 0; i < 4; ++i) {
                padded[v][i] = d[i];
                plain[v][i] = i + skip < 4 ? d[i + skip] : '0';
            }
            len[v] = (unsigned char)(4 - skip);
        }
    }
};
inline const KmapDec4 g_kmap_dec4;

// append the decimal form of v to p (which has >= 4 bytes of slack behind the number), return the new end
inline char *kmap_put_int(char *p, int64_t v) {
    if (v >= 0 && v < 10000) {
        memcpy(p, g_kmap_dec4.plain[v], 4);
        return p + g_kmap_dec4.len[v];
    }
    if (v >= 0 && v < 100000000) {
        const int hi = (int)(v / 10000), lo = (int)(v % 10000);
        memcpy(p, g_kmap_dec4.plain[hi], 4);
        p += g_kmap_dec4.len[hi];
        memcpy(p, g_kmap_dec4.padded[lo], 4);
        return p + 4;
    }
    uint64_t u = (uint64_t)v;
    if (v < 0) {                                                      // through uint64: INT64_MIN has no int64 negation
        *p++ = '-';
        u = 0ull - u;
    }
    char tmp[24];
    int n = 0;
    do { tmp[n++] = (char)('0' + u % 10); u /= 10; } while (u);
    while (n) *p++ = tmp[--n];
    return p;
}

// A file opened read-only and, where it is a regular, non-empty file that mmap accepts, its bytes (MAP_PRIVATE | MAP_POPULATE).
// The descriptor stays open until file.close() or the end, for a caller's own look at the file (gzip magic) or its fall-back
// (read()) for what is not mappable.
struct KmapMappedFile {
    KmapFd file;
    size_t n = 0;                       // size of a regular file (0: anything else), mapped or not
    const char *p = nullptr;            // the n mapped bytes, or null
    ~KmapMappedFile() {
        if (p) munmap((void *)p, n);
    }
    bool open(const char *path) {       // false + errno: cannot open
        file.fd = ::open(path, O_RDONLY | O_CLOEXEC);
        if (file.fd < 0) return false;
        struct stat sb;
        if (fstat(file.fd, &sb) == 0 && S_ISREG(sb.st_mode) && sb.st_size > 0) n = (size_t)sb.st_size;
        return true;
    }
    bool map() {                        // true: regular, non-empty, mapped; false: not mappable
        if (!n || p) return p != nullptr;
        void *m = mmap(nullptr, n, PROT_READ, MAP_PRIVATE | MAP_POPULATE, file.fd, 0);
        if (m != MAP_FAILED) p = (const char *)m;
        return p != nullptr;
    }
};
