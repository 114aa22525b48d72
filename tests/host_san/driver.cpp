// tests/host_san/driver.cpp -- CPU sanitizer harness for the threaded HOST code of libkmap_hip (test infrastructure, never shipped):
// the FASTA(.gz) reader and the occurrence-CSV formatter + pwrite pool of kmap_amd/csrc/host_io.hip, and the conversion pool of
// kmap_amd/csrc/host_pool.h (used by counts_io.hip's table fetch).  Built twice by the Makefile next to it -- -fsanitize=address,undefined
// and -fsanitize=thread -- from the product's own sources compiled host-only; tests/test_host_sanitizers.py drives it.
//   driver fasta <in.fa[.gz]> <seq.bin> <borders.bin>      arrays as kmap_fasta_open / _read return them
//   driver csv <out_i32.csv> <out_u8.csv> <n_seq> <seed>    the same synthetic hit lists through both CSV entry points
//   driver pool <n>                                         u32 -> i64 (unaligned destination), u32 -> u64, u32 -> u32 conversions
//   driver f2 <values.f64> <out.tsv> <medians.f64>          the "%.2f" line writer of the co-occurrence file and the per-read medians
//   driver par | cut | int                                  kmap_parallel_for (every index once; a body's exception), kmap_cut_lines
//                                                           (the ranges' properties), kmap_put_int (against snprintf) of host_pool.h
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <cmath>
#include <new>
#include <string>
#include <vector>

#include "../../include/kmap_hip.h"
#include "../../kmap_amd/csrc/host_pool.h"

static char g_err[512];
void kmap_set_error(const char *fmt, ...) {      // api_core.hip's thread-local message buffer is device-side code's; a plain one here
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
}

static int fail(const char *what, int rc) {
    fprintf(stderr, "driver: %s failed (rc %d): %s\n", what, rc, g_err);
    return 2;
}
static bool dump(const char *path, const void *p, size_t bytes) {
    FILE *fh = fopen(path, "wb");
    if (!fh) return false;
    const bool ok = bytes == 0 || fwrite(p, 1, bytes, fh) == bytes;
    return fclose(fh) == 0 && ok;
}

int main(int argc, char **argv) {
    if (argc >= 5 && !strcmp(argv[1], "fasta")) {
        kmap_fasta *f = nullptr;
        int64_t nb = 0, ns = 0;
        int rc = kmap_fasta_open(argv[2], &f, &nb, &ns);
        if (rc != KMAP_OK) return fail("kmap_fasta_open", rc);
        std::vector<uint8_t> seq((size_t)nb);
        std::vector<int64_t> borders((size_t)ns * 2);
        rc = kmap_fasta_read(f, seq.data(), borders.data());
        if (rc != KMAP_OK) return fail("kmap_fasta_read", rc);
        kmap_fasta_close(f);
        if (!dump(argv[3], seq.data(), seq.size()) || !dump(argv[4], borders.data(), borders.size() * 8)) return fail("dump", -1);
        printf("%lld %lld\n", (long long)nb, (long long)ns);
        return 0;
    }
    if (argc >= 6 && !strcmp(argv[1], "csv")) {
        const int64_t n_seq = atoll(argv[4]);
        uint64_t x = strtoull(argv[5], nullptr, 10) * 2862933555777941757ull + 3037000493ull;
        auto rnd = [&]() { x = x * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(x >> 33); };
        const int n_cons = 3;
        std::vector<int32_t> hits[3], pos[3];
        std::vector<uint8_t> hits8[3];
        std::vector<int64_t> read_len((size_t)n_seq);
        for (int64_t s = 0; s < n_seq; ++s) read_len[(size_t)s] = 30 + rnd() % 20000;     // numbers on both sides of the 4- and 8-digit fast paths
        for (int c = 0; c < n_cons; ++c) {
            hits[c].resize((size_t)n_seq);
            hits8[c].resize((size_t)n_seq);
            for (int64_t s = 0; s < n_seq; ++s) {
                const uint32_t r = rnd() % 16;
                const int h = r < 10 ? 0 : r < 14 ? 1 : (int)(rnd() % 21);
                hits[c][(size_t)s] = h;
                hits8[c][(size_t)s] = (uint8_t)h;
                int32_t p = 0;
                for (int i = 0; i < h; ++i) {
                    p += (int32_t)(rnd() % 997);
                    pos[c].push_back(p);
                }
            }
            if (pos[c].empty()) pos[c].push_back(0);
        }
        const int32_t *hp[3] = {hits[0].data(), hits[1].data(), hits[2].data()};
        const uint8_t *hp8[3] = {hits8[0].data(), hits8[1].data(), hits8[2].data()};
        const int32_t *pp[3] = {pos[0].data(), pos[1].data(), pos[2].data()};
        int64_t rows = 0, rows8 = 0;
        int rc = kmap_write_occurrence_csv(argv[2], "seq_ind;motif_0_A;motif_1_C;motif_2_G;seq_len", n_seq, n_cons, hp, pp, read_len.data(), &rows);
        if (rc != KMAP_OK) return fail("kmap_write_occurrence_csv", rc);
        rc = kmap_write_occurrence_csv_u8(argv[3], "seq_ind;motif_0_A;motif_1_C;motif_2_G;seq_len", n_seq, n_cons, hp8, pp, read_len.data(), &rows8);
        if (rc != KMAP_OK) return fail("kmap_write_occurrence_csv_u8", rc);
        rc = kmap_write_occurrence_csv("/nonexistent-dir/x.csv", "h", n_seq, n_cons, hp, pp, read_len.data(), &rows8);
        if (rc == KMAP_OK) return fail("write to a missing directory must fail", rc);
        printf("%lld\n", (long long)rows);
        return rows == rows8 ? 0 : 3;
    }
    if (argc >= 3 && !strcmp(argv[1], "pool")) {
        const size_t n = (size_t)atoll(argv[2]);
        std::vector<uint32_t> src(n);
        for (size_t i = 0; i < n; ++i) src[i] = (uint32_t)(i * 2654435761u);
        std::vector<char> raw(n * 8 + 16);
        int64_t *un = (int64_t *)(raw.data() + 3);                           // deliberately unaligned (the pickle-file view)
        kmap_convert_pool<uint32_t, int64_t>(un, src.data(), n, 7);
        for (size_t i = 0; i < n; i += (n / 1000) + 1) {
            int64_t v;
            memcpy(&v, raw.data() + 3 + i * 8, 8);
            if (v != (int64_t)src[i]) return fail("u32 -> i64", (int)i);
        }
        std::vector<uint64_t> w(n);
        kmap_convert_pool<uint32_t, uint64_t>(w.data(), src.data(), n, 16);
        std::vector<uint32_t> same(n);
        kmap_convert_pool<uint32_t, uint32_t>(same.data(), src.data(), n, 3);
        for (size_t i = 0; i < n; ++i)
            if (w[i] != src[i] || same[i] != src[i]) return fail("u32 -> u64 / u32", (int)i);
        kmap_convert_pool<uint32_t, uint64_t>(w.data(), src.data(), 0, 4);  // empty
        printf("%zu\n", n);
        return 0;
    }
    if (argc >= 5 && !strcmp(argv[1], "f2")) {      // driver f2 <values.f64> <out.tsv> <medians.f64>: the "%.2f" line writer + the cell medians
        FILE *fh = fopen(argv[2], "rb");
        if (!fh) return fail("open values", -1);
        std::vector<double> v;
        double x;
        while (fread(&x, 8, 1, fh) == 1) v.push_back(x);
        fclose(fh);
        FILE *out = fopen(argv[3], "wb");
        if (!out) return fail("open output", -1);
        fputs("pair\n", out);
        fflush(out);
        int rc = kmap_write_f2_tsv_line(fileno(out), v.data(), (int64_t)v.size());
        if (rc == KMAP_OK) rc = kmap_write_f2_tsv_line(fileno(out), nullptr, 0);          // an empty line
        fclose(out);
        if (rc != KMAP_OK) return fail("kmap_write_f2_tsv_line", rc);
        if (kmap_write_f2_tsv_line(-1, v.data(), 1) == KMAP_OK) return fail("a bad descriptor must fail", 0);
        // medians: cells of 0..4 ascending locations cut from the values' integer parts
        std::vector<int32_t> hits, pos;
        size_t at = 0;
        for (size_t r = 0; at < v.size() && r < 200000; ++r) {
            const int h = (int)(r % 5);
            int32_t p = 0;
            int got = 0;
            for (; got < h && at < v.size(); ++got, ++at) {
                const double a = std::isfinite(v[at]) ? std::fabs(v[at]) : 0.0;
                p += (int32_t)std::fmod(a, 1000.0);
                pos.push_back(p);
            }
            hits.push_back(got);
        }
        std::vector<double> med(hits.size());
        rc = kmap_cell_medians_i32(hits.data(), pos.data(), (int64_t)hits.size(), (int64_t)pos.size(), med.data());
        if (rc != KMAP_OK) return fail("kmap_cell_medians_i32", rc);
        if (!hits.empty() && kmap_cell_medians_i32(hits.data(), pos.data(), (int64_t)hits.size(), (int64_t)pos.size() + 1, med.data()) == KMAP_OK)
            return fail("hit counts that do not add up must fail", 0);
        std::vector<double> packed;                                                         // hits, then positions, then medians, as f64
        for (int32_t h : hits) packed.push_back(h);
        for (int32_t p : pos) packed.push_back(p);
        for (double m : med) packed.push_back(m);
        if (!dump(argv[4], packed.data(), packed.size() * 8)) return fail("dump", -1);
        printf("%zu %zu %zu\n", v.size(), hits.size(), pos.size());
        return 0;
    }
    if (argc >= 2 && !strcmp(argv[1], "par")) {     // driver par: kmap_parallel_for visits every index once; an exception of the body ends on this thread
        for (unsigned nt : {1u, 3u, 16u})
            for (size_t n : {(size_t)0, (size_t)1, (size_t)nt - 1, (size_t)nt, (size_t)nt + 1, (size_t)100000}) {
                std::vector<int> seen(n, 0);
                kmap_parallel_for(n, nt, [&](size_t i) { ++seen[i]; });
                for (size_t i = 0; i < n; ++i)
                    if (seen[i] != 1) return fail("par: an index was not visited exactly once", (int)i);
            }
        const struct { size_t n, at; unsigned nt; } cases[] = {{10000, 5000, 8}, {10000, 0, 8}, {10000, 0, 1}};
        for (const auto &c : cases) {
            std::vector<int> seen(c.n, 0);
            std::atomic<int> running{0};
            bool caught = false;
            try {
                kmap_parallel_for(c.n, c.nt, [&](size_t i) {
                    struct In { std::atomic<int> &r; In(std::atomic<int> &r_) : r(r_) { ++r; } ~In() { --r; } } in(running);
                    ++seen[i];
                    if (i == c.at) throw std::bad_alloc();
                });
            } catch (const std::bad_alloc &) {
                caught = true;
            }
            if (!caught) return fail("par: the body's bad_alloc did not arrive on the calling thread", (int)c.nt);
            if (running.load() != 0) return fail("par: a thread is still in the body after the call", running.load());
            if (seen[c.at] != 1) return fail("par: the throwing index was not visited once", seen[c.at]);
            size_t visited = 0;
            for (size_t i = 0; i < c.n; ++i) {
                if (seen[i] > 1) return fail("par: an index was visited twice", (int)i);
                visited += (size_t)seen[i];
            }
            if (c.nt == 1 && visited != c.at + 1) return fail("par: one thread went on after its exception", (int)visited);
        }
        printf("ok\n");
        return 0;
    }
    if (argc >= 2 && !strcmp(argv[1], "cut")) {     // driver cut: the ranges of kmap_cut_lines tile [lo, n) and begin behind newlines
        std::vector<std::string> texts = {"", "abc", "\n\n\n", std::string((size_t)1 << 20, 'q') + "\nx\n", ""};
        uint64_t x = 88172645463325252ull;
        for (int l = 0; l < 10000; ++l) {
            x = x * 6364136223846793005ull + 1442695040888963407ull;
            texts.back() += std::string((size_t)((x >> 33) % 31), 'a') + "\n";
        }
        for (size_t ti = 0; ti < texts.size(); ++ti) {
            const std::string &t = texts[ti];
            const size_t n = t.size(), nl = t.find('\n');
            for (size_t lo : {(size_t)0, nl == std::string::npos ? n : nl + 1})
                for (size_t min_chunk : {(size_t)1, (size_t)64, (size_t)1 << 40})
                    for (unsigned threads : {1u, 8u}) {
                        const std::vector<size_t> cut = kmap_cut_lines(t.data(), lo, n, threads, min_chunk);
                        if (cut.empty() || cut.front() != lo || cut.back() != n) return fail("cut: the cuts do not run from lo to n", (int)ti);
                        if (cut.size() - 1 > 4 * (size_t)threads) return fail("cut: more than 4 ranges per thread", (int)ti);
                        for (size_t i = 1; i < cut.size(); ++i) {
                            if (cut[i] <= cut[i - 1]) return fail("cut: the cuts are not strictly ascending", (int)ti);
                            if (i + 1 < cut.size() && t[cut[i] - 1] != '\n') return fail("cut: an interior cut is not behind a newline", (int)ti);
                        }
                    }
        }
        printf("ok\n");
        return 0;
    }
    if (argc >= 2 && !strcmp(argv[1], "int")) {     // driver int: kmap_put_int against snprintf("%lld")
        std::vector<int64_t> vals = {0, 9, 10, 999, 1000, 9999, 10000, 99999999, 100000000, -1, -10000, INT64_MAX, INT64_MIN};
        uint64_t x = 0x9E3779B97F4A7C15ull;
        for (int i = 0; i < 100000; ++i) {
            x = x * 6364136223846793005ull + 1442695040888963407ull;
            vals.push_back((int64_t)x >> (int)((x >> 7) % 64));      // every magnitude, both signs
        }
        for (int64_t v : vals) {
            char got[32], want[32];
            char *e = kmap_put_int(got, v);
            const int len = snprintf(want, sizeof want, "%lld", (long long)v);
            if (e - got != len || memcmp(got, want, (size_t)len) != 0) {
                *e = 0;
                fprintf(stderr, "driver: kmap_put_int wrote %s for %s\n", got, want);
                return 2;
            }
        }
        printf("%zu\n", vals.size());
        return 0;
    }
    fprintf(stderr, "usage: driver fasta|csv|pool|f2|par|cut|int ...\n");
    return 64;
}
