// tests/host_san_bed/driver.cpp -- CPU sanitizer harness for kmap_amd/csrc/host_bed.hip (test infrastructure, never shipped).  Built
// twice by the Makefile next to it (-fsanitize=address,undefined and -fsanitize=thread); tests/test_host_sanitizers_bed.py drives it.
//   driver occ <in.csv> <out.bin>    int64 blob: n_rows, n_cols, n_pos[c]..., seq_ind, seq_len, then per column hits and pos
//   driver bed <in.bed> <out.bed>    prints "n_rows n_cols n_chrom int_chrom"; writes every row once as (row, start, start + 5)
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../include/kmap_hip.h"

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

int main(int argc, char **argv) {
    if (argc >= 4 && !strcmp(argv[1], "occ")) {
        kmap_occ *o = nullptr;
        int64_t n = 0;
        int nc = 0;
        int rc = kmap_occ_open(argv[2], &o, &n, &nc);
        if (rc != KMAP_OK) return fail("kmap_occ_open", rc);
        std::vector<int64_t> n_pos((size_t)nc + 1, 0), seq_ind((size_t)n), seq_len((size_t)n);
        kmap_occ_sizes(o, n_pos.data());
        std::vector<std::vector<int32_t>> hits((size_t)nc), pos((size_t)nc);
        std::vector<int32_t *> hp((size_t)nc + 1), pp((size_t)nc + 1);
        for (int c = 0; c < nc; ++c) {
            hits[(size_t)c].resize((size_t)n + 1);
            pos[(size_t)c].resize((size_t)n_pos[(size_t)c] + 1);
            hp[(size_t)c] = hits[(size_t)c].data();
            pp[(size_t)c] = pos[(size_t)c].data();
        }
        rc = kmap_occ_read(o, seq_ind.data(), seq_len.data(), hp.data(), pp.data());
        if (rc != KMAP_OK) return fail("kmap_occ_read", rc);
        kmap_occ_close(o);
        std::vector<int64_t> blob{n, nc};
        for (int c = 0; c < nc; ++c) blob.push_back(n_pos[(size_t)c]);
        blob.insert(blob.end(), seq_ind.begin(), seq_ind.end());
        blob.insert(blob.end(), seq_len.begin(), seq_len.end());
        for (int c = 0; c < nc; ++c) {
            blob.insert(blob.end(), hits[(size_t)c].begin(), hits[(size_t)c].begin() + n);
            blob.insert(blob.end(), pos[(size_t)c].begin(), pos[(size_t)c].begin() + n_pos[(size_t)c]);
        }
        FILE *fh = fopen(argv[3], "wb");
        if (!fh || fwrite(blob.data(), 8, blob.size(), fh) != blob.size() || fclose(fh) != 0) return fail("dump", -1);
        return 0;
    }
    if (argc >= 4 && !strcmp(argv[1], "bed")) {
        kmap_bed *b = nullptr;
        int64_t n = 0;
        int nc = 0, nchr = 0, ic = 0;
        int rc = kmap_bed_open(argv[2], &b, &n, &nc, &nchr, &ic);
        if (rc != KMAP_OK) return fail("kmap_bed_open", rc);
        std::vector<int64_t> start((size_t)n + 1), row((size_t)n + 1), end((size_t)n + 1);
        std::vector<int32_t> rank((size_t)n + 1);
        rc = kmap_bed_rows(b, start.data(), rank.data());
        if (rc != KMAP_OK) return fail("kmap_bed_rows", rc);
        for (int64_t i = 0; i < n; ++i) {
            row[(size_t)i] = i;
            end[(size_t)i] = start[(size_t)i] + 5;
        }
        int64_t bytes = 0;
        rc = kmap_bed_write_locations(b, argv[3], 1, n, row.data(), start.data(), end.data(), &bytes);
        if (rc != KMAP_OK) return fail("kmap_bed_write_locations", rc);
        kmap_bed_close(b);
        printf("%lld %d %d %d\n", (long long)n, nc, nchr, ic);
        return 0;
    }
    fprintf(stderr, "usage: driver occ <in.csv> <out.bin> | bed <in.bed> <out.bed>\n");
    return 1;
}
