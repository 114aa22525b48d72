// host_bed.hip -- native host side of `extract_motif_locations` (no device code): threaded parsers of the occurrence CSV and of the
// BED file, and the threaded writer of the per-consensus BED outputs (the reference, util.py:292-352, walks the rows with pandas
// iterrows and one bed_df.iloc per row).  Both parsers map the file and cut it behind newlines into ranges that host threads parse
// on their own (KMAP_IO_THREADS, like the FASTA reader of host_io.hip; KMAP_TEXT_MIN_CHUNK sets the smallest range, default 1 MiB);
// the ranges' results are concatenated in file order.  Pure host code: tests/host_san_bed compiles it host-only under ASan/UBSan
// and TSan.
#include <errno.h>
#include <fcntl.h>
#include <stdlib.h>
#include <stdio.h>
#include <string.h>
#include <unistd.h>

#include <algorithm>
#include <memory>
#include <new>
#include <string>
#include <string_view>
#include <unordered_map>
#include <vector>

#include "common.h"
#include "host_pool.h"

namespace {
// the whole file, memory-mapped (or read, for what cannot be mapped)
struct Text {
    const char *p = nullptr;
    size_t n = 0;
    KmapMappedFile in;
    std::vector<char> buf;
};
int load_text(const char *path, Text &t, const char *who) {
    if (!t.in.open(path)) {
        kmap_set_error("%s: cannot open %s: %s", who, path, strerror(errno));
        return KMAP_E_IO;
    }
    if (t.in.map()) {
        (void)t.in.file.close();
        t.p = t.in.p;
        t.n = t.in.n;
        return KMAP_OK;
    }
    char chunk[1 << 16];
    for (;;) {
        const ssize_t r = read(t.in.file.fd, chunk, sizeof chunk);
        if (r < 0) {
            kmap_set_error("%s: read error on %s: %s", who, path, strerror(errno));
            return KMAP_E_IO;
        }
        if (r == 0) break;
        t.buf.insert(t.buf.end(), chunk, chunk + r);
    }
    (void)t.in.file.close();
    t.p = t.buf.data();
    t.n = t.buf.size();
    return KMAP_OK;
}

// [lo, n) cut behind newlines into ranges of >= KMAP_TEXT_MIN_CHUNK bytes (default 1 MiB), about 4 per thread
std::vector<size_t> cut_text(const Text &t, size_t lo, unsigned threads) {
    const char *mc = getenv("KMAP_TEXT_MIN_CHUNK");
    return kmap_cut_lines(t.p, lo, t.n, threads, mc ? (size_t)std::max(1ll, atoll(mc)) : ((size_t)1 << 20));
}
// fn(begin, end, byte offset) for every line of [lo, hi) without its '\n' and one trailing '\r'; empty lines are skipped (pandas
// skips them).  fn returns false to stop.
template <typename F>
void for_lines(const char *p, size_t lo, size_t hi, F fn) {
    size_t at = lo;
    while (at < hi) {
        const char *nl = (const char *)memchr(p + at, '\n', hi - at);
        const size_t end = nl ? (size_t)(nl - p) : hi;
        size_t e = end;
        if (e > at && p[e - 1] == '\r') --e;
        if (e > at && !fn(p + at, p + e, at)) return;
        at = end + 1;
    }
}

inline bool is_ws(char c) { return c == ' ' || c == '\t' || c == '\r' || c == '\n' || c == '\v' || c == '\f'; }
inline void strip(const char *&b, const char *&e) {
    while (b < e && is_ws(*b)) ++b;
    while (e > b && is_ws(e[-1])) --e;
}
// Python's int() of a decimal literal: surrounding white space, an optional sign, digits; int64 range
bool parse_int(const char *b, const char *e, int64_t *out) {
    strip(b, e);
    if (b == e) return false;
    bool neg = false;
    if (*b == '+' || *b == '-') neg = *b++ == '-';
    if (b == e) return false;
    uint64_t v = 0;
    for (; b < e; ++b) {
        const unsigned d = (unsigned)(unsigned char)*b - '0';
        if (d > 9 || v > (UINT64_MAX - d) / 10) return false;
        v = v * 10 + d;
    }
    if (v > (neg ? (uint64_t)1 << 63 : ((uint64_t)1 << 63) - 1)) return false;
    *out = neg ? (int64_t)(0ull - v) : (int64_t)v;
    return true;
}
// int(float(x.strip())) of the seq_len cell
bool parse_float_int(const char *b, const char *e, int64_t *out) {
    strip(b, e);
    if (b == e || e - b > 63) return false;
    char tmp[64];
    memcpy(tmp, b, (size_t)(e - b));
    tmp[e - b] = 0;
    char *end = nullptr;
    const double d = strtod(tmp, &end);
    if (end != tmp + (e - b) || !(d > -9.2e18 && d < 9.2e18)) return false;
    *out = (int64_t)d;
    return true;
}
}  // namespace

// ---- occurrence CSV: `seq_ind;loc,loc;...;seq_len` (Occurrence.from_file's reading of gen_motif_occurence_file's format) -------
struct kmap_occ {
    int n_cols = 0;
    struct Part {
        std::vector<int64_t> seq_ind, seq_len;
        std::vector<std::vector<int32_t>> hits, pos;
        std::string err;
    };
    std::vector<Part> parts;
    int64_t n_rows = 0;
    std::vector<int64_t> n_pos;
    unsigned threads = 1;
};

static int occ_open_impl(const char *path, kmap_occ **out, int64_t *n_rows, int *n_cols) {
    KMAP_REQUIRE(path && out && n_rows && n_cols, "occ_open: null argument");
    Text t;
    KMAP_TRY(load_text(path, t, "occ_open"));
    const char *nl = (const char *)memchr(t.p, '\n', t.n);
    size_t hdr_end = nl ? (size_t)(nl - t.p) : t.n;
    KMAP_REQUIRE(t.n > 0 && hdr_end > 0, "occurrence file %s: no header line", path);
    std::unique_ptr<kmap_occ> o(new kmap_occ());
    o->threads = kmap_io_threads();
    const int fields = 1 + (int)std::count(t.p, t.p + hdr_end, ';');
    KMAP_REQUIRE(fields >= 2, "occurrence file %s: the header has %d field(s), `seq_ind;...;seq_len` has at least 2", path, fields);
    const int nc = fields - 2;
    o->n_cols = nc;
    const size_t body = nl ? hdr_end + 1 : t.n;
    const std::vector<size_t> cut = cut_text(t, body, o->threads);
    o->parts.resize(cut.size() - 1);
    kmap_parallel_for(o->parts.size(), o->threads, [&](size_t i) {
        kmap_occ::Part &pt = o->parts[i];
        pt.hits.resize((size_t)nc);
        pt.pos.resize((size_t)nc);
        try {
            for_lines(t.p, cut[i], cut[i + 1], [&](const char *b, const char *e, size_t at) {
                const char *f = b;
                auto field_end = [&](const char *from) { const char *s = (const char *)memchr(from, ';', (size_t)(e - from)); return s ? s : e; };
                auto bad = [&](const char *what) {
                    pt.err = "occurrence file: " + std::string(what) + " in the line at byte " + std::to_string(at);
                    return false;
                };
                const char *fe = field_end(f);
                int64_t v = 0;
                if (!parse_int(f, fe, &v)) return bad("seq_ind is not an integer");
                pt.seq_ind.push_back(v);
                for (int c = 0; c < nc; ++c) {
                    if (fe == e) return bad("too few fields");
                    f = fe + 1;
                    fe = field_end(f);
                    const char *cb = f, *ce = fe;
                    strip(cb, ce);
                    std::vector<int32_t> &pos = pt.pos[(size_t)c];
                    const size_t first = pos.size();
                    while (cb < ce) {
                        const char *comma = (const char *)memchr(cb, ',', (size_t)(ce - cb));
                        const char *te = comma ? comma : ce;
                        if (!parse_int(cb, te, &v) || v < INT32_MIN || v > INT32_MAX) return bad("a location is not a 32-bit integer");
                        pos.push_back((int32_t)v);
                        if (!comma) break;
                        cb = comma + 1;
                        if (cb == ce) return bad("a location is not a 32-bit integer");   // trailing comma: int('') raises
                    }
                    std::sort(pos.begin() + (ptrdiff_t)first, pos.end());
                    pt.hits[(size_t)c].push_back((int32_t)(pos.size() - first));
                }
                if (fe == e) return bad("too few fields");
                f = fe + 1;
                if (memchr(f, ';', (size_t)(e - f))) return bad("too many fields");
                if (!parse_float_int(f, e, &v)) return bad("seq_len is not a number");
                pt.seq_len.push_back(v);
                return true;
            });
        } catch (const std::bad_alloc &) {
            pt.err = "occurrence file: out of memory";
        }
    });
    o->n_pos.assign((size_t)nc, 0);
    for (const kmap_occ::Part &pt : o->parts) {
        if (!pt.err.empty()) {
            kmap_set_error("%s (%s)", pt.err.c_str(), path);
            return pt.err.find("out of memory") != std::string::npos ? KMAP_E_NOMEM : KMAP_E_INVAL;
        }
        o->n_rows += (int64_t)pt.seq_ind.size();
        for (int c = 0; c < nc; ++c) o->n_pos[(size_t)c] += (int64_t)pt.pos[(size_t)c].size();
    }
    *n_rows = o->n_rows;
    *n_cols = nc;
    *out = o.release();
    return KMAP_OK;
}

extern "C" int kmap_occ_open(const char *path, kmap_occ **out, int64_t *n_rows, int *n_cols) {
    try {
        return occ_open_impl(path, out, n_rows, n_cols);
    } catch (const std::bad_alloc &) {
        kmap_set_error("occ_open: out of memory");
        return KMAP_E_NOMEM;
    }
}

extern "C" int kmap_occ_sizes(const kmap_occ *o, int64_t *n_pos) {
    KMAP_REQUIRE(o && (o->n_cols == 0 || n_pos), "occ_sizes: null argument");
    for (int c = 0; c < o->n_cols; ++c) n_pos[c] = o->n_pos[(size_t)c];
    return KMAP_OK;
}

extern "C" int kmap_occ_read(const kmap_occ *o, int64_t *seq_ind, int64_t *seq_len, int32_t *const *hits, int32_t *const *pos) {
    KMAP_REQUIRE(o, "occ_read: null handle");
    KMAP_REQUIRE(o->n_rows == 0 || (seq_ind && seq_len), "occ_read: null output");
    KMAP_REQUIRE(o->n_cols == 0 || (hits && pos), "occ_read: null output");
    for (int c = 0; c < o->n_cols; ++c) KMAP_REQUIRE((o->n_rows == 0 || hits[c]) && (o->n_pos[(size_t)c] == 0 || pos[c]), "occ_read: null output");
    const size_t np = o->parts.size(), nc = (size_t)o->n_cols;
    std::vector<int64_t> row0(np + 1, 0), pos0((np + 1) * nc, 0);
    for (size_t i = 0; i < np; ++i) {
        row0[i + 1] = row0[i] + (int64_t)o->parts[i].seq_ind.size();
        for (size_t c = 0; c < nc; ++c) pos0[(i + 1) * nc + c] = pos0[i * nc + c] + (int64_t)o->parts[i].pos[c].size();
    }
    kmap_parallel_for(np, o->threads, [&](size_t i) {
        const kmap_occ::Part &pt = o->parts[i];
        const size_t n = pt.seq_ind.size();
        if (n) {
            memcpy(seq_ind + row0[i], pt.seq_ind.data(), n * 8);
            memcpy(seq_len + row0[i], pt.seq_len.data(), n * 8);
        }
        for (size_t c = 0; c < nc; ++c) {
            if (n) memcpy(hits[c] + row0[i], pt.hits[c].data(), n * 4);
            if (!pt.pos[c].empty()) memcpy(pos[c] + pos0[i * nc + c], pt.pos[c].data(), pt.pos[c].size() * 4);
        }
    });
    return KMAP_OK;
}

extern "C" int kmap_occ_close(kmap_occ *o) {
    delete o;
    return KMAP_OK;
}

// ---- BED: tab-separated, no header, 3 or 6 columns (chrom, start, end[, name, score, strand]) -----------------------------------
struct kmap_bed {
    int n_cols = 0;
    int int_chrom = 0;                      // every chrom is an integer literal: pandas reads the column as int64
    std::vector<int64_t> start;
    std::vector<int32_t> chrom_rank;        // rank of the row's chrom in the sort order of the output
    std::vector<uint32_t> strand;           // index into strands
    std::vector<std::string> chroms;        // by rank, as written to the output
    std::vector<std::string> strands;
    size_t max_chrom = 0, max_strand = 0;
    unsigned threads = 1;
};

namespace {
bool int_literal(const std::string &s, int64_t *v) {   // what pandas parses as an integer: optional sign, digits
    if (s.empty() || is_ws(s.front()) || is_ws(s.back())) return false;
    return parse_int(s.data(), s.data() + s.size(), v);
}
}  // namespace

static int bed_open_impl(const char *path, kmap_bed **out, int64_t *n_rows, int *n_cols, int *n_chrom, int *int_chrom) {
    KMAP_REQUIRE(path && out && n_rows && n_cols && n_chrom && int_chrom, "bed_open: null argument");
    Text t;
    KMAP_TRY(load_text(path, t, "bed_open"));
    std::unique_ptr<kmap_bed> bed(new kmap_bed());
    bed->threads = kmap_io_threads();
    int nf = 0;                                                   // fields of the first line decide the width
    for_lines(t.p, 0, t.n, [&](const char *b, const char *e, size_t) {
        nf = 1 + (int)std::count(b, e, '\t');
        return false;
    });
    KMAP_REQUIRE(nf == 0 || nf == 3 || nf == 6, "Input BED file should have either 3 or 6 columns (%s has %d)", path, nf);
    bed->n_cols = nf;
    struct Part {
        std::vector<int64_t> start;
        std::vector<uint32_t> chrom, strand;
        std::unordered_map<std::string_view, uint32_t> chrom_ids, strand_ids;
        std::vector<std::string_view> chrom_names, strand_names;
        std::string err;
    };
    const std::vector<size_t> cut = cut_text(t, 0, bed->threads);
    std::vector<Part> parts(cut.size() - 1);
    kmap_parallel_for(parts.size(), bed->threads, [&](size_t i) {
        Part &pt = parts[i];
        auto intern = [](std::unordered_map<std::string_view, uint32_t> &ids, std::vector<std::string_view> &names, std::string_view s) {
            auto it = ids.find(s);
            if (it != ids.end()) return it->second;
            const uint32_t id = (uint32_t)names.size();
            ids.emplace(s, id);
            names.push_back(s);
            return id;
        };
        try {
            for_lines(t.p, cut[i], cut[i + 1], [&](const char *b, const char *e, size_t at) {
                auto bad = [&](const char *what) {
                    pt.err = "BED file: " + std::string(what) + " in the line at byte " + std::to_string(at);
                    return false;
                };
                if (memchr(b, '"', (size_t)(e - b))) return bad("a quoted field (not supported)");
                const char *f[7];
                int k = 0;
                f[k++] = b;
                for (const char *q = b; q < e && k <= 6; ++q)
                    if (*q == '\t') f[k++] = q + 1;
                if (k != nf) return bad(nf == 3 ? "not 3 columns" : "not 6 columns");
                f[k] = e + 1;
                int64_t s = 0;
                if (!parse_int(f[1], f[2] - 1, &s)) return bad("start is not an integer");
                pt.start.push_back(s);
                pt.chrom.push_back(intern(pt.chrom_ids, pt.chrom_names, std::string_view(f[0], (size_t)(f[1] - 1 - f[0]))));
                if (nf == 6) pt.strand.push_back(intern(pt.strand_ids, pt.strand_names, std::string_view(f[5], (size_t)(e - f[5]))));
                return true;
            });
        } catch (const std::bad_alloc &) {
            pt.err = "BED file: out of memory";
        }
    });
    for (const Part &pt : parts)
        if (!pt.err.empty()) {
            kmap_set_error("%s (%s)", pt.err.c_str(), path);
            return pt.err.find("out of memory") != std::string::npos ? KMAP_E_NOMEM : KMAP_E_INVAL;
        }
    // global interning: id per distinct text, then the rank of the value pandas would hold
    std::unordered_map<std::string, uint32_t> cid, sid;
    std::vector<std::string> cnames;
    std::vector<std::vector<uint32_t>> cmap(parts.size()), smap(parts.size());
    if (nf != 6) bed->strands.push_back(".");                   // 3 columns: the reference raises KeyError('strand'); here "."
    for (size_t i = 0; i < parts.size(); ++i) {
        for (std::string_view v : parts[i].chrom_names) {
            auto it = cid.emplace(std::string(v), (uint32_t)cnames.size());
            if (it.second) cnames.emplace_back(v);
            cmap[i].push_back(it.first->second);
        }
        for (std::string_view v : parts[i].strand_names) {
            auto it = sid.emplace(std::string(v), (uint32_t)bed->strands.size());
            if (it.second) bed->strands.emplace_back(v);
            smap[i].push_back(it.first->second);
        }
    }
    std::vector<int64_t> ival(cnames.size());
    bool all_int = !cnames.empty();
    for (size_t j = 0; j < cnames.size() && all_int; ++j) all_int = int_literal(cnames[j], &ival[j]);
    std::vector<uint32_t> order(cnames.size());
    for (size_t j = 0; j < order.size(); ++j) order[j] = (uint32_t)j;
    std::vector<int32_t> rank(cnames.size());
    if (all_int) {
        std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return ival[a] < ival[b]; });
        for (size_t j = 0; j < order.size(); ++j) {
            if (j == 0 || ival[order[j]] != ival[order[j - 1]]) bed->chroms.push_back(std::to_string(ival[order[j]]));
            rank[order[j]] = (int32_t)bed->chroms.size() - 1;   // "1" and "01" are the same integer
        }
    } else {
        std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return cnames[a] < cnames[b]; });   // bytes of UTF-8 = code points
        for (size_t j = 0; j < order.size(); ++j) {
            bed->chroms.push_back(cnames[order[j]]);
            rank[order[j]] = (int32_t)j;
        }
    }
    bed->int_chrom = all_int ? 1 : 0;
    for (const std::string &s : bed->chroms) bed->max_chrom = std::max(bed->max_chrom, s.size());
    for (const std::string &s : bed->strands) bed->max_strand = std::max(bed->max_strand, s.size());
    std::vector<size_t> row0(parts.size() + 1, 0);
    for (size_t i = 0; i < parts.size(); ++i) row0[i + 1] = row0[i] + parts[i].start.size();
    const size_t n = row0.back();
    bed->start.resize(n);
    bed->chrom_rank.resize(n);
    bed->strand.resize(n);
    kmap_parallel_for(parts.size(), bed->threads, [&](size_t i) {
        const Part &pt = parts[i];
        const size_t m = pt.start.size();
        if (m) memcpy(bed->start.data() + row0[i], pt.start.data(), m * 8);
        for (size_t r = 0; r < m; ++r) {
            bed->chrom_rank[row0[i] + r] = rank[cmap[i][pt.chrom[r]]];
            bed->strand[row0[i] + r] = nf == 6 ? smap[i][pt.strand[r]] : 0u;
        }
    });
    *n_rows = (int64_t)n;
    *n_cols = nf;
    *n_chrom = (int)bed->chroms.size();
    *int_chrom = bed->int_chrom;
    *out = bed.release();
    return KMAP_OK;
}

extern "C" int kmap_bed_open(const char *path, kmap_bed **out, int64_t *n_rows, int *n_cols, int *n_chrom, int *int_chrom) {
    try {
        return bed_open_impl(path, out, n_rows, n_cols, n_chrom, int_chrom);
    } catch (const std::bad_alloc &) {
        kmap_set_error("bed_open: out of memory");
        return KMAP_E_NOMEM;
    }
}

extern "C" int kmap_bed_rows(const kmap_bed *b, int64_t *start, int32_t *chrom_rank) {
    KMAP_REQUIRE(b, "bed_rows: null handle");
    const size_t n = b->start.size();
    KMAP_REQUIRE(n == 0 || (start && chrom_rank), "bed_rows: null output");
    if (n) {
        memcpy(start, b->start.data(), n * 8);
        memcpy(chrom_rank, b->chrom_rank.data(), n * 4);
    }
    return KMAP_OK;
}

extern "C" int kmap_bed_chrom(const kmap_bed *b, int rank, char *buf, int cap) {
    KMAP_REQUIRE(b && buf && cap > 0, "bed_chrom: bad arguments");
    KMAP_REQUIRE(rank >= 0 && (size_t)rank < b->chroms.size(), "bed_chrom: rank %d out of range", rank);
    const std::string &s = b->chroms[(size_t)rank];
    KMAP_REQUIRE(s.size() < (size_t)cap, "bed_chrom: buffer of %d bytes too small", cap);
    memcpy(buf, s.data(), s.size());
    buf[s.size()] = 0;
    return (int)s.size();
}

// ---- the per-consensus output: "chrom\tstart\tend\tname\tscore\tstrand" like pandas to_csv(sep='\t', index=False) --------------
static int bed_write_impl(const kmap_bed *b, const char *path, int cons_index, int64_t n, const int64_t *row, const int64_t *start,
                          const int64_t *end, int64_t *bytes_written) {
    KMAP_REQUIRE(b && path && n >= 0 && cons_index >= 0, "bed_write_locations: bad arguments");
    KMAP_REQUIRE(n == 0 || (row && start && end), "bed_write_locations: null arrays");
    const int64_t n_bed = (int64_t)b->start.size();
    for (int64_t i = 0; i < n; ++i) KMAP_REQUIRE(row[i] >= 0 && row[i] < n_bed, "bed_write_locations: row %lld out of range", (long long)row[i]);
    const std::string header = "chrom\tstart\tend\tname\tscore\tstrand\n";
    const std::string name0 = "\tmotif_" + std::to_string(cons_index) + "_";
    const size_t per_row = b->max_chrom + b->max_strand + name0.size() + 3 * 21 + 8;
    const int64_t rows_per_chunk = 1 << 16;
    const int64_t n_chunks = (n + rows_per_chunk - 1) / rows_per_chunk;
    std::vector<KmapChunk> bufs((size_t)n_chunks);
    kmap_parallel_for((size_t)n_chunks, b->threads, [&](size_t ch) {
        const int64_t lo = (int64_t)ch * rows_per_chunk, hi = std::min(n, lo + rows_per_chunk);
        char *const p0 = new char[(size_t)(hi - lo) * per_row];   // a bad_alloc here is the ABI handler's
        bufs[ch].mem.reset(p0);
        char *p = p0;
        for (int64_t i = lo; i < hi; ++i) {
            const int64_t r = row[i];
            const std::string &c = b->chroms[(size_t)b->chrom_rank[(size_t)r]];
            memcpy(p, c.data(), c.size());
            p += c.size();
            *p++ = '\t';
            p = kmap_put_int(p, start[i]);
            *p++ = '\t';
            p = kmap_put_int(p, end[i]);
            memcpy(p, name0.data(), name0.size());
            p += name0.size();
            p = kmap_put_int(p, r);
            memcpy(p, "\t0\t", 3);
            p += 3;
            const std::string &s = b->strands[b->strand[(size_t)r]];
            memcpy(p, s.data(), s.size());
            p += s.size();
            *p++ = '\n';
        }
        bufs[ch].len = (size_t)(p - p0);
    });
    KmapFd out(open(path, O_WRONLY | O_CREAT | O_TRUNC | O_CLOEXEC, 0666));
    if (out.fd < 0) {
        kmap_set_error("bed_write_locations: cannot open %s: %s", path, strerror(errno));
        return KMAP_E_IO;
    }
    const int64_t end_off = kmap_pwrite_all(out.fd, header.data(), header.size(), 0) ? kmap_write_chunks(out.fd, (int64_t)header.size(), bufs, b->threads) : -1;
    if (out.close() != 0 || end_off < 0) {
        kmap_set_error("bed_write_locations: write to %s failed: %s", path, strerror(errno));
        return KMAP_E_IO;
    }
    if (bytes_written) *bytes_written = end_off;
    return KMAP_OK;
}

extern "C" int kmap_bed_write_locations(const kmap_bed *b, const char *path, int cons_index, int64_t n, const int64_t *row,
                                        const int64_t *start, const int64_t *end, int64_t *bytes_written) {
    try {
        return bed_write_impl(b, path, cons_index, n, row, start, end, bytes_written);
    } catch (const std::bad_alloc &) {
        kmap_set_error("bed_write_locations: out of memory");
        return KMAP_E_NOMEM;
    }
}

extern "C" int kmap_bed_close(kmap_bed *b) {
    delete b;
    return KMAP_OK;
}
