// parquet_writer.cpp — see parquet_writer.h. Thrift compact PROTOCOL writer
// (field ids per parquet-format/src/main/thrift/parquet.thrift; the inverse
// of thrift_compact.h's reader).
#include "parquet_writer.h"
#include "def_levels.h"
#include "snappy_compress.h"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

namespace hx {
namespace {

struct TW {  // thrift compact writer
    std::vector<uint8_t> buf;
    void byte(uint8_t b) { buf.push_back(b); }
    void varint(uint64_t v) {
        while (v >= 0x80) {
            byte(uint8_t(v) | 0x80);
            v >>= 7;
        }
        byte(uint8_t(v));
    }
    void zigzag(int64_t v) { varint((uint64_t(v) << 1) ^ uint64_t(v >> 63)); }
    // field header inside a struct (delta-encoded ids; caller tracks last)
    void field(int16_t& last, int16_t id, uint8_t type) {
        int16_t delta = id - last;
        if (delta > 0 && delta <= 15) {
            byte(uint8_t(delta << 4) | type);
        } else {
            byte(type);
            zigzag(id);
        }
        last = id;
    }
    void stop() { byte(0); }
    void i32(int16_t& last, int16_t id, int64_t v) {
        field(last, id, 5);
        zigzag(v);
    }
    void i64f(int16_t& last, int16_t id, int64_t v) {
        field(last, id, 6);
        zigzag(v);
    }
    void binary(int16_t& last, int16_t id, const void* p, size_t n) {
        field(last, id, 8);
        varint(n);
        const uint8_t* b = (const uint8_t*)p;
        buf.insert(buf.end(), b, b + n);
    }
    void str(int16_t& last, int16_t id, const std::string& s) {
        binary(last, id, s.data(), s.size());
    }
    void list_header(int16_t& last, int16_t id, uint8_t elem_type, size_t n) {
        field(last, id, 9);
        if (n < 15) {
            byte(uint8_t(n << 4) | elem_type);
        } else {
            byte(0xF0 | elem_type);
            varint(n);
        }
    }
};

struct ColSpec {
    const char* name;
    int32_t physical;    // 2 = INT64, 5 = DOUBLE
    int32_t converted;   // -1 none; 14 = UINT_64
};

const ColSpec kCols[5] = {
    {"series_id", 2, 14}, {"timestamp", 2, -1}, {"value", 5, -1},
    {"__seq__", 2, 14},   {"__reserved__", 2, 14},
};  // 14 = ConvertedType::UINT_64

void schema_element(TW& w, const ColSpec& c, bool optional) {
    int16_t last = 0;
    w.i32(last, 1, c.physical);            // type
    w.i32(last, 3, optional ? 1 : 0);      // repetition REQUIRED / OPTIONAL
    w.str(last, 4, c.name);                // name
    if (c.converted >= 0) w.i32(last, 6, c.converted);
    w.stop();
}

void statistics(TW& w, const std::string& mn, const std::string& mx) {
    int16_t last = 0;
    w.binary(last, 5, mx.data(), mx.size());  // max_value
    w.binary(last, 6, mn.data(), mn.size());  // min_value
    w.stop();
}

struct ChunkMeta {
    int64_t data_page_offset;
    int64_t total_size;             // page header + uncompressed payload
    int64_t total_compressed = 0;   // page header + payload as written
    int32_t codec = 0;              // 0 UNCOMPRESSED, 1 SNAPPY
    int64_t num_values;
    std::string mn, mx;
    bool has_stats = true;
    // OPTIONAL chunk: RLE joins the encodings and the statistics always carry
    // null_count, with bounds only when has_stats
    bool optional = false;
    int64_t null_count = 0;
};

void statistics_optional(TW& w, const ChunkMeta& m) {
    int16_t last = 0;
    w.i64f(last, 3, m.null_count);
    if (m.has_stats) {
        w.binary(last, 5, m.mx.data(), m.mx.size());
        w.binary(last, 6, m.mn.data(), m.mn.size());
    }
    w.stop();
}

void column_chunk(TW& w, const char* name, int32_t physical,
                  const ChunkMeta& m) {
    int16_t last = 0;
    w.i64f(last, 2, m.data_page_offset);  // file_offset (deprecated, required)
    // meta_data struct (field 3)
    w.field(last, 3, 12);
    {
        int16_t l2 = 0;
        w.i32(l2, 1, physical);                        // type
        if (m.optional) {
            w.list_header(l2, 2, 5, 2);                // encodings: [PLAIN, RLE]
            w.zigzag(0);
            w.zigzag(3);
        } else {
            w.list_header(l2, 2, 5, 1);                // encodings: [PLAIN]
            w.zigzag(0);
        }
        w.list_header(l2, 3, 8, 1);                    // path_in_schema
        w.varint(strlen(name));
        w.buf.insert(w.buf.end(), (const uint8_t*)name,
                     (const uint8_t*)name + strlen(name));
        w.i32(l2, 4, m.codec);                         // UNCOMPRESSED / SNAPPY
        w.i64f(l2, 5, m.num_values);
        w.i64f(l2, 6, m.total_size);                   // uncompressed
        w.i64f(l2, 7, m.total_compressed);             // compressed
        w.i64f(l2, 9, m.data_page_offset);
        if (m.optional) {
            w.field(l2, 12, 12);                       // statistics
            statistics_optional(w, m);
        } else if (m.has_stats) {
            w.field(l2, 12, 12);                       // statistics
            statistics(w, m.mn, m.mx);
        }
        w.stop();
    }
    w.stop();
}

std::vector<uint8_t> page_header(int32_t n_values, int32_t payload,
                                 int32_t compressed) {
    TW w;
    int16_t last = 0;
    w.i32(last, 1, 0);           // type DATA_PAGE
    w.i32(last, 2, payload);     // uncompressed_page_size
    w.i32(last, 3, compressed);  // compressed_page_size
    w.field(last, 5, 12);     // data_page_header
    {
        int16_t l2 = 0;
        w.i32(l2, 1, n_values);
        w.i32(l2, 2, 0);  // encoding PLAIN
        w.i32(l2, 3, 3);  // definition_level_encoding RLE
        w.i32(l2, 4, 3);  // repetition_level_encoding RLE
        w.stop();
    }
    w.stop();
    return std::move(w.buf);
}

// Returns whether the chunk gets statistics at all.
template <typename T>
bool minmax_bytes(const T* v, int64_t n, std::string& mn, std::string& mx) {
    T lo = v[0], hi = v[0];
    for (int64_t i = 1; i < n; i++) {
        if (v[i] < lo) lo = v[i];
        if (v[i] > hi) hi = v[i];
    }
    mn.assign((const char*)&lo, 8);
    mx.assign((const char*)&hi, 8);
    return true;
}

// DOUBLE statistics follow parquet.thrift's ColumnOrder rules for floating
// point: NaN never enters min/max (a chunk of nothing but NaN carries no
// statistics), and a zero bound is written min = -0.0 / max = +0.0 so a
// reader that distinguishes the signs cannot prune the other zero away.
bool minmax_bytes(const double* v, int64_t n, std::string& mn,
                  std::string& mx) {
    bool any = false;
    double lo = 0.0, hi = 0.0;
    for (int64_t i = 0; i < n; i++) {
        const double x = v[i];
        if (x != x) continue;
        if (!any) {
            lo = hi = x;
            any = true;
        } else {
            if (x < lo) lo = x;
            if (x > hi) hi = x;
        }
    }
    if (!any) return false;
    if (lo == 0.0) lo = -0.0;
    if (hi == 0.0) hi = 0.0;
    mn.assign((const char*)&lo, 8);
    mx.assign((const char*)&hi, 8);
    return true;
}

// Writes one data page: header, then the payload as the codec leaves it. The
// uncompressed payload is head (a level block, may be empty) followed by
// body. Under Snappy the payload is `ready` when the caller brought one, else
// the host twin's stream of {head, body}; both are the same bytes. A page
// equal to the column's previous page reuses that page's stream (full pages
// of a constant __seq__, __reserved__ zeros).
struct PageWriter {
    int32_t codec;
    const PagePayload* ready;   // [row group * n_cols + column], or null
    int32_t n_cols;
    struct Prev {
        std::vector<uint8_t> raw, comp;
        bool valid = false;
    };
    std::vector<Prev> prev;
    std::vector<uint8_t> joined;
    PageWriter(int32_t codec_, const PagePayload* ready_, int32_t n_cols_)
        : codec(codec_), ready(ready_), n_cols(n_cols_), prev(n_cols_) {}

    // false on a failed write; m gets sizes, codec and data_page_offset.
    // snappy: this page is written as a Snappy stream. With a ready stream
    // body may be null (body_len still the uncompressed size).
    bool write(FILE* f, int64_t g, int32_t c, bool snappy,
               int32_t n_values, const uint8_t* head, size_t head_len,
               const uint8_t* body, size_t body_len, int64_t& off,
               ChunkMeta& m) {
        const size_t payload = head_len + body_len;
        const uint8_t* out = nullptr;
        size_t out_len = payload;
        if (snappy) {
            const PagePayload* r = ready ? &ready[g * n_cols + c] : nullptr;
            if (r && r->ptr) {
                out = r->ptr;
                out_len = r->len;
            } else {
                const uint8_t* raw = body;
                if (head_len) {
                    joined.assign(head, head + head_len);
                    joined.insert(joined.end(), body, body + body_len);
                    raw = joined.data();
                }
                Prev& pv = prev[c];
                if (!pv.valid || pv.raw.size() != payload ||
                    (payload && std::memcmp(pv.raw.data(), raw, payload))) {
                    pv.raw.assign(raw, raw + payload);
                    pv.comp.resize(size_t(snappy_max_compressed(payload)));
                    pv.comp.resize(snappy_compress_host(
                        raw, payload, pv.comp.data(), pv.comp.size()));
                    pv.valid = true;
                }
                out = pv.comp.data();
                out_len = pv.comp.size();
            }
        }
        auto hdr = page_header(n_values, int32_t(payload), int32_t(out_len));
        m.data_page_offset = off;
        m.codec = snappy ? 1 : 0;
        m.total_size = int64_t(hdr.size() + payload);
        m.total_compressed = int64_t(hdr.size() + out_len);
        if (fwrite(hdr.data(), 1, hdr.size(), f) != hdr.size()) return false;
        if (snappy) {
            if (out_len && fwrite(out, 1, out_len, f) != out_len) return false;
        } else {
            if (head_len && fwrite(head, 1, head_len, f) != head_len)
                return false;
            if (body_len && fwrite(body, 1, body_len, f) != body_len)
                return false;
        }
        off += m.total_compressed;
        return true;
    }
};

// A BYTE_ARRAY chunk of several v1 PLAIN data pages back to back (DESIGN
// §10): page i holds rows[i] values and ulen[i] uncompressed bytes, the
// consecutive slices of `image` (may be null when every stream is given).
// streams (snappy only, may be null): the pages' Snappy streams back to back,
// slen[i] bytes each; otherwise each slice is compressed here. m gets the
// first page's offset and the sums over all headers and payloads.
bool write_ba_pages(FILE* f, bool snappy, uint32_t k, const uint32_t* rows,
                    const uint32_t* ulen, const uint8_t* image,
                    const uint8_t* streams, const uint32_t* slen,
                    int64_t& off, ChunkMeta& m) {
    m.data_page_offset = off;
    m.codec = snappy ? 1 : 0;
    m.total_size = 0;
    m.total_compressed = 0;
    std::vector<uint8_t> comp;
    size_t at = 0, s_at = 0;
    for (uint32_t i = 0; i < k; i++) {
        const uint8_t* out = image ? image + at : nullptr;
        size_t out_len = ulen[i];
        if (snappy && streams) {
            out = streams + s_at;
            out_len = slen[i];
            s_at += slen[i];
        } else if (snappy) {
            comp.resize(size_t(snappy_max_compressed(ulen[i])));
            comp.resize(snappy_compress_host(image + at, ulen[i], comp.data(),
                                             comp.size()));
            out = comp.data();
            out_len = comp.size();
        }
        auto hdr = page_header(int32_t(rows[i]), int32_t(ulen[i]),
                               int32_t(out_len));
        if (fwrite(hdr.data(), 1, hdr.size(), f) != hdr.size()) return false;
        if (out_len && fwrite(out, 1, out_len, f) != out_len) return false;
        m.total_size += int64_t(hdr.size() + ulen[i]);
        m.total_compressed += int64_t(hdr.size() + out_len);
        at += ulen[i];
    }
    off += m.total_compressed;
    return true;
}

// the cuts a ready entry brought: they must add up to rows and bytes
bool split_ok(const PagePayload& r, int64_t rows, uint64_t bytes) {
    if (!r.split_rows || !r.split_ulen) return false;
    uint64_t sr = 0, sb = 0;
    for (uint32_t i = 0; i < r.n_split; i++) {
        if (r.split_rows[i] == 0 || r.split_ulen[i] > 0x7FFFFFFFu)
            return false;
        sr += r.split_rows[i];
        sb += r.split_ulen[i];
    }
    return sr == uint64_t(rows) && sb == bytes;
}

// Statistics a ready page brought along; false = compute from the column.
bool stats_from_ready(const PagePayload* ready, int64_t idx, ChunkMeta& m) {
    if (!ready || !ready[idx].ptr || ready[idx].stats == 0) return false;
    m.has_stats = ready[idx].stats == 1;
    m.mn.assign((const char*)&ready[idx].min_bits, 8);
    m.mx.assign((const char*)&ready[idx].max_bits, 8);
    return true;
}

// A column given as a null pointer needs every page ready with statistics.
bool column_present(const void* data, const PagePayload* ready, int64_t idx,
                    int32_t codec) {
    return data || (codec == 1 && ready && ready[idx].ptr &&
                    ready[idx].stats != 0);
}

struct MetricRG {
    int64_t num_rows;
    ChunkMeta cols[5];
};

// FileMetaData of the 5-column metric layout, footer length and magic.
bool metric_footer(FILE* f, const std::vector<MetricRG>& rgs, int64_t n,
                   bool value_optional) {
    TW w;
    int16_t last = 0;
    w.i32(last, 1, 1);  // version
    w.list_header(last, 2, 12, 6);  // schema: root + 5 leaves
    {
        int16_t l2 = 0;   // root group
        w.str(l2, 4, "schema");
        w.i32(l2, 5, 5);  // num_children
        w.stop();
    }
    for (int c = 0; c < 5; c++)
        schema_element(w, kCols[c], value_optional && c == 2);
    w.i64f(last, 3, n);  // num_rows
    w.list_header(last, 4, 12, rgs.size());
    for (const auto& rg : rgs) {
        int16_t l2 = 0;
        w.list_header(l2, 1, 12, 5);
        int64_t total = 0;
        for (int c = 0; c < 5; c++) total += rg.cols[c].total_size;
        for (int c = 0; c < 5; c++)
            column_chunk(w, kCols[c].name, kCols[c].physical, rg.cols[c]);
        w.i64f(l2, 2, total);        // total_byte_size
        w.i64f(l2, 3, rg.num_rows);  // num_rows
        w.stop();
    }
    w.str(last, 6, "horaedb-amd hx_compact writer");
    // column_orders: TYPE_ORDER for every leaf — required for readers to
    // trust min_value/max_value (parquet.thrift ColumnOrder union)
    w.list_header(last, 7, 12, 5);
    for (int c = 0; c < 5; c++) {
        int16_t l2 = 0;
        w.field(l2, 1, 12);  // TypeDefinedOrder (empty struct)
        w.stop();
        w.stop();
    }
    w.stop();

    uint32_t flen = (uint32_t)w.buf.size();
    return fwrite(w.buf.data(), 1, flen, f) == flen &&
           fwrite(&flen, 4, 1, f) == 1 && fwrite("PAR1", 1, 4, f) == 4;
}

}  // namespace

std::string write_metric_sst(const std::string& path, const uint64_t* series,
                             const int64_t* ts, const double* value,
                             uint64_t seq, int64_t n, int64_t row_group,
                             int32_t codec, const PagePayload* ready) {
    if (n <= 0) return "write_metric_sst: no rows";
    if (codec != 0 && codec != 1) return "write_metric_sst: unknown codec";
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) return "write_metric_sst: cannot open " + path;
    auto fail = [&](const char* m) {
        fclose(f);
        remove(path.c_str());
        return std::string(m);
    };
    if (fwrite("PAR1", 1, 4, f) != 4) return fail("write failed");
    int64_t off = 4;

    std::vector<uint64_t> seq_col;   // constant per file (closure precondition)
    std::vector<uint64_t> zeros;
    std::vector<MetricRG> rgs;
    PageWriter pw(codec, ready, 5);
    for (int64_t g = 0, base = 0; base < n; g++, base += row_group) {
        int64_t rows = std::min<int64_t>(row_group, n - base);
        if ((int64_t)seq_col.size() < rows) {
            seq_col.assign(rows, seq);
            zeros.assign(rows, 0);
        }
        const void* data[5] = {series ? series + base : nullptr,
                               ts ? ts + base : nullptr,
                               value ? value + base : nullptr,
                               seq_col.data(), zeros.data()};
        MetricRG rg;
        rg.num_rows = rows;
        for (int c = 0; c < 5; c++) {
            ChunkMeta& m = rg.cols[c];
            m.num_values = rows;
            if (!column_present(data[c], ready, g * 5 + c, codec))
                return fail("write_metric_sst: column neither given nor ready");
            if (!stats_from_ready(ready, g * 5 + c, m)) switch (c) {
                case 0: case 3: case 4:
                    minmax_bytes((const uint64_t*)data[c], rows, m.mn, m.mx);
                    break;
                case 1:
                    minmax_bytes((const int64_t*)data[c], rows, m.mn, m.mx);
                    break;
                case 2:
                    m.has_stats = minmax_bytes((const double*)data[c], rows,
                                               m.mn, m.mx);
                    break;
            }
            if (!pw.write(f, g, c, codec == 1, (int32_t)rows, nullptr, 0,
                          (const uint8_t*)data[c], size_t(rows) * 8, off, m))
                return fail("write failed");
        }
        rgs.push_back(rg);
    }

    if (!metric_footer(f, rgs, n, false)) return fail("write failed");
    if (fclose(f) != 0) return "write_metric_sst: close failed";
    return "";
}

std::string write_metric_sst_nullable(const std::string& path,
                                      const uint64_t* series,
                                      const int64_t* ts,
                                      const NullableValues& value,
                                      const uint64_t* seqs, uint64_t seq,
                                      int64_t n, int64_t row_group,
                                      int32_t codec,
                                      const PagePayload* ready) {
    if (n <= 0) return "write_metric_sst_nullable: no rows";
    if (codec != 0 && codec != 1)
        return "write_metric_sst_nullable: unknown codec";
    if (row_group <= 0 || row_group % 64)
        return "write_metric_sst_nullable: row_group is not a multiple of 64";
    const int64_t wpg = row_group / 64;
    for (int64_t g = 0, base = 0; base < n; g++, base += row_group)
        if (value.n_valid[g] > std::min<int64_t>(row_group, n - base))
            return "write_metric_sst_nullable: n_valid above the row count";
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) return "write_metric_sst_nullable: cannot open " + path;
    auto fail = [&](const char* m) {
        fclose(f);
        remove(path.c_str());
        return std::string(m);
    };
    if (fwrite("PAR1", 1, 4, f) != 4) return fail("write failed");
    int64_t off = 4;

    std::vector<uint64_t> seq_col, zeros;
    std::vector<uint8_t> levels;
    std::vector<MetricRG> rgs;
    PageWriter pw(codec, ready, 5);
    for (int64_t g = 0, base = 0; base < n; g++, base += row_group) {
        const int64_t rows = std::min<int64_t>(row_group, n - base);
        if (!seqs && (int64_t)seq_col.size() < rows) seq_col.assign(rows, seq);
        if ((int64_t)zeros.size() < rows) zeros.assign(rows, 0);
        const int64_t nv = value.n_valid[g];
        const uint64_t* packed = value.packed + base;
        levels.clear();
        encode_def_levels(value.bitmap_words + g * wpg, (uint32_t)rows,
                          (uint32_t)nv, levels);
        const void* data[5] = {series ? series + base : nullptr,
                               ts ? ts + base : nullptr, packed,
                               seqs ? seqs + base : seq_col.data(),
                               zeros.data()};
        MetricRG rg;
        rg.num_rows = rows;
        for (int c = 0; c < 5; c++) {
            const int64_t body = (c == 2 ? nv : rows) * 8;
            ChunkMeta& m = rg.cols[c];
            m.num_values = rows;
            if (!column_present(data[c], ready, g * 5 + c, codec))
                return fail("write_metric_sst_nullable: column neither given "
                            "nor ready");
            if (c == 2) {
                m.optional = true;
                m.null_count = rows - nv;
            }
            if (!stats_from_ready(ready, g * 5 + c, m)) switch (c) {
                case 0: case 3: case 4:
                    minmax_bytes((const uint64_t*)data[c], rows, m.mn, m.mx);
                    break;
                case 1:
                    minmax_bytes((const int64_t*)data[c], rows, m.mn, m.mx);
                    break;
                case 2:
                    m.has_stats = minmax_bytes((const double*)data[c], nv,
                                               m.mn, m.mx);
                    break;
            }
            if (!pw.write(f, g, c, codec == 1, (int32_t)rows, levels.data(),
                          c == 2 ? levels.size() : 0,
                          (const uint8_t*)data[c], size_t(body), off, m))
                return fail("write failed");
        }
        rgs.push_back(rg);
    }
    if (!metric_footer(f, rgs, n, true)) return fail("write failed");
    if (fclose(f) != 0) return "write_metric_sst_nullable: close failed";
    return "";
}

// ---------------------------------------------------------------------------
// General flat-table writer (BYTE_ARRAY-capable) for the RFC's auxiliary
// tables (rfc:86-137) and per-row-seq compaction outputs. Same page/footer
// layout as write_metric_sst: one PLAIN uncompressed data page v1 per
// chunk, row groups of `row_group` rows, min/max statistics (omitted for
// byte values longer than 64 B), thrift-compact footer with column_orders.
// ---------------------------------------------------------------------------
std::string write_table_sst(const std::string& path, const WriterCol* cols,
                            int32_t n_cols, int64_t n, int64_t row_group,
                            int32_t codec, const PagePayload* ready,
                            int32_t ba_codec, uint32_t ba_page_limit) {
    if (n <= 0 || n_cols <= 0) return "write_table_sst: no rows/cols";
    if (ba_page_limit > BA_PAGE_LIMIT_MAX)
        return "write_table_sst: page limit above 2^30";
    if ((codec != 0 && codec != 1) || (ba_codec != 0 && ba_codec != 1))
        return "write_table_sst: unknown codec";
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) return "write_table_sst: cannot open " + path;
    auto fail = [&](const char* m) {
        fclose(f);
        remove(path.c_str());
        return std::string(m);
    };
    for (int c = 0; c < n_cols; c++) {
        const WriterCol& wc = cols[c];
        if (wc.physical != 2 && wc.physical != 5 && wc.physical != 6)
            return fail("write_table_sst: unsupported physical type");
        if (wc.physical == 6 && !wc.offsets && !ready)
            return fail("write_table_sst: BYTE_ARRAY needs offsets");
    }
    if (fwrite("PAR1", 1, 4, f) != 4) return fail("write failed");
    int64_t off = 4;

    struct RG {
        int64_t num_rows;
        std::vector<ChunkMeta> cols;
    };
    std::vector<RG> rgs;
    std::vector<uint8_t> payload;
    std::vector<uint32_t> cut_rows, cut_ulen, cut_len;
    std::vector<uint64_t> cut_sums, cut_bytes;
    PageWriter pw(codec, ready, n_cols);
    for (int64_t g = 0, base = 0; base < n; g++, base += row_group) {
        int64_t rows = std::min<int64_t>(row_group, n - base);
        RG rg;
        rg.num_rows = rows;
        rg.cols.resize(n_cols);
        for (int c = 0; c < n_cols; c++) {
            const WriterCol& wc = cols[c];
            ChunkMeta& m = rg.cols[c];
            m.num_values = rows;
            const uint8_t* body = nullptr;
            size_t body_len = 0;
            if (wc.physical == 6) {
                // a ready entry IS the uncompressed page image (kernel 1f),
                // or under ba_codec 1 the image's Snappy stream with its
                // size and statistics; otherwise the image is built here
                // from (bytes, offsets)
                const PagePayload* r6 =
                    ready && ready[g * n_cols + c].ptr
                        ? &ready[g * n_cols + c] : nullptr;
                if (r6 && ba_codec == 1) {
                    const BaPageStat* bs = r6->ba_stat;
                    if (!bs || bs->min_len > BA_STAT_MAX ||
                        bs->max_len > BA_STAT_MAX)
                        return fail("write_table_sst: a ready BYTE_ARRAY "
                                    "stream needs its statistics");
                    if (r6->ulen > 0x7FFFFFFFull)
                        return fail("write_table_sst: BYTE_ARRAY page image "
                                    "above INT32_MAX bytes");
                    m.has_stats = bs->has != 0;
                    m.mn.assign((const char*)bs->min, bs->min_len);
                    m.mx.assign((const char*)bs->max, bs->max_len);
                    if (r6->n_split > 1) {
                        uint64_t sl = 0;
                        for (uint32_t i = 0; r6->split_len && i < r6->n_split;
                             i++)
                            sl += r6->split_len[i];
                        if (!split_ok(*r6, rows, r6->ulen) ||
                            !r6->split_len || sl != r6->len)
                            return fail("write_table_sst: a ready BYTE_ARRAY "
                                        "entry's page cuts do not add up");
                        if (!write_ba_pages(f, true, r6->n_split,
                                            r6->split_rows, r6->split_ulen,
                                            nullptr, r6->ptr, r6->split_len,
                                            off, m))
                            return fail("write failed");
                        continue;
                    }
                    if (!pw.write(f, g, c, true, (int32_t)rows, nullptr, 0,
                                  nullptr, r6->ulen, off, m))
                        return fail("write failed");
                    continue;
                }
                uint32_t n_cut = 0;
                const uint32_t *cr_ = nullptr, *cu_ = nullptr;
                if (r6) {
                    body = r6->ptr;
                    body_len = r6->len;
                    if (r6->n_split > 1) {
                        if (!split_ok(*r6, rows, r6->len))
                            return fail("write_table_sst: a ready BYTE_ARRAY "
                                        "entry's page cuts do not add up");
                        n_cut = r6->n_split;
                        cr_ = r6->split_rows;
                        cu_ = r6->split_ulen;
                    }
                } else {
                    if (!wc.offsets)
                        return fail("write_table_sst: BYTE_ARRAY needs "
                                    "offsets");
                    const uint8_t* bytes = (const uint8_t*)wc.data;
                    payload.clear();
                    for (int64_t r = base; r < base + rows; r++) {
                        int64_t b0 = wc.offsets[r], b1 = wc.offsets[r + 1];
                        if (b1 < b0 || b1 - b0 > 0x7FFFFFFF)
                            return fail("write_table_sst: bad offsets");
                        uint32_t len = (uint32_t)(b1 - b0);
                        payload.insert(payload.end(), (const uint8_t*)&len,
                                       (const uint8_t*)&len + 4);
                        payload.insert(payload.end(), bytes + b0, bytes + b1);
                    }
                    body = payload.data();
                    body_len = payload.size();
                    if (ba_page_limit && payload.size() <= 0x7FFFFFFFull) {
                        // the cut rule over this row group's rows
                        cut_len.resize(size_t(rows));
                        for (int64_t r = 0; r < rows; r++)
                            cut_len[r] = uint32_t(wc.offsets[base + r + 1] -
                                                  wc.offsets[base + r]);
                        const size_t nb = size_t(ba_n_batches(rows, rows));
                        cut_sums.resize(nb);
                        cut_bytes.resize(nb);
                        cut_rows.resize(nb);
                        cut_ulen.resize(nb);
                        ba_batch_sizes_host(cut_len.data(), uint64_t(rows),
                                            uint64_t(rows), cut_sums.data());
                        n_cut = ba_cut_pages(cut_sums.data(), uint64_t(rows),
                                             ba_page_limit, cut_rows.data(),
                                             cut_bytes.data());
                        for (uint32_t i = 0; i < n_cut; i++)
                            cut_ulen[i] = uint32_t(cut_bytes[i]);
                        cr_ = cut_rows.data();
                        cu_ = cut_ulen.data();
                    }
                }
                if (body_len > 0x7FFFFFFFull)
                    return fail("write_table_sst: BYTE_ARRAY page image "
                                "above INT32_MAX bytes");
                // statistics by walking the image, whoever built it
                const uint8_t *mn = nullptr, *mx = nullptr;
                uint32_t mn_len = 0, mx_len = 0;
                auto less = [](const uint8_t* a, uint32_t al,
                               const uint8_t* b, uint32_t bl) {
                    const int k = std::memcmp(a, b, al < bl ? al : bl);
                    return k < 0 || (k == 0 && al < bl);
                };
                size_t pos = 0;
                for (int64_t r = 0; r < rows; r++) {
                    if (pos + 4 > body_len)
                        return fail("write_table_sst: short BYTE_ARRAY page");
                    uint32_t len;
                    std::memcpy(&len, body + pos, 4);
                    pos += 4;
                    if (len > body_len - pos)
                        return fail("write_table_sst: short BYTE_ARRAY page");
                    const uint8_t* v = body + pos;
                    if (r == 0 || less(v, len, mn, mn_len)) mn = v, mn_len = len;
                    if (r == 0 || less(mx, mx_len, v, len)) mx = v, mx_len = len;
                    pos += len;
                }
                if (pos != body_len)
                    return fail("write_table_sst: BYTE_ARRAY page longer "
                                "than its rows");
                m.has_stats = mn_len <= 64 && mx_len <= 64;
                m.mn.assign((const char*)mn, mn_len);
                m.mx.assign((const char*)mx, mx_len);
                if (n_cut > 1) {
                    if (!write_ba_pages(f, ba_codec == 1, n_cut, cr_, cu_,
                                        body, nullptr, nullptr, off, m))
                        return fail("write failed");
                    continue;
                }
            } else {
                if (!column_present(wc.data, ready, g * n_cols + c, codec))
                    return fail("write_table_sst: column neither given nor "
                                "ready");
                body = wc.data ? (const uint8_t*)wc.data + base * 8 : nullptr;
                body_len = size_t(rows) * 8;
                if (stats_from_ready(ready, g * n_cols + c, m)) {
                    // the ready page brought them
                } else if (wc.physical == 5)
                    m.has_stats = minmax_bytes((const double*)wc.data + base,
                                               rows, m.mn, m.mx);
                else if (wc.converted == 14)
                    minmax_bytes((const uint64_t*)wc.data + base, rows, m.mn,
                                 m.mx);
                else
                    minmax_bytes((const int64_t*)wc.data + base, rows, m.mn,
                                 m.mx);
            }
            // BYTE_ARRAY chunks follow ba_codec (a ready stream was written
            // above; an image built here is compressed here)
            if (!pw.write(f, g, c,
                          wc.physical != 6 ? codec == 1 : ba_codec == 1,
                          (int32_t)rows, nullptr, 0, body, body_len, off, m))
                return fail("write failed");
        }
        rgs.push_back(std::move(rg));
    }

    TW w;
    int16_t last = 0;
    w.i32(last, 1, 1);  // version
    w.list_header(last, 2, 12, size_t(n_cols) + 1);
    {
        int16_t l2 = 0;
        w.str(l2, 4, "schema");
        w.i32(l2, 5, n_cols);
        w.stop();
    }
    for (int c = 0; c < n_cols; c++) {
        const WriterCol& wc = cols[c];
        int16_t l2 = 0;
        w.i32(l2, 1, wc.physical);
        w.i32(l2, 3, 0);  // REQUIRED
        w.str(l2, 4, wc.name);
        if (wc.converted >= 0) w.i32(l2, 6, wc.converted);
        w.stop();
    }
    w.i64f(last, 3, n);
    w.list_header(last, 4, 12, rgs.size());
    for (const auto& rg : rgs) {
        int16_t l2 = 0;
        w.list_header(l2, 1, 12, n_cols);
        int64_t total = 0;
        for (int c = 0; c < n_cols; c++) total += rg.cols[c].total_size;
        for (int c = 0; c < n_cols; c++)
            column_chunk(w, cols[c].name, cols[c].physical, rg.cols[c]);
        w.i64f(l2, 2, total);
        w.i64f(l2, 3, rg.num_rows);
        w.stop();
    }
    w.str(last, 6, "horaedb-amd hx table writer");
    w.list_header(last, 7, 12, n_cols);
    for (int c = 0; c < n_cols; c++) {
        int16_t l2 = 0;
        w.field(l2, 1, 12);
        w.stop();
        w.stop();
    }
    w.stop();

    uint32_t flen = (uint32_t)w.buf.size();
    if (fwrite(w.buf.data(), 1, flen, f) != flen) return fail("write failed");
    if (fwrite(&flen, 4, 1, f) != 1) return fail("write failed");
    if (fwrite("PAR1", 1, 4, f) != 4) return fail("write failed");
    if (fclose(f) != 0) return "write_table_sst: close failed";
    return "";
}

std::string write_metric_sst_seqs(const std::string& path,
                                  const uint64_t* series, const int64_t* ts,
                                  const double* value, const uint64_t* seqs,
                                  int64_t n, int64_t row_group,
                                  int32_t codec, const PagePayload* ready) {
    std::vector<uint64_t> zeros(n, 0);
    WriterCol cols[5] = {
        {"series_id", 2, 14, series, nullptr},
        {"timestamp", 2, -1, ts, nullptr},
        {"value", 5, -1, value, nullptr},
        {"__seq__", 2, 14, seqs, nullptr},
        {"__reserved__", 2, 14, zeros.data(), nullptr},
    };
    return write_table_sst(path, cols, 5, n, row_group, codec, ready);
}

std::string write_metric_sst_bytes(const std::string& path,
                                   const uint64_t* series, const int64_t* ts,
                                   const uint8_t* bytes,
                                   const int64_t* offsets,
                                   const uint64_t* seqs, uint64_t seq,
                                   int64_t n, int64_t row_group,
                                   const PagePayload* ready, int32_t codec,
                                   uint32_t page_limit) {
    if (n <= 0) return "write_metric_sst_bytes: no rows";
    std::vector<uint64_t> zeros(n, 0), seq_col;
    if (!seqs) {
        seq_col.assign(n, seq);
        seqs = seq_col.data();
    }
    WriterCol cols[5] = {
        {"series_id", 2, 14, series, nullptr},
        {"timestamp", 2, -1, ts, nullptr},
        {"value", 6, -1, bytes, offsets},
        {"__seq__", 2, 14, seqs, nullptr},
        {"__reserved__", 2, 14, zeros.data(), nullptr},
    };
    return write_table_sst(path, cols, 5, n, row_group, codec, ready, codec,
                           page_limit);
}

}  // namespace hx
