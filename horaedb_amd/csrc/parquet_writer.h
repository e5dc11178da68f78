// parquet_writer.h — minimal native Parquet writer for compaction output
// (DESIGN.md §10 / SURVEY §8(f) row 1). Writes exactly the reference writer's
// metric-SST layout (storage.rs:193-298 contract): 5 flat REQUIRED columns
// (series_id u64, timestamp i64, value f64, __seq__ u64, __reserved__ u64),
// row groups of `row_group` rows, one PLAIN data page v1 per chunk
// (uncompressed, or Snappy as the reference's default config writes them),
// min/max statistics, thrift-compact footer. Readable by parquet-rs /
// pyarrow (validated in tests) and by our own reader.
#pragma once
#include <cstdint>
#include <string>

#include "ba_pages.h"

namespace hx {

// Codec of the 8-byte columns' pages: 0 = UNCOMPRESSED (the default; the file
// is what it always was), 1 = SNAPPY. Under Snappy every page payload is the
// stream hx::snappy_compress_host (snappy_compress.h) gives for the page's
// uncompressed bytes — for an OPTIONAL value page {level block, packed
// values}, the level block inside the stream. `ready` optionally brings
// streams made elsewhere (kernel 1e): entry [row group * n_cols + column],
// ptr null = absent, the writer compresses that page itself. A ready stream
// must be the twin's bytes for the page, so the file does not depend on who
// compressed it. BYTE_ARRAY chunks have a codec of their own (ba_codec of
// write_table_sst, codec of write_metric_sst_bytes; 0 by default, so the index
// tables stay uncompressed under every `codec`). Under ba_codec 0 a ready
// entry for one IS its uncompressed page image (u32 length + bytes per row,
// kernel 1f or hx::ba_build_pages_host) and its statistics are computed by
// the writer from the image. Under ba_codec 1 a ready entry is the page's
// Snappy STREAM (kernel 1e over the image, or the twin), with ulen = the
// image's size and ba_stat = the chunk's statistics (kernel 1g or
// hx::ba_page_minmax_host): no value byte reaches the writer.
// A ready entry may bring the chunk's statistics too (k_page_minmax, the raw
// 8 bytes of min and max as minmax over the column would give them); a
// column whose every page comes ready WITH statistics may be passed as a
// null pointer — its rows never reach the host.
struct PagePayload {
    const uint8_t* ptr;
    uint32_t len;
    uint32_t stats;      // 0: the writer computes them from the column;
                         // 1: min_bits / max_bits; 2: the chunk has none
    uint64_t min_bits;
    uint64_t max_bits;
    // BYTE_ARRAY stream entries (ba_codec 1) only
    uint32_t ulen = 0;                     // uncompressed page size
    const BaPageStat* ba_stat = nullptr;   // the chunk's statistics
    // A BYTE_ARRAY entry cut into n_split data pages (hx::ba_cut_pages; 0 or 1
    // = one page, every field above as it always was). split_rows and
    // split_ulen give each page's rows and uncompressed bytes; they add up to
    // the chunk's rows and to the whole image (len under ba_codec 0, ulen
    // under ba_codec 1). Under ba_codec 0 ptr is still the one image and the
    // pages are its consecutive slices; under ba_codec 1 ptr holds the
    // pages' streams back to back, split_len bytes each (len = their sum),
    // each the twin's stream of its slice.
    uint32_t n_split = 0;
    const uint32_t* split_rows = nullptr;
    const uint32_t* split_ulen = nullptr;
    const uint32_t* split_len = nullptr;
};

// columns are caller-provided arrays of n rows; seq is constant per file
// (the compacted file's sequence — see hx_compact's closure precondition).
// Returns empty string on success, else an error message.
std::string write_metric_sst(const std::string& path, const uint64_t* series,
                             const int64_t* ts, const double* value,
                             uint64_t seq, int64_t n, int64_t row_group,
                             int32_t codec = 0,
                             const PagePayload* ready = nullptr);

// Nullable form of the metric writer: the `value` column is declared OPTIONAL
// (the reference's shape for it), the four others stay REQUIRED. The values
// come row-group-major, as kernel 1d (k_pack_optional) and
// hx::pack_optional_host leave them: row group g covers rows
// [g * row_group, min(n, (g + 1) * row_group)); row_group is a multiple of 64.
struct NullableValues {
    const uint64_t* packed;        // packed + g * row_group: n_valid[g]
                                   // present values in row order, 64 bits each
    const uint64_t* bitmap_words;  // + g * (row_group / 64): LSB-first, 1 =
                                   // present, bits at and above the row
                                   // group's row count zero
    const uint32_t* n_valid;       // per row group
};
// Every value page is {level block, n_valid * 8 PLAIN bytes} with
// DataPageHeader.num_values = rows; statistics always carry null_count, and
// min/max over the present values by the DOUBLE rules (none for a chunk
// without a non-NaN value). seqs: per-row __seq__ values, or NULL for the
// constant `seq`.
std::string write_metric_sst_nullable(const std::string& path,
                                      const uint64_t* series,
                                      const int64_t* ts,
                                      const NullableValues& value,
                                      const uint64_t* seqs, uint64_t seq,
                                      int64_t n, int64_t row_group,
                                      int32_t codec = 0,
                                      const PagePayload* ready = nullptr);

// General flat-table writer (same page/footer layout) for the auxiliary
// tables the RFC defines (metrics/series/tags/index,
// docs/rfcs/20240827-metric-engine.md:86-137). Fixed 8-byte columns
// (INT64/DOUBLE, optionally UINT_64-converted) and BYTE_ARRAY columns
// (PLAIN: u32 length + bytes; offsets[n+1] into `bytes`).
struct WriterCol {
    const char* name;
    int32_t physical;        // 2 INT64, 5 DOUBLE, 6 BYTE_ARRAY
    int32_t converted;       // -1 none, 14 UINT_64
    const void* data;        // 8-byte array, or bytes blob for BYTE_ARRAY
    const int64_t* offsets;  // BYTE_ARRAY only: n+1 offsets into data
};

std::string write_table_sst(const std::string& path, const WriterCol* cols,
                            int32_t n_cols, int64_t n, int64_t row_group,
                            int32_t codec = 0,
                            const PagePayload* ready = nullptr,
                            int32_t ba_codec = 0,
                            uint32_t ba_page_limit = 0);

// per-row variable-length seq variant of the metric writer (general
// compaction outputs, executor.rs:155-222 keep_builtin path)
std::string write_metric_sst_seqs(const std::string& path,
                                  const uint64_t* series, const int64_t* ts,
                                  const double* value, const uint64_t* seqs,
                                  int64_t n, int64_t row_group,
                                  int32_t codec = 0,
                                  const PagePayload* ready = nullptr);

// Binary-value form of the metric writer (the schema behind
// BytesMergeOperator / UpdateMode::Append): series_id (INT64/UINT_64),
// timestamp (INT64), value (BYTE_ARRAY, no converted type), __seq__,
// __reserved__, all REQUIRED — the names and types pyarrow-written Binary SSTs
// of a store carry, so both kinds mix in one store. seqs: per-row __seq__, or
// NULL for the constant `seq`. The value column comes as (bytes,
// offsets[n + 1]) or, per row group, as a ready entry [row group * 5 + 2]
// holding the UNCOMPRESSED page image (u32 length + bytes per row; kernel 1f
// or hx::ba_build_pages_host); with every page ready, bytes and offsets may
// be null. codec 0 (the default) writes every page uncompressed, the file it
// always wrote; codec 1 writes all five columns' pages as Snappy streams
// (hx::snappy_compress_host of the page bytes, the stored form for an
// incompressible page), and a ready entry for the value column is then the
// stream with ulen and ba_stat (PagePayload). Statistics are the
// lexicographic min/max of the page's values, omitted above 64 B, so the file
// is a pure function of the rows and the codec whichever route built the
// pages. page_limit (0 = one data page per chunk, the file it always wrote;
// else at most BA_PAGE_LIMIT_MAX) cuts a value image built here from (bytes,
// offsets) into data pages by hx::ba_cut_pages; a ready entry brings its own
// cuts (PagePayload::n_split) and the limit does not touch it.
std::string write_metric_sst_bytes(const std::string& path,
                                   const uint64_t* series, const int64_t* ts,
                                   const uint8_t* bytes,
                                   const int64_t* offsets,
                                   const uint64_t* seqs, uint64_t seq,
                                   int64_t n, int64_t row_group,
                                   const PagePayload* ready = nullptr,
                                   int32_t codec = 0,
                                   uint32_t page_limit = 0);

}  // namespace hx
