/* horaedb_hx.h — C-ABI drop-in boundary for HoraeDB's metric-engine scan/
 * aggregate hot path, MI355X-native (gfx950 HIP kernels behind this ABI).
 *
 * Each entry point names the reference interface it replaces (apache/horaedb
 * `main`, paths relative to /root/reference/src). The reference surface kept
 * (SURVEY.md §8(b)):
 *   trait ColumnarStorage { schema/write/scan/compact }   columnar_storage/src/storage.rs:76-89
 *   ScanRequest { range, predicate, projections }         columnar_storage/src/storage.rs:65-70
 *   trait MergeOperator { merge(batch) -> batch }         columnar_storage/src/operator.rs:30-34
 *
 * Conventions: all structs are POD; caller owns all inputs; callee allocates
 * outputs, freed by the matching hx_*_free; status codes + hx_last_error()
 * (thread-local string). Concurrency: scan-side calls (hx_prepare /
 * hx_scan_agg / hx_scan) may run from many threads of one handle; a given
 * hx_prepared serves ONE call at a time; catalog mutations (hx_write,
 * hx_compact) require external serialization against all other calls, and
 * hx_find_ssts results are invalidated by the next hx_find_ssts on the
 * same handle. All compute is GPU-resident — if no
 * MI355X/HIP runtime is available every scan entry returns HX_ERR_NO_GPU
 * (there is no CPU fallback in this library).
 */
#ifndef HORAEDB_HX_H
#define HORAEDB_HX_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef int32_t hx_status;
enum {
    HX_OK             = 0,
    HX_ERR_IO         = 1,   /* file missing/unreadable */
    HX_ERR_FORMAT     = 2,   /* not a parquet SST / unsupported layout */
    HX_ERR_UNSUPPORTED= 3,   /* encoding/codec outside round-1 scope; nulls
                                in series_id/timestamp/__seq__, in a
                                dictionary-encoded or Binary value column,
                                under Append mode; null values reaching the
                                write side (compaction inputs, a zero bit
                                given to hx_write_nullable) of a handle
                                that has not set hx_set_nullable_values;
                                hx_set_write_codec on a store with a
                                Binary value column                       */
    HX_ERR_NO_GPU     = 4,   /* HIP runtime/device unavailable */
    HX_ERR_HIP        = 5,   /* HIP call failed (see hx_last_error) */
    HX_ERR_INVALID    = 6,   /* bad argument */
    HX_ERR_SCHEMA     = 7,   /* SST schema violates the metric contract */
};

/* Thread-local description of the last error from this thread. */
const char* hx_last_error(void);

/* ---- time range: [start, end), ms — types.rs:46-133 (TimeRange) -------- */
typedef struct { int64_t start; int64_t end; } hx_time_range;

/* ---- SST descriptor — sst.rs:154-160 (SstFile/FileMeta) ---------------- */
typedef struct {
    const char* path;       /* parquet file written by the reference writer */
    uint64_t    sequence;   /* __seq__ of every row in the file (= file id,
                               sst.rs:39-46); dedup winner = max sequence    */
} hx_sst_desc;

/* ---- predicates — ScanRequest.predicate (storage.rs:65-70) ------------- */
typedef enum {
    HX_PRED_SERIES_IN = 1,  /* series_id ∈ set (tag predicate materialized as
                               a series-id set, BASELINE config 3)           */
} hx_pred_kind;

typedef struct {
    int32_t kind;                   /* hx_pred_kind */
    const uint64_t* series_ids;     /* HX_PRED_SERIES_IN: sorted or not */
    size_t          n_series;
} hx_pred;

/* ---- scan spec — ScanRequest (storage.rs:65-70) ------------------------ */
typedef struct {
    hx_time_range   range;      /* ts-range predicate + SST pruning          */
    const hx_pred*  preds;      /* extra predicates, may be NULL             */
    size_t          n_preds;
    const hx_sst_desc* ssts;    /* explicit SST list; NULL => all SSTs the
                                   handle discovered under {store}/data that
                                   overlap `range` (Manifest::find_ssts,
                                   manifest/mod.rs:165-172)                  */
    size_t          n_ssts;
    const int32_t*  projection; /* hx_scan only: user-column indices, NULL =
                                   all user columns (builtins stripped —
                                   types.rs:203-239)                         */
    size_t          n_projection;
} hx_scan_spec;

/* ---- aggregate spec — no reference counterpart;
 * semantics pinned by BASELINE.json configs + rfc:218-231 ----------------- */
enum {
    HX_AGG_SUM   = 1u << 0,
    HX_AGG_COUNT = 1u << 1,
    HX_AGG_MIN   = 1u << 2,
    HX_AGG_MAX   = 1u << 3,
    HX_AGG_AVG   = 1u << 4,   /* finalized as sum/count */
    HX_AGG_FIRST = 1u << 5,   /* value at the group's smallest timestamp */
    HX_AGG_LAST  = 1u << 6,   /* value at the group's greatest timestamp */
};
/* Null values (OPTIONAL f64 value column): a row with a null value is still
 * a row — it passes or fails the filter and takes part in dedup like any
 * other (a newer null shadows an older value of the same PK, and is shadowed
 * by a newer value) and counts in hx_exec_stats.rows_matched. The aggregates
 * run over the non-null survivors: sum/min/max/avg ignore nulls and count
 * counts values. A group all of whose surviving values are null is not
 * emitted (the result table has no validity channel).
 * Write side: a handle writes REQUIRED columns and refuses null values
 * (HX_ERR_UNSUPPORTED, nothing written or unlinked) until
 * hx_set_nullable_values(h, 1); from then on every SST it writes declares
 * `value` OPTIONAL, hx_write_nullable ingests null rows, and hx_compact /
 * hx_compact_files keep a surviving null as a null row — it is still the
 * winner of its PK and goes on shadowing older values in other files.
 *
 * Value domain (every f64 bit pattern is data: NaN of either sign and any
 * payload — the Prometheus stale marker 0x7FF0000000000002 is a signalling
 * NaN — signed zeros, infinities, subnormals):
 *   min / max  IEEE 754 totalOrder over the surviving non-null values:
 *              -NaN < -inf < ... < -0 < +0 < ... < +inf < +NaN, NaNs of one
 *              sign ordered by payload (Rust's f64::total_cmp). The 64 bits
 *              of the chosen value are returned unchanged: payload,
 *              signalling bit and the sign of zero. On one device the
 *              result does not depend on where a row sits in its file.
 *              EXCEPTION, more than one device: the host merge of the
 *              per-device partials still combines vmin/vmax with
 *              std::min/std::max on doubles, so for a group whose rows are
 *              split across devices a NaN may be dropped or kept and the
 *              sign of a zero chosen by the order of the partials.
 *   sum / avg  NaN (payload unspecified) if the group holds a NaN or both
 *              infinities; else the infinity it holds; else the finite sum
 *              of an unspecified order of additions (an overflowing one is
 *              an infinity). Subnormal terms and partial sums are kept on
 *              every route (no flush to zero). The sign of a zero sum is
 *              unspecified (accumulators start at +0.0).
 *   count      a NaN is a value and counts; only nulls drop out.
 *   hx_scan, hx_compact, hx_compact_files, hx_write: every value's 64 bits
 *              come back unchanged. Files written here carry DOUBLE
 *              statistics as parquet-format demands: no NaN in min/max (a
 *              row group of nothing but NaN carries none), a zero bound
 *              written min = -0.0 / max = +0.0.
 *
 * first / last (HX_AGG_FIRST, HX_AGG_LAST): a group is series_id, or
 * (series_id, floor(ts / bucket_ms)). `last` is the value of the group's
 * surviving non-null row with the greatest timestamp and `last_ts` that
 * timestamp; `first` / `first_ts` the same with the smallest. "Surviving" is
 * what every other aggregate means: after the ts-range filter, the series-set
 * filter and dedup. A null is still a row for dedup (a newer null shadows an
 * older value) and drops out afterwards, so `last` is the latest NON-NULL
 * survivor; a group without one is not emitted, as for the other ops.
 *   value      the 64 bits of the chosen value come back unchanged: NaN
 *              payload, signalling bit, the sign of zero, subnormals. The
 *              stale marker 0x7FF0000000000002 is a value: if it is a series'
 *              latest sample, `last` returns exactly it.
 *   timestamp  full-range int64: negative timestamps and an unbounded query
 *              range work.
 *   ties       after dedup two survivors of one group share a timestamp only
 *              if the same primary key survives in two time segments
 *              (segments are unioned without dedup). Among the rows tied at
 *              the extreme timestamp the value greatest in totalOrder wins,
 *              for first and for last: arbitrary, but deterministic and
 *              independent of row position, as min/max are.
 *   devices    on more than one device the partials merge by the same rules
 *              (greater last_ts, smaller first_ts, ties to the totalOrder-
 *              greater value), on bit patterns: no exception as for
 *              vmin/vmax above.
 * A request of only FIRST and/or LAST is valid. On a Binary value store they
 * are refused like every aggregate (HX_ERR_UNSUPPORTED). */
typedef struct {
    uint32_t ops;         /* OR of HX_AGG_*  (over the value column) */
    int64_t  bucket_ms;   /* 0: group by series_id; >0: by (series_id,
                             timestamp/bucket_ms) — config 5 downsample */
} hx_agg_spec;

typedef struct {
    const int32_t* device_ids;  /* HIP device ordinals; NULL => {0} */
    int32_t        n_devices;
} hx_device_set;

/* ---- results ----------------------------------------------------------- */
/* Aggregate result: one row per group, sorted by (series_id, bucket) —
 * the reference stream's PK order (read.rs:479-494). Arrays are owned by the
 * table; NULL when the op was not requested. */
typedef struct hx_result_table {
    size_t          n_groups;
    const uint64_t* series_id;
    const int64_t*  bucket;     /* bucket index (ts/bucket_ms); NULL if bucket_ms==0 */
    const double*   sum;
    const uint64_t* count;
    const double*   vmin;
    const double*   vmax;
    const double*   avg;
    /* Appended members. Tables are produced by the library and handed out
     * by pointer, so callers built against the eight-member struct keep
     * working (hx_col_batch.validity is the precedent). first / first_ts
     * are non-NULL iff HX_AGG_FIRST was asked, last / last_ts iff
     * HX_AGG_LAST. The values are f64 bit patterns: read them as 64-bit
     * words where a NaN payload matters. */
    const double*   first;
    const int64_t*  first_ts;
    const double*   last;
    const int64_t*  last_ts;
} hx_result_table;

/* Streaming columnar batch for the non-aggregating parity mode — the
 * SendableRecordBatchStream analog (storage.rs:84, read.rs:349-385).
 * Columns follow the projection order; builtin __seq__/__reserved__ are
 * stripped as MergeStream does (read.rs:330-343). Column buffers are valid
 * only during the callback. */
/* variable-length byte column payload (Binary value schema): for a column
 * of type 3, the batch's cols[i] points at ONE hx_bytes_col; row r's value
 * is bytes[offsets[r] .. offsets[r+1]). */
typedef struct {
    const int64_t* offsets;       /* n_rows + 1 */
    const uint8_t* bytes;
} hx_bytes_col;

typedef struct {
    size_t   n_rows;
    size_t   n_cols;
    const void* const* cols;      /* col i: n_rows × 8B elements, or ONE
                                     hx_bytes_col when col_types[i] == 3    */
    const int32_t*     col_types; /* 0=u64, 1=i64(ts ms), 2=f64, 3=bytes    */
    /* Appended member (batches are passed by pointer, so callers built
     * against the four-member struct keep working). NULL: every value of
     * every column is present. Otherwise one pointer per column: NULL (all
     * rows valid) or an LSB-first bitmap of n_rows bits, 1 = value present.
     * Only an f64 value column can carry nulls; the 8 bytes in cols[i] at a
     * null row are unspecified. */
    const uint8_t* const* validity;
} hx_col_batch;
typedef int32_t (*hx_batch_cb)(void* ctx, const hx_col_batch* batch); /* nonzero => stop */

/* ---- lifecycle --------------------------------------------------------- */
typedef struct hx_handle   hx_handle;
typedef struct hx_prepared hx_prepared;

/* Replaces ObjectBasedStorage::try_new (storage.rs:138-187): opens a store
 * rooted at `store_path` ({store}/data/*.sst), reads every SST footer into
 * an in-memory catalog (FileMeta: rows, size, ts min/max — sst.rs:154-160).
 * segment_duration_ms partitions SSTs into time segments exactly as
 * storage.rs:106-136 does (server default 12h, server/config.rs:53).
 * Sequence of each file = numeric file stem ({id}.sst, sst.rs:193-205). */
hx_status hx_open(const char* store_path, int64_t segment_duration_ms,
                  hx_handle** out);
void      hx_close(hx_handle*);

/* ColumnarStorage::schema (storage.rs:76-89; StorageSchema contract
 * types.rs:150-240): the store's column layout — user columns (primary keys
 * first) plus the appended builtin __seq__/__reserved__ UInt64 columns. */
typedef struct {
    const char* name;
    int32_t     col_type;     /* 0=u64, 1=i64(ts ms), 2=f64 */
    int32_t     is_primary_key;
    int32_t     is_builtin;
} hx_col_desc;
hx_status hx_schema(hx_handle*, const hx_col_desc** out, size_t* n_out,
                    size_t* n_primary_keys);

/* Catalog introspection (Manifest::find_ssts, manifest/mod.rs:165-172). */
hx_status hx_find_ssts(hx_handle*, hx_time_range range,
                       const hx_sst_desc** out, size_t* n_out);

/* Stage the scan's column chunks into device HBM (file IO + footer/page
 * parse + row-group pruning + PCIe upload). Untimed prep: the timed hot
 * path starts at hx_exec_agg with inputs resident in HBM. */
hx_status hx_prepare(hx_handle*, const hx_scan_spec*, const hx_device_set*,
                     hx_prepared** out);
void      hx_prepared_free(hx_prepared*);

/* The hot path: decode + filter + dedup-merge + group-by aggregate, fully
 * on-GPU. Replaces scan (storage.rs:335-370) + read plan (read.rs:429-494)
 * + MergeExec (read.rs:100-391) + the aggregate the north star adds. */
hx_status hx_exec_agg(hx_prepared*, const hx_agg_spec*, hx_result_table** out);
void      hx_result_free(hx_result_table*);

/* One-shot convenience: prepare + exec_agg + release staging. */
hx_status hx_scan_agg(hx_handle*, const hx_scan_spec*, const hx_agg_spec*,
                      const hx_device_set*, hx_result_table** out);

/* Non-aggregating parity mode: the merged, deduplicated, PK-sorted row
 * stream itself (ColumnarStorage::scan semantics, storage.rs:335-370),
 * delivered as columnar batches through `cb`. GPU decode/filter/merge with
 * host readback; for parity testing, not the bench path. */
hx_status hx_scan(hx_handle*, const hx_scan_spec*, const hx_device_set*,
                  hx_batch_cb cb, void* ctx);

/* Compaction (ColumnarStorage::compact, storage.rs:76-89; executor
 * semantics executor.rs:155-222): GPU-merges the ts-overlap closure of the
 * SSTs overlapping `range` into ONE new SST (fresh file id = old max + 1),
 * updates the catalog, unlinks the inputs (add-before-delete). The closure
 * guarantees no remaining file shares primary keys with the inputs, so the
 * output carries one constant __seq__ without changing future merges. */
hx_status hx_compact(hx_handle*, hx_time_range range, const hx_device_set*,
                     uint64_t* out_new_seq);

/* General compaction of an EXPLICIT input set (the executor's Task{inputs},
 * compaction/mod.rs:26-36 + executor.rs:155-222 keep_builtin path): merges
 * and deduplicates ONLY among the named files and writes one SST whose rows
 * RETAIN their per-row __seq__ values, so later merges against files
 * outside the set still order correctly (MergeStream reads __seq__ from the
 * row, read.rs:289-343). No closure precondition. The scan path detects
 * such mixed-seq files from the __seq__ column statistics and compares
 * per-row sequences during cross-SST dedup. */
hx_status hx_compact_files(hx_handle*, const uint64_t* input_seqs,
                           size_t n_inputs, const hx_device_set*,
                           uint64_t* out_new_seq);

/* UpdateMode (config.rs:166-172): 0 = Overwrite (LastValueOperator), 1 =
 * Append (BytesMergeOperator — requires a Binary value column,
 * operator.rs:47-111). Append changes hx_scan's merge: equal-PK rows'
 * value bytes CONCATENATE in ascending __seq__ order. */
hx_status hx_set_update_mode(hx_handle*, int32_t mode);

/* ColumnarStorage::write (storage.rs:76-89, :307-333): stable PK sort of
 * the batch (sort_batch, storage.rs:244-256), file id allocation
 * (= sequence), one new SST via the native writer, catalog add. Ingest-side
 * prep (not the GPU scan hot path). enable_check enforces the
 * segment-crossing check (storage.rs:309-316). */
hx_status hx_write(hx_handle*, const uint64_t* series, const int64_t* ts,
                   const double* value, int64_t n_rows, int32_t enable_check,
                   uint64_t* out_seq);

/* Writer setting, per handle like hx_set_update_mode; default 0. 0: nothing
 * this handle does changes — same files, same refusals. 1: every SST the
 * handle writes (hx_write, hx_write_nullable, hx_compact, hx_compact_files)
 * declares `value` OPTIONAL, the reference's shape for that column (a page
 * without nulls carries one RLE run of definition levels), and null values
 * are written as null rows instead of being refused. The four other columns
 * stay REQUIRED. Not for stores with a Binary value column. */
hx_status hx_set_nullable_values(hx_handle*, int32_t on);

/* hx_write with missing samples (the reference's Arrow batches can carry
 * them, types.rs:178-179). validity: LSB-first bitmap of n_rows bits, 1 =
 * value present; NULL = all present. The 8 bytes of value[] at a null row
 * are ignored. Validity follows its row through the stable PK sort, so of an
 * equal-PK pair the later row of the batch wins, null or not. A zero bit
 * while the handle's setting is 0 returns HX_ERR_UNSUPPORTED and writes
 * nothing; without one the call is hx_write. */
hx_status hx_write_nullable(hx_handle*, const uint64_t* series,
                            const int64_t* ts, const double* value,
                            const uint8_t* validity, int64_t n_rows,
                            int32_t enable_check, uint64_t* out_seq);

/* Nullable twin of hx_write_sst (no GPU needed): `value` OPTIONAL, validity
 * as for hx_write_nullable, rows written in the order given. row_group must
 * be a multiple of 64 (HX_ERR_INVALID otherwise). */
hx_status hx_write_sst_nullable(const char* path, const uint64_t* series,
                                const int64_t* ts, const double* value,
                                const uint8_t* validity, uint64_t seq,
                                int64_t n_rows, int64_t row_group);

/* Native SST writer (the compaction output path; PLAIN uncompressed,
 * row-group 8192 contract — storage.rs:193-298). Exposed for tests/ingest. */
hx_status hx_write_sst(const char* path, const uint64_t* series,
                       const int64_t* ts, const double* value, uint64_t seq,
                       int64_t n_rows, int64_t row_group);

/* Page codec of the SSTs this library writes. SNAPPY is the reference's
 * default on-disk form (PLAIN pages, Snappy-compressed, config.rs:120-133);
 * all five columns are compressed, an OPTIONAL value page with its level
 * block inside the stream. The bytes of a compressed page are a function of
 * the page bytes alone, whichever route (device ingest or compaction, host
 * ingest, hx_write_sst_codec) wrote the file. */
enum { HX_CODEC_NONE = 0, HX_CODEC_SNAPPY = 1 };

/* Writer setting, per handle like hx_set_nullable_values; default
 * HX_CODEC_NONE (nothing changes). From then on every SST the handle writes
 * (hx_write, hx_write_nullable, hx_compact, hx_compact_files) carries pages
 * of that codec; it combines freely with hx_set_nullable_values. An unknown
 * codec returns HX_ERR_INVALID; HX_CODEC_SNAPPY on a store with a Binary
 * value column returns HX_ERR_UNSUPPORTED (HX_CODEC_NONE changes nothing
 * and is accepted, as hx_set_nullable_values(h, 0) is). */
hx_status hx_set_write_codec(hx_handle*, int32_t codec);

/* GPU-free writer with a codec; nullable = 1 declares value OPTIONAL
 * (validity as for hx_write_sst_nullable), nullable = 0 requires validity
 * NULL. Codec 0 writes the file hx_write_sst / hx_write_sst_nullable write,
 * byte for byte. */
hx_status hx_write_sst_codec(const char* path, const uint64_t* series,
                             const int64_t* ts, const double* value,
                             const uint8_t* validity, int32_t nullable,
                             uint64_t seq, int64_t n_rows, int64_t row_group,
                             int32_t codec);

/* ---- Binary value stores: the write side ------------------------------
 * The schema behind BytesMergeOperator / UpdateMode::Append: series_id,
 * timestamp, value (BYTE_ARRAY), __seq__, __reserved__, all REQUIRED, pages
 * PLAIN, uncompressed by default or Snappy (hx_set_bytes_write_codec, the
 * reference's on-disk form). Read side: value pages may be uncompressed,
 * Snappy or Zstd, data page v1 or v2, the column REQUIRED or OPTIONAL
 * without nulls (the reference declares every column nullable); a null in
 * the value column is refused with HX_ERR_UNSUPPORTED. A value chunk may
 * hold any number of data pages (parquet-rs and arrow-cpp close a page once
 * it reaches 1 MiB); page value counts that do not add up to the chunk's
 * return HX_ERR_FORMAT. The 8-byte columns keep the one-page contract. A
 * Snappy value page that is nothing but literals (an incompressible page,
 * one literal per 64 KiB fragment) is read in place; any other is decoded
 * on the device into a tail of the staged blob, so value handles keep one
 * base.
 * THE VALUE LIMIT: a value is at most 2^20 - 1
 * bytes, because the reader describes a value by a handle with 20 length
 * bits (k_ba_offsets refuses a longer one at read time). Every writer
 * enforces it: a longer value given to hx_write_bytes / hx_write_sst_bytes
 * returns HX_ERR_INVALID; an Append compaction (hx_compact,
 * hx_compact_files) whose concatenation of one equal-PK group would exceed
 * it returns HX_ERR_UNSUPPORTED; hx_index_write refuses such a tag key or
 * value (HX_ERR_INVALID). A row group whose value page would exceed
 * image would exceed INT32_MAX bytes returns HX_ERR_UNSUPPORTED, with or
 * without a page limit (hx_set_bytes_page_limit cuts the image into pages,
 * it does not lift this bound). Every refusal comes before anything is
 * written or unlinked.
 *
 * hx_compact / hx_compact_files on such a store: Overwrite keeps the
 * winner's bytes (last wins). Append turns each equal-PK run of the inputs,
 * in ascending (__seq__, file row) order, into ONE row holding the
 * concatenation; hx_compact gives it the new file's sequence,
 * hx_compact_files the sequence of the run's FIRST row, the smallest
 * (BytesMergeOperator keeps element 0 of every non-value column,
 * operator.rs:99-102). Value bytes stay on the device until they leave as
 * finished page images. */

/* ColumnarStorage::write for the Binary schema: row i's value is
 * bytes[offsets[i], offsets[i + 1]). Segment check, stable PK sort (equal
 * PKs keep batch order), file id = sequence, catalog add. On an empty store
 * the store becomes a Binary store; on an f64 store HX_ERR_SCHEMA; with
 * hx_set_nullable_values(1) or a write codec set, HX_ERR_UNSUPPORTED.
 * hx_write / hx_write_nullable on a Binary store return HX_ERR_UNSUPPORTED.
 * From 65536 rows with a device the sort (the ingest sort hx_write uses)
 * and the page images are made on the GPU; the file is the same either way.
 * Unlike hx_write, which sorts on the host when a HIP call of its device
 * sort fails, a HIP failure on this route returns HX_ERR_HIP and writes
 * nothing. */
hx_status hx_write_bytes(hx_handle*, const uint64_t* series, const int64_t* ts,
                         const uint8_t* bytes, const int64_t* offsets,
                         int64_t n_rows, int32_t enable_check,
                         uint64_t* out_seq);

/* GPU-free writer of one Binary-value SST, rows in the order given; seqs:
 * per-row __seq__ values, or NULL for the constant seq. */
hx_status hx_write_sst_bytes(const char* path, const uint64_t* series,
                             const int64_t* ts, const uint8_t* bytes,
                             const int64_t* offsets, const uint64_t* seqs,
                             uint64_t seq, int64_t n_rows, int64_t row_group);

/* Page codec of the Binary writers, per handle; default HX_CODEC_NONE
 * (nothing changes: the files are what they always were, byte for byte).
 * With HX_CODEC_SNAPPY every SST that hx_write_bytes, hx_compact and
 * hx_compact_files write on a Binary store carries Snappy pages in all five
 * columns. A page's stream is a function of the page bytes alone (the stored
 * form for an incompressible page), and the footer statistics of a value
 * chunk are the lexicographic min/max of its values (omitted above 64
 * bytes), so a file does not depend on the route that wrote it: host ingest,
 * device ingest, either compaction, or hx_write_sst_bytes_codec. On the
 * device routes the page images never reach the host: statistics and streams
 * are made where the images lie.
 * hx_set_write_codec keeps its meaning and its refusals; this is a setting
 * of its own. An unknown codec returns HX_ERR_INVALID; HX_CODEC_SNAPPY on a
 * store with an f64 value column returns HX_ERR_UNSUPPORTED; on an empty
 * store it is accepted, and hx_write / hx_write_nullable then return
 * HX_ERR_UNSUPPORTED. Every refusal comes before anything is written. */
hx_status hx_set_bytes_write_codec(hx_handle*, int32_t codec);

/* hx_write_sst_bytes with a codec; codec 0 writes the file
 * hx_write_sst_bytes writes, byte for byte. */
hx_status hx_write_sst_bytes_codec(const char* path, const uint64_t* series,
                                   const int64_t* ts, const uint8_t* bytes,
                                   const int64_t* offsets,
                                   const uint64_t* seqs, uint64_t seq,
                                   int64_t n_rows, int64_t row_group,
                                   int32_t codec);

/* Data-page limit of the Binary writers' value chunks, per handle; default 0
 * (nothing changes: one data page per chunk, the files byte for byte what
 * they always were). Otherwise a value in [1, 2^30]: every value chunk that
 * hx_write_bytes, hx_compact and hx_compact_files write is cut into v1 PLAIN
 * data pages back to back, by the rule arrow-cpp's writer applies with its
 * write_batch_size of 1024: rows are taken in batches of 1024 counted from
 * the row group's first row, a row adds 4 + its length to the open page, and
 * after a batch a page that has reached the limit closes if rows remain. So
 * a row group of R rows has at most ceil(R / 1024) pages, none empty, and
 * the cuts are a pure function of the rows: every route writes the same
 * file. The pages' bodies concatenated are the one-page image; chunk
 * statistics are unchanged, and there are no page-level statistics and no
 * page index. Under HX_CODEC_SNAPPY each page is compressed on its own, one
 * wave per page on the device routes. A row group that never reaches the
 * limit is written as under limit 0. HX_BYTES_PAGE_LIMIT_REFERENCE is the
 * reference writers' data page size. A value above 2^30 returns
 * HX_ERR_INVALID; a non-zero limit on a store with an f64 value column
 * returns HX_ERR_UNSUPPORTED. */
#define HX_BYTES_PAGE_LIMIT_REFERENCE (1u << 20)
#define HX_BYTES_PAGE_LIMIT_MAX (1u << 30)
hx_status hx_set_bytes_page_limit(hx_handle*, uint32_t bytes);

/* hx_write_sst_bytes_codec with a page limit (same range, HX_ERR_INVALID
 * outside it); limit 0 writes the file hx_write_sst_bytes_codec writes, byte
 * for byte. */
hx_status hx_write_sst_bytes_paged(const char* path, const uint64_t* series,
                                   const int64_t* ts, const uint8_t* bytes,
                                   const int64_t* offsets,
                                   const uint64_t* seqs, uint64_t seq,
                                   int64_t n_rows, int64_t row_group,
                                   int32_t codec, uint32_t page_limit);

/* ---- inverted index (RFC docs/rfcs/20240827-metric-engine.md:86-137) ----
 * The reference's planned index tables (its metric_engine index module is
 * an uncompiled skeleton; semantics pinned by the RFC): an `index` table
 * with rows (MetricID u64, TagKey bytes, TagValue bytes, TSID u64), stored
 * as Parquet SSTs under {store}/index/, rows sorted by
 * (tag_key, tag_value, tsid). A tag-equality predicate resolves to the
 * union of its postings across index SSTs; multiple predicates AND
 * (intersect) or OR (union). The resulting TSID set feeds the scan's
 * series-membership predicate (hx_scan_spec preds / hx_prepare series set),
 * closing the rfc "tag filter -> TSID -> data" query path on GPU. */
typedef struct {
    const char* tag_key;      /* NUL-terminated byte strings */
    const char* tag_value;
} hx_tag_pred;

/* Append one index SST (rows need not be pre-sorted; the writer sorts by
 * (tag_key, tag_value, tsid) — the RFC's index PK order). */
hx_status hx_index_write(hx_handle*, const uint64_t* metric_id,
                         const char* const* tag_keys,
                         const char* const* tag_values,
                         const uint64_t* tsids, int64_t n_rows,
                         uint64_t* out_seq);

/* Evaluate tag-equality predicates on `device`: GPU BYTE_ARRAY decode +
 * postings filter + set combine (AND = sorted intersection, OR = union).
 * Returns the sorted distinct TSID set (callee-allocated; free with
 * hx_tsids_free). */
hx_status hx_index_query(hx_handle*, const hx_tag_pred* preds, size_t n_preds,
                         int combine_and, int device, uint64_t** out_tsids,
                         size_t* n_out);
void hx_tsids_free(uint64_t* tsids);

/* ---- introspection for bench/tests ------------------------------------ */
typedef struct {
    double  exec_ms;          /* wall of last hx_exec_agg (HIP events)      */
    double  agg_kernel_ms;    /* k_scan_agg launch time (HIP events)        */
    double  decode_kernel_ms; /* delta/snappy decode kernels, if any        */
    int64_t rows_scanned;     /* rows examined (pre-filter)                 */
    int64_t rows_matched;     /* rows passing filter+dedup                  */
    int64_t bytes_staged;     /* page payload bytes resident in HBM         */
    double  stage_ms;         /* last hx_prepare wall (IO+parse+PCIe)       */
} hx_exec_stats;
hx_status hx_get_stats(hx_prepared*, hx_exec_stats* out);

/* What staging did with the prepared scan's Snappy data/dictionary pages
 * (summed over devices). A "stored" page — length preamble plus one literal
 * covering the whole page — is read in place from the staged blob; every
 * other Snappy page goes through the GPU decoder on each decode pass. All
 * zero for stores without Snappy pages. */
typedef struct {
    uint64_t pages_in_place;    /* stored pages read in place               */
    uint64_t pages_decoded;     /* pages handed to the GPU Snappy decoder   */
    uint64_t bytes_in_place;    /* uncompressed bytes of the in-place pages */
    uint64_t bytes_decoded_out; /* bytes the decoder writes per decode pass */
} hx_decode_stats;
hx_status hx_get_decode_stats(hx_prepared*, hx_decode_stats* out);

#ifdef __cplusplus
}
#endif
#endif /* HORAEDB_HX_H */
