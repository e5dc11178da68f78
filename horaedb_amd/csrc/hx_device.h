// hx_device.h — structures shared between the host engine and the gfx950
// kernels. All offsets are byte offsets; bit 63 of an
// offset selects the decode blob (dec) over the staged page blob (blob).
#pragma once
#include <cstdint>

namespace hx {

// aggregate op bits (must mirror HX_AGG_* in include/horaedb_hx.h)
enum : uint32_t { HXK_SUM = 1u, HXK_COUNT = 2u, HXK_MIN = 4u, HXK_MAX = 8u,
                  HXK_AVG = 16u };

constexpr uint64_t OFF_DEC = 1ull << 63;   // offset lives in decode blob
constexpr uint64_t OFF_MASK = OFF_DEC - 1;

// One (SST, row group) unit: the fused kernel's workgroup granule.
// Row groups of one SST are staged in ascending row order; next_rg gives the
// SAME SST's next staged row group (for the adjacent-dedup boundary row),
// -1 if none. Grid order of rgs is a speed-only choice (host interleaves by
// row ordinal across SSTs for L3 locality of the group table).
struct RgDesc {
    uint64_t series_off;
    uint64_t ts_off;
    uint64_t val_off;
    uint32_t n_rows;
    uint32_t sst_id;
    int64_t  row_base;     // staged-row index base within the SST (dense)
    int32_t  next_rg;      // index into rg array, -1 = last staged rg of sst
    int32_t  _pad;
};

// Validity of a unit's value column, parallel to the RgDesc array (same
// index) and present only in plans that staged a null: the n_rgs entries sit
// in the same device allocation right behind the n_rgs RgDesc
// ((const RgValid*)(rgs + n_rgs)). Neither RgDesc nor AggParams changed for
// it, so plans without nulls launch the kernel code they launched before.
struct RgValid {
    uint64_t off;          // blob byte offset of the bitmap (LSB-first u64
                           // words, 1 = value present); 0 = no bitmap, every
                           // row of the unit has a value
    uint64_t bit;          // bit of the unit's row 0 within that bitmap
};

// Per-SST device info. overlap==1 => this SST belongs to a ts-overlap
// cluster: rows must check higher-seq SSTs of the cluster for
// equal PKs via binary search over their dense (series, ts) arrays.
struct SstDev {
    int32_t  cluster;        // overlap-cluster id, -1 = none
    int32_t  rank;           // seq rank within cluster (ascending), dense
    uint64_t dense_series;   // byte offset (dec blob) of staged series array
    uint64_t dense_ts;       // byte offset (dec blob) of staged ts array
    int64_t  n_staged;       // staged rows (dense array length)
    // per-row sequences (keep_builtin compaction outputs,
    // executor.rs:155-222): a file whose __seq__ column is NOT constant
    // carries dense_seq (staged per-row seqs); 0 = constant (seq below).
    uint64_t seq;            // the file sequence (constant-seq files)
    uint64_t dense_seq;      // byte offset (dec blob) of per-row seqs, or 0
};

// Overlap cluster: member SSTs sorted by ascending seq; members[] indexes
// the SstDev array. Flattened: cluster c owns members[first..first+n).
struct ClusterDev {
    int32_t first;
    int32_t n;
};

// Aggregate hash table: open addressing, linear probe, one slab of
// fixed-stride slots (probe + update touch one cache line). Two slot forms:
//   key-claim (AggParams::key_claim): {key, sum, cnt[, min, max]}, stride
//     32/64; key == KEY_EMPTY marks a free slot, claimed by one CAS.
//   state-word: {state u32, pad, series, bucket, sum, cnt[, min, max]},
//     stride 48/64; state: 0 empty, 1 claim in flight, 2 ready (key words
//     valid).
// min/max are f64_ordered u64 words (IEEE 754 totalOrder, bits kept).
struct AggTable {
    uint32_t  mask;            // slots-1 (power of two)
    uint8_t*  slab;
    uint32_t  stride;
};

struct AggParams {
    const RgDesc* rgs;
    uint32_t n_rgs;
    const SstDev* ssts;
    const ClusterDev* clusters;
    const int32_t* cluster_members;
    const uint8_t* blob;
    const uint8_t* dec;
    int64_t ts_lo, ts_hi;          // [lo, hi)
    // optional series-membership set (open hash, EMPTY sentinel chosen by host)
    const uint64_t* sset;
    uint32_t sset_mask;
    uint64_t sset_empty;
    int32_t use_sset;
    int64_t bucket_ms;             // 0 = group by series only
    uint32_t ops;                  // HX_AGG_* mask
    int32_t key_claim;             // 1 = one-CAS key-claim mode (no state word)
    int32_t keep_dups;             // 1 = Append: no dedup, every filtered row survives
    AggTable table;
    // direct-indexed bucket mode (bucket_ms > 0, key-claim safe, bucket
    // range known from the scan range): table keyed by series only; each
    // slot owns a dense [n_buckets] accumulator row in bstore.
    int64_t lo_bucket;
    uint32_t n_buckets;            // 0 => generic state-word path
    uint32_t bstride;              // 16 {sum,cnt} or 32 {+min,max}
    uint8_t* bstore;
    // global-table bookkeeping: used by k_scan_agg only (the range kernel
    // never touches the table)
    unsigned long long fill_limit; // early-abort when fill exceeds this
    unsigned long long* fill;      // claimed slots
    unsigned long long* overflow;  // !=0 => rerun with a larger table
    unsigned long long* matched;   // rows surviving filter+dedup
};

// Series-range partitioned aggregation (k_scan_agg_range2): the
// series space is split at equal-sample quantile boundaries; block b owns
// series in [bounds[b], bounds[b+1]) across ALL SSTs, accumulating into an
// LDS table that leaves the block once, as a sorted run (RangeOut) — no
// global-table RMWs at all. Row bounds per (block, sst) are precomputed by
// k_range_bounds (64-ary parallel lower_bound) and cached.
struct RangeAux {
    const uint64_t* bounds;      // n_blocks+1 ascending series boundaries
    const uint64_t* bound_rows;  // (n_blocks+1) x n_ssts packed (pos<<32|row)
    const int32_t* sst_rgs;      // rg-desc indices grouped per SST, row order
    const int32_t* sst_rg_off;   // per SST: offset into sst_rgs
    const int32_t* sst_rg_cnt;   // per SST: count
    uint32_t n_ssts;
    uint32_t n_blocks;
    // LDS table slots (power of two). A key's first probe is its fractional
    // position (s-lo)*ne/(hi-lo) within the block's series range — ascending rows
    // probe ascending slots, so the wave's DS accesses land on consecutive
    // banks (conflict-free) instead of random ones, and collisions stay rare
    // (series values are hashes, ~uniform in value).
    uint32_t ne;
};

// Sorted-run output of k_scan_agg_range2: block b orders its LDS
// entries by key and writes them as one contiguous run into SoA staging at
// an offset reserved from `cursor` (one agent-scope add per block); desc[b]
// = count << 32 | offset. Blocks own disjoint ascending key ranges, so placing
// the runs in blk order (RangePlace) yields the sorted result — no global
// table, compaction or sort.
struct RangeOut {
    uint64_t* key;                 // staging columns, `cap` entries each
    double* sum;
    unsigned long long* cnt;
    double* vmin;                  // MM instance only
    double* vmax;
    uint64_t* desc;                // n_blocks x (count << 32 | offset)
    unsigned long long cap;        // staging capacity (entries, < 2^32)
    unsigned long long* cursor;    // total entries reserved == group count
    unsigned long long* stage_ovf; // != 0: a run did not fit `cap`
    unsigned long long* block_ovf; // != 0: a block met more than ne keys
};

// Placement of the staged runs into the contiguous SoA result (column c of
// the result starts at dst + c * total, total = *cursor). A column index of
// -1 means "not requested".
struct RangePlace {
    const uint64_t* desc;          // count << 32 | offset
    uint32_t* prefix;              // n_blocks exclusive prefix of the counts
    uint32_t n_blocks;
    const uint64_t* key;
    const double* sum;
    const unsigned long long* cnt;
    const double* vmin;
    const double* vmax;
    unsigned long long* dst;       // column 0 = series
    int32_t c_sum, c_cnt, c_min, c_max, c_avg;
    unsigned long long cap;
    const unsigned long long* cursor;
    const unsigned long long* stage_ovf;
    const unsigned long long* block_ovf;
};

// First/last resolve (k_resolve_first_last, DESIGN §4 kernel 3d): the sorted
// groups of the TS pass with their time extrema; a side that was not asked
// has null tmin/ofirst (tmax/olast). Outputs are f64_ordered words,
// zero-filled by the caller.
struct ResolveParams {
    const uint64_t* gkey;          // ng series ids, sorted by (series, bucket)
    const long long* gbucket;      // ng bucket indices, null: series-only
    const long long* tmin;         // ng smallest surviving non-null ts
    const long long* tmax;         // ng greatest
    unsigned long long* ofirst;    // ng
    unsigned long long* olast;     // ng
    uint32_t ng;
    unsigned long long* err;       // rows that found no group (must stay 0)
};

// DELTA_BINARY_PACKED decode unit: one page -> dense i64 at dst_off (dec).
struct DeltaPageDesc {
    uint64_t src_off;     // page payload (bit63: in dec blob, e.g. post-snappy)
    uint64_t dst_off;     // dec blob byte offset for n_values i64
    uint32_t n_values;
    uint32_t src_len;
};

// RLE_DICTIONARY decode unit: one data page + its dictionary page ->
// dense 8-byte values at dst_off (dec). Indices are the Parquet RLE/
// bit-packed hybrid; dictionary is PLAIN 8-byte values.
struct RleDictPageDesc {
    uint64_t dict_off;    // PLAIN dictionary payload (bit63: dec blob)
    uint64_t idx_off;     // data page payload (starts with bit-width byte)
    uint64_t dst_off;     // dec blob
    uint32_t dict_n;
    uint32_t idx_len;
    uint32_t n_values;
    uint32_t _pad;
};

// Snappy decompress unit: one page.
struct SnappyPageDesc {
    uint64_t src_off;     // blob
    uint64_t dst_off;     // dec blob
    uint32_t comp_len;
    uint32_t uncomp_len;
};

// Snappy compress unit (k_snappy_compress, DESIGN §4 kernel 1e): one page of
// n bytes at src + src_off (any byte alignment) into the output slot
// [dst + dst_off, + dst_cap); a slot below 32 + n + n / 6 is refused.
struct SnappyCompDesc {
    uint64_t src_off;
    uint64_t dst_off;
    uint32_t n;
    uint32_t dst_cap;
};

// Statistics of one page of 8-byte values (k_page_minmax), as the Parquet
// writer puts them into the footer. kind: the column's order.
enum : uint32_t { PAGE_ORDER_U64 = 0, PAGE_ORDER_I64 = 1, PAGE_ORDER_F64 = 2 };
struct PageStat {
    uint64_t min_bits;
    uint64_t max_bits;
    uint64_t has;         // 0: no value enters the bounds (f64: NaN only)
};

// OPTIONAL-column PLAIN page unit (k_expand_optional, DESIGN §4 kernel 1c).
// The page's n_valid packed 8-byte values start at src + lvl_bytes: a v1
// page the Snappy decoder wrote to dec opens with its definition-level block
// (lvl_bytes = its size, in general not a multiple of 8); every other page
// was staged without the block (lvl_bytes = 0). The kernel writes a dense
// n_rows column at dst_off: without a bitmap n_valid == n_rows and it is a
// realigning copy; with one, row r takes packed[rank(r)] if its bit is set
// and 0 otherwise.
struct ExpandPageDesc {
    uint64_t src_off;     // page bytes (bit63: dec blob), 8-byte aligned
    uint64_t dst_off;     // dec blob, 64-byte aligned, n_rows * 8 bytes
    uint64_t bitmap_off;  // blob: (n_rows + 63) / 64 LSB-first words; 0 = none
    uint32_t src_len;     // bytes at src: lvl_bytes + n_valid * 8 must fit
    uint32_t lvl_bytes;
    uint32_t n_rows;
    uint32_t n_valid;
};

// Plain copy unit (materialize dense arrays for the overlap path).
struct CopyDesc {
    uint64_t src_off;
    uint64_t dst_off;
    uint32_t n_values;    // 8-byte values
    uint32_t _pad;
};

// ---- inverted-index query units (rfc:86-137 index table) ------------------
// One PLAIN BYTE_ARRAY page (u32 length + bytes per value): walked into a
// packed (offset << 20 | len) per row at out[first_row..first_row+n).
struct BaPageDesc {
    uint64_t src_off;     // page payload offset in the index blob
    uint64_t src_len;
    uint32_t n_values;
    uint32_t _pad;
    int64_t first_row;    // global row index of this page's first value
};

// Tag-equality filter over decoded (key, value) offset arrays + tsid column.
struct TagFilterParams {
    const uint8_t* blob;          // index page blob
    const uint64_t* key_offlen;   // packed per-row (off << 20 | len)
    const uint64_t* val_offlen;
    const uint64_t* tsid;         // dense per-row tsids
    int64_t n_rows;
    const uint8_t* pred_key;      // predicate bytes (device)
    uint32_t pred_key_len;
    uint32_t pred_val_len;
    const uint8_t* pred_val;
    uint64_t* out;                // matching tsids (unordered)
    unsigned long long* cursor;
    unsigned long long cap;
};

}  // namespace hx
