// hx_kernels.h — host-side launcher API implemented in kernels.hip (keeps
// device code in one TU; no -fgpu-rdc needed).
#pragma once
#include <hip/hip_runtime.h>
#include "ba_pages.h"
#include "hx_device.h"

namespace hx {

struct CompactOut {
    uint64_t* series;
    long long* bucket;
    double* sum;
    unsigned long long* cnt;
    double* vmin;
    double* vmax;
    unsigned long long* n_out;
};

hipError_t launch_decode_delta(hipStream_t s, const uint8_t* blob, uint8_t* dec,
                               const DeltaPageDesc* pages, uint32_t n_pages,
                               unsigned long long* err_flag);
hipError_t launch_rledict(hipStream_t s, const uint8_t* blob, uint8_t* dec,
                          const RleDictPageDesc* pages, uint32_t n_pages,
                          unsigned long long* err_flag);
hipError_t launch_snappy(hipStream_t s, const uint8_t* blob, uint8_t* dec,
                         const SnappyPageDesc* pages, uint32_t n_pages,
                         unsigned long long* err_flag);
// One workgroup per page; a page whose descriptor does not fit its source
// (lvl_bytes + n_rows * 8 > src_len) is left unwritten and counted in
// err_flag.
hipError_t launch_expand_optional(hipStream_t s, const uint8_t* blob,
                                  uint8_t* dec, const ExpandPageDesc* pages,
                                  uint32_t n_pages,
                                  unsigned long long* err_flag);
// Kernel 1d, one workgroup per output row group of row_group rows (a multiple
// of 64, else hipErrorInvalidValue): output row i of n is source row perm[i]
// (i when perm is null) of n_src. valid_src: one 0/1 u64 per source row, or
// (valid_bits) an LSB-first bitmap of ceil(n_src / 8) bytes; null = all
// present. Writes, row-group-major: bitmap_out[g * (row_group / 64) ...]
// (every word of every row group, n_groups * row_group / 64 in all),
// packed_out[g * row_group ...] (n slots in all), n_valid[g]. A perm entry
// >= n_src is counted in err_flag and its row written as null.
hipError_t launch_pack_optional(hipStream_t s,
                                const unsigned long long* val_src,
                                const void* valid_src, bool valid_bits,
                                const uint32_t* perm, uint32_t n_src,
                                uint32_t n, uint32_t row_group,
                                unsigned long long* packed_out,
                                uint64_t* bitmap_out, uint32_t* n_valid,
                                unsigned long long* err_flag);
// Kernel 1e, one wave per page: the Snappy stream of src[src_off, + n) goes to
// dst[dst_off, ...) and its size to out_len[page]; the bytes are those of
// hx::snappy_compress_host. A page whose dst_cap is below 32 + n + n / 6 is
// counted in err_flag, gets out_len 0 and its slot is not written.
hipError_t launch_snappy_compress(hipStream_t s, const uint8_t* src,
                                  uint8_t* dst, const SnappyCompDesc* pages,
                                  uint32_t n_pages, uint32_t* out_len,
                                  unsigned long long* err_flag);
// Behind it: an exclusive scan of out_len into offs (n_pages words of device
// scratch), then stream i moves from its slot to packed + offs[i], so one
// copy of sum(out_len) bytes brings every stream to the host.
hipError_t launch_snappy_pack(hipStream_t s, const uint8_t* slots,
                              const SnappyCompDesc* pages, uint32_t n_pages,
                              const uint32_t* out_len,
                              unsigned long long* offs, uint8_t* packed);
// Footer statistics of the same pages (src_off a multiple of 8, n / 8
// values each), one wave per page: min and max in the order kinds[page]
// names. PAGE_ORDER_F64 follows the writer's DOUBLE rules: NaN never enters,
// a zero bound comes out as min -0.0 / max +0.0, has = 0 without a non-NaN
// value.
hipError_t launch_page_minmax(hipStream_t s, const uint8_t* src,
                              const SnappyCompDesc* pages,
                              const uint32_t* kinds, uint32_t n_pages,
                              PageStat* out);
hipError_t launch_copy_u64(hipStream_t s, const uint8_t* blob, uint8_t* dec,
                           const CopyDesc* descs, uint32_t n_descs);
// nulls: the plan staged a validity bitmap — launch the null-aware instance.
// ts: the TS instance (first/last): min/max run over the rows'
// timestamps instead of their values; p.ops must ask for MIN or MAX.
hipError_t launch_scan_agg(hipStream_t s, const AggParams& p, uint32_t grid,
                           bool nulls = false, bool ts = false);
// Series-range mode: sample series for quantile boundaries,
// precompute per-(block,sst) row bounds, then the LDS-table range kernel
// (k_scan_agg_range2; the name is kept so the profiles/ records match).
hipError_t launch_sample_series(hipStream_t s, const RgDesc* rgs,
                                uint32_t n_rgs, const uint8_t* blob,
                                const uint8_t* dec, uint64_t* out);
hipError_t launch_range_bounds(hipStream_t s, const AggParams& p,
                               const RangeAux& r, uint64_t* out);
// Each block emits its groups as one key-ordered run into `out` (p.table is
// not used); launch_place_runs then assembles the result.
hipError_t launch_scan_agg_range2(hipStream_t s, const AggParams& p,
                                  const RangeAux& r, bool minmax,
                                  bool nulls, const RangeOut& out,
                                  bool ts = false);
// Exclusive scan of the run counts in blk order, then one copy of every run
// to its final position in the contiguous SoA result (avg computed here).
hipError_t launch_place_runs(hipStream_t s, const RangePlace& q);
// Kernel 3d: p carries the filter, dedup and bucket_ms of the aggregate; the
// caller zero-fills q.ofirst / q.olast on the same stream first.
hipError_t launch_resolve_first_last(hipStream_t s, const AggParams& p,
                                     const ResolveParams& q, bool nulls);
// In place, n words. to_ts: min/max columns of a TS pass (written through
// ordered_f64) -> i64 timestamps; else ordered value words -> f64 bits.
hipError_t launch_map_words(hipStream_t s, unsigned long long* w, size_t n,
                            bool to_ts);
hipError_t launch_scan_rows(hipStream_t s, const AggParams& p,
                            uint32_t rg_first, uint32_t rg_last,
                            uint64_t* out_series, long long* out_ts,
                            double* out_value, unsigned long long* cursor,
                            unsigned long long cap,
                            uint64_t* out_seq = nullptr,
                            int32_t seq_rowidx = 0,
                            uint64_t* out_valid = nullptr);
hipError_t launch_gather_multi(hipStream_t s,
                               const unsigned long long* const* srcs,
                               uint32_t n_arrays, const uint32_t* perm,
                               unsigned long long* dst, uint32_t n);
// Live slots -> dense unsorted arrays. n_buckets == 0: two-phase (count,
// scan, write) using scratch, a device buffer of 2*2048 u32 (per-block
// counts + bases). n_buckets > 0: single-pass sweep, scratch unused.
hipError_t launch_compact(hipStream_t s, const AggTable& t, uint32_t n_slots,
                          int32_t key_claim, int64_t bucket_ms,
                          int64_t lo_bucket, uint32_t n_buckets,
                          uint32_t bstride, const uint8_t* bstore,
                          const CompactOut& o, uint32_t* scratch);
hipError_t launch_gather_u64(hipStream_t s, const unsigned long long* in,
                             const uint32_t* perm, unsigned long long* out,
                             uint32_t n);
hipError_t launch_avg(hipStream_t s, const double* sum,
                      const unsigned long long* cnt, double* avg, uint32_t n);
hipError_t launch_iota(hipStream_t s, uint32_t* out, uint32_t n);
hipError_t launch_init_slab(hipStream_t s, uint8_t* slab, uint32_t n_slots,
                            uint32_t stride);
// direct-indexed bucket store: total_rows accumulator rows of {sum, cnt
// [, min, max]} (stride 16/32)
hipError_t launch_init_accum_rows(hipStream_t s, uint8_t* rows,
                                  size_t total_rows, uint32_t stride, bool mm);
hipError_t launch_init_state_slab(hipStream_t s, uint8_t* slab,
                                  uint32_t n_slots, uint32_t stride, bool mm);
hipError_t launch_seg_keys(hipStream_t s, const long long* ts, long long seg_ms,
                           unsigned long long* keys, uint32_t n);
hipError_t launch_xor_sign(hipStream_t s, unsigned long long* buf, uint32_t n);

// inverted-index query kernels (rfc:86-137)
hipError_t launch_ba_offsets(hipStream_t s, const uint8_t* blob,
                             const BaPageDesc* pages, uint32_t n_pages,
                             uint64_t* out, unsigned long long* err_flag);
hipError_t launch_tag_filter(hipStream_t s, const TagFilterParams& f);
hipError_t launch_copy_bytes(hipStream_t s, const uint8_t* blob,
                             const uint64_t* handles, const int64_t* dst_off,
                             uint8_t* out, uint32_t n);
// Kernel 1f (ba_pages.h states the contract and is its host twin): PLAIN
// BYTE_ARRAY page images from per-row handles (off << 20 | len relative to
// src, in output order), output row groups of row_group <= 8192 rows, else
// hipErrorInvalidValue. group_start: n_out + 1 entries or null.
// launch_ba_page_sizes writes row_len[n_out], page_size[n_pages] and the
// exclusive scan page_off[n_pages + 1], and adds to counts[0] (bad handles
// and group_start pairs) and counts[1] (rows above BA_MAX_VALUE_LEN).
// launch_ba_build_pages then writes the image, page_off[n_pages] bytes.
hipError_t launch_ba_page_sizes(hipStream_t s, uint64_t src_size,
                                const uint64_t* handles,
                                const uint32_t* group_start, uint32_t n_src,
                                uint32_t n_out, uint32_t row_group,
                                uint32_t* row_len,
                                unsigned long long* page_size,
                                unsigned long long* page_off,
                                unsigned long long* counts);
hipError_t launch_ba_build_pages(hipStream_t s, const uint8_t* src,
                                 uint64_t src_size, const uint64_t* handles,
                                 const uint32_t* group_start, uint32_t n_src,
                                 uint32_t n_out, uint32_t row_group,
                                 const uint32_t* row_len,
                                 const unsigned long long* page_off,
                                 uint8_t* out);
// Kernel 1h, one wave per 1024-row batch of every row group: batch_sum gets
// hx::ba_n_batches(n_out, row_group) byte sums over row_len[n_out] as the
// size pass left it (hx::ba_batch_sizes_host is the twin).
hipError_t launch_ba_batch_sizes(hipStream_t s, const uint32_t* row_len,
                                 uint32_t n_out, uint32_t row_group,
                                 unsigned long long* batch_sum);
// Kernel 1g, one workgroup per page of the image kernel 1f built (page_off
// and row_len as its size pass left them): the chunk's footer statistics by
// ba_pages.h's 65-byte rule, the bytes of hx::ba_page_minmax_host. out: one
// BaPageStat per page.
hipError_t launch_ba_page_minmax(hipStream_t s, const uint8_t* image,
                                 const unsigned long long* page_off,
                                 const uint32_t* row_len, uint32_t n_out,
                                 uint32_t row_group, BaPageStat* out);
// Equal-PK runs of n sorted rows (n > 0): flag and rank are n words of
// scratch; group_start gets n_out + 1 entries (room for n + 1), the head
// columns one entry per run, *n_out the run count. seq_key (may be null):
// the UNSORTED rows' (seq << 32 | file row) keys, read through perm; a run's
// head_seq is the sequence of its first row.
hipError_t launch_group_heads(hipStream_t s, const unsigned long long* series,
                              const unsigned long long* ts,
                              const unsigned long long* seq_key,
                              const uint32_t* perm, uint32_t n,
                              uint32_t* flag, uint32_t* rank,
                              uint32_t* group_start,
                              unsigned long long* head_series,
                              unsigned long long* head_ts,
                              unsigned long long* head_seq,
                              unsigned long long* n_out, void** d_temp,
                              size_t* temp_bytes);
hipError_t launch_tsid_intersect(hipStream_t s, const uint64_t* a,
                                 unsigned long long n_a, const uint64_t* b,
                                 unsigned long long n_b, uint64_t* out,
                                 unsigned long long* cursor);
hipError_t launch_unique_u64(hipStream_t s, const uint64_t* in,
                             unsigned long long n, uint64_t* out,
                             unsigned long long* cursor);
hipError_t sort_keys_u64(hipStream_t s, const uint64_t* keys_in,
                         uint64_t* keys_out, size_t n, void** d_temp,
                         size_t* temp_bytes);

// rocPRIM stable LSD radix sort: sorts values (u32 perm) by u64 keys.
// temp buffer managed internally on the stream (hipMallocAsync-free impl).
hipError_t sort_pairs_u64(hipStream_t s, const uint64_t* keys_in,
                          uint64_t* keys_out, const uint32_t* vals_in,
                          uint32_t* vals_out, size_t n, void** d_temp,
                          size_t* temp_bytes);

}  // namespace hx
