// hx_internal.h — internals shared between engine.cpp and index.cpp
// (single shared library; not part of the public C-ABI).
#pragma once
#include <string>
#include "../../include/horaedb_hx.h"

namespace hx_int {

// route an error through engine.cpp's thread-local hx_last_error() buffer
hx_status set_error(hx_status code, const std::string& msg);

// the handle's store root directory
const std::string& store_path(hx_handle* h);

}  // namespace hx_int

// Test hook (exported, not part of the public C-ABI): run the production
// Snappy decode launch once over n caller-built streams on the current
// device. Stream i is streams[offs[i], offs[i] + comp_lens[i]); it is
// uploaded 64-byte aligned (as staging places page payloads) and decoded
// into uncomp_lens[i] bytes, which are copied back to out + out_offs[i].
// *n_errors receives the decoder's error count (streams it rejected; their
// output bytes are unspecified).
extern "C" hx_status hx_debug_snappy_decompress(
    const uint8_t* streams, const uint64_t* offs, const uint32_t* comp_lens,
    const uint32_t* uncomp_lens, uint32_t n, uint8_t* out,
    const uint64_t* out_offs, uint64_t* n_errors);

// Test hook (exported, not part of the public C-ABI, no GPU needed): stage
// one column chunk exactly as hx_prepare does — hx::read_chunk and
// hx::stage_chunk (stage_chunk.h), into a scratch slot of the reserved size,
// Overwrite mode — and return what staging used; a chunk staging refuses
// (nulls in a key column, ...) is refused here with the same message.
// column is one of series_id, timestamp, value, __seq__.
// bitmap_out (may be NULL) receives (n_rows + 63) / 64 LSB-first words;
// cap_words is its capacity. *level_bytes is the size of the level block in
// front of the page body (0 for a REQUIRED column).
extern "C" hx_status hx_debug_page_levels(
    const char* path, int32_t row_group, const char* column,
    uint64_t* bitmap_out, uint64_t cap_words, int64_t* n_rows,
    int64_t* n_valid, int32_t* level_bytes);

// Test hook (exported, not part of the public C-ABI): run the production
// launch of kernel 1d (hx::launch_pack_optional, hx_kernels.h) once over
// caller-built arrays on the current device. values: n_src 8-byte values.
// Validity over SOURCE rows, at most one of valid_words (one 0/1 word per
// row) and valid_bits (LSB-first bitmap, (n_src + 7) / 8 bytes); both NULL =
// all present. perm: n entries or NULL (identity). Outputs, row-group-major:
// packed_out n slots (row group g's present values from g * row_group; slots
// past its count are unspecified), bitmap_out ceil(n / row_group) *
// (row_group / 64) words, n_valid_out one count per row group. *n_errors
// receives the number of perm entries >= n_src (their rows come back null).
// Every device buffer is exactly as large as stated here.
extern "C" hx_status hx_debug_pack_optional(
    const uint64_t* values, const uint64_t* valid_words,
    const uint8_t* valid_bits, const uint32_t* perm, uint32_t n_src,
    uint32_t n, uint32_t row_group, uint64_t* packed_out,
    uint64_t* bitmap_out, uint32_t* n_valid_out, uint64_t* n_errors);

// Test hook (exported, not part of the public C-ABI, no GPU needed): the host
// twin of kernel 1e, hx::snappy_compress_host (snappy_compress.h). Returns
// the stream's size, 0 when cap is below Snappy's bound 32 + n + n / 6.
extern "C" uint64_t hx_debug_snappy_compress_host(const uint8_t* src,
                                                  uint64_t n, uint8_t* dst,
                                                  uint64_t cap);

// Test hook (exported, not part of the public C-ABI): run the production
// launches of kernel 1f (hx::launch_ba_page_sizes, then
// hx::launch_ba_build_pages; hx_kernels.h, contract in ba_pages.h) once over
// caller-built arrays on the current device. src: src_size bytes; handles:
// n_src words (off << 20 | len relative to src, in output order);
// group_start: n_out + 1 entries or NULL; row_group <= 8192. page_off
// receives ceil(n_out / row_group) + 1 entries, *n_errors the refused handles
// and group_start pairs, *n_over_cap the rows above 2^20 - 1 bytes. With out
// NULL only the size pass runs; otherwise out_cap must equal the last
// page_off entry, the image is built in a device buffer of exactly that size
// (pre-filled with 0xEE) and copied back whole, refused rows as empty values.
// Every device buffer is exactly as large as stated here.
// hx_debug_ba_pages_host is the same over the host twin, no GPU needed.
extern "C" hx_status hx_debug_ba_pages(
    const uint8_t* src, uint64_t src_size, const uint64_t* handles,
    uint32_t n_src, const uint32_t* group_start, uint32_t n_out,
    uint32_t row_group, uint64_t* page_off, uint8_t* out, uint64_t out_cap,
    uint64_t* n_errors, uint64_t* n_over_cap);
extern "C" hx_status hx_debug_ba_pages_host(
    const uint8_t* src, uint64_t src_size, const uint64_t* handles,
    uint32_t n_src, const uint32_t* group_start, uint32_t n_out,
    uint32_t row_group, uint64_t* page_off, uint8_t* out, uint64_t out_cap,
    uint64_t* n_errors, uint64_t* n_over_cap);

// Test hook (exported, not part of the public C-ABI): run the production
// launch of kernel 1e (hx::launch_snappy_compress, hx_kernels.h) once over
// n_pages caller-built pages on the current device. Page i is pages[offs[i],
// offs[i] + lens[i]); it is uploaded at a 64-byte-aligned device address plus
// src_align[i] (0..63). out_offs has n_pages + 1 ascending entries: page i's
// output slot is [out_offs[i], out_offs[i + 1]) of one device buffer of
// out_offs[n_pages] bytes, pre-filled with 0xEE and copied back whole into
// out. out_lens[i] receives the stream's size (0 for a refused page);
// *n_errors the number of pages whose slot was below 32 + n + n / 6. Every
// device buffer is exactly as large as stated here.
extern "C" hx_status hx_debug_snappy_compress(
    const uint8_t* pages, const uint64_t* offs, const uint32_t* lens,
    uint32_t n_pages, const uint32_t* src_align, uint8_t* out,
    const uint64_t* out_offs, uint32_t* out_lens, uint64_t* n_errors);

// Test hook (exported, not part of the public C-ABI): run the production
// launch of kernel 1g (hx::launch_ba_page_minmax, hx_kernels.h; rule and host
// twin in ba_pages.h) once over a caller-built image on the current device.
// image: page_off[n_pages] bytes, n_pages = ceil(n_out / row_group);
// page_off: n_pages + 1 ascending entries from 0; row_len: n_out words as the
// size pass leaves them (BA_ROW_SKIP = a refused row, an empty value), whose
// 4 + len per row must add up to each page's size, else HX_ERR_INVALID;
// row_group <= 8192. stats_out receives n_pages BaPageStat records of 140
// bytes {u32 has, min_len, max_len; u8 min[64]; u8 max[64]}, pre-filled with
// 0xEE on the device and copied back whole. Every device buffer is exactly as
// large as stated here. hx_debug_ba_page_minmax_host is the same over the
// host twin, no GPU needed.
extern "C" hx_status hx_debug_ba_page_minmax(
    const uint8_t* image, const uint64_t* page_off, const uint32_t* row_len,
    uint32_t n_out, uint32_t row_group, uint8_t* stats_out);
extern "C" hx_status hx_debug_ba_page_minmax_host(
    const uint8_t* image, const uint64_t* page_off, const uint32_t* row_len,
    uint32_t n_out, uint32_t row_group, uint8_t* stats_out);

// Debug: run kernel 1h (k_ba_batch_sizes; hx::ba_batch_sizes_host is its twin
// in ba_pages.h) once over caller-built row_len on the current device, by the
// production launch. row_len: n_out words as the size pass leaves them;
// row_group <= 8192; batch_sum receives hx::ba_n_batches(n_out, row_group)
// words: (ceil(n_out / row_group) - 1) * ceil(row_group / 1024) for the full
// row groups plus ceil(rows of the last / 1024). The device output is
// pre-filled with 0xEE and copied back whole. Every device buffer is exactly
// as large as stated here. hx_debug_ba_batch_sizes_host is the same over the
// host twin, no GPU needed.
extern "C" hx_status hx_debug_ba_batch_sizes(const uint32_t* row_len,
                                             uint32_t n_out,
                                             uint32_t row_group,
                                             uint64_t* batch_sum);
extern "C" hx_status hx_debug_ba_batch_sizes_host(const uint32_t* row_len,
                                                  uint32_t n_out,
                                                  uint32_t row_group,
                                                  uint64_t* batch_sum);
