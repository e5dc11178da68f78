// stage_chunk.h — the host half of staging, free of any GPU
// header so it builds and runs under the host sanitizers (stage_check.cpp):
// one column chunk -> its bytes in the page blob plus the decode descriptors
// the kernels consume, and the pure RgDesc work that follows the page walk.
// engine.cpp lays the slots out, runs stage_chunk on its worker threads and
// uploads the result.
#pragma once
#include <atomic>
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/horaedb_hx.h"
#include "hx_device.h"
#include "parquet_meta.h"

namespace hx {

inline size_t align64(size_t x) { return (x + 63) & ~size_t(63); }

// What the catalog (the file's footer) says about one column chunk.
struct ChunkRef {
    int32_t codec = 0;
    bool required = true;
    int64_t chunk_start = 0;
    int64_t comp_size = 0;
    int64_t uncomp_size = 0;
    int64_t num_values = 0;
};

// Slot-capacity rule, read by the layout pass and by stage_chunk alike: a
// chunk's slot holds its bytes as stored; a Zstd chunk is decompressed in
// place on the host, so it gets the larger of the stored and the declared
// decompressed size; a Snappy chunk gets 64 more bytes so a stored-literal
// page can be shifted (pad <= 63) until its body is 64-byte aligned.
// stage_chunk never writes outside [0, chunk_reserve) of its slot.
inline size_t chunk_reserve(const ChunkRef& c) {
    size_t r = size_t(c.comp_size);
    if (c.codec == CODEC_ZSTD && c.uncomp_size > c.comp_size)
        r = size_t(c.uncomp_size);
    if (c.codec == CODEC_SNAPPY) r += 64;
    return r;
}

// Validity words reserved for the chunk: the f64 value column (col 2) of a
// file that declares it OPTIONAL gets one bit per row; nothing else does.
inline size_t bitmap_reserve(const ChunkRef& c, int col, bool bytes_value) {
    if (col != 2 || c.required || bytes_value || c.num_values <= 0) return 0;
    return (size_t(c.num_values) + 63) / 64 * 8;
}

// Where one chunk goes. base[0, cap) is its slot and starts at blob offset
// `off` (64-byte aligned); bitmap[0, bitmap_cap) likewise at bitmap_off, or
// null when no words were reserved (the levels are then only counted).
struct ChunkSlot {
    uint8_t* base = nullptr;
    uint64_t off = 0;
    size_t cap = 0;
    uint64_t* bitmap = nullptr;
    uint64_t bitmap_off = 0;
    size_t bitmap_cap = 0;
};

// What the chunk is staged for.
struct ChunkRole {
    int col = 0;               // 0 series_id, 1 timestamp, 2 value, 3 __seq__
    bool bytes_value = false;  // the store's value column is BYTE_ARRAY
    int32_t update_mode = 0;   // 0 Overwrite / 1 Append
    int64_t row_base = 0;      // staged rows of the SST before this row group
    uint64_t bytes_handles = 0;  // dec offset of the SST's value-handle array
};

// Decode work of the chunks one caller staged. Each staging thread owns one
// and the plan takes their concatenation: the decode kernels give every
// descriptor its own wave or workgroup, so their order carries no meaning.
struct StagedPages {
    std::vector<SnappyPageDesc> snappy;
    std::vector<ExpandPageDesc> expand;
    std::vector<DeltaPageDesc> delta;
    std::vector<RleDictPageDesc> rledict;
    std::vector<BaPageDesc> ba;
    // Snappy pages of a Binary value column: decoded into the blob's tail
    // (dst_off counts from the blob's base, no OFF_DEC), DESIGN §3
    std::vector<SnappyPageDesc> snappy_ba;
    uint64_t pages_in_place = 0;  // stored Snappy pages read from the blob
    uint64_t bytes_in_place = 0;
};

// What the plan keeps of one staged chunk. For the BYTE_ARRAY value chunk of
// a Binary store, which may hold several data pages: n_valid is the chunk's
// value count, level_bytes and raw_size are sums over its pages, stored says
// that every page is a stored Snappy page.
struct ChunkResult {
    uint64_t final_off = 0;   // RgDesc column offset (blob, or OFF_DEC | dec)
    bool has_nulls = false;   // the page holds nulls: its validity words
    uint64_t valid_off = 0;   // are live, at this blob offset (else 0)
    uint32_t n_valid = 0;     // present values
    uint32_t level_bytes = 0; // level block in front of the page body
    bool stored = false;      // stored Snappy page, read in place
    uint64_t raw_size = 0;    // body bytes after the host codec step
};

struct StageStatus {
    hx_status st = HX_OK;
    std::string msg;  // empty = success; the caller adds the file path
    bool ok() const { return msg.empty(); }
};

// Check the catalog's size for the chunk and read it. The message names path.
StageStatus read_chunk(int fd, const std::string& path, const ChunkRef& cr,
                       std::vector<uint8_t>& buf);

// Stage one column chunk (buf = its cr.comp_size bytes as stored): walk its
// pages, run the host codec step, place the bytes in the slot, reserve dec
// space (dec bumps by align64 of what each descriptor will write) and append
// the descriptors. Every write into the slot is bounded by slot.cap, which
// the caller sets to chunk_reserve(cr); a page that needs more is refused.
// tail: the cursor of the blob's decoded tail, an offset from the blob's base
// that starts at the 64-aligned end of the slots. A Snappy page of a Binary
// value column that is no stored literal reserves align64(uncomp_len) there
// and is decoded to that place, so its handles stay relative to the blob;
// without a cursor such a page is refused.
// The 8-byte columns hold exactly one data page per chunk (plus at most one
// dictionary page). The BYTE_ARRAY value chunk of a Binary store
// (role.bytes_value && role.col == 2) may hold any number: each page is
// staged by the same rules into the chunk's one slot at cumulative offsets
// (chunk_reserve covers them: a later page starts 8-aligned, paid for by its
// header) and gets a BaPageDesc of its own, first_row advanced by the rows
// of the pages before it; a tail page gets its own SnappyPageDesc. Page
// value counts that do not add up to cr.num_values are HX_ERR_FORMAT, a page
// of zero values is skipped, a null in any page refuses the chunk, and the
// tail pages' cumulative claim is checked against cr.uncomp_size before
// anything is reserved or appended.
StageStatus stage_chunk(const uint8_t* buf, const ChunkRef& cr,
                        const ChunkRole& role, const ChunkSlot& slot,
                        std::atomic<size_t>& dec, StagedPages& pages,
                        ChunkResult& res,
                        std::atomic<size_t>* tail = nullptr);

// Fill the RgDesc column offsets from the chunk results (results holds, rg by
// rg in rgs order, one entry per staged column: 4 for SSTs with dense_seq,
// else 3), set rg_valid, and emit the dense-array copies of overlap-cluster
// members.
void patch_rg_offsets(std::vector<RgDesc>& rgs, std::vector<RgValid>& rg_valid,
                      const std::vector<SstDev>& ssts,
                      const std::vector<ChunkResult>& results,
                      std::vector<CopyDesc>& copies);

// Per-SST unit lists in row order (RangeAux).
struct SstRgLists {
    std::vector<int32_t> rgs, off, cnt;
};

// Cut every row group into `split` slices (>= 1024 rows each), order the
// units by fractional row position within their SST, remap next_rg, and
// build the per-SST lists. rg_valid stays parallel to rgs.
void slice_and_order(std::vector<RgDesc>& rgs, std::vector<RgValid>& rg_valid,
                     size_t n_ssts, uint32_t split, SstRgLists& lists);

}  // namespace hx
