// stage_chunk.cpp — see stage_chunk.h. Host-only: plain C++17, libdl.
#include "stage_chunk.h"

#include <algorithm>
#include <cstring>
#include <dlfcn.h>
#include <stdexcept>
#include <unistd.h>

#include "def_levels.h"
#include "parquet_meta.h"
#include "snappy_stored.h"

namespace hx {
namespace {

// ---------------------------------------------------------------------------
// Zstd page codec (config.rs:84 includes Zstd): decompressed on the HOST at
// staging time into the page blob — the same place SURVEY §7 allows for
// inherently serial codecs — so the kernels see raw PLAIN pages. The image
// carries libzstd.so.1 without a dev header; dlopen with self-declared
// prototypes (stable ZSTD_* ABI). Fails loudly when the library is absent.
// ---------------------------------------------------------------------------
typedef size_t (*zstd_decompress_fn)(void*, size_t, const void*, size_t);
typedef unsigned (*zstd_iserror_fn)(size_t);

struct ZstdLib {
    zstd_decompress_fn decompress = nullptr;
    zstd_iserror_fn is_error = nullptr;
    bool ok = false;
    ZstdLib() {
        void* h = dlopen("libzstd.so.1", RTLD_NOW | RTLD_LOCAL);
        if (!h) return;
        decompress = (zstd_decompress_fn)dlsym(h, "ZSTD_decompress");
        is_error = (zstd_iserror_fn)dlsym(h, "ZSTD_isError");
        ok = decompress && is_error;
    }
};

const ZstdLib& zstd() {
    static ZstdLib z;
    return z;
}

StageStatus bad(hx_status st, std::string msg) { return {st, std::move(msg)}; }

const char* const kTooLarge = "page larger than its chunk's declared size";

// The two writers of chunk bytes into a slot; both refuse what does not fit
// [at, at + n) inside slot.base[0, slot.cap).
bool slot_fits(const ChunkSlot& s, size_t at, size_t n) {
    return at <= s.cap && n <= s.cap - at;
}

bool slot_put(const ChunkSlot& s, size_t at, const uint8_t* src, size_t n) {
    if (!slot_fits(s, at, n)) return false;
    if (n) std::memcpy(s.base + at, src, n);
    return true;
}

// Zstd stream src[0, n) -> exactly `want` bytes at slot.base + at.
StageStatus slot_inflate(const ChunkSlot& s, size_t at, size_t want,
                         const uint8_t* src, size_t n, const char* what) {
    if (!slot_fits(s, at, want)) return bad(HX_ERR_FORMAT, kTooLarge);
    const size_t got = zstd().decompress(s.base + at, want, src, n);
    if (zstd().is_error(got) || got != want)
        return bad(HX_ERR_FORMAT, std::string("Zstd ") + what +
                                      " decode failed");
    return {};
}

size_t dec_alloc(std::atomic<size_t>& dec, size_t n) {
    return dec.fetch_add(align64(n));
}

// Definition levels of one data page of an OPTIONAL column, read from the
// place that holds them: a v2 page keeps them outside the
// compressed region (page[0, def_level_bytes)); an uncompressed v1 page opens
// with the length-prefixed block (walk_pages sized it); a compressed v1 page
// has the block inside the stream — a Snappy stream gives it up through a
// prefix decode, a Zstd page after the host decompress (`post`, the whole
// decompressed body; unused otherwise). `page` is the page's bytes as stored.
// *in_stream receives the block's size inside the decompressed body (0 when
// def_level_bytes already accounts for it). bitmap may be null. Returns an
// empty string, or what is wrong with the page.
std::string page_levels(const PageDesc& dp, int32_t codec, const uint8_t* page,
                        const uint8_t* post, size_t post_len, uint64_t* bitmap,
                        uint32_t* in_stream, uint32_t* n_valid) {
    *in_stream = 0;
    const uint8_t* lv = nullptr;
    size_t lv_len = 0;
    std::vector<uint8_t> pre;
    if (!dp.levels_in_stream) {
        const size_t skip = dp.page_type == 0 ? 4 : 0;  // v1 length prefix
        if (size_t(dp.def_level_bytes) < skip) return "level block truncated";
        lv = page + skip;
        lv_len = size_t(dp.def_level_bytes) - skip;
    } else if (codec == CODEC_SNAPPY) {
        uint8_t head[4];
        if (hx_snappy_prefix(page, size_t(dp.compressed_size), head, 4) != 4)
            return "Snappy page too short for its level block";
        // framing against the declared page size; the prefix decode below
        // fails if the stream is shorter than that
        const uint64_t rle = uint64_t(head[0]) | uint64_t(head[1]) << 8 |
                             uint64_t(head[2]) << 16 | uint64_t(head[3]) << 24;
        if (4 + rle > uint64_t(dp.uncompressed_size))
            return "v1 def-level block exceeds page";
        const uint32_t bb = uint32_t(4 + rle);
        pre.resize(bb);
        if (hx_snappy_prefix(page, size_t(dp.compressed_size), pre.data(),
                             bb) != long(bb))
            return "Snappy stream ends inside the level block";
        lv = pre.data() + 4;
        lv_len = bb - 4;
        *in_stream = bb;
    } else {
        uint32_t bb = 0;
        if (!post || hx_level_block_bytes(post, post_len, &bb) != HX_LVL_OK)
            return "v1 def-level block exceeds page";
        lv = post + 4;
        lv_len = bb - 4;
        *in_stream = bb;
    }
    if (dp.num_values < 0) return "negative value count";
    const int rc = hx_levels_to_bitmap(lv, lv_len, uint32_t(dp.num_values),
                                       bitmap, n_valid);
    if (rc != HX_LVL_OK)
        return "malformed definition levels (code " + std::to_string(rc) + ")";
    return std::string();
}

const char* const kColNames[4] = {"series_id", "timestamp", "value",
                                  "__seq__"};

// What the nulls of a page mean for its column: refused with a reason, or
// (PLAIN f64 value column, Overwrite) carried as a validity bitmap.
std::string null_policy(int64_t n_null, const ChunkRole& role,
                        int32_t encoding) {
    const std::string n = std::to_string(n_null) + " null(s): ";
    if (role.col != 2) return n + "nulls in a key column are not supported";
    if (role.bytes_value)
        return n + "nulls in a Binary value column are not supported";
    if (role.update_mode == 1)
        return n + "Append mode over null values is not supported";
    if (encoding != ENC_PLAIN)
        return n + "nulls in a dictionary-encoded value page are not "
                   "supported (PLAIN only)";
    return std::string();
}

// One page's worth of bookkeeping between the steps of stage_chunk.
struct Body {
    uint64_t off = 0;    // where the body is (blob offset, or OFF_DEC | dec)
    size_t raw = 0;      // its size after the host codec step
    uint32_t lvl = 0;    // level bytes that still open the body at `off`
};

// RLE_DICTIONARY chunk: the dictionary payload goes right behind the data
// payload in the slot (raw >= payload when Zstd decompressed the data page).
StageStatus stage_dictionary(const uint8_t* buf, const ChunkRef& cr,
                             const ChunkSlot& slot, const PageDesc& dp,
                             const PageDesc& dict, size_t payload,
                             const Body& body, std::atomic<size_t>& dec,
                             StagedPages& pages, ChunkResult& res) {
    const size_t dict_in_chunk = size_t(dict.payload_off - cr.chunk_start);
    const size_t dict_payload = size_t(dict.compressed_size);
    const bool inflate = cr.codec == CODEC_ZSTD && dict.is_compressed;
    const size_t dict_at = (std::max(body.raw, payload) + 15) & ~size_t(15);
    const size_t dict_need =
        inflate ? size_t(dict.uncompressed_size) : dict_payload;
    if (!slot_fits(slot, dict_at, dict_need))
        return bad(HX_ERR_FORMAT, inflate ? kTooLarge
                                          : "dictionary staging overflow");
    if (inflate) {
        StageStatus s = slot_inflate(slot, dict_at, dict_need,
                                     buf + dict_in_chunk, dict_payload, "dict");
        if (!s.ok()) return s;
    } else {
        slot_put(slot, dict_at, buf + dict_in_chunk, dict_payload);
    }
    uint64_t dict_off = slot.off + dict_at;
    uint64_t dict_raw = dict_need;
    if (cr.codec == CODEC_SNAPPY) {
        SnappyPageDesc sp{};
        sp.src_off = dict_off;
        sp.comp_len = (uint32_t)dict_payload;
        sp.uncomp_len = (uint32_t)dict.uncompressed_size;
        sp.dst_off = OFF_DEC | dec_alloc(dec, sp.uncomp_len);
        pages.snappy.push_back(sp);
        dict_off = sp.dst_off;
        dict_raw = sp.uncomp_len;
    }
    if (dict.num_values < 0 || dict_raw != uint64_t(dict.num_values) * 8)
        return bad(HX_ERR_FORMAT, "dictionary size mismatch");
    RleDictPageDesc rd{};
    rd.dict_off = dict_off;
    rd.dict_n = (uint32_t)dict.num_values;
    rd.idx_off = body.off;
    rd.idx_len = (uint32_t)body.raw;
    rd.n_values = (uint32_t)dp.num_values;
    rd.dst_off = OFF_DEC | dec_alloc(dec, size_t(dp.num_values) * 8);
    pages.rledict.push_back(rd);
    res.final_off = rd.dst_off;
    return {};
}


const char* const kBytesPlainOnly =
    "byte value columns support PLAIN pages only (uncompressed, Snappy, Zstd)";

// Binary value column (BytesMergeOperator stores, operator.rs:47-111): the
// PLAIN BYTE_ARRAY payload stays in the blob; per-row handles (off << 20 |
// len) are walked by k_ba_offsets into the SST's handle array at decode time.
// A handle is relative to the blob, so the body must be in the blob's own
// offset space: uncompressed, Zstd (inflated into the slot) and stored Snappy
// pages sit in their slot — stored meaning one literal, placed verbatim, or
// several literals and nothing else (the Snappy library's form above one
// 64 KiB fragment), whose bodies staging lays end to end — and any other
// Snappy page is decoded into the blob's tail (stage_chunk.h), never into
// dec.
//
// The chunk may hold any number of data pages (parquet-rs and arrow-cpp close
// a page once it reaches 1 MiB). Every page is staged by the one
// set of rules; the pages share the chunk's slot at cumulative offsets and
// each gets a BaPageDesc of its own, first_row advanced by the rows of the
// pages before it. The first page sits where a lone page always sat (slot
// start; a stored literal shifted until its body is 64-aligned); a later page
// starts at the next 8-byte boundary, which the k_snappy_decompress word
// loads of a tail page's stream need and which a page header (17 bytes at the
// least) always pays for. Nothing is reserved or appended before every page
// that can be judged without its Zstd inflate has been judged, and the tail
// is claimed in one piece.
StageStatus stage_bytes_chunk(const uint8_t* buf, const ChunkRef& cr,
                              const ChunkRole& role, const ChunkSlot& slot,
                              StagedPages& pages, ChunkResult& res,
                              std::atomic<size_t>* tail) {
    ChunkPageList pl;
    try {
        list_pages(buf, size_t(cr.comp_size), cr.chunk_start, cr.num_values,
                   !cr.required, cr.codec, &pl);
    } catch (const std::exception& e) {
        return bad(HX_ERR_FORMAT, e.what());
    }
    if (pl.data.empty())
        return bad(HX_ERR_UNSUPPORTED,
                   "expected one data page per chunk (row-group 8192 "
                   "writer contract)");
    int64_t total_values = 0;
    for (const PageDesc& dp : pl.data) {
        if (dp.num_values < 0)
            return bad(HX_ERR_FORMAT, "negative value count");
        total_values += dp.num_values;
    }
    if (total_values != cr.num_values)
        return bad(HX_ERR_FORMAT,
                   "data pages hold " + std::to_string(total_values) +
                       " values, the chunk declares " +
                       std::to_string(cr.num_values));
    if (cr.codec != CODEC_UNCOMPRESSED && cr.codec != CODEC_SNAPPY &&
        cr.codec != CODEC_ZSTD)
        return bad(HX_ERR_UNSUPPORTED,
                   "codec unsupported (uncompressed, Snappy and Zstd)");
    if (cr.codec == CODEC_ZSTD && !zstd().ok)
        return bad(HX_ERR_UNSUPPORTED,
                   "Zstd pages but libzstd.so.1 is not loadable");
    const size_t words = (size_t(cr.num_values) + 63) / 64;
    if (slot.bitmap && slot.bitmap_cap < words * 8)
        return bad(HX_ERR_INVALID, "bitmap capacity too small");
    const bool lone = pl.data.size() == 1;

    // the levels of one page: decoded, never trusted to the statistics; any
    // null refuses the chunk. *lvl = level bytes that open the DEcompressed
    // body of a compressed v1 page.
    auto check_levels = [&](const PageDesc& dp, const uint8_t* page,
                            const uint8_t* post, size_t post_len,
                            uint32_t* lvl) {
        uint32_t n_valid = 0;
        std::string why = page_levels(dp, cr.codec, page, post, post_len,
                                      lone ? slot.bitmap : nullptr, lvl,
                                      &n_valid);
        hx_status st = HX_ERR_FORMAT;
        if (why.empty() && int64_t(n_valid) != int64_t(dp.num_values)) {
            why = null_policy(int64_t(dp.num_values) - int64_t(n_valid), role,
                              dp.encoding);
            st = HX_ERR_UNSUPPORTED;
        }
        res.level_bytes += *lvl ? *lvl : uint32_t(dp.def_level_bytes);
        if (why.empty()) return StageStatus{};
        return bad(st, std::string("column ") + kColNames[role.col] + ": " +
                           why);
    };

    // ---- pass 1: judge every page, place nothing ------------------------
    struct Plan {
        size_t in_chunk, payload, ulen;
        bool zstd_page, snappy_page, stored, literals, to_tail;
        uint32_t lvl, body_off;
    };
    std::vector<Plan> plan(pl.data.size());
    uint64_t tail_claim = 0, tail_need = 0;
    for (size_t k = 0; k < pl.data.size(); k++) {
        const PageDesc& dp = pl.data[k];
        Plan& p = plan[k];
        p = Plan{};
        p.in_chunk = size_t(dp.payload_off - cr.chunk_start);
        // size sanity BEFORE any copy (walk_pages validates too; this guards
        // the invariants the code below depends on)
        if (dp.def_level_bytes < 0 || dp.def_level_bytes > dp.compressed_size ||
            dp.def_level_bytes > dp.uncompressed_size ||
            dp.payload_off < cr.chunk_start ||
            p.in_chunk + size_t(dp.compressed_size) > size_t(cr.comp_size))
            return bad(HX_ERR_FORMAT, "page size fields out of bounds");
        const uint8_t* page = buf + p.in_chunk;
        const uint8_t* src = page + dp.def_level_bytes;
        p.payload = size_t(dp.compressed_size) - size_t(dp.def_level_bytes);
        p.ulen = size_t(dp.uncompressed_size) - size_t(dp.def_level_bytes);
        p.zstd_page = cr.codec == CODEC_ZSTD && dp.is_compressed;
        p.snappy_page = cr.codec == CODEC_SNAPPY && dp.is_compressed;
        // Zstd v1 pages are looked at after the inflate
        if (!cr.required && !(p.zstd_page && dp.levels_in_stream)) {
            StageStatus s = check_levels(dp, page, nullptr, 0, &p.lvl);
            if (!s.ok()) return s;
        }
        if (p.snappy_page && dp.encoding == ENC_PLAIN &&
            hx_snappy_stored_literal(src, p.payload, (uint32_t)p.ulen,
                                     &p.body_off)) {
            p.stored = true;
        } else if (p.snappy_page && dp.encoding == ENC_PLAIN &&
                   hx_snappy_literals_only(src, p.payload, (uint32_t)p.ulen,
                                           nullptr)) {
            // several literals and nothing else: the Snappy library's form
            // of an incompressible page above one 64 KiB fragment
            p.literals = true;
        } else if (p.snappy_page && p.ulen != 0) {
            if (dp.encoding != ENC_PLAIN || !tail)
                return bad(HX_ERR_UNSUPPORTED, kBytesPlainOnly);
            p.to_tail = true;
            tail_claim += p.ulen;
            tail_need += align64(p.ulen);
        }
        if (dp.encoding != ENC_PLAIN && !p.zstd_page)
            return bad(HX_ERR_UNSUPPORTED, kBytesPlainOnly);
    }
    // the chunk's declared size bounds what its pages may claim of the tail,
    // before anything is reserved
    if (tail_claim &&
        (cr.uncomp_size < 0 || tail_claim > uint64_t(cr.uncomp_size)))
        return bad(HX_ERR_FORMAT, kTooLarge);

    // ---- pass 2: place the pages ----------------------------------------
    std::vector<BaPageDesc> ba;
    std::vector<SnappyPageDesc> sn;
    uint64_t in_place = 0, in_place_bytes = 0, raw_total = 0;
    size_t at = 0;                 // cursor in the slot
    size_t tail_at = 0;
    bool tail_taken = false;
    int64_t first_row = int64_t(role.bytes_handles / 8) + role.row_base;
    for (size_t k = 0; k < pl.data.size(); k++) {
        const PageDesc& dp = pl.data[k];
        Plan& p = plan[k];
        const uint8_t* src = buf + p.in_chunk + dp.def_level_bytes;
        if (k) at = (at + 7) & ~size_t(7);
        Body body{slot.off + at, p.payload, 0};
        if (p.zstd_page) {
            // host-side inflate from the read buffer into the slot
            StageStatus s =
                slot_inflate(slot, at, p.ulen, src, p.payload, "page");
            if (!s.ok()) return s;
            body.raw = p.ulen;
            if (!cr.required && dp.levels_in_stream) {
                // drop the level block: the body moves to where the page
                // starts, as for a REQUIRED page
                s = check_levels(dp, buf + p.in_chunk, slot.base + at, p.ulen,
                                 &p.lvl);
                if (!s.ok()) return s;
                std::memmove(slot.base + at, slot.base + at + p.lvl,
                             p.ulen - p.lvl);
                body.raw = p.ulen - p.lvl;
            }
            if (dp.encoding != ENC_PLAIN)
                return bad(HX_ERR_UNSUPPORTED, kBytesPlainOnly);
            at += body.raw;
        } else if (p.stored) {
            // nothing to decode: the payload goes in verbatim and the
            // descriptor points at the literal's body (behind an OPTIONAL v1
            // page's level block). A lone or first page is shifted so that
            // body is 64-aligned, as it always was.
            const uint32_t body_off = p.body_off + p.lvl;
            const size_t pad = k ? 0 : (64 - (body_off & 63u)) & 63u;
            if (!slot_put(slot, at + pad, src, p.payload))
                return bad(HX_ERR_FORMAT, kTooLarge);
            body = Body{slot.off + at + pad + body_off, p.ulen - p.lvl, 0};
            in_place++;
            in_place_bytes += body.raw;
            at += pad + p.payload;
        } else if (p.literals) {
            // nothing to decode either: the literals' bodies go into the
            // slot back to back (ulen < payload, so they fit where the
            // payload would), the tags between them dropped, and the page is
            // read in place like a stored one
            const size_t pad = k ? 0 : (64 - (p.lvl & 63u)) & 63u;
            if (!slot_fits(slot, at + pad, p.ulen) ||
                !hx_snappy_literals_only(src, p.payload, (uint32_t)p.ulen,
                                         slot.base + at + pad))
                return bad(HX_ERR_FORMAT, kTooLarge);
            body = Body{slot.off + at + pad + p.lvl, p.ulen - p.lvl, 0};
            in_place++;
            in_place_bytes += body.raw;
            at += pad + p.ulen;
        } else {
            if (!slot_put(slot, at, src, p.payload))
                return bad(HX_ERR_FORMAT, kTooLarge);
            if (p.snappy_page && p.ulen == 0) {
                body.raw = 0;   // v2 page of nulls only: nothing to decode
            } else if (p.to_tail) {
                // decoded into the blob's tail, so the handles k_ba_offsets
                // writes stay relative to the blob
                if (!tail_taken) {
                    tail_at = tail->fetch_add(size_t(tail_need));
                    tail_taken = true;
                }
                SnappyPageDesc sp{};
                sp.src_off = slot.off + at;
                sp.comp_len = (uint32_t)p.payload;
                sp.uncomp_len = (uint32_t)p.ulen;
                sp.dst_off = tail_at;
                tail_at += align64(p.ulen);
                sn.push_back(sp);
                body.off = sp.dst_off + p.lvl;
                body.raw = p.ulen - p.lvl;
            }
            at += p.payload;
        }
        BaPageDesc bp{};
        bp.src_off = body.off;   // blob byte offset (no flag bit)
        bp.src_len = body.raw;
        bp.n_values = (uint32_t)dp.num_values;
        bp.first_row = first_row;
        first_row += dp.num_values;
        ba.push_back(bp);
        raw_total += body.raw;
    }
    if (!lone && slot.bitmap && !cr.required) {
        // no page held a null
        std::memset(slot.bitmap, 0, words * 8);
        hx_bitmap_set_range(slot.bitmap, 0, uint64_t(cr.num_values));
    }
    pages.ba.insert(pages.ba.end(), ba.begin(), ba.end());
    pages.snappy_ba.insert(pages.snappy_ba.end(), sn.begin(), sn.end());
    pages.pages_in_place += in_place;
    pages.bytes_in_place += in_place_bytes;
    res.n_valid = (uint32_t)cr.num_values;
    res.stored = in_place == pl.data.size();
    res.raw_size = raw_total;
    res.final_off =
        OFF_DEC | (role.bytes_handles + uint64_t(role.row_base) * 8);
    return {};
}

// PLAIN 8-byte column: read where it is, unless it sits behind a level block
// in dec (not 8-aligned) or is packed around nulls — then k_expand_optional
// writes the dense column on every decode pass.
StageStatus stage_plain(const ChunkRef& cr, const Body& body,
                        std::atomic<size_t>& dec, StagedPages& pages,
                        ChunkResult& res) {
    // the body holds the present values only
    if (body.raw != size_t(res.n_valid) * 8)
        return bad(HX_ERR_FORMAT, "PLAIN payload size mismatch");
    res.final_off = body.off;
    if (body.lvl || res.has_nulls) {
        ExpandPageDesc ep{};
        ep.src_off = body.off - body.lvl;
        ep.src_len = (uint32_t)(body.raw + body.lvl);
        ep.lvl_bytes = body.lvl;
        ep.n_rows = (uint32_t)cr.num_values;
        ep.n_valid = res.n_valid;
        ep.bitmap_off = res.valid_off;
        ep.dst_off = OFF_DEC | dec_alloc(dec, size_t(cr.num_values) * 8);
        pages.expand.push_back(ep);
        res.final_off = ep.dst_off;
    }
    return {};
}

StageStatus stage_delta(const ChunkRef& cr, const Body& body,
                        std::atomic<size_t>& dec, StagedPages& pages,
                        ChunkResult& res) {
    if (cr.num_values > 8192)
        return bad(HX_ERR_UNSUPPORTED, "delta page > 8192 values");
    DeltaPageDesc dd{};
    dd.src_off = body.off;
    dd.src_len = (uint32_t)body.raw;
    dd.n_values = (uint32_t)cr.num_values;
    dd.dst_off = OFF_DEC | dec_alloc(dec, size_t(cr.num_values) * 8);
    pages.delta.push_back(dd);
    res.final_off = dd.dst_off;
    return {};
}

}  // namespace

StageStatus read_chunk(int fd, const std::string& path, const ChunkRef& cr,
                       std::vector<uint8_t>& buf) {
    if (cr.comp_size <= 0 || cr.comp_size > (int64_t)1 << 31)
        return bad(HX_ERR_FORMAT, path + ": implausible chunk size");
    buf.resize(size_t(cr.comp_size));
    if (pread(fd, buf.data(), buf.size(), cr.chunk_start) !=
        (ssize_t)buf.size())
        return bad(HX_ERR_IO, "chunk read " + path);
    return {};
}

StageStatus stage_chunk(const uint8_t* buf, const ChunkRef& cr,
                        const ChunkRole& role, const ChunkSlot& slot,
                        std::atomic<size_t>& dec, StagedPages& pages,
                        ChunkResult& res, std::atomic<size_t>* tail) {
    res = ChunkResult{};
    // the BYTE_ARRAY value chunk of a Binary store: any number of data pages
    if (role.bytes_value && role.col == 2)
        return stage_bytes_chunk(buf, cr, role, slot, pages, res, tail);
    // layout contract: exactly one v1/v2 data page per chunk, plus an
    // optional dictionary page (RLE_DICTIONARY chunks)
    ChunkPages cp;
    try {
        if (!select_pages(buf, size_t(cr.comp_size), cr.chunk_start,
                          cr.num_values, !cr.required, cr.codec, &cp))
            return bad(HX_ERR_UNSUPPORTED,
                       "expected one data page per chunk (row-group 8192 "
                       "writer contract)");
    } catch (const std::exception& e) {
        return bad(HX_ERR_FORMAT, e.what());
    }
    const PageDesc& dp = cp.data;
    if (cr.codec != CODEC_UNCOMPRESSED && cr.codec != CODEC_SNAPPY &&
        cr.codec != CODEC_ZSTD)
        return bad(HX_ERR_UNSUPPORTED,
                   "codec unsupported (uncompressed, Snappy and Zstd)");
    if (cr.codec == CODEC_ZSTD && !zstd().ok)
        return bad(HX_ERR_UNSUPPORTED,
                   "Zstd pages but libzstd.so.1 is not loadable");
    // size sanity BEFORE any copy: a corrupt header claiming def_level_bytes
    // > compressed_size would underflow `payload` (size_t) and read out of
    // bounds (walk_pages validates too; this guards the invariants the code
    // below depends on)
    const size_t in_chunk = size_t(dp.payload_off - cr.chunk_start);
    if (dp.def_level_bytes < 0 || dp.def_level_bytes > dp.compressed_size ||
        dp.def_level_bytes > dp.uncompressed_size ||
        dp.payload_off < cr.chunk_start ||
        in_chunk + size_t(dp.compressed_size) > size_t(cr.comp_size))
        return bad(HX_ERR_FORMAT, "page size fields out of bounds");
    const size_t words = (size_t(cr.num_values) + 63) / 64;
    if (slot.bitmap && slot.bitmap_cap < words * 8)
        return bad(HX_ERR_INVALID, "bitmap capacity too small");

    const uint8_t* page = buf + in_chunk;
    const uint8_t* src = page + dp.def_level_bytes;
    const size_t payload =
        size_t(dp.compressed_size) - size_t(dp.def_level_bytes);
    // size of the page body once decompressed
    const size_t ulen =
        size_t(dp.uncompressed_size) - size_t(dp.def_level_bytes);
    const bool zstd_page = cr.codec == CODEC_ZSTD && dp.is_compressed;
    const bool snappy_page = cr.codec == CODEC_SNAPPY && dp.is_compressed;
    Body body{slot.off, payload, 0};
    res.n_valid = (uint32_t)cr.num_values;

    // OPTIONAL column: the levels are decoded, never trusted to the
    // statistics. body.lvl = level bytes that open the DEcompressed body of a
    // compressed v1 page (0 otherwise: def_level_bytes already skipped them).
    auto check_levels = [&](const uint8_t* post, size_t post_len) {
        std::string why = page_levels(dp, cr.codec, page, post, post_len,
                                      slot.bitmap, &body.lvl, &res.n_valid);
        hx_status st = HX_ERR_FORMAT;
        if (why.empty() && int64_t(res.n_valid) != cr.num_values) {
            why = null_policy(cr.num_values - int64_t(res.n_valid), role,
                              dp.encoding);
            st = HX_ERR_UNSUPPORTED;
            res.has_nulls = why.empty();
            if (res.has_nulls) res.valid_off = slot.bitmap_off;
        }
        res.level_bytes = body.lvl ? body.lvl : uint32_t(dp.def_level_bytes);
        if (why.empty()) return StageStatus{};
        return bad(st, std::string("column ") + kColNames[role.col] + ": " +
                           why);
    };
    // Zstd v1 pages are looked at after the decompress
    if (!cr.required && !(zstd_page && dp.levels_in_stream)) {
        StageStatus s = check_levels(nullptr, 0);
        if (!s.ok()) return s;
    }

    if (zstd_page) {
        // host-side decompress into the slot (staging, untimed)
        StageStatus s = slot_inflate(slot, 0, ulen, src, payload, "page");
        if (!s.ok()) return s;
        body.raw = ulen;
        if (!cr.required && dp.levels_in_stream) {
            // drop the level block: the body moves to the slot's (64-aligned)
            // start, as for a REQUIRED page
            s = check_levels(slot.base, ulen);
            if (!s.ok()) return s;
            std::memmove(slot.base, slot.base + body.lvl, ulen - body.lvl);
            body.raw = ulen - body.lvl;
            body.lvl = 0;
        }
    }
    // Stored Snappy page (preamble + ONE literal covering the whole page —
    // what the writer emits for incompressible data): nothing to decode. The
    // payload goes into the slot verbatim, shifted by pad so the literal body
    // sits on a 64-byte boundary, and the column offset points at the body:
    // the scan kernels read it in place like an uncompressed PLAIN page (no
    // SnappyPageDesc, no dec space). PLAIN pages only, the BYTE_ARRAY value
    // page of a Binary store included; dictionary/DELTA pages keep the
    // decoder path.
    uint32_t body_off = 0;
    if (snappy_page && dp.encoding == ENC_PLAIN &&
        hx_snappy_stored_literal(src, payload, (uint32_t)ulen, &body_off)) {
        // an OPTIONAL v1 page's literal opens with the level block (lvl <=
        // ulen, checked against the page size): the PLAIN body behind it is
        // what gets aligned
        body_off += body.lvl;
        const size_t pad = (64 - (body_off & 63u)) & 63u;
        if (!slot_put(slot, pad, src, payload))
            return bad(HX_ERR_FORMAT, kTooLarge);
        body = Body{slot.off + pad + body_off, ulen - body.lvl, 0};
        res.stored = true;
        pages.pages_in_place++;
        pages.bytes_in_place += body.raw;
    } else if (!zstd_page) {
        if (!slot_put(slot, 0, src, payload))
            return bad(HX_ERR_FORMAT, kTooLarge);
        if (snappy_page && ulen == 0) {
            body.raw = 0;   // v2 page of nulls only: nothing to decode
        } else if (snappy_page) {
            SnappyPageDesc sp{};
            sp.src_off = slot.off;
            sp.comp_len = (uint32_t)payload;
            sp.uncomp_len = (uint32_t)ulen;
            sp.dst_off = OFF_DEC | dec_alloc(dec, sp.uncomp_len);
            pages.snappy.push_back(sp);
            // the decoder's dst stays 64-aligned; an OPTIONAL v1 page's body
            // follows its level block there
            body.off = sp.dst_off + body.lvl;
            body.raw = sp.uncomp_len - body.lvl;
        }
    }
    res.raw_size = body.raw;

    if (dp.encoding == ENC_PLAIN)
        return stage_plain(cr, body, dec, pages, res);
    if (dp.encoding == ENC_DELTA_BINARY_PACKED && role.col != 2)
        return stage_delta(cr, body, dec, pages, res);
    if ((dp.encoding == ENC_RLE_DICTIONARY ||
         dp.encoding == ENC_PLAIN_DICTIONARY) && cp.has_dict)
        return stage_dictionary(buf, cr, slot, dp, cp.dict, payload, body, dec,
                                pages, res);
    return bad(HX_ERR_UNSUPPORTED, "encoding " + std::to_string(dp.encoding) +
                                       " unsupported (round 1)");
}

void patch_rg_offsets(std::vector<RgDesc>& rgs, std::vector<RgValid>& rg_valid,
                      const std::vector<SstDev>& ssts,
                      const std::vector<ChunkResult>& results,
                      std::vector<CopyDesc>& copies) {
    rg_valid.assign(rgs.size(), RgValid{0, 0});
    size_t k = 0;
    for (size_t i = 0; i < rgs.size(); i++) {
        RgDesc& rd = rgs[i];
        const SstDev& sd = ssts[rd.sst_id];
        const int n_staged_cols = sd.dense_seq ? 4 : 3;
        uint64_t offs[4] = {0, 0, 0, 0};
        for (int c = 0; c < n_staged_cols; c++, k++) {
            offs[c] = results[k].final_off;
            if (c == 2) rg_valid[i].off = results[k].valid_off;
        }
        rd.series_off = offs[0];
        rd.ts_off = offs[1];
        rd.val_off = offs[2];
        auto dense_copy = [&](uint64_t src, uint64_t dense) {
            CopyDesc c{};
            c.src_off = src;
            c.dst_off = (dense & OFF_MASK) + uint64_t(rd.row_base) * 8;
            c.n_values = rd.n_rows;
            copies.push_back(c);
        };
        if (sd.dense_seq) dense_copy(offs[3], sd.dense_seq);
        if (sd.cluster >= 0) {
            // dense (series, ts) arrays for binary-search dedup
            dense_copy(offs[0], sd.dense_series);
            dense_copy(offs[1], sd.dense_ts);
        }
    }
}

void slice_and_order(std::vector<RgDesc>& rgs, std::vector<RgValid>& rg_valid,
                     size_t n_ssts, uint32_t split, SstRgLists& lists) {
    // ---- slice + align row groups across SSTs ----------------------------
    // SSTs may carry different rows-per-series (time windows of 1 vs 2
    // points), so the k-th row group of two SSTs can cover very different
    // series ranges. For the group table's L2/L3 locality under the wave
    // kernel the unit list is (a) split into ~half-row-group slices and
    // (b) ordered by FRACTIONAL row position within its SST — units at
    // the same fraction cover the same series quantile of the shared series
    // universe. Speed-only: dispatch order is never relied on for
    // correctness; dedup successor links (next_rg) are remapped.
    if (split < 1) split = 1;
    const size_t n_old = rgs.size();
    std::vector<RgDesc> sliced;
    std::vector<RgValid> sliced_valid;
    std::vector<int32_t> new_first(n_old);
    std::vector<int32_t> last_slice(n_old);
    for (size_t i = 0; i < n_old; i++) {
        const RgDesc& rd = rgs[i];
        const uint32_t ssize =
            std::max<uint32_t>(1024, (rd.n_rows + split - 1) / split);
        new_first[i] = (int32_t)sliced.size();
        for (uint32_t start = 0; start < rd.n_rows; start += ssize) {
            RgDesc sl = rd;
            sl.series_off = rd.series_off + uint64_t(start) * 8;
            sl.ts_off = rd.ts_off + uint64_t(start) * 8;
            sl.val_off = rd.val_off + uint64_t(start) * 8;
            sl.n_rows = std::min(ssize, rd.n_rows - start);
            sl.row_base = rd.row_base + start;
            // same bitmap, later bit: a slice need not start on a word
            sliced_valid.push_back({rg_valid[i].off, start});
            sl.next_rg = (start + ssize < rd.n_rows)
                             ? (int32_t)sliced.size() + 1
                             : rd.next_rg;  // old id; remapped below
            last_slice[i] = (int32_t)sliced.size();
            sliced.push_back(sl);
        }
    }
    for (size_t i = 0; i < n_old; i++) {
        int32_t nx = rgs[i].next_rg;
        sliced[last_slice[i]].next_rg = nx >= 0 ? new_first[nx] : -1;
    }
    // fractional position of each slice within its SST's staged rows
    std::vector<int64_t> sst_rows(n_ssts, 0);
    for (const auto& sl : sliced) {
        int64_t end = sl.row_base + sl.n_rows;
        if (end > sst_rows[sl.sst_id]) sst_rows[sl.sst_id] = end;
    }
    std::vector<uint32_t> order(sliced.size());
    for (size_t i = 0; i < sliced.size(); i++) order[i] = (uint32_t)i;
    std::vector<double> frac(sliced.size());
    for (size_t i = 0; i < sliced.size(); i++)
        frac[i] = sst_rows[sliced[i].sst_id]
                      ? double(sliced[i].row_base) /
                            double(sst_rows[sliced[i].sst_id])
                      : 0.0;
    // order purely by fractional position: concurrently resident blocks
    // then share one narrow series window across ALL SSTs, keeping the
    // group table's hot lines cache-resident (measured 1.8x on the wave
    // kernel vs size-class-primary ordering)
    std::stable_sort(order.begin(), order.end(),
                     [&](uint32_t a, uint32_t b) { return frac[a] < frac[b]; });
    std::vector<int32_t> inv(sliced.size());
    for (size_t i = 0; i < sliced.size(); i++) inv[order[i]] = (int32_t)i;
    rgs.resize(sliced.size());
    rg_valid.resize(sliced.size());
    for (size_t i = 0; i < sliced.size(); i++) {
        rgs[i] = sliced[order[i]];
        rg_valid[i] = sliced_valid[order[i]];
        if (rgs[i].next_rg >= 0) rgs[i].next_rg = inv[rgs[i].next_rg];
    }

    // per-SST rg lists in row order (series-range kernel): the
    // fractional reorder above scrambles rgs, so the range kernel walks SSTs
    // through these index lists instead
    const size_t n = rgs.size();
    std::vector<uint32_t> idx(n);
    for (size_t i = 0; i < n; i++) idx[i] = (uint32_t)i;
    std::sort(idx.begin(), idx.end(), [&](uint32_t a, uint32_t b) {
        if (rgs[a].sst_id != rgs[b].sst_id)
            return rgs[a].sst_id < rgs[b].sst_id;
        return rgs[a].row_base < rgs[b].row_base;
    });
    lists.rgs.assign(idx.begin(), idx.end());
    lists.off.assign(n_ssts, 0);
    lists.cnt.assign(n_ssts, 0);
    for (size_t i = 0; i < n; i++) {
        uint32_t sid = rgs[idx[i]].sst_id;
        if (lists.cnt[sid] == 0) lists.off[sid] = (int32_t)i;
        lists.cnt[sid]++;
    }
}

}  // namespace hx
