// stage_check.cpp — stand-alone host check of staging (stage_chunk.{h,cpp} +
// parquet_meta.cpp). Built by `make stage_check` with
// -fsanitize=address,undefined when the runtime is available. No GPU.
//
//   stage_check [PATH | fuzz:PATH | tight:PATH]...
//
// Every column chunk of every SST given is staged into a slot that is its own
// heap block of exactly hx::chunk_reserve bytes (the validity words likewise),
// so a write past the reservation trips the sanitizer instead of landing in a
// neighbour's slot; the plain build still runs the bounds assertions below.
// One REC line (JSON) per chunk says what was staged; tests/
// test_stage_chunk_cpu.py compares those with what pyarrow reads.
//   fuzz:  the file's chunks are also staged under seeded byte mutations and
//          rewrites of the header size fields: staged or refused, never out
//          of bounds.
//   tight: the file's Zstd chunks are also staged with the catalog claiming
//          less decompressed size than the pages inflate to: must be refused.
// slice_and_order runs over seeded random layouts regardless of arguments.
// Prints one line per check, "ALL OK" last; exits non-zero on any FAIL.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <memory>
#include <string>
#include <vector>

#include "parquet_meta.h"
#include "stage_chunk.h"

namespace {

int g_fail = 0;

void report(const std::string& what, bool ok) {
    std::printf("%s %s\n", what.c_str(), ok ? "OK" : "FAIL");
    if (!ok) g_fail++;
}

struct Rng {  // xorshift64*, seeded per use so failures repeat
    uint64_t s;
    explicit Rng(uint64_t seed) : s(seed * 0x9E3779B97F4A7C15ull + 1) {}
    uint64_t next() {
        s ^= s >> 12; s ^= s << 25; s ^= s >> 27;
        return s * 0x2545F4914F6CDD1Dull;
    }
    uint64_t below(uint64_t n) { return next() % n; }
};

std::string hex(const uint8_t* p, size_t n) {
    static const char d[] = "0123456789abcdef";
    std::string o(n * 2, '0');
    for (size_t i = 0; i < n; i++) {
        o[2 * i] = d[p[i] >> 4];
        o[2 * i + 1] = d[p[i] & 15];
    }
    return o;
}

constexpr uint64_t kSlotOff = 0x40000;    // blob offsets the test slot claims
constexpr uint64_t kBitmapOff = 0x20000;
constexpr size_t kDecStart = 0x1000;

// One staging attempt with exact-size heap blocks for chunk, slot and bitmap.
struct Attempt {
    hx::ChunkRef cr;
    hx::ChunkRole role;
    std::unique_ptr<uint8_t[]> chunk, mem;
    std::unique_ptr<uint64_t[]> words;
    hx::ChunkSlot slot;
    hx::StagedPages pages;
    hx::ChunkResult res;
    size_t dec_end = kDecStart;
    hx::StageStatus st;

    Attempt(const hx::ChunkRef& c, const hx::ChunkRole& r, const uint8_t* bytes)
        : cr(c), role(r) {
        chunk.reset(new uint8_t[size_t(cr.comp_size)]);
        std::memcpy(chunk.get(), bytes, size_t(cr.comp_size));
        slot.cap = hx::chunk_reserve(cr);
        mem.reset(new uint8_t[slot.cap]);
        std::memset(mem.get(), 0xA5, slot.cap);
        slot.base = mem.get();
        slot.off = kSlotOff;
        slot.bitmap_cap = hx::bitmap_reserve(cr, role.col, role.bytes_value);
        if (slot.bitmap_cap) {
            words.reset(new uint64_t[slot.bitmap_cap / 8]);
            slot.bitmap = words.get();
            slot.bitmap_off = kBitmapOff;
        }
    }
    void run() {
        std::atomic<size_t> dec{kDecStart};
        st = hx::stage_chunk(chunk.get(), cr, role, slot, dec, pages, res);
        dec_end = dec.load();
    }

    // [off, off + len) lies where this chunk may point: its slot for a blob
    // offset, the dec bytes it reserved for an OFF_DEC one
    bool in_bounds(uint64_t off, uint64_t len) const {
        if (off & hx::OFF_DEC) {
            const uint64_t o = off & hx::OFF_MASK;
            return o >= kDecStart && o <= dec_end && len <= dec_end - o;
        }
        return off >= slot.off && off - slot.off <= slot.cap &&
               len <= slot.cap - (off - slot.off);
    }

    // The bounds assertions on a staged chunk; "" when all hold.
    std::string verify() const {
        struct Res { uint64_t off, bytes; };
        std::vector<Res> dst;   // dec reservations: where and how much written
        for (const auto& d : pages.snappy) {
            if (!in_bounds(d.src_off, d.comp_len) || (d.src_off & hx::OFF_DEC))
                return "snappy src out of slot";
            dst.push_back({d.dst_off, d.uncomp_len});
        }
        for (const auto& d : pages.expand) {
            if (!in_bounds(d.src_off, d.src_len)) return "expand src";
            if (uint64_t(d.lvl_bytes) + uint64_t(d.n_valid) * 8 != d.src_len)
                return "expand src_len";
            if (d.bitmap_off && (d.bitmap_off != slot.bitmap_off ||
                                 (uint64_t(d.n_rows) + 63) / 64 * 8 >
                                     slot.bitmap_cap))
                return "expand bitmap";
            if (d.n_valid != d.n_rows && !d.bitmap_off)
                return "expand: nulls without a bitmap";
            dst.push_back({d.dst_off, uint64_t(d.n_rows) * 8});
        }
        for (const auto& d : pages.delta) {
            if (!in_bounds(d.src_off, d.src_len)) return "delta src";
            dst.push_back({d.dst_off, uint64_t(d.n_values) * 8});
        }
        for (const auto& d : pages.rledict) {
            if (!in_bounds(d.dict_off, uint64_t(d.dict_n) * 8)) return "dict";
            if (!in_bounds(d.idx_off, d.idx_len)) return "dict idx";
            dst.push_back({d.dst_off, uint64_t(d.n_values) * 8});
        }
        for (const auto& d : pages.ba)
            if (!in_bounds(d.src_off, d.src_len) || (d.src_off & hx::OFF_DEC))
                return "ba src";
        // reservations tile [kDecStart, dec_end): each is 64-aligned and
        // exactly align64 of what its descriptor writes
        std::sort(dst.begin(), dst.end(),
                  [](const Res& a, const Res& b) { return a.off < b.off; });
        uint64_t at = kDecStart;
        for (const Res& r : dst) {
            if (!(r.off & hx::OFF_DEC) || (r.off & hx::OFF_MASK) != at)
                return "dec reservation misplaced";
            at += hx::align64(r.bytes);
        }
        if (at != dec_end) return "dec reservation size";
        if (!role.bytes_value || role.col != 2) {
            if (!in_bounds(res.final_off, 0)) return "final_off";
            if (!(res.final_off & hx::OFF_DEC) &&
                !in_bounds(res.final_off, res.raw_size))
                return "body out of slot";
        }
        if (slot.bitmap && !cr.required) {
            const uint64_t n = uint64_t(cr.num_values);
            uint64_t pop = 0;
            for (uint64_t w = 0; w < (n + 63) / 64; w++) {
                uint64_t v = slot.bitmap[w];
                if (w == n / 64 && (n & 63) && (v >> (n & 63)))
                    return "bitmap bits above n_rows";
                pop += uint64_t(__builtin_popcountll(v));
            }
            if (pop != res.n_valid) return "bitmap popcount";
        }
        if (res.has_nulls != (int64_t(res.n_valid) != cr.num_values))
            return "has_nulls";
        return "";
    }
};

struct Chunk {  // one column chunk of a file under test
    std::string file;
    int rg = 0;
    hx::ChunkRef cr;
    hx::ChunkRole role;
    const uint8_t* bytes = nullptr;
};

const char* const kCols[4] = {"series_id", "timestamp", "value", "__seq__"};

bool load(const std::string& path, std::vector<uint8_t>& data,
          std::vector<Chunk>& out) {
    std::ifstream f(path, std::ios::binary);
    data.assign(std::istreambuf_iterator<char>(f), {});
    if (data.size() < 12) return false;
    uint32_t flen;
    std::memcpy(&flen, data.data() + data.size() - 8, 4);
    if (size_t(flen) + 8 > data.size()) return false;
    hx::FileMetadata m =
        hx::parse_footer(data.data() + data.size() - 8 - flen, flen + 8,
                         int64_t(data.size()));
    const std::string base = path.substr(path.find_last_of('/') + 1);
    int64_t row_base = 0;
    for (size_t r = 0; r < m.row_groups.size(); r++) {
        for (int c = 0; c < 4; c++) {
            size_t ci = 0;
            while (ci < m.columns.size() && m.columns[ci].name != kCols[c]) ci++;
            if (ci == m.columns.size()) continue;
            const hx::ColumnChunkMeta& cc = m.row_groups[r].columns[ci];
            Chunk k;
            k.file = base;
            k.rg = int(r);
            k.cr.codec = cc.codec;
            k.cr.required = m.columns[ci].required;
            k.cr.chunk_start = cc.chunk_start();
            k.cr.comp_size = cc.total_compressed_size;
            k.cr.uncomp_size = cc.total_uncompressed_size;
            k.cr.num_values = cc.num_values;
            if (k.cr.chunk_start < 0 || k.cr.comp_size <= 0 ||
                uint64_t(k.cr.chunk_start) + uint64_t(k.cr.comp_size) >
                    data.size())
                return false;
            k.role.col = c;
            k.role.row_base = row_base;
            for (const auto& sc : m.columns)
                if (sc.name == "value" && sc.physical_type == hx::PT_BYTE_ARRAY)
                    k.role.bytes_value = true;
            k.bytes = data.data() + k.cr.chunk_start;
            out.push_back(k);
        }
        row_base += m.row_groups[r].num_rows;
    }
    return true;
}

// Stage the chunk as written; print its record; check what must hold.
bool stage_plain(const Chunk& k) {
    Attempt a(k.cr, k.role, k.bytes);
    a.run();
    const std::string id =
        k.file + " rg" + std::to_string(k.rg) + " " + kCols[k.role.col];
    if (!a.st.ok()) {
        report("stage " + id + " (" + a.st.msg + ")", false);
        return false;
    }
    std::string why = a.verify();
    hx::ChunkPages cp;
    hx::select_pages(k.bytes, size_t(k.cr.comp_size), k.cr.chunk_start,
                     k.cr.num_values, !k.cr.required, k.cr.codec, &cp);
    const bool in_blob = !(a.res.final_off & hx::OFF_DEC);
    const bool plain8 = cp.data.encoding == hx::ENC_PLAIN &&
                        !(k.role.bytes_value && k.role.col == 2);
    if (why.empty() && plain8) {
        // a PLAIN body is n_valid * 8 bytes; it is read in place, 64-byte
        // aligned, or a decoder/expander writes the column to dec
        if (a.res.raw_size != uint64_t(a.res.n_valid) * 8)
            why = "PLAIN body size";
        else if (in_blob && (a.res.final_off & 63))
            why = "PLAIN body not 64-byte aligned";
        else if (!in_blob && a.pages.expand.empty() && a.pages.snappy.empty())
            why = "PLAIN body in dec without a descriptor";
    }
    std::string body, packed;
    if (in_blob)
        body = hex(a.slot.base + (a.res.final_off - kSlotOff), a.res.raw_size);
    for (const auto& e : a.pages.expand)
        if (!(e.src_off & hx::OFF_DEC))
            packed = hex(a.slot.base + (e.src_off - kSlotOff) + e.lvl_bytes,
                         size_t(e.n_valid) * 8);
    std::string bitmap;
    if (a.slot.bitmap)
        bitmap = hex((const uint8_t*)a.slot.bitmap,
                     (size_t(k.cr.num_values) + 63) / 64 * 8);
    std::printf(
        "REC {\"file\":\"%s\",\"rg\":%d,\"col\":\"%s\",\"where\":\"%s\","
        "\"off_mod64\":%u,\"raw\":%llu,\"level_bytes\":%u,\"n_valid\":%u,"
        "\"has_nulls\":%d,\"stored\":%d,\"in_place\":%llu,\"snappy\":%zu,"
        "\"expand\":%zu,\"delta\":%zu,\"rledict\":%zu,\"ba\":%zu,"
        "\"bitmap\":\"%s\",\"body\":\"%s\",\"packed\":\"%s\"}\n",
        k.file.c_str(), k.rg, kCols[k.role.col], in_blob ? "blob" : "dec",
        unsigned(a.res.final_off & 63), (unsigned long long)a.res.raw_size,
        a.res.level_bytes, a.res.n_valid, int(a.res.has_nulls),
        int(a.res.stored), (unsigned long long)a.pages.pages_in_place,
        a.pages.snappy.size(), a.pages.expand.size(), a.pages.delta.size(),
        a.pages.rledict.size(), a.pages.ba.size(), bitmap.c_str(),
        body.c_str(), packed.c_str());
    for (const auto& d : a.pages.snappy)
        std::printf("  snappy src=%#llx comp=%u uncomp=%u dst=%#llx\n",
                    (unsigned long long)d.src_off, d.comp_len, d.uncomp_len,
                    (unsigned long long)d.dst_off);
    for (const auto& d : a.pages.expand)
        std::printf("  expand src=%#llx len=%u lvl=%u rows=%u valid=%u "
                    "bitmap=%#llx dst=%#llx\n",
                    (unsigned long long)d.src_off, d.src_len, d.lvl_bytes,
                    d.n_rows, d.n_valid, (unsigned long long)d.bitmap_off,
                    (unsigned long long)d.dst_off);
    for (const auto& d : a.pages.delta)
        std::printf("  delta src=%#llx len=%u n=%u dst=%#llx\n",
                    (unsigned long long)d.src_off, d.src_len, d.n_values,
                    (unsigned long long)d.dst_off);
    for (const auto& d : a.pages.rledict)
        std::printf("  rledict dict=%#llx n=%u idx=%#llx len=%u values=%u "
                    "dst=%#llx\n",
                    (unsigned long long)d.dict_off, d.dict_n,
                    (unsigned long long)d.idx_off, d.idx_len, d.n_values,
                    (unsigned long long)d.dst_off);
    for (const auto& d : a.pages.ba)
        std::printf("  ba src=%#llx len=%llu n=%u first_row=%lld\n",
                    (unsigned long long)d.src_off,
                    (unsigned long long)d.src_len, d.n_values,
                    (long long)d.first_row);
    report("stage " + id + (why.empty() ? "" : " (" + why + ")"), why.empty());
    return why.empty();
}

// ---- hostile input --------------------------------------------------------

struct Tally { int staged = 0, refused = 0, broken = 0; };

void attempt_hostile(const hx::ChunkRef& cr, const hx::ChunkRole& role,
                     const uint8_t* bytes, Tally& t, const std::string& what) {
    Attempt a(cr, role, bytes);
    a.run();
    if (!a.st.ok()) {
        t.refused++;
        return;
    }
    const std::string why = a.verify();
    if (why.empty()) {
        t.staged++;
    } else {
        t.broken++;
        report("hostile " + what + " (" + why + ")", false);
    }
}

std::vector<uint8_t> zigzag_varint(int32_t v) {
    uint32_t z = (uint32_t(v) << 1) ^ uint32_t(v >> 31);
    std::vector<uint8_t> o;
    while (z >= 0x80) {
        o.push_back(uint8_t(z & 0x7f) | 0x80);
        z >>= 7;
    }
    o.push_back(uint8_t(z));
    return o;
}

void fuzz_chunk(const Chunk& k, uint64_t seed, Tally& t) {
    const size_t n = size_t(k.cr.comp_size);
    hx::ChunkPages cp;
    hx::select_pages(k.bytes, n, k.cr.chunk_start, k.cr.num_values,
                     !k.cr.required, k.cr.codec, &cp);
    // hot spots: the 64 bytes that open each page header and each payload
    std::vector<size_t> hot = {0, size_t(cp.data.payload_off - k.cr.chunk_start)};
    if (cp.has_dict) {
        const size_t dpay = size_t(cp.dict.payload_off - k.cr.chunk_start);
        hot.push_back(dpay);
        hot.push_back(dpay + size_t(cp.dict.compressed_size));  // next header
    }
    Rng rng(seed);
    std::vector<uint8_t> buf(k.bytes, k.bytes + n);
    for (int i = 0; i < 700; i++) {
        size_t pos = rng.below(4) ? hot[rng.below(hot.size())] + rng.below(64)
                                  : rng.below(n);
        if (pos >= n) pos = n - 1;
        const uint8_t keep = buf[pos];
        buf[pos] = rng.below(2) ? uint8_t(keep ^ (1u << rng.below(8)))
                                : uint8_t(rng.next());
        attempt_hostile(k.cr, k.role, buf.data(), t,
                        k.file + " byte " + std::to_string(pos));
        buf[pos] = keep;
    }
    // size fields of the page headers, rewritten in place to other values of
    // the same encoded length: uncompressed_size, compressed_size,
    // num_values, and the v2 level byte lengths
    const size_t hdr_end = size_t(cp.data.payload_off - k.cr.chunk_start);
    for (const hx::PageDesc* p : {&cp.data, cp.has_dict ? &cp.dict : nullptr}) {
        if (!p) continue;
        for (int32_t v : {p->uncompressed_size, p->compressed_size,
                          p->num_values, p->def_level_bytes, 0}) {
            const std::vector<uint8_t> pat = zigzag_varint(v);
            for (size_t at = 0; at + pat.size() <= hdr_end; at++) {
                if (std::memcmp(buf.data() + at, pat.data(), pat.size()) != 0)
                    continue;
                const int bits = int(pat.size()) * 7;
                const uint32_t top =
                    bits >= 32 ? 0xFFFFFFFFu : (1u << bits) - 1;
                const uint32_t lo = pat.size() == 1 ? 0 : 1u << (bits - 7);
                const uint32_t zz = (uint32_t(v) << 1) ^ uint32_t(v >> 31);
                for (uint32_t z : {top, top - 1, lo, zz + 2, zz - 2, zz * 2,
                                   zz / 2, zz + 16, zz ^ 1u}) {
                    if (z < lo || z > top || z == zz) continue;
                    uint32_t w = z;
                    for (size_t b = 0; b < pat.size(); b++, w >>= 7)
                        buf[at + b] = uint8_t(w & 0x7f) |
                                      (b + 1 < pat.size() ? 0x80 : 0);
                    attempt_hostile(k.cr, k.role, buf.data(), t,
                                    k.file + " field at " + std::to_string(at));
                }
                std::memcpy(buf.data() + at, pat.data(), pat.size());
            }
        }
    }
    // the catalog's side of the same sizes
    for (int i = 0; i < 6; i++) {
        hx::ChunkRef cr = k.cr;
        if (i == 0) cr.uncomp_size = cr.comp_size;
        if (i == 1) cr.uncomp_size = 0;
        if (i == 2) cr.num_values += 1;
        if (i == 3) cr.num_values = cr.num_values / 2;
        if (i == 4) cr.num_values = int64_t(1) << 20;
        if (i == 5) cr.comp_size = cr.comp_size / 2 + 1;
        attempt_hostile(cr, k.role, k.bytes, t,
                        k.file + " catalog rewrite " + std::to_string(i));
    }
}

// Zstd chunk whose catalog entry claims less than its pages inflate to:
// uncomp_size = comp_size starves the data page; uncomp_size = the data
// page's own size leaves no room for the dictionary behind it.
int tight_chunk(const Chunk& k) {
    if (k.cr.codec != hx::CODEC_ZSTD) return 0;
    hx::ChunkPages cp;
    hx::select_pages(k.bytes, size_t(k.cr.comp_size), k.cr.chunk_start,
                     k.cr.num_values, !k.cr.required, k.cr.codec, &cp);
    hx::ChunkRef cr = k.cr;
    std::string what;
    const int64_t data_ulen =
        cp.data.uncompressed_size - cp.data.def_level_bytes;
    if (cp.has_dict && data_ulen + cp.dict.uncompressed_size >
                           std::max(k.cr.comp_size, data_ulen)) {
        cr.uncomp_size = std::max(cr.comp_size, data_ulen);
        what = "Zstd dictionary page";
    } else if (!cp.has_dict &&
               cp.data.uncompressed_size > 2 * k.cr.comp_size) {
        cr.uncomp_size = cr.comp_size;
        what = "Zstd data page";
    } else {
        return 0;
    }
    Attempt a(cr, k.role, k.bytes);
    a.run();
    const bool refused =
        a.st.msg == "page larger than its chunk's declared size";
    std::printf("tight %s %s: %d bytes into a %zu-byte slot: %s\n",
                k.file.c_str(), what.c_str(),
                cp.has_dict ? cp.dict.uncompressed_size
                            : cp.data.uncompressed_size,
                a.slot.cap, a.st.ok() ? "staged" : a.st.msg.c_str());
    report("tight " + k.file + " " + kCols[k.role.col] + " " + what +
               " refused", refused);
    return 1;
}

// ---- slice_and_order over random layouts ----------------------------------

void check_slicing() {
    int bad = 0, layouts = 0;
    for (uint64_t seed = 1; seed <= 150; seed++) {
        for (uint32_t split = 1; split <= 3; split++, layouts++) {
            Rng rng(seed);
            const size_t n_ssts = 1 + rng.below(5);
            std::vector<hx::RgDesc> rgs;
            std::vector<hx::RgValid> valid;
            std::vector<int64_t> sst_rows(n_ssts, 0);
            for (size_t s = 0; s < n_ssts; s++) {
                const int n_rg = 1 + int(rng.below(6));
                for (int r = 0; r < n_rg; r++) {
                    hx::RgDesc d{};
                    d.n_rows = 1 + uint32_t(rng.below(8192));
                    if (rng.below(4) == 0) d.n_rows = 8192;
                    d.sst_id = uint32_t(s);
                    d.row_base = sst_rows[s];
                    d.series_off = (rgs.size() + 1) << 20;
                    d.next_rg = r + 1 < n_rg ? int32_t(rgs.size()) + 1 : -1;
                    sst_rows[s] += d.n_rows;
                    // off doubles as the row group's identity below
                    valid.push_back({(rgs.size() + 1) << 20, 0});
                    rgs.push_back(d);
                }
            }
            const std::vector<hx::RgDesc> orig = rgs;
            hx::SstRgLists lists;
            hx::slice_and_order(rgs, valid, n_ssts, split, lists);
            std::string why;
            if (valid.size() != rgs.size() || lists.rgs.size() != rgs.size())
                why = "sizes";
            size_t listed = 0;
            for (size_t s = 0; s < n_ssts && why.empty(); s++) {
                // the list: this SST's units in row order
                int64_t row = 0;
                for (int32_t i = 0; i < lists.cnt[s]; i++) {
                    const hx::RgDesc& u = rgs[lists.rgs[lists.off[s] + i]];
                    if (u.sst_id != s || u.row_base != row) why = "list order";
                    row += u.n_rows;
                }
                if (row != sst_rows[s]) why = "list rows";
                listed += size_t(lists.cnt[s]);
                // the chain: rows 0..n contiguously, each unit once
                row = 0;
                int32_t at = lists.rgs[lists.off[s]], steps = 0;
                for (; at >= 0 && steps <= lists.cnt[s]; steps++) {
                    const hx::RgDesc& u = rgs[at];
                    if (u.sst_id != s || u.row_base != row) why = "chain";
                    row += u.n_rows;
                    at = u.next_rg;
                }
                if (row != sst_rows[s] || steps != lists.cnt[s])
                    why = "chain length";
            }
            if (why.empty() && listed != rgs.size()) why = "list counts";
            for (size_t i = 0; i < rgs.size() && why.empty(); i++) {
                const hx::RgDesc& o = orig[(valid[i].off >> 20) - 1];
                if (valid[i].bit != uint64_t(rgs[i].row_base - o.row_base) ||
                    rgs[i].series_off != o.series_off + valid[i].bit * 8 ||
                    rgs[i].sst_id != o.sst_id)
                    why = "slice start";
            }
            if (!why.empty()) {
                bad++;
                report("slice_and_order seed " + std::to_string(seed) +
                           " split " + std::to_string(split) + " (" + why + ")",
                       false);
            }
        }
    }
    report("slice_and_order over " + std::to_string(layouts) +
               " random layouts", bad == 0);
}

}  // namespace

int main(int argc, char** argv) {
#if defined(__SANITIZE_ADDRESS__)
    std::printf("stage_check: ASan+UBSan build\n");
#else
    std::printf("stage_check: plain build (bounds assertions only)\n");
#endif
    check_slicing();
    uint64_t seed = 1;
    for (int i = 1; i < argc; i++) {
        std::string path = argv[i];
        const bool fuzz = path.rfind("fuzz:", 0) == 0;
        const bool tight = path.rfind("tight:", 0) == 0;
        if (fuzz || tight) path = path.substr(path.find(':') + 1);
        std::vector<uint8_t> data;
        std::vector<Chunk> chunks;
        bool ok = false;
        try {
            ok = load(path, data, chunks);
        } catch (const std::exception& e) {
            std::printf("%s: %s\n", path.c_str(), e.what());
        }
        if (!ok || chunks.empty()) {
            report("load " + path, false);
            continue;
        }
        // the unmutated chunks must stage, so nothing below can pass by
        // refusing everything
        bool staged = true;
        for (const Chunk& k : chunks) staged = stage_plain(k) && staged;
        if (fuzz && staged) {
            Tally t;
            for (const Chunk& k : chunks) fuzz_chunk(k, seed++, t);
            std::printf("hostile %s: %d mutations, %d staged, %d refused\n",
                        chunks[0].file.c_str(),
                        t.staged + t.refused + t.broken, t.staged, t.refused);
            report("hostile " + chunks[0].file + " stays in bounds",
                   t.broken == 0 && t.staged + t.refused >= 2000);
        }
        if (tight && staged) {
            int n = 0;
            for (const Chunk& k : chunks) n += tight_chunk(k);
            report("tight " + chunks[0].file + " has a case", n > 0);
        }
    }
    if (g_fail) {
        std::printf("%d FAILED\n", g_fail);
        return 1;
    }
    std::printf("ALL OK\n");
    return 0;
}
