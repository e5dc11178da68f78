// ba_multipage_check.cpp — stand-alone host check (own main, no GPU) of value
// chunks that hold several data pages, built by
// `make ba_multipage_check` under ASan/UBSan:
//   - hand-built chunks of 1, 2 and 8 pages in every form (uncompressed, Zstd,
//     stored Snappy, decoded Snappy; data page v1 and v2; REQUIRED and
//     OPTIONAL) go through stage_chunk into a slot of exactly chunk_reserve
//     bytes; pages for the tail are decoded with hx_snappy_prefix into a tail
//     of exactly the claimed size, and a walk of the BaPageDescs must return
//     every value, with first_row advancing by the pages' rows;
//   - the refusals: a multi-page 8-byte column, a null in a later page, a
//     non-PLAIN page, a dictionary page, value counts that fall short of or
//     overshoot the chunk's, a tail claim above the footer's size, a slot
//     that is too small;
//   - the cut rule (ba_pages.h) against a row-by-row walk, and the writer
//     under a page limit read back through list_pages and stage_chunk.
#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstring>
#include <dlfcn.h>
#include <memory>
#include <string>
#include <unistd.h>
#include <vector>

#include "ba_pages.h"
#include "def_levels.h"
#include "parquet_meta.h"
#include "parquet_writer.h"
#include "snappy_compress.h"
#include "snappy_stored.h"
#include "stage_chunk.h"

namespace {

int g_fail = 0;
void report(const std::string& what, bool ok) {
    std::printf("%-64s %s\n", what.c_str(), ok ? "ok" : "FAIL");
    if (!ok) g_fail = 1;
}

uint64_t g_rng = 0x9E3779B97F4A7C15ull;
uint32_t rnd() {
    g_rng ^= g_rng << 13;
    g_rng ^= g_rng >> 7;
    g_rng ^= g_rng << 17;
    return uint32_t(g_rng >> 32);
}
std::string rand_bytes(size_t n) {
    std::string s(n, '\0');
    for (auto& c : s) c = char(rnd());
    return s;
}
std::string text(size_t n) {
    static const char* const w[4] = {"host=web-", "region=eu-west,", "dc=ams3,",
                                     "rack=17,"};
    std::string s;
    while (s.size() < n) s += w[rnd() % 4];
    s.resize(n);
    return s;
}

typedef size_t (*zstd_compress_fn)(void*, size_t, const void*, size_t, int);
typedef size_t (*zstd_bound_fn)(size_t);
zstd_compress_fn g_zc = nullptr;
zstd_bound_fn g_zb = nullptr;

// SNAPPY_FRAG: a Snappy stream as the Snappy library writes incompressible
// input, nothing but literals of at most one fragment each
enum Form { UNC, ZSTD, SNAPPY, SNAPPY_FRAG };
constexpr size_t kFragment = 1000;
using Values = std::vector<std::string>;

void put_varint(std::vector<uint8_t>& o, uint64_t v) {
    while (v >= 0x80) {
        o.push_back(uint8_t(v) | 0x80);
        v >>= 7;
    }
    o.push_back(uint8_t(v));
}
void put_i32(std::vector<uint8_t>& o, int delta, int64_t v) {
    o.push_back(uint8_t(delta << 4) | 5);
    put_varint(o, (uint64_t(v) << 1) ^ uint64_t(v >> 63));
}

std::vector<uint8_t> compress(Form f, const std::vector<uint8_t>& raw) {
    std::vector<uint8_t> out;
    if (f == UNC) return raw;
    if (f == SNAPPY_FRAG) {
        put_varint(out, raw.size());
        for (size_t at = 0; at < raw.size(); at += kFragment) {
            const size_t len = std::min(kFragment, raw.size() - at);
            if (len <= 60) {
                out.push_back(uint8_t((len - 1) << 2));
            } else {
                out.push_back(uint8_t(61 << 2));   // two length bytes
                out.push_back(uint8_t(len - 1));
                out.push_back(uint8_t((len - 1) >> 8));
            }
            out.insert(out.end(), raw.begin() + at, raw.begin() + at + len);
        }
        return out;
    }
    if (f == SNAPPY) {
        out.resize(size_t(hx::snappy_max_compressed(raw.size())));
        out.resize(hx::snappy_compress_host(raw.data(), raw.size(), out.data(),
                                            out.size()));
        return out;
    }
    out.resize(g_zb(raw.size()));
    out.resize(g_zc(out.data(), out.size(), raw.data(), raw.size(), 3));
    return out;
}

struct PageOpt {
    int32_t encoding = 0;
    int null_at = -1;        // OPTIONAL: this row of the page is null
    int64_t claim_values = -1;
};

// one data page (header + payload) appended to `chunk`
void add_page(std::vector<uint8_t>& chunk, const Values& vals, Form f, bool v2,
              bool optional, const PageOpt& po = PageOpt{}) {
    const uint32_t n = uint32_t(vals.size());
    std::vector<uint8_t> body, lv;
    for (uint32_t i = 0; i < n; i++) {
        if (int(i) == po.null_at) continue;
        const uint32_t len = uint32_t(vals[i].size());
        for (int b = 0; b < 4; b++) body.push_back(uint8_t(len >> (8 * b)));
        body.insert(body.end(), vals[i].begin(), vals[i].end());
    }
    if (optional) {
        std::vector<uint64_t> words((n + 63) / 64 + 1, 0);
        uint32_t nv = 0;
        for (uint32_t i = 0; i < n; i++)
            if (int(i) != po.null_at) {
                words[i >> 6] |= 1ull << (i & 63);
                nv++;
            }
        hx::encode_def_levels(words.data(), n, nv, lv);
    }
    std::vector<uint8_t> hdr, payload;
    const int64_t nvals = po.claim_values >= 0 ? po.claim_values : n;
    if (!v2) {
        std::vector<uint8_t> raw = lv;
        raw.insert(raw.end(), body.begin(), body.end());
        payload = compress(f, raw);
        put_i32(hdr, 1, 0);
        put_i32(hdr, 1, int64_t(raw.size()));
        put_i32(hdr, 1, int64_t(payload.size()));
        hdr.push_back(uint8_t(2 << 4) | 12);   // field 5: DataPageHeader
        put_i32(hdr, 1, nvals);
        put_i32(hdr, 1, po.encoding);
        put_i32(hdr, 1, 3);
        put_i32(hdr, 1, 3);
        hdr.push_back(0);
    } else {
        // levels outside the compressed region, without the length prefix
        std::vector<uint8_t> l2(lv.begin() + (lv.empty() ? 0 : 4), lv.end());
        std::vector<uint8_t> comp = compress(f, body);
        payload = l2;
        payload.insert(payload.end(), comp.begin(), comp.end());
        put_i32(hdr, 1, 3);
        put_i32(hdr, 1, int64_t(l2.size() + body.size()));
        put_i32(hdr, 1, int64_t(payload.size()));
        hdr.push_back(uint8_t(5 << 4) | 12);   // field 8: DataPageHeaderV2
        put_i32(hdr, 1, nvals);
        put_i32(hdr, 1, po.null_at >= 0 ? 1 : 0);
        put_i32(hdr, 1, nvals);
        put_i32(hdr, 1, po.encoding);
        put_i32(hdr, 1, int64_t(l2.size()));
        put_i32(hdr, 1, 0);
        hdr.push_back(uint8_t(1 << 4) | (f == UNC ? 2 : 1));  // is_compressed
        hdr.push_back(0);
    }
    hdr.push_back(0);
    chunk.insert(chunk.end(), hdr.begin(), hdr.end());
    chunk.insert(chunk.end(), payload.begin(), payload.end());
}

void add_dict_page(std::vector<uint8_t>& chunk) {
    std::vector<uint8_t> hdr;
    put_i32(hdr, 1, 2);
    put_i32(hdr, 1, 5);
    put_i32(hdr, 1, 5);
    hdr.push_back(uint8_t(4 << 4) | 12);       // field 7: DictionaryPageHeader
    put_i32(hdr, 1, 1);
    put_i32(hdr, 1, 0);
    hdr.push_back(0);
    hdr.push_back(0);
    chunk.insert(chunk.end(), hdr.begin(), hdr.end());
    const uint8_t one[5] = {1, 0, 0, 0, 'x'};
    chunk.insert(chunk.end(), one, one + 5);
}

constexpr uint64_t kSlotOff = 0x40000, kTail = 0x4000000;
constexpr int64_t kChunkStart = 4096;

struct Staged {
    hx::StageStatus st;
    hx::StagedPages pages;
    hx::ChunkResult res;
    std::unique_ptr<uint8_t[]> slot;
    size_t cap = 0, tail_end = 0;
};

hx::ChunkRef chunk_ref(const std::vector<uint8_t>& chunk, Form f,
                       bool optional, int64_t num_values,
                       int64_t uncomp_size) {
    hx::ChunkRef cr;
    cr.codec = f == UNC ? hx::CODEC_UNCOMPRESSED
                        : f == ZSTD ? hx::CODEC_ZSTD : hx::CODEC_SNAPPY;
    cr.required = !optional;
    cr.chunk_start = kChunkStart;
    cr.comp_size = int64_t(chunk.size());
    cr.uncomp_size = uncomp_size;
    cr.num_values = num_values;
    return cr;
}

Staged stage(const std::vector<uint8_t>& chunk, const hx::ChunkRef& cr,
             int col = 2, size_t cap_cut = 0, int64_t row_base = 100,
             bool with_tail = true) {
    Staged s;
    s.cap = hx::chunk_reserve(cr) - cap_cut;
    s.slot.reset(new uint8_t[s.cap ? s.cap : 1]);
    std::memset(s.slot.get(), 0xA5, s.cap);
    std::unique_ptr<uint8_t[]> buf(new uint8_t[chunk.size()]);   // exact size
    std::memcpy(buf.get(), chunk.data(), chunk.size());
    hx::ChunkSlot slot;
    slot.base = s.slot.get();
    slot.off = kSlotOff;
    slot.cap = s.cap;
    hx::ChunkRole role;
    role.col = col;
    role.bytes_value = true;
    role.row_base = row_base;
    role.bytes_handles = 8000;
    std::atomic<size_t> dec{0}, tail{kTail};
    s.st = hx::stage_chunk(buf.get(), cr, role, slot, dec, s.pages, s.res,
                           with_tail ? &tail : nullptr);
    s.tail_end = tail.load();
    return s;
}

// decode the tail pages on the host and walk the descriptors: every value
bool walk(const Staged& s, const std::vector<Values>& pages, int64_t row_base,
          size_t* n_tail, size_t* n_in_place) {
    std::unique_ptr<uint8_t[]> tail(
        new uint8_t[s.tail_end - kTail ? s.tail_end - kTail : 1]);
    size_t tail_need = 0;
    for (const hx::SnappyPageDesc& sp : s.pages.snappy_ba) {
        if (sp.src_off < kSlotOff || (sp.src_off & 7) ||
            sp.src_off - kSlotOff + sp.comp_len > s.cap)
            return false;
        if (sp.dst_off < kTail || (sp.dst_off & 63) ||
            sp.dst_off + sp.uncomp_len > s.tail_end)
            return false;
        if (hx_snappy_prefix(s.slot.get() + (sp.src_off - kSlotOff),
                             sp.comp_len, tail.get() + (sp.dst_off - kTail),
                             sp.uncomp_len) != long(sp.uncomp_len))
            return false;
        tail_need += hx::align64(sp.uncomp_len);
    }
    if (s.tail_end - kTail != tail_need) return false;
    *n_tail = s.pages.snappy_ba.size();
    *n_in_place = size_t(s.pages.pages_in_place);
    std::vector<const Values*> live;
    for (const Values& v : pages)
        if (!v.empty()) live.push_back(&v);
    if (s.pages.ba.size() != live.size()) return false;
    int64_t row = 8000 / 8 + row_base;
    for (size_t k = 0; k < live.size(); k++) {
        const hx::BaPageDesc& d = s.pages.ba[k];
        const Values& v = *live[k];
        if (d.first_row != row || d.n_values != v.size()) return false;
        row += int64_t(v.size());
        const uint8_t* p;
        if (d.src_off >= kTail) {
            if (d.src_off + d.src_len > s.tail_end) return false;
            p = tail.get() + (d.src_off - kTail);
        } else {
            if (d.src_off < kSlotOff ||
                d.src_off - kSlotOff + d.src_len > s.cap)
                return false;
            p = s.slot.get() + (d.src_off - kSlotOff);
        }
        size_t pos = 0;
        for (const std::string& x : v) {
            if (pos + 4 > d.src_len) return false;
            uint32_t len;
            std::memcpy(&len, p + pos, 4);
            pos += 4;
            if (len != x.size() || len > d.src_len - pos ||
                (len && std::memcmp(p + pos, x.data(), len)))
                return false;
            pos += len;
        }
        if (pos != d.src_len) return false;
    }
    return true;
}

// page shapes: unequal row counts, empty values, one value longer than the
// others together
std::vector<Values> make_pages(int k, bool random) {
    std::vector<Values> pages(k);
    for (int p = 0; p < k; p++) {
        const uint32_t rows = p == 0 ? 37 : 5 + (rnd() % 60) + (p == 1 ? 300 : 0);
        for (uint32_t i = 0; i < rows; i++) {
            // random values of 300 bytes and more: below that the repeating
            // length prefixes still compress and the page is not stored
            const size_t len = (i % 7 == 3) ? 0
                               : random     ? 300 + rnd() % 120
                                            : 40 + rnd() % 120;
            pages[p].push_back(random ? rand_bytes(len) : text(len));
        }
    }
    // the last page: one value longer than everything else in the chunk
    size_t total = 0;
    for (const Values& v : pages)
        for (const std::string& x : v) total += x.size();
    pages[k - 1][pages[k - 1].size() / 2] =
        random ? rand_bytes(total + 1) : text(total + 1);
    return pages;
}

int64_t uncomp_total(const std::vector<Values>& pages) {
    int64_t t = 0;
    for (const Values& v : pages) {
        t += 64;   // header and levels, generously
        for (const std::string& x : v) t += 4 + int64_t(x.size());
    }
    return t;
}

void check_forms() {
    const char* const fname[3] = {"uncompressed", "Zstd", "Snappy"};
    for (int k : {1, 2, 8})
        for (int f = 0; f < 3; f++)
            for (int random = 0; random < 2; random++)
                for (int v2 = 0; v2 < 2; v2++)
                    for (int optional = 0; optional < 2; optional++) {
                        if (f == ZSTD && !g_zc) continue;
                        if (f != SNAPPY && random) continue;
                        std::vector<Values> pages = make_pages(k, random);
                        std::vector<uint8_t> chunk;
                        int64_t n = 0;
                        for (const Values& v : pages) {
                            add_page(chunk, v, Form(f), v2, optional);
                            n += int64_t(v.size());
                        }
                        hx::ChunkRef cr = chunk_ref(chunk, Form(f), optional, n,
                                                    uncomp_total(pages));
                        Staged s = stage(chunk, cr);
                        size_t n_tail = 0, n_place = 0;
                        bool ok = s.st.ok() &&
                                  walk(s, pages, 100, &n_tail, &n_place);
                        if (ok && f == SNAPPY)
                            ok = random ? (n_place == size_t(k) && !n_tail &&
                                           s.res.stored)
                                        : (n_tail == size_t(k) && !n_place);
                        if (ok && f != SNAPPY) ok = !n_tail && !n_place;
                        ok = ok && s.res.n_valid == uint32_t(n);
                        report(std::string(fname[f]) +
                                   (f == SNAPPY ? (random ? " stored" : " tail")
                                                : "") +
                                   (v2 ? " v2" : " v1") +
                                   (optional ? " OPTIONAL " : " REQUIRED ") +
                                   std::to_string(k) + " page(s)" +
                                   (s.st.ok() ? "" : ": " + s.st.msg),
                               ok);
                    }
    // literal-only streams of many fragments: read in place, tags dropped
    for (int k : {1, 2, 8})
        for (int v2 = 0; v2 < 2; v2++)
            for (int optional = 0; optional < 2; optional++) {
                std::vector<Values> pages = make_pages(k, true);
                std::vector<uint8_t> chunk;
                int64_t n = 0;
                for (const Values& v : pages) {
                    add_page(chunk, v, SNAPPY_FRAG, v2, optional);
                    n += int64_t(v.size());
                }
                Staged s = stage(chunk, chunk_ref(chunk, SNAPPY_FRAG, optional,
                                                  n, uncomp_total(pages)));
                size_t n_tail = 0, n_place = 0;
                const bool ok = s.st.ok() &&
                                walk(s, pages, 100, &n_tail, &n_place) &&
                                n_place == size_t(k) && !n_tail &&
                                s.res.stored && s.tail_end == kTail &&
                                (s.pages.ba[0].src_off & 63) == 0;
                report(std::string("Snappy literal fragments") +
                           (v2 ? " v2" : " v1") +
                           (optional ? " OPTIONAL " : " REQUIRED ") +
                           std::to_string(k) + " page(s)" +
                           (s.st.ok() ? "" : ": " + s.st.msg),
                       ok);
            }
    {
        // the literal-only test itself: a copy element, a trailer, a short
        // stream and a wrong preamble are no such stream
        std::vector<uint8_t> raw(2500);
        for (auto& b : raw) b = uint8_t(rnd());
        std::vector<uint8_t> st = compress(SNAPPY_FRAG, raw);
        std::unique_ptr<uint8_t[]> in(new uint8_t[st.size() + 3]);
        std::unique_ptr<uint8_t[]> out(new uint8_t[raw.size()]);
        std::memcpy(in.get(), st.data(), st.size());
        bool ok = hx_snappy_literals_only(in.get(), st.size(), 2500,
                                          out.get()) &&
                  !std::memcmp(out.get(), raw.data(), raw.size()) &&
                  hx_snappy_literals_only(in.get(), st.size(), 2500, nullptr);
        ok = ok && !hx_snappy_literals_only(in.get(), st.size() - 1, 2500,
                                            nullptr) &&
             !hx_snappy_literals_only(in.get(), st.size(), 2499, nullptr) &&
             !hx_snappy_literals_only(in.get(), 0, 2500, nullptr);
        in[st.size()] = 0;   // one more literal of one byte: a trailer
        in[st.size() + 1] = 7;
        ok = ok && !hx_snappy_literals_only(in.get(), st.size() + 2, 2500,
                                            nullptr);
        in[2] = 0x15;        // the first element becomes a copy
        ok = ok && !hx_snappy_literals_only(in.get(), st.size(), 2500,
                                            nullptr);
        report("hx_snappy_literals_only: bodies out, malformed streams refused",
               ok);
    }
    // stored and decoded pages in one chunk, an empty page between them
    std::vector<Values> pages = make_pages(3, false);
    pages[1].clear();
    for (int i = 0; i < 50; i++) pages[1].push_back(rand_bytes(300));
    pages.insert(pages.begin() + 1, Values{});
    std::vector<uint8_t> chunk;
    int64_t n = 0;
    for (const Values& v : pages) {
        add_page(chunk, v, SNAPPY, false, true);
        n += int64_t(v.size());
    }
    Staged s = stage(chunk, chunk_ref(chunk, SNAPPY, true, n,
                                      uncomp_total(pages)));
    size_t n_tail = 0, n_place = 0;
    report("Snappy: stored and decoded pages mixed, a page of zero values",
           s.st.ok() && walk(s, pages, 100, &n_tail, &n_place) && n_tail == 2 &&
               n_place == 1 && !s.res.stored);
}

void check_refusals() {
    std::vector<Values> pages = make_pages(3, false);
    int64_t n = 0;
    for (const Values& v : pages) n += int64_t(v.size());
    auto build = [&](Form f, bool v2, bool optional, int bad_page,
                     const PageOpt& po) {
        std::vector<uint8_t> chunk;
        for (int p = 0; p < 3; p++)
            add_page(chunk, pages[p], f, v2, optional,
                     p == bad_page ? po : PageOpt{});
        return chunk;
    };
    {
        std::vector<uint8_t> c = build(UNC, false, false, -1, PageOpt{});
        Staged s = stage(c, chunk_ref(c, UNC, false, n, uncomp_total(pages)),
                         0);
        report("8-byte column of three pages: one-page contract kept",
               !s.st.ok() && s.st.st == HX_ERR_UNSUPPORTED &&
                   s.st.msg.find("expected one data page") == 0);
    }
    for (int f = 0; f < 3; f++)
        for (int v2 = 0; v2 < 2; v2++) {
            if (f == ZSTD && !g_zc) continue;
            PageOpt po;
            po.null_at = 3;
            std::vector<uint8_t> c = build(Form(f), v2, true, 2, po);
            Staged s = stage(c, chunk_ref(c, Form(f), true, n,
                                          uncomp_total(pages)));
            report(std::string("null in the last page refused, codec ") +
                       std::to_string(f) + (v2 ? " v2" : " v1"),
                   !s.st.ok() && s.st.st == HX_ERR_UNSUPPORTED &&
                       s.st.msg.find("column value: 1 null(s): nulls in a "
                                     "Binary value column") == 0 &&
                       s.pages.ba.empty() && s.pages.snappy_ba.empty() &&
                       (f == ZSTD || s.tail_end == kTail));
        }
    for (int f = 0; f < 3; f++) {
        if (f == ZSTD && !g_zc) continue;
        PageOpt po;
        po.encoding = hx::ENC_DELTA_LENGTH_BA;
        std::vector<uint8_t> c = build(Form(f), false, false, 1, po);
        Staged s = stage(c, chunk_ref(c, Form(f), false, n,
                                      uncomp_total(pages)));
        report("non-PLAIN page refused, codec " + std::to_string(f),
               !s.st.ok() && s.st.st == HX_ERR_UNSUPPORTED &&
                   s.st.msg.find("byte value columns support PLAIN") == 0 &&
                   s.pages.ba.empty() && s.pages.snappy_ba.empty() &&
                   s.tail_end == kTail);
    }
    {
        std::vector<uint8_t> c;
        add_dict_page(c);
        PageOpt po;
        po.encoding = hx::ENC_RLE_DICTIONARY;
        add_page(c, pages[0], UNC, false, false, po);
        Staged s = stage(c, chunk_ref(c, UNC, false, int64_t(pages[0].size()),
                                      uncomp_total(pages)));
        report("dictionary page in the chunk refused",
               !s.st.ok() && s.st.st == HX_ERR_UNSUPPORTED &&
                   s.st.msg.find("byte value columns support PLAIN") == 0);
    }
    {
        std::vector<uint8_t> c = build(SNAPPY, false, false, -1, PageOpt{});
        Staged lo = stage(c, chunk_ref(c, SNAPPY, false, n + 1,
                                       uncomp_total(pages)));
        report("pages short of the chunk's value count: HX_ERR_FORMAT",
               !lo.st.ok() && lo.st.st == HX_ERR_FORMAT &&
                   lo.pages.ba.empty() && lo.tail_end == kTail);
        Staged hi = stage(c, chunk_ref(c, SNAPPY, false, n - 1,
                                       uncomp_total(pages)));
        report("pages overshoot the chunk's value count: HX_ERR_FORMAT",
               !hi.st.ok() && hi.st.st == HX_ERR_FORMAT &&
                   hi.pages.ba.empty() && hi.pages.snappy_ba.empty() &&
                   hi.tail_end == kTail);
        // the pages' cumulative claim on the tail against the footer's size
        int64_t image = 0;
        for (const Values& v : pages)
            for (const std::string& x : v) image += 4 + int64_t(x.size());
        Staged fit = stage(c, chunk_ref(c, SNAPPY, false, n, image));
        Staged over = stage(c, chunk_ref(c, SNAPPY, false, n, image - 1));
        report("tail claim equal to the footer's size accepted", fit.st.ok());
        report("tail claim above the footer's size refused, nothing reserved",
               !over.st.ok() && over.st.st == HX_ERR_FORMAT &&
                   over.tail_end == kTail && over.pages.snappy_ba.empty() &&
                   over.pages.ba.empty());
        Staged nt = stage(c, chunk_ref(c, SNAPPY, false, n, image), 2, 0, 100,
                          false);
        report("no tail cursor: decoded Snappy pages refused",
               !nt.st.ok() && nt.st.st == HX_ERR_UNSUPPORTED &&
                   nt.pages.snappy_ba.empty());
    }
    {
        // every write is compared with the slot: 200 bytes short
        std::vector<uint8_t> c = build(UNC, false, false, -1, PageOpt{});
        Staged s = stage(c, chunk_ref(c, UNC, false, n, uncomp_total(pages)),
                         2, 200);
        report("slot below the chunk's bytes refused",
               !s.st.ok() && s.st.st == HX_ERR_FORMAT && s.pages.ba.empty());
    }
}

// the rule, row by row
std::vector<std::pair<uint32_t, uint64_t>> cut_walk(
    const std::vector<uint32_t>& row_len, uint32_t limit) {
    std::vector<std::pair<uint32_t, uint64_t>> pages;
    uint32_t rows = 0;
    uint64_t bytes = 0;
    const size_t n = row_len.size();
    for (size_t i = 0; i < n; i++) {
        rows++;
        bytes += 4 + ((row_len[i] & hx::BA_ROW_SKIP) ? 0u : row_len[i]);
        const bool batch_end = (i + 1) % 1024 == 0, last = i + 1 == n;
        if (last || (batch_end && limit && bytes >= limit)) {
            pages.push_back({rows, bytes});
            rows = 0;
            bytes = 0;
        }
    }
    return pages;
}

bool cut_case(const std::vector<uint32_t>& row_len, uint32_t limit) {
    const uint64_t n = row_len.size();
    const size_t nb = size_t(hx::ba_n_batches(n, n ? n : 1));
    std::unique_ptr<uint64_t[]> sums(new uint64_t[nb ? nb : 1]);
    std::unique_ptr<uint32_t[]> pr(new uint32_t[nb ? nb : 1]);
    std::unique_ptr<uint64_t[]> pb(new uint64_t[nb ? nb : 1]);
    std::unique_ptr<uint32_t[]> rl(new uint32_t[n ? n : 1]);
    if (n) std::memcpy(rl.get(), row_len.data(), n * 4);
    hx::ba_batch_sizes_host(rl.get(), n, n ? n : 1, sums.get());
    const uint32_t k = hx::ba_cut_pages(sums.get(), n, limit, pr.get(),
                                        pb.get());
    auto want = cut_walk(row_len, limit);
    if (k != want.size() || k > (n + 1023) / 1024) return false;
    for (uint32_t i = 0; i < k; i++)
        if (pr[i] != want[i].first || pb[i] != want[i].second || pr[i] == 0)
            return false;
    return true;
}

void check_cut_rule() {
    for (uint32_t n : {0u, 1u, 1023u, 1024u, 1025u, 8192u}) {
        std::vector<uint32_t> row_len(n);
        for (auto& l : row_len) l = rnd() % 40;
        for (uint32_t i = 5; i < n; i += 97) row_len[i] = hx::BA_ROW_SKIP;
        uint64_t first_batch = 0;
        for (uint32_t i = 0; i < n && i < 1024; i++)
            first_batch += 4 + ((row_len[i] & hx::BA_ROW_SKIP) ? 0 : row_len[i]);
        bool ok = cut_case(row_len, 0) && cut_case(row_len, 1) &&
                  cut_case(row_len, 4096) &&
                  cut_case(row_len, hx::BA_PAGE_LIMIT_MAX);
        // a limit hit exactly by the first batch, and one byte above it
        if (first_batch) {
            ok = ok && cut_case(row_len, uint32_t(first_batch)) &&
                 cut_case(row_len, uint32_t(first_batch) + 1);
            if (n > 1024) {
                auto at = cut_walk(row_len, uint32_t(first_batch));
                auto above = cut_walk(row_len, uint32_t(first_batch) + 1);
                ok = ok && at[0].first == 1024 && above[0].first > 1024;
            }
        }
        report("cut rule == row walk, " + std::to_string(n) + " rows", ok);
    }
    {
        std::vector<uint32_t> row_len(8192, 100);
        auto one = cut_walk(row_len, 0), all = cut_walk(row_len, 1),
             never = cut_walk(row_len, 8192 * 104 + 1);
        report("limit 0 and a limit never reached: one page; limit 1: a page "
               "a batch",
               cut_case(row_len, 1) && one.size() == 1 && never.size() == 1 &&
                   all.size() == 8 && one[0].first == 8192);
    }
    {
        // batch sums over row groups of a size that is no multiple of 1024
        const uint64_t n = 20000, R = 3000;
        std::unique_ptr<uint32_t[]> rl(new uint32_t[n]);
        for (uint64_t i = 0; i < n; i++)
            rl[i] = i % 31 == 0 ? hx::BA_ROW_SKIP : rnd() % 5000;
        const uint64_t nb = hx::ba_n_batches(n, R);
        std::unique_ptr<uint64_t[]> sums(new uint64_t[nb]);
        hx::ba_batch_sizes_host(rl.get(), n, R, sums.get());
        bool ok = nb == 6 * 3 + 2;
        uint64_t b = 0;
        for (uint64_t g0 = 0; g0 < n; g0 += R)
            for (uint64_t r0 = g0; r0 < std::min(n, g0 + R); r0 += 1024, b++) {
                uint64_t s = 0;
                for (uint64_t i = r0;
                     i < std::min(std::min(n, g0 + R), r0 + 1024); i++)
                    s += 4 + ((rl[i] & hx::BA_ROW_SKIP) ? 0 : rl[i]);
                ok = ok && b < nb && sums[b] == s;
            }
        report("batch sums, row groups of 3000 rows", ok && b == nb);
    }
}

std::vector<uint8_t> slurp(const std::string& p) {
    std::vector<uint8_t> v;
    if (FILE* f = fopen(p.c_str(), "rb")) {
        uint8_t buf[65536];
        size_t n;
        while ((n = fread(buf, 1, sizeof buf, f)) > 0)
            v.insert(v.end(), buf, buf + n);
        fclose(f);
    }
    return v;
}

void check_writer() {
    const uint32_t R = 4096, n = 2 * R + 500;
    Values v;
    for (uint32_t i = 0; i < n; i++)
        v.push_back(i < R ? rand_bytes(20 + rnd() % 20) : text(rnd() % 40));
    std::unique_ptr<uint64_t[]> series(new uint64_t[n]);
    std::unique_ptr<int64_t[]> ts(new int64_t[n]);
    std::unique_ptr<int64_t[]> offs(new int64_t[n + 1]);
    std::string bytes;
    offs[0] = 0;
    for (uint32_t i = 0; i < n; i++) {
        series[i] = i / 3;
        ts[i] = int64_t(i % 3) * 1000;
        bytes += v[i];
        offs[i + 1] = int64_t(bytes.size());
    }
    char tmpl[] = "/tmp/ba_multipage_check_XXXXXX";
    if (!mkdtemp(tmpl)) {
        report("mkdtemp", false);
        return;
    }
    const std::string dir = tmpl;
    for (int codec = 0; codec < 2; codec++) {
        const std::string p0 = dir + "/a.sst", p1 = dir + "/b.sst",
                          p2 = dir + "/c.sst";
        const uint32_t limit = 30000;
        std::string e0 = hx::write_metric_sst_bytes(
            p0, series.get(), ts.get(), (const uint8_t*)bytes.data(),
            offs.get(), nullptr, 9, n, R, nullptr, codec);
        std::string e1 = hx::write_metric_sst_bytes(
            p1, series.get(), ts.get(), (const uint8_t*)bytes.data(),
            offs.get(), nullptr, 9, n, R, nullptr, codec, limit);
        std::string e2 = hx::write_metric_sst_bytes(
            p2, series.get(), ts.get(), (const uint8_t*)bytes.data(),
            offs.get(), nullptr, 9, n, R, nullptr, codec,
            hx::BA_PAGE_LIMIT_MAX);
        std::vector<uint8_t> f0 = slurp(p0), f1 = slurp(p1), f2 = slurp(p2);
        report("writer: a limit never reached is the one-page file, codec " +
                   std::to_string(codec),
               e0.empty() && e2.empty() && !f0.empty() && f0 == f2);
        bool ok = e1.empty() && !f1.empty();
        try {
            hx::FileMetadata m0 = hx::parse_footer(f0.data(), f0.size(),
                                                   int64_t(f0.size()));
            hx::FileMetadata m = hx::parse_footer(f1.data(), f1.size(),
                                                  int64_t(f1.size()));
            ok = ok && m.row_groups.size() == 3;
            for (size_t g = 0; ok && g < 3; g++) {
                const hx::ColumnChunkMeta& c = m.row_groups[g].columns[2];
                const hx::ColumnChunkMeta& c0 = m0.row_groups[g].columns[2];
                const uint32_t r0 = uint32_t(g) * R;
                const uint32_t rows = std::min(R, n - r0);
                std::vector<uint32_t> rl(rows);
                for (uint32_t i = 0; i < rows; i++)
                    rl[i] = uint32_t(v[r0 + i].size());
                auto want = cut_walk(rl, limit);
                hx::ChunkPageList pl;
                hx::list_pages(f1.data() + c.chunk_start(),
                               size_t(c.total_compressed_size),
                               c.chunk_start(), c.num_values, false, c.codec,
                               &pl);
                // the short last row group never reaches the limit
                ok = pl.data.size() == want.size() &&
                     (want.size() > 1) == (g < 2) &&
                     c.num_values == rows && c.stat_min == c0.stat_min &&
                     c.stat_max == c0.stat_max && c.has_stats == c0.has_stats;
                std::vector<Values> pv;
                uint32_t at = r0;
                for (size_t k = 0; ok && k < want.size(); k++) {
                    ok = uint32_t(pl.data[k].num_values) == want[k].first &&
                         uint64_t(pl.data[k].uncompressed_size) ==
                             want[k].second;
                    pv.emplace_back(v.begin() + at,
                                    v.begin() + at + want[k].first);
                    at += want[k].first;
                }
                if (!ok) break;
                hx::ChunkRef cr;
                cr.codec = c.codec;
                cr.chunk_start = c.chunk_start();
                cr.comp_size = c.total_compressed_size;
                cr.uncomp_size = c.total_uncompressed_size;
                cr.num_values = c.num_values;
                std::vector<uint8_t> chunk(
                    f1.begin() + c.chunk_start(),
                    f1.begin() + c.chunk_start() + c.total_compressed_size);
                Staged s = stage(chunk, cr, 2, 0, 0);
                size_t n_tail = 0, n_place = 0;
                ok = s.st.ok() && walk(s, pv, 0, &n_tail, &n_place) &&
                     n_tail + n_place == (codec ? want.size() : 0);
            }
        } catch (const std::exception& e) {
            std::printf("  %s\n", e.what());
            ok = false;
        }
        report("writer: pages cut by the rule, staged back, codec " +
                   std::to_string(codec),
               ok);
        for (const std::string& p : {p0, p1, p2}) unlink(p.c_str());
    }
    std::string e = hx::write_metric_sst_bytes(
        dir + "/x.sst", series.get(), ts.get(), (const uint8_t*)bytes.data(),
        offs.get(), nullptr, 9, n, R, nullptr, 0, hx::BA_PAGE_LIMIT_MAX + 1);
    report("writer: a limit above 2^30 refused, no file left",
           !e.empty() && access((dir + "/x.sst").c_str(), F_OK) != 0);
    rmdir(dir.c_str());
}

}  // namespace

int main() {
    if (void* h = dlopen("libzstd.so.1", RTLD_NOW | RTLD_LOCAL)) {
        g_zc = (zstd_compress_fn)dlsym(h, "ZSTD_compress");
        g_zb = (zstd_bound_fn)dlsym(h, "ZSTD_compressBound");
        if (!g_zc || !g_zb) g_zc = nullptr;
    }
    if (!g_zc) std::printf("libzstd.so.1 not loadable: Zstd forms left out\n");
    check_forms();
    check_refusals();
    check_cut_rule();
    check_writer();
    std::printf("%s\n", g_fail ? "FAILED" : "all ok");
    return g_fail ? 1 : 0;
}
