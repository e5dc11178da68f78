// ba_snappy_check.cpp — stand-alone host check of the Snappy path of Binary
// value stores: page images (ba_pages.h) -> hx::ba_page_minmax_host against
// the writer's full walk of the image -> hx::snappy_compress_host -> a
// decoder of its own, all required equal; the Binary-value writer under codec
// Snappy with ready streams against the (bytes, offsets) route; and
// hx::stage_chunk over one stored and one decoded Snappy value page of such a
// file. Built by `make ba_snappy_check` with -fsanitize=address,undefined when
// the runtime is available; every buffer handed to the code under test is an
// exact-size heap allocation. Prints one line per case, "all ok" last; exits
// non-zero on any mismatch.
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <unistd.h>
#include <vector>

#include "ba_pages.h"
#include "parquet_meta.h"
#include "parquet_writer.h"
#include "snappy_compress.h"
#include "stage_chunk.h"

namespace {

int g_fail = 0;

void report(const std::string& name, bool ok) {
    std::printf("%-56s %s\n", name.c_str(), ok ? "ok" : "FAIL");
    if (!ok) g_fail++;
}

uint64_t g_rng = 0x9E3779B97F4A7C15ull;
uint64_t rnd() {  // xorshift64*
    g_rng ^= g_rng >> 12;
    g_rng ^= g_rng << 25;
    g_rng ^= g_rng >> 27;
    return g_rng * 0x2545F4914F6CDD1Dull;
}

typedef std::vector<std::string> Values;

// the values as one source with handles, then the twin's two passes
struct Built {
    std::unique_ptr<uint8_t[]> src, image;
    std::unique_ptr<uint64_t[]> handles, page_off;
    std::unique_ptr<uint32_t[]> row_len;
    uint64_t n = 0, n_pages = 0, total = 0, R = 0;
};

Built build(const Values& v, uint64_t R) {
    Built b;
    b.n = v.size();
    b.R = R;
    uint64_t bytes = 0;
    for (const auto& s : v) bytes += s.size();
    b.src.reset(new uint8_t[bytes ? bytes : 1]);
    b.handles.reset(new uint64_t[b.n]);
    uint64_t off = 0;
    for (uint64_t i = 0; i < b.n; i++) {
        if (!v[i].empty()) std::memcpy(b.src.get() + off, v[i].data(), v[i].size());
        b.handles[i] = (off << hx::BA_LEN_BITS) | v[i].size();
        off += v[i].size();
    }
    b.n_pages = hx::ba_n_pages(b.n, R);
    b.page_off.reset(new uint64_t[b.n_pages + 1]);
    b.row_len.reset(new uint32_t[b.n]);
    hx::ba_page_sizes_host(bytes, b.handles.get(), b.n, nullptr, b.n, R,
                           b.row_len.get(), b.page_off.get());
    b.total = b.page_off[b.n_pages];
    b.image.reset(new uint8_t[b.total ? b.total : 1]);
    hx::ba_build_pages_host(b.src.get(), bytes, b.handles.get(), b.n, nullptr,
                            b.n, R, b.row_len.get(), b.page_off.get(),
                            b.image.get());
    return b;
}

// the writer's rule: a full walk of the page image
hx::BaPageStat full_walk(const uint8_t* page, uint64_t len, uint64_t rows) {
    hx::BaPageStat st;
    std::memset(&st, 0, sizeof st);
    const uint8_t *mn = nullptr, *mx = nullptr;
    uint32_t mn_len = 0, mx_len = 0;
    auto less = [](const uint8_t* a, uint32_t al, const uint8_t* b,
                   uint32_t bl) {
        const int k = std::memcmp(a, b, al < bl ? al : bl);
        return k < 0 || (k == 0 && al < bl);
    };
    uint64_t pos = 0;
    for (uint64_t r = 0; r < rows; r++) {
        uint32_t l;
        std::memcpy(&l, page + pos, 4);
        pos += 4;
        const uint8_t* v = page + pos;
        if (r == 0 || less(v, l, mn, mn_len)) mn = v, mn_len = l;
        if (r == 0 || less(mx, mx_len, v, l)) mx = v, mx_len = l;
        pos += l;
    }
    if (pos != len) g_fail++;
    if (mn_len <= 64 && mx_len <= 64) {
        st.has = 1;
        st.min_len = mn_len;
        st.max_len = mx_len;
        std::memcpy(st.min, mn, mn_len);
        std::memcpy(st.max, mx, mx_len);
    }
    return st;
}

// Snappy decoder of its own (format description: literals, 1-, 2- and 4-byte
// offset copies); false on any malformed element. out: exactly `want` bytes.
bool decode(const uint8_t* s, size_t n, std::vector<uint8_t>& out,
            size_t want) {
    size_t pos = 0, ulen = 0;
    for (int sh = 0;; sh += 7) {
        if (pos >= n || sh > 28) return false;
        const uint8_t b = s[pos++];
        ulen |= size_t(b & 0x7F) << sh;
        if (!(b & 0x80)) break;
    }
    if (ulen != want) return false;
    out.clear();
    out.reserve(ulen);
    while (pos < n) {
        const uint8_t tag = s[pos++];
        if ((tag & 3) == 0) {
            size_t len = (tag >> 2) + 1;
            if (len > 60) {
                const size_t nb = len - 60;
                if (pos + nb > n) return false;
                len = 0;
                for (size_t k = 0; k < nb; k++) len |= size_t(s[pos + k]) << (8 * k);
                len += 1;
                pos += nb;
            }
            if (pos + len > n) return false;
            out.insert(out.end(), s + pos, s + pos + len);
            pos += len;
            continue;
        }
        size_t len, off;
        if ((tag & 3) == 1) {
            if (pos + 1 > n) return false;
            len = 4 + ((tag >> 2) & 7);
            off = (size_t(tag >> 5) << 8) | s[pos];
            pos += 1;
        } else if ((tag & 3) == 2) {
            if (pos + 2 > n) return false;
            len = (tag >> 2) + 1;
            off = s[pos] | size_t(s[pos + 1]) << 8;
            pos += 2;
        } else {
            return false;   // never emitted
        }
        if (off == 0 || off > out.size()) return false;
        for (size_t k = 0; k < len; k++) out.push_back(out[out.size() - off]);
    }
    return out.size() == want;
}

std::string rand_bytes(size_t n, uint32_t lo = 0, uint32_t span = 256) {
    std::string s(n, '\0');
    for (auto& c : s) c = char(lo + rnd() % span);
    return s;
}

struct Case {
    std::string name;
    Values v;
    uint64_t R;
};

std::vector<Case> shapes() {
    std::vector<Case> out;
    for (uint64_t n : {1u, 63u, 64u, 65u, 255u, 256u, 257u, 8191u, 8192u,
                       8193u}) {
        Values v;
        for (uint64_t i = 0; i < n; i++) v.push_back(rand_bytes(rnd() % 21));
        out.push_back({"rows " + std::to_string(n), v, 8192});
    }
    out.push_back({"all equal", Values(300, "same value"), 8192});
    {
        Values v;
        for (int i = 0; i < 500; i++) v.push_back(rand_bytes(1 + rnd() % 12));
        v[123] = "";
        out.push_back({"empty value is the min", v, 8192});
    }
    out.push_back({"bytes >= 0x80",
                   {"\x7f\xff", "\x80", "\xff", std::string("\x00\xff", 2),
                    "\xfe\xff\xff"}, 8192});
    for (int where : {0, 300, 599})
        for (int mx = 0; mx < 2; mx++) {
            Values v;
            for (int i = 0; i < 600; i++)
                v.push_back("\x40" + rand_bytes(rnd() % 11));
            v[where] = mx ? std::string(9, '\xfe') : std::string("\x01");
            out.push_back({std::string(mx ? "max" : "min") + " at row " +
                               std::to_string(where), v, 8192});
        }
    for (size_t p : {63u, 64u, 65u, 66u}) {
        const std::string pre = rand_bytes(p);
        Values v;
        for (int k = 0; k < 20; k++)
            for (int b : {7, 3, 200, 3, 9})
                v.push_back(pre + char(b) + "tail");
        out.push_back({"shared prefix " + std::to_string(p), v, 8192});
        v.insert(v.begin(), std::string(1, '\0'));
        v.push_back("\xff\xff");
        out.push_back({"shared prefix " + std::to_string(p) + ", short bounds",
                       v, 8192});
    }
    out.push_back({"min of 64 bytes kept",
                   {std::string(64, 'a'), "b", std::string(64, 'a') + "z"},
                   8192});
    out.push_back({"min of 65 bytes omitted",
                   {std::string(65, 'a'), "b", std::string(65, 'a') + "z"},
                   8192});
    out.push_back({"short min, 70-byte max",
                   {"b", std::string(70, 'z'), "c"}, 8192});
    out.push_back({"65-byte key ties",
                   {std::string(65, 'm'), std::string(66, 'm'),
                    std::string(64, 'm'), std::string(200, 'm')}, 8192});
    out.push_back({"one value of 2^20 - 1 bytes",
                   {"k", rand_bytes(hx::BA_MAX_VALUE_LEN, 1, 254),
                    std::string("\x00q", 2)}, 8192});
    {
        Values v;
        const std::string pre = "0123456789abcdefghijklmnopqrs";
        for (int i = 0; i < 400; i++)
            v.push_back(pre.substr(0, 8 + (i * 5) % 21) +
                        std::string(i % 8, char(i % 251)));
        out.push_back({"every start alignment", v, 128});
    }
    {
        Values v;   // text-like: compresses, several pages
        for (int i = 0; i < 3000; i++)
            v.push_back("host=web-" + std::to_string(i % 17) +
                        ",region=eu-west-" + std::to_string(i % 3));
        out.push_back({"compressible text", v, 1024});
    }
    return out;
}

void check_shapes() {
    for (const Case& c : shapes()) {
        Built b = build(c.v, c.R);
        std::unique_ptr<hx::BaPageStat[]> st(new hx::BaPageStat[b.n_pages]);
        hx::ba_page_minmax_host(b.image.get(), b.page_off.get(),
                                b.row_len.get(), b.n, c.R, st.get());
        bool stats_ok = true, codec_ok = true;
        for (uint64_t g = 0; g < b.n_pages; g++) {
            const uint64_t len = b.page_off[g + 1] - b.page_off[g];
            const uint64_t rows =
                (g + 1) * c.R < b.n ? c.R : b.n - g * c.R;
            // the page as an exact-size block of its own
            std::unique_ptr<uint8_t[]> page(new uint8_t[len]);
            std::memcpy(page.get(), b.image.get() + b.page_off[g], len);
            const hx::BaPageStat want = full_walk(page.get(), len, rows);
            stats_ok = stats_ok && !std::memcmp(&want, &st[g], sizeof want);
            const size_t cap = size_t(hx::snappy_max_compressed(len));
            std::unique_ptr<uint8_t[]> comp(new uint8_t[cap]);
            const size_t got =
                hx::snappy_compress_host(page.get(), len, comp.get(), cap);
            std::unique_ptr<uint8_t[]> exact(new uint8_t[got ? got : 1]);
            std::memcpy(exact.get(), comp.get(), got);
            std::vector<uint8_t> back;
            codec_ok = codec_ok && got > 0 &&
                       decode(exact.get(), got, back, len) &&
                       !std::memcmp(back.data(), page.get(), len);
        }
        report(c.name + ": statistics == full walk", stats_ok);
        report(c.name + ": stream decodes to the image", codec_ok);
    }
    // a refused row is an empty value
    {
        Built b = build({"bb", "a", "cc"}, 8192);
        b.row_len[1] = hx::BA_ROW_SKIP;
        const uint8_t img[] = {2, 0, 0, 0, 'b', 'b', 0, 0, 0, 0,
                               2, 0, 0, 0, 'c', 'c'};
        const uint64_t off[2] = {0, sizeof img};
        hx::BaPageStat st;
        hx::ba_page_minmax_host(img, off, b.row_len.get(), 3, 8192, &st);
        report("refused row counts as the empty value",
               st.has == 1 && st.min_len == 0 && st.max_len == 2 &&
                   !std::memcmp(st.max, "cc", 2));
    }
}

std::vector<uint8_t> slurp(const std::string& path) {
    std::vector<uint8_t> v;
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) return v;
    fseek(f, 0, SEEK_END);
    v.resize((size_t)ftell(f));
    fseek(f, 0, SEEK_SET);
    if (!v.empty() && fread(v.data(), 1, v.size(), f) != v.size()) v.clear();
    fclose(f);
    return v;
}

// One staging attempt of the value chunk of row group g: exact-size blocks.
struct Staged {
    hx::StageStatus st;
    hx::StagedPages pages;
    hx::ChunkResult res;
    std::unique_ptr<uint8_t[]> mem;
    size_t cap = 0, tail_end = 0;
};
constexpr uint64_t kSlotOff = 0x40000, kTail = 0x100000;

Staged stage_value(const std::vector<uint8_t>& file,
                   const hx::ColumnChunkMeta& c, bool with_tail,
                   int64_t claim_uncomp = -1) {
    hx::ChunkRef cr;
    cr.codec = c.codec;
    cr.required = true;
    cr.chunk_start = c.chunk_start();
    cr.comp_size = c.total_compressed_size;
    cr.uncomp_size = claim_uncomp >= 0 ? claim_uncomp
                                       : c.total_uncompressed_size;
    cr.num_values = c.num_values;
    std::unique_ptr<uint8_t[]> chunk(new uint8_t[size_t(cr.comp_size)]);
    std::memcpy(chunk.get(), file.data() + cr.chunk_start,
                size_t(cr.comp_size));
    Staged s;
    s.cap = hx::chunk_reserve(cr);
    s.mem.reset(new uint8_t[s.cap]);
    std::memset(s.mem.get(), 0xA5, s.cap);
    hx::ChunkSlot slot;
    slot.base = s.mem.get();
    slot.off = kSlotOff;
    slot.cap = s.cap;
    hx::ChunkRole role;
    role.col = 2;
    role.bytes_value = true;
    std::atomic<size_t> dec{0}, tail{kTail};
    s.st = hx::stage_chunk(chunk.get(), cr, role, slot, dec, s.pages, s.res,
                           with_tail ? &tail : nullptr);
    s.tail_end = tail.load();
    return s;
}

void check_writer_and_staging() {
    // row group 0: random bytes (a stored page); row group 1: text
    const uint32_t R = 256, n = 2 * R;
    Values v;
    for (uint32_t i = 0; i < R; i++) v.push_back(rand_bytes(40 + rnd() % 40));
    for (uint32_t i = 0; i < R; i++)
        v.push_back("host=web-" + std::to_string(i % 17) + ",region=eu-west");
    Built b = build(v, R);
    std::unique_ptr<uint64_t[]> series(new uint64_t[n]);
    std::unique_ptr<int64_t[]> ts(new int64_t[n]);
    std::unique_ptr<int64_t[]> offs(new int64_t[n + 1]);
    offs[0] = 0;
    for (uint32_t i = 0; i < n; i++) {
        series[i] = i / 3;
        ts[i] = int64_t(i % 3) * 1000;
        offs[i + 1] = offs[i] + int64_t(v[i].size());
    }
    // ready streams + statistics, as the device routes bring them
    std::vector<std::vector<uint8_t>> streams(b.n_pages);
    std::unique_ptr<hx::BaPageStat[]> st(new hx::BaPageStat[b.n_pages]);
    hx::ba_page_minmax_host(b.image.get(), b.page_off.get(), b.row_len.get(),
                            n, R, st.get());
    std::vector<hx::PagePayload> ready(b.n_pages * 5, hx::PagePayload{});
    for (uint64_t g = 0; g < b.n_pages; g++) {
        const size_t len = size_t(b.page_off[g + 1] - b.page_off[g]);
        streams[g].resize(size_t(hx::snappy_max_compressed(len)));
        streams[g].resize(hx::snappy_compress_host(
            b.image.get() + b.page_off[g], len, streams[g].data(),
            streams[g].size()));
        ready[g * 5 + 2].ptr = streams[g].data();
        ready[g * 5 + 2].len = uint32_t(streams[g].size());
        ready[g * 5 + 2].ulen = uint32_t(len);
        ready[g * 5 + 2].ba_stat = &st[g];
    }
    char tmpl[] = "/tmp/ba_snappy_check_XXXXXX";
    if (!mkdtemp(tmpl)) {
        report("mkdtemp", false);
        return;
    }
    const std::string dir = tmpl;
    const std::string p1 = dir + "/a.sst", p2 = dir + "/b.sst",
                      p3 = dir + "/c.sst", p4 = dir + "/d.sst";
    std::string e1 = hx::write_metric_sst_bytes(
        p1, series.get(), ts.get(), b.src.get(), offs.get(), nullptr, 9, n, R,
        nullptr, 1);
    std::string e2 = hx::write_metric_sst_bytes(
        p2, series.get(), ts.get(), nullptr, nullptr, nullptr, 9, n, R,
        ready.data(), 1);
    std::vector<uint8_t> f1 = slurp(p1), f2 = slurp(p2);
    report("writer: ready streams == offsets route (Snappy)",
           e1.empty() && e2.empty() && !f1.empty() && f1 == f2);
    std::string e3 = hx::write_metric_sst_bytes(
        p3, series.get(), ts.get(), b.src.get(), offs.get(), nullptr, 9, n, R,
        nullptr, 0);
    std::string e4 = hx::write_metric_sst_bytes(
        p4, series.get(), ts.get(), b.src.get(), offs.get(), nullptr, 9, n, R);
    std::vector<uint8_t> f3 = slurp(p3), f4 = slurp(p4);
    report("writer: codec 0 is the file it always wrote",
           e3.empty() && e4.empty() && !f3.empty() && f3 == f4 &&
               f3.size() > f1.size());
    // a ready stream without statistics is refused, no file left
    ready[2].ba_stat = nullptr;
    std::string e5 = hx::write_metric_sst_bytes(
        p3, series.get(), ts.get(), nullptr, nullptr, nullptr, 9, n, R,
        ready.data(), 1);
    report("writer: ready stream without statistics refused",
           !e5.empty() && access(p3.c_str(), F_OK) != 0);

    try {
        hx::FileMetadata m = hx::parse_footer(f1.data(), f1.size(),
                                              (int64_t)f1.size());
        bool ok = m.row_groups.size() == 2;
        for (size_t g = 0; ok && g < 2; g++)
            for (int c = 0; c < 5; c++)
                ok = ok && m.row_groups[g].columns[c].codec == hx::CODEC_SNAPPY;
        for (size_t g = 0; ok && g < 2; g++) {
            const hx::ColumnChunkMeta& c = m.row_groups[g].columns[2];
            ok = c.has_stats == (st[g].has != 0) &&
                 c.stat_min == std::string((const char*)st[g].min,
                                           st[g].min_len) &&
                 c.stat_max == std::string((const char*)st[g].max,
                                           st[g].max_len);
        }
        report("writer: footer parses back, five Snappy chunks", ok);

        // the stored page: read in place, nothing decoded
        const hx::ColumnChunkMeta& c0 = m.row_groups[0].columns[2];
        const size_t len0 = size_t(b.page_off[1] - b.page_off[0]);
        Staged s0 = stage_value(f1, c0, true);
        ok = s0.st.ok() && s0.res.stored && s0.pages.snappy_ba.empty() &&
             s0.pages.snappy.empty() && s0.pages.pages_in_place == 1 &&
             s0.pages.bytes_in_place == len0 && s0.pages.ba.size() == 1 &&
             s0.tail_end == kTail;
        if (ok) {
            const hx::BaPageDesc& d = s0.pages.ba[0];
            ok = d.src_len == len0 && d.src_off >= kSlotOff &&
                 (d.src_off & 63) == 0 &&
                 d.src_off - kSlotOff + len0 <= s0.cap &&
                 !std::memcmp(s0.mem.get() + (d.src_off - kSlotOff),
                              b.image.get(), len0);
        }
        report("staging: stored value page read in place", ok);
        // and without a tail cursor, since it needs none
        Staged s0n = stage_value(f1, c0, false);
        report("staging: stored value page needs no tail", s0n.st.ok());

        // the compressed page: a piece of the tail, decoded there
        const hx::ColumnChunkMeta& c1 = m.row_groups[1].columns[2];
        const size_t len1 = size_t(b.page_off[2] - b.page_off[1]);
        Staged s1 = stage_value(f1, c1, true);
        ok = s1.st.ok() && !s1.res.stored && s1.pages.snappy.empty() &&
             s1.pages.snappy_ba.size() == 1 && s1.pages.ba.size() == 1 &&
             s1.pages.pages_in_place == 0 &&
             s1.tail_end == kTail + hx::align64(len1);
        if (ok) {
            const hx::SnappyPageDesc& sp = s1.pages.snappy_ba[0];
            const hx::BaPageDesc& d = s1.pages.ba[0];
            ok = sp.dst_off == kTail && sp.uncomp_len == len1 &&
                 sp.src_off == kSlotOff && sp.comp_len <= s1.cap &&
                 d.src_off == kTail && d.src_len == len1 &&
                 d.n_values == R;
            std::vector<uint8_t> back;
            ok = ok && decode(s1.mem.get(), sp.comp_len, back, len1) &&
                 !std::memcmp(back.data(), b.image.get() + b.page_off[1],
                              len1);
        }
        report("staging: Snappy value page decodes into the tail", ok);
        Staged s1n = stage_value(f1, c1, false);
        report("staging: no tail cursor, Snappy value page refused",
               !s1n.st.ok() && s1n.st.st == HX_ERR_UNSUPPORTED &&
                   s1n.pages.snappy_ba.empty());
        // a page claiming more than its chunk's footer declared
        Staged s1t = stage_value(f1, c1, true, int64_t(len1) - 1);
        report("staging: page above the chunk's declared size refused",
               !s1t.st.ok() && s1t.st.st == HX_ERR_FORMAT &&
                   s1t.tail_end == kTail && s1t.pages.snappy_ba.empty());
    } catch (const std::exception& e) {
        std::printf("  parse_footer: %s\n", e.what());
        report("writer: footer parses back", false);
    }
    for (const std::string& p : {p1, p2, p3, p4}) unlink(p.c_str());
    rmdir(dir.c_str());
}

}  // namespace

int main() {
    check_shapes();
    check_writer_and_staging();
    std::printf("%s\n", g_fail ? "FAILED" : "all ok");
    return g_fail ? 1 : 0;
}
