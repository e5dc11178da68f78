// ba_pages_check.cpp — stand-alone host check of ba_pages.h (the host twin of
// kernel 1f) against a scalar construction of the page images, of its
// refusals, and of hx::write_metric_sst_bytes over its pages: the file parsed
// back with parquet_meta.cpp, and the ready route against the
// (bytes, offsets) route byte for byte. Built by `make ba_pages_check` with
// -fsanitize=address,undefined when the runtime is available; every buffer
// handed to the code under test is an exact-size heap allocation so a read or
// write outside it trips the sanitizer. Prints one line per case, exits
// non-zero on any mismatch.
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

namespace {

int g_fail = 0;

void report(const std::string& name, bool ok) {
    std::printf("%-52s %s\n", name.c_str(), ok ? "ok" : "FAIL");
    if (!ok) g_fail++;
}

uint64_t g_rng = 0x9E3779B97F4A7C15ull;
uint64_t rnd() {  // xorshift64*
    g_rng ^= g_rng >> 12;
    g_rng ^= g_rng << 25;
    g_rng ^= g_rng >> 27;
    return g_rng * 0x2545F4914F6CDD1Dull;
}

struct Source {
    std::unique_ptr<uint8_t[]> bytes;   // exact size
    uint64_t size = 0;
    std::unique_ptr<uint64_t[]> handles;
    uint64_t n = 0;
};

// rows of the given lengths, laid out back to back with `gap` unused bytes
// between them (so source offsets take every residue)
Source make_source(const std::vector<uint32_t>& lens, uint32_t gap) {
    Source s;
    s.n = lens.size();
    for (uint32_t l : lens) s.size += l + gap;
    s.bytes.reset(new uint8_t[s.size ? s.size : 1]);
    for (uint64_t i = 0; i < s.size; i++) s.bytes[i] = uint8_t(rnd());
    s.handles.reset(new uint64_t[s.n ? s.n : 1]);
    uint64_t off = 0;
    for (uint64_t i = 0; i < s.n; i++) {
        off += gap;
        s.handles[i] = (off << 20) | lens[i];
        off += lens[i];
    }
    return s;
}

// the page images by the definition: per output row u32 length + bytes
std::vector<uint8_t> scalar_image(const Source& s,
                                  const std::vector<uint32_t>* gs,
                                  uint64_t n_out) {
    std::vector<uint8_t> out;
    for (uint64_t i = 0; i < n_out; i++) {
        const uint64_t a = gs ? (*gs)[i] : i, b = gs ? (*gs)[i + 1] : i + 1;
        std::string v;
        for (uint64_t j = a; j < b; j++)
            v.append((const char*)s.bytes.get() + (s.handles[j] >> 20),
                     s.handles[j] & 0xFFFFF);
        const uint32_t len = (uint32_t)v.size();
        out.insert(out.end(), (const uint8_t*)&len, (const uint8_t*)&len + 4);
        out.insert(out.end(), v.begin(), v.end());
    }
    return out;
}

struct Built {
    hx::BaPagesCounts counts{};
    std::vector<uint64_t> page_off;
    std::unique_ptr<uint8_t[]> image;
    uint64_t total = 0;
};

Built build(const Source& s, const std::vector<uint32_t>* gs, uint64_t n_out,
            uint64_t R) {
    Built b;
    const uint64_t n_pages = hx::ba_n_pages(n_out, R);
    std::unique_ptr<uint32_t[]> row_len(new uint32_t[n_out ? n_out : 1]);
    std::unique_ptr<uint64_t[]> po(new uint64_t[n_pages + 1]);
    b.counts = hx::ba_page_sizes_host(s.size, s.handles.get(), s.n,
                                      gs ? gs->data() : nullptr, n_out, R,
                                      row_len.get(), po.get());
    b.page_off.assign(po.get(), po.get() + n_pages + 1);
    b.total = po[n_pages];
    b.image.reset(new uint8_t[b.total ? b.total : 1]);
    hx::ba_build_pages_host(s.bytes.get(), s.size, s.handles.get(), s.n,
                            gs ? gs->data() : nullptr, n_out, R,
                            row_len.get(), po.get(), b.image.get());
    return b;
}

bool same(const Built& b, const std::vector<uint8_t>& exp) {
    return b.total == exp.size() &&
           (exp.empty() || !std::memcmp(b.image.get(), exp.data(), exp.size()));
}

const uint32_t kLens[] = {0, 1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 255, 256,
                          4097};

void check_rows() {
    for (uint32_t n : {1u, 63u, 64u, 65u, 300u, 1000u}) {
        for (uint32_t gap : {0u, 1u, 7u}) {
            std::vector<uint32_t> lens(n);
            for (auto& l : lens) l = kLens[rnd() % 14];
            Source s = make_source(lens, gap);
            Built b = build(s, nullptr, n, 128);
            report("rows n=" + std::to_string(n) + " gap=" +
                       std::to_string(gap),
                   b.counts.n_errors == 0 && b.counts.n_over_cap == 0 &&
                       same(b, scalar_image(s, nullptr, n)));
        }
    }
    // one value at the limit
    Source s = make_source({5, (1u << 20) - 1, 0, 9}, 3);
    Built b = build(s, nullptr, 4, 8192);
    report("value of 2^20 - 1 bytes",
           b.counts.n_errors == 0 && same(b, scalar_image(s, nullptr, 4)));
}

void check_groups() {
    std::vector<uint32_t> lens(700);
    for (auto& l : lens) l = kLens[rnd() % 13];
    for (uint32_t i = 100; i < 140; i++) lens[i] = 0;   // an all-empty group
    Source s = make_source(lens, 5);
    std::vector<uint32_t> gs = {0};
    for (uint32_t sz : {1u, 2u, 63u, 34u, 40u, 64u, 65u, 300u, 1u, 130u})
        gs.push_back(gs.back() + sz);
    const uint64_t n_out = gs.size() - 1;
    Built b = build(s, &gs, n_out, 4);
    report("groups 1/2/63/64/65/300, empty group",
           gs.back() == 700 && b.counts.n_errors == 0 &&
               b.counts.n_over_cap == 0 && same(b, scalar_image(s, &gs, n_out)));

    // a group totalling exactly the limit, and one byte more
    for (uint32_t extra : {0u, 1u}) {
        Source t = make_source({1u << 19, (1u << 19) - 2 + extra, 1, 7}, 0);
        std::vector<uint32_t> g2 = {0, 3, 4};
        Built c = build(t, &g2, 2, 8192);
        if (!extra) {
            report("group total 2^20 - 1",
                   c.counts.n_over_cap == 0 &&
                       same(c, scalar_image(t, &g2, 2)));
        } else {
            // the refused row is written empty, the other one intact
            std::vector<uint8_t> exp = {0, 0, 0, 0, 7, 0, 0, 0};
            exp.insert(exp.end(), t.bytes.get() + (t.handles[3] >> 20),
                       t.bytes.get() + (t.handles[3] >> 20) + 7);
            report("group total 2^20 refused",
                   c.counts.n_over_cap == 1 && c.counts.n_errors == 0 &&
                       same(c, exp));
        }
    }
}

void check_refusals() {
    Source s = make_source({4, 4, 4, 4}, 0);
    s.handles[2] = (uint64_t(s.size - 3) << 20) | 4;   // 1 byte past the end
    Built b = build(s, nullptr, 4, 8192);
    std::vector<uint8_t> exp;
    for (int i = 0; i < 4; i++) {
        const uint32_t len = i == 2 ? 0 : 4;
        exp.insert(exp.end(), (const uint8_t*)&len, (const uint8_t*)&len + 4);
        if (len)
            exp.insert(exp.end(), s.bytes.get() + 4 * i,
                       s.bytes.get() + 4 * i + 4);
    }
    report("handle past the source end", b.counts.n_errors == 1 && same(b, exp));

    Source t = make_source({4, 4, 4, 4}, 0);
    std::vector<uint32_t> gs = {0, 3, 2, 4};   // decreasing
    Built c = build(t, &gs, 3, 8192);
    report("decreasing group_start", c.counts.n_errors == 1 &&
                                         c.total == 12 + 12 + 8);
    std::vector<uint32_t> g2 = {0, 2, 9};      // past the source rows
    Built d = build(t, &g2, 2, 8192);
    report("group_start past the source rows",
           d.counts.n_errors == 1 && d.total == 12 + 4);
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

void check_writer() {
    const uint32_t n = 300, R = 128;
    std::vector<uint32_t> lens(n);
    for (auto& l : lens) l = kLens[rnd() % 11];
    lens[7] = 70;   // the first row group's max is long or not by chance
    Source s = make_source(lens, 0);
    std::unique_ptr<uint64_t[]> series(new uint64_t[n]);
    std::unique_ptr<int64_t[]> ts(new int64_t[n]);
    std::unique_ptr<uint64_t[]> seqs(new uint64_t[n]);
    std::unique_ptr<int64_t[]> offs(new int64_t[n + 1]);
    offs[0] = 0;
    for (uint32_t i = 0; i < n; i++) {
        series[i] = i / 3;
        ts[i] = int64_t(i % 3) * 1000 - 500;
        seqs[i] = 1 + rnd() % 5;
        offs[i + 1] = offs[i] + lens[i];
    }
    Built b = build(s, nullptr, n, R);
    std::vector<hx::PagePayload> ready(b.page_off.size() * 5 - 5,
                                       hx::PagePayload{});
    for (size_t g = 0; g + 1 < b.page_off.size(); g++) {
        ready[g * 5 + 2].ptr = b.image.get() + b.page_off[g];
        ready[g * 5 + 2].len = uint32_t(b.page_off[g + 1] - b.page_off[g]);
    }
    char tmpl[] = "/tmp/ba_pages_check_XXXXXX";
    if (!mkdtemp(tmpl)) {
        report("mkdtemp", false);
        return;
    }
    const std::string dir = tmpl;
    for (int per_row = 0; per_row < 2; per_row++) {
        const std::string p1 = dir + "/a.sst", p2 = dir + "/b.sst";
        std::string e1 = hx::write_metric_sst_bytes(
            p1, series.get(), ts.get(), s.bytes.get(), offs.get(),
            per_row ? seqs.get() : nullptr, 9, n, R);
        std::string e2 = hx::write_metric_sst_bytes(
            p2, series.get(), ts.get(), nullptr, nullptr,
            per_row ? seqs.get() : nullptr, 9, n, R, ready.data());
        std::vector<uint8_t> f1 = slurp(p1), f2 = slurp(p2);
        report(std::string("writer: ready route == offsets route") +
                   (per_row ? " (per-row seq)" : ""),
               e1.empty() && e2.empty() && !f1.empty() && f1 == f2);
        bool ok = false;
        try {
            hx::FileMetadata m = hx::parse_footer(f1.data(), f1.size(),
                                                  (int64_t)f1.size());
            ok = m.num_rows == n && m.columns.size() == 5 &&
                 m.columns[2].name == "value" &&
                 m.columns[2].physical_type == hx::PT_BYTE_ARRAY &&
                 m.columns[2].required && m.row_groups.size() == 3;
            for (size_t g = 0; ok && g < m.row_groups.size(); g++) {
                const hx::ColumnChunkMeta& c = m.row_groups[g].columns[2];
                const uint64_t len = b.page_off[g + 1] - b.page_off[g];
                ok = c.codec == 0 && c.data_page_offset > 0 &&
                     uint64_t(c.total_uncompressed_size) > len &&
                     uint64_t(c.total_compressed_size) ==
                         uint64_t(c.total_uncompressed_size);
                // the page payload closes the chunk
                const uint64_t end = c.data_page_offset +
                                     c.total_compressed_size;
                ok = ok && end <= f1.size() &&
                     !std::memcmp(f1.data() + end - len,
                                  b.image.get() + b.page_off[g], len);
            }
        } catch (const std::exception& e) {
            std::printf("  parse_footer: %s\n", e.what());
        }
        report(std::string("writer: footer and pages parse back") +
                   (per_row ? " (per-row seq)" : ""), ok);
        unlink(p1.c_str());
        unlink(p2.c_str());
    }
    // a ready page that is shorter than its rows is refused, no file left
    ready[2].len -= 1;
    const std::string p3 = dir + "/c.sst";
    std::string e3 = hx::write_metric_sst_bytes(p3, series.get(), ts.get(),
                                                nullptr, nullptr, nullptr, 9,
                                                n, R, ready.data());
    report("writer: short ready page refused",
           !e3.empty() && access(p3.c_str(), F_OK) != 0);
    rmdir(dir.c_str());
}

}  // namespace

int main() {
    check_rows();
    check_groups();
    check_refusals();
    check_writer();
    std::printf("%s\n", g_fail ? "FAILED" : "all ok");
    return g_fail ? 1 : 0;
}
