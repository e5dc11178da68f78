// def_levels_check.cpp — stand-alone host check of def_levels.h
// (hx_levels_to_bitmap, hx_level_block_bytes, hx_snappy_prefix). Built by
// `make def_levels_check` with -fsanitize=address,undefined when the runtime
// is available; every input, bitmap and output buffer is an exact-size heap
// allocation so a read or write outside it trips the sanitizer. Prints one
// line per case, exits non-zero on any mismatch.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "def_levels.h"

namespace {

int g_fail = 0;
typedef std::vector<uint8_t> Bytes;

void report(const std::string& name, bool ok) {
    std::printf("%-52s %s\n", name.c_str(), ok ? "ok" : "FAIL");
    if (!ok) g_fail++;
}

Bytes cat(std::initializer_list<Bytes> parts) {
    Bytes o;
    for (const auto& p : parts) o.insert(o.end(), p.begin(), p.end());
    return o;
}

Bytes varint(uint64_t v) {
    Bytes o;
    while (v >= 0x80) {
        o.push_back(uint8_t(v & 0x7f) | 0x80);
        v >>= 7;
    }
    o.push_back(uint8_t(v));
    return o;
}

Bytes rle(uint32_t count, uint8_t v) {
    return cat({varint(uint64_t(count) << 1), {v}});
}

// bit-packed run holding `bits` (padded with zero bits to a multiple of 8)
Bytes packed(const std::vector<int>& bits) {
    const size_t groups = (bits.size() + 7) / 8;
    Bytes o = varint((uint64_t(groups) << 1) | 1);
    for (size_t g = 0; g < groups; g++) {
        uint8_t b = 0;
        for (size_t k = 0; k < 8 && g * 8 + k < bits.size(); k++)
            if (bits[g * 8 + k]) b |= uint8_t(1u << k);
        o.push_back(b);
    }
    return o;
}

uint8_t* exact(const Bytes& b) {
    uint8_t* p = b.empty() ? nullptr : new uint8_t[b.size()];
    if (p) std::memcpy(p, b.data(), b.size());
    return p;
}

// decode `lv` for n rows and compare with `want_bits` (size n) or want_rc
void levels(const std::string& name, const Bytes& lv, uint32_t n, int want_rc,
            const std::vector<int>& want_bits = {}) {
    uint8_t* p = exact(lv);
    const size_t nw = (size_t(n) + 63) / 64;
    uint64_t* w = nw ? new uint64_t[nw] : nullptr;
    for (size_t i = 0; i < nw; i++) w[i] = ~0ull;  // must be overwritten
    uint32_t nv = 0xDEADBEEFu;
    const int rc = hx_levels_to_bitmap(p, lv.size(), n, w, &nv);
    bool ok = rc == want_rc;
    if (ok && rc == HX_LVL_OK) {
        uint32_t cnt = 0;
        for (uint32_t i = 0; i < n && ok; i++) {
            const int bit = int((w[i >> 6] >> (i & 63)) & 1);
            ok = bit == want_bits[i];
            cnt += uint32_t(bit);
        }
        // bits at and above n stay zero
        if (ok && (n & 63)) ok = (w[nw - 1] >> (n & 63)) == 0;
        ok = ok && nv == cnt;
        // the count-only form agrees
        uint32_t nv2 = 0;
        ok = ok && hx_levels_to_bitmap(p, lv.size(), n, nullptr, &nv2) == 0 &&
             nv2 == nv;
    }
    if (ok && rc != HX_LVL_OK) ok = nv == 0xDEADBEEFu;
    report(name, ok);
    delete[] p;
    delete[] w;
}

void prefix(const std::string& name, const Bytes& stream, size_t want,
            long want_rc, const Bytes& want_out = {}) {
    uint8_t* p = exact(stream);
    uint8_t* o = want ? new uint8_t[want] : nullptr;
    const long rc = hx_snappy_prefix(p, stream.size(), o, want);
    bool ok = rc == want_rc;
    if (ok && rc > 0) ok = std::memcmp(o, want_out.data(), size_t(rc)) == 0;
    report(name, ok);
    delete[] p;
    delete[] o;
}

Bytes lit(const Bytes& body, int form) {  // form = extra length bytes, 0..4
    Bytes o;
    const uint32_t l = uint32_t(body.size()) - 1;
    if (form == 0) {
        o.push_back(uint8_t(l << 2));
    } else {
        o.push_back(uint8_t((59 + form) << 2));
        for (int k = 0; k < form; k++) o.push_back(uint8_t(l >> (8 * k)));
    }
    o.insert(o.end(), body.begin(), body.end());
    return o;
}

Bytes seq(size_t n, unsigned mul = 131) {
    Bytes o(n);
    for (size_t i = 0; i < n; i++) o[i] = uint8_t(i * mul + 7);
    return o;
}

}  // namespace

int main() {
    // ---- levels: one all-ones RLE run ------------------------------------
    for (uint32_t n : {1u, 63u, 64u, 65u, 8192u})
        levels("rle ones n=" + std::to_string(n), rle(n, 1), n, HX_LVL_OK,
               std::vector<int>(n, 1));
    for (uint32_t n : {1u, 64u, 100u})
        levels("rle zeros n=" + std::to_string(n), rle(n, 0), n, HX_LVL_OK,
               std::vector<int>(n, 0));
    levels("n = 0, empty block", {}, 0, HX_LVL_OK);
    // ---- one bit-packed run, n not a multiple of 8 -------------------------
    for (uint32_t n : {1u, 13u, 59u, 67u, 101u}) {
        std::vector<int> bits(n);
        for (uint32_t i = 0; i < n; i++) bits[i] = (i * 7 + 3) % 3 != 0;
        levels("bit-packed n=" + std::to_string(n), packed(bits), n, HX_LVL_OK,
               bits);
    }
    {   // padding bits set to 1 are ignored
        Bytes lv = {0x03, 0xFF};
        levels("bit-packed padding ones n=3", lv, 3, HX_LVL_OK, {1, 1, 1});
    }
    {   // alternating valid/null
        std::vector<int> bits(200);
        for (size_t i = 0; i < bits.size(); i++) bits[i] = int(i & 1);
        levels("bit-packed alternating n=200", packed(bits), 200, HX_LVL_OK,
               bits);
    }
    // ---- RLE and bit-packed alternating across a 64-bit word edge ----------
    {
        std::vector<int> want;
        Bytes lv;
        auto add_rle = [&](uint32_t c, int v) {
            auto r = rle(c, uint8_t(v));
            lv.insert(lv.end(), r.begin(), r.end());
            want.insert(want.end(), c, v);
        };
        auto add_packed = [&](const std::vector<int>& b) {  // size % 8 == 0
            auto r = packed(b);
            lv.insert(lv.end(), r.begin(), r.end());
            want.insert(want.end(), b.begin(), b.end());
        };
        add_rle(61, 1);                                   // rows 0..60
        add_packed({0, 1, 1, 0, 1, 0, 0, 1});             // 61..68 (crosses 64)
        add_rle(50, 0);                                   // 69..118
        add_packed({1, 1, 1, 1, 0, 0, 0, 0, 1, 0, 1, 0, 1, 0, 1, 0});  // ..134
        add_rle(130, 1);                                  // crosses 192, 256
        std::vector<int> tail = {1, 0, 1};                // final partial group
        auto r = packed(tail);
        lv.insert(lv.end(), r.begin(), r.end());
        want.insert(want.end(), tail.begin(), tail.end());
        levels("mixed runs across word edges", lv, uint32_t(want.size()),
               HX_LVL_OK, want);
        // the same block read for fewer rows: the last run overshoots
        levels("mixed runs, rle past n_rows", lv, 200, HX_LVL_OVERRUN);
    }
    // ---- malformed ----------------------------------------------------------
    levels("rle value 2", rle(10, 2), 10, HX_LVL_BAD_VALUE);
    levels("rle value 255", rle(10, 255), 10, HX_LVL_BAD_VALUE);
    levels("zero-length rle run", {0x00, 0x01}, 4, HX_LVL_ZERO_RUN);
    levels("zero-length bit-packed run", {0x01}, 4, HX_LVL_ZERO_RUN);
    levels("truncated varint", {0x80}, 4, HX_LVL_TRUNCATED);
    levels("truncated varint 3", {0x80, 0x80, 0x80}, 4, HX_LVL_TRUNCATED);
    levels("over-long varint", {0x80, 0x80, 0x80, 0x80, 0x80, 0x01, 0x01}, 4,
           HX_LVL_TRUNCATED);
    levels("rle without value byte", varint(8u << 1), 8, HX_LVL_TRUNCATED);
    levels("bit-packed data cut short", {0x05, 0xFF}, 16, HX_LVL_TRUNCATED);
    levels("empty block, rows wanted", {}, 8, HX_LVL_TOO_FEW);
    levels("too few values (rle)", rle(7, 1), 8, HX_LVL_TOO_FEW);
    levels("too few values (bit-packed)", packed(std::vector<int>(8, 1)), 9,
           HX_LVL_TOO_FEW);
    levels("rle run past n_rows", rle(9, 1), 8, HX_LVL_OVERRUN);
    levels("rle run past n_rows after a run",
           cat({rle(4, 1), rle(5, 0)}), 8, HX_LVL_OVERRUN);
    levels("bit-packed 8 past n_rows", packed(std::vector<int>(16, 1)), 8,
           HX_LVL_OVERRUN);
    levels("bit-packed 7 past n_rows (padding)",
           packed(std::vector<int>(8, 1)), 1, HX_LVL_OK, {1});
    // ---- v1 block framing ---------------------------------------------------
    {
        struct { Bytes page; int rc; uint32_t bytes; } fr[] = {
            {{2, 0, 0, 0, 0x10, 0x01, 9, 9}, HX_LVL_OK, 6},
            {{4, 0, 0, 0, 1, 2, 3, 4}, HX_LVL_OK, 8},       // block == page
            {{5, 0, 0, 0, 1, 2, 3, 4}, HX_LVL_TRUNCATED, 0},  // longer than page
            {{0xFF, 0xFF, 0xFF, 0xFF, 1}, HX_LVL_TRUNCATED, 0},
            {{1, 0, 0}, HX_LVL_TRUNCATED, 0},               // prefix cut
            {{}, HX_LVL_TRUNCATED, 0},
        };
        int k = 0;
        for (const auto& f : fr) {
            uint8_t* p = exact(f.page);
            uint32_t bb = 0;
            const int rc = hx_level_block_bytes(p, f.page.size(), &bb);
            report("level block framing " + std::to_string(k++),
                   rc == f.rc && (rc != HX_LVL_OK || bb == f.bytes));
            delete[] p;
        }
    }
    // ---- snappy prefix: every literal length form ---------------------------
    struct { int form; size_t len; } forms[] = {
        {0, 1}, {0, 8}, {0, 60}, {1, 61}, {1, 256}, {2, 257}, {2, 65536},
        {3, 65537}, {4, 100},
    };
    for (const auto& f : forms) {
        const Bytes body = seq(f.len);
        const Bytes s = cat({varint(f.len), lit(body, f.form)});
        const std::string nm = "literal form=" + std::to_string(f.form) +
                               " len=" + std::to_string(f.len);
        const size_t w = f.len < 4 ? f.len : 4;
        prefix(nm + " want 4", s, w, long(w), body);
        prefix(nm + " want all", s, f.len, long(f.len), body);
        prefix(nm + " want beyond", s, f.len + 9, long(f.len), body);
        Bytes cut = s;
        cut.pop_back();
        prefix(nm + " truncated", cut, f.len, -1);
    }
    {   // the reference-shaped value page: 8 level bytes + 64 KB, two literals
        Bytes page = cat({{4, 0, 0, 0, 0x80, 0x80, 0x01, 0x01}, seq(65536, 37)});
        Bytes s = cat({varint(page.size()),
                       lit(Bytes(page.begin(), page.begin() + 65536), 2),
                       lit(Bytes(page.begin() + 65536, page.end()), 0)});
        prefix("value page, want 4", s, 4, 4, page);
        prefix("value page, want 8", s, 8, 8, page);
        prefix("value page, want across literals", s, 65540, 65540, page);
    }
    // ---- copies -------------------------------------------------------------
    {
        // "abcd" then copy1 len 4 off 4, copy2 len 6 off 2, copy4 len 5 off 8
        const Bytes a = {'a', 'b', 'c', 'd'};
        const Bytes full = {'a', 'b', 'c', 'd', 'a', 'b', 'c', 'd', 'c', 'd',
                            'c', 'd', 'c', 'd', 'c', 'd', 'c', 'd', 'c'};
        const Bytes s = cat({varint(19), lit(a, 0),
                             {0x01, 0x04},                     // copy1
                             {uint8_t((6 - 1) << 2 | 2), 2, 0},  // copy2, overlap
                             {uint8_t((5 - 1) << 2 | 3), 8, 0, 0, 0}});
        prefix("copies, whole stream", s, 19, 19, full);
        prefix("copy inside the prefix", s, 7, 7, full);
        prefix("overlapping copy cut by want", s, 11, 11, full);
        prefix("want beyond stream with copies", s, 64, 19, full);
        prefix("want 0", s, 0, 0);
        Bytes cut(s.begin(), s.begin() + 7);  // copy1 tag without its offset
        prefix("truncated copy1", cut, 8, -1);
        cut.assign(s.begin(), s.begin() + 10);  // copy2 with one offset byte
        prefix("truncated copy2", cut, 12, -1);
        cut.assign(s.begin(), s.begin() + 14);  // copy4 with two offset bytes
        prefix("truncated copy4", cut, 19, -1);
        cut.assign(s.begin(), s.begin() + 8);   // ends after copy1
        prefix("input ends before prefix complete", cut, 12, -1);
        prefix("input ends, prefix already complete", cut, 8, 8, full);
    }
    prefix("copy1 offset 0", cat({varint(8), lit({'a', 'b', 'c', 'd'}, 0),
                                  {0x01, 0x00}}), 8, -1);
    prefix("copy2 offset 0", cat({varint(8), lit({'a', 'b', 'c', 'd'}, 0),
                                  {uint8_t(3 << 2 | 2), 0, 0}}), 8, -1);
    prefix("copy before start", cat({varint(8), lit({'a', 'b', 'c', 'd'}, 0),
                                     {0x01, 0x05}}), 8, -1);
    prefix("copy as first element", cat({varint(8), {0x11, 0x01}}), 4, -1);
    prefix("copy4 far before start",
           cat({varint(8), lit({'a', 'b', 'c', 'd'}, 0),
                {uint8_t(3 << 2 | 3), 0xFF, 0xFF, 0xFF, 0xFF}}), 8, -1);
    prefix("literal past declared length",
           cat({varint(3), lit({'a', 'b', 'c', 'd'}, 0)}), 3, -1);
    prefix("copy past declared length",
           cat({varint(6), lit({'a', 'b', 'c', 'd'}, 0), {0x01, 0x04}}), 6, -1);
    // ---- preamble -----------------------------------------------------------
    prefix("n = 0", {}, 4, -1);
    prefix("truncated preamble", {0x80}, 4, -1);
    prefix("6-byte preamble", {0x88, 0x80, 0x80, 0x80, 0x80, 0x00, 0x00}, 4, -1);
    prefix("preamble > u32", {0xFF, 0xFF, 0xFF, 0xFF, 0x7F, 0x00, 0x00}, 4, -1);
    prefix("preamble only", varint(40), 4, -1);
    prefix("declared length 0", varint(0), 4, 0);
    prefix("truncated literal length bytes", cat({varint(300), {0xF4, 0x2B}}),
           4, -1);
    std::printf("%s\n", g_fail ? "FAILED" : "ALL OK");
    return g_fail ? 1 : 0;
}
