// snappy_stored_check.cpp — stand-alone host check of
// hx_snappy_stored_literal (snappy_stored.h). Built by `make
// snappy_stored_check` with -fsanitize=address,undefined when the runtime is
// available; every buffer is an exact-size heap allocation so a read past
// p[0, n) trips the sanitizer. Prints one line per case, exits non-zero on
// the first mismatch.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "snappy_stored.h"

namespace {

int g_fail = 0;

std::vector<uint8_t> varint(uint64_t v, int force_bytes = 0) {
    std::vector<uint8_t> o;
    while (v >= 0x80 || (force_bytes && (int)o.size() + 1 < force_bytes)) {
        o.push_back(uint8_t(v & 0x7f) | 0x80);
        v >>= 7;
    }
    o.push_back(uint8_t(v));
    return o;
}

// literal tag + extra length bytes for `len` using `form` extra bytes
// (0 = inline, 1..4)
std::vector<uint8_t> lit_header(uint32_t len, int form) {
    std::vector<uint8_t> o;
    if (form == 0) {
        o.push_back(uint8_t((len - 1) << 2));
    } else {
        o.push_back(uint8_t((59 + form) << 2));
        uint32_t l = len - 1;
        for (int k = 0; k < form; k++) o.push_back(uint8_t(l >> (8 * k)));
    }
    return o;
}

std::vector<uint8_t> cat(std::initializer_list<std::vector<uint8_t>> parts) {
    std::vector<uint8_t> o;
    for (const auto& p : parts) o.insert(o.end(), p.begin(), p.end());
    return o;
}

std::vector<uint8_t> body(size_t n) {
    std::vector<uint8_t> o(n);
    for (size_t i = 0; i < n; i++) o[i] = uint8_t(i * 131 + 7);
    return o;
}

void check(const char* name, const std::vector<uint8_t>& buf, uint32_t expect,
           bool want, uint32_t want_off = 0) {
    // exact-size heap copy: any over-read is a heap-buffer-overflow
    uint8_t* p = buf.empty() ? nullptr : new uint8_t[buf.size()];
    if (p) std::memcpy(p, buf.data(), buf.size());
    uint32_t off = 0xDEADBEEFu;
    const bool got = hx_snappy_stored_literal(p, buf.size(), expect, &off);
    bool ok = got == want;
    if (ok && want) ok = off == want_off;
    if (ok && !want) ok = off == 0xDEADBEEFu;
    std::printf("%-44s %s\n", name, ok ? "ok" : "FAIL");
    if (!ok) g_fail++;
    delete[] p;
}

}  // namespace

int main() {
    // the four literal-length forms (plus the 4-byte form) at exact fit
    struct { int form; uint32_t len; } fits[] = {
        {0, 1}, {0, 40}, {0, 60}, {1, 61}, {1, 256}, {2, 257}, {2, 65536},
        {3, 65537}, {3, 70000}, {4, 65536}, {4, 100},
    };
    for (const auto& f : fits) {
        auto pre = varint(f.len);
        auto hdr = lit_header(f.len, f.form);
        auto buf = cat({pre, hdr, body(f.len)});
        std::string nm = "fit form=" + std::to_string(f.form) + " len=" +
                         std::to_string(f.len);
        check(nm.c_str(), buf, f.len, true,
              uint32_t(pre.size() + hdr.size()));
        // buffer one byte short / one byte long of the literal
        auto shorter = buf;
        shorter.pop_back();
        check((nm + " short").c_str(), shorter, f.len, false);
        auto longer = buf;
        longer.push_back(0);
        check((nm + " long").c_str(), longer, f.len, false);
        // literal length one off the preamble
        auto l1 = cat({pre, lit_header(f.len + 1, f.form ? f.form : 1),
                       body(f.len + 1)});
        check((nm + " lit+1").c_str(), l1, f.len, false);
    }
    // the bench-shaped page: 3-byte preamble, tag 0xF4 + 2 bytes, 64 KB
    {
        auto buf = cat({varint(65536), lit_header(65536, 2), body(65536)});
        check("value page 65542 bytes, body at 6", buf, 65536,
              buf.size() == 65542, 6);
    }
    // preamble differs from expect_ulen
    check("preamble != expect",
          cat({varint(41), lit_header(40, 0), body(40)}), 40, false);
    check("expect != preamble == literal",
          cat({varint(40), lit_header(40, 0), body(40)}), 41, false);
    // truncated preamble (continuation bit set on the last byte)
    check("truncated preamble", {0x80}, 0, false);
    check("truncated preamble 3", {0x80, 0x80, 0x80}, 0, false);
    check("preamble only", varint(40), 40, false);
    // 6-byte preamble (non-canonical padding of a small value)
    check("6-byte preamble",
          cat({varint(40, 6), lit_header(40, 0), body(40)}), 40, false);
    // 5-byte non-canonical preamble is still well-formed
    {
        auto pre = varint(40, 5);
        check("5-byte preamble",
              cat({pre, lit_header(40, 0), body(40)}), 40, true,
              uint32_t(pre.size() + 1));
    }
    // 5-byte preamble carrying bits above 2^32
    check("preamble > u32", {0xFF, 0xFF, 0xFF, 0xFF, 0x7F, 0x00, 0x00},
          0xFFFFFFFFu, false);
    // first element is a copy (1-, 2- and 4-byte offset kinds)
    check("first element copy1", cat({varint(8), {0x11, 0x01}}), 8, false);
    check("first element copy2", cat({varint(8), {0x1E, 0x01, 0x00}}), 8,
          false);
    check("first element copy4",
          cat({varint(8), {0x1F, 0x01, 0x00, 0x00, 0x00}}), 8, false);
    // literal followed by one more element
    check("literal + copy",
          cat({varint(44), lit_header(40, 0), body(40), {0x01, 0x08}}), 44,
          false);
    check("literal + literal",
          cat({varint(41), lit_header(40, 0), body(40), {0x00, 0x55}}), 41,
          false);
    // n = 0
    check("n = 0", {}, 0, false);
    check("n = 0, expect 8", {}, 8, false);
    // truncated extra length bytes
    check("truncated length bytes", cat({varint(300), {0xF4, 0x2B}}), 300,
          false);
    // 4-byte length of 0xFFFFFFFF (len = 2^32): no wrap to 0
    check("len bytes 0xFFFFFFFF, expect 0",
          cat({varint(0), {0xFC, 0xFF, 0xFF, 0xFF, 0xFF}}), 0, false);
    check("len bytes 0xFFFFFFFF, expect max",
          cat({varint(0xFFFFFFFFu), {0xFC, 0xFF, 0xFF, 0xFF, 0xFF}, body(16)}),
          0xFFFFFFFFu, false);
    std::printf("%s\n", g_fail ? "FAILED" : "ALL OK");
    return g_fail ? 1 : 0;
}
