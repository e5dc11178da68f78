// snappy_compress_check.cpp — stand-alone host check of
// hx::snappy_compress_host (snappy_compress.h). Built by `make
// snappy_compress_check` with -fsanitize=address,undefined when the runtime
// is available; source and destination are exact-size heap allocations, so a
// read past src[0, n) or a write past dst[0, cap) trips the sanitizer. Every
// stream is decoded by the decoder below (not the project's) and must give
// the page back; its size must respect Snappy's bound and the stored form;
// a call with cap one byte short must be refused with dst untouched.
//
// Pages: a built-in list (the lengths 0..200000 of the GPU test over three
// contents), plus every page of the files named on the command line — the
// format tests/snappy_shapes.py writes: u32 count, then {u32 len, bytes} per
// page. Prints one line per page, exits non-zero on the first mismatch.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "snappy_compress.h"
#include "snappy_stored.h"

namespace {

int g_fail = 0;

// A plain Snappy decoder with every bound checked; false on any malformed
// element or a size mismatch.
bool decode(const uint8_t* p, size_t n, std::vector<uint8_t>& out) {
    size_t pos = 0;
    uint64_t ulen = 0;
    for (int shift = 0;; shift += 7) {
        if (pos >= n || shift > 28) return false;
        const uint8_t b = p[pos++];
        ulen |= uint64_t(b & 0x7f) << shift;
        if (!(b & 0x80)) break;
    }
    out.clear();
    out.reserve(ulen);
    while (pos < n) {
        const uint8_t tag = p[pos++];
        if ((tag & 3) == 0) {
            uint64_t len = uint64_t(tag >> 2) + 1;
            if (len > 60) {
                const size_t nb = size_t(len - 60);
                if (n - pos < nb) return false;
                uint64_t l = 0;
                for (size_t k = 0; k < nb; k++)
                    l |= uint64_t(p[pos + k]) << (8 * k);
                pos += nb;
                len = l + 1;
            }
            if (n - pos < len) return false;
            out.insert(out.end(), p + pos, p + pos + len);
            pos += len;
            continue;
        }
        uint32_t len, off;
        if ((tag & 3) == 1) {
            if (n - pos < 1) return false;
            len = 4 + ((tag >> 2) & 7);
            off = (uint32_t(tag >> 5) << 8) | p[pos];
            pos += 1;
        } else if ((tag & 3) == 2) {
            if (n - pos < 2) return false;
            len = 1 + (tag >> 2);
            off = p[pos] | (uint32_t(p[pos + 1]) << 8);
            pos += 2;
        } else {
            return false;   // 4-byte-offset copies are never emitted
        }
        if (off == 0 || off > out.size()) return false;
        for (uint32_t k = 0; k < len; k++) out.push_back(out[out.size() - off]);
    }
    return out.size() == ulen;
}

void check(const std::string& name, const std::vector<uint8_t>& page) {
    const size_t n = page.size();
    const size_t cap = size_t(hx::snappy_max_compressed(n));
    uint8_t* src = n ? new uint8_t[n] : nullptr;
    if (n) std::memcpy(src, page.data(), n);
    uint8_t* dst = new uint8_t[cap];
    const size_t size = hx::snappy_compress_host(src, n, dst, cap);
    bool ok = size >= 1 && size <= cap;
    std::vector<uint8_t> back;
    ok = ok && decode(dst, size, back) && back == page;
    // never longer than the stored form; a stored stream is recognised
    const size_t stored = hx::snappy_stored_size(uint32_t(n));
    ok = ok && size <= stored;
    uint32_t off = 0;
    const bool is_stored =
        ok && n && hx_snappy_stored_literal(dst, size, uint32_t(n), &off);
    if (ok && size == stored && n && !is_stored) ok = false;
    // one byte short: refused, dst untouched (the allocation is cap - 1
    // bytes, so a write at or past it is a heap overflow)
    uint8_t* small = new uint8_t[cap - 1];
    std::memset(small, 0xA5, cap - 1);
    ok = ok && hx::snappy_compress_host(src, n, small, cap - 1) == 0;
    for (size_t i = 0; ok && i < cap - 1; i++) ok = small[i] == 0xA5;
    printf("%-28s n=%-7zu size=%-7zu %s%s\n", name.c_str(), n, size,
           is_stored ? "stored " : "", ok ? "ok" : "FAIL");
    if (!ok) g_fail++;
    delete[] small;
    delete[] dst;
    delete[] src;
}

uint64_t g_rng = 0x9E3779B97F4A7C15ull;
uint8_t rnd() {
    g_rng ^= g_rng << 13;
    g_rng ^= g_rng >> 7;
    g_rng ^= g_rng << 17;
    return uint8_t(g_rng >> 32);
}

bool run_file(const char* path) {
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    uint32_t count = 0;
    bool ok = fread(&count, 4, 1, f) == 1;
    for (uint32_t i = 0; ok && i < count; i++) {
        uint32_t len = 0;
        ok = fread(&len, 4, 1, f) == 1 && len <= (64u << 20);
        std::vector<uint8_t> page(len);
        ok = ok && (len == 0 || fread(page.data(), 1, len, f) == len);
        if (ok) check(std::string("file#") + std::to_string(i), page);
    }
    fclose(f);
    return ok;
}

}  // namespace

int main(int argc, char** argv) {
    const size_t lens[] = {0, 1, 3, 4, 5, 63, 64, 65, 67, 68,
                           4095, 65536, 65544, 200000};
    for (size_t n : lens) {
        std::vector<uint8_t> page(n);
        for (auto& b : page) b = rnd();
        check("random", page);
        for (size_t i = 0; i < n; i++) page[i] = 0x5A;
        check("constant", page);
        for (size_t i = 0; i < n; i++) page[i] = uint8_t((i % 72) * 3 + i / 4096);
        check("period72+drift", page);
    }
    for (int a = 1; a < argc; a++)
        if (!run_file(argv[a])) {
            printf("%s: unreadable FAIL\n", argv[a]);
            g_fail++;
        }
    if (g_fail) {
        printf("%d FAILED\n", g_fail);
        return 1;
    }
    printf("ALL OK\n");
    return 0;
}
