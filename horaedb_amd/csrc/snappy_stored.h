// snappy_stored.h — host-side test for "stored" Snappy pages: a stream that is
// nothing but the length preamble plus ONE literal element covering the whole
// page (what the Snappy writer emits for incompressible input, e.g. random f64
// value pages). Such a page needs no decoding: its body is the page's PLAIN
// bytes, and staging places it so the aggregate kernels read it in place.
// Header-only and free of other project headers so it compiles stand-alone
// (snappy_stored_check.cpp runs it under the host sanitizers).
#pragma once
#include <cstddef>
#include <cstdint>

// True iff p[0, n) is {varint preamble == expect_ulen, one literal element of
// exactly expect_ulen bytes} and nothing else; *body_off receives the offset
// of the literal's first byte. Anything else (malformed, truncated, a copy
// element first, trailing elements, any length mismatch) returns false and
// leaves *body_off untouched. Never reads outside p[0, n).
static inline bool hx_snappy_stored_literal(const uint8_t* p, size_t n,
                                            uint32_t expect_ulen,
                                            uint32_t* body_off) {
    size_t pos = 0;
    uint64_t ulen = 0;
    int shift = 0;
    for (;;) {  // preamble: LE base-128 varint, at most 5 bytes (u32)
        if (pos >= n || pos >= 5) return false;
        const uint8_t b = p[pos++];
        ulen |= uint64_t(b & 0x7f) << shift;
        if (!(b & 0x80)) break;
        shift += 7;
    }
    if (ulen != uint64_t(expect_ulen)) return false;
    if (pos >= n) return false;
    const uint8_t tag = p[pos++];
    if ((tag & 3u) != 0) return false;  // first element is a copy
    uint64_t len = uint64_t(tag >> 2) + 1;  // 1..60 inline
    if (len > 60) {
        const size_t nb = size_t(len - 60);  // 1..4 extra length bytes
        if (n - pos < nb) return false;
        uint64_t l = 0;
        for (size_t k = 0; k < nb; k++) l |= uint64_t(p[pos + k]) << (8 * k);
        pos += nb;
        len = l + 1;  // 64-bit: 0xFFFFFFFF + 1 does not wrap
    }
    if (len != uint64_t(expect_ulen)) return false;
    if (uint64_t(n - pos) != len) return false;  // exact fit, no trailer
    *body_off = uint32_t(pos);
    return true;
}

// The same for a stream of SEVERAL literals and nothing else — what the
// Snappy library emits for incompressible input above 65 536 bytes, one
// literal per 64 KiB fragment (a 1 MiB BYTE_ARRAY value page of random bytes
// is 16 of them). True iff p[0, n) is {varint preamble == expect_ulen, one or
// more literal elements whose bodies add up to exactly expect_ulen} with no
// copy element and no trailer. With out non-null the bodies are written back
// to back to out[0, expect_ulen): the page's PLAIN bytes, no decode needed.
// A false return may have written a prefix of out. Never reads outside
// p[0, n) or writes outside out[0, expect_ulen).
static inline bool hx_snappy_literals_only(const uint8_t* p, size_t n,
                                           uint32_t expect_ulen,
                                           uint8_t* out) {
    size_t pos = 0;
    uint64_t ulen = 0;
    int shift = 0;
    for (;;) {  // preamble: LE base-128 varint, at most 5 bytes (u32)
        if (pos >= n || pos >= 5) return false;
        const uint8_t b = p[pos++];
        ulen |= uint64_t(b & 0x7f) << shift;
        if (!(b & 0x80)) break;
        shift += 7;
    }
    if (ulen != uint64_t(expect_ulen)) return false;
    uint64_t done = 0;
    while (pos < n) {
        const uint8_t tag = p[pos++];
        if ((tag & 3u) != 0) return false;  // a copy element
        uint64_t len = uint64_t(tag >> 2) + 1;  // 1..60 inline
        if (len > 60) {
            const size_t nb = size_t(len - 60);  // 1..4 extra length bytes
            if (n - pos < nb) return false;
            uint64_t l = 0;
            for (size_t k = 0; k < nb; k++)
                l |= uint64_t(p[pos + k]) << (8 * k);
            pos += nb;
            len = l + 1;
        }
        if (len > ulen - done || len > uint64_t(n - pos)) return false;
        if (out)
            for (uint64_t k = 0; k < len; k++) out[done + k] = p[pos + k];
        pos += size_t(len);
        done += len;
    }
    return done == ulen && ulen != 0;
}
