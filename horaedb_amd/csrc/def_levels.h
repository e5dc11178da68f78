// def_levels.h — host-side helpers for OPTIONAL (nullable) columns: the
// definition levels of a flat OPTIONAL column are one bit per row (1 = value
// present), stored as the Parquet RLE/bit-packed hybrid at bit width 1. v1
// data pages carry them as a 4-byte-length-prefixed block at the start of the
// page body — inside the compressed stream when the page is compressed — so
// staging also needs the first few bytes of a Snappy stream without decoding
// the page. Header-only and free of other project headers so it compiles
// stand-alone (def_levels_check.cpp runs it under the host sanitizers).
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

enum : int {
    HX_LVL_OK = 0,
    HX_LVL_TRUNCATED = -1,   // varint / run payload / block runs past `len`
    HX_LVL_BAD_VALUE = -2,   // RLE value above 1 (max level of a flat column)
    HX_LVL_ZERO_RUN = -3,    // run header with a zero count
    HX_LVL_TOO_FEW = -4,     // block ended before n_rows values
    HX_LVL_OVERRUN = -5,     // run extends past n_rows (beyond bit-pack padding)
};

// bits [from, from + cnt) of LSB-first 64-bit words := 1
static inline void hx_bitmap_set_range(uint64_t* w, uint64_t from,
                                       uint64_t cnt) {
    while (cnt) {
        const uint64_t bit = from & 63u;
        const uint64_t take = cnt < 64u - bit ? cnt : 64u - bit;
        const uint64_t m = take == 64u ? ~0ull : ((1ull << take) - 1ull) << bit;
        w[from >> 6] |= m;
        from += take;
        cnt -= take;
    }
}

// v1 level block framing: page[0, page_len) starts with a u32 LE length and
// that many bytes of levels. *block_bytes = 4 + length. A page too short for
// the prefix, or a block longer than the page, is HX_LVL_TRUNCATED.
static inline int hx_level_block_bytes(const uint8_t* page, size_t page_len,
                                       uint32_t* block_bytes) {
    if (page_len < 4) return HX_LVL_TRUNCATED;
    const uint64_t rle = uint64_t(page[0]) | uint64_t(page[1]) << 8 |
                         uint64_t(page[2]) << 16 | uint64_t(page[3]) << 24;
    if (4 + rle > uint64_t(page_len)) return HX_LVL_TRUNCATED;
    *block_bytes = uint32_t(4 + rle);
    return HX_LVL_OK;
}

// Decode levels[0, len) (RLE/bit-packed hybrid, bit width 1, no length
// prefix) into n_rows validity bits: bitmap_words[(n_rows + 63) / 64],
// LSB-first, bits at and above n_rows zero. bitmap_words may be null (count
// only). *n_valid receives the number of set bits. A bit-packed run may
// overshoot n_rows by up to 7 padding values; every other irregularity is an
// error (see the enum). Never reads outside levels[0, len), never writes
// outside the words. Bytes after the run that completes n_rows are ignored.
static inline int hx_levels_to_bitmap(const uint8_t* levels, size_t len,
                                      uint32_t n_rows, uint64_t* bitmap_words,
                                      uint32_t* n_valid) {
    const size_t n_words = (size_t(n_rows) + 63) / 64;
    if (bitmap_words)
        for (size_t i = 0; i < n_words; i++) bitmap_words[i] = 0;
    size_t pos = 0;
    uint32_t out = 0, valid = 0;
    while (out < n_rows) {
        if (pos >= len) return HX_LVL_TOO_FEW;
        uint64_t hdr = 0;
        for (int shift = 0;; shift += 7) {  // run header fits a u32
            if (pos >= len || shift > 28) return HX_LVL_TRUNCATED;
            const uint8_t b = levels[pos++];
            hdr |= uint64_t(b & 0x7f) << shift;
            if (!(b & 0x80)) break;
        }
        const uint64_t count = hdr >> 1;
        if (count == 0) return HX_LVL_ZERO_RUN;
        const uint32_t left = n_rows - out;
        if (hdr & 1) {  // bit-packed: `count` groups of 8 values, 1 byte each
            if (uint64_t(len - pos) < count) return HX_LVL_TRUNCATED;
            const uint64_t vals = count * 8;
            if (vals > uint64_t(left) + 7) return HX_LVL_OVERRUN;
            const uint32_t take = vals < left ? uint32_t(vals) : left;
            for (uint32_t i = 0; i < take; i++) {
                if ((levels[pos + (i >> 3)] >> (i & 7)) & 1) {
                    if (bitmap_words)
                        bitmap_words[(out + i) >> 6] |= 1ull << ((out + i) & 63);
                    valid++;
                }
            }
            pos += size_t(count);
            out += take;
        } else {  // RLE: one value byte, repeated `count` times
            if (pos >= len) return HX_LVL_TRUNCATED;
            const uint8_t v = levels[pos++];
            if (v > 1) return HX_LVL_BAD_VALUE;
            if (count > left) return HX_LVL_OVERRUN;
            if (v) {
                if (bitmap_words) hx_bitmap_set_range(bitmap_words, out, count);
                valid += uint32_t(count);
            }
            out += uint32_t(count);
        }
    }
    *n_valid = valid;
    return HX_LVL_OK;
}

// Decode the first `want` output bytes of the Snappy stream src[0, n) into
// out[0, want). Returns the bytes produced — min(want, the stream's declared
// length) — or -1 on a malformed or truncated stream: bad preamble, an
// element running past the declared length, input ending before the prefix
// is complete, a copy with offset 0 or reaching before the first output
// byte. Handles the inline and 1..4-byte literal lengths and the 1-, 2- and
// 4-byte-offset copies. Never reads outside src[0, n) or writes outside
// out[0, want).
static inline long hx_snappy_prefix(const uint8_t* src, size_t n, uint8_t* out,
                                    size_t want) {
    size_t pos = 0;
    uint64_t ulen = 0;
    for (int shift = 0;; shift += 7) {  // preamble: varint, at most 5 bytes
        if (pos >= n || pos >= 5) return -1;
        const uint8_t b = src[pos++];
        ulen |= uint64_t(b & 0x7f) << shift;
        if (!(b & 0x80)) break;
    }
    if (ulen > 0xFFFFFFFFull) return -1;
    const uint64_t target = uint64_t(want) < ulen ? uint64_t(want) : ulen;
    uint64_t done = 0;  // output bytes decoded == written (all < target)
    while (done < target) {
        if (pos >= n) return -1;
        const uint8_t tag = src[pos++];
        uint64_t len, off = 0;
        if ((tag & 3u) == 0) {  // literal
            len = uint64_t(tag >> 2) + 1;
            if (len > 60) {
                const size_t nb = size_t(len - 60);
                if (n - pos < nb) return -1;
                uint64_t l = 0;
                for (size_t k = 0; k < nb; k++)
                    l |= uint64_t(src[pos + k]) << (8 * k);
                pos += nb;
                len = l + 1;
            }
            if (len > ulen - done) return -1;
            const uint64_t take = len < target - done ? len : target - done;
            if (uint64_t(n - pos) < take) return -1;
            for (uint64_t k = 0; k < take; k++) out[done + k] = src[pos + k];
            done += take;
            // a literal cut by `target` ends the loop; otherwise it was taken
            // whole and pos + len <= n holds
            pos += size_t(take);
            continue;
        }
        if ((tag & 3u) == 1) {  // copy, 1-byte offset
            if (n - pos < 1) return -1;
            len = 4 + ((tag >> 2) & 7u);
            off = (uint64_t(tag >> 5) << 8) | src[pos];
            pos += 1;
        } else if ((tag & 3u) == 2) {  // copy, 2-byte offset
            if (n - pos < 2) return -1;
            len = uint64_t(tag >> 2) + 1;
            off = uint64_t(src[pos]) | uint64_t(src[pos + 1]) << 8;
            pos += 2;
        } else {  // copy, 4-byte offset
            if (n - pos < 4) return -1;
            len = uint64_t(tag >> 2) + 1;
            off = uint64_t(src[pos]) | uint64_t(src[pos + 1]) << 8 |
                  uint64_t(src[pos + 2]) << 16 | uint64_t(src[pos + 3]) << 24;
            pos += 4;
        }
        if (off == 0 || off > done) return -1;
        if (len > ulen - done) return -1;
        const uint64_t take = len < target - done ? len : target - done;
        for (uint64_t k = 0; k < take; k++)  // may overlap itself: bytewise
            out[done + k] = out[done + k - off];
        done += take;
    }
    return long(done);
}

// ---------------------------------------------------------------------------
// Write side (DESIGN §2 / §4 kernel 1d): the inverse of the above for the
// native writer. Host-only; <vector> is the one extra dependency.
// ---------------------------------------------------------------------------

namespace hx {

// Append the v1 level block of one page of a flat OPTIONAL column to `out`:
// u32 LE length, then RLE/bit-packed hybrid runs at bit width 1.
// bitmap_words: (n_rows + 63) / 64 LSB-first words, bits at and above n_rows
// zero, n_valid of them set. A page without nulls is ONE RLE run of 1s (the
// 6/7/8-byte block of a page of <64 / <8192 / 8192 rows), a page of nothing
// but nulls one RLE run of 0s; anything else is ONE bit-packed run whose
// payload is the first ceil(n_rows / 8) bitmap bytes verbatim — the LSB-first
// bitmap is the 1-bit bit-packed layout, and the zero pad bits of the last
// group are what the format allows a final run.
static inline void encode_def_levels(const uint64_t* bitmap_words,
                                     uint32_t n_rows, uint32_t n_valid,
                                     std::vector<uint8_t>& out) {
    const size_t at = out.size();
    out.insert(out.end(), 4, uint8_t(0));
    auto varint = [&](uint64_t v) {
        while (v >= 0x80) {
            out.push_back(uint8_t(v) | 0x80);
            v >>= 7;
        }
        out.push_back(uint8_t(v));
    };
    if (n_valid == n_rows || n_valid == 0) {
        varint(uint64_t(n_rows) << 1);
        out.push_back(n_valid ? 1 : 0);
    } else {
        const uint32_t n_bytes = (n_rows + 7) / 8;
        varint((uint64_t(n_bytes) << 1) | 1u);
        for (uint32_t b = 0; b < n_bytes; b++)
            out.push_back(uint8_t(bitmap_words[b >> 3] >> ((b & 7u) * 8u)));
    }
    const uint32_t len = uint32_t(out.size() - at - 4);
    for (int b = 0; b < 4; b++) out[at + b] = uint8_t(len >> (8 * b));
}

// Host twin of kernel 1d (k_pack_optional), same contract: output row i of n
// is source row perm[i] (i when perm is null) of n_src; valid_bits is an
// LSB-first bitmap over SOURCE rows (null: all present). Per row group g of
// row_group rows (a multiple of 64): bitmap_out + g * (row_group / 64)
// receives row_group / 64 words (bits at and above the group's row count
// zero), packed_out + g * row_group the group's present values in row order,
// n_valid_out[g] their number. A perm entry >= n_src is counted in the
// return value and its row written as null.
static inline uint64_t pack_optional_host(
    const uint64_t* values, const uint8_t* valid_bits, const uint32_t* perm,
    uint64_t n_src, uint64_t n, uint64_t row_group, uint64_t* packed_out,
    uint64_t* bitmap_out, uint32_t* n_valid_out) {
    const uint64_t wpg = row_group / 64;
    uint64_t errors = 0;
    for (uint64_t g = 0, row0 = 0; row0 < n; g++, row0 += row_group) {
        const uint64_t rows = n - row0 < row_group ? n - row0 : row_group;
        uint64_t* bm = bitmap_out + g * wpg;
        for (uint64_t w = 0; w < wpg; w++) bm[w] = 0;
        uint32_t k = 0;
        for (uint64_t r = 0; r < rows; r++) {
            const uint64_t p = perm ? perm[row0 + r] : row0 + r;
            if (p >= n_src) {
                errors++;
                continue;
            }
            if (valid_bits && !((valid_bits[p >> 3] >> (p & 7u)) & 1u))
                continue;
            bm[r >> 6] |= 1ull << (r & 63u);
            packed_out[row0 + k++] = values[p];
        }
        n_valid_out[g] = k;
    }
    return errors;
}

}  // namespace hx
