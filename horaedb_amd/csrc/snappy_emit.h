// snappy_emit.h — the element emitters of the Snappy page compressor, shared
// by the host twin (snappy_compress.h) and kernel 1e (k_snappy_compress in
// kernels.hip) so both write the same tag bytes. Nothing but plain byte
// stores through the pointer given; no other header of the project, no GPU
// header (the qualifier below is empty for a host compiler).
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define HX_SNAPPY_HD __host__ __device__
#else
#define HX_SNAPPY_HD
#endif

namespace hx {

enum : uint32_t {
    SNAPPY_HASH_BITS = 12,             // 4096 table entries of position + 1
    SNAPPY_HASH_SIZE = 1u << SNAPPY_HASH_BITS,
    SNAPPY_MAX_OFFSET = 65535,         // the 2-byte-offset copy form's limit
    SNAPPY_CHUNK = 64,                 // positions examined per step
    SNAPPY_PROBE_CAP = 16,             // candidate ranking: prefix capped here
};

HX_SNAPPY_HD inline uint32_t snappy_hash(uint32_t w) {
    return (w * 0x1e35a7bdu) >> (32 - SNAPPY_HASH_BITS);
}

// Snappy's bound on the compressed size of n bytes; an output slot smaller
// than this is refused by the twin and the kernel alike.
HX_SNAPPY_HD inline uint64_t snappy_max_compressed(uint64_t n) {
    return 32 + n + n / 6;
}

// LE base-128 varint of a u32; returns the bytes written (1..5).
HX_SNAPPY_HD inline uint32_t snappy_emit_varint(uint8_t* d, uint32_t v) {
    uint32_t k = 0;
    while (v >= 0x80) {
        d[k++] = uint8_t(v) | 0x80;
        v >>= 7;
    }
    d[k++] = uint8_t(v);
    return k;
}

// Tag (and length bytes) of a literal of len >= 1 bytes; the literal's bytes
// follow. Returns the bytes written (1..5).
HX_SNAPPY_HD inline uint32_t snappy_emit_literal_tag(uint8_t* d, uint32_t len) {
    const uint32_t n = len - 1;
    if (n < 60) {
        d[0] = uint8_t(n << 2);
        return 1;
    }
    const uint32_t nb = n < (1u << 8) ? 1 : n < (1u << 16) ? 2
                      : n < (1u << 24) ? 3 : 4;
    d[0] = uint8_t((59 + nb) << 2);
    for (uint32_t k = 0; k < nb; k++) d[1 + k] = uint8_t(n >> (8 * k));
    return 1 + nb;
}

// One copy element, 4 <= len <= 64, 1 <= offset <= 65535.
HX_SNAPPY_HD inline uint32_t snappy_emit_copy1(uint8_t* d, uint32_t offset,
                                               uint32_t len) {
    if (len < 12 && offset < 2048) {
        d[0] = uint8_t(1 | ((len - 4) << 2) | ((offset >> 8) << 5));
        d[1] = uint8_t(offset);
        return 2;
    }
    d[0] = uint8_t(2 | ((len - 1) << 2));
    d[1] = uint8_t(offset);
    d[2] = uint8_t(offset >> 8);
    return 3;
}

// A copy of len >= 4 split as Snappy's EmitCopy does: 64 while len >= 68, 60
// if more than 64 is left, then the rest. Returns the bytes written, at most
// 3 * (len / 64 + 2).
HX_SNAPPY_HD inline uint32_t snappy_emit_copy(uint8_t* d, uint32_t offset,
                                              uint32_t len) {
    uint32_t k = 0;
    while (len >= 68) {
        k += snappy_emit_copy1(d + k, offset, 64);
        len -= 64;
    }
    if (len > 64) {
        k += snappy_emit_copy1(d + k, offset, 60);
        len -= 60;
    }
    k += snappy_emit_copy1(d + k, offset, len);
    return k;
}

// Bytes of the stored form of an n-byte page: {varint(n), one literal}.
HX_SNAPPY_HD inline uint32_t snappy_stored_size(uint32_t n) {
    uint8_t t[8];
    uint32_t k = snappy_emit_varint(t, n);
    if (n) k += snappy_emit_literal_tag(t, n) + n;
    return k;
}

}  // namespace hx
