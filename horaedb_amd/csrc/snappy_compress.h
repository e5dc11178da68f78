// snappy_compress.h — host twin of kernel 1e (k_snappy_compress, kernels.hip;
// DESIGN §4). The compressed bytes of a page are a pure function of the page
// bytes, and this function and the kernel produce the same bytes: the kernel
// examines 64 positions per step, one per lane, and this twin walks the same
// 64 positions in a loop, with the same candidates, the same ranking and the
// same table updates. Header-only; includes only snappy_emit.h (the emitters
// shared with the kernel) so it compiles stand-alone under a host compiler.
//
//   H[4096] = 0                      position + 1, 0 = empty
//   pos = lit_start = 0
//   while pos + 4 <= n:
//     end = min(pos + 64, n - 3)
//     per p in [pos, end): w = load32(p); candidates p - d for d = 8, 16 ..
//       64 (p >= d, load32 equal) and t = H[hash(w)] - 1 (t >= 0, p - t <=
//       65535, load32 equal); a candidate's rank is its common prefix with
//       p, capped at 16 and at n - p; best(p) = longest, ties to the
//       smallest distance
//     first = lowest p with a best of >= 8, else lowest p with any
//     none:  insert every p of [pos, end); pos = end
//     else:  L = full common prefix of first and its best, up to n
//            literal [lit_start, first), copy (first - best, L)
//            insert p of [pos, min(end, first + L)); lit_start = pos =
//            first + L
//   literal [lit_start, n)
//   a stream not shorter than the stored form {varint(n), one literal} is
//   replaced by it (what hx_snappy_stored_literal recognises)
//
// Output bound. This function writes dst without a check per element: cap >=
// 32 + n + n / 6 is tested once, and no prefix of the stream can pass it. A
// copy element takes at most 3 bytes for at least 4 source bytes, so every
// copy saves at least one byte; a literal of l bytes costs l + 1 up to l = 60
// and at most l + 5 above that, and between two literals there is always a
// copy. So an element pair {literal, copy} expands by at most 4 bytes, and
// only when it covers more than 64 source bytes: under n / 16 in all, plus
// the 5-byte preamble and the last literal's tag, which is below 32 + n / 6.
// The kernel walks the same steps but checks every emit against its slot all
// the same (a device write out of bounds is not a risk to take on an
// argument); with cap at the bound that path is never taken, so the bytes
// do not differ.
//
// Only consumed positions enter the table, and an insert is max-wins (the
// kernel's LDS atomicMax), so the table never depends on lane order.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "snappy_emit.h"

namespace hx {

// Compresses src[0, n) into dst[0, cap). Returns the stream's size, or 0 when
// cap is below snappy_max_compressed(n) (nothing is written then; a stream is
// never empty, n = 0 gives the single byte 00). Reads nothing outside
// src[0, n), writes nothing outside dst[0, returned size).
inline size_t snappy_compress_host(const uint8_t* src, size_t n, uint8_t* dst,
                                   size_t cap) {
    if (n > 0xFFFFFFFFull || cap < snappy_max_compressed(n)) return 0;
    const uint32_t N = uint32_t(n);
    auto load32 = [&](uint32_t p) {
        uint32_t w;
        std::memcpy(&w, src + p, 4);
        return w;
    };
    auto emit_literal = [&](size_t o, uint32_t from, uint32_t to) {
        o += snappy_emit_literal_tag(dst + o, to - from);
        std::memcpy(dst + o, src + from, to - from);
        return o + (to - from);
    };
    const uint32_t stored = snappy_stored_size(N);
    size_t o = snappy_emit_varint(dst, N);
    uint32_t H[SNAPPY_HASH_SIZE];
    std::memset(H, 0, sizeof(H));
    uint32_t pos = 0, lit_start = 0;
    while (uint64_t(pos) + 4 <= N) {
        const uint32_t end =
            N - 3 - pos < SNAPPY_CHUNK ? N - 3 : pos + SNAPPY_CHUNK;
        uint32_t first = 0, first_c = 0, any = 0, any_c = 0;
        bool have8 = false, have_any = false;
        for (uint32_t p = pos; p < end && !have8; p++) {
            const uint32_t w = load32(p);
            const uint32_t lim =
                N - p < SNAPPY_PROBE_CAP ? N - p : SNAPPY_PROBE_CAP;
            uint32_t best_len = 0, best_c = 0;
            auto probe = [&](uint32_t c) {
                if (load32(c) != w) return;
                uint32_t len = 4;
                while (len < lim && src[c + len] == src[p + len]) len++;
                if (len > best_len || (len == best_len && c > best_c)) {
                    best_len = len;
                    best_c = c;
                }
            };
            for (uint32_t d = 8; d <= 64; d += 8)
                if (p >= d) probe(p - d);
            const uint32_t h = H[snappy_hash(w)];
            if (h && p - (h - 1) <= SNAPPY_MAX_OFFSET) probe(h - 1);
            if (best_len >= 8) {
                have8 = true;
                first = p;
                first_c = best_c;
            } else if (best_len && !have_any) {
                have_any = true;
                any = p;
                any_c = best_c;
            }
        }
        if (!have8 && have_any) {
            first = any;
            first_c = any_c;
        }
        uint32_t ins_end = end;
        if (have8 || have_any) {
            uint32_t L = 4;
            while (first + L < N && src[first_c + L] == src[first + L]) L++;
            if (first > lit_start) o = emit_literal(o, lit_start, first);
            o += snappy_emit_copy(dst + o, first - first_c, L);
            if (first + L < end) ins_end = first + L;
            lit_start = first + L;
        }
        for (uint32_t p = pos; p < ins_end; p++) {
            uint32_t& e = H[snappy_hash(load32(p))];
            if (p + 1 > e) e = p + 1;
        }
        pos = (have8 || have_any) ? lit_start : end;
    }
    if (lit_start < N) o = emit_literal(o, lit_start, N);
    if (o >= stored) {
        o = snappy_emit_varint(dst, N);
        if (N) o = emit_literal(o, 0, N);
    }
    return o;
}

}  // namespace hx
