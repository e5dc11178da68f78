// ba_pages.h — host twin of kernel 1f (k_ba_page_sizes / k_ba_build_pages in
// kernels.hip): the PLAIN BYTE_ARRAY page images of a Binary
// `value` column, built from per-row handles. No GPU header is included; the
// stand-alone check (ba_pages_check.cpp) compiles this file with a host
// compiler under ASan/UBSan. Further down: the rule that cuts a row group's
// image into data pages with kernel 1h's twin (ba_multipage_check.cpp), and
// kernel 1g's twin.
//
// A handle is what k_ba_offsets leaves per row: (offset << 20) | length, the
// offset relative to a source base of src_size bytes. The 20 length bits are
// the limit every writer of this library enforces: no value, and no Append
// concatenation, of 2^20 bytes or more is ever written, because the reader
// could not describe it.
//
// Output row i is source row i, or with group_start (n_out + 1 entries) the
// concatenation of source rows [group_start[i], group_start[i + 1]) in that
// order under ONE length prefix (BytesMergeOperator::merge). The page of
// output row group g (rows [g * R, min(n_out, (g + 1) * R))) is, per row,
// u32 length little-endian followed by the bytes, back to back; page g starts
// at page_off[g] of one contiguous image of page_off[n_pages] bytes.
//
// The two passes and their rules are the kernels', statement by statement:
//   sizes  row_len[i] = the row's byte count, or BA_ROW_SKIP when the row is
//          refused: a group_start pair that decreases or passes n_src (one
//          error per pair), a handle that does not fit the source (one error
//          per such HANDLE, so a group with k of them counts k), or a
//          concatenation above BA_MAX_VALUE_LEN (one over-cap row; not
//          counted for a row already refused for a handle). A
//          refused row is written as an empty value and none of its handles
//          is followed.
//   build  a page above BA_MAX_PAGE_BYTES is left unwritten (the caller has
//          refused it from page_off before it gets here).
#pragma once
#include <cstdint>
#include <cstring>

namespace hx {

constexpr uint32_t BA_LEN_BITS = 20;
constexpr uint32_t BA_LEN_MASK = (1u << BA_LEN_BITS) - 1u;
// the longest value a handle can describe: 2^20 - 1 bytes
constexpr uint32_t BA_MAX_VALUE_LEN = BA_LEN_MASK;
// Parquet's page sizes are i32, and so is BaPageDesc::src_len's use of them
constexpr uint64_t BA_MAX_PAGE_BYTES = 0x7FFFFFFFull;
constexpr uint32_t BA_ROW_SKIP = 0x80000000u;
// rows per row group the build pass can hold offsets for (32 KB of LDS)
constexpr uint32_t BA_MAX_ROW_GROUP = 8192;

struct BaPagesCounts {
    uint64_t n_errors;     // bad handles + bad group_start pairs
    uint64_t n_over_cap;   // rows whose concatenation exceeds BA_MAX_VALUE_LEN
};

inline uint64_t ba_n_pages(uint64_t n_out, uint64_t R) {
    return R ? (n_out + R - 1) / R : 0;
}

// row_len: n_out words; page_off: n_pages + 1 words (exclusive scan of the
// page sizes, the total last).
inline BaPagesCounts ba_page_sizes_host(uint64_t src_size,
                                        const uint64_t* handles,
                                        uint64_t n_src,
                                        const uint32_t* group_start,
                                        uint64_t n_out, uint64_t R,
                                        uint32_t* row_len,
                                        uint64_t* page_off) {
    BaPagesCounts c{0, 0};
    const uint64_t n_pages = ba_n_pages(n_out, R);
    uint64_t total = 0;
    for (uint64_t g = 0; g < n_pages; g++) {
        page_off[g] = total;
        const uint64_t r1 = (g + 1) * R < n_out ? (g + 1) * R : n_out;
        for (uint64_t i = g * R; i < r1; i++) {
            const uint64_t a = group_start ? group_start[i] : i;
            const uint64_t b = group_start ? group_start[i + 1] : i + 1;
            bool skip = false;
            uint64_t sum = 0;
            if (a > b || b > n_src) {
                c.n_errors++;
                skip = true;
            } else {
                for (uint64_t j = a; j < b; j++) {
                    const uint64_t h = handles[j];
                    const uint64_t off = h >> BA_LEN_BITS;
                    const uint64_t len = h & BA_LEN_MASK;
                    if (off > src_size || len > src_size - off) {
                        c.n_errors++;
                        skip = true;
                    }
                    sum += len;
                }
                if (!skip && sum > BA_MAX_VALUE_LEN) {
                    c.n_over_cap++;
                    skip = true;
                }
            }
            row_len[i] = skip ? BA_ROW_SKIP : uint32_t(sum);
            total += 4 + (skip ? 0 : sum);
        }
    }
    page_off[n_pages] = total;
    return c;
}

// out: page_off[n_pages] bytes. Reads nothing outside [src, src + src_size),
// writes nothing outside a page's own [page_off[g], page_off[g + 1]).
inline void ba_build_pages_host(const uint8_t* src, uint64_t src_size,
                                const uint64_t* handles, uint64_t n_src,
                                const uint32_t* group_start, uint64_t n_out,
                                uint64_t R, const uint32_t* row_len,
                                const uint64_t* page_off, uint8_t* out) {
    const uint64_t n_pages = ba_n_pages(n_out, R);
    for (uint64_t g = 0; g < n_pages; g++) {
        if (page_off[g + 1] - page_off[g] > BA_MAX_PAGE_BYTES) continue;
        uint8_t* p = out + page_off[g];
        const uint64_t r1 = (g + 1) * R < n_out ? (g + 1) * R : n_out;
        for (uint64_t i = g * R; i < r1; i++) {
            const bool skip = (row_len[i] & BA_ROW_SKIP) != 0;
            const uint32_t len = skip ? 0u : row_len[i];
            p[0] = uint8_t(len);
            p[1] = uint8_t(len >> 8);
            p[2] = uint8_t(len >> 16);
            p[3] = uint8_t(len >> 24);
            p += 4;
            if (skip) continue;
            const uint64_t a = group_start ? group_start[i] : i;
            const uint64_t b = group_start ? group_start[i + 1] : i + 1;
            uint32_t pos = 0;
            for (uint64_t j = a; j < b && j < n_src; j++) {
                const uint64_t off = handles[j] >> BA_LEN_BITS;
                const uint32_t l = uint32_t(handles[j] & BA_LEN_MASK);
                if (off > src_size || l > src_size - off || l > len - pos)
                    break;
                if (l) std::memcpy(p + pos, src + off, l);
                pos += l;
            }
            p += len;
        }
    }
}

// ---------------------------------------------------------------------------
// Data pages of a value chunk (kernel 1h). A row group's image may
// be cut into several data pages, by the rule arrow-cpp's column writer
// applies (and, to our knowledge, parquet-rs: DESIGN §10): rows are taken in
// batches of BA_CUT_BATCH counted from the row group's first row; a row adds
// 4 + len to the open page (4 for a BA_ROW_SKIP row); after a batch, a page
// that has reached `limit` bytes closes if rows remain; the last page closes
// at the row group's end. So there are at most ceil(rows / 1024) pages, none
// of them empty, and the cuts are a pure function of the rows. limit 0 means
// one page per row group. This is the one statement of the rule: it works on
// the per-batch byte sums, which the host computes from row_len
// (ba_batch_sizes_host) and the device with k_ba_batch_sizes.
// ---------------------------------------------------------------------------
constexpr uint32_t BA_CUT_BATCH = 1024;
constexpr uint32_t BA_PAGE_LIMIT_MAX = 1u << 30;

inline uint64_t ba_batches_per_group(uint64_t R) {
    return (R + BA_CUT_BATCH - 1) / BA_CUT_BATCH;
}
// batches of n_out rows in row groups of R: every row group but the last is
// full, batch b covers rows [g * R + j * 1024, ...) with g = b / per_group,
// j = b % per_group, clipped to its row group and to n_out
inline uint64_t ba_n_batches(uint64_t n_out, uint64_t R) {
    const uint64_t n_rg = ba_n_pages(n_out, R);
    if (n_rg == 0) return 0;
    const uint64_t last = n_out - (n_rg - 1) * R;
    return (n_rg - 1) * ba_batches_per_group(R) +
           (last + BA_CUT_BATCH - 1) / BA_CUT_BATCH;
}

// Host twin of k_ba_batch_sizes: batch_sum[ba_n_batches(n_out, R)].
inline void ba_batch_sizes_host(const uint32_t* row_len, uint64_t n_out,
                                uint64_t R, uint64_t* batch_sum) {
    const uint64_t per = ba_batches_per_group(R);
    const uint64_t n_b = ba_n_batches(n_out, R);
    for (uint64_t b = 0; b < n_b; b++) {
        const uint64_t g = b / per, j = b % per;
        const uint64_t r0 = g * R + j * BA_CUT_BATCH;
        uint64_t r1 = r0 + BA_CUT_BATCH;
        if (r1 > (g + 1) * R) r1 = (g + 1) * R;
        if (r1 > n_out) r1 = n_out;
        uint64_t sum = 0;
        for (uint64_t i = r0; i < r1; i++)
            sum += 4ull + ((row_len[i] & BA_ROW_SKIP) ? 0u : row_len[i]);
        batch_sum[b] = sum;
    }
}

// THE RULE, for one row group of `rows` rows whose batches' byte sums are
// batch_sum[0, ceil(rows / 1024)). Writes the pages' row counts and byte
// sizes (room for ceil(rows / 1024) entries each, at least one) and returns
// the number of pages: 0 only for rows == 0.
inline uint32_t ba_cut_pages(const uint64_t* batch_sum, uint64_t rows,
                             uint32_t limit, uint32_t* page_rows,
                             uint64_t* page_bytes) {
    uint32_t k = 0;
    uint64_t open_rows = 0, open_bytes = 0;
    for (uint64_t r0 = 0, j = 0; r0 < rows; r0 += BA_CUT_BATCH, j++) {
        const uint64_t n = rows - r0 < BA_CUT_BATCH ? rows - r0 : BA_CUT_BATCH;
        open_rows += n;
        open_bytes += batch_sum[j];
        const bool more = r0 + n < rows;
        if (!more || (limit != 0 && open_bytes >= limit)) {
            page_rows[k] = uint32_t(open_rows);
            page_bytes[k] = open_bytes;
            k++;
            open_rows = open_bytes = 0;
        }
    }
    return k;
}

// ---------------------------------------------------------------------------
// Host twin of kernel 1g (k_ba_page_minmax): the footer statistics of the
// page images above, one BaPageStat per page, without a walk of whole values.
//
// The writer's rule (write_table_sst's walk of an image): lexicographic order
// on unsigned bytes, a proper prefix is smaller; the chunk carries min/max
// only when both are at most BA_STAT_MAX bytes long.
//
// Here a value v is looked at through K(v), its first min(len, 65) bytes,
// under the same order, and no more than 65 bytes of any value are read.
// That gives the writer's verdict and bytes:
//   - the true min m has len <= 64: then K(m) = m, and no other value v has
//     K(v) < m without v < m. A key of 65 bytes is longer than m, so it is no
//     prefix of m, and it sorts below m only through a byte inside both,
//     which v has too. So the K-min is m (or a value equal to it).
//   - len(m) > 64: every v >= m. If a v with len(v) <= 64 had K(v) = v <=
//     K(m), then v <= K(m) <= m (a prefix is smaller), so v = m, a
//     contradiction. The K-min winner is longer than 64 bytes and the
//     statistics are omitted either way.
//   - the true max M has len <= 64: K(M) = M, and every K(v) <= v <= M (a
//     prefix is never larger), so the K-max is M.
//   - len(M) > 64: K(M) has 65 bytes. A K-max winner w with len(w) <= 64
//     would be its own key, w = K(w) >= K(M); being shorter than K(M) it
//     can only be larger through a byte inside both, which M has too, so
//     w > M: a contradiction. The winner is longer than 64 bytes and the
//     statistics are omitted either way.
// has = 0 (no min/max for the chunk) leaves the lengths 0 and the bytes zero;
// unused bytes of min/max are zero, so twin and kernel compare as memory.
// A refused row (BA_ROW_SKIP) is the empty value its page carries. A row that
// would not fit its page (never true for sizes from the size pass over the
// same arrays) is left out.
// ---------------------------------------------------------------------------
constexpr uint32_t BA_STAT_MAX = 64;

struct BaPageStat {
    uint32_t has, min_len, max_len;
    uint8_t min[BA_STAT_MAX];
    uint8_t max[BA_STAT_MAX];
};
static_assert(sizeof(BaPageStat) == 140, "BaPageStat is 140 bytes");

// a < b on keys (pointer, key length <= 65)
inline bool ba_key_less(const uint8_t* a, uint32_t al, const uint8_t* b,
                        uint32_t bl) {
    const uint32_t n = al < bl ? al : bl;
    const int k = n ? std::memcmp(a, b, n) : 0;
    return k < 0 || (k == 0 && al < bl);
}

inline void ba_page_minmax_host(const uint8_t* image, const uint64_t* page_off,
                                const uint32_t* row_len, uint64_t n_out,
                                uint64_t R, BaPageStat* out) {
    const uint64_t n_pages = ba_n_pages(n_out, R);
    for (uint64_t g = 0; g < n_pages; g++) {
        BaPageStat st;
        std::memset(&st, 0, sizeof st);
        const uint64_t p_len = page_off[g + 1] - page_off[g];
        const uint8_t* page = image + page_off[g];
        const uint8_t *mn = nullptr, *mx = nullptr;
        uint32_t mn_k = 0, mx_k = 0;
        bool any = false;
        uint64_t pos = 0;
        const uint64_t r1 = (g + 1) * R < n_out ? (g + 1) * R : n_out;
        for (uint64_t i = g * R; i < r1 && p_len <= BA_MAX_PAGE_BYTES; i++) {
            const uint32_t len = (row_len[i] & BA_ROW_SKIP) ? 0u : row_len[i];
            const uint64_t o = pos;
            pos += 4ull + len;
            if (o + 4ull + len > p_len) continue;
            const uint8_t* v = page + o + 4;
            const uint32_t kl = len < BA_STAT_MAX + 1 ? len : BA_STAT_MAX + 1;
            if (!any || ba_key_less(v, kl, mn, mn_k)) mn = v, mn_k = kl;
            if (!any || ba_key_less(mx, mx_k, v, kl)) mx = v, mx_k = kl;
            any = true;
        }
        if (any && mn_k <= BA_STAT_MAX && mx_k <= BA_STAT_MAX) {
            st.has = 1;
            st.min_len = mn_k;
            st.max_len = mx_k;
            if (mn_k) std::memcpy(st.min, mn, mn_k);
            if (mx_k) std::memcpy(st.max, mx, mx_k);
        }
        out[g] = st;
    }
}

}  // namespace hx
