// nullable_write_check.cpp — stand-alone host check of the nullable write
// side: hx::encode_def_levels against the level decoder of the read side
// (hx_levels_to_bitmap), hx::pack_optional_host against a scalar loop, and
// one file from hx::write_metric_sst_nullable parsed back with
// parquet_meta.cpp. Built by `make nullable_write_check` with
// -fsanitize=address,undefined when the runtime is available; every buffer
// handed to the code under test is an exact-size heap allocation so a read or
// write outside it trips the sanitizer. Prints one line per case, exits
// non-zero on any mismatch.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <unistd.h>
#include <vector>

#include "def_levels.h"
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

const char* const kPatterns[] = {
    "all_present", "all_null",       "one_null_first", "one_null_last",
    "one_null_mid", "one_present",   "alternating",    "null_word_first_bit",
    "null_word_last_bit", "null_group_first_row", "null_group_last_row",
    "random30"};
const int kNPatterns = sizeof(kPatterns) / sizeof(kPatterns[0]);

// validity of row r of n under pattern k (row groups of `rg` rows)
std::vector<int> pattern(int k, uint32_t n, uint32_t rg) {
    std::vector<int> v(n, 1);
    switch (k) {
        case 0: break;
        case 1: v.assign(n, 0); break;
        case 2: v[0] = 0; break;
        case 3: v[n - 1] = 0; break;
        case 4: v[n / 2] = 0; break;
        case 5: v.assign(n, 0); v[n / 3] = 1; break;
        case 6: for (uint32_t r = 0; r < n; r++) v[r] = r & 1; break;
        case 7: for (uint32_t r = 0; r < n; r += 64) v[r] = 0; break;
        case 8: for (uint32_t r = 63; r < n; r += 64) v[r] = 0; break;
        case 9: for (uint32_t r = 0; r < n; r += rg) v[r] = 0; break;
        case 10:
            for (uint32_t r = rg - 1; r < n; r += rg) v[r] = 0;
            v[n - 1] = 0;
            break;
        default:
            for (uint32_t r = 0; r < n; r++) v[r] = rnd() % 10 >= 3;
    }
    return v;
}

// encode -> decode round trip of one page of n rows
bool levels_round_trip(const std::vector<int>& bits) {
    const uint32_t n = (uint32_t)bits.size();
    const size_t nw = (size_t(n) + 63) / 64;
    uint64_t* w = new uint64_t[nw];
    uint32_t nv = 0;
    for (size_t i = 0; i < nw; i++) w[i] = 0;
    for (uint32_t r = 0; r < n; r++)
        if (bits[r]) {
            w[r >> 6] |= 1ull << (r & 63);
            nv++;
        }
    std::vector<uint8_t> enc;
    hx::encode_def_levels(w, n, nv, enc);
    bool ok = enc.size() >= 6;
    uint8_t* p = new uint8_t[enc.size()];   // exact size for the decoder
    std::memcpy(p, enc.data(), enc.size());
    uint32_t block = 0;
    ok = ok && hx_level_block_bytes(p, enc.size(), &block) == HX_LVL_OK &&
         block == enc.size();
    if (nv == n)   // the 6/7/8-byte block of a page without nulls
        ok = ok && enc.size() == (n < 64 ? 6u : n < 8192 ? 7u : 8u);
    if (nv == 0) ok = ok && enc.size() <= 8;
    uint64_t* back = new uint64_t[nw];
    for (size_t i = 0; i < nw; i++) back[i] = ~0ull;
    uint32_t nv2 = 0xDEADBEEFu;
    ok = ok && hx_levels_to_bitmap(p + 4, enc.size() - 4, n, back, &nv2) ==
                   HX_LVL_OK;
    ok = ok && nv2 == nv && std::memcmp(back, w, nw * 8) == 0;
    delete[] w;
    delete[] p;
    delete[] back;
    return ok;
}

// pack_optional_host against a scalar loop; perm_kind 0 none, 1 reversed,
// 2 random (with repeats), source validity = bits
bool pack_matches(const std::vector<int>& bits, uint32_t rg, int perm_kind) {
    const uint32_t n = (uint32_t)bits.size();
    uint64_t* values = new uint64_t[n];
    uint8_t* vb = new uint8_t[(n + 7) / 8];
    std::memset(vb, 0, (n + 7) / 8);
    for (uint32_t r = 0; r < n; r++) {
        values[r] = rnd();
        if (bits[r]) vb[r >> 3] |= uint8_t(1u << (r & 7));
    }
    uint32_t* perm = perm_kind ? new uint32_t[n] : nullptr;
    for (uint32_t r = 0; perm && r < n; r++)
        perm[r] = perm_kind == 1 ? n - 1 - r : uint32_t(rnd() % n);
    const size_t groups = (size_t(n) + rg - 1) / rg, wpg = rg / 64;
    uint64_t* packed = new uint64_t[n];
    uint64_t* bm = new uint64_t[groups * wpg];
    uint32_t* nv = new uint32_t[groups];
    for (size_t i = 0; i < groups * wpg; i++) bm[i] = ~0ull;
    const uint64_t errs = hx::pack_optional_host(values, vb, perm, n, n, rg,
                                                 packed, bm, nv);
    bool ok = errs == 0;
    for (size_t g = 0; g < groups && ok; g++) {
        const uint32_t row0 = uint32_t(g * rg);
        const uint32_t rows = n - row0 < rg ? n - row0 : rg;
        uint32_t k = 0;
        for (uint32_t r = 0; r < rg; r++) {
            const uint32_t p = r < rows ? (perm ? perm[row0 + r] : row0 + r)
                                        : 0;
            const bool present = r < rows && bits[p];
            if (bool((bm[g * wpg + (r >> 6)] >> (r & 63)) & 1) != present)
                ok = false;
            if (present && packed[row0 + k++] != values[p]) ok = false;
        }
        if (nv[g] != k) ok = false;
    }
    delete[] values;
    delete[] vb;
    delete[] perm;
    delete[] packed;
    delete[] bm;
    delete[] nv;
    return ok;
}

bool perm_error_counted() {
    uint64_t values[4] = {1, 2, 3, 4};
    uint32_t perm[4] = {3, 4, 0, 1};   // entry 1 == n_src
    uint64_t packed[4], bm[1];
    uint32_t nv[1];
    const uint64_t errs = hx::pack_optional_host(values, nullptr, perm, 4, 4,
                                                 64, packed, bm, nv);
    return errs == 1 && nv[0] == 3 && bm[0] == 0xDull && packed[0] == 4 &&
           packed[1] == 1 && packed[2] == 2;
}

// one nullable file, written and parsed back with parquet_meta.cpp
bool file_round_trip(const std::string& dir, bool per_row_seq) {
    const uint32_t n = 200, rg = 64;
    std::vector<int> bits = pattern(11, n, rg);
    for (uint32_t r = 64; r < 128; r++) bits[r] = 0;   // an all-null row group
    std::vector<uint64_t> series(n), seqs(n), values(n);
    std::vector<int64_t> ts(n);
    std::vector<uint8_t> vb((n + 7) / 8, 0);
    for (uint32_t r = 0; r < n; r++) {
        series[r] = r / 4 + 1;
        ts[r] = int64_t(r) * 1000 - 7;
        seqs[r] = 1 + r % 3;
        double d = double(r) * 0.5 - 20.0;
        std::memcpy(&values[r], &d, 8);
        if (bits[r]) vb[r >> 3] |= uint8_t(1u << (r & 7));
    }
    const size_t groups = (n + rg - 1) / rg, wpg = rg / 64;
    std::vector<uint64_t> packed(n), bm(groups * wpg);
    std::vector<uint32_t> nv(groups);
    hx::pack_optional_host(values.data(), vb.data(), nullptr, n, n, rg,
                           packed.data(), bm.data(), nv.data());
    const std::string path = dir + "/1.sst";
    hx::NullableValues v{packed.data(), bm.data(), nv.data()};
    std::string err = hx::write_metric_sst_nullable(
        path, series.data(), ts.data(), v, per_row_seq ? seqs.data() : nullptr,
        9, n, rg);
    if (!err.empty()) {
        std::printf("writer: %s\n", err.c_str());
        return false;
    }
    FILE* f = std::fopen(path.c_str(), "rb");
    if (!f) return false;
    std::fseek(f, 0, SEEK_END);
    const long size = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    std::vector<uint8_t> file(size);
    bool ok = std::fread(file.data(), 1, size, f) == size_t(size);
    std::fclose(f);
    std::remove(path.c_str());
    if (!ok) return false;
    try {
        hx::FileMetadata md = hx::parse_footer(file.data(), file.size(), size);
        ok = md.num_rows == n && md.columns.size() == 5 &&
             md.row_groups.size() == groups;
        for (size_t c = 0; ok && c < 5; c++)
            ok = md.columns[c].required == (c != 2);
        for (size_t g = 0; ok && g < groups; g++) {
            const uint32_t rows = n - g * rg < rg ? n - uint32_t(g) * rg : rg;
            const hx::ColumnChunkMeta& cm = md.row_groups[g].columns[2];
            ok = md.row_groups[g].num_rows == rows && cm.num_values == rows &&
                 cm.codec == hx::CODEC_UNCOMPRESSED &&
                 cm.total_compressed_size == cm.total_uncompressed_size;
            if (!ok) break;
            hx::ChunkPages cp;
            ok = hx::select_pages(file.data() + cm.chunk_start(),
                                  size_t(cm.total_compressed_size),
                                  cm.chunk_start(), rows, true, cm.codec,
                                  &cp) &&
                 !cp.has_dict && cp.data.num_values == int32_t(rows) &&
                 cp.data.encoding == hx::ENC_PLAIN;
            if (!ok) break;
            const uint8_t* body = file.data() + cp.data.payload_off;
            uint32_t block = 0;
            ok = hx_level_block_bytes(body, size_t(cp.data.compressed_size),
                                      &block) == HX_LVL_OK &&
                 int32_t(block) == cp.data.def_level_bytes &&
                 size_t(cp.data.compressed_size) == block + size_t(nv[g]) * 8;
            if (!ok) break;
            uint64_t back[1] = {~0ull};
            uint32_t nv2 = 0;
            ok = hx_levels_to_bitmap(body + 4, block - 4, rows, back, &nv2) ==
                     HX_LVL_OK &&
                 nv2 == nv[g] && back[0] == bm[g * wpg] &&
                 std::memcmp(body + block, packed.data() + g * rg,
                             size_t(nv[g]) * 8) == 0;
            // a chunk without a present value carries no bounds
            ok = ok && cm.has_stats == (nv[g] != 0);
        }
    } catch (const std::exception& e) {
        std::printf("parse: %s\n", e.what());
        ok = false;
    }
    return ok;
}

}  // namespace

int main() {
    for (uint32_t n = 1; n <= 300; n++) {
        bool lv = true, pk = true;
        for (int k = 0; k < kNPatterns; k++) {
            for (uint32_t rg : {64u, 128u}) {
                const std::vector<int> bits = pattern(k, n, rg);
                lv = lv && levels_round_trip(bits);
                for (int pm = 0; pm < 3; pm++)
                    pk = pk && pack_matches(bits, rg, pm);
            }
        }
        report("levels round trip, n=" + std::to_string(n), lv);
        report("host pack vs scalar loop, n=" + std::to_string(n), pk);
    }
    for (uint32_t n : {8191u, 8192u, 8193u}) {
        bool ok = true;
        for (int k = 0; k < kNPatterns; k++)
            ok = ok && levels_round_trip(pattern(k, n, 8192)) &&
                 pack_matches(pattern(k, n, 8192), 8192, 2);
        report("levels + pack, n=" + std::to_string(n), ok);
    }
    report("perm entry == n_src counts one error", perm_error_counted());

    const char* tmp = std::getenv("TMPDIR");
    std::string tmpl = std::string(tmp && *tmp ? tmp : "/tmp") +
                       "/nullable_write_check.XXXXXX";
    const char* dir = mkdtemp(&tmpl[0]);
    if (!dir) {
        report("mkdtemp", false);
    } else {
        report("nullable file parses back (constant seq)",
               file_round_trip(dir, false));
        report("nullable file parses back (per-row seq)",
               file_round_trip(dir, true));
        rmdir(dir);
    }
    if (g_fail) {
        std::printf("%d FAILED\n", g_fail);
        return 1;
    }
    std::printf("ALL OK\n");
    return 0;
}
