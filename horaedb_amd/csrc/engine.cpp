// engine.cpp — C-ABI implementation (include/horaedb_hx.h): catalog (replaces
// ObjectBasedStorage::try_new + Manifest::find_ssts), staging (replaces the
// ParquetExec reader factory, read.rs:78-93, incl. the reference's row-group
// pruning pushdown read.rs:459-470), and the GPU execution path (DESIGN.md
// §3-§5). Compute is GPU-only; no CPU fallback exists here. Of staging, this
// file keeps the slot layout, the reader threads and the upload; what happens
// to one column chunk between its bytes and its descriptors (page walk, host
// codec step, definition levels, Zstd via dlopen) is stage_chunk.{h,cpp},
// which needs no GPU to build or run.
#include "../../include/horaedb_hx.h"
#include "parquet_meta.h"
#include "parquet_writer.h"
#include "snappy_compress.h"
#include "hx_device.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <dirent.h>
#include <fcntl.h>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <unistd.h>
#include <vector>

#include "hx_kernels.h"
#include "hx_internal.h"
#include "stage_chunk.h"
#include "def_levels.h"
#include "ba_pages.h"
#include "first_last.h"

using hx::align64;
using hx::ChunkRef;

// ---------------------------------------------------------------------------
// error plumbing
// ---------------------------------------------------------------------------
static thread_local std::string g_last_error;

extern "C" const char* hx_last_error(void) { return g_last_error.c_str(); }

static hx_status fail(hx_status code, const std::string& msg) {
    g_last_error = msg;
    return code;
}

#define HIP_TRY(expr)                                                         \
    do {                                                                      \
        hipError_t _e = (expr);                                               \
        if (_e != hipSuccess)                                                 \
            return fail(HX_ERR_HIP, std::string(#expr) + ": " +               \
                                        hipGetErrorString(_e));               \
    } while (0)

// the same inside a function that returns the hipError_t itself
#define HIP_RET(expr)                                                         \
    do {                                                                      \
        hipError_t _e = (expr);                                               \
        if (_e != hipSuccess) return _e;                                      \
    } while (0)

// ---------------------------------------------------------------------------
// catalog (hx_open)
// ---------------------------------------------------------------------------
namespace {

struct CatRg {
    int64_t n_rows = 0;
    int64_t ts_min = 0, ts_max = 0;
    bool has_ts_stats = false;
    ChunkRef cols[4];  // series, ts, value, __seq__ (staged only if mixed)
    bool seq_mixed = false;  // __seq__ stats absent or min != max
};

struct CatSst {
    std::string path;
    uint64_t seq = 0;
    int64_t n_rows = 0;
    int64_t ts_min = 0, ts_max = 0;
    bool series_stats_ok = true;    // every chunk has series stats
    uint64_t series_max = 0;        // max over chunks (unsigned order)
    bool seq_mixed = false;         // any rg with non-constant __seq__
    bool bytes_value = false;       // value column is BYTE_ARRAY (Binary
                                    // value schema, BytesMergeOperator /
                                    // Append stores — operator.rs:47-111)
    std::vector<CatRg> rgs;
};

}  // namespace

struct hx_handle {
    std::string store;
    int64_t segment_ms = 0;
    int32_t update_mode = 0;             // 0 Overwrite / 1 Append
                                         // (config.rs:166-172)
    bool bytes_value = false;            // value column is BYTE_ARRAY
    int32_t nullable_values = 0;         // writer setting: 1 = every SST this
                                         // handle writes declares `value`
                                         // OPTIONAL (hx_set_nullable_values)
    int32_t write_codec = 0;             // writer setting: page codec of
                                         // every SST this handle writes
                                         // (hx_set_write_codec)
    int32_t bytes_write_codec = 0;       // the same for the Binary writers
                                         // (hx_set_bytes_write_codec)
    uint32_t bytes_page_limit = 0;       // data-page limit of their value
                                         // chunks (hx_set_bytes_page_limit)
    std::vector<CatSst> ssts;            // ascending seq
    std::vector<hx_sst_desc> find_out;   // scratch for hx_find_ssts
};

namespace hx_int {
hx_status set_error(hx_status code, const std::string& msg) {
    return fail(code, msg);
}
const std::string& store_path(hx_handle* h) { return h->store; }
}  // namespace hx_int

static hx_status read_file_meta(const std::string& path, uint64_t seq,
                                CatSst& out) {
    int fd = open(path.c_str(), O_RDONLY);
    if (fd < 0) return fail(HX_ERR_IO, "open " + path);
    off_t fsize = lseek(fd, 0, SEEK_END);
    uint8_t tail8[8];
    if (fsize < 12 || pread(fd, tail8, 8, fsize - 8) != 8) {
        close(fd);
        return fail(HX_ERR_FORMAT, path + ": too small");
    }
    if (std::memcmp(tail8 + 4, "PAR1", 4) != 0) {
        close(fd);
        return fail(HX_ERR_FORMAT, path + ": missing PAR1 magic");
    }
    uint32_t flen;
    std::memcpy(&flen, tail8, 4);
    if ((int64_t)flen + 8 > fsize) {
        close(fd);
        return fail(HX_ERR_FORMAT, path + ": bad footer length");
    }
    std::vector<uint8_t> tail(flen + 8);
    if (pread(fd, tail.data(), flen + 8, fsize - 8 - flen) != (ssize_t)(flen + 8)) {
        close(fd);
        return fail(HX_ERR_IO, path + ": footer read failed");
    }
    close(fd);

    hx::FileMetadata m;
    try {
        m = hx::parse_footer(tail.data(), tail.size(), fsize);
    } catch (const std::exception& e) {
        return fail(HX_ERR_FORMAT, path + ": " + e.what());
    }

    // schema contract (types.rs:150-240): series_id/timestamp/value present,
    // INT64/INT64/DOUBLE physical
    int ci[4] = {-1, -1, -1, -1};
    for (size_t i = 0; i < m.columns.size(); i++) {
        const auto& c = m.columns[i];
        if (c.name == "series_id") ci[0] = (int)i;
        else if (c.name == "timestamp") ci[1] = (int)i;
        else if (c.name == "value") ci[2] = (int)i;
        else if (c.name == "__seq__") ci[3] = (int)i;
    }
    if (ci[0] < 0 || ci[1] < 0 || ci[2] < 0)
        return fail(HX_ERR_SCHEMA, path + ": metric schema columns missing");
    if (m.columns[ci[0]].physical_type != hx::PT_INT64 ||
        m.columns[ci[1]].physical_type != hx::PT_INT64 ||
        (m.columns[ci[2]].physical_type != hx::PT_DOUBLE &&
         m.columns[ci[2]].physical_type != hx::PT_BYTE_ARRAY))
        return fail(HX_ERR_SCHEMA, path + ": unexpected physical types");
    out.bytes_value = m.columns[ci[2]].physical_type == hx::PT_BYTE_ARRAY;

    out.path = path;
    out.seq = seq;
    out.n_rows = m.num_rows;
    bool first = true;
    for (const auto& rg : m.row_groups) {
        CatRg cr;
        cr.n_rows = rg.num_rows;
        const int n_cols_here = ci[3] >= 0 ? 4 : 3;
        for (int k = 0; k < n_cols_here; k++) {
            if ((size_t)ci[k] >= rg.columns.size())
                return fail(HX_ERR_FORMAT, path + ": column chunk missing");
            const auto& cc = rg.columns[ci[k]];
            cr.cols[k].codec = cc.codec;
            cr.cols[k].required = m.columns[ci[k]].required;
            cr.cols[k].chunk_start = cc.chunk_start();
            cr.cols[k].comp_size = cc.total_compressed_size;
            cr.cols[k].uncomp_size = cc.total_uncompressed_size;
            cr.cols[k].num_values = cc.num_values;
        }
        // per-row __seq__ detection (keep_builtin compaction outputs,
        // executor.rs:155-222): constant iff stats prove min == max
        if (ci[3] >= 0) {
            const auto& qcc = rg.columns[ci[3]];
            cr.seq_mixed = !(qcc.has_stats && qcc.stat_min.size() == 8 &&
                             qcc.stat_max.size() == 8 &&
                             qcc.stat_min == qcc.stat_max);
            if (cr.seq_mixed) out.seq_mixed = true;
        }
        const auto& secc = rg.columns[ci[0]];
        if (secc.has_stats && secc.stat_max.size() == 8) {
            uint64_t mx;
            std::memcpy(&mx, secc.stat_max.data(), 8);
            if (mx > out.series_max) out.series_max = mx;
        } else {
            out.series_stats_ok = false;
        }
        const auto& tscc = rg.columns[ci[1]];
        if (tscc.has_stats && tscc.stat_min.size() == 8 &&
            tscc.stat_max.size() == 8) {
            cr.has_ts_stats = true;
            cr.ts_min = hx::stat_i64(tscc.stat_min);
            cr.ts_max = hx::stat_i64(tscc.stat_max);
            if (first || cr.ts_min < out.ts_min) out.ts_min = cr.ts_min;
            if (first || cr.ts_max > out.ts_max) out.ts_max = cr.ts_max;
            first = false;
        }
        out.rgs.push_back(std::move(cr));
    }
    if (first) {  // no stats anywhere: unbounded range (never pruned)
        out.ts_min = INT64_MIN;
        out.ts_max = INT64_MAX;
    }
    return HX_OK;
}

extern "C" hx_status hx_open(const char* store_path, int64_t segment_duration_ms,
                             hx_handle** out) {
    if (!store_path || !out) return fail(HX_ERR_INVALID, "null argument");
    auto h = std::make_unique<hx_handle>();
    h->store = store_path;
    h->segment_ms = segment_duration_ms > 0 ? segment_duration_ms
                                            : 12ll * 3600 * 1000;  // server/config.rs:53
    std::string data_dir = h->store + "/data";
    DIR* d = opendir(data_dir.c_str());
    if (!d) return fail(HX_ERR_IO, "no data dir: " + data_dir);
    std::vector<std::pair<uint64_t, std::string>> files;
    while (dirent* e = readdir(d)) {
        std::string name = e->d_name;
        if (name.size() < 5 || name.substr(name.size() - 4) != ".sst") continue;
        errno = 0;
        char* endp = nullptr;
        uint64_t seq = strtoull(name.c_str(), &endp, 10);
        if (errno || !endp || std::string(endp) != ".sst") continue;  // sst.rs:193-205
        files.emplace_back(seq, data_dir + "/" + name);
    }
    closedir(d);
    std::sort(files.begin(), files.end());
    for (auto& [seq, path] : files) {
        CatSst c;
        hx_status st = read_file_meta(path, seq, c);
        if (st != HX_OK) return st;
        if (h->ssts.empty()) {
            h->bytes_value = c.bytes_value;
        } else if (c.bytes_value != h->bytes_value) {
            return fail(HX_ERR_SCHEMA,
                        path + ": value column type differs from the rest "
                               "of the store");
        }
        h->ssts.push_back(std::move(c));
    }
    *out = h.release();
    return HX_OK;
}

extern "C" void hx_close(hx_handle* h) { delete h; }

// UpdateMode (config.rs:166-172): selects the MergeOperator the scan plugs
// in (read.rs:482-492): Overwrite -> LastValueOperator, Append ->
// BytesMergeOperator (requires a Binary value column, operator.rs:47-111).
extern "C" hx_status hx_set_update_mode(hx_handle* h, int32_t mode) {
    if (!h || (mode != 0 && mode != 1))
        return fail(HX_ERR_INVALID, "mode: 0 Overwrite / 1 Append");
    if (mode == 1 && !h->bytes_value && !h->ssts.empty())
        return fail(HX_ERR_UNSUPPORTED,
                    "Append mode needs a Binary value column "
                    "(BytesMergeOperator, operator.rs:47-111)");
    h->update_mode = mode;
    return HX_OK;
}

// Writer setting (no reference counterpart: the reference's writer always
// declares every column nullable). 0: files as before, REQUIRED columns, and
// null values are refused on the write side. 1: `value` is written OPTIONAL
// and nulls are kept by hx_write_nullable, hx_compact and hx_compact_files.
extern "C" hx_status hx_set_nullable_values(hx_handle* h, int32_t on) {
    if (!h || (on != 0 && on != 1))
        return fail(HX_ERR_INVALID, "nullable values: 0 off / 1 on");
    if (on && h->bytes_value)
        return fail(HX_ERR_UNSUPPORTED,
                    "nullable values need an f64 value column");
    h->nullable_values = on;
    return HX_OK;
}

// Writer setting: the page codec of every SST the handle writes from now on
// (the reference's config.rs:120-133 default is Snappy). 0 launches and
// writes exactly what it always did.
extern "C" hx_status hx_set_write_codec(hx_handle* h, int32_t codec) {
    if (!h || (codec != HX_CODEC_NONE && codec != HX_CODEC_SNAPPY))
        return fail(HX_ERR_INVALID, "write codec: 0 none / 1 snappy");
    if (codec != HX_CODEC_NONE && h->bytes_value)
        return fail(HX_ERR_UNSUPPORTED,
                    "a write codec needs an f64 value column");
    h->write_codec = codec;
    return HX_OK;
}

// The Binary writers' codec (hx_write_bytes, and hx_compact /
// hx_compact_files on a Binary store); hx_set_write_codec keeps its meaning
// and its refusals. 0 launches and writes exactly what it always did.
extern "C" hx_status hx_set_bytes_write_codec(hx_handle* h, int32_t codec) {
    if (!h || (codec != HX_CODEC_NONE && codec != HX_CODEC_SNAPPY))
        return fail(HX_ERR_INVALID, "bytes write codec: 0 none / 1 snappy");
    if (codec != HX_CODEC_NONE && !h->bytes_value && !h->ssts.empty())
        return fail(HX_ERR_UNSUPPORTED,
                    "a bytes write codec needs a Binary value column");
    h->bytes_write_codec = codec;
    return HX_OK;
}

// Data-page limit of the Binary writers' value chunks (hx::ba_cut_pages).
// 0 launches and writes exactly what it always did: one page per chunk.
extern "C" hx_status hx_set_bytes_page_limit(hx_handle* h, uint32_t bytes) {
    if (!h || bytes > hx::BA_PAGE_LIMIT_MAX)
        return fail(HX_ERR_INVALID,
                    "bytes page limit: 0 (one page per chunk) or 1 .. 2^30");
    if (bytes != 0 && !h->bytes_value && !h->ssts.empty())
        return fail(HX_ERR_UNSUPPORTED,
                    "a bytes page limit needs a Binary value column");
    h->bytes_page_limit = bytes;
    return HX_OK;
}

// TimeRange::overlaps (types.rs:125-127): [start,end) vs file [min,max]
static bool overlaps(const CatSst& s, hx_time_range r) {
    return s.ts_min < r.end && s.ts_max >= r.start;
}

extern "C" hx_status hx_schema(hx_handle* h, const hx_col_desc** out,
                               size_t* n_out, size_t* n_primary_keys) {
    // the metric-engine schema contract (types.rs:150-240): 2 PKs, one f64
    // value, builtin __seq__/__reserved__ appended
    static const hx_col_desc kSchema[5] = {
        {"series_id", 0, 1, 0},   {"timestamp", 1, 1, 0},
        {"value", 2, 0, 0},       {"__seq__", 0, 0, 1},
        {"__reserved__", 0, 0, 1},
    };
    static const hx_col_desc kSchemaBytes[5] = {
        {"series_id", 0, 1, 0},   {"timestamp", 1, 1, 0},
        {"value", 3, 0, 0},       {"__seq__", 0, 0, 1},
        {"__reserved__", 0, 0, 1},
    };
    if (!h || !out || !n_out || !n_primary_keys)
        return fail(HX_ERR_INVALID, "null argument");
    *out = h->bytes_value ? kSchemaBytes : kSchema;
    *n_out = 5;
    *n_primary_keys = 2;
    return HX_OK;
}

extern "C" hx_status hx_find_ssts(hx_handle* h, hx_time_range range,
                                  const hx_sst_desc** out, size_t* n_out) {
    if (!h || !out || !n_out) return fail(HX_ERR_INVALID, "null argument");
    h->find_out.clear();
    for (const auto& s : h->ssts)
        if (overlaps(s, range))
            h->find_out.push_back({s.path.c_str(), s.seq});
    *out = h->find_out.data();
    *n_out = h->find_out.size();
    return HX_OK;
}

// ---------------------------------------------------------------------------
// prepared scan (staging)
// ---------------------------------------------------------------------------
namespace {

struct DevPlan {
    int device = 0;
    std::vector<hx::RgDesc> rgs;
    std::vector<hx::RgValid> rg_valid;   // parallel to rgs; has_nulls only
    std::vector<hx::SstDev> ssts;
    std::vector<hx::ClusterDev> clusters;
    std::vector<int32_t> cluster_members;
    std::vector<hx::DeltaPageDesc> delta_pages;
    std::vector<hx::BaPageDesc> ba_pages;   // byte-value stores: handle walk
    std::vector<hx::SnappyPageDesc> snappy_pages;
    // Snappy pages of a Binary value column, decoded into the blob's tail
    std::vector<hx::SnappyPageDesc> snappy_ba_pages;
    std::vector<hx::ExpandPageDesc> expand_pages;  // OPTIONAL PLAIN bodies
    std::vector<hx::RleDictPageDesc> rledict_pages;
    std::vector<hx::CopyDesc> copies;
    size_t blob_bytes = 0;   // staged (uploaded) bytes of d_blob
    // d_blob's whole extent: [blob_bytes, blob_span) is the decoded tail of
    // Snappy byte-value pages, never uploaded, written by ensure_decoded with
    // dec's lifetime and rewrite rules. Value handles address [0, blob_span).
    size_t blob_span = 0;
    size_t dec_bytes = 0;
    int64_t rows_scanned = 0;
    // stored Snappy pages read in place from the blob (hx_get_decode_stats)
    uint64_t pages_in_place = 0;
    uint64_t bytes_in_place = 0;
    // a value page with real nulls was staged: its validity bitmap is in the
    // blob and the null-aware kernel instances run
    bool has_nulls = false;

    // host staging
    uint8_t* h_blob = nullptr;
    bool h_blob_pinned = false;

    // device memory
    uint8_t* d_blob = nullptr;
    uint8_t* d_dec = nullptr;
    hx::RgDesc* d_rgs = nullptr;
    hx::SstDev* d_ssts = nullptr;
    hx::ClusterDev* d_clusters = nullptr;
    int32_t* d_members = nullptr;
    hx::DeltaPageDesc* d_delta = nullptr;
    hx::BaPageDesc* d_ba = nullptr;
    hx::SnappyPageDesc* d_snappy = nullptr;
    hx::SnappyPageDesc* d_snappy_ba = nullptr;
    hx::ExpandPageDesc* d_expand = nullptr;
    hx::RleDictPageDesc* d_rledict = nullptr;
    hx::CopyDesc* d_copies = nullptr;

    // aggregate table (lazily sized)
    uint32_t slots = 0;
    uint8_t* t_slab = nullptr;      // slot slab (key-claim or state-word)
    uint32_t slab_stride = 0;
    uint8_t* t_bstore = nullptr;    // direct-indexed bucket accumulators
    uint64_t bstore_cap = 0;
    // six words, zeroed per attempt. Table route: 0 fill, 1 overflow,
    // 2 matched. Sorted-run route: 0 cursor (= group count), 1 staging
    // overflow, 2 matched, 4 block overflow. Decode: 1 error flag. Word 3 is
    // free (it counted the range kernel's LDS misses until the table flush
    // was removed); 5 is unused.
    unsigned long long* d_counters = nullptr;
    uint64_t* d_sset = nullptr;
    size_t sset_cap = 0;
    uint64_t sset_empty = ~0ull;
    uint32_t sset_mask = 0;

    bool decoded = false;       // delta/copy kernels already ran
    double decode_ms = 0;

    // cached result scratch (device)
    void* d_scratch = nullptr;
    size_t scratch_cap = 0;
    void* d_sort_temp = nullptr;
    size_t sort_temp_cap = 0;

    // series-range mode (k_scan_agg_range2)
    std::vector<int32_t> h_sst_rgs;     // rg indices grouped per SST, row order
    std::vector<int32_t> h_sst_rg_off;
    std::vector<int32_t> h_sst_rg_cnt;
    int32_t* d_sst_rgs = nullptr;
    int32_t* d_sst_rg_off = nullptr;
    int32_t* d_sst_rg_cnt = nullptr;
    uint64_t* d_range_bounds = nullptr;   // n_blocks+1 series boundaries
    uint64_t* d_bound_rows = nullptr;     // (n_blocks+1) x n_ssts packed
    uint32_t range_nblocks = 0;
    double range_xest = 0;   // distinct-series estimate (sizes the table)
    bool range_ready = false;
    uint64_t sorted_cap = 0;       // sorted-run staging capacity that fit
    bool sorted_gave_up = false;   // retries ran out once: global-table route

    hipStream_t stream = nullptr;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};  // timing
};

static hx_status ensure_dev(void** p, size_t* cap, size_t need) {
    if (*cap >= need) return HX_OK;
    if (*p) hipFree(*p);
    *p = nullptr;
    *cap = 0;
    HIP_TRY(hipMalloc(p, need));
    *cap = need;
    return HX_OK;
}

struct StagedSst {  // host-side bookkeeping per prepared SST
    const CatSst* cat;
    std::vector<int> rg_idx;   // selected row groups (ascending)
    int64_t staged_rows = 0;
    int32_t cluster = -1;
    int32_t rank = 0;
    int dev_slot = -1;         // index into DevPlan.ssts
    int plan = -1;             // which DevPlan
    uint64_t bytes_handles = 0;  // dec offset of the value-handle array
                                 // (byte-value stores only)
};

}  // namespace

struct hx_prepared {
    hx_handle* h = nullptr;
    bool key_claim_safe = true;   // no staged series_id == ~0 (proven by stats)
    hx_scan_spec spec{};
    std::vector<uint64_t> sset_keys;   // owned copy of series-set predicate
    std::vector<DevPlan> plans;
    int64_t rows_scanned_total = 0;
    int64_t bytes_staged = 0;
    double stage_ms = 0;
    hx_exec_stats last_stats{};
};

static int hip_device_count() {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

namespace {

struct PageJob {  // one (rg, col) column chunk to read + stage
    StagedSst* ss;
    const ChunkRef* cr;
    hx::ChunkRole role;
    size_t dst_off;      // blob offset of its slot, hx::chunk_reserve bytes
    size_t bitmap_off;   // blob offset of its validity words, 0 = none
};

}  // namespace

// Layout pass: SstDev / RgDesc entries in plan order, the dense dec arrays
// of each SST, and one job with a blob slot per staged column chunk (3 per
// row group, 4 where per-row seqs are staged). Returns the dec bytes laid out
// so far; the decode targets are reserved behind them during the page walk
// (which chunks need one is not known until their headers are read).
static size_t layout_jobs(hx_prepared* P, DevPlan& plan,
                          std::vector<StagedSst*>& members,
                          std::vector<PageJob>& jobs) {
    const bool bytes_val = P->h->bytes_value;
    size_t blob_off = 0, dec_off = 0;
    auto dense = [&](int64_t rows) {
        const uint64_t off = dec_off;
        dec_off = align64(dec_off + size_t(rows) * 8);
        return off;
    };
    for (StagedSst* ss : members) {
        hx::SstDev sd{};
        sd.cluster = ss->cluster;
        sd.rank = ss->rank;
        sd.seq = ss->cat->seq;
        sd.n_staged = ss->staged_rows;
        const bool need_dense = ss->cluster >= 0;
        // per-row seqs are only consulted by the cross-SST dedup, so they
        // are staged only for overlap-cluster members with mixed seqs
        const bool need_seq = need_dense && ss->cat->seq_mixed;
        if (need_dense) {
            sd.dense_series = hx::OFF_DEC | dense(ss->staged_rows);
            sd.dense_ts = hx::OFF_DEC | dense(ss->staged_rows);
        }
        if (need_seq) sd.dense_seq = hx::OFF_DEC | dense(ss->staged_rows);
        if (bytes_val) ss->bytes_handles = dense(ss->staged_rows);
        ss->dev_slot = (int)plan.ssts.size();
        plan.ssts.push_back(sd);

        int64_t row_base = 0;
        int prev_rg_desc = -1;
        for (int rgi : ss->rg_idx) {
            const CatRg& rg = ss->cat->rgs[rgi];
            hx::RgDesc rd{};
            rd.n_rows = (uint32_t)rg.n_rows;
            rd.sst_id = (uint32_t)ss->dev_slot;
            rd.row_base = row_base;
            rd.next_rg = -1;
            int this_desc = (int)plan.rgs.size();
            if (prev_rg_desc >= 0) plan.rgs[prev_rg_desc].next_rg = this_desc;
            prev_rg_desc = this_desc;
            plan.rgs.push_back(rd);
            for (int c = 0; c < (need_seq ? 4 : 3); c++) {
                PageJob j{};
                j.ss = ss;
                j.cr = &rg.cols[c];
                j.role.col = c;
                j.role.bytes_value = bytes_val;
                j.role.update_mode = P->h->update_mode;
                j.role.row_base = row_base;
                j.role.bytes_handles = ss->bytes_handles;
                j.dst_off = blob_off;
                blob_off = align64(blob_off + hx::chunk_reserve(*j.cr));
                if (const size_t bm = hx::bitmap_reserve(*j.cr, c, bytes_val)) {
                    j.bitmap_off = blob_off;
                    blob_off = align64(blob_off + bm);
                }
                jobs.push_back(j);
            }
            row_base += rg.n_rows;
            plan.rows_scanned += rg.n_rows;
        }
    }
    plan.blob_bytes = blob_off;
    return dec_off;
}

// Read + page walk, parallel over jobs: each worker claims a job, reads the
// chunk and stages it into the job's slot (stage_chunk.h). Workers share the
// dec cursor (atomic) and the error string; each collects descriptors in a
// bundle of its own, and the plan takes the bundles one after the other once
// all have joined. Descriptor order therefore depends on thread timing, as it
// always has: every decode kernel takes one descriptor per wave or workgroup
// and none looks at its neighbours, so the order carries no meaning.
static hx_status stage_chunks(DevPlan& plan, const std::vector<PageJob>& jobs,
                              std::vector<hx::ChunkResult>& results,
                              std::atomic<size_t>& dec,
                              std::atomic<size_t>& tail) {
    const unsigned n_threads = std::min<unsigned>(
        16, std::max(1u, std::thread::hardware_concurrency()));
    std::vector<hx::StagedPages> bundles(n_threads);
    std::atomic<size_t> next{0};
    std::atomic<int> err_flag{0};
    std::mutex mu;  // guards the error string, nothing else
    std::string err_msg;
    auto worker = [&](hx::StagedPages& out) {
        std::vector<uint8_t> tmp;
        int fd = -1;
        const CatSst* cat = nullptr;
        for (;;) {
            const size_t i = next.fetch_add(1);
            if (i >= jobs.size() || err_flag.load()) break;
            const PageJob& j = jobs[i];
            if (cat != j.ss->cat) {
                if (fd >= 0) close(fd);
                cat = j.ss->cat;
                fd = open(cat->path.c_str(), O_RDONLY);
            }
            hx::StageStatus s;
            if (fd < 0)
                s.msg = "open " + cat->path;
            else
                s = hx::read_chunk(fd, cat->path, *j.cr, tmp);
            if (s.ok()) {
                hx::ChunkSlot slot;
                slot.base = plan.h_blob + j.dst_off;
                slot.off = j.dst_off;
                slot.cap = hx::chunk_reserve(*j.cr);
                if (j.bitmap_off) {
                    slot.bitmap = (uint64_t*)(plan.h_blob + j.bitmap_off);
                    slot.bitmap_off = j.bitmap_off;
                    slot.bitmap_cap = hx::bitmap_reserve(
                        *j.cr, j.role.col, j.role.bytes_value);
                }
                s = hx::stage_chunk(tmp.data(), *j.cr, j.role, slot, dec, out,
                                    results[i], &tail);
                if (!s.ok()) s.msg = cat->path + ": " + s.msg;
            }
            if (!s.ok()) {
                std::lock_guard<std::mutex> g(mu);
                err_msg = s.msg;
                err_flag = 1;
                break;
            }
        }
        if (fd >= 0) close(fd);
    };
    {
        std::vector<std::thread> ts;
        for (auto& b : bundles) ts.emplace_back(worker, std::ref(b));
        for (auto& t : ts) t.join();
    }
    if (err_flag.load()) return fail(HX_ERR_UNSUPPORTED, err_msg);
    auto append = [](auto& dst, const auto& src) {
        dst.insert(dst.end(), src.begin(), src.end());
    };
    for (const hx::StagedPages& b : bundles) {
        append(plan.snappy_pages, b.snappy);
        append(plan.snappy_ba_pages, b.snappy_ba);
        append(plan.expand_pages, b.expand);
        append(plan.delta_pages, b.delta);
        append(plan.rledict_pages, b.rledict);
        append(plan.ba_pages, b.ba);
        plan.pages_in_place += b.pages_in_place;
        plan.bytes_in_place += b.bytes_in_place;
    }
    for (const hx::ChunkResult& r : results)
        if (r.has_nulls) plan.has_nulls = true;
    return HX_OK;
}

// RgDesc offsets from the chunk results, then the unit list the kernels run
// over (stage_chunk.h has both; HX_RG_SPLIT sets the slices per row group).
static void slice_and_order(DevPlan& plan,
                            const std::vector<hx::ChunkResult>& results) {
    hx::patch_rg_offsets(plan.rgs, plan.rg_valid, plan.ssts, results,
                         plan.copies);
    uint32_t split = 2;   // ~4096-row units
    if (const char* se = getenv("HX_RG_SPLIT"))
        split = (uint32_t)strtoul(se, nullptr, 10);
    hx::SstRgLists lists;
    hx::slice_and_order(plan.rgs, plan.rg_valid, plan.ssts.size(), split,
                        lists);
    plan.h_sst_rgs.swap(lists.rgs);
    plan.h_sst_rg_off.swap(lists.off);
    plan.h_sst_rg_cnt.swap(lists.cnt);
    if (!plan.has_nulls) plan.rg_valid.clear();   // nothing to upload
}

static hx_status upload_plan(DevPlan& plan) {
    HIP_TRY(hipSetDevice(plan.device));
    if (!plan.stream) HIP_TRY(hipStreamCreate(&plan.stream));
    if (plan.blob_bytes) {
        // the tail behind blob_bytes is decode output, not uploaded
        HIP_TRY(hipMalloc((void**)&plan.d_blob, plan.blob_span + 64));
        HIP_TRY(hipMemcpyAsync(plan.d_blob, plan.h_blob, plan.blob_bytes,
                               hipMemcpyHostToDevice, plan.stream));
    }
    if (plan.dec_bytes)
        HIP_TRY(hipMalloc((void**)&plan.d_dec, plan.dec_bytes + 64));
    auto upload = [&](auto*& dptr, const auto& vec) -> hipError_t {
        using T = std::remove_reference_t<decltype(vec[0])>;
        if (vec.empty()) { dptr = nullptr; return hipSuccess; }
        hipError_t e = hipMalloc((void**)&dptr, vec.size() * sizeof(T));
        if (e != hipSuccess) return e;
        return hipMemcpyAsync(dptr, vec.data(), vec.size() * sizeof(T),
                              hipMemcpyHostToDevice, plan.stream);
    };
    if (plan.has_nulls && !plan.rgs.empty()) {
        // the RgValid entries ride behind the RgDesc array (hx_device.h)
        const size_t rg_bytes = plan.rgs.size() * sizeof(hx::RgDesc);
        const size_t rv_bytes = plan.rg_valid.size() * sizeof(hx::RgValid);
        HIP_TRY(hipMalloc((void**)&plan.d_rgs, rg_bytes + rv_bytes));
        HIP_TRY(hipMemcpyAsync(plan.d_rgs, plan.rgs.data(), rg_bytes,
                               hipMemcpyHostToDevice, plan.stream));
        HIP_TRY(hipMemcpyAsync((uint8_t*)plan.d_rgs + rg_bytes,
                               plan.rg_valid.data(), rv_bytes,
                               hipMemcpyHostToDevice, plan.stream));
    } else {
        HIP_TRY(upload(plan.d_rgs, plan.rgs));
    }
    HIP_TRY(upload(plan.d_ssts, plan.ssts));
    HIP_TRY(upload(plan.d_clusters, plan.clusters));
    HIP_TRY(upload(plan.d_members, plan.cluster_members));
    HIP_TRY(upload(plan.d_delta, plan.delta_pages));
    HIP_TRY(upload(plan.d_ba, plan.ba_pages));
    HIP_TRY(upload(plan.d_snappy, plan.snappy_pages));
    HIP_TRY(upload(plan.d_snappy_ba, plan.snappy_ba_pages));
    HIP_TRY(upload(plan.d_expand, plan.expand_pages));
    HIP_TRY(upload(plan.d_rledict, plan.rledict_pages));
    HIP_TRY(upload(plan.d_copies, plan.copies));
    HIP_TRY(upload(plan.d_sst_rgs, plan.h_sst_rgs));
    HIP_TRY(upload(plan.d_sst_rg_off, plan.h_sst_rg_off));
    HIP_TRY(upload(plan.d_sst_rg_cnt, plan.h_sst_rg_cnt));
    HIP_TRY(hipMalloc((void**)&plan.d_counters, 6 * sizeof(unsigned long long)));
    HIP_TRY(hipStreamSynchronize(plan.stream));
    return HX_OK;
}

static void free_host_blob(DevPlan& plan) {
    if (!plan.h_blob) return;
    if (plan.h_blob_pinned) hipHostFree(plan.h_blob);
    else free(plan.h_blob);
    plan.h_blob = nullptr;
}

static hx_status stage_device(hx_prepared* P, DevPlan& plan,
                              std::vector<StagedSst*>& members) {
    std::vector<PageJob> jobs;
    std::atomic<size_t> dec{layout_jobs(P, plan, members, jobs)};
    if (plan.h_blob == nullptr && plan.blob_bytes > 0) {
        if (hipHostMalloc((void**)&plan.h_blob, plan.blob_bytes,
                          hipHostMallocDefault) == hipSuccess) {
            plan.h_blob_pinned = true;
        } else {
            plan.h_blob = (uint8_t*)malloc(plan.blob_bytes);
            plan.h_blob_pinned = false;
            if (!plan.h_blob) return fail(HX_ERR_IO, "staging alloc failed");
        }
    }
    std::vector<hx::ChunkResult> results(jobs.size());
    // blob_bytes is a multiple of 64 (layout_jobs), so every tail piece is
    std::atomic<size_t> tail{plan.blob_bytes};
    hx_status st = stage_chunks(plan, jobs, results, dec, tail);
    if (st != HX_OK) return st;
    plan.dec_bytes = dec.load();
    plan.blob_span = tail.load();
    if (P->h->bytes_value && uint64_t(plan.blob_span) >= (1ull << 44))
        return fail(HX_ERR_UNSUPPORTED,
                    "Binary value store: staged and decoded value pages of "
                    "one plan exceed 2^44 bytes (a value handle has 44 "
                    "offset bits)");
    slice_and_order(plan, results);
    st = upload_plan(plan);
    // staging buffer no longer needed once resident in HBM (frees up to
    // 12 GB of pinned host memory per rank for the 8-GPU runs)
    if (st == HX_OK) free_host_blob(plan);
    return st;
}

extern "C" hx_status hx_prepare(hx_handle* h, const hx_scan_spec* spec,
                                const hx_device_set* devs, hx_prepared** out) {
    if (!h || !spec || !out) return fail(HX_ERR_INVALID, "null argument");
    auto t0 = std::chrono::steady_clock::now();
    int n_gpu = hip_device_count();
    if (n_gpu <= 0)
        return fail(HX_ERR_NO_GPU, "no HIP device visible (the scan path is "
                                   "GPU-only; there is no CPU fallback)");
    std::vector<int> device_ids;
    if (devs && devs->device_ids && devs->n_devices > 0)
        device_ids.assign(devs->device_ids, devs->device_ids + devs->n_devices);
    else
        device_ids = {0};
    for (int d : device_ids)
        if (d < 0 || d >= n_gpu)
            return fail(HX_ERR_INVALID, "bad device id");

    // every early return below frees what was built so far (pinned blob,
    // device buffers and streams of the plans already staged)
    struct PreparedFree {
        void operator()(hx_prepared* p) const { hx_prepared_free(p); }
    };
    std::unique_ptr<hx_prepared, PreparedFree> P(new hx_prepared);
    P->h = h;
    // retain ONLY the fields the exec paths read (the time range): the
    // caller owns preds/ssts/projection and may free them right after this
    // call — a shallow struct copy would dangle (sset keys are deep-copied
    // into sset_keys below; the SST subset is resolved into `chosen` here)
    P->spec = hx_scan_spec{};
    P->spec.range = spec->range;
    for (size_t i = 0; i < spec->n_preds; i++) {
        const hx_pred& p = spec->preds[i];
        if (p.kind != HX_PRED_SERIES_IN)
            return fail(HX_ERR_UNSUPPORTED, "unknown predicate kind");
        P->sset_keys.insert(P->sset_keys.end(), p.series_ids,
                            p.series_ids + p.n_series);
    }

    // resolve SSTs
    std::vector<const CatSst*> chosen;
    if (spec->ssts && spec->n_ssts) {
        for (size_t i = 0; i < spec->n_ssts; i++) {
            const CatSst* found = nullptr;
            for (const auto& s : h->ssts)
                if (s.path == spec->ssts[i].path) { found = &s; break; }
            if (!found)
                return fail(HX_ERR_INVALID,
                            std::string("sst not in catalog: ") + spec->ssts[i].path);
            chosen.push_back(found);
        }
    } else {
        for (const auto& s : h->ssts)
            if (overlaps(s, spec->range)) chosen.push_back(&s);
    }

    for (const CatSst* c : chosen)
        if (!c->series_stats_ok || c->series_max == ~0ull)
            P->key_claim_safe = false;

    // select row groups (reference pushdown pruning read.rs:459-470)
    std::vector<StagedSst> staged;
    staged.reserve(chosen.size());
    for (const CatSst* c : chosen) {
        StagedSst ss;
        ss.cat = c;
        for (size_t r = 0; r < c->rgs.size(); r++) {
            const CatRg& rg = c->rgs[r];
            if (rg.has_ts_stats &&
                !(rg.ts_min < spec->range.end && rg.ts_max >= spec->range.start))
                continue;
            ss.rg_idx.push_back((int)r);
            ss.staged_rows += rg.n_rows;
        }
        if (!ss.rg_idx.empty()) staged.push_back(std::move(ss));
    }

    // overlap clusters: connected components of ts-range
    // intersection; members sorted by seq => dense ranks. Clusters are the
    // unit of device assignment (binary-search dedup needs co-location).
    size_t n = staged.size();
    std::vector<int> parent(n);
    for (size_t i = 0; i < n; i++) parent[i] = (int)i;
    std::function<int(int)> find = [&](int x) {
        while (parent[x] != x) { parent[x] = parent[parent[x]]; x = parent[x]; }
        return x;
    };
    for (size_t i = 0; i < n; i++)
        for (size_t j = i + 1; j < n; j++) {
            const CatSst* a = staged[i].cat;
            const CatSst* b = staged[j].cat;
            if (a->ts_min <= b->ts_max && b->ts_min <= a->ts_max)
                parent[find((int)i)] = find((int)j);
        }
    // group indexes by root; singleton groups get cluster = -1
    std::vector<std::vector<int>> groups;
    {
        std::vector<int> root_to_group((int)n, -1);
        for (size_t i = 0; i < n; i++) {
            int r = find((int)i);
            if (root_to_group[r] < 0) {
                root_to_group[r] = (int)groups.size();
                groups.emplace_back();
            }
            groups[root_to_group[r]].push_back((int)i);
        }
    }

    // assign groups to devices (least-loaded by staged rows)
    P->plans.resize(device_ids.size());
    for (size_t d = 0; d < device_ids.size(); d++)
        P->plans[d].device = device_ids[d];
    std::vector<int64_t> load(device_ids.size(), 0);
    std::vector<int32_t> member_count(device_ids.size(), 0);
    std::vector<std::vector<StagedSst*>> members_per_plan(device_ids.size());
    // big groups first for balance
    std::sort(groups.begin(), groups.end(), [&](const auto& a, const auto& b) {
        int64_t ra = 0, rb = 0;
        for (int i : a) ra += staged[i].staged_rows;
        for (int i : b) rb += staged[i].staged_rows;
        return ra > rb;
    });
    for (auto& g : groups) {
        size_t best = 0;
        for (size_t d = 1; d < load.size(); d++)
            if (load[d] < load[best]) best = d;
        DevPlan& plan = P->plans[best];
        // sort group members by seq => ranks
        std::sort(g.begin(), g.end(), [&](int a, int b) {
            return staged[a].cat->seq < staged[b].cat->seq;
        });
        int32_t cluster_id = -1;
        if (g.size() > 1) {
            cluster_id = (int32_t)plan.clusters.size();
            hx::ClusterDev cd{member_count[best], (int32_t)g.size()};
            member_count[best] += (int32_t)g.size();
            plan.clusters.push_back(cd);
        }
        int32_t rank = 0;
        for (int idx : g) {
            staged[idx].cluster = cluster_id;
            staged[idx].rank = rank++;
            staged[idx].plan = (int)best;
            members_per_plan[best].push_back(&staged[idx]);
            load[best] += staged[idx].staged_rows;
        }
        if (cluster_id >= 0) {
            // dev_slot not known yet; fill members after staging assigns slots
        }
    }

    for (size_t d = 0; d < P->plans.size(); d++) {
        hx_status st = stage_device(P.get(), P->plans[d], members_per_plan[d]);
        if (st != HX_OK) return st;
        // cluster member lists (dev slots) — members were pushed in group
        // order, so slots ascend within each cluster
        DevPlan& plan = P->plans[d];
        plan.cluster_members.assign(plan.ssts.size(), 0);
        {
            std::vector<int32_t> cursor(plan.clusters.size());
            for (size_t c = 0; c < plan.clusters.size(); c++)
                cursor[c] = plan.clusters[c].first;
            for (StagedSst* ss : members_per_plan[d])
                if (ss->cluster >= 0)
                    plan.cluster_members[cursor[ss->cluster]++] = ss->dev_slot;
        }
        if (!plan.cluster_members.empty()) {
            HIP_TRY(hipSetDevice(plan.device));
            if (plan.d_members) hipFree(plan.d_members);
            plan.d_members = nullptr;
            HIP_TRY(hipMalloc((void**)&plan.d_members,
                              plan.cluster_members.size() * sizeof(int32_t)));
            HIP_TRY(hipMemcpy(plan.d_members, plan.cluster_members.data(),
                              plan.cluster_members.size() * sizeof(int32_t),
                              hipMemcpyHostToDevice));
        }
        P->rows_scanned_total += plan.rows_scanned;
        P->bytes_staged += (int64_t)plan.blob_bytes;
    }
    P->stage_ms = std::chrono::duration<double, std::milli>(
                      std::chrono::steady_clock::now() - t0).count();
    *out = P.release();
    return HX_OK;
}

extern "C" void hx_prepared_free(hx_prepared* P) {
    if (!P) return;
    for (auto& plan : P->plans) {
        hipSetDevice(plan.device);
        free_host_blob(plan);
        for (void* p : {(void*)plan.d_blob, (void*)plan.d_dec, (void*)plan.d_rgs,
                        (void*)plan.d_ssts, (void*)plan.d_clusters,
                        (void*)plan.d_members, (void*)plan.d_delta,
                        (void*)plan.d_ba,
                        (void*)plan.d_snappy, (void*)plan.d_snappy_ba,
                        (void*)plan.d_expand,
                        (void*)plan.d_rledict,
                        (void*)plan.d_copies, (void*)plan.t_slab,
                        (void*)plan.t_bstore, (void*)plan.d_counters,
                        (void*)plan.d_sset, (void*)plan.d_sst_rgs,
                        (void*)plan.d_sst_rg_off, (void*)plan.d_sst_rg_cnt,
                        (void*)plan.d_range_bounds, (void*)plan.d_bound_rows,
                        plan.d_scratch, plan.d_sort_temp})
            if (p) hipFree(p);
        for (auto ev : plan.ev)
            if (ev) hipEventDestroy(ev);
        if (plan.stream) hipStreamDestroy(plan.stream);
    }
    delete P;
}

// ---------------------------------------------------------------------------
// execution (hx_exec_agg): the timed hot path — DESIGN.md §4/§8
// ---------------------------------------------------------------------------
namespace {

// Pinned result buffers are recycled process-wide: hipHostMalloc/hipHostFree
// page-lock and unlock the whole region, a multi-ms host cost per exec at
// config-2 sizes (~240 MB per result). The pool keeps a few buffers alive
// across hx_exec_agg/hx_result_free cycles. HX_HOSTPOOL=0 disables it (A/B).
struct PinnedPool {
    std::mutex mu;
    std::vector<std::pair<void*, size_t>> bufs;  // free pinned buffers
    bool enabled() {
        const char* e = getenv("HX_HOSTPOOL");
        return !(e && e[0] == '0');
    }
    void* acquire(size_t bytes, bool* pinned, size_t* cap) {
        if (enabled()) {
            std::lock_guard<std::mutex> g(mu);
            // smallest free buffer that fits
            size_t best = bufs.size();
            for (size_t i = 0; i < bufs.size(); i++)
                if (bufs[i].second >= bytes &&
                    (best == bufs.size() || bufs[i].second < bufs[best].second))
                    best = i;
            if (best < bufs.size()) {
                void* p = bufs[best].first;
                *cap = bufs[best].second;
                bufs.erase(bufs.begin() + best);
                *pinned = true;
                return p;
            }
        }
        void* p = nullptr;
        if (hipHostMalloc(&p, bytes, hipHostMallocDefault) == hipSuccess) {
            *pinned = true;
            *cap = bytes;
            return p;
        }
        *pinned = false;
        *cap = bytes;
        return malloc(bytes);
    }
    void release(void* p, size_t cap, bool pinned) {
        if (!p) return;
        if (!pinned) { free(p); return; }
        if (enabled()) {
            std::lock_guard<std::mutex> g(mu);
            size_t held = 0;
            for (auto& b : bufs) held += b.second;
            // bound the pinned hoard: big (bucket-mode) results free normally
            if (bufs.size() < 4 && held + cap <= (4ull << 30)) {
                bufs.emplace_back(p, cap);
                return;
            }
        }
        hipHostFree(p);
    }
};
PinnedPool g_result_pool;

struct HostTable {  // one device's sorted aggregate table, on host
    size_t n = 0;
    void* buf = nullptr;   // pinned when possible (single D2H copy)
    size_t cap = 0;
    bool pinned = false;
    uint64_t* series = nullptr;
    int64_t* bucket = nullptr;
    double* sum = nullptr;
    unsigned long long* cnt = nullptr;
    double* vmin = nullptr;
    double* vmax = nullptr;
    double* avg = nullptr;
    // first/last (a TS pass): extreme timestamps and the bit
    // patterns of the values there. When a value pass ran too, they live in
    // the TS pass's own buffer (buf2), whose keys were checked against buf's.
    int64_t* first_ts = nullptr;
    uint64_t* first = nullptr;
    int64_t* last_ts = nullptr;
    uint64_t* last = nullptr;
    void* buf2 = nullptr;
    size_t cap2 = 0;
    bool pinned2 = false;
    void release() {
        if (buf) {
            g_result_pool.release(buf, cap, pinned);
            buf = nullptr;
        }
        if (buf2) {
            g_result_pool.release(buf2, cap2, pinned2);
            buf2 = nullptr;
        }
        n = 0;
        cap = 0;
        cap2 = 0;
    }
};

uint32_t next_pow2_u32(uint64_t x) {
    uint32_t p = 1;
    while (p < x && p < (1u << 30)) p <<= 1;
    return p;
}

hx_status alloc_table(DevPlan& plan, uint32_t slots, uint32_t ops,
                      bool key_claim) {
    // slab strides: key-claim {key,sum,cnt[,min,max]} = 32/64;
    // state mode {state,pad,series,bucket,sum,cnt[,min,max]} = 48/64
    uint32_t stride = key_claim
                          ? ((ops & (HX_AGG_MIN | HX_AGG_MAX)) ? 64u : 32u)
                          : ((ops & (HX_AGG_MIN | HX_AGG_MAX)) ? 64u : 48u);
    if (plan.slots == slots && plan.t_slab && plan.slab_stride == stride)
        return HX_OK;
    if (plan.t_slab) { hipFree(plan.t_slab); plan.t_slab = nullptr; }
    plan.slots = slots;
    plan.slab_stride = stride;
    HIP_TRY(hipMalloc((void**)&plan.t_slab, size_t(slots) * stride));
    return HX_OK;
}

hx::AggTable agg_table(const DevPlan& plan) {
    return hx::AggTable{plan.slots - 1, plan.t_slab, plan.slab_stride};
}

// ops mask for the kernel: AVG implies SUM+COUNT accumulation
uint32_t kernel_ops(uint32_t ops) {
    uint32_t k = ops;
    if (ops & HX_AGG_AVG) k |= HX_AGG_SUM | HX_AGG_COUNT;
    return k;
}

static hx_status ensure_events(DevPlan& plan) {
    for (auto& ev : plan.ev)
        if (!ev) HIP_TRY(hipEventCreate(&ev));
    return HX_OK;
}

hx_status ensure_decoded(DevPlan& plan, hipStream_t s) {
    if (plan.decoded) return HX_OK;
    hx_status est = ensure_events(plan);
    if (est != HX_OK) return est;
    hipEvent_t d0 = plan.ev[2], d1 = plan.ev[3];
    HIP_TRY(hipMemsetAsync(plan.d_counters, 0, 32, s));
    HIP_TRY(hipEventRecord(d0, s));
    if (!plan.snappy_pages.empty())
        HIP_TRY(hx::launch_snappy(s, plan.d_blob, plan.d_dec, plan.d_snappy,
                                  (uint32_t)plan.snappy_pages.size(),
                                  plan.d_counters + 1));
    if (!plan.expand_pages.empty())
        // after the Snappy decode: its output is this kernel's source
        HIP_TRY(hx::launch_expand_optional(s, plan.d_blob, plan.d_dec,
                                           plan.d_expand,
                                           (uint32_t)plan.expand_pages.size(),
                                           plan.d_counters + 1));
    if (!plan.rledict_pages.empty())
        HIP_TRY(hx::launch_rledict(s, plan.d_blob, plan.d_dec, plan.d_rledict,
                                   (uint32_t)plan.rledict_pages.size(),
                                   plan.d_counters + 1));
    if (!plan.delta_pages.empty())
        HIP_TRY(hx::launch_decode_delta(s, plan.d_blob, plan.d_dec,
                                        plan.d_delta,
                                        (uint32_t)plan.delta_pages.size(),
                                        plan.d_counters + 1));
    if (!plan.snappy_ba_pages.empty())
        // Snappy pages of a Binary value column go to the blob's tail: the
        // blob is source and decode base at once, the ranges are disjoint
        // (streams below blob_bytes, output at and above it)
        HIP_TRY(hx::launch_snappy(s, plan.d_blob, plan.d_blob,
                                  plan.d_snappy_ba,
                                  (uint32_t)plan.snappy_ba_pages.size(),
                                  plan.d_counters + 1));
    if (!plan.ba_pages.empty())
        // byte-value stores: walk the PLAIN BYTE_ARRAY length prefixes of
        // the value pages into per-row handles (off << 20 | len) in dec
        HIP_TRY(hx::launch_ba_offsets(s, plan.d_blob, plan.d_ba,
                                      (uint32_t)plan.ba_pages.size(),
                                      (uint64_t*)plan.d_dec,
                                      plan.d_counters + 1));
    if (!plan.copies.empty())
        HIP_TRY(hx::launch_copy_u64(s, plan.d_blob, plan.d_dec, plan.d_copies,
                                    (uint32_t)plan.copies.size()));
    HIP_TRY(hipEventRecord(d1, s));
    HIP_TRY(hipStreamSynchronize(s));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, d0, d1));
    plan.decode_ms = ms;
    unsigned long long decode_err = 0;
    HIP_TRY(hipMemcpy(&decode_err, plan.d_counters + 1, 8,
                      hipMemcpyDeviceToHost));
    if (decode_err)
        return fail(HX_ERR_FORMAT, "page decode failed (malformed snappy "
                                   "stream, delta page or OPTIONAL page "
                                   "body; in a Binary value page a bad "
                                   "length prefix or a value of 2^20 bytes "
                                   "or more, a value handle has 20 length "
                                   "bits)");
    plan.decoded = true;
    return HX_OK;
}

hx_status ensure_sset(hx_prepared* P, DevPlan& plan) {
    if (P->sset_keys.empty() || plan.d_sset) return HX_OK;
    std::vector<uint64_t> keys(P->sset_keys);
    std::sort(keys.begin(), keys.end());
    keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
    uint64_t empty = ~0ull;
    while (std::binary_search(keys.begin(), keys.end(), empty)) empty--;
    uint32_t cap = next_pow2_u32(keys.size() * 2 + 16);
    std::vector<uint64_t> table(cap, empty);
    auto mix = [](uint64_t x) {
        x += 0x9E3779B97F4A7C15ull;
        x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
        x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
        return x ^ (x >> 31);
    };
    for (uint64_t kk : keys) {
        uint32_t i = (uint32_t)mix(kk) & (cap - 1);
        while (table[i] != empty) i = (i + 1) & (cap - 1);
        table[i] = kk;
    }
    HIP_TRY(hipMalloc((void**)&plan.d_sset, size_t(cap) * 8));
    HIP_TRY(hipMemcpy(plan.d_sset, table.data(), size_t(cap) * 8,
                      hipMemcpyHostToDevice));
    plan.sset_mask = cap - 1;
    plan.sset_empty = empty;
    return HX_OK;
}

// builds the filter/dedup AggParams shared by the aggregate and streaming
// kernels (table fields zeroed for streaming use)
static hx::AggParams base_params(hx_prepared* P, DevPlan& plan) {
    hx::AggParams A{};
    A.rgs = plan.d_rgs;
    A.n_rgs = (uint32_t)plan.rgs.size();
    A.ssts = plan.d_ssts;
    A.clusters = plan.d_clusters;
    A.cluster_members = plan.d_members;
    A.blob = plan.d_blob;
    A.dec = plan.d_dec;
    A.ts_lo = P->spec.range.start;
    A.ts_hi = P->spec.range.end;
    A.sset = plan.d_sset;
    A.sset_mask = plan.sset_mask;
    A.sset_empty = plan.sset_empty;
    A.use_sset = plan.d_sset ? 1 : 0;
    return A;
}

// Series-range partition build, once per prepared: stride-512
// device samples -> host sort -> distinct-count solve (u = x(1 - e^{-m/x})
// inverted by bisection) -> equal-sample quantile boundaries -> cached
// per-(block, sst) row bounds via k_range_bounds. Decode is deterministic,
// so the cached row bounds stay valid under HX_REDECODE.
// min_nb > 0 (a retry after an LDS block overflow) forces at least that many
// blocks and interpolates the boundaries between adjacent samples, so the
// split keeps refining where there are fewer samples than blocks.
static hx_status ensure_range(DevPlan& plan, const hx::AggParams& base,
                              uint32_t min_nb = 0) {
    plan.range_ready = false;
    const uint32_t n_rgs = (uint32_t)plan.rgs.size();
    const uint32_t n_ssts = (uint32_t)plan.ssts.size();
    if (!n_rgs || !n_ssts) return HX_OK;  // leaves range_ready false
    hipStream_t s = plan.stream;
    const size_t n_samp = (size_t)n_rgs * 16;
    uint64_t* d_samp = nullptr;
    HIP_TRY(hipMalloc((void**)&d_samp, n_samp * 8));
    hipError_t ke = hx::launch_sample_series(s, plan.d_rgs, n_rgs,
                                             plan.d_blob, plan.d_dec, d_samp);
    std::vector<uint64_t> samp(n_samp);
    if (ke == hipSuccess)
        ke = hipMemcpyAsync(samp.data(), d_samp, n_samp * 8,
                            hipMemcpyDeviceToHost, s);
    hipStreamSynchronize(s);
    hipFree(d_samp);
    if (ke != hipSuccess)
        return fail(HX_ERR_HIP, std::string("range sampling failed: ") +
                                    hipGetErrorString(ke));
    std::sort(samp.begin(), samp.end());
    while (!samp.empty() && samp.back() == ~0ull) samp.pop_back();
    const size_t m = samp.size();
    if (m == 0) return HX_OK;
    size_t u = 1;
    for (size_t i = 1; i < m; i++) u += samp[i] != samp[i - 1];
    double staged = 0;
    for (const auto& sd : plan.ssts) staged += (double)sd.n_staged;
    // solve u = x (1 - e^{-m/x}) for the distinct-series count x
    double x_lo = (double)u, x_hi = std::max<double>(staged, (double)u + 1);
    for (int it = 0; it < 60; it++) {
        double x = 0.5 * (x_lo + x_hi);
        double g = x * (1.0 - std::exp(-(double)m / x));
        (g < (double)u ? x_lo : x_hi) = x;
    }
    const double x_est = 0.5 * (x_lo + x_hi);
    plan.range_xest = x_est;
    double target = 650.0;   // series per block: ne=1024 at load ~0.3.
                             // History: measured when an LDS miss went to
                             // the global table — load 0.6 sent ~0.3% of
                             // heads there, 13.5 ms vs 7.5 ms at the 1B
                             // shape. Today a block that overflows ne costs
                             // a full rerun of the kernel with twice the
                             // blocks, so the margin still pays.
    if (const char* e = getenv("HX_RANGE_TARGET")) target = atof(e);
    uint32_t nb = 512;
    while (nb < (uint32_t)std::min(1e9, x_est * 1.3 / target) &&
           nb < (1u << 17))
        nb <<= 1;
    // safety floor against a residual under-estimate: cap rows per block
    // at 32768 (64-SST shapes: ~512 rows/sst/block). Empty or tiny blocks
    // are cheap; a block that overflows its LDS table reruns the whole
    // kernel with twice the blocks. History: the floor dates from r01, when
    // an overflow spilled to the global table instead (286M of 320M updates
    // went global at the 1B shape).
    if (!getenv("HX_RANGE_TARGET"))   // explicit target: trust the caller
        while ((double)nb * 32768.0 < staged && nb < (1u << 17)) nb <<= 1;
    while (nb < min_nb && nb < (1u << 17)) nb <<= 1;
    if (nb < min_nb) return HX_OK;   // cannot split further: not ready
    std::vector<uint64_t> bounds(nb + 1);
    bounds[0] = 0;
    for (uint32_t b = 1; b < nb; b++) {
        if (!min_nb) {
            bounds[b] = samp[(size_t)b * m / nb];
            continue;
        }
        const double pos = (double)b * (double)m / (double)nb;
        const size_t i = std::min((size_t)pos, m - 1);
        const uint64_t lo = samp[i], hi = samp[std::min(i + 1, m - 1)];
        const uint64_t v = lo + (uint64_t)((double)(hi - lo) * (pos - (double)i));
        bounds[b] = std::max(bounds[b - 1], std::min(v, hi));
    }
    bounds[nb] = ~0ull;
    if (plan.d_range_bounds) { hipFree(plan.d_range_bounds); plan.d_range_bounds = nullptr; }
    if (plan.d_bound_rows) { hipFree(plan.d_bound_rows); plan.d_bound_rows = nullptr; }
    HIP_TRY(hipMalloc((void**)&plan.d_range_bounds, (size_t)(nb + 1) * 8));
    HIP_TRY(hipMemcpyAsync(plan.d_range_bounds, bounds.data(),
                           (size_t)(nb + 1) * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMalloc((void**)&plan.d_bound_rows,
                      (size_t)(nb + 1) * n_ssts * 8));
    hx::RangeAux R{plan.d_range_bounds, plan.d_bound_rows, plan.d_sst_rgs,
                   plan.d_sst_rg_off,   plan.d_sst_rg_cnt, n_ssts,
                   nb,                  2048};
    ke = hx::launch_range_bounds(s, base, R, plan.d_bound_rows);
    if (ke != hipSuccess)
        return fail(HX_ERR_HIP, std::string("range bounds failed: ") +
                                    hipGetErrorString(ke));
    HIP_TRY(hipStreamSynchronize(s));
    plan.range_nblocks = nb;
    plan.range_ready = true;
    return HX_OK;
}

// Columns of a TS pass's contiguous SoA result (column c at d_dst + c * ng):
// where its time extrema sit and where the resolved values go. -1: side not
// asked.
struct TsCols {
    int32_t c_bucket = -1;
    int32_t c_min = -1, c_max = -1;       // tmin / tmax, as the pass left them
    int32_t c_first = -1, c_last = -1;    // value outputs behind the pass's own
};

// Host view of a TS pass's table: its min/max columns are the timestamps.
static void set_ts_columns(HostTable& out, uint64_t* hb, size_t ng,
                           const TsCols& c) {
    out.vmin = out.vmax = nullptr;
    out.first_ts = c.c_first >= 0 ? (int64_t*)(hb + size_t(c.c_min) * ng)
                                  : nullptr;
    out.first = c.c_first >= 0 ? hb + size_t(c.c_first) * ng : nullptr;
    out.last_ts = c.c_last >= 0 ? (int64_t*)(hb + size_t(c.c_max) * ng)
                                : nullptr;
    out.last = c.c_last >= 0 ? hb + size_t(c.c_last) * ng : nullptr;
}

// On-device finish of a TS pass (kernel 3d), before the single
// D2H: turn the pass's min/max columns into i64 timestamps in place, resolve
// the values at those extrema under the same filter and dedup, and map the
// value words to f64 bit patterns. Everything stays on plan.stream; the one
// host read is the error word.
static hx_status resolve_first_last(hx_prepared* P, DevPlan& plan,
                                    int64_t bucket_ms,
                                    unsigned long long* d_dst, size_t ng,
                                    const TsCols& c, double* kernel_ms) {
    hipStream_t s = plan.stream;
    auto col = [&](int32_t i) {
        return i >= 0 ? d_dst + size_t(i) * ng : nullptr;
    };
    if (c.c_min >= 0) HIP_TRY(hx::launch_map_words(s, col(c.c_min), ng, true));
    if (c.c_max >= 0) HIP_TRY(hx::launch_map_words(s, col(c.c_max), ng, true));
    if (c.c_first >= 0)
        HIP_TRY(hipMemsetAsync(col(c.c_first), 0, ng * 8, s));
    if (c.c_last >= 0) HIP_TRY(hipMemsetAsync(col(c.c_last), 0, ng * 8, s));
    unsigned long long* d_err = plan.d_counters + 5;
    HIP_TRY(hipMemsetAsync(d_err, 0, 8, s));
    hx::AggParams A = base_params(P, plan);
    A.bucket_ms = bucket_ms;
    hx::ResolveParams Q{};
    Q.gkey = (const uint64_t*)d_dst;
    Q.gbucket = (const long long*)col(c.c_bucket);
    Q.tmin = (const long long*)col(c.c_min);
    Q.tmax = (const long long*)col(c.c_max);
    Q.ofirst = col(c.c_first);
    Q.olast = col(c.c_last);
    Q.ng = (uint32_t)ng;
    Q.err = d_err;
    hipEvent_t e0 = plan.ev[0], e1 = plan.ev[1];
    HIP_TRY(hipEventRecord(e0, s));
    hipError_t ke = hx::launch_resolve_first_last(s, A, Q, plan.has_nulls);
    if (ke != hipSuccess)
        return fail(HX_ERR_HIP,
                    std::string("first/last resolve launch failed: ") +
                        hipGetErrorString(ke));
    HIP_TRY(hipEventRecord(e1, s));
    if (c.c_first >= 0)
        HIP_TRY(hx::launch_map_words(s, col(c.c_first), ng, false));
    if (c.c_last >= 0)
        HIP_TRY(hx::launch_map_words(s, col(c.c_last), ng, false));
    unsigned long long err = 0;
    HIP_TRY(hipMemcpyAsync(&err, d_err, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
    if (getenv("HX_DEBUG"))
        fprintf(stderr, "[hx] first/last resolve groups=%zu kernel_ms=%.2f "
                        "unmatched_rows=%llu\n", ng, ms, err);
    if (err)
        return fail(HX_ERR_HIP, "first/last resolve: " + std::to_string(err) +
                                    " surviving rows matched no group of "
                                    "the time pass");
    *kernel_ms += ms;
    return HX_OK;
}

// Series-only grouping on the range path: the range kernel emits
// each block's groups as one key-ordered run, two small kernels place the
// runs in block order into the contiguous SoA result, and the host syncs
// once to read the counters before the single D2H. No global table, no
// compaction, no sort. Both overflows are retried exactly: a full staging
// area with the capacity the cursor reported, a block that met more than ne
// keys with twice the blocks. *done stays false when the attempts run out;
// the caller then takes the global-table route.
static hx_status exec_range_sorted(hx_prepared* P, DevPlan& plan,
                                   const hx_agg_spec* agg, uint32_t ops,
                                   HostTable& out, double* agg_kernel_ms,
                                   unsigned long long* matched_out,
                                   bool* done, uint32_t fl = 0) {
    // fl != 0: the TS pass of a first/last request — ops is MIN and/or MAX
    // over the rows' timestamps, and the values at those extrema are
    // resolved on the device before the D2H
    hipStream_t s = plan.stream;
    const bool mm = (ops & (HX_AGG_MIN | HX_AGG_MAX)) != 0;
    const bool has_sum = (ops & (HX_AGG_SUM | HX_AGG_AVG)) != 0;
    const bool has_cnt = (ops & (HX_AGG_COUNT | HX_AGG_AVG)) != 0;
    const bool has_min = (ops & HX_AGG_MIN) != 0;
    const bool has_max = (ops & HX_AGG_MAX) != 0;
    const bool has_avg = (agg->ops & HX_AGG_AVG) != 0;
    int32_t na = 1;
    const int32_t c_sum = has_sum ? na++ : -1;
    const int32_t c_cnt = has_cnt ? na++ : -1;
    const int32_t c_min = has_min ? na++ : -1;
    const int32_t c_max = has_max ? na++ : -1;
    const int32_t c_avg = has_avg ? na++ : -1;
    const uint32_t n_stage = mm ? 5 : 3;
    TsCols tc;
    tc.c_min = c_min;
    tc.c_max = c_max;
    if (fl & HX_AGG_FIRST) tc.c_first = na++;
    if (fl & HX_AGG_LAST) tc.c_last = na++;
    const uint32_t n_cols = (uint32_t)na;   // the pass's own + resolved

    uint64_t staged = 0;
    for (const auto& sd : plan.ssts) staged += (uint64_t)sd.n_staged;
    uint64_t cap = plan.sorted_cap;
    if (!cap) {
        // the estimate that sizes the global table; never more than one
        // group per staged row
        if (const char* env = getenv("HX_TABLE_SLOTS"))
            cap = next_pow2_u32(strtoull(env, nullptr, 10));
        else
            cap = std::max<uint64_t>(
                std::max<uint64_t>(1 << 16, (uint64_t)plan.rows_scanned / 32),
                (uint64_t)(plan.range_xest * 1.4));
        cap = std::min(cap, std::max<uint64_t>(staged, 1));
    }
    unsigned long long counters[6];
    for (int attempt = 0; attempt < 4; attempt++) {
        if (cap > 0xFFFFFFFFull)
            return fail(HX_ERR_UNSUPPORTED, "result exceeds 2^32 groups");
        const uint32_t nb = plan.range_nblocks;
        uint32_t ne = 1024;
        if (const char* e = getenv("HX_RANGE_NE"))
            ne = (uint32_t)strtoul(e, nullptr, 10);
        const size_t need = size_t(cap) * 8 * (n_stage + n_cols) +
                            size_t(nb) * 12 + 256;
        hx_status st = ensure_dev(&plan.d_scratch, &plan.scratch_cap, need);
        if (st != HX_OK) return st;
        uint8_t* base = (uint8_t*)plan.d_scratch;
        auto carve8 = [&](size_t count) {
            uint8_t* p = base;
            base += count * 8;
            return p;
        };
        hx::RangeOut O{};
        O.key = (uint64_t*)carve8(cap);
        O.sum = (double*)carve8(cap);
        O.cnt = (unsigned long long*)carve8(cap);
        O.vmin = mm ? (double*)carve8(cap) : nullptr;
        O.vmax = mm ? (double*)carve8(cap) : nullptr;
        unsigned long long* d_dst =
            (unsigned long long*)carve8(size_t(cap) * n_cols);
        O.desc = (uint64_t*)carve8(nb);
        uint32_t* d_prefix = (uint32_t*)base;
        O.cap = cap;
        O.cursor = plan.d_counters + 0;
        O.stage_ovf = plan.d_counters + 1;
        O.block_ovf = plan.d_counters + 4;
        HIP_TRY(hipMemsetAsync(plan.d_counters, 0, 48, s));

        hx::AggParams A = base_params(P, plan);
        A.ops = ops;
        A.key_claim = 1;
        A.fill = plan.d_counters + 0;
        A.overflow = plan.d_counters + 1;
        A.matched = plan.d_counters + 2;
        hx::RangeAux R{plan.d_range_bounds, plan.d_bound_rows,
                       plan.d_sst_rgs,     plan.d_sst_rg_off,
                       plan.d_sst_rg_cnt,  (uint32_t)plan.ssts.size(),
                       nb,                 ne};
        hx::RangePlace Q{};
        Q.desc = O.desc;
        Q.prefix = d_prefix;
        Q.n_blocks = nb;
        Q.key = O.key;
        Q.sum = O.sum;
        Q.cnt = O.cnt;
        Q.vmin = O.vmin;
        Q.vmax = O.vmax;
        Q.dst = d_dst;
        Q.c_sum = c_sum;
        Q.c_cnt = c_cnt;
        Q.c_min = c_min;
        Q.c_max = c_max;
        Q.c_avg = c_avg;
        Q.cap = cap;
        Q.cursor = O.cursor;
        Q.stage_ovf = O.stage_ovf;
        Q.block_ovf = O.block_ovf;

        hx_status est = ensure_events(plan);
        if (est != HX_OK) return est;
        hipEvent_t e0 = plan.ev[0], e1 = plan.ev[1];
        HIP_TRY(hipEventRecord(e0, s));
        hipError_t ke = hx::launch_scan_agg_range2(s, A, R, mm,
                                                   plan.has_nulls, O,
                                                   fl != 0);
        if (ke != hipSuccess)
            return fail(HX_ERR_HIP,
                        std::string("range kernel launch failed: ") +
                            hipGetErrorString(ke));
        HIP_TRY(hipEventRecord(e1, s));
        ke = hx::launch_place_runs(s, Q);
        if (ke != hipSuccess)
            return fail(HX_ERR_HIP,
                        std::string("run placement launch failed: ") +
                            hipGetErrorString(ke));
        HIP_TRY(hipStreamSynchronize(s));
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
        HIP_TRY(hipMemcpy(counters, plan.d_counters, 48,
                          hipMemcpyDeviceToHost));
        if (getenv("HX_DEBUG"))
            fprintf(stderr,
                    "[hx] exec attempt=%d kernel=range-sorted cap=%llu nb=%u "
                    "ne=%u xest=%.0f kernel_ms=%.2f groups=%llu "
                    "stage_overflow=%llu block_overflow=%llu matched=%llu\n",
                    attempt, (unsigned long long)cap, nb, ne, plan.range_xest,
                    ms, counters[0], counters[1], counters[4], counters[2]);
        if (counters[4]) {   // > ne keys in one block: halve the ranges
            if (attempt == 3) break;
            hx::AggParams rb{};
            rb.rgs = plan.d_rgs;
            rb.blob = plan.d_blob;
            rb.dec = plan.d_dec;
            hx_status rs = ensure_range(plan, rb, nb * 2);
            if (rs != HX_OK) return rs;
            if (!plan.range_ready) break;
            continue;
        }
        const unsigned long long total = counters[0];
        if (counters[1] || total > cap) {   // staging full: total is exact
            if (attempt == 3) break;
            cap = total;
            continue;
        }
        plan.sorted_cap = cap;
        *agg_kernel_ms = ms;
        *matched_out = counters[2];
        *done = true;
        out.release();
        out.n = total;
        if (total == 0) return HX_OK;
        const size_t ng = (size_t)total;
        if (fl) {
            hx_status fs = resolve_first_last(P, plan, 0, d_dst, ng, tc,
                                              agg_kernel_ms);
            if (fs != HX_OK) return fs;
        }
        const size_t bytes = ng * 8 * n_cols;
        out.buf = g_result_pool.acquire(bytes, &out.pinned, &out.cap);
        if (!out.buf) return fail(HX_ERR_IO, "result alloc failed");
        HIP_TRY(hipMemcpyAsync(out.buf, d_dst, bytes, hipMemcpyDeviceToHost,
                               s));
        HIP_TRY(hipStreamSynchronize(s));
        uint64_t* hb = (uint64_t*)out.buf;
        out.series = hb;
        out.bucket = nullptr;
        out.sum = has_sum ? (double*)(hb + size_t(c_sum) * ng) : nullptr;
        out.cnt = has_cnt ? (unsigned long long*)(hb + size_t(c_cnt) * ng)
                          : nullptr;
        out.vmin = has_min ? (double*)(hb + size_t(c_min) * ng) : nullptr;
        out.vmax = has_max ? (double*)(hb + size_t(c_max) * ng) : nullptr;
        out.avg = has_avg ? (double*)(hb + size_t(c_avg) * ng) : nullptr;
        if (fl) set_ts_columns(out, hb, ng, tc);
        return HX_OK;
    }
    plan.sorted_gave_up = true;
    return HX_OK;
}

// Direct-indexed bucket decision (bucket queries, key-claim safe): when the
// bucket range — known exactly from the scan range clamped to the catalog —
// fits a dense per-slot accumulator row, the table is keyed by series only
// and the bucket becomes an array index: no (series,bucket) hashing at all.
// n_buckets == 0 means "take the generic state-word path".
struct BucketPlan {
    int64_t lo_bucket = 0;
    uint32_t n_buckets = 0;
    uint32_t bstride = 0;   // 16 {sum,cnt} or 32 {+min,max}
};

static BucketPlan direct_buckets(hx_prepared* P, const DevPlan& plan,
                                 const hx_agg_spec* agg) {
    BucketPlan bp;
    if (agg->bucket_ms <= 0 || !P->key_claim_safe || getenv("HX_FORCE_STATE"))
        return bp;
    int64_t lo_ts = P->spec.range.start, hi_ts = P->spec.range.end;
    int64_t cat_lo = INT64_MAX, cat_hi = INT64_MIN;
    for (const auto& c : P->h->ssts) {
        cat_lo = std::min(cat_lo, c.ts_min);
        cat_hi = std::max(cat_hi, c.ts_max);
    }
    if (cat_lo <= cat_hi) {
        lo_ts = std::max(lo_ts, cat_lo);
        hi_ts = std::min(hi_ts, cat_hi + 1);
    }
    if (lo_ts >= hi_ts) return bp;
    auto fdiv = [&](int64_t t) {
        int64_t q = t / agg->bucket_ms;
        if ((t % agg->bucket_ms) != 0 && t < 0) q--;
        return q;
    };
    bp.lo_bucket = fdiv(lo_ts);
    const int64_t nb = fdiv(hi_ts - 1) - bp.lo_bucket + 1;
    const uint32_t bstride =
        (agg->ops & (HX_AGG_MIN | HX_AGG_MAX)) ? 32u : 16u;
    // memory cap: take the generic path beyond ~24 GB
    const uint64_t est_slots = std::max<uint64_t>(
        1 << 16, next_pow2_u32((uint64_t)plan.rows_scanned / 32));
    if (nb > 0 && (uint64_t)nb * est_slots * bstride <= (24ull << 30)) {
        bp.n_buckets = (uint32_t)nb;
        bp.bstride = bstride;
    }
    return bp;
}

// The global-table route: every grouping the range path does not take
// (buckets, the state-word path, HX_RANGE=0, a range plan that gave up).
// The wave kernel (k_scan_agg) aggregates into the hash table, retried with
// a larger table on overflow; then compaction, sort, gather and one D2H.
static hx_status exec_table(hx_prepared* P, DevPlan& plan,
                            const hx_agg_spec* agg, uint32_t ops,
                            BucketPlan bp, int32_t key_claim, HostTable& out,
                            double* agg_kernel_ms,
                            unsigned long long* matched_out,
                            uint32_t fl = 0) {
    // fl != 0: the TS pass of a first/last request, as in exec_range_sorted
    hipStream_t s = plan.stream;
    const bool bucket = agg->bucket_ms > 0;
    const bool mm = (ops & (HX_AGG_MIN | HX_AGG_MAX)) != 0;

    // table size heuristic; grows on overflow
    uint32_t slots = plan.slots;
    if (!slots) {
        const char* env = getenv("HX_TABLE_SLOTS");
        if (env) slots = next_pow2_u32(strtoull(env, nullptr, 10));
        else slots = next_pow2_u32(std::max<uint64_t>(
                 1 << 16,
                 // generic (series,bucket) hashing needs generous sizing;
                 // the direct-indexed path is keyed by series only
                 (uint64_t)plan.rows_scanned /
                     ((bucket && !bp.n_buckets) ? 2 : 32)));
        // the range partition's distinct-series estimate, when one was built
        if (plan.range_xest > 0 && key_claim && !bucket) {
            uint32_t rs = next_pow2_u32((uint64_t)(plan.range_xest * 1.4));
            if (rs > slots) slots = rs;
        }
        if (slots > (1u << 28)) slots = 1u << 28;
    }

    unsigned long long counters[6];
    for (int attempt = 0; attempt < 4; attempt++) {
        hx_status st = alloc_table(plan, slots, ops, key_claim);
        if (st != HX_OK) return st;
        if (bp.n_buckets) {
            uint64_t need_b = (uint64_t)slots * bp.n_buckets * bp.bstride;
            if (need_b > plan.bstore_cap) {
                if (plan.t_bstore) hipFree(plan.t_bstore);
                plan.t_bstore = nullptr;
                plan.bstore_cap = 0;
                HIP_TRY(hipMalloc((void**)&plan.t_bstore, need_b));
                plan.bstore_cap = need_b;
            }
        }
        // reset table + counters (part of the step)
        if (key_claim) {
            HIP_TRY(hx::launch_init_slab(s, plan.t_slab, slots,
                                         plan.slab_stride));
            if (bp.n_buckets)
                HIP_TRY(hx::launch_init_accum_rows(
                    s, plan.t_bstore, (size_t)slots * bp.n_buckets,
                    bp.bstride, mm));
        } else {
            HIP_TRY(hx::launch_init_state_slab(s, plan.t_slab, slots,
                                               plan.slab_stride, mm));
        }
        HIP_TRY(hipMemsetAsync(plan.d_counters, 0, 48, s));

        hx::AggParams A = base_params(P, plan);
        A.bucket_ms = bucket ? agg->bucket_ms : 0;
        A.ops = bp.n_buckets ? (ops | HX_AGG_COUNT) : ops;  // cnt = liveness
        A.key_claim = key_claim;
        A.lo_bucket = bp.lo_bucket;
        A.n_buckets = bp.n_buckets;
        A.bstride = bp.bstride;
        A.bstore = plan.t_bstore;
        A.table = agg_table(plan);
        A.fill_limit = (unsigned long long)(double(slots) * 0.85);
        A.fill = plan.d_counters + 0;
        A.overflow = plan.d_counters + 1;
        A.matched = plan.d_counters + 2;

        hx_status est = ensure_events(plan);
        if (est != HX_OK) return est;
        hipEvent_t e0 = plan.ev[0], e1 = plan.ev[1];
        HIP_TRY(hipEventRecord(e0, s));
        HIP_TRY(hx::launch_scan_agg(s, A, 0, plan.has_nulls, fl != 0));
        HIP_TRY(hipEventRecord(e1, s));
        HIP_TRY(hipStreamSynchronize(s));
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
        HIP_TRY(hipMemcpy(counters, plan.d_counters, 48, hipMemcpyDeviceToHost));
        if (getenv("HX_DEBUG"))
            fprintf(stderr,
                    "[hx] exec attempt=%d kernel=wave slots=%u xest=%.0f "
                    "kernel_ms=%.2f fill=%llu overflow=%llu matched=%llu\n",
                    attempt, slots, plan.range_xest, ms, counters[0],
                    counters[1], counters[2]);
        if (counters[1] == 0) {  // no overflow
            *agg_kernel_ms = ms;
            break;
        }
        if (attempt == 3)
            return fail(HX_ERR_HIP, "aggregate table overflow persisted");
        if (bp.n_buckets) {
            // direct-indexed bucket overflow (e.g. footer ts stats under-
            // reported the range): fall back to the generic hashed path
            bp.n_buckets = 0;
            bp.bstride = 0;
            key_claim = 0;
        } else {
            slots = slots >= (1u << 28) ? slots : slots * 4;
        }
        plan.slots = 0;  // force realloc
    }
    *matched_out = counters[2];
    unsigned long long fill = counters[0];

    // ---- compact + sort + gather + single D2H ---------------------------
    out.release();
    out.n = fill;
    if (fill == 0) return HX_OK;
    // capacity: series-only => one group per claimed slot (= fill);
    // direct-indexed buckets => up to fill x n_buckets groups, but never
    // more than the surviving-row count
    uint64_t cap64 = fill;
    if (bp.n_buckets)
        cap64 = std::min<uint64_t>(fill * (uint64_t)bp.n_buckets, counters[2]);
    if (cap64 > 0xFFFFFFFFull)
        return fail(HX_ERR_UNSUPPORTED, "result exceeds 2^32 groups");
    const uint32_t n = (uint32_t)cap64;
    const bool has_sum = (ops & (HX_AGG_SUM | HX_AGG_AVG)) != 0;
    const bool has_cnt = (ops & (HX_AGG_COUNT | HX_AGG_AVG)) != 0;
    const bool has_min = (ops & HX_AGG_MIN) != 0;
    const bool has_max = (ops & HX_AGG_MAX) != 0;
    const bool has_avg = (agg->ops & HX_AGG_AVG) != 0;
    const uint32_t n_core = 1 + (bucket ? 1 : 0) + has_sum + has_cnt +
                            has_min + has_max;
    const uint32_t n_total = n_core + (has_avg ? 1 : 0);
    // resolved first/last value columns behind the pass's own (TS pass only)
    const uint32_t n_cols = n_total + ((fl & HX_AGG_FIRST) ? 1 : 0) +
                            ((fl & HX_AGG_LAST) ? 1 : 0);
    // scratch: compact arrays (n_core) + sort keys in/out (2) + dst (n_cols)
    // + 3 perm arrays + counter
    size_t need = size_t(n) * 8 * (n_core + 2 + n_cols) +
                  size_t(n) * 4 * 3 + 256 + 2 * 2048 * 4;
    hx_status st = ensure_dev(&plan.d_scratch, &plan.scratch_cap, need);
    if (st != HX_OK) return st;
    uint8_t* base = (uint8_t*)plan.d_scratch;
    auto carve8 = [&](size_t count) {
        uint8_t* p = base;
        base += (count * 8 + 7) & ~size_t(7);
        return p;
    };
    uint64_t* c_series = (uint64_t*)carve8(n);
    long long* c_bucket = bucket ? (long long*)carve8(n) : nullptr;
    double* c_sum = has_sum ? (double*)carve8(n) : nullptr;
    unsigned long long* c_cnt = has_cnt ? (unsigned long long*)carve8(n) : nullptr;
    double* c_min = has_min ? (double*)carve8(n) : nullptr;
    double* c_max = has_max ? (double*)carve8(n) : nullptr;
    uint64_t* keys_tmp = (uint64_t*)carve8(n);
    uint64_t* keys_out = (uint64_t*)carve8(n);
    unsigned long long* d_dst = (unsigned long long*)carve8(size_t(n) * n_cols);
    unsigned long long* d_nout = (unsigned long long*)carve8(1);
    uint32_t* compact_scratch = (uint32_t*)carve8(2048);  // 2x2048 u32
    uint32_t* perm_a = (uint32_t*)base; base += size_t(n) * 4;
    uint32_t* perm_b = (uint32_t*)base; base += size_t(n) * 4;
    uint32_t* perm_c = (uint32_t*)base; base += size_t(n) * 4;

    HIP_TRY(hipMemsetAsync(d_nout, 0, 8, s));
    hx::CompactOut co{c_series, c_bucket, c_sum, c_cnt, c_min, c_max, d_nout};
    HIP_TRY(hx::launch_compact(s, agg_table(plan), plan.slots, key_claim,
                               bucket ? agg->bucket_ms : 0, bp.lo_bucket,
                               bp.n_buckets, bp.bstride, plan.t_bstore, co,
                               compact_scratch));
    unsigned long long n_groups64 = 0;
    HIP_TRY(hipStreamSynchronize(s));
    HIP_TRY(hipMemcpy(&n_groups64, d_nout, 8, hipMemcpyDeviceToHost));
    if (n_groups64 > n)
        return fail(HX_ERR_HIP, "compact overran its capacity bound");
    const uint32_t ng = (uint32_t)n_groups64;
    out.n = ng;
    if (ng == 0) return HX_OK;

    // sort: LSD-stable — by bucket first (if any), then by series
    HIP_TRY(hx::launch_iota(s, perm_a, ng));
    const uint32_t* perm_in = perm_a;
    uint32_t* perm_out = perm_b;
    if (bucket) {
        HIP_TRY(hx::launch_gather_u64(s, (const unsigned long long*)c_bucket,
                                      perm_a, (unsigned long long*)keys_tmp, ng));
        HIP_TRY(hx::launch_xor_sign(s, (unsigned long long*)keys_tmp, ng));
        HIP_TRY(hx::sort_pairs_u64(s, keys_tmp, keys_out, perm_a, perm_out, ng,
                                   &plan.d_sort_temp, &plan.sort_temp_cap));
        perm_in = perm_out;
        perm_out = perm_c;
    }
    HIP_TRY(hx::launch_gather_u64(s, (const unsigned long long*)c_series, perm_in,
                                  (unsigned long long*)keys_tmp, ng));
    HIP_TRY(hx::sort_pairs_u64(s, keys_tmp, keys_out, perm_in, perm_out, ng,
                               &plan.d_sort_temp, &plan.sort_temp_cap));
    const uint32_t* perm = perm_out;

    // one multi-array gather into the contiguous dst, then ONE D2H copy
    const unsigned long long* srcs[8];
    uint32_t na = 0;
    srcs[na++] = (const unsigned long long*)c_series;
    size_t off_bucket = bucket ? na : 0;
    if (bucket) srcs[na++] = (const unsigned long long*)c_bucket;
    size_t off_sum = has_sum ? na : 0;
    if (has_sum) srcs[na++] = (const unsigned long long*)c_sum;
    size_t off_cnt = has_cnt ? na : 0;
    if (has_cnt) srcs[na++] = (const unsigned long long*)c_cnt;
    size_t off_min = has_min ? na : 0;
    if (has_min) srcs[na++] = (const unsigned long long*)c_min;
    size_t off_max = has_max ? na : 0;
    if (has_max) srcs[na++] = (const unsigned long long*)c_max;
    HIP_TRY(hx::launch_gather_multi(s, srcs, na, perm, d_dst, ng));
    if (has_avg)
        HIP_TRY(hx::launch_avg(s,
                               (const double*)(d_dst + size_t(off_sum) * ng),
                               d_dst + size_t(off_cnt) * ng,
                               (double*)(d_dst + size_t(n_core) * ng), ng));

    TsCols tc;
    if (fl) {
        uint32_t nc = n_total;
        tc.c_bucket = bucket ? (int32_t)off_bucket : -1;
        tc.c_min = has_min ? (int32_t)off_min : -1;
        tc.c_max = has_max ? (int32_t)off_max : -1;
        if (fl & HX_AGG_FIRST) tc.c_first = (int32_t)nc++;
        if (fl & HX_AGG_LAST) tc.c_last = (int32_t)nc++;
        hx_status fs = resolve_first_last(P, plan, bucket ? agg->bucket_ms : 0,
                                          d_dst, ng, tc, agg_kernel_ms);
        if (fs != HX_OK) return fs;
    }

    const size_t bytes = size_t(ng) * 8 * n_cols;
    out.buf = g_result_pool.acquire(bytes, &out.pinned, &out.cap);
    if (!out.buf) return fail(HX_ERR_IO, "result alloc failed");
    HIP_TRY(hipMemcpyAsync(out.buf, d_dst, bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    uint64_t* hb = (uint64_t*)out.buf;
    out.series = hb;
    out.bucket = bucket ? (int64_t*)(hb + off_bucket * ng) : nullptr;
    out.sum = has_sum ? (double*)(hb + off_sum * ng) : nullptr;
    out.cnt = has_cnt ? (unsigned long long*)(hb + off_cnt * ng) : nullptr;
    out.vmin = has_min ? (double*)(hb + off_min * ng) : nullptr;
    out.vmax = has_max ? (double*)(hb + off_max * ng) : nullptr;
    out.avg = has_avg ? (double*)(hb + size_t(n_core) * ng) : nullptr;
    if (fl) set_ts_columns(out, hb, ng, tc);
    return HX_OK;
}

// One aggregate pass over a decoded plan into `out` (sorted by series[,
// bucket]). Two routes: series-only grouping with a key-claim-safe sentinel
// takes the range path (exec_range_sorted); everything else, and a range plan
// that gave up, takes the global table (exec_table). fl != 0: the TS pass of
// a first/last request (agg->ops is then MIN and/or MAX, run over the rows'
// timestamps); route selection, partition and table sizing are those of any
// other pass.
static hx_status exec_pass(hx_prepared* P, DevPlan& plan,
                           const hx_agg_spec* agg, uint32_t fl, HostTable& out,
                           double* agg_kernel_ms,
                           unsigned long long* matched_out) {
    const uint32_t ops = kernel_ops(agg->ops);
    const bool bucket = agg->bucket_ms > 0;

    // one-CAS key claim: series-only grouping, or direct-indexed buckets,
    // with a stats-proven sentinel (HX_FORCE_STATE=1 forces the generic
    // state-word path for A/B runs)
    const BucketPlan bp = direct_buckets(P, plan, agg);
    const int32_t key_claim =
        ((!bucket || bp.n_buckets) && P->key_claim_safe &&
         !getenv("HX_FORCE_STATE")) ? 1 : 0;

    // series-range partition: built once per prepared. A plan
    // whose sorted path gave up (a block range that will not fit LDS; the
    // wave kernel has no such limit) stays on the table route and does not
    // rebuild the partition.
    bool use_range =
        !bucket && key_claim && !bp.n_buckets && !plan.sorted_gave_up;
    if (const char* renv = getenv("HX_RANGE"))
        use_range = use_range && atoi(renv) != 0;
    if (use_range && !plan.range_ready) {
        hx::AggParams base{};
        base.rgs = plan.d_rgs;
        base.blob = plan.d_blob;
        base.dec = plan.d_dec;
        hx_status rs = ensure_range(plan, base);
        if (rs != HX_OK) return rs;
    }
    if (use_range && plan.range_ready) {
        bool done = false;
        hx_status rs = exec_range_sorted(P, plan, agg, ops, out,
                                         agg_kernel_ms, matched_out, &done,
                                         fl);
        if (rs != HX_OK || done) return rs;
    }
    return exec_table(P, plan, agg, ops, bp, key_claim, out, agg_kernel_ms,
                      matched_out, fl);
}

// Aggregate one device's plan into `out`. The request splits into the value
// ops (sum, count, min, max, avg: one pass, as before first/last existed) and
// first/last (a TS pass plus the on-device resolve). Both passes
// skip the same rows, so they must agree on the group set and on the matched
// row count; that is checked, never assumed.
hx_status exec_plan(hx_prepared* P, DevPlan& plan, const hx_agg_spec* agg,
                    HostTable& out, double* agg_kernel_ms,
                    unsigned long long* matched_out) {
    if (P->h->bytes_value)
        return fail(HX_ERR_UNSUPPORTED,
                    "aggregates over Binary value columns are undefined "
                    "(scan the rows with hx_scan instead)");
    HIP_TRY(hipSetDevice(plan.device));

    hx_status sst_ = ensure_sset(P, plan);
    if (sst_ != HX_OK) return sst_;

    // decode results persist across exec calls on one prepared scan; for
    // benchmarking encoded/compressed workloads HX_REDECODE=1 forces every
    // step to repeat the decompress/decode stage (no cached decode output
    // inside the timed region). Once per exec, not once per pass.
    if (getenv("HX_REDECODE")) plan.decoded = false;
    hx_status dst_ = ensure_decoded(plan, plan.stream);
    if (dst_ != HX_OK) return dst_;

    const uint32_t fl = agg->ops & (HX_AGG_FIRST | HX_AGG_LAST);
    const uint32_t vops = agg->ops & ~fl;
    if (!fl)
        return exec_pass(P, plan, agg, 0, out, agg_kernel_ms, matched_out);
    const hx_agg_spec tspec{((fl & HX_AGG_FIRST) ? (uint32_t)HX_AGG_MIN : 0u) |
                                ((fl & HX_AGG_LAST) ? (uint32_t)HX_AGG_MAX : 0u),
                            agg->bucket_ms};
    if (!vops)
        return exec_pass(P, plan, &tspec, fl, out, agg_kernel_ms, matched_out);

    const hx_agg_spec vspec{vops, agg->bucket_ms};
    hx_status st = exec_pass(P, plan, &vspec, 0, out, agg_kernel_ms,
                             matched_out);
    if (st != HX_OK) return st;
    HostTable ts;
    double ts_ms = 0;
    unsigned long long ts_matched = 0;
    st = exec_pass(P, plan, &tspec, fl, ts, &ts_ms, &ts_matched);
    if (st == HX_OK && ts_matched != *matched_out)
        st = fail(HX_ERR_HIP, "first/last: the time pass matched " +
                                  std::to_string(ts_matched) +
                                  " rows, the value pass " +
                                  std::to_string(*matched_out));
    if (st == HX_OK &&
        (ts.n != out.n ||
         (ts.n && memcmp(ts.series, out.series, ts.n * 8) != 0) ||
         (ts.n && agg->bucket_ms > 0 &&
          memcmp(ts.bucket, out.bucket, ts.n * 8) != 0)))
        st = fail(HX_ERR_HIP, "first/last: the time pass and the value pass "
                              "disagree on the group set");
    if (st != HX_OK) {
        ts.release();
        return st;
    }
    *agg_kernel_ms += ts_ms;
    out.first_ts = ts.first_ts;
    out.first = ts.first;
    out.last_ts = ts.last_ts;
    out.last = ts.last;
    out.buf2 = ts.buf;   // ownership moves with the columns
    out.cap2 = ts.cap;
    out.pinned2 = ts.pinned;
    return HX_OK;
}

}  // namespace

// ---------------------------------------------------------------------------
// result assembly + public entry points
// ---------------------------------------------------------------------------
namespace {

struct ResultStorage {  // backs hx_result_table arrays
    std::vector<uint64_t> series;
    std::vector<int64_t> bucket;
    std::vector<double> sum;
    std::vector<unsigned long long> cnt;
    std::vector<double> vmin, vmax, avg;
    std::vector<int64_t> first_ts, last_ts;
    std::vector<uint64_t> first, last;   // f64 bit patterns
};

// n-way merge of per-device sorted partials, combining equal (series,bucket)
// groups: the host partial-aggregate merge of SURVEY §8(e) (partials are
// O(groups), not O(rows)).
void merge_partials(std::vector<HostTable>& parts, uint32_t ops,
                    bool bucket, ResultStorage& out) {
    const uint32_t kops = kernel_ops(ops);
    std::vector<size_t> idx(parts.size(), 0);
    for (;;) {
        // find smallest key among cursors
        bool any = false;
        uint64_t ks = 0;
        int64_t kb = 0;
        for (size_t p = 0; p < parts.size(); p++) {
            if (idx[p] >= parts[p].n) continue;
            uint64_t s = parts[p].series[idx[p]];
            int64_t b = bucket ? parts[p].bucket[idx[p]] : 0;
            if (!any || s < ks || (s == ks && b < kb)) { ks = s; kb = b; any = true; }
        }
        if (!any) break;
        double sum = 0, vmin = 0, vmax = 0;
        unsigned long long cnt = 0;
        hx::FlPick pf{0, 0}, pl{0, 0};   // first_last.h states the rules
        bool first = true;
        for (size_t p = 0; p < parts.size(); p++) {
            size_t i = idx[p];
            if (i >= parts[p].n || parts[p].series[i] != ks ||
                (bucket && parts[p].bucket[i] != kb))
                continue;
            if (kops & HX_AGG_SUM) sum += parts[p].sum[i];
            if (kops & HX_AGG_COUNT) cnt += parts[p].cnt[i];
            if (kops & HX_AGG_MIN)
                vmin = first ? parts[p].vmin[i] : std::min(vmin, parts[p].vmin[i]);
            if (kops & HX_AGG_MAX)
                vmax = first ? parts[p].vmax[i] : std::max(vmax, parts[p].vmax[i]);
            if (ops & HX_AGG_FIRST) {
                const hx::FlPick x{parts[p].first_ts[i], parts[p].first[i]};
                pf = first ? x : hx::fl_merge_first(pf, x);
            }
            if (ops & HX_AGG_LAST) {
                const hx::FlPick x{parts[p].last_ts[i], parts[p].last[i]};
                pl = first ? x : hx::fl_merge_last(pl, x);
            }
            first = false;
            idx[p]++;
        }
        out.series.push_back(ks);
        if (bucket) out.bucket.push_back(kb);
        if (ops & HX_AGG_SUM) out.sum.push_back(sum);
        if (ops & HX_AGG_COUNT) out.cnt.push_back(cnt);
        if (ops & HX_AGG_MIN) out.vmin.push_back(vmin);
        if (ops & HX_AGG_MAX) out.vmax.push_back(vmax);
        if (ops & HX_AGG_AVG) out.avg.push_back(sum / double(cnt));
        if (ops & HX_AGG_FIRST) {
            out.first_ts.push_back(pf.ts);
            out.first.push_back(pf.bits);
        }
        if (ops & HX_AGG_LAST) {
            out.last_ts.push_back(pl.ts);
            out.last.push_back(pl.bits);
        }
    }
}

}  // namespace

struct hx_result_impl {
    hx_result_table pub_{};
    HostTable owned;       // single-device fast path: pub_ points into owned
    ResultStorage store;   // multi-device merge path
    ~hx_result_impl() { owned.release(); }
};

extern "C" hx_status hx_exec_agg(hx_prepared* P, const hx_agg_spec* agg,
                                 hx_result_table** out) {
    if (!P || !agg || !out) return fail(HX_ERR_INVALID, "null argument");
    if (agg->ops == 0) return fail(HX_ERR_INVALID, "no aggregate ops requested");
    if (agg->bucket_ms < 0) return fail(HX_ERR_INVALID, "negative bucket_ms");
    auto t0 = std::chrono::steady_clock::now();
    const bool bucket = agg->bucket_ms > 0;

    std::vector<HostTable> parts(P->plans.size());
    double agg_ms_max = 0, decode_ms_max = 0;
    unsigned long long matched = 0;
    for (size_t d = 0; d < P->plans.size(); d++) {
        double agg_ms = 0;
        unsigned long long m = 0;
        hx_status st = exec_plan(P, P->plans[d], agg, parts[d], &agg_ms, &m);
        if (st != HX_OK) return st;
        agg_ms_max = std::max(agg_ms_max, agg_ms);
        decode_ms_max = std::max(decode_ms_max, P->plans[d].decode_ms);
        matched += m;
    }

    auto R = std::make_unique<hx_result_impl>();
    hx_result_table& T = R->pub_;
    if (parts.size() == 1) {
        R->owned = parts[0];
        parts[0].buf = nullptr;  // ownership moved
        parts[0].buf2 = nullptr;
        const HostTable& H = R->owned;
        T.n_groups = H.n;
        T.series_id = H.series;
        T.bucket = bucket ? H.bucket : nullptr;
        T.sum = (agg->ops & HX_AGG_SUM) ? H.sum : nullptr;
        T.count = (agg->ops & HX_AGG_COUNT) ? (const uint64_t*)H.cnt : nullptr;
        T.vmin = (agg->ops & HX_AGG_MIN) ? H.vmin : nullptr;
        T.vmax = (agg->ops & HX_AGG_MAX) ? H.vmax : nullptr;
        T.avg = (agg->ops & HX_AGG_AVG) ? H.avg : nullptr;
        if (agg->ops & HX_AGG_FIRST) {
            T.first = (const double*)H.first;
            T.first_ts = H.first_ts;
        }
        if (agg->ops & HX_AGG_LAST) {
            T.last = (const double*)H.last;
            T.last_ts = H.last_ts;
        }
    } else {
        merge_partials(parts, agg->ops, bucket, R->store);
        for (auto& p : parts) p.release();
        T.n_groups = R->store.series.size();
        T.series_id = R->store.series.data();
        T.bucket = bucket ? R->store.bucket.data() : nullptr;
        T.sum = (agg->ops & HX_AGG_SUM) ? R->store.sum.data() : nullptr;
        T.count = (agg->ops & HX_AGG_COUNT) ? (const uint64_t*)R->store.cnt.data() : nullptr;
        T.vmin = (agg->ops & HX_AGG_MIN) ? R->store.vmin.data() : nullptr;
        T.vmax = (agg->ops & HX_AGG_MAX) ? R->store.vmax.data() : nullptr;
        T.avg = (agg->ops & HX_AGG_AVG) ? R->store.avg.data() : nullptr;
        if (agg->ops & HX_AGG_FIRST) {
            T.first = (const double*)R->store.first.data();
            T.first_ts = R->store.first_ts.data();
        }
        if (agg->ops & HX_AGG_LAST) {
            T.last = (const double*)R->store.last.data();
            T.last_ts = R->store.last_ts.data();
        }
    }

    P->last_stats.exec_ms = std::chrono::duration<double, std::milli>(
                                std::chrono::steady_clock::now() - t0).count();
    P->last_stats.agg_kernel_ms = agg_ms_max;
    P->last_stats.decode_kernel_ms = decode_ms_max;
    P->last_stats.rows_scanned = P->rows_scanned_total;
    P->last_stats.rows_matched = (int64_t)matched;
    P->last_stats.bytes_staged = P->bytes_staged;
    P->last_stats.stage_ms = P->stage_ms;

    *out = &R.release()->pub_;
    return HX_OK;
}

extern "C" void hx_result_free(hx_result_table* t) {
    if (!t) return;
    // pub_ is the first member of hx_result_impl
    delete reinterpret_cast<hx_result_impl*>(t);
}

extern "C" hx_status hx_get_stats(hx_prepared* P, hx_exec_stats* out) {
    if (!P || !out) return fail(HX_ERR_INVALID, "null argument");
    *out = P->last_stats;
    return HX_OK;
}

extern "C" hx_status hx_get_decode_stats(hx_prepared* P, hx_decode_stats* out) {
    if (!P || !out) return fail(HX_ERR_INVALID, "null argument");
    hx_decode_stats s{};
    for (const DevPlan& plan : P->plans) {
        s.pages_in_place += plan.pages_in_place;
        s.bytes_in_place += plan.bytes_in_place;
        s.pages_decoded += plan.snappy_pages.size() +
                           plan.snappy_ba_pages.size();
        for (const auto& sp : plan.snappy_pages)
            s.bytes_decoded_out += sp.uncomp_len;
        for (const auto& sp : plan.snappy_ba_pages)
            s.bytes_decoded_out += sp.uncomp_len;
    }
    *out = s;
    return HX_OK;
}

namespace {

// device allocations freed at scope exit
struct DevBufs {
    std::vector<void*> p;
    explicit DevBufs(size_t n_slots = 0) : p(n_slots, nullptr) {}
    ~DevBufs() {
        for (void* q : p)
            if (q) (void)hipFree(q);
    }
    hipError_t alloc(void** out, size_t bytes) {
        hipError_t e = hipMalloc(out, bytes ? bytes : 1);
        if (e == hipSuccess) p.push_back(*out);
        return e;
    }
};

// the radix sort's temporary storage where no plan owns it
struct SortTemp {
    void* p = nullptr;
    size_t cap = 0;
    ~SortTemp() { if (p) (void)hipFree(p); }
};

// HX_DEBUG stage timers: N events, created on demand, destroyed at scope exit
template <int N>
struct HipEvents {
    hipEvent_t e[N] = {};
    ~HipEvents() {
        for (hipEvent_t v : e)
            if (v) (void)hipEventDestroy(v);
    }
    hipError_t create() {
        for (hipEvent_t& v : e) HIP_RET(hipEventCreate(&v));
        return hipSuccess;
    }
    hipEvent_t operator[](int i) const { return e[i]; }
};

}  // namespace

extern "C" hx_status hx_debug_page_levels(
    const char* path, int32_t row_group, const char* column,
    uint64_t* bitmap_out, uint64_t cap_words, int64_t* n_rows,
    int64_t* n_valid, int32_t* level_bytes) {
    if (!path || !column || !n_rows || !n_valid || !level_bytes)
        return fail(HX_ERR_INVALID, "null argument");
    static const char* const names[4] = {"series_id", "timestamp", "value",
                                         "__seq__"};
    int col = -1;
    for (int k = 0; k < 4; k++)
        if (std::strcmp(column, names[k]) == 0) col = k;
    if (col < 0)
        return fail(HX_ERR_INVALID, std::string("column ") + column +
                                        " is not one staging reads");
    CatSst cat;
    hx_status st = read_file_meta(path, 0, cat);
    if (st != HX_OK) return st;
    if (row_group < 0 || size_t(row_group) >= cat.rgs.size())
        return fail(HX_ERR_INVALID, "row group out of range");
    const ChunkRef& cr = cat.rgs[row_group].cols[col];
    int fd = open(path, O_RDONLY);
    if (fd < 0) return fail(HX_ERR_IO, "open " + cat.path);
    std::vector<uint8_t> tmp;
    hx::StageStatus s = hx::read_chunk(fd, cat.path, cr, tmp);
    close(fd);
    if (!s.ok()) return fail(s.st, s.msg);
    // the chunk is staged as hx_prepare stages it, into a slot of its own
    std::vector<uint8_t> slot_mem(hx::chunk_reserve(cr));
    hx::ChunkSlot slot;
    slot.base = slot_mem.data();
    slot.cap = slot_mem.size();
    slot.bitmap = bitmap_out;
    slot.bitmap_cap = size_t(cap_words) * 8;
    hx::ChunkRole role;
    role.col = col;
    role.bytes_value = cat.bytes_value;
    std::atomic<size_t> dec{0};
    std::atomic<size_t> tail{hx::align64(slot_mem.size())};
    hx::StagedPages pages;
    hx::ChunkResult res;
    s = hx::stage_chunk(tmp.data(), cr, role, slot, dec, pages, res, &tail);
    if (!s.ok()) return fail(s.st, cat.path + ": " + s.msg);
    *n_rows = cr.num_values;
    *n_valid = res.n_valid;
    *level_bytes = int32_t(res.level_bytes);
    if (cr.required && bitmap_out) {
        for (size_t i = 0; i < (size_t(cr.num_values) + 63) / 64; i++)
            bitmap_out[i] = 0;
        hx_bitmap_set_range(bitmap_out, 0, uint64_t(cr.num_values));
    }
    return HX_OK;
}

extern "C" hx_status hx_debug_snappy_decompress(
    const uint8_t* streams, const uint64_t* offs, const uint32_t* comp_lens,
    const uint32_t* uncomp_lens, uint32_t n, uint8_t* out,
    const uint64_t* out_offs, uint64_t* n_errors) {
    if (!n_errors || (n && (!streams || !offs || !comp_lens || !uncomp_lens ||
                            !out || !out_offs)))
        return fail(HX_ERR_INVALID, "null argument");
    *n_errors = 0;
    if (n == 0) return HX_OK;
    // same layout staging produces: payloads 64-byte aligned in one blob,
    // outputs 64-byte aligned in one dec region, 64 bytes of slack on each
    std::vector<hx::SnappyPageDesc> pages(n);
    size_t blob_bytes = 0, dec_bytes = 0;
    for (uint32_t i = 0; i < n; i++) {
        pages[i].src_off = blob_bytes;
        pages[i].dst_off = hx::OFF_DEC | dec_bytes;
        pages[i].comp_len = comp_lens[i];
        pages[i].uncomp_len = uncomp_lens[i];
        blob_bytes = align64(blob_bytes + comp_lens[i]);
        dec_bytes = align64(dec_bytes + uncomp_lens[i]);
    }
    std::vector<uint8_t> h_blob(blob_bytes + 64, 0);
    for (uint32_t i = 0; i < n; i++)
        std::memcpy(h_blob.data() + pages[i].src_off, streams + offs[i],
                    comp_lens[i]);
    DevBufs dev(4);
    HIP_TRY(hipMalloc(&dev.p[0], h_blob.size()));
    HIP_TRY(hipMalloc(&dev.p[1], dec_bytes + 64));
    HIP_TRY(hipMalloc(&dev.p[2], size_t(n) * sizeof(hx::SnappyPageDesc)));
    HIP_TRY(hipMalloc(&dev.p[3], sizeof(unsigned long long)));
    HIP_TRY(hipMemcpy(dev.p[0], h_blob.data(), h_blob.size(),
                      hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(dev.p[1], 0xEE, dec_bytes + 64));
    HIP_TRY(hipMemcpy(dev.p[2], pages.data(),
                      size_t(n) * sizeof(hx::SnappyPageDesc),
                      hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(dev.p[3], 0, sizeof(unsigned long long)));
    HIP_TRY(hx::launch_snappy(nullptr, (const uint8_t*)dev.p[0],
                              (uint8_t*)dev.p[1],
                              (const hx::SnappyPageDesc*)dev.p[2], n,
                              (unsigned long long*)dev.p[3]));
    HIP_TRY(hipDeviceSynchronize());
    std::vector<uint8_t> h_dec(dec_bytes + 64);
    HIP_TRY(hipMemcpy(h_dec.data(), dev.p[1], h_dec.size(),
                      hipMemcpyDeviceToHost));
    unsigned long long errs = 0;
    HIP_TRY(hipMemcpy(&errs, dev.p[3], sizeof(errs), hipMemcpyDeviceToHost));
    for (uint32_t i = 0; i < n; i++)
        std::memcpy(out + out_offs[i],
                    h_dec.data() + (pages[i].dst_off & hx::OFF_MASK),
                    uncomp_lens[i]);
    *n_errors = errs;
    return HX_OK;
}

extern "C" hx_status hx_debug_pack_optional(
    const uint64_t* values, const uint64_t* valid_words,
    const uint8_t* valid_bits, const uint32_t* perm, uint32_t n_src,
    uint32_t n, uint32_t row_group, uint64_t* packed_out,
    uint64_t* bitmap_out, uint32_t* n_valid_out, uint64_t* n_errors) {
    if (!n_errors || (valid_words && valid_bits) || (n_src && !values) ||
        (n && (!packed_out || !bitmap_out || !n_valid_out)))
        return fail(HX_ERR_INVALID, "bad argument");
    if (row_group == 0 || row_group % 64)
        return fail(HX_ERR_INVALID, "row_group is not a multiple of 64");
    *n_errors = 0;
    if (n == 0) return HX_OK;
    const size_t n_groups = (size_t(n) + row_group - 1) / row_group;
    const size_t bm_words = n_groups * (row_group / 64);
    const size_t valid_bytes =
        valid_words ? size_t(n_src) * 8 : valid_bits ? (size_t(n_src) + 7) / 8
                                                     : 0;
    DevBufs dev(7);
    // every buffer exactly as large as the contract says it is
    HIP_TRY(hipMalloc(&dev.p[0], std::max<size_t>(size_t(n_src) * 8, 8)));
    HIP_TRY(hipMalloc(&dev.p[1], std::max<size_t>(valid_bytes, 8)));
    HIP_TRY(hipMalloc(&dev.p[2], size_t(n) * 4));
    HIP_TRY(hipMalloc(&dev.p[3], size_t(n) * 8));
    HIP_TRY(hipMalloc(&dev.p[4], bm_words * 8));
    HIP_TRY(hipMalloc(&dev.p[5], n_groups * 4));
    HIP_TRY(hipMalloc(&dev.p[6], 8));
    if (n_src)
        HIP_TRY(hipMemcpy(dev.p[0], values, size_t(n_src) * 8,
                          hipMemcpyHostToDevice));
    if (valid_bytes)
        HIP_TRY(hipMemcpy(dev.p[1],
                          valid_words ? (const void*)valid_words
                                      : (const void*)valid_bits,
                          valid_bytes, hipMemcpyHostToDevice));
    if (perm)
        HIP_TRY(hipMemcpy(dev.p[2], perm, size_t(n) * 4,
                          hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(dev.p[3], 0xEE, size_t(n) * 8));
    HIP_TRY(hipMemset(dev.p[4], 0xEE, bm_words * 8));
    HIP_TRY(hipMemset(dev.p[5], 0xEE, n_groups * 4));
    HIP_TRY(hipMemset(dev.p[6], 0, 8));
    HIP_TRY(hx::launch_pack_optional(
        nullptr, (const unsigned long long*)dev.p[0],
        valid_bytes ? dev.p[1] : nullptr, valid_bits != nullptr,
        perm ? (const uint32_t*)dev.p[2] : nullptr, n_src, n, row_group,
        (unsigned long long*)dev.p[3], (uint64_t*)dev.p[4],
        (uint32_t*)dev.p[5], (unsigned long long*)dev.p[6]));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(packed_out, dev.p[3], size_t(n) * 8,
                      hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(bitmap_out, dev.p[4], bm_words * 8,
                      hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(n_valid_out, dev.p[5], n_groups * 4,
                      hipMemcpyDeviceToHost));
    unsigned long long errs = 0;
    HIP_TRY(hipMemcpy(&errs, dev.p[6], 8, hipMemcpyDeviceToHost));
    *n_errors = errs;
    return HX_OK;
}

extern "C" hx_status hx_debug_snappy_compress(
    const uint8_t* pages, const uint64_t* offs, const uint32_t* lens,
    uint32_t n_pages, const uint32_t* src_align, uint8_t* out,
    const uint64_t* out_offs, uint32_t* out_lens, uint64_t* n_errors) {
    if (!n_errors || !out_offs ||
        (n_pages && (!pages || !offs || !lens || !src_align || !out ||
                     !out_lens)))
        return fail(HX_ERR_INVALID, "null argument");
    *n_errors = 0;
    if (n_pages == 0) return HX_OK;
    std::vector<hx::SnappyCompDesc> descs(n_pages);
    size_t src_bytes = 0;
    for (uint32_t i = 0; i < n_pages; i++) {
        if (src_align[i] > 63 || out_offs[i + 1] < out_offs[i] ||
            out_offs[i + 1] - out_offs[i] > 0xFFFFFFFFull)
            return fail(HX_ERR_INVALID, "bad src_align or out_offs");
        descs[i].src_off = align64(src_bytes) + src_align[i];
        descs[i].dst_off = out_offs[i];
        descs[i].n = lens[i];
        descs[i].dst_cap = uint32_t(out_offs[i + 1] - out_offs[i]);
        src_bytes = descs[i].src_off + lens[i];
    }
    const size_t out_bytes = out_offs[n_pages];
    std::vector<uint8_t> h_src(src_bytes, 0);
    for (uint32_t i = 0; i < n_pages; i++)
        if (lens[i])
            std::memcpy(h_src.data() + descs[i].src_off, pages + offs[i],
                        lens[i]);
    DevBufs dev(5);
    // every buffer exactly as large as the contract says it is
    HIP_TRY(hipMalloc(&dev.p[0], std::max<size_t>(src_bytes, 1)));
    HIP_TRY(hipMalloc(&dev.p[1], std::max<size_t>(out_bytes, 1)));
    HIP_TRY(hipMalloc(&dev.p[2], size_t(n_pages) * sizeof(descs[0])));
    HIP_TRY(hipMalloc(&dev.p[3], size_t(n_pages) * 4));
    HIP_TRY(hipMalloc(&dev.p[4], 8));
    if (src_bytes)
        HIP_TRY(hipMemcpy(dev.p[0], h_src.data(), src_bytes,
                          hipMemcpyHostToDevice));
    if (out_bytes) HIP_TRY(hipMemset(dev.p[1], 0xEE, out_bytes));
    HIP_TRY(hipMemcpy(dev.p[2], descs.data(),
                      size_t(n_pages) * sizeof(descs[0]),
                      hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(dev.p[3], 0xEE, size_t(n_pages) * 4));
    HIP_TRY(hipMemset(dev.p[4], 0, 8));
    HIP_TRY(hx::launch_snappy_compress(
        nullptr, (const uint8_t*)dev.p[0], (uint8_t*)dev.p[1],
        (const hx::SnappyCompDesc*)dev.p[2], n_pages, (uint32_t*)dev.p[3],
        (unsigned long long*)dev.p[4]));
    HIP_TRY(hipDeviceSynchronize());
    if (out_bytes)
        HIP_TRY(hipMemcpy(out, dev.p[1], out_bytes, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(out_lens, dev.p[3], size_t(n_pages) * 4,
                      hipMemcpyDeviceToHost));
    unsigned long long errs = 0;
    HIP_TRY(hipMemcpy(&errs, dev.p[4], 8, hipMemcpyDeviceToHost));
    *n_errors = errs;
    return HX_OK;
}

extern "C" hx_status hx_scan_agg(hx_handle* h, const hx_scan_spec* spec,
                                 const hx_agg_spec* agg,
                                 const hx_device_set* devs,
                                 hx_result_table** out) {
    hx_prepared* prep = nullptr;
    hx_status st = hx_prepare(h, spec, devs, &prep);
    if (st != HX_OK) return st;
    st = hx_exec_agg(prep, agg, out);
    hx_prepared_free(prep);
    return st;
}

namespace {

// The (series, ts) sort permutation of the ingest sort and of every row
// stream: stable, equal PKs keep the order they come in. Two stable LSD radix
// passes over a u32 permutation, ts (sign-biased) then series; pc receives
// the result, d_ka / d_kb / pb are N-entry scratch. pa is the order the rows
// come in: iota, written here, unless pa_given (the Append pass of
// sorted_row_stream has already ordered it by sequence).
hipError_t ingest_sort_perm(hipStream_t s, const uint64_t* d_series,
                            const int64_t* d_ts, uint64_t* d_ka,
                            uint64_t* d_kb, uint32_t* pa, uint32_t* pb,
                            uint32_t* pc, size_t N, void** d_temp,
                            size_t* temp_cap, bool pa_given = false) {
    if (!pa_given) HIP_RET(hx::launch_iota(s, pa, (uint32_t)N));
    HIP_RET(hx::launch_gather_u64(s, (const unsigned long long*)d_ts, pa,
                                  (unsigned long long*)d_ka, (uint32_t)N));
    HIP_RET(hx::launch_xor_sign(s, (unsigned long long*)d_ka, (uint32_t)N));
    HIP_RET(hx::sort_pairs_u64(s, d_ka, d_kb, pa, pb, N, d_temp, temp_cap));
    HIP_RET(hx::launch_gather_u64(s, (const unsigned long long*)d_series, pb,
                                  (unsigned long long*)d_ka, (uint32_t)N));
    HIP_RET(hx::sort_pairs_u64(s, d_ka, d_kb, pb, pc, N, d_temp, temp_cap));
    return hipSuccess;
}

using PreparedPtr = std::unique_ptr<hx_prepared, void (*)(hx_prepared*)>;

// hx_prepare on the first device given (device 0 without one): the row
// stream routes are single-device
hx_status prepare_single(hx_handle* h, const hx_scan_spec* spec,
                         const hx_device_set* devs, PreparedPtr& out) {
    int32_t dev0 = (devs && devs->device_ids && devs->n_devices > 0)
                       ? devs->device_ids[0] : 0;
    hx_device_set one{&dev0, 1};
    hx_prepared* P = nullptr;
    hx_status st = hx_prepare(h, spec, &one, &P);
    out.reset(P);
    return st;
}

// The filtered row stream of a prepared plan, in (series, ts) order: what
// hx_scan, compact_rows and compact_rows_bytes start from. Views into
// plan.d_scratch, valid until the plan's scratch is used again.
struct RowStream {
    uint64_t* series = nullptr;
    long long* ts = nullptr;
    double* val = nullptr;        // f64 values, or Binary value handles
    uint64_t* seq = nullptr;      // null unless asked for (or Append)
    uint64_t* valid = nullptr;    // one 0/1 word per row; null unless the
                                  // plan staged a null
    uint64_t* keys = nullptr;     // two n-word buffers, free for the caller
    uint64_t* keys_out = nullptr; // after the sort
    uint32_t* perm = nullptr;     // rows in (series, ts) order
    uint32_t* spare_a = nullptr;  // two more n-entry permutations
    uint32_t* spare_b = nullptr;
    uint32_t n = 0;               // surviving rows; 0: no view is to be used
};

// Scan (filter, and last-wins dedup unless Append), count, sort. Append
// (UpdateMode config.rs:166-172 -> BytesMergeOperator, operator.rs:47-111)
// keeps every row, and a leading stable pass on the packed (seq << 32 | file
// row) key leaves equal-PK rows in ascending __seq__ order, the operator's
// concat order (MergeStream group order, read.rs:289-343). `what` names the
// caller in the overflow message.
hx_status sorted_row_stream(hx_handle* h, hx_prepared* P, DevPlan& plan,
                            bool want_seq, bool append, const char* what,
                            RowStream& out) {
    out = RowStream{};
    HIP_TRY(hipSetDevice(plan.device));
    hipStream_t s = plan.stream;
    hx_status st = ensure_decoded(plan, s);
    if (st != HX_OK) return st;
    st = ensure_sset(P, plan);
    if (st != HX_OK) return st;
    const uint64_t cap = (uint64_t)plan.rows_scanned;
    if (cap == 0) return HX_OK;
    if (cap > 0xFFFFFFFFull)
        return fail(HX_ERR_UNSUPPORTED,
                    "row streams above 2^32 rows per call: split the range");
    if (append)   // the packed sort key has 32 bits for the sequence
        for (const auto& c : h->ssts)
            if (c.seq >= (1ull << 32))
                return fail(HX_ERR_UNSUPPORTED,
                            "append stores need file sequences < 2^32");
    want_seq = want_seq || append;
    const bool nulls = plan.has_nulls;   // never with Append / Binary values
    // 8-byte buffers first (3 columns, 2 key buffers [, seq] [, valid], the
    // cursor), the three permutations last
    const size_t need =
        cap * 8 * (5 + (want_seq ? 1 : 0) + (nulls ? 1 : 0)) + cap * 4 * 3 + 64;
    st = ensure_dev(&plan.d_scratch, &plan.scratch_cap, need);
    if (st != HX_OK) return st;
    uint64_t* w = (uint64_t*)plan.d_scratch;
    auto carve8 = [&](size_t count) {
        uint64_t* p = w;
        w += count;
        return p;
    };
    out.series = carve8(cap);
    out.ts = (long long*)carve8(cap);
    out.val = (double*)carve8(cap);
    if (want_seq) out.seq = carve8(cap);
    if (nulls) out.valid = carve8(cap);
    out.keys = carve8(cap);
    out.keys_out = carve8(cap);
    unsigned long long* d_cursor = (unsigned long long*)carve8(1);
    uint32_t* pa = (uint32_t*)w;
    uint32_t* pb = pa + cap;
    uint32_t* pc = pb + cap;

    HIP_TRY(hipMemsetAsync(d_cursor, 0, 8, s));
    hx::AggParams A = base_params(P, plan);
    if (append) A.keep_dups = 1;   // keep every row: groups concatenate
    HIP_TRY(hx::launch_scan_rows(s, A, 0, A.n_rgs, out.series, out.ts,
                                 out.val, d_cursor, cap, out.seq,
                                 append ? 1 : 0, out.valid));
    unsigned long long n64 = 0;
    HIP_TRY(hipStreamSynchronize(s));
    HIP_TRY(hipMemcpy(&n64, d_cursor, 8, hipMemcpyDeviceToHost));
    if (n64 > cap)
        return fail(HX_ERR_HIP, std::string(what) + " row buffer overflow");
    const uint32_t n = (uint32_t)n64;
    if (n == 0) return HX_OK;

    // LSD-stable ordering: [seq,] ts, then series
    if (append) {
        HIP_TRY(hx::launch_iota(s, pa, n));
        HIP_TRY(hx::launch_gather_u64(s, (const unsigned long long*)out.seq,
                                      pa, (unsigned long long*)out.keys, n));
        HIP_TRY(hx::sort_pairs_u64(s, out.keys, out.keys_out, pa, pb, n,
                                   &plan.d_sort_temp, &plan.sort_temp_cap));
        std::swap(pa, pb);
    }
    HIP_TRY(ingest_sort_perm(s, out.series, (const int64_t*)out.ts, out.keys,
                             out.keys_out, pa, pb, pc, n, &plan.d_sort_temp,
                             &plan.sort_temp_cap, append));
    out.perm = pc;
    out.spare_a = pa;
    out.spare_b = pb;
    out.n = n;
    return HX_OK;
}

}  // namespace

extern "C" hx_status hx_scan(hx_handle* h, const hx_scan_spec* spec,
                             const hx_device_set* devs, hx_batch_cb cb,
                             void* ctx) {
    // Streaming parity mode: the merged, deduplicated
    // row stream of ColumnarStorage::scan (storage.rs:335-370): segments in
    // ascending time order, rows sorted by (series_id, timestamp) within
    // each segment (the per-segment SortPreservingMerge + MergeExec output,
    // read.rs:429-494). GPU: filter/dedup append + radix sorts; single
    // device.
    if (!h || !spec || !cb) return fail(HX_ERR_INVALID, "null argument");
    const bool bytesv = h->bytes_value;
    // Append mode: equal-PK groups concatenate their value bytes in the
    // order sorted_row_stream leaves them in
    const bool append = h->update_mode == 1;
    if (append && !bytesv)
        return fail(HX_ERR_UNSUPPORTED,
                    "Append mode needs a Binary value column");
    PreparedPtr P(nullptr, hx_prepared_free);
    hx_status st = prepare_single(h, spec, devs, P);
    if (st != HX_OK) return st;
    DevPlan& plan = P->plans[0];
    RowStream rs;
    st = sorted_row_stream(h, P.get(), plan, false, append, "scan", rs);
    if (st != HX_OK) return st;
    const uint32_t n = rs.n;
    if (n == 0) return HX_OK;
    hipStream_t s = plan.stream;
    const bool nulls = rs.valid != nullptr;
    // fourth pass, most significant: the time segment of the (permuted) ts
    HIP_TRY(hx::launch_gather_u64(s, (const unsigned long long*)rs.ts,
                                  rs.perm, (unsigned long long*)rs.keys_out,
                                  n));
    HIP_TRY(hx::launch_seg_keys(s, (const long long*)rs.keys_out,
                                h->segment_ms, (unsigned long long*)rs.keys,
                                n));
    HIP_TRY(hx::sort_pairs_u64(s, rs.keys, rs.keys_out, rs.perm, rs.spare_a,
                               n, &plan.d_sort_temp, &plan.sort_temp_cap));
    const uint32_t* perm = rs.spare_a;

    // gather the three columns by the final permutation, one D2H
    const unsigned long long* srcs[4] = {
        (const unsigned long long*)rs.series, (const unsigned long long*)rs.ts,
        (const unsigned long long*)rs.val, (const unsigned long long*)rs.valid};
    const uint32_t n_src = nulls ? 4 : 3;
    // reuse keys buffers as gather dst (need 3n; keys has 2n) — allocate
    std::vector<uint64_t> host(n_src * size_t(n));
    DevBufs dev;
    unsigned long long* d_dst = nullptr;
    HIP_TRY(dev.alloc((void**)&d_dst, n_src * size_t(n) * 8));
    HIP_TRY(hx::launch_gather_multi(s, srcs, n_src, perm, d_dst, n));
    HIP_TRY(hipMemcpyAsync(host.data(), d_dst, n_src * size_t(n) * 8,
                           hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));

    // Binary value columns: the gathered "value" words are per-row handles
    // (blob_off << 20 | len, from k_ba_offsets). Materialize the output
    // byte stream on the GPU (k_copy_bytes moves the bytes; the host does
    // only the O(n) offset arithmetic), then batch groups to the caller.
    std::vector<uint8_t> hbytes;
    std::vector<int64_t> group_off;      // per emitted row (or group)
    std::vector<uint64_t> gseries;
    std::vector<int64_t> gts;
    uint32_t n_out_rows = n;
    if (bytesv) {
        const uint64_t* hnd = host.data() + 2 * size_t(n);
        const uint64_t* hs = host.data();
        const int64_t* ht = (const int64_t*)(host.data() + n);
        std::vector<int64_t> row_off(n + 1);
        row_off[0] = 0;
        for (uint32_t i = 0; i < n; i++)
            row_off[i + 1] = row_off[i] + int64_t(hnd[i] & 0xFFFFFu);
        // group layout: Append concatenates equal-PK runs (already
        // adjacent and seq-ordered); Overwrite has one row per group
        group_off.clear();
        gseries.clear();
        gts.clear();
        if (append) {
            for (uint32_t i = 0; i < n; i++) {
                if (i == 0 || hs[i] != hs[i - 1] || ht[i] != ht[i - 1]) {
                    gseries.push_back(hs[i]);
                    gts.push_back(ht[i]);
                    group_off.push_back(row_off[i]);
                }
            }
            group_off.push_back(row_off[n]);
            n_out_rows = (uint32_t)gseries.size();
        } else {
            n_out_rows = n;
        }
        const int64_t total = row_off[n];
        int64_t* d_offs = nullptr;
        uint8_t* d_bytes = nullptr;
        HIP_TRY(dev.alloc((void**)&d_offs, (size_t(n) + 1) * 8));
        HIP_TRY(dev.alloc((void**)&d_bytes, size_t(std::max<int64_t>(
                                                total, 1))));
        HIP_TRY(hipMemcpyAsync(d_offs, row_off.data(), (size_t(n) + 1) * 8,
                               hipMemcpyHostToDevice, s));
        HIP_TRY(hx::launch_copy_bytes(s, plan.d_blob,
                                      (const uint64_t*)(d_dst + 2 * size_t(n)),
                                      d_offs, d_bytes, n));
        hbytes.resize(size_t(std::max<int64_t>(total, 0)));
        if (total > 0)
            HIP_TRY(hipMemcpyAsync(hbytes.data(), d_bytes, size_t(total),
                                   hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        if (!append) {
            group_off = std::move(row_off);
        }
    }

    // projection over user columns (storage.rs:65-70; builtins stripped as
    // MergeStream does, read.rs:330-343)
    std::vector<int32_t> proj;
    if (spec->projection && spec->n_projection) {
        for (size_t i = 0; i < spec->n_projection; i++) {
            int32_t c = spec->projection[i];
            if (c < 0 || c > 2)
                return fail(HX_ERR_INVALID, "projection index out of range");
            proj.push_back(c);
        }
    } else {
        proj = {0, 1, 2};
    }
    const int32_t val_type = bytesv ? 3 : 2;
    const int32_t kTypes[3] = {0, 1, val_type};  // u64, i64, f64|bytes
    const uint64_t* cols_base[3] = {host.data(), host.data() + n,
                                    host.data() + 2 * size_t(n)};
    if (bytesv && append) {
        // group-level fixed columns replace the row-level ones
        cols_base[0] = gseries.data();
        cols_base[1] = (const uint64_t*)gts.data();
    }
    const uint32_t BATCH = 65536;
    std::vector<const void*> colptrs(proj.size());
    std::vector<int32_t> coltypes(proj.size());
    std::vector<int64_t> rebased;
    for (size_t i = 0; i < proj.size(); i++) coltypes[i] = kTypes[proj[i]];
    // validity: one bitmap per batch for the value column, NULL pointers for
    // the key columns; no array at all for a plan without nulls
    std::vector<uint8_t> vbits;
    std::vector<const uint8_t*> validity(proj.size(), nullptr);
    for (uint32_t off = 0; off < n_out_rows; off += BATCH) {
        uint32_t len = std::min(BATCH, n_out_rows - off);
        if (nulls) {
            const uint64_t* hv = host.data() + 3 * size_t(n) + off;
            vbits.assign((len + 7) / 8, 0);
            for (uint32_t r = 0; r < len; r++)
                if (hv[r]) vbits[r >> 3] |= uint8_t(1u << (r & 7));
            for (size_t i = 0; i < proj.size(); i++)
                validity[i] = proj[i] == 2 ? vbits.data() : nullptr;
        }
        hx_bytes_col bc{};
        for (size_t i = 0; i < proj.size(); i++) {
            if (proj[i] == 2 && bytesv) {
                rebased.assign(group_off.begin() + off,
                               group_off.begin() + off + len + 1);
                const int64_t base0 = rebased[0];
                for (auto& x : rebased) x -= base0;
                bc.offsets = rebased.data();
                bc.bytes = hbytes.data() + base0;
                colptrs[i] = (const void*)&bc;
            } else {
                colptrs[i] = (const void*)(cols_base[proj[i]] + off);
            }
        }
        hx_col_batch b{len, proj.size(), colptrs.data(), coltypes.data(),
                       nulls ? validity.data() : nullptr};
        if (cb(ctx, &b)) break;
    }
    return HX_OK;
}

extern "C" hx_status hx_write_sst(const char* path, const uint64_t* series,
                                  const int64_t* ts, const double* value,
                                  uint64_t seq, int64_t n_rows,
                                  int64_t row_group) {
    if (!path || !series || !ts || !value || n_rows <= 0 || row_group <= 0)
        return fail(HX_ERR_INVALID, "bad argument");
    std::string err = hx::write_metric_sst(path, series, ts, value, seq,
                                           n_rows, row_group);
    if (!err.empty()) return fail(HX_ERR_IO, err);
    return HX_OK;
}

namespace {

const int64_t kRowGroup = 8192;   // rows per row group of every SST written

// A value column in the nullable writer's row-group-major form (kernel 1d /
// pack_optional_host output), on the host.
struct PackedValues {
    std::vector<uint64_t> packed, bitmap;
    std::vector<uint32_t> n_valid;
    void resize(int64_t n, int64_t row_group) {
        const size_t n_groups = size_t((n + row_group - 1) / row_group);
        packed.resize(size_t(n));
        bitmap.resize(n_groups * size_t(row_group / 64));
        n_valid.resize(n_groups);
    }
    hx::NullableValues view() const {
        return {packed.data(), bitmap.data(), n_valid.data()};
    }
    // kernel 1d's host twin over n rows; order: the sort permutation or null
    void pack_host(const double* value, const uint8_t* validity,
                   const uint32_t* order, int64_t n, int64_t row_group) {
        resize(n, row_group);
        hx::pack_optional_host((const uint64_t*)value, validity, order,
                               (uint64_t)n, (uint64_t)n, (uint64_t)row_group,
                               packed.data(), bitmap.data(), n_valid.data());
    }
};

// Snappy streams of a file's pages, made on the device (kernel 1e) and
// brought to the host in one copy; `ready` is the table the writers take.
struct DeviceStreams {
    std::vector<uint8_t> bytes;
    std::vector<hx::PagePayload> ready;   // [row group * 5 + file column]
    bool on_device[5] = {};               // the column's rows stayed there
    size_t d2h_bytes = 0;                 // lengths, statistics and streams
};

// Kernel 1e over the kRowGroup-row slices of the columns that sit on the
// device: col_words[c] is file column c's offset in 8-byte words from d_base
// (n rows each), or -1 for a column the writer compresses itself. Then the
// scan-and-pack pass, the lengths and one contiguous D2H of the streams.
// k_page_minmax gives every page's footer statistics, so the rows of these
// columns need not cross PCIe at all (out.on_device).
// after_pack (may be null) is recorded behind the pack kernel. A page the
// kernel refused is an error: the slots here are at Snappy's bound.
hipError_t compress_columns_device(hipStream_t s, const uint8_t* d_base,
                                   const int64_t col_words[5], uint32_t n,
                                   hipEvent_t after_pack, DeviceStreams& out) {
    const size_t n_groups = (size_t(n) + kRowGroup - 1) / kRowGroup;
    std::vector<hx::SnappyCompDesc> descs;
    std::vector<uint32_t> entry;   // ready-table index of page i
    std::vector<uint32_t> kinds;   // the page's order, for its statistics
    const uint32_t col_kind[5] = {hx::PAGE_ORDER_U64, hx::PAGE_ORDER_I64,
                                  hx::PAGE_ORDER_F64, hx::PAGE_ORDER_U64,
                                  hx::PAGE_ORDER_U64};
    size_t slot_bytes = 0;
    for (int c = 0; c < 5; c++) {
        if (col_words[c] < 0) continue;
        for (size_t g = 0; g < n_groups; g++) {
            const size_t row0 = g * size_t(kRowGroup);
            const size_t rows = std::min<size_t>(kRowGroup, n - row0);
            hx::SnappyCompDesc d;
            d.src_off = (uint64_t(col_words[c]) + row0) * 8;
            d.n = uint32_t(rows * 8);
            d.dst_cap = uint32_t(hx::snappy_max_compressed(d.n));
            d.dst_off = slot_bytes;
            slot_bytes = align64(slot_bytes + d.dst_cap);
            descs.push_back(d);
            entry.push_back(uint32_t(g * 5 + size_t(c)));
            kinds.push_back(col_kind[c]);
        }
    }
    for (int c = 0; c < 5; c++) out.on_device[c] = col_words[c] >= 0;
    out.ready.assign(n_groups * 5, hx::PagePayload{nullptr, 0, 0, 0, 0});
    out.bytes.clear();
    out.d2h_bytes = 0;
    const uint32_t n_pages = uint32_t(descs.size());
    if (n_pages == 0)   // nothing on the device: the pair closes empty
        return after_pack ? hipEventRecord(after_pack, s) : hipSuccess;
    // one allocation: slots, packed streams, descriptors, kinds, the scan's
    // offsets, then what the host reads back first: lengths, error count,
    // statistics
    const size_t desc_bytes = align64(size_t(n_pages) * sizeof(descs[0]));
    const size_t kind_bytes = align64(size_t(n_pages) * 4);
    const size_t off_bytes = align64(size_t(n_pages) * 8);
    // the error count sits behind the lengths, 8-byte aligned, the
    // statistics behind it
    const size_t err_word = (size_t(n_pages) * 4 + 7) / 8;
    const size_t back_words =
        err_word + 1 + size_t(n_pages) * (sizeof(hx::PageStat) / 8);
    uint8_t* dev = nullptr;
    DevBufs bufs;
    HIP_RET(bufs.alloc((void**)&dev, 2 * slot_bytes + desc_bytes +
                                         kind_bytes + off_bytes +
                                         back_words * 8));
    uint8_t* d_slots = dev;
    uint8_t* d_packed = dev + slot_bytes;
    auto* d_descs = (hx::SnappyCompDesc*)(d_packed + slot_bytes);
    uint32_t* d_kinds = (uint32_t*)((uint8_t*)d_descs + desc_bytes);
    auto* d_offs = (unsigned long long*)((uint8_t*)d_kinds + kind_bytes);
    uint32_t* d_lens = (uint32_t*)((uint8_t*)d_offs + off_bytes);
    unsigned long long* d_err = (unsigned long long*)d_lens + err_word;
    hx::PageStat* d_stats = (hx::PageStat*)(d_err + 1);
    HIP_RET(hipMemcpyAsync(d_descs, descs.data(),
                           size_t(n_pages) * sizeof(descs[0]),
                           hipMemcpyHostToDevice, s));
    HIP_RET(hipMemcpyAsync(d_kinds, kinds.data(), size_t(n_pages) * 4,
                           hipMemcpyHostToDevice, s));
    HIP_RET(hipMemsetAsync(d_err, 0, 8, s));
    HIP_RET(hx::launch_snappy_compress(s, d_base, d_slots, d_descs, n_pages,
                                       d_lens, d_err));
    HIP_RET(hx::launch_page_minmax(s, d_base, d_descs, d_kinds, n_pages,
                                   d_stats));
    HIP_RET(hx::launch_snappy_pack(s, d_slots, d_descs, n_pages, d_lens,
                                   d_offs, d_packed));
    if (after_pack) HIP_RET(hipEventRecord(after_pack, s));
    std::vector<uint64_t> lens_host(back_words);
    HIP_RET(hipMemcpyAsync(lens_host.data(), d_lens, lens_host.size() * 8,
                           hipMemcpyDeviceToHost, s));
    HIP_RET(hipStreamSynchronize(s));
    if (lens_host[err_word] != 0) return hipErrorUnknown;
    const uint32_t* lens = (const uint32_t*)lens_host.data();
    size_t total = 0;
    for (uint32_t i = 0; i < n_pages; i++) total += lens[i];
    out.bytes.resize(total);
    HIP_RET(hipMemcpyAsync(out.bytes.data(), d_packed, total,
                           hipMemcpyDeviceToHost, s));
    HIP_RET(hipStreamSynchronize(s));
    const hx::PageStat* stats =
        (const hx::PageStat*)(lens_host.data() + err_word + 1);
    size_t at = 0;
    for (uint32_t i = 0; i < n_pages; i++) {
        out.ready[entry[i]] = hx::PagePayload{
            out.bytes.data() + at, lens[i], stats[i].has ? 1u : 2u,
            stats[i].min_bits, stats[i].max_bits};
        at += lens[i];
    }
    out.d2h_bytes = lens_host.size() * 8 + total;
    return hipSuccess;
}

// number of zero bits among the first n of an LSB-first bitmap
int64_t count_nulls(const uint8_t* validity, int64_t n) {
    if (!validity) return 0;
    int64_t ones = 0;
    for (int64_t b = 0; b < n / 8; b++) ones += __builtin_popcount(validity[b]);
    if (n % 8)
        ones += __builtin_popcount(validity[n / 8] & ((1u << (n % 8)) - 1u));
    return n - ones;
}

}  // namespace

extern "C" hx_status hx_write_sst_nullable(
    const char* path, const uint64_t* series, const int64_t* ts,
    const double* value, const uint8_t* validity, uint64_t seq,
    int64_t n_rows, int64_t row_group) {
    return hx_write_sst_codec(path, series, ts, value, validity, 1, seq,
                              n_rows, row_group, HX_CODEC_NONE);
}

extern "C" hx_status hx_write_sst_codec(
    const char* path, const uint64_t* series, const int64_t* ts,
    const double* value, const uint8_t* validity, int32_t nullable,
    uint64_t seq, int64_t n_rows, int64_t row_group, int32_t codec) {
    if (!path || !series || !ts || !value || n_rows <= 0 || row_group <= 0)
        return fail(HX_ERR_INVALID, "bad argument");
    if (codec != HX_CODEC_NONE && codec != HX_CODEC_SNAPPY)
        return fail(HX_ERR_INVALID, "write codec: 0 none / 1 snappy");
    if (nullable != 0 && nullable != 1)
        return fail(HX_ERR_INVALID, "nullable: 0 REQUIRED / 1 OPTIONAL");
    std::string err;
    if (!nullable) {
        if (validity)
            return fail(HX_ERR_INVALID,
                        "validity given for a REQUIRED value column");
        err = hx::write_metric_sst(path, series, ts, value, seq, n_rows,
                                   row_group, codec);
    } else {
        if (row_group % 64)
            return fail(HX_ERR_INVALID, "row_group is not a multiple of 64");
        PackedValues pv;
        pv.pack_host(value, validity, nullptr, n_rows, row_group);
        err = hx::write_metric_sst_nullable(path, series, ts, pv.view(),
                                            nullptr, seq, n_rows, row_group,
                                            codec);
    }
    if (!err.empty()) return fail(HX_ERR_IO, err);
    return HX_OK;
}

extern "C" uint64_t hx_debug_snappy_compress_host(const uint8_t* src,
                                                  uint64_t n, uint8_t* dst,
                                                  uint64_t cap) {
    return hx::snappy_compress_host(src, size_t(n), dst, size_t(cap));
}

// ---------------------------------------------------------------------------
// what hx_write, hx_write_bytes and the compactions share around their routes
// ---------------------------------------------------------------------------

// Segment-crossing check of a write (storage.rs:309-316). The reference uses
// Rust truncating division on start/seg vs (end-1)/seg, where end is the
// exclusive max; C++ `/` truncates the same way, so negative-timestamp writes
// agree with the reference.
static hx_status check_segment(const hx_handle* h, const int64_t* ts,
                               int64_t n) {
    const auto mm = std::minmax_element(ts, ts + n);
    if (*mm.first / h->segment_ms != *mm.second / h->segment_ms)
        return fail(HX_ERR_INVALID,
                    "write crosses a segment boundary (storage.rs:309-316)");
    return HX_OK;
}

// The host route's ingest sort: the stable (series, ts) order, equal PKs keep
// batch order (LastValueOperator's last-wins, operator.rs:37-44, and the
// scan's Append key (seq << 32 | file row) depend on it).
static std::vector<uint32_t> host_pk_order(const uint64_t* series,
                                           const int64_t* ts, int64_t n) {
    std::vector<uint32_t> order(n);
    for (int64_t i = 0; i < n; i++) order[i] = (uint32_t)i;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
        if (series[a] != series[b]) return series[a] < series[b];
        return ts[a] < ts[b];
    });
    return order;
}

// A fresh file: its id (= sequence, one above the catalog's highest,
// sst.rs:39-46) and its path.
struct NewSst {
    uint64_t seq;
    std::string path;
};

static NewSst next_sst(const hx_handle* h) {
    uint64_t max_seq = 0;
    for (const auto& s : h->ssts) max_seq = std::max(max_seq, s.seq);
    return {max_seq + 1,
            h->store + "/data/" + std::to_string(max_seq + 1) + ".sst"};
}

// manifest add_file (manifest/mod.rs:115-157): the written file, read back
static hx_status catalog_add(hx_handle* h, const NewSst& f) {
    CatSst fresh;
    hx_status st = read_file_meta(f.path, f.seq, fresh);
    if (st != HX_OK) return st;
    h->ssts.push_back(std::move(fresh));
    return HX_OK;
}

// A compaction's catalog update: add the new file, drop + unlink the inputs
// (add-before-delete, executor.rs:206-220).
static hx_status finish_compaction(hx_handle* h, const NewSst& f,
                                   const std::vector<char>& in_set,
                                   uint64_t* out_new_seq) {
    CatSst fresh;
    hx_status st = read_file_meta(f.path, f.seq, fresh);
    if (st != HX_OK) return st;
    std::vector<CatSst> kept;
    for (size_t i = 0; i < h->ssts.size(); i++) {
        if (in_set[i]) {
            unlink(h->ssts[i].path.c_str());  // best-effort, like the reference
            continue;
        }
        kept.push_back(std::move(h->ssts[i]));
    }
    kept.push_back(std::move(fresh));
    std::sort(kept.begin(), kept.end(),
              [](const CatSst& a, const CatSst& b) { return a.seq < b.seq; });
    h->ssts = std::move(kept);
    *out_new_seq = f.seq;
    return HX_OK;
}

// GPU ingest sort (stable by (series, ts); equal PKs keep input order):
// ingest_sort_perm, then a device gather and one D2H. Any HIP error is
// returned, not reported: the caller falls back to the host sort. With `pv`
// (nullable writer) the validity bitmap is uploaded as it is, n / 8 bytes,
// the gather takes series and ts only, and kernel 1d packs the values by the
// same permutation; v2 is not written. With `streams` (write codec Snappy)
// kernel 1e compresses the sorted columns where the gather left them (series,
// ts and, in the REQUIRED form, value) and their streams come back too.
static hipError_t gpu_sort_batch(const uint64_t* series, const int64_t* ts,
                                 const double* value, int64_t n,
                                 std::vector<uint64_t>& s2,
                                 std::vector<int64_t>& t2,
                                 std::vector<double>& v2,
                                 const uint8_t* validity = nullptr,
                                 PackedValues* pv = nullptr,
                                 DeviceStreams* streams = nullptr) {
    hipStream_t s = nullptr;
    uint8_t* dev = nullptr;
    DevBufs bufs;
    SortTemp temp;
    const size_t N = (size_t)n;
    const size_t n_groups = (N + kRowGroup - 1) / kRowGroup;
    const size_t bm_words = n_groups * (kRowGroup / 64);
    // layout: series, ts, value, keys_a, keys_b, dst(3N), perm a/b/c
    // [, validity bitmap, output bitmaps, n_valid, error count]
    size_t bytes = N * 8 * 8 + N * 4 * 3 + 256;
    if (pv) bytes += (N + 7) / 8 + 8 + bm_words * 8 + n_groups * 4 + 8 + 16;
    HIP_RET(bufs.alloc((void**)&dev, bytes));
    uint8_t* p = dev;
    auto carve = [&](size_t cnt, size_t w) {
        uint8_t* q = p;
        p += (cnt * w + 7) & ~size_t(7);
        return q;
    };
    uint64_t* d_series = (uint64_t*)carve(N, 8);
    int64_t* d_ts = (int64_t*)carve(N, 8);
    double* d_val = (double*)carve(N, 8);
    uint64_t* d_ka = (uint64_t*)carve(N, 8);
    uint64_t* d_kb = (uint64_t*)carve(N, 8);
    unsigned long long* d_dst = (unsigned long long*)carve(N * 3, 8);
    uint32_t* pa = (uint32_t*)carve(N, 4);
    uint32_t* pb = (uint32_t*)carve(N, 4);
    uint32_t* pc = (uint32_t*)carve(N, 4);
    HIP_RET(hipMemcpyAsync(d_series, series, N * 8, hipMemcpyHostToDevice, s));
    HIP_RET(hipMemcpyAsync(d_ts, ts, N * 8, hipMemcpyHostToDevice, s));
    HIP_RET(hipMemcpyAsync(d_val, value, N * 8, hipMemcpyHostToDevice, s));
    HIP_RET(ingest_sort_perm(s, d_series, d_ts, d_ka, d_kb, pa, pb, pc, N,
                             &temp.p, &temp.cap));
    const unsigned long long* srcs[3] = {
        (const unsigned long long*)d_series, (const unsigned long long*)d_ts,
        (const unsigned long long*)d_val};
    std::vector<uint64_t> host(3 * N);
    if (pv) {
        uint8_t* d_vbits = carve((N + 7) / 8, 1);
        uint64_t* d_bm = (uint64_t*)carve(bm_words, 8);
        uint32_t* d_nv = (uint32_t*)carve(n_groups, 4);
        unsigned long long* d_err = (unsigned long long*)carve(1, 8);
        if (validity)
            HIP_RET(hipMemcpyAsync(d_vbits, validity, (N + 7) / 8,
                                   hipMemcpyHostToDevice, s));
        HIP_RET(hipMemsetAsync(d_err, 0, 8, s));
        HIP_RET(hx::launch_gather_multi(s, srcs, 2, pc, d_dst, (uint32_t)N));
        HIP_RET(hx::launch_pack_optional(
            s, (const unsigned long long*)d_val, validity ? d_vbits : nullptr,
            true, pc, (uint32_t)N, (uint32_t)N, (uint32_t)kRowGroup,
            d_dst + 2 * N, d_bm, d_nv, d_err));
        pv->resize(n, kRowGroup);
        unsigned long long errs = 0;
        // with streams only the packed values come back, series and ts stay
        const size_t from = streams ? 2 * N : 0;
        HIP_RET(hipMemcpyAsync(host.data() + from, d_dst + from,
                               (3 * N - from) * 8, hipMemcpyDeviceToHost, s));
        HIP_RET(hipMemcpyAsync(pv->bitmap.data(), d_bm, bm_words * 8,
                               hipMemcpyDeviceToHost, s));
        HIP_RET(hipMemcpyAsync(pv->n_valid.data(), d_nv, n_groups * 4,
                               hipMemcpyDeviceToHost, s));
        HIP_RET(hipMemcpyAsync(&errs, d_err, 8, hipMemcpyDeviceToHost, s));
        HIP_RET(hipStreamSynchronize(s));
        if (errs) return hipErrorUnknown;   // a sort permutation out of range
        std::memcpy(pv->packed.data(), host.data() + 2 * N, N * 8);
    } else {
        HIP_RET(hx::launch_gather_multi(s, srcs, 3, pc, d_dst, (uint32_t)N));
        if (!streams) {   // with streams the three columns stay on the device
            HIP_RET(hipMemcpyAsync(host.data(), d_dst, 3 * N * 8,
                                   hipMemcpyDeviceToHost, s));
            HIP_RET(hipStreamSynchronize(s));
            std::memcpy(v2.data(), host.data() + 2 * N, N * 8);
        }
    }
    if (streams) {
        // the OPTIONAL value page opens with its level block: host twin
        const int64_t col_words[5] = {0, (int64_t)N, pv ? -1 : 2 * (int64_t)N,
                                      -1, -1};
        HIP_RET(compress_columns_device(s, (const uint8_t*)d_dst, col_words,
                                        (uint32_t)N, nullptr, *streams));
    }
    if (!streams) {
        std::memcpy(s2.data(), host.data(), N * 8);
        std::memcpy(t2.data(), host.data() + N, N * 8);
    }
    return hipSuccess;
}

// hx_write and hx_write_nullable. validity: LSB-first bitmap over the batch
// rows, NULL = all present; under writer setting 0 the caller has already
// refused a batch with a null, and the file is the REQUIRED one.
static hx_status write_batch(hx_handle* h, const uint64_t* series,
                             const int64_t* ts, const double* value,
                             const uint8_t* validity, int64_t n,
                             int32_t enable_check, uint64_t* out_seq) {
    // ColumnarStorage::write (storage.rs:76-89, :307-333): sort the batch by
    // primary key (sort_batch, storage.rs:244-256 — GPU radix sort when a
    // device is visible, the reference's CPU SortExec otherwise is NOT
    // mirrored: ingest prep stays a host-side stable sort in that case),
    // allocate the file id (= sequence, sst.rs:39-46), write one SST,
    // add it to the catalog (manifest add_file, manifest/mod.rs:115-157).
    if (!h || !series || !ts || !value || n <= 0 || !out_seq)
        return fail(HX_ERR_INVALID, "bad argument");
    *out_seq = 0;
    // an f64 SST in a Binary store would make the next hx_open refuse it
    if (h->bytes_value)
        return fail(HX_ERR_UNSUPPORTED,
                    "the store's value column is Binary: write it with "
                    "hx_write_bytes");
    if (h->bytes_write_codec)
        return fail(HX_ERR_UNSUPPORTED,
                    "a bytes write codec is set (hx_set_bytes_write_codec): "
                    "the handle writes a Binary value column");
    if (enable_check) {
        hx_status st = check_segment(h, ts, n);
        if (st != HX_OK) return st;
    }
    // stable sort by (series, ts). Large batches sort on the GPU (rocPRIM LSD radix, stable): the
    // ingest-side analog of sort_batch's SortExec (storage.rs:244-256) —
    // SURVEY §8(f) row 3's sort half. Small batches (or no device) stay
    // on the host.
    std::vector<uint64_t> s2(n);
    std::vector<int64_t> t2(n);
    std::vector<double> v2(n);
    // nullable writer: validity follows its row through the sort, and the
    // values are packed per row group by the sort permutation (kernel 1d on
    // the device path, its host twin here)
    const bool nullable = h->nullable_values != 0;
    PackedValues pv;
    const int32_t codec = h->write_codec;
    DeviceStreams streams;   // codec Snappy on the device route, else empty:
                             // the writer compresses with the host twin
    bool sorted_on_gpu = false;
    if (n >= (1 << 16) && hip_device_count() > 0) {
        sorted_on_gpu =
            gpu_sort_batch(series, ts, value, n, s2, t2, v2, validity,
                           nullable ? &pv : nullptr,
                           codec ? &streams : nullptr) == hipSuccess;
        if (!sorted_on_gpu) streams = DeviceStreams();
    }
    if (!sorted_on_gpu) {
        const std::vector<uint32_t> order = host_pk_order(series, ts, n);
        for (int64_t i = 0; i < n; i++) {
            s2[i] = series[order[i]];
            t2[i] = ts[order[i]];
            v2[i] = value[order[i]];
        }
        if (nullable)
            pv.pack_host(value, validity, order.data(), n, kRowGroup);
    }
    const NewSst out = next_sst(h);
    const hx::PagePayload* ready =
        streams.ready.empty() ? nullptr : streams.ready.data();
    // a column kernel 1e compressed never came to the host: its pages and
    // statistics are in `ready`
    const uint64_t* w_series = streams.on_device[0] ? nullptr : s2.data();
    const int64_t* w_ts = streams.on_device[1] ? nullptr : t2.data();
    const double* w_value = streams.on_device[2] ? nullptr : v2.data();
    std::string werr =
        nullable ? hx::write_metric_sst_nullable(out.path, w_series, w_ts,
                                                 pv.view(), nullptr, out.seq,
                                                 n, kRowGroup, codec, ready)
                 : hx::write_metric_sst(out.path, w_series, w_ts, w_value,
                                        out.seq, n, kRowGroup, codec, ready);
    if (!werr.empty()) return fail(HX_ERR_IO, werr);
    hx_status st = catalog_add(h, out);
    if (st != HX_OK) return st;
    *out_seq = out.seq;
    return HX_OK;
}

extern "C" hx_status hx_write(hx_handle* h, const uint64_t* series,
                              const int64_t* ts, const double* value,
                              int64_t n, int32_t enable_check,
                              uint64_t* out_seq) {
    return write_batch(h, series, ts, value, nullptr, n, enable_check,
                       out_seq);
}

extern "C" hx_status hx_write_nullable(hx_handle* h, const uint64_t* series,
                                       const int64_t* ts, const double* value,
                                       const uint8_t* validity, int64_t n,
                                       int32_t enable_check,
                                       uint64_t* out_seq) {
    if (h && out_seq && n > 0 && validity && !h->nullable_values &&
        !h->bytes_value) {   // a Binary store is refused by write_batch
        if (count_nulls(validity, n) > 0) {
            *out_seq = 0;
            return fail(HX_ERR_UNSUPPORTED,
                        "batch holds null values and the handle writes "
                        "REQUIRED columns (hx_set_nullable_values)");
        }
        validity = nullptr;   // all present: the file hx_write writes
    }
    return write_batch(h, series, ts, value, validity, n, enable_check,
                       out_seq);
}

// ---------------------------------------------------------------------------
// Binary value stores (BytesMergeOperator / UpdateMode::Append schema): the
// write side. Values travel as handles (off << 20 | len, k_ba_offsets'
// format) and kernel 1f (or its host twin, ba_pages.h) turns them into the
// PLAIN BYTE_ARRAY page images write_metric_sst_bytes takes ready-made.
// ---------------------------------------------------------------------------
namespace {

const char kBaLimit[] =
    "2^20 - 1 bytes (a value handle has 20 length bits)";

// The one refusal of a row group's value image above Parquet's i32 page sizes
// (and BaPageDesc::src_len; with or without a page limit, read_chunk needs
// it too): page_off has n_pages + 1 entries.
hx_status check_page_sizes(const uint64_t* page_off, uint64_t n_pages) {
    for (uint64_t g = 0; g < n_pages; g++)
        if (page_off[g + 1] - page_off[g] > hx::BA_MAX_PAGE_BYTES)
            return fail(HX_ERR_UNSUPPORTED,
                        "row group " + std::to_string(g) + ": the value "
                        "image would exceed INT32_MAX bytes (a page limit "
                        "cuts the image, it does not lift this bound)");
    return HX_OK;
}

// argument check shared by hx_debug_ba_pages and hx_debug_ba_pages_host
bool ba_debug_args_ok(const uint8_t* src, uint64_t src_size,
                      const uint64_t* handles, uint32_t n_src,
                      uint32_t row_group, const uint64_t* page_off,
                      const uint64_t* n_errors, const uint64_t* n_over_cap) {
    return page_off && n_errors && n_over_cap && row_group != 0 &&
           row_group <= hx::BA_MAX_ROW_GROUP && (!n_src || handles) &&
           (!src_size || src);
}

// The size pass of kernel 1f with its device buffers, and what the caller
// must refuse before anything is written: rows the kernel refused, Append
// groups above the value limit, page images above Parquet's i32 sizes.
struct BaPageBuilder {
    DevBufs dev;
    uint32_t* d_row_len = nullptr;
    unsigned long long* d_words = nullptr;   // page_off[n_pages + 1],
                                             // counts[2], batch_sum[n_batches],
                                             // page_size[n_pages]
    uint32_t n_pages = 0;                    // row groups (one image each)
    uint32_t n_batches = 0;                  // 0 without a page limit
    std::vector<uint64_t> page_off;          // n_pages + 1, counts and the
                                             // batch sums behind
    uint64_t n_errors = 0, n_over_cap = 0;

    const uint64_t* batch_sum() const {
        return n_batches ? page_off.data() + n_pages + 3 : nullptr;
    }

    uint64_t total() const { return page_off[n_pages]; }

    // launches, one small D2H, no verdict yet. With a page limit kernel 1h
    // adds the 1024-row batch sums, which ride home in the same copy.
    hx_status run(hipStream_t s, uint64_t src_size, const uint64_t* d_handles,
                  const uint32_t* d_group_start, uint32_t n_src,
                  uint32_t n_out, uint32_t row_group,
                  uint32_t page_limit = 0) {
        n_pages = (uint32_t)hx::ba_n_pages(n_out, row_group);
        n_batches =
            page_limit ? (uint32_t)hx::ba_n_batches(n_out, row_group) : 0;
        const size_t head = size_t(n_pages) + 3 + n_batches;
        HIP_TRY(dev.alloc((void**)&d_row_len, size_t(n_out) * 4));
        HIP_TRY(dev.alloc((void**)&d_words, (head + size_t(n_pages)) * 8));
        unsigned long long* d_counts = d_words + n_pages + 1;
        HIP_TRY(hipMemsetAsync(d_counts, 0, 16, s));
        HIP_TRY(hx::launch_ba_page_sizes(s, src_size, d_handles,
                                         d_group_start, n_src, n_out,
                                         row_group, d_row_len, d_words + head,
                                         d_words, d_counts));
        if (n_batches)
            HIP_TRY(hx::launch_ba_batch_sizes(s, d_row_len, n_out, row_group,
                                              d_counts + 2));
        page_off.resize(head);
        HIP_TRY(hipMemcpyAsync(page_off.data(), d_words, head * 8,
                               hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        n_errors = page_off[n_pages + 1];
        n_over_cap = page_off[n_pages + 2];
        return HX_OK;
    }

    hx_status verdict() const {
        if (n_errors)
            return fail(HX_ERR_FORMAT,
                        "byte pages: a value handle does not fit its source "
                        "or the group bounds are out of order");
        if (n_over_cap)
            return fail(HX_ERR_UNSUPPORTED,
                        std::string("an Append group's concatenated value "
                                    "exceeds ") + kBaLimit);
        return check_page_sizes(page_off.data(), n_pages);
    }
};

// The data pages of a value column: row group g holds pages [first[g],
// first[g + 1]), each with its rows and uncompressed bytes. Without a limit
// every row group is one page; with one, hx::ba_cut_pages over the batch sums
// (kernel 1h's or hx::ba_batch_sizes_host's) says where the pages end.
struct BaCuts {
    std::vector<uint32_t> first, rows, ulen;
    uint32_t n() const { return (uint32_t)rows.size(); }
};

BaCuts ba_cuts(const uint64_t* batch_sum, const uint64_t* page_off,
               uint32_t n_rg, uint64_t n_out, uint32_t limit) {
    BaCuts c;
    c.first.assign(1, 0);
    const uint64_t per = hx::ba_batches_per_group(kRowGroup);
    std::vector<uint32_t> pr(per ? per : 1);
    std::vector<uint64_t> pb(per ? per : 1);
    for (uint32_t g = 0; g < n_rg; g++) {
        const uint64_t rows =
            std::min<uint64_t>(kRowGroup, n_out - uint64_t(g) * kRowGroup);
        if (limit && batch_sum) {
            const uint32_t k = hx::ba_cut_pages(batch_sum + g * per, rows,
                                                limit, pr.data(), pb.data());
            for (uint32_t i = 0; i < k; i++) {
                c.rows.push_back(pr[i]);
                c.ulen.push_back(uint32_t(pb[i]));
            }
        } else {
            c.rows.push_back(uint32_t(rows));
            c.ulen.push_back(uint32_t(page_off[g + 1] - page_off[g]));
        }
        c.first.push_back(c.n());
    }
    return c;
}

// The pages of every row group must add up to its image, byte for byte,
// before a device pass slices the image by them.
hx_status check_cuts(const BaCuts& c, const uint64_t* page_off,
                     uint32_t n_rg) {
    for (uint32_t g = 0; g < n_rg; g++) {
        uint64_t sum = 0;
        for (uint32_t p = c.first[g]; p < c.first[g + 1]; p++)
            sum += c.ulen[p];
        if (sum != page_off[g + 1] - page_off[g])
            return fail(HX_ERR_HIP, "byte pages: the batch sums do not add "
                                    "up to the row group's image");
    }
    return HX_OK;
}

// a ready entry's cuts (none for a row group of one page: the entry it
// always was)
void ba_ready_split(hx::PagePayload& r, const BaCuts& cuts, uint32_t g) {
    const uint32_t k = cuts.first[g + 1] - cuts.first[g];
    if (k <= 1) return;
    r.n_split = k;
    r.split_rows = cuts.rows.data() + cuts.first[g];
    r.split_ulen = cuts.ulen.data() + cuts.first[g];
}

// ready table of the 5-column metric layout: the value column's page images
std::vector<hx::PagePayload> ba_ready(const uint64_t* page_off,
                                      uint32_t n_pages,
                                      const uint8_t* image,
                                      const BaCuts& cuts) {
    std::vector<hx::PagePayload> r(size_t(n_pages) * 5, hx::PagePayload{});
    for (uint32_t g = 0; g < n_pages; g++) {
        r[size_t(g) * 5 + 2].ptr = image + page_off[g];
        r[size_t(g) * 5 + 2].len = uint32_t(page_off[g + 1] - page_off[g]);
        ba_ready_split(r[size_t(g) * 5 + 2], cuts, g);
    }
    return r;
}

// Snappy streams and footer statistics of a value column's page images, as
// the writer takes them under codec Snappy (PagePayload: stream, ulen,
// ba_stat), whoever made them.
struct BaStreams {
    std::vector<uint8_t> bytes;          // the streams, back to back
    std::vector<uint32_t> lens;          // per data page (BaCuts order)
    std::vector<hx::BaPageStat> stats;   // per row group
    size_t d2h_bytes = 0;                // device route: what came back
    float stats_ms = 0, compress_ms = 0; // device route under HX_DEBUG
};

// the host route: hx::ba_page_minmax_host and hx::snappy_compress_host
void ba_streams_host(const uint8_t* image, const uint64_t* page_off,
                     uint32_t n_pages, const uint32_t* row_len,
                     uint64_t n_out, const BaCuts& cuts, BaStreams& out) {
    out.stats.resize(n_pages);
    out.lens.resize(cuts.n());
    hx::ba_page_minmax_host(image, page_off, row_len, n_out, kRowGroup,
                            out.stats.data());
    out.bytes.clear();
    for (uint32_t g = 0; g < n_pages; g++) {
        size_t src = size_t(page_off[g]);
        for (uint32_t p = cuts.first[g]; p < cuts.first[g + 1]; p++) {
            const size_t n = cuts.ulen[p];
            const size_t at = out.bytes.size();
            out.bytes.resize(at + size_t(hx::snappy_max_compressed(n)));
            const size_t got = hx::snappy_compress_host(
                image + src, n, out.bytes.data() + at, out.bytes.size() - at);
            out.lens[p] = uint32_t(got);
            out.bytes.resize(at + got);
            src += n;
        }
    }
}

// the value column's entries of a ready table (n_pages * 5 entries)
void ba_ready_streams(std::vector<hx::PagePayload>& ready,
                      const uint64_t* page_off, uint32_t n_pages,
                      const BaCuts& cuts, const BaStreams& st) {
    ready.resize(size_t(n_pages) * 5, hx::PagePayload{});
    size_t at = 0;
    for (uint32_t g = 0; g < n_pages; g++) {
        hx::PagePayload& r = ready[size_t(g) * 5 + 2];
        r = hx::PagePayload{};
        r.ptr = st.bytes.data() + at;
        uint32_t len = 0;
        for (uint32_t p = cuts.first[g]; p < cuts.first[g + 1]; p++)
            len += st.lens[p];
        r.len = len;
        r.ulen = uint32_t(page_off[g + 1] - page_off[g]);
        r.ba_stat = &st.stats[g];
        ba_ready_split(r, cuts, g);
        if (r.n_split) r.split_len = st.lens.data() + cuts.first[g];
        at += len;
    }
}

// The device route: kernel 1g over the image kernel 1f left in HBM (per row
// group), kernel 1e with one SnappyCompDesc per DATA PAGE (cuts: consecutive
// slices of each row group's image; slots at Snappy's bound; n and dst_cap
// are u32, which a page of at most INT32_MAX bytes fits), the
// scan-and-pack pass, then lengths + statistics and ONE contiguous copy of
// the streams. d_page_off / d_row_len as the size pass left them; page_off
// its host copy (every page already checked against BA_MAX_PAGE_BYTES).
hipError_t compress_ba_pages_device(hipStream_t s, const uint8_t* d_image,
                                    const uint64_t* page_off,
                                    uint32_t n_pages,
                                    const unsigned long long* d_page_off,
                                    const uint32_t* d_row_len, uint32_t n_out,
                                    const BaCuts& cuts, bool timed,
                                    BaStreams& out) {
    const uint32_t n_descs = cuts.n();
    std::vector<hx::SnappyCompDesc> descs(n_descs);
    size_t slot_bytes = 0;
    for (uint32_t g = 0; g < n_pages; g++) {
        uint64_t src = page_off[g];
        for (uint32_t p = cuts.first[g]; p < cuts.first[g + 1]; p++) {
            hx::SnappyCompDesc& d = descs[p];
            d.src_off = src;
            d.n = cuts.ulen[p];
            d.dst_cap = uint32_t(hx::snappy_max_compressed(d.n));
            d.dst_off = slot_bytes;
            slot_bytes = align64(slot_bytes + d.dst_cap);
            src += d.n;
        }
    }
    out.bytes.clear();
    out.lens.assign(n_descs, 0);
    out.stats.assign(n_pages, hx::BaPageStat{});
    out.d2h_bytes = 0;
    if (n_pages == 0) return hipSuccess;
    const size_t desc_bytes = align64(size_t(n_descs) * sizeof(descs[0]));
    const size_t off_bytes = align64(size_t(n_descs) * 8);
    // read back first, in one copy: lengths, error count, statistics
    const size_t len_bytes = (size_t(n_descs) * 4 + 7) & ~size_t(7);
    const size_t stat_bytes = size_t(n_pages) * sizeof(hx::BaPageStat);
    const size_t back_bytes = len_bytes + 8 + stat_bytes;
    uint8_t* dev = nullptr;
    DevBufs bufs;
    HIP_RET(bufs.alloc((void**)&dev, 2 * slot_bytes + desc_bytes + off_bytes +
                                         back_bytes));
    HipEvents<3> ev;
    uint8_t* d_slots = dev;
    uint8_t* d_packed = dev + slot_bytes;
    auto* d_descs = (hx::SnappyCompDesc*)(d_packed + slot_bytes);
    auto* d_offs = (unsigned long long*)((uint8_t*)d_descs + desc_bytes);
    uint32_t* d_lens = (uint32_t*)((uint8_t*)d_offs + off_bytes);
    unsigned long long* d_err =
        (unsigned long long*)((uint8_t*)d_lens + len_bytes);
    hx::BaPageStat* d_stats = (hx::BaPageStat*)(d_err + 1);
    if (timed) HIP_RET(ev.create());
    HIP_RET(hipMemcpyAsync(d_descs, descs.data(),
                           size_t(n_descs) * sizeof(descs[0]),
                           hipMemcpyHostToDevice, s));
    HIP_RET(hipMemsetAsync(d_err, 0, 8, s));
    if (timed) HIP_RET(hipEventRecord(ev[0], s));
    HIP_RET(hx::launch_ba_page_minmax(s, d_image, d_page_off, d_row_len, n_out,
                                      (uint32_t)kRowGroup, d_stats));
    if (timed) HIP_RET(hipEventRecord(ev[1], s));
    HIP_RET(hx::launch_snappy_compress(s, d_image, d_slots, d_descs, n_descs,
                                       d_lens, d_err));
    HIP_RET(hx::launch_snappy_pack(s, d_slots, d_descs, n_descs, d_lens,
                                   d_offs, d_packed));
    if (timed) HIP_RET(hipEventRecord(ev[2], s));
    std::vector<uint64_t> back((back_bytes + 7) / 8);
    HIP_RET(hipMemcpyAsync(back.data(), d_lens, back_bytes,
                           hipMemcpyDeviceToHost, s));
    HIP_RET(hipStreamSynchronize(s));
    if (back[len_bytes / 8] != 0) return hipErrorUnknown;
    std::memcpy(out.lens.data(), back.data(), size_t(n_descs) * 4);
    std::memcpy(out.stats.data(), (const uint8_t*)back.data() + len_bytes + 8,
                stat_bytes);
    size_t total = 0;
    for (uint32_t p = 0; p < n_descs; p++) total += out.lens[p];
    out.bytes.resize(total);
    HIP_RET(hipMemcpyAsync(out.bytes.data(), d_packed, total,
                           hipMemcpyDeviceToHost, s));
    HIP_RET(hipStreamSynchronize(s));
    if (timed) {
        HIP_RET(hipEventElapsedTime(&out.stats_ms, ev[0], ev[1]));
        HIP_RET(hipEventElapsedTime(&out.compress_ms, ev[1], ev[2]));
    }
    out.d2h_bytes = back_bytes + total;
    return hipSuccess;
}

// (bytes, offsets) batches of hx_write_bytes / hx_write_sst_bytes
hx_status check_value_offsets(const int64_t* offsets, int64_t n) {
    if (offsets[0] < 0) return fail(HX_ERR_INVALID, "negative offset");
    for (int64_t i = 0; i < n; i++) {
        const int64_t l = offsets[i + 1] - offsets[i];
        if (l < 0) return fail(HX_ERR_INVALID, "offsets decrease");
        if (l > (int64_t)hx::BA_MAX_VALUE_LEN)
            return fail(HX_ERR_INVALID,
                        "row " + std::to_string(i) + ": value of " +
                            std::to_string(l) + " bytes; the limit is " +
                            kBaLimit);
        if (uint64_t(offsets[i]) >= (1ull << 44))
            return fail(HX_ERR_INVALID, "batch above 2^44 value bytes");
    }
    return HX_OK;
}

}  // namespace

extern "C" hx_status hx_write_sst_bytes(const char* path,
                                        const uint64_t* series,
                                        const int64_t* ts,
                                        const uint8_t* bytes,
                                        const int64_t* offsets,
                                        const uint64_t* seqs, uint64_t seq,
                                        int64_t n_rows, int64_t row_group) {
    return hx_write_sst_bytes_codec(path, series, ts, bytes, offsets, seqs,
                                    seq, n_rows, row_group, HX_CODEC_NONE);
}

extern "C" hx_status hx_write_sst_bytes_codec(
    const char* path, const uint64_t* series, const int64_t* ts,
    const uint8_t* bytes, const int64_t* offsets, const uint64_t* seqs,
    uint64_t seq, int64_t n_rows, int64_t row_group, int32_t codec) {
    return hx_write_sst_bytes_paged(path, series, ts, bytes, offsets, seqs,
                                    seq, n_rows, row_group, codec, 0);
}

extern "C" hx_status hx_write_sst_bytes_paged(
    const char* path, const uint64_t* series, const int64_t* ts,
    const uint8_t* bytes, const int64_t* offsets, const uint64_t* seqs,
    uint64_t seq, int64_t n_rows, int64_t row_group, int32_t codec,
    uint32_t page_limit) {
    if (!path || !series || !ts || !offsets || n_rows <= 0 || row_group <= 0)
        return fail(HX_ERR_INVALID, "bad argument");
    if (page_limit > hx::BA_PAGE_LIMIT_MAX)
        return fail(HX_ERR_INVALID,
                    "bytes page limit: 0 (one page per chunk) or 1 .. 2^30");
    if (codec != HX_CODEC_NONE && codec != HX_CODEC_SNAPPY)
        return fail(HX_ERR_INVALID, "write codec: 0 none / 1 snappy");
    hx_status st = check_value_offsets(offsets, n_rows);
    if (st != HX_OK) return st;
    if (!bytes && offsets[n_rows] != offsets[0])
        return fail(HX_ERR_INVALID, "bad argument");
    // from the offsets alone, before a value byte is read
    std::vector<uint64_t> page_off(1, 0);
    for (int64_t base = 0; base < n_rows; base += row_group) {
        const int64_t rows = std::min<int64_t>(row_group, n_rows - base);
        page_off.push_back(page_off.back() + 4ull * rows +
                           uint64_t(offsets[base + rows] - offsets[base]));
    }
    st = check_page_sizes(page_off.data(), page_off.size() - 1);
    if (st != HX_OK) return st;
    // the writer builds each page image from (bytes, offsets), the bytes
    // hx::ba_build_pages_host gives, cuts it by hx::ba_cut_pages under a
    // limit, and under Snappy compresses each page with
    // hx::snappy_compress_host
    std::string err = hx::write_metric_sst_bytes(path, series, ts, bytes,
                                                 offsets, seqs, seq, n_rows,
                                                 row_group, nullptr, codec,
                                                 page_limit);
    if (!err.empty()) return fail(HX_ERR_IO, err);
    return HX_OK;
}

extern "C" hx_status hx_debug_ba_pages_host(
    const uint8_t* src, uint64_t src_size, const uint64_t* handles,
    uint32_t n_src, const uint32_t* group_start, uint32_t n_out,
    uint32_t row_group, uint64_t* page_off, uint8_t* out, uint64_t out_cap,
    uint64_t* n_errors, uint64_t* n_over_cap) {
    if (!ba_debug_args_ok(src, src_size, handles, n_src, row_group, page_off,
                          n_errors, n_over_cap))
        return fail(HX_ERR_INVALID, "bad argument");
    std::vector<uint32_t> row_len(n_out);
    hx::BaPagesCounts c = hx::ba_page_sizes_host(
        src_size, handles, n_src, group_start, n_out, row_group,
        row_len.data(), page_off);
    *n_errors = c.n_errors;
    *n_over_cap = c.n_over_cap;
    const uint64_t total = page_off[hx::ba_n_pages(n_out, row_group)];
    if (!out) return HX_OK;
    if (out_cap != total)
        return fail(HX_ERR_INVALID, "out_cap is not the image size");
    hx::ba_build_pages_host(src, src_size, handles, n_src, group_start, n_out,
                            row_group, row_len.data(), page_off, out);
    return HX_OK;
}

extern "C" hx_status hx_debug_ba_pages(
    const uint8_t* src, uint64_t src_size, const uint64_t* handles,
    uint32_t n_src, const uint32_t* group_start, uint32_t n_out,
    uint32_t row_group, uint64_t* page_off, uint8_t* out, uint64_t out_cap,
    uint64_t* n_errors, uint64_t* n_over_cap) {
    if (!ba_debug_args_ok(src, src_size, handles, n_src, row_group, page_off,
                          n_errors, n_over_cap))
        return fail(HX_ERR_INVALID, "bad argument");
    // every buffer exactly as large as the contract says it is
    DevBufs dev;
    uint8_t* d_src = nullptr;
    uint64_t* d_handles = nullptr;
    uint32_t* d_gs = nullptr;
    uint8_t* d_out = nullptr;
    HIP_TRY(dev.alloc((void**)&d_src, src_size));
    HIP_TRY(dev.alloc((void**)&d_handles, size_t(n_src) * 8));
    if (src_size)
        HIP_TRY(hipMemcpy(d_src, src, src_size, hipMemcpyHostToDevice));
    if (n_src)
        HIP_TRY(hipMemcpy(d_handles, handles, size_t(n_src) * 8,
                          hipMemcpyHostToDevice));
    if (group_start) {
        HIP_TRY(dev.alloc((void**)&d_gs, (size_t(n_out) + 1) * 4));
        HIP_TRY(hipMemcpy(d_gs, group_start, (size_t(n_out) + 1) * 4,
                          hipMemcpyHostToDevice));
    }
    BaPageBuilder b;
    hx_status st = b.run(nullptr, src_size, d_handles, d_gs, n_src, n_out,
                         row_group);
    if (st != HX_OK) return st;
    std::memcpy(page_off, b.page_off.data(), (size_t(b.n_pages) + 1) * 8);
    *n_errors = b.n_errors;
    *n_over_cap = b.n_over_cap;
    if (!out) return HX_OK;
    if (out_cap != b.total())
        return fail(HX_ERR_INVALID, "out_cap is not the image size");
    HIP_TRY(dev.alloc((void**)&d_out, b.total()));
    if (b.total()) HIP_TRY(hipMemset(d_out, 0xEE, b.total()));
    HIP_TRY(hx::launch_ba_build_pages(nullptr, d_src, src_size, d_handles,
                                      d_gs, n_src, n_out, row_group,
                                      b.d_row_len, b.d_words, d_out));
    HIP_TRY(hipDeviceSynchronize());
    if (b.total())
        HIP_TRY(hipMemcpy(out, d_out, b.total(), hipMemcpyDeviceToHost));
    return HX_OK;
}

// Kernel 1h and its twin over caller-built row_len: batch_sum gets
// hx::ba_n_batches(n_out, row_group) words.
static bool ba_batch_args_ok(const uint32_t* row_len, uint32_t n_out,
                             uint32_t row_group, const uint64_t* batch_sum) {
    return row_group != 0 && row_group <= hx::BA_MAX_ROW_GROUP &&
           (!n_out || (row_len && batch_sum));
}

extern "C" hx_status hx_debug_ba_batch_sizes_host(const uint32_t* row_len,
                                                  uint32_t n_out,
                                                  uint32_t row_group,
                                                  uint64_t* batch_sum) {
    if (!ba_batch_args_ok(row_len, n_out, row_group, batch_sum))
        return fail(HX_ERR_INVALID, "bad argument");
    hx::ba_batch_sizes_host(row_len, n_out, row_group, batch_sum);
    return HX_OK;
}

extern "C" hx_status hx_debug_ba_batch_sizes(const uint32_t* row_len,
                                             uint32_t n_out,
                                             uint32_t row_group,
                                             uint64_t* batch_sum) {
    if (!ba_batch_args_ok(row_len, n_out, row_group, batch_sum))
        return fail(HX_ERR_INVALID, "bad argument");
    const size_t n_b = hx::ba_n_batches(n_out, row_group);
    if (n_b == 0) return HX_OK;
    // every buffer exactly as large as the contract says it is
    DevBufs dev;
    uint32_t* d_len = nullptr;
    unsigned long long* d_sum = nullptr;
    HIP_TRY(dev.alloc((void**)&d_len, size_t(n_out) * 4));
    HIP_TRY(dev.alloc((void**)&d_sum, n_b * 8));
    HIP_TRY(hipMemcpy(d_len, row_len, size_t(n_out) * 4,
                      hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(d_sum, 0xEE, n_b * 8));
    HIP_TRY(hx::launch_ba_batch_sizes(nullptr, d_len, n_out, row_group,
                                      d_sum));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(batch_sum, d_sum, n_b * 8, hipMemcpyDeviceToHost));
    return HX_OK;
}

// argument check shared by hx_debug_ba_page_minmax and its host form
static bool ba_minmax_args_ok(const uint8_t* image, const uint64_t* page_off,
                              const uint32_t* row_len, uint32_t n_out,
                              uint32_t row_group, const uint8_t* stats_out) {
    if (!page_off || !row_len || !stats_out || n_out == 0 ||
        row_group == 0 || row_group > hx::BA_MAX_ROW_GROUP ||
        page_off[0] != 0)
        return false;
    const uint64_t n_pages = hx::ba_n_pages(n_out, row_group);
    for (uint64_t g = 0; g < n_pages; g++) {
        uint64_t sum = 0;
        const uint64_t r1 = std::min<uint64_t>((g + 1) * row_group, n_out);
        for (uint64_t i = g * row_group; i < r1; i++)
            sum += 4ull + ((row_len[i] & hx::BA_ROW_SKIP) ? 0u : row_len[i]);
        if (page_off[g + 1] < page_off[g] ||
            page_off[g + 1] - page_off[g] != sum ||
            sum > hx::BA_MAX_PAGE_BYTES)
            return false;
    }
    return image != nullptr;
}

extern "C" hx_status hx_debug_ba_page_minmax_host(
    const uint8_t* image, const uint64_t* page_off, const uint32_t* row_len,
    uint32_t n_out, uint32_t row_group, uint8_t* stats_out) {
    if (!ba_minmax_args_ok(image, page_off, row_len, n_out, row_group,
                           stats_out))
        return fail(HX_ERR_INVALID, "bad argument");
    std::vector<hx::BaPageStat> st(hx::ba_n_pages(n_out, row_group));
    hx::ba_page_minmax_host(image, page_off, row_len, n_out, row_group,
                            st.data());
    std::memcpy(stats_out, st.data(), st.size() * sizeof(hx::BaPageStat));
    return HX_OK;
}

extern "C" hx_status hx_debug_ba_page_minmax(
    const uint8_t* image, const uint64_t* page_off, const uint32_t* row_len,
    uint32_t n_out, uint32_t row_group, uint8_t* stats_out) {
    if (!ba_minmax_args_ok(image, page_off, row_len, n_out, row_group,
                           stats_out))
        return fail(HX_ERR_INVALID, "bad argument");
    const size_t n_pages = hx::ba_n_pages(n_out, row_group);
    const size_t total = page_off[n_pages];
    const size_t st_bytes = n_pages * sizeof(hx::BaPageStat);
    DevBufs dev;
    uint8_t* d_image = nullptr;
    unsigned long long* d_off = nullptr;
    uint32_t* d_len = nullptr;
    hx::BaPageStat* d_st = nullptr;
    HIP_TRY(dev.alloc((void**)&d_image, total));
    HIP_TRY(dev.alloc((void**)&d_off, (n_pages + 1) * 8));
    HIP_TRY(dev.alloc((void**)&d_len, size_t(n_out) * 4));
    HIP_TRY(dev.alloc((void**)&d_st, st_bytes));
    HIP_TRY(hipMemcpy(d_image, image, total, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_off, page_off, (n_pages + 1) * 8,
                      hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_len, row_len, size_t(n_out) * 4,
                      hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(d_st, 0xEE, st_bytes));
    HIP_TRY(hx::launch_ba_page_minmax(nullptr, d_image, d_off, d_len, n_out,
                                      row_group, d_st));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(stats_out, d_st, st_bytes, hipMemcpyDeviceToHost));
    return HX_OK;
}

// The device route of hx_write_bytes: the ingest sort's permutation (two
// stable LSD passes, ts then series), the handles gathered by it, kernel 1f
// over the uploaded value bytes, and ONE copy back: sorted series, sorted ts
// and the page images, in that order in `host`. Under codec Snappy (keys and
// values given) nothing of that comes back: kernel 1g and kernel 1e run over
// the image, kernel 1e over the sorted series and ts where the gather left
// them, and the host receives lengths, statistics and streams.
static hx_status gpu_write_bytes(const uint64_t* series, const int64_t* ts,
                                 const uint8_t* bytes, uint64_t n_bytes,
                                 const std::vector<uint64_t>& handles,
                                 int64_t n, std::vector<uint8_t>& host,
                                 std::vector<uint64_t>& page_off,
                                 uint32_t page_limit, BaCuts& cuts,
                                 DeviceStreams* keys = nullptr,
                                 BaStreams* values = nullptr) {
    hipStream_t s = nullptr;
    const size_t N = (size_t)n;
    DevBufs dev;
    SortTemp temp;
    uint64_t *d_series, *d_ts, *d_h, *d_ka, *d_kb, *d_hs;
    uint32_t *pa, *pb, *pc;
    uint8_t *d_bytes, *d_final;
    HIP_TRY(dev.alloc((void**)&d_series, N * 8));
    HIP_TRY(dev.alloc((void**)&d_ts, N * 8));
    HIP_TRY(dev.alloc((void**)&d_h, N * 8));
    HIP_TRY(dev.alloc((void**)&d_ka, N * 8));
    HIP_TRY(dev.alloc((void**)&d_kb, N * 8));
    HIP_TRY(dev.alloc((void**)&d_hs, N * 8));
    HIP_TRY(dev.alloc((void**)&pa, N * 4));
    HIP_TRY(dev.alloc((void**)&pb, N * 4));
    HIP_TRY(dev.alloc((void**)&pc, N * 4));
    HIP_TRY(dev.alloc((void**)&d_bytes, n_bytes));
    HIP_TRY(hipMemcpyAsync(d_series, series, N * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d_ts, ts, N * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d_h, handles.data(), N * 8, hipMemcpyHostToDevice,
                           s));
    if (n_bytes)
        HIP_TRY(hipMemcpyAsync(d_bytes, bytes, n_bytes, hipMemcpyHostToDevice,
                               s));
    HIP_TRY(ingest_sort_perm(s, d_series, (const int64_t*)d_ts, d_ka, d_kb,
                             pa, pb, pc, N, &temp.p, &temp.cap));
    HIP_TRY(hx::launch_gather_u64(s, (const unsigned long long*)d_h, pc,
                                  (unsigned long long*)d_hs, (uint32_t)N));
    BaPageBuilder b;
    hx_status st = b.run(s, n_bytes, d_hs, nullptr, (uint32_t)N, (uint32_t)N,
                         (uint32_t)kRowGroup, page_limit);
    if (st == HX_OK) st = b.verdict();
    if (st != HX_OK) return st;
    cuts = ba_cuts(b.batch_sum(), b.page_off.data(), b.n_pages, N,
                   page_limit);
    st = check_cuts(cuts, b.page_off.data(), b.n_pages);
    if (st != HX_OK) return st;
    const size_t key_bytes = 2 * N * 8;
    HIP_TRY(dev.alloc((void**)&d_final, key_bytes + b.total()));
    const unsigned long long* srcs[2] = {
        (const unsigned long long*)d_series, (const unsigned long long*)d_ts};
    HIP_TRY(hx::launch_gather_multi(s, srcs, 2, pc,
                                    (unsigned long long*)d_final,
                                    (uint32_t)N));
    HIP_TRY(hx::launch_ba_build_pages(s, d_bytes, n_bytes, d_hs, nullptr,
                                      (uint32_t)N, (uint32_t)N,
                                      (uint32_t)kRowGroup, b.d_row_len,
                                      b.d_words, d_final + key_bytes));
    page_off.assign(b.page_off.begin(), b.page_off.begin() + b.n_pages + 1);
    if (keys && values) {
        HIP_TRY(compress_ba_pages_device(s, d_final + key_bytes,
                                         page_off.data(), b.n_pages,
                                         b.d_words, b.d_row_len, (uint32_t)N,
                                         cuts, false, *values));
        const int64_t col_words[5] = {0, (int64_t)N, -1, -1, -1};
        HIP_TRY(compress_columns_device(s, d_final, col_words, (uint32_t)N,
                                        nullptr, *keys));
        return HX_OK;
    }
    host.resize(key_bytes + b.total());
    HIP_TRY(hipMemcpyAsync(host.data(), d_final, host.size(),
                           hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return HX_OK;
}

extern "C" hx_status hx_write_bytes(hx_handle* h, const uint64_t* series,
                                    const int64_t* ts, const uint8_t* bytes,
                                    const int64_t* offsets, int64_t n,
                                    int32_t enable_check, uint64_t* out_seq) {
    // ColumnarStorage::write (storage.rs:76-89, :307-333) for the Binary
    // schema: segment check, stable PK sort (equal PKs keep batch order — the
    // scan's Append key (seq << 32 | file row) depends on it), file id =
    // sequence, catalog add.
    if (!h || !series || !ts || !offsets || n <= 0 || !out_seq)
        return fail(HX_ERR_INVALID, "bad argument");
    *out_seq = 0;
    if (n > 0xFFFFFFFFll)
        return fail(HX_ERR_UNSUPPORTED, "batches above 2^32 rows");
    if (!h->bytes_value && !h->ssts.empty())
        return fail(HX_ERR_SCHEMA,
                    "hx_write_bytes: the store's value column is f64");
    if (h->nullable_values || h->write_codec)
        return fail(HX_ERR_UNSUPPORTED,
                    "hx_write_bytes: nullable values and write codecs need "
                    "an f64 value column");
    hx_status st = check_value_offsets(offsets, n);
    if (st != HX_OK) return st;
    if (!bytes && offsets[n] != offsets[0])
        return fail(HX_ERR_INVALID, "bad argument");
    if (enable_check) {
        st = check_segment(h, ts, n);
        if (st != HX_OK) return st;
    }
    // handles relative to bytes + offsets[0]
    const uint8_t* src = bytes ? bytes + offsets[0] : nullptr;
    const uint64_t n_bytes = uint64_t(offsets[n] - offsets[0]);
    std::vector<uint64_t> handles(n);
    for (int64_t i = 0; i < n; i++)
        handles[i] = (uint64_t(offsets[i] - offsets[0]) << hx::BA_LEN_BITS) |
                     uint64_t(offsets[i + 1] - offsets[i]);
    std::vector<uint8_t> host;        // sorted series, sorted ts, page images
    std::vector<uint64_t> page_off;
    const size_t N = (size_t)n;
    const int32_t codec = h->bytes_write_codec;
    const uint32_t page_limit = h->bytes_page_limit;
    BaCuts cuts;
    DeviceStreams key_streams;        // codec Snappy, device route
    BaStreams value_streams;          // codec Snappy, either route
    bool on_device = false;
    if (n >= (1 << 16) && hip_device_count() > 0) {
        on_device = codec == HX_CODEC_SNAPPY;
        st = gpu_write_bytes(series, ts, src, n_bytes, handles, n, host,
                             page_off, page_limit, cuts,
                             on_device ? &key_streams : nullptr,
                             on_device ? &value_streams : nullptr);
        if (st != HX_OK) return st;
    } else {
        const std::vector<uint32_t> order = host_pk_order(series, ts, n);
        std::vector<uint64_t> hs(n);
        for (int64_t i = 0; i < n; i++) hs[i] = handles[order[i]];
        const uint64_t n_pages = hx::ba_n_pages(N, kRowGroup);
        std::vector<uint32_t> row_len(n);
        page_off.resize(n_pages + 1);
        hx::ba_page_sizes_host(n_bytes, hs.data(), N, nullptr, N, kRowGroup,
                               row_len.data(), page_off.data());
        st = check_page_sizes(page_off.data(), n_pages);
        if (st != HX_OK) return st;
        std::vector<uint64_t> sums;
        if (page_limit) {
            sums.resize(hx::ba_n_batches(N, kRowGroup));
            hx::ba_batch_sizes_host(row_len.data(), N, kRowGroup,
                                    sums.data());
        }
        cuts = ba_cuts(page_limit ? sums.data() : nullptr, page_off.data(),
                       (uint32_t)n_pages, N, page_limit);
        host.resize(2 * N * 8 + page_off[n_pages]);
        uint64_t* s2 = (uint64_t*)host.data();
        int64_t* t2 = (int64_t*)(host.data() + N * 8);
        for (int64_t i = 0; i < n; i++) {
            s2[i] = series[order[i]];
            t2[i] = ts[order[i]];
        }
        hx::ba_build_pages_host(src, n_bytes, hs.data(), N, nullptr, N,
                                kRowGroup, row_len.data(), page_off.data(),
                                host.data() + 2 * N * 8);
        if (codec == HX_CODEC_SNAPPY)
            ba_streams_host(host.data() + 2 * N * 8, page_off.data(),
                            (uint32_t)n_pages, row_len.data(), N, cuts,
                            value_streams);
    }
    const NewSst out = next_sst(h);
    const uint32_t n_pages32 = (uint32_t)(page_off.size() - 1);
    std::vector<hx::PagePayload> ready;
    if (codec == HX_CODEC_SNAPPY) {
        // the key columns' streams (device route), then the value column's
        if (on_device) ready = key_streams.ready;
        ba_ready_streams(ready, page_off.data(), n_pages32, cuts,
                         value_streams);
    } else {
        ready = ba_ready(page_off.data(), n_pages32, host.data() + 2 * N * 8,
                         cuts);
    }
    std::string werr = hx::write_metric_sst_bytes(
        out.path, on_device ? nullptr : (const uint64_t*)host.data(),
        on_device ? nullptr : (const int64_t*)(host.data() + N * 8), nullptr,
        nullptr, nullptr, out.seq, n, kRowGroup, ready.data(), codec);
    if (!werr.empty()) return fail(HX_ERR_IO, werr);
    st = catalog_add(h, out);
    if (st != HX_OK) return st;
    h->bytes_value = true;
    *out_seq = out.seq;
    return HX_OK;
}

// compact_rows for a Binary value column. The row stream's value words are
// handles into the staged blob. Overwrite: survivors as the f64 path (last
// wins), the winner's handle. Append: the stream keeps every row, equal-PK
// rows in ascending sequence order, exactly as hx_scan sees it; equal-PK runs
// become ONE output row whose value is the concatenation in that order and
// whose sequence (keep_seq) is that of the run's FIRST row (BytesMergeOperator
// takes element 0 of every non-value column, operator.rs:99-102, and under
// keep_builtin __seq__ is one). Kernel 1f builds the page images from the
// blob; value bytes never cross PCIe as rows: one D2H of the output rows' key
// columns and the page images.
static hx_status compact_rows_bytes(hx_handle* h, hx_prepared* P,
                                    const std::vector<char>& in_set,
                                    bool keep_seq, uint64_t* out_new_seq) {
    DevPlan& plan = P->plans[0];
    const bool append = h->update_mode == 1;
    RowStream rs;
    hx_status st =
        sorted_row_stream(h, P, plan, keep_seq, append, "compact", rs);
    if (st != HX_OK) return st;
    const uint32_t n = rs.n;
    if (n == 0) return HX_OK;
    hipStream_t s = plan.stream;
    const uint32_t* perm = rs.perm;

    // sorted rows: series, ts, handle [, seq (Overwrite)]
    DevBufs dev;
    const uint32_t n_sorted = (keep_seq && !append) ? 4 : 3;
    unsigned long long* d_sorted = nullptr;
    HIP_TRY(dev.alloc((void**)&d_sorted, size_t(n_sorted) * n * 8));
    const unsigned long long* srcs[4] = {
        (const unsigned long long*)rs.series, (const unsigned long long*)rs.ts,
        (const unsigned long long*)rs.val, (const unsigned long long*)rs.seq};
    HIP_TRY(hx::launch_gather_multi(s, srcs, n_sorted, perm, d_sorted, n));
    const uint64_t* d_handles = (const uint64_t*)(d_sorted + 2 * size_t(n));

    // output rows' key columns on the device, and the group bounds
    const unsigned long long* k_series = d_sorted;
    const unsigned long long* k_ts = d_sorted + n;
    const unsigned long long* k_seq = keep_seq ? d_sorted + 3 * size_t(n)
                                               : nullptr;
    uint32_t* d_gs = nullptr;
    uint32_t n_out = n;
    if (append) {
        uint32_t *d_flag, *d_rank;
        unsigned long long *d_heads, *d_nout;
        HIP_TRY(dev.alloc((void**)&d_flag, size_t(n) * 4));
        HIP_TRY(dev.alloc((void**)&d_rank, size_t(n) * 4));
        HIP_TRY(dev.alloc((void**)&d_gs, (size_t(n) + 1) * 4));
        HIP_TRY(dev.alloc((void**)&d_heads, 3 * size_t(n) * 8));
        HIP_TRY(dev.alloc((void**)&d_nout, 8));
        HIP_TRY(hx::launch_group_heads(
            s, d_sorted, d_sorted + n,
            keep_seq ? (const unsigned long long*)rs.seq : nullptr, perm, n,
            d_flag, d_rank, d_gs, d_heads, d_heads + n,
            d_heads + 2 * size_t(n), d_nout, &plan.d_sort_temp,
            &plan.sort_temp_cap));
        unsigned long long no = 0;
        HIP_TRY(hipMemcpyAsync(&no, d_nout, 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        if (no == 0 || no > n)
            return fail(HX_ERR_HIP, "compact: group count out of range");
        n_out = (uint32_t)no;
        k_series = d_heads;
        k_ts = d_heads + n;
        k_seq = keep_seq ? d_heads + 2 * size_t(n) : nullptr;
    }

    // HX_DEBUG: one event pair around the page-build launches
    const bool timed = getenv("HX_DEBUG") != nullptr;
    HipEvents<2> ev;
    if (timed) {
        HIP_TRY(ev.create());
        HIP_TRY(hipEventRecord(ev[0], s));
    }
    BaPageBuilder b;
    st = b.run(s, plan.blob_span, d_handles, d_gs, n, n_out,
               (uint32_t)kRowGroup, h->bytes_page_limit);
    if (st == HX_OK) st = b.verdict();
    if (st != HX_OK) return st;   // nothing written, nothing unlinked
    const BaCuts cuts = ba_cuts(b.batch_sum(), b.page_off.data(), b.n_pages,
                                n_out, h->bytes_page_limit);
    st = check_cuts(cuts, b.page_off.data(), b.n_pages);
    if (st != HX_OK) return st;
    const size_t n_keys = keep_seq ? 3 : 2;
    const size_t key_bytes = n_keys * size_t(n_out) * 8;
    uint8_t* d_final = nullptr;
    HIP_TRY(dev.alloc((void**)&d_final, key_bytes + b.total()));
    HIP_TRY(hx::launch_ba_build_pages(s, plan.d_blob, plan.blob_span,
                                      d_handles, d_gs, n, n_out,
                                      (uint32_t)kRowGroup, b.d_row_len,
                                      b.d_words, d_final + key_bytes));
    if (timed) HIP_TRY(hipEventRecord(ev[1], s));
    const unsigned long long* keys[3] = {k_series, k_ts, k_seq};
    for (size_t k = 0; k < n_keys; k++)
        HIP_TRY(hipMemcpyAsync(d_final + k * size_t(n_out) * 8, keys[k],
                               size_t(n_out) * 8, hipMemcpyDeviceToDevice,
                               s));
    const NewSst out = next_sst(h);
    if (h->bytes_write_codec == HX_CODEC_SNAPPY) {
        // the image stays in HBM: statistics (kernel 1g) and streams (kernel
        // 1e) of the value pages, streams and statistics of the key columns;
        // lengths + statistics + one contiguous copy of the streams each
        BaStreams vs;
        DeviceStreams ks;
        HIP_TRY(compress_ba_pages_device(s, d_final + key_bytes,
                                         b.page_off.data(), b.n_pages,
                                         b.d_words, b.d_row_len, n_out, cuts,
                                         timed, vs));
        const int64_t col_words[5] = {
            0, (int64_t)n_out, -1, keep_seq ? 2 * (int64_t)n_out : -1, -1};
        HIP_TRY(compress_columns_device(s, d_final, col_words, n_out, nullptr,
                                        ks));
        if (timed) {
            float pages_ms = 0;
            HIP_TRY(hipEventElapsedTime(&pages_ms, ev[0], ev[1]));
            size_t stream_bytes = vs.bytes.size();
            fprintf(stderr,
                    "[hx] compact_bytes rows=%u out_rows=%u append=%d "
                    "keep_seq=%d pages=%u data_pages=%u codec=snappy "
                    "pages_ms=%.4f "
                    "stats_ms=%.4f compress_ms=%.4f value_stream_bytes=%zu "
                    "image_bytes=%zu decode_ms=%.4f d2h_bytes=%zu\n",
                    n, n_out, int(append), int(keep_seq), b.n_pages, cuts.n(),
                    pages_ms, vs.stats_ms, vs.compress_ms, stream_bytes,
                    size_t(b.total()), plan.decode_ms,
                    vs.d2h_bytes + ks.d2h_bytes +
                        (size_t(b.n_pages) + 3 + b.n_batches) * 8 +
                        (append ? 8 : 0) + 8);
        }
        std::vector<hx::PagePayload> ready = ks.ready;
        ba_ready_streams(ready, b.page_off.data(), b.n_pages, cuts, vs);
        std::string werr = hx::write_metric_sst_bytes(
            out.path, nullptr, nullptr, nullptr, nullptr, nullptr, out.seq,
            n_out, kRowGroup, ready.data(), HX_CODEC_SNAPPY);
        if (!werr.empty()) return fail(HX_ERR_IO, werr);
        return finish_compaction(h, out, in_set, out_new_seq);
    }
    std::vector<uint8_t> host(key_bytes + b.total());
    HIP_TRY(hipMemcpyAsync(host.data(), d_final, host.size(),
                           hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (timed) {
        float pages_ms = 0;
        HIP_TRY(hipEventElapsedTime(&pages_ms, ev[0], ev[1]));
        fprintf(stderr,
                "[hx] compact_bytes rows=%u out_rows=%u append=%d "
                "keep_seq=%d pages=%u pages_ms=%.4f decode_ms=%.4f "
                "d2h_bytes=%zu\n",
                n, n_out, int(append), int(keep_seq), b.n_pages, pages_ms,
                plan.decode_ms,
                host.size() + (size_t(b.n_pages) + 3 + b.n_batches) * 8 +
                    (append ? 8 : 0) + 8);
    }

    std::vector<hx::PagePayload> ready =
        ba_ready(b.page_off.data(), b.n_pages, host.data() + key_bytes, cuts);
    const uint64_t* hk = (const uint64_t*)host.data();
    std::string werr = hx::write_metric_sst_bytes(
        out.path, hk, (const int64_t*)(hk + n_out), nullptr, nullptr,
        keep_seq ? hk + 2 * size_t(n_out) : nullptr, out.seq, n_out,
        kRowGroup, ready.data());
    if (!werr.empty()) return fail(HX_ERR_IO, werr);
    return finish_compaction(h, out, in_set, out_new_seq);
}

// The shared body of hx_compact and hx_compact_files, from the prepared plan
// to the catalog update: the sorted row stream, a gather by its permutation,
// one D2H, the native writer, then add-before-delete. keep_seq: the rows keep
// their own __seq__ (hx_compact_files); otherwise the file carries the fresh
// id. Writer setting 1 (hx_set_nullable_values): null values survive. The
// stream has one validity word per row when the plan staged a null; series,
// ts (and seq) are gathered as before and kernel 1d packs the values per
// output row group by the same permutation, so the host receives packed
// values, bitmaps and counts, never the 8-byte validity words.
static hx_status compact_rows(hx_handle* h, hx_prepared* P,
                              const std::vector<char>& in_set, bool keep_seq,
                              uint64_t* out_new_seq) {
    // Binary value column: the value words are handles, not values
    if (h->bytes_value)
        return compact_rows_bytes(h, P, in_set, keep_seq, out_new_seq);
    DevPlan& plan = P->plans[0];
    const bool nullable = h->nullable_values != 0;
    const int32_t codec = h->write_codec;
    // the REQUIRED writer cannot keep a null: dropping it would be data
    // loss. Refused before anything is written or unlinked.
    if (plan.has_nulls && !nullable)
        return fail(HX_ERR_UNSUPPORTED,
                    "compaction inputs hold null values (the native writer "
                    "writes REQUIRED columns)");
    RowStream rs;
    hx_status st =
        sorted_row_stream(h, P, plan, keep_seq, false, "compact", rs);
    if (st != HX_OK) return st;
    const uint32_t n = rs.n;
    if (n == 0) return HX_OK;
    hipStream_t s = plan.stream;
    const bool nulls = rs.valid != nullptr;
    const uint32_t n_cols = keep_seq ? 4 : 3;
    const uint32_t* perm = rs.perm;

    // gather destination, one D2H: series, ts, value [, seq]; the nullable
    // form has the packed values in the value slot and the bitmaps, counts
    // and the error count behind the columns
    const size_t n_groups = (size_t(n) + kRowGroup - 1) / kRowGroup;
    const size_t bm_words = n_groups * size_t(kRowGroup / 64);
    const size_t nv_words = (n_groups + 1) / 2;   // u32 counts, in 8-byte units
    const size_t words = size_t(n_cols) * n +
                         (nullable ? bm_words + nv_words + 1 : 0);
    // under Snappy without the nullable form nothing comes back raw
    std::vector<uint64_t> host(!codec || nullable ? words : 0);
    unsigned long long* d_dst = nullptr;
    HIP_TRY(hipMalloc((void**)&d_dst, words * 8));
    std::unique_ptr<void, void (*)(void*)> dst_guard(
        d_dst, [](void* q) { (void)hipFree(q); });
    // HX_DEBUG: HIP-event times of the final gather, of kernel 1d and of
    // kernel 1e with its pack pass
    HipEvents<4> ev;
    const bool timed = getenv("HX_DEBUG") != nullptr;
    if (timed) {
        HIP_TRY(ev.create());
        HIP_TRY(hipEventRecord(ev[0], s));
    }
    if (nullable) {
        // slots 0 and 1 by the gather, slot 2 by the pack kernel, slot 3
        // (seq) by a gather of its own
        unsigned long long* d_bm = d_dst + size_t(n_cols) * n;
        unsigned long long* d_nv = d_bm + bm_words;
        unsigned long long* d_err = d_nv + nv_words;
        HIP_TRY(hipMemsetAsync(d_err, 0, 8, s));
        const unsigned long long* srcs[2] = {
            (const unsigned long long*)rs.series,
            (const unsigned long long*)rs.ts};
        HIP_TRY(hx::launch_gather_multi(s, srcs, 2, perm, d_dst, n));
        if (keep_seq)
            HIP_TRY(hx::launch_gather_u64(
                s, (const unsigned long long*)rs.seq, perm,
                d_dst + 3 * size_t(n), n));
        if (timed) HIP_TRY(hipEventRecord(ev[1], s));
        HIP_TRY(hx::launch_pack_optional(
            s, (const unsigned long long*)rs.val, rs.valid, false, perm, n, n,
            (uint32_t)kRowGroup, d_dst + 2 * size_t(n), (uint64_t*)d_bm,
            (uint32_t*)d_nv, d_err));
    } else {
        const unsigned long long* srcs[4] = {
            (const unsigned long long*)rs.series,
            (const unsigned long long*)rs.ts,
            (const unsigned long long*)rs.val,
            (const unsigned long long*)rs.seq};
        HIP_TRY(hx::launch_gather_multi(s, srcs, n_cols, perm, d_dst, n));
        if (timed) HIP_TRY(hipEventRecord(ev[1], s));
    }
    if (timed) HIP_TRY(hipEventRecord(ev[2], s));
    // Writer codec Snappy: kernel 1e over the 8192-row slices of the columns
    // where they sit in d_dst (series, ts, per-row seq, and value in its
    // REQUIRED form; an OPTIONAL value page opens with its level block and
    // goes through the host twin), then scan-and-pack and one D2H of the
    // streams. Codec 0 launches nothing here.
    DeviceStreams streams;
    if (codec) {
        const int64_t col_words[5] = {
            0, (int64_t)n, nullable ? -1 : 2 * (int64_t)n,
            keep_seq ? 3 * (int64_t)n : -1, -1};
        HIP_TRY(compress_columns_device(s, (const uint8_t*)d_dst, col_words,
                                        n, timed ? ev[3] : nullptr, streams));
    } else if (timed) {
        HIP_TRY(hipEventRecord(ev[3], s));
    }
    // what still has to come back raw: everything under codec 0; under
    // Snappy only what kernel 1e did not take — the packed values and, behind
    // the columns, the bitmaps, counts and error word of the nullable form
    size_t raw_bytes = 0;
    auto bring = [&](size_t w0, size_t w1) {
        raw_bytes += (w1 - w0) * 8;
        return hipMemcpyAsync(host.data() + w0, d_dst + w0, (w1 - w0) * 8,
                              hipMemcpyDeviceToHost, s);
    };
    if (!codec) {
        HIP_TRY(bring(0, words));
    } else if (nullable) {
        HIP_TRY(bring(2 * size_t(n), 3 * size_t(n)));
        HIP_TRY(bring(size_t(n_cols) * n, words));
    }
    HIP_TRY(hipStreamSynchronize(s));
    dst_guard.reset();
    if (timed) {
        float gather_ms = 0, pack_ms = 0, comp_ms = 0;
        HIP_TRY(hipEventElapsedTime(&gather_ms, ev[0], ev[1]));
        HIP_TRY(hipEventElapsedTime(&pack_ms, ev[1], ev[2]));
        HIP_TRY(hipEventElapsedTime(&comp_ms, ev[2], ev[3]));
        fprintf(stderr,
                "[hx] compact rows=%u cols_gathered=%u nullable=%d nulls=%d "
                "codec=%d gather_ms=%.4f pack_ms=%.4f comp_ms=%.4f "
                "d2h_bytes=%zu\n",
                n, nullable ? n_cols - 1 : n_cols, int(nullable), int(nulls),
                codec, gather_ms, pack_ms, comp_ms,
                raw_bytes + streams.d2h_bytes);
    }
    const hx::PagePayload* ready =
        streams.ready.empty() ? nullptr : streams.ready.data();

    const NewSst out = next_sst(h);
    // a column kernel 1e compressed never came to the host (null here): its
    // pages and statistics are in `ready`
    const uint64_t* h_series = streams.on_device[0] ? nullptr : host.data();
    const int64_t* h_ts =
        streams.on_device[1] ? nullptr : (const int64_t*)(host.data() + n);
    const uint64_t* h_val =
        streams.on_device[2] ? nullptr : host.data() + 2 * size_t(n);
    const uint64_t* h_seq = keep_seq && !streams.on_device[3]
                                ? host.data() + 3 * size_t(n) : nullptr;
    std::string werr;
    if (nullable) {
        const uint64_t* h_bm = host.data() + size_t(n_cols) * n;
        if (h_bm[bm_words + nv_words] != 0)
            return fail(HX_ERR_HIP, "compact: sort permutation out of range");
        hx::NullableValues nv{h_val, h_bm,
                              (const uint32_t*)(h_bm + bm_words)};
        werr = hx::write_metric_sst_nullable(out.path, h_series, h_ts, nv,
                                             h_seq, out.seq, n, kRowGroup,
                                             codec, ready);
    } else if (keep_seq) {
        werr = hx::write_metric_sst_seqs(out.path, h_series, h_ts,
                                         (const double*)h_val, h_seq, n,
                                         kRowGroup, codec, ready);
    } else {
        werr = hx::write_metric_sst(out.path, h_series, h_ts,
                                    (const double*)h_val, out.seq, n,
                                    kRowGroup, codec, ready);
    }
    if (!werr.empty()) return fail(HX_ERR_IO, werr);
    return finish_compaction(h, out, in_set, out_new_seq);
}

// What hx_compact and hx_compact_files do with their input set: one scan
// plan over whole files (like the executor) on the first device given, then
// compact_rows.
static hx_status prepare_and_compact(hx_handle* h,
                                     const std::vector<char>& in_set,
                                     bool keep_seq, const hx_device_set* devs,
                                     uint64_t* out_new_seq) {
    std::vector<hx_sst_desc> inputs;
    for (size_t i = 0; i < h->ssts.size(); i++)
        if (in_set[i])
            inputs.push_back({h->ssts[i].path.c_str(), h->ssts[i].seq});
    if (inputs.empty()) return HX_OK;
    hx_scan_spec spec{};
    spec.range = {INT64_MIN, INT64_MAX};
    spec.ssts = inputs.data();
    spec.n_ssts = inputs.size();
    PreparedPtr P(nullptr, hx_prepared_free);
    hx_status st = prepare_single(h, &spec, devs, P);
    if (st != HX_OK) return st;
    return compact_rows(h, P.get(), in_set, keep_seq, out_new_seq);
}

extern "C" hx_status hx_compact(hx_handle* h, hx_time_range range,
                                const hx_device_set* devs,
                                uint64_t* out_new_seq) {
    // Compaction (Executor::do_compaction,
    // executor.rs:155-222): re-runs the scan (GPU decode+dedup) over the
    // ts-overlap CLOSURE of the files overlapping `range` and rewrites them
    // as ONE new SST (native Parquet writer). The closure guarantees no
    // remaining file shares primary keys with the inputs, so the output may
    // carry one constant __seq__ (the freshly allocated file id) without
    // changing any future merge outcome — the reference instead preserves
    // per-row seqs (keep_builtin), which only matters when compacting a
    // PARTIAL overlap set (picker.rs smallest-first can do that; round 2).
    if (!h || !out_new_seq) return fail(HX_ERR_INVALID, "null argument");
    *out_new_seq = 0;
    // ts-overlap closure over the catalog
    std::vector<char> in_set(h->ssts.size(), 0);
    bool grew = true;
    for (size_t i = 0; i < h->ssts.size(); i++)
        if (overlaps(h->ssts[i], range)) in_set[i] = 1;
    while (grew) {
        grew = false;
        for (size_t i = 0; i < h->ssts.size(); i++) {
            if (in_set[i]) continue;
            for (size_t j = 0; j < h->ssts.size(); j++) {
                if (!in_set[j]) continue;
                if (h->ssts[i].ts_min <= h->ssts[j].ts_max &&
                    h->ssts[j].ts_min <= h->ssts[i].ts_max) {
                    in_set[i] = 1;
                    grew = true;
                    break;
                }
            }
        }
    }
    return prepare_and_compact(h, in_set, false, devs, out_new_seq);
}

extern "C" hx_status hx_compact_files(hx_handle* h,
                                      const uint64_t* input_seqs,
                                      size_t n_inputs,
                                      const hx_device_set* devs,
                                      uint64_t* out_new_seq) {
    // Executor general case (executor.rs:155-222, Task{inputs}
    // compaction/mod.rs:26-36): re-run the scan over ONLY the named input
    // files (keep_builtin=true) and rewrite them as one SST that preserves
    // per-row __seq__ — correct for ANY input set, because rows shadowed by
    // files outside the set keep losing future merges through their
    // retained sequences.
    if (!h || !input_seqs || n_inputs == 0 || !out_new_seq)
        return fail(HX_ERR_INVALID, "bad argument");
    *out_new_seq = 0;
    std::vector<char> in_set(h->ssts.size(), 0);
    for (size_t k = 0; k < n_inputs; k++) {
        bool found = false;
        for (size_t i = 0; i < h->ssts.size(); i++)
            if (h->ssts[i].seq == input_seqs[k]) {
                in_set[i] = 1;
                found = true;
            }
        if (!found)
            return fail(HX_ERR_INVALID,
                        "input seq not in catalog: " +
                            std::to_string(input_seqs[k]));
    }
    return prepare_and_compact(h, in_set, true, devs, out_new_seq);
}

// introspection used by CPU tests (no GPU needed): per-SST catalog entries
extern "C" hx_status hx_catalog_size(hx_handle* h, size_t* n) {
    if (!h || !n) return fail(HX_ERR_INVALID, "null");
    *n = h->ssts.size();
    return HX_OK;
}
extern "C" hx_status hx_catalog_entry(hx_handle* h, size_t i, uint64_t* seq,
                                      int64_t* n_rows, int64_t* ts_min,
                                      int64_t* ts_max, int64_t* n_rgs) {
    if (!h || i >= h->ssts.size()) return fail(HX_ERR_INVALID, "bad index");
    const CatSst& s = h->ssts[i];
    *seq = s.seq;
    *n_rows = s.n_rows;
    *ts_min = s.ts_min;
    *ts_max = s.ts_max;
    *n_rgs = (int64_t)s.rgs.size();
    return HX_OK;
}
