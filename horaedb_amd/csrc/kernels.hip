// kernels.hip — gfx950 (MI355X, CDNA4) kernels for the scan/aggregate hot
// path. HBM-bandwidth-bound: wave = 64, coalesced 8B loads,
// one workgroup per 8192-row row group; group table updated with device
// atomics (distinct addresses; L2/L3-resident by grid ordering).
// Replaces the decode/filter/merge arithmetic the reference runs in
// parquet-rs/arrow-rs/datafusion (SURVEY §2 third-party row) plus the
// north-star aggregate (no reference counterpart).
#include <hip/hip_runtime.h>
#include "hx_device.h"
#include "snappy_emit.h"
#include "ba_pages.h"

namespace hx {

#define RLX __ATOMIC_RELAXED
#define AGT __HIP_MEMORY_SCOPE_AGENT

// sentinel for the one-CAS key-claim table mode (host proves, from column
// statistics, that no staged series_id equals it before enabling the mode)
#define KEY_EMPTY 0xFFFFFFFFFFFFFFFFull

__device__ __forceinline__ const uint8_t* hx_ptr(const uint8_t* blob,
                                                 const uint8_t* dec,
                                                 uint64_t off) {
    return ((off & OFF_DEC) ? dec : blob) + (off & OFF_MASK);
}

__device__ __forceinline__ uint64_t mix64(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

// monotone f64 -> u64 map onto IEEE 754 totalOrder (-NaN < -inf < ... < -0 <
// +0 < ... < +inf < +NaN, NaNs by payload): u64 min/max of these words, by
// atomicMin/Max or in registers, pick one operand and ordered_f64 returns
// its 64 bits unchanged — NaN payload, signalling bit and the sign of zero
// included. Every min/max reduction runs on these words, none
// on fmin/fmax (which drop NaN, may quiet it, and are free in the sign of
// zero). Identities: ~0 for min, 0 for max — neither is the image of a
// double a reduction could lose to (the slab initialisers use the same).
__device__ __forceinline__ unsigned long long f64_ordered(double v) {
    unsigned long long u = __double_as_longlong(v);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double ordered_f64(unsigned long long u) {
    return __longlong_as_double((u >> 63) ? (u & 0x7FFFFFFFFFFFFFFFull) : ~u);
}

// order-preserving i64 -> u64 map of a timestamp, full range: the TS
// instances of the aggregate kernels run their min/max machinery on it
__device__ __forceinline__ unsigned long long ts_ordered(int64_t t) {
    return (unsigned long long)t ^ 0x8000000000000000ull;
}

__device__ __forceinline__ int64_t floordiv(int64_t a, int64_t b) {
    int64_t q = a / b;
    if ((a % b) != 0 && ((a < 0) != (b < 0))) q--;
    return q;
}

__device__ __forceinline__ bool sset_has(const AggParams& P, uint64_t s) {
    if (s == P.sset_empty) return false;  // host guarantees sentinel ∉ set
    uint32_t i = (uint32_t)mix64(s) & P.sset_mask;
    for (uint32_t probes = 0; probes <= P.sset_mask; ++probes) {
        uint64_t k = P.sset[i];
        if (k == s) return true;
        if (k == P.sset_empty) return false;
        i = (i + 1) & P.sset_mask;
    }
    return false;
}

// Cross-SST dedup: is row (s,t) of SST `me` (row sequence
// my_seq) shadowed by an equal PK with a HIGHER sequence in another SST of
// the same ts-overlap cluster? SSTs are PK-sorted (storage.rs:244-256), so
// a binary search per candidate member. Constant-seq members below my_seq
// are pruned outright; mixed-seq members (keep_builtin compaction outputs)
// compare the matched row's own __seq__ (read.rs:289-343 orders by
// (pk..., __seq__) read from the row).
__device__ bool shadowed(const AggParams& P, const SstDev& me,
                         uint64_t my_seq, uint64_t s, int64_t t) {
    ClusterDev c = P.clusters[me.cluster];
    for (int32_t j = c.first; j < c.first + c.n; ++j) {
        const SstDev o = P.ssts[P.cluster_members[j]];
        if (o.rank == me.rank) continue;
        if (!o.dense_seq && o.seq <= my_seq) continue;
        const uint64_t* S = (const uint64_t*)(P.dec + (o.dense_series & OFF_MASK));
        const int64_t* T = (const int64_t*)(P.dec + (o.dense_ts & OFF_MASK));
        int64_t lo = 0, hi = o.n_staged;
        while (lo < hi) {
            int64_t mid = (lo + hi) >> 1;
            uint64_t sm = S[mid];
            if (sm < s || (sm == s && T[mid] < t)) lo = mid + 1;
            else hi = mid;
        }
        if (lo < o.n_staged && S[lo] == s && T[lo] == t) {
            uint64_t o_seq = o.dense_seq
                ? ((const uint64_t*)(P.dec + (o.dense_seq & OFF_MASK)))[lo]
                : o.seq;
            if (o_seq > my_seq) return true;
        }
    }
    return false;
}

// row sequence of staged row (rg.row_base + r) of `sst`
__device__ __forceinline__ uint64_t row_seq(const AggParams& P,
                                            const SstDev& sst,
                                            const RgDesc& rg, uint32_t r) {
    return sst.dense_seq
        ? ((const uint64_t*)(P.dec + (sst.dense_seq & OFF_MASK)))
              [rg.row_base + r]
        : sst.seq;
}

// accumulate into key-claim slot i: its slab accumulators, or (direct-
// indexed bucket mode) bucket b's row of the slot's dense accumulator rows
__device__ __forceinline__ void keycas_add(const AggParams& P, uint32_t i,
                                           int64_t b, double vsum,
                                           unsigned long long cnt,
                                           unsigned long long mn,
                                           unsigned long long mx) {
    uint8_t* slot;
    uint32_t off8, off16, off24, off32;
    if (P.n_buckets) {  // direct-indexed bucket row of this series slot
        // bounds check: lo_bucket/n_buckets derive from footer ts stats; an
        // SST whose stats under-report the data range must not index out of
        // the dense row (host sees overflow and retries the hashed path)
        const uint64_t bi = (uint64_t)(b - P.lo_bucket);
        if (bi >= (uint64_t)P.n_buckets) {
            __hip_atomic_fetch_add(P.overflow, 1ull, RLX, AGT);
            return;
        }
        slot = P.bstore + ((size_t)i * P.n_buckets + (size_t)bi) * P.bstride;
        off8 = 0; off16 = 8; off24 = 16; off32 = 24;
    } else {
        slot = P.table.slab + (size_t)i * P.table.stride;
        off8 = 8; off16 = 16; off24 = 24; off32 = 32;
    }
    if (P.ops & (HXK_SUM | HXK_AVG)) atomicAdd((double*)(slot + off8), vsum);
    if (P.ops & (HXK_COUNT | HXK_AVG))
        atomicAdd((unsigned long long*)(slot + off16), cnt);
    if (P.ops & HXK_MIN)
        atomicMin((unsigned long long*)(slot + off24), mn);
    if (P.ops & HXK_MAX)
        atomicMax((unsigned long long*)(slot + off32), mx);
}

// Fast claim path (AoS slab): slot i = {key, sum, cnt[, min, max]} in one
// cache line. key claimed by one CAS against KEY_EMPTY (host proves via
// column statistics that no series == KEY_EMPTY; series-only grouping);
// probe is a plain cached load (a slot transitions KEY_EMPTY -> key exactly
// once per exec, so a stale read can only be KEY_EMPTY, which the CAS
// corrects).
__device__ __forceinline__ void agg_update_keycas(const AggParams& P, uint64_t s,
                                                  int64_t b, double vsum,
                                                  unsigned long long cnt,
                                                  unsigned long long mn,
                                                  unsigned long long mx,
                                                  uint32_t hint_i = 0xFFFFFFFFu,
                                                  uint64_t hint_k = 0) {
    const uint32_t stride = P.table.stride;
    uint32_t i = (uint32_t)mix64(s) & P.table.mask;
    if (hint_i == i && hint_k == s) {  // prefetched probe already matched
        keycas_add(P, i, b, vsum, cnt, mn, mx);
        return;
    }
    const uint32_t probe_cap = P.table.mask < 4096u ? P.table.mask : 4096u;
    for (uint32_t probes = 0; probes <= probe_cap; ++probes) {
        uint8_t* slot = P.table.slab + (size_t)i * stride;
        uint64_t k = *(uint64_t*)slot;
        if (k == KEY_EMPTY) {
            uint64_t expected = KEY_EMPTY;
            if (__hip_atomic_compare_exchange_strong((uint64_t*)slot,
                    &expected, s, RLX, RLX, AGT)) {
                // P.fill is ONE word: per-claim increments serialize at the
                // coherence point and backpressure the whole vmcnt pipeline
                // (measured ~17 ms of a 24 ms launch). The wave kernel still
                // pays this; the one caller that counted claims in bulk (the
                // range kernel's table flush) is gone.
                __hip_atomic_fetch_add(P.fill, 1ull, RLX, AGT);
                k = s;
            } else {
                k = expected;
            }
        }
        if (k == s) {
            keycas_add(P, i, b, vsum, cnt, mn, mx);
            return;
        }
        i = (i + 1) & P.table.mask;
    }
    __hip_atomic_fetch_add(P.overflow, 1ull, RLX, AGT);
}

extern "C" __global__ void __launch_bounds__(256)
k_init_state_slab(uint8_t* slab, uint32_t n_slots, uint32_t stride,
                  uint32_t mm) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n_slots;
         i += blockDim.x * gridDim.x) {
        uint8_t* slot = slab + (size_t)i * stride;
        ((uint64_t*)slot)[0] = 0;   // state + pad
        ((uint64_t*)slot)[3] = 0;   // sum
        ((uint64_t*)slot)[4] = 0;   // cnt
        if (mm) {
            ((uint64_t*)slot)[5] = ~0ull;
            ((uint64_t*)slot)[6] = 0;
        }
    }
}

// direct-indexed bucket store init: rows of {sum, cnt[, min, max]}
extern "C" __global__ void __launch_bounds__(256)
k_init_accum_rows(uint8_t* rows, size_t total_rows, uint32_t stride,
                  uint32_t mm) {
    for (size_t i = blockIdx.x * blockDim.x + threadIdx.x; i < total_rows;
         i += (size_t)blockDim.x * gridDim.x) {
        uint8_t* slot = rows + i * stride;
        ((uint64_t*)slot)[0] = 0;   // sum
        ((uint64_t*)slot)[1] = 0;   // cnt
        if (mm) {
            ((uint64_t*)slot)[2] = ~0ull;
            ((uint64_t*)slot)[3] = 0;
        }
    }
}

// slab init: key=KEY_EMPTY, sum=0, cnt=0, min=~0 (ordered), max=0
extern "C" __global__ void __launch_bounds__(256)
k_init_slab(uint8_t* slab, uint32_t n_slots, uint32_t stride) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n_slots;
         i += blockDim.x * gridDim.x) {
        uint8_t* slot = slab + (size_t)i * stride;
        ((uint64_t*)slot)[0] = KEY_EMPTY;
        ((uint64_t*)slot)[1] = 0;   // sum
        ((uint64_t*)slot)[2] = 0;   // cnt
        if (stride >= 64) {
            ((uint64_t*)slot)[3] = ~0ull;  // min (ordered)
            ((uint64_t*)slot)[4] = 0;      // max (ordered)
        }
    }
}

// General path (16-byte keys, e.g. (series,bucket)): claim via a CAS on a
// state word (0 empty / 1 claiming / 2 ready), then key words; readers are
// gated by the control dependency on state==2 (agent-scope atomics =>
// L2-bypassing, coherent at the memory side).
__device__ __forceinline__ void agg_update(const AggParams& P, uint64_t s,
                                           int64_t b, double vsum,
                                           unsigned long long cnt,
                                           unsigned long long mn,
                                           unsigned long long mx,
                                           uint32_t hint_i = 0xFFFFFFFFu,
                                           uint64_t hint_k = 0) {
    if (P.key_claim) {
        agg_update_keycas(P, s, b, vsum, cnt, mn, mx, hint_i, hint_k);
        return;
    }
    // AoS slot: {state u32, pad u32, series u64, bucket i64, sum, cnt
    // [, min, max]} — probe + claim + update on one/two cache lines
    const uint32_t stride = P.table.stride;
    uint64_t h = mix64(s ^ ((uint64_t)b * 0xD1B54A32D192ED03ull));
    uint32_t i = (uint32_t)h & P.table.mask;
    const uint32_t probe_cap = P.table.mask < 4096u ? P.table.mask : 4096u;
    for (uint32_t probes = 0; probes <= probe_cap; ++probes) {
        uint8_t* slot = P.table.slab + (size_t)i * stride;
        uint32_t* stp = (uint32_t*)slot;
        uint32_t st = __hip_atomic_load(stp, RLX, AGT);
        if (st == 0) {
            uint32_t expected = 0;
            if (__hip_atomic_compare_exchange_strong(stp, &expected, 1u, RLX,
                                                     RLX, AGT)) {
                __hip_atomic_store((uint64_t*)(slot + 8), s, RLX, AGT);
                __hip_atomic_store((unsigned long long*)(slot + 16),
                                   (unsigned long long)b, RLX, AGT);
                __hip_atomic_fetch_add(P.fill, 1ull, RLX, AGT);
                __hip_atomic_store(stp, 2u, __ATOMIC_RELEASE, AGT);
                st = 2;
            } else {
                st = expected;
            }
        }
        if (st == 1) {  // claimer is storing the key; bounded spin
            uint32_t spins = 0;
            do {
                st = __hip_atomic_load(stp, RLX, AGT);
                if (++spins > (1u << 22)) {
                    __hip_atomic_fetch_add(P.overflow, 1ull, RLX, AGT);
                    return;
                }
            } while (st != 2);
        }
        if (__hip_atomic_load((uint64_t*)(slot + 8), RLX, AGT) == s &&
            (int64_t)__hip_atomic_load((unsigned long long*)(slot + 16), RLX,
                                       AGT) == b) {
            if (P.ops & (HXK_SUM | HXK_AVG))
                atomicAdd((double*)(slot + 24), vsum);
            if (P.ops & (HXK_COUNT | HXK_AVG))
                atomicAdd((unsigned long long*)(slot + 32), cnt);
            if (P.ops & HXK_MIN)
                atomicMin((unsigned long long*)(slot + 40), mn);
            if (P.ops & HXK_MAX)
                atomicMax((unsigned long long*)(slot + 48), mx);
            return;
        }
        i = (i + 1) & P.table.mask;
    }
    __hip_atomic_fetch_add(P.overflow, 1ull, RLX, AGT);
}

// Value validity of row r of unit rgi (nullable f64 value column, DESIGN
// §3): the unit's bitmap is LSB-first in the page blob, its row 0 at bit
// RgValid::bit. Units without a bitmap (off == 0) hold no nulls. Only the
// null-aware launches call this; r must be a row of the unit.
__device__ __forceinline__ bool row_valid(const AggParams& P, uint32_t rgi,
                                          uint32_t r) {
    const RgValid rv = ((const RgValid*)(P.rgs + P.n_rgs))[rgi];
    if (!rv.off) return true;
    const uint64_t bit = rv.bit + r;
    const uint64_t w = ((const uint64_t*)(P.blob + rv.off))[bit >> 6];
    return (w >> (bit & 63u)) & 1ull;
}

// Per-row filter + dedup (shared by both aggregate kernels).
// Returns alive; s/t are the row's PK. DESIGN.md §5.
__device__ __forceinline__ bool row_alive(const AggParams& P, const RgDesc& rg,
                                          const SstDev& sst, const uint64_t* S,
                                          const int64_t* T, uint32_t r,
                                          uint32_t n, uint64_t s, int64_t t) {
    bool alive = (t >= P.ts_lo) & (t < P.ts_hi);
    if (alive && P.use_sset) alive = sset_has(P, s);
    if (alive && !P.keep_dups) {
        // within-SST dedup: the LAST row of an equal-PK run survives
        // (LastValueOperator, operator.rs:37-44; plan order read.rs:456-480)
        bool dup = false;
        if (r + 1 < n) {
            dup = (S[r + 1] == s) & (T[r + 1] == t);
        } else if (rg.next_rg >= 0) {
            const RgDesc nx = P.rgs[rg.next_rg];
            uint64_t s2 = *(const uint64_t*)hx_ptr(P.blob, P.dec, nx.series_off);
            int64_t t2 = *(const int64_t*)hx_ptr(P.blob, P.dec, nx.ts_off);
            dup = (s2 == s) & (t2 == t);
        }
        if (!dup && sst.cluster >= 0)
            dup = shadowed(P, sst, row_seq(P, sst, rg, r), s, t);
        alive = !dup;
    }
    return alive;
}

// ---------------------------------------------------------------------------
// The headline fused kernel: decode(PLAIN in place) + ts-range/series-set
// filter + MergeExec dedup + hash group-by aggregate. One workgroup per row
// group, grid-stride; each thread strides rows (coalesced 8B column loads).
// ---------------------------------------------------------------------------
// Per-window worker for k_scan_agg: 64 consecutive rows on one wave —
// loads, filter, dedup, wave-segmented pre-reduction. Returns whether this
// lane must issue a table update (run head with survivors) via out params.
struct WinResult {
    uint64_t s;
    int64_t b;
    double vv;
    unsigned long long mn, mx;   // f64_ordered words
    unsigned long long c;
    bool head;
    uint32_t hint_i;    // early-probed slot index (key-claim tables)
    uint64_t hint_k;    // its key value at probe time
};

template <bool NULLS, bool MM, bool TS>
__device__ __forceinline__ void scan_window(const AggParams& P,
                                            const RgDesc& rg, uint32_t rgi,
                                            const SstDev& sst,
                                            const uint64_t* S,
                                            const int64_t* T, const double* V,
                                            uint32_t base, uint32_t n,
                                            int lane,
                                            unsigned long long& my_matched,
                                            WinResult& W) {
    const uint32_t r = base + threadIdx.x;
    const bool inb = r < n;
    const bool has_next = r + 1 < n;
    uint64_t s = KEY_EMPTY;
    int64_t t = 0;
    double v = 0.0;
    uint64_t s1 = 0;
    int64_t t1 = 0;
    bool alive = false;
    // issue ALL of the window's loads together (row, value, successor):
    // one memory round-trip per window instead of a 3-deep dependent chain
    if (inb) {
        t = T[r];
        s = S[r];
        v = V[r];
        if (has_next) {
            s1 = S[r + 1];
            t1 = T[r + 1];
        }
    }
    if (inb) {
        alive = (t >= P.ts_lo) & (t < P.ts_hi);
        if (alive && P.use_sset) alive = sset_has(P, s);
        if (alive && !P.keep_dups) {
            bool dup = false;
            if (has_next) {
                dup = (s1 == s) & (t1 == t);
            } else if (rg.next_rg >= 0) {
                const RgDesc nx = P.rgs[rg.next_rg];
                uint64_t s2 = *(const uint64_t*)hx_ptr(P.blob, P.dec,
                                                       nx.series_off);
                int64_t t2 = *(const int64_t*)hx_ptr(P.blob, P.dec, nx.ts_off);
                dup = (s2 == s) & (t2 == t);
            }
            if (!dup && sst.cluster >= 0)
            dup = shadowed(P, sst, row_seq(P, sst, rg, r), s, t);
            alive = !dup;
        }
        if (!alive) v = 0.0;
    }
    int64_t b = (inb && P.bucket_ms) ? floordiv(t, P.bucket_ms) : 0;
    // a null value is still a row: it counts into matched (and took part in
    // the dedup above), then drops out of the aggregates
    if (NULLS && alive) {
        my_matched += 1ull;
        alive = row_valid(P, rgi, r);
    }
    unsigned long long c = alive ? 1ull : 0ull;
    double vv = alive ? v : 0.0;
    // ordered words with the ordered identities: a dead lane must lose to
    // every live value, +NaN in a min and -NaN in a max included. Only the
    // MM instances (min or max requested) carry them through the reduction.
    // The TS instances (first/last) feed the same reduction the
    // row's timestamp as an ordered word in place of the value's.
    const unsigned long long ov = TS ? ts_ordered(t) : f64_ordered(v);
    unsigned long long mn = (MM && alive) ? ov : ~0ull;
    unsigned long long mx = (MM && alive) ? ov : 0ull;
    if (!NULLS) my_matched += c;
    // issue the table probe NOW: its L3 latency hides under the cross-lane
    // reduction, and a hit skips the dependent probe load in agg_update
    W.hint_i = 0xFFFFFFFFu;
    W.hint_k = 0;
    if (P.key_claim && alive) {
        W.hint_i = (uint32_t)mix64(s) & P.table.mask;
        W.hint_k = *(const uint64_t*)(P.table.slab +
                                      (size_t)W.hint_i * P.table.stride);
    }
    const uint64_t sp = __shfl_up(s, 1, 64);
    const int64_t bp = __shfl_up((long long)b, 1, 64);
    const bool head = (lane == 0) || sp != s || bp != b;
    bool done = false;
    for (int d = 1; d < 64; d++) {
        const uint64_t s2 = __shfl_down(s, d, 64);
        const long long b2 = __shfl_down((long long)b, d, 64);
        const double v2 = __shfl_down(vv, d, 64);
        const unsigned long long c2 = __shfl_down(c, d, 64);
        done = done || (lane + d >= 64) || s2 != s || b2 != b;
        if (head && !done) {
            vv += v2;
            c += c2;
        }
        if (MM) {
            const unsigned long long mn2 = __shfl_down(mn, d, 64);
            const unsigned long long mx2 = __shfl_down(mx, d, 64);
            if (head && !done) {
                mn = mn2 < mn ? mn2 : mn;
                mx = mx2 > mx ? mx2 : mx;
            }
        }
        if (__all(done)) break;
    }
    W.s = s;
    W.b = b;
    W.vv = vv;
    W.mn = mn;
    W.mx = mx;
    W.c = c;
    W.head = head;
}

// The headline fused kernel: decode(PLAIN in place) + ts-range/series-set
// filter + MergeExec dedup + hash group-by aggregate. One workgroup per
// row-group slice, grid-stride; TWO 64-row windows per iteration so two
// dependent table-update chains (L3 probe + atomics) overlap — the kernel
// is memory-latency-bound (SQ_WAIT_ANY 76%) at full occupancy, so the
// lever is per-wave memory-level parallelism.
template <bool NULLS, bool MM, bool TS>
__global__ void __launch_bounds__(256)
k_scan_agg(AggParams P) {
    unsigned long long my_matched = 0;
    const int lane = threadIdx.x & 63;
    for (uint32_t rgi = blockIdx.x; rgi < P.n_rgs; rgi += gridDim.x) {
        // early-abort once the table saturates: the host retries with a
        // larger table, so finishing a doomed pass only burns time.
        // One lane per wave polls the hot counter (same-address loads from
        // every lane would serialize at the coherence point).
        if ((rgi & 7u) == (blockIdx.x & 7u)) {
            // best-effort saturation check: a PLAIN (L1-served) load — a
            // coherent load of this hot word from every wave serializes at
            // the coherence point (~88/us) and cost 50% kernel time; stale
            // reads only delay the abort, which the probe cap bounds anyway
            unsigned long long f = 0;
            if (lane == 0) f = *(volatile const unsigned long long*)P.fill;
            f = __shfl(f, 0, 64);
            if (f > P.fill_limit) {
                if (threadIdx.x == 0)
                    __hip_atomic_fetch_add(P.overflow, 1ull, RLX, AGT);
                break;
            }
        }
        const RgDesc rg = P.rgs[rgi];
        const uint64_t* S = (const uint64_t*)hx_ptr(P.blob, P.dec, rg.series_off);
        const int64_t* T = (const int64_t*)hx_ptr(P.blob, P.dec, rg.ts_off);
        const double* V = (const double*)hx_ptr(P.blob, P.dec, rg.val_off);
        const SstDev sst = P.ssts[rg.sst_id];
        const uint32_t n = rg.n_rows;
        for (uint32_t base = 0; base < n; base += blockDim.x * 2) {
            WinResult A, B;
            B.c = 0;
            B.head = false;
            scan_window<NULLS, MM, TS>(P, rg, rgi, sst, S, T, V, base, n, lane,
                                   my_matched, A);
            const uint32_t base2 = base + blockDim.x;
            if (base2 < n)
                scan_window<NULLS, MM, TS>(P, rg, rgi, sst, S, T, V, base2, n,
                                       lane, my_matched, B);
            const bool upA = A.head && A.c > 0;
            const bool upB = B.head && B.c > 0;
            if (upA && upB) {  // two independent chains: overlap them
                agg_update(P, A.s, A.b, A.vv, A.c, A.mn, A.mx, A.hint_i,
                           A.hint_k);
                agg_update(P, B.s, B.b, B.vv, B.c, B.mn, B.mx, B.hint_i,
                           B.hint_k);
            } else if (upA) {
                agg_update(P, A.s, A.b, A.vv, A.c, A.mn, A.mx, A.hint_i,
                           A.hint_k);
            } else if (upB) {
                agg_update(P, B.s, B.b, B.vv, B.c, B.mn, B.mx, B.hint_i,
                           B.hint_k);
            }
        }
    }
    for (int off = 32; off > 0; off >>= 1)
        my_matched += __shfl_down(my_matched, off, 64);
    if ((threadIdx.x & 63) == 0 && my_matched)
        atomicAdd(P.matched, my_matched);
}

// ---------------------------------------------------------------------------
// Series-range partitioned aggregation. Position-aligned LDS
// gangs lose to series-position jitter (sqrt-scale fluctuations between
// SSTs dwarf a window), so the partition here is by series VALUE: block b
// owns [bounds[b], bounds[b+1]) across every SST; its series fit an LDS
// table by construction and leave it once, as one key-ordered run — no
// global RMW per row or per window-run at all.
// ---------------------------------------------------------------------------

// Stride-512 series samples per rg slice (16 fixed slots, ~0 padding): the
// host sorts these into equal-sample quantile boundaries. The stride phase
// is JITTERED per slice (deterministic hash of the slice index): SSTs of one
// store share the same sorted series universe, so un-jittered samples land
// on near-identical series in every SST and the distinct-count solve
// under-estimates by ~the SST count (measured 39k for 10M at the 1B shape —
// the round-1 LDS-fallback storm). Jitter makes samples ~independent row
// draws, which is exactly the model the u = x(1-e^{-m/x}) solver assumes.
extern "C" __global__ void __launch_bounds__(256)
k_sample_series(const RgDesc* __restrict__ rgs, uint32_t n_rgs,
                const uint8_t* __restrict__ blob,
                const uint8_t* __restrict__ dec, uint64_t* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const uint32_t wave_id = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint32_t n_waves = (gridDim.x * blockDim.x) >> 6;
    for (uint32_t g = wave_id; g < n_rgs; g += n_waves) {
        const RgDesc rg = rgs[g];
        const uint64_t* S =
            (const uint64_t*)hx_ptr(blob, dec, rg.series_off);
        const uint32_t phase =
            (uint32_t)(mix64((uint64_t)g ^ 0x9E3779B97F4A7C15ull) >> 40) &
            511u;
        if (lane < 16) {
            uint32_t r = phase + (uint32_t)lane * 512u;
            out[(size_t)g * 16 + lane] = (r < rg.n_rows) ? S[r] : ~0ull;
        }
    }
}

// Wave-parallel 64-ary lower_bound: count of indices in [0,n) whose probed
// key is < target (keys ascending). ~log64(n) rounds of one parallel load.
template <typename Pred>
__device__ __forceinline__ uint32_t lb64(uint32_t n, uint64_t target,
                                         int lane, Pred key_at) {
    uint32_t lo = 0, rem = n;
    while (rem > 0) {
        const uint32_t step = (rem + 63u) >> 6;
        const uint32_t p = lo + (uint32_t)lane * step;
        const bool in = (uint32_t)lane * step < rem;
        const bool t = in && (key_at(p) < target);
        const uint32_t k = (uint32_t)__popcll(__ballot(t));
        if (k == 0) break;
        const uint32_t adv = (k - 1) * step + 1;
        lo += adv;
        rem = (step - 1u) < (rem - adv) ? (step - 1u) : (rem - adv);
    }
    return lo;   // first index with key >= target (== n if none)
}

// Row bounds per (boundary, sst): first staged row with series >= bounds[b],
// packed (rg-list position << 32 | row within slice). Computed once per
// prepare (decode is deterministic, so bounds survive re-decode).
extern "C" __global__ void __launch_bounds__(256)
k_range_bounds(AggParams P, RangeAux R, uint64_t* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const uint32_t wave_id = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint32_t n_waves = (gridDim.x * blockDim.x) >> 6;
    const uint32_t total = (R.n_blocks + 1) * R.n_ssts;
    for (uint32_t w = wave_id; w < total; w += n_waves) {
        const uint32_t b = w / R.n_ssts, si = w % R.n_ssts;
        const uint64_t target = R.bounds[b];
        const int32_t off = R.sst_rg_off[si];
        const uint32_t cnt = (uint32_t)R.sst_rg_cnt[si];
        // level 1: over slices by their first-row series
        const uint32_t g = lb64(cnt, target, lane, [&](uint32_t p) {
            const RgDesc rg = P.rgs[R.sst_rgs[off + (int32_t)p]];
            return *(const uint64_t*)hx_ptr(P.blob, P.dec, rg.series_off);
        });
        uint64_t packed;
        if (g == 0) {
            packed = 0;   // boundary at the very first row
        } else {
            // boundary row is inside slice g-1, or at the start of slice g
            const RgDesc rg = P.rgs[R.sst_rgs[off + (int32_t)(g - 1)]];
            const uint64_t* S =
                (const uint64_t*)hx_ptr(P.blob, P.dec, rg.series_off);
            const uint32_t r = lb64(rg.n_rows, target, lane,
                                    [&](uint32_t p) { return S[p]; });
            packed = (r == rg.n_rows) ? ((uint64_t)g << 32)
                                      : (((uint64_t)(g - 1) << 32) | r);
        }
        if (lane == 0) out[w] = packed;
    }
}

// ---------------------------------------------------------------------------
// Pair-load series-range kernel. Its predecessor (one row per lane, wave
// shuffle pre-reduction) was 95% SQ_WAIT_ANY at ~2% LDS-array
// utilization: pure latency exposure, not throughput. This kernel removes
// latency sources:
//   - 16 B/lane dwordx4 loads (the calibrated wide-stream width): each lane
//     owns TWO consecutive rows, halving load instructions per row;
//   - the successor row for dedup comes from the register pair / one
//     cross-lane shuffle instead of a second global read of S and T;
//   - NO cross-lane run pre-reduction (measured ±3%): each lane merges its
//     own pair in registers (36% of adjacent rows share a series at the
//     headline shape) and issues its 1-2 LDS updates directly.
// Per block: reset the LDS table, scan the block's series range in every
// SST, then emit the live slots as one key-ordered run. The
// kernel never touches the global hash table: it has no saturation poll,
// and its only overflow policy is "report the block, emit nothing".
// ---------------------------------------------------------------------------

// Add one (key, partial aggregate) to the block's LDS table, first probe at
// slot i. `pre` is lkey[i] as the caller read it right after the row loads,
// so the common-case key check pays no fresh LDS round-trip on the update
// critical path. A stale EMPTY only re-routes through the CAS (keys
// transition EMPTY->key exactly once), never corrupts.
//
// The probe walks the WHOLE table, so a key that finds no slot proves the
// block holds more than ne distinct keys; that returns false (block
// overflow, the host re-partitions). Nothing here goes to global memory.
template <bool MM>
__device__ __forceinline__ bool lds_update(uint64_t* lkey, double* lsum,
                                           unsigned int* lcnt,
                                           unsigned long long* lmin,
                                           unsigned long long* lmax,
                                           uint32_t ne, uint64_t sv, double v,
                                           uint32_t cnt,
                                           unsigned long long mn,
                                           unsigned long long mx,
                                           uint32_t i, uint64_t pre) {
#pragma unroll 1
    for (uint32_t probes = 0; probes < ne; probes++) {
        uint64_t kk = (probes == 0) ? pre : lkey[i];
        if (kk == KEY_EMPTY) {
            uint64_t old = atomicCAS(&lkey[i], KEY_EMPTY, sv);
            kk = (old == KEY_EMPTY) ? sv : old;
        }
        if (kk == sv) {
            atomicAdd(&lsum[i], v);
            atomicAdd(&lcnt[i], cnt);
            if (MM) {
                atomicMin(&lmin[i], mn);
                atomicMax(&lmax[i], mx);
            }
            return true;
        }
        i = (i + 1) & (ne - 1);
    }
    return false;
}

// Sorted-run epilogue of one block: order the live LDS
// entries by ascending unsigned key and write them as one contiguous run.
// The slot function is order-preserving but linear probing displaces keys
// (and wraps), so the order is established exactly: live slot indices are
// compacted into lidx (u16, arbitrary order), padded to a power of two with
// the index of an EMPTY slot (key ~0 sorts last; one exists whenever padding
// is needed, since ne is itself a power of two), and bitonic-sorted by the
// keys they point at. Output space is reserved with ONE agent-scope add per
// block; no block ever waits on another.
template <bool MM>
__device__ __forceinline__ void emit_sorted_run(
    const RangeOut& O, uint32_t blk, uint32_t ne, const uint64_t* lkey,
    const double* lsum, const unsigned int* lcnt,
    const unsigned long long* lmin, const unsigned long long* lmax,
    unsigned short* lidx, uint32_t* s_live, uint32_t* s_empty,
    unsigned long long* s_off) {
    for (uint32_t i = threadIdx.x; i < ne; i += blockDim.x) {
        if (lkey[i] != KEY_EMPTY)
            lidx[atomicAdd(s_live, 1u)] = (unsigned short)i;
        else
            *s_empty = i;   // any empty slot will do
    }
    __syncthreads();
    const uint32_t live = *s_live;
    uint32_t m = 1;
    while (m < live) m <<= 1;
    if (threadIdx.x == 0) {
        // reserve now; the add's latency hides under the sort
        unsigned long long off = 0;
        if (live) off = __hip_atomic_fetch_add(O.cursor,
                                               (unsigned long long)live, RLX,
                                               AGT);
        const bool fits = off + live <= O.cap;
        if (!fits) {
            __hip_atomic_fetch_add(O.stage_ovf, 1ull, RLX, AGT);
            off = ~0ull;
        }
        *s_off = off;
        O.desc[blk] = fits ? (((uint64_t)live << 32) | (uint64_t)off) : 0ull;
    }
    const uint32_t pad = *s_empty;
    for (uint32_t p = live + threadIdx.x; p < m; p += blockDim.x)
        lidx[p] = (unsigned short)pad;
    __syncthreads();
    for (uint32_t k = 2; k <= m; k <<= 1) {
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            for (uint32_t t = threadIdx.x; t < (m >> 1); t += blockDim.x) {
                const uint32_t lo = 2u * t - (t & (j - 1u));   // bit j clear
                const uint32_t hi = lo + j;
                const unsigned short a = lidx[lo], b = lidx[hi];
                const bool up = (lo & k) == 0;
                if ((lkey[a] > lkey[b]) == up) {
                    lidx[lo] = b;
                    lidx[hi] = a;
                }
            }
            __syncthreads();
        }
    }
    const unsigned long long off = *s_off;
    if (off == ~0ull) return;   // staging full: host retries larger
    for (uint32_t t = threadIdx.x; t < live; t += blockDim.x) {
        const uint32_t a = lidx[t];
        O.key[off + t] = lkey[a];
        O.sum[off + t] = lsum[a];
        O.cnt[off + t] = (unsigned long long)lcnt[a];
        if (MM) {
            O.vmin[off + t] = ordered_f64(lmin[a]);
            O.vmax[off + t] = ordered_f64(lmax[a]);
        }
    }
}

template <bool MM, bool NULLS, bool TS>
__global__ void __launch_bounds__(256)
k_scan_agg_range2(AggParams P, RangeAux R, RangeOut O) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ uint32_t s_live, s_empty, s_bovf;
    __shared__ unsigned long long s_off;
    const uint32_t ne = R.ne;
    uint64_t* lkey = (uint64_t*)smem;
    double* lsum = (double*)(smem + (size_t)ne * 8);
    unsigned long long* lmin = (unsigned long long*)(smem + (size_t)ne * 16);
    unsigned long long* lmax = (unsigned long long*)(smem + (size_t)ne * 24);
    unsigned int* lcnt = (unsigned int*)(smem + (size_t)ne * (MM ? 32 : 16));
    unsigned short* lidx =   // sort permutation, 2 B per slot
        (unsigned short*)(smem + (size_t)ne * (MM ? 36 : 20));
    const int lane = threadIdx.x & 63;
    const uint32_t wave = threadIdx.x >> 6;
    const uint32_t n_waves = blockDim.x >> 6;
    unsigned long long my_matched = 0;
    for (uint32_t blk = blockIdx.x; blk < R.n_blocks; blk += gridDim.x) {
        if (threadIdx.x == 0) {
            s_live = 0;
            s_empty = 0;
            s_bovf = 0;
        }
        for (uint32_t i = threadIdx.x; i < ne; i += blockDim.x) {
            lkey[i] = KEY_EMPTY;
            lsum[i] = 0.0;
            lcnt[i] = 0u;
            if (MM) {
                lmin[i] = ~0ull;
                lmax[i] = 0ull;
            }
        }
        // slot of a key = its fractional position within the block's series
        // range (RangeAux::ne); collisions fall back to linear probing
        const uint64_t ilo = R.bounds[blk];
        const uint64_t ihi = R.bounds[blk + 1];
        const double islope = (double)ne / ((double)(ihi - ilo) + 1.0);
        __syncthreads();
        bool lost = false;   // a key of this lane found no LDS slot
        for (uint32_t si = wave; si < R.n_ssts; si += n_waves) {
            const int32_t loff = R.sst_rg_off[si];
            const uint64_t pk0 = R.bound_rows[(size_t)blk * R.n_ssts + si];
            const uint64_t pk1 =
                R.bound_rows[(size_t)(blk + 1) * R.n_ssts + si];
            uint32_t pos = (uint32_t)(pk0 >> 32);
            uint32_t row = (uint32_t)pk0;
            const uint32_t epos = (uint32_t)(pk1 >> 32);
            const uint32_t erow = (uint32_t)pk1;
            while ((pos < epos || (pos == epos && row < erow)) &&
                   !__any(lost)) {
                const int32_t rgi = R.sst_rgs[loff + (int32_t)pos];
                const RgDesc rg = P.rgs[rgi];
                const uint64_t* S =
                    (const uint64_t*)hx_ptr(P.blob, P.dec, rg.series_off);
                const int64_t* T =
                    (const int64_t*)hx_ptr(P.blob, P.dec, rg.ts_off);
                const double* V =
                    (const double*)hx_ptr(P.blob, P.dec, rg.val_off);
                const SstDev sst = P.ssts[rg.sst_id];
                const uint32_t hi = (pos == epos) ? erow : rg.n_rows;
                const uint32_t nt = rg.n_rows;   // true slice rows
                for (uint32_t base = row & ~1u;
                     base < hi && !__any(lost); base += 128) {
                    const uint32_t r0 = base + 2u * (uint32_t)lane;
                    const uint32_t r1 = r0 + 1u;
                    // load the pair (dwordx4); mask by the ARRAY bound nt —
                    // rows in [hi, nt) load safely and are filtered below
                    uint64_t s0 = KEY_EMPTY, s1 = KEY_EMPTY;
                    int64_t t0 = 0, t1 = 0;
                    double v0 = 0.0, v1 = 0.0;
                    if (r1 < nt) {
                        const ulonglong2 sp =
                            *(const ulonglong2*)(S + r0);
                        const longlong2 tp = *(const longlong2*)(T + r0);
                        const double2 vp = *(const double2*)(V + r0);
                        s0 = sp.x;
                        s1 = sp.y;
                        t0 = tp.x;
                        t1 = tp.y;
                        v0 = vp.x;
                        v1 = vp.y;
                    } else if (r0 < nt) {
                        s0 = S[r0];
                        t0 = T[r0];
                        v0 = V[r0];
                    }
                    // slot + probe prefetch: issue the LDS probe reads NOW
                    // so their ~50-cycle latency hides under filter/dedup
                    const uint32_t x0 =
                        (uint32_t)((double)(s0 - ilo) * islope);
                    const uint32_t x1 =
                        (uint32_t)((double)(s1 - ilo) * islope);
                    const uint32_t iA = x0 < ne ? x0 : ne - 1;
                    const uint32_t iB = x1 < ne ? x1 : ne - 1;
                    const uint64_t preA = lkey[iA];
                    const uint64_t preB = lkey[iB];
                    // window validity: [max(row, base), hi)
                    bool a0 = r0 >= row && r0 < hi;
                    bool a1 = r1 >= row && r1 < hi;
                    a0 = a0 && (t0 >= P.ts_lo) & (t0 < P.ts_hi);
                    a1 = a1 && (t1 >= P.ts_lo) & (t1 < P.ts_hi);
                    if (P.use_sset) {
                        if (a0) a0 = sset_has(P, s0);
                        if (a1) a1 = sset_has(P, s1);
                    }
                    // successor of r1 = next lane's r0 (one 64-bit shuffle
                    // pair); lane 63 / slice-tail fall back to scalar loads
                    const uint64_t sn = __shfl_down(s0, 1, 64);
                    const int64_t tn = __shfl_down((long long)t0, 1, 64);
                    if (a0 && !P.keep_dups) {
                        bool dup;
                        if (r1 < nt) {
                            dup = (s1 == s0) & (t1 == t0);
                        } else if (rg.next_rg >= 0) {
                            const RgDesc nx = P.rgs[rg.next_rg];
                            dup = (*(const uint64_t*)hx_ptr(
                                       P.blob, P.dec, nx.series_off) == s0) &
                                  (*(const int64_t*)hx_ptr(
                                       P.blob, P.dec, nx.ts_off) == t0);
                        } else {
                            dup = false;
                        }
                        if (!dup && sst.cluster >= 0)
                            dup = shadowed(P, sst, row_seq(P, sst, rg, r0),
                                           s0, t0);
                        a0 = !dup;
                    }
                    if (a1 && !P.keep_dups) {
                        bool dup;
                        const uint32_t r2 = r1 + 1u;
                        if (r2 < nt) {
                            if (lane < 63) {
                                dup = (sn == s1) & (tn == t1);
                            } else {
                                dup = (S[r2] == s1) & (T[r2] == t1);
                            }
                        } else if (rg.next_rg >= 0) {
                            const RgDesc nx = P.rgs[rg.next_rg];
                            dup = (*(const uint64_t*)hx_ptr(
                                       P.blob, P.dec, nx.series_off) == s1) &
                                  (*(const int64_t*)hx_ptr(
                                       P.blob, P.dec, nx.ts_off) == t1);
                        } else {
                            dup = false;
                        }
                        if (!dup && sst.cluster >= 0)
                            dup = shadowed(P, sst, row_seq(P, sst, rg, r1),
                                           s1, t1);
                        a1 = !dup;
                    }
                    my_matched += (a0 ? 1u : 0u) + (a1 ? 1u : 0u);
                    // null values: matched above, no update — each row of
                    // the pair on its own, so the merge below sees only
                    // rows that carry a value
                    if (NULLS) {
                        if (a0) a0 = row_valid(P, (uint32_t)rgi, r0);
                        if (a1) a1 = row_valid(P, (uint32_t)rgi, r1);
                    }
                    // in-lane pair merge, then direct LDS updates; min/max
                    // travel as ordered words, mapped only for rows that
                    // survived (only the MM instances read them, so the
                    // others compute none of this)
                    const bool merge = a0 && a1 && (s0 == s1);
                    if (merge) {
                        const unsigned long long o0 =
                            TS ? ts_ordered(t0) : f64_ordered(v0);
                        const unsigned long long o1 =
                            TS ? ts_ordered(t1) : f64_ordered(v1);
                        const bool lt = o1 < o0;
                        lost |= !lds_update<MM>(
                            lkey, lsum, lcnt, lmin, lmax, ne, s0, v0 + v1,
                            2u, lt ? o1 : o0, lt ? o0 : o1, iA, preA);
                    } else {
                        if (a0) {
                            const unsigned long long o =
                                TS ? ts_ordered(t0) : f64_ordered(v0);
                            lost |= !lds_update<MM>(
                                lkey, lsum, lcnt, lmin, lmax, ne, s0, v0,
                                1u, o, o, iA, preA);
                        }
                        if (a1) {
                            const unsigned long long o =
                                TS ? ts_ordered(t1) : f64_ordered(v1);
                            lost |= !lds_update<MM>(
                                lkey, lsum, lcnt, lmin, lmax, ne, s1, v1,
                                1u, o, o, iB, preB);
                        }
                    }
                }
                pos++;
                row = 0;
            }
        }
        if (lost) s_bovf = 1u;
        __syncthreads();
        if (s_bovf) {
            // more than ne distinct keys in this block's range: the host
            // re-partitions with more blocks; emit nothing
            if (threadIdx.x == 0) {
                __hip_atomic_fetch_add(O.block_ovf, 1ull, RLX, AGT);
                O.desc[blk] = 0ull;
            }
        } else {
            emit_sorted_run<MM>(O, blk, ne, lkey, lsum, lcnt, lmin, lmax,
                                lidx, &s_live, &s_empty, &s_off);
        }
        __syncthreads();
    }
    for (int off = 32; off > 0; off >>= 1)
        my_matched += __shfl_down(my_matched, off, 64);
    if ((threadIdx.x & 63) == 0 && my_matched)
        atomicAdd(P.matched, my_matched);
}

// ---------------------------------------------------------------------------
// Placement of the sorted runs. Runs sit in staging in block
// COMPLETION order; block b's keys all precede block b+1's, so the result
// is the runs concatenated in blk order. k_place_scan: exclusive prefix of
// the per-block counts (one workgroup, n_blocks <= 131072); k_place_runs:
// one wave per run copies every column to its final position and computes
// avg. Both are no-ops after an overflow (the host retries).
// ---------------------------------------------------------------------------
extern "C" __global__ void __launch_bounds__(1024)
k_place_scan(RangePlace Q) {
    __shared__ uint32_t part[1024];
    const uint32_t per = (Q.n_blocks + 1023u) / 1024u;
    const uint32_t b0 = threadIdx.x * per;
    const uint32_t b1 = b0 + per < Q.n_blocks ? b0 + per : Q.n_blocks;
    uint32_t mine = 0;
    for (uint32_t b = b0; b < b1; b++) mine += (uint32_t)(Q.desc[b] >> 32);
    part[threadIdx.x] = mine;
    __syncthreads();
    for (uint32_t d = 1; d < 1024; d <<= 1) {
        const uint32_t add = threadIdx.x >= d ? part[threadIdx.x - d] : 0u;
        __syncthreads();
        part[threadIdx.x] += add;
        __syncthreads();
    }
    uint32_t run = part[threadIdx.x] - mine;   // exclusive
    for (uint32_t b = b0; b < b1; b++) {
        Q.prefix[b] = run;
        run += (uint32_t)(Q.desc[b] >> 32);
    }
}

extern "C" __global__ void __launch_bounds__(256)
k_place_runs(RangePlace Q) {
    const unsigned long long total = *Q.cursor;
    if (*Q.stage_ovf || *Q.block_ovf || total > Q.cap) return;
    const int lane = threadIdx.x & 63;
    const uint32_t wave_id = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint32_t n_waves = (gridDim.x * blockDim.x) >> 6;
    unsigned long long* d_key = Q.dst;
    double* d_sum = Q.c_sum >= 0 ? (double*)(Q.dst + Q.c_sum * total) : nullptr;
    unsigned long long* d_cnt = Q.c_cnt >= 0 ? Q.dst + Q.c_cnt * total : nullptr;
    double* d_min = Q.c_min >= 0 ? (double*)(Q.dst + Q.c_min * total) : nullptr;
    double* d_max = Q.c_max >= 0 ? (double*)(Q.dst + Q.c_max * total) : nullptr;
    double* d_avg = Q.c_avg >= 0 ? (double*)(Q.dst + Q.c_avg * total) : nullptr;
    for (uint32_t b = wave_id; b < Q.n_blocks; b += n_waves) {
        const uint64_t d = Q.desc[b];
        const uint32_t cnt = (uint32_t)(d >> 32);
        if (!cnt) continue;
        const uint32_t src = (uint32_t)d;
        const uint32_t dst = Q.prefix[b];
        // src + cnt <= cap by the reservation; dst + cnt <= total as the
        // prefix sums the same counts the cursor added up
        for (uint32_t t = lane; t < cnt; t += 64) {
            const size_t i = (size_t)src + t, o = (size_t)dst + t;
            d_key[o] = Q.key[i];
            const double sm = Q.sum[i];
            const unsigned long long c = Q.cnt[i];
            if (d_sum) d_sum[o] = sm;
            if (d_cnt) d_cnt[o] = c;
            if (d_min) d_min[o] = Q.vmin[i];
            if (d_max) d_max[o] = Q.vmax[i];
            if (d_avg) d_avg[o] = sm / (double)c;
        }
    }
}

// ---------------------------------------------------------------------------
// Kernel 3d, first/last resolve. The TS pass left, per group, the
// smallest and greatest timestamp of its surviving non-null rows. This kernel
// walks the rows once more under the same filter and dedup (row_alive,
// row_valid, hx_ptr) and, for every such row whose timestamp IS its group's
// extreme, atomicMax-es the value's ordered word into the group's output
// word: on a well-formed store one row per group and side gets there, and
// when two tie (the same PK surviving in two time segments) the
// totalOrder-greater value wins whatever the row order. Outputs are
// zero-filled by the host (the ordered identity of max).
// Group lookup: rows of a slice ascend by (series, ts), so by (series,
// bucket). Per 64-row window two wave-cooperative 64-ary lower bounds over
// the sorted group keys (first and last row of the window) bracket the
// window's groups; each lane finishes with a binary search inside the
// bracket. A row that finds no group is counted in Q.err and skipped.
// Reads: the slices' columns and bitmaps, [0, ng) of the group arrays.
// Writes: ofirst/olast[0, ng) and the error counter.
// ---------------------------------------------------------------------------
template <typename Less>
__device__ __forceinline__ uint32_t lb64_if(uint32_t n, int lane,
                                            Less lt_target) {
    uint32_t lo = 0, rem = n;
    while (rem > 0) {
        const uint32_t step = (rem + 63u) >> 6;
        const uint32_t p = lo + (uint32_t)lane * step;
        const bool in = (uint32_t)lane * step < rem;
        const bool t = in && lt_target(p);
        const uint32_t k = (uint32_t)__popcll(__ballot(t));
        if (k == 0) break;
        const uint32_t adv = (k - 1) * step + 1;
        lo += adv;
        rem = (step - 1u) < (rem - adv) ? (step - 1u) : (rem - adv);
    }
    return lo;   // first index whose key is not below the target (n if none)
}

template <bool NULLS>
__global__ void __launch_bounds__(256)
k_resolve_first_last(AggParams P, ResolveParams Q) {
    const int lane = threadIdx.x & 63;
    const uint32_t wave = threadIdx.x >> 6;
    const uint32_t n_waves = blockDim.x >> 6;
    const uint32_t ng = Q.ng;
    // group g's key < (s, b)?  g < ng at every call
    auto key_lt = [&](uint32_t g, uint64_t s, int64_t b) {
        const uint64_t ks = Q.gkey[g];
        if (ks != s) return ks < s;
        return Q.gbucket ? (Q.gbucket[g] < b) : false;
    };
    unsigned long long bad = 0;
    for (uint32_t rgi = blockIdx.x; rgi < P.n_rgs; rgi += gridDim.x) {
        const RgDesc rg = P.rgs[rgi];
        const uint64_t* S = (const uint64_t*)hx_ptr(P.blob, P.dec, rg.series_off);
        const int64_t* T = (const int64_t*)hx_ptr(P.blob, P.dec, rg.ts_off);
        const double* V = (const double*)hx_ptr(P.blob, P.dec, rg.val_off);
        const SstDev sst = P.ssts[rg.sst_id];
        const uint32_t n = rg.n_rows;
        for (uint32_t base = wave * 64u; base < n; base += n_waves * 64u) {
            const uint32_t r = base + (uint32_t)lane;
            const bool inb = r < n;
            uint64_t s = 0;
            int64_t t = 0;
            double v = 0.0;
            if (inb) {
                s = S[r];
                t = T[r];
                v = V[r];
            }
            bool alive = inb && row_alive(P, rg, sst, S, T, r, n, s, t);
            if (NULLS && alive) alive = row_valid(P, rgi, r);
            if (!__any(alive)) continue;   // wave-uniform
            const int64_t b = P.bucket_ms ? floordiv(t, P.bucket_ms) : 0;
            // bracket: the keys of the window's first and last row (alive or
            // not, they bound every row between them)
            const int last = (int)((n - base < 64u ? n - base : 64u) - 1u);
            const uint64_t sF = __shfl(s, 0, 64);
            const int64_t bF = __shfl((long long)b, 0, 64);
            const uint64_t sL = __shfl(s, last, 64);
            const int64_t bL = __shfl((long long)b, last, 64);
            const uint32_t g0 = lb64_if(
                ng, lane, [&](uint32_t p) { return key_lt(p, sF, bF); });
            const uint32_t g1 = lb64_if(
                ng, lane, [&](uint32_t p) { return key_lt(p, sL, bL); });
            if (!alive) continue;
            uint32_t lo = g0 < ng ? g0 : ng;
            uint32_t hi = g1 < ng ? g1 + 1u : ng;   // search [lo, hi)
            while (lo < hi) {
                const uint32_t mid = lo + ((hi - lo) >> 1);
                if (key_lt(mid, s, b)) lo = mid + 1u;
                else hi = mid;
            }
            const bool found = lo < ng && Q.gkey[lo] == s &&
                               (!Q.gbucket || Q.gbucket[lo] == b);
            if (!found) {   // the TS pass saw every row this pass sees
                bad++;
                continue;
            }
            const unsigned long long o = f64_ordered(v);
            if (Q.olast && t == Q.tmax[lo]) atomicMax(&Q.olast[lo], o);
            if (Q.ofirst && t == Q.tmin[lo]) atomicMax(&Q.ofirst[lo], o);
        }
    }
    if (bad) __hip_atomic_fetch_add(Q.err, bad, RLX, AGT);
}

// In-place word maps around kernel 3d. to_ts: a column the aggregate emit
// paths wrote through ordered_f64 holds the image of a time word; f64_ordered
// inverts that bijection exactly and the sign flip gives the i64 timestamp.
// Otherwise: ordered value words -> the f64 bit patterns they stand for.
// No floating-point arithmetic touches either.
extern "C" __global__ void __launch_bounds__(256)
k_map_words(unsigned long long* w, size_t n, uint32_t to_ts) {
    for (size_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += (size_t)blockDim.x * gridDim.x) {
        const unsigned long long u = w[i];
        w[i] = to_ts
            ? (f64_ordered(__longlong_as_double((long long)u)) ^
               0x8000000000000000ull)
            : (unsigned long long)__double_as_longlong(ordered_f64(u));
    }
}

// ---------------------------------------------------------------------------
// RLE_DICTIONARY decode (parquet-format Encodings.md "RLE/bit-packed
// hybrid"; the encoding config.rs:54-75 enables with dictionaries on).
// One workgroup per page: lane-serial run-header walk into LDS (varints are
// sequential), then threads expand runs in parallel through the dictionary.
// ---------------------------------------------------------------------------
#define RLED_MAX_RUNS 8192

extern "C" __global__ void __launch_bounds__(256)
k_decode_rledict(const uint8_t* __restrict__ blob, uint8_t* __restrict__ dec,
                 const RleDictPageDesc* __restrict__ pages, uint32_t n_pages,
                 unsigned long long* err_flag) {
    struct Run { uint32_t out_pos, count, byte_off, rle_val_or_flag; };
    __shared__ Run runs[RLED_MAX_RUNS];
    __shared__ int n_runs;
    __shared__ int hdr_err;
    __shared__ uint32_t bw_sh;
    for (uint32_t pg = blockIdx.x; pg < n_pages; pg += gridDim.x) {
        const RleDictPageDesc pd = pages[pg];
        const uint8_t* idx = ((pd.idx_off & OFF_DEC) ? dec : blob) +
                             (pd.idx_off & OFF_MASK);
        const uint64_t* dict = (const uint64_t*)(((pd.dict_off & OFF_DEC)
                                                      ? dec : blob) +
                                                 (pd.dict_off & OFF_MASK));
        uint64_t* dst = (uint64_t*)(dec + (pd.dst_off & OFF_MASK));
        if (threadIdx.x == 0) {
            hdr_err = 0;
            n_runs = 0;
            const uint32_t len = pd.idx_len;
            uint32_t pos = 0;
            uint32_t bw = (len > 0) ? idx[pos++] : 0xFF;
            bw_sh = bw;
            if (bw > 32) hdr_err = 1;
            uint32_t out = 0;
            while (!hdr_err && out < pd.n_values) {
                // varint header
                uint64_t hdrv = 0;
                int sh = 0;
                for (;;) {
                    if (pos >= len || sh > 28) { hdr_err = 2; break; }
                    uint8_t bb = idx[pos++];
                    hdrv |= (uint64_t)(bb & 0x7f) << sh;
                    if (!(bb & 0x80)) break;
                    sh += 7;
                }
                if (hdr_err) break;
                if (n_runs >= RLED_MAX_RUNS) { hdr_err = 3; break; }
                if (hdrv & 1) {  // bit-packed: (hdr>>1) groups of 8
                    uint32_t cnt = (uint32_t)(hdrv >> 1) * 8;
                    uint32_t nbytes = (uint32_t)(hdrv >> 1) * bw;
                    if (pos + nbytes > len) { hdr_err = 4; break; }
                    if (cnt > pd.n_values - out) cnt = pd.n_values - out;
                    runs[n_runs++] = {out, cnt, pos, 0x80000000u};
                    pos += nbytes;
                    out += cnt;
                } else {          // RLE run
                    uint32_t cnt = (uint32_t)(hdrv >> 1);
                    uint32_t vbytes = (bw + 7) / 8;
                    if (pos + vbytes > len) { hdr_err = 5; break; }
                    uint32_t v = 0;
                    for (uint32_t i = 0; i < vbytes; i++)
                        v |= (uint32_t)idx[pos + i] << (8 * i);
                    pos += vbytes;
                    if (cnt > pd.n_values - out) cnt = pd.n_values - out;
                    runs[n_runs++] = {out, cnt, 0, v};
                    out += cnt;
                }
            }
            if (!hdr_err && out < pd.n_values) hdr_err = 6;
        }
        __syncthreads();
        if (hdr_err) {
            if (threadIdx.x == 0) atomicAdd(err_flag, 1ull);
            __syncthreads();
            continue;
        }
        const uint32_t bw = bw_sh;
        const int nr = n_runs;
        for (int rI = 0; rI < nr; rI++) {
            const Run run = runs[rI];
            if (run.rle_val_or_flag != 0x80000000u) {  // RLE: broadcast
                const uint32_t v = run.rle_val_or_flag;
                if (v >= pd.dict_n) {
                    if (threadIdx.x == 0) atomicAdd(err_flag, 1ull);
                    break;
                }
                const uint64_t dv = dict[v];
                for (uint32_t i = threadIdx.x; i < run.count; i += blockDim.x)
                    dst[run.out_pos + i] = dv;
            } else {  // bit-packed: value i at bit i*bw
                bool bad = false;
                for (uint32_t i = threadIdx.x; i < run.count; i += blockDim.x) {
                    const uint64_t bitpos = (uint64_t)i * bw;
                    const uint8_t* base = idx + run.byte_off + (bitpos >> 3);
                    const int shift = (int)(bitpos & 7);
                    uint64_t window = 0;
                    for (int b2 = 0; b2 < 5; b2++)
                        window |= (uint64_t)base[b2] << (8 * b2);
                    uint32_t v = (uint32_t)((window >> shift) &
                                            ((bw < 32) ? ((1u << bw) - 1u)
                                                       : 0xFFFFFFFFu));
                    if (v >= pd.dict_n) { bad = true; break; }
                    dst[run.out_pos + i] = dict[v];
                }
                if (bad) {
                    atomicAdd(err_flag, 1ull);
                    break;
                }
            }
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------
// Streaming parity mode (hx_scan): emit the filtered, deduplicated rows
// themselves. Appends survivors (series, ts, value) unordered; the host then
// radix-sorts by (series, ts) — MergeStream's PK order (equal PKs cannot
// survive dedup, so no stability requirement remains).
// ---------------------------------------------------------------------------
struct ScanRowsParams {
    AggParams P;              // filter/dedup context (table unused)
    uint32_t rg_first, rg_last;   // process rgs [first, last) (one segment)
    uint64_t* out_series;
    long long* out_ts;
    double* out_value;
    uint64_t* out_seq;        // per-row __seq__ of survivors (nullable)
    int32_t seq_rowidx;       // 1: out_seq = (seq << 32) | staged row index
                              // — the Append sort key: equal-PK equal-seq
                              // rows keep FILE ROW ORDER (the writer's
                              // stable sort; MergeStream stream order)
    int32_t _pad;
    unsigned long long* cursor;
    unsigned long long cap;
    uint64_t* out_valid;      // 1 / 0 per survivor: value present (nullable;
                              // set when the plan staged a validity bitmap)
};

extern "C" __global__ void __launch_bounds__(256)
k_scan_rows(ScanRowsParams R) {
    const AggParams& P = R.P;
    for (uint32_t rgi = R.rg_first + blockIdx.x; rgi < R.rg_last;
         rgi += gridDim.x) {
        const RgDesc rg = P.rgs[rgi];
        const uint64_t* S = (const uint64_t*)hx_ptr(P.blob, P.dec, rg.series_off);
        const int64_t* T = (const int64_t*)hx_ptr(P.blob, P.dec, rg.ts_off);
        const double* V = (const double*)hx_ptr(P.blob, P.dec, rg.val_off);
        const SstDev sst = P.ssts[rg.sst_id];
        const uint32_t n = rg.n_rows;
        const int lane = threadIdx.x & 63;
        for (uint32_t base = 0; base < n; base += blockDim.x) {
            const uint32_t r = base + threadIdx.x;
            const bool inb = r < n;
            const int64_t t = inb ? T[r] : 0;
            const uint64_t s = inb ? S[r] : 0;
            const bool live = inb && row_alive(P, rg, sst, S, T, r, n, s, t);
            // one cursor atomic per wave (guideline 12)
            const unsigned long long mask = __ballot(live);
            if (!mask) continue;
            const int leader = __ffsll((unsigned long long)mask) - 1;
            unsigned long long wave_base = 0;
            if (lane == leader)
                wave_base = atomicAdd(R.cursor,
                                      (unsigned long long)__popcll(mask));
            wave_base = __shfl(wave_base, leader, 64);
            if (live) {
                const unsigned long long j =
                    wave_base + __popcll(mask & ((1ull << lane) - 1ull));
                if (j < R.cap) {
                    R.out_series[j] = s;
                    R.out_ts[j] = t;
                    R.out_value[j] = V[r];
                    if (R.out_valid)
                        R.out_valid[j] = row_valid(P, rgi, r) ? 1ull : 0ull;
                    if (R.out_seq) {
                        uint64_t q = row_seq(P, sst, rg, r);
                        R.out_seq[j] = R.seq_rowidx
                            ? (q << 32) |
                                  (uint64_t)(uint32_t)(rg.row_base + r)
                            : q;
                    }
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------
// Inverted-index query kernels (rfc:86-137): PLAIN BYTE_ARRAY offset walk,
// tag-equality postings filter, sorted-set intersection / adjacent-unique.
// All HBM-bound byte work; no MFMA.
// ---------------------------------------------------------------------------
extern "C" __global__ void __launch_bounds__(256)
k_ba_offsets(const uint8_t* __restrict__ blob,
             const BaPageDesc* __restrict__ pages, uint32_t n_pages,
             uint64_t* __restrict__ out, unsigned long long* err_flag) {
    // the length-prefixed layout is a serial chain per page; pages decode in
    // parallel (one thread walks one page: ~8192 values)
    const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t n_threads = gridDim.x * blockDim.x;
    for (uint32_t pg = tid; pg < n_pages; pg += n_threads) {
        const BaPageDesc pd = pages[pg];
        uint64_t pos = 0;
        bool bad = false;
        for (uint32_t i = 0; i < pd.n_values; i++) {
            if (pos + 4 > pd.src_len) { bad = true; break; }
            const uint8_t* p = blob + pd.src_off + pos;
            uint32_t len = (uint32_t)p[0] | ((uint32_t)p[1] << 8) |
                           ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
            pos += 4;
            if (len >= (1u << 20) || pos + len > pd.src_len) {
                bad = true;
                break;
            }
            out[pd.first_row + i] = ((pd.src_off + pos) << 20) | len;
            pos += len;
        }
        if (bad) atomicAdd(err_flag, 1ull);
    }
}

__device__ __forceinline__ bool bytes_eq(const uint8_t* a, const uint8_t* b,
                                         uint32_t n) {
    uint32_t i = 0;
    for (; i + 8 <= n; i += 8) {
        uint64_t x, y;
        __builtin_memcpy(&x, a + i, 8);
        __builtin_memcpy(&y, b + i, 8);
        if (x != y) return false;
    }
    for (; i < n; i++)
        if (a[i] != b[i]) return false;
    return true;
}

extern "C" __global__ void __launch_bounds__(256)
k_tag_filter(TagFilterParams F) {
    const int lane = threadIdx.x & 63;
    for (int64_t r = blockIdx.x * blockDim.x + threadIdx.x;
         __any(r < F.n_rows); r += (int64_t)blockDim.x * gridDim.x) {
        bool hit = false;
        uint64_t id = 0;
        if (r < F.n_rows) {
            const uint64_t ko = F.key_offlen[r];
            const uint32_t klen = (uint32_t)(ko & 0xFFFFFu);
            if (klen == F.pred_key_len &&
                bytes_eq(F.blob + (ko >> 20), F.pred_key, klen)) {
                const uint64_t vo = F.val_offlen[r];
                const uint32_t vlen = (uint32_t)(vo & 0xFFFFFu);
                if (vlen == F.pred_val_len &&
                    bytes_eq(F.blob + (vo >> 20), F.pred_val, vlen)) {
                    hit = true;
                    id = F.tsid[r];
                }
            }
        }
        const unsigned long long mask = __ballot(hit);
        if (!mask) continue;
        const int leader = __ffsll((unsigned long long)mask) - 1;
        unsigned long long base = 0;
        if (lane == leader)
            base = atomicAdd(F.cursor, (unsigned long long)__popcll(mask));
        base = __shfl(base, leader, 64);
        if (hit) {
            const unsigned long long j =
                base + __popcll(mask & ((1ull << lane) - 1ull));
            if (j < F.cap) F.out[j] = id;
        }
    }
}

// gather variable-length byte values: row i copies its bytes (handle =
// blob_off << 20 | len, from k_ba_offsets) to out[dst_off[i]..dst_off[i+1])
struct CopyBytesParams {
    const uint8_t* blob;
    const uint64_t* handles;    // per OUTPUT row, already permuted
    const int64_t* dst_off;     // n+1 prefix offsets into out
    uint8_t* out;
    uint32_t n;
};

extern "C" __global__ void __launch_bounds__(256)
k_copy_bytes(CopyBytesParams C) {
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < C.n;
         r += blockDim.x * gridDim.x) {
        const uint64_t h = C.handles[r];
        const uint8_t* src = C.blob + (h >> 20);
        const uint32_t len = (uint32_t)(h & 0xFFFFFu);
        uint8_t* dst = C.out + C.dst_off[r];
        for (uint32_t i = 0; i < len; i++) dst[i] = src[i];
    }
}

// sorted-set intersection: keep a[i] iff it appears in sorted b[0..n_b)
extern "C" __global__ void __launch_bounds__(256)
k_tsid_intersect(const uint64_t* __restrict__ a, unsigned long long n_a,
                 const uint64_t* __restrict__ b, unsigned long long n_b,
                 uint64_t* __restrict__ out, unsigned long long* cursor) {
    const int lane = threadIdx.x & 63;
    for (unsigned long long r = blockIdx.x * blockDim.x + threadIdx.x;
         __any(r < n_a); r += (unsigned long long)blockDim.x * gridDim.x) {
        bool hit = false;
        uint64_t v = 0;
        if (r < n_a) {
            v = a[r];
            unsigned long long lo = 0, hi = n_b;
            while (lo < hi) {
                unsigned long long mid = (lo + hi) >> 1;
                if (b[mid] < v) lo = mid + 1;
                else hi = mid;
            }
            hit = lo < n_b && b[lo] == v;
        }
        const unsigned long long mask = __ballot(hit);
        if (!mask) continue;
        const int leader = __ffsll((unsigned long long)mask) - 1;
        unsigned long long base = 0;
        if (lane == leader)
            base = atomicAdd(cursor, (unsigned long long)__popcll(mask));
        base = __shfl(base, leader, 64);
        if (hit)
            out[base + __popcll(mask & ((1ull << lane) - 1ull))] = v;
    }
}

// adjacent-unique over a SORTED array
extern "C" __global__ void __launch_bounds__(256)
k_unique_u64(const uint64_t* __restrict__ in, unsigned long long n,
             uint64_t* __restrict__ out, unsigned long long* cursor) {
    const int lane = threadIdx.x & 63;
    for (unsigned long long r = blockIdx.x * blockDim.x + threadIdx.x;
         __any(r < n); r += (unsigned long long)blockDim.x * gridDim.x) {
        const bool keep = (r < n) && (r == 0 || in[r] != in[r - 1]);
        const unsigned long long mask = __ballot(keep);
        if (!mask) continue;
        const int leader = __ffsll((unsigned long long)mask) - 1;
        unsigned long long base = 0;
        if (lane == leader)
            base = atomicAdd(cursor, (unsigned long long)__popcll(mask));
        base = __shfl(base, leader, 64);
        if (keep)
            out[base + __popcll(mask & ((1ull << lane) - 1ull))] = in[r];
    }
}

// ---------------------------------------------------------------------------
// Result compaction: live slots -> dense arrays (unsorted; host sorts with
// rocPRIM then gathers).
// ---------------------------------------------------------------------------
struct CompactParams {
    AggTable table;
    uint32_t n_slots;
    int32_t key_claim;
    int64_t bucket_ms;
    // direct-indexed bucket mode
    int64_t lo_bucket;
    uint32_t n_buckets;
    uint32_t bstride;
    const uint8_t* bstore;
    uint64_t* out_series;
    long long* out_bucket;
    double* out_sum;
    unsigned long long* out_cnt;
    double* out_min;
    double* out_max;
    unsigned long long* n_out;
};

// Sweep positions: one per slot, or (direct-indexed bucket mode) one per
// (slot, bucket) accumulator row.
__device__ __forceinline__ size_t compact_total(const CompactParams& C) {
    return C.n_buckets ? (size_t)C.n_slots * C.n_buckets : (size_t)C.n_slots;
}

__device__ __forceinline__ bool compact_live(const CompactParams& C,
                                             size_t p) {
    if (C.n_buckets) {  // direct-indexed bucket mode: p = (slot, bucket)
        const uint32_t slot_i = (uint32_t)(p / C.n_buckets);
        const uint64_t key = *(const uint64_t*)(
            C.table.slab + (size_t)slot_i * C.table.stride);
        return key != KEY_EMPTY &&
               *(const unsigned long long*)(C.bstore + p * C.bstride + 8) > 0;
    }
    const uint8_t* slot = C.table.slab + p * C.table.stride;
    return C.key_claim ? (*(const uint64_t*)slot != KEY_EMPTY)
                       : (*(const uint32_t*)slot == 2u);
}

// Write live position p as output group j.
__device__ __forceinline__ void compact_emit(const CompactParams& C,
                                             size_t p,
                                             unsigned long long j) {
    const uint8_t* acc;   // {sum, cnt[, min, max]} of this group
    if (C.n_buckets) {
        const uint32_t slot_i = (uint32_t)(p / C.n_buckets);
        C.out_series[j] = *(const uint64_t*)(
            C.table.slab + (size_t)slot_i * C.table.stride);
        C.out_bucket[j] = C.lo_bucket + (long long)(p % C.n_buckets);
        acc = C.bstore + p * C.bstride;
    } else {
        const uint8_t* slot = C.table.slab + p * C.table.stride;
        if (C.key_claim) {   // {key, sum, ...}
            C.out_series[j] = *(const uint64_t*)slot;
            acc = slot + 8;
        } else {   // {state, pad, series, bucket, sum, ...}
            C.out_series[j] = *(const uint64_t*)(slot + 8);
            if (C.bucket_ms) C.out_bucket[j] = *(const long long*)(slot + 16);
            acc = slot + 24;
        }
    }
    if (C.out_sum) C.out_sum[j] = *(const double*)acc;
    if (C.out_cnt) C.out_cnt[j] = *(const unsigned long long*)(acc + 8);
    if (C.out_min)
        C.out_min[j] = ordered_f64(*(const unsigned long long*)(acc + 16));
    if (C.out_max)
        C.out_max[j] = ordered_f64(*(const unsigned long long*)(acc + 24));
}

// Single-pass compaction: output positions reserved with one atomicAdd on
// n_out per live wave. The route for direct-indexed bucket tables, whose
// sweep walks slots x n_buckets positions at a low live fraction: few live
// waves, so few atomics, and sweeping twice measured slower.
extern "C" __global__ void __launch_bounds__(256)
k_compact(CompactParams C) {
    const int lane = threadIdx.x & 63;
    const size_t total = compact_total(C);
    const size_t stride = (size_t)blockDim.x * gridDim.x;
    for (size_t p = blockIdx.x * blockDim.x + threadIdx.x; __any(p < total);
         p += stride) {
        const bool live = p < total && compact_live(C, p);
        const unsigned long long mask = __ballot(live);
        if (!mask) continue;
        // first live lane reserves for the wave
        const int leader = __ffsll(mask) - 1;
        unsigned long long wave_base = 0;
        if (lane == leader)
            wave_base = atomicAdd(C.n_out, (unsigned long long)__popcll(mask));
        wave_base = __shfl(wave_base, leader, 64);
        if (live)
            compact_emit(C, p,
                         wave_base + __popcll(mask & ((1ull << lane) - 1ull)));
    }
}

// ---- two-phase compaction (non-bucket slab/state tables) ------------------
// k_compact reserves output positions with one agent-scope atomicAdd per
// live wave on ONE counter word. At headline fill (10M live in a 16M-slot
// table) that is ~250k serialized hot-word RMWs ≈ 2.8 ms — the same
// coherence-point storm the scan kernel's fill counter had (§9c). The
// two-phase form removes the hot word entirely: per-block live counts
// (no atomics), a one-block exclusive scan, then an atomic-free write pass
// positioned by block base + LDS-local offset. Sweep traffic is paid twice
// but is only ~0.5 GB at headline size.

extern "C" __global__ void __launch_bounds__(256)
k_compact_count(CompactParams C, uint32_t* __restrict__ counts) {
    __shared__ uint32_t wsum[4];
    const size_t total = compact_total(C);
    const size_t chunk = (total + gridDim.x - 1) / gridDim.x;
    const size_t beg = blockIdx.x * chunk;
    const size_t end = beg + chunk < total ? beg + chunk : total;
    uint32_t cnt = 0;
    for (size_t i0 = beg; i0 < end; i0 += blockDim.x) {
        const size_t i = i0 + threadIdx.x;
        const bool live = i < end && compact_live(C, i);
        const unsigned long long m = __ballot(live);
        if ((threadIdx.x & 63) == 0) cnt += (uint32_t)__popcll(m);
    }
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0)
        counts[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// One-block exclusive scan of <=2048 per-block counts -> bases + total.
extern "C" __global__ void __launch_bounds__(256)
k_scan_counts(const uint32_t* __restrict__ counts, uint32_t nb,
              uint32_t* __restrict__ bases,
              unsigned long long* __restrict__ n_out) {
    __shared__ uint32_t tsum[256];
    const uint32_t per = (nb + 255) / 256;
    const uint32_t b0 = threadIdx.x * per;
    const uint32_t b1 = b0 + per < nb ? b0 + per : nb;
    uint32_t s = 0;
    for (uint32_t j = b0; j < b1; j++) s += counts[j];
    tsum[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t acc = 0;
        for (int t = 0; t < 256; t++) {
            const uint32_t v = tsum[t];
            tsum[t] = acc;
            acc += v;
        }
        *n_out = acc;
    }
    __syncthreads();
    uint32_t acc = tsum[threadIdx.x];
    for (uint32_t j = b0; j < b1; j++) {
        bases[j] = acc;
        acc += counts[j];
    }
}

extern "C" __global__ void __launch_bounds__(256)
k_compact_write(CompactParams C, const uint32_t* __restrict__ bases) {
    __shared__ uint32_t blk_off;
    if (threadIdx.x == 0) blk_off = 0;
    __syncthreads();
    const size_t total = compact_total(C);
    const size_t chunk = (total + gridDim.x - 1) / gridDim.x;
    const size_t beg = blockIdx.x * chunk;
    const size_t end = beg + chunk < total ? beg + chunk : total;
    const unsigned long long base = bases[blockIdx.x];
    const int lane = threadIdx.x & 63;
    for (size_t i0 = beg; i0 < end; i0 += blockDim.x) {
        const size_t i = i0 + threadIdx.x;
        const bool live = i < end && compact_live(C, i);
        const unsigned long long mask = __ballot(live);
        if (!mask) continue;
        const int leader = __ffsll((unsigned long long)mask) - 1;
        uint32_t wave_base = 0;
        if (lane == leader)
            wave_base = atomicAdd(&blk_off, (uint32_t)__popcll(mask));
        wave_base = __shfl(wave_base, leader, 64);
        if (live)
            compact_emit(C, i,
                         base + wave_base +
                             __popcll(mask & ((1ull << lane) - 1ull)));
    }
}

// Gather 8-byte elements by permutation (applies the sort order).
struct GatherMulti {
    const unsigned long long* src[8];
    unsigned long long* dst;   // dst array a at dst + a*n
    const uint32_t* perm;
    uint32_t n;
    uint32_t n_arrays;
};

extern "C" __global__ void __launch_bounds__(256)
k_gather_multi(GatherMulti g) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < g.n;
         i += blockDim.x * gridDim.x) {
        const uint32_t p = g.perm[i];
        for (uint32_t a = 0; a < g.n_arrays; a++)
            g.dst[(size_t)a * g.n + i] = g.src[a][p];
    }
}

extern "C" __global__ void __launch_bounds__(256)
k_gather_u64(const unsigned long long* in, const uint32_t* perm,
             unsigned long long* out, uint32_t n) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += blockDim.x * gridDim.x)
        out[i] = in[perm[i]];
}

extern "C" __global__ void __launch_bounds__(256)
k_avg(const double* sum, const unsigned long long* cnt, double* avg, uint32_t n) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += blockDim.x * gridDim.x)
        avg[i] = sum[i] / (double)cnt[i];
}

// ---------------------------------------------------------------------------
// Dense materialization (overlap path / streaming mode): copy staged PLAIN
// page payloads into dense 8B arrays. One unit per page, grid-stride.
// ---------------------------------------------------------------------------
extern "C" __global__ void __launch_bounds__(256)
k_copy_u64(const uint8_t* blob, const uint8_t* dec_in, uint8_t* dec,
           const CopyDesc* descs, uint32_t n_descs) {
    for (uint32_t d = blockIdx.x; d < n_descs; d += gridDim.x) {
        CopyDesc c = descs[d];
        const uint64_t* src = (const uint64_t*)hx_ptr(blob, dec_in, c.src_off);
        uint64_t* dst = (uint64_t*)(dec + (c.dst_off & OFF_MASK));
        for (uint32_t i = threadIdx.x; i < c.n_values; i += blockDim.x)
            dst[i] = src[i];
    }
}

// ---------------------------------------------------------------------------
// OPTIONAL-column PLAIN pages (DESIGN §4 kernel 1c). Two things keep such a
// page from being read in place. A v1 page that went through the Snappy
// decoder sits in dec as {level block, values}; the block is 6-8 bytes for a
// page without nulls, so the values start at a byte offset that is not a
// multiple of 8. And a page with nulls stores only its n_valid present
// values, packed. One workgroup per page writes the dense, 64-byte-aligned
// n_rows column the scan kernels index by row:
//   * no bitmap: rank(r) = r, a realigning copy;
//   * bitmap: tiles of 8192 rows = 128 words; popcount per word, exclusive
//     scan over the tile in LDS, rank carried from tile to tile; a valid row
//     gathers packed[rank], a null row stores 0.
// A packed value is read as the two ALIGNED words that straddle it,
// funnel-shifted together (no unaligned 8-byte load); the value whose upper
// word would reach past the page is assembled from bytes, so nothing outside
// [src, src + src_len) is read, and a rank at or above n_valid is never
// followed. Stores are 8 B per lane, coalesced. A descriptor that does not
// fit its source, is not 8-byte aligned, or whose bitmap disagrees with
// n_valid counts one decode error (the exec then fails with HX_ERR_FORMAT);
// in the first two cases nothing is written.
// ---------------------------------------------------------------------------
#define EXPAND_TILE_WORDS 128u   // 8192 rows

__device__ __forceinline__ uint64_t packed_u64(const uint8_t* body,
                                               uint32_t mis, uint64_t w_base,
                                               uint32_t src_len, uint32_t k) {
    const uint64_t* w = (const uint64_t*)(body - mis);
    if (mis == 0) return w[k];
    if (w_base + 8ull * (k + 2) <= src_len)
        return (w[k] >> (mis * 8u)) | (w[k + 1] << (64u - mis * 8u));
    uint64_t v = 0;
    for (int b = 0; b < 8; b++)
        v |= (uint64_t)body[8ull * k + b] << (8 * b);
    return v;
}

extern "C" __global__ void __launch_bounds__(256)
k_expand_optional(const uint8_t* blob, const uint8_t* dec_in, uint8_t* dec,
                  const ExpandPageDesc* __restrict__ pages, uint32_t n_pages,
                  unsigned long long* err_flag) {
    __shared__ uint32_t wrank[EXPAND_TILE_WORDS];   // exclusive, within tile
    __shared__ uint32_t tile_total;
    for (uint32_t pg = blockIdx.x; pg < n_pages; pg += gridDim.x) {
        const ExpandPageDesc pd = pages[pg];
        if ((uint64_t)pd.lvl_bytes + (uint64_t)pd.n_valid * 8 > pd.src_len ||
            ((pd.src_off | pd.dst_off | pd.bitmap_off) & 7u) ||
            pd.n_valid > pd.n_rows ||
            (!pd.bitmap_off && pd.n_valid != pd.n_rows)) {
            if (threadIdx.x == 0) atomicAdd(err_flag, 1ull);
            continue;
        }
        const uint8_t* body = hx_ptr(blob, dec_in, pd.src_off) + pd.lvl_bytes;
        uint64_t* dst = (uint64_t*)(dec + (pd.dst_off & OFF_MASK));
        // src_off is 8-aligned, so the misalignment is lvl_bytes & 7 and the
        // aligned-down start lies inside the page
        const uint32_t mis = pd.lvl_bytes & 7u;
        const uint64_t w_base = pd.lvl_bytes - mis;  // byte offset of word 0
        if (!pd.bitmap_off) {
            for (uint32_t i = threadIdx.x; i < pd.n_rows; i += blockDim.x)
                dst[i] = packed_u64(body, mis, w_base, pd.src_len, i);
            continue;
        }
        const uint64_t* bm = (const uint64_t*)(blob + pd.bitmap_off);
        const uint32_t n_words = (pd.n_rows + 63u) >> 6;
        uint32_t carry = 0;       // valid rows before this tile
        bool bad = false;
        for (uint32_t w0 = 0; w0 < n_words; w0 += EXPAND_TILE_WORDS) {
            const uint32_t tw = n_words - w0 < EXPAND_TILE_WORDS
                                    ? n_words - w0 : EXPAND_TILE_WORDS;
            __syncthreads();   // previous tile's wrank fully consumed
            if (threadIdx.x < EXPAND_TILE_WORDS) {
                uint64_t wv = threadIdx.x < tw ? bm[w0 + threadIdx.x] : 0ull;
                // bits at and above n_rows do not count
                const uint32_t row0 = (w0 + threadIdx.x) << 6;
                if (threadIdx.x < tw && pd.n_rows - row0 < 64u)
                    wv &= (1ull << (pd.n_rows - row0)) - 1ull;
                wrank[threadIdx.x] = (uint32_t)__popcll(wv);
            }
            __syncthreads();
            // inclusive Hillis-Steele scan over the 128 counts
            for (uint32_t d = 1; d < EXPAND_TILE_WORDS; d <<= 1) {
                uint32_t add = 0;
                if (threadIdx.x < EXPAND_TILE_WORDS && threadIdx.x >= d)
                    add = wrank[threadIdx.x - d];
                __syncthreads();
                if (threadIdx.x < EXPAND_TILE_WORDS) wrank[threadIdx.x] += add;
                __syncthreads();
            }
            if (threadIdx.x == 0) tile_total = wrank[EXPAND_TILE_WORDS - 1];
            __syncthreads();
            const uint32_t r_end = (w0 + tw) << 6 < pd.n_rows
                                       ? (w0 + tw) << 6 : pd.n_rows;
            for (uint32_t r = (w0 << 6) + threadIdx.x; r < r_end;
                 r += blockDim.x) {
                const uint32_t wi = (r >> 6) - w0;
                const uint64_t wv = bm[w0 + wi];
                uint64_t v = 0;
                if ((wv >> (r & 63u)) & 1ull) {
                    const uint32_t before =
                        (uint32_t)__popcll(wv & ((1ull << (r & 63u)) - 1ull));
                    // exclusive rank of the word = inclusive - its own count
                    const uint32_t own = (uint32_t)__popcll(
                        (r | 63u) < pd.n_rows
                            ? wv
                            : wv & ((1ull << (pd.n_rows & 63u)) - 1ull));
                    const uint32_t k = carry + wrank[wi] - own + before;
                    if (k < pd.n_valid)
                        v = packed_u64(body, mis, w_base, pd.src_len, k);
                    else
                        bad = true;
                }
                dst[r] = v;
            }
            carry += tile_total;
        }
        // the bitmap must account for exactly the packed values
        if (threadIdx.x == 0 && carry != pd.n_valid) bad = true;
        if (bad) atomicAdd(err_flag, 1ull);
    }
}

// ---------------------------------------------------------------------------
// Kernel 1d: the inverse of kernel 1c, fused with the last gather
// of the row-stream pipeline. One workgroup per OUTPUT row group g of R rows
// (R a multiple of 64): output row i = g * R + r is source row perm[i] (i when
// perm is null). A wave64 ballot of "row present" is one bitmap word; the
// words' popcounts go through the same LDS scan as kernel 1c (tiles of 128
// words, rank carried from tile to tile), and a present row stores its value
// at packed_out[g * R + rank]. The tile's words stay in LDS, so the validity
// source is gathered once per row; perm is read a second time (coalesced) for
// the value gather. A block writes its own row group's slots only: plain
// stores, no atomics but the error counter. Validity source: one 0/1 word
// per source row (k_scan_rows' out_valid), or an LSB-first bitmap read by
// bytes (nothing past ceil(n_src / 8) bytes is touched); null = all present.
// A perm entry >= n_src counts one error and its row is written as null.
// All R / 64 bitmap words of a row group are written, the ones past a short
// last row group as zero.
// ---------------------------------------------------------------------------
template <bool BITS>
__global__ void __launch_bounds__(256)
k_pack_optional(const unsigned long long* __restrict__ val_src,
                const void* __restrict__ valid_src,
                const uint32_t* __restrict__ perm, uint32_t n_src, uint32_t n,
                uint32_t R, unsigned long long* __restrict__ packed_out,
                uint64_t* __restrict__ bitmap_out,
                uint32_t* __restrict__ n_valid,
                unsigned long long* err_flag) {
    __shared__ uint64_t words[EXPAND_TILE_WORDS];
    __shared__ uint32_t wrank[EXPAND_TILE_WORDS];   // inclusive, within tile
    __shared__ uint32_t tile_total;
    const uint32_t wpg = R >> 6;
    const uint32_t n_groups = (uint32_t)(((uint64_t)n + R - 1) / R);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint32_t g = blockIdx.x; g < n_groups; g += gridDim.x) {
        const uint64_t row0 = (uint64_t)g * R;
        const uint32_t rows =
            (uint64_t)n - row0 < R ? (uint32_t)(n - row0) : R;
        uint32_t carry = 0;       // present rows before this tile
        for (uint32_t w0 = 0; w0 < wpg; w0 += EXPAND_TILE_WORDS) {
            const uint32_t tw = wpg - w0 < EXPAND_TILE_WORDS
                                    ? wpg - w0 : EXPAND_TILE_WORDS;
            __syncthreads();   // previous tile's words/wrank fully consumed
            for (uint32_t wi = wave; wi < EXPAND_TILE_WORDS; wi += 4) {
                bool present = false;
                const uint32_t r = ((w0 + wi) << 6) + lane;
                if (wi < tw && r < rows) {
                    const uint32_t p =
                        perm ? perm[row0 + r] : (uint32_t)(row0 + r);
                    if (p >= n_src)
                        atomicAdd(err_flag, 1ull);
                    else if (!valid_src)
                        present = true;
                    else if (BITS)
                        present = (((const uint8_t*)valid_src)[p >> 3] >>
                                   (p & 7u)) & 1u;
                    else
                        present = ((const uint64_t*)valid_src)[p] != 0;
                }
                const uint64_t m = __ballot(present);
                if (lane == 0) {
                    words[wi] = m;
                    wrank[wi] = (uint32_t)__popcll(m);
                    if (wi < tw) bitmap_out[(uint64_t)g * wpg + w0 + wi] = m;
                }
            }
            __syncthreads();
            // inclusive Hillis-Steele scan over the 128 counts
            for (uint32_t d = 1; d < EXPAND_TILE_WORDS; d <<= 1) {
                uint32_t add = 0;
                if (threadIdx.x < EXPAND_TILE_WORDS && threadIdx.x >= d)
                    add = wrank[threadIdx.x - d];
                __syncthreads();
                if (threadIdx.x < EXPAND_TILE_WORDS) wrank[threadIdx.x] += add;
                __syncthreads();
            }
            if (threadIdx.x == 0) tile_total = wrank[EXPAND_TILE_WORDS - 1];
            __syncthreads();
            const uint32_t r_end = (w0 + tw) << 6 < rows ? (w0 + tw) << 6
                                                         : rows;
            for (uint32_t r = (w0 << 6) + threadIdx.x; r < r_end;
                 r += blockDim.x) {
                const uint32_t wi = (r >> 6) - w0;
                const uint64_t wv = words[wi];
                if ((wv >> (r & 63u)) & 1ull) {
                    const uint32_t before =
                        (uint32_t)__popcll(wv & ((1ull << (r & 63u)) - 1ull));
                    // exclusive rank of the word = inclusive - its own count
                    const uint32_t k = carry + wrank[wi] -
                                       (uint32_t)__popcll(wv) + before;
                    // a set bit means p < n_src was checked above
                    const uint32_t p =
                        perm ? perm[row0 + r] : (uint32_t)(row0 + r);
                    packed_out[row0 + k] = val_src[p];
                }
            }
            carry += tile_total;
        }
        if (threadIdx.x == 0) n_valid[g] = carry;
    }
}

// ---------------------------------------------------------------------------
// Snappy raw-block decompression (the reference's default page codec,
// config.rs:120-133). One WAVE per page: the tag stream is inherently
// sequential, so every lane parses the (wave-uniform) element headers and
// the 64 lanes copy the element's bytes cooperatively. Overlapping copies
// (offset < length) use the periodic-pattern equivalence of the sequential
// byte copy. Parallelism comes from the page count (~one 64KB page per
// 8192-row column chunk).
// ---------------------------------------------------------------------------
__device__ __forceinline__ uint32_t snappy_varint(const uint8_t* p,
                                                  uint32_t& pos, uint32_t len,
                                                  int* err) {
    uint32_t r = 0;
    int s = 0;
    for (;;) {
        if (pos >= len || s > 28) { *err = 1; return 0; }
        uint8_t b = p[pos++];
        r |= (uint32_t)(b & 0x7f) << s;
        if (!(b & 0x80)) return r;
        s += 7;
    }
}

// Per-wave LDS mirror of the most recent output bytes: back-references with
// offset <= SNAP_MIRROR read the mirror (LDS, wave-ordered) instead of the
// global dst — the old kernel drained ALL outstanding stores
// (`s_waitcnt vmcnt(0)`, ~600-900 cycles) before EVERY match, and the
// ts/series pages of PLAIN metric data are nothing but small periodic
// matches (measured 94 ms/step at the 1B snappy shape, ~4x the aggregate
// kernel). Offsets beyond the mirror still take the drained global path.
// Snappy decode, fourth design. The decode loop is VALU-ISSUE-BOUND: a
// ts/series page is thousands of tiny matches, and each one paid ~500
// instructions of copy setup, exec-mask bookkeeping and flush checks (the
// memory-level rewrites v2/v3 moved the bytes into LDS and changed almost
// nothing). Two levers here:
//   1. FUSE runs of same-offset matches at parse time: periodic metric
//      columns compress into long chains of off=8/16 matches whose fused
//      form is ONE long periodic copy — the per-tag cost drops to the bare
//      parse (~40 instructions), the copy amortizes over the fused length;
//   2. 4 KB LDS output ring per wave (16 KB per 256-thread block => full
//      32-wave occupancy), flushed to HBM in coalesced spans; matches read
//      the ring, never global dst (no vmcnt round trips).
//   3. DIRECT runs: where a run's output is a function of a few registers
//      it is stored straight to dst, 16 B per lane, and never round-trips
//      through the ring: pair runs ([x, x] per pair, taken when d is
//      8-aligned) and fused same-offset runs with off in {1,2,4,8,16} of at
//      least SNAP_DIRECT_MIN bytes (one 16-byte pattern, any d: the ragged
//      ends up to the 16-aligned middle go out as bytes). Huge literals
//      copy src -> dst the same way.
// RING INVARIANT, which every direct path restores before the element loop
// continues: flushed == d; the ring holds the valid output bytes of
// [max(0, d - SNAP_RING), d) (direct paths mirror their last SNAP_RING bytes
// with wide LDS stores); tail0/tail1/pend are reloaded from the ring
// (rwin_reload). Back-references up to SNAP_RING / 2 read the ring, longer
// ones the drained global path. No path reads past comp_len or writes past
// uncomp_len; a malformed stream bumps err_flag.
#define SNAP_RING 4096u
// fused same-offset runs at least this long bypass the ring (direct stores)
#define SNAP_DIRECT_MIN 256u

struct SnapStream {
    const uint64_t* words;   // aligned view of the page payload
    uint64_t w0, w1, w2;     // words [wi, wi+3)
    uint32_t wi;             // aligned word index of w0
    uint32_t n_words;        // ceil(payload/8) — loads are clamped

    __device__ void init(const uint8_t* src, uint32_t clen) {
        words = (const uint64_t*)src;
        n_words = (clen + 7u) >> 3;
        wi = 0;
        w0 = n_words > 0 ? words[0] : 0;
        w1 = n_words > 1 ? words[1] : 0;
        w2 = n_words > 2 ? words[2] : 0;
    }
    __device__ __forceinline__ void advance_to(uint32_t pos) {
        const uint32_t target = pos >> 3;
        if (target >= wi + 3) {  // long jump (after a big literal): reseat
            wi = target;
            w0 = wi < n_words ? words[wi] : 0;
            w1 = wi + 1 < n_words ? words[wi + 1] : 0;
            w2 = wi + 2 < n_words ? words[wi + 2] : 0;
            return;
        }
        while (target > wi) {
            wi++;
            w0 = w1;
            w1 = w2;
            w2 = (wi + 2 < n_words) ? words[wi + 2] : 0;
        }
    }
    // 8 bytes starting at byte `pos` (pos in [wi*8, wi*8+8))
    __device__ __forceinline__ uint64_t peek8(uint32_t pos) {
        const uint32_t sh = (pos & 7u) * 8u;
        return sh ? ((w0 >> sh) | (w1 << (64 - sh))) : w0;
    }
};

// flush ring bytes [f, f+len) to dst: 16 B per lane while the ring offset
// and the dst offset are both 16-aligned (dst itself is 64-aligned), then
// coalesced u32 stores when everything left is 4-aligned, else bytes. Ring
// spans wrap at SNAP_RING.
__device__ __forceinline__ void snap_flush(uint8_t* __restrict__ dst,
                                           const uint8_t* ring, uint32_t f,
                                           uint32_t len, uint32_t lane) {
    while (len) {
        uint32_t r0 = f & (SNAP_RING - 1);
        uint32_t span = min(len, SNAP_RING - r0);
        len -= span;
        if (((r0 | f) & 15u) == 0 && span >= 16u) {
            const uint32_t n16 = span >> 4;
            for (uint32_t i = lane; i < n16; i += 64)
                *(ulonglong2*)(dst + f + 16 * i) =
                    *(const ulonglong2*)(ring + r0 + 16 * i);
            r0 += n16 << 4;
            f += n16 << 4;
            span -= n16 << 4;
        }
        if ((r0 & 3u) == 0 && (f & 3u) == 0 && (span & 3u) == 0) {
            const uint32_t words = span >> 2;
            for (uint32_t i = lane; i < words; i += 64) {
                uint32_t v;
                __builtin_memcpy(&v, ring + r0 + 4 * i, 4);
                *(uint32_t*)(dst + f + 4 * i) = v;
            }
        } else {
            for (uint32_t i = lane; i < span; i += 64)
                dst[f + i] = ring[r0 + i];
        }
        f += span;
    }
}

// Byte a (0..15) of a 16-byte pattern held as two LE u64 halves.
__device__ __forceinline__ uint8_t snap_qbyte(uint64_t q0, uint64_t q1,
                                              uint32_t a) {
    return (uint8_t)(((a & 8u) ? q1 : q0) >> (8u * (a & 7u)));
}

// Write output bytes [A, B) of a 16-periodic run, out[a] = Q[a & 15], to
// `base` (dst, or the ring with MASK = SNAP_RING - 1): bytes up to the
// first 16-aligned position, 16 B per lane over the aligned middle, bytes
// after it. Correct for any A, B; base + (a & MASK) is 16-aligned whenever
// a is.
template <uint32_t MASK>
__device__ __forceinline__ void snap_emit_q(uint8_t* base, uint32_t A,
                                            uint32_t B, uint64_t q0,
                                            uint64_t q1, uint32_t lane) {
    uint32_t A16 = (A + 15u) & ~15u;
    uint32_t B16 = B & ~15u;
    if (A16 >= B16) A16 = B16 = B;   // no aligned middle: all bytes
    for (uint32_t a = A + lane; a < A16; a += 64)
        base[a & MASK] = snap_qbyte(q0, q1, a & 15u);
    const ulonglong2 q = make_ulonglong2(q0, q1);
    for (uint32_t a = A16 + 16u * lane; a < B16; a += 1024u)
        *(ulonglong2*)(base + (a & MASK)) = q;
    for (uint32_t a = B16 + lane; a < B; a += 64)
        base[a & MASK] = snap_qbyte(q0, q1, a & 15u);
}

template <int MINW>
__global__ void __launch_bounds__(256, MINW)
k_snappy_decompress(const uint8_t* __restrict__ blob, uint8_t* __restrict__ dec,
                    const SnappyPageDesc* __restrict__ pages, uint32_t n_pages,
                    unsigned long long* err_flag) {
    __shared__ __attribute__((aligned(16))) uint8_t ring_all[4][SNAP_RING];
    const uint32_t lane = threadIdx.x & 63;
    uint8_t* const ring = ring_all[(threadIdx.x >> 6) & 3];
    const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint32_t n_waves = (gridDim.x * blockDim.x) >> 6;
    for (uint32_t pg = wave; pg < n_pages; pg += n_waves) {
        const SnappyPageDesc pd = pages[pg];
        const uint8_t* src = blob + (pd.src_off & OFF_MASK);
        uint8_t* dst = dec + (pd.dst_off & OFF_MASK);
        const uint32_t clen = pd.comp_len;
        int err = 0;
        SnapStream st;
        st.init(src, clen);
        uint32_t pos = 0;
        uint64_t v = st.peek8(0);
        uint32_t ulen = 0;
        {
            int sh = 0;
            for (;;) {
                if (pos >= clen || sh > 28 || pos >= 7) { err = 1; break; }
                uint8_t b = (uint8_t)(v >> (8 * pos));
                ulen |= (uint32_t)(b & 0x7f) << sh;
                pos++;
                if (!(b & 0x80)) break;
                sh += 7;
            }
        }
        if (err || ulen != pd.uncomp_len) {
            if (lane == 0) atomicAdd(err_flag, 1ull);
            continue;
        }
        uint32_t d = 0;        // output cursor
        uint32_t flushed = 0;  // dst bytes already written
        // Register sliding window (v5 fast path): series pages are 8k
        // ALTERNATING {7-byte literal, off=8 match} elements per page —
        // per-element cost must be tens of instructions, not hundreds.
        // tail0 = output[d-8, d), tail1 = output[d-16, d-8) (LE-packed);
        // pend accumulates the aligned 8-byte word at (d & ~7), written
        // with ONE ds_write_b64 per 8 output bytes. Writing the full pend
        // word early is safe: the slop bytes at [d, dA+8) sit beyond the
        // cursor in the ring and are rewritten before any flush reads them.
        uint64_t tail0 = 0, tail1 = 0, pend = 0;
        const uint64_t* const ring64 = (const uint64_t*)ring;
        // append n (1..8) bytes (LE in low bytes of nv) to the output
        auto rwin_append = [&](uint64_t nv, uint32_t n) {
            const uint32_t sh = 8u * n;
            if (n == 8) {
                tail1 = tail0;
                tail0 = nv;
            } else {
                tail1 = (tail1 >> sh) | (tail0 << (64 - sh));
                tail0 = (tail0 >> sh) | (nv << (64 - sh));
            }
            const uint32_t a = d & 7u;
            pend |= nv << (8u * a);   // a == 0 shifts by 0
            if (a + n >= 8) {
                if (lane == 0)
                    *(uint64_t*)(ring + ((d - a) & (SNAP_RING - 1) & ~7u)) =
                        pend;
                pend = a ? (nv >> (8u * (8u - a))) : 0;
            }
            d += n;
        };
        // spill the pending partial word (slop-safe) before any path that
        // reads/writes the ring directly or flushes
        auto rwin_spill = [&]() {
            if ((d & 7u) && lane == 0)
                *(uint64_t*)(ring + (d & (SNAP_RING - 1) & ~7u)) = pend;
        };
        // reload tail/pend from the ring after direct-ring paths
        auto rwin_reload = [&]() {
            const uint32_t a = d & 7u;
            const uint32_t base = (d - a) & (SNAP_RING - 1);
            const uint64_t w0 = ring64[base >> 3];
            const uint64_t w1 = ring64[((base + SNAP_RING - 8) &
                                        (SNAP_RING - 1)) >> 3];
            const uint64_t w2 = ring64[((base + SNAP_RING - 16) &
                                        (SNAP_RING - 1)) >> 3];
            if (a == 0) {
                pend = 0;
                tail0 = w1;
                tail1 = w2;
            } else {
                const uint32_t sh = 8u * a;
                pend = w0 & ((1ull << sh) - 1u);
                tail0 = (w1 >> sh) | (w0 << (64 - sh));
                tail1 = (w2 >> sh) | (w1 << (64 - sh));
            }
        };
        while (pos < clen && d < ulen && !err) {
            st.advance_to(pos);
            v = st.peek8(pos);
            uint32_t tag = (uint32_t)(v & 0xFFu);
            uint32_t kind = tag & 3u;
            // ---- v6 BULK-PAIR path: series pages are runs of the exact
            // 10-byte pair {lit7 (tag 0x18), match off=8 len=9 (tag 0x15,
            // off byte 0x08)} — 16 output bytes per pair, and the pair's
            // output is [b0..b6, p, b0..b6, p] where p = the byte at d-1,
            // INVARIANT across the run (the off-8 source telescopes).
            // 64 lanes decode 64 pairs per wave iteration: the serial
            // element loop costs ~500 instructions per element; this path
            // costs ~2.
            if (tag == 0x18u && d >= 1 && pos + 10 <= clen) {
                rwin_spill();
                const uint8_t pbyte =
                    ring[(d - 1) & (SNAP_RING - 1)];
                uint32_t consumed = 0;
                // d 8-aligned (the data shape: an 8-byte literal, then 16
                // bytes per pair): DIRECT mode — each lane builds its pair's
                // 8 output bytes x in a register and stores [x, x] straight
                // to dst (16 B per lane, 1 KB per wave iteration) and, with
                // two 8-byte LDS stores, to the ring mirror; flushed tracks
                // d, so no flush/room bookkeeping. Any other alignment keeps
                // the ring path below.
                const bool direct = (d & 7u) == 0;
                for (;;) {
                    const uint32_t pp = pos + 10u * lane;
                    bool ok = pp + 10 <= clen &&
                              d + 16u * (lane + 1u) <= ulen;
                    // the pair's 10 bytes: one 8-byte and one 2-byte load
                    // (in bounds: pp + 10 <= clen)
                    uint64_t w = 0;
                    if (ok) {
                        uint16_t t2;
                        __builtin_memcpy(&w, src + pp, 8);
                        __builtin_memcpy(&t2, src + pp + 8, 2);
                        ok = (w & 0xFFu) == 0x18u && t2 == 0x0815u;
                    }
                    const unsigned long long bm = __ballot(ok);
                    const uint32_t m =
                        (~bm == 0ull) ? 64u
                                      : (uint32_t)(__ffsll((long long)~bm) - 1);
                    if (m == 0) break;
                    if (direct) {
                        if (consumed == 0) {
                            snap_flush(dst, ring, flushed, d - flushed, lane);
                            flushed = d;
                        }
                        if (lane < m) {
                            const uint64_t x =
                                (w >> 8) | ((uint64_t)pbyte << 56);
                            const uint32_t base = d + 16u * lane;
                            if ((d & 15u) == 0) {
                                *(ulonglong2*)(dst + base) =
                                    make_ulonglong2(x, x);
                            } else {
                                // d = 8 mod 16: two 8-byte stores (rotating
                                // 16 B chunks through the neighbour lane
                                // measured no faster, profiles/README.md)
                                *(uint64_t*)(dst + base) = x;
                                *(uint64_t*)(dst + base + 8) = x;
                            }
                            *(uint64_t*)(ring + (base & (SNAP_RING - 1))) = x;
                            *(uint64_t*)(ring +
                                         ((base + 8) & (SNAP_RING - 1))) = x;
                        }
                        d += 16u * m;
                        flushed = d;
                        pos += 10u * m;
                        consumed += m;
                        if (m < 64u) break;
                        continue;
                    }
                    uint8_t b[7];
                    for (int k = 0; k < 7; k++)
                        b[k] = (uint8_t)(w >> (8 * (k + 1)));
                    // ring room for 16*m bytes (+8 slop margin)
                    if (d + 16u * m + 8u > flushed + SNAP_RING) {
                        uint32_t want = d + 16u * m - (SNAP_RING / 2);
                        uint32_t take = want > flushed ? want - flushed : 0;
                        if (take > d - flushed) take = d - flushed;
                        snap_flush(dst, ring, flushed, take, lane);
                        flushed += take;
                    }
                    if (lane < m) {
                        const uint32_t base = d + 16u * lane;
                        for (int k = 0; k < 7; k++) {
                            ring[(base + k) & (SNAP_RING - 1)] = b[k];
                            ring[(base + 8 + k) & (SNAP_RING - 1)] = b[k];
                        }
                        ring[(base + 7) & (SNAP_RING - 1)] = pbyte;
                        ring[(base + 15) & (SNAP_RING - 1)] = pbyte;
                    }
                    d += 16u * m;
                    pos += 10u * m;
                    consumed += m;
                    if (m < 64u) break;
                }
                if (consumed) {
                    rwin_reload();
                    continue;
                }
                // zero pairs matched: fall through to the per-element paths
                // (the register window is still consistent after the spill)
            }
            // ---- v5 fast path: tiny literal / pow2-offset short match ----
            if (kind == 0) {
                // len <= 7: the literal's bytes are exactly the upper 7
                // bytes of the peek window (tag occupies byte 0)
                const uint32_t len = (tag >> 2) + 1;
                if (len <= 7 && pos + 1 + len <= clen && d + len <= ulen &&
                    d + len + 8 <= flushed + SNAP_RING) {
                    const uint64_t nv = (v >> 8) & ((1ull << (8 * len)) - 1);
                    rwin_append(nv, len);
                    pos += 1 + len;
                    continue;
                }
            } else if (kind == 1 || kind == 2) {
                uint32_t len, off, hdr;
                if (kind == 1) {
                    len = ((tag >> 2) & 0x7u) + 4;
                    off = (uint32_t)((tag >> 5) << 8) |
                          (uint32_t)((v >> 8) & 0xFFu);
                    hdr = 2;
                } else {
                    len = (tag >> 2) + 1;
                    off = (uint32_t)((v >> 8) & 0xFFFFu);
                    hdr = 3;
                }
                // head of a chain of identical long 2-byte-offset copies (a
                // ts page is ~1000 of them): leave it to the fusing general
                // path, whose direct run writes the whole chain at once
                const bool chain =
                    kind == 2 && len >= 32 &&
                    (v & 0xFFFFFFull) == ((v >> 24) & 0xFFFFFFull) &&
                    (v & 0xFFFFull) == ((v >> 48) & 0xFFFFull);
                if (!chain &&
                    (off == 1 || off == 2 || off == 4 || off == 8) &&
                    off <= d && pos + hdr <= clen && d + len <= ulen &&
                    d + len + 8 <= flushed + SNAP_RING) {
                    // pow2 period divides 8: the replicated pattern word is
                    // constant across every emitted 8-byte chunk
                    // (doubling: 8*off -> 16*off -> ... -> 64 bits; off = 2
                    // needs the << 32 step too)
                    uint64_t rep = tail0 >> (64 - 8 * off);
                    for (uint32_t s = 8 * off; s < 64; s <<= 1)
                        rep |= rep << s;
                    uint32_t rem = len;
                    while (rem >= 8) {
                        rwin_append(rep, 8);
                        rem -= 8;
                    }
                    if (rem)
                        rwin_append(rep & ((1ull << (8 * rem)) - 1), rem);
                    pos += hdr;
                    continue;
                }
            }
            // ---- general paths (ring-direct): sync the register window --
            rwin_spill();
            bool slow = true;
            if (kind == 0) {  // literal
                uint32_t len = (tag >> 2) + 1;
                uint32_t hdr = 1;
                if (len > 60) {
                    const uint32_t nb = len - 60;
                    if (pos + 1 + nb > clen) { err = 1; break; }
                    len = (uint32_t)((v >> 8) &
                                     ((nb >= 4) ? 0xFFFFFFFFull
                                                : ((1ull << (8 * nb)) - 1)));
                    len += 1;
                    hdr = 1 + nb;
                }
                pos += hdr;
                if (pos + len > clen || d + len > ulen) { err = 1; break; }
                if (len >= SNAP_RING) {
                    // huge literal (incompressible value pages): flush the
                    // ring, copy src->dst directly, re-prime the ring tail
                    snap_flush(dst, ring, flushed, d - flushed, lane);
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                    if ((d & 7u) == 0) {
                        // dst 8-aligned (whole-page literals start at 0):
                        // copy 8 output bytes per lane from two aligned
                        // source words + funnel shift — 8x fewer
                        // instructions than the byte loop
                        const uint64_t* sw =
                            (const uint64_t*)(src + ((pos) & ~7u));
                        const uint32_t sh = 8u * (pos & 7u);
                        // sh != 0 reads sw[w+1]: stop a word early so the
                        // last aligned read never crosses the blob slack
                        const uint32_t words =
                            sh ? ((len >> 3) ? (len >> 3) - 1 : 0)
                               : (len >> 3);
                        for (uint32_t w = lane; w < words; w += 64) {
                            uint64_t lo = sw[w];
                            uint64_t x;
                            if (sh) {
                                uint64_t hi2 = sw[w + 1];
                                x = (lo >> sh) | (hi2 << (64 - sh));
                            } else {
                                x = lo;
                            }
                            *(uint64_t*)(dst + d + 8 * w) = x;
                        }
                        for (uint32_t i = (words << 3) + lane; i < len;
                             i += 64)
                            dst[d + i] = src[pos + i];
                    } else {
                        for (uint32_t i = lane; i < len; i += 64)
                            dst[d + i] = src[pos + i];
                    }
                    // re-prime the ring with the literal's last SNAP_RING
                    // bytes: 8 B per lane over the 8-aligned output
                    // positions, bytes at the two ragged ends (source reads
                    // stay inside the literal)
                    {
                        const uint32_t e = d + len;
                        const uint32_t a_lo = e - SNAP_RING;   // >= d
                        const uint32_t a8 = (a_lo + 7u) & ~7u;
                        const uint32_t e8 = e & ~7u;
                        // output position a <-> src[pos + (a - d)]
                        for (uint32_t a = a_lo + lane; a < a8; a += 64)
                            ring[a & (SNAP_RING - 1)] = src[pos + (a - d)];
                        for (uint32_t a = a8 + 8u * lane; a < e8; a += 512u) {
                            uint64_t x;
                            __builtin_memcpy(&x, src + pos + (a - d), 8);
                            *(uint64_t*)(ring + (a & (SNAP_RING - 1))) = x;
                        }
                        for (uint32_t a = e8 + lane; a < e; a += 64)
                            ring[a & (SNAP_RING - 1)] = src[pos + (a - d)];
                    }
                    d += len;
                    flushed = d;
                } else {
                    if (d + len + 8 > flushed + SNAP_RING) {
                        uint32_t want = d + len - (SNAP_RING / 2);
                        uint32_t take = want > flushed ? want - flushed : 0;
                        if (take > d - flushed) take = d - flushed;
                        snap_flush(dst, ring, flushed, take, lane);
                        flushed += take;
                    }
                    for (uint32_t i = lane; i < len; i += 64)
                        ring[(d + i) & (SNAP_RING - 1)] = src[pos + i];
                    d += len;
                }
                pos += len;
            } else {
                uint32_t len, off;
                if (kind == 1) {
                    len = ((tag >> 2) & 0x7u) + 4;
                    off = (uint32_t)((tag >> 5) << 8) |
                          (uint32_t)((v >> 8) & 0xFFu);
                    pos += 2;
                } else if (kind == 2) {
                    len = (tag >> 2) + 1;
                    off = (uint32_t)((v >> 8) & 0xFFFFu);
                    pos += 3;
                } else {
                    len = (tag >> 2) + 1;
                    off = (uint32_t)((v >> 8) & 0xFFFFFFFFull);
                    pos += 5;
                }
                if (pos > clen || off == 0 || off > d) { err = 1; break; }
                // FUSE adjacent same-offset matches: copy k covers
                // [d+L, d+L+len_k) from [d+L-off, ...) — the continuation
                // of one periodic/shifted copy. The fused run executes as
                // a single cooperative loop; per-tag cost = the parse.
                // A ts page is ~1000 IDENTICAL 3-byte tags: count those 64
                // at a time (lane k compares the tag at pos + 3k, ballot
                // prefix) instead of parsing them one by one; the serial
                // loop below picks up whatever differs.
                if (kind == 2 && d + len <= ulen) {
                    const uint32_t tag3 = (uint32_t)(v & 0xFFFFFFull);
                    const uint32_t elen = len;
                    for (;;) {
                        const uint32_t pp = pos + 3u * lane;
                        bool ok = pp + 3 <= clen;
                        if (ok) {
                            const uint32_t t = (uint32_t)src[pp] |
                                               ((uint32_t)src[pp + 1] << 8) |
                                               ((uint32_t)src[pp + 2] << 16);
                            ok = t == tag3;
                        }
                        const unsigned long long bm = __ballot(ok);
                        uint32_t m =
                            (~bm == 0ull) ? 64u
                                          : (uint32_t)(__ffsll((long long)~bm) - 1);
                        m = min(m, (ulen - d - len) / elen);
                        if (m == 0) break;
                        len += m * elen;
                        pos += 3u * m;
                        if (m < 64u) break;
                    }
                }
                for (;;) {
                    st.advance_to(pos);
                    const uint64_t nv = st.peek8(pos);
                    const uint32_t ntag = (uint32_t)(nv & 0xFFu);
                    const uint32_t nkind = ntag & 3u;
                    uint32_t nlen, noff, nhdr;
                    if (nkind == 1) {
                        nlen = ((ntag >> 2) & 0x7u) + 4;
                        noff = (uint32_t)((ntag >> 5) << 8) |
                               (uint32_t)((nv >> 8) & 0xFFu);
                        nhdr = 2;
                    } else if (nkind == 2) {
                        nlen = (ntag >> 2) + 1;
                        noff = (uint32_t)((nv >> 8) & 0xFFFFu);
                        nhdr = 3;
                    } else {
                        break;   // literal or 4-byte-offset copy: stop
                    }
                    if (noff != off || pos + nhdr > clen ||
                        d + len + nlen > ulen)
                        break;
                    len += nlen;
                    pos += nhdr;
                }
                if (d + len > ulen) { err = 1; break; }
                if (len >= SNAP_DIRECT_MIN &&
                    (off == 1 || off == 2 || off == 4 || off == 8 ||
                     off == 16)) {
                    // DIRECT same-offset run: off divides 16, so every
                    // 16-aligned output chunk of the run is the SAME 16
                    // bytes Q, Q[a & 15] = out[a] = S[(a - d) mod off] with
                    // S = the last off output bytes (register tail). Build
                    // Q rotated for d's alignment, drain the ring, store the
                    // run straight to dst 16 B per lane, and mirror its last
                    // min(len, SNAP_RING) bytes into the ring the same way.
                    uint64_t q0, q1;
                    if (off <= 8) {
                        // R[i] = out[d + i], period off | 8
                        uint64_t rep = tail0 >> (64 - 8 * off);
                        for (uint32_t s = 8 * off; s < 64; s <<= 1)
                            rep |= rep << s;
                        const uint32_t r = 8u * (d & 7u);
                        q0 = r ? ((rep << r) | (rep >> (64 - r))) : rep;
                        q1 = q0;
                    } else {
                        // T = out[d-16, d) = (tail1, tail0); Q = T rotated
                        // left by d & 15 bytes
                        uint64_t lo = tail1, hi = tail0;
                        uint32_t r = d & 15u;
                        if (r >= 8) {
                            const uint64_t t = lo;
                            lo = hi;
                            hi = t;
                            r -= 8;
                        }
                        if (r) {
                            const uint32_t s = 8u * r;
                            q0 = (lo << s) | (hi >> (64 - s));
                            q1 = (hi << s) | (lo >> (64 - s));
                        } else {
                            q0 = lo;
                            q1 = hi;
                        }
                    }
                    snap_flush(dst, ring, flushed, d - flushed, lane);
                    const uint32_t e = d + len;
                    snap_emit_q<0xFFFFFFFFu>(dst, d, e, q0, q1, lane);
                    snap_emit_q<SNAP_RING - 1>(
                        ring, len >= SNAP_RING ? e - SNAP_RING : d, e, q0, q1,
                        lane);
                    d = e;
                    flushed = e;
                } else if (off > SNAP_RING / 2) {
                    // far back-reference (not produced for this data
                    // shape): flush + drain once, then chunked global
                    // reads of the (flushed, stable) pre-run bytes
                    snap_flush(dst, ring, flushed, d - flushed, lane);
                    flushed = d;
                    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
                    const uint32_t D = d;
                    uint32_t done = 0;
                    while (done < len) {
                        const uint32_t chunk =
                            min(len - done, SNAP_RING / 2);
                        if (d + chunk + 8 > flushed + SNAP_RING) {
                            uint32_t want = d + chunk - (SNAP_RING / 2);
                            uint32_t take =
                                want > flushed ? want - flushed : 0;
                            if (take > d - flushed) take = d - flushed;
                            snap_flush(dst, ring, flushed, take, lane);
                            flushed += take;
                        }
                        for (uint32_t i = lane; i < chunk; i += 64) {
                            const uint32_t j = done + i;
                            const uint8_t b =
                                (off >= len) ? dst[D - off + j]
                                             : dst[D - off + (j % off)];
                            ring[(d + i) & (SNAP_RING - 1)] = b;
                        }
                        d += chunk;
                        done += chunk;
                    }
                } else {
                    // ring-resident source, period-doubling: after `done`
                    // bytes of the run, everything in [d - done - off, d)
                    // repeats with period (done + off), so each chunk can
                    // copy with shift P = min(done + off, 2048) — sources
                    // are all pre-chunk and at most ~2 KB behind the
                    // cursor (always ring-resident). Chunks grow
                    // geometrically: a 64 KB off=8 run takes ~40 rounds.
                    uint32_t done = 0;
                    while (done < len) {
                        // shift P must stay a MULTIPLE of off (periodicity)
                        // and <= RING/2 (so P + chunk <= RING: this chunk's
                        // writes never clobber its sources). done + off is
                        // a multiple of off by construction (done sums
                        // previous P's).
                        uint32_t P = done + off;
                        if (P > SNAP_RING / 2)
                            P = off * ((SNAP_RING / 2) / off);
                        const uint32_t chunk = min(len - done, P);
                        if (d + chunk + 8 > flushed + SNAP_RING) {
                            uint32_t want = d + chunk - (SNAP_RING / 2);
                            uint32_t take =
                                want > flushed ? want - flushed : 0;
                            if (take > d - flushed) take = d - flushed;
                            snap_flush(dst, ring, flushed, take, lane);
                            flushed += take;
                        }
                        for (uint32_t i = lane; i < chunk; i += 64)
                            ring[(d + i) & (SNAP_RING - 1)] =
                                ring[(d - P + i) & (SNAP_RING - 1)];
                        d += chunk;
                        done += chunk;
                    }
                }
            }
            if (slow) rwin_reload();
        }
        rwin_spill();
        if (!err && d == ulen) {
            snap_flush(dst, ring, flushed, d - flushed, lane);
        } else if (lane == 0) {
            atomicAdd(err_flag, 1ull);
        }
    }
}

// ---------------------------------------------------------------------------
// DELTA_BINARY_PACKED i64 decode (parquet-format Encodings.md; the encoding
// the reference's config enables for ts, config.rs:54-75). One workgroup per
// page: lane-serial header walk, parallel miniblock bit-unpack, hierarchical
// prefix sum in LDS, dense i64 output. Page <= 8192 values (the writer
// contract: row group 8192, one data page per chunk — engine validates).
// ---------------------------------------------------------------------------
#define DELTA_MAX_VALUES 8192
#define DELTA_MAX_BLOCKS 128   // >= max_values / min_block_size(128)

struct DeltaHdr {
    int32_t values_per_mb;
    int32_t n_mb_per_block;
    int32_t total_count;
    int64_t first_value;
    int32_t n_blocks;
    int32_t err;
};

__device__ inline uint64_t d_varint(const uint8_t* p, uint32_t len, uint32_t& pos,
                                    int32_t* err) {
    uint64_t r = 0;
    int s = 0;
    for (;;) {
        if (pos >= len || s > 63) { *err = 1; return 0; }
        uint8_t b = p[pos++];
        r |= (uint64_t)(b & 0x7f) << s;
        if (!(b & 0x80)) return r;
        s += 7;
    }
}
__device__ inline int64_t d_zigzag(const uint8_t* p, uint32_t len, uint32_t& pos,
                                   int32_t* err) {
    uint64_t u = d_varint(p, len, pos, err);
    return (int64_t)(u >> 1) ^ -(int64_t)(u & 1);
}

extern "C" __global__ void __launch_bounds__(256)
k_decode_delta_i64(const uint8_t* blob, uint8_t* dec,
                   const DeltaPageDesc* pages, uint32_t n_pages,
                   unsigned long long* err_flag) {
    __shared__ DeltaHdr H;
    __shared__ int64_t vals[DELTA_MAX_VALUES];          // deltas -> prefix
    __shared__ int64_t blk_min_delta[DELTA_MAX_BLOCKS];
    __shared__ uint32_t mb_off[DELTA_MAX_BLOCKS * 8];   // per-miniblock data offset
    __shared__ uint8_t mb_w[DELTA_MAX_BLOCKS * 8];
    __shared__ int64_t tsum[256 / 64];                  // per-wave partials
    __shared__ int64_t chunk_sum[256];

    for (uint32_t pg = blockIdx.x; pg < n_pages; pg += gridDim.x) {
        const DeltaPageDesc pd = pages[pg];
        const uint8_t* src = ((pd.src_off & OFF_DEC) ? dec : blob) +
                             (pd.src_off & OFF_MASK);
        const uint32_t len = pd.src_len;

        if (threadIdx.x == 0) {
            int32_t err = 0;
            uint32_t pos = 0;
            int32_t block_size = (int32_t)d_varint(src, len, pos, &err);
            int32_t n_mb = (int32_t)d_varint(src, len, pos, &err);
            int32_t total = (int32_t)d_varint(src, len, pos, &err);
            int64_t first = d_zigzag(src, len, pos, &err);
            H.err = err;
            if (!err && (n_mb <= 0 || block_size <= 0 || n_mb > 8 ||
                         block_size % n_mb != 0 || total > DELTA_MAX_VALUES ||
                         (uint32_t)total != pd.n_values ||
                         (block_size / n_mb) % 32 != 0)) {
                H.err = 2;
            }
            if (!H.err) {
                H.values_per_mb = block_size / n_mb;
                H.n_mb_per_block = n_mb;
                H.total_count = total;
                H.first_value = first;
                int32_t deltas = total - 1;
                int32_t nblk = deltas <= 0 ? 0 : (deltas + block_size - 1) / block_size;
                H.n_blocks = nblk;
                // serial walk of block headers (varints force it; 64 blocks max)
                int32_t remaining = deltas;
                for (int32_t b = 0; b < nblk && !H.err; b++) {
                    blk_min_delta[b] = d_zigzag(src, len, pos, &err);
                    if (err) { H.err = 3; break; }
                    uint32_t wpos = pos;
                    pos += n_mb;  // bit width bytes
                    if (pos > len) { H.err = 3; break; }
                    for (int32_t m = 0; m < n_mb; m++) {
                        uint8_t w = src[wpos + m];
                        mb_w[b * 8 + m] = w;
                        mb_off[b * 8 + m] = pos;
                        // data present for miniblocks that hold any values
                        if (remaining > 0) pos += (uint32_t)H.values_per_mb * w / 8;
                        remaining -= H.values_per_mb;
                    }
                    if (pos > len) { H.err = 3; }
                }
            }
        }
        __syncthreads();
        if (H.err) {
            if (threadIdx.x == 0) atomicAdd(err_flag, 1ull);
            __syncthreads();
            continue;
        }
        const int32_t total = H.total_count;
        const int32_t vpm = H.values_per_mb;
        const int32_t deltas = total - 1;

        // parallel unpack: delta j (0-based, value index j+1)
        for (int32_t j = threadIdx.x; j < deltas; j += blockDim.x) {
            int32_t blk = j / (vpm * H.n_mb_per_block);
            int32_t inblk = j - blk * vpm * H.n_mb_per_block;
            int32_t mb = inblk / vpm;
            int32_t inmb = inblk - mb * vpm;
            uint8_t w = mb_w[blk * 8 + mb];
            uint64_t raw = 0;
            if (w > 0) {
                uint64_t bitpos = (uint64_t)inmb * w;
                const uint8_t* base = src + mb_off[blk * 8 + mb] + (bitpos >> 3);
                int shift = (int)(bitpos & 7);
                // assemble enough bytes for w bits + shift (<= 9 bytes)
                uint64_t lo = 0;
                for (int k = 0; k < 8; k++) lo |= (uint64_t)base[k] << (8 * k);
                raw = lo >> shift;
                if (w + shift > 64) {
                    uint64_t hi = base[8];
                    raw |= hi << (64 - shift);
                }
                if (w < 64) raw &= ((1ull << w) - 1);
            }
            vals[j + 1] = (int64_t)raw + blk_min_delta[blk];
        }
        if (threadIdx.x == 0) vals[0] = 0;
        __syncthreads();

        // hierarchical inclusive prefix sum over vals[0..total)
        // each thread scans a contiguous chunk of 32, then chunk offsets
        const int32_t CH = 32;
        int32_t c0 = threadIdx.x * CH;
        int64_t acc = 0;
        for (int32_t j = c0; j < min(c0 + CH, total); j++) {
            acc += vals[j];
            vals[j] = acc;
        }
        chunk_sum[threadIdx.x] = acc;
        __syncthreads();
        if (threadIdx.x < 64) {  // single wave scans the 256 chunk sums
            int64_t s0 = 0;
            for (int k = 0; k < 4; k++) {
                int idx = threadIdx.x * 4 + k;
                s0 += chunk_sum[idx];
            }
            // wave inclusive scan of s0 over 64 lanes
            int64_t sc = s0;
            for (int off = 1; off < 64; off <<= 1) {
                int64_t up = __shfl_up(sc, off, 64);
                if ((int)(threadIdx.x) >= off) sc += up;
            }
            tsum[0] = 0;  // unused; keep LDS referenced
            // exclusive base for each 4-chunk group of this lane
            int64_t base4 = sc - s0;
            int64_t run = base4;
            for (int k = 0; k < 4; k++) {
                int idx = threadIdx.x * 4 + k;
                int64_t cs = chunk_sum[idx];
                chunk_sum[idx] = run;  // exclusive chunk base
                run += cs;
            }
        }
        __syncthreads();
        int64_t base = chunk_sum[threadIdx.x] + H.first_value;
        for (int32_t j = c0; j < min(c0 + CH, total); j++) vals[j] += base;
        // note: vals[0] = 0 + base = first_value ✓
        __syncthreads();

        int64_t* dst = (int64_t*)(dec + (pd.dst_off & OFF_MASK));
        for (int32_t j = threadIdx.x; j < total; j += blockDim.x)
            dst[j] = vals[j];
        __syncthreads();
    }
}

}  // namespace hx

// ---------------------------------------------------------------------------
// host-side launchers (hx_kernels.h)
// ---------------------------------------------------------------------------
#include "hx_kernels.h"
#include <algorithm>
#include <cstring>
#include <cstdlib>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

namespace hx {

extern "C" __global__ void __launch_bounds__(256)
k_seg_keys(const long long* ts, long long seg_ms, unsigned long long* keys,
           uint32_t n) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += blockDim.x * gridDim.x) {
        long long t = ts[i];
        long long q = t / seg_ms;
        if ((t % seg_ms) != 0 && t < 0) q--;
        keys[i] = (unsigned long long)q ^ 0x8000000000000000ull;
    }
}

extern "C" __global__ void __launch_bounds__(256)
k_iota(uint32_t* out, uint32_t n) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += blockDim.x * gridDim.x)
        out[i] = i;
}

// ---------------------------------------------------------------------------
// Kernel 1e: Snappy page compressor, the write side's twin of
// k_snappy_decompress. One wave (one 64-thread block) per page; the 16 KB
// hash table of position + 1 lives in LDS. The stream is a pure function of
// the page bytes and equals hx::snappy_compress_host (snappy_compress.h),
// whose header comment states the algorithm: each step examines the 64
// positions [pos, pos + 64), one per lane, ranks each lane's candidates by a
// prefix capped at 16 bytes, a ballot picks the first lane, the match is
// extended 64 bytes per ballot, lane 0 writes the tags (snappy_emit.h, shared
// with the twin) and the wave copies literal bytes. Table inserts are
// atomicMax on the LDS word, consumed positions only.
// Reads nothing outside src[0, n) (any byte alignment), writes nothing
// outside dst[0, dst_cap); a slot below Snappy's bound 32 + n + n / 6 counts
// one error, gets out_len 0 and is left untouched.
// ---------------------------------------------------------------------------
__device__ __forceinline__ uint32_t sc_load32(const uint8_t* p) {
    uint32_t w;
    __builtin_memcpy(&w, p, 4);
    return w;
}
__device__ __forceinline__ uint64_t sc_load64(const uint8_t* p) {
    uint64_t w;
    __builtin_memcpy(&w, p, 8);
    return w;
}

// d and s congruent modulo sizeof(T): bytes up to d's alignment, T-wide
// body, bytes at the end. nt threads, thread t of them.
template <typename T>
__device__ __forceinline__ void sc_copy_as(uint8_t* d, const uint8_t* s,
                                           uint32_t len, uint32_t t,
                                           uint32_t nt) {
    uint32_t head = uint32_t(-(uintptr_t)d) & uint32_t(sizeof(T) - 1);
    if (head > len) head = len;
    if (t < head) d[t] = s[t];
    const uint32_t body = (len - head) / uint32_t(sizeof(T));
    const T* sv = (const T*)(s + head);
    T* dv = (T*)(d + head);
    for (uint32_t i = t; i < body; i += nt) dv[i] = sv[i];
    const uint32_t done = head + body * uint32_t(sizeof(T));
    if (t < len - done) d[done + t] = s[done + t];
}

// Cooperative copy of len bytes, non-overlapping, any alignment: the widest
// access (up to 16 B per thread) that the distance between d and s allows.
__device__ __forceinline__ void sc_copy(uint8_t* d, const uint8_t* s,
                                        uint32_t len, uint32_t t,
                                        uint32_t nt) {
    const uint32_t diff = uint32_t((uintptr_t)d - (uintptr_t)s) | 16u;
    const uint32_t width = diff & (0u - diff);   // lowest set bit: 1..16
    if (len < 64 || width == 1) {
        for (uint32_t i = t; i < len; i += nt) d[i] = s[i];
    } else if (width == 16) {
        sc_copy_as<uint4>(d, s, len, t, nt);
    } else if (width == 8) {
        sc_copy_as<uint2>(d, s, len, t, nt);
    } else if (width == 4) {
        sc_copy_as<uint32_t>(d, s, len, t, nt);
    } else {
        sc_copy_as<uint16_t>(d, s, len, t, nt);
    }
}

__global__ void __launch_bounds__(64)
k_snappy_compress(const uint8_t* __restrict__ src_base,
                  uint8_t* __restrict__ dst_base,
                  const SnappyCompDesc* __restrict__ pages, uint32_t n_pages,
                  uint32_t* __restrict__ out_len,
                  unsigned long long* err_flag) {
    __shared__ uint32_t H[SNAPPY_HASH_SIZE];
    const uint32_t lane = threadIdx.x;
    for (uint32_t pg = blockIdx.x; pg < n_pages; pg += gridDim.x) {
        const SnappyCompDesc pd = pages[pg];
        const uint32_t N = pd.n;
        const uint32_t cap = pd.dst_cap;
        if ((uint64_t)cap < snappy_max_compressed(N)) {
            if (lane == 0) {
                atomicAdd(err_flag, 1ull);
                out_len[pg] = 0;
            }
            continue;
        }
        const uint8_t* src = src_base + pd.src_off;
        uint8_t* dst = dst_base + pd.dst_off;
        __syncthreads();   // the previous page's table reads are done
        for (uint32_t i = lane; i < SNAPPY_HASH_SIZE; i += 64) H[i] = 0;
        __syncthreads();

        // lane 0 writes tag bytes; their count goes to every lane
        uint32_t k = 0;
        if (lane == 0) k = snappy_emit_varint(dst, N);
        uint32_t o = __shfl(k, 0);
        bool overflow = false;
        // literal [from, to), to > from
        auto emit_literal = [&](uint32_t from, uint32_t to) {
            const uint32_t len = to - from;
            if ((uint64_t)o + 5 + len > cap) {
                overflow = true;
                return;
            }
            uint32_t kk = 0;
            if (lane == 0) kk = snappy_emit_literal_tag(dst + o, len);
            o += __shfl(kk, 0);
            sc_copy(dst + o, src + from, len, lane, 64);
            o += len;
        };

        uint32_t pos = 0, lit_start = 0;
        while ((uint64_t)pos + 4 <= N && !overflow) {
            const uint32_t end =
                N - 3 - pos < SNAPPY_CHUNK ? N - 3 : pos + SNAPPY_CHUNK;
            const uint32_t p = pos + lane;
            const bool active = p < end;
            uint32_t w = 0, best_len = 0, best_c = 0;
            if (active) {
                w = sc_load32(src + p);
                const uint32_t lim =
                    N - p < SNAPPY_PROBE_CAP ? N - p : SNAPPY_PROBE_CAP;
                const bool full = lim == SNAPPY_PROBE_CAP;
                uint64_t a0 = 0, a1 = 0;
                if (full) {
                    a0 = sc_load64(src + p);
                    a1 = sc_load64(src + p + 8);
                }
                auto probe = [&](uint32_t c) {
                    uint32_t len;
                    if (full) {   // c + 16 < p + 16 <= N
                        const uint64_t x = a0 ^ sc_load64(src + c);
                        if ((uint32_t)x) return;
                        if (x) {
                            len = uint32_t(__builtin_ctzll(x)) >> 3;
                        } else {
                            const uint64_t y = a1 ^ sc_load64(src + c + 8);
                            len = 8 + (y ? uint32_t(__builtin_ctzll(y)) >> 3
                                         : 8u);
                        }
                    } else {
                        if (sc_load32(src + c) != w) return;
                        len = 4;
                        while (len < lim && src[c + len] == src[p + len])
                            len++;
                    }
                    if (len > best_len || (len == best_len && c > best_c)) {
                        best_len = len;
                        best_c = c;
                    }
                };
                for (uint32_t d = 8; d <= 64; d += 8)
                    if (p >= d) probe(p - d);
                const uint32_t h = H[snappy_hash(w)];
                if (h && p - (h - 1) <= SNAPPY_MAX_OFFSET) probe(h - 1);
            }
            const unsigned long long m8 = __ballot(best_len >= 8);
            const unsigned long long many = __ballot(best_len > 0);
            const unsigned long long sel = m8 ? m8 : many;
            uint32_t ins_end = end;
            if (sel) {
                const int fl = __ffsll(sel) - 1;
                const uint32_t first = pos + (uint32_t)fl;
                const uint32_t c = __shfl(best_c, fl);
                // full common prefix of src[first..] and src[c..], up to N
                uint32_t L = 4;
                for (;;) {
                    const uint32_t q = first + L + lane;   // c + L + lane < q
                    const bool stop = q >= N || src[c + L + lane] != src[q];
                    const unsigned long long sm = __ballot(stop);
                    if (sm) {
                        L += (uint32_t)(__ffsll(sm) - 1);
                        break;
                    }
                    L += 64;
                }
                if (first > lit_start) emit_literal(lit_start, first);
                // copies of 64 while L >= 68 (one 3-byte element per lane and
                // round), then the tail as snappy_emit_copy splits it
                const uint32_t k64 = L >= 68 ? (L - 68) / 64 + 1 : 0;
                if (!overflow && (uint64_t)o + 3ull * k64 + 6 > cap)
                    overflow = true;
                if (!overflow) {
                    const uint32_t off = first - c;
                    for (uint32_t i = lane; i < k64; i += 64)
                        snappy_emit_copy1(dst + o + 3 * i, off, 64);
                    o += 3 * k64;
                    uint32_t kk = 0;
                    if (lane == 0)
                        kk = snappy_emit_copy(dst + o, off, L - 64 * k64);
                    o += __shfl(kk, 0);
                }
                if (first + L < end) ins_end = first + L;
                lit_start = first + L;
            }
            if (active && p < ins_end) atomicMax(&H[snappy_hash(w)], p + 1);
            pos = sel ? lit_start : end;
            __syncthreads();   // inserts land before the next step's lookups
        }
        if (!overflow && lit_start < N) emit_literal(lit_start, N);
        if (overflow) {   // cannot happen with cap at the bound; never write past
            if (lane == 0) {
                atomicAdd(err_flag, 1ull);
                out_len[pg] = 0;
            }
            continue;
        }
        if (o >= snappy_stored_size(N)) {
            // the stored form: what hx_snappy_stored_literal recognises
            __threadfence();   // the stream's stores are ordered before these
            k = 0;
            if (lane == 0) k = snappy_emit_varint(dst, N);
            o = __shfl(k, 0);
            if (N) emit_literal(0, N);
        }
        if (lane == 0) out_len[pg] = o;
    }
}

// Scan-and-pack behind kernel 1e, so the host takes the streams in one
// contiguous copy of sum(out_len) bytes. The scan: ONE block walks out_len in
// tiles of 256, an inclusive LDS scan per tile and a carry from tile to tile,
// and writes offs[i] = sum(out_len[0, i)) — linear in the page count.
__global__ void __launch_bounds__(256)
k_snappy_scan(const uint32_t* __restrict__ out_len, uint32_t n_pages,
              unsigned long long* __restrict__ offs) {
    __shared__ unsigned long long part[256];
    const uint32_t t = threadIdx.x;
    unsigned long long carry = 0;
    for (uint32_t base = 0; base < n_pages; base += 256) {
        const uint32_t i = base + t;
        const unsigned long long own = i < n_pages ? out_len[i] : 0;
        part[t] = own;
        __syncthreads();
        for (uint32_t st = 1; st < 256; st <<= 1) {
            const unsigned long long add = t >= st ? part[t - st] : 0;
            __syncthreads();
            part[t] += add;
            __syncthreads();
        }
        if (i < n_pages) offs[i] = carry + part[t] - own;
        carry += part[255];
        __syncthreads();   // part[255] read by all before the next tile
    }
}

// The pack: one block per page copies its stream from its slot to
// packed + offs[page].
__global__ void __launch_bounds__(256)
k_snappy_pack(const uint8_t* __restrict__ slots,
              const SnappyCompDesc* __restrict__ pages, uint32_t n_pages,
              const uint32_t* __restrict__ out_len,
              const unsigned long long* __restrict__ offs,
              uint8_t* __restrict__ packed) {
    for (uint32_t pg = blockIdx.x; pg < n_pages; pg += gridDim.x)
        sc_copy(packed + offs[pg], slots + pages[pg].dst_off, out_len[pg],
                threadIdx.x, 256);
}

// Footer statistics of the pages kernel 1e compresses, so the raw columns
// need not cross PCIe for them: one wave per page of 8-byte values, min and
// max through an order-preserving u64 key (u64: the bits; i64: sign flipped;
// f64: the usual total-order key, NaN skipped). The f64 bounds leave as the
// writer's minmax_bytes leaves them: a zero bound is min -0.0 / max +0.0.
__global__ void __launch_bounds__(64)
k_page_minmax(const uint8_t* __restrict__ src_base,
              const SnappyCompDesc* __restrict__ pages,
              const uint32_t* __restrict__ kinds, uint32_t n_pages,
              PageStat* __restrict__ out) {
    const uint64_t SIGN = 0x8000000000000000ull;
    for (uint32_t pg = blockIdx.x; pg < n_pages; pg += gridDim.x) {
        const SnappyCompDesc pd = pages[pg];
        const uint32_t kind = kinds[pg];
        const uint64_t* v = (const uint64_t*)(src_base + pd.src_off);
        const uint32_t n_vals = pd.n >> 3;
        unsigned long long lo = ~0ull, hi = 0ull;
        bool any = false;
        for (uint32_t i = threadIdx.x; i < n_vals; i += 64) {
            const uint64_t b = v[i];
            uint64_t key = b;
            if (kind == PAGE_ORDER_I64) {
                key = b ^ SIGN;
            } else if (kind == PAGE_ORDER_F64) {
                if ((b & ~SIGN) > 0x7FF0000000000000ull) continue;   // NaN
                key = (b & SIGN) ? ~b : (b | SIGN);
            }
            any = true;
            lo = key < lo ? key : lo;
            hi = key > hi ? key : hi;
        }
        for (int m = 32; m > 0; m >>= 1) {
            const unsigned long long l2 = __shfl_xor(lo, m);
            const unsigned long long h2 = __shfl_xor(hi, m);
            lo = l2 < lo ? l2 : lo;
            hi = h2 > hi ? h2 : hi;
        }
        const bool has = __ballot(any) != 0;
        if (threadIdx.x == 0) {
            uint64_t mn = lo, mx = hi;
            if (kind == PAGE_ORDER_I64) {
                mn ^= SIGN;
                mx ^= SIGN;
            } else if (kind == PAGE_ORDER_F64) {
                mn = (mn & SIGN) ? (mn & ~SIGN) : ~mn;
                mx = (mx & SIGN) ? (mx & ~SIGN) : ~mx;
                if ((mn & ~SIGN) == 0) mn = SIGN;   // -0.0
                if ((mx & ~SIGN) == 0) mx = 0;      // +0.0
            }
            out[pg] = PageStat{has ? mn : 0, has ? mx : 0, has ? 1ull : 0ull};
        }
    }
}

// ---------------------------------------------------------------------------
// Kernel 1f: PLAIN BYTE_ARRAY page images of a Binary value
// column, the write side's twin of k_ba_offsets. Input is one handle per
// source row (off << 20 | len relative to src, already in output order) and
// optionally group_start[n_out + 1]: output row i is the concatenation of
// source rows [group_start[i], group_start[i + 1]) under one length prefix
// (BytesMergeOperator::merge); without it output row i is source row i. The
// bytes equal hx::ba_build_pages_host (ba_pages.h), whose header states the
// refusal rules. Three launches:
//   k_ba_page_sizes   one block per output row group: row_len[i] (or
//                     BA_ROW_SKIP) and the page's byte count, a u64 block sum
//   k_ba_page_scan    one block: exclusive scan of the page sizes
//   k_ba_build_pages  one block per output row group: a wave-shuffle scan of
//                     4 + len in tiles of 256 rows gives each row its offset
//                     in the page (LDS, R <= 8192 rows); then each wave takes
//                     64 rows at a time, row per lane for short rows, the
//                     whole wave on one row for long ones (sc_copy: up to
//                     16 B per lane where the two alignments allow it).
// Nothing outside [src, src + src_size) is read, nothing outside the page's
// own [page_off[g], page_off[g + 1]) is written; plain vector stores, no
// atomics but the two counters.
// ---------------------------------------------------------------------------
struct BaBuildParams {
    const uint8_t* src;
    uint64_t src_size;
    const uint64_t* handles;       // n_src
    const uint32_t* group_start;   // n_out + 1, or null
    uint32_t n_src, n_out, R, n_pages;
    uint32_t* row_len;             // n_out
    unsigned long long* page_size; // n_pages
    unsigned long long* page_off;  // n_pages + 1
    uint8_t* out;                  // page_off[n_pages] bytes
    unsigned long long* counts;    // [0] errors, [1] rows over the value cap
};

// rows below both bounds are copied by their own lane (unmeasured split)
#define BA_LANE_MAX_BYTES 256u
#define BA_LANE_MAX_PARTS 8u

__global__ void __launch_bounds__(256)
k_ba_page_sizes(BaBuildParams B) {
    __shared__ unsigned long long wsum[4];
    unsigned long long n_err = 0, n_cap = 0;
    for (uint32_t pg = blockIdx.x; pg < B.n_pages; pg += gridDim.x) {
        const uint64_t row0 = (uint64_t)pg * B.R;
        const uint64_t row1 = row0 + B.R < B.n_out ? row0 + B.R : B.n_out;
        unsigned long long sum = 0;
        for (uint64_t i = row0 + threadIdx.x; i < row1; i += blockDim.x) {
            const uint64_t a = B.group_start ? B.group_start[i] : i;
            const uint64_t b = B.group_start ? B.group_start[i + 1] : i + 1;
            bool skip = false;
            uint64_t len_sum = 0;
            if (a > b || b > B.n_src) {
                n_err++;
                skip = true;
            } else {
                for (uint64_t j = a; j < b; j++) {
                    const uint64_t h = B.handles[j];
                    const uint64_t off = h >> BA_LEN_BITS;
                    const uint64_t len = h & BA_LEN_MASK;
                    if (off > B.src_size || len > B.src_size - off) {
                        n_err++;
                        skip = true;
                    }
                    len_sum += len;
                }
                if (!skip && len_sum > BA_MAX_VALUE_LEN) {
                    n_cap++;
                    skip = true;
                }
            }
            B.row_len[i] = skip ? BA_ROW_SKIP : (uint32_t)len_sum;
            sum += 4 + (skip ? 0 : len_sum);
        }
        for (int m = 32; m > 0; m >>= 1) sum += __shfl_xor(sum, m);
        __syncthreads();   // the previous page's wsum is consumed
        if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = sum;
        __syncthreads();
        if (threadIdx.x == 0)
            B.page_size[pg] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
    }
    if (n_err) atomicAdd(&B.counts[0], n_err);
    if (n_cap) atomicAdd(&B.counts[1], n_cap);
}

// Kernel 1h: the byte sum (4 + len per row, 4 for a refused row)
// of every 1024-row batch of every row group, over the row_len the size pass
// left — what hx::ba_cut_pages needs to cut a value chunk into data pages.
// One wave per batch: 16 coalesced 4-byte loads per lane, a shuffle
// reduction, one u64 store by lane 0. Reads row_len[0, n_out) only, writes
// batch_sum[0, n_batches) only; no atomics. The sums equal
// hx::ba_batch_sizes_host.
__global__ void __launch_bounds__(256)
k_ba_batch_sizes(const uint32_t* __restrict__ row_len, uint32_t n_out,
                 uint32_t R, uint32_t per_group, uint32_t n_batches,
                 unsigned long long* __restrict__ batch_sum) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint32_t n_waves = (gridDim.x * blockDim.x) >> 6;
    for (uint32_t b = wave; b < n_batches; b += n_waves) {
        const uint64_t g = b / per_group, j = b % per_group;
        const uint64_t r0 = g * R + j * BA_CUT_BATCH;
        uint64_t r1 = r0 + BA_CUT_BATCH;
        if (r1 > (g + 1) * R) r1 = (g + 1) * R;
        if (r1 > n_out) r1 = n_out;
        unsigned long long sum = 0;
        for (uint64_t i = r0 + lane; i < r1; i += 64) {
            const uint32_t l = row_len[i];
            sum += 4ull + ((l & BA_ROW_SKIP) ? 0u : l);
        }
        for (int m = 32; m > 0; m >>= 1) sum += __shfl_xor(sum, m);
        if (lane == 0) batch_sum[b] = sum;
    }
}

// offs[i] = sum(size[0, i)), offs[n] = the total; k_snappy_scan's pattern.
__global__ void __launch_bounds__(256)
k_ba_page_scan(const unsigned long long* __restrict__ size, uint32_t n,
               unsigned long long* __restrict__ offs) {
    __shared__ unsigned long long part[256];
    const uint32_t t = threadIdx.x;
    unsigned long long carry = 0;
    for (uint32_t base = 0; base < n; base += 256) {
        const uint32_t i = base + t;
        const unsigned long long own = i < n ? size[i] : 0;
        part[t] = own;
        __syncthreads();
        for (uint32_t st = 1; st < 256; st <<= 1) {
            const unsigned long long add = t >= st ? part[t - st] : 0;
            __syncthreads();
            part[t] += add;
            __syncthreads();
        }
        if (i < n) offs[i] = carry + part[t] - own;
        carry += part[255];
        __syncthreads();
    }
    if (t == 0) offs[n] = carry;
}

// One lane copies len bytes: 8- or 4-byte words where d and s agree modulo
// the width, bytes up to d's alignment and at the end.
__device__ __forceinline__ void ba_lane_copy(uint8_t* d, const uint8_t* s,
                                             uint32_t len) {
    const uint32_t diff = uint32_t((uintptr_t)d ^ (uintptr_t)s);
    uint32_t i = 0;
    if ((diff & 7u) == 0 && len >= 8) {
        for (; i < len && ((uintptr_t)(d + i) & 7u); i++) d[i] = s[i];
        for (; i + 8 <= len; i += 8)
            *(uint64_t*)(d + i) = *(const uint64_t*)(s + i);
    } else if ((diff & 3u) == 0 && len >= 4) {
        for (; i < len && ((uintptr_t)(d + i) & 3u); i++) d[i] = s[i];
        for (; i + 4 <= len; i += 4)
            *(uint32_t*)(d + i) = *(const uint32_t*)(s + i);
    }
    for (; i < len; i++) d[i] = s[i];
}

// One tile of 256 rows of the page-offset scan kernels 1f and 1g share: v is
// the thread's row size (4 + len, 0 past the page's rows). Inclusive wave scan
// by shuffles, wave totals through LDS (wtot, 4 words), a carry from tile to
// tile (a page fits 31 bits, so u32 holds). Returns the row's offset in the
// page. Every thread of the block calls it.
__device__ __forceinline__ uint32_t ba_tile_scan(uint32_t v, uint32_t lane,
                                                 uint32_t wave, uint32_t* wtot,
                                                 uint32_t& carry) {
    uint32_t incl = v;
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint32_t x = __shfl_up(incl, d);
        if (lane >= d) incl += x;
    }
    __syncthreads();   // the previous tile's wtot is consumed
    if (lane == 63) wtot[wave] = incl;
    __syncthreads();
    uint32_t wbase = 0, tile = 0;
    for (uint32_t w = 0; w < 4; w++) {
        if (w < wave) wbase += wtot[w];
        tile += wtot[w];
    }
    const uint32_t o = carry + wbase + incl - v;
    carry += tile;
    return o;
}

__global__ void __launch_bounds__(256)
k_ba_build_pages(BaBuildParams B) {
    __shared__ uint32_t roff[BA_MAX_ROW_GROUP];   // row's offset in the page
    __shared__ uint32_t wtot[4];
    const uint32_t t = threadIdx.x;
    const uint32_t lane = t & 63u, wave = t >> 6;
    for (uint32_t pg = blockIdx.x; pg < B.n_pages; pg += gridDim.x) {
        const unsigned long long p0 = B.page_off[pg];
        const unsigned long long p_len = B.page_off[pg + 1] - p0;
        if (p_len > BA_MAX_PAGE_BYTES) continue;   // block-uniform
        const uint64_t row0 = (uint64_t)pg * B.R;
        const uint32_t rows = uint32_t(
            (row0 + B.R < B.n_out ? row0 + B.R : B.n_out) - row0);
        uint8_t* page = B.out + p0;

        // offsets (ba_tile_scan; p_len fits 31 bits)
        uint32_t carry = 0;
        for (uint32_t base = 0; base < rows; base += 256) {
            const uint32_t r = base + t;
            uint32_t v = 0;
            if (r < rows) {
                const uint32_t rl = B.row_len[row0 + r];
                v = 4u + ((rl & BA_ROW_SKIP) ? 0u : rl);
            }
            const uint32_t o = ba_tile_scan(v, lane, wave, wtot, carry);
            if (r < rows) roff[r] = o;
        }
        __syncthreads();

        // copy: each wave takes 64 rows at a time
        for (uint32_t c0 = wave * 64u; c0 < rows; c0 += 256u) {
            const uint32_t r = c0 + lane;
            uint32_t len = 0, a = 0, b = 0, o = 0;
            bool live = false;
            if (r < rows) {
                const uint32_t rl = B.row_len[row0 + r];
                o = roff[r];
                live = !(rl & BA_ROW_SKIP);
                len = live ? rl : 0u;
                // the slot must hold the row; always true for sizes that
                // came from k_ba_page_sizes over the same arrays
                if ((unsigned long long)o + 4u + len > p_len) {
                    live = false;
                } else {
                    uint8_t* d = page + o;
                    if (((uintptr_t)d & 3u) == 0) {
                        *(uint32_t*)d = len;
                    } else {
                        d[0] = uint8_t(len);
                        d[1] = uint8_t(len >> 8);
                        d[2] = uint8_t(len >> 16);
                        d[3] = uint8_t(len >> 24);
                    }
                }
                a = B.group_start ? B.group_start[row0 + r]
                                  : uint32_t(row0 + r);
                b = B.group_start ? B.group_start[row0 + r + 1] : a + 1u;
                if (len == 0) live = false;
            }
            const bool own = live && len < BA_LANE_MAX_BYTES &&
                             b - a <= BA_LANE_MAX_PARTS;
            if (own) {
                uint8_t* d = page + o + 4u;
                uint32_t pos = 0;
                for (uint32_t j = a; j < b; j++) {
                    const uint64_t h = B.handles[j];
                    const uint64_t off = h >> BA_LEN_BITS;
                    const uint32_t l = uint32_t(h & BA_LEN_MASK);
                    if (off > B.src_size || l > B.src_size - off ||
                        l > len - pos)
                        break;
                    ba_lane_copy(d + pos, B.src + off, l);
                    pos += l;
                }
            }
            unsigned long long coop = __ballot(live && !own);
            while (coop) {
                const int k = __ffsll(coop) - 1;
                coop &= coop - 1ull;
                const uint32_t ka = __shfl(a, k), kb = __shfl(b, k);
                const uint32_t klen = __shfl(len, k);
                uint8_t* d = page + __shfl(o, k) + 4u;
                uint32_t pos = 0;
                for (uint32_t j = ka; j < kb; j++) {
                    const uint64_t h = B.handles[j];   // wave-uniform
                    const uint64_t off = h >> BA_LEN_BITS;
                    const uint32_t l = uint32_t(h & BA_LEN_MASK);
                    if (off > B.src_size || l > B.src_size - off ||
                        l > klen - pos)
                        break;
                    sc_copy(d + pos, B.src + off, l, lane, 64);
                    pos += l;
                }
            }
        }
        __syncthreads();   // roff is rewritten by the next page
    }
}

// ---------------------------------------------------------------------------
// Kernel 1g: footer statistics of the page images kernel 1f
// built, so the images need not reach the host for them. One workgroup per
// page; ba_pages.h states the rule (keys of at most 65 bytes decide) and
// holds the host twin, hx::ba_page_minmax_host. Row offsets come from the
// build pass's tile scan; each thread folds its rows into a running min and
// max, kept as (offset of the value in the page, key length, first key word);
// keys compare as zero-padded big-endian 8-byte words, then by key length.
// The four waves reduce by shuffles, then through LDS; 64 threads copy the
// min, 64 the max. Reads stay inside the page's own [page_off[g],
// page_off[g + 1]): a key word is assembled from the aligned words around it
// where both lie in the page, from the value's bytes otherwise, and masked to
// the value's own bytes. Writes only the page's BaPageStat; plain vector
// stores, no atomics.
// ---------------------------------------------------------------------------
struct BaKey {
    uint32_t off;    // of the value's first byte in the page
    uint32_t klen;   // min(len, 65)
    uint64_t w0;     // key word 0
};

// key word w (bytes [8w, 8w + 8) of the key, zero past klen), big-endian
__device__ __forceinline__ uint64_t ba_key_word(const uint8_t* page,
                                                uint32_t p_len, uint32_t off,
                                                uint32_t klen, uint32_t w) {
    if (klen <= 8u * w) return 0;
    const uint32_t n = klen - 8u * w < 8u ? klen - 8u * w : 8u;
    const uint8_t* p = page + off + 8u * w;
    const uint32_t mis = uint32_t((uintptr_t)p & 7u);
    const uint8_t* a = p - mis;
    uint64_t v;
    if (a >= page && a + (mis ? 16u : 8u) <= page + p_len) {
        v = *(const uint64_t*)a;
        if (mis)
            v = (v >> (mis * 8u)) |
                (*(const uint64_t*)(a + 8) << (64u - mis * 8u));
    } else {
        v = 0;
        for (uint32_t b = 0; b < n; b++) v |= (uint64_t)p[b] << (8u * b);
    }
    if (n < 8u) v &= (1ull << (8u * n)) - 1ull;
    return __builtin_bswap64(v);
}

__device__ __forceinline__ bool ba_key_lt(const uint8_t* page, uint32_t p_len,
                                          const BaKey& a, const BaKey& b) {
    if (a.w0 != b.w0) return a.w0 < b.w0;
    const uint32_t top = a.klen > b.klen ? a.klen : b.klen;
    for (uint32_t w = 1; 8u * w < top; w++) {
        const uint64_t x = ba_key_word(page, p_len, a.off, a.klen, w);
        const uint64_t y = ba_key_word(page, p_len, b.off, b.klen, w);
        if (x != y) return x < y;
    }
    return a.klen < b.klen;
}

__device__ __forceinline__ BaKey ba_key_shfl_xor(const BaKey& k, int m) {
    BaKey o;
    o.off = __shfl_xor(k.off, m);
    o.klen = __shfl_xor(k.klen, m);
    o.w0 = __shfl_xor(k.w0, m);
    return o;
}

__global__ void __launch_bounds__(256)
k_ba_page_minmax(const uint8_t* __restrict__ image,
                 const unsigned long long* __restrict__ page_off,
                 const uint32_t* __restrict__ row_len, uint32_t n_out,
                 uint32_t R, uint32_t n_pages, BaPageStat* __restrict__ out) {
    __shared__ uint32_t wtot[4];
    __shared__ BaKey wmin[4], wmax[4];
    __shared__ uint32_t wany[4];
    const uint32_t t = threadIdx.x;
    const uint32_t lane = t & 63u, wave = t >> 6;
    for (uint32_t pg = blockIdx.x; pg < n_pages; pg += gridDim.x) {
        const unsigned long long p0 = page_off[pg];
        const unsigned long long p_len64 = page_off[pg + 1] - p0;
        const uint64_t row0 = (uint64_t)pg * R;
        const uint32_t rows = uint32_t(
            (row0 + R < n_out ? row0 + R : n_out) - row0);
        const bool page_ok = p_len64 <= BA_MAX_PAGE_BYTES;   // block-uniform
        const uint32_t p_len = page_ok ? (uint32_t)p_len64 : 0u;
        const uint8_t* page = image + p0;
        BaKey mn{0, 0, 0}, mx{0, 0, 0};
        bool any = false;
        uint32_t carry = 0;
        for (uint32_t base = 0; page_ok && base < rows; base += 256) {
            const uint32_t r = base + t;
            uint32_t v = 0, len = 0;
            if (r < rows) {
                const uint32_t rl = row_len[row0 + r];
                len = (rl & BA_ROW_SKIP) ? 0u : rl;
                v = 4u + len;
            }
            const uint32_t o = ba_tile_scan(v, lane, wave, wtot, carry);
            if (r < rows && (unsigned long long)o + v <= p_len) {
                BaKey k;
                k.off = o + 4u;
                k.klen = len < BA_STAT_MAX + 1u ? len : BA_STAT_MAX + 1u;
                k.w0 = ba_key_word(page, p_len, k.off, k.klen, 0);
                if (!any || ba_key_lt(page, p_len, k, mn)) mn = k;
                if (!any || ba_key_lt(page, p_len, mx, k)) mx = k;
                any = true;
            }
        }
        // across the wave, then the four waves
        for (int m = 32; m > 0; m >>= 1) {
            const BaKey omn = ba_key_shfl_xor(mn, m);
            const BaKey omx = ba_key_shfl_xor(mx, m);
            const bool oany = __shfl_xor((int)any, m) != 0;
            if (oany) {
                if (!any || ba_key_lt(page, p_len, omn, mn)) mn = omn;
                if (!any || ba_key_lt(page, p_len, mx, omx)) mx = omx;
                any = true;
            }
        }
        __syncthreads();   // the previous page's wmin / wmax are consumed
        if (lane == 0) {
            wmin[wave] = mn;
            wmax[wave] = mx;
            wany[wave] = any ? 1u : 0u;
        }
        __syncthreads();
        // every thread folds the four entries the same way
        bool f_any = false;
        BaKey f_mn{0, 0, 0}, f_mx{0, 0, 0};
        for (uint32_t w = 0; w < 4; w++) {
            if (!wany[w]) continue;
            const BaKey a = wmin[w], b = wmax[w];
            if (!f_any || ba_key_lt(page, p_len, a, f_mn)) f_mn = a;
            if (!f_any || ba_key_lt(page, p_len, f_mx, b)) f_mx = b;
            f_any = true;
        }
        const bool has = f_any && f_mn.klen <= BA_STAT_MAX &&
                         f_mx.klen <= BA_STAT_MAX;
        BaPageStat* st = out + pg;
        if (t == 0) {
            st->has = has ? 1u : 0u;
            st->min_len = has ? f_mn.klen : 0u;
            st->max_len = has ? f_mx.klen : 0u;
        }
        if (t < 2u * BA_STAT_MAX) {
            const bool is_max = t >= BA_STAT_MAX;
            const uint32_t i = is_max ? t - BA_STAT_MAX : t;
            const BaKey& k = is_max ? f_mx : f_mn;
            const uint8_t b = (has && i < k.klen) ? page[k.off + i]
                                                  : (uint8_t)0;
            (is_max ? st->max : st->min)[i] = b;
        }
    }
}

// Append compaction, behind the sort: equal-PK runs of the sorted rows.
// flag[i] = 1 where row i opens a run.
__global__ void __launch_bounds__(256)
k_group_flags(const unsigned long long* __restrict__ series,
              const unsigned long long* __restrict__ ts, uint32_t n,
              uint32_t* __restrict__ flag) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += blockDim.x * gridDim.x)
        flag[i] = (i == 0 || series[i] != series[i - 1] ||
                   ts[i] != ts[i - 1]) ? 1u : 0u;
}

// rank[i] = exclusive scan of flag. Run g opens at row group_start[g]; its
// series, ts and (seq_key given) the sequence of its FIRST row, the smallest
// of the run, go to the head columns. group_start[n_out] = n and *n_out are
// written by the last row's thread.
__global__ void __launch_bounds__(256)
k_group_heads(const uint32_t* __restrict__ flag,
              const uint32_t* __restrict__ rank,
              const unsigned long long* __restrict__ series,
              const unsigned long long* __restrict__ ts,
              const unsigned long long* __restrict__ seq_key,
              const uint32_t* __restrict__ perm, uint32_t n,
              uint32_t* __restrict__ group_start,
              unsigned long long* __restrict__ head_series,
              unsigned long long* __restrict__ head_ts,
              unsigned long long* __restrict__ head_seq,
              unsigned long long* __restrict__ n_out) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += blockDim.x * gridDim.x) {
        const uint32_t g = rank[i];
        if (flag[i]) {
            group_start[g] = i;
            head_series[g] = series[i];
            head_ts[g] = ts[i];
            if (seq_key) head_seq[g] = seq_key[perm[i]] >> 32;
        }
        if (i == n - 1) {
            group_start[g + flag[i]] = n;
            *n_out = g + flag[i];
        }
    }
}

static uint32_t grid_for(uint32_t work, uint32_t per_block) {
    uint32_t g = (work + per_block - 1) / per_block;
    return g == 0 ? 1 : (g > 2048u ? 2048u : g);
}

hipError_t launch_decode_delta(hipStream_t s, const uint8_t* blob, uint8_t* dec,
                               const DeltaPageDesc* pages, uint32_t n_pages,
                               unsigned long long* err_flag) {
    uint32_t grid = n_pages > 4096 ? 4096 : n_pages;
    hipLaunchKernelGGL(k_decode_delta_i64, dim3(grid), dim3(256), 0, s,
                       blob, dec, pages, n_pages, err_flag);
    return hipGetLastError();
}

hipError_t launch_rledict(hipStream_t s, const uint8_t* blob, uint8_t* dec,
                          const RleDictPageDesc* pages, uint32_t n_pages,
                          unsigned long long* err_flag) {
    uint32_t grid = n_pages > 4096 ? 4096 : (n_pages ? n_pages : 1);
    hipLaunchKernelGGL(k_decode_rledict, dim3(grid), dim3(256), 0, s,
                       blob, dec, pages, n_pages, err_flag);
    return hipGetLastError();
}

hipError_t launch_snappy(hipStream_t s, const uint8_t* blob, uint8_t* dec,
                         const SnappyPageDesc* pages, uint32_t n_pages,
                         unsigned long long* err_flag) {
    uint32_t waves_needed = n_pages;
    uint32_t blocks = (waves_needed + 3) / 4;  // 4 waves per 256-thread block
    if (blocks > 8192) blocks = 8192;
    if (blocks == 0) blocks = 1;
    // decode is 31% issue-busy / 62% parked at the unconstrained 111 VGPRs
    // (16 waves/CU) — unlike the aggregate it benefits from occupancy;
    // HX_SNAPPY_MINW selects. Default 6 (24 waves/CU, 440 B scratch):
    // measured best in two same-box headline A/Bs (26.1 vs 27.0/27.1 ms
    // per step against MINW 1/5 at pipeline 3; 30.4 vs 31.0/31.3 solo) —
    // the extra waves buy more than the spill costs. Re-checked after the
    // direct-run rewrite (576 B scratch at 6): 5/6/7 within run-to-run
    // spread of each other, no value wins every pair — stays 6.
    int minw = 6;
    if (const char* e = getenv("HX_SNAPPY_MINW")) minw = atoi(e);
    if (minw >= 8)
        hipLaunchKernelGGL(k_snappy_decompress<8>, dim3(blocks), dim3(256),
                           0, s, blob, dec, pages, n_pages, err_flag);
    else if (minw == 7)
        hipLaunchKernelGGL(k_snappy_decompress<7>, dim3(blocks), dim3(256),
                           0, s, blob, dec, pages, n_pages, err_flag);
    else if (minw == 6)
        hipLaunchKernelGGL(k_snappy_decompress<6>, dim3(blocks), dim3(256),
                           0, s, blob, dec, pages, n_pages, err_flag);
    else if (minw == 5)
        hipLaunchKernelGGL(k_snappy_decompress<5>, dim3(blocks), dim3(256),
                           0, s, blob, dec, pages, n_pages, err_flag);
    else
        hipLaunchKernelGGL(k_snappy_decompress<1>, dim3(blocks), dim3(256),
                           0, s, blob, dec, pages, n_pages, err_flag);
    return hipGetLastError();
}

hipError_t launch_snappy_compress(hipStream_t s, const uint8_t* src,
                                  uint8_t* dst, const SnappyCompDesc* pages,
                                  uint32_t n_pages, uint32_t* out_len,
                                  unsigned long long* err_flag) {
    if (n_pages == 0) return hipSuccess;
    // one wave per page, 16 KB of LDS each: 10 blocks fit a CU
    const uint32_t grid = n_pages > 65536u ? 65536u : n_pages;
    hipLaunchKernelGGL(k_snappy_compress, dim3(grid), dim3(64), 0, s, src,
                       dst, pages, n_pages, out_len, err_flag);
    return hipGetLastError();
}

hipError_t launch_page_minmax(hipStream_t s, const uint8_t* src,
                              const SnappyCompDesc* pages,
                              const uint32_t* kinds, uint32_t n_pages,
                              PageStat* out) {
    if (n_pages == 0) return hipSuccess;
    const uint32_t grid = n_pages > 65536u ? 65536u : n_pages;
    hipLaunchKernelGGL(k_page_minmax, dim3(grid), dim3(64), 0, s, src, pages,
                       kinds, n_pages, out);
    return hipGetLastError();
}

hipError_t launch_snappy_pack(hipStream_t s, const uint8_t* slots,
                              const SnappyCompDesc* pages, uint32_t n_pages,
                              const uint32_t* out_len,
                              unsigned long long* offs, uint8_t* packed) {
    if (n_pages == 0) return hipSuccess;
    hipLaunchKernelGGL(k_snappy_scan, dim3(1), dim3(256), 0, s, out_len,
                       n_pages, offs);
    const uint32_t grid = n_pages > 65536u ? 65536u : n_pages;
    hipLaunchKernelGGL(k_snappy_pack, dim3(grid), dim3(256), 0, s, slots,
                       pages, n_pages, out_len, offs, packed);
    return hipGetLastError();
}

hipError_t launch_expand_optional(hipStream_t s, const uint8_t* blob,
                                  uint8_t* dec, const ExpandPageDesc* pages,
                                  uint32_t n_pages,
                                  unsigned long long* err_flag) {
    uint32_t grid = n_pages > 65535 ? 65535 : n_pages;
    hipLaunchKernelGGL(k_expand_optional, dim3(grid), dim3(256), 0, s,
                       blob, dec, dec, pages, n_pages, err_flag);
    return hipGetLastError();
}

hipError_t launch_pack_optional(hipStream_t s,
                                const unsigned long long* val_src,
                                const void* valid_src, bool valid_bits,
                                const uint32_t* perm, uint32_t n_src,
                                uint32_t n, uint32_t row_group,
                                unsigned long long* packed_out,
                                uint64_t* bitmap_out, uint32_t* n_valid,
                                unsigned long long* err_flag) {
    if (row_group == 0 || (row_group & 63u)) return hipErrorInvalidValue;
    if (n == 0) return hipSuccess;
    const uint64_t n_groups = ((uint64_t)n + row_group - 1) / row_group;
    const uint32_t grid = n_groups > 65535 ? 65535u : (uint32_t)n_groups;
    if (valid_bits)
        hipLaunchKernelGGL(k_pack_optional<true>, dim3(grid), dim3(256), 0, s,
                           val_src, valid_src, perm, n_src, n, row_group,
                           packed_out, bitmap_out, n_valid, err_flag);
    else
        hipLaunchKernelGGL(k_pack_optional<false>, dim3(grid), dim3(256), 0,
                           s, val_src, valid_src, perm, n_src, n, row_group,
                           packed_out, bitmap_out, n_valid, err_flag);
    return hipGetLastError();
}

hipError_t launch_copy_u64(hipStream_t s, const uint8_t* blob, uint8_t* dec,
                           const CopyDesc* descs, uint32_t n_descs) {
    uint32_t grid = n_descs > 4096 ? 4096 : n_descs;
    hipLaunchKernelGGL(k_copy_u64, dim3(grid), dim3(256), 0, s,
                       blob, dec, dec, descs, n_descs);
    return hipGetLastError();
}

hipError_t launch_scan_agg(hipStream_t s, const AggParams& p, uint32_t grid,
                           bool nulls, bool ts) {
    if (grid == 0) grid = p.n_rgs > 65535 ? 65535 : (p.n_rgs ? p.n_rgs : 1);
    // NULLS is a launch-level template parameter, as for the range kernel:
    // a wrapper around one shared body costs the null-off instance 3 VGPRs.
    // MM likewise: the ordered-word min/max reduction is compiled into the
    // instances a min/max query launches and into no other.
    const bool mm = (p.ops & (HXK_MIN | HXK_MAX)) != 0;
    if (ts) {   // TS implies MM: the time words ride the min/max slots
        if (!mm) return hipErrorInvalidValue;
        if (nulls)
            hipLaunchKernelGGL((k_scan_agg<true, true, true>), dim3(grid),
                               dim3(256), 0, s, p);
        else
            hipLaunchKernelGGL((k_scan_agg<false, true, true>), dim3(grid),
                               dim3(256), 0, s, p);
    } else if (nulls && mm)
        hipLaunchKernelGGL((k_scan_agg<true, true, false>), dim3(grid),
                           dim3(256), 0, s, p);
    else if (nulls)
        hipLaunchKernelGGL((k_scan_agg<true, false, false>), dim3(grid),
                           dim3(256), 0, s, p);
    else if (mm)
        hipLaunchKernelGGL((k_scan_agg<false, true, false>), dim3(grid),
                           dim3(256), 0, s, p);
    else
        hipLaunchKernelGGL((k_scan_agg<false, false, false>), dim3(grid),
                           dim3(256), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_sample_series(hipStream_t s, const RgDesc* rgs,
                                uint32_t n_rgs, const uint8_t* blob,
                                const uint8_t* dec, uint64_t* out) {
    uint32_t blocks = (n_rgs * 64 + 255) / 256;
    if (blocks > 65535) blocks = 65535;
    if (blocks == 0) blocks = 1;
    hipLaunchKernelGGL(k_sample_series, dim3(blocks), dim3(256), 0, s, rgs,
                       n_rgs, blob, dec, out);
    return hipGetLastError();
}

hipError_t launch_range_bounds(hipStream_t s, const AggParams& p,
                               const RangeAux& r, uint64_t* out) {
    const uint64_t total_waves = (uint64_t)(r.n_blocks + 1) * r.n_ssts;
    uint64_t blocks = (total_waves + 3) / 4;   // 4 waves per 256-thread block
    if (blocks > 262144) blocks = 262144;
    if (blocks == 0) blocks = 1;
    hipLaunchKernelGGL(k_range_bounds, dim3((uint32_t)blocks), dim3(256), 0,
                       s, p, r, out);
    return hipGetLastError();
}

template <bool MM, bool NULLS, bool TS>
static hipError_t launch_range2_inst(hipStream_t s, const AggParams& p,
                                     const RangeAux& r, const RangeOut& o) {
    // per slot: key 8 + sum 8 + cnt 4 [+ min 8 + max 8] + sort index 2
    const size_t lds = (size_t)r.ne * (MM ? 38 : 22);
    if (lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(
            reinterpret_cast<const void*>(&k_scan_agg_range2<MM, NULLS, TS>),
            hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL((k_scan_agg_range2<MM, NULLS, TS>), dim3(r.n_blocks),
                       dim3(256), lds, s, p, r, o);
    return hipGetLastError();
}

hipError_t launch_scan_agg_range2(hipStream_t s, const AggParams& p,
                                  const RangeAux& r, bool minmax,
                                  bool nulls, const RangeOut& out,
                                  bool ts) {
    // the sort permutation is u16 and the slot mask needs a power of two
    if (r.ne == 0 || (r.ne & (r.ne - 1)) || r.ne > 32768u)
        return hipErrorInvalidValue;
    if (ts) {   // TS implies MM
        if (!minmax) return hipErrorInvalidValue;
        return nulls ? launch_range2_inst<true, true, true>(s, p, r, out)
                     : launch_range2_inst<true, false, true>(s, p, r, out);
    }
    if (nulls)
        return minmax ? launch_range2_inst<true, true, false>(s, p, r, out)
                      : launch_range2_inst<false, true, false>(s, p, r, out);
    return minmax ? launch_range2_inst<true, false, false>(s, p, r, out)
                  : launch_range2_inst<false, false, false>(s, p, r, out);
}

hipError_t launch_place_runs(hipStream_t s, const RangePlace& q) {
    if (q.n_blocks == 0 || q.n_blocks > 131072u) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_place_scan, dim3(1), dim3(1024), 0, s, q);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_place_runs, dim3(grid_for(q.n_blocks, 4)), dim3(256),
                       0, s, q);
    return hipGetLastError();
}

hipError_t launch_resolve_first_last(hipStream_t s, const AggParams& p,
                                     const ResolveParams& q, bool nulls) {
    if (q.ng == 0 || !q.gkey || !q.err || (!q.ofirst && !q.olast) ||
        (q.ofirst && !q.tmin) || (q.olast && !q.tmax))
        return hipErrorInvalidValue;
    const uint32_t grid = p.n_rgs > 65535 ? 65535 : (p.n_rgs ? p.n_rgs : 1);
    if (nulls)
        hipLaunchKernelGGL((k_resolve_first_last<true>), dim3(grid),
                           dim3(256), 0, s, p, q);
    else
        hipLaunchKernelGGL((k_resolve_first_last<false>), dim3(grid),
                           dim3(256), 0, s, p, q);
    return hipGetLastError();
}

hipError_t launch_map_words(hipStream_t s, unsigned long long* w, size_t n,
                            bool to_ts) {
    if (n == 0) return hipSuccess;
    size_t blocks = (n + 255) / 256;
    if (blocks > 65535) blocks = 65535;
    hipLaunchKernelGGL(k_map_words, dim3((uint32_t)blocks), dim3(256), 0, s,
                       w, n, to_ts ? 1u : 0u);
    return hipGetLastError();
}

hipError_t launch_scan_rows(hipStream_t s, const AggParams& p,
                            uint32_t rg_first, uint32_t rg_last,
                            uint64_t* out_series, long long* out_ts,
                            double* out_value, unsigned long long* cursor,
                            unsigned long long cap, uint64_t* out_seq,
                            int32_t seq_rowidx, uint64_t* out_valid) {
    ScanRowsParams R;
    R.P = p;
    R.rg_first = rg_first;
    R.rg_last = rg_last;
    R.out_series = out_series;
    R.out_ts = out_ts;
    R.out_value = out_value;
    R.out_seq = out_seq;
    R.seq_rowidx = seq_rowidx;
    R._pad = 0;
    R.cursor = cursor;
    R.cap = cap;
    R.out_valid = out_valid;
    uint32_t n = rg_last - rg_first;
    hipLaunchKernelGGL(k_scan_rows, dim3(n > 4096 ? 4096 : (n ? n : 1)),
                       dim3(256), 0, s, R);
    return hipGetLastError();
}

hipError_t launch_gather_multi(hipStream_t s,
                               const unsigned long long* const* srcs,
                               uint32_t n_arrays, const uint32_t* perm,
                               unsigned long long* dst, uint32_t n) {
    GatherMulti g{};
    for (uint32_t a = 0; a < n_arrays && a < 8; a++) g.src[a] = srcs[a];
    g.dst = dst;
    g.perm = perm;
    g.n = n;
    g.n_arrays = n_arrays;
    hipLaunchKernelGGL(k_gather_multi, dim3(grid_for(n, 256)), dim3(256), 0, s, g);
    return hipGetLastError();
}

hipError_t launch_compact(hipStream_t s, const AggTable& t, uint32_t n_slots,
                          int32_t key_claim, int64_t bucket_ms,
                          int64_t lo_bucket, uint32_t n_buckets,
                          uint32_t bstride, const uint8_t* bstore,
                          const CompactOut& o, uint32_t* scratch) {
    CompactParams C;
    C.table = t;
    C.n_slots = n_slots;
    C.key_claim = key_claim;
    C.bucket_ms = bucket_ms;
    C.lo_bucket = lo_bucket;
    C.n_buckets = n_buckets;
    C.bstride = bstride;
    C.bstore = bstore;
    C.out_series = o.series;
    C.out_bucket = o.bucket;
    C.out_sum = o.sum;
    C.out_cnt = o.cnt;
    C.out_min = o.vmin;
    C.out_max = o.vmax;
    C.n_out = o.n_out;
    const size_t total =
        n_buckets ? (size_t)n_slots * n_buckets : (size_t)n_slots;
    const uint32_t grid =
        total > (size_t)2048 * 256
            ? 2048u
            : (uint32_t)((total + 255) / 256 ? (total + 255) / 256 : 1);
    // two-phase compaction (count -> scan -> write) avoids the single hot
    // n_out counter (~250k serialized agent-scope RMWs = ~3 ms at headline
    // fill). scratch = 2*grid u32 (counts, bases). NON-BUCKET ONLY: the
    // bucket sweep walks slots x n_buckets positions at low live fraction,
    // and doubling that sweep measured ~5% SLOWER than the single-pass
    // kernel's atomics (201.8 vs 192.9 ms/step same-box) — the storm is
    // proportional to LIVE waves, which bucket sweeps have few of.
    if (n_buckets == 0) {
        uint32_t* counts = scratch;
        uint32_t* bases = scratch + grid;
        hipLaunchKernelGGL(k_compact_count, dim3(grid), dim3(256), 0, s,
                           C, counts);
        hipLaunchKernelGGL(k_scan_counts, dim3(1), dim3(256), 0, s,
                           counts, grid, bases, C.n_out);
        hipLaunchKernelGGL(k_compact_write, dim3(grid), dim3(256), 0, s,
                           C, bases);
        return hipGetLastError();
    }
    hipLaunchKernelGGL(k_compact, dim3(grid), dim3(256), 0, s, C);
    return hipGetLastError();
}

hipError_t launch_gather_u64(hipStream_t s, const unsigned long long* in,
                             const uint32_t* perm, unsigned long long* out,
                             uint32_t n) {
    hipLaunchKernelGGL(k_gather_u64, dim3(grid_for(n, 256)), dim3(256), 0, s,
                       in, perm, out, n);
    return hipGetLastError();
}

hipError_t launch_avg(hipStream_t s, const double* sum,
                      const unsigned long long* cnt, double* avg, uint32_t n) {
    hipLaunchKernelGGL(k_avg, dim3(grid_for(n, 256)), dim3(256), 0, s,
                       sum, cnt, avg, n);
    return hipGetLastError();
}

extern "C" __global__ void __launch_bounds__(256)
k_xor_sign(unsigned long long* buf, uint32_t n) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += blockDim.x * gridDim.x)
        buf[i] ^= 0x8000000000000000ull;
}

hipError_t launch_xor_sign(hipStream_t s, unsigned long long* buf, uint32_t n) {
    hipLaunchKernelGGL(k_xor_sign, dim3(grid_for(n, 256)), dim3(256), 0, s, buf, n);
    return hipGetLastError();
}

hipError_t launch_seg_keys(hipStream_t s, const long long* ts, long long seg_ms,
                           unsigned long long* keys, uint32_t n) {
    hipLaunchKernelGGL(k_seg_keys, dim3(grid_for(n, 256)), dim3(256), 0, s,
                       ts, seg_ms, keys, n);
    return hipGetLastError();
}

hipError_t launch_init_slab(hipStream_t s, uint8_t* slab, uint32_t n_slots,
                            uint32_t stride) {
    hipLaunchKernelGGL(k_init_slab, dim3(grid_for(n_slots, 256)), dim3(256),
                       0, s, slab, n_slots, stride);
    return hipGetLastError();
}

hipError_t launch_init_state_slab(hipStream_t s, uint8_t* slab,
                                  uint32_t n_slots, uint32_t stride, bool mm) {
    hipLaunchKernelGGL(k_init_state_slab, dim3(grid_for(n_slots, 256)),
                       dim3(256), 0, s, slab, n_slots, stride, mm ? 1u : 0u);
    return hipGetLastError();
}

hipError_t launch_init_accum_rows(hipStream_t s, uint8_t* rows,
                                  size_t total_rows, uint32_t stride,
                                  bool mm) {
    hipLaunchKernelGGL(k_init_accum_rows,
                       dim3(grid_for((uint32_t)std::min<size_t>(
                                         total_rows, 0x7FFFFFFF), 256)),
                       dim3(256), 0, s, rows, total_rows, stride,
                       mm ? 1u : 0u);
    return hipGetLastError();
}

hipError_t launch_iota(hipStream_t s, uint32_t* out, uint32_t n) {
    hipLaunchKernelGGL(k_iota, dim3(grid_for(n, 256)), dim3(256), 0, s, out, n);
    return hipGetLastError();
}

hipError_t launch_copy_bytes(hipStream_t s, const uint8_t* blob,
                             const uint64_t* handles, const int64_t* dst_off,
                             uint8_t* out, uint32_t n) {
    CopyBytesParams C{blob, handles, dst_off, out, n};
    hipLaunchKernelGGL(k_copy_bytes, dim3(grid_for(n, 256)), dim3(256), 0, s,
                       C);
    return hipGetLastError();
}

hipError_t launch_ba_offsets(hipStream_t s, const uint8_t* blob,
                             const BaPageDesc* pages, uint32_t n_pages,
                             uint64_t* out, unsigned long long* err_flag) {
    hipLaunchKernelGGL(k_ba_offsets, dim3(grid_for(n_pages, 256)), dim3(256),
                       0, s, blob, pages, n_pages, out, err_flag);
    return hipGetLastError();
}

hipError_t launch_tag_filter(hipStream_t s, const TagFilterParams& f) {
    uint32_t work = (uint32_t)std::min<int64_t>(f.n_rows, 0x7FFFFFFF);
    hipLaunchKernelGGL(k_tag_filter, dim3(grid_for(work, 256)), dim3(256), 0,
                       s, f);
    return hipGetLastError();
}

hipError_t launch_tsid_intersect(hipStream_t s, const uint64_t* a,
                                 unsigned long long n_a, const uint64_t* b,
                                 unsigned long long n_b, uint64_t* out,
                                 unsigned long long* cursor) {
    uint32_t work = (uint32_t)std::min<unsigned long long>(n_a, 0x7FFFFFFF);
    hipLaunchKernelGGL(k_tsid_intersect, dim3(grid_for(work, 256)), dim3(256),
                       0, s, a, n_a, b, n_b, out, cursor);
    return hipGetLastError();
}

hipError_t launch_unique_u64(hipStream_t s, const uint64_t* in,
                             unsigned long long n, uint64_t* out,
                             unsigned long long* cursor) {
    uint32_t work = (uint32_t)std::min<unsigned long long>(n, 0x7FFFFFFF);
    hipLaunchKernelGGL(k_unique_u64, dim3(grid_for(work, 256)), dim3(256), 0,
                       s, in, n, out, cursor);
    return hipGetLastError();
}

hipError_t launch_ba_page_sizes(hipStream_t s, uint64_t src_size,
                                const uint64_t* handles,
                                const uint32_t* group_start, uint32_t n_src,
                                uint32_t n_out, uint32_t row_group,
                                uint32_t* row_len,
                                unsigned long long* page_size,
                                unsigned long long* page_off,
                                unsigned long long* counts) {
    if (row_group == 0 || row_group > BA_MAX_ROW_GROUP)
        return hipErrorInvalidValue;
    const uint32_t n_pages = (uint32_t)ba_n_pages(n_out, row_group);
    BaBuildParams B{};
    B.src_size = src_size;
    B.handles = handles;
    B.group_start = group_start;
    B.n_src = n_src;
    B.n_out = n_out;
    B.R = row_group;
    B.n_pages = n_pages;
    B.row_len = row_len;
    B.page_size = page_size;
    B.page_off = page_off;
    B.counts = counts;
    if (n_pages)
        hipLaunchKernelGGL(k_ba_page_sizes,
                           dim3(n_pages > 65536u ? 65536u : n_pages),
                           dim3(256), 0, s, B);
    hipLaunchKernelGGL(k_ba_page_scan, dim3(1), dim3(256), 0, s, page_size,
                       n_pages, page_off);
    return hipGetLastError();
}

hipError_t launch_ba_build_pages(hipStream_t s, const uint8_t* src,
                                 uint64_t src_size, const uint64_t* handles,
                                 const uint32_t* group_start, uint32_t n_src,
                                 uint32_t n_out, uint32_t row_group,
                                 const uint32_t* row_len,
                                 const unsigned long long* page_off,
                                 uint8_t* out) {
    if (row_group == 0 || row_group > BA_MAX_ROW_GROUP)
        return hipErrorInvalidValue;
    const uint32_t n_pages = (uint32_t)ba_n_pages(n_out, row_group);
    if (n_pages == 0) return hipSuccess;
    BaBuildParams B{};
    B.src = src;
    B.src_size = src_size;
    B.handles = handles;
    B.group_start = group_start;
    B.n_src = n_src;
    B.n_out = n_out;
    B.R = row_group;
    B.n_pages = n_pages;
    B.row_len = const_cast<uint32_t*>(row_len);
    B.page_off = const_cast<unsigned long long*>(page_off);
    B.out = out;
    hipLaunchKernelGGL(k_ba_build_pages,
                       dim3(n_pages > 65536u ? 65536u : n_pages), dim3(256),
                       0, s, B);
    return hipGetLastError();
}

hipError_t launch_ba_batch_sizes(hipStream_t s, const uint32_t* row_len,
                                 uint32_t n_out, uint32_t row_group,
                                 unsigned long long* batch_sum) {
    if (row_group == 0 || row_group > BA_MAX_ROW_GROUP)
        return hipErrorInvalidValue;
    const uint32_t n_b = (uint32_t)ba_n_batches(n_out, row_group);
    if (n_b == 0) return hipSuccess;
    const uint32_t blocks = (n_b + 3u) / 4u;   // four waves, a batch each
    hipLaunchKernelGGL(k_ba_batch_sizes,
                       dim3(blocks > 65536u ? 65536u : blocks), dim3(256), 0,
                       s, row_len, n_out, row_group,
                       (uint32_t)ba_batches_per_group(row_group), n_b,
                       batch_sum);
    return hipGetLastError();
}

hipError_t launch_ba_page_minmax(hipStream_t s, const uint8_t* image,
                                 const unsigned long long* page_off,
                                 const uint32_t* row_len, uint32_t n_out,
                                 uint32_t row_group, BaPageStat* out) {
    if (row_group == 0 || row_group > BA_MAX_ROW_GROUP)
        return hipErrorInvalidValue;
    const uint32_t n_pages = (uint32_t)ba_n_pages(n_out, row_group);
    if (n_pages == 0) return hipSuccess;
    hipLaunchKernelGGL(k_ba_page_minmax,
                       dim3(n_pages > 65536u ? 65536u : n_pages), dim3(256),
                       0, s, image, page_off, row_len, n_out, row_group,
                       n_pages, out);
    return hipGetLastError();
}

hipError_t launch_group_heads(hipStream_t s, const unsigned long long* series,
                              const unsigned long long* ts,
                              const unsigned long long* seq_key,
                              const uint32_t* perm, uint32_t n,
                              uint32_t* flag, uint32_t* rank,
                              uint32_t* group_start,
                              unsigned long long* head_series,
                              unsigned long long* head_ts,
                              unsigned long long* head_seq,
                              unsigned long long* n_out, void** d_temp,
                              size_t* temp_bytes) {
    if (n == 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_group_flags, dim3(grid_for(n, 256)), dim3(256), 0, s,
                       series, ts, n, flag);
    size_t need = 0;
    hipError_t e = rocprim::exclusive_scan(nullptr, need, flag, rank, 0u,
                                           (size_t)n, rocprim::plus<uint32_t>(),
                                           s);
    if (e != hipSuccess) return e;
    if (need > *temp_bytes) {
        if (*d_temp) (void)hipFree(*d_temp);
        e = hipMalloc(d_temp, need);
        if (e != hipSuccess) { *temp_bytes = 0; *d_temp = nullptr; return e; }
        *temp_bytes = need;
    }
    e = rocprim::exclusive_scan(*d_temp, *temp_bytes, flag, rank, 0u,
                                (size_t)n, rocprim::plus<uint32_t>(), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_group_heads, dim3(grid_for(n, 256)), dim3(256), 0, s,
                       flag, rank, series, ts, seq_key, perm, n, group_start,
                       head_series, head_ts, head_seq, n_out);
    return hipGetLastError();
}

hipError_t sort_keys_u64(hipStream_t s, const uint64_t* keys_in,
                         uint64_t* keys_out, size_t n, void** d_temp,
                         size_t* temp_bytes) {
    size_t need = 0;
    hipError_t e = rocprim::radix_sort_keys(nullptr, need, keys_in, keys_out,
                                            n, 0, 64, s);
    if (e != hipSuccess) return e;
    if (need > *temp_bytes) {
        if (*d_temp) (void)hipFree(*d_temp);
        e = hipMalloc(d_temp, need);
        if (e != hipSuccess) { *temp_bytes = 0; *d_temp = nullptr; return e; }
        *temp_bytes = need;
    }
    return rocprim::radix_sort_keys(*d_temp, *temp_bytes, keys_in, keys_out,
                                    n, 0, 64, s);
}

hipError_t sort_pairs_u64(hipStream_t s, const uint64_t* keys_in,
                          uint64_t* keys_out, const uint32_t* vals_in,
                          uint32_t* vals_out, size_t n, void** d_temp,
                          size_t* temp_bytes) {
    size_t need = 0;
    hipError_t e = rocprim::radix_sort_pairs(nullptr, need, keys_in, keys_out,
                                             vals_in, vals_out, n, 0, 64, s);
    if (e != hipSuccess) return e;
    if (need > *temp_bytes) {
        if (*d_temp) hipFree(*d_temp);
        e = hipMalloc(d_temp, need);
        if (e != hipSuccess) { *temp_bytes = 0; *d_temp = nullptr; return e; }
        *temp_bytes = need;
    }
    return rocprim::radix_sort_pairs(*d_temp, *temp_bytes, keys_in, keys_out,
                                     vals_in, vals_out, n, 0, 64, s);
}

}  // namespace hx
