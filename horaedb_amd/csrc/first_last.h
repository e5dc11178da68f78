// first_last.h — the compare rules of the first/last aggregates
// (include/horaedb_hx.h, HX_AGG_FIRST / HX_AGG_LAST), stated once. GPU-free:
// the host merge of per-device partials (engine.cpp, merge_partials) uses
// them, and first_last_check.cpp drives them on their own. Values travel as
// 64-bit patterns; nothing here compares or converts a double.
#pragma once
#include <cstdint>

namespace hx {

// f64 bit pattern -> u64 word whose unsigned order is IEEE 754 totalOrder
// (-NaN < -inf < ... < -0 < +0 < ... < +inf < +NaN, NaNs by payload): the
// host twin of the kernels' f64_ordered.
inline uint64_t fl_total_order_word(uint64_t bits) {
    return (bits >> 63) ? ~bits : (bits | 0x8000000000000000ull);
}

// One side of one group in one partial: the extreme timestamp and the bits
// of the value there.
struct FlPick {
    int64_t ts;
    uint64_t bits;
};

// last: the greater timestamp wins; at equal timestamps the value greater in
// totalOrder. Commutative and associative, so the order of partials is free.
inline FlPick fl_merge_last(FlPick a, FlPick b) {
    if (a.ts != b.ts) return a.ts > b.ts ? a : b;
    return fl_total_order_word(a.bits) >= fl_total_order_word(b.bits) ? a : b;
}

// first: the smaller timestamp wins; ties as for last (the greater value).
inline FlPick fl_merge_first(FlPick a, FlPick b) {
    if (a.ts != b.ts) return a.ts < b.ts ? a : b;
    return fl_total_order_word(a.bits) >= fl_total_order_word(b.bits) ? a : b;
}

}  // namespace hx
