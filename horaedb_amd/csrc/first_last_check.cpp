// first_last_check.cpp — stand-alone host check of first_last.h, the compare
// rules the host merge applies to the first/last columns of per-device
// partials. Built by `make first_last_check` with
// -fsanitize=address,undefined when the runtime is available. The expected
// winners are worked out here by an independent statement of IEEE 754
// totalOrder (sign, then magnitude, on the bit pattern). Prints one line per
// case, "all ok" at the end, exits non-zero on a mismatch.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "first_last.h"

namespace {

int g_fail = 0;

void report(const char* name, bool ok) {
    printf("%-46s %s\n", name, ok ? "ok" : "FAIL");
    if (!ok) g_fail++;
}

// totalOrder a < b, stated on sign and magnitude (not on the mapped word)
bool total_lt(uint64_t a, uint64_t b) {
    const bool na = a >> 63, nb = b >> 63;
    const uint64_t ma = a & 0x7FFFFFFFFFFFFFFFull;
    const uint64_t mb = b & 0x7FFFFFFFFFFFFFFFull;
    if (na != nb) return na;          // negative below positive, -0 < +0
    return na ? ma > mb : ma < mb;    // negatives: larger magnitude is lower
}

bool same(hx::FlPick a, hx::FlPick b) {
    return a.ts == b.ts && a.bits == b.bits;
}

// fold the partials in the order given, as merge_partials does
hx::FlPick fold(const std::vector<hx::FlPick>& v, bool last) {
    hx::FlPick acc = v[0];
    for (size_t i = 1; i < v.size(); i++)
        acc = last ? hx::fl_merge_last(acc, v[i])
                   : hx::fl_merge_first(acc, v[i]);
    return acc;
}

// the rule restated: extreme ts, then the totalOrder-greatest value
hx::FlPick expect(const std::vector<hx::FlPick>& v, bool last) {
    hx::FlPick best = v[0];
    for (size_t i = 1; i < v.size(); i++) {
        const hx::FlPick x = v[i];
        const bool better_ts = last ? x.ts > best.ts : x.ts < best.ts;
        if (better_ts || (x.ts == best.ts && total_lt(best.bits, x.bits)))
            best = x;
    }
    return best;
}

const uint64_t kVals[] = {
    0x0000000000000000ull,   // +0
    0x8000000000000000ull,   // -0
    0x0000000000000001ull,   // smallest subnormal
    0x8000000000000001ull,   // its negative
    0x3FF0000000000000ull,   // 1.0
    0xBFF0000000000000ull,   // -1.0
    0x7FF0000000000000ull,   // +inf
    0xFFF0000000000000ull,   // -inf
    0x7FF0000000000001ull,   // signalling NaN, payload 1
    0x7FF0000000000002ull,   // the Prometheus stale marker
    0x7FF8000000000000ull,   // quiet NaN
    0x7FFFFFFFFFFFFFFFull,   // +NaN, full payload
    0xFFF0000000000002ull,   // -NaN, signalling
    0xFFF8000000000000ull,   // -NaN, quiet
    0xFFFFFFFFFFFFFFFFull,   // -NaN, full payload
};
const int64_t kTs[] = {INT64_MIN, INT64_MIN + 1, -1000, -1, 0, 1, 1000,
                       INT64_MAX - 1, INT64_MAX};

}  // namespace

int main() {
    const size_t nv = sizeof(kVals) / sizeof(kVals[0]);
    const size_t nt = sizeof(kTs) / sizeof(kTs[0]);

    // the order word is monotone in totalOrder and loses no bit
    {
        bool ok = true;
        for (size_t i = 0; i < nv; i++)
            for (size_t j = 0; j < nv; j++) {
                const bool lt = total_lt(kVals[i], kVals[j]);
                const bool wlt = hx::fl_total_order_word(kVals[i]) <
                                 hx::fl_total_order_word(kVals[j]);
                ok = ok && lt == wlt;
                ok = ok && ((hx::fl_total_order_word(kVals[i]) ==
                             hx::fl_total_order_word(kVals[j])) == (i == j));
            }
        report("order word monotone and injective", ok);
    }

    // single partial: passes through bit for bit
    {
        bool ok = true;
        for (size_t i = 0; i < nv; i++)
            for (size_t t = 0; t < nt; t++) {
                const std::vector<hx::FlPick> one{{kTs[t], kVals[i]}};
                ok = ok && same(fold(one, true), one[0]) &&
                     same(fold(one, false), one[0]);
            }
        report("single partial passes through", ok);
    }

    // every pair, both orders: distinct and equal timestamps, every value
    {
        bool ok_last = true, ok_first = true, ok_comm = true;
        for (size_t ta = 0; ta < nt; ta++)
            for (size_t tb = 0; tb < nt; tb++)
                for (size_t i = 0; i < nv; i++)
                    for (size_t j = 0; j < nv; j++) {
                        const hx::FlPick a{kTs[ta], kVals[i]};
                        const hx::FlPick b{kTs[tb], kVals[j]};
                        const std::vector<hx::FlPick> ab{a, b}, ba{b, a};
                        ok_last = ok_last &&
                                  same(fold(ab, true), expect(ab, true));
                        ok_first = ok_first &&
                                   same(fold(ab, false), expect(ab, false));
                        ok_comm = ok_comm &&
                                  same(fold(ab, true), fold(ba, true)) &&
                                  same(fold(ab, false), fold(ba, false));
                    }
        report("last: pairs over all ts and values", ok_last);
        report("first: pairs over all ts and values", ok_first);
        report("pairs: order of the partials is free", ok_comm);
    }

    // the named cases, spelled out
    {
        const hx::FlPick stale{5, 0x7FF0000000000002ull};
        const hx::FlPick one{4, 0x3FF0000000000000ull};
        report("last: a later stale marker beats a value",
               same(hx::fl_merge_last(one, stale), stale) &&
                   same(hx::fl_merge_last(stale, one), stale));
        report("first: the earlier value beats the marker",
               same(hx::fl_merge_first(one, stale), one) &&
                   same(hx::fl_merge_first(stale, one), one));
        const hx::FlPick pz{7, 0}, nz{7, 0x8000000000000000ull};
        report("tie: +0 beats -0 on both sides",
               same(hx::fl_merge_last(pz, nz), pz) &&
                   same(hx::fl_merge_last(nz, pz), pz) &&
                   same(hx::fl_merge_first(pz, nz), pz) &&
                   same(hx::fl_merge_first(nz, pz), pz));
        const hx::FlPick n1{7, 0x7FF0000000000001ull};
        const hx::FlPick n2{7, 0x7FF0000000000002ull};
        const hx::FlPick inf{7, 0x7FF0000000000000ull};
        report("tie: NaNs order by payload, above +inf",
               same(hx::fl_merge_last(n1, n2), n2) &&
                   same(hx::fl_merge_first(n2, n1), n2) &&
                   same(hx::fl_merge_last(inf, n1), n1));
        const hx::FlPick nn{7, 0xFFF8000000000000ull};
        const hx::FlPick ninf{7, 0xFFF0000000000000ull};
        report("tie: -NaN sits below -inf",
               same(hx::fl_merge_last(nn, ninf), ninf) &&
                   same(hx::fl_merge_first(ninf, nn), ninf));
        const hx::FlPick lo{INT64_MIN, 1}, hi{INT64_MAX, 2};
        report("INT64_MIN / INT64_MAX do not wrap",
               same(hx::fl_merge_last(lo, hi), hi) &&
                   same(hx::fl_merge_first(lo, hi), lo) &&
                   same(hx::fl_merge_last(hi, lo), hi) &&
                   same(hx::fl_merge_first(hi, lo), lo));
    }

    // triples in all six orders: the fold is associative
    {
        bool ok = true;
        const hx::FlPick t3[][3] = {
            {{1, kVals[4]}, {1, kVals[9]}, {1, kVals[1]}},
            {{1, kVals[4]}, {2, kVals[14]}, {2, kVals[7]}},
            {{INT64_MIN, kVals[0]}, {0, kVals[1]}, {INT64_MAX, kVals[12]}},
            {{-5, kVals[11]}, {-5, kVals[10]}, {-6, kVals[6]}},
        };
        const int perm[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2},
                                {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
        for (const auto& tr : t3)
            for (const auto& pm : perm) {
                const std::vector<hx::FlPick> v{tr[pm[0]], tr[pm[1]],
                                                tr[pm[2]]};
                const std::vector<hx::FlPick> base{tr[0], tr[1], tr[2]};
                ok = ok && same(fold(v, true), expect(base, true)) &&
                     same(fold(v, false), expect(base, false));
            }
        report("triples: every order of three partials", ok);
    }

    if (g_fail) {
        printf("%d FAILED\n", g_fail);
        return 1;
    }
    printf("all ok\n");
    return 0;
}
