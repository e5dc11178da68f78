# The f64 value domain (value rules in include/horaedb_hx.h):
# the reference helpers of oracle/value_domain.py, the dataset builder of
# tools/gen_ssts.py (vd_*), and the native Parquet writer's DOUBLE
# statistics. No GPU needed. tests/test_value_domain_gpu.py takes its
# expectation (vd_expected) and its comparison (check_agg) from here.
#
# The comparison, per group:
#   keys, counts      exact
#   vmin / vmax       equal as uint64 bit patterns (IEEE 754 totalOrder; NaN
#                     payload, signalling bit and sign of zero included)
#   sum               by kind (nan / +inf / -inf / finite); a finite sum
#                     within n * 2**-53 * sum|x| of math.fsum — the bound for
#                     ANY order of the n-1 additions (Higham, Accuracy and
#                     Stability of Numerical Algorithms, §4.2), so it needs
#                     no measurement; the sign of a zero sum is free
#   avg               same kind; finite within that bound / n plus one ulp
#                     of the quotient (the division's own rounding, here and
#                     in the code under test)
import math
import struct

import numpy as np
import pytest

from oracle.value_domain import (bits_of, from_bits, group_max_bits,
                                 group_min_bits, group_sum_expect,
                                 key_to_bits, sum_bound, total_order_key)
from tools.gen_ssts import (VD_BITS, VD_BUCKET_MS, VD_NAN, VD_RANGE,
                            VD_SPECIAL, vd_base_rows, vd_class_of,
                            vd_coverage, vd_overwrite_rows)

FULL = (0, 2**62)
MIN_NORMAL = 2.2250738585072014e-308   # 2**-1022


class Rows:
    """Rows of one file for the expectation: seq, series, ts, value (f64
    carrying the bit patterns), valid."""

    def __init__(self, seq, d):
        self.seq = seq
        self.series, self.ts = d["series"], d["ts"]
        self.value = from_bits(d["bits"])
        null = d.get("null")
        self.valid = (np.ones(len(self.series), dtype=bool) if null is None
                      else ~null)


def dedup_rows(ssts, ts_range=FULL, series_in=None):
    """Rows surviving filter + dedup (last row per PK by (seq, file row)),
    in (series, ts) order: series, ts, value, valid. Values are only ever
    moved, never computed on, so their bits survive."""
    series = np.concatenate([s.series for s in ssts])
    ts = np.concatenate([s.ts for s in ssts])
    value = np.concatenate([s.value for s in ssts])
    valid = np.concatenate([s.valid for s in ssts])
    seq = np.concatenate([np.full(len(s.series), s.seq, dtype=np.uint64)
                          for s in ssts])
    row = np.concatenate([np.arange(len(s.series)) for s in ssts])
    keep = (ts >= ts_range[0]) & (ts < ts_range[1])
    if series_in is not None:
        keep &= np.isin(series, np.asarray(series_in, dtype=np.uint64))
    series, ts, value, valid, seq, row = (a[keep] for a in
                                          (series, ts, value, valid, seq, row))
    order = np.lexsort((row, seq, ts, series))
    series, ts, value, valid = (a[order] for a in (series, ts, value, valid))
    last = np.ones(len(series), dtype=bool)
    last[:-1] = (series[1:] != series[:-1]) | (ts[1:] != ts[:-1])
    return series[last], ts[last], value[last], valid[last]


def vd_expected(ssts, ts_range=FULL, series_in=None, bucket_ms=0):
    series, ts, value, valid = dedup_rows(ssts, ts_range, series_in)
    matched = len(series)
    series, ts, value = series[valid], ts[valid], value[valid]
    bucket = ts // bucket_ms if bucket_ms else np.zeros(len(ts), np.int64)
    first = np.ones(len(series), dtype=bool)
    first[1:] = (series[1:] != series[:-1]) | (bucket[1:] != bucket[:-1])
    starts = np.flatnonzero(first)
    ends = np.append(starts[1:], len(series))
    return {"series_id": series[starts], "bucket": bucket[starts],
            "matched": matched, "count": (ends - starts).astype(np.uint64),
            "vmin_bits": group_min_bits(value, starts) if len(starts)
            else np.empty(0, np.uint64),
            "vmax_bits": group_max_bits(value, starts) if len(starts)
            else np.empty(0, np.uint64),
            "groups": [value[s:e] for s, e in zip(starts, ends)],
            "sums": [group_sum_expect(value[s:e])
                     for s, e in zip(starts, ends)]}


def needs_subnormals(n, kind, abs_sum):
    """A finite group whose any-order bound n * 2**-53 * sum|x| is below half
    the f64 grid spacing 2**-1074 (n * sum|x| < 2**-1022): only arithmetic
    that keeps subnormals gets it right, and then exactly."""
    return kind == "finite" and 0 < n * abs_sum < MIN_NORMAL


def check_sum(got, n, expect, what):
    kind, exact, abs_sum = expect
    if kind == "nan":
        assert math.isnan(got), f"{what}: {got!r}, expected NaN"
    elif kind != "finite":
        assert got == exact, f"{what}: {got!r}, expected {exact!r}"
    else:
        assert math.isfinite(got), f"{what}: {got!r}, expected finite"
        assert abs(got - exact) <= sum_bound(n, abs_sum), \
            f"{what}: {got!r} vs {exact!r} (n={n}, sum|x|={abs_sum!r})"


def check_avg(got, n, expect, what):
    kind, exact, abs_sum = expect
    if kind == "nan":
        assert math.isnan(got), f"{what}: {got!r}, expected NaN"
    elif kind != "finite":
        assert got == exact, f"{what}: {got!r}, expected {exact!r}"
    else:
        q = exact / n
        tol = sum_bound(n, abs_sum) / n + math.ulp(q)
        assert math.isfinite(got) and abs(got - q) <= tol, \
            f"{what}: {got!r} vs {q!r} (n={n}, tol={tol!r})"


def check_agg(res, exp, bucket_ms=0, sums="ordinary"):
    """sums='ordinary': every group but those that need_subnormals;
    'subnormal': those only (and nothing else of the result)."""
    keys = np.asarray(res["series_id"], dtype=np.uint64)
    if bucket_ms:
        order = np.lexsort((res["bucket"], keys))
        res = {k: v[order] for k, v in res.items()}
    if sums == "ordinary":
        if bucket_ms:
            assert res["bucket"].tolist() == exp["bucket"].tolist()
        assert res["series_id"].tolist() == exp["series_id"].tolist()
        assert res["count"].tolist() == exp["count"].tolist()
        for name in ("vmin", "vmax"):
            got = bits_of(res[name])
            want = exp[name + "_bits"]
            bad = np.flatnonzero(got != want)
            assert len(bad) == 0, (
                f"{name}: {len(bad)} groups differ in bits, first "
                f"series {int(exp['series_id'][bad[0]])}: got "
                f"{int(got[bad[0]]):#018x}, expected "
                f"{int(want[bad[0]]):#018x}, group "
                f"{[hex(int(b)) for b in bits_of(exp['groups'][bad[0]])]}")
    n_checked = 0
    for i, e in enumerate(exp["sums"]):
        n = int(exp["count"][i])
        if needs_subnormals(n, e[0], e[2]) != (sums == "subnormal"):
            continue
        what = f"series {int(exp['series_id'][i])} bucket " \
               f"{int(exp['bucket'][i])}"
        check_sum(float(res["sum"][i]), n, e, "sum of " + what)
        check_avg(float(res["avg"][i]), n, e, "avg of " + what)
        n_checked += 1
    return n_checked


# ---- the key map ---------------------------------------------------------------

def _py_total_order(bits):
    """IEEE 754-2019 §5.10 totalOrder as a sort key. The bit pattern becomes
    a Python float through struct, and the float's sign, exponent and
    fraction fields are read back from its big-endian bytes: negative before
    positive; within a sign by (exponent, fraction), descending for
    negatives — NaNs have the largest exponent field, so they sort
    outermost, by payload."""
    (x,) = struct.unpack("<d", struct.pack("<Q", bits))
    be = struct.pack(">d", x)
    hi, lo = struct.unpack(">HQ", be[:2] + b"\0\0" + be[2:])   # 16 + 48 bits
    sign, exponent = hi >> 15, (hi >> 4) & 0x7FF
    fraction = ((hi & 0xF) << 48) | lo
    return (0, -exponent, -fraction) if sign else (1, exponent, fraction)


EXTRA_BITS = [0x7FF0000000000001, 0xFFF0000000000002, 0xFFFFFFFFFFFFFFFF,
              0x4000000000000000, 0xC000000000000000, 0x000FFFFFFFFFFFFF,
              0x800FFFFFFFFFFFFF, 0x3FEFFFFFFFFFFFFF]


def test_total_order_key_matches_struct_sort():
    bits = [int(b) for b in VD_BITS] + EXTRA_BITS
    keys = total_order_key(from_bits(np.array(bits, dtype=np.uint64)))
    by_key = [b for _, b in sorted(zip(keys.tolist(), bits))]
    by_py = sorted(bits, key=_py_total_order)
    assert by_key == by_py
    assert len(set(keys.tolist())) == len(bits)         # injective
    assert key_to_bits(keys).tolist() == bits           # and invertible
    # the landmarks of the order, spelled out
    name = {b: n for n, b in VD_SPECIAL}
    landmarks = [name[b] for b in by_py if b in name]
    assert landmarks == ["-qnan", "-inf", "-dbl_max", "-1", "-min_normal",
                         "-denorm_min", "-0", "+0", "+denorm_min",
                         "+min_normal", "+1", "+dbl_max", "+inf", "stale",
                         "+qnan", "+nan_max"]
    # the accumulator identities lose to every double but the two extreme
    # NaNs, which they equal (min: 0x7FFF... = +nan_max; max: 0xFFFF...)
    assert int(keys.max()) == 0xFFFFFFFFFFFFFFFF
    assert int(keys.min()) == 0


def _b(*xs):
    return np.array(xs, dtype=np.uint64)


QNAN, NQNAN, STALE = 0x7FF8000000000000, 0xFFF8000000000000, 0x7FF0000000000002
PZ, NZ = 0, 0x8000000000000000
ONE = 0x3FF0000000000000
PINF, NINF = 0x7FF0000000000000, 0xFFF0000000000000


@pytest.mark.parametrize("group,lo,hi", [
    ([QNAN, ONE], ONE, QNAN),
    ([ONE, QNAN], ONE, QNAN),
    ([NQNAN, ONE], NQNAN, ONE),
    ([STALE, ONE, QNAN], ONE, QNAN),          # stale < qNaN by payload
    ([STALE, ONE], ONE, STALE),
    ([STALE, STALE], STALE, STALE),           # the signalling bit survives
    ([PZ, NZ], NZ, PZ),
    ([NZ, PZ, NZ], NZ, PZ),
    ([PINF, QNAN], PINF, QNAN),               # +inf does not beat +NaN
    ([NINF, NQNAN], NQNAN, NINF),
    ([QNAN], QNAN, QNAN),
    ([NQNAN], NQNAN, NQNAN),
    ([1, 0x8000000000000001, PZ], 0x8000000000000001, 1),
])
def test_group_min_max_bits(group, lo, hi):
    v = from_bits(_b(*group))
    assert int(group_min_bits(v, [0])[0]) == lo
    assert int(group_max_bits(v, [0])[0]) == hi


def test_group_min_max_several_groups():
    v = from_bits(_b(QNAN, ONE, NZ, PZ, STALE))
    starts = np.array([0, 2, 4])
    assert group_min_bits(v, starts).tolist() == [ONE, NZ, STALE]
    assert group_max_bits(v, starts).tolist() == [QNAN, PZ, STALE]


def test_oracle_scan_agg_uses_total_order():
    import oracle
    from oracle.scan import AGG_MIN, AGG_MAX
    sst = oracle.SstBatch([np.array([1, 1, 2, 2], dtype=np.uint64),
                           np.array([10, 20, 10, 20], dtype=np.int64),
                           from_bits(_b(STALE, ONE, PZ, NZ))], 1)
    res = oracle.scan_agg([sst], (0, 100), ops=AGG_MIN | AGG_MAX)
    assert bits_of(res["vmin"]).tolist() == [ONE, NZ]
    assert bits_of(res["vmax"]).tolist() == [STALE, PZ]


@pytest.mark.parametrize("values,kind", [
    ([1.0, math.nan, 2.0], "nan"),
    ([math.inf, -math.inf], "nan"),
    ([math.inf, 1.0, math.nan], "nan"),
    ([math.inf, 1e308, -1e308], "+inf"),
    ([-math.inf, 5.0], "-inf"),
    ([1e308, 1e308, 1e308], "+inf"),
    ([-1e308, -1e308, -1e308], "-inf"),
    ([1e16, 1.0, -1e16, 3.0], "finite"),
    ([0.0, -0.0], "finite"),
    ([5e-324] * 5, "finite"),
])
def test_group_sum_expect_kinds(values, kind):
    k, exact, abs_sum = group_sum_expect(np.array(values))
    assert k == kind
    if kind == "finite":
        assert exact == math.fsum(values)
        assert abs_sum == math.fsum(abs(x) for x in values)
    elif kind == "nan":
        assert math.isnan(exact)
    else:
        assert exact == float(kind)


def test_group_sum_expect_cancellation_and_subnormals():
    assert group_sum_expect(np.array([1e16, 1.0, -1e16, 3.0]))[1] == 4.0
    k, exact, abs_sum = group_sum_expect(np.array([5e-324] * 5))
    assert exact == 25e-324 and needs_subnormals(5, k, abs_sum)
    k, exact, abs_sum = group_sum_expect(np.array([1.0, 5e-324]))
    assert not needs_subnormals(2, k, abs_sum)
    # the NaN stale marker is a NaN for sums
    stale = from_bits(_b(STALE, ONE))
    assert group_sum_expect(stale)[0] == "nan"


# ---- the dataset builder -------------------------------------------------------

@pytest.fixture(scope="module")
def base():
    return vd_base_rows()


@pytest.fixture(scope="module")
def variants(base):
    """name -> list of Rows (the files of one store)."""
    o, n = vd_overwrite_rows(base)
    on, nn = vd_overwrite_rows(base, nullable=True)
    return {"single": [Rows(1, base)],
            "two": [Rows(1, o), Rows(2, n)],
            "nullable": [Rows(1, on), Rows(2, nn)]}


def _sorted_by_pk(d):
    s, t = d["series"].astype(object), d["ts"]
    return all((s[i], t[i]) < (s[i + 1], t[i + 1]) for i in range(len(s) - 1))


def test_builder_rows_sorted_unique_and_sized(base):
    assert _sorted_by_pk(base)
    for nullable in (False, True):
        for d in vd_overwrite_rows(base, nullable=nullable):
            assert _sorted_by_pk(d)
    n = len(base["series"])
    assert 8192 < n < 12_000          # past one default row group, still small
    runs = np.diff(np.flatnonzero(np.append(
        np.append(True, base["series"][1:] != base["series"][:-1]), True)))
    assert set(runs.tolist()) == {1, 2, 3, 4, 5}


@pytest.mark.parametrize("row_group", [64, 8192])
def test_builder_covers_every_class_role_and_position(base, row_group):
    missing, straddles = vd_coverage(base["series"], base["bits"], row_group)
    assert missing == []
    assert straddles >= 1
    # vd_coverage itself: a file without the stale marker misses it 3*128x
    cut = base["bits"].copy()
    cut[cut == STALE] = ONE
    m2, _ = vd_coverage(base["series"], cut, row_group)
    assert len(m2) == 3 * 128 and {m[0] for m in m2} == {"stale"}


def test_builder_group_kinds_present(variants):
    exp = vd_expected(variants["single"])
    kinds = [e[0] for e in exp["sums"]]
    assert {"nan", "+inf", "-inf", "finite"} <= set(kinds)
    groups = exp["groups"]
    assert any(bits_of(g).tolist() == bits_of([1e16, 1.0, -1e16, 3.0]).tolist()
               for g in groups)
    assert any(len(g) == 3 and (g == 1e308).all() for g in groups)
    sub = [i for i, e in enumerate(exp["sums"])
           if needs_subnormals(len(groups[i]), e[0], e[2])]
    assert len(sub) >= 6
    # all-subnormal groups with a subnormal exact sum exist
    assert any(0 < abs(exp["sums"][i][1]) < 2.2250738585072014e-308 and
               (np.abs(groups[i]) < 2.2250738585072014e-308).all()
               for i in sub)
    # mixed-sign ordinary groups
    assert any(e[0] == "finite" and (g > 0).any() and (g < 0).any()
               for g, e in zip(groups, exp["sums"]))
    # no group's kind depends on the order of additions: at most one
    # |x| = DBL_MAX among finite-or-overflowing groups of mixed sign
    for name in ("single", "two", "nullable"):
        for g in vd_expected(variants[name])["groups"]:
            big = np.abs(g) == np.finfo(np.float64).max
            assert big.sum() <= 1


def _sole_value(rows, sid, ts_range):
    series, ts, value, valid = dedup_rows(rows, ts_range, [sid])
    return len(series), bits_of(value[valid]).tolist()


def test_builder_identity_traps(base, variants):
    # ts-range traps: 5 rows of one series in a row, only the NaN in range
    trap = np.flatnonzero(base["kind"] == 3)
    assert len(trap) == 10
    sids = np.unique(base["series"][trap])
    assert len(sids) == 2
    for sid, nan in zip(sids, (QNAN, NQNAN)):
        rows = np.flatnonzero(base["series"] == sid)
        assert (np.diff(rows) == 1).all() and len(rows) == 5
        assert int(base["bits"][rows[2]]) == nan
        for name in ("single", "two", "nullable"):
            assert _sole_value(variants[name], sid, VD_RANGE) == (1, [nan])
            assert _sole_value(variants[name], sid, FULL)[0] == 5
    # superseded-row traps: the NaN of the older file between four rows the
    # newer file rewrites — with nulls in the nullable store, so the NaN is
    # the only surviving value there
    top = int(base["series"].max())
    for name in ("two", "nullable"):
        old, new = variants[name]
        tsid = np.unique(old.series[old.series > top])
        assert len(tsid) == 2
        for sid, nan in zip(tsid, (QNAN, NQNAN)):
            o = np.flatnonzero(old.series == sid)
            assert len(o) == 5 and int(bits_of(old.value)[o[2]]) == nan
            assert (new.series == sid).sum() == 4
            n_rows, vals = _sole_value(variants[name], sid, VD_RANGE)
            assert n_rows == 5 and nan in vals
            if name == "nullable":
                assert vals == [nan]
            else:
                assert len(vals) == 5


def test_builder_overwrites_both_ways(base, variants):
    old, new = variants["two"]
    key_old = {(int(s), int(t)): int(b) for s, t, b in
               zip(old.series, old.ts, bits_of(old.value))}
    to_finite = to_special = 0
    for s, t, b in zip(new.series, new.ts, bits_of(new.value)):
        ob = key_old[(int(s), int(t))]          # every new PK rewrites one
        was = vd_class_of([ob])[0] >= 0
        now = vd_class_of([int(b)])[0] >= 0
        to_finite += was and not now
        to_special += now and not was
    assert to_finite > 1000 and to_special > 1000


def test_builder_nullable_shape(variants):
    old, new = variants["nullable"]
    for f in (old, new):
        assert 0.25 < (~f.valid).mean() < 0.40
        cls = vd_class_of(bits_of(f.value))
        nan = np.flatnonzero(np.isin(cls, list(VD_NAN)) & f.valid)
        nxt = np.clip(nan + 1, 0, len(cls) - 1)
        prv = np.clip(nan - 1, 0, len(cls) - 1)
        assert (~f.valid[nxt]).sum() > 50 and (~f.valid[prv]).sum() > 50
    exp = vd_expected(variants["nullable"])
    series, _, _, valid = dedup_rows(variants["nullable"])
    all_null = set(series.tolist()) - set(exp["series_id"].tolist())
    assert len(all_null) >= 1


QUERIES = [dict(), dict(ts_range=VD_RANGE),
           dict(ts_range=VD_RANGE, bucket_ms=VD_BUCKET_MS),
           dict(bucket_ms=VD_BUCKET_MS)]


@pytest.mark.parametrize("name", ["single", "two", "nullable"])
def test_sequential_numpy_sum_is_inside_the_bound(variants, name):
    # the bound the GPU test applies is not tighter than a plain left-to-
    # right f64 sum: every finite group of every dataset and query passes
    n_finite = n_sub = 0
    for q in QUERIES:
        exp = vd_expected(variants[name], **q)
        for g, e in zip(exp["groups"], exp["sums"]):
            if e[0] != "finite":
                continue
            with np.errstate(over="ignore", invalid="ignore"):
                seq = float(np.add.reduceat(g, [0])[0])
            check_sum(seq, len(g), e, f"{name} {q}")
            check_avg(seq / len(g), len(g), e, f"{name} {q}")
            n_finite += 1
            if needs_subnormals(len(g), e[0], e[2]):
                assert seq == e[1]
                n_sub += 1
    assert n_finite > 1000 and n_sub >= 6


# ---- the native writer's DOUBLE statistics -----------------------------------

def _native(tmp_path, bits, row_group, name="1.sst"):
    from horaedb_amd.store import write_sst_native
    n = len(bits)
    ddir = tmp_path / "data"
    ddir.mkdir(exist_ok=True)
    path = str(ddir / name)
    write_sst_native(path, np.arange(n, dtype=np.uint64),
                     np.arange(n, dtype=np.int64) * 10,
                     from_bits(np.asarray(bits, dtype=np.uint64)), 1,
                     row_group=row_group)
    return path


def _stat_bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def test_native_writer_statistics_skip_nan_and_sign_zero(tmp_path):
    import pyarrow.parquet as pq
    rg = 16
    TWO = 0x4000000000000000
    chunks = [                  # (leading values, value filling the chunk)
        ([QNAN, ONE, TWO, STALE], ONE),       # NaN first: skipped
        ([QNAN, STALE, NQNAN], QNAN),         # nothing but NaN
        ([PZ, PZ], ONE),                      # min zero -> -0.0
        ([NZ, NZ], 0xBFF0000000000000),       # max zero -> +0.0
        ([NZ], NZ),                           # both bounds zero
        ([PZ], PZ),
        ([PINF, NINF, QNAN], ONE),
        ([int(b) for b in VD_BITS], ONE),
    ]
    bits = []
    for lead, fill in chunks:
        bits += lead + [fill] * (rg - len(lead))
    path = _native(tmp_path, bits, rg)
    f = pq.ParquetFile(path)
    got = f.read().column("value").to_numpy()
    assert bits_of(got).tolist() == bits                # values bit-exact
    vi = f.schema_arrow.names.index("value")
    for g in range(f.metadata.num_row_groups):
        st = f.metadata.row_group(g).column(vi).statistics
        vals = from_bits(np.array(bits[g * rg:(g + 1) * rg], dtype=np.uint64))
        real = vals[~np.isnan(vals)]
        if len(real) == 0:
            assert st is None or not st.has_min_max
            continue
        assert st is not None and st.has_min_max
        assert not math.isnan(st.min) and not math.isnan(st.max)
        assert st.min <= real.min() and st.max >= real.max()
        assert st.min == real.min() and st.max == real.max()   # and tight
        if st.min == 0.0:
            assert _stat_bits(st.min) == NZ
        if st.max == 0.0:
            assert _stat_bits(st.max) == PZ
    # key columns keep their statistics
    st = f.metadata.row_group(1).column(0).statistics
    assert st.has_min_max and st.min == rg and st.max == 2 * rg - 1


@pytest.mark.parametrize("writer", ["native", "pyarrow"])
def test_open_accepts_value_chunk_without_statistics(tmp_path, writer):
    # an all-NaN value chunk carries no min/max (pyarrow omits them too);
    # hx_open and the footer reader take the file as any other
    import pyarrow.parquet as pq
    from horaedb_amd import Store
    from tools.gen_ssts import gen_sst_from_arrays
    n, rg = 40, 16
    bits = [QNAN] * 16 + [ONE] * 16 + [STALE] * 8
    if writer == "native":
        path = _native(tmp_path, bits, rg)
    else:
        path = gen_sst_from_arrays(
            str(tmp_path), 1, np.arange(n), np.arange(n) * 10,
            from_bits(np.array(bits, dtype=np.uint64)), row_group=rg)
    f = pq.ParquetFile(path)
    vi = f.schema_arrow.names.index("value")
    for g in (0, 2):
        st = f.metadata.row_group(g).column(vi).statistics
        assert st is None or not st.has_min_max
    with Store(str(tmp_path)) as st:
        cat = st.catalog()
    assert len(cat) == 1 and cat[0]["n_rows"] == n
    assert cat[0]["n_row_groups"] == 3
    assert (cat[0]["ts_min"], cat[0]["ts_max"]) == (0, (n - 1) * 10)
