# first / last on the GPU path (HX_AGG_FIRST, HX_AGG_LAST; DESIGN §4 kernel
# 3d): the TS pass on every aggregate route, the resolve kernel, the host
# merge of two plans. The expectation (fl_expected) and the comparison
# (check_first_last) are those test_first_last_cpu.py checks without a GPU.
#
# Every comparison of first, last, first_ts and last_ts is exact: values as
# uint64 bit patterns, timestamps as integers. There is no tolerance.
import re

import numpy as np
import pytest

from horaedb_amd import AGG_COUNT, AGG_FIRST, AGG_LAST, AGG_SUM, HxError, Store
from oracle.value_domain import bits_of, from_bits
from test_first_last_cpu import check_first_last, fl_expected
from test_optional_gpu import FULL, OPS_ALL, UNSUPPORTED, _env, write_sst
from test_value_domain_cpu import (NZ, ONE, PZ, QNAN, STALE, check_agg,
                                   vd_expected)
from test_value_domain_gpu import ROUTES, build_store

pytestmark = pytest.mark.gpu

FL = AGG_FIRST | AGG_LAST
FL_KEYS = ("first", "first_ts", "last", "last_ts")
TWO = 0x4000000000000000
I64_MIN, I64_MAX = -2**63, 2**63 - 1


def run_fl(store, ops=OPS_ALL | FL, ts_range=FULL, series_in=None,
           bucket_ms=0, devices=(0,), segment_ms=0, execs=1):
    """(results of `execs` executions of one prepared plan, stats)."""
    with Store(store, segment_duration_ms=segment_ms) as st:
        with st.prepare(ts_range, series_in, devices=list(devices)) as p:
            res = [p.exec_agg(ops=ops, bucket_ms=bucket_ms)
                   for _ in range(execs)]
            return (res if execs > 1 else res[0]), p.stats()


def same_bits(a, b, keys=FL_KEYS):
    for k in keys:
        assert a[k].dtype == b[k].dtype
        assert a[k].view(np.uint64).tolist() == b[k].view(np.uint64).tolist(), k


# ---- every aggregate route ---------------------------------------------------

STORES = [("single", 64), ("two", 64), ("two", 8192), ("nullable", 64),
          ("nullable", 8192)]


@pytest.fixture(scope="module", params=STORES,
                ids=[f"{k}-rg{rg}" for k, rg in STORES])
def fl_store(request, tmp_path_factory):
    kind, row_group = request.param
    store = str(tmp_path_factory.mktemp(f"fl_{kind}_{row_group}"))
    return store, build_store(store, kind, row_group=row_group, codec="none")


def _route_kw(files, route):
    kw, env = ROUTES[route]
    kw = dict(kw)
    if kw.get("series_in") == "most":
        ids = np.unique(np.concatenate([f.series for f in files]))
        kw["series_in"] = np.concatenate([ids[::3], ids[1::3],
                                          ids[-4:]]).tolist()
    return kw, env


@pytest.mark.parametrize("route", list(ROUTES))
def test_route_first_last_exact_old_columns_unchanged(fl_store, route):
    store, files = fl_store
    kw, env = _route_kw(files, route)
    bucket_ms = kw.get("bucket_ms", 0)
    with _env(**env):
        res, stats = run_fl(store, **kw)
    assert list(res)[-4:] == list(FL_KEYS)
    n = check_first_last(res, fl_expected(files, **kw), bucket_ms)
    assert n > 1000
    exp = vd_expected(files, **kw)
    assert check_agg(res, exp, bucket_ms) > 1000
    assert stats["rows_matched"] == exp["matched"]


@pytest.mark.parametrize("route", ["default", "bucket_direct"])
def test_first_or_last_alone_and_without_value_ops(fl_store, route):
    store, files = fl_store
    kw, env = _route_kw(files, route)
    bucket_ms = kw.get("bucket_ms", 0)
    exp = fl_expected(files, **kw)
    with _env(**env):
        both, _ = run_fl(store, **kw)
        for ops, sides in ((AGG_LAST, ("last",)), (AGG_FIRST, ("first",)),
                           (FL, ("first", "last"))):
            res, stats = run_fl(store, ops=ops, **kw)
            want = ["series_id"] + (["bucket"] if bucket_ms else []) + \
                [k for k in FL_KEYS if k.split("_")[0] in sides]
            assert list(res) == want     # unrequested pointers are NULL
            check_first_last(res, exp, bucket_ms, sides)
            same_bits(res, both, [k for k in want if k != "bucket"])
            assert stats["rows_matched"] == vd_expected(files, **kw)["matched"]


# ---- a hand-built store: overlapping files, a second segment -------------------

SEG_MS = 100_000


def _rows(seq, series, ts, bits, null=None):
    series = np.asarray(series, dtype=np.uint64)
    ts = np.asarray(ts, dtype=np.int64)
    bits = np.asarray(bits, dtype=np.uint64)
    null = (np.zeros(len(series), dtype=bool) if null is None
            else np.asarray(null, dtype=bool))
    order = np.lexsort((ts, series))          # stable: equal PKs keep order
    return seq, series[order], ts[order], from_bits(bits[order]), null[order]


def _write(store, rows, **kw):
    seq, series, ts, value, null = rows
    kw.setdefault("row_group", 64)
    kw.setdefault("codec", "none")
    return write_sst(store, seq, series, ts, value, nullable=True,
                     value_null=null, **kw)


@pytest.fixture(scope="module")
def hand_store(tmp_path_factory):
    """Series k * 7919 (k = 1..40), 20 points each at 0, 1000, ..., 19000 in
    file 1; series 40 only at 50000 ... 69000. Row 63 of file 1 is written
    three times (an equal-PK run over the row-group edge at 64: the third
    copy wins). File 2 rewrites the latest point of series 1 (new value), of
    series 2 (null: last falls back to 18000) and of series 3 (stale
    marker). File 3 rewrites the first point of series 4 (new value) and of
    series 5 (null: first moves on to 1000), and nulls every point of series
    6 (no group). File 4 lies in the second segment and extends series 1, 2
    and 7; its newest point of series 7 is null."""
    store = str(tmp_path_factory.mktemp("fl_hand"))
    sid = lambda k: k * 7919
    s1, t1, b1 = [], [], []
    for k in range(1, 41):
        base = 50_000 if k == 40 else 0
        for j in range(20):
            s1.append(sid(k))
            t1.append(base + j * 1000)
            b1.append(int(bits_of(np.array([k + j / 32.0]))[0]))
    # sorted row 63 = series 4, ts 3000: two older copies in front of it
    s1 = s1[:63] + [s1[63]] * 2 + s1[63:]
    t1 = t1[:63] + [t1[63]] * 2 + t1[63:]
    b1 = b1[:63] + [QNAN, NZ] + b1[63:]
    # rows 63 | 64, 65: the run straddles the edge of row group 64
    assert (s1[63], t1[63]) == (s1[65], t1[65]) == (sid(4), 3000)
    assert (s1[62], t1[62]) != (s1[63], t1[63]) != (s1[66], t1[66])
    n6 = 20
    files = [
        _write(store, _rows(1, s1, t1, b1)),
        _write(store, _rows(2, [sid(1), sid(2), sid(3), sid(9)],
                            [19_000, 19_000, 19_000, 5_000],
                            [TWO, ONE, STALE, NZ],
                            [False, True, False, False])),
        _write(store, _rows(3, [sid(4), sid(5)] + [sid(6)] * n6,
                            [0, 0] + [j * 1000 for j in range(n6)],
                            [TWO, ONE] + [ONE] * n6,
                            [False, True] + [True] * n6)),
        _write(store, _rows(4, [sid(1)] * 2 + [sid(2)] + [sid(7)] * 2,
                            [SEG_MS + 500, SEG_MS + 900, SEG_MS + 100,
                             SEG_MS + 200, SEG_MS + 300],
                            [ONE, NZ, STALE, PZ, ONE],
                            [False, False, False, False, True])),
    ]
    return store, files, sid


HAND_QUERIES = {
    "full": dict(),
    "end_cuts_series": dict(ts_range=(0, 9_500)),
    "excludes_series_40": dict(ts_range=(0, 30_000)),
    "second_segment_only": dict(ts_range=(SEG_MS, 2 * SEG_MS)),
    "series_in": dict(series_in=[7919 * k for k in (1, 2, 4, 6, 7, 40, 99)]),
    "bucket": dict(bucket_ms=4_000),
}


def test_hand_store_shape(hand_store):
    _, files, sid = hand_store
    exp = fl_expected(files)
    at = {int(s): i for i, s in enumerate(exp["series_id"])}
    last = lambda k: (int(exp["last_ts"][at[sid(k)]]),
                      int(exp["last_bits"][at[sid(k)]]))
    first = lambda k: (int(exp["first_ts"][at[sid(k)]]),
                       int(exp["first_bits"][at[sid(k)]]))
    assert last(1) == (SEG_MS + 900, NZ)
    assert last(2) == (SEG_MS + 100, STALE)
    assert last(3) == (19_000, STALE)
    assert last(7) == (SEG_MS + 200, PZ)
    assert first(4) == (0, TWO) and first(5)[0] == 1000
    assert sid(6) not in at and sid(40) in at
    cut = fl_expected(files, ts_range=(0, 9_500))
    assert set(cut["last_ts"].tolist()) == {9_000} and sid(40) not in set(
        cut["series_id"].tolist())
    # without file 4, file 2 decides: new value, fallback, stale marker
    seg0 = fl_expected(files, ts_range=(0, SEG_MS))
    at0 = {int(s): i for i, s in enumerate(seg0["series_id"])}
    assert int(seg0["last_bits"][at0[sid(1)]]) == TWO
    assert int(seg0["last_ts"][at0[sid(2)]]) == 18_000
    # the equal-PK run: the third copy is the survivor
    v = vd_expected(files, ts_range=(3000, 3001), series_in=[sid(4)])
    assert v["count"].tolist() == [1] and v["matched"] == 1
    assert int(v["vmax_bits"][0]) not in (QNAN, NZ)


@pytest.mark.parametrize("route", ["default", "table", "state"])
@pytest.mark.parametrize("query", list(HAND_QUERIES))
def test_hand_store(hand_store, query, route):
    store, files, _ = hand_store
    kw = HAND_QUERIES[query]
    bucket_ms = kw.get("bucket_ms", 0)
    with _env(**ROUTES[route][1]):
        res, stats = run_fl(store, segment_ms=SEG_MS, **kw)
    exp = fl_expected(files, **kw)
    assert check_first_last(res, exp, bucket_ms) == len(exp["series_id"]) > 0
    vd = vd_expected(files, **kw)
    check_agg(res, vd, bucket_ms)
    assert stats["rows_matched"] == vd["matched"]


# ---- timestamps: negative with buckets, the ends of int64 ----------------------

def test_negative_timestamps_with_buckets(tmp_path):
    store = str(tmp_path)
    rng = np.random.default_rng(21)
    n = 6_000
    series = rng.integers(0, 150, n).astype(np.uint64) * np.uint64(104_729)
    ts = rng.integers(-100_000, 100_000, n).astype(np.int64)
    bits = bits_of(rng.standard_normal(n)).copy()
    bits[::11] = STALE
    bits[5::13] = NZ
    null = rng.random(n) < 0.2
    files = [_write(store, _rows(1, series, ts, bits, null))]
    for kw, env in ((dict(ts_range=(-200_000, 200_000), bucket_ms=7_000), {}),
                    (dict(ts_range=(-200_000, 200_000), bucket_ms=7_000),
                     {"HX_FORCE_STATE": "1"}),
                    (dict(ts_range=(-50_000, 50_000)), {}),
                    (dict(ts_range=(-50_001, -3), bucket_ms=1_000), {})):
        with _env(**env):
            res, stats = run_fl(store, **kw)
        exp = fl_expected(files, **kw)
        assert (exp["bucket"] < 0).any() or not kw.get("bucket_ms")
        assert check_first_last(res, exp, kw.get("bucket_ms", 0)) > 100
        assert stats["rows_matched"] == vd_expected(files, **kw)["matched"]


@pytest.mark.parametrize("route", ["default", "table", "state"])
def test_int64_extremes_under_the_widest_range(tmp_path, route):
    # [start, end) is half-open, so the widest range the API takes ends at
    # INT64_MAX and a row at INT64_MAX itself can never match
    store = str(tmp_path)
    series = [3, 3, 3, 5, 5, 8]
    ts = [I64_MIN + 1, 0, I64_MAX - 1, -7, 7, I64_MIN + 1]
    bits = [STALE, ONE, NZ, ONE, TWO, PZ]
    files = [_write(store, _rows(1, series, ts, bits))]
    kw = dict(ts_range=(I64_MIN, I64_MAX))
    with _env(**ROUTES[route][1]):
        res, stats = run_fl(store, **kw)
    exp = fl_expected(files, **kw)
    assert exp["first_ts"].tolist() == [I64_MIN + 1, -7, I64_MIN + 1]
    assert exp["last_ts"].tolist() == [I64_MAX - 1, 7, I64_MIN + 1]
    assert exp["first_bits"].tolist()[0] == STALE
    assert exp["last_bits"].tolist()[0] == NZ
    check_first_last(res, exp)
    assert stats["rows_matched"] == 6


# ---- decoded timestamps, expanded OPTIONAL value pages, re-execution ------------

@pytest.fixture(scope="module")
def delta_store(tmp_path_factory):
    store = str(tmp_path_factory.mktemp("fl_delta"))
    rng = np.random.default_rng(5)
    files = []
    for seq in (1, 2):
        n = 5_000
        series = rng.integers(0, 300, n).astype(np.uint64) * np.uint64(65_537)
        ts = rng.integers(0, 400, n).astype(np.int64) * 250
        bits = bits_of(rng.standard_normal(n)).copy()
        bits[seq::9] = STALE
        bits[3::17] = NZ
        files.append(_write(store, _rows(seq, series, ts, bits,
                                         rng.random(n) < 0.3),
                            row_group=1024, codec="snappy",
                            ts_encoding="DELTA_BINARY_PACKED"))
    return store, files


@pytest.mark.parametrize("kw", [dict(), dict(ts_range=(10_000, 70_001)),
                                dict(bucket_ms=9_000)],
                         ids=["full", "range", "bucket"])
def test_delta_timestamps_snappy_optional_values(delta_store, kw):
    store, files = delta_store
    with Store(store) as st, st.prepare(kw.get("ts_range", FULL),
                                        devices=[0]) as p:
        d = p.decode_stats()
        assert d["pages_decoded"] > 0
        res = p.exec_agg(ops=OPS_ALL | FL, bucket_ms=kw.get("bucket_ms", 0))
        stats = p.stats()
    assert check_first_last(res, fl_expected(files, **kw),
                            kw.get("bucket_ms", 0)) >= 300
    vd = vd_expected(files, **kw)
    check_agg(res, vd, kw.get("bucket_ms", 0))
    assert stats["rows_matched"] == vd["matched"]


@pytest.mark.parametrize("redecode", [False, True], ids=["cached", "redecode"])
@pytest.mark.parametrize("kw", [dict(), dict(bucket_ms=9_000)],
                         ids=["series", "bucket"])
def test_reexecuted_plan_returns_identical_bits(delta_store, kw, redecode):
    store, files = delta_store
    with _env(**({"HX_REDECODE": "1"} if redecode else {})):
        runs, _ = run_fl(store, execs=3, **kw)
    bucket_ms = kw.get("bucket_ms", 0)
    exp = fl_expected(files, **kw)
    for r in runs:
        check_first_last(r, exp, bucket_ms)
    if bucket_ms:
        runs = [{k: v[np.lexsort((r["bucket"], r["series_id"]))]
                 for k, v in r.items()} for r in runs]
    same_bits(runs[0], runs[1])
    same_bits(runs[0], runs[2])


# ---- overflow and retry ----------------------------------------------------------

@pytest.fixture(scope="module")
def wide_store(tmp_path_factory):
    # 40 000 series of two rows, one file: with the partition pinned at 512
    # blocks that is ~78 keys per block
    store = str(tmp_path_factory.mktemp("fl_wide"))
    rng = np.random.default_rng(9)
    k = 40_000
    series = np.repeat(np.unique(rng.integers(1, 2**62, k + 64,
                                              dtype=np.uint64))[:k], 2)
    ts = np.tile(np.array([1_000, 2_000]), k)
    bits = bits_of(rng.standard_normal(2 * k)).copy()
    bits[::7] = STALE
    null = rng.random(2 * k) < 0.25
    files = [_write(store, _rows(1, series, ts, bits, null), row_group=8192)]
    return store, files, fl_expected(files), vd_expected(files)


def test_block_overflow_retry(wide_store, capfd):
    store, files, exp, vd = wide_store
    with _env(HX_RANGE_TARGET="1000000000", HX_RANGE_NE="64", HX_DEBUG="1"):
        res, stats = run_fl(store)
    err = capfd.readouterr().err
    # both passes overflow their blocks and re-partition
    assert len(re.findall(r"attempt=0 kernel=range-sorted .*nb=512 "
                          r".*block_overflow=[1-9]", err)) >= 1, err
    assert "first/last resolve groups=%d " % len(exp["series_id"]) in err, err
    check_first_last(res, exp)
    check_agg(res, vd)
    assert stats["rows_matched"] == vd["matched"]


def test_table_growth_retry(delta_store, capfd):
    # 300 series against 64 slots: the table grows twice (x4 per retry, a
    # retry once the fill passes 85 %), in the value pass and, on a plan
    # whose table was reset by the stride change, in the TS pass
    store, files = delta_store
    with _env(HX_RANGE="0", HX_TABLE_SLOTS="64", HX_DEBUG="1"):
        res, stats = run_fl(store)
    err = capfd.readouterr().err
    assert re.search(r"attempt=0 kernel=wave slots=64 .*overflow=[1-9]",
                     err), err
    assert re.search(r"kernel=wave slots=1024 .*overflow=0 ", err), err
    assert "kernel=range-sorted" not in err
    exp, vd = fl_expected(files), vd_expected(files)
    assert check_first_last(res, exp) == 300
    check_agg(res, vd)
    assert stats["rows_matched"] == vd["matched"]


# ---- two plans on one card: the host merge ----------------------------------------

def test_two_plans_merge_equals_single_device(tmp_path):
    # two files whose time ranges do not touch form two overlap clusters,
    # which a device set spreads over its plans: every series below has rows
    # in both, so its group reaches the host merge from both partials
    store = str(tmp_path)
    rng = np.random.default_rng(13)
    n_series, per = 300, 6
    sid = np.arange(1, n_series + 1, dtype=np.uint64) * np.uint64(2**33 + 9)
    files = []
    for seq, t0 in ((1, -30_000), (2, 40_000)):
        series = np.repeat(sid, per)
        ts = np.tile(np.arange(per, dtype=np.int64) * 1_000 + t0, n_series)
        bits = bits_of(rng.standard_normal(len(series))).copy()
        bits[seq::5] = STALE
        bits[2::7] = NZ
        bits[3::7] = PZ
        null = rng.random(len(series)) < 0.35
        null[:per * 3] = seq == 2        # three series: nothing but nulls late
        keep = np.ones(len(series), dtype=bool)
        keep[per * 10:per * 20] = seq == 1   # ten series in the early file only
        files.append(_write(store, _rows(seq, series[keep], ts[keep],
                                         bits[keep], null[keep])))
    for kw in (dict(ts_range=(-10**6, 10**6)),
               dict(ts_range=(-10**6, 10**6), bucket_ms=50_000)):
        one, st1 = run_fl(store, **kw)
        two, st2 = run_fl(store, devices=(0, 0), **kw)
        bucket_ms = kw.get("bucket_ms", 0)
        exp = fl_expected(files, **kw)
        check_first_last(one, exp, bucket_ms)
        check_first_last(two, exp, bucket_ms)
        # a group's first comes from one partial, its last from the other
        if not bucket_ms:
            assert ((exp["first_ts"] < 0) & (exp["last_ts"] > 0)).sum() > 200
            assert ((exp["last_ts"] < 0)).sum() >= 10
        assert st1["rows_matched"] == st2["rows_matched"] == \
            vd_expected(files, **kw)["matched"]
        assert two["count"].tolist() == one["count"].tolist()


# ---- refusals -------------------------------------------------------------------

def test_binary_value_store_refuses_last(tmp_path):
    store = str(tmp_path)
    import os
    os.makedirs(os.path.join(store, "data"))
    with Store(store) as st:
        st.write_bytes(np.array([1, 2], dtype=np.uint64),
                       np.array([10, 20], dtype=np.int64), [b"a", b"bc"],
                       enable_check=False)
        for ops in (AGG_LAST, AGG_FIRST, AGG_SUM | AGG_COUNT | AGG_LAST):
            with pytest.raises(HxError) as ei:
                st.scan_agg(FULL, ops=ops, devices=[0])
            assert ei.value.code == UNSUPPORTED
