# OPTIONAL (nullable) columns on the GPU path (DESIGN §2/§4 kernel 1c). The
# reference writes every column nullable, v1 pages, PLAIN, Snappy — so every
# page opens with a definition-level block, inside the compressed stream.
# A column without nulls must read exactly like a REQUIRED one under every
# codec, page version and encoding. Null f64 values on PLAIN pages are read:
# a null row is still a row for filter, dedup and rows_matched, and drops out
# of the aggregates; hx_scan returns it with a validity bit. Nulls anywhere
# else are rejected loudly with HX_ERR_UNSUPPORTED, and a refused compaction
# writes and unlinks nothing.
#
# Expectations are computed here with numpy from the pyarrow tables that were
# written: concatenate rows with their file sequence, apply the ts range and
# series set, keep the last row per PK by (seq, file row), drop null values,
# group. Keys, counts, min and max are exact; sums and avg rtol=1e-9.
import contextlib
import ctypes
import os

import numpy as np
import pytest

from horaedb_amd import (AGG_SUM, AGG_COUNT, AGG_MIN, AGG_MAX, AGG_AVG,
                         HxError)
from oracle.value_domain import group_max, group_min

pytestmark = pytest.mark.gpu

OPS_ALL = AGG_SUM | AGG_COUNT | AGG_MIN | AGG_MAX | AGG_AVG
FULL = (0, 2**62)
COLS = ["series_id", "timestamp", "value", "__seq__", "__reserved__"]
UNSUPPORTED = 3


def _zstd_loadable():
    try:
        ctypes.CDLL("libzstd.so.1")
        return True
    except OSError:
        return False


def _need(codec):
    if codec == "zstd" and not _zstd_loadable():
        pytest.skip("libzstd.so.1 not loadable")


@contextlib.contextmanager
def _env(**kv):
    assert not any(k in os.environ for k in kv)
    os.environ.update(kv)
    try:
        yield
    finally:
        for k in kv:
            del os.environ[k]


class Sst:
    """Rows of one written file, kept for the numpy expectation."""

    def __init__(self, seq, series, ts, value, valid):
        self.seq, self.series, self.ts = seq, series, ts
        self.value, self.valid = value, valid


def write_sst(store, seq, series, ts, value, *, nullable=True, value_null=None,
              null_col=None, row_group=8192, codec="snappy", version="1.0",
              ts_encoding="PLAIN", dict_series=False):
    """{store}/data/{seq}.sst from (series, ts)-sorted rows. nullable=True is
    the reference's shape: five nullable fields, __reserved__ all null.
    value_null: bool mask of null value rows. null_col: (name, row) puts one
    null into a key column."""
    import pyarrow as pa
    import pyarrow.parquet as pq
    series = np.ascontiguousarray(series, dtype=np.uint64)
    ts = np.ascontiguousarray(ts, dtype=np.int64)
    value = np.ascontiguousarray(value, dtype=np.float64)
    n = len(series)
    masks = {c: None for c in COLS}
    masks["value"] = value_null
    if null_col:
        m = np.zeros(n, dtype=bool)
        m[null_col[1]] = True
        masks[null_col[0]] = m
    types = [pa.uint64(), pa.int64(), pa.float64(), pa.uint64(), pa.uint64()]
    schema = pa.schema([pa.field(c, t, nullable=nullable)
                        for c, t in zip(COLS, types)])
    tbl = pa.table([
        pa.array(series, mask=masks["series_id"]),
        pa.array(ts, mask=masks["timestamp"]),
        pa.array(value, mask=masks["value"]),
        pa.array(np.full(n, seq, dtype=np.uint64)),
        pa.nulls(n, pa.uint64()) if nullable
        else pa.array(np.zeros(n, dtype=np.uint64))], schema=schema)
    enc = {c: "PLAIN" for c in COLS}
    enc["timestamp"] = ts_encoding
    kw = {"use_dictionary": False}
    if dict_series:
        kw = {"use_dictionary": ["series_id"],
              "dictionary_pagesize_limit": 1 << 30}
        del enc["series_id"]
    ddir = os.path.join(store, "data")
    os.makedirs(ddir, exist_ok=True)
    pq.write_table(tbl, os.path.join(ddir, f"{seq}.sst"),
                   row_group_size=row_group,
                   compression="NONE" if codec == "none" else codec.upper(),
                   data_page_version=version, column_encoding=enc,
                   write_statistics=True, **kw)
    valid = np.ones(n, dtype=bool) if value_null is None else ~value_null
    return Sst(seq, series, ts, value, valid)


def dedup_rows(ssts, ts_range=FULL, series_in=None):
    """Rows surviving filter + dedup (last row per PK by (seq, file row)),
    in (series, ts) order: series, ts, value, valid."""
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


def expected_agg(ssts, ts_range=FULL, series_in=None, bucket_ms=0):
    series, ts, value, valid = dedup_rows(ssts, ts_range, series_in)
    matched = len(series)
    series, ts, value = series[valid], ts[valid], value[valid]
    bucket = ts // bucket_ms if bucket_ms else np.zeros(len(ts), np.int64)
    first = np.ones(len(series), dtype=bool)
    first[1:] = (series[1:] != series[:-1]) | (bucket[1:] != bucket[:-1])
    starts = np.flatnonzero(first)
    exp = {"series_id": series[starts], "bucket": bucket[starts],
           "matched": matched}
    if len(starts):
        exp["count"] = np.diff(np.append(starts, len(series))).astype(np.uint64)
        exp["sum"] = np.add.reduceat(value, starts)
        exp["vmin"] = group_min(value, starts)   # totalOrder, bits kept
        exp["vmax"] = group_max(value, starts)
    else:
        exp["count"] = np.empty(0, np.uint64)
        exp["sum"] = exp["vmin"] = exp["vmax"] = np.empty(0)
    exp["avg"] = exp["sum"] / np.maximum(exp["count"], 1)
    return exp


def compare(res, exp, bucket_ms=0):
    keys = np.asarray(res["series_id"], dtype=np.uint64)
    if bucket_ms:
        order = np.lexsort((res["bucket"], keys))
        res = {k: v[order] for k, v in res.items()}
        assert res["bucket"].tolist() == exp["bucket"].tolist()
    assert res["series_id"].tolist() == exp["series_id"].tolist()
    assert res["count"].tolist() == exp["count"].tolist()
    np.testing.assert_array_equal(res["vmin"], exp["vmin"])
    np.testing.assert_array_equal(res["vmax"], exp["vmax"])
    np.testing.assert_allclose(res["sum"], exp["sum"], rtol=1e-9)
    np.testing.assert_allclose(res["avg"], exp["avg"], rtol=1e-9)


def same_result(a, b):
    """Two runs of one query: keys, counts, min and max identical; sums and
    avg within the suite's 1e-9 (float atomics land in a run-dependent
    order)."""
    assert sorted(a) == sorted(b)
    for k in a:
        if k in ("sum", "avg"):
            np.testing.assert_allclose(a[k], b[k], rtol=1e-9)
        else:
            np.testing.assert_array_equal(a[k], b[k])


def run_agg(store, ts_range=FULL, series_in=None, bucket_ms=0):
    from horaedb_amd import Store
    with Store(store) as st:
        with st.prepare(ts_range, series_in, devices=[0]) as p:
            res = p.exec_agg(ops=OPS_ALL, bucket_ms=bucket_ms)
            return res, p.stats(), p.decode_stats()


def run_scan(store, ts_range=FULL, series_in=None):
    from horaedb_amd import Store
    with Store(store) as st:
        return st.scan(ts_range, series_in=series_in, devices=[0])


# ---- reference-shaped files without nulls -----------------------------------

N_SERIES, N_PER = 2_000, 10        # 20 000 rows per SST


def _ref_rows(k, rng):
    """SST k of the reference-shaped store: SSTs 1 and 2 hold disjoint time
    windows, SST 3 rewrites half of SST 1's PKs (ts-overlap dedup), SST 4 is
    40 rows (a 6-byte level block)."""
    ids = np.sort(rng.integers(0, np.iinfo(np.uint64).max, N_SERIES,
                               dtype=np.uint64))
    if k == 4:
        series, ts = ids[:40], np.full(40, 5_000_000, dtype=np.int64)
    else:
        series = np.repeat(ids, N_PER)
        t0 = {1: 0, 2: N_PER, 3: N_PER // 2}[k]
        ts = np.tile(np.arange(t0, t0 + N_PER, dtype=np.int64) * 1000,
                     N_SERIES)
    return series, ts, rng.random(len(series))


def _build_ref(store, nullable, **kw):
    ssts = []
    for k in (1, 2, 3, 4):
        series, ts, value = _ref_rows(k, np.random.default_rng(100))
        value = value + k   # same ids in every file, other values per file
        ssts.append(write_sst(store, k, series, ts, value, nullable=nullable,
                              **kw))
    return ssts


REF_CASES = [("none", "1.0"), ("snappy", "1.0"), ("zstd", "1.0"),
             ("snappy", "2.0")]


@pytest.fixture(scope="module", params=REF_CASES,
                ids=[f"{c}-v{v[0]}" for c, v in REF_CASES])
def ref_pair(request, tmp_path_factory):
    codec, version = request.param
    _need(codec)
    opt = str(tmp_path_factory.mktemp("opt"))
    req = str(tmp_path_factory.mktemp("req"))
    ssts = _build_ref(opt, True, codec=codec, version=version)
    _build_ref(req, False, codec=codec, version=version)
    return opt, req, ssts, codec, version


QUERIES = [dict(), dict(ts_range=(3_000, 14_000)), dict(bucket_ms=4_000),
           dict(ts_range=(0, 20_000), bucket_ms=4_000),
           dict(series_in="some")]


@pytest.mark.parametrize("q", range(len(QUERIES)),
                         ids=["full", "ts_range", "bucket", "bucket_bounded",
                              "series_in"])
def test_reference_shaped_equals_required_twin(ref_pair, q):
    opt, req, ssts, codec, version = ref_pair
    kw = dict(QUERIES[q])
    if kw.get("series_in") == "some":
        kw["series_in"] = ssts[0].series[::N_PER * 7].tolist()
    res, stats, _ = run_agg(opt, **kw)
    twin, twin_stats, _ = run_agg(req, **kw)
    exp = expected_agg(ssts, **kw)
    compare(res, exp, kw.get("bucket_ms", 0))
    assert stats["rows_matched"] == exp["matched"]
    assert stats["rows_matched"] == twin_stats["rows_matched"]
    if kw.get("bucket_ms"):
        order = np.lexsort((twin["bucket"], twin["series_id"]))
        twin = {k: v[order] for k, v in twin.items()}
        order = np.lexsort((res["bucket"], res["series_id"]))
        res = {k: v[order] for k, v in res.items()}
    same_result(res, twin)


def test_reference_shaped_table_route(ref_pair):
    opt, _, ssts, _, _ = ref_pair
    with _env(HX_RANGE="0"):
        res, _, _ = run_agg(opt)
    compare(res, expected_agg(ssts))


def test_reference_shaped_scan_rows(ref_pair):
    opt, req, ssts, _, _ = ref_pair
    rows = run_scan(opt)
    twin = run_scan(req)
    series, ts, value, _ = dedup_rows(ssts)
    np.testing.assert_array_equal(rows["series_id"], series)
    np.testing.assert_array_equal(rows["timestamp"], ts)
    np.testing.assert_array_equal(rows["value"], value)
    assert "value_valid" not in rows
    for k in rows:
        np.testing.assert_array_equal(rows[k], twin[k])


def test_snappy_v1_value_pages_leave_the_in_place_path(tmp_path):
    # a 8192-row OPTIONAL f64 page is 8 level bytes + 64 KB: the Snappy
    # writer splits it into two literals, so it is not a stored page and goes
    # through the GPU decoder and the realigning kernel; its REQUIRED twin is
    # one stored literal and is read in place
    got = {}
    for nullable in (True, False):
        store = str(tmp_path / str(nullable))
        rng = np.random.default_rng(2)
        n = 8192
        write_sst(store, 1, np.sort(rng.integers(0, 1 << 63, n,
                                                 dtype=np.uint64)),
                  rng.integers(0, 1 << 62, n), rng.random(n),
                  nullable=nullable)
        got[nullable] = run_agg(store)[2]
    assert got[False]["pages_decoded"] == 0 and got[False]["pages_in_place"] > 0
    assert got[True]["pages_decoded"] > 0


def test_reexecute_identical(ref_pair):
    from horaedb_amd import Store
    opt, _, ssts, _, _ = ref_pair
    with _env(HX_REDECODE="1"):
        with Store(opt) as st, st.prepare(FULL, devices=[0]) as p:
            a = p.exec_agg(ops=OPS_ALL)
            b = p.exec_agg(ops=OPS_ALL)
    compare(a, expected_agg(ssts))
    same_result(a, b)


# ---- page sizes around the level block's length steps and the tile ----------

@pytest.mark.parametrize("codec", ["none", "snappy", "zstd"])
def test_row_group_sizes(tmp_path, codec):
    # row groups of 63, 64, 65 rows (6- and 7-byte blocks), 8192 followed by
    # one of 1 row, in one store; compressible values so that Snappy pages
    # hold copies and go through the decoder
    _need(codec)
    store = str(tmp_path)
    rng = np.random.default_rng(7)
    ssts = []
    for seq, (n, rg) in enumerate([(63 * 3, 63), (64 * 3, 64), (65 * 3, 65),
                                   (8193, 8192)], start=1):
        series = np.sort(rng.integers(0, 1 << 63, n, dtype=np.uint64))
        ts = rng.integers(0, 100_000, n)
        value = np.floor(rng.random(n) * 16) / 4 if seq % 2 else rng.random(n)
        ssts.append(write_sst(store, seq, series, ts, value, row_group=rg,
                              codec=codec))
    res, stats, _ = run_agg(store)
    exp = expected_agg(ssts)
    compare(res, exp)
    assert stats["rows_matched"] == exp["matched"]
    rows = run_scan(store)
    series, ts, value, _ = dedup_rows(ssts)
    np.testing.assert_array_equal(rows["series_id"], series)
    np.testing.assert_array_equal(rows["value"], value)


# ---- encodings ----------------------------------------------------------------

@pytest.mark.parametrize("enc", ["delta_ts", "dict_series"])
def test_encodings_optional_snappy(tmp_path, enc):
    # the Snappy-decoded DELTA / RLE_DICTIONARY stream starts behind the
    # level block; both decoders are byte-addressed
    kw = dict(ts_encoding="DELTA_BINARY_PACKED") if enc == "delta_ts" \
        else dict(dict_series=True)
    rng = np.random.default_rng(11)
    ids = np.sort(rng.integers(0, 1 << 63, 300, dtype=np.uint64))
    files = []
    for seq in (1, 2, 3):
        series = np.repeat(ids, 40)
        # file 3 rewrites the second half of file 1's points
        ts = np.tile(np.arange(40, dtype=np.int64) * 1000 +
                     {1: 0, 2: 40_000, 3: 20_000}[seq], 300)
        files.append((seq, series, ts, rng.random(len(series))))
    res = {}
    for nullable in (True, False):
        store = str(tmp_path / ("opt" if nullable else "req"))
        ssts = [write_sst(store, seq, series, ts, value, nullable=nullable,
                          codec="snappy", **kw)
                for seq, series, ts, value in files]
        res[nullable], _, _ = run_agg(store)
        compare(res[nullable], expected_agg(ssts))
    same_result(res[True], res[False])


# ---- rejections -------------------------------------------------------------

def _small_store(store, **kw):
    n = 500
    series = np.repeat(np.arange(1, 51, dtype=np.uint64) * 1000, 10)
    ts = np.tile(np.arange(10, dtype=np.int64) * 1000, 50)
    return [write_sst(store, seq, series, ts + seq, np.ones(n) * seq, **kw)
            for seq in (1, 2)]


@pytest.mark.parametrize("codec", ["none", "snappy", "zstd"])
@pytest.mark.parametrize("col", ["series_id", "timestamp"])
def test_null_in_key_column_rejected(tmp_path, col, codec):
    _need(codec)
    store = str(tmp_path)
    _small_store(store, codec=codec, null_col=(col, 250))
    with pytest.raises(HxError) as ei:
        run_agg(store)
    assert ei.value.code == UNSUPPORTED
    msg = str(ei.value)
    assert ".sst" in msg and col in msg


@pytest.mark.parametrize("how", ["compact", "compact_files"])
def test_compaction_over_null_values_refused(tmp_path, how):
    from horaedb_amd import Store
    store = str(tmp_path)
    mask = np.zeros(500, dtype=bool)
    mask[::7] = True
    _small_store(store, value_null=mask)
    ddir = os.path.join(store, "data")
    before = sorted(os.listdir(ddir))
    with Store(store) as st:
        cat = st.catalog()
        with pytest.raises(HxError) as ei:
            if how == "compact":
                st.compact(FULL, devices=[0])
            else:
                st.compact_files([1, 2], devices=[0])
        assert ei.value.code == UNSUPPORTED
        assert st.catalog() == cat
    assert sorted(os.listdir(ddir)) == before


def test_compaction_of_optional_inputs_without_nulls(tmp_path):
    from horaedb_amd import Store
    store = str(tmp_path)
    ssts = _small_store(store)
    before = run_scan(store)
    with Store(store) as st:
        new_seq = st.compact(FULL, devices=[0])
        assert new_seq > 2
        assert [e["seq"] for e in st.catalog()] == [new_seq]
    after = run_scan(store)
    for k in before:
        np.testing.assert_array_equal(before[k], after[k])
    res, _, _ = run_agg(store)
    compare(res, expected_agg(ssts))


# ---- null values ---------------------------------------------------------------

def _null_store(store, codec):
    """The reference-shaped rows with 30 % random null values; series 0 is
    null in every file (a group that must not be emitted) and series 1 is
    null throughout file 1 only."""
    rng = np.random.default_rng(5)
    ssts = []
    for k in (1, 2, 3, 4):
        series, ts, value = _ref_rows(k, np.random.default_rng(100))
        mask = rng.random(len(series)) < 0.3
        ids = np.unique(series)
        mask |= series == ids[0]
        if k == 1:
            mask |= series == ids[1]
        ssts.append(write_sst(store, k, series, ts, value + k,
                              value_null=mask, codec=codec))
    return ssts


@pytest.fixture(scope="module", params=["none", "snappy", "zstd"])
def null_store(request, tmp_path_factory):
    _need(request.param)
    store = str(tmp_path_factory.mktemp("nulls"))
    return store, _null_store(store, request.param)


NULL_ROUTES = {
    "default": (dict(), {}),
    "table": (dict(), {"HX_RANGE": "0"}),
    "bucket_direct": (dict(ts_range=(0, 20_000), bucket_ms=4_000), {}),
    "bucket_state": (dict(ts_range=(0, 20_000), bucket_ms=4_000),
                     {"HX_FORCE_STATE": "1"}),
    "bucket_unbounded": (dict(bucket_ms=4_000), {}),
    "series_in": (dict(series_in="some"), {}),
}


@pytest.mark.parametrize("route", list(NULL_ROUTES))
def test_null_values_all_ops(null_store, route):
    store, ssts = null_store
    kw, env = NULL_ROUTES[route]
    kw = dict(kw)
    if kw.get("series_in") == "some":
        # includes the all-null series 0 and the partly-null series 1
        kw["series_in"] = np.unique(ssts[0].series)[:40].tolist()
    with _env(**env):
        res, stats, _ = run_agg(store, **kw)
    exp = expected_agg(ssts, **kw)
    compare(res, exp, kw.get("bucket_ms", 0))
    assert stats["rows_matched"] == exp["matched"]
    assert np.unique(ssts[0].series)[0] not in res["series_id"]


def test_null_values_scan_rows(null_store):
    store, ssts = null_store
    rows = run_scan(store)
    series, ts, value, valid = dedup_rows(ssts)
    np.testing.assert_array_equal(rows["series_id"], series)
    np.testing.assert_array_equal(rows["timestamp"], ts)
    np.testing.assert_array_equal(rows["value_valid"], valid)
    np.testing.assert_array_equal(rows["value"][valid], value[valid])


def test_null_values_reexecute(null_store):
    from horaedb_amd import Store
    store, ssts = null_store
    with _env(HX_REDECODE="1"):
        with Store(store) as st, st.prepare(FULL, devices=[0]) as p:
            a = p.exec_agg(ops=OPS_ALL)
            b = p.exec_agg(ops=OPS_ALL)
    compare(a, expected_agg(ssts))
    same_result(a, b)


def _check_store(store, ssts):
    exp = expected_agg(ssts)
    for env in ({}, {"HX_RANGE": "0"}):
        with _env(**env):
            res, stats, _ = run_agg(store)
        compare(res, exp)
        assert stats["rows_matched"] == exp["matched"]
    rows = run_scan(store)
    series, ts, value, valid = dedup_rows(ssts)
    np.testing.assert_array_equal(rows["series_id"], series)
    np.testing.assert_array_equal(rows["timestamp"], ts)
    if valid.all():
        assert "value_valid" not in rows
    else:
        np.testing.assert_array_equal(rows["value_valid"], valid)
    np.testing.assert_array_equal(rows["value"][valid], value[valid])
    return exp


@pytest.mark.parametrize("codec", ["none", "snappy", "zstd"])
def test_null_shapes(tmp_path, codec):
    # row groups of 63/64/65 rows, 8192 + 1, a page whose first 5000 rows are
    # null (RLE runs), an alternating page (bit-packed), compressible values
    _need(codec)
    store = str(tmp_path)
    rng = np.random.default_rng(3)
    ssts = []
    shapes = [(63 * 3, 63, "rand"), (64 * 3, 64, "rand"), (65 * 3, 65, "rand"),
              (8193, 8192, "rand"), (8192, 8192, "head5000"),
              (8192, 8192, "alt"), (9000, 8192, "tail")]
    for seq, (n, rg, kind) in enumerate(shapes, start=1):
        series = np.sort(rng.integers(0, 1 << 63, n, dtype=np.uint64))
        ts = rng.integers(0, 100_000, n)
        value = np.floor(rng.random(n) * 16) / 4 if seq % 2 else rng.random(n)
        mask = {"rand": rng.random(n) < 0.3,
                "head5000": np.arange(n) < 5000,
                "alt": np.arange(n) % 2 == 1,
                "tail": np.arange(n) >= 8192}[kind]   # 2nd row group all null
        ssts.append(write_sst(store, seq, series, ts, value, row_group=rg,
                              value_null=mask, codec=codec))
    _check_store(store, ssts)


@pytest.mark.parametrize("codec", ["none", "snappy", "zstd"])
def test_only_row_is_null(tmp_path, codec):
    _need(codec)
    store = str(tmp_path)
    ssts = [write_sst(store, 1, [7], [1000], [1.5],
                      value_null=np.array([True]), codec=codec)]
    res, stats, _ = run_agg(store)
    assert len(res["series_id"]) == 0
    assert stats["rows_matched"] == 1
    rows = run_scan(store)
    assert rows["series_id"].tolist() == [7]
    assert rows["value_valid"].tolist() == [False]
    _check_store(store, ssts)


def test_all_null_series_beside_one_with_values(tmp_path):
    store = str(tmp_path)
    series = np.repeat(np.array([10, 20], dtype=np.uint64), 50)
    ts = np.tile(np.arange(50, dtype=np.int64) * 1000, 2)
    ssts = [write_sst(store, 1, series, ts, np.arange(100.0),
                      value_null=series == 10)]
    exp = _check_store(store, ssts)
    assert exp["series_id"].tolist() == [20] and exp["matched"] == 100


def test_dedup_null_across_ssts(tmp_path):
    # same PKs in two SSTs of one segment: a newer null shadows an older
    # value (the PK contributes nothing), an older null is shadowed by a
    # newer value (the value counts)
    store = str(tmp_path)
    n = 3000
    series = np.repeat(np.arange(1, 31, dtype=np.uint64) * 77, 100)
    ts = np.tile(np.arange(100, dtype=np.int64) * 1000, 30)
    rng = np.random.default_rng(9)
    old_null = rng.random(n) < 0.4
    new_null = rng.random(n) < 0.4
    ssts = [write_sst(store, 1, series, ts, rng.random(n), value_null=old_null),
            write_sst(store, 2, series, ts, rng.random(n) + 10,
                      value_null=new_null)]
    exp = _check_store(store, ssts)
    assert exp["matched"] == n
    assert int(exp["count"].sum()) == int((~new_null).sum())
    assert exp["vmin"].min() >= 10     # no older value leaks through


@pytest.mark.parametrize("row_group", [64, 8192])
def test_dedup_null_runs_on_pair_lane_and_row_group_edges(tmp_path, row_group):
    # equal-PK runs inside one SST, placed across the in-lane pair (rows
    # 2k/2k+1), the wave window (row 127/128) and the row-group edge; runs
    # alternate between "last row null" (the run contributes nothing) and
    # "last row the only non-null one"
    store = str(tmp_path)
    n = 3 * row_group + 40
    rng = np.random.default_rng(21)
    series = np.sort(rng.integers(0, 1 << 63, n, dtype=np.uint64))
    ts = np.full(n, 5000, dtype=np.int64)
    valid = np.ones(n, dtype=bool)
    e = row_group
    runs = [(0, 2), (3, 2), (6, 3), (9, 3), (20, 4), (125, 4), (126, 3),
            (e - 1, 2), (2 * e - 2, 3), (2 * e + 5, 2), (3 * e - 1, 2),
            (n - 2, 2)]
    used = np.zeros(n, dtype=bool)
    k = 0
    for start, length in runs:
        if used[start:start + length].any() or start + length > n:
            continue
        used[start:start + length] = True
        series[start:start + length] = series[start]
        if k % 2 == 0:
            valid[start + length - 1] = False          # last row null
        else:
            valid[start:start + length - 1] = False    # only the last valid
        k += 1
    assert k >= 8
    ssts = [write_sst(store, 1, series, ts, rng.random(n), row_group=row_group,
                      value_null=~valid)]
    exp = _check_store(store, ssts)
    assert exp["matched"] == len(np.unique(series))


def test_null_in_dictionary_value_page_rejected(tmp_path):
    import pyarrow as pa
    import pyarrow.parquet as pq
    store = str(tmp_path)
    ssts = _small_store(store)
    n = len(ssts[0].series)
    mask = np.arange(n) % 5 == 0
    types = [pa.uint64(), pa.int64(), pa.float64(), pa.uint64(), pa.uint64()]
    tbl = pa.table([pa.array(ssts[0].series), pa.array(ssts[0].ts),
                    pa.array(np.floor(np.arange(n) / 50.0), mask=mask),
                    pa.array(np.full(n, 1, dtype=np.uint64)),
                    pa.nulls(n, pa.uint64())],
                   schema=pa.schema([pa.field(c, t) for c, t in
                                     zip(COLS, types)]))
    pq.write_table(tbl, os.path.join(store, "data", "1.sst"),
                   use_dictionary=["value"], compression="NONE",
                   dictionary_pagesize_limit=1 << 30, data_page_version="1.0")
    with pytest.raises(HxError) as ei:
        run_agg(store)
    assert ei.value.code == UNSUPPORTED and "value" in str(ei.value)
