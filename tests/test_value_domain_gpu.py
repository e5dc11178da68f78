# The f64 value domain on the GPU path (value rules in
# include/horaedb_hx.h): NaN of either sign (quiet, signalling, the
# Prometheus stale marker), signed zeros, infinities, subnormals, DBL_MAX,
# cancelling and overflowing groups — through every aggregate route, the row
# stream, every codec, compaction and the ingest sort.
#
# min/max follow IEEE 754 totalOrder and return the chosen value's bits;
# sums are compared by kind and, when finite, against math.fsum within the
# any-order bound n * 2**-53 * sum|x|. The dataset (tools/gen_ssts.py vd_*),
# the expectation and the comparison are those test_value_domain_cpu.py
# checks without a GPU; see its header for the tolerances.
import os

import numpy as np
import pytest

from oracle.value_domain import bits_of, from_bits
from test_optional_gpu import (FULL, OPS_ALL, _env, _need, run_agg, run_scan,
                               write_sst)
from test_value_domain_cpu import (NQNAN, NZ, ONE, PZ, QNAN, STALE, Rows,
                                   check_agg, dedup_rows, vd_expected)
from tools.gen_ssts import (VD_BITS, VD_BUCKET_MS, VD_RANGE, vd_base_rows,
                            vd_overwrite_rows)

pytestmark = pytest.mark.gpu


def write_rows(store, rows, nullable, **kw):
    """One file of a store from a Rows; REQUIRED columns unless nullable."""
    write_sst(store, rows.seq, rows.series, rows.ts, rows.value,
              nullable=nullable,
              value_null=~rows.valid if nullable else None, **kw)


def build_store(store, kind, **kw):
    """kind: 'single' (REQUIRED, the one file whose coverage of every class,
    role and row position test_value_domain_cpu.py asserts — every row of it
    is live), 'two' (REQUIRED, two files, the newer rewriting half the
    special rows with finite values and half the ordinary rows with
    specials) or 'nullable' (the same with ~30 % null values)."""
    nullable = kind == "nullable"
    if kind == "single":
        files = [Rows(1, vd_base_rows())]
    else:
        files = [Rows(q, d) for q, d in zip(
            (1, 2), vd_overwrite_rows(vd_base_rows(), nullable=nullable))]
    for f in files:
        write_rows(store, f, nullable, **kw)
    return files


# ---- every aggregate route ---------------------------------------------------
# All routes but the unbounded ones query VD_RANGE, so the ts-range identity
# traps have their filler rows filtered out next to the surviving NaN.

ROUTES = {
    "default": (dict(ts_range=VD_RANGE), {}),
    "table": (dict(ts_range=VD_RANGE), {"HX_RANGE": "0"}),
    "state": (dict(ts_range=VD_RANGE), {"HX_FORCE_STATE": "1"}),
    "bucket_direct": (dict(ts_range=VD_RANGE, bucket_ms=VD_BUCKET_MS), {}),
    "bucket_state": (dict(ts_range=VD_RANGE, bucket_ms=VD_BUCKET_MS),
                     {"HX_FORCE_STATE": "1"}),
    "bucket_unbounded": (dict(bucket_ms=VD_BUCKET_MS), {}),
    "series_in": (dict(ts_range=VD_RANGE, series_in="most"), {}),
    "unbounded": (dict(), {}),
}
STORES = [("single", 64), ("single", 8192), ("two", 64), ("two", 8192),
          ("nullable", 64), ("nullable", 8192)]


@pytest.fixture(scope="module", params=STORES,
                ids=[f"{k}-rg{rg}" for k, rg in STORES])
def vd_store(request, tmp_path_factory):
    kind, row_group = request.param
    store = str(tmp_path_factory.mktemp(f"vd_{kind}_{row_group}"))
    return store, build_store(store, kind, row_group=row_group,
                              codec="none"), {}


def _route(vd_store, route):
    """(result, stats, expectation, bucket_ms) of one route on one store,
    computed once for the tests that look at different parts of it."""
    store, files, cache = vd_store
    if route not in cache:
        kw, env = ROUTES[route]
        kw = dict(kw)
        if kw.get("series_in") == "most":
            # two of every three series, the traps (last ids) included
            ids = np.unique(np.concatenate([f.series for f in files]))
            kw["series_in"] = np.concatenate([ids[::3], ids[1::3],
                                              ids[-4:]]).tolist()
        with _env(**env):
            res, stats, _ = run_agg(store, **kw)
        cache[route] = (res, stats, vd_expected(files, **kw),
                        kw.get("bucket_ms", 0))
    return cache[route]


@pytest.mark.parametrize("route", list(ROUTES))
def test_route_keys_counts_minmax_bits_and_sums(vd_store, route):
    res, stats, exp, bucket_ms = _route(vd_store, route)
    n = check_agg(res, exp, bucket_ms)
    assert n > 1000
    assert stats["rows_matched"] == exp["matched"]


@pytest.mark.parametrize("route", list(ROUTES))
def test_route_subnormal_sums_exact(vd_store, route):
    # groups whose every partial sum is subnormal: exact, or the atomic
    # unit of that route flushes
    res, _, exp, bucket_ms = _route(vd_store, route)
    assert res["series_id"].shape == exp["series_id"].shape
    n = check_agg(res, exp, bucket_ms, sums="subnormal")
    assert n >= 4


def test_sentinel_series_state_word_path(tmp_path):
    # series id 2**64-1 is the key-claim sentinel: the store really takes
    # the state-word table, not the forced one
    store = str(tmp_path)
    files = [Rows(1, vd_base_rows(sentinel_series=True))]
    write_rows(store, files[0], False, row_group=64, codec="none")
    for kw in (dict(), dict(bucket_ms=VD_BUCKET_MS)):
        res, stats, _ = run_agg(store, **kw)
        exp = vd_expected(files, **kw)
        assert int(exp["series_id"][-1]) == 2**64 - 1
        check_agg(res, exp, kw.get("bucket_ms", 0))
        check_agg(res, exp, kw.get("bucket_ms", 0), sums="subnormal")
        assert stats["rows_matched"] == exp["matched"]


# ---- the defects, each on the smallest store that shows it -------------------

def _tiny(store, seq, series, ts, bits, **kw):
    d = {"series": np.array(series, dtype=np.uint64),
         "ts": np.array(ts, dtype=np.int64),
         "bits": np.array(bits, dtype=np.uint64)}
    rows = Rows(seq, d)
    write_rows(store, rows, False, codec="none", **kw)
    return rows


def _check_routes(store, files, routes=("default", "table", "state"), **kw):
    for route in routes:
        with _env(**ROUTES[route][1]):
            res, stats, _ = run_agg(store, **kw)
        exp = vd_expected(files, **kw)
        check_agg(res, exp)
        assert stats["rows_matched"] == exp["matched"]


@pytest.mark.parametrize("shift", [0, 1])
def test_nan_on_either_pair_slot(tmp_path, shift):
    # series [NaN, 1.0] and [1.0, NaN] starting on an even and on an odd
    # row: min/max must not depend on where the rows sit
    store = str(tmp_path)
    series = [1] * shift + [5, 5, 6, 6, 7, 7, 8, 8, 9]
    ts = [10] * shift + [10, 20] * 4 + [10]
    bits = [ONE] * shift + [QNAN, ONE, ONE, QNAN, NQNAN, ONE, ONE, NQNAN, ONE]
    files = [_tiny(store, 1, series, ts, bits)]
    _check_routes(store, files)


@pytest.mark.parametrize("shift", [0, 1])
def test_stale_marker_payload_survives(tmp_path, shift):
    # the stale marker is a signalling NaN: max of [stale, 1.0] and of
    # [stale, stale] is the marker itself, not a quieted copy and not 1.0
    store = str(tmp_path)
    series = [1] * shift + [5, 5, 6, 6, 7, 7, 7]
    ts = [10] * shift + [10, 20, 10, 20, 10, 20, 30]
    bits = [ONE] * shift + [STALE, ONE, STALE, STALE, ONE, STALE, PZ]
    files = [_tiny(store, 1, series, ts, bits)]
    exp = vd_expected(files)
    assert exp["vmax_bits"].tolist()[-3:] == [STALE] * 3
    _check_routes(store, files)


@pytest.mark.parametrize("shift", [0, 1])
def test_signed_zero_min_max(tmp_path, shift):
    store = str(tmp_path)
    series = [1] * shift + [5, 5, 6, 6, 7, 7, 7]
    ts = [10] * shift + [10, 20, 10, 20, 10, 20, 30]
    bits = [ONE] * shift + [PZ, NZ, NZ, PZ, NZ, PZ, NZ]
    files = [_tiny(store, 1, series, ts, bits)]
    exp = vd_expected(files)
    assert exp["vmin_bits"].tolist()[-3:] == [NZ] * 3
    assert exp["vmax_bits"].tolist()[-3:] == [PZ] * 3
    _check_routes(store, files)


@pytest.mark.parametrize("nan", [QNAN, NQNAN], ids=["+nan", "-nan"])
def test_sole_nan_between_rows_outside_ts_range(tmp_path, nan):
    # one surviving value, NaN, among filtered-out rows of its own series in
    # the same wave: a dead lane's identity must lose to it (+inf would beat
    # +NaN in a min, -inf would beat -NaN in a max)
    store = str(tmp_path)
    series = [4, 4] + [5] * 7 + [6]
    ts = [100, 110] + [10, 20, 30, 100, 200, 210, 220] + [100]
    bits = [ONE] * 5 + [nan] + [ONE] * 4
    files = [_tiny(store, 1, series, ts, bits)]
    exp = vd_expected(files, ts_range=(50, 150))
    assert exp["count"].tolist() == [2, 1, 1]
    assert exp["vmin_bits"].tolist()[1] == exp["vmax_bits"].tolist()[1] == nan
    _check_routes(store, files, ts_range=(50, 150))


@pytest.mark.parametrize("nan", [QNAN, NQNAN], ids=["+nan", "-nan"])
def test_sole_nan_between_rows_superseded_by_newer_file(tmp_path, nan):
    # as above with the neighbours filtered by cross-file dedup. In a store
    # without nulls the rewriting rows themselves survive, so the group has
    # five values; the older file's wave still holds the NaN as its only
    # live row of the series, and -inf from its dead lanes would replace
    # +NaN in the max (+inf would replace -NaN in the min)
    store = str(tmp_path)
    ts5 = [10, 20, 30, 40, 50]
    old = _tiny(store, 1, [4] + [5] * 5 + [6], [10] + ts5 + [10],
                [ONE] * 3 + [nan] + [ONE] * 3)
    two = 0x4000000000000000
    new = _tiny(store, 2, [5] * 4, [10, 20, 40, 50], [two] * 4)
    exp = vd_expected([old, new])
    assert exp["count"].tolist() == [1, 5, 1]
    assert nan in (exp["vmin_bits"][1], exp["vmax_bits"][1])
    _check_routes(store, [old, new])


# ---- row stream, codecs, compaction, ingest ------------------------------------

def _assert_rows(rows, files, ts_range=FULL):
    series, ts, value, valid = dedup_rows(files, ts_range)
    assert rows["series_id"].tolist() == series.tolist()
    assert rows["timestamp"].tolist() == ts.tolist()
    if valid.all():
        assert "value_valid" not in rows
    else:
        assert rows["value_valid"].tolist() == valid.tolist()
    got, want = bits_of(rows["value"])[valid], bits_of(value)[valid]
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, (
        f"{len(bad)} values differ in bits, first {int(got[bad[0]]):#018x} "
        f"for {int(want[bad[0]]):#018x}")


@pytest.mark.parametrize("ts_range", [FULL, VD_RANGE], ids=["full", "range"])
def test_scan_rows_bit_for_bit(vd_store, ts_range):
    store, files, _ = vd_store
    _assert_rows(run_scan(store, ts_range=ts_range), files, ts_range)


CODECS = [("snappy", "1.0"), ("zstd", "1.0"), ("none", "2.0"),
          ("snappy", "2.0"), ("zstd", "2.0")]


@pytest.mark.parametrize("kind", ["two", "nullable"])
@pytest.mark.parametrize("codec,version", CODECS,
                         ids=[f"{c}-v{v[0]}" for c, v in CODECS])
def test_codecs_and_page_versions_keep_bits(tmp_path, codec, version, kind):
    _need(codec)
    store = str(tmp_path)
    files = build_store(store, kind, row_group=8192, codec=codec,
                        version=version)
    _assert_rows(run_scan(store), files)
    res, stats, _ = run_agg(store, ts_range=VD_RANGE)
    exp = vd_expected(files, ts_range=VD_RANGE)
    check_agg(res, exp)
    assert stats["rows_matched"] == exp["matched"]


def test_dictionary_encoded_value_column_keeps_bits(tmp_path):
    import pyarrow as pa
    import pyarrow.parquet as pq
    from tools.gen_ssts import _pa_schema
    store = str(tmp_path)
    os.makedirs(os.path.join(store, "data"))
    files = [Rows(q, d) for q, d in
             zip((1, 2), vd_overwrite_rows(vd_base_rows()))]
    for f in files:
        n = len(f.series)
        tbl = pa.table({"series_id": f.series, "timestamp": f.ts,
                        "value": f.value,
                        "__seq__": np.full(n, f.seq, dtype=np.uint64),
                        "__reserved__": np.zeros(n, dtype=np.uint64)},
                       schema=_pa_schema())
        path = os.path.join(store, "data", f"{f.seq}.sst")
        pq.write_table(tbl, path, row_group_size=8192, compression="NONE",
                       use_dictionary=["value"],
                       dictionary_pagesize_limit=1 << 30,
                       data_page_version="1.0", write_statistics=True)
        meta = pq.ParquetFile(path).metadata.row_group(0).column(2)
        assert "RLE_DICTIONARY" in meta.encodings
        # the writer's dictionary keeps one entry per bit pattern
        back = pq.read_table(path).column("value").to_numpy()
        assert bits_of(back).tolist() == bits_of(f.value).tolist()
    _assert_rows(run_scan(store), files)
    res, stats, _ = run_agg(store, ts_range=VD_RANGE)
    check_agg(res, vd_expected(files, ts_range=VD_RANGE))


@pytest.mark.parametrize("how", ["compact", "compact_files"])
def test_compaction_keeps_bits(tmp_path, how):
    import pyarrow.parquet as pq
    from horaedb_amd import Store
    store = str(tmp_path)
    files = build_store(store, "two", row_group=8192, codec="none")
    before = run_scan(store)
    _assert_rows(before, files)
    with Store(store) as st:
        if how == "compact":
            new_seq = st.compact(FULL, devices=[0])
        else:
            new_seq = st.compact_files([1, 2], devices=[0])
        assert [e["seq"] for e in st.catalog()] == [new_seq]
    after = run_scan(store)
    assert sorted(after) == sorted(before)
    for k in before:
        assert before[k].view(np.uint64).tolist() == \
            after[k].view(np.uint64).tolist(), k
    # the compacted file's statistics hold no NaN and bound its values
    f = pq.ParquetFile(os.path.join(store, "data", f"{new_seq}.sst"))
    vi = f.schema_arrow.names.index("value")
    vals = f.read().column("value").to_numpy()
    at = 0
    for g in range(f.metadata.num_row_groups):
        rg = f.metadata.row_group(g)
        v = vals[at:at + rg.num_rows]
        at += rg.num_rows
        st_ = rg.column(vi).statistics
        real = v[~np.isnan(v)]
        if len(real) == 0:
            assert st_ is None or not st_.has_min_max
            continue
        assert st_ is not None and st_.has_min_max
        assert st_.min == real.min() and st_.max == real.max()
    res, stats, _ = run_agg(store, ts_range=VD_RANGE)
    exp = vd_expected(files, ts_range=VD_RANGE)
    check_agg(res, exp)
    check_agg(res, exp, sums="subnormal")


def test_ingest_sort_carries_value_bits(tmp_path):
    # one 65 536-row batch through hx_write (the GPU ingest sort): equal PKs
    # keep batch order, every value's 64 bits arrive unchanged
    import pyarrow.parquet as pq
    from horaedb_amd import Store
    store = str(tmp_path)
    os.makedirs(os.path.join(store, "data"))
    n = 65_536
    rng = np.random.default_rng(17)
    series = rng.integers(0, 300, n).astype(np.uint64) * np.uint64(2**40 + 7)
    ts = rng.integers(0, 40, n).astype(np.int64) * 1000    # heavy duplicates
    bits = bits_of(np.arange(n, dtype=np.float64) - n / 2).copy()
    bits[::3] = VD_BITS[np.arange(len(bits[::3])) % len(VD_BITS)]
    # distinct NaN payloads encode the batch position among equal values
    nanp = np.arange(n, dtype=np.uint64)[1::7]
    bits[1::7] = np.uint64(0x7FF0000000000001) + nanp
    with Store(store) as st:
        seq = st.write(series, ts, from_bits(bits), enable_check=False)
    t = pq.read_table(os.path.join(store, "data", f"{seq}.sst"))
    order = np.lexsort((ts, series))            # stable
    assert t.column("series_id").to_numpy().tolist() == series[order].tolist()
    assert t.column("timestamp").to_numpy().tolist() == ts[order].tolist()
    got = bits_of(t.column("value").to_numpy())
    assert got.tolist() == bits[order].tolist()


@pytest.mark.parametrize("route", ["default", "table", "bucket_direct"])
def test_reexecuted_plan_returns_identical_minmax_bits(vd_store, route):
    from horaedb_amd import Store
    store, files, _ = vd_store
    kw, env = ROUTES[route]
    bucket_ms = kw.get("bucket_ms", 0)
    with _env(**env):
        with Store(store) as st, st.prepare(kw["ts_range"],
                                            devices=[0]) as p:
            a = p.exec_agg(ops=OPS_ALL, bucket_ms=bucket_ms)
            b = p.exec_agg(ops=OPS_ALL, bucket_ms=bucket_ms)
    exp = vd_expected(files, **kw)
    check_agg(a, exp, bucket_ms)
    check_agg(b, exp, bucket_ms)
    if bucket_ms:
        a, b = ({k: v[np.lexsort((r["bucket"], r["series_id"]))]
                 for k, v in r.items()} for r in (a, b))
    for k in ("series_id", "count", "vmin", "vmax"):
        assert a[k].view(np.uint64).tolist() == b[k].view(np.uint64).tolist()
