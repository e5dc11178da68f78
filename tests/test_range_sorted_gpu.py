# Sorted-run result path of the series-range aggregate: each
# block of k_scan_agg_range2 emits its groups as one key-ordered run and two
# placement kernels assemble the result — no global table, compaction or
# sort. Every case compares against oracle.scan_agg with the suite's bar:
# keys, counts, min and max exact; sums and avg at rtol=1e-9.
import contextlib
import os
import re

import numpy as np
import pytest

import oracle
from oracle.scan import AGG_SUM, AGG_COUNT, AGG_MIN, AGG_MAX, AGG_AVG
from tools.gen_ssts import gen_dataset, gen_sst_from_arrays, middle_range

pytestmark = pytest.mark.gpu

OPS_ALL = AGG_SUM | AGG_COUNT | AGG_MIN | AGG_MAX | AGG_AVG
SUM_COUNT = AGG_SUM | AGG_COUNT
FULL = (0, 2**62)


def _sst_paths(store_dir):
    ddir = os.path.join(store_dir, "data")
    return sorted((os.path.join(ddir, f) for f in os.listdir(ddir)
                   if f.endswith(".sst")),
                  key=lambda p: int(os.path.basename(p).split(".")[0]))


_oracle_cache = {}


def _expected(store_dir, ts_range, ops, series_in=None):
    # one oracle run per (store, query), shared by the cases that repeat it
    key = (store_dir, ts_range, ops,
           None if series_in is None else tuple(series_in))
    if key not in _oracle_cache:
        ssts = [oracle.read_sst(p) for p in _sst_paths(store_dir)]
        _oracle_cache[key] = oracle.scan_agg(ssts, ts_range,
                                             series_set=series_in, ops=ops)
    return _oracle_cache[key]


def _compare(res, exp, ops):
    keys = np.asarray(res["series_id"], dtype=np.uint64)
    assert keys.tolist() == exp["series_id"].tolist(), "group keys differ"
    if len(keys) > 1:
        assert bool(np.all(keys[1:] > keys[:-1])), \
            "keys not strictly ascending as uint64"
    if ops & AGG_COUNT:
        assert res["count"].tolist() == exp["count"].tolist()
    if ops & AGG_MIN:
        np.testing.assert_array_equal(res["vmin"], exp["vmin"])
    if ops & AGG_MAX:
        np.testing.assert_array_equal(res["vmax"], exp["vmax"])
    if ops & AGG_SUM:
        np.testing.assert_allclose(res["sum"], exp["sum"], rtol=1e-9)
    if ops & AGG_AVG:
        np.testing.assert_allclose(res["avg"], exp["avg"], rtol=1e-9)


def check(store_dir, ts_range, ops, series_in=None):
    from horaedb_amd import Store
    with Store(store_dir) as st:
        res = st.scan_agg(ts_range, ops=ops, series_in=series_in,
                          devices=[0])
    _compare(res, _expected(store_dir, ts_range, ops, series_in), ops)
    return res


@contextlib.contextmanager
def _env(**kv):
    """Set environment variables for a block, unset them after."""
    assert not any(k in os.environ for k in kv)
    os.environ.update(kv)
    try:
        yield
    finally:
        for k in kv:
            del os.environ[k]


@pytest.fixture(scope="module")
def ds_plain(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("rs_plain"))
    m = gen_dataset(out, n_rows=400_000, n_series=2_000, n_ssts=8, seed=42)
    return out, m


# ---- plain parity -----------------------------------------------------------

@pytest.mark.parametrize("ops", [SUM_COUNT, OPS_ALL],
                         ids=["sum_count", "all_ops"])
@pytest.mark.parametrize("rng", ["full", "middle"])
def test_plain_parity(ds_plain, ops, rng):
    # SUM|COUNT and all-ops run different kernel instances (the min/max one
    # has another LDS layout)
    out, m = ds_plain
    res = check(out, FULL if rng == "full" else middle_range(m), ops)
    assert len(res["series_id"]) == 2_000


def test_table_route_same_queries(ds_plain):
    # HX_RANGE=0: series-only grouping on the global-table route (wave
    # kernel, compaction, sort, gather) answers the same queries
    out, m = ds_plain
    with _env(HX_RANGE="0"):
        check(out, FULL, SUM_COUNT)
        check(out, middle_range(m), OPS_ALL)


# ---- key order --------------------------------------------------------------

def test_ids_spanning_sign_bit(tmp_path):
    # the order must be unsigned: ids on both sides of 2^63
    store = str(tmp_path)
    rng = np.random.default_rng(7)
    ids = np.unique(rng.integers(1, 2**64 - 2, 300, dtype=np.uint64,
                                 endpoint=True))
    ids[-1] = np.uint64(2**63 + 12345)
    ids[0] = np.uint64(2**63 - 1)
    ids = np.unique(ids)
    assert (ids >= np.uint64(2**63)).any() and (ids < np.uint64(2**63)).any()
    for seq in (1, 2):
        series = np.repeat(ids, 4)
        ts = np.tile(np.arange(4, dtype=np.int64), len(ids)) * 10 + seq * 1000
        gen_sst_from_arrays(store, seq, series, ts, rng.random(len(series)))
    res = check(store, FULL, OPS_ALL)
    assert len(res["series_id"]) == len(ids)
    assert int(res["series_id"][-1]) >= 2**63


def test_probe_chain_stress(tmp_path):
    # 50,000 consecutive ids plus 50 ids next to 2^64-2 in one store: the
    # sampled bounds leave the last block(s) a range that is almost the whole
    # u64 space with tightly clustered keys, so every key of such a block
    # maps to the first or the last LDS slot (long probe chains that wrap) —
    # the case that used to leave LDS after 16 probes
    store = str(tmp_path)
    rng = np.random.default_rng(11)
    low = np.arange(1, 50_001, dtype=np.uint64)
    high = np.sort(np.uint64(2**64 - 2) -
                   np.arange(50, dtype=np.uint64) * np.uint64(19))
    for seq in (1, 2):
        series = np.concatenate([np.repeat(low, 2), high])
        ts = np.concatenate([np.tile(np.array([0, 10], dtype=np.int64),
                                     len(low)),
                             np.zeros(len(high), dtype=np.int64)])
        ts = ts + seq * 1000
        assert len(series) == 100_050
        gen_sst_from_arrays(store, seq, series, ts, rng.random(len(series)))
    res = check(store, FULL, OPS_ALL)
    assert len(res["series_id"]) == 50_050


# ---- overflow and retry -----------------------------------------------------

@pytest.fixture(scope="module")
def ds_wide(tmp_path_factory):
    # 100,000 series, 2 rows per series in each of 2 SSTs
    out = str(tmp_path_factory.mktemp("rs_wide"))
    m = gen_dataset(out, n_rows=400_000, n_series=100_000, n_ssts=2, seed=3)
    return out, m


def test_block_overflow_retry(ds_wide, capfd):
    # HX_RANGE_TARGET=1e9 pins the partition at 512 blocks, ~195 keys per
    # block against ne=64: attempt 0 must report block overflow, and the
    # result is exact through the re-partitioning (block count doubles per
    # attempt, up to 4096 here) — or through the global-table route if a
    # block still holds more than 64 keys at the last attempt
    out, m = ds_wide
    with _env(HX_RANGE_TARGET="1000000000", HX_RANGE_NE="64", HX_DEBUG="1"):
        res = check(out, FULL, SUM_COUNT)
    err = capfd.readouterr().err
    assert re.search(r"attempt=0 kernel=range-sorted .*nb=512 "
                     r".*block_overflow=[1-9]", err), err
    assert re.search(r"kernel=range-sorted .*nb=1024 ", err), err
    assert len(res["series_id"]) == 100_000


def test_block_overflow_retries_exhausted(ds_wide, capfd):
    # ne=16 cannot hold the ~24 keys per block of the last attempt (4096
    # blocks): the retries run out and the query finishes on the global-table
    # route (wave kernel, compaction, sort, gather), still exact
    out, m = ds_wide
    with _env(HX_RANGE_TARGET="1000000000", HX_RANGE_NE="16", HX_DEBUG="1"):
        res = check(out, FULL, OPS_ALL)
    err = capfd.readouterr().err
    assert re.search(r"attempt=3 kernel=range-sorted .*block_overflow=[1-9]",
                     err), err
    assert "kernel=wave" in err, err
    assert len(res["series_id"]) == 100_000


def test_gave_up_plan_stays_on_table_route(ds_wide, capfd):
    # one prepared, two execs: the first runs out of re-partitioning retries
    # (as above) and finishes on the wave kernel; the second must go to the
    # wave kernel directly, without another range launch
    from horaedb_amd import Store
    out, m = ds_wide
    exp = _expected(out, FULL, OPS_ALL)
    with _env(HX_RANGE_TARGET="1000000000", HX_RANGE_NE="16", HX_DEBUG="1"):
        with Store(out) as st, st.prepare(FULL, devices=[0]) as pr:
            first = pr.exec_agg(ops=OPS_ALL)
            err1 = capfd.readouterr().err
            second = pr.exec_agg(ops=OPS_ALL)
            err2 = capfd.readouterr().err
    _compare(first, exp, OPS_ALL)
    _compare(second, exp, OPS_ALL)
    assert "kernel=range-sorted" in err1 and "kernel=wave" in err1, err1
    assert "kernel=wave" in err2, err2
    assert "kernel=range-sorted" not in err2, err2


def test_staging_overflow_retry(ds_plain, capfd):
    # HX_TABLE_SLOTS=64 is the initial staging capacity: 2,000 groups do not
    # fit, the cursor reports the exact need and the second attempt fits
    out, m = ds_plain
    with _env(HX_TABLE_SLOTS="64", HX_DEBUG="1"):
        res = check(out, middle_range(m), OPS_ALL)
    err = capfd.readouterr().err
    assert re.search(r"attempt=0 kernel=range-sorted cap=64 "
                     r".*stage_overflow=[1-9]", err), err
    assert re.search(r"attempt=1 kernel=range-sorted cap=2000 "
                     r".*stage_overflow=0 block_overflow=0", err), err
    assert len(res["series_id"]) == 2_000


# ---- sparse blocks ----------------------------------------------------------

def test_three_series_one_row_each(tmp_path):
    store = str(tmp_path)
    gen_sst_from_arrays(store, 1, [3, 2**63 + 5, 2**64 - 2], [100, 200, 300],
                        [1.5, -2.5, 4.0])
    res = check(store, (0, 1000), OPS_ALL)
    assert res["series_id"].tolist() == [3, 2**63 + 5, 2**64 - 2]
    assert res["count"].tolist() == [1, 1, 1]


def test_series_set_one_percent(ds_plain):
    out, m = ds_plain
    ids = np.load(os.path.join(out, "series_ids.npy"))
    sel = ids[::100].tolist()
    res = check(out, middle_range(m), OPS_ALL, series_in=sel)
    assert len(res["series_id"]) == 20


def test_range_matching_no_row(ds_plain):
    out, m = ds_plain
    res = check(out, (17, 18), OPS_ALL)
    assert len(res["series_id"]) == 0


# ---- dedup interplay --------------------------------------------------------

def test_dedup_overlapping_generations(tmp_path):
    store = str(tmp_path)
    gen_dataset(store, n_rows=100_000, n_series=1_000, n_ssts=4, seed=8,
                overlap_gens=2)
    res = check(store, FULL, SUM_COUNT)
    assert len(res["series_id"]) == 1_000
    assert res["count"].tolist() == [100] * 1_000


def test_dedup_runs_on_pair_lane_and_row_group_edges(tmp_path):
    # equal-PK runs placed to straddle row 2k/2k+1 (one lane's pair), row
    # 2k+1/2k+2 (two lanes), lane 63/64 of a 128-row window (rows 127/128)
    # and the row-group boundary 8191/8192; plus a run every 37 rows so that
    # blocks entering the file mid-stream meet runs at every alignment
    store = str(tmp_path)
    n = 8192 + 512
    run_id = np.arange(n, dtype=np.int64)
    for a, b in [(4, 6), (127, 128), (255, 257), (8191, 8192), (8319, 8320)]:
        run_id[a:b + 1] = run_id[a]
    for a in range(300, n - 3, 37):
        run_id[a:a + 2 + (a % 2)] = run_id[a]
    run_id = np.maximum.accumulate(run_id)
    series = (run_id.astype(np.uint64) + np.uint64(1)) * np.uint64(2**40 + 1)
    ts = np.full(n, 500, dtype=np.int64)
    vals = np.arange(n, dtype=np.float64)
    assert series[127] == series[128] and series[8191] == series[8192]
    gen_sst_from_arrays(store, 1, series, ts, vals, sort=False,
                        row_group=8192)
    res = check(store, (0, 1000), SUM_COUNT)
    assert res["count"].tolist() == [1] * len(np.unique(series))


# ---- re-execution -----------------------------------------------------------

def _same(a, b):
    assert a["series_id"].tolist() == b["series_id"].tolist()
    assert a["count"].tolist() == b["count"].tolist()
    np.testing.assert_allclose(a["sum"], b["sum"], rtol=1e-12)


def test_reexecute_one_prepared(ds_plain):
    from horaedb_amd import Store
    out, m = ds_plain
    with Store(out) as st, st.prepare(middle_range(m), devices=[0]) as pr:
        rs = [pr.exec_agg(ops=OPS_ALL) for _ in range(3)]
    _compare(rs[0], _expected(out, middle_range(m), OPS_ALL), OPS_ALL)
    for r in rs[1:]:
        _same(r, rs[0])
        np.testing.assert_array_equal(r["vmin"], rs[0]["vmin"])
        np.testing.assert_array_equal(r["vmax"], rs[0]["vmax"])


def test_three_prepared_three_threads(ds_plain):
    from concurrent.futures import ThreadPoolExecutor
    from horaedb_amd import Store
    out, m = ds_plain
    with Store(out) as st:
        preps = [st.prepare(middle_range(m), devices=[0]) for _ in range(3)]
        try:
            with ThreadPoolExecutor(3) as ex:
                rs = list(ex.map(lambda p: p.exec_agg(ops=SUM_COUNT), preps))
        finally:
            for p in preps:
                p.close()
    _compare(rs[0], _expected(out, middle_range(m), SUM_COUNT), SUM_COUNT)
    for r in rs[1:]:
        _same(r, rs[0])
