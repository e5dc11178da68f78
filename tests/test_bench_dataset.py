# The driver's bench entry starts with get_dataset: guard generation +
# reuse + oracle readability on a tiny config (CPU-only).
import json
import os
import sys
import types

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def _args(tmp, rows=20_000, series=100, ssts=4):
    a = types.SimpleNamespace()
    a.rows, a.series, a.ssts = rows, series, ssts
    a.seed = 7
    a.compression = "none"
    a.ts_encoding = "PLAIN"
    a.data_dir = str(tmp)
    return a


class _FakeResult:
    """Stands in for store.HeldResult: n_groups + take(idx)."""

    def __init__(self, n):
        self.n_groups = n

    def take(self, idx=None):
        n = self.n_groups
        cols = {"series_id": np.arange(n, dtype=np.uint64) *
                np.uint64(0x9E3779B97F4A7C15),
                "sum": np.arange(n) * 0.5,
                "count": np.arange(n, dtype=np.uint64)}
        return {k: (v if idx is None else v[idx]) for k, v in cols.items()}


def _load_dir(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_outputs_small_table_is_written_whole(tmp_path):
    import bench

    res = _FakeResult(1000)
    bench.dump_outputs(str(tmp_path / "a"), res, seed=7)
    got = _load_dir(str(tmp_path / "a"))
    assert set(got) == {"series_id_hi", "series_id_lo", "sum", "count",
                        "rows", "n_groups"}
    assert all(a.dtype == np.float64 for a in got.values())
    exp = res.take()
    sid = (got["series_id_hi"].astype(np.uint64) << np.uint64(32)) | \
        got["series_id_lo"].astype(np.uint64)
    np.testing.assert_array_equal(sid, exp["series_id"])  # exact round trip
    np.testing.assert_array_equal(got["sum"], exp["sum"])
    np.testing.assert_array_equal(got["count"], exp["count"])
    np.testing.assert_array_equal(got["rows"], np.arange(1000))
    assert got["n_groups"].tolist() == [1000]


def test_dump_outputs_large_table_is_a_fixed_seeded_sample(tmp_path):
    import bench

    n = 2_000_000  # 3 columns x 8 B x 2M rows + ids split in two > budget
    res = _FakeResult(n)
    bench.dump_outputs(str(tmp_path / "a"), res, seed=7)
    bench.dump_outputs(str(tmp_path / "b"), res, seed=7)
    a, b = _load_dir(str(tmp_path / "a")), _load_dir(str(tmp_path / "b"))
    total = sum(os.path.getsize(os.path.join(str(tmp_path / "a"), f))
                for f in os.listdir(str(tmp_path / "a")))
    assert total <= 64 * 10**6
    for k in a:
        np.testing.assert_array_equal(a[k], b[k])  # same args => same rows
    rows = a["rows"].astype(np.int64)
    assert 0 < len(rows) < n and bool(np.all(np.diff(rows) > 0))
    np.testing.assert_array_equal(a["sum"], res.take(rows)["sum"])
    np.testing.assert_array_equal(a["count"], rows)
    assert a["n_groups"].tolist() == [n]


def test_get_dataset_generate_reuse_and_scan(tmp_path):
    import bench
    import oracle
    from oracle.scan import AGG_SUM, AGG_COUNT
    from tools.gen_ssts import middle_range

    out, m = bench.get_dataset(_args(tmp_path), rank=0)
    assert m["n_rows"] == 20_000 and m["n_ssts"] == 4
    # reuse hits the cache (same tag)
    out2, m2 = bench.get_dataset(_args(tmp_path), rank=0)
    assert out2 == out and m2["n_rows"] == m["n_rows"]
    # a different rank gets a different seed => different dir
    out3, _ = bench.get_dataset(_args(tmp_path), rank=1)
    assert out3 != out

    # the generated store is oracle-readable and internally consistent
    ddir = os.path.join(out, "data")
    ssts = [oracle.read_sst(os.path.join(ddir, f))
            for f in sorted(os.listdir(ddir)) if f.endswith(".sst")]
    assert sum(s.n_rows for s in ssts) == 20_000
    res = oracle.scan_agg(ssts, middle_range(m), ops=AGG_SUM | AGG_COUNT)
    assert 0 < len(res["series_id"]) <= 100
    assert int(res["count"].sum()) > 0
    # SSTs are PK-sorted (writer invariant; series stays u64 — ids span
    # the full u64 range)
    for s in ssts:
        sid, ts = s.cols[0], s.cols[1]
        adj = (sid[:-1] < sid[1:]) | ((sid[:-1] == sid[1:]) &
                                      (ts[:-1] <= ts[1:]))
        assert bool(np.all(adj))
