# Writing Binary value stores, host side (DESIGN §2 write side, §4 kernel
# 1f's host twin, §9n): hx::ba_build_pages_host through its ctypes export
# against the page's definition, the Binary-value writer through
# hx_write_sst_bytes read back by pyarrow and the oracle, hx_write_bytes'
# host route, and the refusals. No GPU involved.
import os
import subprocess

import numpy as np
import pytest

import ba_shapes as shapes

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "horaedb_amd", "csrc")
COLS = ["series_id", "timestamp", "value", "__seq__", "__reserved__"]
UNSUPPORTED, INVALID, SCHEMA = 3, 6, 7


def test_check_program():
    b = subprocess.run(["make", "-C", CSRC, "ba_pages_check"],
                       capture_output=True, text=True)
    assert b.returncode == 0, b.stdout + b.stderr
    r = subprocess.run([os.path.join(CSRC, "ba_pages_check")],
                       capture_output=True, text=True)
    print(b.stdout + r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == "all ok"
    assert len(lines) > 25
    assert not any(ln.endswith("FAIL") for ln in lines)


# ---- host twin against the definition of the page -------------------------

def test_twin_every_length_at_every_alignment():
    from horaedb_amd.store import ba_pages_host
    src, handles = shapes.lens_by_alignment()
    pages, errs, over = ba_pages_host(src, handles)
    assert (errs, over) == (0, 0)
    assert pages == shapes.expected_pages(src, handles)


@pytest.mark.parametrize("n", shapes.ROW_COUNTS)
def test_twin_row_counts(n):
    from horaedb_amd.store import ba_pages_host
    src, handles = shapes.rows_case(n)
    pages, errs, over = ba_pages_host(src, handles)
    assert (errs, over) == (0, 0)
    assert len(pages) == (n + 8191) // 8192
    assert pages == shapes.expected_pages(src, handles)


def test_twin_groups():
    from horaedb_amd.store import ba_pages_host
    src, handles, gs = shapes.groups_case()
    pages, errs, over = ba_pages_host(src, handles, group_start=gs)
    assert (errs, over) == (0, 0)
    assert len(pages) == 2
    assert pages == shapes.expected_pages(src, handles, gs)


def test_twin_refusals():
    from horaedb_amd.store import ba_pages_host
    src, handles = shapes.rows_case(65)
    bad = handles.copy()
    bad[7] = (np.uint64(len(src) - 2) << np.uint64(20)) | np.uint64(3)
    pages, errs, over = ba_pages_host(src, bad)
    assert (errs, over) == (1, 0)
    assert pages == shapes.expected_pages(src, bad, refused={7})
    # group bounds that decrease, and that pass the source rows
    gs = np.array([0, 10, 8, 30, 66], dtype=np.uint32)
    pages, errs, over = ba_pages_host(src, handles, group_start=gs)
    assert (errs, over) == (2, 0)
    assert pages == shapes.expected_pages(src, handles, gs, refused={1, 3})
    # one byte above the value limit
    src2, h2 = shapes.make_source([1 << 19, 1 << 19, 5], 3)
    gs2 = np.array([0, 2, 3], dtype=np.uint32)
    pages, errs, over = ba_pages_host(src2, h2, group_start=gs2)
    assert (errs, over) == (0, 1)
    assert pages == shapes.expected_pages(src2, h2, gs2, refused={0})


# ---- the writer ------------------------------------------------------------

def _rows(n, seed, n_series=50, n_ts=30):
    rng = np.random.default_rng(seed)
    series = np.sort(rng.integers(0, 2**63, n_series, dtype=np.uint64))
    s = rng.choice(series, size=n)
    t = rng.integers(0, n_ts, n).astype(np.int64) * 1000
    order = np.lexsort((t, s))
    lens = rng.choice([0, 1, 3, 8, 17, 64, 65, 300], size=n)
    vals = [rng.integers(0, 256, int(k), dtype=np.uint8).tobytes()
            for k in lens]
    return s[order], t[order], [vals[i] for i in order]


@pytest.mark.parametrize("per_row_seq", [False, True])
def test_native_file_reads_back(tmp_path, per_row_seq):
    import pyarrow as pa
    import pyarrow.parquet as pq
    import oracle
    from horaedb_amd.store import write_sst_native_bytes
    n = 20_000
    s, t, vals = _rows(n, 5)
    seqs = (np.random.default_rng(6).integers(1, 9, n).astype(np.uint64)
            if per_row_seq else None)
    path = str(tmp_path / "7.sst")
    write_sst_native_bytes(path, s, t, vals, 7, seqs=seqs)
    tbl = pq.read_table(path)
    assert tbl.schema.names == COLS
    assert tbl.schema.field("value").type == pa.binary()
    assert not any(tbl.schema.field(c).nullable for c in COLS)
    md = pq.ParquetFile(path).metadata
    assert md.num_row_groups == 3
    for g in range(3):
        c = md.row_group(g).column(2)
        assert c.compression == "UNCOMPRESSED"
        assert c.physical_type == "BYTE_ARRAY"
    want_seq = seqs if per_row_seq else np.full(n, 7, np.uint64)
    np.testing.assert_array_equal(
        tbl.column("series_id").to_numpy().astype(np.uint64), s)
    np.testing.assert_array_equal(tbl.column("timestamp").to_numpy(), t)
    assert tbl.column("value").to_pylist() == vals
    np.testing.assert_array_equal(
        tbl.column("__seq__").to_numpy().astype(np.uint64), want_seq)
    assert not tbl.column("__reserved__").to_numpy().any()
    b = oracle.read_sst(path, with_builtins=True)
    np.testing.assert_array_equal(b.cols[0], s)
    np.testing.assert_array_equal(b.cols[1], t)
    assert b.cols[2].tolist() == vals
    np.testing.assert_array_equal(b.cols[3], want_seq)


def test_statistics_are_lexicographic_and_capped(tmp_path):
    import pyarrow.parquet as pq
    from horaedb_amd.store import write_sst_native_bytes
    vals = [b"b", b"", b"ab", b"\xff\x00", b"b\x00"]
    path = str(tmp_path / "1.sst")
    write_sst_native_bytes(path, np.arange(5), np.zeros(5), vals, 1)
    st = pq.ParquetFile(path).metadata.row_group(0).column(2).statistics
    assert (st.min, st.max) == (b"", b"\xff\x00")
    write_sst_native_bytes(path, np.arange(2), np.zeros(2),
                           [b"a", b"z" * 65], 1)
    c = pq.ParquetFile(path).metadata.row_group(0).column(2)
    assert c.statistics is None or not c.statistics.has_min_max


def test_native_and_pyarrow_files_mix(tmp_path):
    from tools.gen_ssts import write_bytes_sst
    from horaedb_amd import Store
    from horaedb_amd.store import write_sst_native_bytes
    d = str(tmp_path / "store")
    s, t, vals = _rows(500, 9)
    write_bytes_sst(os.path.join(d, "data", "1.sst"), s, t, vals, 1)
    write_sst_native_bytes(os.path.join(d, "data", "2.sst"), s, t, vals, 2)
    with Store(d) as st:
        cat = st.catalog()
        assert [c["seq"] for c in cat] == [1, 2]
        assert cat[0]["n_rows"] == cat[1]["n_rows"] == 500
        assert cat[0]["ts_min"] == cat[1]["ts_min"]
        assert cat[0]["ts_max"] == cat[1]["ts_max"]
        assert st.schema()["columns"][2]["type"] == "binary"


def test_write_bytes_host_route(tmp_path):
    # below 64k rows the batch is sorted and paged on the host: the file is
    # the one write_sst_native_bytes writes for the stably sorted rows
    from horaedb_amd import Store
    from horaedb_amd.store import write_sst_native_bytes
    d = str(tmp_path / "store")
    os.makedirs(os.path.join(d, "data"))
    rng = np.random.default_rng(12)
    s, t, vals = _rows(3000, 11)
    order = rng.permutation(3000)
    s, t, vals = s[order], t[order], [vals[i] for i in order]
    with Store(d) as st:
        seq = st.write_bytes(s, t, vals)
        assert seq == 1
        assert [c["seq"] for c in st.catalog()] == [1]
        assert st.write_bytes(s[:10], t[:10], vals[:10]) == 2
    stable = np.lexsort((t, s))
    ref = str(tmp_path / "ref.sst")
    write_sst_native_bytes(ref, s[stable], t[stable],
                           [vals[i] for i in stable], 1)
    with open(ref, "rb") as f, open(os.path.join(d, "data", "1.sst"),
                                    "rb") as g:
        assert f.read() == g.read()
    with Store(d) as st:                     # reopens as a Binary store
        assert st.schema()["columns"][2]["type"] == "binary"


# ---- refusals: the stated code, nothing written -----------------------------

def _state(d, st):
    return sorted(os.listdir(os.path.join(d, "data"))), st.catalog()


def test_value_at_the_limit_is_written_and_above_refused(tmp_path):
    from horaedb_amd import Store, HxError
    from horaedb_amd.store import write_sst_native_bytes
    d = str(tmp_path / "store")
    os.makedirs(os.path.join(d, "data"))
    ok = [b"x", b"y" * shapes.MAX_LEN]
    over = [b"x", b"y" * (shapes.MAX_LEN + 1)]
    k = np.arange(2)
    path = str(tmp_path / "1.sst")
    write_sst_native_bytes(path, k, k, ok, 1)
    os.unlink(path)
    with pytest.raises(HxError) as ei:
        write_sst_native_bytes(path, k, k, over, 1)
    assert ei.value.code == INVALID and "2^20" in str(ei.value)
    assert not os.path.exists(path)
    with Store(d) as st:
        assert st.write_bytes(k, k, ok) == 1
        before = _state(d, st)
        with pytest.raises(HxError) as ei:
            st.write_bytes(k, k, over)
        assert ei.value.code == INVALID and "2^20" in str(ei.value)
        assert _state(d, st) == before


def test_row_group_page_above_int32_max_is_refused(tmp_path):
    # 2049 rows declaring 2^20 - 1 bytes each make one row group's page
    # 2049 * (2^20 - 1 + 4) = 2 148 538 371 bytes > INT32_MAX. Both entry
    # points refuse from the offsets (the handles) alone, before a value byte
    # is read, so the declared bytes need not exist: raw entry points, a
    # 16-byte buffer.
    import ctypes as C
    from horaedb_amd import Store, HxError
    from horaedb_amd.store import _lib, _check
    n = 2049
    assert n * (shapes.MAX_LEN + 4) > 2**31 - 1
    series = np.arange(n, dtype=np.uint64)
    ts = np.zeros(n, dtype=np.int64)
    offs = np.arange(n + 1, dtype=np.int64) * shapes.MAX_LEN
    tiny = np.zeros(16, dtype=np.uint8)
    sp = series.ctypes.data_as(C.POINTER(C.c_uint64))
    tp = ts.ctypes.data_as(C.POINTER(C.c_int64))
    op = offs.ctypes.data_as(C.POINTER(C.c_int64))

    path = str(tmp_path / "1.sst")
    for row_group in (8192, n):
        with pytest.raises(HxError) as ei:
            _check(_lib.hx_write_sst_bytes(path.encode(), sp, tp,
                                           tiny.ctypes.data, op, None, 1, n,
                                           row_group))
        assert ei.value.code == UNSUPPORTED and "INT32_MAX" in str(ei.value)
        assert not os.path.exists(path)

    d = str(tmp_path / "store")
    os.makedirs(os.path.join(d, "data"))
    with Store(d) as st:
        assert st.write_bytes([1], [0], [b"a"]) == 1
        before = _state(d, st)
        out = C.c_uint64(99)
        with pytest.raises(HxError) as ei:
            _check(_lib.hx_write_bytes(st._h, sp, tp, tiny.ctypes.data, op, n,
                                       1, C.byref(out)))
        assert ei.value.code == UNSUPPORTED and "INT32_MAX" in str(ei.value)
        assert out.value == 0
        assert _state(d, st) == before
    with Store(d) as st:
        assert _state(d, st) == before


def test_write_bytes_refused_on_f64_store_and_writer_settings(tmp_path):
    from horaedb_amd import Store, HxError
    from horaedb_amd.store import write_sst_native, CODEC_SNAPPY
    d = str(tmp_path / "store")
    os.makedirs(os.path.join(d, "data"))
    k = np.arange(4)
    write_sst_native(os.path.join(d, "data", "1.sst"), k, k, k * 1.0, 1)
    with Store(d) as st:
        before = _state(d, st)
        with pytest.raises(HxError) as ei:
            st.write_bytes(k, k, [b"a"] * 4)
        assert ei.value.code == SCHEMA
        assert _state(d, st) == before
    e = str(tmp_path / "empty")
    os.makedirs(os.path.join(e, "data"))
    for setting in ("nullable", "codec"):
        with Store(e) as st:
            if setting == "nullable":
                st.set_nullable_values(True)
            else:
                st.set_write_codec(CODEC_SNAPPY)
            with pytest.raises(HxError) as ei:
                st.write_bytes(k, k, [b"a"] * 4)
            assert ei.value.code == UNSUPPORTED
            assert _state(e, st) == ([], [])


def test_f64_write_refused_on_binary_store(tmp_path):
    # it used to add an f64 SST, after which hx_open refused the store
    from horaedb_amd import Store, HxError
    d = str(tmp_path / "store")
    os.makedirs(os.path.join(d, "data"))
    k = np.arange(4)
    with Store(d) as st:
        st.write_bytes(k, k, [b"a", b"", b"ccc", b"dd"])
        before = _state(d, st)
        for kw in ({}, {"valid": np.array([True, False, True, True])}):
            with pytest.raises(HxError) as ei:
                st.write(k, k, k * 1.0, **kw)
            assert ei.value.code == UNSUPPORTED
            assert "hx_write_bytes" in str(ei.value)
        assert _state(d, st) == before
    with Store(d) as st:
        assert [c["seq"] for c in st.catalog()] == [1]


def test_segment_check_and_argument_checks(tmp_path):
    from horaedb_amd import Store, HxError
    d = str(tmp_path / "store")
    os.makedirs(os.path.join(d, "data"))
    with Store(d, segment_duration_ms=1000) as st:
        with pytest.raises(HxError) as ei:
            st.write_bytes([1, 1], [10, 1010], [b"a", b"b"])
        assert ei.value.code == INVALID
        assert _state(d, st) == ([], [])
        assert st.write_bytes([1, 1], [10, 1010], [b"a", b"b"],
                              enable_check=False) == 1


def test_index_write_refuses_a_tag_at_the_limit(tmp_path):
    from horaedb_amd import Store, HxError
    d = str(tmp_path / "store")
    os.makedirs(os.path.join(d, "data"))
    with Store(d) as st:
        for keys, vals in (([b"k" * (1 << 20)], [b"v"]),
                           ([b"k"], [b"v" * (1 << 20)])):
            with pytest.raises(HxError) as ei:
                st.index_write(keys, vals, [1])
            assert ei.value.code == INVALID and "2^20" in str(ei.value)
        assert not os.path.exists(os.path.join(d, "index")) or \
            os.listdir(os.path.join(d, "index")) == []
        assert st.index_write([b"k" * ((1 << 20) - 1)], [b"v"], [1]) == 1
