# The sorted row stream that hx_scan, hx_compact and hx_compact_files share
# (DESIGN.md §4 item 5): what the one helper decides for all of its callers,
# at the smallest shapes where it can go wrong. Expectations are
# oracle/scan.py's merge_scan over the rows that were written: MergeStream's
# order and operators, with the per-row validity riding as one more column
# and keep_builtin for the per-row sequences. Keys, sequences, validity and
# the 64 bits of every present value are compared exactly.
import ctypes as C
import glob
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

pytestmark = pytest.mark.gpu

ALL = (-10**15, 10**15)
UNSUPPORTED = 3


def _listing(d):
    return sorted(os.path.basename(p)
                  for p in glob.glob(os.path.join(d, "data", "*")))


# ---- every optional buffer at once: seq and valid, odd row counts -------------

NULL_FILE_ROWS = (70, 8192, 8193)   # odd total; one and two row groups


def _null_files(d):
    """Three nullable f64 files over a 300 x 40 PK grid (unique PKs within a
    file, about half shared between two files), ~30% nulls. Returns the
    oracle's batches: cols [series, ts, value bits, valid]."""
    from horaedb_amd.store import write_sst_native_nullable
    from oracle.scan import SstBatch
    os.makedirs(os.path.join(d, "data"))
    rng = np.random.default_rng(14)
    batches = []
    for seq, n in enumerate(NULL_FILE_ROWS, start=1):
        pk = np.sort(rng.choice(300 * 40, size=n, replace=False))
        series = (pk // 40 + 1).astype(np.uint64) * 1000
        ts = (pk % 40).astype(np.int64) * 1000
        value = rng.standard_normal(n) + seq
        valid = rng.random(n) >= 0.3
        write_sst_native_nullable(os.path.join(d, "data", f"{seq}.sst"),
                                  series, ts, value, seq, valid=valid)
        batches.append(SstBatch([series, ts, value.view(np.uint64), valid],
                                seq))
    return batches


def test_seq_and_valid_buffers_together(tmp_path):
    import pyarrow.parquet as pq
    from horaedb_amd import Store
    from oracle.scan import merge_scan, MERGE_LAST
    d = str(tmp_path / "store")
    batches = _null_files(d)
    series, ts, bits, valid, seqs = merge_scan(
        batches, num_primary_keys=2, merge_op=MERGE_LAST, keep_builtin=True)
    assert sum(NULL_FILE_ROWS) % 2 == 1
    assert 0 < (~valid).sum() < len(valid) < sum(NULL_FILE_ROWS)
    assert len(set(seqs.tolist())) == 3

    def check_scan(rows):
        np.testing.assert_array_equal(rows["series_id"], series)
        np.testing.assert_array_equal(rows["timestamp"], ts)
        np.testing.assert_array_equal(rows["value_valid"], valid)
        np.testing.assert_array_equal(
            rows["value"].view(np.uint64)[valid], bits[valid])

    with Store(d) as st:
        st.set_nullable_values(True)
        check_scan(st.scan(ALL, devices=[0]))          # valid, no seq
        assert st.compact_files([1, 2, 3], devices=[0]) == 4   # valid and seq
        assert [e["seq"] for e in st.catalog()] == [4]
        check_scan(st.scan(ALL, devices=[0]))
    assert _listing(d) == ["4.sst"]
    tbl = pq.read_table(os.path.join(d, "data", "4.sst"))
    col = tbl["value"].combine_chunks()
    np.testing.assert_array_equal(tbl["series_id"].to_numpy(), series)
    np.testing.assert_array_equal(tbl["timestamp"].to_numpy(), ts)
    np.testing.assert_array_equal(tbl["__seq__"].to_numpy(), seqs)
    np.testing.assert_array_equal(
        col.is_valid().to_numpy(zero_copy_only=False), valid)
    np.testing.assert_array_equal(
        col.drop_null().to_numpy(zero_copy_only=False).view(np.uint64),
        bits[valid])


# ---- the Append pass through both of its callers ------------------------------

def _append_files(d):
    """Three Binary files of 33 rows, every PK in all three."""
    from tools.gen_ssts import write_bytes_sst
    from oracle.scan import SstBatch
    rng = np.random.default_rng(33)
    series = np.repeat(np.arange(1, 12, dtype=np.uint64) * 77, 3)
    ts = np.tile(np.arange(3, dtype=np.int64) * 1000, 11)
    batches = []
    for seq in (1, 2, 3):
        vals = np.empty(33, dtype=object)
        for i in range(33):
            vals[i] = b"%d:" % seq + bytes(
                rng.integers(97, 123, rng.integers(0, 9)).astype(np.uint8)
                .tolist())
        write_bytes_sst(os.path.join(d, "data", f"{seq}.sst"), series, ts,
                        vals.tolist(), seq)
        batches.append(SstBatch([series, ts, vals], seq))
    return batches


def test_append_order_through_scan_and_compact(tmp_path):
    import oracle
    from horaedb_amd import Store
    from oracle.scan import merge_scan, MERGE_APPEND
    d = str(tmp_path / "store")
    batches = _append_files(d)
    series, ts, values = merge_scan(batches, num_primary_keys=2,
                                    merge_op=MERGE_APPEND, value_idxes=[2])
    assert len(series) == 33
    assert all(v.startswith(b"1:") and v.index(b"2:") < v.index(b"3:")
               for v in values)

    def check_scan(rows):
        np.testing.assert_array_equal(rows["series_id"], series)
        np.testing.assert_array_equal(rows["timestamp"], ts)
        assert rows["value"].tolist() == values.tolist()

    with Store(d, update_mode="append") as st:
        check_scan(st.scan(ALL, devices=[0]))
        assert st.compact(ALL, devices=[0]) == 4
        assert [e["seq"] for e in st.catalog()] == [4]
        check_scan(st.scan(ALL, devices=[0]))
    assert _listing(d) == ["4.sst"]
    out = oracle.read_sst(os.path.join(d, "data", "4.sst"))
    np.testing.assert_array_equal(out.cols[0], series)
    np.testing.assert_array_equal(out.cols[1], ts)
    assert out.cols[2].tolist() == values.tolist()
    assert (out.seq == 4).all()


# ---- an empty stream ----------------------------------------------------------

def _count_batches(st, ts_range):
    """hx_scan with a callback that only counts."""
    from horaedb_amd import store as S
    calls = []
    cb_type = C.CFUNCTYPE(C.c_int32, C.c_void_p, C.POINTER(S._ColBatch))
    cb = cb_type(lambda ctx, b: calls.append(b.contents.n_rows) or 0)
    spec, keep = st._spec(ts_range)
    ds = st._devset([0], keep)
    S._check(S._lib.hx_scan(st._h, C.byref(spec), C.byref(ds),
                            C.cast(cb, C.c_void_p), None))
    return len(calls)


def test_empty_stream(tmp_path):
    from tools.gen_ssts import write_sst
    from horaedb_amd import Store
    d = str(tmp_path / "store")
    os.makedirs(os.path.join(d, "data"))
    for seq in (1, 2):
        write_sst(os.path.join(d, "data", f"{seq}.sst"), [5, 5, 6],
                  [0, 10_000, 10_000], [1.0 * seq, 2.0, 3.0], seq)
    before = _listing(d)
    with Store(d) as st:
        cat = st.catalog()
        assert _count_batches(st, (0, 20_000)) == 1
        # inside the files' time span, between their rows: staged, all
        # filtered; and outside it: nothing staged
        assert _count_batches(st, (4_000, 5_000)) == 0
        assert _count_batches(st, (50_000, 60_000)) == 0
        assert st.compact((50_000, 60_000), devices=[0]) == 0
        assert st.catalog() == cat
    assert _listing(d) == before


# ---- refusals -----------------------------------------------------------------

def test_append_refuses_wide_file_sequences(tmp_path):
    from horaedb_amd import Store, HxError
    from horaedb_amd.store import write_sst_native_bytes
    d = str(tmp_path / "store")
    os.makedirs(os.path.join(d, "data"))
    for seq in (1, 1 << 32):
        write_sst_native_bytes(os.path.join(d, "data", f"{seq}.sst"), [5, 6],
                               [1000, 1000], [b"a", b"b"], seq)
    before = _listing(d)
    with Store(d, update_mode="append") as st:
        cat = st.catalog()
        assert [e["seq"] for e in cat] == [1, 1 << 32]
        for call in (lambda: st.scan(ALL, devices=[0]),
                     lambda: st.compact(ALL, devices=[0]),
                     lambda: st.compact_files([1, 1 << 32], devices=[0])):
            with pytest.raises(HxError) as ei:
                call()
            assert ei.value.code == UNSUPPORTED
            assert "file sequences < 2^32" in str(ei.value)
            assert st.catalog() == cat
            assert _listing(d) == before
    # Overwrite has no packed key: the same store scans
    with Store(d) as st:
        rows = st.scan(ALL, devices=[0])
    assert rows["value"].tolist() == [b"a", b"b"]
