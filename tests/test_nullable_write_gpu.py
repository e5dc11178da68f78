# Writing null values on the GPU path (DESIGN §4 kernel 1d, §2 write side):
# k_pack_optional byte-exact through its test hook, the round trip through
# the read side's kernel 1c, compaction under hx_set_nullable_values(1), and
# the device ingest sort of hx_write_nullable.
#
# Expectations are numpy over the rows that were written, by the recipe at
# the top of tests/test_optional_gpu.py (concatenate, keep the last row per
# PK by (seq, file row), keep the validity bit with its row). Keys, counts,
# validity bits and every value are compared as uint64; rtol=1e-9 applies to
# sums and avg only.
import os

import numpy as np
import pytest

from test_optional_gpu import (FULL, Sst, _check_store, _ref_rows,
                               _small_store, dedup_rows, run_scan, write_sst)

pytestmark = pytest.mark.gpu

STALE = 0x7FF0000000000002
SPECIAL = np.array([STALE, 0x8000000000000000, 0x0000000000000001,
                    0x7FF0000000000000, 0xFFF0000000000000],
                   dtype=np.uint64)

PATTERNS = ["all_present", "all_null", "one_null", "one_present",
            "alternating", "null_word_first_bit", "null_word_last_bit",
            "null_group_first_row", "null_group_last_row", "random30"]


def _pattern(kind, n, row_group, rng):
    r = np.arange(n)
    return {"all_present": lambda: np.ones(n, dtype=bool),
            "all_null": lambda: np.zeros(n, dtype=bool),
            "one_null": lambda: r != n // 2,
            "one_present": lambda: r == n // 3,
            "alternating": lambda: r % 2 == 1,
            "null_word_first_bit": lambda: r % 64 != 0,
            "null_word_last_bit": lambda: r % 64 != 63,
            "null_group_first_row": lambda: r % row_group != 0,
            "null_group_last_row":
                lambda: (r % row_group != row_group - 1) & (r != n - 1),
            "random30": lambda: rng.random(n) >= 0.3}[kind]()


def _expected_pack(values, present_out, src_rows, n, row_group):
    """What kernel 1d must leave for output rows whose source row is
    src_rows[i] and whose presence is present_out[i]: (bitmap words,
    n_valid per group, slot index and value of every present row)."""
    groups = (n + row_group - 1) // row_group
    padded = np.zeros(groups * row_group, dtype=bool)
    padded[:n] = present_out
    bitmap = np.packbits(padded, bitorder="little").view(np.uint64)
    per_group = padded.reshape(groups, row_group)
    n_valid = per_group.sum(axis=1).astype(np.uint32)
    rank = (np.cumsum(per_group, axis=1) - 1).reshape(-1)[:n]
    rows = np.flatnonzero(present_out)
    slots = rows // row_group * row_group + rank[rows]
    return bitmap, n_valid, slots, values[src_rows[rows]]


@pytest.mark.parametrize("row_group", [64, 8192, 16384])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 8191, 8192, 8193, 16384 + 65])
def test_pack_optional_kernel_byte_exact(n, row_group):
    # row_group 16384 = 256 bitmap words: the smallest that needs a second
    # 128-word tile and the carry between tiles
    from horaedb_amd.store import pack_optional
    rng = np.random.default_rng(n * 7 + row_group)
    for perm_kind in ("null", "identity", "reversed", "random"):
        # a random permutation draws (with repeats) from MORE source rows
        # than it emits
        n_src = n + 37 if perm_kind == "random" else n
        values = rng.integers(0, 1 << 64, n_src, dtype=np.uint64)
        values[rng.permutation(n_src)[:len(SPECIAL)]] = SPECIAL[:n_src]
        perm = {"null": None, "identity": np.arange(n, dtype=np.uint32),
                "reversed": np.arange(n, dtype=np.uint32)[::-1].copy(),
                "random": rng.integers(0, n_src, n).astype(np.uint32)
                }[perm_kind]
        src_rows = np.arange(n) if perm is None else perm.astype(np.int64)
        for kind in PATTERNS:
            valid_src = _pattern(kind, n_src, row_group, rng)
            exp = _expected_pack(values, valid_src[src_rows], src_rows, n,
                                 row_group)
            for form in ("words", "bits"):
                kw = ({"valid_words": valid_src.astype(np.uint64)}
                      if form == "words" else
                      {"valid_bits": np.packbits(valid_src,
                                                 bitorder="little")})
                packed, bitmap, n_valid, errs = pack_optional(
                    values, n, row_group, perm=perm, **kw)
                where = f"{perm_kind}/{kind}/{form}"
                assert errs == 0, where
                # bits above the row count and whole trailing words are zero
                # because the expectation's are
                np.testing.assert_array_equal(bitmap, exp[0], err_msg=where)
                np.testing.assert_array_equal(n_valid, exp[1], err_msg=where)
                np.testing.assert_array_equal(packed[exp[2]], exp[3],
                                              err_msg=where)
        # no validity source at all: every row present
        packed, bitmap, n_valid, errs = pack_optional(values, n, row_group,
                                                      perm=perm)
        exp = _expected_pack(values, np.ones(n, dtype=bool), src_rows, n,
                             row_group)
        assert errs == 0
        np.testing.assert_array_equal(bitmap, exp[0])
        np.testing.assert_array_equal(n_valid, exp[1])
        np.testing.assert_array_equal(packed[exp[2]], exp[3])


@pytest.mark.parametrize("form", ["words", "bits"])
def test_pack_optional_perm_entry_out_of_range_counts_one_error(form):
    from horaedb_amd.store import pack_optional
    n = 200
    values = np.arange(n, dtype=np.uint64) + 1000
    perm = np.arange(n, dtype=np.uint32)[::-1].copy()
    perm[70] = n                                  # == n_src: not followed
    valid_src = np.arange(n) % 3 != 0
    kw = ({"valid_words": valid_src.astype(np.uint64)} if form == "words"
          else {"valid_bits": np.packbits(valid_src, bitorder="little")})
    packed, bitmap, n_valid, errs = pack_optional(values, n, 64, perm=perm,
                                                  **kw)
    assert errs == 1
    src_rows = perm.astype(np.int64)
    present = np.zeros(n, dtype=bool)
    ok = src_rows < n
    present[ok] = valid_src[src_rows[ok]]         # row 70 comes back null
    src_rows[70] = 0
    exp = _expected_pack(values, present, src_rows, n, 64)
    np.testing.assert_array_equal(bitmap, exp[0])
    np.testing.assert_array_equal(n_valid, exp[1])
    np.testing.assert_array_equal(packed[exp[2]], exp[3])


# ---- files ---------------------------------------------------------------------

def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _assert_scan(store, ssts):
    """hx_scan against the numpy dedup: rows, validity, every present value's
    64 bits."""
    rows = run_scan(store)
    series, ts, value, valid = dedup_rows(ssts)
    np.testing.assert_array_equal(rows["series_id"], series)
    np.testing.assert_array_equal(rows["timestamp"], ts)
    if valid.all():
        assert "value_valid" not in rows
    else:
        np.testing.assert_array_equal(rows["value_valid"], valid)
    np.testing.assert_array_equal(_bits(rows["value"])[valid],
                                  _bits(value)[valid])


def _read_value(path):
    import pyarrow.parquet as pq
    pf = pq.ParquetFile(path)
    tbl = pf.read()
    col = tbl["value"].combine_chunks()
    nulls = sum(pf.metadata.row_group(g).column(2).statistics.null_count
                for g in range(pf.num_row_groups))
    return {"series": tbl["series_id"].to_numpy(),
            "ts": tbl["timestamp"].to_numpy(),
            "seq": tbl["__seq__"].to_numpy(),
            "valid": col.is_valid().to_numpy(zero_copy_only=False),
            "bits": col.drop_null().to_numpy(zero_copy_only=False)
            .view(np.uint64),
            "nullable": tbl.schema.field("value").nullable,
            "null_count": nulls, "row_groups": pf.num_row_groups}


def test_nullable_file_round_trips_through_kernel_1c(tmp_path):
    from horaedb_amd.store import write_sst_native_nullable
    store = str(tmp_path)
    os.makedirs(os.path.join(store, "data"))
    n = 20_000
    rng = np.random.default_rng(12)
    series = np.sort(rng.integers(0, 1 << 63, n, dtype=np.uint64))
    ts = rng.integers(0, 100_000, n).astype(np.int64)
    value = rng.standard_normal(n)
    value[rng.permutation(n)[:len(SPECIAL)]] = SPECIAL.view(np.float64)
    valid = rng.random(n) >= 0.3
    valid[8192:8192 + 64] = False          # a null word at a row-group edge
    write_sst_native_nullable(os.path.join(store, "data", "1.sst"), series,
                              ts, value, 1, valid=valid)
    _assert_scan(store, [Sst(1, series, ts, value, valid)])
    # and a nullable file without nulls reads like a REQUIRED one
    store2 = str(tmp_path / "b")
    os.makedirs(os.path.join(store2, "data"))
    write_sst_native_nullable(os.path.join(store2, "data", "1.sst"), series,
                              ts, value, 1)
    _assert_scan(store2, [Sst(1, series, ts, value, np.ones(n, dtype=bool))])


def _overlap_store(store):
    """Two files of the _small_store shape (500 rows, ts overlap): file 2
    rewrites the PKs of the first 25 series, nulls every 7th row in either
    file at different phases — so file 2 puts nulls over file 1's values and
    values over file 1's nulls."""
    n = 500
    series = np.repeat(np.arange(1, 51, dtype=np.uint64) * 1000, 10)
    ts = np.tile(np.arange(10, dtype=np.int64) * 1000, 50)
    i = np.arange(n)
    ts2 = np.where(i < 250, ts, ts + 2)
    rng = np.random.default_rng(8)
    return [write_sst(store, 1, series, ts, rng.random(n) + 1,
                      value_null=i % 7 == 0),
            write_sst(store, 2, series, ts2, rng.random(n) + 2,
                      value_null=i % 7 == 3)]


@pytest.mark.parametrize("how", ["compact", "compact_files"])
def test_compaction_keeps_null_values(tmp_path, how):
    from horaedb_amd import Store
    store = str(tmp_path)
    ssts = _overlap_store(store)
    _, _, _, valid = dedup_rows(ssts)
    assert 0 < (~valid).sum() < len(valid)
    _check_store(store, ssts)              # before: scan rows + both routes
    ddir = os.path.join(store, "data")
    with Store(store) as st:
        st.set_nullable_values(True)
        new_seq = (st.compact(FULL, devices=[0]) if how == "compact"
                   else st.compact_files([1, 2], devices=[0]))
        assert new_seq == 3
        assert [e["seq"] for e in st.catalog()] == [new_seq]
    assert os.listdir(ddir) == [f"{new_seq}.sst"]
    _check_store(store, ssts)              # after: identical to the numpy rows
    _assert_scan(store, ssts)
    out = _read_value(os.path.join(ddir, f"{new_seq}.sst"))
    assert out["nullable"]
    np.testing.assert_array_equal(out["valid"], valid)
    assert out["null_count"] == int((~valid).sum())


def test_null_keeps_shadowing_across_the_set_boundary(tmp_path):
    from horaedb_amd import Store
    store = str(tmp_path)
    one = np.array([False])
    ssts = [write_sst(store, 1, [7], [1000], [1.5]),
            write_sst(store, 2, [7], [1000], [2.5], value_null=~one),
            write_sst(store, 3, [7], [2000], [3.5])]
    with Store(store) as st:
        st.set_nullable_values(True)
        new_seq = st.compact_files([2, 3], devices=[0])
        assert [e["seq"] for e in st.catalog()] == [1, new_seq]
    out = _read_value(os.path.join(store, "data", f"{new_seq}.sst"))
    assert out["ts"].tolist() == [1000, 2000]
    assert out["seq"].tolist() == [2, 3]
    assert out["valid"].tolist() == [False, True]
    rows = run_scan(store)                 # all files: seq 1 stays shadowed
    assert rows["timestamp"].tolist() == [1000, 2000]
    assert rows["value_valid"].tolist() == [False, True]
    assert _bits(rows["value"])[1] == _bits([3.5])[0]
    _check_store(store, ssts)


def test_second_level_compaction_of_a_nullable_output(tmp_path):
    from horaedb_amd import Store
    store = str(tmp_path)
    ssts = _overlap_store(store)
    with Store(store) as st:
        st.set_nullable_values(True)
        assert st.compact(FULL, devices=[0]) == 3
    # a newer pyarrow file over the OPTIONAL PLAIN uncompressed output
    i = np.arange(500)
    ssts.append(write_sst(store, 4, ssts[0].series, ssts[0].ts,
                          np.full(500, 4.0), value_null=i % 5 == 1))
    _check_store(store, ssts)
    with Store(store) as st:
        st.set_nullable_values(True)
        assert st.compact(FULL, devices=[0]) == 5
        assert [e["seq"] for e in st.catalog()] == [5]
    _check_store(store, ssts)
    _assert_scan(store, ssts)


def test_compaction_of_20000_row_files_spans_row_groups(tmp_path):
    # 2 x 20 000 rows, half of them the same PKs: 30 000 survivors = three
    # full row groups and a short one; compacted twice
    from horaedb_amd import Store
    store = str(tmp_path)
    rng = np.random.default_rng(6)
    ssts = []
    for k in (1, 3):
        series, ts, value = _ref_rows(k, np.random.default_rng(100))
        ssts.append(write_sst(store, k, series, ts, value + k,
                              value_null=rng.random(len(series)) < 0.3))
    _, _, _, valid = dedup_rows(ssts)
    assert len(valid) == 30_000
    with Store(store) as st:
        st.set_nullable_values(True)
        first = st.compact(FULL, devices=[0])
        out = _read_value(os.path.join(store, "data", f"{first}.sst"))
        assert out["row_groups"] == 4
        np.testing.assert_array_equal(out["valid"], valid)
        second = st.compact_files([first], devices=[0])
        assert [e["seq"] for e in st.catalog()] == [second]
    _check_store(store, ssts)
    _assert_scan(store, ssts)
    out = _read_value(os.path.join(store, "data", f"{second}.sst"))
    np.testing.assert_array_equal(out["valid"], valid)
    assert out["null_count"] == int((~valid).sum())


def test_setting_1_over_inputs_without_nulls(tmp_path):
    from horaedb_amd import Store
    store = str(tmp_path)
    ssts = _small_store(store)
    with Store(store) as st:
        st.set_nullable_values(True)
        new_seq = st.compact(FULL, devices=[0])
        assert [e["seq"] for e in st.catalog()] == [new_seq]
    out = _read_value(os.path.join(store, "data", f"{new_seq}.sst"))
    assert out["nullable"] and out["null_count"] == 0 and out["valid"].all()
    _check_store(store, ssts)


def test_write_nullable_device_sort_equals_host_stable_sort(tmp_path):
    from horaedb_amd import Store
    store = str(tmp_path)
    os.makedirs(os.path.join(store, "data"))
    n = 65536 + 65                         # at the device-sort threshold
    rng = np.random.default_rng(23)
    series = rng.integers(1, 3000, n, dtype=np.uint64)
    ts = rng.integers(0, 40, n).astype(np.int64) * 1000     # many equal PKs
    value = rng.standard_normal(n)
    value[rng.permutation(n)[:len(SPECIAL)]] = SPECIAL.view(np.float64)
    valid = rng.random(n) >= 0.3
    with Store(store) as st:
        st.set_nullable_values(True)
        seq = st.write(series, ts, value, enable_check=False, valid=valid)
    order = np.lexsort((ts, series))       # stable: batch order among ties
    out = _read_value(os.path.join(store, "data", f"{seq}.sst"))
    assert out["nullable"]
    np.testing.assert_array_equal(out["series"], series[order])
    np.testing.assert_array_equal(out["ts"], ts[order])
    np.testing.assert_array_equal(out["valid"], valid[order])
    np.testing.assert_array_equal(out["bits"],
                                  _bits(value[order][valid[order]]))
    _assert_scan(store, [Sst(seq, series[order], ts[order], value[order],
                             valid[order])])
