# OPTIONAL (nullable) columns, host side: the reference marks
# every column nullable, so its default files carry a definition-level block
# in every page — inside the compressed stream for v1 Snappy/Zstd pages.
# Staging decodes that block (horaedb_amd/csrc/def_levels.h) instead of
# trusting the page statistics. Two checks, no GPU involved:
#   * the stand-alone check program (`make def_levels_check`, ASan+UBSan when
#     the host compiler links them) over level and Snappy-prefix vectors;
#   * the real staging parse of pyarrow-written files (hx_debug_page_levels:
#     chunk read, page walk, codec step, levels -> bitmap) against pyarrow's
#     is_valid().
import ctypes
import os
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "horaedb_amd", "csrc")

COLS = ["series_id", "timestamp", "value", "__seq__", "__reserved__"]


def test_def_levels_check_program():
    b = subprocess.run(["make", "-C", CSRC, "def_levels_check"],
                       capture_output=True, text=True)
    assert b.returncode == 0, b.stdout + b.stderr
    r = subprocess.run([os.path.join(CSRC, "def_levels_check")],
                       capture_output=True, text=True)
    print(b.stdout + r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == "ALL OK"
    assert len(lines) > 90 and not any(ln.endswith("FAIL") for ln in lines)


def _zstd_loadable():
    try:
        ctypes.CDLL("libzstd.so.1")
        return True
    except OSError:
        return False


def write_nullable_sst(path, series, ts, value, seq, value_null=None,
                       row_group=8192, compression="none", version="1.0",
                       nullable=True):
    """One SST shaped like the reference's: five nullable fields,
    __reserved__ all null. value_null is a bool mask of null value rows."""
    import pyarrow as pa
    import pyarrow.parquet as pq
    n = len(series)
    types = [pa.uint64(), pa.int64(), pa.float64(), pa.uint64(), pa.uint64()]
    schema = pa.schema([pa.field(c, t, nullable=nullable)
                        for c, t in zip(COLS, types)])
    reserved = pa.nulls(n, pa.uint64()) if nullable else \
        pa.array(np.zeros(n, dtype=np.uint64))
    tbl = pa.table([
        pa.array(np.ascontiguousarray(series, dtype=np.uint64)),
        pa.array(np.ascontiguousarray(ts, dtype=np.int64)),
        pa.array(np.ascontiguousarray(value, dtype=np.float64),
                 mask=value_null),
        pa.array(np.full(n, seq, dtype=np.uint64)),
        reserved], schema=schema)
    pq.write_table(tbl, path, row_group_size=row_group,
                   compression="NONE" if compression == "none"
                   else compression.upper(),
                   data_page_version=version, use_dictionary=False,
                   column_encoding={c: "PLAIN" for c in COLS},
                   write_statistics=True)
    return tbl


@pytest.mark.parametrize("rows", [1, 40, 100, 8192, 8193])
@pytest.mark.parametrize("null_frac", [0.0, 0.3])
@pytest.mark.parametrize("version", ["1.0", "2.0"])
@pytest.mark.parametrize("codec", ["none", "snappy", "zstd"])
def test_staging_levels_match_pyarrow(tmp_path, codec, version, null_frac,
                                      rows):
    if codec == "zstd" and not _zstd_loadable():
        pytest.skip("libzstd.so.1 not loadable")
    import pyarrow.parquet as pq
    from horaedb_amd.store import page_levels
    rng = np.random.default_rng(rows * 7 + int(null_frac * 10))
    series = np.sort(rng.integers(0, 1 << 62, rows, dtype=np.uint64))
    ts = np.arange(rows, dtype=np.int64) * 1000
    value = rng.random(rows)
    mask = rng.random(rows) < null_frac
    path = str(tmp_path / "1.sst")
    write_nullable_sst(path, series, ts, value, 1, value_null=mask,
                       compression=codec, version=version)
    pf = pq.ParquetFile(path)
    assert pf.num_row_groups == (2 if rows == 8193 else 1)
    for rg in range(pf.num_row_groups):
        tbl = pf.read_row_group(rg)
        for col in ("series_id", "timestamp", "value"):
            exp = tbl[col].is_valid().to_numpy(zero_copy_only=False)
            valid, n_valid, lvl = page_levels(path, rg, col)
            assert len(valid) == len(exp)
            assert n_valid == int(exp.sum())
            np.testing.assert_array_equal(valid, exp)
            assert lvl > 0  # every OPTIONAL page carries a level block


def test_level_block_sizes_v1(tmp_path):
    # the block's length moves with the page size: 6 bytes below 64 values,
    # 7 up to 8191, 8 at 8192 (4-byte length + RLE header + value byte), so
    # the PLAIN body behind it is in general not 8-byte aligned
    from horaedb_amd.store import page_levels
    for rows, want in ((40, 6), (63, 6), (64, 7), (8191, 7), (8192, 8)):
        path = str(tmp_path / f"{rows}.sst")
        write_nullable_sst(path, np.arange(rows), np.arange(rows),
                           np.ones(rows), 1, compression="snappy")
        valid, n_valid, lvl = page_levels(path, 0, "value")
        assert (n_valid, lvl) == (rows, want) and valid.all()


def test_required_column_reports_all_valid(tmp_path):
    from horaedb_amd.store import page_levels
    path = str(tmp_path / "1.sst")
    write_nullable_sst(path, np.arange(100), np.arange(100), np.ones(100), 1,
                       nullable=False, compression="snappy")
    valid, n_valid, lvl = page_levels(path, 0, "value")
    assert valid.all() and len(valid) == 100 and n_valid == 100 and lvl == 0


def test_open_mixed_required_and_optional(tmp_path):
    # hx_open reads footers only: a store may mix both kinds of file
    from horaedb_amd import Store
    ddir = tmp_path / "data"
    ddir.mkdir()
    n = 300
    for seq, nullable in ((1, False), (2, True), (3, True)):
        write_nullable_sst(str(ddir / f"{seq}.sst"),
                           np.arange(n, dtype=np.uint64),
                           np.arange(n, dtype=np.int64) + seq * 10_000,
                           np.ones(n), seq, nullable=nullable,
                           compression="snappy" if seq != 3 else "none",
                           value_null=(np.arange(n) % 3 == 0)
                           if seq == 3 else None)
    with Store(str(tmp_path)) as st:
        cat = st.catalog()
    assert sorted(e["seq"] for e in cat) == [1, 2, 3]
    assert all(e["n_rows"] == n for e in cat)
