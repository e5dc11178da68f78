# Value chunks of several data pages in Binary value stores, host side
# (DESIGN §2, §3, §4 kernel 1h's host twin, §10): staging of pyarrow-written
# multi-page value chunks under every codec, page version and column form; the
# GPU-free writer under a page limit (hx::ba_cut_pages) read back by pyarrow
# and by our own staging; the setter's refusals; the stand-alone check. No GPU
# involved.
import os
import subprocess

import numpy as np
import pytest

from test_bytes_snappy_cpu import _image, _skip_struct

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "horaedb_amd", "csrc")
FORMAT, UNSUPPORTED, INVALID = 2, 3, 6
CODECS = ["NONE", "SNAPPY", "ZSTD"]
FORMS = [(c, v, n) for c in CODECS for v in ("1.0", "2.0")
         for n in (False, True)]
# pyarrow looks at the page size every 64 rows and closes a page at 70 000
# bytes: row groups of 1024 rows of ~300 B values split 4 / 4 / 2
MULTI = dict(row_group=1024, write_batch_size=64, data_page_size=70_000)


def test_check_program():
    b = subprocess.run(["make", "-C", CSRC, "ba_multipage_check"],
                       capture_output=True, text=True)
    assert b.returncode == 0, b.stdout + b.stderr
    r = subprocess.run([os.path.join(CSRC, "ba_multipage_check")],
                       capture_output=True, text=True)
    print(b.stdout + r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == "all ok"
    assert len(lines) > 10
    assert not any(ln.endswith("FAIL") for ln in lines)


# ---- read ---------------------------------------------------------------------

def letter_rows(n, seed, n_series=60, n_ts=40, max_len=601,
                random_bytes=False, min_len=0):
    """n rows sorted by PK, values of min_len .. max_len - 1 letters (or
    random bytes)."""
    rng = np.random.default_rng(seed)
    pool = np.sort(rng.integers(0, 2**63, n_series, dtype=np.uint64))
    s = rng.choice(pool, size=n)
    t = rng.integers(0, n_ts, n).astype(np.int64) * 1000
    lo, hi = (0, 256) if random_bytes else (65, 90)
    vals = [bytes(rng.integers(lo, hi, rng.integers(min_len, max_len)).astype(
        np.uint8).tolist()) for _ in range(n)]
    order = np.lexsort((t, s))
    return s[order], t[order], [vals[i] for i in order]


def chunk_pages(path, rg, col):
    """[(num_values, uncompressed_size, payload as stored)] of every data page
    of a chunk whose pages are v1 (this library's writer)."""
    import pyarrow.parquet as pq
    cm = pq.ParquetFile(path).metadata.row_group(rg).column(col)
    with open(path, "rb") as f:
        f.seek(cm.data_page_offset)
        chunk = f.read(cm.total_compressed_size)
    pages, pos, unc = [], 0, 0
    while pos < len(chunk):
        top = {}
        end = _skip_struct(chunk, pos, top)
        # DataPageHeader.num_values: the first i32 of the nested struct
        n_values = _nested_first_i32(chunk, pos)
        pages.append((n_values, top[2], chunk[end:end + top[3]]))
        unc += (end - pos) + top[2]
        pos = end + top[3]
    assert pos == len(chunk)
    assert cm.total_uncompressed_size == unc
    return pages


def _nested_first_i32(buf, pos):
    """num_values of a v1 PageHeader as this library writes it: fields 1, 2, 3
    are i32, field 5 the DataPageHeader whose field 1 is num_values."""
    from test_bytes_snappy_cpu import _varint
    for _ in range(3):
        assert buf[pos] & 15 == 5
        _, pos = _varint(buf, pos + 1)
    assert buf[pos] == 0x2C         # field 5 (delta 2), struct
    assert buf[pos + 1] == 0x15     # field 1, i32
    v, _ = _varint(buf, pos + 2)
    return (v >> 1) ^ -(v & 1)


def n_data_pages(path, rg, col):
    """Pages of a chunk anyone wrote (v1 or v2 headers, statistics or not),
    counted by walking the thrift page headers; the files here have no
    dictionary pages."""
    import pyarrow.parquet as pq
    cm = pq.ParquetFile(path).metadata.row_group(rg).column(col)
    with open(path, "rb") as f:
        f.seek(cm.data_page_offset)
        chunk = f.read(cm.total_compressed_size)
    pos, n = 0, 0
    while pos < len(chunk):
        top, pos = _generic_header(chunk, pos)
        pos += top[3]
        n += 1
    return n


def _generic_header(buf, pos):
    """Any thrift-compact PageHeader: returns ({field id: i32}, end)."""
    from test_bytes_snappy_cpu import _varint

    def skip(pos, typ):
        if typ in (1, 2):
            return pos
        if typ == 3:
            return pos + 1
        if typ in (4, 5, 6):
            return _varint(buf, pos)[1]
        if typ == 7:
            return pos + 8
        if typ == 8:
            n, pos = _varint(buf, pos)
            return pos + n
        if typ == 12:
            return struct(pos, None)
        raise AssertionError("thrift type %d" % typ)

    def struct(pos, top):
        fid = 0
        while True:
            b = buf[pos]
            pos += 1
            if b == 0:
                return pos
            if b >> 4:
                fid += b >> 4
            else:
                z, pos = _varint(buf, pos)
                fid = (z >> 1) ^ -(z & 1)
            if b & 15 == 5 and top is not None:
                v, pos = _varint(buf, pos)
                top[fid] = (v >> 1) ^ -(v & 1)
            else:
                pos = skip(pos, b & 15)

    top = {}
    return top, struct(pos, top)


@pytest.fixture(scope="module")
def multi_rows():
    return letter_rows(2500, 31)


@pytest.mark.parametrize("codec,version,nullable", FORMS)
def test_staging_reads_multi_page_value_chunks(tmp_path, multi_rows, codec,
                                               version, nullable):
    from tools.gen_ssts import write_bytes_sst
    from horaedb_amd.store import page_levels
    s, t, vals = multi_rows
    path = str(tmp_path / "1.sst")
    write_bytes_sst(path, s, t, vals, 1, sort=False, compression=codec,
                    nullable=nullable, data_page_version=version, **MULTI)
    assert [n_data_pages(path, g, 2) for g in range(3)] == [4, 4, 2]
    assert all(n_data_pages(path, g, c) == 1
               for g in range(3) for c in (0, 1, 3))
    for g, rows in enumerate((1024, 1024, 2500 - 2048)):
        valid, n_valid, lvl = page_levels(path, g, "value")
        assert len(valid) == rows and n_valid == rows and valid.all()
        assert (lvl > 0) == nullable
        for col in ("series_id", "timestamp", "__seq__"):
            valid, n_valid, _ = page_levels(path, g, col)
            assert n_valid == rows and valid.all()


def test_staging_reads_a_reference_default_file(tmp_path):
    # what the reference's writer gives with its defaults (1 MiB pages looked
    # at every 1024 rows): 8192 values of mean 200 B are two pages
    from tools.gen_ssts import write_bytes_sst
    from horaedb_amd.store import page_levels
    s, t, vals = letter_rows(8192, 32, max_len=401)
    path = str(tmp_path / "1.sst")
    write_bytes_sst(path, s, t, vals, 1, sort=False, compression="SNAPPY",
                    nullable=True)
    assert n_data_pages(path, 0, 2) == 2
    valid, n_valid, lvl = page_levels(path, 0, "value")
    assert len(valid) == 8192 and n_valid == 8192 and valid.all() and lvl > 0


@pytest.mark.parametrize("codec", CODECS)
@pytest.mark.parametrize("version", ["1.0", "2.0"])
def test_null_in_a_later_page_is_refused(tmp_path, multi_rows, codec,
                                         version):
    from tools.gen_ssts import write_bytes_sst
    from horaedb_amd import HxError
    from horaedb_amd.store import page_levels
    s, t, vals = multi_rows
    vals = list(vals)
    vals[900] = None              # row group 0, its last page
    path = str(tmp_path / "1.sst")
    write_bytes_sst(path, s, t, vals, 1, sort=False, compression=codec,
                    nullable=True, data_page_version=version, **MULTI)
    assert n_data_pages(path, 0, 2) == 4
    with pytest.raises(HxError) as ei:
        page_levels(path, 0, "value")
    assert ei.value.code == UNSUPPORTED
    assert "column value" in str(ei.value) and "1.sst" in str(ei.value)
    assert "Binary value column" in str(ei.value)
    page_levels(path, 1, "value")         # the other row groups are fine


def test_multi_page_key_columns_are_refused_as_before(tmp_path, multi_rows):
    from tools.gen_ssts import write_bytes_sst
    from horaedb_amd import HxError
    from horaedb_amd.store import page_levels
    s, t, vals = multi_rows
    path = str(tmp_path / "1.sst")
    write_bytes_sst(path, s, t, vals, 1, sort=False, row_group=1024,
                    write_batch_size=64, data_page_size=4096)
    assert n_data_pages(path, 0, 0) > 1
    for col in ("series_id", "timestamp"):
        with pytest.raises(HxError) as ei:
            page_levels(path, 0, col)
        assert ei.value.code == UNSUPPORTED
        assert "expected one data page per chunk" in str(ei.value)
    valid, n_valid, _ = page_levels(path, 0, "value")
    assert n_valid == 1024


# ---- write --------------------------------------------------------------------

def cut_rule(lens, limit):
    """The rule of ba_pages.h over one row group's value lengths, restated:
    [(rows, bytes)] per page."""
    pages, rows, size = [], 0, 0
    for r0 in range(0, len(lens), 1024):
        batch = lens[r0:r0 + 1024]
        rows += len(batch)
        size += sum(4 + ln for ln in batch)
        if r0 + 1024 >= len(lens) or (limit and size >= limit):
            pages.append((rows, size))
            rows = size = 0
    return pages


@pytest.fixture(scope="module")
def write_rows():
    # 20 000 rows: three row groups, the last short
    s, t, vals = letter_rows(20_000, 33, n_series=400, max_len=12)
    seqs = np.arange(20_000, dtype=np.uint64) % 5 + 1
    return s, t, vals, seqs


@pytest.mark.parametrize("codec", [0, 1])
@pytest.mark.parametrize("limit", [4096, 40_000])
def test_writer_cuts_pages_by_the_rule(tmp_path, write_rows, codec, limit):
    from horaedb_amd.store import (write_sst_native_bytes, page_levels,
                                   snappy_compress_host)
    import pyarrow.parquet as pq
    s, t, vals, seqs = write_rows
    p1, p0 = str(tmp_path / "cut.sst"), str(tmp_path / "one.sst")
    write_sst_native_bytes(p1, s, t, vals, 9, seqs=seqs, codec=codec,
                           page_limit=limit)
    write_sst_native_bytes(p0, s, t, vals, 9, seqs=seqs, codec=codec,
                           page_limit=0)
    tb = pq.read_table(p1)
    assert tb.equals(pq.read_table(p0))
    np.testing.assert_array_equal(tb["series_id"].to_numpy(), s)
    np.testing.assert_array_equal(tb["timestamp"].to_numpy(), t)
    assert tb["value"].to_pylist() == vals
    np.testing.assert_array_equal(tb["__seq__"].to_numpy(), seqs)
    m1, m0 = pq.ParquetFile(p1).metadata, pq.ParquetFile(p0).metadata
    assert m1.num_row_groups == m0.num_row_groups == 3
    n_cut = 0
    for g in range(3):
        rows = vals[g * 8192:(g + 1) * 8192]
        want = cut_rule([len(v) for v in rows], limit)
        assert 1 <= len(want) <= (len(rows) + 1023) // 1024
        pages = chunk_pages(p1, g, 2)
        assert [(p[0], p[1]) for p in pages] == want
        n_cut += len(pages) > 1
        a, b = m1.row_group(g).column(2), m0.row_group(g).column(2)
        assert a.num_values == b.num_values == len(rows)
        assert a.statistics.min == b.statistics.min == min(rows)
        assert a.statistics.max == b.statistics.max == max(rows)
        image, at = _image(rows), 0
        for n_values, ulen, payload in pages:
            part = image[at:at + ulen]
            at += ulen
            if codec:
                assert payload == snappy_compress_host(part)
            else:
                assert payload == part
        assert at == len(image)
        for c in (0, 1, 3, 4):
            assert len(chunk_pages(p1, g, c)) == 1
        valid, n_valid, _ = page_levels(p1, g, "value")
        assert n_valid == len(rows) and valid.all()
    # ~9.5 B a row: a full row group is ~78 KB and is cut under both limits;
    # the last one (3616 rows, ~34 KB) never reaches 40 000 and stays whole
    assert n_cut == {4096: 3, 40_000: 2}[limit]


@pytest.mark.parametrize("codec", [0, 1])
def test_limit_never_reached_and_limit_zero(tmp_path, write_rows, codec):
    from horaedb_amd.store import write_sst_native_bytes
    s, t, vals, seqs = write_rows
    paths = [str(tmp_path / x) for x in ("old", "zero", "big", "ref")]
    write_sst_native_bytes(paths[0], s, t, vals, 9, seqs=seqs, codec=codec)
    write_sst_native_bytes(paths[1], s, t, vals, 9, seqs=seqs, codec=codec,
                           page_limit=0)
    write_sst_native_bytes(paths[2], s, t, vals, 9, seqs=seqs, codec=codec,
                           page_limit=1 << 30)
    from horaedb_amd.store import BYTES_PAGE_LIMIT_REFERENCE
    write_sst_native_bytes(paths[3], s, t, vals, 9, seqs=seqs, codec=codec,
                           page_limit=BYTES_PAGE_LIMIT_REFERENCE)
    files = []
    for p in paths:
        with open(p, "rb") as f:
            files.append(f.read())
    assert files[0] == files[1] == files[2] == files[3]


def test_out_of_range_limits_are_refused(tmp_path, write_rows):
    from horaedb_amd import HxError, Store
    from horaedb_amd.store import write_sst_native_bytes
    s, t, vals, seqs = write_rows
    path = str(tmp_path / "x.sst")
    for bad in ((1 << 30) + 1, 0xFFFFFFFF, -1, 1 << 32):
        with pytest.raises(HxError) as ei:
            write_sst_native_bytes(path, s[:10], t[:10], vals[:10], 1,
                                   page_limit=bad)
        assert ei.value.code == INVALID
        assert not os.path.exists(path)
    d = str(tmp_path / "store")
    os.makedirs(os.path.join(d, "data"))
    with Store(d) as st:
        for bad in ((1 << 30) + 1, 0xFFFFFFFF, -1, 1 << 32):
            with pytest.raises(HxError) as ei:
                st.set_bytes_page_limit(bad)
            assert ei.value.code == INVALID
        st.set_bytes_page_limit(1)
        st.set_bytes_page_limit(1 << 30)
        st.set_bytes_page_limit(0)


def test_page_limit_needs_a_binary_store(tmp_path):
    from horaedb_amd import HxError, Store
    d = str(tmp_path / "store")
    os.makedirs(os.path.join(d, "data"))
    with Store(d) as st:
        st.write(np.arange(10, dtype=np.uint64), np.arange(10) * 1000,
                 np.arange(10, dtype=np.float64))
        with pytest.raises(HxError) as ei:
            st.set_bytes_page_limit(4096)
        assert ei.value.code == UNSUPPORTED
        st.set_bytes_page_limit(0)


def test_write_bytes_host_route_with_limit(tmp_path):
    # below 64k rows the ingest runs on the host: the same file as the
    # GPU-free writer's over the sorted rows
    from horaedb_amd import Store
    from horaedb_amd.store import write_sst_native_bytes
    rng = np.random.default_rng(34)
    n = 9000
    s = rng.integers(0, 300, n).astype(np.uint64)
    t = rng.integers(0, 40, n).astype(np.int64) * 1000
    vals = [bytes(rng.integers(65, 90, rng.integers(0, 30)).astype(
        np.uint8).tolist()) for _ in range(n)]
    order = np.lexsort((t, s))
    for codec in (0, 1):
        d = str(tmp_path / f"store{codec}")
        os.makedirs(os.path.join(d, "data"))
        with Store(d) as st:
            st.set_bytes_write_codec(codec)
            st.set_bytes_page_limit(30_000)
            assert st.write_bytes(s, t, vals, enable_check=False) == 1
        ref = str(tmp_path / f"ref{codec}.sst")
        write_sst_native_bytes(ref, s[order], t[order],
                               [vals[i] for i in order], 1, codec=codec,
                               page_limit=30_000)
        out = os.path.join(d, "data", "1.sst")
        with open(ref, "rb") as f, open(out, "rb") as g:
            assert f.read() == g.read()
        assert len(chunk_pages(out, 0, 2)) > 1


# ---- kernel 1h's host twin ------------------------------------------------------

BATCH_ROW_COUNTS = [0, 1, 1023, 1024, 1025, 8192, 8193, 20000]
BATCH_ROW_GROUPS = [1024, 8192, 3000]


def batch_row_len(n, seed=35):
    """row_len as the size pass leaves it: lengths with a few refused rows."""
    rng = np.random.default_rng(seed + n)
    row_len = rng.integers(0, 5000, n).astype(np.uint32)
    if n:
        row_len[rng.integers(0, n, max(1, n // 50))] = 0x80000000
        row_len[n - 1] = (1 << 20) - 1
    return row_len


def expected_batch_sums(row_len, row_group):
    out = []
    for g0 in range(0, len(row_len), row_group):
        rg = row_len[g0:g0 + row_group]
        for b0 in range(0, len(rg), 1024):
            b = rg[b0:b0 + 1024].astype(np.uint64)
            out.append(int(np.where(b & 0x80000000, 4, b + 4).sum()))
    return out


@pytest.mark.parametrize("row_group", BATCH_ROW_GROUPS)
@pytest.mark.parametrize("n", BATCH_ROW_COUNTS)
def test_batch_sizes_twin(n, row_group):
    from horaedb_amd.store import ba_batch_sizes_host
    row_len = batch_row_len(n)
    assert ba_batch_sizes_host(row_len, row_group).tolist() == \
        expected_batch_sums(row_len, row_group)
