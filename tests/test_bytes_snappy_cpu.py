# Snappy pages for Binary value stores, host side (DESIGN §2, §3 the blob's
# tail, §4 kernel 1g's host twin, §9o): staging of pyarrow-written Snappy
# BYTE_ARRAY value pages, the Binary-value writer under codec Snappy read back
# by pyarrow, hx::ba_page_minmax_host against Python's min()/max(), the host
# route of hx_write_bytes under hx_set_bytes_write_codec, the setter's
# refusals, and the stand-alone check. No GPU involved.
import os
import subprocess

import numpy as np
import pytest

import ba_minmax_shapes as mm
import snappy_shapes

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "horaedb_amd", "csrc")
UNSUPPORTED, INVALID = 3, 6
FORMS = [("1.0", False), ("1.0", True), ("2.0", False), ("2.0", True)]


def test_check_program():
    b = subprocess.run(["make", "-C", CSRC, "ba_snappy_check"],
                       capture_output=True, text=True)
    assert b.returncode == 0, b.stdout + b.stderr
    r = subprocess.run([os.path.join(CSRC, "ba_snappy_check")],
                       capture_output=True, text=True)
    print(b.stdout + r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == "all ok"
    assert len(lines) > 10
    assert not any(ln.endswith("FAIL") for ln in lines)


# ---- staging ----------------------------------------------------------------

def _rows(n, seed, n_series=50, n_ts=30, max_len=9):
    rng = np.random.default_rng(seed)
    pool = np.sort(rng.integers(0, 2**63, n_series, dtype=np.uint64))
    s = rng.choice(pool, size=n)
    t = rng.integers(0, n_ts, n).astype(np.int64) * 1000
    vals = [bytes(rng.integers(65, 90, rng.integers(0, max_len)).astype(
        np.uint8).tolist()) for _ in range(n)]
    order = np.lexsort((t, s))
    return s[order], t[order], [vals[i] for i in order]


@pytest.mark.parametrize("version,nullable", FORMS)
def test_staging_reads_pyarrow_snappy_value_pages(tmp_path, version,
                                                  nullable):
    from tools.gen_ssts import write_bytes_sst
    from horaedb_amd.store import page_levels
    import pyarrow.parquet as pq
    s, t, vals = _rows(20_000, 5)
    path = str(tmp_path / "1.sst")
    write_bytes_sst(path, s, t, vals, 1, sort=False, compression="SNAPPY",
                    nullable=nullable, data_page_version=version)
    md = pq.ParquetFile(path).metadata
    assert md.num_row_groups == 3
    for g, rows in enumerate((8192, 8192, 20_000 - 2 * 8192)):
        assert md.row_group(g).column(2).compression == "SNAPPY"
        valid, n_valid, lvl = page_levels(path, g, "value")
        assert len(valid) == rows and n_valid == rows and valid.all()
        assert (lvl > 0) == nullable


@pytest.mark.parametrize("version", ["1.0", "2.0"])
def test_null_value_is_still_refused(tmp_path, version):
    from tools.gen_ssts import write_bytes_sst
    from horaedb_amd import HxError
    from horaedb_amd.store import page_levels
    s, t, vals = _rows(500, 6)
    vals[77] = None
    path = str(tmp_path / "1.sst")
    write_bytes_sst(path, s, t, vals, 1, sort=False, compression="SNAPPY",
                    nullable=True, data_page_version=version)
    with pytest.raises(HxError) as ei:
        page_levels(path, 0, "value")
    assert ei.value.code == UNSUPPORTED
    assert "column value" in str(ei.value) and "1.sst" in str(ei.value)
    assert "Binary value column" in str(ei.value)


# ---- the writer under codec Snappy -----------------------------------------

def _varint(buf, pos):
    v = shift = 0
    while True:
        b = buf[pos]
        pos += 1
        v |= (b & 0x7F) << shift
        shift += 7
        if not b & 0x80:
            return v, pos


def _skip_struct(buf, pos, top=None):
    """Thrift compact struct of i32 fields and nested structs (a v1
    PageHeader as this library writes it); top collects the outer i32s."""
    fid = 0
    while True:
        b = buf[pos]
        pos += 1
        if b == 0:
            return pos
        assert b >> 4, "long-form field ids are not written"
        fid += b >> 4
        if b & 15 == 5:
            v, pos = _varint(buf, pos)
            if top is not None:
                top[fid] = (v >> 1) ^ -(v & 1)
        else:
            assert b & 15 == 12
            pos = _skip_struct(buf, pos)


def _page(path, rg, col):
    """(uncompressed_page_size, payload as stored) of the chunk's one page."""
    import pyarrow.parquet as pq
    cm = pq.ParquetFile(path).metadata.row_group(rg).column(col)
    with open(path, "rb") as f:
        f.seek(cm.data_page_offset)
        chunk = f.read(cm.total_compressed_size)
    top = {}
    pos = _skip_struct(chunk, 0, top)
    assert top[3] == len(chunk) - pos
    assert cm.total_uncompressed_size == pos + top[2]
    return top[2], chunk[pos:]


def _image(vals):
    return b"".join(len(v).to_bytes(4, "little") + v for v in vals)


def test_codec_snappy_file_reads_back(tmp_path):
    from horaedb_amd.store import write_sst_native_bytes, CODEC_SNAPPY
    import pyarrow as pa
    import pyarrow.parquet as pq
    n = 20_000
    s, t, vals = _rows(n, 7, max_len=40)
    seqs = np.arange(n, dtype=np.uint64) % 5 + 1
    p1, p0, pold = (str(tmp_path / x) for x in ("s.sst", "n.sst", "old.sst"))
    write_sst_native_bytes(p1, s, t, vals, 9, seqs=seqs, codec=CODEC_SNAPPY)
    write_sst_native_bytes(p0, s, t, vals, 9, seqs=seqs, codec=0)
    write_sst_native_bytes(pold, s, t, vals, 9, seqs=seqs)
    with open(p0, "rb") as f, open(pold, "rb") as g:
        assert f.read() == g.read()
    tb = pq.read_table(p1)
    assert tb.equals(pq.read_table(p0))
    np.testing.assert_array_equal(tb["series_id"].to_numpy(), s)
    np.testing.assert_array_equal(tb["timestamp"].to_numpy(), t)
    assert tb["value"].to_pylist() == vals
    np.testing.assert_array_equal(tb["__seq__"].to_numpy(), seqs)
    m1, m0 = pq.ParquetFile(p1).metadata, pq.ParquetFile(p0).metadata
    assert m1.num_row_groups == m0.num_row_groups == 3
    codec = pa.Codec("snappy")
    for g in range(3):
        rows = vals[g * 8192:(g + 1) * 8192]
        for c in range(5):
            a, b = m1.row_group(g).column(c), m0.row_group(g).column(c)
            assert a.compression == "SNAPPY" and \
                b.compression == "UNCOMPRESSED"
            assert a.statistics.min == b.statistics.min
            assert a.statistics.max == b.statistics.max
            u1, stream = _page(p1, g, c)
            u0, raw = _page(p0, g, c)
            assert u1 == u0 == len(raw)
            assert a.total_compressed_size < b.total_compressed_size
            got = codec.decompress(stream, decompressed_size=u1).to_pybytes()
            assert got == raw
            if c == 2:
                assert raw == _image(rows)
                assert a.statistics.min == min(rows)
                assert a.statistics.max == max(rows)


def _value_stream(tmp_path, vals):
    from horaedb_amd.store import write_sst_native_bytes, CODEC_SNAPPY
    import pyarrow as pa
    import pyarrow.parquet as pq
    n = len(vals)
    path = str(tmp_path / f"v{n}_{len(vals[0])}.sst")
    write_sst_native_bytes(path, np.arange(n), np.zeros(n, np.int64), vals, 1,
                           codec=CODEC_SNAPPY)
    ulen, stream = _page(path, 0, 2)
    assert pa.Codec("snappy").decompress(
        stream, decompressed_size=ulen).to_pybytes() == _image(vals)
    assert pq.read_table(path)["value"].to_pylist() == vals
    return ulen, stream


def test_incompressible_page_is_stored(tmp_path):
    rng = np.random.default_rng(3)
    vals = [bytes(rng.integers(0, 256, 4000, dtype=np.uint8).tolist())
            for _ in range(30)]
    ulen, stream = _value_stream(tmp_path, vals)
    n, elements = snappy_shapes.parse(stream)
    # hx_snappy_stored_literal's shape: the preamble and ONE literal
    assert n == ulen and elements == [("L", ulen)]
    assert len(stream) <= ulen + 10


@pytest.mark.parametrize("distance", [65535, 65536])
def test_far_repetition(tmp_path, distance):
    # value 1 opens with the 32 bytes value 0 opens with, exactly `distance`
    # bytes further on in the page image (len0, v0, len1, v1). The zeros in
    # between leave as one long copy, so the block's table entries survive
    # (snappy_shapes' distance pages, as values).
    rng = np.random.default_rng(4)
    blk = bytes(rng.integers(1, 256, 32, dtype=np.uint8).tolist())
    vals = [blk + b"\0" * (distance - 36),
            blk + bytes(rng.integers(1, 256, 8, dtype=np.uint8).tolist())]
    image = _image(vals)
    at = 8 + len(vals[0])
    assert image[at:at + 32] == image[at - distance:at - distance + 32] == blk
    ulen, stream = _value_stream(tmp_path, vals)
    n, elements = snappy_shapes.parse(stream)
    assert n == ulen
    far = [e for e in elements if e[0] == "C" and e[1] > 64]
    if distance == 65535:
        # the repeat as the image has it: the two zero bytes that close len1
        # repeat the two that close len0
        start = at
        while image[start - 1] == image[start - 1 - distance]:
            start -= 1
        assert at - start == 2
        assert far == [("C", 65535, at + 32 - start, 2)]
    else:
        # a 2-byte offset cannot say 65536 and longer offsets are not emitted
        assert far == []


# ---- kernel 1g's host twin ---------------------------------------------------

@pytest.mark.parametrize("case", mm.cases(), ids=lambda c: c[0])
def test_minmax_twin(case):
    from horaedb_amd.store import ba_page_minmax_host
    _, vals, row_group, skip = case
    assert ba_page_minmax_host(vals, row_group, skip) == \
        mm.expected(vals, row_group, skip)


def test_minmax_hook_refuses_sizes_that_do_not_add_up():
    import ctypes as C
    from horaedb_amd import HxError
    from horaedb_amd.store import _lib, _check
    image = np.frombuffer(_image([b"ab", b"c"]), dtype=np.uint8)
    page_off = np.array([0, len(image)], dtype=np.uint64)
    out = np.zeros(140, dtype=np.uint8)
    for lens in ([2, 2], [3, 1]):
        row_len = np.array(lens, dtype=np.uint32)
        with pytest.raises(HxError) as ei:
            _check(_lib.hx_debug_ba_page_minmax_host(
                image.ctypes.data,
                page_off.ctypes.data_as(C.POINTER(C.c_uint64)),
                row_len.ctypes.data_as(C.POINTER(C.c_uint32)), 2, 8192,
                out.ctypes.data))
        assert ei.value.code == INVALID


# ---- host ingest and the setting --------------------------------------------

def _state(d, st):
    return sorted(os.listdir(os.path.join(d, "data"))), st.catalog()


def test_write_bytes_host_route_with_codec(tmp_path):
    from horaedb_amd import Store
    from horaedb_amd.store import write_sst_native_bytes, CODEC_SNAPPY
    import pyarrow.parquet as pq
    d = str(tmp_path / "store")
    os.makedirs(os.path.join(d, "data"))
    rng = np.random.default_rng(12)
    s, t, vals = _rows(3000, 11, max_len=30)
    order = rng.permutation(3000)
    s, t, vals = s[order], t[order], [vals[i] for i in order]
    with Store(d) as st:
        st.set_bytes_write_codec(CODEC_SNAPPY)
        assert st.write_bytes(s, t, vals) == 1
        st.set_bytes_write_codec(0)
        assert st.write_bytes(s, t, vals) == 2
    stable = np.lexsort((t, s))
    for seq, codec in ((1, CODEC_SNAPPY), (2, 0)):
        ref = str(tmp_path / "ref.sst")
        write_sst_native_bytes(ref, s[stable], t[stable],
                               [vals[i] for i in stable], seq, codec=codec)
        with open(ref, "rb") as f, open(os.path.join(d, "data",
                                                     f"{seq}.sst"), "rb") as g:
            assert f.read() == g.read()
    md = pq.ParquetFile(os.path.join(d, "data", "1.sst")).metadata
    assert all(md.row_group(0).column(c).compression == "SNAPPY"
               for c in range(5))
    with Store(d) as st:                     # reopens as a Binary store
        assert st.schema()["columns"][2]["type"] == "binary"
        assert [c["n_rows"] for c in st.catalog()] == [3000, 3000]


def test_setter_refusals(tmp_path):
    from horaedb_amd import Store, HxError
    from horaedb_amd.store import CODEC_SNAPPY
    k = np.arange(4)
    # an unknown codec
    e = str(tmp_path / "empty")
    os.makedirs(os.path.join(e, "data"))
    with Store(e) as st:
        for bad in (2, -1):
            with pytest.raises(HxError) as ei:
                st.set_bytes_write_codec(bad)
            assert ei.value.code == INVALID
        assert _state(e, st) == ([], [])
        # the default changes nothing and is accepted anywhere
        st.set_bytes_write_codec(0)
        assert st.write(k, k, k * 1.0) == 1
    # Snappy on a store with an f64 value column
    with Store(e) as st:
        before = _state(e, st)
        with pytest.raises(HxError) as ei:
            st.set_bytes_write_codec(CODEC_SNAPPY)
        assert ei.value.code == UNSUPPORTED
        st.set_bytes_write_codec(0)
        assert st.write(k, k, k * 1.0) == 2     # the setting did not stick
        assert _state(e, st) != before
    # on an empty store it is accepted; f64 writes are then refused
    e2 = str(tmp_path / "empty2")
    os.makedirs(os.path.join(e2, "data"))
    with Store(e2) as st:
        st.set_bytes_write_codec(CODEC_SNAPPY)
        for valid in (None, np.array([True, False, True, True])):
            with pytest.raises(HxError) as ei:
                st.write(k, k, k * 1.0, valid=valid)
            assert ei.value.code == UNSUPPORTED
            assert _state(e2, st) == ([], [])
        assert st.write_bytes(k, k, [b"a", b"", b"ccc", b"dd"]) == 1
    # hx_set_write_codec keeps its refusal on a Binary store
    with Store(e2) as st:
        with pytest.raises(HxError) as ei:
            st.set_write_codec(CODEC_SNAPPY)
        assert ei.value.code == UNSUPPORTED
    # an unknown codec for the GPU-free writer: nothing written
    from horaedb_amd.store import write_sst_native_bytes
    path = str(tmp_path / "x.sst")
    with pytest.raises(HxError) as ei:
        write_sst_native_bytes(path, k, k, [b"a"] * 4, 1, codec=2)
    assert ei.value.code == INVALID and not os.path.exists(path)
