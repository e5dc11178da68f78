# Writing Snappy pages, host side (DESIGN §2 write side, §4 kernel 1e's host
# twin, §9m): hx::snappy_compress_host through its ctypes export, the writer
# under codec 1 through hx_write_sst_codec, hx_set_write_codec's argument
# checks. No GPU involved.
#
# The reference for a stream is pyarrow's Snappy: its decoder must give the
# page back, and for the key-column page classes its encoder's size is the
# yardstick (ours <= pyarrow * 1.01 + 64). The other size bars come from the
# format: never longer than the stored form {varint(n), one literal}; random
# bytes ARE the stored form; one repeated 8-byte word costs at most 4 bytes
# per 64 (n / 16 + 64).
import hashlib
import os
import subprocess

import numpy as np
import pytest

import snappy_shapes as shapes

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "horaedb_amd", "csrc")
COLS = ["series_id", "timestamp", "value", "__seq__", "__reserved__"]
UNSUPPORTED, INVALID = 3, 6


def varint(n):
    out = bytearray()
    while n >= 0x80:
        out.append((n & 0x7F) | 0x80)
        n >>= 7
    out.append(n)
    return bytes(out)


def stored_form(page):
    """{varint(n), one literal of n bytes}; n = 0 is the single byte 00."""
    n = len(page)
    if n == 0:
        return b"\0"
    m = n - 1
    if m < 60:
        tag = bytes([m << 2])
    else:
        nb = (m.bit_length() + 7) // 8
        tag = bytes([(59 + nb) << 2]) + m.to_bytes(nb, "little")
    return varint(n) + tag + page


@pytest.fixture(scope="module")
def streams():
    from horaedb_amd.store import snappy_compress_host
    return [(name, page, snappy_compress_host(page))
            for name, page in shapes.shape_pages()]


def test_check_program(tmp_path):
    pages = tmp_path / "pages.bin"
    shapes.dump(str(pages), shapes.shape_pages())
    b = subprocess.run(["make", "-C", CSRC, "snappy_compress_check"],
                       capture_output=True, text=True)
    assert b.returncode == 0, b.stdout + b.stderr
    r = subprocess.run([os.path.join(CSRC, "snappy_compress_check"),
                        str(pages)], capture_output=True, text=True)
    print(b.stdout + r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == "ALL OK"
    assert len(lines) > len(shapes.shape_pages())
    assert not any(ln.endswith("FAIL") for ln in lines)


def test_round_trip_through_pyarrow(streams):
    import pyarrow as pa
    for name, page, stream in streams:
        assert stream is not None, name
        back = pa.decompress(stream, decompressed_size=len(page),
                             codec="snappy", asbytes=True) if page else b""
        assert back == page, name
        assert len(stream) <= len(stored_form(page)), name
        assert len(stream) <= 32 + len(page) + len(page) // 6, name


def test_shapes_hold_the_intended_elements(streams):
    # the constructed shapes are there for particular element forms: every
    # literal length form in front of a match, every copy split at a 1-byte
    # and a 2-byte offset, the offset limit. Parse the twin's streams so the
    # shapes stay pinned to them.
    pins = shapes.pinned_elements()
    by_name = {name: (page, stream) for name, page, stream in streams}
    assert set(pins) <= set(by_name)
    seen = set()
    for name, check in pins.items():
        page, stream = by_name[name]
        ulen, elements = shapes.parse(stream)
        assert ulen == len(page), name
        check(elements)
        seen |= {(e[2], e[3]) for e in elements if e[0] == "C" and e[1] > 64}
    # copy pieces emitted at a far offset, by (length, tag form)
    for piece in [(4, 1), (4, 2), (11, 1), (11, 2), (12, 2), (64, 2),
                  (60, 2), (5, 1), (5, 2), (7, 1), (7, 2)]:
        assert piece in seen, piece


def test_short_slot_is_refused(streams):
    from horaedb_amd.store import snappy_compress_host, snappy_max_compressed
    for name, page, _ in streams[:40]:
        # the wrapper raises if a refused call wrote anything
        assert snappy_compress_host(
            page, cap=snappy_max_compressed(len(page)) - 1) is None, name


def test_random_pages_are_the_stored_form():
    from horaedb_amd.store import snappy_compress_host
    rng = np.random.default_rng(5)
    for n in (1, 59, 60, 61, 255, 256, 257, 4096, 65536, 65544, 70000):
        page = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        assert snappy_compress_host(page) == stored_form(page), n
    assert snappy_compress_host(b"") == b"\0"


def test_repeated_word_bar():
    from horaedb_amd.store import snappy_compress_host
    rng = np.random.default_rng(6)
    for n in (128, 129, 1000, 4095, 65536, 65544, 200000, 1 << 20):
        word = rng.integers(0, 256, 8, dtype=np.uint8).tobytes()
        page = (word * (n // 8 + 1))[:n]
        size = len(snappy_compress_host(page))
        print(f"repeated word n={n}: {size} (bar {n // 16 + 64})")
        assert size <= n // 16 + 64, n


def test_offset_limit(streams):
    by_name = {name: (page, stream) for name, page, stream in streams}
    size = {d: len(by_name[f"distance{d}"][1]) for d in shapes.DISTANCES}
    # 65535 is a copy; one byte further the 32-byte block goes out again
    assert size[65536] >= size[65535] + 28
    assert size[65537] >= size[65535] + 28


def test_size_against_reference_encoder():
    import pyarrow as pa
    from horaedb_amd.store import snappy_compress_host
    rows = []
    for name, page, kind in shapes.metric_pages():
        ours = len(snappy_compress_host(page))
        ref = len(pa.compress(page, codec="snappy", asbytes=True))
        rows.append((name, kind, ref, ours))
        print(f"{name:14s} pyarrow={ref:6d} ours={ours:6d} "
              f"ratio={ours / ref:.3f}")
    for name, kind, ref, ours in rows:
        assert ours <= len(stored_form(b"\0" * 65536)), name
        if kind == "keys":
            assert ours <= ref * 1.01 + 64, (name, ref, ours)


# ---- files ------------------------------------------------------------------

def rows_of(n, rng):
    series = np.repeat(np.sort(rng.integers(0, 1 << 62, (n + 1) // 2,
                                            dtype=np.uint64)), 2)[:n]
    ts = (np.arange(n, dtype=np.int64) % 2) * 1000 - 5000
    return series, ts, rng.standard_normal(n)


FORMS = [("required", False, None, 3 * 8192),
         ("optional_no_nulls", True, 0.0, 3 * 8192),
         ("optional_nulls30", True, 0.3, 3 * 8192),
         ("short_last_group", True, 0.3, 2 * 8192 + 77)]


@pytest.mark.parametrize("form", FORMS, ids=[f[0] for f in FORMS])
def test_codec1_file(tmp_path, form):
    import pyarrow.parquet as pq
    from horaedb_amd.store import (CODEC_SNAPPY, page_levels,
                                   write_sst_native_codec)
    _, nullable, null_frac, n = form
    rng = np.random.default_rng(n + int(nullable))
    series, ts, value = rows_of(n, rng)
    valid = None if null_frac is None else rng.random(n) >= null_frac
    path = str(tmp_path / "1.sst")
    write_sst_native_codec(path, series, ts, value, 9, CODEC_SNAPPY,
                           valid=valid, nullable=nullable)
    pf = pq.ParquetFile(path)
    assert [f.name for f in pf.schema_arrow] == COLS
    assert pf.schema_arrow.field("value").nullable == nullable
    tbl = pf.read()
    np.testing.assert_array_equal(tbl["series_id"].to_numpy(), series)
    np.testing.assert_array_equal(tbl["timestamp"].to_numpy(), ts)
    assert tbl["__seq__"].to_numpy().tolist() == [9] * n
    assert not tbl["__reserved__"].to_numpy().any()
    col = tbl["value"].combine_chunks()
    want_valid = np.ones(n, dtype=bool) if valid is None else valid
    np.testing.assert_array_equal(
        col.is_valid().to_numpy(zero_copy_only=False), want_valid)
    np.testing.assert_array_equal(
        col.drop_null().to_numpy(zero_copy_only=False).view(np.uint64),
        value[want_valid].view(np.uint64))
    md = pf.metadata
    assert md.num_row_groups == (n + 8191) // 8192
    for g in range(md.num_row_groups):
        lo, hi = g * 8192, min(n, (g + 1) * 8192)
        for c in range(5):
            cm = md.row_group(g).column(c)
            assert cm.compression == "SNAPPY"
            assert cm.total_compressed_size <= cm.total_uncompressed_size + 8
        # key columns shrink; the real sizes are in the footer
        assert (md.row_group(g).column(4).total_compressed_size <
                md.row_group(g).column(4).total_uncompressed_size // 10)
        # the project's own footer and page parser
        bits, n_valid, lvl = page_levels(path, g, "value")
        np.testing.assert_array_equal(bits, want_valid[lo:hi])
        assert n_valid == int(want_valid[lo:hi].sum())
        assert (lvl > 0) == nullable
        for column in ("series_id", "timestamp", "__seq__"):
            bits, n_valid, lvl = page_levels(path, g, column)
            assert bits.all() and n_valid == hi - lo and lvl == 0


def sha(path):
    with open(path, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()


def test_codec0_is_the_file_written_before(tmp_path):
    from horaedb_amd.store import (CODEC_NONE, write_sst_native,
                                   write_sst_native_codec,
                                   write_sst_native_nullable)
    rng = np.random.default_rng(3)
    n = 8192 + 500
    series, ts, value = rows_of(n, rng)
    valid = rng.random(n) >= 0.3
    a, b = str(tmp_path / "a.sst"), str(tmp_path / "b.sst")
    write_sst_native(a, series, ts, value, 5)
    write_sst_native_codec(b, series, ts, value, 5, CODEC_NONE)
    assert sha(a) == sha(b)
    write_sst_native_nullable(a, series, ts, value, 5, valid=valid)
    write_sst_native_codec(b, series, ts, value, 5, CODEC_NONE, valid=valid,
                           nullable=True)
    assert sha(a) == sha(b)
    write_sst_native_nullable(a, series, ts, value, 5, row_group=128)
    write_sst_native_codec(b, series, ts, value, 5, CODEC_NONE, nullable=True,
                           row_group=128)
    assert sha(a) == sha(b)


def test_bad_arguments(tmp_path):
    from horaedb_amd import HxError
    from horaedb_amd.store import write_sst_native_codec
    path = str(tmp_path / "1.sst")
    for kwargs in (dict(codec=2), dict(codec=-1),
                   dict(codec=1, valid=[True, False])):   # REQUIRED + validity
        with pytest.raises(HxError) as ei:
            write_sst_native_codec(path, [1, 2], [1, 2], [1.0, 2.0], 1,
                                   **kwargs)
        assert ei.value.code == INVALID
        assert not os.path.exists(path)


def test_set_write_codec_argument_checks(tmp_path):
    from horaedb_amd import HxError, Store
    from horaedb_amd.store import CODEC_NONE, CODEC_SNAPPY
    os.makedirs(tmp_path / "data")
    with Store(str(tmp_path)) as st:
        st.set_write_codec(CODEC_SNAPPY)
        st.set_nullable_values(True)
        st.set_write_codec(CODEC_NONE)
        for bad in (2, -1, 7):
            with pytest.raises(HxError) as ei:
                st.set_write_codec(bad)
            assert ei.value.code == INVALID


@pytest.mark.parametrize("nullable", [False, True])
def test_host_ingest_route_writes_the_same_file(tmp_path, nullable):
    # hx_write of a small batch sorts on the host and compresses with the
    # twin: the file is hx_write_sst_codec's for the sorted rows
    from horaedb_amd import Store
    from horaedb_amd.store import CODEC_SNAPPY, write_sst_native_codec
    rng = np.random.default_rng(11)
    n = 1000
    series = rng.integers(1, 300, n, dtype=np.uint64)
    ts = rng.integers(0, 4, n).astype(np.int64) * 1000
    value = rng.standard_normal(n)
    valid = rng.random(n) >= 0.3 if nullable else None
    (tmp_path / "s" / "data").mkdir(parents=True)
    with Store(str(tmp_path / "s")) as st:
        st.set_write_codec(CODEC_SNAPPY)
        st.set_nullable_values(nullable)
        seq = st.write(series, ts, value, valid=valid)
        assert st.catalog()[0]["n_rows"] == n
    order = np.lexsort((ts, series))
    want = str(tmp_path / "want.sst")
    write_sst_native_codec(want, series[order], ts[order], value[order], seq,
                           CODEC_SNAPPY, nullable=nullable,
                           valid=None if valid is None else valid[order])
    assert sha(str(tmp_path / "s" / "data" / f"{seq}.sst")) == sha(want)


def test_binary_value_store_is_unsupported(tmp_path):
    import sys
    sys.path.insert(0, REPO)
    from tools.gen_ssts import write_bytes_sst
    from horaedb_amd import HxError, Store
    d = str(tmp_path / "store")
    write_bytes_sst(os.path.join(d, "data", "1.sst"), [1, 2], [0, 0],
                    [b"a", b"bc"], 1)
    with Store(d) as st:
        with pytest.raises(HxError) as ei:
            st.set_write_codec(1)
        assert ei.value.code == UNSUPPORTED
        st.set_write_codec(0)            # changes nothing: accepted
