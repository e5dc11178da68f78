# Snappy pages for Binary value stores on the device (DESIGN §2, §3 the
# blob's decoded tail, §4 kernel 1g, §9o): kernel 1g through
# hx_debug_ba_page_minmax against its host twin and Python's min()/max();
# scans of pyarrow-written Snappy Binary stores against the oracle and against
# their uncompressed twins; hx_write_bytes and both compactions under
# hx_set_bytes_write_codec(SNAPPY), byte for byte the GPU-free writer's file.
import os
import sys

import numpy as np
import pytest

import ba_minmax_shapes as mm
from test_append_gpu import _oracle_merge
from test_bytes_write_gpu import (_batch, _read, _files, _expected_compaction,
                                  _scan, _same_rows)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

pytestmark = pytest.mark.gpu
ALL = (-10**15, 10**15)
SNAPPY = 1
FORMS = [("1.0", False), ("1.0", True), ("2.0", False), ("2.0", True)]


# ---- kernel 1g --------------------------------------------------------------

@pytest.mark.parametrize("case", mm.cases(), ids=lambda c: c[0])
def test_kernel_minmax(case):
    from horaedb_amd.store import ba_page_minmax_device, ba_page_minmax_host
    _, vals, row_group, skip = case
    got = ba_page_minmax_device(vals, row_group, skip)
    assert got == ba_page_minmax_host(vals, row_group, skip)
    assert got == mm.expected(vals, row_group, skip)


# ---- read -------------------------------------------------------------------

def _rand_rows(n_files=3, n_rows=3000, n_series=80):
    """The rows of test_append_gpu's store (every PK collides)."""
    rng = np.random.default_rng(8)
    pool = np.sort(rng.integers(0, 2**63, n_series, dtype=np.uint64))
    files = []
    for _ in range(n_files):
        s = rng.choice(pool, size=n_rows)
        t = rng.integers(0, 40, n_rows) * 1000
        vals = [bytes(rng.integers(65, 90, rng.integers(1, 9)).astype(
            np.uint8).tolist()) for _ in range(n_rows)]
        files.append((s, t, vals))
    return files


def _store(tmp_path, name, files, **kw):
    from tools.gen_ssts import write_bytes_sst
    d = str(tmp_path / name)
    for seq, (s, t, vals) in enumerate(files, 1):
        write_bytes_sst(os.path.join(d, "data", f"{seq}.sst"), s, t, vals,
                        seq, **kw)
    return d


def _check_scans(d, twin=None, ts_range=ALL):
    """Both modes against the oracle (and the uncompressed twin's scan);
    returns the decode counters of the Overwrite plan."""
    from horaedb_amd import Store
    stats = None
    for mode, op in (("overwrite", "last"), ("append", "append")):
        with Store(d, update_mode=mode) as st:
            rows = st.scan(ts_range, devices=[0])
            if stats is None:
                with st.prepare(ts_range, devices=[0]) as p:
                    stats = p.decode_stats()
        exp = _oracle_merge(d, ts_range, op)
        np.testing.assert_array_equal(rows["series_id"], exp[0])
        np.testing.assert_array_equal(rows["timestamp"], exp[1])
        assert rows["value"].tolist() == exp[2].tolist()
        if twin is not None:
            with Store(twin, update_mode=mode) as st:
                _same_rows(rows, st.scan(ts_range, devices=[0]))
    return stats


@pytest.mark.parametrize("version,nullable", FORMS)
def test_scan_pyarrow_snappy_store(tmp_path, version, nullable):
    files = _rand_rows()
    twin = _store(tmp_path, "plain", files)
    d = _store(tmp_path, "snappy", files, compression="SNAPPY",
               nullable=nullable, data_page_version=version)
    stats = _check_scans(d, twin)
    # the three value pages are not stored literals (letters compress): they
    # were decoded, whatever became of the six key pages
    image = [sum(4 + len(v) for v in f[2]) for f in files]
    assert stats["pages_decoded"] >= 3
    key_pages = stats["pages_decoded"] - 3
    lvl = stats["bytes_decoded_out"] - sum(image) - key_pages * 3000 * 8
    # v1 nullable pages carry their level block inside the stream: a few
    # bytes per page, nothing otherwise
    if nullable and version == "1.0":
        assert 0 < lvl <= 9 * 16
    else:
        assert lvl == 0
    _check_scans(d, twin, (5_000, 30_000))


def test_scan_row_group_edge(tmp_path):
    # 20 000 rows: three row groups, the last short
    rng = np.random.default_rng(5)
    n = 20_000
    s = rng.integers(0, 500, n).astype(np.uint64)
    t = rng.integers(0, 40, n).astype(np.int64) * 1000
    vals = [b"v%d-" % (i % 97) + bytes([65 + i % 26]) * (i % 13)
            for i in range(n)]
    files = [(s, t, vals)]
    twin = _store(tmp_path, "plain", files)
    d = _store(tmp_path, "snappy", files, compression="SNAPPY",
               nullable=True)
    stats = _check_scans(d, twin)
    assert stats["pages_decoded"] >= 3


def _mixed_lengths():
    """Values of 0, 1, 4095, 4096, 4097 and 70 000 bytes; the long ones hold
    one 3000-byte block again at distances 2049, 4097 and 60 000."""
    rng = np.random.default_rng(17)

    def rnd(n):
        return bytes(rng.integers(0, 256, n, dtype=np.uint8).tolist())

    period = rnd(2049)
    region = (period * 3)[:2049 + 3000]     # block again 2049 further on
    block = region[2049:]
    assert block == region[:3000]
    big = region + rnd(1097) + block        # 4097 behind the last start
    assert big[2049:5049] == big[6146:9146]
    big += rnd(57_000) + block              # 60 000 behind the last start
    assert big[6146:9146] == big[66146:69146]
    big += rnd(70_000 - len(big))
    lens = [0, 1, 4095, 4096, 4097]
    vals = []
    for i in range(40):
        k = lens[i % 5]
        vals.append(block[:k] if k <= 3000 else block + rnd(k - 3000))
    vals[7] = big
    vals[23] = big[:30_000] + big[:40_000]
    return vals


def test_scan_mixed_lengths_one_large_page(tmp_path):
    vals = _mixed_lengths()
    n = len(vals)
    assert {len(v) for v in vals} == {0, 1, 4095, 4096, 4097, 70_000}
    s = np.arange(n, dtype=np.uint64) // 2
    t = (np.arange(n, dtype=np.int64) % 2) * 1000
    files = [(s, t, vals), (s[:10], t[:10], [b"x" * i for i in range(10)])]
    twin = _store(tmp_path, "plain", files, data_page_size=8 << 20)
    d = _store(tmp_path, "snappy", files, compression="SNAPPY",
               data_page_size=8 << 20)
    stats = _check_scans(d, twin)
    image = sum(4 + len(v) for v in vals)
    assert stats["bytes_decoded_out"] >= image


def test_scan_mixed_codecs_in_one_store(tmp_path):
    from tools.gen_ssts import write_bytes_sst
    files = _rand_rows()
    twin = _store(tmp_path, "plain", files)
    d = str(tmp_path / "mixed")
    for seq, comp in ((1, "NONE"), (2, "SNAPPY"), (3, "ZSTD")):
        s, t, vals = files[seq - 1]
        write_bytes_sst(os.path.join(d, "data", f"{seq}.sst"), s, t, vals,
                        seq, compression=comp)
    stats = _check_scans(d, twin)
    assert stats["pages_decoded"] >= 1


def test_own_writer_random_values_are_read_in_place(tmp_path):
    # random bytes do not compress: our writer stores the value page, and
    # staging reads it in place; nothing of it is decoded. (300-byte values:
    # the only repeat in the page is the length prefix; a 2-byte copy for it
    # behind the 3-byte tag of a 300-byte literal loses to the stored form.
    # Up to 256 bytes a value the tags are shorter and the copies still win
    # a few bytes a page, so such a page is decoded.)
    from horaedb_amd import Store
    from horaedb_amd.store import write_sst_native_bytes
    rng = np.random.default_rng(2)
    n = 3000
    s = np.sort(rng.integers(0, 100, n)).astype(np.uint64)
    t = np.arange(n, dtype=np.int64)
    vals = [bytes(rng.integers(0, 256, 300, dtype=np.uint8).tolist())
            for _ in range(n)]
    d = str(tmp_path / "store")
    os.makedirs(os.path.join(d, "data"))
    write_sst_native_bytes(os.path.join(d, "data", "1.sst"), s, t, vals, 1,
                           codec=SNAPPY)
    image = sum(4 + len(v) for v in vals)
    with Store(d) as st:
        with st.prepare(ALL, devices=[0]) as p:
            stats = p.decode_stats()
        rows = st.scan(ALL, devices=[0])
    assert stats["pages_in_place"] + stats["pages_decoded"] == 3
    assert stats["pages_in_place"] >= 1
    assert stats["bytes_in_place"] == \
        image + (stats["pages_in_place"] - 1) * n * 8
    assert stats["bytes_decoded_out"] == stats["pages_decoded"] * n * 8
    np.testing.assert_array_equal(rows["series_id"], s)
    assert rows["value"].tolist() == vals


# ---- write ------------------------------------------------------------------

def test_write_bytes_both_routes_with_codec(tmp_path):
    from horaedb_amd import Store
    from horaedb_amd.store import write_sst_native_bytes
    import pyarrow.parquet as pq
    d = str(tmp_path / "store")
    os.makedirs(os.path.join(d, "data"))
    small = _batch(3_000, 21, 200, 40, 40)      # host route
    big = _batch(70_000, 22, 200, 40, 12)       # device route (>= 64k rows)
    with Store(d) as st:
        st.set_bytes_write_codec(SNAPPY)
        assert st.write_bytes(*small) == 1
        assert st.write_bytes(*big) == 2
        assert [c["n_rows"] for c in st.catalog()] == [3_000, 70_000]
    for seq, (s, t, vals) in ((1, small), (2, big)):
        order = np.lexsort((t, s))
        ref = str(tmp_path / "ref.sst")
        write_sst_native_bytes(ref, s[order], t[order],
                               [vals[i] for i in order], seq, codec=SNAPPY)
        out = os.path.join(d, "data", f"{seq}.sst")
        assert _read(ref) == _read(out)
        md = pq.ParquetFile(out).metadata
        assert all(md.row_group(g).column(c).compression == "SNAPPY"
                   for g in range(md.num_row_groups) for c in range(5))
    _check_scans(d, ts_range=(0, 40_000))


# ---- compaction -------------------------------------------------------------

def _compaction_store(tmp_path, compression):
    """test_bytes_write_gpu's compaction store (3 x 3 000 rows where every PK
    collides, plus 65 rows of one PK), the inputs in the given codec."""
    files = _rand_rows()
    order = np.lexsort((files[0][1], files[0][0]))
    s0, t0 = files[0][0][order][1500], files[0][1][order][1500]
    rng = np.random.default_rng(9)
    vals = [bytes(rng.integers(97, 123, rng.integers(0, 9)).astype(
        np.uint8).tolist()) for _ in range(65)]
    files.append((np.full(65, s0), np.full(65, t0), vals))
    return _store(tmp_path, "store", files, compression=compression,
                  nullable=compression == "SNAPPY")


def _check_output(tmp_path, d, new_seq, exp, want_seq, mode, codec):
    import oracle
    from horaedb_amd.store import write_sst_native_bytes
    import pyarrow.parquet as pq
    out = os.path.join(d, "data", f"{new_seq}.sst")
    got = oracle.read_sst(out, with_builtins=True)
    np.testing.assert_array_equal(got.cols[0], exp[0])
    np.testing.assert_array_equal(got.cols[1], exp[1])
    assert got.cols[2].tolist() == exp[2].tolist()
    np.testing.assert_array_equal(got.cols[3], want_seq)
    assert not got.cols[4].any()
    ref = str(tmp_path / "ref.sst")
    write_sst_native_bytes(ref, exp[0], exp[1], exp[2].tolist(), new_seq,
                           seqs=want_seq, codec=codec)
    assert _read(ref) == _read(out)
    md = pq.ParquetFile(out).metadata
    want = "SNAPPY" if codec else "UNCOMPRESSED"
    assert all(md.row_group(g).column(c).compression == want
               for g in range(md.num_row_groups) for c in range(5))
    after = _scan(d, mode)
    o = _oracle_merge(d, ALL, "append" if mode == "append" else "last")
    np.testing.assert_array_equal(after["series_id"], o[0])
    np.testing.assert_array_equal(after["timestamp"], o[1])
    assert after["value"].tolist() == o[2].tolist()
    return after


@pytest.mark.parametrize("inputs", ["NONE", "SNAPPY"])
@pytest.mark.parametrize("mode", ["overwrite", "append"])
def test_compact_closure_with_codec(tmp_path, mode, inputs):
    from horaedb_amd import Store
    d = _compaction_store(tmp_path, inputs)
    exp = _expected_compaction(d, [1, 2, 3, 4], mode)
    before = _scan(d, mode)
    with Store(d, update_mode=mode) as st:
        st.set_bytes_write_codec(SNAPPY)
        assert st.compact(ALL, devices=[0]) == 5
        assert [c["seq"] for c in st.catalog()] == [5]
        assert st.catalog()[0]["n_rows"] == len(exp[0])
    assert [os.path.basename(p) for p in _files(d)] == ["5.sst"]
    after = _check_output(tmp_path, d, 5, exp,
                          np.full(len(exp[0]), 5, np.uint64), mode, SNAPPY)
    _same_rows(after, before)


@pytest.mark.parametrize("inputs", ["NONE", "SNAPPY"])
@pytest.mark.parametrize("mode", ["overwrite", "append"])
def test_compact_files_partial_set_with_codec(tmp_path, mode, inputs):
    from horaedb_amd import Store
    d = _compaction_store(tmp_path, inputs)
    exp = _expected_compaction(d, [1, 2], mode)
    before = _scan(d, mode)
    with Store(d, update_mode=mode) as st:
        st.set_bytes_write_codec(SNAPPY)
        assert st.compact_files([1, 2], devices=[0]) == 5
        assert [c["seq"] for c in st.catalog()] == [3, 4, 5]
    assert [os.path.basename(p) for p in _files(d)] == \
        ["3.sst", "4.sst", "5.sst"]
    if mode == "append":
        assert set(np.unique(exp[3]).tolist()) == {1, 2}
    after = _check_output(tmp_path, d, 5, exp, exp[3], mode, SNAPPY)
    _same_rows(after, before)      # {1, 2} is seq-contiguous


@pytest.mark.parametrize("inputs", ["NONE", "SNAPPY"])
def test_append_compaction_of_one_pk_group_with_codec(tmp_path, inputs):
    # 65 rows of one PK in one file, 300 in another: one output row
    from horaedb_amd import Store
    rng = np.random.default_rng(3)
    files = []
    for n in (65, 300):
        vals = [bytes(rng.integers(97, 123, rng.integers(0, 200)).astype(
            np.uint8).tolist()) for _ in range(n)]
        files.append((np.full(n, 77), np.full(n, 5000), vals))
    d = _store(tmp_path, "store", files, compression=inputs)
    exp = _expected_compaction(d, [1, 2], "append")
    assert len(exp[0]) == 1
    with Store(d, update_mode="append") as st:
        st.set_bytes_write_codec(SNAPPY)
        assert st.compact_files([1, 2], devices=[0]) == 3
    _check_output(tmp_path, d, 3, exp, exp[3], "append", SNAPPY)


@pytest.mark.parametrize("mode", ["overwrite", "append"])
def test_codec_off_writes_the_old_file(tmp_path, mode):
    # the default setting over Snappy inputs: the output is the file the
    # writer wrote before there was a codec
    from horaedb_amd import Store
    d = _compaction_store(tmp_path, "SNAPPY")
    exp = _expected_compaction(d, [1, 2, 3, 4], mode)
    with Store(d, update_mode=mode) as st:
        assert st.compact(ALL, devices=[0]) == 5
    _check_output(tmp_path, d, 5, exp, np.full(len(exp[0]), 5, np.uint64),
                  mode, 0)
