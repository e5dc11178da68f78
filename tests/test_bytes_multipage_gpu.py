# Value chunks of several data pages in Binary value stores on the device
# (DESIGN §3, §4 kernel 1h, §10, §9p): kernel 1h through
# hx_debug_ba_batch_sizes against its host twin; scans of pyarrow-written
# multi-page stores in every form against the oracle and a single-page twin;
# compaction over multi-page inputs; hx_write_bytes and both compactions under
# hx_set_bytes_page_limit, byte for byte the GPU-free writer's file.
import os
import sys

import numpy as np
import pytest

from test_append_gpu import _oracle_merge
from test_bytes_write_gpu import (_batch, _read, _files, _expected_compaction,
                                  _scan, _same_rows)
from test_bytes_multipage_cpu import (BATCH_ROW_COUNTS, BATCH_ROW_GROUPS, FORMS,
                                      MULTI, batch_row_len, chunk_pages,
                                      expected_batch_sums, letter_rows,
                                      n_data_pages)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

pytestmark = pytest.mark.gpu
ALL = (-10**15, 10**15)
SNAPPY = 1
LIMIT = 30_000


# ---- kernel 1h ------------------------------------------------------------------

@pytest.mark.parametrize("row_group", BATCH_ROW_GROUPS)
@pytest.mark.parametrize("n", BATCH_ROW_COUNTS)
def test_kernel_batch_sizes(n, row_group):
    from horaedb_amd.store import ba_batch_sizes_device, ba_batch_sizes_host
    row_len = batch_row_len(n)
    got = ba_batch_sizes_device(row_len, row_group).tolist()
    assert got == ba_batch_sizes_host(row_len, row_group).tolist()
    assert got == expected_batch_sums(row_len, row_group)


# ---- read -----------------------------------------------------------------------

def _files_rows(random_bytes=False):
    """Three files of 2500 rows over one small PK pool: every PK collides."""
    if random_bytes:
        # 300 bytes and more: such a page does not compress and is stored
        return [letter_rows(2500, 40 + k, random_bytes=True, min_len=300)
                for k in range(3)]
    return [letter_rows(2500, 40 + k) for k in range(3)]


def _store(d, files, **kw):
    from tools.gen_ssts import write_bytes_sst
    for seq, (s, t, vals) in enumerate(files, 1):
        write_bytes_sst(os.path.join(d, "data", f"{seq}.sst"), s, t, vals,
                        seq, sort=False, **kw)
    return d


@pytest.fixture(scope="module")
def letter_files():
    return _files_rows()


@pytest.fixture(scope="module")
def letter_twin(tmp_path_factory, letter_files):
    """The same rows, one data page per chunk."""
    d = str(tmp_path_factory.mktemp("twin"))
    return _store(d, letter_files, row_group=1024, data_page_size=8 << 20)


def _scans(d, ts_range):
    from horaedb_amd import Store
    out, stats = {}, None
    for mode in ("overwrite", "append"):
        with Store(d, update_mode=mode) as st:
            out[mode] = st.scan(ts_range, devices=[0])
            if stats is None:
                with st.prepare(ts_range, devices=[0]) as p:
                    stats = p.decode_stats()
    return out, stats


@pytest.fixture(scope="module")
def twin_scans(letter_twin):
    """The twin's scans and the oracle's, once for every form."""
    res = {}
    for r in (ALL, (5_000, 30_000)):
        rows, _ = _scans(letter_twin, r)
        for mode, op in (("overwrite", "last"), ("append", "append")):
            exp = _oracle_merge(letter_twin, r, op)
            np.testing.assert_array_equal(rows[mode]["series_id"], exp[0])
            np.testing.assert_array_equal(rows[mode]["timestamp"], exp[1])
            assert rows[mode]["value"].tolist() == exp[2].tolist()
        res[r] = rows
    return res


@pytest.mark.parametrize("codec,version,nullable", FORMS)
def test_scan_multi_page_store(tmp_path, letter_files, twin_scans, codec,
                               version, nullable):
    d = _store(str(tmp_path / "store"), letter_files, compression=codec,
               nullable=nullable, data_page_version=version, **MULTI)
    assert [n_data_pages(os.path.join(d, "data", "1.sst"), g, 2)
            for g in range(3)] == [4, 4, 2]
    for r in (ALL, (5_000, 30_000)):
        rows, stats = _scans(d, r)
        for mode in ("overwrite", "append"):
            # the twin's scan is the oracle's (twin_scans)
            _same_rows(rows[mode], twin_scans[r][mode])
        if r == ALL and codec == "SNAPPY" and version == "1.0":
            # a v1 page is always a Snappy stream (a v2 page that does not
            # shrink is left uncompressed): each of the 30 value pages is
            # counted as a page, read in place or decoded
            assert stats["pages_in_place"] + stats["pages_decoded"] >= 30


def _check_against_oracle_and_twin(d, twin):
    """Both ranges, both modes; returns the decode counters of the full
    range."""
    full = None
    for r in (ALL, (5_000, 30_000)):
        rows, stats = _scans(d, r)
        twin_rows, _ = _scans(twin, r)
        for mode, op in (("overwrite", "last"), ("append", "append")):
            exp = _oracle_merge(d, r, op)
            np.testing.assert_array_equal(rows[mode]["series_id"], exp[0])
            np.testing.assert_array_equal(rows[mode]["timestamp"], exp[1])
            assert rows[mode]["value"].tolist() == exp[2].tolist()
            _same_rows(rows[mode], twin_rows[mode])
        if r == ALL:
            full = stats
    return full


def _value_pages(d):
    return sum(n_data_pages(os.path.join(d, "data", f"{q}.sst"), g, 2)
               for q in (1, 2, 3) for g in range(3))


def _assert_value_pages_in_place(stats, n_value_pages, files, page_bytes,
                                 may_decode=0):
    # 18 key pages (3 files x 3 row groups x 2 columns) of at most 8192 bytes
    # each, and may_decode value pages, are all that may have been decoded
    key_pages = 18
    print("pages_in_place", stats["pages_in_place"], "pages_decoded",
          stats["pages_decoded"], "value pages", n_value_pages)
    assert stats["pages_in_place"] + stats["pages_decoded"] == \
        n_value_pages + key_pages
    assert stats["pages_decoded"] <= key_pages + may_decode
    assert stats["pages_in_place"] >= n_value_pages - may_decode
    if may_decode == 0:
        # a value page here is some page_bytes, more than all the slack the
        # short key pages leave under this bound
        assert page_bytes > 6 * (8192 - 452 * 8)
        assert stats["bytes_decoded_out"] <= stats["pages_decoded"] * 1024 * 8
        image = sum(4 + len(v) for f in files for v in f[2])
        assert stats["bytes_in_place"] >= image


@pytest.fixture(scope="module")
def random_stores(tmp_path_factory):
    """The stores above with random bytes for letters, and their one-page
    twin, scanned against the oracle and each other."""
    files = [letter_rows(2500, 40 + k, random_bytes=True) for k in range(3)]
    base = tmp_path_factory.mktemp("random")
    twin = _store(str(base / "twin"), files, row_group=1024,
                  data_page_size=8 << 20)
    d = _store(str(base / "store"), files, compression="SNAPPY", **MULTI)
    return files, d, twin


def test_scan_random_bytes_multi_page_store(random_stores):
    files, d, twin = random_stores
    assert _value_pages(d) == 30
    _check_against_oracle_and_twin(d, twin)


def test_random_bytes_value_pages_are_read_in_place(random_stores):
    """A page of these stores closes at 70 000 bytes and so holds more than
    65 536; the Snappy library behind pyarrow compresses in fragments of
    64 KiB, so an incompressible page is TWO literals and nothing else.
    Staging lays the literals' bodies end to end in the slot
    (hx_snappy_literals_only), and the page is read in place like a page of
    one stored literal."""
    from horaedb_amd import Store
    files, d, twin = random_stores
    with Store(d) as st:
        with st.prepare(ALL, devices=[0]) as p:
            stats = p.decode_stats()
    _assert_value_pages_in_place(stats, 30, files, 70_000)


def test_scan_stored_multi_page_store(tmp_path):
    # random values of 300 to 600 bytes in pages closed at 40 000 bytes, two
    # batches of 64 rows and some 58 KB: one Snappy fragment, so pyarrow's
    # stream is one literal and the page is stored
    files = _files_rows(random_bytes=True)
    twin = _store(str(tmp_path / "twin"), files, row_group=1024,
                  data_page_size=8 << 20)
    d = _store(str(tmp_path / "store"), files, compression="SNAPPY",
               row_group=1024, write_batch_size=64, data_page_size=40_000)
    n_value_pages = _value_pages(d)
    assert n_value_pages >= 3 * (8 + 8 + 4)
    stats = _check_against_oracle_and_twin(d, twin)
    # the pages the limit closed are two full batches; the last page of each
    # of the nine row groups holds whatever rows remain, and what pyarrow's
    # Snappy makes of such a remainder is not this test's business
    _assert_value_pages_in_place(stats, n_value_pages, files, 55_000,
                                 may_decode=9)


# ---- compaction -----------------------------------------------------------------

def _check_output(tmp_path, d, new_seq, exp, want_seq, mode, codec, limit):
    import oracle
    from horaedb_amd.store import write_sst_native_bytes
    out = os.path.join(d, "data", f"{new_seq}.sst")
    got = oracle.read_sst(out, with_builtins=True)
    np.testing.assert_array_equal(got.cols[0], exp[0])
    np.testing.assert_array_equal(got.cols[1], exp[1])
    assert got.cols[2].tolist() == exp[2].tolist()
    np.testing.assert_array_equal(got.cols[3], want_seq)
    ref = str(tmp_path / "ref.sst")
    write_sst_native_bytes(ref, exp[0], exp[1], exp[2].tolist(), new_seq,
                           seqs=want_seq, codec=codec, page_limit=limit)
    assert _read(ref) == _read(out)
    n_pages = len(chunk_pages(out, 0, 2))
    assert (n_pages > 1) == (limit != 0)
    after = _scan(d, mode)
    o = _oracle_merge(d, ALL, "append" if mode == "append" else "last")
    np.testing.assert_array_equal(after["series_id"], o[0])
    np.testing.assert_array_equal(after["timestamp"], o[1])
    assert after["value"].tolist() == o[2].tolist()
    return after


SETTINGS = [(0, 0), (0, LIMIT), (SNAPPY, LIMIT)]


@pytest.mark.parametrize("codec,limit", SETTINGS)
@pytest.mark.parametrize("mode", ["overwrite", "append"])
def test_compact_multi_page_inputs(tmp_path, letter_files, mode, codec,
                                   limit):
    from horaedb_amd import Store
    d = _store(str(tmp_path / "store"), letter_files, compression="SNAPPY",
               nullable=True, **MULTI)
    exp = _expected_compaction(d, [1, 2, 3], mode)
    before = _scan(d, mode)
    with Store(d, update_mode=mode) as st:
        st.set_bytes_write_codec(codec)
        st.set_bytes_page_limit(limit)
        assert st.compact(ALL, devices=[0]) == 4
        assert [c["seq"] for c in st.catalog()] == [4]
    assert [os.path.basename(p) for p in _files(d)] == ["4.sst"]
    after = _check_output(tmp_path, d, 4, exp,
                          np.full(len(exp[0]), 4, np.uint64), mode, codec,
                          limit)
    _same_rows(after, before)


@pytest.mark.parametrize("codec,limit", SETTINGS)
@pytest.mark.parametrize("mode", ["overwrite", "append"])
def test_compact_files_multi_page_inputs(tmp_path, letter_files, mode, codec,
                                         limit):
    from horaedb_amd import Store
    d = _store(str(tmp_path / "store"), letter_files, compression="ZSTD",
               data_page_version="2.0", **MULTI)
    exp = _expected_compaction(d, [1, 2], mode)
    before = _scan(d, mode)
    with Store(d, update_mode=mode) as st:
        st.set_bytes_write_codec(codec)
        st.set_bytes_page_limit(limit)
        assert st.compact_files([1, 2], devices=[0]) == 4
        assert [c["seq"] for c in st.catalog()] == [3, 4]
    after = _check_output(tmp_path, d, 4, exp, exp[3], mode, codec, limit)
    _same_rows(after, before)      # {1, 2} is seq-contiguous


# ---- ingest ---------------------------------------------------------------------

@pytest.mark.parametrize("codec", [0, SNAPPY])
def test_write_bytes_both_routes_with_limit(tmp_path, codec):
    from horaedb_amd import Store
    from horaedb_amd.store import write_sst_native_bytes
    d = str(tmp_path / "store")
    os.makedirs(os.path.join(d, "data"))
    small = _batch(3_000, 21, 200, 40, 40)      # host route
    big = _batch(70_000, 22, 200, 40, 12)       # device route (>= 64k rows)
    with Store(d) as st:
        st.set_bytes_write_codec(codec)
        st.set_bytes_page_limit(LIMIT)
        assert st.write_bytes(*small) == 1
        assert st.write_bytes(*big) == 2
    for seq, (s, t, vals) in ((1, small), (2, big)):
        order = np.lexsort((t, s))
        ref = str(tmp_path / "ref.sst")
        write_sst_native_bytes(ref, s[order], t[order],
                               [vals[i] for i in order], seq, codec=codec,
                               page_limit=LIMIT)
        out = os.path.join(d, "data", f"{seq}.sst")
        assert _read(ref) == _read(out)
        assert len(chunk_pages(out, 0, 2)) > 1
    for mode, op in (("overwrite", "last"), ("append", "append")):
        with Store(d, update_mode=mode) as st:
            rows = st.scan((0, 40_000), devices=[0])
        exp = _oracle_merge(d, (0, 40_000), op)
        np.testing.assert_array_equal(rows["series_id"], exp[0])
        np.testing.assert_array_equal(rows["timestamp"], exp[1])
        assert rows["value"].tolist() == exp[2].tolist()
