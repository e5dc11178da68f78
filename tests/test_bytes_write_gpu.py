# Writing and compacting Binary value stores on the device (DESIGN §2 write
# side, §4 kernel 1f, §5 Append compaction, §9n): kernel 1f through
# hx_debug_ba_pages byte-exact against the page's definition; hx_write_bytes
# on both routes; hx_compact / hx_compact_files in both update modes against
# oracle.scan.merge_scan(keep_builtin=True); the refusals.
import glob
import os
import sys

import numpy as np
import pytest

import ba_shapes as shapes
from test_append_gpu import _rand_bytes_store, _oracle_merge

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

pytestmark = pytest.mark.gpu
UNSUPPORTED = 3
ALL = (-10**15, 10**15)


# ---- kernel 1f --------------------------------------------------------------

def test_kernel_every_length_at_every_alignment():
    from horaedb_amd.store import ba_pages_device
    src, handles = shapes.lens_by_alignment()
    pages, errs, over = ba_pages_device(src, handles)
    assert (errs, over) == (0, 0)
    assert pages == shapes.expected_pages(src, handles)


@pytest.mark.parametrize("n", shapes.ROW_COUNTS)
def test_kernel_row_counts(n):
    from horaedb_amd.store import ba_pages_device
    src, handles = shapes.rows_case(n)
    pages, errs, over = ba_pages_device(src, handles)
    assert (errs, over) == (0, 0)
    assert len(pages) == (n + 8191) // 8192
    assert pages == shapes.expected_pages(src, handles)


def test_kernel_groups():
    from horaedb_amd.store import ba_pages_device
    src, handles, gs = shapes.groups_case()
    pages, errs, over = ba_pages_device(src, handles, group_start=gs)
    assert (errs, over) == (0, 0)
    assert len(pages) == 2
    assert pages == shapes.expected_pages(src, handles, gs)


def test_kernel_refusals_touch_nothing_else():
    # the device buffers are exactly as large as the arrays: a refused row
    # is an empty value, every other row is intact, the counts are exact
    from horaedb_amd.store import ba_pages_device
    src, handles = shapes.rows_case(65)
    bad = handles.copy()
    bad[7] = (np.uint64(len(src) - 2) << np.uint64(20)) | np.uint64(3)
    pages, errs, over = ba_pages_device(src, bad)
    assert (errs, over) == (1, 0)
    assert pages == shapes.expected_pages(src, bad, refused={7})
    gs = np.array([0, 10, 8, 30, 66], dtype=np.uint32)
    pages, errs, over = ba_pages_device(src, handles, group_start=gs)
    assert (errs, over) == (2, 0)
    assert pages == shapes.expected_pages(src, handles, gs, refused={1, 3})
    src2, h2 = shapes.make_source([1 << 19, 1 << 19, 5], 3)
    gs2 = np.array([0, 2, 3], dtype=np.uint32)
    pages, errs, over = ba_pages_device(src2, h2, group_start=gs2)
    assert (errs, over) == (0, 1)
    assert pages == shapes.expected_pages(src2, h2, gs2, refused={0})


# ---- ingest -----------------------------------------------------------------

def _batch(n, seed, n_series, n_ts, max_len):
    rng = np.random.default_rng(seed)
    pool = np.sort(rng.integers(0, 2**63, n_series, dtype=np.uint64))
    s = rng.choice(pool, size=n)
    t = rng.integers(0, n_ts, n).astype(np.int64) * 1000
    lens = rng.integers(0, max_len + 1, n)
    blob = rng.integers(65, 91, int(lens.sum()), dtype=np.uint8).tobytes()
    ends = np.cumsum(lens)
    vals = [blob[e - k:e] for e, k in zip(ends.tolist(), lens.tolist())]
    return s, t, vals


def _read(path):
    with open(path, "rb") as f:
        return f.read()


def test_write_bytes_both_routes_scan_back(tmp_path):
    from horaedb_amd import Store
    from horaedb_amd.store import write_sst_native_bytes
    d = str(tmp_path / "store")
    os.makedirs(os.path.join(d, "data"))
    small = _batch(3_000, 21, 200, 40, 40)      # host route
    big = _batch(70_000, 22, 200, 40, 12)       # device route (>= 64k rows)
    with Store(d) as st:
        assert st.write_bytes(*small) == 1
        assert st.write_bytes(*big) == 2
        assert [c["n_rows"] for c in st.catalog()] == [3_000, 70_000]
    # each file is the GPU-free writer's file of the stably sorted rows
    for seq, (s, t, vals) in ((1, small), (2, big)):
        order = np.lexsort((t, s))
        ref = str(tmp_path / "ref.sst")
        write_sst_native_bytes(ref, s[order], t[order],
                               [vals[i] for i in order], seq)
        assert _read(ref) == _read(os.path.join(d, "data", f"{seq}.sst"))
    for mode, op in (("overwrite", "last"), ("append", "append")):
        with Store(d, update_mode=mode) as st:
            rows = st.scan((0, 40_000), devices=[0])
        exp = _oracle_merge(d, (0, 40_000), op)
        np.testing.assert_array_equal(rows["series_id"], exp[0])
        np.testing.assert_array_equal(rows["timestamp"], exp[1])
        assert rows["value"].tolist() == exp[2].tolist()


# ---- compaction -------------------------------------------------------------

def _compaction_store(tmp_path):
    """test_append_gpu's 3 x 3 000-row store (every PK collides) plus file 4:
    65 rows of one PK."""
    from tools.gen_ssts import write_bytes_sst
    import oracle
    d = _rand_bytes_store(tmp_path)
    first = oracle.read_sst(os.path.join(d, "data", "1.sst"))
    s0, t0 = first.cols[0][1500], first.cols[1][1500]
    rng = np.random.default_rng(9)
    vals = [bytes(rng.integers(97, 123, rng.integers(0, 9)).astype(
        np.uint8).tolist()) for _ in range(65)]
    write_bytes_sst(os.path.join(d, "data", "4.sst"), np.full(65, s0),
                    np.full(65, t0), vals, 4)
    return d


def _files(d):
    return sorted(glob.glob(os.path.join(d, "data", "*.sst")),
                  key=lambda p: int(os.path.basename(p)[:-4]))


def _expected_compaction(d, seqs, mode):
    import oracle
    from oracle.scan import merge_scan, MERGE_APPEND, MERGE_LAST
    inputs = [oracle.read_sst(os.path.join(d, "data", f"{q}.sst"))
              for q in seqs]
    return merge_scan(inputs, num_primary_keys=2,
                      merge_op=MERGE_APPEND if mode == "append"
                      else MERGE_LAST, value_idxes=[2], keep_builtin=True)


def _scan(d, mode):
    from horaedb_amd import Store
    with Store(d, update_mode=mode) as st:
        return st.scan(ALL, devices=[0])


def _same_rows(a, b):
    np.testing.assert_array_equal(a["series_id"], b["series_id"])
    np.testing.assert_array_equal(a["timestamp"], b["timestamp"])
    assert a["value"].tolist() == b["value"].tolist()


def _check_output(tmp_path, d, new_seq, exp, want_seq, mode):
    import oracle
    from horaedb_amd.store import write_sst_native_bytes
    out = os.path.join(d, "data", f"{new_seq}.sst")
    got = oracle.read_sst(out, with_builtins=True)
    np.testing.assert_array_equal(got.cols[0], exp[0])
    np.testing.assert_array_equal(got.cols[1], exp[1])
    assert got.cols[2].tolist() == exp[2].tolist()
    np.testing.assert_array_equal(got.cols[3], want_seq)
    assert not got.cols[4].any()
    ref = str(tmp_path / "ref.sst")
    write_sst_native_bytes(ref, exp[0], exp[1], exp[2].tolist(), new_seq,
                           seqs=want_seq)
    assert _read(ref) == _read(out)
    # the scan over the new file set is the oracle's
    after = _scan(d, mode)
    o = _oracle_merge(d, ALL, "append" if mode == "append" else "last")
    np.testing.assert_array_equal(after["series_id"], o[0])
    np.testing.assert_array_equal(after["timestamp"], o[1])
    assert after["value"].tolist() == o[2].tolist()
    return after


@pytest.mark.parametrize("mode", ["overwrite", "append"])
def test_compact_closure(tmp_path, mode):
    from horaedb_amd import Store
    d = _compaction_store(tmp_path)
    exp = _expected_compaction(d, [1, 2, 3, 4], mode)
    before = _scan(d, mode)
    with Store(d, update_mode=mode) as st:
        new_seq = st.compact(ALL, devices=[0])
        assert new_seq == 5
        assert [c["seq"] for c in st.catalog()] == [5]
        assert st.catalog()[0]["n_rows"] == len(exp[0])
    assert [os.path.basename(p) for p in _files(d)] == ["5.sst"]
    # hx_compact: the rows carry the new file's sequence
    after = _check_output(tmp_path, d, 5, exp,
                          np.full(len(exp[0]), 5, np.uint64), mode)
    _same_rows(after, before)
    # one row per distinct PK in either mode; the 65-row PK among them
    pk = np.stack([exp[0].astype(np.int64), exp[1]], axis=1)
    assert len(np.unique(pk, axis=0)) == len(pk)


@pytest.mark.parametrize("mode", ["overwrite", "append"])
def test_compact_files_partial_set(tmp_path, mode):
    from horaedb_amd import Store
    d = _compaction_store(tmp_path)
    exp = _expected_compaction(d, [1, 2], mode)
    before = _scan(d, mode)
    with Store(d, update_mode=mode) as st:
        new_seq = st.compact_files([1, 2], devices=[0])
        assert new_seq == 5
        assert [c["seq"] for c in st.catalog()] == [3, 4, 5]
    assert [os.path.basename(p) for p in _files(d)] == \
        ["3.sst", "4.sst", "5.sst"]
    # hx_compact_files: Overwrite keeps the winner's sequence, Append the
    # sequence of the group's first row (merge_scan's out_seq)
    if mode == "append":
        assert set(np.unique(exp[3]).tolist()) == {1, 2}
    after = _check_output(tmp_path, d, 5, exp, exp[3], mode)
    _same_rows(after, before)      # {1, 2} is seq-contiguous


def test_append_compaction_of_one_pk_group(tmp_path):
    # 65 rows of one PK in one file, 300 in another: one output row
    from tools.gen_ssts import write_bytes_sst
    from horaedb_amd import Store
    d = str(tmp_path / "store")
    rng = np.random.default_rng(3)
    for seq, n in ((1, 65), (2, 300)):
        vals = [bytes(rng.integers(97, 123, rng.integers(0, 200)).astype(
            np.uint8).tolist()) for _ in range(n)]
        write_bytes_sst(os.path.join(d, "data", f"{seq}.sst"),
                        np.full(n, 77), np.full(n, 5000), vals, seq)
    exp = _expected_compaction(d, [1, 2], "append")
    assert len(exp[0]) == 1
    with Store(d, update_mode="append") as st:
        assert st.compact_files([1, 2], devices=[0]) == 3
    _check_output(tmp_path, d, 3, exp, exp[3], "append")


# ---- refusals ---------------------------------------------------------------

@pytest.mark.parametrize("how", ["compact", "compact_files"])
def test_append_group_over_the_value_limit_is_refused(tmp_path, how):
    from tools.gen_ssts import write_bytes_sst
    from horaedb_amd import Store, HxError
    d = str(tmp_path / "store")
    for seq in (1, 2):
        write_bytes_sst(os.path.join(d, "data", f"{seq}.sst"), [5, 6],
                        [1000, 1000], [bytes([64 + seq]) * (1 << 19), b"ok"],
                        seq)
    listing = [os.path.basename(p) for p in _files(d)]
    with Store(d, update_mode="append") as st:
        cat = st.catalog()
        with pytest.raises(HxError) as ei:
            if how == "compact":
                st.compact(ALL, devices=[0])
            else:
                st.compact_files([1, 2], devices=[0])
        assert ei.value.code == UNSUPPORTED and "2^20" in str(ei.value)
        assert st.catalog() == cat
        assert [os.path.basename(p) for p in _files(d)] == listing
        rows = st.scan(ALL, devices=[0])
    assert rows["series_id"].tolist() == [5, 6]
    assert rows["value"].tolist() == \
        [b"A" * (1 << 19) + b"B" * (1 << 19), b"okok"]
    # Overwrite has no concatenation: the same store compacts
    with Store(d) as st:
        assert st.compact(ALL, devices=[0]) == 3
        rows = st.scan(ALL, devices=[0])
    assert rows["value"].tolist() == [b"B" * (1 << 19), b"ok"]


def test_f64_write_on_binary_store_is_refused_and_store_reopens(tmp_path):
    from horaedb_amd import Store, HxError
    d = _rand_bytes_store(tmp_path, n_files=1, n_rows=100, n_series=10)
    k = np.arange(4)
    with Store(d) as st:
        with pytest.raises(HxError) as ei:
            st.write(k, k, k * 1.0)
        assert ei.value.code == UNSUPPORTED
    with Store(d) as st:
        assert [c["seq"] for c in st.catalog()] == [1]
        assert len(st.scan(ALL, devices=[0])["series_id"]) > 0
