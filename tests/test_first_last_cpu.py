# first / last (HX_AGG_FIRST, HX_AGG_LAST; include/horaedb_hx.h, DESIGN §4
# kernel 3d): the interface constants and struct layout, the expectation the
# GPU tests compare against, what that expectation covers, and the stand-alone
# check of the host merge rules. No GPU needed.
#
# Every comparison of first, last, first_ts and last_ts is exact: values as
# uint64 bit patterns, timestamps as integers. There is no tolerance.
import os
import re
import subprocess

import numpy as np
import pytest

from oracle.value_domain import bits_of, from_bits, total_order_key
from test_value_domain_cpu import (FULL, NZ, STALE, Rows, dedup_rows,
                                   vd_expected)
from tools.gen_ssts import (VD_BUCKET_MS, VD_RANGE, vd_base_rows,
                            vd_overwrite_rows)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "horaedb_hx.h")
CSRC = os.path.join(REPO, "horaedb_amd", "csrc")

KINDS = ("single", "two", "nullable")
QUERIES = {"full": dict(), "range": dict(ts_range=VD_RANGE),
           "bucket": dict(bucket_ms=VD_BUCKET_MS)}


def vd_files(kind):
    """The files of test_value_domain_gpu.build_store, as Rows."""
    if kind == "single":
        return [Rows(1, vd_base_rows())]
    return [Rows(q, d) for q, d in zip(
        (1, 2), vd_overwrite_rows(vd_base_rows(),
                                  nullable=kind == "nullable"))]


def fl_expected(ssts, ts_range=FULL, series_in=None, bucket_ms=0):
    """Per group (series, or series and ts // bucket_ms) of the surviving
    non-null rows: the smallest and greatest timestamp and the bits of the
    values there. A store opened without segments holds one survivor per
    primary key, so neither extreme has a tie."""
    series, ts, value, valid = dedup_rows(ssts, ts_range, series_in)
    series, ts, value = series[valid], ts[valid], value[valid]
    bits = bits_of(value)
    bucket = ts // bucket_ms if bucket_ms else np.zeros(len(ts), np.int64)
    head = np.ones(len(series), dtype=bool)
    head[1:] = (series[1:] != series[:-1]) | (bucket[1:] != bucket[:-1])
    starts = np.flatnonzero(head)
    ends = np.append(starts[1:], len(series))
    lo = np.array([s + int(np.argmin(ts[s:e])) for s, e in zip(starts, ends)],
                  dtype=np.int64)
    hi = np.array([s + int(np.argmax(ts[s:e])) for s, e in zip(starts, ends)],
                  dtype=np.int64)
    return {"series_id": series[starts], "bucket": bucket[starts],
            "first_ts": ts[lo], "first_bits": bits[lo],
            "last_ts": ts[hi], "last_bits": bits[hi]}


def check_first_last(res, exp, bucket_ms=0, sides=("first", "last")):
    """Exact comparison of the first/last columns of a result."""
    keys = np.asarray(res["series_id"], dtype=np.uint64)
    if bucket_ms:
        order = np.lexsort((res["bucket"], keys))
        res = {k: v[order] for k, v in res.items()}
        assert res["bucket"].tolist() == exp["bucket"].tolist()
    assert res["series_id"].tolist() == exp["series_id"].tolist()
    for side in sides:
        got_ts = np.asarray(res[side + "_ts"])
        assert got_ts.dtype == np.int64
        bad = np.flatnonzero(got_ts != exp[side + "_ts"])
        assert len(bad) == 0, (
            f"{side}_ts: {len(bad)} groups differ, first series "
            f"{int(exp['series_id'][bad[0]])}: got {int(got_ts[bad[0]])}, "
            f"expected {int(exp[side + '_ts'][bad[0]])}")
        got = bits_of(res[side])
        want = exp[side + "_bits"]
        bad = np.flatnonzero(got != want)
        assert len(bad) == 0, (
            f"{side}: {len(bad)} groups differ in bits, first series "
            f"{int(exp['series_id'][bad[0]])}: got {int(got[bad[0]]):#018x}, "
            f"expected {int(want[bad[0]]):#018x}")
    return len(exp["series_id"])


# ---- the interface ---------------------------------------------------------------

def _header():
    with open(HEADER) as f:
        return f.read()


def test_header_constants_match_wrapper():
    import horaedb_amd
    text = _header()
    vals = {}
    for name in ("FIRST", "LAST"):
        m = re.search(r"HX_AGG_%s\s*=\s*1u\s*<<\s*(\d+)" % name, text)
        assert m, name
        vals[name] = 1 << int(m.group(1))
    assert vals == {"FIRST": 1 << 5, "LAST": 1 << 6}
    assert horaedb_amd.AGG_FIRST == vals["FIRST"]
    assert horaedb_amd.AGG_LAST == vals["LAST"]
    # no clash with the five older ops
    older = [horaedb_amd.AGG_SUM, horaedb_amd.AGG_COUNT, horaedb_amd.AGG_MIN,
             horaedb_amd.AGG_MAX, horaedb_amd.AGG_AVG]
    assert not (vals["FIRST"] | vals["LAST"]) & sum(older)


def test_header_result_table_members_match_wrapper():
    from horaedb_amd.store import _ResultTable
    import ctypes as C
    m = re.search(r"typedef struct hx_result_table \{(.*?)\} hx_result_table;",
                  _header(), re.S)
    assert m
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    decls = [re.sub(r"\s+", " ", d).strip() for d in body.split(";")]
    decls = [d for d in decls if d]
    names = [d.split()[-1].lstrip("*") for d in decls]
    assert names == ["n_groups", "series_id", "bucket", "sum", "count", "vmin",
                     "vmax", "avg", "first", "first_ts", "last", "last_ts"]
    assert decls[-4:] == ["const double* first", "const int64_t* first_ts",
                          "const double* last", "const int64_t* last_ts"]
    assert [f for f, _ in _ResultTable._fields_] == names
    want = {"first": C.c_double, "first_ts": C.c_int64, "last": C.c_double,
            "last_ts": C.c_int64}
    for f, t in _ResultTable._fields_[-4:]:
        assert t._type_ is want[f], f


# ---- the expectation ---------------------------------------------------------------

def _loop_expected(ssts, ts_range=FULL, bucket_ms=0):
    """The same, row by row in plain Python: replay the files in sequence
    order into a dict per primary key, then walk the survivors."""
    rows = {}
    for f in sorted(ssts, key=lambda f: f.seq):
        fb = bits_of(f.value)
        for i in range(len(f.series)):
            rows[(int(f.series[i]), int(f.ts[i]))] = (int(fb[i]),
                                                      bool(f.valid[i]))
    groups = {}
    for (s, t), (b, ok) in rows.items():
        if not (ts_range[0] <= t < ts_range[1]) or not ok:
            continue
        g = groups.setdefault((s, t // bucket_ms if bucket_ms else 0),
                              [t, b, t, b])
        if t < g[0]:
            g[0], g[1] = t, b
        if t > g[2]:
            g[2], g[3] = t, b
    return [(k[0], k[1]) + tuple(groups[k]) for k in sorted(groups)]


@pytest.fixture(scope="module")
def files():
    return {k: vd_files(k) for k in KINDS}


@pytest.mark.parametrize("query", list(QUERIES))
@pytest.mark.parametrize("kind", KINDS)
def test_expectation_matches_row_loop(files, kind, query):
    kw = QUERIES[query]
    exp = fl_expected(files[kind], **kw)
    got = list(zip(*(exp[k].tolist() for k in
                     ("series_id", "bucket", "first_ts", "first_bits",
                      "last_ts", "last_bits"))))
    assert got == _loop_expected(files[kind], **kw)
    assert len(got) > 1000
    # the group set is the one every other aggregate has
    vd = vd_expected(files[kind], **kw)
    assert exp["series_id"].tolist() == vd["series_id"].tolist()
    assert exp["bucket"].tolist() == vd["bucket"].tolist()


# ---- what the expectation covers (so the GPU comparison cannot pass
# vacuously) -------------------------------------------------------------------

def _is_nan(bits):
    return (bits & np.uint64(0x7FFFFFFFFFFFFFFF)) > np.uint64(
        0x7FF0000000000000)


@pytest.mark.parametrize("kind", KINDS)
def test_coverage_of_last_values(files, kind):
    exp = fl_expected(files[kind], ts_range=VD_RANGE)
    vd = vd_expected(files[kind], ts_range=VD_RANGE)
    last, first = exp["last_bits"], exp["first_bits"]
    assert _is_nan(last).any()
    assert (last == np.uint64(STALE)).any()
    assert (last == np.uint64(NZ)).any()
    assert ((last != vd["vmax_bits"]) & (first != vd["vmin_bits"])).any()
    # first and last are not one column twice
    assert (exp["first_ts"] < exp["last_ts"]).any()
    assert (first != last).any()


def test_coverage_nullable_latest_row_is_null(files):
    f = files["nullable"]
    exp = fl_expected(f, ts_range=VD_RANGE)
    series, ts, _, valid = dedup_rows(f, VD_RANGE)
    greatest = {}
    for s, t in zip(series.tolist(), ts.tolist()):
        greatest[s] = max(t, greatest.get(s, t))
    assert not valid.all()
    fell_back = [s for s, t in zip(exp["series_id"].tolist(),
                                   exp["last_ts"].tolist())
                 if t < greatest[s]]
    assert len(fell_back) >= 1
    # and the mirror: a group whose earliest surviving row is null
    smallest = {}
    for s, t in zip(series.tolist(), ts.tolist()):
        smallest[s] = min(t, smallest.get(s, t))
    assert any(t > smallest[s] for s, t in zip(exp["series_id"].tolist(),
                                               exp["first_ts"].tolist()))


def test_coverage_two_files_last_from_either(files):
    old, new = files["two"]
    exp = fl_expected(files["two"], ts_range=VD_RANGE)
    new_pk = set(zip(new.series.tolist(), new.ts.tolist()))
    from_new = [(s, t) in new_pk for s, t in zip(exp["series_id"].tolist(),
                                                 exp["last_ts"].tolist())]
    assert any(from_new) and not all(from_new)
    first_new = [(s, t) in new_pk for s, t in zip(exp["series_id"].tolist(),
                                                  exp["first_ts"].tolist())]
    assert any(first_new) and not all(first_new)


def test_total_order_key_breaks_ties_as_documented():
    # the tie rule of the header: the totalOrder-greater value wins
    b = np.array([NZ, 0, STALE, 0x7FF0000000000001, 0xFFF8000000000000,
                  0xFFF0000000000000], dtype=np.uint64)
    k = total_order_key(from_bits(b))
    assert k[1] > k[0] and k[2] > k[3] and k[5] > k[4]


# ---- the host merge rules -------------------------------------------------------

def test_check_program():
    b = subprocess.run(["make", "-C", CSRC, "first_last_check"],
                       capture_output=True, text=True)
    assert b.returncode == 0, b.stdout + b.stderr
    r = subprocess.run([os.path.join(CSRC, "first_last_check")],
                       capture_output=True, text=True)
    print(b.stdout + r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == "all ok"
    assert len(lines) > 10
    assert not any(ln.endswith("FAIL") for ln in lines)
