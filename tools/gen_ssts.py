#!/usr/bin/env python3
# tools/gen_ssts.py — synthetic SST generator (shared by tests and bench.py).
#
# Writes metric-shaped Parquet SSTs exactly as the reference writer contract
# produces them (storage.rs:193-213; defaults config.rs:120-133: row-group
# 8192, PLAIN, dict off; encodings enum config.rs:54-75; Snappy or
# uncompressed per config):
#   (series_id u64 PK, timestamp i64 PK, value f64, __seq__ u64, __reserved__ u64)
#   rows sorted by (series_id, timestamp); one __seq__ per file = file id;
#   file path {out}/data/{seq}.sst (sst.rs:193-205).
#
# Dataset shape per BASELINE.json / SURVEY §8(d): n_series ids (sorted unique
# u64), n_points = n_rows/n_series timestamps per series at 10s steps from
# ts_start; SST w holds the w-th contiguous time-index window (disjoint ts
# ranges => no cross-SST duplicate PKs, the compacted layout; overlap
# scenarios for dedup tests are built with gen_sst_from_arrays).
#
# value(s_idx, t) is a counter-based splitmix64 hash -> U[0,1) so any row's
# value is reproducible independent of chunking or worker count.
import argparse
import os
import json
import numpy as np

TS_START_DEFAULT = 1735689600000  # 2025-01-01T00:00:00Z, SURVEY §8(d)
STEP_MS_DEFAULT = 10_000

SCHEMA_COLS = ["series_id", "timestamp", "value", "__seq__", "__reserved__"]


def _pa_schema():
    import pyarrow as pa
    return pa.schema([
        pa.field("series_id", pa.uint64(), nullable=False),
        pa.field("timestamp", pa.int64(), nullable=False),
        pa.field("value", pa.float64(), nullable=False),
        pa.field("__seq__", pa.uint64(), nullable=False),
        pa.field("__reserved__", pa.uint64(), nullable=False),
    ])


def splitmix64(x):
    """Vectorized splitmix64 on uint64 arrays (wrapping arithmetic)."""
    x = x.astype(np.uint64, copy=True)
    x += np.uint64(0x9E3779B97F4A7C15)
    z = x
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def value_of(seed, global_idx):
    """value = U[0,1) from splitmix64(seed*GOLDEN ^ global_idx)."""
    mixed_seed = np.uint64((int(seed) * 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF)
    h = splitmix64(mixed_seed ^ global_idx.astype(np.uint64))
    return (h >> np.uint64(11)).astype(np.float64) * (2.0 ** -53)


def make_series_ids(n_series, seed):
    """n_series sorted unique u64 ids (seahash-of-labels style)."""
    rng = np.random.default_rng(np.random.PCG64(seed))
    ids = rng.integers(0, np.iinfo(np.uint64).max, n_series, dtype=np.uint64)
    ids = np.unique(ids)
    while len(ids) < n_series:  # collision top-up (vanishingly rare)
        extra = rng.integers(0, np.iinfo(np.uint64).max,
                             n_series - len(ids) + 16, dtype=np.uint64)
        ids = np.unique(np.concatenate([ids, extra]))
    return ids[:n_series]


def write_sst(path, series, ts, value, seq, row_group=8192,
              compression="none", ts_encoding="PLAIN", dict_columns=(),
              slim_builtins=False, data_page_version="1.0"):
    """Write one SST from explicit row arrays (must be (series,ts)-sorted)."""
    import pyarrow as pa
    import pyarrow.parquet as pq
    n = len(series)
    tbl = pa.table({
        "series_id": np.ascontiguousarray(series, dtype=np.uint64),
        "timestamp": np.ascontiguousarray(ts, dtype=np.int64),
        "value": np.ascontiguousarray(value, dtype=np.float64),
        "__seq__": np.full(n, seq, dtype=np.uint64),
        "__reserved__": np.zeros(n, dtype=np.uint64),
    }, schema=_pa_schema())
    kw = {}
    if slim_builtins and not dict_columns:
        # __seq__/__reserved__ are constant per file and never read by the
        # scan (seq comes from the file id); dictionary-encode them to cut
        # ~40% of file size for the 8-GPU bench datasets. The three DATA
        # columns keep their configured encodings.
        dict_columns = ("__seq__", "__reserved__")
    if dict_columns:
        # RLE_DICTIONARY chunks (config.rs:54-75 with dictionaries on);
        # large limits keep one dictionary per chunk (no PLAIN fallback)
        kw["use_dictionary"] = list(dict_columns)
        kw["dictionary_pagesize_limit"] = 1 << 30
        enc = {c: "PLAIN" for c in SCHEMA_COLS if c not in dict_columns}
        enc["timestamp"] = ts_encoding if "timestamp" not in dict_columns \
            else None
        enc = {c: v for c, v in enc.items() if v}
    else:
        kw["use_dictionary"] = False
        enc = {c: "PLAIN" for c in SCHEMA_COLS}
        enc["timestamp"] = ts_encoding
    pq.write_table(
        tbl, path, row_group_size=row_group,
        compression="NONE" if compression == "none" else compression.upper(),
        data_page_version=data_page_version, column_encoding=enc,
        write_statistics=True, **kw)
    return n


def gen_sst_from_arrays(store_dir, seq, series, ts, value, sort=True, **kw):
    """Test scenario helper: build {store}/data/{seq}.sst from explicit rows.
    sort=True applies the writer's (pk...)-stable sort (storage.rs:244-256)."""
    series = np.asarray(series, dtype=np.uint64)
    ts = np.asarray(ts, dtype=np.int64)
    value = np.asarray(value, dtype=np.float64)
    if sort:
        order = np.lexsort((ts, series))  # stable: equal PKs keep input order
        series, ts, value = series[order], ts[order], value[order]
    ddir = os.path.join(store_dir, "data")
    os.makedirs(ddir, exist_ok=True)
    path = os.path.join(ddir, f"{seq}.sst")
    write_sst(path, series, ts, value, seq, **kw)
    return path


def _gen_one(args):
    (j, out_dir, ids_path, n_series, n_points, n_ssts, seed, ts_start,
     step_ms, row_group, compression, ts_encoding) = args
    # j enumerates (generation, window): generation g re-writes the SAME
    # (series, ts) PKs of window w with new values and a higher seq — the
    # ts-overlap layout (overwrite churn before compaction) that exercises
    # the cross-SST MergeExec dedup (read.rs:100-391) at scale. g = 0 is the
    # plain disjoint layout.
    w, g = j % n_ssts, j // n_ssts
    ids = np.load(ids_path, mmap_mode="r")
    t0 = w * n_points // n_ssts
    t1 = (w + 1) * n_points // n_ssts
    k = t1 - t0
    if k == 0:
        return None
    series = np.repeat(ids, k)
    t_idx = np.tile(np.arange(t0, t1, dtype=np.int64), n_series)
    ts = ts_start + t_idx * step_ms
    gidx = (np.repeat(np.arange(n_series, dtype=np.uint64), k) *
            np.uint64(n_points)) + t_idx.astype(np.uint64)
    value = value_of(seed + 7919 * g, gidx)
    seq = j + 1
    path = os.path.join(out_dir, "data", f"{seq}.sst")
    n = write_sst(path, series, ts, value, seq, row_group=row_group,
                  compression=compression, ts_encoding=ts_encoding,
                  slim_builtins=True)
    return {"seq": seq, "path": path, "rows": int(n),
            "ts_min": int(ts_start + t0 * step_ms),
            "ts_max": int(ts_start + (t1 - 1) * step_ms)}


def gen_dataset(out_dir, n_rows, n_series, n_ssts, seed=42,
                ts_start=TS_START_DEFAULT, step_ms=STEP_MS_DEFAULT,
                row_group=8192, compression="none", ts_encoding="PLAIN",
                workers=1, overlap_gens=1):
    """overlap_gens > 1: each further generation re-writes the SAME PKs with
    new values under higher seqs (ts-overlapping SSTs) — the pre-compaction
    overwrite-churn layout; total rows = n_rows * overlap_gens, surviving
    rows after dedup = the newest generation only."""
    assert n_rows % n_series == 0, "n_rows must be a multiple of n_series"
    n_points = n_rows // n_series
    os.makedirs(os.path.join(out_dir, "data"), exist_ok=True)
    ids = make_series_ids(n_series, seed)
    ids_path = os.path.join(out_dir, "series_ids.npy")
    np.save(ids_path, ids)
    jobs = [(j, out_dir, ids_path, n_series, n_points, n_ssts, seed,
             ts_start, step_ms, row_group, compression, ts_encoding)
            for j in range(n_ssts * max(1, overlap_gens))]
    if workers > 1:
        import multiprocessing as mp
        with mp.get_context("spawn").Pool(workers) as pool:
            metas = pool.map(_gen_one, jobs)
    else:
        metas = [_gen_one(j) for j in jobs]
    metas = [m for m in metas if m]
    manifest = {
        "n_rows": n_rows * max(1, overlap_gens), "n_series": n_series,
        "n_points": n_points, "overlap_gens": max(1, overlap_gens),
        "n_ssts": len(metas), "seed": seed, "ts_start": ts_start,
        "step_ms": step_ms, "row_group": row_group,
        "compression": compression, "ts_encoding": ts_encoding,
        "ts_end": ts_start + n_points * step_ms, "ssts": metas,
    }
    with open(os.path.join(out_dir, "dataset.json"), "w") as f:
        json.dump(manifest, f, indent=1)
    return manifest


def write_bytes_sst(path, series, ts, values, seq, row_group=8192,
                    sort=True, compression="NONE", nullable=False,
                    data_page_version="1.0", data_page_size=None,
                    write_batch_size=None):
    """One Binary-value SST (BytesMergeOperator stores, operator.rs:47-111):
    (series u64 PK, ts i64 PK, value binary, builtins), PLAIN, writer-sorted
    by (series, ts) stable (equal PKs keep input order). compression: "NONE"
    (default), "SNAPPY" (the reference's default, config.rs:120-133) or
    "ZSTD". nullable: every column is declared OPTIONAL, the reference's
    shape; a value may then be None. data_page_size: pyarrow's page-size
    limit (the default closes a page at 1 MiB). write_batch_size: the rows
    after which pyarrow looks at the page size (its default is 1024). The
    8-byte columns must stay one page per chunk; the value chunk may hold
    several."""
    import pyarrow as pa
    import pyarrow.parquet as pq
    series = np.asarray(series, dtype=np.uint64)
    ts = np.asarray(ts, dtype=np.int64)
    values = list(values)
    if sort:
        order = np.lexsort((ts, series))
        series = series[order]
        ts = ts[order]
        values = [values[i] for i in order]
    n = len(series)
    schema = pa.schema([
        pa.field("series_id", pa.uint64(), nullable=nullable),
        pa.field("timestamp", pa.int64(), nullable=nullable),
        pa.field("value", pa.binary(), nullable=nullable),
        pa.field("__seq__", pa.uint64(), nullable=nullable),
        pa.field("__reserved__", pa.uint64(), nullable=nullable),
    ])
    tbl = pa.table({
        "series_id": pa.array(series, pa.uint64()),
        "timestamp": pa.array(ts, pa.int64()),
        "value": pa.array([v if v is None or isinstance(v, bytes)
                           else v.encode() for v in values], pa.binary()),
        "__seq__": pa.array(np.full(n, seq, np.uint64), pa.uint64()),
        "__reserved__": pa.array(np.zeros(n, np.uint64), pa.uint64()),
    }, schema=schema)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    extra = {} if data_page_size is None else \
        {"data_page_size": int(data_page_size)}
    if write_batch_size is not None:
        extra["write_batch_size"] = int(write_batch_size)
    pq.write_table(tbl, path, row_group_size=row_group,
                   compression=compression, use_dictionary=False,
                   data_page_version=data_page_version,
                   column_encoding={c: "PLAIN" for c in
                                    ("series_id", "timestamp", "value",
                                     "__seq__", "__reserved__")},
                   write_statistics=True, **extra)
    return path


def gen_tag_index(store_dir, n_dc=100):
    """Write {store}/index/1.sst (the RFC index table, rfc:86-137) for the
    dataset's series: tags dc=dc{i%n_dc} (1/n_dc selectivity each) and
    env in {prod, dev}. Vectorized pyarrow write (PLAIN uncompressed,
    row-group 8192, stats) matching the native reader's layout contract;
    rows sorted by (tag_key, tag_value, tsid)."""
    import pyarrow as pa
    import pyarrow.parquet as pq
    idx_path = os.path.join(store_dir, "index", "1.sst")
    if os.path.exists(idx_path):
        return idx_path
    os.makedirs(os.path.dirname(idx_path), exist_ok=True)
    ids = np.load(os.path.join(store_dir, "series_ids.npy"))
    n = len(ids)
    # dc block: values dc0..dc{n_dc-1} in STRING sort order, tsids ascending
    dc_strings = sorted(f"dc{k}" for k in range(n_dc))
    rank = np.empty(n_dc, np.int64)
    for r, sname in enumerate(dc_strings):
        rank[int(sname[2:])] = r
    codes = rank[np.arange(n) % n_dc]
    order = np.lexsort((ids, codes))   # ids already ascending per group
    dc_vals = np.array([f"dc{k}" for k in range(n_dc)], dtype=object)
    dc_value_col = dc_vals[np.arange(n) % n_dc][order]
    dc_tsid = ids[order]
    # env block: dev (odd i) then prod (even i), tsids ascending per value
    env_is_prod = (np.arange(n) % 2) == 0
    env_order = np.lexsort((ids, env_is_prod))  # dev(False=0) first? no:
    # lexsort ascending: False(0) < True(1) -> dev rows first... but string
    # order is "dev" < "prod" and dev rows are the odd ones (is_prod False)
    env_value_col = np.where(env_is_prod[env_order], "prod", "dev")
    env_tsid = ids[env_order]
    schema = pa.schema([
        pa.field("metric_id", pa.uint64(), nullable=False),
        pa.field("tag_key", pa.binary(), nullable=False),
        pa.field("tag_value", pa.binary(), nullable=False),
        pa.field("tsid", pa.uint64(), nullable=False),
    ])   # REQUIRED columns: v1 pages carry no def-level prefix
    tbl = pa.table({
        "metric_id": pa.array(np.zeros(2 * n, np.uint64), pa.uint64()),
        "tag_key": pa.array([b"dc"] * n + [b"env"] * n, pa.binary()),
        "tag_value": pa.array(
            [x.encode() for x in dc_value_col] +
            [x.encode() for x in env_value_col], pa.binary()),
        "tsid": pa.array(np.concatenate([dc_tsid, env_tsid]), pa.uint64()),
    }, schema=schema)
    pq.write_table(tbl, idx_path, row_group_size=8192, compression="NONE",
                   use_dictionary=False, data_page_version="1.0",
                   column_encoding={c: "PLAIN" for c in
                                    ("metric_id", "tag_key", "tag_value",
                                     "tsid")},
                   write_statistics=True)
    return idx_path


def middle_range(manifest, frac=0.5):
    """The benchmark's ts-range: middle `frac` of the dataset span."""
    span = manifest["ts_end"] - manifest["ts_start"]
    lo = manifest["ts_start"] + int(span * (0.5 - frac / 2))
    hi = manifest["ts_start"] + int(span * (0.5 + frac / 2))
    return lo, hi


# ---------------------------------------------------------------------------
# Value-domain datasets (tests/test_value_domain_*.py): the f64 values a
# metric engine meets beyond U[0,1) — NaN of either sign (quiet, signalling,
# the Prometheus stale marker), signed zeros, infinities, subnormals,
# DBL_MAX — placed so every one of them meets every lane and pair slot of
# the aggregate kernels as the first, an inner and the last row of its
# group. Values travel as uint64 bit patterns throughout.
# ---------------------------------------------------------------------------
VD_SPECIAL = [
    ("+0", 0x0000000000000000), ("-0", 0x8000000000000000),
    ("+inf", 0x7FF0000000000000), ("-inf", 0xFFF0000000000000),
    ("+qnan", 0x7FF8000000000000), ("-qnan", 0xFFF8000000000000),
    ("stale", 0x7FF0000000000002),      # Prometheus stale marker (signalling)
    ("+nan_max", 0x7FFFFFFFFFFFFFFF),
    ("+denorm_min", 0x0000000000000001), ("-denorm_min", 0x8000000000000001),
    ("+min_normal", 0x0010000000000000), ("-min_normal", 0x8010000000000000),
    ("+dbl_max", 0x7FEFFFFFFFFFFFFF), ("-dbl_max", 0xFFEFFFFFFFFFFFFF),
    ("+1", 0x3FF0000000000000), ("-1", 0xBFF0000000000000),
]
VD_BITS = np.array([b for _, b in VD_SPECIAL], dtype=np.uint64)
_VD_DBL_MAX = {i for i, (n, _) in enumerate(VD_SPECIAL) if "dbl_max" in n}
VD_NAN = {i for i, (n, _) in enumerate(VD_SPECIAL)
          if "nan" in n or n == "stale"}

VD_T0 = 1_000_000            # ts of row j of an ordinary group: T0 + j*STEP
VD_STEP = 1_000
VD_MAX_RUN = 5
VD_RANGE = (VD_T0, VD_T0 + VD_MAX_RUN * VD_STEP)   # holds every group row;
#   the filler rows of the ts-range identity traps lie outside it
VD_BUCKET_MS = 2 * VD_STEP   # splits a 5-row group into rows 01 | 23 | 4
VD_BOUNDARY = 8192           # the default row-group size


def _f2b(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def vd_class_of(bits):
    """Index into VD_SPECIAL of each bit pattern, -1 for any other value."""
    bits = np.asarray(bits, dtype=np.uint64)
    cls = np.full(len(bits), -1, dtype=np.int64)
    for i, b in enumerate(VD_BITS):
        cls[bits == b] = i
    return cls


def _vd_filler(rng, n):
    """Mixed-sign ordinary values, |x| in [1e-3, 1e3]."""
    mag = 10.0 ** rng.uniform(-3, 3, n)
    return _f2b(mag * rng.choice([-1.0, 1.0], n))


def _vd_cover_groups(rng):
    """Groups (lists of bit patterns, run length 1..5) that put every class
    of VD_SPECIAL at every row position mod 128 as the first, an inner and
    the last row of a group, assuming the first group starts at a row that
    is a multiple of 128. At most one |x| = DBL_MAX per group: two of them
    make the sum's overflow depend on the order of the additions."""
    n_cls = len(VD_SPECIAL)
    need = np.ones((n_cls, 3, 128), dtype=bool)   # class, role, position
    order = rng.permutation(n_cls)

    def roles(j, L):
        r = []
        if j == 0:
            r.append(0)
        if j == L - 1:
            r.append(2)
        return r or [1]

    groups, r = [], 0
    while need.any():
        # the run length that serves the most open (role, position) pairs
        best, best_score = 1, -1.0
        for L in range(1, VD_MAX_RUN + 1):
            score = sum(need[:, ro, (r + j) % 128].any()
                        for j in range(L) for ro in roles(j, L)) / L
            if score > best_score + 1e-12:
                best, best_score = L, score
        L = best
        g, has_max = [], False
        for j in range(L):
            pos = (r + j) % 128
            pick = -1
            for c in order:
                if has_max and c in _VD_DBL_MAX:
                    continue
                if any(need[c, ro, pos] for ro in roles(j, L)):
                    pick = int(c)
                    break
            if pick < 0:
                g.append(int(_vd_filler(rng, 1)[0]))
                continue
            for ro in roles(j, L):
                need[pick, ro, pos] = False
            has_max |= pick in _VD_DBL_MAX
            g.append(int(VD_BITS[pick]))
            order = np.roll(order, 1)
        groups.append(g)
        r += L
    return groups


def _vd_fixed_groups():
    """Hand-written groups: cancellation, same-sign overflow, all-subnormal
    (every partial sum of those is a representable subnormal, so their sum
    is exact under any order)."""
    d = 5e-324
    vals = [
        [1e16, 1.0, -1e16, 3.0],
        [1e100, -1e100, 1e-100],
        [-1e16, 1e16, 1.0, -1.0, 2.5],
        [0.1, 0.2, -0.3],
        [1e308, 1e308, 1e308],             # +inf
        [-1e308, -1e308, -1e308],          # -inf
        [d, d, d, d, d],
        [3 * d, -d, 7 * d],
        [-d, -2 * d, -4 * d, -8 * d],
        [2.0 ** -1030, 2.0 ** -1040, -(2.0 ** -1050), d],
        [1023 * d],
        [2.0 ** -1023, 2.0 ** -1024, 2.0 ** -1025, 2.0 ** -1026],
    ]
    return [[int(b) for b in _f2b(v)] for v in vals]


def vd_base_rows(seed=0, sentinel_series=False):
    """The one-SST value-domain table: dict of row arrays sorted by
    (series, ts) — series u64, ts i64, bits u64, kind i8 per row
    (0 padding, 1 coverage, 2 fixed, 3 identity trap).
    Layout: mixed-sign padding groups (a multiple of 128 rows, sized so the
    file passes VD_BOUNDARY and a coverage group holding a special straddles
    it), the coverage groups, the fixed groups, then the two ts-range
    identity traps: a series whose only row inside VD_RANGE is +NaN (-NaN in
    the second), between rows of the same series outside the range.
    sentinel_series: the last fixed group gets series id 2**64-1 (a store
    the one-CAS key claim cannot serve) and the traps are left out."""
    rng = np.random.default_rng(seed)
    cover = _vd_cover_groups(rng)
    starts = np.cumsum([0] + [len(g) for g in cover])
    n_cover = int(starts[-1])
    pad = None
    lo = -(-(VD_BOUNDARY + 64 - n_cover) // 128) * 128
    for p in range(max(lo, 0), max(lo, 0) + 128 * 64, 128):
        for g, s in zip(cover, starts):
            if s + p < VD_BOUNDARY < s + p + len(g) and \
                    (vd_class_of(g) >= 0).any():
                pad = p
                break
        if pad is not None:
            break
    assert pad is not None, "no coverage group straddles the boundary"
    groups, kinds = [], []
    left, L = pad, 1
    while left > 0:
        k = min(L, left)
        groups.append([int(b) for b in _vd_filler(rng, k)])
        kinds.append(0)
        left -= k
        L = L % VD_MAX_RUN + 1
    groups += cover
    kinds += [1] * len(cover)
    fixed = _vd_fixed_groups()
    groups += fixed
    kinds += [2] * len(fixed)
    n_groups = len(groups) + 2
    stride = (2 ** 63) // n_groups     # ids spread over half the u64 range
    series, ts, bits, kind = [], [], [], []
    for k, (g, kd) in enumerate(zip(groups, kinds)):
        sid = (k + 1) * stride + (k * 7919) % 1000
        if sentinel_series and k == len(groups) - 1:
            sid = 2 ** 64 - 1
        for j, b in enumerate(g):
            series.append(sid)
            ts.append(VD_T0 + j * VD_STEP)
            bits.append(b)
            kind.append(kd)
    if not sentinel_series:
        out_ts = [VD_RANGE[0] - 2 * VD_STEP, VD_RANGE[0] - VD_STEP,
                  VD_T0 + 2 * VD_STEP, VD_RANGE[1], VD_RANGE[1] + VD_STEP]
        for t, nan in enumerate((0x7FF8000000000000, 0xFFF8000000000000)):
            sid = (len(groups) + 1 + t) * stride + 13
            fill = _vd_filler(rng, 5)
            for j in range(5):
                series.append(sid)
                ts.append(out_ts[j])
                bits.append(nan if j == 2 else int(fill[j]))
                kind.append(3)
    return {"series": np.array(series, dtype=np.uint64),
            "ts": np.array(ts, dtype=np.int64),
            "bits": np.array(bits, dtype=np.uint64),
            "kind": np.array(kind, dtype=np.int8)}


def vd_overwrite_rows(base, seed=1, nullable=False):
    """The newer SST of the two-file variants: it rewrites, by PK, every
    second special row of the coverage groups with a finite value and every
    second ordinary row (padding and coverage filler) with a special (never
    |x| = DBL_MAX, see _vd_cover_groups), so dedup has to decide by key
    alone. It also carries the superseded-row identity traps: two new series
    whose rows sit in BOTH files; the older file's middle row is +NaN (-NaN),
    the newer file rewrites the four rows around it and not the NaN.
    nullable: the rewriting trap rows are null, so the NaN is the series'
    only surviving value.
    Returns (older, newer): row dicts like vd_base_rows' plus 'null'."""
    rng = np.random.default_rng(seed)
    cls = vd_class_of(base["bits"])
    grp = base["kind"]
    special = np.flatnonzero((cls >= 0) & (grp == 1))[::2]
    plain = np.flatnonzero((cls < 0) & (grp <= 1))[::2]
    ok = np.array([i for i in range(len(VD_SPECIAL))
                   if i not in _VD_DBL_MAX])
    take = np.sort(np.concatenate([special, plain]))
    new_bits = base["bits"][take].copy()
    is_sp = np.isin(take, special)
    new_bits[is_sp] = _vd_filler(rng, int(is_sp.sum()))
    new_bits[~is_sp] = VD_BITS[ok[np.arange(int((~is_sp).sum())) % len(ok)]]
    older = {k: v.copy() for k, v in base.items()}
    newer = {"series": base["series"][take], "ts": base["ts"][take],
             "bits": new_bits, "kind": base["kind"][take]}
    # superseded-row traps, after every other series
    top = int(base["series"].max())
    o_rows, n_rows = [], []
    for t, nan in enumerate((0x7FF8000000000000, 0xFFF8000000000000)):
        sid = top + 1000 * (t + 1)
        fill = _vd_filler(rng, 10)
        for j in range(5):
            tsj = VD_T0 + j * VD_STEP
            o_rows.append((sid, tsj, nan if j == 2 else int(fill[j])))
            if j != 2:
                n_rows.append((sid, tsj, int(fill[5 + j])))
    for d, rows in ((older, o_rows), (newer, n_rows)):
        d["series"] = np.concatenate(
            [d["series"], np.array([r[0] for r in rows], dtype=np.uint64)])
        d["ts"] = np.concatenate(
            [d["ts"], np.array([r[1] for r in rows], dtype=np.int64)])
        d["bits"] = np.concatenate(
            [d["bits"], np.array([r[2] for r in rows], dtype=np.uint64)])
        d["kind"] = np.concatenate(
            [d["kind"], np.full(len(rows), 3, dtype=np.int8)])
    older["null"] = np.zeros(len(older["series"]), dtype=bool)
    newer["null"] = np.zeros(len(newer["series"]), dtype=bool)
    if nullable:
        # ~30 % nulls; a null next to every third NaN row; one series null
        # throughout; traps: the rewriting rows null, the NaN row never
        all_null = base["series"][np.flatnonzero(grp == 1)[40]]
        for d in (older, newer):
            n = len(d["series"])
            m = rng.random(n) < 0.3
            nan_rows = np.flatnonzero(np.isin(vd_class_of(d["bits"]),
                                              list(VD_NAN)))[::3]
            m[np.clip(nan_rows[0::2] - 1, 0, n - 1)] = True
            m[np.clip(nan_rows[1::2] + 1, 0, n - 1)] = True
            m[nan_rows] = False
            m[d["series"] == all_null] = True
            trap = d["kind"] == 3
            m[trap] = False
            if d is newer:
                m[trap & (d["series"] > top)] = True
            d["null"] = m
    return older, newer


def vd_coverage(series, bits, row_group):
    """Where the special classes sit in one (series, ts)-sorted file:
    (missing, straddles). missing lists every (class name, role, position
    mod 128) that does not occur, role being first/inner/last row of a
    run-length 1..5 group; straddles counts special values inside groups
    that cross a multiple of row_group."""
    series = np.asarray(series, dtype=np.uint64)
    n = len(series)
    cls = vd_class_of(bits)
    first = np.ones(n, dtype=bool)
    first[1:] = series[1:] != series[:-1]
    last = np.ones(n, dtype=bool)
    last[:-1] = first[1:]
    gid = np.cumsum(first) - 1
    gstart = np.flatnonzero(first)[gid]
    glen = np.bincount(gid)[gid]
    seen = np.zeros((len(VD_SPECIAL), 3, 128), dtype=bool)
    rows = np.flatnonzero((cls >= 0) & (glen <= VD_MAX_RUN))
    pos = rows % 128
    seen[cls[rows[first[rows]]], 0, pos[first[rows]]] = True
    inner = ~first[rows] & ~last[rows]
    seen[cls[rows[inner]], 1, pos[inner]] = True
    seen[cls[rows[last[rows]]], 2, pos[last[rows]]] = True
    missing = [(VD_SPECIAL[c][0], ("first", "inner", "last")[ro], int(p))
               for c, ro, p in zip(*np.nonzero(~seen))]
    crosses = (gstart // row_group) != ((gstart + glen - 1) // row_group)
    return missing, int((crosses & (cls >= 0)).sum())


def main():
    p = argparse.ArgumentParser()
    p.add_argument("out_dir")
    p.add_argument("--rows", type=int, default=10_000_000)
    p.add_argument("--series", type=int, default=100_000)
    p.add_argument("--ssts", type=int, default=1)
    p.add_argument("--seed", type=int, default=42)
    p.add_argument("--compression", default="none", choices=["none", "snappy", "zstd"])
    p.add_argument("--ts-encoding", default="PLAIN",
                   choices=["PLAIN", "DELTA_BINARY_PACKED"])
    p.add_argument("--workers", type=int, default=1)
    args = p.parse_args()
    m = gen_dataset(args.out_dir, args.rows, args.series, args.ssts,
                    seed=args.seed, compression=args.compression,
                    ts_encoding=args.ts_encoding, workers=args.workers)
    print(json.dumps({k: v for k, v in m.items() if k != "ssts"}))


if __name__ == "__main__":
    main()
