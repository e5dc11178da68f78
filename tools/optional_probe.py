#!/usr/bin/env python3
# What reading reference-shaped files costs. Generates the same
# seeded Snappy store twice — once with REQUIRED columns, once the way the
# reference writes it (five nullable fields, __reserved__ all null, no other
# nulls) — and reports ms per exec_agg step under HX_REDECODE=1 (so the
# Snappy decode and k_expand_optional run inside every step) together with
# hx_get_decode_stats for both: the OPTIONAL value pages are 8 level bytes +
# 64 KB, two Snappy literals, so they leave the in-place path.
#
# Each measurement is a child process under its own time limit; a child that
# fails or times out ends the probe. Prints one JSON line.
#
#   python tools/optional_probe.py [--rows 200000000] [--ssts 16]
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

import numpy as np  # noqa: E402

COLS = ["series_id", "timestamp", "value", "__seq__", "__reserved__"]


def _write_one(job):
    out, j, n_ssts, n_series, n_points, seed, nullable = job
    import pyarrow as pa
    import pyarrow.parquet as pq
    from tools.gen_ssts import (make_series_ids, value_of, TS_START_DEFAULT,
                                STEP_MS_DEFAULT)
    ids = make_series_ids(n_series, seed)
    t0, t1 = j * n_points // n_ssts, (j + 1) * n_points // n_ssts
    k = t1 - t0
    series = np.repeat(ids, k)
    t_idx = np.tile(np.arange(t0, t1, dtype=np.int64), n_series)
    gidx = (np.repeat(np.arange(n_series, dtype=np.uint64), k) *
            np.uint64(n_points)) + t_idx.astype(np.uint64)
    n = len(series)
    types = [pa.uint64(), pa.int64(), pa.float64(), pa.uint64(), pa.uint64()]
    schema = pa.schema([pa.field(c, t, nullable=nullable)
                        for c, t in zip(COLS, types)])
    tbl = pa.table([
        pa.array(series), pa.array(TS_START_DEFAULT + t_idx * STEP_MS_DEFAULT),
        pa.array(value_of(seed, gidx)),
        pa.array(np.full(n, j + 1, dtype=np.uint64)),
        pa.nulls(n, pa.uint64()) if nullable
        else pa.array(np.zeros(n, dtype=np.uint64))], schema=schema)
    # the builtins are never read by the scan: dictionary-encode them (as
    # tools/gen_ssts.py does) to keep the files small
    pq.write_table(tbl, os.path.join(out, "data", f"{j + 1}.sst"),
                   row_group_size=8192, compression="SNAPPY",
                   data_page_version="1.0",
                   use_dictionary=["__seq__", "__reserved__"],
                   column_encoding={c: "PLAIN" for c in COLS[:3]},
                   write_statistics=True)
    return n


def gen(out, rows, series, ssts, seed, nullable, workers):
    os.makedirs(os.path.join(out, "data"), exist_ok=True)
    jobs = [(out, j, ssts, series, rows // series, seed, nullable)
            for j in range(ssts)]
    import multiprocessing as mp
    with mp.get_context("spawn").Pool(workers) as pool:
        return sum(pool.map(_write_one, jobs))


def measure(store, steps, warmup):
    """Child process: stage, warm up, time `steps` exec_agg passes."""
    from horaedb_amd import Store, AGG_SUM, AGG_COUNT
    from tools.gen_ssts import TS_START_DEFAULT
    with Store(store) as st, st.prepare((TS_START_DEFAULT, 2**62),
                                        devices=[0]) as p:
        for _ in range(warmup):
            p.exec_agg(ops=AGG_SUM | AGG_COUNT, copy=False)
        ms, dec = [], []
        for _ in range(steps):
            t0 = time.perf_counter()
            r = p.exec_agg(ops=AGG_SUM | AGG_COUNT, copy=False)
            ms.append((time.perf_counter() - t0) * 1e3)
            dec.append(p.stats()["decode_kernel_ms"])
        print(json.dumps({"ms_per_step": sorted(ms),
                          "decode_kernel_ms": sorted(dec),
                          "n_groups": int(r["n_groups"]),
                          "rows_scanned": p.stats()["rows_scanned"],
                          "decode_stats": p.decode_stats()}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=200_000_000)
    ap.add_argument("--series", type=int, default=2_000_000)
    ap.add_argument("--ssts", type=int, default=16)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--data-dir", default="/tmp/hx_optional_probe")
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--step-timeout", type=int, default=300)
    ap.add_argument("--measure", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.measure:
        return measure(a.measure, a.steps, a.warmup)
    out = {}
    env = dict(os.environ, HX_REDECODE="1")
    for name, nullable in (("required", False), ("reference_shaped", True)):
        store = os.path.join(a.data_dir, f"{name}_r{a.rows}_f{a.ssts}")
        if not os.path.isdir(os.path.join(store, "data")):
            gen(store, a.rows, a.series, a.ssts, a.seed, nullable, a.workers)
        r = subprocess.run(
            [sys.executable, os.path.abspath(__file__), "--measure", store,
             "--steps", str(a.steps), "--warmup", str(a.warmup)],
            env=env, capture_output=True, text=True, timeout=a.step_timeout)
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-2000:])
            sys.exit(f"{name}: measurement failed (rc={r.returncode})")
        out[name] = json.loads(r.stdout.strip().splitlines()[-1])
    med = lambda v: v[len(v) // 2]  # noqa: E731
    out["ratio_ms_per_step"] = (med(out["reference_shaped"]["ms_per_step"]) /
                                med(out["required"]["ms_per_step"]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
