#!/usr/bin/env python3
# What first/last cost. Builds the benchmark's dataset through
# the same generator (tools/gen_ssts.gen_dataset, seed 42, Snappy pages) at a
# scale given on the command line, stages the benchmark's query (the
# middle half of the time span, group by series) once and times hx_exec_agg
# for three op sets on that one prepared scan:
#   min,max          the closest existing query (one MM pass)
#   last             the TS pass plus the resolve kernel, no value pass
#   sum,count,last   a value pass, then the TS pass and the resolve
# Per op set: the median over --steps executions (after --warmup) of
# hx_exec_stats.agg_kernel_ms (aggregate kernels plus, for first/last, the
# resolve kernel) and exec_ms (wall of hx_exec_agg, D2H included). One more
# `last` execution under HX_DEBUG=1 reads the resolve kernel's own time off
# the library's debug line, which splits `last` into TS pass and resolve.
# Prints one JSON line and, with --out, writes it to a file.
#
#   python tools/first_last_cost.py [--rows 100000000] [--series 1000000]
import argparse
import json
import os
import re
import statistics
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)


def timed(p, ops, steps, warmup):
    for _ in range(warmup):
        p.exec_agg(ops=ops, copy=False)
    kern, wall, groups = [], [], 0
    for _ in range(steps):
        groups = p.exec_agg(ops=ops, copy=False)["n_groups"]
        st = p.stats()
        kern.append(st["agg_kernel_ms"])
        wall.append(st["exec_ms"])
    return {"kernel_ms": statistics.median(kern),
            "kernel_ms_min": min(kern), "kernel_ms_max": max(kern),
            "wall_ms": statistics.median(wall),
            "wall_ms_min": min(wall), "wall_ms_max": max(wall),
            "n_groups": groups, "rows_matched": st["rows_matched"]}


def resolve_kernel_ms(p, ops):
    """One execution with the library's debug lines caught from fd 2."""
    with tempfile.TemporaryFile() as f:
        saved = os.dup(2)
        os.dup2(f.fileno(), 2)
        os.environ["HX_DEBUG"] = "1"
        try:
            p.exec_agg(ops=ops, copy=False)
        finally:
            del os.environ["HX_DEBUG"]
            os.dup2(saved, 2)
            os.close(saved)
        f.seek(0)
        text = f.read().decode(errors="replace")
    m = re.search(r"first/last resolve groups=\d+ kernel_ms=([0-9.]+)", text)
    route = re.findall(r"kernel=([a-z-]+)", text)
    return (float(m.group(1)) if m else None), route


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--series", type=int, default=1_000_000)
    ap.add_argument("--ssts", type=int, default=64)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--compression", default="snappy")
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--data-dir", default="/tmp/hx_bench_data")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    from horaedb_amd import (AGG_COUNT, AGG_LAST, AGG_MAX, AGG_MIN, AGG_SUM,
                             Store)
    from tools.gen_ssts import gen_dataset, middle_range

    # the directory name bench.py gives the same dataset, so one is reused
    tag = (f"r{args.rows}_s{args.series}_f{args.ssts}_seed{args.seed}"
           f"_{args.compression}_PLAIN")
    out = os.path.join(args.data_dir, tag)
    meta = os.path.join(out, "dataset.json")
    if os.path.exists(meta):
        with open(meta) as f:
            m = json.load(f)
    else:
        m = gen_dataset(out, args.rows, args.series, args.ssts, seed=args.seed,
                        compression=args.compression, ts_encoding="PLAIN",
                        workers=min(16, os.cpu_count() or 2))
    queries = [("min,max", AGG_MIN | AGG_MAX), ("last", AGG_LAST),
               ("sum,count,last", AGG_SUM | AGG_COUNT | AGG_LAST)]
    res = {"rows": args.rows, "series": args.series, "ssts": args.ssts,
           "compression": args.compression,
           "steps": args.steps, "warmup": args.warmup, "queries": {}}
    with Store(out) as st, st.prepare(middle_range(m), devices=[0]) as p:
        for name, ops in queries:
            res["queries"][name] = timed(p, ops, args.steps, args.warmup)
        ms, route = resolve_kernel_ms(p, AGG_LAST)
        res["rows_scanned"] = p.stats()["rows_scanned"]
    q = res["queries"]
    res["route_of_last"] = route
    res["resolve_kernel_ms"] = ms
    if ms is not None:
        res["ts_pass_kernel_ms"] = q["last"]["kernel_ms"] - ms
    for k in ("kernel_ms", "wall_ms"):
        res[f"last_over_minmax_{k}"] = q["last"][k] / q["min,max"][k]
        res[f"sum_count_last_over_minmax_{k}"] = \
            q["sum,count,last"][k] / q["min,max"][k]
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
