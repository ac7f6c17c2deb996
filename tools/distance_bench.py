#!/usr/bin/env python3
"""te_run_distance on a 4096^2 map at 0.05 m -> profiles/distance_bench.json.  One row per (seeds, cap, route), each timed twice:

  call_ms              host clock around te_run_distance + te_sync: median of --iters calls with p10 and p90
  pass1_ms / pass2_ms  each pass alone, by device events (te_time_distance_samples with TE_DISTANCE_TIME_PASS1 / _PASS2)
  copy_ms              a device copy of the layer (mode 0): 4 B read and 4 B written per cell
  host_ms              (--host, the 10-cell cap) the route a user has without this call: download, an exact capped transform in
                       numpy (the same two passes, vectorised), upload; wall clock, the median of 3
  region rows          te_run_distance_region of one 256^2 tile on a 2048^2 and on an 8192^2 map, host clock as above

Seeds: `none` (0 %), `scatter_0.1` and `scatter_10` (that share of the cells, scattered), `boxes` (200 boxes of 8 .. 64 cells).
Routes: TE_OPT_DISTANCE_ROUTE 1 (tiled wherever it fits) and 2 (the route of any reach).

    python tools/distance_bench.py [--size 4096] [--iters 200] [--host] [--json profiles/distance_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

RES = 0.05
SEEDS = ("none", "scatter_0.1", "scatter_10", "boxes")
CAP_CELLS = (10, 40, 200)
IN, OUT = "traversability", "traversability_roughness"


def layer(size, kind, seed=1):
    """1.0 everywhere, 0.0 on the seeds: [cols][rows] float32"""
    rng = np.random.default_rng(seed)
    a = np.ones((size, size), np.float32)
    if kind.startswith("scatter_"):
        share = float(kind.split("_")[1]) / 100.0
        a.ravel()[rng.choice(a.size, int(a.size * share), replace=False)] = 0.0
    elif kind == "boxes":
        for _ in range(200):
            h, w = rng.integers(8, 65, 2)
            i, j = rng.integers(0, size - h), rng.integers(0, size - w)
            a[j:j + w, i:i + h] = 0.0
    return a


def spread(ms):
    ms = np.asarray(ms, np.float64)
    return {"median": round(float(np.median(ms)), 4), "p10": round(float(np.percentile(ms, 10)), 4), "p90": round(float(np.percentile(ms, 90)), 4)}


def host_clock(call, sync, iters, warmup=5):
    out = []
    for k in range(-warmup, iters):
        t0 = time.perf_counter()
        call()
        sync()
        if k >= 0:
            out.append((time.perf_counter() - t0) * 1e3)
    return spread(out)


def host_transform(a, cells, max_distance):
    """The capped exact transform in numpy: nearest seed along axis 1 by two running scans, then the minimum over the other axis."""
    seed = a < np.float32(0.5)
    n = a.shape[1]
    idx = np.arange(n, dtype=np.int32)[None, :]
    last = np.maximum.accumulate(np.where(seed, idx, -(1 << 20)), axis=1)
    nxt = np.minimum.accumulate(np.where(seed, idx, 1 << 20)[:, ::-1], axis=1)[:, ::-1]
    g = np.minimum(np.minimum(idx - last, nxt - idx), cells + 1).astype(np.int32)
    g2 = g * g
    cap2 = int((max_distance / RES) ** 2)
    best = np.full(a.shape, cap2 + 1, np.int32)
    for d in range(-cells, cells + 1):
        lo, hi = max(0, -d), a.shape[0] - max(0, d)
        np.minimum(best[lo:hi], g2[lo + d:hi + d] + d * d, out=best[lo:hi])
    return np.where(best <= cap2, np.sqrt(best.astype(np.float64)) * RES, max_distance).astype(np.float32)


def whole_map(capi, size, iters, host, rows):
    for kind in SEEDS:
        a = layer(size, kind)
        with capi.Context(0) as ctx:
            ctx.set_params(capi.default_params())
            ctx.set_geometry(size, size, 1, RES)
            ctx.upload_layer(IN, a)
            copy_ms = spread(ctx.time_distance_samples(0, 0.5, 1.0, IN, OUT, iters=iters))
            for cells in CAP_CELLS:
                md = (cells + 0.5) * RES
                for route in (1, 2):
                    ctx.set_option(capi.OPT_DISTANCE_ROUTE, route)
                    for repeat in (0, 1):
                        row = {"size": size, "seeds": kind, "cap_cells": cells, "route_option": route, "repeat": repeat, "copy_ms": copy_ms}
                        row["call_ms"] = host_clock(lambda: ctx.run_distance(capi.DISTANCE_BELOW, 0.5, md, IN, OUT), ctx.sync, iters)
                        row["blocks"] = ctx.distance_stats()
                        n = max(10, iters // 4)
                        row["pass1_ms"] = spread(ctx.time_distance_samples(capi.DISTANCE_BELOW | capi.DISTANCE_TIME_PASS1, 0.5, md, IN, OUT, iters=n))
                        row["pass2_ms"] = spread(ctx.time_distance_samples(capi.DISTANCE_BELOW | capi.DISTANCE_TIME_PASS2, 0.5, md, IN, OUT, iters=n))
                        print(json.dumps(row), flush=True)
                        rows.append(row)
                if host and cells == CAP_CELLS[0]:
                    buf = np.empty(size * size, np.float32)
                    wall = []
                    for _ in range(3):
                        t0 = time.perf_counter()
                        ctx.download_into(IN, buf)
                        ctx.upload_layer(OUT, host_transform(buf.reshape(size, size), cells, md))
                        ctx.sync()
                        wall.append((time.perf_counter() - t0) * 1e3)
                    row = {"size": size, "seeds": kind, "cap_cells": cells, "host_ms": round(float(np.median(wall)), 1)}
                    print(json.dumps(row), flush=True)
                    rows.append(row)


def regions(capi, iters, rows):
    for size in (2048, 8192):
        a = layer(size, "scatter_0.1")
        with capi.Context(0) as ctx:
            ctx.set_params(capi.default_params())
            ctx.set_geometry(size, size, 1, RES)
            ctx.upload_layer(IN, a)
            for cells in CAP_CELLS:
                md = (cells + 0.5) * RES
                ctx.run_distance(capi.DISTANCE_BELOW, 0.5, md, IN, OUT)
                for repeat in (0, 1):
                    r0 = size // 2 - 128
                    row = {"size": size, "seeds": "scatter_0.1", "cap_cells": cells, "region": [r0, r0, 256, 256], "repeat": repeat}
                    row["call_ms"] = host_clock(lambda: ctx.run_distance_region(capi.DISTANCE_BELOW, 0.5, md, IN, OUT, 0, r0, r0, 256, 256), ctx.sync, iters)
                    row["blocks"] = ctx.distance_stats()
                    print(json.dumps(row), flush=True)
                    rows.append(row)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--no-regions", action="store_true")
    ap.add_argument("--json")
    a = ap.parse_args()
    from traversability_estimation_amd import capi
    rows = []
    whole_map(capi, a.size, a.iters, a.host, rows)
    if not a.no_regions:
        regions(capi, a.iters, rows)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
