#!/usr/bin/env python3
"""te_run_components / te_run_reachable on a 4096^2 map at 0.05 m -> profiles/components_bench.json.  One row per (input,
connectivity, call), each measured in two runs:

  call_ms   host clock around the call + te_sync: median of --iters calls with p10 and p90
  copy_ms   the same clock around a device copy of the layer (te_copy_layer): 4 B read and 4 B written per cell
  host_ms   (--host) the route a user has without these calls: download, scipy.ndimage.label and the sizes by bincount,
            upload; wall clock, the median of 3
  stats     te_components_stats after the call: components, free cells, the largest component, cells written 1.0

Inputs: `all_free`; `random_593` (random free cells at 59.3 %, the site-percolation threshold of the square lattice); `spiral`
(one corridor of width 1 wound to the centre: the longest chain); `boxes` (200 blocked boxes of 8 .. 64 cells).  te_run_reachable
starts from one cell, (0, 0), which every input leaves free.

    python tools/components_bench.py [--size 4096] [--iters 200] [--host] [--json profiles/components_bench.json]
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
INPUTS = ("all_free", "random_593", "spiral", "boxes")
IN, OUT = "traversability", "traversability_roughness"


def layer(size, kind, seed=1):
    """1.0 on the free cells, 0.0 on the blocked ones: [cols][rows] float32"""
    rng = np.random.default_rng(seed)
    a = np.ones((size, size), np.float32)
    if kind == "random_593":
        a = (rng.random((size, size)) < 0.593).astype(np.float32)
    elif kind == "spiral":
        i, j = np.indices((size, size))
        inset = np.minimum(np.minimum(i, j), np.minimum(size - 1 - i, size - 1 - j))
        a = (inset % 2 == 0).astype(np.float32)
        for k in range(0, size // 2 - 2, 2):  # every ring is cut behind its first corner and led into the next one
            a[k, k + 1] = 0.0
            a[k + 1, k + 2] = 1.0
    elif kind == "boxes":
        for _ in range(200):
            h, w = rng.integers(8, 65, 2)
            i, j = rng.integers(0, size - h), rng.integers(0, size - w)
            a[j:j + w, i:i + h] = 0.0
    a[0, 0] = 1.0
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


def host_sizes(a, connectivity):
    from scipy import ndimage
    lab, _n = ndimage.label(a >= np.float32(0.5), structure=np.ones((3, 3)) if connectivity == 8 else None)
    counts = np.bincount(lab.ravel())
    counts[0] = 0
    return counts[lab].astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--json")
    a = ap.parse_args()
    from traversability_estimation_amd import capi
    size, rows = a.size, []
    for kind in INPUTS:
        v = layer(size, kind)
        with capi.Context(0) as ctx:
            ctx.set_params(capi.default_params())
            ctx.set_geometry(size, size, 1, RES)
            ctx.upload_layer(IN, v)
            for repeat in (0, 1):
                copy_ms = host_clock(lambda: ctx.copy_layer(IN, OUT), ctx.sync, a.iters)
                for conn in (4, 8):
                    for call in ("components", "reachable"):
                        if call == "components":
                            run = lambda: ctx.run_components(capi.DISTANCE_BELOW, 0.5, conn, IN, OUT)
                        else:
                            run = lambda: ctx.run_reachable(capi.DISTANCE_BELOW, 0.5, [(0, 0)], conn, IN, OUT)
                        row = {"size": size, "input": kind, "connectivity": conn, "call": call, "repeat": repeat, "copy_ms": copy_ms}
                        row["call_ms"] = host_clock(run, ctx.sync, a.iters)
                        row["stats"] = ctx.components_stats()
                        print(json.dumps(row), flush=True)
                        rows.append(row)
            if a.host:
                buf = np.empty(size * size, np.float32)
                for conn in (4, 8):
                    wall = []
                    for _ in range(3):
                        t0 = time.perf_counter()
                        ctx.download_into(IN, buf)
                        ctx.upload_layer(OUT, host_sizes(buf.reshape(size, size), conn))
                        ctx.sync()
                        wall.append((time.perf_counter() - t0) * 1e3)
                    row = {"size": size, "input": kind, "connectivity": conn, "call": "host", "host_ms": round(float(np.median(wall)), 1)}
                    print(json.dumps(row), flush=True)
                    rows.append(row)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
