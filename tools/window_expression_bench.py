#!/usr/bin/env python3
"""te_run_window_expression on a 4096^2 map at 0.05 m, edge handling `crop`.  Per expression and window the median of event-timed
launches after warm-ups (te_time_window_expression_samples):

  copy_ms       a device copy of the layer: the floor, 4 B read and 4 B written per cell
  plan_ms       TE_OPT_WINDOW_EXPR_ROUTE 0: the route the plan names
  separable_ms  route 1: the separable route wherever allowed (the standard deviation nests a reduction: it walks directly)
  direct_ms     route 2: the direct walk
  blocks        (separable, direct) workgroups by plan
  host_ms       (--host, w = 5) the route a user has today: download, numpy over the window, upload; wall clock, the median of 3

Expressions: `std_dev`, the local standard deviation of the filter chains, and `box_mean`, meanOfFinites(elevation).

    python tools/window_expression_bench.py [--size 4096] [--iters 20] [--host] [--json out.json]
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
WINDOWS = (3, 5, 9, 21)
HOST_WINDOW = 5
TEXTS = {"std_dev": "sqrt(sumOfFinites(square(elevation - meanOfFinites(elevation))) ./ numberOfFinites(elevation))",
         "box_mean": "meanOfFinites(elevation)"}


def elevation(size, seed=1):
    rng = np.random.default_rng(seed)
    i, j = np.meshgrid(np.arange(size, dtype=np.float32), np.arange(size, dtype=np.float32), indexing="ij")
    z = (1.0 + 0.3 * np.sin(i / 37.0) * np.cos(j / 53.0) + 0.02 * rng.standard_normal((size, size))).astype(np.float32)
    z.ravel()[rng.choice(z.size, z.size // 100, replace=False)] = np.nan
    return z


def host_window(z, w, kind):
    """numpy over the cropped window: counts and sums of the finite values by shifted views."""
    m = (w - 1) // 2
    pad = np.pad(z, m, constant_values=np.nan)
    ok = np.isfinite(pad)
    v = np.where(ok, pad, 0.0).astype(np.float64)
    total, square, count = np.zeros(z.shape), np.zeros(z.shape), np.zeros(z.shape, np.int32)
    for di in range(w):
        for dj in range(w):
            s = v[di:di + z.shape[0], dj:dj + z.shape[1]]
            total += s
            square += s * s
            count += ok[di:di + z.shape[0], dj:dj + z.shape[1]]
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = total / count
        out = mean if kind == "box_mean" else np.sqrt(np.maximum(square / count - mean * mean, 0.0))
    return out.astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--json")
    a = ap.parse_args()
    from traversability_estimation_amd import capi
    z = elevation(a.size)
    med = lambda ms: round(float(np.median(ms)), 4)
    rows = []
    with capi.Context(0) as ctx:
        ctx.set_params(capi.default_params())
        ctx.set_geometry(a.size, a.size, 1, RES)
        ctx.upload_elevation(z.T)
        copy_ms = med(ctx.time_window_expression_samples(None, None, iters=a.iters))
        for kind, text in TEXTS.items():
            for w in WINDOWS:
                p = capi.window_expr_params(window_size=w, edge_handling="crop", compute_empty_cells=kind == "box_mean")
                res = {"size": a.size, "expression": kind, "w": w, "copy_ms": copy_ms}
                for route, tag in ((0, "plan"), (1, "separable"), (2, "direct")):
                    ctx.set_option(capi.OPT_WINDOW_EXPR_ROUTE, route)
                    n = a.iters if w < 21 else max(3, a.iters // 4)
                    res[tag + "_ms"] = med(ctx.time_window_expression_samples(text, p, iters=n, warmup=2))
                    if route == 0:
                        res["blocks"] = ctx.window_expression_stats()
                ctx.set_option(capi.OPT_WINDOW_EXPR_ROUTE, 0)
                if a.host and w == HOST_WINDOW:
                    buf = np.empty(a.size * a.size, np.float32)
                    wall = []
                    for _ in range(3):
                        t0 = time.perf_counter()
                        ctx.download_into("elevation", buf)
                        ctx.upload_layer("traversability_roughness", host_window(buf.reshape(a.size, a.size), w, kind))
                        wall.append((time.perf_counter() - t0) * 1e3)
                    res["host_ms"] = round(float(np.median(wall)), 1)
                print(json.dumps(res), flush=True)
                rows.append(res)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
