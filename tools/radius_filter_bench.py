#!/usr/bin/env python3
"""te_run_radius_filter on a 4096^2 map at 0.05 m.  Every map kind runs in a fresh process and reports, per radius, the median of
event-timed launches after warm-ups (te_time_radius_filter_samples):

  copy_ms              a device copy of the layer: the floor, 4 B read and 4 B written per cell
  mean_ms / min_ms     by plan (TE_OPT_RADIUS_ROUTE 0: the sliding kernels)
  mean_gather_ms / min_gather_ms   the in-order gather (route 2)
  mean_blocks          (sliding, gather) workgroups of the Mean by plan: how many the predicate handed to the gather
  chain_any_ms         the WHOLE chain (te_time_chain_samples) with all four filter radii at this radius on the route of any radius
                       (TE_OPT_FILTER_ANY_RADIUS 2, as tools/filter_radius_bench.py times it): k_fa_step_height, the nearest existing
                       kernel, is one of its kernels; no entry point times it alone
  host_ms              (--host, 1.5 and 3 cells) the route a user has today: download, a numpy mean over the disc, upload;
                       wall clock, the median of 3

Maps: `clean`; `speckle_1` (1 % NaN); `crossing` (the surface crosses zero: tiny values beside ordinary ones).

    python tools/radius_filter_bench.py [--size 4096] [--iters 30] [--host] [--json out.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

RES = 0.05
MAPS = ("clean", "speckle_1", "crossing")
CELLS = (0.0, 0.5, 1.5, 3.0, 9.0, 20.0)
HOST_CELLS = (1.5, 3.0)


def elevation(size, kind, seed=1):
    rng = np.random.default_rng(seed)
    i, j = np.meshgrid(np.arange(size, dtype=np.float32), np.arange(size, dtype=np.float32), indexing="ij")
    z = (0.3 * np.sin(i / 37.0) * np.cos(j / 53.0) + 0.02 * rng.standard_normal((size, size))).astype(np.float32)
    if kind == "clean":
        z += np.float32(1.0)
    elif kind == "speckle_1":
        z += np.float32(1.0)
        z.ravel()[rng.choice(z.size, z.size // 100, replace=False)] = np.nan
    return z  # crossing: as it is, around zero


def host_mean(z, cells):
    r = int(np.floor(cells))
    pad = np.pad(z, r, constant_values=np.nan)
    total, count = np.zeros(z.shape, np.float64), np.zeros(z.shape, np.int32)
    for di in range(-r, r + 1):
        for dj in range(-r, r + 1):
            if di * di + dj * dj <= cells * cells:
                v = pad[r + di:r + di + z.shape[0], r + dj:r + dj + z.shape[1]]
                ok = np.isfinite(v)
                total += np.where(ok, v, 0.0)
                count += ok
    with np.errstate(invalid="ignore", divide="ignore"):
        return (total / count).astype(np.float32)


def chain_any(size, z, cells, iters):
    """The whole chain with every filter disc at `cells` on the route of any radius (k_fa_step_height among its kernels)."""
    from traversability_estimation_amd import capi
    p = capi.default_params()
    p.normals_radius = p.rough_radius = p.step_radius1 = p.step_radius2 = cells * RES
    with capi.Context(0) as c:
        c.set_option(capi.OPT_FILTER_ANY_RADIUS, 2)
        c.set_params(p)
        c.set_geometry(size, size, 1, RES)
        c.upload_elevation(z.T)
        return round(float(np.median(c.time_chain_samples(0, 2, iters))), 4)


def one_case(size, kind, iters, host):
    from traversability_estimation_amd import capi
    z = elevation(size, kind)
    med = lambda ms: round(float(np.median(ms)), 4)
    with capi.Context(0) as ctx:
        ctx.set_params(capi.default_params())
        ctx.set_geometry(size, size, 1, RES)
        ctx.upload_elevation(z.T)
        copy_ms = med(ctx.time_radius_filter_samples(0, 0.0, iters=iters))
        for cells in CELLS:
            res = {"size": size, "map": kind, "cells": cells, "copy_ms": copy_ms}
            for route, tag in ((0, ""), (2, "_gather")):
                ctx.set_option(capi.OPT_RADIUS_ROUTE, route)
                n = iters if route == 0 or cells < 9 else max(3, iters // 6)
                res["mean" + tag + "_ms"] = med(ctx.time_radius_filter_samples(capi.RADIUS_MEAN, cells * RES, iters=n))
                if route == 0:
                    res["mean_blocks"] = ctx.radius_filter_stats()
                res["min" + tag + "_ms"] = med(ctx.time_radius_filter_samples(capi.RADIUS_MIN, cells * RES, iters=n))
            if host and cells in HOST_CELLS:
                buf = np.empty(size * size, np.float32)
                wall = []
                for _ in range(3):
                    t0 = time.perf_counter()
                    ctx.download_into("elevation", buf)
                    ctx.upload_elevation(host_mean(buf.reshape(size, size), cells))
                    wall.append((time.perf_counter() - t0) * 1e3)
                    ctx.upload_elevation(z.T)
                res["host_ms"] = round(float(np.median(wall)), 1)
            if cells >= 1.0 and kind == "clean":
                res["chain_any_ms"] = chain_any(size, z, cells, max(3, iters // 4))
            print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--json")
    ap.add_argument("--case", metavar="MAP", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.case:
        one_case(a.size, a.case, a.iters, a.host)
        return 0
    rows = []
    for kind in MAPS:
        cmd = [sys.executable, os.path.abspath(__file__), "--size", str(a.size), "--iters", str(a.iters), "--case", kind]
        out = subprocess.run(cmd + (["--host"] if a.host and kind == "clean" else []), capture_output=True, text=True, timeout=900)
        if out.returncode != 0:
            print(out.stdout + out.stderr, file=sys.stderr)
            return 1
        for line in out.stdout.strip().splitlines():
            print(line, flush=True)
            rows.append(json.loads(line))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
