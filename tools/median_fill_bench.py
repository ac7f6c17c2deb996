#!/usr/bin/env python3
"""te_run_median_fill on a 4096^2 map at 0.05 m: what the fill costs and what it buys.  Every case runs in a fresh process and
reports the median of event-timed launches after warm-ups (te_time_median_fill_samples / te_time_chain_samples):

  copy_ms          a device copy of the layer: the fill's floor, 4 B read and 4 B written per cell
  fill_ms          the fill alone, elevation -> another layer
  chain_holes_ms   chain + footprint on the UNFILLED map (what a user without the fill pays)
  chain_filled_ms  chain + footprint on the filled map; fill_ms + chain_filled_ms is the route with the fill
  host_ms          (--host) the route a user has today: download, a C-speed numpy median fill of the NaN cells (k = 0), upload

    python tools/median_fill_bench.py [--size 4096] [--iters 50] [--host] [--json out.json]
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
HOLES = ("speckle_0.1", "speckle_1", "unobserved_20")


def elevation(size, holes, seed=1):
    rng = np.random.default_rng(seed)
    i, j = np.meshgrid(np.arange(size, dtype=np.float32), np.arange(size, dtype=np.float32), indexing="ij")
    z = (0.3 * np.sin(i / 37.0) * np.cos(j / 53.0) + 0.02 * rng.standard_normal((size, size))).astype(np.float32)
    if holes.startswith("speckle_"):
        frac = float(holes.split("_")[1]) / 100.0
        z.ravel()[rng.choice(z.size, int(frac * z.size), replace=False)] = np.nan
    elif holes == "unobserved_20":  # blobs, the way an elevation map is unobserved behind obstacles
        n_blobs = 400
        ci, cj = rng.integers(0, size, n_blobs), rng.integers(0, size, n_blobs)
        side = int(size * (0.2 / n_blobs) ** 0.5)
        for a, b in zip(ci, cj):
            z[a:a + side, b:b + side] = np.nan
    return z


def host_fill(z, r):
    """Median of the finite values in the square window for every NaN cell (k = 0), vectorised over the holes."""
    out = z.copy()
    idx = np.argwhere(~np.isfinite(z))
    pad = np.pad(z, r, constant_values=np.nan)
    for lo in range(0, len(idx), 1 << 16):
        part = idx[lo:lo + (1 << 16)]
        win = np.stack([pad[part[:, 0] + di, part[:, 1] + dj] for di in range(2 * r + 1) for dj in range(2 * r + 1)], 1)
        win = np.where(np.isfinite(win), win, np.inf)
        win.sort(1)
        n = np.isfinite(win).sum(1)
        ok = n > 0
        out[part[ok, 0], part[ok, 1]] = win[ok, n[ok] // 2]
    return out


def one_case(size, holes, r, k, iters, host):
    from traversability_estimation_amd import capi
    z = elevation(size, holes)
    p = capi.default_median_fill_params(fill_hole_radius=(r + 0.5) * RES, num_erode_dilation_iterations=k)
    med = lambda ms: float(np.median(ms))
    res = {"size": size, "holes": holes, "r": r, "k": k, "invalid": int((~np.isfinite(z)).sum())}
    with capi.Context(0) as ctx:
        ctx.set_params(capi.default_params())
        ctx.set_geometry(size, size, 1, RES)
        ctx.upload_elevation(z.T)
        res["copy_ms"] = med(ctx.time_median_fill_samples(None, iters=iters))
        res["fill_ms"] = med(ctx.time_median_fill_samples(p, iters=iters))
        res["chain_holes_ms"] = med(ctx.time_chain_samples(capi.RUN_FOOTPRINT, 5, iters))
        ctx.run_median_fill(p)
        left = ctx.download("elevation")
        res["invalid_after"] = int((~np.isfinite(left)).sum())
        res["chain_filled_ms"] = med(ctx.time_chain_samples(capi.RUN_FOOTPRINT, 5, iters))
        res["fill_plus_chain_ms"] = res["fill_ms"] + res["chain_filled_ms"]
        if host:
            buf = np.empty(size * size, np.float32)
            t0 = time.perf_counter()
            ctx.upload_elevation(z.T)  # (the unfilled layer is resident again)
            t1 = time.perf_counter()
            ctx.download_into("elevation", buf)
            filled = host_fill(buf.reshape(size, size), r)
            ctx.upload_elevation(filled)
            res["host_ms"] = (time.perf_counter() - t1) * 1e3
            res["host_upload_only_ms"] = (t1 - t0) * 1e3
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--json")
    ap.add_argument("--case", nargs=3, metavar=("HOLES", "R", "K"), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.case:
        one_case(a.size, a.case[0], int(a.case[1]), int(a.case[2]), a.iters, a.host)
        return 0
    rows = []
    for holes in HOLES:
        for r in (2, 3):
            for k in (0, 4):
                cmd = [sys.executable, os.path.abspath(__file__), "--size", str(a.size), "--iters", str(a.iters), "--case", holes, str(r), str(k)]
                out = subprocess.run(cmd + (["--host"] if a.host and k == 0 and r == 2 else []), capture_output=True, text=True, timeout=600)
                if out.returncode != 0:
                    print(out.stdout + out.stderr, file=sys.stderr)
                    return 1
                line = out.stdout.strip().splitlines()[-1]
                print(line, flush=True)
                rows.append(json.loads(line))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
