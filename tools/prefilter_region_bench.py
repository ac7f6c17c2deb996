#!/usr/bin/env python3
"""The region forms of the pre-filters on a resident map: te_run_median_fill_region and te_run_radius_filter_region on one
256 x 256 dirty tile of a 2048^2 and of an 8192^2 map at 0.05 m with 1 % NaN (BASELINE config 5's shape).  One process per map
size.  Every region figure is a host clock around the call and the te_sync that ends it (the calls are asynchronous), after
warm-ups, `--iters` samples: the median with the 10th and 90th percentile as the spread.  That includes the launches' host cost,
which is what a tick pays.

  fill_r2_k0 / fill_r2_k4        te_run_median_fill_region, fill_hole_radius 2 cells, 0 / 4 opening iterations
  mean_1.5 / mean_3              te_run_radius_filter_region, Mean at 1.5 / 3 cells
  whole_*                        the whole-map calls in the same run: device events (te_time_median_fill_samples,
                                 te_time_radius_filter_samples)
  tick_region                    the tile into the holding layer (te_upload_layer_tile), region fill, region mean into the
                                 elevation, te_run_chain_region on the last out_rect, te_sync
  tick_whole                     what the incremental chain costs without the region calls: the tile into the holding layer, the
                                 whole-map fill and mean into a spare layer, out_rect of it moved into the elevation
                                 (te_download_tile + te_upload_tile), te_run_chain_region, te_sync
  scales_with_map                per region case: whether the 8192^2 median lies above the 2048^2 90th percentile

    python tools/prefilter_region_bench.py [--sizes 2048,8192] [--tile 256] [--iters 200] [--json profiles/prefilter_region_bench.json]
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
HOLD, MID, SPARE = "robot_slope", "traversability_footprint", "step_footprint"


def raw_map(size, seed=1):
    """(cols, rows): smooth relief with sensor noise, 1 % NaN"""
    rng = np.random.default_rng(seed)
    i = np.arange(size, dtype=np.float32)
    z = (1.0 + 0.3 * np.sin(i / 37.0)[None, :] * np.cos(i / 53.0)[:, None]).astype(np.float32)
    z += (0.02 * rng.standard_normal((size, size), dtype=np.float32))
    z.ravel()[rng.integers(0, z.size, z.size // 100)] = np.nan
    return z


def stats(ms):
    ms = np.asarray(ms, np.float64)
    return {"median_ms": round(float(np.median(ms)), 4), "p10_ms": round(float(np.percentile(ms, 10)), 4), "p90_ms": round(float(np.percentile(ms, 90)), 4),
            "samples": int(ms.size)}


def host_timed(ctx, call, warmup, iters):
    out = []
    for k in range(-warmup, iters):
        ctx.sync()
        t0 = time.perf_counter()
        call()
        ctx.sync()
        if k >= 0:
            out.append((time.perf_counter() - t0) * 1e3)
    return stats(out)


def one_size(size, tile, iters):
    from traversability_estimation_amd import capi
    raw = raw_map(size)
    r0 = c0 = (size - tile) // 2 + 7  # (off the workgroup grid of the whole-map calls)
    rng = np.random.default_rng(2)
    patch = raw[c0:c0 + tile, r0:r0 + tile] + (0.01 * rng.standard_normal((tile, tile), dtype=np.float32))
    fills = {"r2_k0": capi.default_median_fill_params(fill_hole_radius=2.5 * RES, num_erode_dilation_iterations=0),
             "r2_k4": capi.default_median_fill_params(fill_hole_radius=2.5 * RES, num_erode_dilation_iterations=4)}
    res = {"size": size, "tile": tile, "tile_origin": [r0, c0]}
    whole_iters = max(5, min(iters, 20))
    with capi.Context(0) as ctx:
        ctx.set_params(capi.default_params())
        ctx.set_geometry(size, size, 1, RES)
        ctx.upload_layer(HOLD, raw)
        for name, p in fills.items():
            ctx.run_median_fill(p, HOLD, MID)
            res["fill_" + name] = host_timed(ctx, lambda: ctx.run_median_fill_region(p, HOLD, MID, 0, r0, c0, tile, tile), 10, iters)
            res["fill_" + name]["out_rect"] = list(ctx.run_median_fill_region(p, HOLD, MID, 0, r0, c0, tile, tile))
            res["whole_fill_" + name] = stats(ctx.time_median_fill_samples(p, HOLD, MID, 2, whole_iters))
        p = fills["r2_k4"]
        for cells in (1.5, 3.0):
            name = "%g" % cells
            ctx.run_radius_filter("mean", cells * RES, MID, SPARE)
            res["mean_" + name] = host_timed(ctx, lambda: ctx.run_radius_filter_region("mean", cells * RES, MID, SPARE, 0, r0, c0, tile, tile), 10, iters)
            res["mean_" + name]["blocks_slide_gather"] = list(ctx.radius_filter_stats())
            res["whole_mean_" + name] = stats(ctx.time_radius_filter_samples(capi.RADIUS_MEAN, cells * RES, MID, SPARE, 2, whole_iters))
        # the full tick: fill, mean at 1.5 cells into the elevation, the chain around it
        ctx.run_median_fill(p, HOLD, MID)
        ctx.run_radius_filter("mean", 1.5 * RES, MID, "elevation")
        ctx.run_chain()
        ctx.sync()

        def tick_region():
            ctx.upload_layer_tile(HOLD, patch, 0, r0, c0)
            filled = ctx.run_median_fill_region(p, HOLD, MID, 0, r0, c0, tile, tile)
            smoothed = ctx.run_radius_filter_region("mean", 1.5 * RES, MID, "elevation", 0, *filled)
            ctx.run_chain_region(0, *smoothed)

        res["tick_region"] = host_timed(ctx, tick_region, 5, iters)
        reach = 2 + 2 * 4 + 1
        lo, hi = max(r0 - reach, 0), min(r0 + tile + reach, size)

        def tick_whole():
            ctx.upload_layer_tile(HOLD, patch, 0, r0, c0)
            ctx.run_median_fill(p, HOLD, MID)
            ctx.run_radius_filter("mean", 1.5 * RES, MID, SPARE)
            ctx.upload_tile(ctx.download_tile(SPARE, 0, lo, lo, hi - lo, hi - lo), 0, lo, lo)
            ctx.run_chain_region(0, lo, lo, hi - lo, hi - lo)

        res["tick_whole"] = host_timed(ctx, tick_whole, 2, whole_iters)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="2048,8192")
    ap.add_argument("--tile", type=int, default=256)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--json")
    ap.add_argument("--child", type=int)
    a = ap.parse_args()
    if a.child:
        print("RESULT " + json.dumps(one_size(a.child, a.tile, a.iters)), flush=True)
        return
    out = {"what": __doc__.split("\n\n")[0].replace("\n", " "), "resolution": RES, "runs": []}
    for size in [int(s) for s in a.sizes.split(",")]:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(size), "--tile", str(a.tile), "--iters", str(a.iters)],
                           capture_output=True, text=True, timeout=900)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            sys.exit("size %d failed (%d):\n%s\n%s" % (size, r.returncode, r.stdout[-2000:], r.stderr[-4000:]))
        out["runs"].append(json.loads(line[0][len("RESULT "):]))
        print(json.dumps(out["runs"][-1]), flush=True)
    if len(out["runs"]) >= 2:
        small, large = out["runs"][0], out["runs"][-1]
        out["scales_with_map"] = {k: bool(large[k]["median_ms"] > small[k]["p90_ms"]) for k in small
                                  if isinstance(small[k], dict) and not k.startswith("whole_") and k != "tick_whole"}
        print(json.dumps({"scales_with_map": out["scales_with_map"]}), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
