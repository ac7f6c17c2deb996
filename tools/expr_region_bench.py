#!/usr/bin/env python3
"""The region forms of the two expression filters on a resident map: te_run_window_expression_region, te_run_expression_region
and te_run_chain_region_expression on one 256 x 256 dirty tile of a 2048^2 and of an 8192^2 map at 0.05 m with 1 % NaN.  One
process per map size.  Every region figure is a host clock around the call and the te_sync that ends it (the calls are
asynchronous), after warm-ups, `--iters` samples: the median with the 10th and 90th percentile as the spread.  That includes the
launches' host cost, which is what a tick pays.

  window_std_w5 / _w21, window_mean_w5 / _w21   te_run_window_expression_region: the local standard deviation and
                                 meanOfFinites at w = 5 and 21, edge handling crop
  whole_window_*                 the whole-map calls in the same run: device events (te_time_window_expression_samples)
  expr_region                    te_run_expression_region of cwiseMin of the three scores on the tile
  tick_one_call                  te_upload_tile, then te_run_chain_region_expression with the footprint flag, te_sync
  tick_workaround                the route without it: te_upload_tile, te_run_chain_region without the flag, the whole-map
                                 te_run_expression, the whole-map te_run_footprint, te_sync
  tick_weighted                  te_upload_tile, te_run_chain_region with the footprint flag (the weighted sum), te_sync
  scales_with_map                per region case: whether the 8192^2 median lies above the 2048^2 90th percentile

    python tools/expr_region_bench.py [--sizes 2048,8192] [--tile 256] [--iters 200] [--json profiles/expr_region_bench.json]
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
HOLD, OUT = "robot_slope", "step_footprint"
STD_DEV = "sqrt(sumOfFinites(square(robot_slope - meanOfFinites(robot_slope))) ./ numberOfFinites(robot_slope))"
MEAN = "meanOfFinites(robot_slope)"
CWISE_MIN = "cwiseMin(cwiseMin(traversability_slope, traversability_step), traversability_roughness)"


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
    from traversability_estimation_amd import capi, synth
    raw = raw_map(size)
    r0 = c0 = (size - tile) // 2 + 7  # (off the workgroup grid of the whole-map calls)
    rng = np.random.default_rng(2)
    patch = raw[c0:c0 + tile, r0:r0 + tile] + (0.01 * rng.standard_normal((tile, tile), dtype=np.float32))
    res = {"size": size, "tile": tile, "tile_origin": [r0, c0]}
    whole_iters = max(5, min(iters, 20))
    radius = synth.benchmark_radius(5, RES)  # tie-free discs of 5 cells: the region footprint is defined at this resolution
    with capi.Context(0) as ctx:
        ctx.set_params(capi.default_params(normals_radius=radius, rough_radius=radius, step_radius1=radius, step_radius2=radius, fp_radius=radius, fp_offset=0.0))
        ctx.set_geometry(size, size, 1, RES)
        ctx.upload_layer(HOLD, raw)
        for name, text in (("std", STD_DEV), ("mean", MEAN)):
            for w in (5, 21):
                p = capi.window_expr_params(window_size=w, edge_handling="crop")
                key = "window_%s_w%d" % (name, w)
                ctx.run_window_expression(text, p, HOLD, OUT)
                res[key] = host_timed(ctx, lambda: ctx.run_window_expression_region(text, p, HOLD, OUT, 0, r0, c0, tile, tile), 10, iters)
                res[key]["out_rect"] = list(ctx.run_window_expression_region(text, p, HOLD, OUT, 0, r0, c0, tile, tile))
                res[key]["blocks_separable_direct"] = list(ctx.window_expression_stats())
                res["whole_" + key] = stats(ctx.time_window_expression_samples(text, p, HOLD, OUT, 2, whole_iters))
        ctx.upload_elevation(np.nan_to_num(raw, nan=1.0))
        ctx.run_chain()
        ctx.run_expression(CWISE_MIN)
        ctx.run_footprint()
        ctx.sync()
        res["expr_region"] = host_timed(ctx, lambda: ctx.run_expression_region(CWISE_MIN, 0, r0, c0, tile, tile), 10, iters)
        clean = np.nan_to_num(patch, nan=1.0)

        def tick_one_call():
            ctx.upload_tile(clean, 0, r0, c0)
            ctx.run_chain_region_expression(CWISE_MIN, 0, r0, c0, tile, tile, capi.RUN_FOOTPRINT)

        def tick_workaround():
            ctx.upload_tile(clean, 0, r0, c0)
            ctx.run_chain_region(0, r0, c0, tile, tile)
            ctx.run_expression(CWISE_MIN)
            ctx.run_footprint()

        res["tick_one_call"] = host_timed(ctx, tick_one_call, 5, iters)
        res["tick_workaround"] = host_timed(ctx, tick_workaround, 2, whole_iters)
        ctx.run_chain(capi.RUN_FOOTPRINT)  # the weighted sum again, a complete footprint layer over it
        ctx.sync()

        def tick_weighted():
            ctx.upload_tile(clean, 0, r0, c0)
            ctx.run_chain_region(0, r0, c0, tile, tile, capi.RUN_FOOTPRINT)

        res["tick_weighted"] = host_timed(ctx, tick_weighted, 5, iters)
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
                                  if isinstance(small[k], dict) and not k.startswith("whole_") and k != "tick_workaround"}
        print(json.dumps({"scales_with_map": out["scales_with_map"]}), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
