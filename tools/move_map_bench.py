#!/usr/bin/env python3
"""te_move_map on a resident map, and the robot-centric tick it makes possible, against the route it replaces: 2048^2 and 8192^2
maps at 0.05 m, tie-free radii of 5 cells (results are kept), shifts of (1, 0), (0, 1) and (3, -2) cells.  One process per map
size and shift.  Every figure but the floor is a host clock around the calls and the te_sync that ends them (the calls are
asynchronous), after warm-ups, `--iters` samples: the median with the 10th and 90th percentile as the spread.  That includes
the launches' host cost, which is what a tick pays.  Moves alternate between +shift and -shift, so the map stays where it is.

  move                   te_move_map alone
  tick                   the tick as Context.refresh_moved runs it: the move, the exposed strips uploaded, te_run_chain_region on
                         every rectangle without the footprint flag, one whole-map te_run_footprint (include/travgpu.h, caveat 3)
  tick_region_footprint  the same with TE_RUN_FOOTPRINT on the region runs and no whole-map pass: the footprint layer is then the
                         old position's on the few cells caveat 3 names
  replaced_route         what a move cost before: te_set_geometry to the new position, a whole te_upload_elevation and
                         te_run_chain(TE_RUN_FOOTPRINT); at most 20 samples
  copy_floor             device events around a device-to-device copy of one layer (te_time_median_fill_samples without
                         parameters), times the float layers' worth of bytes a move shifts: the 12 slab layers, the step
                         filter's height layer and the untraversable mask (a quarter layer) -- one read and one write of each

    python tools/move_map_bench.py [--sizes 2048,8192] [--iters 200] [--json profiles/move_map_bench.json]
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
SHIFTS = [(1, 0), (0, 1), (3, -2)]
LAYERS_MOVED = 13.25


def relief(size, seed=1):
    """(cols, rows): smooth relief with sensor noise"""
    rng = np.random.default_rng(seed)
    i = np.arange(size, dtype=np.float32)
    z = (1.0 + 0.3 * np.sin(i / 37.0)[None, :] * np.cos(i / 53.0)[:, None]).astype(np.float32)
    z += (0.02 * rng.standard_normal((size, size), dtype=np.float32))
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
        call(k)
        ctx.sync()
        if k >= 0:
            out.append((time.perf_counter() - t0) * 1e3)
    return stats(out)


def one_case(size, shift, iters):
    from traversability_estimation_amd import capi, synth
    elev = relief(size)
    r = synth.benchmark_radius(5, RES)
    p = capi.default_params(normals_radius=r, rough_radius=r, step_radius1=r, step_radius2=r, fp_radius=r, fp_offset=0.0)
    home = (12.3, -7.1)
    away = (home[0] + shift[0] * RES, home[1] + shift[1] * RES)
    res = {"size": size, "shift": list(shift)}
    with capi.Context(0) as ctx:
        ctx.set_params(p)
        ctx.set_geometry(size, size, 1, RES, home)
        ctx.upload_elevation(elev)
        ctx.run_chain(capi.RUN_FOOTPRINT)
        ctx.sync()
        plan = capi.move_geometry(size, size, RES, home, away, p)
        assert plan.results_kept == 1 and (plan.shift_rows, plan.shift_cols) == tuple(shift)
        res["rects"] = [list(rect) + [int(e)] for rect, e in plan.rectangles()]

        def target(k):  # even samples move away, odd ones home again: the same number of cells either way
            return away if k % 2 == 0 else home

        res["move"] = host_timed(ctx, lambda k: ctx.move_map(*target(k)), 6, iters)

        def strips(info):
            return [np.ascontiguousarray(elev[c0:c0 + w, r0:r0 + h]) if e else None for (r0, c0, h, w), e in info.rectangles()]

        def tick(k):
            info = ctx.move_map(*target(k))
            ctx.refresh_moved(info, capi.RUN_FOOTPRINT, strips(info))

        def tick_region_footprint(k):
            info = ctx.move_map(*target(k))
            for ((r0, c0, h, w), e), t in zip(info.rectangles(), strips(info)):
                if e:
                    ctx.upload_tile(t, 0, r0, c0)
                ctx.run_chain_region(0, r0, c0, h, w, capi.RUN_FOOTPRINT)

        ctx.upload_elevation(elev)  # (the moves above left NaN strips behind)
        ctx.run_chain(capi.RUN_FOOTPRINT)
        res["tick"] = host_timed(ctx, tick, 6, iters)
        res["tick_region_footprint"] = host_timed(ctx, tick_region_footprint, 6, iters)

        def replaced(k):
            ctx.set_geometry(size, size, 1, RES, target(k))
            ctx.upload_elevation(elev)
            ctx.run_chain(capi.RUN_FOOTPRINT)

        res["replaced_route"] = host_timed(ctx, replaced, 2, max(5, min(iters, 20)))
        copy = stats(ctx.time_median_fill_samples(None, "elevation", "traversability_roughness", 3, 20))
        res["copy_one_layer"] = copy
        res["copy_floor_ms"] = round(copy["median_ms"] * LAYERS_MOVED, 4)
        res["move_over_floor"] = round(res["move"]["median_ms"] / res["copy_floor_ms"], 2)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="2048,8192")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--json")
    ap.add_argument("--child")
    a = ap.parse_args()
    if a.child:
        size, kr, kc = (int(v) for v in a.child.split(","))
        print("RESULT " + json.dumps(one_case(size, (kr, kc), a.iters)), flush=True)
        return
    out = {"what": __doc__.split("\n\n")[0].replace("\n", " "), "resolution": RES, "layers_moved": LAYERS_MOVED, "runs": []}
    for size in [int(s) for s in a.sizes.split(",")]:
        for kr, kc in SHIFTS:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "%d,%d,%d" % (size, kr, kc), "--iters", str(a.iters)],
                               capture_output=True, text=True, timeout=600)
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
            if r.returncode != 0 or not line:
                sys.exit("size %d shift (%d, %d) failed (%d):\n%s\n%s" % (size, kr, kc, r.returncode, r.stdout[-2000:], r.stderr[-4000:]))
            out["runs"].append(json.loads(line[0][len("RESULT "):]))
            print(json.dumps(out["runs"][-1]), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
