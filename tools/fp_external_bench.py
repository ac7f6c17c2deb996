"""te_run_footprint over an UPLOADED traversability layer (no bound: the route of any reach; before the route plan knew
the double kernels' bound, k_fp_slide3): ms per pass on one 4096^2 map, tie-free R = 9.  No bench.py configuration covers it.
A/B two builds on the same box, each in a process of its own:  TRAVGPU_LIB=<other libtravgpu.so> python tools/fp_external_bench.py
Prints one JSON line."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from traversability_estimation_amd import capi, synth  # noqa: E402


def main(n=4096, res=0.05, warmup=5, iters=30, repeats=7):
    capi.load()
    r = synth.benchmark_radius(3, res)
    p = capi.default_params(normals_radius=r, rough_radius=r, step_radius1=r, step_radius2=r,
                            fp_radius=synth.benchmark_radius(6, res), fp_offset=synth.benchmark_radius(3, res))
    elev = synth.with_steps(synth.perlin_elevation(n, n, seed=1, amplitude=0.12), 30, seed=2)
    t = np.random.default_rng(3).uniform(0.0, 1.0, n * n).astype(np.float32)  # (in range for both builds: only the time is compared)
    with capi.Context(0) as ctx:
        ctx.set_params(p)
        ctx.set_geometry(n, n, 1, res)
        ctx.upload_elevation(elev)
        ctx.run_chain(0)
        ctx.upload_layer("traversability", t)
        for _ in range(warmup):
            ctx.run_footprint()
        ctx.sync()
        ms = []
        for _ in range(repeats):
            t0 = time.perf_counter()
            for _ in range(iters):
                ctx.run_footprint()
            ctx.sync()
            ms.append((time.perf_counter() - t0) * 1e3 / iters)
        fp = ctx.download("traversability_footprint")
    print(json.dumps({"what": "te_run_footprint, uploaded layer, 4096^2, tie-free R = 9 (mask + sum)", "lib": capi.LIB_PATH,
                      "ms_per_pass_median": round(float(np.median(ms)), 4), "ms_per_pass_min": round(min(ms), 4),
                      "ms_per_pass_max": round(max(ms), 4), "checksum": float(np.nansum(fp.astype(np.float64)))}))


if __name__ == "__main__":
    main()
