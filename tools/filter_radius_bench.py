#!/usr/bin/env python3
"""The filters at any radius (TE_OPT_FILTER_ANY_RADIUS, te_filter_any.hip) on a 4096^2 map at 0.01 m: the chain with
normals = roughness = step radii of 20 (option 2: the route forced), 40 and 80 cells, and at 30 cells the forced route
against the generic kernels (TE_RUN_GENERIC_KERNELS).  Every case in a process of its own, the median of event-timed
launches after warm-up (te_time_chain_samples).  Prints one JSON object.  Needs an MI355X."""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from traversability_estimation_amd import capi, synth  # noqa: E402

CASES = [("R20 forced", 20.3, 2, 0), ("R40", 40.3, 1, 0), ("R80", 80.3, 1, 0), ("R30 forced", 30.3, 2, 0),
         ("R30 generic kernels", 30.3, 0, capi.RUN_GENERIC_KERNELS)]


def one(k, n):
    name, cells, option, flags = CASES[k]
    capi.load()
    res = 0.01
    e = synth.with_steps(synth.perlin_elevation(n, n, seed=1234), 200, seed=1235)
    p = capi.default_params()
    p.normals_radius = p.rough_radius = p.step_radius1 = p.step_radius2 = cells * res
    with capi.Context(0) as c:
        c.set_option(capi.OPT_FILTER_ANY_RADIUS, option)
        c.set_params(p)
        c.set_geometry(n, n, 1, res)
        c.upload_elevation(e)
        s = c.time_chain_samples(flags, warmup=2, iters=int(os.environ.get("TE_ITERS", "10")))
    return {"ms": round(float(np.median(s)), 3), "min_ms": round(float(np.min(s)), 3), "cells": cells, "option": option}


def main():
    if "--one" in sys.argv:
        k = sys.argv.index("--one")
        print(json.dumps(one(int(sys.argv[k + 1]), int(sys.argv[k + 2]))))
        return
    n = int(os.environ.get("TE_SIZE", "4096"))
    out = {}
    for k, case in enumerate(CASES):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", str(k), str(n)], capture_output=True, text=True,
                           check=True, timeout=600)
        out[f"{case[0]} {n}x{n}"] = json.loads(r.stdout.strip().splitlines()[-1])
    t40, t80 = out[f"R40 {n}x{n}"]["ms"], out[f"R80 {n}x{n}"]["ms"]
    out["t80/t40"] = round(t80 / t40, 3)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
