#!/usr/bin/env python3
"""The reference's DEFAULT parameters (robot_footprint_parameter.yaml: radius 0.30 m + offset 0.15 m) on 4096^2 maps at the
fine resolutions elevation_mapping is also run at: 0.02 m (reach 22 cells) and 0.01 m (reach 45 cells, a tie radius), where
the circular footprint pass takes the route of any reach (te_footprint_any.hip).  Event-timed launches, chain and chain +
footprint, on a Perlin map and on the same map with 400 raised / lowered boxes (discs with untraversable cells: the
spiral walks).  Every case in a process of its own (tools/defaults_bench.py says why).  Prints one JSON object.  Needs an
MI355X."""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from traversability_estimation_amd import capi, synth  # noqa: E402


def one(res, n, boxes):
    capi.load()
    e = synth.perlin_elevation(n, n, seed=1234)
    if boxes:
        e = synth.with_steps(e, boxes, seed=1235)
    with capi.Context(0) as c:
        c.set_params(capi.default_params())
        c.set_geometry(n, n, 1, res)
        c.upload_elevation(e)
        row = {}
        for name, flags in (("chain", 0), ("chain+footprint", capi.RUN_FOOTPRINT)):
            s = c.time_chain_samples(flags, warmup=5, iters=30)
            row[name] = {"ms": round(float(np.median(s)), 4), "cells_per_s": round(n * n / (float(np.median(s)) * 1e-3))}
        c.sync()
        fp = c.download("traversability_footprint")
        row["footprint_zero_frac"] = round(float((fp == 0).mean()), 4)
    return row


def main():
    if "--one" in sys.argv:
        k = sys.argv.index("--one")
        print(json.dumps(one(float(sys.argv[k + 1]), int(sys.argv[k + 2]), int(sys.argv[k + 3]))))
        return
    n = int(os.environ.get("TE_SIZE", "4096"))
    out = {}
    for res in (0.02, 0.01):
        for boxes in (0, 400):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", str(res), str(n), str(boxes)], capture_output=True,
                               text=True, check=True, timeout=600)
            out[f"res {res} {n}x{n} boxes {boxes}"] = json.loads(r.stdout.strip().splitlines()[-1])
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
