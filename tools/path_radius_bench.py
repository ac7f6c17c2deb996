#!/usr/bin/env python3
"""A CheckFootprintPath request of P circular paths with k distinct radii on one resident 4096^2 map, timed two ways:
  dense      per radius te_set_params, te_run_footprint and te_check_footprint_paths on the paths of that radius;
  on_demand  one te_check_footprint_paths_radius for the whole request.
P in {1, 100, 10000}, k in {1, 4}, resolutions 0.05 and 0.02 m.  Paths are planner-sized: 2 to 6 poses, steps of up to 1 m.
Every case in a process of its own; wall-clock time of the synchronous calls around a te_sync, the median of TE_ITERS
repetitions after two warm-up rounds.  Prints one JSON object.  Needs an MI355X."""
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from traversability_estimation_amd import capi, synth  # noqa: E402

RADII = (0.3, 0.2, 0.45, 0.6)
CASES = [(res, P, k) for res in (0.05, 0.02) for P in (1, 100, 10000) for k in (1, 4)]


def make_paths(rng, n, res, count):
    half = 0.5 * n * res
    paths = []
    for _ in range(count):
        m = int(rng.integers(2, 7))
        p = np.cumsum(np.vstack([rng.uniform(-0.9 * half, 0.9 * half, (1, 2)), rng.uniform(-1.0, 1.0, (m - 1, 2))]), axis=0)
        paths.append(np.clip(p, -0.99 * half, 0.99 * half))
    return paths


def one(idx, n):
    res, P, k = CASES[idx]
    capi.load()
    rng = np.random.default_rng(100 + idx)
    e = synth.with_steps(synth.perlin_elevation(n, n, seed=1234), 200, seed=1235)
    paths = make_paths(rng, n, res, P)
    radii = np.array([RADII[i % k] for i in range(P)])
    groups = [(r, [paths[i] for i in np.flatnonzero(radii == r)]) for r in RADII[:k] if (radii == r).any()]
    packed = [(r, capi.pack_paths(g)) for r, g in groups]
    iters = int(os.environ.get("TE_ITERS", "15"))
    with capi.Context(0) as c:
        p = capi.default_params()
        p.fp_offset = 0.15
        c.set_params(p)
        c.set_geometry(n, n, 1, res)
        c.upload_elevation(e)
        c.run_chain(0)
        c.sync()

        def dense():
            out = []
            for r, (off, xy) in packed:
                p.fp_radius = r
                c.set_params(p)
                c.run_footprint()
                out.append(c.check_footprint_paths_packed(off, xy))
            return out

        def on_demand():
            return c.check_footprint_paths_radius(paths, radii, want_stats=True)

        t = {}
        for name, fn in (("dense", dense), ("on_demand", on_demand)):
            for _ in range(2):
                fn()
            s = []
            for _ in range(iters):
                c.sync()
                t0 = time.perf_counter()
                last = fn()
                s.append((time.perf_counter() - t0) * 1e3)
            t[name] = {"ms": round(float(np.median(s)), 3), "min_ms": round(float(np.min(s)), 3)}
        stats = last[3]
        n_safe = int(last[0].sum())
    return {"res": res, "paths": P, "radii": k, "dense": t["dense"], "on_demand": t["on_demand"], "n_safe": n_safe, **stats}


def main():
    n = int(os.environ.get("TE_SIZE", "4096"))
    if "--one" in sys.argv:
        k = sys.argv.index("--one")
        print(json.dumps(one(int(sys.argv[k + 1]), n)))
        return
    out = []
    for idx in range(len(CASES)):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", str(idx)], capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            sys.exit(1)  # (nothing more is started on the GPU after a failed case)
        out.append(json.loads(r.stdout.strip().splitlines()[-1]))
        print(json.dumps(out[-1]), flush=True)
    print(json.dumps({"size": n, "cases": out}))


if __name__ == "__main__":
    main()
