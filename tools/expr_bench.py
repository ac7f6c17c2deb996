"""te_run_expression on a 4096 x 4096 map against the weighted sum's own kernel (report only).

Every case runs in a fresh process and reports the median device time of event-timed launches (te_time_expression_samples):
  combine        te_run_filter(TE_FILTER_COMBINE), the yardstick
  shipped        the shipped expression through te_run_expression (7 instructions)
  one_reduction  elevation - meanOfFinites(elevation) (reduce + finish + map)
  thirty         a 30-instruction expression over three layers
Prints one JSON line per case and a last line with the ratios to `combine`.

    python tools/expr_bench.py [--size 4096] [--iters 50]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

A, B, C = "traversability_slope", "traversability_step", "traversability_roughness"
CASES = {
    "combine": None,
    "shipped": f"(1.0 / 3.0) * ({A} + {B} + {C})",
    "one_reduction": "elevation - meanOfFinites(elevation)",
    "thirty": f"cwiseMax(cwiseMin(abs({A} - {B}) .* {C} + 0.25 * {A}, 1.0), 0.0) + square({B} - 0.5) ./ (1.0 + abs({C})) - 0.125 * ({A} + {B})",
}


def one(case, size, iters):
    import numpy as np
    from traversability_estimation_amd import capi
    text = CASES[case]
    info = capi.expr_check(text) if text else {"n_instructions": 0, "n_reductions": 0}
    rng = np.random.default_rng(3)
    with capi.Context(0) as ctx:
        ctx.set_params(capi.default_params())
        ctx.set_geometry(size, size, 1, 0.05)
        for name in ("elevation", A, B, C):
            x = rng.random(size * size, dtype=np.float32)
            x[rng.random(size * size) < 0.02] = np.nan
            ctx.upload_layer(name, x)
        ms = ctx.time_expression_samples(text, warmup=5, iters=iters)
    cells = size * size
    med = float(np.median(ms))
    print(json.dumps({"case": case, "size": size, "instructions": info["n_instructions"], "reductions": info["n_reductions"], "median_ms": round(med, 5),
                      "min_ms": round(float(ms.min()), 5), "ns_per_cell": round(med * 1e6 / cells, 5), "iters": iters}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--case")
    a = ap.parse_args()
    if a.case:
        return one(a.case, a.size, a.iters)
    med = {}
    for case in CASES:  # a fresh process each: no case inherits another's clocks, allocations or cache state
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", case, "--size", str(a.size), "--iters", str(a.iters)],
                           capture_output=True, text=True, timeout=300)
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            return r.returncode
        line = r.stdout.strip().splitlines()[-1]
        print(line, flush=True)
        med[case] = json.loads(line)["median_ms"]
    print(json.dumps({"ratio_to_combine": {k: round(v / med["combine"], 3) for k, v in med.items()}}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
