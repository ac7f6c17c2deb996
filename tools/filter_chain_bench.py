#!/usr/bin/env python3
"""The point-wise end of a grid_map filter chain on a 4096^2 map at 0.05 m with 1 % NaN: te_run_layer_expression into a user
layer against te_run_expression (the same kernel), te_run_threshold and te_copy_layer against the device copy of a layer, and
an expression with two thresholds behind it fused into one launch against the three calls.  Every figure is a host clock around
the calls and the te_sync that ends them (the calls are asynchronous), after warm-ups, `--iters` samples: the median with the
10th and 90th percentile as the spread; te_run_expression also by device events (te_time_expression_samples).  The whole
measurement runs twice in one process: the spread between the two runs is what "fused beats separate" has to clear.

    python tools/filter_chain_bench.py [--size 4096] [--iters 200] [--json profiles/filter_chain_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

RES = 0.05
WEIGHTED = "(1.0 * traversability_slope + 1.0 * traversability_step + 1.0 * traversability_roughness) / 3.0"
STEPS = [("lower", 0.2, 0.0), ("upper", 0.8, 1.0)]


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


def one_run(ctx, iters):
    res = {}
    res["expression_traversability"] = host_timed(ctx, lambda: ctx.run_expression(WEIGHTED), 10, iters)
    res["expression_traversability_events"] = stats(ctx.time_expression_samples(WEIGHTED, 3, min(iters, 50)))
    res["layer_expression_user"] = host_timed(ctx, lambda: ctx.run_layer_expression(WEIGHTED, "combined"), 10, iters)
    res["threshold"] = host_timed(ctx, lambda: ctx.run_threshold("combined", "lower", 0.2, 0.0), 10, iters)
    res["copy_layer"] = host_timed(ctx, lambda: ctx.copy_layer("combined", "copy"), 10, iters)

    def separate():
        ctx.run_layer_expression(WEIGHTED, "combined")
        for mode, thr, set_to in STEPS:
            ctx.run_threshold("combined", mode, thr, set_to)

    res["expression_two_thresholds_separate"] = host_timed(ctx, separate, 10, iters)
    res["expression_two_thresholds_fused"] = host_timed(ctx, lambda: ctx.run_layer_expression(WEIGHTED, "combined", thresholds=STEPS), 10, iters)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--json")
    a = ap.parse_args()
    from traversability_estimation_amd import capi
    rng = np.random.default_rng(1)
    out = {"what": __doc__.split("\n\n")[0].replace("\n", " "), "size": a.size, "resolution": RES, "runs": []}
    with capi.Context(0) as ctx:
        ctx.set_params(capi.default_params())
        ctx.set_geometry(a.size, a.size, 1, RES)
        for k in ("traversability_slope", "traversability_step", "traversability_roughness"):
            s = rng.random((a.size, a.size), dtype=np.float32)
            s.ravel()[rng.integers(0, s.size, s.size // 100)] = np.nan
            ctx.upload_layer(k, s)
        ctx.add_layer("combined"), ctx.add_layer("copy")
        for _ in range(2):
            out["runs"].append(one_run(ctx, a.iters))
            print(json.dumps(out["runs"][-1]), flush=True)
    r0, r1 = out["runs"]
    key_f, key_s = "expression_two_thresholds_fused", "expression_two_thresholds_separate"
    spread = max(abs(r0[k]["median_ms"] - r1[k]["median_ms"]) for k in (key_f, key_s))
    gain = min(r[key_s]["median_ms"] - r[key_f]["median_ms"] for r in (r0, r1))
    out["between_runs_spread_ms"] = round(spread, 4)
    out["fused_gain_ms"] = round(gain, 4)
    out["fused_beats_separate"] = bool(gain > spread)
    print(json.dumps({k: out[k] for k in ("between_runs_spread_ms", "fused_gain_ms", "fused_beats_separate")}), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
