#!/usr/bin/env python3
"""Which kernels the filter chain launches, case by case: the evidence that plan_chain_route (te_chain_route.h) routes as
the cascade of launchers before it did.

    rocprofv3 --kernel-trace --output-format csv -d OUT -- python tools/chain_route_trace.py run
    python tools/chain_route_trace.py compare PARENT_kernel_trace.csv THIS_kernel_trace.csv [STDOUT_OF_RUN] > profiles/chain_route_trace.json

`run` goes through a fixed list of small cases in one process and starts no profiler itself.  A kernel trace carries no
markers, so every case is preceded by a sentinel launch the cases themselves never make: te_run_filter(combine) on a
64 x (1000 + case number) map, i.e. k_combine with grid (1, 1000 + n, 1).  `compare` cuts two traces at the sentinels and
compares, per case, the sequence of (kernel, grid, workgroup, LDS bytes) in dispatch order.  The runtime's own kernels
(__amd_rocclr_*: the fills and copies of a context's set-up, uploads and teardown) are left out: only the library's count.
"""
import csv
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.environ.get("TRACE_PACKAGE_ROOT", ROOT))

RES = 0.05
SENTINEL = 1000


def tie_free(cells, res=RES):
    return cells * res * (1.0 + 1e-6)


def radii(capi, cells, res=RES, **over):
    r = cells * res if over.pop("tie", False) else tie_free(cells, res)
    return capi.default_params(**dict(dict(normals_radius=r, rough_radius=r, step_radius1=r, step_radius2=r), **over))


def terrain(rows, cols, seed=7):
    from traversability_estimation_amd import synth
    return np.asarray(synth.perlin_elevation(rows, cols, seed=seed), np.float32).reshape(cols, rows)


def speckle(e, fraction, seed=3):
    e = e.copy()
    e[np.random.default_rng(seed).random(e.shape) < fraction] = np.nan
    return e


def block(e):
    e = e.copy()
    e[30:54, 40:64] = np.nan
    return e


def cases(capi):
    """Yields (name, function of a fresh context)."""
    def chain(params, rows, cols, elev=None, flags=0, batch=1, res=RES, options=(), launches=1, pos=(0.0, 0.0)):
        def go(c):
            for k, v in options:
                c.set_option(k, v)
            c.set_params(params)
            c.set_geometry(rows, cols, batch, res, pos)
            e = terrain(rows, cols) if elev is None else elev
            c.upload_elevation(np.tile(e.reshape(-1), batch))
            for _ in range(launches):
                c.run_chain(flags)
                c.sync()
        return go

    bag = np.load(os.path.join(ROOT, "tests", "golden", "bag_map.npz"))
    yield "01 bag map, default YAML", chain(capi.default_params(), int(bag["rows"]), int(bag["cols"]), bag["elevation"], res=float(bag["resolution"]),
                                            pos=tuple(bag["position"]))
    yield "02 640x640 res 0.05, default YAML", chain(capi.default_params(), 640, 640)
    e = terrain(128, 96)
    for hname, elev in (("hole-free", e), ("0.1% speckle", speckle(e, 0.001)), ("5% speckle", speckle(e, 0.05)), ("24x24 NaN block", block(e))):
        for kname, flags in (("kept", capi.RUN_KEEP_NORMALS), ("scores", 0)):
            yield f"03 128x96 R9 {hname} {kname}", chain(radii(capi, 9), 128, 96, elev, flags)
    yield "04 128x96 tie radius 4", chain(radii(capi, 4, tie=True), 128, 96)
    yield "05 48x96 R5", chain(radii(capi, 5), 48, 96)
    yield "06 128x128 R14", chain(radii(capi, 14), 128, 128)
    yield "07 normals 5 cells, roughness 7 cells", chain(radii(capi, 5, rough_radius=tie_free(7)), 128, 96)
    yield "08 TE_RUN_GENERIC_KERNELS", chain(radii(capi, 5), 128, 96, flags=capi.RUN_GENERIC_KERNELS)
    yield "09 TE_OPT_FILTER_ANY_RADIUS=2 R5", chain(radii(capi, 5), 128, 96, options=((capi.OPT_FILTER_ANY_RADIUS, 2),))
    yield "10 batch of 3 maps 128x96", chain(radii(capi, 5), 128, 96, batch=3)

    def region(flags):
        def go(c):
            chain(radii(capi, 5), 256, 256, flags=flags)(c)
            c.run_chain_region(0, 93, 91, 70, 70, flags)
            c.sync()
        return go
    yield "11 70x70 region of 256x256", region(0)
    yield "11 70x70 region of 256x256, footprint", region(capi.RUN_FOOTPRINT)
    for sname, cells, tie in (("below one cell", 0.8, False), ("exactly one cell", 1, True), ("two cells", 2, True), ("five cells", 5, False)):
        r = cells * RES if tie else tie_free(cells)
        yield f"12 step radii {sname}", chain(radii(capi, 5, step_radius1=r, step_radius2=r), 128, 96)
    yield "13 2048x1024 chain", chain(radii(capi, 9), 2048, 1024)
    yield "13 2048x1024 chain + footprint", chain(radii(capi, 9), 2048, 1024, flags=capi.RUN_FOOTPRINT)
    yield "14 2048x2048 two launches (graph replay)", chain(radii(capi, 9), 2048, 2048, launches=2)

    def filters(c):
        chain(radii(capi, 5), 128, 96, flags=capi.RUN_KEEP_NORMALS)(c)  # (leaves the normal layers the plugins read)
        for f in ("normals", "slope", "step", "roughness", "combine"):
            c.run_filter(f)
            c.sync()
    yield "15 every TE_FILTER_* on 128x96", filters

    def rough_ties(c):
        chain(radii(capi, 4, tie=True), 128, 96, flags=capi.RUN_KEEP_NORMALS)(c)
        c.run_filter("roughness")
        c.sync()
    yield "15 TE_FILTER_ROUGHNESS at a tie radius", rough_ties


def run():
    from traversability_estimation_amd import capi
    capi.load()
    for n, (name, go) in enumerate(cases(capi)):
        with capi.Context(0) as s:  # the sentinel
            s.set_params(capi.default_params())
            s.set_geometry(64, SENTINEL + n, 1, RES)
            s.run_filter("combine")
            s.sync()
        print(f"case {n}: {name}", flush=True)
        with capi.Context(0) as c:
            go(c)
    print("done", flush=True)


def read_trace(path):
    """[(kernel, grid, workgroup, lds)] in dispatch order."""
    with open(path, newline="") as f:
        rows = list(csv.DictReader(f))
    rows.sort(key=lambda r: int(r["Dispatch_Id"]))
    out = []
    for r in rows:
        name = r["Kernel_Name"].split(" [clone")[0]
        if name.startswith("__amd_rocclr_"):
            continue
        out.append((name, [int(r["Grid_Size_X"]), int(r["Grid_Size_Y"]), int(r["Grid_Size_Z"])],
                    [int(r["Workgroup_Size_X"]), int(r["Workgroup_Size_Y"]), int(r["Workgroup_Size_Z"])], int(r["LDS_Block_Size"])))
    return out


def cut(trace):
    """{case number: its launches}, cut at the sentinels."""
    out, cur = {}, None
    for k in trace:
        if "k_combine" in k[0] and k[1][0] == 256 and k[1][1] >= SENTINEL and k[1][2] == 1:
            cur = k[1][1] - SENTINEL
            out[cur] = []
        elif cur is not None:
            out[cur].append(k)
    return out


def compare(parent_csv, this_csv, names_txt=None):
    """names_txt: the standard output of `run` (its "case N: name" lines), to name the cases in the result."""
    a, b = cut(read_trace(parent_csv)), cut(read_trace(this_csv))
    names = {}
    if names_txt:
        with open(names_txt) as f:
            names = {int(ln.split(":")[0].split()[1]): ln.split(": ", 1)[1].strip() for ln in f if ln.startswith("case ")}
    res = {"what": "per case, the (kernel, grid in threads, workgroup, LDS bytes) of every launch in dispatch order: parent commit against this one "
                   "(rocprofv3 --kernel-trace alone; the runtime's own fill and copy kernels left out; tools/chain_route_trace.py)", "cases": [], "kernels_compared": 0}
    same = sorted(a) == sorted(b)
    for n in sorted(set(a) | set(b)):
        pa, pb = a.get(n, []), b.get(n, [])
        ok = pa == pb
        same = same and ok
        res["kernels_compared"] += len(pa)
        entry = {"case": n, "name": names.get(n, ""), "identical": ok, "launches": [list(k) for k in pa]}
        if not ok:
            entry["this_commit"] = [list(k) for k in pb]
            entry["same_multiset"] = sorted(map(repr, pa)) == sorted(map(repr, pb))
        res["cases"].append(entry)
    res["n_cases"] = len(res["cases"])
    res["notes"] = ["graph replay (the second launch of the 2048 x 2048 case): the kernel trace lists the kernels of the replayed graph; both launches are compared",
                    "identical sequences are stored once (launches)"]
    res["verdict"] = "identical" if same else "DIFFERENT"
    return res


if __name__ == "__main__":
    if len(sys.argv) == 2 and sys.argv[1] == "run":
        run()
    elif len(sys.argv) in (4, 5) and sys.argv[1] == "compare":
        print(json.dumps(compare(*sys.argv[2:]), indent=0))
    else:
        sys.exit(__doc__)
