"""te_download_occupancy and te_download_cloud on one MI355X, a 4096 x 4096 map, each case in a fresh process; medians of 20
runs after 3 warm-ups (the method of tools/image_upload_bench.py).

  occupancy1 / occupancy4   one score layer / the four layers of config/visualization/traversability.yaml -> int8 grids
  cloud0 / cloud20          the elevation cloud (x, y, z) with no holes / 20 % holes
  (a) the conversion kernels alone (HIP events: k_occupancy; k_cloud_count + k_cloud_scan, k_cloud_scatter) against a
      hipMemcpyDtoDAsync of one float layer in the same process (tools/output_kernel_bench.hip, built by `--build` with hipcc
      on any machine and linked against libtravgpu.so): the "kernel" entry of every line;
  (b) wall time of the whole call, PCIe included, with a pageable and with a page-locked host buffer, against the route a host
      had before: te_download_layer of the same layers, then the conversion in numpy.

  python tools/output_bench.py --build                 # compile the kernel bench (no GPU needed)
  python tools/output_bench.py [--n 4096] [--out F]    # run every case, print one JSON line each
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
EXE = os.path.join(ROOT, "tools", "output_kernel_bench")
CASES = ("occupancy1", "occupancy4", "cloud0", "cloud20")
SCORES = ["traversability", "traversability_slope", "traversability_step", "traversability_roughness"]
WARMUP, ITERS = 3, 20


def build():
    from traversability_estimation_amd import build as b
    pkg = os.path.join(ROOT, "traversability_estimation_amd")
    b.build_lib()
    cmd = [b.hipcc()] + [f for f in b.CFLAGS if f != "-fPIC"] + ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(pkg, "csrc"),
           os.path.join(ROOT, "tools", "output_kernel_bench.hip"), "-L" + pkg, "-ltravgpu", "-Wl,-rpath," + pkg, "-o", EXE]
    subprocess.check_call(cmd)
    return EXE


def kernel_alone(case, n):
    what = "occupancy" if case.startswith("occupancy") else "cloud"
    k = subprocess.run([EXE, what, case[len(what):], str(n)], capture_output=True, text=True, timeout=120)
    if k.returncode != 0:
        raise SystemExit("output_kernel_bench failed: " + k.stdout + k.stderr)
    return json.loads(k.stdout)


def timed(fn):
    t = []
    for k in range(WARMUP + ITERS):
        t0 = time.perf_counter()
        fn()
        t1 = time.perf_counter()
        if k >= WARMUP:
            t.append((t1 - t0) * 1e3)
    return round(statistics.median(t), 3)


def host_occupancy(x, data_min, data_max, out):
    """toOccupancyGrid in numpy, as a host would write it: float32 throughout, reversed into `out`."""
    import numpy as np
    v = (x - np.float32(data_min)) / np.float32(np.float32(data_max) - np.float32(data_min))
    nan = np.isnan(v)
    np.clip(v, np.float32(0.0), np.float32(1.0), out=v)
    v *= np.float32(100.0)
    v[nan] = np.float32(-1.0)
    out[:] = v[::-1].astype(np.int8)


def host_cloud(z, x_of_row, y_of_col, rows):
    """toPointCloud of one layer in numpy: drop the invalid cells, attach the positions."""
    import numpy as np
    cells = np.nonzero(np.isfinite(z))[0]
    pts = np.empty((len(cells), 3), np.float32)
    pts[:, 0] = x_of_row[cells % rows]
    pts[:, 1] = y_of_col[cells // rows]
    pts[:, 2] = z[cells]
    return pts


def one_case(case, n):
    import numpy as np
    from traversability_estimation_amd import capi
    rng = np.random.default_rng(0)
    cells = n * n
    out = {"case": case, "n": n, "kernel": kernel_alone(case, n)}
    with capi.Context(0) as ctx:
        ctx.set_geometry(n, n, 1, 0.05)
        if case.startswith("occupancy"):
            names = SCORES[:int(case[len("occupancy"):])]
            for k, name in enumerate(names):
                x = rng.random(cells, dtype=np.float32)
                x[rng.random(cells) < 0.02] = np.nan
                ctx.upload_layer(name, x)
            got = np.empty((len(names), cells), np.int8)
            floats = np.empty((len(names), cells), np.float32)
            want = np.empty_like(got)

            def parent():
                for k, name in enumerate(names):
                    ctx.download_into(name, floats[k])
                    host_occupancy(floats[k], 1.0, 0.0, want[k])

            def download_only():
                for k, name in enumerate(names):
                    ctx.download_into(name, floats[k])

            out["bytes_over_pcie"] = got.nbytes
            out["parent_bytes_over_pcie"] = floats.nbytes
            out["device_ms"] = timed(lambda: ctx.download_occupancy(names, 1.0, 0.0, out=got))
            out["parent_route_ms"] = timed(parent)
            out["parent_download_ms"] = timed(download_only)
            assert np.array_equal(got, want), "the two routes disagree"
            capi.pin_host(got)
            capi.pin_host(floats)
            try:
                out["device_pinned_ms"] = timed(lambda: ctx.download_occupancy(names, 1.0, 0.0, out=got))
                out["parent_route_pinned_ms"] = timed(parent)
                out["parent_download_pinned_ms"] = timed(download_only)
            finally:
                capi.unpin_host(got)
                capi.unpin_host(floats)
        else:
            holes = int(case[len("cloud"):]) / 100.0
            z = rng.standard_normal(cells).astype(np.float32)
            z[rng.random(cells) < holes] = np.nan
            ctx.upload_elevation(z)
            from tests.ref_py.cloud_ref import cell_positions
            xr, yc = cell_positions(n, n, 0.05, (0.0, 0.0))
            got = np.empty(cells * 3, np.float32)
            floats = np.empty(cells, np.float32)
            res = {}

            def device():
                res["pts"] = ctx.download_cloud(["elevation"], "elevation", out=got)

            def parent():
                ctx.download_into("elevation", floats)
                res["want"] = host_cloud(floats, xr, yc, n)

            out["device_ms"] = timed(device)
            out["parent_route_ms"] = timed(parent)
            out["parent_download_ms"] = timed(lambda: ctx.download_into("elevation", floats))
            out["count_only_ms"] = timed(lambda: ctx.count_cloud(["elevation"], "elevation"))
            assert np.array_equal(res["pts"].view(np.uint32), res["want"].view(np.uint32)), "the two routes disagree"
            out["points"] = len(res["pts"])
            out["bytes_over_pcie"] = int(res["pts"].nbytes)
            out["parent_bytes_over_pcie"] = floats.nbytes
            capi.pin_host(got)
            capi.pin_host(floats)
            try:
                out["device_pinned_ms"] = timed(device)
                out["parent_route_pinned_ms"] = timed(parent)
            finally:
                capi.unpin_host(got)
                capi.unpin_host(floats)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--build", action="store_true")
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--case")
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.build:
        print(build())
        return
    if not os.path.exists(EXE):
        raise SystemExit("tools/output_kernel_bench is missing: python tools/output_bench.py --build")
    if args.case:
        print(json.dumps(one_case(args.case, args.n)), flush=True)
        return
    lines = []
    for case in CASES:  # each case in a process of its own
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", case, "--n", str(args.n)], capture_output=True,
                           text=True, timeout=600)
        if r.returncode != 0:
            raise SystemExit(f"{case}: {r.stdout}{r.stderr}")
        lines.append(r.stdout.strip().splitlines()[-1])
        print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
