"""te_upload_image on one MI355X, a 4096 x 4096 map, each case in a fresh process; medians of 20 runs after 3 warm-ups.

  (a) the conversion kernel alone (event-timed) against a hipMemcpyDtoDAsync of one float layer in the same process
      (tools/image_kernel_bench.hip, built by `--build` with hipcc on any machine);
  (b) whole-route wall time of te_upload_image against what a host had to do before: convert and transpose with numpy,
      then te_upload_elevation -- both with pageable and with page-locked buffers.

  python tools/image_upload_bench.py --build                 # compile the kernel bench (no GPU needed)
  python tools/image_upload_bench.py [--n 4096] [--out F]    # run every case, print one JSON line each
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
EXE = os.path.join(ROOT, "tools", "image_kernel_bench")
CASES = ("mono8", "mono16", "rgba8")
WARMUP, ITERS = 3, 20


def build():
    from traversability_estimation_amd import build as b
    csrc = os.path.join(ROOT, "traversability_estimation_amd", "csrc")
    cmd = [b.hipcc()] + [f for f in b.CFLAGS if f != "-fPIC"] + ["-I" + os.path.join(ROOT, "include"), "-I" + csrc,
           os.path.join(ROOT, "tools", "image_kernel_bench.hip"), os.path.join(csrc, "te_image.hip"), "-o", EXE]
    subprocess.check_call(cmd)
    return EXE


def host_convert(a, lower, upper):
    """What the host did before: addLayerFromImage in numpy, then the column-major layer te_upload_elevation takes."""
    import numpy as np
    maxv = np.float32(np.iinfo(a.dtype).max)
    if a.ndim == 3:
        c = a.astype(np.uint32)
        g = (c[..., 0] * 3735 + c[..., 1] * 19235 + c[..., 2] * 9798 + 16384) >> 15
    else:
        g = a
    v = np.float32(lower) + np.float32(upper - lower) * (g.astype(np.float32) / maxv)
    if a.ndim == 3 and a.shape[2] == 4:
        v[a[..., 3] < int(0.5 * float(maxv))] = np.nan
    return np.ascontiguousarray(v.T)


def timed(fn):
    t = []
    for k in range(WARMUP + ITERS):
        t0 = time.perf_counter()
        fn()
        t1 = time.perf_counter()
        if k >= WARMUP:
            t.append((t1 - t0) * 1e3)
    return round(statistics.median(t), 3)


def one_case(enc, n):
    import numpy as np
    from traversability_estimation_amd import capi
    ch, bpc = capi.IMAGE_ENCODINGS[enc]
    rng = np.random.default_rng(0)
    a = rng.integers(0, 256 ** bpc, (n, n, ch) if ch > 1 else (n, n), dtype=np.uint16 if bpc == 2 else np.uint8)
    if ch == 4:
        a[..., 3] = np.where(rng.random((n, n)) < 0.01, 0, 256 ** bpc - 1)
    out = {"encoding": enc, "n": n, "bytes_per_cell": ch * bpc}
    k = subprocess.run([EXE, str(ch), str(bpc), str(n)], capture_output=True, text=True, timeout=120)
    if k.returncode != 0:
        raise SystemExit("image_kernel_bench failed: " + k.stdout + k.stderr)
    out["kernel"] = json.loads(k.stdout)
    with capi.Context(0) as ctx:
        ctx.set_geometry(n, n, 1, 0.05)
        floats = host_convert(a, 0.0, 1.0)
        out["upload_image_ms"] = timed(lambda: ctx.upload_image(a, enc, 0.0, 1.0))
        got = ctx.download("elevation")
        assert np.array_equal(got.view(np.uint32), floats.reshape(-1).view(np.uint32)), "the two routes disagree"
        out["host_convert_ms"] = timed(lambda: host_convert(a, 0.0, 1.0))
        out["upload_elevation_ms"] = timed(lambda: ctx.upload_elevation(floats))
        capi.pin_host(a)
        capi.pin_host(floats)
        try:
            out["upload_image_pinned_ms"] = timed(lambda: ctx.upload_image(a, enc, 0.0, 1.0))
            out["upload_elevation_pinned_ms"] = timed(lambda: ctx.upload_elevation(floats))
        finally:
            capi.unpin_host(a)
            capi.unpin_host(floats)
    out["parent_route_ms"] = round(out["host_convert_ms"] + out["upload_elevation_ms"], 3)
    out["parent_route_pinned_ms"] = round(out["host_convert_ms"] + out["upload_elevation_pinned_ms"], 3)
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
        raise SystemExit("tools/image_kernel_bench is missing: python tools/image_upload_bench.py --build")
    if args.case:
        print(json.dumps(one_case(args.case, args.n)), flush=True)
        return
    lines = []
    for enc in CASES:  # each case in a process of its own
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", enc, "--n", str(args.n)], capture_output=True,
                           text=True, timeout=600)
        if r.returncode != 0:
            raise SystemExit(f"{enc}: {r.stdout}{r.stderr}")
        lines.append(r.stdout.strip().splitlines()[-1])
        print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
