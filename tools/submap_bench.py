"""te_download_submap on one MI355X: a 4096 x 4096 map at 0.03 m, after the chain and the footprint pass, the reference node's
default 5 m x 5 m submap around a point off the map's centre; each case in a fresh process, medians of 30 timed calls after
5 warm-ups.

  scores4 / score1   the four score layers / the traversability layer alone
  (a) the pack kernel alone (HIP events) against a device-to-device copy of the same bytes in the same process
      (tools/submap_kernel_bench.hip, built by `--build` with hipcc on any machine and linked against libtravgpu.so): the
      "kernel" entry of every line;
  (b) wall time of the whole call, PCIe included, into a pageable and into a page-locked buffer (the submap call and the tile
      route take turns, three rounds of 5 + 30 calls each: the figure is the median of the three medians, the rounds are listed):
        submap_ms        te_download_submap
        submap_msg_ms    te_download_submap_msg (pageable only: the message buffer)
        tile_route_ms    what a host had before: one te_download_tile per layer on the same rectangle
        whole_msg_ms     te_download_msg of the same layers (every cell of every layer)

  python tools/submap_bench.py --build                 # compile the kernel bench (no GPU needed)
  python tools/submap_bench.py [--n 4096] [--out F]    # run every case, print one JSON line each
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
EXE = os.path.join(ROOT, "tools", "submap_kernel_bench")
SCORES = ["traversability", "traversability_slope", "traversability_step", "traversability_roughness"]
CASES = {"scores4": SCORES, "score1": SCORES[:1]}
RES, LENGTH = 0.03, (5.0, 5.0)
WARMUP, ITERS = 5, 30


def build():
    from traversability_estimation_amd import build as b
    pkg = os.path.join(ROOT, "traversability_estimation_amd")
    b.build_lib()
    cmd = [b.hipcc()] + [f for f in b.CFLAGS if f != "-fPIC"] + ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(pkg, "csrc"),
           os.path.join(ROOT, "tools", "submap_kernel_bench.hip"), "-L" + pkg, "-ltravgpu", "-Wl,-rpath," + pkg, "-o", EXE]
    subprocess.check_call(cmd)
    return EXE


def kernel_alone(n_layers, n, h, w):
    k = subprocess.run([EXE, str(n_layers), str(n), str(h), str(w)], capture_output=True, text=True, timeout=300)
    if k.returncode != 0:
        raise SystemExit("submap_kernel_bench failed: " + k.stdout + k.stderr)
    return json.loads(k.stdout)


def timed(fn):
    t = []
    for k in range(WARMUP + ITERS):
        t0 = time.perf_counter()
        fn()
        t1 = time.perf_counter()
        if k >= WARMUP:
            t.append((t1 - t0) * 1e3)
    return round(statistics.median(t), 4)


def one_case(case, n):
    import numpy as np
    from traversability_estimation_amd import capi, synth
    names = CASES[case]
    L = capi.load()
    out = {"case": case, "n": n, "layers": len(names)}
    with capi.Context(0) as ctx:
        ctx.set_params(capi.default_params())
        ctx.set_geometry(n, n, 1, RES)
        ctx.upload_elevation(synth.with_steps(synth.perlin_elevation(n, n, 1), 40, 2))
        ctx.run_chain(capi.RUN_FOOTPRINT)
        ctx.sync()
        position = (0.1 * n * RES + 0.011, -0.07 * n * RES + 0.017)
        sub = capi.submap_geometry(n, n, RES, (0.0, 0.0), position, LENGTH)
        assert sub.ok == 1
        h, w = sub.rows, sub.cols
        out.update(h=h, w=w, row0=sub.row0, col0=sub.col0, bytes_over_pcie=len(names) * h * w * 4, whole_msg_bytes_over_pcie=len(names) * n * n * 4)
        out["kernel"] = kernel_alone(len(names), n, h, w)
        packed = np.zeros(len(names) * h * w, np.float32)
        tiles = np.zeros((len(names), w, h), np.float32)
        fp = C.POINTER(C.c_float)
        ids, nl = capi._layer_ids(names)

        def submap():
            ctx.download_submap(position, LENGTH, names, out=packed)

        def tile_route():
            for k in range(nl):
                capi._check(L.te_download_tile(ctx._h, ids[k], 0, sub.row0, sub.col0, h, w, tiles[k].ctypes.data_as(fp)))

        for kind in ("pageable", "pinned"):
            if kind == "pinned":
                capi.pin_host(packed)
                capi.pin_host(tiles)
            try:
                # the two routes take turns, so that neither owns the quieter half of the run
                a, b = [], []
                for r in range(3):
                    a.append(timed(submap))
                    b.append(timed(tile_route))
                out[f"submap_{kind}_ms"], out[f"tile_route_{kind}_ms"] = statistics.median(a), statistics.median(b)
                out[f"submap_{kind}_rounds_ms"], out[f"tile_route_{kind}_rounds_ms"] = a, b
            finally:
                if kind == "pinned":
                    capi.unpin_host(packed)
                    capi.unpin_host(tiles)
        assert np.array_equal(packed.view(np.uint32), tiles.reshape(-1).view(np.uint32)), "the two routes disagree"
        # the message variants into reused buffers (no allocation inside the timed call)
        hdr, need, si = capi.TeMsgInfo(), C.c_size_t(), capi.TeSubmapInfo()
        args = (ctx._h, C.byref(hdr), position[0], position[1], LENGTH[0], LENGTH[1], nl, ids, capi._names(names), 0, None, C.byref(si))
        L.te_download_submap_msg(*args, None, 0, C.byref(need))
        buf = np.zeros(need.value, np.uint8)
        out["submap_msg_ms"] = timed(lambda: capi._check(L.te_download_submap_msg(*args, C.c_void_p(buf.ctypes.data), buf.size, C.byref(need))))
        out["submap_msg_bytes"] = need.value
        wargs = (ctx._h, C.byref(hdr), nl, ids, capi._names(names), 0, None)
        L.te_download_msg(*wargs, None, 0, C.byref(need))
        big = np.zeros(need.value, np.uint8)
        out["whole_msg_ms"] = timed(lambda: capi._check(L.te_download_msg(*wargs, C.c_void_p(big.ctypes.data), big.size, C.byref(need))))
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
        raise SystemExit("tools/submap_kernel_bench is missing: python tools/submap_bench.py --build")
    if args.case:
        print(json.dumps(one_case(args.case, args.n)), flush=True)
        return
    lines = []
    for case in CASES:  # each case in a process of its own
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", case, "--n", str(args.n)], capture_output=True,
                           text=True, timeout=900)
        if r.returncode != 0:
            raise SystemExit(f"{case}: {r.stdout}{r.stderr}")
        lines.append(r.stdout.strip().splitlines()[-1])
        print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
