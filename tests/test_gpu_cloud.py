"""te_download_cloud / te_download_cloud_msg on the device against the numpy restatement of toPointCloud
(tests/ref_py/cloud_ref.py): which cells are emitted, their order, every float bit for bit.  The holes put emitted cells on both
sides of every boundary of the compaction -- a wavefront's ballot, a counting workgroup, a scan workgroup's span
(te_cloud_spans)."""
import ctypes as C

import numpy as np
import pytest

from tests.ref_py import cloud_ref as R

pytestmark = pytest.mark.gpu

RES, POS = 0.05, (1.5, -2.25)
NAMES = ["elevation", "traversability", "traversability_slope"]


@pytest.fixture(scope="module")
def capi():
    from traversability_estimation_amd import build, capi
    build.build_lib()
    return capi


def same_bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == np.float32 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, (what, len(bad), bad[:4])


def layers_with_holes(n, seed, holes, keep=(), drop=()):
    """elevation with about `holes` invalid cells (NaN and both infinities), the cells `keep` valid and `drop` invalid; two
    further layers with holes of their own."""
    rng = np.random.default_rng(seed)
    out = {}
    for k, name in enumerate(NAMES):
        x = rng.standard_normal(n).astype(np.float32)
        bad = rng.random(n) < (holes if k == 0 else 0.2)
        x[bad] = rng.choice(np.array([np.nan, np.inf, -np.inf], np.float32), int(bad.sum()))
        out[name] = x
    e = out["elevation"]
    for c in keep:
        if 0 <= c < n:
            e[c] = np.float32(c % 1000) * np.float32(0.5)
    for c in drop:
        if 0 <= c < n:
            e[c] = np.nan
    return out


def upload(ctx, layers, map0=0):
    for name, x in layers.items():
        if name == "elevation":
            ctx.upload_elevation(x, map0)
        else:
            ctx.upload_layer(name, x, map0)


def check(capi, ctx, layers, rows, cols, names, point="elevation", basic=(), what=None):
    fields, want = R.to_point_cloud(layers, names, point, rows, cols, RES, POS, basic)
    assert ctx.count_cloud(names, point, basic) == len(want), what
    same_bits(ctx.download_cloud(names, point, basic), want, what)
    return fields, want


@pytest.mark.parametrize("case", ["all valid", "all invalid", "last cell only", "1 x 1", "1 x 1 invalid", "67 x 131, 30 % holes"])
def test_shapes(capi, case):
    rows, cols = (1, 1) if case.startswith("1 x 1") else (67, 131)
    n = rows * cols
    layers = layers_with_holes(n, 5, 0.3 if "30 %" in case else 0.0)
    if case in ("all invalid", "last cell only", "1 x 1 invalid"):
        layers["elevation"][:] = np.nan
    if case == "last cell only":
        layers["elevation"][-1] = np.float32(0.75)
    with capi.Context(0) as ctx:
        ctx.set_geometry(rows, cols, 1, RES, POS)
        upload(ctx, layers)
        _, want = check(capi, ctx, layers, rows, cols, ["elevation"], what=case)
        assert len(want) == {"all valid": n, "all invalid": 0, "last cell only": 1, "1 x 1": 1, "1 x 1 invalid": 0}.get(case, len(want))
        if "30 %" in case:
            assert 0.6 * n < len(want) < 0.8 * n
        # the point layer first, in the middle and last
        for names in (["elevation", "traversability", "traversability_slope"], ["traversability", "elevation", "traversability_slope"],
                      ["traversability", "traversability_slope", "elevation"]):
            fields, _ = check(capi, ctx, layers, rows, cols, names, what=(case, names))
            assert len(fields) == 5 and fields[names.index("elevation"):names.index("elevation") + 3] == ["x", "y", "z"]
        # another point layer; basic layers whose holes differ from the point layer's
        check(capi, ctx, layers, rows, cols, ["elevation", "traversability"], point="traversability", what=(case, "point = traversability"))
        _, w1 = check(capi, ctx, layers, rows, cols, ["elevation"], basic=["traversability"], what=(case, "one basic layer"))
        _, w2 = check(capi, ctx, layers, rows, cols, ["elevation", "traversability"], basic=["traversability_slope", "elevation", "traversability"],
                      what=(case, "three basic layers"))
        if case in ("all valid", "67 x 131, 30 % holes"):
            assert len(w2) < len(w1) < len(want)


def test_boundaries_of_the_compaction(capi):
    """A map larger than one scan workgroup's span, with emitted cells either side of every kind of boundary, and runs of
    holes that empty whole wavefronts and whole workgroups next to them."""
    wave, block, span = capi.cloud_spans()
    rows, cols = 397, 401
    n = rows * cols
    assert span < n < 2 * span and n % block != 0 and n % wave != 0
    edges = [wave, 2 * wave, block, 2 * block, block + wave, span, span + block, span - block, n - (n % block), n - (n % wave)]
    keep = [c + d for c in edges for d in (-1, 0)] + [0, n - 1]
    # an empty wavefront and an empty workgroup just in front of a boundary, an empty one right behind the span's
    drop = list(range(3 * wave, 4 * wave)) + list(range(5 * block, 6 * block)) + list(range(span + block, span + 2 * block))
    drop = [c for c in drop if c not in keep]
    layers = layers_with_holes(n, 9, 0.3, keep, drop)
    valid = np.isfinite(layers["elevation"])
    for c in edges:
        assert valid[c - 1] and valid[c], c
    assert not valid[3 * wave + 1:4 * wave - 1].any() and not valid[5 * block + 1:6 * block - 1].any()
    with capi.Context(0) as ctx:
        ctx.set_geometry(rows, cols, 1, RES, POS)
        upload(ctx, layers)
        _, want = check(capi, ctx, layers, rows, cols, ["traversability", "elevation"], what="boundaries")
        assert 0.6 * n < len(want) < 0.8 * n
        check(capi, ctx, layers, rows, cols, ["elevation"], basic=["traversability_slope"], what="boundaries, basic layer")
        # every cell valid: the offsets are the cell indices themselves
        full = {"elevation": np.arange(n, dtype=np.float32)}
        upload(ctx, full)
        _, want = check(capi, ctx, full, rows, cols, ["elevation"], what="all valid, large")
        assert len(want) == n


def test_one_map_of_a_batch(capi):
    rows, cols = 33, 17
    n = rows * cols
    with capi.Context(0) as ctx:
        ctx.set_geometry(rows, cols, 3, RES, POS)
        maps = [layers_with_holes(n, 20 + m, (0.0, 0.9, 0.3)[m]) for m in range(3)]
        for name in NAMES:
            upload(ctx, {name: np.concatenate([m[name] for m in maps])})
        for m in (2, 0, 1):
            fields, want = R.to_point_cloud(maps[m], NAMES, "elevation", rows, cols, RES, POS, ["traversability"])
            assert ctx.count_cloud(NAMES, "elevation", ["traversability"], map_index=m) == len(want)
            same_bits(ctx.download_cloud(NAMES, "elevation", ["traversability"], map_index=m), want, ("map", m))


def test_capacity_sizing_and_pinned_buffer(capi):
    rows, cols = 67, 131
    n = rows * cols
    L = capi.load()
    layers = layers_with_holes(n, 31, 0.3)
    with capi.Context(0) as ctx:
        ctx.set_geometry(rows, cols, 1, RES, POS)
        upload(ctx, layers)
        _, want = R.to_point_cloud(layers, ["elevation", "traversability"], "elevation", rows, cols, RES, POS)
        ids = (C.c_int * 2)(capi.LAYERS["elevation"], capi.LAYERS["traversability"])
        cnt = C.c_size_t(12345)
        # the sizing call
        assert L.te_download_cloud(ctx._h, 0, 2, ids, 0, 0, None, None, 0, C.byref(cnt)) == capi.TE_OK and cnt.value == len(want)
        # room for one point too few: refused, the count set, nothing written
        out = np.full(n * 4, 77.0, np.float32)
        o = C.c_void_p(out.ctypes.data)
        cnt = C.c_size_t(12345)
        assert L.te_download_cloud(ctx._h, 0, 2, ids, 0, 0, None, o, len(want) - 1, C.byref(cnt)) == capi.TE_ERR_INVALID_ARG
        assert cnt.value == len(want) and b"room for" in L.te_last_error() and (out == 77.0).all()
        # exactly enough: nothing behind the last record is touched
        assert L.te_download_cloud(ctx._h, 0, 2, ids, 0, 0, None, o, len(want), C.byref(cnt)) == capi.TE_OK
        same_bits(out[:len(want) * 4].reshape(-1, 4), want, "exact capacity")
        assert (out[len(want) * 4:] == 77.0).all()
        # a reused page-locked buffer with room for every cell
        pinned = np.full(n * 4, 77.0, np.float32)
        capi.pin_host(pinned)
        try:
            same_bits(ctx.download_cloud(["elevation", "traversability"], "elevation", out=pinned), want, "pinned")
        finally:
            capi.unpin_host(pinned)


def test_message(capi):
    rows, cols = 37, 53
    n = rows * cols
    L = capi.load()
    with capi.Context(0) as ctx:
        ctx.set_geometry(rows, cols, 1, RES, POS)
        layers = layers_with_holes(n, 41, 0.3)
        upload(ctx, layers)
        hdr = capi.TeMsgInfo(seq=4, stamp_sec=5, stamp_nsec=6, frame_id=b"odom")
        req = {"trav": "traversability", "elevation": "elevation", "slope": "traversability_slope"}
        renamed = {"trav": layers["traversability"], "elevation": layers["elevation"], "slope": layers["traversability_slope"]}
        fields, want = R.to_point_cloud(renamed, list(req), "elevation", rows, cols, RES, POS, ["slope"])
        msg = ctx.download_cloud_msg(hdr, req, "elevation", ["traversability_slope"])
        info, got_fields, off = capi.cloud_parse(msg)
        assert (info.seq, info.stamp_sec, info.stamp_nsec, info.frame_id) == (4, 5, 6, b"odom")
        assert (info.height, info.width, info.n_fields, info.point_step, info.row_step) == (1, len(want), 5, 20, 20 * len(want))
        assert (info.is_bigendian, info.is_dense) == (0, 0)
        assert got_fields == [(f, 4 * k, capi.POINTFIELD_FLOAT32, 1) for k, f in enumerate(fields)] and fields == ["trav", "x", "y", "z", "slope"]
        assert off + 20 * len(want) + 1 == len(msg)
        pts = np.frombuffer(msg, "<f4", len(want) * 5, off).reshape(-1, 5)
        same_bits(pts, want, "message")
        assert capi.cloud_msg_write(info, fields, pts) == msg  # the host-only writer gives the same bytes
        # sizing call; a buffer one byte short is refused and untouched
        ids = (C.c_int * 3)(*[capi.LAYERS[v] for v in req.values()])
        names = (C.c_char_p * 3)(*[k.encode() for k in req])
        basic = (C.c_int * 1)(capi.LAYERS["traversability_slope"])
        need = C.c_size_t()
        args = (ctx._h, C.byref(hdr), 3, ids, names, 0, 1, basic)
        assert L.te_download_cloud_msg(*args, None, 0, C.byref(need)) == capi.TE_ERR_INVALID_ARG and need.value == len(msg)
        buf = C.create_string_buffer(b"\xa5" * len(msg), len(msg))
        assert L.te_download_cloud_msg(*args, buf, len(msg) - 1, C.byref(need)) == capi.TE_ERR_INVALID_ARG
        assert buf.raw == b"\xa5" * len(msg) and need.value == len(msg)
        # no valid cell: a valid, empty message
        ctx.upload_elevation(np.full(n, np.nan, np.float32))
        empty = ctx.download_cloud_msg(hdr, {"elevation": "elevation"}, "elevation")
        info, got_fields, off = capi.cloud_parse(empty)
        assert (info.height, info.width, info.row_step) == (1, 0, 0) and [f[0] for f in got_fields] == ["x", "y", "z"]
        assert off + 1 == len(empty)


def test_context_is_left_untouched_and_error_codes(capi):
    import os
    from tests.conftest import ROOT
    d = np.load(os.path.join(ROOT, "tests", "golden", "bag_map.npz"))
    rows, cols, res = int(d["rows"]), int(d["cols"]), float(d["resolution"])
    L = capi.load()
    cnt = C.c_size_t()
    ids = (C.c_int * 20)(*([0] * 20))
    with capi.Context(0) as ctx:
        assert L.te_download_cloud(ctx._h, 0, 1, ids, 0, 0, None, None, 0, C.byref(cnt)) == capi.TE_ERR_NOT_READY  # no geometry
        ctx.set_params(capi.default_params())
        ctx.set_geometry(rows, cols, 1, res, tuple(d["position"]))
        ctx.upload_elevation(d["elevation"])
        ctx.run_chain(capi.RUN_FOOTPRINT)
        ctx.sync()
        names = ["elevation", "traversability", "traversability_slope", "traversability_step", "traversability_roughness", "traversability_footprint"]

        def state():
            return ({k: ctx.download(k).view(np.uint32).copy() for k in names}, bytes(ctx.get_params()),
                    L.te_set_layer_present(ctx._h, capi.LAYERS["robot_slope"], 1))

        before = state()
        held = {k: before[0][k].view(np.float32) for k in names}
        fields, want = R.to_point_cloud(held, names[:3], "elevation", rows, cols, res, tuple(d["position"]), ["traversability"])
        same_bits(ctx.download_cloud(names[:3], "elevation", ["traversability"]), want, "bag map")
        assert 0 < len(want) <= rows * cols
        ctx.download_cloud_msg(capi.TeMsgInfo(), {"elevation": "elevation"}, "elevation")
        after = state()
        assert before[1:] == after[1:] and after[2] == capi.TE_ERR_NOT_READY
        for k in names:
            assert np.array_equal(before[0][k], after[0][k]), k
        ctx.run_chain_region(0, 3, 4, 5, 6, capi.RUN_FOOTPRINT)  # (the chain's results are still in place)
        ctx.sync()
        # the error codes
        out = np.full(rows * cols * 4, 77.0, np.float32)
        o, cap = C.c_void_p(out.ctypes.data), rows * cols
        for args in ((None, 0, 1, ids, 0, 0, None, o, cap, C.byref(cnt)), (ctx._h, 0, 1, None, 0, 0, None, o, cap, C.byref(cnt)),
                     (ctx._h, 0, 1, ids, 0, 0, None, o, cap, None), (ctx._h, 0, 1, ids, 0, 0, None, None, cap, C.byref(cnt))):
            assert L.te_download_cloud(*args) == capi.TE_ERR_INVALID_ARG and b"NULL" in L.te_last_error()
        assert L.te_download_cloud(ctx._h, 0, 1, ids, 0, 1, None, o, cap, C.byref(cnt)) == capi.TE_ERR_INVALID_ARG  # basic list missing
        for map_index in (-1, 1):
            assert L.te_download_cloud(ctx._h, map_index, 1, ids, 0, 0, None, o, cap, C.byref(cnt)) == capi.TE_ERR_INVALID_ARG
        for n_layers in (-1, 0, 17):
            assert L.te_download_cloud(ctx._h, 0, n_layers, ids, 0, 0, None, o, cap, C.byref(cnt)) == capi.TE_ERR_INVALID_ARG
        for bad in (-1, 15, 1000):
            assert L.te_download_cloud(ctx._h, 0, 2, (C.c_int * 2)(0, bad), 0, 0, None, o, cap, C.byref(cnt)) == capi.TE_ERR_INVALID_ARG
            assert b"bad layer" in L.te_last_error()
            assert L.te_download_cloud(ctx._h, 0, 1, ids, 0, 1, (C.c_int * 1)(bad), o, cap, C.byref(cnt)) == capi.TE_ERR_INVALID_ARG
        # the point layer nowhere, and more than once (sixteen times: the record would not fit)
        assert L.te_download_cloud(ctx._h, 0, 2, (C.c_int * 2)(4, 1), 0, 0, None, o, cap, C.byref(cnt)) == capi.TE_ERR_INVALID_ARG
        assert b"nowhere" in L.te_last_error()
        for k in (2, 16):
            assert L.te_download_cloud(ctx._h, 0, k, ids, 0, 0, None, o, cap, C.byref(cnt)) == capi.TE_ERR_INVALID_ARG
            assert b"more than once" in L.te_last_error()
        for name in ("traversability_x", "robot_slope"):
            assert L.te_download_cloud(ctx._h, 0, 2, (C.c_int * 2)(0, capi.LAYERS[name]), 0, 0, None, o, cap, C.byref(cnt)) == capi.TE_ERR_NOT_READY
            assert L.te_download_cloud(ctx._h, 0, 1, ids, 0, 1, (C.c_int * 1)(capi.LAYERS[name]), o, cap, C.byref(cnt)) == capi.TE_ERR_NOT_READY
        assert (out == 77.0).all()
