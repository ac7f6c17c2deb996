"""te_download_submap / te_download_submap_msg on the device: every result bit for bit against numpy slicing of
te_download_layer's result at the rectangle tests/ref_py/grid_map_ref.py::GridMapRef.submap gives for the same request -- the
alignments at which the packed copy can go wrong, the borders, 1 / 5 / 16 layers and the values a copy could disturb, one map
of a batch, refused requests, the message, pageable and page-locked buffers, and the state of the context afterwards."""
import ctypes as C
import os

import numpy as np
import pytest

from tests.conftest import ROOT
from tests.ref_py.grid_map_ref import GridMapRef

pytestmark = pytest.mark.gpu

SCORES = ["traversability", "traversability_slope", "traversability_step", "traversability_roughness"]
POISON = np.float32(-777.25)


@pytest.fixture(scope="module")
def capi():
    from traversability_estimation_amd import build, capi
    build.build_lib()
    return capi


def distinct_layer(n, k):
    """n cells no two of which share their bits (nor with another k), with the values a copy must not disturb in front."""
    x = (np.arange(n, dtype=np.uint32) * np.uint32(2654435761) + np.uint32(0x3f000000 + 7919 * k)).astype(np.uint32)
    x = (x & np.uint32(0x007fffff)) | np.uint32(0x3e800000 + (k << 23))  # finite, exponent by layer
    special = np.array([0x7fc00000, 0xffc00001, 0x7f800001, 0x7f800000, 0xff800000, 0x80000000, 0x00000000, 0x00000001, 0x807fffff,
                        0x00400000], np.uint32)  # NaNs (quiet, signed with a payload, signalling), +-inf, -0.0, 0.0, denormals
    m = min(n, special.size)
    x[:m] = special[:m]
    return x.view(np.float32)


def request_for(gm, row0, col0, h, w):
    """A request (position, length) whose submap is the h x w rectangle at (row0, col0): the corners a third of a cell inside
    the outer cells."""
    top = gm.position((row0, col0))
    bottom = gm.position((row0 + h - 1, col0 + w - 1))
    third = gm.res / 3.0
    hi = (top[0] + third, top[1] + third)
    lo = (bottom[0] - third, bottom[1] - third)
    return (0.5 * (hi[0] + lo[0]), 0.5 * (hi[1] + lo[1])), (hi[0] - lo[0], hi[1] - lo[1])


def expect(gm, whole, position, length):
    """(ok, (row0, col0, h, w), {name: array[h, w]}) by the restatement and numpy slicing; whole: {name: array[rows, cols]}."""
    ok, tl, size, sub = gm.submap(position, length)
    if not ok:
        return False, None, None, {}
    return True, (tl[0], tl[1], size[0], size[1]), sub, {k: v[tl[0]:tl[0] + size[0], tl[1]:tl[1] + size[1]] for k, v in whole.items()}


def same_bits(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    g, w = np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32)
    bad = np.argwhere(g != w)
    assert bad.size == 0, (what, len(bad), bad[:6].tolist())


def check_request(ctx, gm, whole, names, position, length, what, map_index=0):
    ok, rect, sub, want = expect(gm, whole, position, length)
    info, got = ctx.download_submap(position, length, names, map=map_index)
    assert bool(info.ok) == ok, what
    if not ok:
        assert got == {}
        return None
    assert (info.row0, info.col0, info.rows, info.cols) == rect, (what, rect)
    assert (info.pos_x, info.pos_y, info.length_x, info.length_y) == (sub.pos[0], sub.pos[1], sub.length[0], sub.length[1]), what
    for name in names:
        same_bits(got[name], want[name], (what, name))
    return rect


def fill(ctx, capi, rows, cols, names, batch=1, seed=0):
    """Uploads distinct layers; returns {name: array[batch, rows, cols]} as te_download_layer gives them back."""
    for k, name in enumerate(names):
        ctx.upload_layer(name, np.concatenate([distinct_layer(rows * cols, seed + 16 * b + k) for b in range(batch)]))
    return {name: ctx.download(name).reshape(batch, cols, rows).transpose(0, 2, 1) for name in names}


@pytest.mark.parametrize("shape", [(37, 29), (64, 48)])
def test_alignment(capi, shape):
    """rows odd: every source column has another alignment; h * 4 bytes between the destination columns: every h mod 4 with
    every row0 mod 4, for h in 1 .. 9 and w in 1, 2, 5, one layer and three (the second layer starts at w * h floats)."""
    rows, cols = shape
    gm = GridMapRef(rows, cols, 0.05, (1.5, -2.25))
    names = ["elevation", "traversability", "traversability_step"]
    with capi.Context(0) as ctx:
        ctx.set_geometry(rows, cols, 1, 0.05, (1.5, -2.25))
        whole = {k: v[0] for k, v in fill(ctx, capi, rows, cols, names).items()}
        seen = set()
        for row0 in (0, 1, 2, 3, rows - 12):
            for h in range(1, 10):
                for w in (1, 2, 5):
                    col0 = (3 * row0 + h + w) % (cols - w + 1)
                    position, length = request_for(gm, row0, col0, h, w)
                    rect = check_request(ctx, gm, whole, names if (h + w) % 2 else names[:1], position, length, (shape, row0, col0, h, w))
                    assert rect == (row0, col0, h, w), (rect, row0, col0, h, w)  # (the request is the rectangle it was made for)
                    seen.add((row0 % 4, h % 4))
        assert len(seen) == 16


def test_borders_corners_whole_map_and_one_cell(capi):
    rows, cols, res, pos = 37, 29, 0.1, (100.0, -250.3)
    gm = GridMapRef(rows, cols, res, pos)
    ext = (rows * res, cols * res)
    with capi.Context(0) as ctx:
        ctx.set_geometry(rows, cols, 1, res, pos)
        whole = {k: v[0] for k, v in fill(ctx, capi, rows, cols, SCORES).items()}
        # each border and each corner: a request of 0.73 x 0.55 m centred 0.2 m inside, reaching over the border (clamped)
        rects = set()
        for sx in (-1, 0, 1):
            for sy in (-1, 0, 1):
                position = (pos[0] + sx * (0.5 * ext[0] - 0.2), pos[1] + sy * (0.5 * ext[1] - 0.2))
                rect = check_request(ctx, gm, whole, SCORES, position, (0.73, 0.55), ("border", sx, sy))
                assert rect is not None
                rects.add(rect)
                if sx == 1:
                    assert rect[0] == 0
                if sx == -1:
                    assert rect[0] + rect[2] == rows
                if sy == 1:
                    assert rect[1] == 0
                if sy == -1:
                    assert rect[1] + rect[3] == cols
        assert len(rects) == 9
        # the whole map: exactly, and a request larger than the map
        for f in (1.0, 3.0):
            assert check_request(ctx, gm, whole, SCORES, pos, (f * ext[0], f * ext[1]), ("whole", f)) == (0, 0, rows, cols)
        # zero length: one cell
        assert check_request(ctx, gm, whole, SCORES[:1], gm.position((36, 28)), (0.0, 0.0), "far corner cell") == (36, 28, 1, 1)
    with capi.Context(0) as ctx:  # a 1 x 1 map
        ctx.set_geometry(1, 1, 1, 0.03, (0.5, 0.5))
        whole = {k: v[0] for k, v in fill(ctx, capi, 1, 1, SCORES).items()}
        gm1 = GridMapRef(1, 1, 0.03, (0.5, 0.5))
        assert check_request(ctx, gm1, whole, SCORES, (0.5, 0.5), (1.0, 1.0), "1 x 1") == (0, 0, 1, 1)
        assert check_request(ctx, gm1, whole, SCORES, (0.51, 0.49), (0.0, 0.0), "1 x 1, zero length") == (0, 0, 1, 1)


def test_layers_1_5_16_and_special_values(capi):
    rows, cols = 23, 11
    gm = GridMapRef(rows, cols, 0.05)
    five = ["elevation"] + SCORES
    with capi.Context(0) as ctx:
        ctx.set_geometry(rows, cols, 1, 0.05)
        whole = {k: v[0] for k, v in fill(ctx, capi, rows, cols, five + ["traversability_footprint", "surface_normal_x"]).items()}
        # the special values sit in the first cells of column 0: the rectangle holds them
        head = whole["elevation"][:10, 0].view(np.uint32)
        assert head[0] == 0x7fc00000 and head[2] == 0x7f800001 and head[5] == 0x80000000 and head[7] == 1
        position, length = request_for(gm, 0, 0, 13, 7)
        assert check_request(ctx, gm, whole, five[:1], position, length, "1 layer") == (0, 0, 13, 7)
        check_request(ctx, gm, whole, five, position, length, "5 layers")
        # 16 ids, some repeated: the packed buffer holds 16 matrices in the order of the ids
        sixteen = [five[k % 5] for k in range(9)] + ["traversability_footprint", "surface_normal_x"] + five
        info = capi.TeSubmapInfo()
        ids = (C.c_int * 16)(*[capi.LAYERS[k] for k in sixteen])
        out = np.full(16 * 13 * 7 + 5, POISON, np.float32)
        L = capi.load()
        capi._check(L.te_download_submap(ctx._h, 0, position[0], position[1], length[0], length[1], 16, ids, C.byref(info),
                                         C.c_void_p(out.ctypes.data), out.size))
        assert (info.ok, info.row0, info.col0, info.rows, info.cols) == (1, 0, 0, 13, 7)
        packed = out[:16 * 13 * 7].reshape(16, 7, 13)
        for k, name in enumerate(sixteen):
            same_bits(packed[k].T, whole[name][:13, :7], ("16 ids", k, name))
        assert (out[16 * 13 * 7:] == POISON).all()  # nothing behind the submap
        assert L.te_download_submap(ctx._h, 0, position[0], position[1], length[0], length[1], 17, ids, C.byref(info),
                                    C.c_void_p(out.ctypes.data), out.size) == capi.TE_ERR_INVALID_ARG


def test_one_map_of_a_batch(capi):
    rows, cols = 33, 17
    gm = GridMapRef(rows, cols, 0.1, (-4.0, 2.0))
    with capi.Context(0) as ctx:
        ctx.set_geometry(rows, cols, 3, 0.1, (-4.0, 2.0))
        maps = fill(ctx, capi, rows, cols, SCORES, batch=3)
        position, length = request_for(gm, 5, 3, 14, 9)
        for m in (2, 0, 1):
            assert check_request(ctx, gm, {k: v[m] for k, v in maps.items()}, SCORES, position, length, ("map", m), map_index=m) == (5, 3, 14, 9)
        assert not np.array_equal(maps["traversability"][2].view(np.uint32), maps["traversability"][1].view(np.uint32))
        L = capi.load()
        info = capi.TeSubmapInfo()
        ids = (C.c_int * 1)(4)
        for m in (-1, 3):
            assert L.te_download_submap(ctx._h, m, position[0], position[1], length[0], length[1], 1, ids, C.byref(info), None, 0) == capi.TE_ERR_INVALID_ARG
            assert b"map" in L.te_last_error()


def test_failures_write_nothing(capi):
    rows, cols = 21, 34
    gm = GridMapRef(rows, cols, 0.05, (3.0, 3.0))
    L = capi.load()
    with capi.Context(0) as ctx:
        info = capi.TeSubmapInfo()
        ids = (C.c_int * 4)(*[capi.LAYERS[k] for k in SCORES])
        out = np.full(4 * rows * cols, POISON, np.float32)
        o = C.c_void_p(out.ctypes.data)
        assert L.te_download_submap(ctx._h, 0, 3.0, 3.0, 0.5, 0.5, 4, ids, C.byref(info), o, out.size) == capi.TE_ERR_NOT_READY  # no geometry
        ctx.set_geometry(rows, cols, 1, 0.05, (3.0, 3.0))
        whole = {k: v[0] for k, v in fill(ctx, capi, rows, cols, SCORES).items()}
        # ok == 0: TE_OK, info says so, nothing is written
        for position in ((3.0 + rows * 0.05, 3.0), (3.0, 3.0 - cols * 0.05), (1e9, -1e9)):
            assert not gm.submap(position, (0.5, 0.5))[0]
            info.ok = 7
            assert L.te_download_submap(ctx._h, 0, position[0], position[1], 0.5, 0.5, 4, ids, C.byref(info), o, out.size) == capi.TE_OK
            assert (info.ok, info.rows, info.cols) == (0, 0, 0)
            assert check_request(ctx, gm, whole, SCORES, position, (0.5, 0.5), position) is None
        # too little room: TE_ERR_INVALID_ARG, info filled, nothing is written; exactly enough room works
        ok, rect, sub, want = expect(gm, whole, (3.1, 2.9), (0.5, 0.4))
        assert ok
        need = 4 * rect[2] * rect[3]
        for cap in (0, 1, need - 1):
            info = capi.TeSubmapInfo()
            assert L.te_download_submap(ctx._h, 0, 3.1, 2.9, 0.5, 0.4, 4, ids, C.byref(info), o, cap) == capi.TE_ERR_INVALID_ARG
            assert b"room for" in L.te_last_error()
            assert (info.ok, info.row0, info.col0, info.rows, info.cols) == (1,) + rect
        # arguments: refused before anything is computed
        for args in ((float("nan"), 2.9, 0.5, 0.4), (3.1, float("inf"), 0.5, 0.4), (3.1, 2.9, -0.5, 0.4), (3.1, 2.9, 0.5, float("nan"))):
            assert L.te_download_submap(ctx._h, 0, *args, 4, ids, C.byref(info), o, out.size) == capi.TE_ERR_INVALID_ARG
            assert info.ok == 0
        for n_layers in (-1, 0, 17):
            assert L.te_download_submap(ctx._h, 0, 3.1, 2.9, 0.5, 0.4, n_layers, ids, C.byref(info), o, out.size) == capi.TE_ERR_INVALID_ARG
        for bad in (-1, 15, 1000, capi.LAYERS["traversability_x"], capi.LAYERS["robot_slope"]):  # no such id / not there yet: as te_download_msg
            assert L.te_download_submap(ctx._h, 0, 3.1, 2.9, 0.5, 0.4, 2, (C.c_int * 2)(4, bad), C.byref(info), o, out.size) == capi.TE_ERR_INVALID_ARG
            assert b"bad layer" in L.te_last_error()
        for args in ((None, 0, 3.1, 2.9, 0.5, 0.4, 4, ids, C.byref(info), o, out.size), (ctx._h, 0, 3.1, 2.9, 0.5, 0.4, 4, None, C.byref(info), o, out.size),
                     (ctx._h, 0, 3.1, 2.9, 0.5, 0.4, 4, ids, None, o, out.size), (ctx._h, 0, 3.1, 2.9, 0.5, 0.4, 4, ids, C.byref(info), None, out.size)):
            assert L.te_download_submap(*args) == capi.TE_ERR_INVALID_ARG and b"NULL" in L.te_last_error()
        assert (out == POISON).all()  # none of the calls above wrote
        assert L.te_download_submap(ctx._h, 0, 3.1, 2.9, 0.5, 0.4, 4, ids, C.byref(info), o, need) == capi.TE_OK
        packed = out[:need].reshape(4, rect[3], rect[2])
        for k, name in enumerate(SCORES):
            same_bits(packed[k].T, want[name], ("exact room", name))
        assert (out[need:] == POISON).all()


def test_message(capi):
    rows, cols, res, pos = 37, 53, 0.05, (1.5, -2.25)
    gm = GridMapRef(rows, cols, res, pos)
    L = capi.load()
    with capi.Context(0) as ctx:
        ctx.set_geometry(rows, cols, 1, res, pos)
        whole = {k: v[0] for k, v in fill(ctx, capi, rows, cols, SCORES).items()}
        position, length = request_for(gm, 6, 9, 15, 22)
        hdr = capi.TeMsgInfo(seq=4, stamp_sec=5, stamp_nsec=6, frame_id=b"odom", start_row=9, start_col=9, rows=1, cols=1, resolution=7.0)
        hdr.pose[2], hdr.pose[6] = 0.75, 1.0
        layers = {"trav": "traversability", "step": "traversability_step", "trav_again": "traversability"}
        sub, msg = ctx.download_submap_msg(hdr, position, length, layers, basic_layers=("trav", "step"))
        ok, rect, ref, want = expect(gm, whole, position, length)
        assert ok and rect == (6, 9, 15, 22) and (sub.ok, sub.row0, sub.col0, sub.rows, sub.cols) == (1,) + rect
        # geometry, names and basic layers
        info, offsets = capi.msg_parse(msg)
        assert (info.seq, info.stamp_sec, info.stamp_nsec, info.frame_id) == (4, 5, 6, b"odom")
        assert (info.rows, info.cols, info.start_row, info.start_col) == (15, 22, 0, 0)
        assert (info.resolution, info.length_x, info.length_y) == (res, ref.length[0], ref.length[1]) == (res, sub.length_x, sub.length_y)
        assert tuple(info.pose) == (ref.pos[0], ref.pos[1], 0.75, 0.0, 0.0, 0.0, 1.0)
        assert list(offsets) == list(layers) and (info.n_layers, info.n_basic_layers) == (3, 2)
        assert offsets["step"] % 4 != offsets["trav"] % 4  # (the payloads do not share an alignment: the dimension labels lie between)
        # the payload equals the packed buffer
        _, packed = ctx.download_submap(position, length, list(layers.values()))
        for name, layer in layers.items():
            got = capi.msg_layer(msg, info, offsets[name])  # (cols, rows)
            same_bits(got.T, want[layer], ("message", name))
            same_bits(got.T, packed[layer], ("message against the packed buffer", name))
        # the host-only writer gives the same bytes from the same cells
        assert capi.msg_write(info, {k: capi.msg_layer(msg, info, offsets[k]) for k in layers}, basic_layers=("trav", "step")) == msg
        # sizing, and a buffer one byte short: the size is named, nothing is written
        ids, n = capi._layer_ids(layers.values())
        need = C.c_size_t()
        s2 = capi.TeSubmapInfo()
        args = (ctx._h, C.byref(hdr), position[0], position[1], length[0], length[1], n, ids, capi._names(list(layers)), 0, None, C.byref(s2))
        assert L.te_download_submap_msg(*args, None, 0, C.byref(need)) == capi.TE_ERR_INVALID_ARG and need.value > 3 * 15 * 22 * 4 and s2.ok == 1
        buf = C.create_string_buffer(b"\xa5" * need.value, need.value)
        assert L.te_download_submap_msg(*args, buf, need.value - 1, C.byref(need)) == capi.TE_ERR_INVALID_ARG
        assert buf.raw == b"\xa5" * need.value
        # a refused request: TE_OK, no bytes
        s3, none = ctx.download_submap_msg(hdr, (pos[0] + 10.0, pos[1]), length, layers)
        assert s3.ok == 0 and none == b""
        # the message goes back into a second context, whose geometry is the submap's
        with capi.Context(0) as other:
            up = other.upload_msg(msg, "step", "elevation")
            assert (other.rows, other.cols) == (15, 22) and (up.pose[0], up.pose[1]) == (sub.pos_x, sub.pos_y)
            same_bits(other.download("elevation").reshape(22, 15).T, want["traversability_step"], "uploaded again")
            again = capi.submap_geometry(15, 22, res, (sub.pos_x, sub.pos_y), (sub.pos_x, sub.pos_y), (sub.length_x, sub.length_y))
            assert (again.ok, again.row0, again.col0, again.rows, again.cols) == (1, 0, 0, 15, 22)


def test_context_is_left_untouched(capi):
    d = np.load(os.path.join(ROOT, "tests", "golden", "bag_map.npz"))
    rows, cols, res = int(d["rows"]), int(d["cols"]), float(d["resolution"])
    centre = np.asarray(d["position"], np.float64)
    gm = GridMapRef(rows, cols, res, tuple(centre))
    L = capi.load()
    with capi.Context(0) as ctx:
        ctx.set_params(capi.default_params())
        ctx.set_geometry(rows, cols, 1, res, tuple(centre))
        ctx.upload_elevation(d["elevation"])
        ctx.run_chain(capi.RUN_FOOTPRINT)
        ctx.sync()
        names = ["elevation"] + SCORES + ["traversability_footprint"]
        paths = [np.array([[0.0, 0.0], [0.3, 0.2]]) + centre, np.array([[0.1, -0.2]]) + centre]

        def state():
            layers = {k: ctx.download(k).view(np.uint32).copy() for k in names}
            absent = [L.te_download_layer(ctx._h, capi.LAYERS[k], np.zeros(rows * cols, np.float32).ctypes.data_as(C.POINTER(C.c_float)), 0, 1)
                      for k in ("traversability_x", "traversability_rot", "robot_slope")]
            safe, trav, st = ctx.check_footprint_paths(paths)  # (needs the complete footprint layer)
            return layers, absent, bytes(ctx.get_params()), safe.tolist(), trav.tolist(), st.tolist()

        before = state()
        whole = {k: before[0][k].view(np.float32).reshape(cols, rows).T for k in names}
        position = (centre[0] + 0.21, centre[1] - 0.13)
        assert check_request(ctx, gm, whole, names, position, (1.0, 0.8), "chain results") is not None
        ctx.download_submap_msg(capi.TeMsgInfo(), position, (1.0, 0.8), {k: k for k in SCORES})
        ctx.download_submap((centre[0] + 100.0, centre[1]), (1.0, 1.0), SCORES)  # (a refused request)
        after = state()
        assert before[1] == after[1] == [capi.TE_ERR_INVALID_ARG] * 3
        assert before[2:] == after[2:]
        for k in names:
            assert np.array_equal(before[0][k], after[0][k]), k
        # a region run with the footprint flag still finds chain and footprint results in place
        ctx.run_chain_region(0, 3, 4, 5, 6, capi.RUN_FOOTPRINT)
        ctx.sync()
        assert ctx.check_footprint_paths(paths)[0].tolist() == before[3]


def test_pageable_pinned_and_the_staging_ring(capi):
    """1100 x 1000 cells: the whole map of four layers is 17.6 MB, beyond the 4 MiB from which a pageable buffer goes through
    the staging ring; a 150 x 140 submap stays below it.  Both with a pageable and with a page-locked buffer."""
    rows, cols, res = 1100, 1000, 0.03
    gm = GridMapRef(rows, cols, res)
    with capi.Context(0) as ctx:
        ctx.set_geometry(rows, cols, 1, res)
        whole = {k: v[0] for k, v in fill(ctx, capi, rows, cols, SCORES).items()}
        small = request_for(gm, 333, 517, 150, 140)
        big = ((0.0, 0.0), (rows * res, cols * res))
        for what, (position, length) in (("small", small), ("whole", big)):
            ok, rect, sub, want = expect(gm, whole, position, length)
            assert ok and rect == ((333, 517, 150, 140) if what == "small" else (0, 0, rows, cols))
            n = 4 * rect[2] * rect[3]
            for kind in ("pageable", "pinned"):
                out = np.full(n + 3, POISON, np.float32)
                if kind == "pinned":
                    capi.pin_host(out)
                try:
                    info, got = ctx.download_submap(position, length, SCORES, out=out)
                    assert info.ok == 1
                    for name in SCORES:
                        same_bits(got[name], want[name], (what, kind, name))
                    assert (out[n:] == POISON).all()
                finally:
                    if kind == "pinned":
                        capi.unpin_host(out)
