"""The submap entry points of the C-ABI without a device: the symbols are exported, te_submap_geometry needs no context, the
calls that need one refuse NULL before they touch anything, and a message assembled on the host from a packed submap buffer
-- [layer][col][row], what te_download_submap writes -- and te_submap_geometry's result is accepted by te_msg_parse with the
submap's geometry."""
import ctypes as C

import numpy as np
import pytest

from tests.ref_py.grid_map_ref import GridMapRef


@pytest.fixture(scope="module")
def capi():
    from traversability_estimation_amd import build, capi
    build.build_lib()
    return capi


def test_symbols_and_struct(capi):
    L = capi.load()
    for s in ("te_submap_geometry", "te_download_submap", "te_download_submap_msg"):
        assert s in capi.SYMBOLS and hasattr(L, s), s
    # int32 x 5, padding, double x 4: the layout include/travgpu.h declares
    assert C.sizeof(capi.TeSubmapInfo) == 56 and capi.TeSubmapInfo.pos_x.offset == 24
    assert capi.SUBMAP_MAX_LAYERS == 16


def test_geometry_needs_no_context(capi):
    got = capi.submap_geometry(100, 133, 0.03, (100.0, -250.3), (100.4, -250.0), (1.0, 0.5))
    ok, tl, size, sub = GridMapRef(100, 133, 0.03, (100.0, -250.3)).submap((100.4, -250.0), (1.0, 0.5))
    assert ok and got.ok == 1
    assert (got.row0, got.col0, got.rows, got.cols) == tl + size
    assert (got.pos_x, got.pos_y, got.length_x, got.length_y) == sub.pos + sub.length
    out = capi.submap_geometry(100, 133, 0.03, (100.0, -250.3), (90.0, -250.0), (1.0, 0.5))  # a centre outside the map
    assert (out.ok, out.rows, out.cols, out.length_x) == (0, 0, 0, 0.0)


def test_null_arguments_are_refused_without_a_device(capi):
    L = capi.load()
    info, hdr, need = capi.TeSubmapInfo(), capi.TeMsgInfo(), C.c_size_t(5)
    ids = (C.c_int * 1)(4)
    out = np.zeros(4, np.float32)
    assert L.te_download_submap(None, 0, 0.0, 0.0, 1.0, 1.0, 1, ids, C.byref(info), C.c_void_p(out.ctypes.data), 4) == capi.TE_ERR_INVALID_ARG
    assert b"te_download_submap" in L.te_last_error()
    assert L.te_download_submap_msg(None, C.byref(hdr), 0.0, 0.0, 1.0, 1.0, 1, ids, capi._names(["a"]), 0, None, C.byref(info), None, 0,
                                    C.byref(need)) == capi.TE_ERR_INVALID_ARG
    assert b"te_download_submap_msg" in L.te_last_error()
    assert not out.any()


def test_a_message_assembled_on_the_host_from_a_packed_buffer(capi):
    rows, cols, res, pos = 37, 29, 0.1, (100.0, -250.3)
    sub = capi.submap_geometry(rows, cols, res, pos, (100.6, -250.9), (1.05, 0.8))
    assert sub.ok == 1 and 1 < sub.rows < rows and 1 < sub.cols < cols
    # the whole layers, and the packed buffer te_download_submap would give for them: [layer][col][row]
    rng = np.random.default_rng(5)
    whole = {k: rng.random((rows, cols), dtype=np.float32) for k in ("traversability", "traversability_step")}
    whole["traversability"][sub.row0, sub.col0] = np.nan
    packed = np.stack([whole[k][sub.row0:sub.row0 + sub.rows, sub.col0:sub.col0 + sub.cols].T for k in whole])
    assert packed.shape == (2, sub.cols, sub.rows)
    info = capi.TeMsgInfo(seq=3, stamp_sec=10, stamp_nsec=20, frame_id=b"map", resolution=res, length_x=sub.length_x, length_y=sub.length_y,
                          rows=sub.rows, cols=sub.cols)
    info.pose[0], info.pose[1], info.pose[6] = sub.pos_x, sub.pos_y, 1.0
    msg = capi.msg_write(info, {k: packed[n] for n, k in enumerate(whole)}, basic_layers=("traversability",))
    got, offsets = capi.msg_parse(msg)  # (checks round(length / resolution) against the layer sizes)
    assert (got.rows, got.cols, got.start_row, got.start_col) == (sub.rows, sub.cols, 0, 0)
    assert (got.resolution, got.length_x, got.length_y, got.pose[0], got.pose[1]) == (res, sub.length_x, sub.length_y, sub.pos_x, sub.pos_y)
    for k in whole:
        cells = capi.msg_layer(msg, got, offsets[k]).T  # [row, col] of the submap
        want = whole[k][sub.row0:sub.row0 + sub.rows, sub.col0:sub.col0 + sub.cols]
        assert np.array_equal(np.ascontiguousarray(cells).view(np.uint32), np.ascontiguousarray(want).view(np.uint32)), k
    # cell (i, j) of the submap lies where cell (row0 + i, col0 + j) of the map lies
    gm, gs = GridMapRef(rows, cols, res, pos), GridMapRef(sub.rows, sub.cols, res, (sub.pos_x, sub.pos_y))
    for i, j in ((0, 0), (sub.rows - 1, sub.cols - 1), (sub.rows // 2, 1)):
        a, b = gs.position((i, j)), gm.position((sub.row0 + i, sub.col0 + j))
        assert abs(a[0] - b[0]) < 1e-9 and abs(a[1] - b[1]) < 1e-9
