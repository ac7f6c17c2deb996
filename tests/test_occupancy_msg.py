"""nav_msgs/OccupancyGrid on the wire (te_occupancy_msg_write / te_occupancy_parse) and the numpy restatement of
toOccupancyGrid the GPU tests compare against (tests/ref_py/occupancy_ref.py).  No device: writer and parser are host code, and
the download entry points check their pointers before they touch one."""
import ctypes as C
import struct

import numpy as np
import pytest

from tests.ref_py import occupancy_ref as R


@pytest.fixture(scope="module")
def capi():
    from traversability_estimation_amd import build, capi
    build.build_lib()
    return capi


def make_info(capi, width=5, height=3, frame=b"map"):
    info = capi.TeOccupancyInfo(seq=7, stamp_sec=1529564943, stamp_nsec=122772932, frame_id=frame, map_load_sec=11, map_load_nsec=12,
                                resolution=0.05, width=width, height=height)
    info.origin[:] = [-1.5, 2.25, 0.0, 0.0, 0.0, 0.0, 1.0]
    return info


def hand_built(info, data):
    f = info.frame_id
    return (struct.pack("<IIII", info.seq, info.stamp_sec, info.stamp_nsec, len(f)) + f +
            struct.pack("<IIfII7d", info.map_load_sec, info.map_load_nsec, info.resolution, info.width, info.height, *info.origin) +
            struct.pack("<I", len(data)) + bytes(data))


def rejected(capi, msg, *words):
    info, off = capi.TeOccupancyInfo(), C.c_size_t()
    L = capi.load()
    assert L.te_occupancy_parse(msg, len(msg), C.byref(info), C.byref(off)) == capi.TE_ERR_INVALID_ARG, words
    err = L.te_last_error().decode()
    assert err.startswith("te_occupancy_parse: ") and all(w in err for w in words), (err, words)


def test_writer_matches_a_hand_built_message_and_round_trips(capi):
    data = np.arange(-1, 14, dtype=np.int8)
    for frame in (b"", b"map", b"f" * 63):
        info = make_info(capi, frame=frame)
        msg = capi.occupancy_msg_write(info, data)
        assert msg == hand_built(info, data.tobytes())
        got, off = capi.occupancy_parse(msg)
        assert off == 12 + 4 + len(frame) + 8 + 4 + 8 + 56 + 4 and off + 15 == len(msg)
        assert bytes(got) == bytes(info)  # every field, the padding included (both zero-initialised)
        assert np.array_equal(np.frombuffer(msg, np.int8, 15, off), data)
    # an empty grid is a valid message
    info = make_info(capi, width=0, height=9)
    msg = capi.occupancy_msg_write(info, np.zeros(0, np.int8))
    assert capi.occupancy_parse(msg)[1] == len(msg)


def test_sizing_call_and_small_buffers(capi):
    L = capi.load()
    info = make_info(capi)
    data = np.zeros(15, np.int8)
    need = C.c_size_t()
    assert L.te_occupancy_msg_write(C.byref(info), None, None, 0, C.byref(need)) == capi.TE_ERR_INVALID_ARG
    assert need.value == len(hand_built(info, data.tobytes()))
    buf = C.create_string_buffer(b"\xa5" * (need.value + 8), need.value + 8)
    d = data.ctypes.data_as(C.POINTER(C.c_int8))
    assert L.te_occupancy_msg_write(C.byref(info), d, buf, need.value - 1, C.byref(need)) == capi.TE_ERR_INVALID_ARG
    assert b"needs" in L.te_last_error() and buf.raw == b"\xa5" * (need.value + 8)  # nothing written
    assert L.te_occupancy_msg_write(C.byref(info), d, buf, need.value, C.byref(need)) == capi.TE_OK
    assert buf.raw[need.value:] == b"\xa5" * 8
    # NULL pointers, cells missing, a count that does not fit the length field
    assert L.te_occupancy_msg_write(None, d, buf, 100, C.byref(need)) == capi.TE_ERR_INVALID_ARG
    assert L.te_occupancy_msg_write(C.byref(info), d, buf, 100, None) == capi.TE_ERR_INVALID_ARG
    assert L.te_occupancy_msg_write(C.byref(info), None, buf, need.value, C.byref(need)) == capi.TE_ERR_INVALID_ARG
    big = make_info(capi, width=0x10000, height=0x10000)
    assert L.te_occupancy_msg_write(C.byref(big), None, None, 0, C.byref(need)) == capi.TE_ERR_INVALID_ARG
    assert b"overflows" in L.te_last_error()


def test_malformed_messages_are_rejected(capi):
    info = make_info(capi)
    good = hand_built(info, bytes(range(15)))
    _, off = capi.occupancy_parse(good)
    for cut in (0, 3, 11, 15, 17, 19, 20, 30, off - 5, off - 1, off, off + 1, len(good) - 1):
        rejected(capi, good[:cut], "truncated")
    w_at, h_at, n_at = 12 + 4 + 3 + 12, 12 + 4 + 3 + 16, off - 4
    # width * height != data length
    for n in (0, 14, 16):
        rejected(capi, good[:n_at] + struct.pack("<I", n) + good[off:], "width * height = 15")
    rejected(capi, good[:w_at] + struct.pack("<I", 4) + good[w_at + 4:], "width * height = 12")
    # products that overflow
    both = good[:w_at] + struct.pack("<II", 0x10000, 0x10000) + good[h_at + 4:]
    rejected(capi, both, "overflows")
    rejected(capi, good[:w_at] + struct.pack("<II", 0xFFFFFFFF, 0xFFFFFFFF) + good[h_at + 4:], "overflows")
    # (2^32 + 15 cells would wrap to the data length)
    wrap = good[:w_at] + struct.pack("<II", 0x10003, 0xFFFD) + good[h_at + 4:]
    assert (0x10003 * 0xFFFD) % 2 ** 32 != 15
    rejected(capi, wrap, "width * height")
    # a data length beyond the buffer
    rejected(capi, good[:w_at] + struct.pack("<II", 4, 4) + good[h_at + 4:n_at] + struct.pack("<I", 16) + good[off:], "data truncated")
    # a frame_id that does not fit
    rejected(capi, hand_built(make_info(capi), b"")[:12] + struct.pack("<I", 64) + b"f" * 64 + good[19:], "frame_id")
    # a frame_id length that points beyond the message
    rejected(capi, good[:12] + struct.pack("<I", 0xFFFFFFF0) + good[16:], "truncated")
    L = capi.load()
    i, o = capi.TeOccupancyInfo(), C.c_size_t()
    for args in ((None, 10, C.byref(i), C.byref(o)), (good, len(good), None, C.byref(o)), (good, len(good), C.byref(i), None)):
        assert L.te_occupancy_parse(*args) == capi.TE_ERR_INVALID_ARG
        assert b"te_occupancy_parse: NULL" in L.te_last_error()


def test_download_entry_points_reject_null_without_a_device(capi):
    L = capi.load()
    need = C.c_size_t()
    ids = (C.c_int * 1)(4)
    f = (C.c_float * 1)(0.0)
    out = (C.c_int8 * 16)()
    assert L.te_download_occupancy(None, 0, 1, ids, f, f, out) == capi.TE_ERR_INVALID_ARG
    assert b"te_download_occupancy: NULL" in L.te_last_error()
    assert L.te_download_occupancy_msg(None, C.byref(capi.TeMsgInfo()), 4, 1.0, 0.0, None, 0, C.byref(need)) == capi.TE_ERR_INVALID_ARG
    assert b"te_download_occupancy_msg: NULL" in L.te_last_error()


def test_reference_restatement_known_answers(capi):
    # the restated info fields are the ones the writer puts on the wire
    res, width, height, origin = R.info_fields(4, 6, 0.5, (1.0, -2.0))
    info = capi.TeOccupancyInfo(resolution=res, width=width, height=height)
    info.origin[:] = origin
    cells = R.to_occupancy(np.arange(24, dtype=np.float32) / 24, 0.0, 1.0)
    msg = capi.occupancy_msg_write(info, cells)
    back, off = capi.occupancy_parse(msg)
    assert np.array_equal(np.frombuffer(msg, np.int8, 24, off), cells)
    assert (back.width, back.height, tuple(back.origin)) == (4, 6, origin) and np.float32(back.resolution) == res
    nan, inf = np.float32("nan"), np.float32("inf")
    # the reference's config: data_min 1, data_max 0 -- traversability 1 is free (0), 0 is occupied (100)
    x = np.array([1.0, 0.0, 0.5, nan, inf, -inf, 2.0, -1.0, 0.25], np.float32)
    assert R.to_occupancy(x, 1.0, 0.0)[::-1].tolist() == [0, 100, 50, -1, 0, 100, 0, 100, 75]
    assert R.to_occupancy(x, 0.0, 1.0)[::-1].tolist() == [100, 0, 50, -1, 100, 0, 100, 0, 25]
    # the operations one at a time, in float32; the conversion truncates
    v = np.float32(np.float32(np.float32(0.999) - np.float32(0.0)) / np.float32(1.0))
    assert R.to_occupancy([0.999], 0.0, 1.0)[0] == int(np.float32(np.float32(0.0) + v * np.float32(100.0))) == 99
    # data_min == data_max: 0 / 0 = NaN -> -1, +-x / 0 = +-inf -> 100 / 0
    assert R.to_occupancy([0.5, 0.7, 0.2], 0.5, 0.5)[::-1].tolist() == [-1, 100, 0]
    # reversed storage order
    assert R.to_occupancy(np.arange(4, dtype=np.float32) / 4, 0.0, 1.0).tolist() == [75, 50, 25, 0]
    # the variants the GPU test searches with do differ from the contract somewhere
    x = np.concatenate([R.boundary_inputs(mn, mx) for mn, mx in ((0.1, 3.1), (-0.3, 1.7), (1.0, 0.3))])
    assert (R.to_occupancy(x, 0.1, 3.1) != R.to_occupancy_reciprocal(x, 0.1, 3.1)).sum() >= 10
    assert R.info_fields(4, 6, 0.5, (1.0, -2.0)) == (np.float32(0.5), 4, 6, (0.0, -3.5, 0.0, 0.0, 0.0, 0.0, 1.0))
