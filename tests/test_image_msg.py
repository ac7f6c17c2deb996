"""sensor_msgs/Image on the wire (te_image_parse) and the numpy restatement of addLayerFromImage the GPU tests compare
against (tests/ref_py/image_ref.py).  No device: the parser is host code, and the upload entry points check their pointers
before they touch one."""
import ctypes as C
import struct

import numpy as np
import pytest

from tests.ref_py import image_ref as R


@pytest.fixture(scope="module")
def capi():
    from traversability_estimation_amd import build, capi
    build.build_lib()
    return capi


def random_image(capi, encoding, h, w, seed=0):
    ch, bpc = capi.IMAGE_ENCODINGS[encoding]
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256 ** bpc, (h, w, ch), dtype=np.uint16 if bpc == 2 else np.uint8)
    return a[:, :, 0] if ch == 1 else a


def rejected(capi, msg, *words):
    info, off = capi.TeImageInfo(), C.c_size_t()
    L = capi.load()
    assert L.te_image_parse(msg, len(msg), C.byref(info), C.byref(off)) == capi.TE_ERR_INVALID_ARG, words
    err = L.te_last_error().decode()
    assert err.startswith("te_image_parse: ") and all(w in err for w in words), (err, words)


def test_parse_round_trips_every_encoding(capi):
    assert len(capi.IMAGE_ENCODINGS) == 16
    for n, (enc, (ch, bpc)) in enumerate(capi.IMAGE_ENCODINGS.items()):
        for big in (0, 1):
            a = random_image(capi, enc, 5, 7, seed=n)
            step = 7 * ch * bpc + (n % 4)
            frame = "odom"[:n % 5]
            msg = capi.image_msg(a, enc, step=step, is_bigendian=big, frame_id=frame, seq=100 + n, stamp=(1529564943, 122772932 + n))
            info, off = capi.image_parse(msg)
            assert (info.seq, info.stamp_sec, info.stamp_nsec) == (100 + n, 1529564943, 122772932 + n)
            assert info.frame_id == frame.encode() and info.encoding == enc.encode()
            assert (info.height, info.width, info.step) == (5, 7, step)
            assert (info.channels, info.bytes_per_channel, info.is_bigendian) == (ch, bpc, big)
            assert off + step * 5 == len(msg)
            # the pixels are where the offset says, in the byte order the message names
            got = R.samples_from_bytes(msg[off:], 5, 7, step, ch, bpc, big)
            assert np.array_equal(got.reshape(a.shape), a)


def test_malformed_images_are_rejected(capi):
    a = random_image(capi, "rgba16", 5, 7)
    good = capi.image_msg(a, "rgba16", step=60, frame_id="map")
    info, off = capi.image_parse(good)
    assert off == 12 + 4 + 3 + 8 + 4 + 6 + 1 + 4 + 4
    # any other encoding
    for enc in ("", "mono32", "32FC1", "yuv422", "bayer_rggb8", "8UC2", "16SC1", "MONO8", "mono8 ", "x" * 100):
        rejected(capi, capi.image_msg(a, enc), "encoding")
    # truncation: inside the header, inside a string, inside the data
    for cut in (0, 3, 11, 14, 17, 20, 33, 37, off - 1, off, off + 1, len(good) - 1):
        rejected(capi, good[:cut], "truncated")
    # step below the row's bytes
    rejected(capi, capi.image_msg(a, "rgba16", step=55), "step 55")
    # a data length other than step * height
    at = off - 4
    for n in (0, 299, 301):
        rejected(capi, good[:at] + struct.pack("<I", n) + good[off:], "step * height = 300")
    # sizes whose product overflows
    h_at, w_at, s_at = 12 + 4 + 3, 12 + 4 + 3 + 4, off - 8
    big_w = good[:w_at] + struct.pack("<I", 0x7FFFFFFF) + good[w_at + 4:s_at] + struct.pack("<I", 0x7FFFFFFF) + good[s_at + 4:]
    rejected(capi, big_w, "overflow")
    big_h = good[:h_at] + struct.pack("<I", 0x7FFFFFFF) + good[h_at + 4:]
    rejected(capi, big_h, "step * height")
    for field in (h_at, w_at, s_at):
        rejected(capi, good[:field] + struct.pack("<I", 0xFFFFFFFF) + good[field + 4:], "overflow")
    # an image without pixels is no grid map
    rejected(capi, good[:h_at] + struct.pack("<I", 0) + good[h_at + 4:], "0 x 7")
    # a frame_id that does not fit te_image_info
    rejected(capi, capi.image_msg(a, "rgba16", frame_id="f" * 64), "frame_id")
    assert capi.image_parse(capi.image_msg(a, "rgba16", frame_id="f" * 63))[0].frame_id == b"f" * 63
    # NULL pointers
    L = capi.load()
    i, o = capi.TeImageInfo(), C.c_size_t()
    for args in ((None, 10, C.byref(i), C.byref(o)), (good, len(good), None, C.byref(o)), (good, len(good), C.byref(i), None)):
        assert L.te_image_parse(*args) == capi.TE_ERR_INVALID_ARG
        assert b"te_image_parse: NULL" in L.te_last_error()


def test_parser_survives_corrupted_input(capi):
    """20 000 seeded mutations of a valid 5 x 7 rgba16 message: each ends in TE_OK or TE_ERR_INVALID_ARG, and an accepted one
    has its pixels inside the buffer."""
    good = capi.image_msg(random_image(capi, "rgba16", 5, 7, seed=3), "rgba16", step=59, frame_id="base", seq=7, stamp=(12, 34))
    rng = np.random.default_rng(2025)
    L = capi.load()
    info, off = capi.TeImageInfo(), C.c_size_t()
    parsed = rejected_n = 0
    for trial in range(20000):
        b = bytearray(good)
        kind = trial % 3
        if kind == 0:  # flip a few bytes
            for _ in range(int(rng.integers(1, 4))):
                b[int(rng.integers(0, len(b)))] = int(rng.integers(0, 256))
        elif kind == 1:  # truncate
            b = b[:int(rng.integers(0, len(b)))]
        else:  # overwrite a 32-bit length-like field with an extreme or a nearby value
            at = int(rng.integers(0, 64))
            old = struct.unpack_from("<I", b, at)[0]
            b[at:at + 4] = struct.pack("<I", int(rng.choice([0, 1, 0x7FFFFFFF, 0xFFFFFFFF, 0xFFFFFFF0, len(b), len(b) - at, (old + 1) & 0xFFFFFFFF,
                                                              (old - 1) & 0xFFFFFFFF])))
        b = bytes(b)
        rc = L.te_image_parse(b, len(b), C.byref(info), C.byref(off))
        assert rc in (capi.TE_OK, capi.TE_ERR_INVALID_ARG), (trial, rc)
        if rc == capi.TE_OK:
            parsed += 1
            assert off.value + info.step * info.height <= len(b), trial
            assert info.step >= info.width * info.channels * info.bytes_per_channel and info.height > 0 and info.width > 0
        else:
            rejected_n += 1
            assert L.te_last_error().startswith(b"te_image_parse: "), trial
    assert parsed > 1000 and rejected_n > 5000, (parsed, rejected_n)


def test_upload_entry_points_reject_null_without_a_device(capi):
    L = capi.load()
    a = np.zeros((4, 4), np.uint8)
    info = capi.TeImageInfo(height=4, width=4, step=4, channels=1, bytes_per_channel=1)
    msg = capi.image_msg(a, "mono8")
    assert L.te_upload_image(None, C.byref(info), C.c_void_p(a.ctypes.data), 0, 0, 0.0, 1.0, 0.5) == capi.TE_ERR_INVALID_ARG
    assert b"te_upload_image: NULL" in L.te_last_error()
    assert L.te_upload_image_msg(None, msg, len(msg), 0, 0.0, 1.0, 0.5, 0.1, 0.0, 0.0, None) == capi.TE_ERR_INVALID_ARG
    assert b"te_upload_image_msg: NULL" in L.te_last_error()


def test_reference_restatement_known_answers():
    lo, hi = np.float32(-0.3), np.float32(1.7)
    v = R.add_layer_from_image(np.array([[0, 255, 128]], np.uint8), lo, hi)
    assert v.dtype == np.float32 and v[0, 0] == lo and v[0, 1] == hi
    # the operations one at a time, in float32
    assert v[0, 2] == np.float32(lo + np.float32(np.float32(hi - lo) * np.float32(np.float32(128) / np.float32(255))))
    v = R.add_layer_from_image(np.array([[0, 65535]], np.uint16), lo, hi)
    assert v[0, 0] == lo and v[0, 1] == hi
    # a grey pixel keeps its value: the weights sum to 2^15
    assert sum(R.GREY_WEIGHTS) == 1 << R.GREY_SHIFT == 1 << 15
    for dtype in (np.uint8, np.uint16):
        val = np.arange(np.iinfo(dtype).max + 1, dtype=np.uint64)
        assert np.array_equal(R.grey(val, val, val), val)
        grey_px = np.stack([val.astype(dtype)] * 3, axis=-1)[None]
        assert np.array_equal(R.add_layer_from_image(grey_px, lo, hi), R.add_layer_from_image(val.astype(dtype)[None], lo, hi))
    # memory order: the weights belong to channels 0, 1, 2 as they lie, whatever the encoding's name says
    assert int(R.grey(255, 0, 0)) == (255 * 3735 + 16384) >> 15 and int(R.grey(0, 0, 255)) == (255 * 9798 + 16384) >> 15
    # alpha: thr = 127 / 32767 at 0.5; below it the cell stays NaN, at it the pixel counts
    assert R.alpha_threshold_sample(0.5, np.uint8) == 127 and R.alpha_threshold_sample(0.5, np.uint16) == 32767
    assert R.alpha_threshold_sample(1.0, np.uint8) == 255 and R.alpha_threshold_sample(0.0, np.uint16) == 0
    px = np.array([[[10, 20, 30, 126], [10, 20, 30, 127]]], np.uint8)
    v = R.add_layer_from_image(px, lo, hi)
    assert np.isnan(v[0, 0]) and v[0, 1] == R.add_layer_from_image(px[:, 1:, :3], lo, hi)[0, 0]
    px16 = np.array([[[10, 20, 30, 32766], [10, 20, 30, 32767]]], np.uint16)
    v = R.add_layer_from_image(px16, lo, hi)
    assert np.isnan(v[0, 0]) and np.isfinite(v[0, 1])
    # layer order: element (i, j) at j * H + i
    m = np.arange(6, dtype=np.float32).reshape(2, 3)
    assert np.array_equal(R.layer_order(m), [0, 3, 1, 4, 2, 5])
