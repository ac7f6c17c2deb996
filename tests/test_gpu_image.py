"""te_upload_image / te_upload_image_msg on the device: every encoding, byte order, pitch and shape against the numpy
restatement of addLayerFromImage (tests/ref_py/image_ref.py), bit for bit, NaN positions included; and the state of the
context afterwards, which must be the one te_upload_elevation of the same floats leaves."""
import ctypes as C

import numpy as np
import pytest

from tests.ref_py import image_ref as R

pytestmark = pytest.mark.gpu

LOWER, UPPER = -0.3, 1.7


@pytest.fixture(scope="module")
def capi():
    from traversability_estimation_amd import build, capi
    build.build_lib()
    return capi


def assert_bits(got, want, what):
    got, want = np.asarray(got, np.float32).reshape(-1), np.asarray(want, np.float32).reshape(-1)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), (what, "NaN positions", int((gn != wn).sum()))
    bad = got[~gn].view(np.uint32) != want[~wn].view(np.uint32)
    assert not bad.any(), (what, int(bad.sum()), got[~gn][bad][:4], want[~wn][bad][:4])


def random_samples(capi, encoding, h, w, seed, alpha_threshold=0.5, holes=0.1):
    """Random sample values; with an alpha channel about `holes` of the alphas below the threshold and the two values either
    side of it present."""
    ch, bpc = capi.IMAGE_ENCODINGS[encoding]
    dtype = np.uint16 if bpc == 2 else np.uint8
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256 ** bpc, (h, w, ch), dtype=dtype)
    if ch == 4:
        thr = R.alpha_threshold_sample(alpha_threshold, dtype)
        below = rng.random((h, w)) < holes
        a[..., 3] = np.where(below, rng.integers(0, thr, (h, w)), rng.integers(thr, 256 ** bpc, (h, w))).astype(dtype)
        flat = a.reshape(-1, 4)
        if len(flat) >= 2:
            flat[0, 3], flat[-1, 3] = thr - 1, thr
    return a[:, :, 0] if ch == 1 else a


def upload_raw(capi, ctx, info, pixels, layer=0, map_index=0, lower=LOWER, upper=UPPER, alpha=0.5):
    buf = np.frombuffer(pixels, np.uint8)
    return capi.load().te_upload_image(ctx._h, C.byref(info), C.c_void_p(buf.ctypes.data), layer, map_index, lower, upper, alpha)


def geometry_of(capi, ctx):
    info, _ = capi.msg_parse(ctx.download_msg(capi.TeMsgInfo(), {"elevation": "elevation"}))
    return info.rows, info.cols, info.resolution, info.pose[0], info.pose[1]


def test_every_encoding_odd_pitch_both_byte_orders(capi):
    h, w = 37, 53
    with capi.Context(0) as ctx:
        ctx.set_geometry(h, w, 1, 0.1)
        for n, (enc, (ch, bpc)) in enumerate(capi.IMAGE_ENCODINGS.items()):
            for big in ((0, 1) if bpc == 2 else (0,)):
                a = random_samples(capi, enc, h, w, seed=10 + n)
                step = w * ch * bpc + 5
                msg = capi.image_msg(a, enc, step=step, is_bigendian=big)
                info, off = capi.image_parse(msg)
                assert info.step == step and step % 2 == (w * ch * bpc + 1) % 2
                assert upload_raw(capi, ctx, info, msg[off:]) == capi.TE_OK, capi.load().te_last_error()
                want = R.add_layer_from_image(a, LOWER, UPPER)
                if ch == 4:
                    assert 0.03 < np.isnan(want).mean() < 0.25 and np.isnan(want[0, 0]) and not np.isnan(want[-1, -1])
                assert_bits(ctx.download("elevation"), R.layer_order(want), (enc, big))
        # an even pitch takes the aligned loads: the same values
        for enc in ("mono16", "rgba8", "rgba16"):
            ch, bpc = capi.IMAGE_ENCODINGS[enc]
            a = random_samples(capi, enc, h, w, seed=99)
            ctx.upload_image(a, enc, LOWER, UPPER)
            assert_bits(ctx.download("elevation"), R.layer_order(R.add_layer_from_image(a, LOWER, UPPER)), (enc, "packed"))
        # another alpha threshold moves the holes
        a = random_samples(capi, "bgra16", h, w, seed=5, alpha_threshold=0.9)
        ctx.upload_image(a, "bgra16", LOWER, UPPER, alpha_threshold=0.9)
        assert_bits(ctx.download("elevation"), R.layer_order(R.add_layer_from_image(a, LOWER, UPPER, 0.9)), "alpha 0.9")


@pytest.mark.parametrize("shape", [(1, 1), (1, 300), (300, 1), (130, 70)])
def test_shapes(capi, shape):
    h, w = shape
    with capi.Context(0) as ctx:
        ctx.set_geometry(h, w, 1, 0.1)
        for enc in ("mono16", "bgra8"):
            a = random_samples(capi, enc, h, w, seed=h + w)
            ctx.upload_image(a, enc, LOWER, UPPER)
            assert_bits(ctx.download("elevation"), R.layer_order(R.add_layer_from_image(a, LOWER, UPPER)), (enc, shape))


def test_message_at_an_odd_offset_sets_the_geometry(capi):
    L = capi.load()
    with capi.Context(0) as ctx:
        a = random_samples(capi, "mono16", 37, 53, seed=1)
        msg = capi.image_msg(a, "mono16", is_bigendian=1, frame_id="odom", seq=4, stamp=(5, 6))
        assert capi.image_parse(msg)[1] % 2 == 1  # 16-bit samples on odd addresses
        info = ctx.upload_image_msg(msg, 0.1, (1.5, -2.25), LOWER, UPPER)
        assert (info.height, info.width, info.frame_id, info.seq) == (37, 53, b"odom", 4)
        assert geometry_of(capi, ctx) == (37, 53, 0.1, 1.5, -2.25)
        assert_bits(ctx.download("elevation"), R.layer_order(R.add_layer_from_image(a, LOWER, UPPER)), "message")
        # a second image of another size resets the geometry
        b = random_samples(capi, "rgba8", 20, 31, seed=2)
        ctx.upload_image_msg(capi.image_msg(b, "rgba8", frame_id="ab"), 0.25, (0.5, 0.75), LOWER, UPPER)
        assert geometry_of(capi, ctx) == (20, 31, 0.25, 0.5, 0.75)
        want = R.layer_order(R.add_layer_from_image(b, LOWER, UPPER))
        assert_bits(ctx.download("elevation"), want, "second message")
        # te_upload_image does not: an image of another size is refused and the layer stays as it was
        info = capi.TeImageInfo(height=37, width=53, step=106, channels=1, bytes_per_channel=2)
        assert upload_raw(capi, ctx, info, a.tobytes()) == capi.TE_ERR_INVALID_ARG
        assert b"does not correspond to grid map size" in L.te_last_error()
        assert_bits(ctx.download("elevation"), want, "after the refused image")
        # the other refusals that need a context
        info = capi.TeImageInfo(height=20, width=31, step=124, channels=4, bytes_per_channel=1)
        for kw, word in ((dict(alpha=-0.01), b"alpha_threshold"), (dict(alpha=1.5), b"alpha_threshold"), (dict(alpha=float("nan")), b"alpha_threshold"),
                         (dict(lower=float("inf")), b"lower"), (dict(upper=float("nan")), b"upper")):
            assert upload_raw(capi, ctx, info, b.tobytes(), **kw) == capi.TE_ERR_INVALID_ARG, kw
            assert word in L.te_last_error(), (kw, L.te_last_error())
        info.step = 123
        assert upload_raw(capi, ctx, info, b.tobytes()) == capi.TE_ERR_INVALID_ARG and b"step 123" in L.te_last_error()
        info.step, info.channels = 124, 2
        assert upload_raw(capi, ctx, info, b.tobytes()) == capi.TE_ERR_INVALID_ARG
        assert L.te_upload_image(ctx._h, None, None, 0, 0, 0.0, 1.0, 0.5) == capi.TE_ERR_INVALID_ARG
        assert_bits(ctx.download("elevation"), want, "after the refused arguments")
    with capi.Context(0) as ctx:  # no geometry yet
        info = capi.TeImageInfo(height=20, width=31, step=124, channels=4, bytes_per_channel=1)
        assert upload_raw(capi, ctx, info, b.tobytes()) == capi.TE_ERR_NOT_READY


def test_state_equals_upload_elevation_of_the_same_floats(capi):
    h, w = 96, 80
    flags = capi.RUN_FOOTPRINT | capi.RUN_KEEP_NORMALS
    layers = ("elevation", "traversability_slope", "traversability_step", "traversability_roughness", "traversability",
              "traversability_footprint", "surface_normal_x", "surface_normal_y", "surface_normal_z")
    # a smooth surface with noise in the colour channels, 1 % alpha holes
    rng = np.random.default_rng(7)
    ii, jj = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    base = 120 + 60 * np.sin(ii / 9.0) * np.cos(jj / 7.0)
    a = np.clip(base[..., None] + rng.integers(-3, 4, (h, w, 4)), 0, 255).astype(np.uint8)
    a[..., 3] = np.where(rng.random((h, w)) < 0.01, 0, 255)
    floats = R.add_layer_from_image(a, 0.0, 0.4)
    assert 20 < np.isnan(floats).sum() < 200
    with capi.Context(0) as A, capi.Context(0) as B:
        for ctx in (A, B):
            ctx.set_params(capi.default_params())
            ctx.set_geometry(h, w, 1, 0.03, (0.3, -0.4))
        A.upload_image(a, "rgba8", 0.0, 0.4)
        B.upload_elevation(R.layer_order(floats))
        for ctx in (A, B):
            ctx.run_chain(flags)
            ctx.sync()
        for k in layers:
            assert_bits(A.download(k), B.download(k), k)
        assert np.isfinite(A.download("traversability")).sum() > h * w // 2
        # a new image drops what was computed from the old one: the footprint pass needs the chain again
        A.run_chain(0)
        A.upload_image(a, "rgba8", 0.0, 0.4)
        with pytest.raises(capi.TeError) as e:
            A.run_footprint()
        assert e.value.code == capi.TE_ERR_NOT_READY


def test_batch_image_goes_into_one_map(capi):
    h, w = 37, 53
    with capi.Context(0) as ctx:
        ctx.set_geometry(h, w, 3, 0.1)
        before = np.random.default_rng(0).random(3 * h * w).astype(np.float32)
        ctx.upload_elevation(before)
        a = random_samples(capi, "rgb8", h, w, seed=3)
        ctx.upload_image(a, "rgb8", LOWER, UPPER, map_index=1)
        got = ctx.download("elevation").reshape(3, -1)
        assert_bits(got[0], before[:h * w], "map 0")
        assert_bits(got[1], R.layer_order(R.add_layer_from_image(a, LOWER, UPPER)), "map 1")
        assert_bits(got[2], before[2 * h * w:], "map 2")
        for m in (3, -1):
            with pytest.raises(capi.TeError) as e:
                ctx.upload_image(a, "rgb8", LOWER, UPPER, map_index=m)
            assert e.value.code == capi.TE_ERR_INVALID_ARG


def test_image_into_robot_slope(capi):
    h, w, res = 24, 40, 0.1
    with capi.Context(0) as ctx:
        ctx.set_geometry(h, w, 1, res)
        a = np.full((h, w), 255, np.uint8)
        a[5, 11] = 0

        def pos(i, j):  # centre of cell (i, j): grid_map's x runs against the rows, y against the columns
            return (0.5 * h * res - (i + 0.5) * res, 0.5 * w * res - (j + 0.5) * res)
        seg = np.array([pos(5, 11) * 2, pos(6, 11) * 2, pos(5, 0) + pos(5, 30), pos(4, 0) + pos(4, 30)])
        with pytest.raises(capi.TeError) as e:
            ctx.check_inclination(seg)
        assert e.value.code == capi.TE_ERR_NOT_READY
        ctx.upload_image(a, "mono8", 0.0, 1.0, layer="robot_slope")
        assert_bits(ctx.download("robot_slope"), R.layer_order(R.add_layer_from_image(a, 0.0, 1.0)), "robot_slope")
        ok, st = ctx.check_inclination(seg)
        assert list(st) == [0, 0, 0, 0] and list(ok) == [False, True, False, True]


def test_python_row_stride_is_the_step(capi):
    h, w = 37, 53
    with capi.Context(0) as ctx:
        ctx.set_geometry(h, w, 1, 0.1)
        for enc in ("mono16", "rgb8"):
            ch, bpc = capi.IMAGE_ENCODINGS[enc]
            a = random_samples(capi, enc, h, w, seed=8)
            wide = np.full((h, w + 3) + a.shape[2:], 0xAB, a.dtype)
            wide[:, :w] = a
            view = wide[:, :w][:, ::1]
            assert not view.flags["C_CONTIGUOUS"] and view.strides[0] == (w + 3) * ch * bpc
            ctx.upload_image(view, enc, LOWER, UPPER)
            got = ctx.download("elevation")
            ctx.upload_image(np.ascontiguousarray(view), enc, LOWER, UPPER)
            assert_bits(got, ctx.download("elevation"), enc)
            assert_bits(got, R.layer_order(R.add_layer_from_image(a, LOWER, UPPER)), enc)
        # a view no step describes (every other column) is copied first
        a = random_samples(capi, "mono8", h, 2 * w, seed=9)
        ctx.upload_image(a[:, ::2], None, LOWER, UPPER)
        assert_bits(ctx.download("elevation"), R.layer_order(R.add_layer_from_image(a[:, ::2], LOWER, UPPER)), "strided columns")
