"""te_run_median_fill on the device, through capi, against the numpy restatement tests/ref_py/median_fill_ref.py.  Selection has no
rounding, so every comparison is array_equal on the bit patterns; both kernels (TE_OPT_MEDIAN_ROUTE 1: the tile kernel, 2: the
general kernel) unless a test says otherwise.  Shapes, radii and inputs: tests/median_fill_cases.py (tests/test_median_plan.py
checks on the CPU that each of them takes the kernel claimed here)."""
import numpy as np
import pytest

from tests import median_fill_cases as K
from tests.ref_py import median_fill_ref as R

pytestmark = pytest.mark.gpu

ROUTES = (1, 2)
FIVE = ("traversability_slope", "traversability_step", "traversability_roughness", "traversability", "traversability_footprint")


@pytest.fixture(scope="module")
def capi():
    from traversability_estimation_amd import build, capi
    build.build_lib()
    return capi


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


_REF = {}


def reference(maps, r_fill, k=0, filter_existing=False, r_exist=0):
    """(outputs, masks) of a [batch] list of (rows, cols) layers; computed once per input and setting, never changed."""
    key = (tuple(m.tobytes() for m in maps), maps[0].shape, r_fill, k, filter_existing, r_exist)
    if key not in _REF:
        got = [R.median_fill(m, K.RES, K.radius_for(r_fill), filter_existing, K.radius_for(r_exist) if r_exist else 0.0, k) for m in maps]
        outs, masks = np.stack([g[0] for g in got]), np.stack([g[1] for g in got])
        outs.setflags(write=False)
        masks.setflags(write=False)
        _REF[key] = (outs, masks)
    return _REF[key]


def params(capi, r_fill, k=0, filter_existing=False, r_exist=0):
    return capi.default_median_fill_params(fill_hole_radius=K.radius_for(r_fill), num_erode_dilation_iterations=k,
                                           filter_existing_values=1 if filter_existing else 0,
                                           existing_value_radius=K.radius_for(r_exist) if r_exist else 0.0)


def to_device(maps):
    """[batch] (rows, cols) arrays -> the flat column-major layers."""
    return np.ascontiguousarray(np.stack([m.T for m in maps]), np.float32).reshape(-1)


def from_device(flat, batch, rows, cols):
    return flat.reshape(batch, cols, rows).transpose(0, 2, 1)


def context(capi, rows, cols, batch, maps=None, route=0):
    ctx = capi.Context(0)
    ctx.set_params(capi.default_params())
    ctx.set_geometry(rows, cols, batch, K.RES)
    ctx.set_option(capi.OPT_MEDIAN_ROUTE, route)
    if maps is not None:
        ctx.upload_elevation(to_device(maps))
    return ctx


def fill_and_check(capi, maps, r_fill, k=0, filter_existing=False, r_exist=0, routes=ROUTES, what=""):
    """Fills elevation -> traversability_roughness on every route; layer and mask against the reference.  Returns the output."""
    batch, (rows, cols) = len(maps), maps[0].shape
    want, want_mask = reference(maps, r_fill, k, filter_existing, r_exist)
    p = params(capi, r_fill, k, filter_existing, r_exist)
    for route in routes:
        with context(capi, rows, cols, batch, maps, route) as ctx:
            ctx.run_median_fill(p, "elevation", "traversability_roughness")
            got = from_device(ctx.download("traversability_roughness"), batch, rows, cols)
            bad = np.argwhere(bits(got) != bits(want))
            assert bad.size == 0, f"{what} route {route} {(rows, cols, batch)} r {r_fill} k {k}: {[(tuple(b), float(got[tuple(b)]), float(want[tuple(b)])) for b in bad[:6]]}"
            for m in range(batch):
                mask = ctx.download_fill_mask(m).T
                assert np.array_equal(mask, want_mask[m].astype(np.uint8)), (what, "mask, route", route, "map", m, np.argwhere(mask != want_mask[m])[:6])
            # the input is as it was
            assert np.array_equal(bits(from_device(ctx.download("elevation"), batch, rows, cols)), bits(np.stack(maps)))
    return want


def holey_maps(rows, cols, batch, seed, kinds, values="bag"):
    rng = np.random.default_rng(seed)
    maps = [K.punch(kinds[m % len(kinds)], rng, K.values(values, rng, rows, cols)) for m in range(batch)]
    assert not any(np.any(np.signbit(m) & (m == 0)) for m in maps)  # no -0.0: the one value whose sign the contract leaves open
    return maps


# maps smaller than the window (5 x 7 at r = 3 and 7); 70 x 37 and 130 x 33: tile edges and partial tiles in both directions;
# a batch of 3, every map with another hole pattern
@pytest.mark.parametrize("r", K.RADII)
@pytest.mark.parametrize("rows,cols,batch", K.SHAPES)
def test_shapes_radii_and_hole_patterns(capi, rows, cols, batch, r):
    for n, kind in enumerate(K.HOLE_KINDS):
        kinds = [kind] if batch == 1 else [kind, K.HOLE_KINDS[(n + 3) % len(K.HOLE_KINDS)], K.HOLE_KINDS[(n + 5) % len(K.HOLE_KINDS)]]
        maps = holey_maps(rows, cols, batch, 100 * rows + cols + r, kinds)
        want = fill_and_check(capi, maps, r, what=kind)
        if kind == "none" and batch == 1:  # nothing to fill: the output is the input bit for bit
            assert np.array_equal(bits(want), bits(np.stack(maps)))
        if kind == "all_nan" and batch == 1:
            assert np.isnan(want).all()
        if kind == "frame" and batch == 1 and rows > 4 * r + 6 and cols > 4 * r + 6:
            assert np.isnan(want[0][rows // 2, cols // 2]) and (r == 0 or np.isfinite(want[0][2, cols // 2]))


def test_a_map_range_leaves_the_other_maps_untouched(capi):
    rows, cols, batch = K.SHAPES[3]
    maps = holey_maps(rows, cols, batch, 5, ["speckle_5", "block_30", "inf_cells"])
    want, want_mask = reference(maps, 1)
    for route in ROUTES:
        with context(capi, rows, cols, batch, maps, route) as ctx:
            marker = np.full(batch * rows * cols, 7.25, np.float32)
            ctx.upload_layer("traversability_roughness", marker)
            ctx.run_median_fill(params(capi, 1), "elevation", "traversability_roughness", map0=1, nmaps=2)
            got = from_device(ctx.download("traversability_roughness"), batch, rows, cols)
            assert (got[0] == 7.25).all()
            assert np.array_equal(bits(got[1:]), bits(want[1:]))
            assert np.array_equal(ctx.download_fill_mask(2).T, want_mask[2].astype(np.uint8))
            with pytest.raises(capi.TeError) as e:  # map 0 was never covered
                ctx.download_fill_mask(0)
            assert e.value.code == capi.TE_ERR_NOT_READY


@pytest.mark.parametrize("kind", K.VALUE_KINDS)
def test_values(capi, kind):
    rows, cols = 70, 37
    for r in (1, 3):
        maps = holey_maps(rows, cols, 1, 17 + r, ["speckle_5"], kind)
        fill_and_check(capi, maps, r, what=kind)
        maps = holey_maps(rows, cols, 1, 19 + r, ["inf_cells"], kind)
        fill_and_check(capi, maps, r, what=kind + " with inf")
        fill_and_check(capi, maps, r, filter_existing=True, r_exist=1, what=kind + " with inf, filtered")


@pytest.mark.parametrize("k", [0, 1, 4])
def test_erode_dilate_iterations(capi, k):
    for rows, cols in ((70, 37), (130, 33)):
        rng = np.random.default_rng(rows + k)
        a = K.values("bag", rng, rows, cols)
        a[rng.random((rows, cols)) < 0.55] = np.nan  # islands of every size: the opening removes the small ones
        a[: rows // 3, : cols // 2] = K.values("bag", rng, rows, cols)[: rows // 3, : cols // 2]  # and a solid part that survives
        a[5, 5] = np.nan
        want_mask = reference([a], 1, k)[1]
        if k == 4:
            assert want_mask.any() and (want_mask.sum() < reference([a], 1, 0)[1].sum())  # (the opening does something here)
        fill_and_check(capi, [a], 1, k=k)
        fill_and_check(capi, [a], 3, k=k)
    for kind in ("single_finite", "frame", "all_nan", "none"):
        fill_and_check(capi, holey_maps(70, 37, 1, 3, [kind]), 1, k=k, what=kind)


@pytest.mark.parametrize("r_exist", [0, 1])
def test_filter_existing_values(capi, r_exist):
    for rows, cols in ((70, 37), (5, 7)):
        maps = holey_maps(rows, cols, 1, 23, ["speckle_5"], "mixed_signs")
        want = fill_and_check(capi, maps, 3, filter_existing=True, r_exist=r_exist)
        plain = reference(maps, 3)[0]
        if r_exist == 0:  # the identity on finite cells
            assert np.array_equal(bits(want), bits(plain))
        else:
            assert not np.array_equal(bits(want), bits(plain))
    # the existing radius above the fill radius: the halo is the larger one
    fill_and_check(capi, holey_maps(70, 37, 1, 29, ["speckle_5"]), 1, k=1, filter_existing=True, r_exist=3)


def test_in_place_equals_out_of_place(capi):
    rows, cols, batch = 70, 37, 1
    maps = holey_maps(rows, cols, batch, 31, ["speckle_5"])
    for r, k, fe, re_ in ((3, 0, False, 0), (1, 1, True, 1)):
        want = reference(maps, r, k, fe, re_)[0]
        for route in ROUTES:
            with context(capi, rows, cols, batch, maps, route) as ctx:
                ctx.run_median_fill(params(capi, r, k, fe, re_), "elevation", "traversability_roughness")
                scratch = ctx.download("traversability_roughness")
                ctx.run_median_fill(params(capi, r, k, fe, re_))  # elevation, in place
                inplace = ctx.download("elevation")
                assert np.array_equal(bits(inplace), bits(scratch))
                assert np.array_equal(bits(from_device(inplace, batch, rows, cols)), bits(want))


def test_a_window_the_tile_kernel_does_not_take(capi):
    """r = 40 on 96 x 80 takes the general kernel by plan (tests/test_median_plan.py); forced at r = 1 and 3 it equals the tile kernel."""
    rows, cols, batch, r = K.BIG_WINDOW
    for kind in ("speckle_5", "single_finite"):
        fill_and_check(capi, holey_maps(rows, cols, batch, 41, [kind]), r, routes=(0,), what=kind)
    fill_and_check(capi, holey_maps(rows, cols, batch, 43, ["speckle_5"]), r, k=1, filter_existing=True, r_exist=1, routes=(0,))
    for small in (1, 3):
        maps = holey_maps(rows, cols, batch, 47, ["speckle_5"])
        fill_and_check(capi, maps, small, routes=(1, 2))


def chain_and_footprint(capi, ctx):
    ctx.run_chain(capi.RUN_FOOTPRINT)
    ctx.sync()
    return {name: ctx.download(name) for name in FIVE}, ctx.download_face_flags()


@pytest.mark.parametrize("kind,r", [("speckle_1", 1), ("frame", 2)])
def test_state_after_the_fill(capi, kind, r):
    """Context A fills in place, context B is given the reference-filled array through te_upload_elevation; chain and footprint
    must give the same five layers bit for bit (the routing facts are those of the new contents, so the same kernels run) and the
    same face flags.  speckle: every hole is filled, both take the hole-free kernel; frame: holes stay, both take their march."""
    rows, cols, batch = K.STATE_SHAPE
    rng = np.random.default_rng(53)
    a = K.values("bag", rng, rows, cols)
    if kind == "speckle_1":
        a.ravel()[rng.choice(a.size, a.size // 100, replace=False)] = np.nan
    else:
        a = K.punch("frame", rng, a)
    filled = reference([a], r)[0]
    assert np.isnan(filled).any() == (kind == "frame") and np.isnan(a).sum() > np.isnan(filled).sum()
    for route in ROUTES:
        with context(capi, rows, cols, batch, [a], route) as A, context(capi, rows, cols, batch, list(filled)) as B:
            A.run_median_fill(params(capi, r))
            assert np.array_equal(bits(from_device(A.download("elevation"), batch, rows, cols)), bits(filled))
            got, got_flags = chain_and_footprint(capi, A)
            want, want_flags = chain_and_footprint(capi, B)
            for name in FIVE:
                assert np.array_equal(bits(got[name]), bits(want[name])), (kind, route, name)
            assert np.array_equal(got_flags, want_flags)
            # and once more after a second fill of the (now filled) layer: nothing left to do in the speckle case
            A.run_median_fill(params(capi, r))
            again, again_flags = chain_and_footprint(capi, A)
            if kind == "speckle_1":
                for name in FIVE:
                    assert np.array_equal(bits(again[name]), bits(want[name])), (kind, route, name, "second fill")
                assert np.array_equal(again_flags, want_flags)


def test_writing_another_layer_follows_its_upload(capi):
    """traversability written by the fill has no known bound (te_run_footprint still runs, on the route of any reach, and gives
    what it gives for the same values uploaded); robot_slope becomes present."""
    rows, cols, batch = 70, 37, 1
    maps = holey_maps(rows, cols, batch, 59, ["speckle_5"])
    want = reference(maps, 1)[0]
    with context(capi, rows, cols, batch, maps) as A, context(capi, rows, cols, batch, maps) as B:
        for ctx in (A, B):
            ctx.run_chain(0)
        A.run_median_fill(params(capi, 1), "elevation", "traversability")
        B.upload_layer("traversability", to_device(list(want)))
        for ctx in (A, B):
            ctx.run_footprint()
            ctx.sync()
        assert np.array_equal(bits(A.download("traversability")), bits(B.download("traversability")))
        assert np.array_equal(bits(A.download("traversability_footprint")), bits(B.download("traversability_footprint")))
        A.run_median_fill(params(capi, 1), "elevation", "robot_slope")
        assert np.array_equal(bits(from_device(A.download("robot_slope"), batch, rows, cols)), bits(want))
        A.run_median_fill(params(capi, 1), "robot_slope", "traversability_step")  # (present now: it can be read)


def test_repeated_calls_give_identical_bits(capi):
    rows, cols, batch = 130, 33, 1
    maps = holey_maps(rows, cols, batch, 61, ["speckle_5"])
    for route in ROUTES:
        with context(capi, rows, cols, batch, maps, route) as ctx:
            outs = []
            for _ in range(3):
                ctx.run_median_fill(params(capi, 3, 1, True, 1), "elevation", "traversability_roughness")
                outs.append(ctx.download("traversability_roughness"))
            assert np.array_equal(bits(outs[0]), bits(outs[1])) and np.array_equal(bits(outs[0]), bits(outs[2]))


def test_refusals(capi):
    p = capi.default_median_fill_params()
    with capi.Context(0) as ctx:
        with pytest.raises(capi.TeError) as e:  # no geometry
            ctx.run_median_fill(p, nmaps=1)
        assert e.value.code == capi.TE_ERR_NOT_READY
        ctx.set_geometry(16, 9, 2, K.RES)
        with pytest.raises(capi.TeError) as e:  # before any call
            ctx.download_fill_mask(0)
        assert e.value.code == capi.TE_ERR_NOT_READY
        for layer in ("elevation", "surface_normal_x", "robot_slope", "traversability_x", "slope_footprint"):  # do not exist yet
            with pytest.raises(capi.TeError) as e:
                ctx.run_median_fill(p, layer, "traversability_roughness")
            assert e.value.code == capi.TE_ERR_NOT_READY, layer
        ctx.upload_elevation(np.zeros(2 * 16 * 9, np.float32))
        for layer, out in ((-1, 3), (15, 3), (0, -1), (0, 15), (0, 12)):  # bad ids; traversability_x has no memory
            with pytest.raises(capi.TeError) as e:
                ctx.run_median_fill(p, layer, out)
            assert e.value.code == capi.TE_ERR_INVALID_ARG, (layer, out)
        for map0, nmaps in ((-1, 1), (0, 0), (0, 3), (2, 1), (1, 2)):
            with pytest.raises(capi.TeError) as e:
                ctx.run_median_fill(p, map0=map0, nmaps=nmaps)
            assert e.value.code == capi.TE_ERR_INVALID_ARG, (map0, nmaps)
        with pytest.raises(capi.TeError) as e:
            ctx.run_median_fill(capi.default_median_fill_params(fill_hole_radius=-1.0))
        assert e.value.code == capi.TE_ERR_BAD_PARAM
        ctx.run_median_fill(p)
        assert ctx.download_fill_mask(1).shape == (9, 16)
        with pytest.raises(capi.TeError) as e:
            capi._check(capi.load().te_download_fill_mask(ctx._h, 0, np.zeros(4, np.uint8).ctypes.data_as(capi.C.POINTER(capi.C.c_ubyte)), 4))
        assert e.value.code == capi.TE_ERR_INVALID_ARG
        with pytest.raises(capi.TeError) as e:
            ctx.set_option(capi.OPT_MEDIAN_ROUTE, 3)
        assert e.value.code == capi.TE_ERR_INVALID_ARG
        ctx.set_geometry(16, 9, 2, K.RES)  # the same shape: the mask is still not this geometry's
        with pytest.raises(capi.TeError) as e:
            ctx.download_fill_mask(0)
        assert e.value.code == capi.TE_ERR_NOT_READY
