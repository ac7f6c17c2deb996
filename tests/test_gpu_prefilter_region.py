"""te_upload_layer_tile, te_run_median_fill_region and te_run_radius_filter_region on the device.  Both filters are defined bit
for bit, so the yardstick of a region call is the library's own whole-map call on the updated input (a second context):
out_layer, the fill mask and out_rect agree bit for bit, and nothing outside out_rect is written (a sentinel survives there).
The planned rectangle is restated here: the dirty rectangle grown by the reach and clamped to the map; the reach of the fill is
max(r_fill + 2 k, r_existing if filter_existing_values else 0), that of a disc of c cells is floor(c) (the radii used here
have their farthest cell on an axis).  Every TE_OPT_MEDIAN_ROUTE / TE_OPT_RADIUS_ROUTE, every rectangle of the list below.
The full tick of INTEGRATION.md (tile into a holding layer, region fill, region mean into the elevation, te_run_chain_region) is
held against the oracle on the filtered elevation within helpers.TOL."""
import math

import numpy as np
import pytest

from tests.helpers import OUT_LAYERS, assert_layers_match, to_te_params

pytestmark = pytest.mark.gpu

RES = 0.05
HOLD, MID, OUT = "robot_slope", "traversability_footprint", "traversability_roughness"
SENTINEL = np.float32(-12345.0)
# (rows, cols, batch, the map the region lies on)
SHAPES = [(67, 45, 1, 0), (131, 70, 3, 1)]
ROUTES = (0, 1, 2)
# (r_fill, k, filter_existing_values, r_existing) in cells; 16 cells takes the general kernel on every route
MEDIAN_CASES = [(1, 0, False, 0), (1, 2, False, 0), (2, 0, False, 0), (2, 2, False, 0), (16, 0, False, 0), (16, 2, False, 0), (2, 2, True, 1), (1, 0, True, 1)]
RADIUS_CELLS = [0.0, 1.5, 2.0, 3.0, 9.0]
OPS = (1, 2)


@pytest.fixture(scope="module")
def capi():
    from traversability_estimation_amd import build, capi
    build.build_lib()
    return capi


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def relief(rows, cols, batch, seed):
    """[batch][cols][rows] (the device's order): smooth relief, 10 % scattered NaN, a NaN block, a few +-inf."""
    from traversability_estimation_amd import synth
    rng = np.random.default_rng(seed)
    maps = []
    for b in range(batch):
        a = synth.perlin_elevation(rows, cols, seed=seed * 10 + b, amplitude=0.3).astype(np.float32).reshape(cols, rows).copy()
        a[rng.random(a.shape) < 0.10] = np.nan
        a[cols // 3:cols // 3 + 9, rows // 4:rows // 4 + 14] = np.nan
        idx = rng.choice(a.size, 6, replace=False)
        a.ravel()[idx[:3]] = np.inf
        a.ravel()[idx[3:]] = -np.inf
        maps.append(a)
    return np.stack(maps)


def patch_for(rng, h, w):
    """New values of a dirty rectangle, shape (w, h): other relief, other holes."""
    t = rng.uniform(-0.5, 0.5, (w, h)).astype(np.float32)
    t[rng.random(t.shape) < 0.2] = np.nan
    if t.size > 4:
        t.ravel()[rng.integers(0, t.size)] = np.inf
    return t


def rectangles(rows, cols):
    """name -> a list of (row0, col0, h, w) run in sequence with no whole-map call between them"""
    return {"one_cell": [(rows // 2, cols // 2, 1, 1)],
            "corner_00": [(0, 0, 8, 8)], "corner_0c": [(0, cols - 8, 8, 8)], "corner_r0": [(rows - 8, 0, 8, 8)], "corner_rc": [(rows - 8, cols - 8, 8, 8)],
            "strip": [(0, cols // 2, rows, 5)],
            "whole": [(0, 0, rows, cols)],
            "overlapping": [(10, 6, 20, 12), (22, 12, 30, 14)]}


def planned(rect, reach, rows, cols):
    r0, c0, h, w = rect
    i0, j0, i1, j1 = max(r0 - reach, 0), max(c0 - reach, 0), min(r0 + h + reach, rows), min(c0 + w + reach, cols)
    return (i0, j0, i1 - i0, j1 - j0)


def union(a, b):
    i0, j0 = min(a[0], b[0]), min(a[1], b[1])
    i1, j1 = max(a[0] + a[2], b[0] + b[2]), max(a[1] + a[3], b[1] + b[3])
    return (i0, j0, i1 - i0, j1 - j0)


def inside_mask(rect, rows, cols):
    m = np.zeros((cols, rows), bool)
    m[rect[1]:rect[1] + rect[3], rect[0]:rect[0] + rect[2]] = True
    return m


def context(capi, rows, cols, batch, option=None, value=0):
    ctx = capi.Context(0)
    ctx.set_params(capi.default_params())
    ctx.set_geometry(rows, cols, batch, RES)
    if option is not None:
        ctx.set_option(option, value)
    return ctx


def median_params(capi, r_fill, k, fev, r_exist):
    return capi.default_median_fill_params(fill_hole_radius=(r_fill + 0.5) * RES, num_erode_dilation_iterations=k, filter_existing_values=1 if fev else 0,
                                           existing_value_radius=(r_exist + 0.5) * RES if fev else 0.0)


def run_region_cases(capi, shape, option, route, reach, whole, region, with_mask, seed):
    """whole(ctx): the whole-map call HOLD -> OUT; region(ctx, map, rect) -> out_rect.  Every rectangle list of rectangles():
    assertions 1 and 2 of the module's docstring.  Contexts A (incremental) and B (from scratch) are shared by the lists."""
    rows, cols, batch, m = shape
    rng = np.random.default_rng(seed)
    base = relief(rows, cols, batch, seed)
    with context(capi, rows, cols, batch, option, route) as A, context(capi, rows, cols, batch, option, route) as B:
        for name, rects in rectangles(rows, cols).items():
            what = f"{name} {shape} route {route} reach {reach}"
            cur = base.copy()
            A.upload_layer(HOLD, cur)
            whole(A)
            before = A.download(OUT).reshape(batch, cols, rows).copy()
            written = None
            for n, rect in enumerate(rects):
                r0, c0, h, w = rect
                patch = patch_for(rng, h, w)
                cur[m, c0:c0 + w, r0:r0 + h] = patch
                A.upload_layer_tile(HOLD, patch, m, r0, c0)
                plan = planned(rect, reach, rows, cols)
                if len(rects) == 1:  # 2.: a sentinel everywhere outside the planned rectangle
                    marked = before.copy()
                    marked[m][~inside_mask(plan, rows, cols)] = SENTINEL
                    A.upload_layer(OUT, marked)
                got_rect = region(A, m, rect)
                assert got_rect == plan, (what, n, got_rect, plan)
                written = plan if written is None else union(written, plan)
            B.upload_layer(HOLD, cur)
            whole(B)
            want = B.download(OUT).reshape(batch, cols, rows)
            got = A.download(OUT).reshape(batch, cols, rows)
            assert np.array_equal(bits(A.download(HOLD)), bits(cur.reshape(-1))), what  # upload_layer_tile == upload_layer of the patched array
            ins = inside_mask(written, rows, cols)
            bad = np.argwhere((bits(got[m]) != bits(want[m])) & ins)
            assert bad.size == 0, f"{what}: {len(bad)} cells of out_rect differ from the whole-map call, first (col, row) {bad[:5].tolist()}"
            if len(rects) == 1:
                assert np.all(bits(got[m][~ins]) == bits(SENTINEL)), f"{what}: written outside out_rect"
            else:  # 1.: the whole layer, after two region calls in sequence
                assert np.array_equal(bits(got[m]), bits(want[m])), what
            for other in range(batch):
                if other != m:
                    assert np.array_equal(bits(got[other]), bits(before[other])) and np.array_equal(bits(want[other]), bits(before[other])), (what, other)
            if with_mask:
                assert np.array_equal(A.download_fill_mask(m), B.download_fill_mask(m)), f"{what}: fill mask"


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s[:3])))
@pytest.mark.parametrize("case", MEDIAN_CASES, ids=lambda c: "r%d_k%d_%s%d" % (c[0], c[1], "fev" if c[2] else "keep", c[3]))
def test_median_fill_region_equals_the_whole_call(capi, shape, case):
    r_fill, k, fev, r_exist = case
    p = median_params(capi, r_fill, k, fev, r_exist)
    reach = max(r_fill + 2 * k, r_exist if fev else 0)
    for route in ROUTES:
        run_region_cases(capi, shape, capi.OPT_MEDIAN_ROUTE, route, reach, lambda ctx: ctx.run_median_fill(p, HOLD, OUT),
                         lambda ctx, m, rect: ctx.run_median_fill_region(p, HOLD, OUT, m, *rect), True, 1000 * r_fill + 10 * k + shape[0])


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s[:3])))
@pytest.mark.parametrize("cells", RADIUS_CELLS)
@pytest.mark.parametrize("op", OPS, ids=["mean", "min"])
def test_radius_filter_region_equals_the_whole_call(capi, shape, cells, op):
    reach = int(math.floor(cells))
    for route in ROUTES:
        run_region_cases(capi, shape, capi.OPT_RADIUS_ROUTE, route, reach, lambda ctx: ctx.run_radius_filter(op, cells * RES, HOLD, OUT),
                         lambda ctx, m, rect: ctx.run_radius_filter_region(op, cells * RES, HOLD, OUT, m, *rect), False, int(10 * cells) + shape[0] + op)


def test_radius_region_stats_count_the_region_call(capi):
    rows, cols, batch, m = SHAPES[1]
    base = relief(rows, cols, batch, 5)
    for route, slot in ((1, 0), (2, 1)):
        with context(capi, rows, cols, batch, capi.OPT_RADIUS_ROUTE, route) as ctx:
            ctx.upload_layer(HOLD, base)
            ctx.run_radius_filter(1, 1.5 * RES, HOLD, OUT)
            assert sum(ctx.radius_filter_stats()) > 3
            rect = ctx.run_radius_filter_region(2, 1.5 * RES, HOLD, OUT, m, 70, 20, 3, 3)  # Min: every sliding workgroup settles
            assert rect == (69, 19, 5, 5)
            counts = ctx.radius_filter_stats()
            assert counts[slot] >= 1 and counts[1 - slot] == 0 and sum(counts) <= 2, (route, counts)  # 5 x 5 cells: one tile / two column groups


def test_full_tick_into_the_elevation_matches_the_oracle(capi, oracle):
    """the raw tile into the holding layer, region fill into a second layer, region mean into the elevation,
    te_run_chain_region on the last out_rect.  The elevation equals the whole-map fill + mean bit for bit and the scores match
    the oracle on that elevation."""
    from traversability_estimation_amd import synth
    rows, cols = 131, 70
    op = oracle.default_params()
    p = median_params(capi, 2, 1, False, 0)
    rng = np.random.default_rng(77)
    raw = synth.with_holes(synth.perlin_elevation(rows, cols, seed=31, amplitude=0.3), 0.05, seed=3).astype(np.float32).reshape(cols, rows).copy()
    raw[20:29, 40:52] = np.nan

    def prefilter(ctx):
        ctx.upload_layer(HOLD, raw)
        ctx.run_median_fill(p, HOLD, MID)
        ctx.run_radius_filter("mean", 1.5 * RES, MID, "elevation")

    with context(capi, rows, cols, 1) as A, context(capi, rows, cols, 1) as B:
        A.set_params(to_te_params(capi, op))
        prefilter(A)
        A.run_chain()
        for rect in [(50, 30, 24, 16), (0, 0, 8, 8), (60, 38, 40, 20)]:
            r0, c0, h, w = rect
            patch = synth.perlin_elevation(h, w, seed=int(rng.integers(1 << 20)), amplitude=0.4).astype(np.float32).reshape(w, h).copy()
            patch[rng.random(patch.shape) < 0.1] = np.nan
            raw[c0:c0 + w, r0:r0 + h] = patch
            A.upload_layer_tile(HOLD, patch, 0, r0, c0)
            filled = A.run_median_fill_region(p, HOLD, MID, 0, r0, c0, h, w)
            assert filled == planned(rect, 4, rows, cols)
            smoothed = A.run_radius_filter_region("mean", 1.5 * RES, MID, "elevation", 0, *filled)
            assert smoothed == planned(filled, 1, rows, cols)
            A.run_chain_region(0, *smoothed)
        A.sync()
        prefilter(B)
        elev = B.download("elevation")
        assert np.array_equal(bits(A.download("elevation")), bits(elev))
        assert np.array_equal(bits(A.download(MID)), bits(B.download(MID)))
        got = {k: A.download(k) for k in OUT_LAYERS}
    want = oracle.chain(oracle.geom(rows, cols, RES), op, elev.reshape(cols, rows))
    assert_layers_match(got, want, ctx="prefiltered region tick")


def all_layers(ctx):
    return {k: bits(ctx.download(k)).copy() for k in ("elevation", HOLD, MID, OUT) + OUT_LAYERS}


def test_errors_leave_every_layer_as_it_was(capi):
    rows, cols, batch = 67, 45, 2
    base = relief(rows, cols, batch, 9)
    p = median_params(capi, 1, 1, False, 0)
    with context(capi, rows, cols, batch) as ctx:
        ctx.upload_elevation(base)
        ctx.upload_layer(HOLD, base)
        ctx.run_median_fill(p, HOLD, MID)
        ctx.run_radius_filter("min", 1.5 * RES, HOLD, OUT)
        ctx.run_chain()
        before = all_layers(ctx)
        mask = ctx.download_fill_mask(1).copy()
        calls = {"fill": lambda i, o, m, rect: ctx.run_median_fill_region(p, i, o, m, *rect),
                 "radius": lambda i, o, m, rect: ctx.run_radius_filter_region("mean", 1.5 * RES, i, o, m, *rect)}
        ok = (3, 4, 5, 6)
        refused = [(HOLD, HOLD, 0, ok, capi.TE_ERR_INVALID_ARG, "in_layer == out_layer"), ("elevation", "elevation", 1, ok, capi.TE_ERR_INVALID_ARG, "in_layer == out_layer"),
                   (HOLD, OUT, 0, (-1, 0, 4, 4), capi.TE_ERR_INVALID_ARG, "rectangle"), (HOLD, OUT, 0, (0, 0, 0, 4), capi.TE_ERR_INVALID_ARG, "rectangle"),
                   (HOLD, OUT, 0, (0, 0, 4, -2), capi.TE_ERR_INVALID_ARG, "rectangle"), (HOLD, OUT, 0, (60, 0, 8, 4), capi.TE_ERR_INVALID_ARG, "rectangle"),
                   (HOLD, OUT, 0, (0, 40, 4, 6), capi.TE_ERR_INVALID_ARG, "rectangle"), (HOLD, OUT, 0, (0, 2 ** 31 - 1, 1, 1), capi.TE_ERR_INVALID_ARG, "rectangle"),
                   (HOLD, OUT, batch, ok, capi.TE_ERR_INVALID_ARG, "map"), (HOLD, OUT, -1, ok, capi.TE_ERR_INVALID_ARG, "map"),
                   (15, OUT, 0, ok, capi.TE_ERR_INVALID_ARG, "layer"), (HOLD, 15, 0, ok, capi.TE_ERR_INVALID_ARG, "layer"), (-1, OUT, 0, ok, capi.TE_ERR_INVALID_ARG, "layer"),
                   ("traversability_x", OUT, 0, ok, capi.TE_ERR_NOT_READY, "layer"), (HOLD, "traversability_x", 0, ok, capi.TE_ERR_INVALID_ARG, "memory")]
        for name, call in calls.items():
            for i, o, m, rect, code, word in refused:
                with pytest.raises(capi.TeError) as e:
                    call(i, o, m, rect)
                assert e.value.code == code and word in str(e.value), (name, i, o, m, rect, str(e.value))
        with pytest.raises(capi.TeError) as e:
            ctx.run_radius_filter_region(3, 0.1, HOLD, OUT, 0, *ok)
        assert e.value.code == capi.TE_ERR_INVALID_ARG
        with pytest.raises(capi.TeError) as e:
            ctx.run_radius_filter_region(1, -0.1, HOLD, OUT, 0, *ok)
        assert e.value.code == capi.TE_ERR_BAD_PARAM
        with pytest.raises(capi.TeError) as e:
            ctx.run_median_fill_region(median_params(capi, 1, -1, False, 0), HOLD, OUT, 0, *ok)
        assert e.value.code == capi.TE_ERR_BAD_PARAM
        tile = np.zeros((4, 4), np.float32)
        for layer, m, r0, c0, code in [(15, 0, 0, 0, capi.TE_ERR_INVALID_ARG), ("traversability_x", 0, 0, 0, capi.TE_ERR_INVALID_ARG), (HOLD, batch, 0, 0, capi.TE_ERR_INVALID_ARG),
                                       (HOLD, 0, 64, 0, capi.TE_ERR_INVALID_ARG), (HOLD, 0, 0, -1, capi.TE_ERR_INVALID_ARG), ("elevation", 0, 0, 42, capi.TE_ERR_INVALID_ARG)]:
            with pytest.raises(capi.TeError) as e:
                ctx.upload_layer_tile(layer, tile, m, r0, c0)
            assert e.value.code == code, (layer, m, r0, c0)
        after = all_layers(ctx)
        for k in before:
            assert np.array_equal(before[k], after[k]), k
        assert np.array_equal(mask, ctx.download_fill_mask(1))
        ctx.run_chain_region(0, 0, 0, 4, 4)  # the refused calls changed no fact of the context either: the chain's results still stand


def test_fill_mask_needs_a_whole_fill_first(capi):
    rows, cols, batch = 67, 45, 2
    base = relief(rows, cols, batch, 11)
    p = median_params(capi, 1, 0, False, 0)
    with context(capi, rows, cols, batch) as ctx:
        ctx.upload_layer(HOLD, base)
        assert ctx.run_median_fill_region(p, HOLD, OUT, 0, 5, 5, 4, 4) == (4, 4, 6, 6)
        with pytest.raises(capi.TeError) as e:
            ctx.download_fill_mask(0)
        assert e.value.code == capi.TE_ERR_NOT_READY
        ctx.run_median_fill(p, HOLD, OUT, 1, 1)  # map 1 only
        ctx.run_median_fill_region(p, HOLD, OUT, 0, 5, 5, 4, 4)
        with pytest.raises(capi.TeError) as e:
            ctx.download_fill_mask(0)
        assert e.value.code == capi.TE_ERR_NOT_READY
        assert ctx.download_fill_mask(1).shape == (cols, rows)


def test_upload_layer_tile_on_the_elevation_is_upload_tile(capi):
    from traversability_estimation_amd import synth
    rows, cols = 131, 70
    elev = synth.perlin_elevation(rows, cols, seed=5, amplitude=0.3).astype(np.float32)
    patch = synth.perlin_elevation(20, 12, seed=6, amplitude=0.4).astype(np.float32).reshape(12, 20)
    got = []
    for use_layer_call in (False, True):
        with context(capi, rows, cols, 1) as ctx:
            ctx.upload_elevation(elev)
            ctx.run_chain()
            if use_layer_call:
                ctx.upload_layer_tile("elevation", patch, 0, 40, 30)
            else:
                ctx.upload_tile(patch, 0, 40, 30)
            ctx.run_chain_region(0, 40, 30, 20, 12)  # (needs the done-flags the tile upload keeps)
            ctx.sync()
            got.append({k: bits(ctx.download(k)) for k in ("elevation",) + OUT_LAYERS})
    for k in got[0]:
        assert np.array_equal(got[0][k], got[1][k]), k
    assert not np.array_equal(got[0]["elevation"], bits(elev.reshape(-1)))


def test_upload_layer_tile_on_another_layer_is_upload_layer_of_the_patched_array(capi):
    rows, cols, batch = 67, 45, 3
    base = relief(rows, cols, batch, 13)
    patch = patch_for(np.random.default_rng(1), 9, 7)
    for layer in (HOLD, OUT, "traversability", "surface_normal_z"):
        with context(capi, rows, cols, batch) as ctx:
            ctx.upload_layer(layer, base)
            ctx.upload_layer_tile(layer, patch, 2, 58, 38)
            want = base.copy()
            want[2, 38:45, 58:67] = patch
            assert np.array_equal(bits(ctx.download(layer)), bits(want.reshape(-1))), layer
    with context(capi, rows, cols, batch) as ctx:  # robot_slope gets its memory from its first write, a tile included: NaN elsewhere
        ctx.upload_layer_tile(HOLD, patch, 0, 0, 0)
        got = ctx.download(HOLD).reshape(batch, cols, rows)
        assert np.array_equal(bits(got[0, :7, :9]), bits(patch)) and np.isnan(got[1:]).all() and np.isnan(got[0, 7:]).all()
