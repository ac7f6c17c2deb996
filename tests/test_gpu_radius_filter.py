"""te_run_radius_filter on the device, through capi, against the numpy restatement tests/ref_py/radius_filter_ref.py.  The Mean
is defined bit for bit (a double sum in iterator order) and the Min is one of its inputs, so every comparison is array_equal on
the bit patterns, under every TE_OPT_RADIUS_ROUTE: 0 by plan, 1 the sliding kernel, 2 the in-order gather.  te_radius_filter_stats
shows which kernel settled the workgroups.  Shapes, radii and inputs: tests/radius_filter_cases.py (tests/test_radius_plan.py checks on
the CPU that each of them takes the kernel claimed here)."""
import numpy as np
import pytest

from tests import median_fill_cases as M
from tests import radius_filter_cases as K
from tests.helpers import OUT_LAYERS
from tests.ref_py import radius_filter_ref as R
from tests.ref_py.grid_map_ref import GridMapRef

pytestmark = pytest.mark.gpu

ROUTES = (0, 1, 2)
OUT = "traversability_roughness"


@pytest.fixture(scope="module")
def capi():
    from traversability_estimation_amd import build, capi
    build.build_lib()
    return capi


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


_REF = {}


def reference(maps, cells, op, pos=(0.0, 0.0)):
    """[batch] (rows, cols) layers -> the filtered stack; computed once per input and setting, never changed."""
    key = (tuple(m.tobytes() for m in maps), maps[0].shape, cells, op, pos)
    if key not in _REF:
        gm = GridMapRef(maps[0].shape[0], maps[0].shape[1], K.RES, pos)
        out = np.stack([R.radius_filter(m, gm, K.radius_of(cells), op) for m in maps])
        out.setflags(write=False)
        _REF[key] = out
    return _REF[key]


def to_device(maps):
    return np.ascontiguousarray(np.stack([m.T for m in maps]), np.float32).reshape(-1)


def from_device(flat, batch, rows, cols):
    return flat.reshape(batch, cols, rows).transpose(0, 2, 1)


def context(capi, rows, cols, batch, maps=None, route=0, pos=(0.0, 0.0), params=None):
    ctx = capi.Context(0)
    ctx.set_params(capi.default_params() if params is None else params)
    ctx.set_geometry(rows, cols, batch, K.RES, pos)
    ctx.set_option(capi.OPT_RADIUS_ROUTE, route)
    if maps is not None:
        ctx.upload_elevation(to_device(maps))
    return ctx


def run_and_check(capi, maps, cells, ops=K.OPS, routes=ROUTES, pos=(0.0, 0.0), what=""):
    """elevation -> traversability_roughness for every op on every route, against the reference.  -> {(op, route): stats}"""
    batch, (rows, cols) = len(maps), maps[0].shape
    stats = {}
    for route in routes:
        with context(capi, rows, cols, batch, maps, route, pos) as ctx:
            for op in ops:
                want = reference(maps, cells, op, pos)
                ctx.run_radius_filter(op, K.radius_of(cells), "elevation", OUT)
                got = from_device(ctx.download(OUT), batch, rows, cols)
                bad = np.argwhere(bits(got) != bits(want))
                assert bad.size == 0, f"{what} op {op} route {route} {(rows, cols, batch)} at {cells} cells: {len(bad)} cells differ, " \
                                      f"{[(tuple(b), float(got[tuple(b)]), float(want[tuple(b)])) for b in bad[:6]]}"
                stats[(op, route)] = ctx.radius_filter_stats()
                if route == 2:
                    assert stats[(op, route)][0] == 0 and stats[(op, route)][1] > 0, (what, op, stats[(op, route)])
            # the input is as it was
            assert np.array_equal(bits(from_device(ctx.download("elevation"), batch, rows, cols)), bits(np.stack(maps)))
    return stats


holey_maps = K.holey_maps


def hole_kinds_for(n, batch):
    kind = M.HOLE_KINDS[n]
    return [kind] if batch == 1 else [kind, M.HOLE_KINDS[(n + 3) % len(M.HOLE_KINDS)], M.HOLE_KINDS[(n + 5) % len(M.HOLE_KINDS)]]


# maps smaller than the window (5 x 7); 70 x 37 and 130 x 33: workgroup edges and partial workgroups in both directions; a batch
# of 3, every map with another hole pattern
@pytest.mark.parametrize("cells", K.RADII_CELLS)
@pytest.mark.parametrize("rows,cols,batch", K.SHAPES)
def test_radii_and_hole_patterns(capi, rows, cols, batch, cells):
    for n, kind in enumerate(M.HOLE_KINDS):
        maps = holey_maps(rows, cols, batch, 100 * rows + cols + int(2 * cells), hole_kinds_for(n, batch))
        stats = run_and_check(capi, maps, cells, what=kind)
        assert stats[(K.MEAN, 0)][1] == 0 and stats[(K.MEAN, 0)][0] > 0, (kind, stats)  # `bag` values: every workgroup is provable
        assert stats[(K.MIN, 0)][1] == 0, (kind, stats)
        if cells == 0.0 and batch == 1 and kind != "inf_cells":  # the centre cell alone: the identity on finite cells
            assert np.array_equal(bits(reference(maps, cells, K.MIN)[0]), bits(maps[0]))
            assert np.array_equal(bits(reference(maps, cells, K.MEAN)[0]), bits(maps[0]))
        if kind == "all_nan" and batch == 1:
            assert np.isnan(reference(maps, cells, K.MEAN)).all()


@pytest.mark.parametrize("cells", K.TIE_CELLS)
@pytest.mark.parametrize("rows,cols,batch", K.SHAPES)
def test_tie_radii_with_an_off_grid_map_position(capi, rows, cols, batch, cells):
    for n, kind in enumerate(M.HOLE_KINDS):
        maps = holey_maps(rows, cols, batch, 7 * rows + cols + cells, hole_kinds_for(n, batch))
        stats = run_and_check(capi, maps, cells, pos=K.OFF_GRID, what=kind)
        assert stats[(K.MEAN, 0)][1] == 0, (kind, stats)


@pytest.mark.parametrize("kind", K.VALUE_KINDS)
def test_values(capi, kind):
    for rows, cols in K.VALUE_SHAPES:
        for cells in K.VALUE_RADII_CELLS:
            for holes in K.VALUE_HOLES:
                maps = holey_maps(rows, cols, 1, K.value_seed(rows, cells), [holes], kind)
                stats = run_and_check(capi, maps, cells, what=f"{kind} {holes}")
                for route in (0, 1):
                    if kind in K.UNPROVABLE_KINDS:  # the sliding Mean hands its workgroups to the gather
                        assert stats[(K.MEAN, route)][1] > 0, (kind, route, stats)
                    else:
                        assert stats[(K.MEAN, route)][1] == 0 and stats[(K.MEAN, route)][0] > 0, (kind, route, stats)
                    assert stats[(K.MIN, route)][1] == 0, (kind, route, stats)  # a minimum has no order


def test_block_level_routing(capi):
    """One tiny region of cancelling values costs the workgroups that read it, not the map."""
    rows, cols, batch = K.BLOCK_ROUTING
    a = K.block_routing_map(np.random.default_rng(K.BLOCK_ROUTING_SEED))
    for cells in K.VALUE_RADII_CELLS:
        stats = run_and_check(capi, [a], cells, what="block routing")
        for route in (0, 1):
            slide, gather = stats[(K.MEAN, route)]
            assert slide > 0 and gather > 0, (cells, route, stats)


def test_a_window_larger_than_the_map(capi):
    rows, cols, batch, cells = K.BIG_WINDOW
    for kind in ("speckle_5", "single_finite"):
        run_and_check(capi, holey_maps(rows, cols, batch, 41, [kind]), cells, what=kind)
    maps = holey_maps(5, 7, 1, 43, ["speckle_5"])
    run_and_check(capi, maps, 1.0e6, what="a radius far beyond the map")
    assert len(np.unique(bits(reference(maps, 1.0e6, K.MEAN)[np.isfinite(reference(maps, 1.0e6, K.MEAN))]))) == 1


def test_a_map_range_leaves_the_other_maps_untouched(capi):
    rows, cols, batch = K.SHAPES[3]
    maps = holey_maps(rows, cols, batch, 5, ["speckle_5", "block_30", "inf_cells"])
    for route in ROUTES:
        for op in K.OPS:
            want = reference(maps, 3.5, op)
            with context(capi, rows, cols, batch, maps, route) as ctx:
                ctx.upload_layer(OUT, np.full(batch * rows * cols, 7.25, np.float32))
                ctx.run_radius_filter(op, K.radius_of(3.5), "elevation", OUT, map0=1, nmaps=2)
                got = from_device(ctx.download(OUT), batch, rows, cols)
                assert (got[0] == 7.25).all()
                assert np.array_equal(bits(got[1:]), bits(want[1:])), (route, op)


def test_in_place_equals_out_of_place(capi):
    rows, cols, batch = 70, 37, 1
    maps = holey_maps(rows, cols, batch, 31, ["speckle_5"])
    for route in ROUTES:
        for op in K.OPS:
            want = reference(maps, 3.5, op)
            with context(capi, rows, cols, batch, maps, route) as ctx:
                ctx.run_radius_filter(op, K.radius_of(3.5), "elevation", OUT)
                scratch = ctx.download(OUT)
                ctx.run_radius_filter(op, K.radius_of(3.5))  # elevation, in place
                inplace = ctx.download("elevation")
                assert np.array_equal(bits(inplace), bits(scratch)), (route, op)
                assert np.array_equal(bits(from_device(inplace, batch, rows, cols)), bits(want)), (route, op)


def test_chain_after_a_mean_in_place(capi, oracle):
    """A Mean that leaves no NaN: the recount finds a hole-free elevation, and the chain equals the oracle chain run on the
    reference's smoothed map (and the chain of a context that was given that map through te_upload_elevation, bit for bit)."""
    from tests.helpers import assert_layers_match, to_te_params
    rows, cols, batch = 200, 128, 1
    rng = np.random.default_rng(53)
    a = M.values("bag", rng, rows, cols)
    a.ravel()[rng.choice(a.size, a.size // 100, replace=False)] = np.nan
    smooth = reference([a], 3.5, K.MEAN)
    assert np.isnan(a).any() and not np.isnan(smooth).any()
    op = oracle.default_params()
    want = oracle.chain(oracle.geom(rows, cols, K.RES), op, to_device(list(smooth)))
    p = to_te_params(capi, op)
    for route in ROUTES:
        with context(capi, rows, cols, batch, [a], route, params=p) as A, context(capi, rows, cols, batch, list(smooth), params=p) as B:
            A.run_radius_filter(K.MEAN, K.radius_of(3.5))
            assert np.array_equal(bits(from_device(A.download("elevation"), batch, rows, cols)), bits(smooth))
            for ctx in (A, B):
                ctx.run_chain(0)
                ctx.sync()
            got = {k: A.download(k) for k in OUT_LAYERS}
            assert_layers_match(got, want, ctx=f"route {route}")
            for k in OUT_LAYERS:
                assert np.array_equal(bits(got[k]), bits(B.download(k))), (route, k)
            assert np.array_equal(A.download_face_flags(), B.download_face_flags())


def test_another_layer_leaves_the_elevation_alone(capi):
    rows, cols, batch = 70, 37, 1
    maps = holey_maps(rows, cols, batch, 59, ["speckle_5"])
    other = holey_maps(rows, cols, batch, 60, ["inf_cells"], "mixed_signs")
    for op in K.OPS:
        want = reference(other, 1.5, op)
        with context(capi, rows, cols, batch, maps) as ctx:
            ctx.upload_layer("traversability_slope", to_device(other))
            ctx.run_radius_filter(op, K.radius_of(1.5), "traversability_slope", "robot_slope")
            assert np.array_equal(bits(from_device(ctx.download("robot_slope"), batch, rows, cols)), bits(want))
            ctx.run_radius_filter(op, K.radius_of(1.5), "traversability_slope")  # in place on a layer that is not the elevation
            assert np.array_equal(bits(from_device(ctx.download("traversability_slope"), batch, rows, cols)), bits(want))
            assert np.array_equal(bits(from_device(ctx.download("elevation"), batch, rows, cols)), bits(np.stack(maps)))


def test_mean_of_negative_zeros_is_positive_zero(capi):
    rows, cols = 70, 37
    a = np.full((rows, cols), -0.0, np.float32)
    a[40:, 20:] = 1.5
    for route in ROUTES:
        with context(capi, rows, cols, 1, [a], route) as ctx:
            ctx.run_radius_filter(K.MEAN, K.radius_of(1.5), "elevation", OUT)
            got = from_device(ctx.download(OUT), 1, rows, cols)[0]
            assert bits(got[:30, :15]).max() == 0, route  # +0.0, not -0.0
            assert np.array_equal(bits(got), bits(reference([a], 1.5, K.MEAN)[0]))


def test_repeated_calls_give_identical_bits(capi):
    rows, cols, batch = 130, 33, 1
    for kind in ("bag", "cancel"):
        maps = holey_maps(rows, cols, batch, 61, ["speckle_5"], kind)
        for route in ROUTES:
            for op in K.OPS:
                with context(capi, rows, cols, batch, maps, route) as ctx:
                    outs = []
                    for _ in range(2):
                        ctx.run_radius_filter(op, K.radius_of(3.5), "elevation", OUT)
                        outs.append(ctx.download(OUT))
                    assert np.array_equal(bits(outs[0]), bits(outs[1])), (kind, route, op)


def test_refusals(capi):
    with capi.Context(0) as ctx:
        with pytest.raises(capi.TeError) as e:  # before any call
            ctx.radius_filter_stats()
        assert e.value.code == capi.TE_ERR_NOT_READY
        with pytest.raises(capi.TeError) as e:  # no geometry
            ctx.run_radius_filter(K.MEAN, 0.1, nmaps=1)
        assert e.value.code == capi.TE_ERR_NOT_READY
        ctx.set_geometry(16, 9, 2, K.RES)
        for layer in ("elevation", "surface_normal_x", "robot_slope", "traversability_x", "slope_footprint"):  # do not exist yet
            with pytest.raises(capi.TeError) as e:
                ctx.run_radius_filter(K.MIN, 0.1, layer, OUT)
            assert e.value.code == capi.TE_ERR_NOT_READY, layer
        ctx.upload_elevation(np.zeros(2 * 16 * 9, np.float32))
        for layer, out in ((-1, 3), (15, 3), (0, -1), (0, 15), (0, 12)):  # bad ids; traversability_x has no memory
            with pytest.raises(capi.TeError) as e:
                ctx.run_radius_filter(K.MEAN, 0.1, layer, out)
            assert e.value.code == capi.TE_ERR_INVALID_ARG, (layer, out)
        for map0, nmaps in ((-1, 1), (0, 0), (0, 3), (2, 1), (1, 2)):
            with pytest.raises(capi.TeError) as e:
                ctx.run_radius_filter(K.MEAN, 0.1, map0=map0, nmaps=nmaps)
            assert e.value.code == capi.TE_ERR_INVALID_ARG, (map0, nmaps)
        for bad in (-0.05, float("nan"), float("inf")):
            with pytest.raises(capi.TeError) as e:
                ctx.run_radius_filter(K.MEAN, bad)
            assert e.value.code == capi.TE_ERR_BAD_PARAM, bad
        for op in (0, 3, -1):
            with pytest.raises(capi.TeError) as e:
                ctx.run_radius_filter(op, 0.1)
            assert e.value.code == capi.TE_ERR_INVALID_ARG, op
        with pytest.raises(capi.TeError) as e:
            ctx.set_option(capi.OPT_RADIUS_ROUTE, 3)
        assert e.value.code == capi.TE_ERR_INVALID_ARG
        ctx.run_radius_filter("min", 0.1)
        assert sum(ctx.radius_filter_stats()) > 0
