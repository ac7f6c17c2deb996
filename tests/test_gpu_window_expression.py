"""te_run_window_expression on the device, through capi, against the numpy restatement tests/ref_py/window_expression_ref.py.
Rule 5 of the contract defines the reductions bit for bit, so every comparison but the transcendental one is array_equal on the
bit patterns (every NaN counting as the same value), under every TE_OPT_WINDOW_EXPR_ROUTE: 0 by plan, 1 the separable route
wherever allowed, 2 the direct walk.  te_window_expression_stats shows which route settled the workgroups.  Shapes, windows and
expressions: tests/window_expression_cases.py (tests/test_window_plan.py checks on the CPU that each of them takes the route
claimed here)."""
import numpy as np
import pytest

from tests import window_expression_cases as K
from tests.helpers import OUT_LAYERS
from tests.ref_py import expression_ref as E
from tests.ref_py import window_expression_ref as R

pytestmark = pytest.mark.gpu

ROUTES = (0, 1, 2)
OUT = "traversability_roughness"
X = K.X


@pytest.fixture(scope="module")
def capi():
    from traversability_estimation_amd import build, capi
    build.build_lib()
    return capi


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    from tests import test_window_plan as P
    exe = P.build(tmp_path_factory.mktemp("window_plan_gpu"), ["-O2"])
    return lambda *a: P.route(exe, *a), P.off_lds_window(exe)


_REF = {}


def reference(maps, text, w, edge, empty=True):
    """[batch] (rows, cols) layers -> the filtered stack; computed once per input and setting, never changed."""
    key = (tuple(m.tobytes() for m in maps), maps[0].shape, text, w, edge, empty)
    if key not in _REF:
        out = np.stack([R.window_expression(m, text, X, w, edge, empty) for m in maps])
        out.setflags(write=False)
        _REF[key] = out
    return _REF[key]


def to_device(maps):
    return np.ascontiguousarray(np.stack([m.T for m in maps]), np.float32).reshape(-1)


def from_device(flat, batch, rows, cols):
    return flat.reshape(batch, cols, rows).transpose(0, 2, 1)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def context(capi, maps, route=0, params=None):
    batch, (rows, cols) = len(maps), maps[0].shape
    ctx = capi.Context(0)
    ctx.set_params(capi.default_params() if params is None else params)
    ctx.set_geometry(rows, cols, batch, K.RES)
    ctx.set_option(capi.OPT_WINDOW_EXPR_ROUTE, route)
    ctx.upload_elevation(to_device(maps))
    return ctx


def prm(capi, w, edge, empty=True):
    return capi.window_expr_params(window_size=w, edge_handling=edge, compute_empty_cells=empty)


def run(ctx, capi, maps, text, w, edge, empty=True, out=OUT):
    ctx.run_window_expression(text, prm(capi, w, edge, empty), "elevation", out)
    return from_device(ctx.download(out), len(maps), *maps[0].shape)


def check_exact(capi, plan, maps, texts, windows, edges, empties=(True, False), what=""):
    route_of, _ = plan
    batch, (rows, cols) = len(maps), maps[0].shape
    for option in ROUTES:
        with context(capi, maps, option) as ctx:
            for text, reductions, outer in texts:
                for w in windows:
                    for edge in edges:
                        for empty in empties:
                            want = reference(maps, text, w, edge, empty)
                            got = run(ctx, capi, maps, text, w, edge, empty)
                            assert E.same_bits(got, want), f"{what} {text} w {w} {edge} empty {empty} option {option} {(rows, cols, batch)}: " \
                                                           f"{int((bits(got) != bits(want)).sum())} cells differ"
                        # the stats: what the plan says, per map
                        _kind, _staged, sep, direct = route_of(rows, cols, w, edge, reductions, outer, option)
                        assert ctx.window_expression_stats() == (sep * batch, direct * batch), (text, w, edge, option)
                        if option == 2 or outer:
                            assert ctx.window_expression_stats()[0] == 0
            # the input is as it was
            assert np.array_equal(bits(from_device(ctx.download("elevation"), batch, rows, cols)), bits(np.stack(maps)))


@pytest.mark.parametrize("w", K.WINDOWS)
@pytest.mark.parametrize("rows,cols,batch", K.SHAPES)
def test_windows_edge_handlings_and_expressions(capi, plan, rows, cols, batch, w):
    maps = K.maps(rows, cols, batch, 100 * rows + cols + w)
    check_exact(capi, plan, maps, K.EXACT, [w], K.EDGES)


@pytest.mark.parametrize("kind", ["none", "all_nan", "inf_cells", "single_finite", "block_30", "frame"])
def test_hole_patterns(capi, plan, kind):
    maps = K.maps(70, 37, 1, 7, [kind])
    check_exact(capi, plan, maps, K.EXACT[:6], [5], K.EDGES, empties=(True, False), what=kind)


@pytest.mark.parametrize("rows,cols,batch", K.OFF_LDS_SHAPES)
def test_the_smallest_window_off_the_lds_tile(capi, plan, rows, cols, batch):
    route_of, off = plan
    assert not route_of(rows, cols, off, "crop", 1, 0, 1)[1] and route_of(rows, cols, off - 2, "crop", 1, 0, 1)[1]  # staged below it, not at it
    maps = K.maps(rows, cols, batch, 3)
    small = rows < 10
    check_exact(capi, plan, maps, K.EXACT[:2] if not small else K.EXACT, [off], K.EDGES if small else ("crop", "mean"), empties=(True,))


def test_window_length(capi):
    maps = K.maps(70, 37, 1, 11)
    text = K.EXACT[1][0]
    for length, w in ((0.25, 5), (0.1, 3), (0.02, 1)):
        assert R.window_size(window_length=length, resolution=K.RES) == w
        for option in ROUTES:
            with context(capi, maps, option) as ctx:
                ctx.run_window_expression(text, capi.window_expr_params(window_length=length, edge_handling="crop"), "elevation", OUT)
                got = from_device(ctx.download(OUT), 1, 70, 37)
                assert E.same_bits(got, reference(maps, text, w, "crop")), (length, option)


# Largest distance of meanOfFinites(exp(x)) to the float64 numpy reference measured on the MI355X over this test's inputs
# (printed by the test).  The terms are positive, so a per-term bound carries to the sum: the bound is
# twice the measured distance plus 1 for the final rounding, at least 2 ulp.  Above 8 ulp the function is refused outright.
MEASURED_EXP_MEAN_ULP = 2


def test_mean_of_exp_within_the_measured_bound(capi):
    rng = np.random.default_rng(19)
    a = rng.uniform(-4.0, 4.0, (70, 37)).astype(np.float32)
    a[rng.random(a.shape) < 0.05] = np.nan
    worst = 0
    for option in ROUTES:
        with context(capi, [a], option) as ctx:
            for w in (3, 9):
                for edge in ("crop", "empty"):
                    got = run(ctx, capi, [a], K.EXP_MEAN, w, edge)
                    d = E.ulp_distance(got, reference([a], K.EXP_MEAN, w, edge))  # (asserts that the NaN positions agree)
                    print(f"{K.EXP_MEAN} w {w} {edge} option {option}: {d} ulp")
                    worst = max(worst, d)
    assert worst <= 8, worst
    assert worst <= max(2, 2 * MEASURED_EXP_MEAN_ULP + 1), worst


def test_window_one_is_the_identity_on_finite_cells(capi):
    maps = K.maps(70, 37, 1, 13, ["inf_cells"])
    for option in ROUTES:
        with context(capi, maps, option) as ctx:
            got = run(ctx, capi, maps, f"meanOfFinites({X})", 1, "crop")
            fin = np.isfinite(maps[0])
            assert np.array_equal(bits(got[0][fin]), bits(maps[0][fin])) and np.isnan(got[0][~fin]).all(), option


def test_a_window_over_the_whole_map_equals_the_per_map_reductions(capi):
    """w = 2 * max(rows, cols) - 1 with `crop`: every cell's window is the map, and min / max / count of the finite values do not
    depend on the order: they equal te_run_expression's reductions over the map exactly."""
    rows, cols = 5, 7
    maps = K.maps(rows, cols, 1, 17)
    w = 2 * max(rows, cols) - 1
    for option in ROUTES:
        with context(capi, maps, option) as ctx:
            for fn in ("minOfFinites", "maxOfFinites", "numberOfFinites"):
                got = run(ctx, capi, maps, f"{fn}({X})", w, "crop")
                ctx.run_expression(f"{fn}({X})")
                whole = from_device(ctx.download("traversability"), 1, rows, cols)
                assert np.array_equal(bits(got), bits(whole)), (fn, option)
                assert len(np.unique(bits(got))) == 1


def test_in_place_equals_out_of_place_and_other_layers(capi):
    maps = K.maps(70, 37, 1, 23)
    other = K.maps(70, 37, 1, 24, ["inf_cells"], "mixed_signs")
    text = K.STD_DEV.replace(X, "traversability_slope")
    for option in ROUTES:
        with context(capi, maps, option) as ctx:
            ctx.upload_layer("traversability_slope", to_device(other))
            p = prm(capi, 5, "crop")
            ctx.run_window_expression(text, p, "traversability_slope", "robot_slope")
            apart = ctx.download("robot_slope")
            assert np.array_equal(bits(ctx.download("traversability_slope")), bits(to_device(other)))  # the input is bit-identical afterwards
            ctx.run_window_expression(text, p, "traversability_slope")  # in place
            assert np.array_equal(bits(ctx.download("traversability_slope")), bits(apart)), option
            want = R.window_expression(other[0], text, "traversability_slope", 5, "crop")
            assert E.same_bits(from_device(apart, 1, 70, 37)[0], want), option
            assert np.array_equal(bits(from_device(ctx.download("elevation"), 1, 70, 37)), bits(np.stack(maps)))


def test_a_map_range_leaves_the_other_maps_untouched(capi):
    rows, cols, batch = K.SHAPES[3]
    maps = K.maps(rows, cols, batch, 5)
    for option in ROUTES:
        for text, _, _ in K.EXACT[:2]:
            want = reference(maps, text, 3, "crop")
            with context(capi, maps, option) as ctx:
                ctx.upload_layer(OUT, np.full(batch * rows * cols, 7.25, np.float32))
                ctx.run_window_expression(text, prm(capi, 3, "crop"), "elevation", OUT, map0=1, nmaps=2)
                got = from_device(ctx.download(OUT), batch, rows, cols)
                assert (got[0] == 7.25).all()
                assert E.same_bits(got[1:], want[1:]), (option, text)


def test_chain_after_a_box_mean_in_place(capi):
    """The elevation written in place, then te_run_chain: the layers of a context that uploaded the same filtered values."""
    rows, cols = 200, 128
    rng = np.random.default_rng(53)
    from tests import median_fill_cases as M
    a = M.values("bag", rng, rows, cols)
    a.ravel()[rng.choice(a.size, a.size // 100, replace=False)] = np.nan
    text = f"meanOfFinites({X})"
    smooth = reference([a], text, 5, "crop")
    assert np.isnan(a).any() and not np.isnan(smooth).any()
    for option in ROUTES:
        with context(capi, [a], option) as A, context(capi, list(smooth)) as B:
            A.run_window_expression(text, prm(capi, 5, "crop"))
            assert np.array_equal(bits(from_device(A.download("elevation"), 1, rows, cols)), bits(smooth))
            for ctx in (A, B):
                ctx.run_chain(0)
                ctx.sync()
            for k in OUT_LAYERS:
                assert np.array_equal(bits(A.download(k)), bits(B.download(k))), (option, k)
            assert np.array_equal(A.download_face_flags(), B.download_face_flags())


def test_refusals(capi):
    with capi.Context(0) as ctx:
        with pytest.raises(capi.TeError) as e:  # before any call
            ctx.window_expression_stats()
        assert e.value.code == capi.TE_ERR_NOT_READY
        p = prm(capi, 3, "crop")
        with pytest.raises(capi.TeError) as e:  # no geometry
            ctx.run_window_expression(f"mean({X})", p, nmaps=1)
        assert e.value.code == capi.TE_ERR_NOT_READY
        ctx.set_geometry(16, 9, 2, K.RES)
        with pytest.raises(capi.TeError) as e:  # no elevation yet
            ctx.run_window_expression(f"mean({X})", p, "elevation", OUT)
        assert e.value.code == capi.TE_ERR_NOT_READY
        ctx.upload_elevation(np.zeros(2 * 16 * 9, np.float32))
        for layer, out in ((-1, 3), (15, 3), (0, -1), (0, 15), (0, 12)):  # bad ids; traversability_x has no memory
            with pytest.raises(capi.TeError) as e:
                ctx.run_window_expression(f"mean({X})", p, layer, out)
            assert e.value.code == capi.TE_ERR_INVALID_ARG, (layer, out)
        for map0, nmaps in ((-1, 1), (0, 0), (0, 3), (2, 1), (1, 2)):
            with pytest.raises(capi.TeError) as e:
                ctx.run_window_expression(f"mean({X})", p, map0=map0, nmaps=nmaps)
            assert e.value.code == capi.TE_ERR_INVALID_ARG, (map0, nmaps)
        for text, code in ((f"abs({X})", capi.TE_ERR_BAD_PARAM), ("mean(traversability)", capi.TE_ERR_BAD_PARAM), (f"sum(sum(sum({X})))", capi.TE_ERR_BAD_PARAM),
                           (f"sum({X} * {X})", capi.TE_ERR_UNSUPPORTED)):
            with pytest.raises(capi.TeError) as e:
                ctx.run_window_expression(text, p)
            assert e.value.code == code and "column" in str(e.value), text
        with pytest.raises(capi.TeError) as e:
            ctx.set_option(capi.OPT_WINDOW_EXPR_ROUTE, 3)
        assert e.value.code == capi.TE_ERR_INVALID_ARG
        ctx.run_window_expression(f"mean({X})", p)
        assert sum(ctx.window_expression_stats()) == 4  # 1 x 2 workgroups per map, 2 maps
