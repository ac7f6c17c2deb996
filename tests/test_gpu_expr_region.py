"""te_run_window_expression_region, te_run_expression_region and te_run_chain_region_expression on the device.  Both
expression filters are defined bit for bit, so the yardstick of a region call is the library's own whole-map call on the edited
input in a second context: bits plus NaN pattern on every cell of every map, and nothing outside the planned rectangle moves.
The footprint layer behind the one-call tick is held to the CPU oracle on the context's own device layers, with the helpers and
the tolerance of the existing footprint tests."""
import numpy as np
import pytest

from tests.helpers import OUT_LAYERS, assert_layers_match, to_te_params
from tests.test_gpu_chain import check_fp
from tests.test_gpu_fp_any_reach import oracle_fp

pytestmark = pytest.mark.gpu

RES = 0.05
ROWS, COLS = 70, 45
HOLD, OUT = "robot_slope", "traversability_roughness"
STD_DEV = "sqrt(sumOfFinites(square(robot_slope - meanOfFinites(robot_slope))) ./ numberOfFinites(robot_slope))"
MEAN = "meanOfFinites(robot_slope)"
EDGES = ("inside", "crop", "empty", "mean")
# 1 x 1 in each corner, 1 x 1 interior at an odd origin, one straddling a 32-row and an 8-column tile seam, one touching two
# borders, the whole map
RECTS = [(0, 0, 1, 1), (ROWS - 1, 0, 1, 1), (0, COLS - 1, 1, 1), (ROWS - 1, COLS - 1, 1, 1), (37, 23, 1, 1), (29, 6, 7, 5), (58, 0, 12, 9), (0, 0, ROWS, COLS)]
SCORES = ("traversability_slope", "traversability_step", "traversability_roughness")
WEIGHTED = "(1.0 * traversability_slope + 1.0 * traversability_step + 1.0 * traversability_roughness) / 3.0"
CWISE_MIN = "cwiseMin(cwiseMin(traversability_slope, traversability_step), traversability_roughness)"


@pytest.fixture(scope="module")
def capi():
    from traversability_estimation_amd import build, capi
    build.build_lib()
    return capi


@pytest.fixture(scope="module")
def off_lds(tmp_path_factory):
    """the smallest window te_window_plan.h does not stage in LDS, and the plan's word on it"""
    from tests import test_window_region as P
    exe = P.build(tmp_path_factory.mktemp("window_region_gpu"), ["-O2"])
    w = int(P.out(exe, "offlds"))
    assert P.out(exe, "plan", ROWS, COLS, w, 1, 0, 0, 29, 6, 7, 5).split()[-1] == "0"      # not staged ...
    assert P.out(exe, "plan", ROWS, COLS, w - 2, 1, 0, 0, 29, 6, 7, 5).split()[-1] == "1"  # ... and the window before it is
    return w


def bits(a):
    return np.ascontiguousarray(a, np.float32).reshape(-1).view(np.uint32)


def same(a, b):
    """bits plus NaN pattern: every NaN counts as the same value"""
    a, b = np.asarray(a, np.float32).reshape(-1), np.asarray(b, np.float32).reshape(-1)
    an, bn = np.isnan(a), np.isnan(b)
    return np.array_equal(an, bn) and np.array_equal(bits(a[~an]), bits(b[~bn]))


def differing(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return ~((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b)))


def context(capi, rows, cols, batch=1, params=None):
    ctx = capi.Context(0)
    ctx.set_params(capi.default_params() if params is None else params)
    ctx.set_geometry(rows, cols, batch, RES)
    return ctx


def holed(rows, cols, batch, seed):
    """[batch][cols][rows]: relief with 5 % NaN"""
    rng = np.random.default_rng(seed)
    a = rng.uniform(-1.0, 3.0, (batch, cols, rows)).astype(np.float32)
    a[rng.random(a.shape) < 0.05] = np.nan
    return a


def patch_for(base, m, rect, seed):
    """the new values of the rectangle, shape (w, h); a single cell flips between a hole and a value"""
    r0, c0, h, w = rect
    rng = np.random.default_rng(seed)
    t = rng.uniform(-4.0, 9.0, (w, h)).astype(np.float32)
    t[rng.random(t.shape) < 0.2] = np.nan
    if h * w == 1:
        t[0, 0] = np.nan if np.isfinite(base[m, c0, r0]) and seed % 2 else np.float32(7.5)
    return t


def planned(rect, reach, rows=ROWS, cols=COLS):
    r0, c0, h, w = rect
    i0, j0, i1, j1 = max(r0 - reach, 0), max(c0 - reach, 0), min(r0 + h + reach, rows), min(c0 + w + reach, cols)
    return (i0, j0, i1 - i0, j1 - j0)


def inside_mask(rect, rows=ROWS, cols=COLS):
    m = np.zeros((cols, rows), bool)
    m[rect[1]:rect[1] + rect[3], rect[0]:rect[0] + rect[2]] = True
    return m


# ---- 1. the window expression on a rectangle ---------------------------------------------------------------------------------
def window_region_cases(capi, batch, m, w, edge, empty, seed):
    p = capi.window_expr_params(window_size=w, compute_empty_cells=bool(empty), edge_handling=edge)
    base = holed(ROWS, COLS, batch, seed)
    reach = (w - 1) // 2
    changed = 0
    with context(capi, ROWS, COLS, batch) as A, context(capi, ROWS, COLS, batch) as B:
        for text in (STD_DEV, MEAN):
            for ri, rect in enumerate(RECTS):
                r0, c0, h, wd = rect
                patch = patch_for(base, m, rect, seed + ri)
                cur = base.copy()
                cur[m, c0:c0 + wd, r0:r0 + h] = patch
                B.upload_layer(HOLD, cur)
                B.run_window_expression(text, p, HOLD, OUT)
                want = B.download(OUT).reshape(batch, COLS, ROWS).copy()
                plan = planned(rect, reach)
                ins = inside_mask(plan)
                got_by_route = []
                for route in (1, 2):
                    what = (text, w, edge, empty, rect, batch, route)
                    A.set_option(capi.OPT_WINDOW_EXPR_ROUTE, route)
                    A.upload_layer(HOLD, base)
                    A.run_window_expression(text, p, HOLD, OUT)
                    before = A.download(OUT).reshape(batch, COLS, ROWS).copy()
                    A.upload_layer_tile(HOLD, patch, m, r0, c0)
                    assert A.run_window_expression_region(text, p, HOLD, OUT, m, r0, c0, h, wd) == plan, what
                    got = A.download(OUT).reshape(batch, COLS, ROWS).copy()
                    bad = np.argwhere(differing(got, want))
                    assert bad.size == 0, f"{what}: {len(bad)} cells differ from the whole-map call, first (map, col, row) {bad[:5].tolist()}"
                    moved = differing(got, before)
                    assert not moved[m][~ins].any(), f"{what}: written outside out_rect"
                    assert not any(moved[o].any() for o in range(batch) if o != m), f"{what}: another map moved"
                    changed += int(moved.any())
                    got_by_route.append(got)
                assert same(got_by_route[0], got_by_route[1]), (text, w, edge, empty, rect)
    # (under `inside` a wide window leaves every cell unvisited; elsewhere the edits do move the result)
    assert changed > 0 or (edge == "inside" and 2 * reach >= min(ROWS, COLS))


@pytest.mark.parametrize("empty", (1, 0), ids=["all_cells", "finite_cells"])
@pytest.mark.parametrize("edge", EDGES)
@pytest.mark.parametrize("w", (1, 3, 9))
@pytest.mark.parametrize("batch,m", [(1, 0), (3, 1)], ids=["one_map", "batch3_map1"])
def test_window_region_equals_the_whole_map_call(capi, batch, m, w, edge, empty):
    window_region_cases(capi, batch, m, w, edge, empty, 100 * w + 10 * EDGES.index(edge) + empty)


@pytest.mark.parametrize("edge", EDGES)
def test_window_region_with_a_window_the_plan_does_not_stage(capi, off_lds, edge):
    window_region_cases(capi, 1, 0, off_lds, edge, 1, 7 + EDGES.index(edge))


def test_window_region_stats_count_the_region_call(capi):
    base = holed(ROWS, COLS, 1, 3)
    with context(capi, ROWS, COLS) as ctx:
        ctx.set_option(capi.OPT_WINDOW_EXPR_ROUTE, 1)
        ctx.upload_layer(HOLD, base)
        for edge in ("crop", "mean"):
            p = capi.window_expr_params(window_size=5, edge_handling=edge)
            ctx.run_window_expression(MEAN, p, HOLD, OUT)
            assert sum(ctx.window_expression_stats()) == 3 * 6  # the whole map: 3 x 6 tiles
            assert ctx.run_window_expression_region(MEAN, p, HOLD, OUT, 0, 30, 20, 3, 3) == (28, 18, 7, 7)  # interior: one tile, no window clipped
            sep, direct = ctx.window_expression_stats()
            assert sep >= 1 and sep + direct == 1, (edge, sep, direct)
        # `mean` on a rectangle whose tiles all have clipped windows: every workgroup walks directly
        p = capi.window_expr_params(window_size=5, edge_handling="mean")
        assert ctx.run_window_expression_region(MEAN, p, HOLD, OUT, 0, 0, 0, 3, 3) == (0, 0, 5, 5)
        assert ctx.window_expression_stats() == (0, 1)
        assert ctx.run_window_expression_region(MEAN, p, HOLD, OUT, 0, 0, 40, ROWS, 5) == (0, 38, ROWS, 7)  # the last columns: every tile at the border
        assert ctx.window_expression_stats() == (0, 3)


def test_window_region_into_the_elevation_is_followed_by_the_region_chain(capi):
    from traversability_estimation_amd import synth
    raw = synth.perlin_elevation(ROWS, COLS, seed=5, amplitude=0.3).astype(np.float32).reshape(1, COLS, ROWS).copy()
    p = capi.window_expr_params(window_size=3, edge_handling="crop")
    patch = np.full((6, 9), 0.4, np.float32)
    with context(capi, ROWS, COLS) as A, context(capi, ROWS, COLS) as B:
        A.upload_layer(HOLD, raw)
        A.run_window_expression(MEAN, p, HOLD, "elevation")
        A.run_chain()
        A.upload_layer_tile(HOLD, patch, 0, 30, 20)
        rect = A.run_window_expression_region(MEAN, p, HOLD, "elevation", 0, 30, 20, 9, 6)
        assert rect == (29, 19, 11, 8)
        A.run_chain_region(0, *rect)  # accepted: the done-flags stay, as after te_upload_tile
        A.sync()
        raw[0, 20:26, 30:39] = patch
        B.upload_layer(HOLD, raw)
        B.run_window_expression(MEAN, p, HOLD, "elevation")
        B.run_chain()
        B.sync()
        assert same(A.download("elevation"), B.download("elevation"))
        assert_layers_match({k: A.download(k) for k in OUT_LAYERS}, {k: B.download(k) for k in OUT_LAYERS}, ctx="window region into the elevation")


# ---- 2. errors ---------------------------------------------------------------------------------------------------------------
def test_window_region_errors_leave_the_layers_as_they_were(capi):
    base = holed(ROWS, COLS, 2, 9)
    p = capi.window_expr_params(window_size=3)
    with capi.Context(0) as ctx:
        ctx.set_params(capi.default_params())
        with pytest.raises(capi.TeError) as e:  # no geometry yet
            ctx.run_window_expression_region(MEAN, p, HOLD, OUT, 0, 3, 4, 5, 6)
        assert e.value.code == capi.TE_ERR_NOT_READY
    with context(capi, ROWS, COLS, 2) as ctx:
        ctx.upload_layer(HOLD, base)
        ctx.run_window_expression(MEAN, p, HOLD, OUT)
        before = {k: ctx.download(k).copy() for k in (HOLD, OUT)}
        ok = (3, 4, 5, 6)
        refused = [(HOLD, HOLD, 0, ok, capi.TE_ERR_INVALID_ARG, "in_layer == out_layer"),
                   (HOLD, OUT, 0, (-1, 0, 4, 4), capi.TE_ERR_INVALID_ARG, "rectangle"), (HOLD, OUT, 0, (0, 0, 0, 4), capi.TE_ERR_INVALID_ARG, "rectangle"),
                   (HOLD, OUT, 0, (64, 0, 8, 4), capi.TE_ERR_INVALID_ARG, "rectangle"), (HOLD, OUT, 0, (0, 40, 4, 6), capi.TE_ERR_INVALID_ARG, "rectangle"),
                   (HOLD, OUT, 0, (0, 2 ** 31 - 1, 1, 1), capi.TE_ERR_INVALID_ARG, "rectangle"),
                   (HOLD, OUT, 2, ok, capi.TE_ERR_INVALID_ARG, "map"), (HOLD, OUT, -1, ok, capi.TE_ERR_INVALID_ARG, "map"),
                   (HOLD, 15, 0, ok, capi.TE_ERR_INVALID_ARG, "layer"), ("surface_normal_z", OUT, 0, ok, capi.TE_ERR_NOT_READY, "layer")]
        for i, o, m, rect, code, word in refused:
            text = MEAN if i == HOLD else "meanOfFinites(surface_normal_z)"
            with pytest.raises(capi.TeError) as e:
                ctx.run_window_expression_region(text, p, i, o, m, *rect)
            assert e.value.code == code and word in str(e.value), (i, o, m, rect, str(e.value))
        with pytest.raises(capi.TeError) as e:  # the expression: as the whole-map call
            ctx.run_window_expression_region("abs(robot_slope)", p, HOLD, OUT, 0, *ok)
        assert e.value.code == capi.TE_ERR_BAD_PARAM
        for k in before:
            assert same(ctx.download(k), before[k]), k


# ---- 3. a general expression on a rectangle ----------------------------------------------------------------------------------
EXPR_TEXTS = [WEIGHTED, CWISE_MIN, "cwiseMax(traversability_slope - 0.1, 0.0)", "acos(surface_normal_z) + traversability_step"]


def test_expression_region_equals_the_whole_map_call(capi):
    from traversability_estimation_amd import synth
    elev = synth.with_steps(synth.perlin_elevation(ROWS, COLS, seed=3, amplitude=0.3), 6, seed=4).astype(np.float32)
    rng = np.random.default_rng(5)
    with context(capi, ROWS, COLS) as A, context(capi, ROWS, COLS) as B:
        for ctx in (A, B):
            ctx.upload_elevation(elev)
            ctx.run_chain(capi.RUN_KEEP_NORMALS)
        scores = {k: A.download(k).reshape(COLS, ROWS).copy() for k in SCORES}
        for text in EXPR_TEXTS:
            for rect in RECTS:
                r0, c0, h, wd = rect
                what = (text, rect)
                for ctx in (A, B):  # the same start: the chain's scores
                    for k in SCORES:
                        ctx.upload_layer(k, scores[k])
                A.run_expression(text)
                before = A.download("traversability").reshape(COLS, ROWS).copy()
                edit = {k: rng.uniform(0.0, 1.0, (wd, h)).astype(np.float32) for k in SCORES}
                edit["traversability_step"][rng.random((wd, h)) < 0.3] = np.nan
                for k in SCORES:
                    A.upload_layer_tile(k, edit[k], 0, r0, c0)
                    cur = scores[k].copy()
                    cur[c0:c0 + wd, r0:r0 + h] = edit[k]
                    B.upload_layer(k, cur)
                A.run_expression_region(text, 0, r0, c0, h, wd)
                B.run_expression(text)
                got, want = A.download("traversability").reshape(COLS, ROWS), B.download("traversability").reshape(COLS, ROWS)
                ins = inside_mask(rect)
                assert not differing(got, want)[ins].any(), what       # B's whole call on the rectangle
                assert not differing(got, before)[~ins].any(), what    # nothing else moved
                assert differing(got, before)[ins].any(), what         # (the edit shows)


def test_expression_region_refusals(capi):
    from traversability_estimation_amd import synth
    elev = synth.perlin_elevation(ROWS, COLS, seed=3, amplitude=0.3).astype(np.float32)
    with context(capi, ROWS, COLS) as ctx:
        ctx.upload_elevation(elev)
        ctx.run_chain()  # (normals dropped: surface_normal_z does not exist)
        ctx.run_expression(CWISE_MIN)
        before = {k: ctx.download(k).copy() for k in OUT_LAYERS}
        ok = (3, 4, 5, 6)
        for text, code, word in [("traversability_slope - meanOfFinites(traversability_slope)", capi.TE_ERR_UNSUPPORTED, "reduction"),
                                 ("0.5 * traversability + 0.5 * traversability_step", capi.TE_ERR_UNSUPPORTED, "reads the traversability layer"),
                                 ("acos(surface_normal_z)", capi.TE_ERR_NOT_READY, "surface_normal_z")]:
            for call in (lambda: ctx.run_expression_region(text, 0, *ok), lambda: ctx.run_chain_region_expression(text, 0, *ok)):
                with pytest.raises(capi.TeError) as e:
                    call()
                assert e.value.code == code and word in str(e.value), (text, str(e.value))
        for args, code in [((CWISE_MIN, 0, 66, 0, 8, 4), capi.TE_ERR_INVALID_ARG), ((CWISE_MIN, 1, *ok), capi.TE_ERR_INVALID_ARG), ((CWISE_MIN, 0, 0, 0, 0, 4), capi.TE_ERR_INVALID_ARG)]:
            with pytest.raises(capi.TeError) as e:
                ctx.run_expression_region(*args)
            assert e.value.code == code, args
        with pytest.raises(capi.TeError) as e:
            ctx.run_expression_region(CWISE_MIN, 0, *ok, out="traversability_slope")
        assert e.value.code == capi.TE_ERR_INVALID_ARG
        for k in before:
            assert same(ctx.download(k), before[k]), k


# ---- 4. the one-call tick ----------------------------------------------------------------------------------------------------
T_ROWS, T_COLS = 96, 80
BLOCK = (29, 22, 24, 30)  # (row0, col0, h, w)


def tie_free_over():
    from traversability_estimation_amd import synth
    r = synth.benchmark_radius(5, RES)
    return dict(normals_radius=r, rough_radius=r, step_radius1=r, step_radius2=r, fp_radius=r, fp_offset=0.0)


def tie_free(oracle):
    return oracle.default_params(**tie_free_over())


def is_min_of_scores(layers):
    """traversability is the expression, not the weighted sum: the minimum of the scores wherever all three are finite"""
    s = [np.asarray(layers[k], np.float32).reshape(-1) for k in SCORES]
    ok = np.isfinite(s[0]) & np.isfinite(s[1]) & np.isfinite(s[2])
    t = np.asarray(layers["traversability"], np.float32).reshape(-1)
    return ok.sum() > 1000 and np.array_equal(t[ok], np.minimum(np.minimum(s[0], s[1]), s[2])[ok])


def tick_terrain():
    from traversability_estimation_amd import synth
    elev = synth.with_steps(synth.perlin_elevation(T_ROWS, T_COLS, seed=11, amplitude=0.2), 5, seed=12).astype(np.float32).reshape(T_COLS, T_ROWS).copy()
    r0, c0, h, w = BLOCK
    tile = elev[c0:c0 + w, r0:r0 + h].copy()
    tile[8:20, 6:18] += np.float32(0.35)  # a raised block
    return elev, tile


def start(capi, op, elev, text):
    ctx = context(capi, T_ROWS, T_COLS, 1, to_te_params(capi, op))
    ctx.upload_elevation(elev)
    ctx.run_chain()
    if text is not None:
        ctx.run_expression(text)
    ctx.run_footprint()
    return ctx


def test_one_call_tick_equals_the_documented_workaround(capi, oracle):
    op = tie_free(oracle)
    elev, tile = tick_terrain()
    r0, c0, h, w = BLOCK
    with start(capi, op, elev, CWISE_MIN) as A, start(capi, op, elev, CWISE_MIN) as B:
        fp_before = A.download("traversability_footprint").copy()
        A.upload_tile(tile, 0, r0, c0)
        A.run_chain_region_expression(CWISE_MIN, 0, r0, c0, h, w, capi.RUN_FOOTPRINT | capi.RUN_FOOTPRINT_MEMO)
        B.upload_tile(tile, 0, r0, c0)
        B.run_chain_region(0, r0, c0, h, w)
        B.run_expression(CWISE_MIN)
        B.run_footprint()
        A.sync()
        B.sync()
        new_elev = elev.copy()
        new_elev[c0:c0 + w, r0:r0 + h] = tile
        layers = {}
        for name, ctx in (("one call", A), ("workaround", B)):
            assert same(ctx.download("elevation"), new_elev)
            layers[name] = {k: ctx.download(k) for k in OUT_LAYERS + ("traversability_footprint", "slope_footprint", "step_footprint", "roughness_footprint")}
        for k in OUT_LAYERS:
            assert same(layers["one call"][k], layers["workaround"][k]), k
        assert is_min_of_scores(layers["one call"])
        for name, got in layers.items():
            want, _, _ = oracle_fp(oracle, new_elev, T_ROWS, T_COLS, RES, trav=got["traversability"], **tie_free_over())
            check_fp(got, want, op, "tick footprint: " + name)
        assert differing(layers["one call"]["traversability_footprint"], fp_before).any()  # the guard: the edit reaches the footprint


def test_one_call_tick_without_a_text_is_the_region_chain(capi, oracle):
    op = tie_free(oracle)
    elev, tile = tick_terrain()
    r0, c0, h, w = BLOCK
    with start(capi, op, elev, None) as A, start(capi, op, elev, None) as B:
        for ctx, call in ((A, lambda: A.run_chain_region_expression(None, 0, r0, c0, h, w, capi.RUN_FOOTPRINT)), (B, lambda: B.run_chain_region(0, r0, c0, h, w, capi.RUN_FOOTPRINT))):
            ctx.upload_tile(tile, 0, r0, c0)
            call()
            ctx.sync()
        for k in OUT_LAYERS + ("traversability_footprint",):
            assert same(A.download(k), B.download(k)), k


def test_one_call_tick_is_refused_under_raster_normals(capi, oracle):
    elev, tile = tick_terrain()
    r0, c0, h, w = BLOCK
    with context(capi, T_ROWS, T_COLS, 1, to_te_params(capi, tie_free(oracle))) as ctx:
        ctx.set_option(capi.OPT_NORMALS_ALGORITHM, 1)
        ctx.upload_elevation(elev)
        ctx.run_chain()
        ctx.run_expression(CWISE_MIN)
        before = ctx.download("traversability").copy()
        with pytest.raises(capi.TeError) as e:
            ctx.run_chain_region_expression(CWISE_MIN, 0, r0, c0, h, w)
        assert e.value.code == capi.TE_ERR_UNSUPPORTED and "raster" in str(e.value)
        assert same(ctx.download("traversability"), before)


# ---- 5. a moved map ----------------------------------------------------------------------------------------------------------
def test_refresh_moved_with_an_expression_equals_a_fresh_context(capi, oracle):
    from traversability_estimation_amd import synth
    from tests.test_gpu_move import TICK_LAYERS
    op = tie_free(oracle)
    kr, kc = 3, -2
    world = synth.with_steps(synth.perlin_elevation(T_ROWS + 16, T_COLS + 16, seed=21, amplitude=0.3), 8, seed=22).astype(np.float32)  # (cols + 16, rows + 16)
    i0, j0 = 8, 8
    win = lambda a, b: np.ascontiguousarray(world[b:b + T_COLS, a:a + T_ROWS])
    pos = (12.3, -7.1)
    with context(capi, T_ROWS, T_COLS, 1, to_te_params(capi, op)) as A:
        A.set_geometry(T_ROWS, T_COLS, 1, RES, pos)
        A.upload_elevation(win(i0, j0))
        A.run_chain()
        A.run_expression(CWISE_MIN)
        A.run_footprint()
        info = A.move_map(pos[0] + kr * RES, pos[1] + kc * RES)
        assert (info.shift_rows, info.shift_cols) == (kr, kc) and info.results_kept == 1
        elev = win(i0 - kr, j0 - kc)  # old cell i is now i + kr
        tiles = [elev[c0:c0 + w, r0:r0 + h] if exposed else None for (r0, c0, h, w), exposed in info.rectangles()]
        A.refresh_moved(info, capi.RUN_FOOTPRINT, tiles, expression=CWISE_MIN)
        A.sync()
        assert same(A.download("elevation"), elev)
        got = {k: A.download(k) for k in TICK_LAYERS}
        new_pos = (info.pos_x, info.pos_y)
    with context(capi, T_ROWS, T_COLS, 1, to_te_params(capi, op)) as B:
        B.set_geometry(T_ROWS, T_COLS, 1, RES, new_pos)
        B.upload_elevation(elev)
        B.run_chain()
        B.run_expression(CWISE_MIN)
        B.run_footprint()
        B.sync()
        want = {k: B.download(k) for k in TICK_LAYERS}
    assert_layers_match(got, want, layers=TICK_LAYERS, ctx="moved map with an expression")
    assert is_min_of_scores(got)
