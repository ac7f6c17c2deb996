"""te_move_map on the device: the movement of every layer bit for bit against the numpy statement of the contract
(tests/ref_py/move_ref.py), and the robot-centric tick -- move, upload the exposed strips, re-filter the rectangles -- against
the CPU oracle on the new window at the NEW position."""
import numpy as np
import pytest

from tests.helpers import OUT_LAYERS, TOL, assert_layers_match, compare_layer, to_te_params
from tests.ref_py import move_ref

pytestmark = pytest.mark.gpu

RES = 0.05
TICK_LAYERS = OUT_LAYERS + ("traversability_footprint",)


@pytest.fixture(scope="module")
def capi():
    from traversability_estimation_amd import capi
    capi.load()
    assert capi.device_count() >= 1, "no MI355X visible"
    return capi


def bits(a):
    return np.ascontiguousarray(a, np.float32).reshape(-1).view(np.uint32)


def same_with_nan(got, want):
    got, want = np.asarray(got, np.float32).reshape(-1), np.asarray(want, np.float32).reshape(-1)
    gn, wn = np.isnan(got), np.isnan(want)
    return np.array_equal(gn, wn) and np.array_equal(bits(got[~gn]), bits(want[~wn]))


# ---- 1. movement, bit for bit --------------------------------------------------------------------------------------------
def shifts_of(rows, cols):
    return [(0, 0), (1, 0), (0, -1), (3, -2), (-5, 7), (2, 1), (4, 0), (-3, 0), (rows - 1, 0), (rows, 0), (0, -cols - 3)]


@pytest.mark.parametrize("rows,cols,batch", [(70, 45, 1), (200, 130, 1), (129, 257, 3)])
def test_every_layer_and_the_fill_mask_move_bit_for_bit(capi, rows, cols, batch):
    pos = (12.3, -7.1)
    n = rows * cols
    assert n < 65536 and batch <= 8  # layer * 65536 + cell + map * 2^20: exact in float32, distinct per layer and map
    cell = (np.arange(n, dtype=np.float32).reshape(1, cols, rows) + (np.arange(batch, dtype=np.float32) * float(1 << 20)).reshape(batch, 1, 1))
    with capi.Context(0) as ctx:
        ctx.set_params(capi.default_params())
        ctx.set_geometry(rows, cols, batch, RES, pos)
        names = [k for k in capi.LAYERS if k not in ("traversability_x", "traversability_rot")]  # (those exist after a polygon pass only)
        held = {}
        for k in names:
            held[k] = (capi.LAYERS[k] * 65536 + cell).astype(np.float32)
            ctx.upload_layer(k, held[k])
        # a fill mask: holes in a holding layer, filled into another (both are re-uploaded below)
        holes = held["slope_footprint"].copy()
        holes[:, 5:27, 8:41] = np.nan  # (wider than the fill radius: its inside stays 0 in the mask)
        ctx.upload_layer("slope_footprint", holes)
        ctx.run_median_fill(capi.default_median_fill_params(fill_hole_radius=2 * RES, num_erode_dilation_iterations=0), "slope_footprint", "step_footprint")
        mask = np.stack([ctx.download_fill_mask(b) for b in range(batch)])
        assert mask.any() and not mask.all()
        for k in ("slope_footprint", "step_footprint"):
            ctx.upload_layer(k, held[k])
        for shift in shifts_of(rows, cols):
            new = (pos[0] + shift[0] * RES, pos[1] + shift[1] * RES)
            plan = capi.move_geometry(rows, cols, RES, pos, new, capi.default_params())
            info = ctx.move_map(*new)
            ctx.sync()
            assert (info.shift_rows, info.shift_cols) == shift == (plan.shift_rows, plan.shift_cols)
            assert info.rectangles() == plan.rectangles() == move_ref.rectangles(rows, cols, shift)
            assert (info.pos_x, info.pos_y) == (plan.pos_x, plan.pos_y) == move_ref.shift_and_position(RES, pos, new)[1]
            assert info.results_kept == (1 if shift == (0, 0) else 0)  # (the shipped radii: a one-cell tie)
            for k in names:
                held[k] = move_ref.moved(held[k], shift)
                assert same_with_nan(ctx.download(k), held[k]), (k, shift)
            mask = move_ref.moved(mask, shift, fill=0)
            for b in range(batch):
                assert np.array_equal(ctx.download_fill_mask(b), mask[b]), (shift, b)
            pos = (info.pos_x, info.pos_y)
            parsed = capi.msg_parse(ctx.download_msg(capi.TeMsgInfo(), {"elevation": "elevation"}))[0]
            assert (parsed.pose[0], parsed.pose[1]) == pos, shift
            if np.isnan(held["elevation"]).all():  # everything has left the window: fill the layers again for the shifts that follow
                for k in names:
                    held[k] = (capi.LAYERS[k] * 65536 + cell).astype(np.float32)
                    ctx.upload_layer(k, held[k])


# ---- 2. the tick against the oracle --------------------------------------------------------------------------------------
W_ROWS, W_COLS, ROWS, COLS = 300, 240, 256, 192
I0, J0 = 24, 20  # the window's first row / column in the world before any move


def world(seed=7, speckle=0.0):
    from traversability_estimation_amd import synth
    w = synth.with_steps(synth.perlin_elevation(W_ROWS, W_COLS, seed=seed, amplitude=0.4), 40, seed=seed + 1)
    return synth.with_holes(w, speckle, seed=seed + 2) if speckle else w


def window(w, i0, j0):
    return np.ascontiguousarray(w[j0:j0 + COLS, i0:i0 + ROWS])


def tie_free(oracle, fp_cells=5):
    from traversability_estimation_amd import synth
    r = synth.benchmark_radius(5, RES)
    return oracle.default_params(normals_radius=r, rough_radius=r, step_radius1=r, step_radius2=r, fp_radius=synth.benchmark_radius(fp_cells, RES), fp_offset=0.0)


def oracle_tick(oracle, op, elev, pos):
    g = oracle.geom(ROWS, COLS, RES, pos)
    want = oracle.chain(g, op, elev)
    want["traversability_footprint"] = oracle.footprint(g, op, elev, want)
    return want


def tiles_of(info, elev):
    return [elev[c0:c0 + w, r0:r0 + h] if exposed else None for (r0, c0, h, w), exposed in info.rectangles()]


def tick(capi, oracle, op, w, moves, only_exposed=False, region_footprint=False):
    """run_chain on the first window, then each move with its refresh; returns (the layers, the oracle's, the last info).
    region_footprint: every rectangle with TE_RUN_FOOTPRINT on its region run and no whole-map footprint pass."""
    pos, i0, j0 = (12.3, -7.1), I0, J0
    with capi.Context(0) as ctx:
        ctx.set_params(to_te_params(capi, op))
        ctx.set_geometry(ROWS, COLS, 1, RES, pos)
        ctx.upload_elevation(window(w, i0, j0))
        ctx.run_chain(capi.RUN_FOOTPRINT)
        for kr, kc in moves:
            info = ctx.move_map(pos[0] + kr * RES, pos[1] + kc * RES)
            assert (info.shift_rows, info.shift_cols) == (kr, kc) and info.results_kept == 1
            pos, i0, j0 = (info.pos_x, info.pos_y), i0 - kr, j0 - kc  # old cell i is now i + kr: the window starts kr cells earlier
            elev = window(w, i0, j0)
            tiles = tiles_of(info, elev)
            if region_footprint:
                for ((r0, c0, h, wd), exposed), t in zip(info.rectangles(), tiles):
                    if exposed:
                        ctx.upload_tile(t, 0, r0, c0)
                    ctx.run_chain_region(0, r0, c0, h, wd, capi.RUN_FOOTPRINT)
            elif only_exposed:
                for ((r0, c0, h, wd), exposed), t in zip(info.rectangles(), tiles):
                    if exposed:
                        ctx.upload_tile(t, 0, r0, c0)
                        ctx.run_chain_region(0, r0, c0, h, wd)
                ctx.run_footprint()  # (whole-map, as refresh_moved ends: the mask is decided at the new position)
            else:
                ctx.refresh_moved(info, capi.RUN_FOOTPRINT, tiles)
        ctx.sync()
        assert same_with_nan(ctx.download("elevation"), elev)
        got = {k: ctx.download(k) for k in TICK_LAYERS}
    return got, oracle_tick(oracle, op, elev, pos), info


@pytest.mark.parametrize("name,speckle,fp_cells,moves", [("two axes", 0.0, 5, [(7, -3)]), ("speckle", 0.01, 5, [(7, -3)]), ("any reach", 0.0, 23, [(7, -3)]),
                                                         ("single axis", 0.0, 5, [(0, 4)]), ("two moves", 0.0, 5, [(7, -3), (-2, 5)])])
def test_the_tick_matches_the_oracle_at_the_new_position(capi, oracle, name, speckle, fp_cells, moves):
    """The oracle alone is the yardstick, at helpers.TOL with exact NaN patterns, on the four chain layers and the footprint layer.
    refresh_moved serves the footprint by one whole-map te_run_footprint behind the region chains.  With the footprint flag on
    the region runs instead, the four chain layers matched and traversability_footprint missed the oracle on 10 / 12 / 2 / 1 / 0
    cells of the five cases (differences up to 0.89) -- exactly the cells on which the ORACLE's own footprint layers of the two
    positions differ on the same terrain (10 / - / - / 1 / 0, interior cells, measured on the CPU alone): circle(3 res) and
    circle(2.5 res) of the footprint checks have cells on their circle at every resolution (include/travgpu.h, caveat 3)."""
    got, want, _ = tick(capi, oracle, tie_free(oracle, fp_cells), world(speckle=speckle), moves)
    assert_layers_match(got, want, layers=TICK_LAYERS, ctx="tick: " + name)


@pytest.mark.parametrize("fp_cells", [5, 23])
def test_region_footprint_runs_after_a_move_miss_the_oracle_only_where_its_own_positions_differ(capi, oracle, fp_cells):
    """The region form of the footprint pass behind a move -- at 23 cells the region form of the route of any reach, which the
    tick above never runs because refresh_moved serves the footprint by the whole-map pass.  The bound is the reference's own:
    a cell may miss the oracle of the new position only if the oracle of the OLD position, carried to the cell, differs from it
    too (the tie cells of caveat 3 in the interior).  The four chain layers match everywhere."""
    op, w, (kr, kc) = tie_free(oracle, fp_cells), world(), (7, -3)
    got, want, _ = tick(capi, oracle, op, w, [(kr, kc)], region_footprint=True)
    assert_layers_match(got, want, layers=OUT_LAYERS, ctx="region footprint runs: chain layers")
    old = oracle_tick(oracle, op, window(w, I0, J0), (12.3, -7.1))["traversability_footprint"]
    carried = move_ref.moved(old.reshape(COLS, ROWS), (kr, kc))
    x = want["traversability_footprint"].reshape(COLS, ROWS)
    g = got["traversability_footprint"].reshape(COLS, ROWS)
    own = ~((np.abs(carried - x) <= TOL) | (np.isnan(carried) & np.isnan(x)))
    miss = ~((np.abs(g - x) <= TOL) | (np.isnan(g) & np.isnan(x)))
    assert not (miss & ~own).any(), int((miss & ~own).sum())
    inner = np.zeros_like(own)
    inner[40:-40, 40:-40] = True
    assert (miss & inner).sum() <= (own & inner).sum() <= 64  # (a few cells: not a licence for the layer)


# ---- 3. trailing edges matter --------------------------------------------------------------------------------------------
def test_without_the_trailing_lines_cells_near_the_trailing_borders_are_stale(capi, oracle):
    op, w, (kr, kc) = tie_free(oracle), world(), (7, -3)
    reach = 24  # both step windows (10), the mask (3), the footprint (5) and the gap walk behind them, with slack
    near = np.zeros((COLS, ROWS), bool)  # within reach of a trailing border: the last rows (kr > 0), the first columns (kc < 0)
    near[:, ROWS - reach:] = True
    near[:reach, :] = True
    # the oracle's own two windows: a result of the old window, carried to its new cell, differs from the new window's
    old = oracle_tick(oracle, op, window(w, I0, J0), (12.3, -7.1))
    new = oracle_tick(oracle, op, window(w, I0 - kr, J0 - kc), (12.3 + kr * RES, -7.1 + kc * RES))
    carried = {k: move_ref.moved(old[k].reshape(COLS, ROWS), (kr, kc)) for k in TICK_LAYERS}
    stale = sum(int((np.abs(carried[k] - new[k].reshape(COLS, ROWS))[near] > TOL).sum()) for k in TICK_LAYERS)
    assert stale > 0, "the world does not show the effect: choose another"
    got, want, info = tick(capi, oracle, op, w, [(kr, kc)], only_exposed=True)
    assert [e for _, e in info.rectangles()] == [True, True, False, False]
    bad = sum(int((np.abs(got[k].reshape(COLS, ROWS) - want[k].reshape(COLS, ROWS))[near] > TOL).sum()) for k in TICK_LAYERS)
    assert bad > 0
    # ... and nowhere else, and nowhere at all with the full refresh
    for k in TICK_LAYERS:
        g, x = got[k].reshape(COLS, ROWS), want[k].reshape(COLS, ROWS)
        assert compare_layer(k, g[~near], x[~near])[0] == 0, k
    full, want, _ = tick(capi, oracle, op, w, [(kr, kc)])
    assert_layers_match(full, want, layers=TICK_LAYERS, ctx="full refresh")


# ---- 4. tie radii --------------------------------------------------------------------------------------------------------
def test_at_a_tie_radius_the_move_keeps_the_inputs_and_drops_the_results(capi, oracle):
    op, w, pos = oracle.default_params(), world(), (12.3, -7.1)
    with capi.Context(0) as ctx:
        ctx.set_params(to_te_params(capi, op))
        ctx.set_geometry(ROWS, COLS, 1, RES, pos)
        ctx.upload_elevation(window(w, I0, J0))
        ctx.run_chain(capi.RUN_FOOTPRINT)
        info = ctx.move_map(pos[0] + 7 * RES, pos[1] - 3 * RES)
        assert info.results_kept == 0 and (info.shift_rows, info.shift_cols) == (7, -3)
        with pytest.raises(capi.TeError) as e:
            ctx.run_chain_region(0, *info.rectangles()[0][0])
        assert e.value.code == capi.TE_ERR_NOT_READY
        elev = window(w, I0 - 7, J0 + 3)
        ctx.refresh_moved(info, capi.RUN_FOOTPRINT, tiles_of(info, elev))
        ctx.sync()
        assert same_with_nan(ctx.download("elevation"), elev)
        got = {k: ctx.download(k) for k in TICK_LAYERS}
    assert_layers_match(got, oracle_tick(oracle, op, elev, (info.pos_x, info.pos_y)), layers=TICK_LAYERS, ctx="tie radii: whole run after the move")


# ---- 5. geometry follows -------------------------------------------------------------------------------------------------
def test_submaps_and_path_checks_in_world_coordinates_survive_the_move(capi, oracle):
    op, w, pos = tie_free(oracle), world(), (12.3, -7.1)
    centre, length = (12.1, -7.0), (4.0, 3.0)  # a world rectangle inside both windows
    paths = [[(11.0, -8.5), (13.0, -6.0)], [(12.3, -7.1), (12.3, -5.2), (10.5, -5.2)], [(14.0, -9.0), (14.5, -8.0)]]
    radii = [0.2, 0.33, 0.27]
    with capi.Context(0) as ctx:
        ctx.set_params(to_te_params(capi, op))
        ctx.set_geometry(ROWS, COLS, 1, RES, pos)
        ctx.upload_elevation(window(w, I0, J0))
        ctx.run_chain(capi.RUN_FOOTPRINT)
        # (the four chain layers and the elevation: tie-free, they do not depend on the position; the footprint layer is
        # decided anew at the new position wherever its fixed windows have a cell on their circle)
        before_info, before = ctx.download_submap(centre, length, list(OUT_LAYERS) + ["elevation"])
        before_paths = ctx.check_footprint_paths_radius(paths, radii, offset=0.1)
        info = ctx.move_map(pos[0] + 7 * RES, pos[1] - 3 * RES)
        ctx.refresh_moved(info, capi.RUN_FOOTPRINT, tiles_of(info, window(w, I0 - 7, J0 + 3)))
        after_info, after = ctx.download_submap(centre, length, list(OUT_LAYERS) + ["elevation"])
        after_paths = ctx.check_footprint_paths_radius(paths, radii, offset=0.1)
    assert before_info.ok and after_info.ok
    assert (after_info.row0, after_info.col0) == (before_info.row0 + 7, before_info.col0 - 3)
    assert (after_info.rows, after_info.cols) == (before_info.rows, before_info.cols)
    for k in before:
        assert same_with_nan(after[k], before[k]), k
    for a, b in zip(after_paths, before_paths):
        assert np.array_equal(np.asarray(a), np.asarray(b))


# ---- 6. pre-filters on the tick ------------------------------------------------------------------------------------------
def test_prefilters_on_the_tick_equal_a_fresh_context(capi, oracle):
    HOLD, MID = "slope_footprint", "step_footprint"
    op, w, pos = tie_free(oracle), world(speckle=0.03), (12.3, -7.1)
    p = capi.default_median_fill_params(fill_hole_radius=2 * RES, num_erode_dilation_iterations=1)

    def prefilter(ctx, raw):
        ctx.upload_layer(HOLD, raw)
        ctx.run_median_fill(p, HOLD, MID)
        ctx.run_radius_filter("mean", 1.5 * RES, MID, "elevation")

    with capi.Context(0) as A, capi.Context(0) as B:
        for ctx in (A, B):
            ctx.set_params(to_te_params(capi, op))
        A.set_geometry(ROWS, COLS, 1, RES, pos)
        prefilter(A, window(w, I0, J0))
        A.run_chain()
        info = A.move_map(pos[0] + 7 * RES, pos[1] - 3 * RES)
        assert info.results_kept == 1
        raw = window(w, I0 - 7, J0 + 3)
        for (r0, c0, h, wd), exposed in info.rectangles():
            if exposed:
                A.upload_layer_tile(HOLD, raw[c0:c0 + wd, r0:r0 + h], 0, r0, c0)
            filled = A.run_median_fill_region(p, HOLD, MID, 0, r0, c0, h, wd)
            smoothed = A.run_radius_filter_region("mean", 1.5 * RES, MID, "elevation", 0, *filled)
            A.run_chain_region(0, *smoothed)
        # (no footprint pass here: te_run_footprint writes the three memo layers, two of which hold the raw and the filled map
        # in this test; the footprint layer behind a move is the subject of the tick tests above)
        A.sync()
        B.set_geometry(ROWS, COLS, 1, RES, (info.pos_x, info.pos_y))
        prefilter(B, raw)
        B.run_chain()
        B.sync()
        for k in (HOLD, MID, "elevation"):
            assert same_with_nan(A.download(k), B.download(k)), k
        assert np.array_equal(A.download_fill_mask(0), B.download_fill_mask(0))
        assert_layers_match({k: A.download(k) for k in OUT_LAYERS}, {k: B.download(k) for k in OUT_LAYERS}, layers=OUT_LAYERS, ctx="pre-filtered tick")


# ---- the polygon layers, and a move before any elevation ------------------------------------------------------------------
def test_the_polygon_layers_move_too(capi):
    from traversability_estimation_amd import synth
    rows, cols, pos = 70, 45, (1.0, 2.0)
    with capi.Context(0) as ctx:
        ctx.set_params(capi.default_params())
        ctx.set_geometry(rows, cols, 1, RES, pos)
        ctx.upload_elevation(synth.with_steps(synth.perlin_elevation(rows, cols, seed=3, amplitude=0.2), 4, seed=4))
        ctx.run_chain(capi.RUN_FOOTPRINT)
        ctx.run_polygon_footprint([(0.2, 0.1), (0.2, -0.1), (-0.2, -0.1), (-0.2, 0.1)], 0.4)
        ctx.sync()
        names = ("traversability_x", "traversability_rot", "traversability")
        before = {k: ctx.download(k).reshape(cols, rows).copy() for k in names}
        assert np.isfinite(before["traversability_x"]).any() and not np.array_equal(bits(before["traversability_x"]), bits(before["traversability_rot"]))
        info = ctx.move_map(pos[0] + 3 * RES, pos[1] - 2 * RES)
        ctx.sync()
        assert (info.shift_rows, info.shift_cols) == (3, -2)
        for k in names:
            assert same_with_nan(ctx.download(k), move_ref.moved(before[k], (3, -2))), k


def test_a_move_before_any_elevation_makes_none_up(capi):
    with capi.Context(0) as ctx:
        ctx.set_params(capi.default_params())  # (a tie radius: results_kept = 0, the transition of a whole upload)
        ctx.set_geometry(70, 45, 1, RES, (1.0, 2.0))
        info = ctx.move_map(1.0 + 3 * RES, 2.0)
        assert info.n_rects == 2 and info.results_kept == 0
        with pytest.raises(capi.TeError) as e:
            ctx.run_chain()
        assert e.value.code == capi.TE_ERR_NOT_READY  # no elevation uploaded, before the move and after it
        ctx.upload_elevation(np.zeros((45, 70), np.float32))
        ctx.run_chain()
        ctx.sync()


# ---- 7. errors -----------------------------------------------------------------------------------------------------------
def test_refusals_and_the_zero_shift(capi):
    from traversability_estimation_amd import synth
    rows, cols = 70, 45
    with capi.Context(0) as ctx:
        with pytest.raises(capi.TeError) as e:
            ctx.move_map(1.0, 1.0)
        assert e.value.code == capi.TE_ERR_NOT_READY
        ctx.set_params(capi.default_params())
        ctx.set_geometry(rows, cols, 1, RES, (1.0, 2.0))
        elev = synth.perlin_elevation(rows, cols, seed=3)
        ctx.upload_elevation(elev)
        ctx.run_chain(capi.RUN_FOOTPRINT)
        ctx.sync()
        before = {k: bits(ctx.download(k)).copy() for k in ("elevation",) + TICK_LAYERS}
        for bad in ((float("nan"), 1.0), (1.0, float("inf"))):
            with pytest.raises(capi.TeError) as e:
                ctx.move_map(*bad)
            assert e.value.code == capi.TE_ERR_BAD_PARAM
        info = ctx.move_map(1.0 + 0.4 * RES, 2.0 - 0.4 * RES)
        assert info.n_rects == 0 and (info.shift_rows, info.shift_cols) == (0, 0) and (info.pos_x, info.pos_y) == (1.0, 2.0)
        ctx.refresh_moved(info, capi.RUN_FOOTPRINT)
        ctx.sync()
        for k, v in before.items():
            assert np.array_equal(bits(ctx.download(k)), v), k
        ctx.run_chain_region(0, 0, 0, 8, 8, capi.RUN_FOOTPRINT)  # (the results stand: a region run is still accepted)
        ctx.sync()
