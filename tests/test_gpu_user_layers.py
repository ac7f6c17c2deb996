"""User layers on the device: every call that takes "any float layer" takes a user id, with the bits the same call gives
through a borrowed reference layer; te_move_map shifts them; a removed layer's id comes back without contents; and writing one
leaves the chain's cached results alone."""
import numpy as np
import pytest

from tests.ref_py import move_ref
from tests.user_layer_cases import RES, SHAPES, context, grid, holed, same

pytestmark = pytest.mark.gpu
MEAN = "meanOfFinites(%s)"


@pytest.fixture(scope="module")
def capi():
    from traversability_estimation_amd import build, capi
    build.build_lib()
    return capi


@pytest.mark.parametrize("rows, cols, batch", SHAPES)
def test_transfers_round_trip(capi, rows, cols, batch):
    a = holed(rows, cols, batch, 1)
    with context(capi, rows, cols, batch) as ctx:
        lid = ctx.add_layer("elevation_raw")
        assert lid == capi.LAYER_COUNT and ctx.layer_id("elevation_raw") == lid and ctx.layer_name(lid) == "elevation_raw"
        assert ctx.add_layer("elevation_raw") == lid and ctx.layer_id("traversability") == 4
        with pytest.raises(capi.TeError) as e:  # absent until written
            ctx.download("elevation_raw")
        assert e.value.code == capi.TE_ERR_NOT_READY
        with pytest.raises(capi.TeError) as e:  # never added: as an id out of range
            ctx.download(lid + 1)
        assert e.value.code == capi.TE_ERR_INVALID_ARG
        ctx.upload_layer("elevation_raw", a)
        assert same(ctx.download("elevation_raw"), a)
        assert same(ctx.download(lid, 0, 1), a[0])
        t = np.full((5, 7), 2.5, np.float32)  # (w, h)
        ctx.upload_layer_tile(lid, t, batch - 1, 3, 4)
        want = a.copy()
        want[batch - 1, 4:9, 3:10] = t
        assert same(ctx.download("elevation_raw"), want)
        assert same(ctx.download_tile("elevation_raw", batch - 1, 2, 3, 9, 7), want[batch - 1, 3:10, 2:11])
        # circular order, through a second layer that gets its memory from this write
        lid2 = ctx.add_layer("second")
        ctx.upload_layer_circular(lid2, a[0], (5, 3))
        assert same(ctx.download_layer_circular(lid2, (5, 3)), a[0])
        # the device pointer is the layer's memory
        ptr, nbytes = ctx.device_ptr("elevation_raw")
        assert ptr and nbytes == a.size * 4


@pytest.mark.parametrize("rows, cols, batch", SHAPES)
def test_filters_equal_the_same_call_through_a_reference_layer(capi, rows, cols, batch):
    a = holed(rows, cols, batch, 2)
    wp = capi.window_expr_params(window_size=3)
    mp = capi.default_median_fill_params()
    with context(capi, rows, cols, batch) as U, context(capi, rows, cols, batch) as B:
        U.add_layer("hold"), U.add_layer("mid")
        U.upload_layer("hold", a)
        B.upload_layer("robot_slope", a)
        # user -> user, user -> reference, in place on a user layer
        U.run_median_fill(mp, "hold", "mid")
        B.run_median_fill(mp, "robot_slope", "traversability_roughness")
        assert same(U.download("mid"), B.download("traversability_roughness"))
        U.run_radius_filter(capi.RADIUS_MEAN, 0.11, "mid", "traversability_step")
        B.run_radius_filter(capi.RADIUS_MEAN, 0.11, "traversability_roughness", "traversability_step")
        assert same(U.download("traversability_step"), B.download("traversability_step"))
        U.run_radius_filter(capi.RADIUS_MIN, 0.11, "hold", "hold")
        B.run_radius_filter(capi.RADIUS_MIN, 0.11, "robot_slope", "robot_slope")
        assert same(U.download("hold"), B.download("robot_slope"))
        U.run_window_expression(MEAN % "hold", wp, "hold", "mid")
        B.run_window_expression(MEAN % "robot_slope", wp, "robot_slope", "traversability_roughness")
        assert same(U.download("mid"), B.download("traversability_roughness"))
        # the region forms: a changed rectangle of the input, the output refreshed around it
        t = np.full((4, 6), 1.25, np.float32)
        U.upload_layer_tile("hold", t, 0, 8, 5), B.upload_layer_tile("robot_slope", t, 0, 8, 5)
        assert U.run_window_expression_region(MEAN % "hold", wp, "hold", "mid", 0, 8, 5, 6, 4) == \
            B.run_window_expression_region(MEAN % "robot_slope", wp, "robot_slope", "traversability_roughness", 0, 8, 5, 6, 4)
        assert same(U.download("mid"), B.download("traversability_roughness"))
        U.run_radius_filter_region(capi.RADIUS_MEAN, 0.11, "hold", "traversability_step", 0, 8, 5, 6, 4)
        B.run_radius_filter_region(capi.RADIUS_MEAN, 0.11, "robot_slope", "traversability_step", 0, 8, 5, 6, 4)
        assert same(U.download("traversability_step"), B.download("traversability_step"))


@pytest.mark.parametrize("rows, cols, batch", SHAPES)
def test_outputs_equal_the_same_call_through_a_reference_layer(capi, rows, cols, batch):
    a = holed(rows, cols, batch, 3, 0.0, 1.0)
    with context(capi, rows, cols, batch) as ctx:
        ctx.add_layer("score")
        ctx.upload_layer("score", a)
        ctx.upload_layer("traversability", a)
        assert np.array_equal(ctx.download_occupancy(["score"]), ctx.download_occupancy(["traversability"]))
        ctx.upload_elevation(a)
        assert np.array_equal(ctx.download_cloud(["elevation", "score"], "elevation"), ctx.download_cloud(["elevation", "traversability"], "elevation"))
        pos, length = (0.3 * RES, -0.2 * RES), (10 * RES, 8 * RES)
        (iu, su), (ib, sb) = ctx.download_submap(pos, length, ["score"]), ctx.download_submap(pos, length, ["traversability"])
        assert iu.ok == 1 and (iu.rows, iu.cols) == (ib.rows, ib.cols) and same(su["score"], sb["traversability"])
        if batch == 1:
            info = capi.TeMsgInfo()
            mu, mb = ctx.download_msg(info, {"x": "score"}), ctx.download_msg(info, {"x": "traversability"})
            assert mu == mb
            with context(capi, rows, cols, 1) as other:
                other.add_layer("from_msg")
                other.upload_msg(mu, "x", "from_msg")
                assert same(other.download("from_msg"), a)


@pytest.mark.parametrize("rows, cols, batch", SHAPES)
def test_move_map_shifts_a_user_layer(capi, rows, cols, batch):
    a, b = holed(rows, cols, batch, 4), holed(rows, cols, batch, 5)
    pos = (12.3, -7.1)
    with context(capi, rows, cols, batch, pos) as ctx:
        ctx.add_layer("kept"), ctx.add_layer("never_written")
        ctx.upload_layer("kept", a)
        ctx.upload_layer("traversability_slope", b)
        info = ctx.move_map(pos[0] + 3 * RES, pos[1] - 2 * RES)
        assert (info.shift_rows, info.shift_cols) == (3, -2)
        assert same(ctx.download("kept"), move_ref.moved(a, (3, -2)))
        assert same(ctx.download("traversability_slope"), move_ref.moved(b, (3, -2)))
        with pytest.raises(capi.TeError) as e:
            ctx.download("never_written")
        assert e.value.code == capi.TE_ERR_NOT_READY


def test_remove_then_add_returns_fresh_memory(capi):
    rows, cols, batch = SHAPES[0]
    a = holed(rows, cols, batch, 6)
    with context(capi, rows, cols, batch) as ctx:
        ids = [ctx.add_layer("l%d" % k) for k in range(capi.MAX_USER_LAYERS)]
        assert ids == list(range(capi.LAYER_COUNT, capi.LAYER_COUNT + 16))
        with pytest.raises(capi.TeError) as e:
            ctx.add_layer("one_too_many")
        assert e.value.code == capi.TE_ERR_UNSUPPORTED
        with pytest.raises(capi.TeError) as e:
            ctx.add_layer("sqrt")
        assert e.value.code == capi.TE_ERR_BAD_PARAM
        ctx.upload_layer("l3", a)
        ctx.remove_layer("l3")
        with pytest.raises(capi.TeError) as e:
            ctx.download(ids[3])  # never added again: a bad id
        assert e.value.code == capi.TE_ERR_INVALID_ARG
        with pytest.raises(capi.TeError) as e:
            ctx.remove_layer("elevation")
        assert e.value.code == capi.TE_ERR_INVALID_ARG
        assert ctx.add_layer("again") == ids[3]  # lowest free id first
        with pytest.raises(capi.TeError) as e:
            ctx.download("again")
        assert e.value.code == capi.TE_ERR_NOT_READY
        t = np.zeros((1, 1), np.float32)
        ctx.upload_layer_tile("again", t, 0, 2, 2)  # the first write: every other cell is NaN, not the removed layer's values
        got = grid(ctx, "again")
        assert got[0, 2, 2] == 0.0 and np.isnan(got).sum() == got.size - 1
        # another shape drops the contents and keeps the names
        ctx.upload_layer("l5", a)
        ctx.set_geometry(rows + 1, cols, batch, RES)
        assert ctx.layer_id("l5") == ids[5]
        with pytest.raises(capi.TeError) as e:
            ctx.download("l5")
        assert e.value.code == capi.TE_ERR_NOT_READY


def test_writes_to_user_layers_keep_the_chain_results(capi):
    rows, cols, batch = SHAPES[1]
    rng = np.random.default_rng(7)
    elev = rng.uniform(0.0, 0.3, (batch, cols, rows)).astype(np.float32)
    with context(capi, rows, cols, batch) as ctx:
        ctx.upload_elevation(elev)
        ctx.run_chain(capi.RUN_FOOTPRINT)
        before = {k: ctx.download(k) for k in ("traversability", "traversability_footprint")}
        ctx.add_layer("mine")
        ctx.upload_layer("mine", elev)
        ctx.run_radius_filter(capi.RADIUS_MEAN, 0.11, "mine", "mine")
        ctx.run_threshold("mine", "lower", 0.1, 0.0)
        ctx.copy_layer("mine", ctx.add_layer("mine2"))
        # the region contract still holds: chain_done and footprint_done were not dropped
        ctx.run_chain_region(0, 10, 10, 8, 8, capi.RUN_FOOTPRINT)
        for k, v in before.items():
            assert same(ctx.download(k), v), k


def test_prefetch_into_a_user_layer_and_remove_joins_it(capi):
    rows, cols, batch = SHAPES[1]
    a, b = holed(rows, cols, batch, 8), holed(rows, cols, batch, 9)
    with context(capi, rows, cols, batch) as ctx:
        first = ctx.add_layer("ahead")
        ctx.prefetch_layers({"ahead": a, "traversability_slope": b})
        assert same(ctx.download("ahead"), a)  # (the download joins the prefetch that writes the layer)
        ctx.wait_prefetch()
        assert same(ctx.download("traversability_slope"), b)
        # a remove beside a prefetch in flight on the layer joins it first; the id comes back without contents
        ctx.prefetch_layers({"ahead": b})
        ctx.remove_layer("ahead")
        ctx.wait_prefetch()
        assert ctx.add_layer("next") == first
        with pytest.raises(capi.TeError) as e:
            ctx.download("next")
        assert e.value.code == capi.TE_ERR_NOT_READY


def test_a_refused_first_write_leaves_the_layer_absent(capi):
    rows, cols, batch = SHAPES[0]
    a = holed(rows, cols, batch, 10)
    with context(capi, rows, cols, batch) as ctx:
        ctx.add_layer("fresh")
        for write in (lambda: ctx.upload_layer("fresh", a[0], batch),                      # a map behind the batch
                      lambda: ctx.upload_layer_circular("fresh", a[0], (rows, 0)),         # a start index outside the map
                      lambda: ctx.upload_layer_circular("fresh", a[0], (0, 0), batch)):
            with pytest.raises(capi.TeError) as e:
                write()
            assert e.value.code == capi.TE_ERR_INVALID_ARG
            for read in (lambda: ctx.download("fresh"), lambda: ctx.run_radius_filter(capi.RADIUS_MEAN, 0.11, "fresh", "traversability_step"),
                         lambda: ctx.run_layer_expression("fresh + 1", "traversability_step"), lambda: ctx.run_threshold("fresh", "lower", 0.0, 0.0)):
                with pytest.raises(capi.TeError) as e:
                    read()
                assert e.value.code == capi.TE_ERR_NOT_READY
        ctx.upload_layer("fresh", a)
        assert same(ctx.download("fresh"), a)
