"""The flat-tile path of the footprint pass's mask kernel (k_fp_mask): tiles whose face flags -- built from the elevation by
the upload's pass, te_face_flags.h -- are clear skip the step-check staging.  The yardstick is the same library with
TE_OPT_FACE_FLAGS = 0 (every tile stages): every layer a footprint run leaves must be bit-identical between the two settings,
and on maps of at most 320 x 320 both agree with the oracle.  (The mask bytes and their flag bytes cannot be downloaded; the
footprint layer and the three memo layers are functions of them.)  The face flags the device built are downloaded after every
upload made with the flags on and must equal the definition (flags_numpy): a missing flag and an extra one both fail."""
import numpy as np
import pytest

from tests.helpers import OUT_LAYERS, compare_layer, to_te_params
from tests.test_face_flags import flags_numpy, terrain

pytestmark = pytest.mark.gpu

LAYERS = list(OUT_LAYERS) + ["traversability_footprint", "slope_footprint", "step_footprint", "roughness_footprint"]


@pytest.fixture(scope="module")
def capi():
    from traversability_estimation_amd import capi
    capi.load()
    assert capi.device_count() >= 1
    return capi


# step windows of 3 cells at 0.05 m (the reference's 0.04 m windows hold one cell there and never give a step score of 0)
STEP = dict(step_radius1=0.15, step_radius2=0.15)


def smooth(rows, cols, seed):
    """(cols, rows) terrain whose adjacent cells differ by millimetres: no tile holds a face at fp_critical_step = 0.12."""
    from traversability_estimation_amd import synth
    return synth.perlin_elevation(rows, cols, seed=seed, amplitude=0.3).astype(np.float32)


def box(e, i0, j0, h=20, w=12, height=0.3):
    e[j0:j0 + w, i0:i0 + h] += np.float32(height)
    return e


def download(ctx, layers=LAYERS):
    ctx.sync()
    return {k: ctx.download(k) for k in layers}


def run(capi, elevs, p, res, origin, face, run_flags=None):
    elevs = np.asarray(elevs, np.float32)
    batch, cols, rows = elevs.shape
    with capi.Context(0) as ctx:
        ctx.set_option(capi.OPT_FACE_FLAGS, face)
        ctx.set_params(p)
        ctx.set_geometry(rows, cols, batch, res, origin)
        ctx.upload_elevation(elevs)
        if face:
            assert_device_flags(ctx, elevs, p.fp_critical_step)
        ctx.run_chain(capi.RUN_FOOTPRINT | capi.RUN_FOOTPRINT_MEMO if run_flags is None else run_flags)
        return download(ctx)


def assert_device_flags(ctx, elevs, crit):
    got, want = ctx.download_face_flags(), flags_numpy(elevs, crit)[0]
    assert got.shape == want.shape
    assert np.array_equal(got, want), f"device face flags: {int((got < want).sum())} missing, {int((got > want).sum())} extra of {int(want.sum())} set"


@pytest.mark.parametrize("rows,cols,batch", [(200, 150, 2), (1, 37, 1), (67, 1, 1), (130, 35, 3), (257, 70, 1)])
def test_device_flags_equal_the_definition(capi, rows, cols, batch):
    """What the upload's pass writes against the numpy restatement, byte for byte: NaN speckle and regions, plateaus, spikes
    (infinite ones too); rows no multiple of 64, columns no multiple of 4 or 32, one-cell-wide maps, more than one map."""
    rng = np.random.default_rng(1000 * rows + cols)
    elevs = np.stack([terrain(rng, rows, cols) for _ in range(batch)])
    elevs[-1, -1, -1] = np.float32(1.0)  # a drop at the layer's last cell
    with capi.Context(0) as ctx:
        ctx.set_geometry(rows, cols, batch, 0.05, (0.0, 0.0))
        ctx.upload_elevation(elevs)
        assert_device_flags(ctx, elevs, ctx.get_params().fp_critical_step)
        ctx.set_option(capi.OPT_FACE_FLAGS, 0)
        with pytest.raises(Exception):
            ctx.download_face_flags()


def assert_identical(got, want, what):
    for k in want:
        a, b = np.asarray(got[k], np.float32).view(np.uint32), np.asarray(want[k], np.float32).view(np.uint32)
        assert np.array_equal(a, b), f"{what}: layer {k} differs in {int((a != b).sum())} cells between TE_OPT_FACE_FLAGS 1 and 0"


def assert_oracle(oracle, got, elevs, op, res, origin, what):
    batch, cols, rows = elevs.shape
    assert rows <= 320 and cols <= 320
    g = oracle.geom(rows, cols, res, origin)
    per = rows * cols
    for b in range(batch):
        want = oracle.chain(g, op, elevs[b])
        want["traversability_footprint"] = oracle.footprint(g, op, elevs[b], want)
        for k in list(OUT_LAYERS) + ["traversability_footprint"]:
            n_bad, mx, nn = compare_layer(k, got[k][b * per:(b + 1) * per], want[k])
            assert n_bad == 0, f"{what}, map {b}, {k}: {n_bad} mismatches (NaN pattern {nn}), max |d| = {mx:.3g}"


def both(capi, oracle, elevs, op, res=0.05, origin=(0.0, 0.0), what="", mixed=True):
    """Flags on against flags off (bit for bit), the oracle on small maps; the map must have flat granules (and faces, if mixed)."""
    elevs = np.asarray(elevs, np.float32)
    if elevs.ndim == 2:
        elevs = elevs[None]
    fl, _ = flags_numpy(elevs, op.fp_critical_step)
    assert (fl == 0).any(), "the case has no flat granule"
    assert not mixed or (fl == 1).any(), "the case has no face"
    p = to_te_params(capi, op)
    on = run(capi, elevs, p, res, origin, 1)
    off = run(capi, elevs, p, res, origin, 0)
    assert_identical(on, off, what)
    assert not mixed or (np.asarray(on["traversability_step"]) == 0.0).any(), "the case has no cell with a step score of 0"
    if elevs.shape[1] <= 320 and elevs.shape[2] <= 320:
        assert_oracle(oracle, on, elevs, op, res, origin, what)
    return on


@pytest.mark.parametrize("d", [0, 1, 2, 3])
def test_box_edges_near_tile_borders_on_a_small_map(capi, oracle, d):
    """200 x 136 (tiles of 64 x 4): a 0.3 m box whose corner lies d cells inside the tile corner (64, 32) -- its edges d cells
    from the tile borders i = 64 and j = 32 -- and one whose far edges end d cells before the borders i = 128 and j = 96."""
    e = smooth(200, 136, 11)
    box(e, 64 + d, 32 + d)
    box(e, 128 - d - 20, 96 - d - 12)
    both(capi, oracle, e, oracle.default_params(**STEP), what=f"box {d} cells from the tile borders")


@pytest.mark.parametrize("rows,cols", [(520, 300), (520, 520)])
def test_box_edges_near_tile_borders_on_mid_size_maps(capi, oracle, rows, cols):
    """520 x 300 (90 tiles of 64 x 32 cells: still the 4-row tiles) and 520 x 520 (153: the 8-row tiles, k_fp_mask<8>): boxes whose edges lie 0 .. 3
    cells from the borders of the 8-row tiles and at their corners; flags on against flags off."""
    e = smooth(rows, cols, 12)
    for d in range(4):
        box(e, 64 + d, 40 * (d + 1) + d)                       # corner d cells inside the tile corner (64, 8 k)
        box(e, 320 - d - 20, 40 * (d + 1) + 16 - d - 12 + 8)   # far edges d cells before i = 320 and a multiple of 8
    both(capi, oracle, e, oracle.default_params(**STEP), what=f"{rows} x {cols}")


def test_slow_cells_on_flat_tiles(capi, oracle):
    """Flat tiles that hold slow cells: a ramp steeper than slope_critical whose adjacent cells differ by less than fp_critical_step
    (slope score 0, checkForSlope counts its window) and, with fp_check_roughness, a rough patch (roughness score 0)."""
    rows, cols = 200, 136
    rng = np.random.default_rng(5)
    e = smooth(rows, cols, 13)
    e[20:60, 70:130] += (0.05 * np.arange(60, dtype=np.float32))[None, :]   # 45 degrees at 0.05 m cells: 0.05 m per cell
    e[20:60, 130:] += np.float32(0.05 * 59)
    e[80:120, 10:60] += rng.uniform(-0.03, 0.03, (40, 50)).astype(np.float32)  # rough, drops below 0.12
    box(e, 150, 100)  # (and one face elsewhere)
    op = oracle.default_params(**STEP, slope_critical=0.5, rough_critical=0.01, fp_check_roughness=1)
    got = both(capi, oracle, e, op, what="slow cells on flat tiles")
    fl, _ = flags_numpy(e[None], op.fp_critical_step)
    slope0 = np.asarray(got["traversability_slope"]).reshape(cols, rows) == 0.0
    rough0 = np.asarray(got["traversability_roughness"]).reshape(cols, rows) == 0.0
    flat_cells = np.repeat(np.repeat(fl[0] == 0, 4, axis=0), 64, axis=1)[:cols, :rows]
    assert (slope0 & flat_cells).sum() > 100 and (rough0 & flat_cells).sum() > 100, "no slow cells on flat granules"


def test_nan_regions_next_to_a_face_and_an_all_nan_map(capi, oracle):
    rows, cols = 200, 136
    e = smooth(rows, cols, 14)
    box(e, 60, 30)
    e[28:36, 50:64] = np.nan      # an unobserved region against the box's edge
    e[35:50, 78:100] = np.nan     # and one that swallows a corner of it
    e[100:104, 0:200:7] = np.nan
    both(capi, oracle, e, oracle.default_params(**STEP), what="NaN regions next to a face")
    both(capi, oracle, np.full((cols, rows), np.nan, np.float32), oracle.default_params(**STEP), what="all cells NaN", mixed=False)


def test_batch_of_three_with_a_face_in_map_1_only(capi, oracle):
    rows, cols = 200, 136
    elevs = np.stack([smooth(rows, cols, 20 + b) for b in range(3)])
    box(elevs[1], 90, 50)
    fl, _ = flags_numpy(elevs, 0.12)
    assert not fl[0].any() and fl[1].any() and not fl[2].any()
    both(capi, oracle, elevs, oracle.default_params(**STEP), what="batch of 3")


def submap_edge_failures(rows, cols, res, px, py):
    """te_footprint.hip: the border sides on which the 2.5 res submap lookup of checkForStep fails (restated to pick a geometry)."""
    lx, ly = rows * res, cols * res
    ax, ay = px + (0.5 * lx - 0.5 * res), py + (0.5 * ly - 0.5 * res)

    def bound(position, ln, mp):
        sh = position - mp + 0.5 * ln
        eps = 10.0 * 2.220446049250313e-16
        if abs(position) > 1.0:
            eps *= abs(position)
        sh = eps if sh <= 0 else (ln - eps if sh >= ln else sh)
        return sh + mp - 0.5 * ln

    def ok(x, ln, mp, n):
        t = -((x - mp) - 0.5 * ln)
        idx = int(-(((x - 0.5 * ln) - mp) / res))
        return 0.0 <= t < ln and 0 <= idx < n
    half = 0.5 * (2.5 * res)
    x1, y1 = ax + res * float(-(rows - 1)), ay + res * float(-(cols - 1))
    return ((0 if ok(bound(ax + half, lx, px), lx, px, rows) else 1) | (0 if ok(bound(x1 - half, lx, px), lx, px, rows) else 2) |
            (0 if ok(bound(ay + half, ly, py), ly, py, cols) else 4) | (0 if ok(bound(y1 - half, ly, py), ly, py, cols) else 8))


def test_map_border_whose_submap_lookups_fail(capi, oracle):
    """A geometry on whose last row and last column the submap lookup fails (the map's far corner lies at the origin, 100 m
    from its other end): the tiles along those borders keep the staged path, step == 0 cells there are decided by check_step."""
    rows, cols, res, origin = 200, 136, 0.5, (50.0, 34.0)
    assert submap_edge_failures(rows, cols, res, *origin) == 10
    e = smooth(rows, cols, 15)
    box(e, rows - 12, cols - 9, h=8, w=6)   # step == 0 cells within 3 cells of both failing borders
    box(e, rows - 30, 20, h=28, w=10)       # ... along i = rows - 1 only
    box(e, 30, 60)
    op = oracle.default_params(normals_radius=0.5, rough_radius=0.5, step_radius1=1.5, step_radius2=1.5, fp_radius=3.0, fp_offset=1.5,
                               fp_max_gap=3.0)
    got = both(capi, oracle, e, op, res=res, origin=origin, what="failing border")
    step0 = np.asarray(got["traversability_step"]).reshape(cols, rows) == 0.0
    assert step0[:, rows - 3:].any() and step0[cols - 3:, :].any(), "no step == 0 cell at the failing borders"


def test_stale_flags_tile_upload_and_whole_upload_with_graph_replay(capi, oracle):
    """2048 x 2048 (2^22 cells: whole-map launches are captured and replayed).  A flat map, a run; a 64 x 64 tile with a box
    (te_upload_tile: the flags are unknown from then on), a run; the whole layer again (flags rebuilt, now with the face), a
    run.  Each result against a context with TE_OPT_FACE_FLAGS = 0 that was given that elevation whole."""
    n = 2048
    flat = smooth(n, n, 16)
    assert not flags_numpy(flat[None], 0.12)[0].any()
    tile = np.ascontiguousarray(flat[1000:1064, 700:764] + np.float32(0.0))
    tile[20:40, 10:50] += np.float32(0.3)
    boxed = flat.copy()
    boxed[1000:1064, 700:764] = tile
    p = capi.default_params(**STEP)
    rf = capi.RUN_FOOTPRINT | capi.RUN_FOOTPRINT_MEMO
    with capi.Context(0) as ctx, capi.Context(0) as ref:
        ref.set_option(capi.OPT_FACE_FLAGS, 0)
        for c in (ctx, ref):
            c.set_params(p)
            c.set_geometry(n, n, 1, 0.05, (0.0, 0.0))
        ctx.upload_elevation(flat)
        ctx.run_chain(rf)
        ctx.run_chain(rf)  # (the second launch replays the captured graph)
        ref.upload_elevation(flat)
        ref.run_chain(rf)
        assert_identical(download(ctx), download(ref), "flat map")
        ctx.upload_tile(tile, 0, 700, 1000)
        ctx.run_chain(rf)
        ref.upload_elevation(boxed)
        ref.run_chain(rf)
        want = download(ref)
        assert_identical(download(ctx), want, "after te_upload_tile of a box")
        ctx.upload_elevation(boxed)
        ctx.run_chain(rf)
        ctx.run_chain(rf)
        assert_identical(download(ctx), want, "after the whole layer was uploaded again")


def test_lowering_fp_critical_step_with_a_flat_map_resident(capi, oracle):
    """Flags built at 0.12 (all clear) say nothing at 0.03, where the same terrain has faces."""
    rows, cols = 320, 200
    e = smooth(rows, cols, 17) * np.float32(2.0)  # adjacent cells up to several centimetres apart
    assert not flags_numpy(e[None], 0.12)[0].any() and flags_numpy(e[None], 0.03)[0].any()
    rf = capi.RUN_FOOTPRINT | capi.RUN_FOOTPRINT_MEMO
    with capi.Context(0) as ctx:
        ctx.set_params(capi.default_params(**STEP))
        ctx.set_geometry(rows, cols, 1, 0.05, (0.0, 0.0))
        ctx.upload_elevation(e)
        ctx.run_chain(rf)
        ctx.set_params(capi.default_params(**STEP, fp_critical_step=0.03))
        ctx.run_chain(rf)
        got = download(ctx)
    want = run(capi, e[None], capi.default_params(**STEP, fp_critical_step=0.03), 0.05, (0.0, 0.0), 0)
    assert_identical(got, want, "fp_critical_step 0.12 -> 0.03")
    assert_identical(run(capi, e[None], capi.default_params(**STEP, fp_critical_step=0.03), 0.05, (0.0, 0.0), 1), want, "a context built at 0.03")
    assert_oracle(oracle, got, e[None], oracle.default_params(**STEP, fp_critical_step=0.03), 0.05, (0.0, 0.0), "fp_critical_step 0.03")


def test_region_run_over_a_flat_tile_and_a_face_tile(capi, oracle):
    """te_run_chain_region with the footprint flag: the mask kernel runs on the region's tiles alone, with the flags of its map."""
    rows, cols = 320, 264
    elevs = np.stack([smooth(rows, cols, 30), smooth(rows, cols, 31)])
    box(elevs[1], 130, 100)  # in the tiles right of i = 128; the region below also covers flat tiles left of it
    rf = capi.RUN_FOOTPRINT | capi.RUN_FOOTPRINT_MEMO
    out = []
    for face in (1, 0):
        with capi.Context(0) as ctx:
            ctx.set_option(capi.OPT_FACE_FLAGS, face)
            ctx.set_params(capi.default_params(**STEP))
            ctx.set_geometry(rows, cols, 2, 0.05, (0.0, 0.0))
            ctx.upload_elevation(elevs)
            ctx.run_chain(rf)
            ctx.run_chain_region(1, 70, 80, 100, 60, flags=rf)
            out.append(download(ctx))
    assert_identical(out[0], out[1], "region run")
    assert_oracle(oracle, out[0], elevs, oracle.default_params(**STEP), 0.05, (0.0, 0.0), "region run")


def test_large_map_kernel_with_three_boxes(capi, oracle):
    """2048 x 1024: 1024 tiles of 64 x 32 cells, k_fp_mask<32>.  Flags on against flags off."""
    rows, cols = 2048, 1024
    e = smooth(rows, cols, 18)
    box(e, 64 * 5 + 1, 32 * 7 + 2)
    box(e, 64 * 20 - 22, 32 * 11 - 13, height=-0.25)
    box(e, 1000, 500, h=150, w=90)
    both(capi, oracle, e, oracle.default_params(**STEP), what="2048 x 1024")
