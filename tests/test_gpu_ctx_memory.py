"""One context through a sequence that makes every device buffer it keeps exist, regrow and be released: geometry 48 x 40,
the calls below, te_set_geometry to 96 x 72 (everything freed with the layers is released and comes back larger), the same
calls, back to 48 x 40, the same calls once more.  What can go wrong is a pointer DERIVED from a buffer that was released or
regrown (the tables of the footprint of any reach, the filter discs' tables, the tie scratch, the hole queue, the second
polygon layer, the face flags, the slab's layers): a stale one reads or writes freed memory and the layers differ.  So after
each round every downloaded layer and every path result must be bit-identical to the same calls on a FRESH context of
that geometry, and the chain's layers must match the oracle like in the parity tests (tests/helpers.py, 1e-5).

The calls of a round: te_upload_image (two transparent pixels: the sparse-hole march and its queue), chain + footprint at a
tie radius of the step filter (the tie scratch), TE_OPT_FP_ANY_REACH = 1 and TE_OPT_FILTER_ANY_RADIUS = 2 passes, occupancy,
cloud and an expression with a reduction, robot_slope + te_check_inclination, the polygon footprint (twice: its table stream
is reused) and the polygon checks, the circular path checks on the footprint layer and te_check_footprint_paths_radius
with 20 distinct radii (more than the 16 cached tables: the tables of the call alone), two tiles through the staging slots,
and the radius filter, a window expression and the median fill in place on traversability_slope (the copy of the input
such a call reads: allocated, released with the layers, back larger).

That the inputs reach the tie scratch and the hole queue is checked, not trusted: the step radius is on the circle by
build_disc's own rule (tie_offsets below restates it) and the upload's counts satisfy te_hole_routing.h's rule for the sparse
march (sparse_march below); the chain is also run on the generic kernels, which use neither buffer, against the same oracle.

The sizes are the smallest that still regrow; no figure of free device memory is looked at (the machines are shared)."""
import numpy as np
import pytest

from tests.helpers import OUT_LAYERS, assert_layers_match, to_te_params
from tests.test_hole_routing import count_invalid
from tests.test_path_options import random_segments, robot_slope_layer
from tests.test_paths import random_paths

pytestmark = pytest.mark.gpu

RES, POS = 0.05, (1.0, -0.5)
SMALL, LARGE = (48, 40), (96, 72)
FOOTPRINT = np.array([[0.2, 0.15], [0.2, -0.15], [-0.2, -0.15], [-0.2, 0.15]])
ALL_LAYERS = OUT_LAYERS + ("traversability_footprint", "slope_footprint", "step_footprint", "roughness_footprint")


@pytest.fixture(scope="module")
def capi():
    from traversability_estimation_amd import capi
    capi.load()
    return capi


def params(oracle):
    # the step windows at exactly 2 cells: cells on their circle (a tie radius); the footprint of 9 cells takes the
    # shape-specialised route unless TE_OPT_FP_ANY_REACH says otherwise
    return oracle.default_params(normals_radius=0.15, rough_radius=0.15, step_radius1=2 * RES, step_radius2=2 * RES, fp_radius=0.3, fp_offset=0.15)


def tie_offsets(radius, res):
    """build_disc (te_disc.h): the offsets whose squared norm equals (radius / res)^2 to within 1e-9 relative."""
    q = (radius / res) * (radius / res)
    tol = 1e-9 * max(q, 1.0)
    lim = int(np.floor(np.sqrt(q + tol))) + 1
    return [(a, b) for a in range(-lim, lim + 1) for b in range(-lim, lim + 1) if abs(a * a + b * b - q) <= tol]


def sparse_march(elev):
    """holes_sparse (te_hole_routing.h) on the upload's two counts: at most 2 per mille of the cells, in runs below 8 on average."""
    invalid, runs = count_invalid(elev)
    return 0 < invalid <= 0.002 * elev.size and not runs * 8 <= invalid


def inputs(shape):
    """The round's inputs, a function of the geometry alone: every round of a geometry and its fresh context get the same."""
    from traversability_estimation_amd import synth
    rows, cols = shape
    rng = np.random.default_rng(rows * 1000 + cols)
    elev = synth.with_steps(synth.perlin_elevation(rows, cols, seed=rows, amplitude=0.15), 4, seed=cols).reshape(cols, rows).T  # (rows, cols): the image
    grey = np.clip((elev - elev.min()) / (elev.max() - elev.min()), 0.0, 1.0)
    img = np.empty((rows, cols, 4), np.uint16)
    img[..., :3] = np.round(grey * 65535.0).astype(np.uint16)[..., None]
    img[..., 3] = 65535
    img[rows // 3, cols // 2, 3] = 0  # two unobserved cells, apart: few and scattered
    img[rows // 2, cols // 4, 3] = 0

    class G:  # (what random_paths / random_segments read)
        pass
    g = G()
    g.rows, g.cols, g.res, g.pos_x, g.pos_y, g.len_x, g.len_y = rows, cols, RES, POS[0], POS[1], rows * RES, cols * RES
    paths = random_paths(rng, g, 60)
    yaw = rng.uniform(-3.0, 3.0, 40)
    poses = [np.array([[x, y, 0.0, 0.0, 0.0, np.sin(0.5 * a), np.cos(0.5 * a)] for (x, y) in p]) for p, a in zip(paths[:40], yaw) if len(p)]
    return dict(img=img, robot_slope=robot_slope_layer(rng, g), segments=random_segments(rng, g, 50), paths=paths,
                radii=0.05 + 0.02 * (np.arange(len(paths)) % 20), poses=poses,
                polygons=[c + 0.4 * FOOTPRINT for c in rng.uniform([POS[0] - 1.0, POS[1] - 0.8], [POS[0] + 1.0, POS[1] + 0.8], (30, 2))])


def run_round(capi, ctx, shape, te_p):
    """Steps 1 .. 8 on `ctx`; returns {name: array} of everything the calls gave back."""
    rows, cols = shape
    m = inputs(shape)
    out = {}

    def layers(tag, names=ALL_LAYERS):
        ctx.sync()
        for k in names:
            out[f"{tag}/{k}"] = ctx.download(k)

    fp = capi.RUN_FOOTPRINT | capi.RUN_FOOTPRINT_MEMO
    ctx.set_params(te_p)
    ctx.set_geometry(rows, cols, 1, RES, POS)
    ctx.upload_image(m["img"], "rgba16", lower=0.0, upper=0.6)
    layers("image", ("elevation",))
    ctx.run_chain(fp)
    layers("chain")
    out["face_flags"] = ctx.download_face_flags()
    ctx.run_chain(fp | capi.RUN_GENERIC_KERNELS)
    layers("generic")
    ctx.set_option(capi.OPT_FP_ANY_REACH, 1)
    ctx.run_chain(fp)
    layers("fp_any_reach")
    ctx.set_option(capi.OPT_FP_ANY_REACH, 0)
    ctx.set_option(capi.OPT_FILTER_ANY_RADIUS, 2)
    ctx.run_chain(fp)
    layers("filter_any_radius")
    ctx.set_option(capi.OPT_FILTER_ANY_RADIUS, 0)
    ctx.run_chain(fp)
    layers("chain_again")
    out["occupancy"] = ctx.download_occupancy(["traversability", "traversability_footprint"], data_min=0.0, data_max=1.0).copy()
    out["cloud"] = ctx.download_cloud(["elevation", "traversability"], "elevation").copy()
    ctx.run_expression("traversability - meanOfFinites(traversability) + maxOfFinites(elevation)")
    layers("expression", ("traversability",))
    ctx.run_chain(fp)  # (the chain's own combined layer again, for the checks below)
    ctx.sync()
    ctx.upload_layer("robot_slope", m["robot_slope"])
    out["incl_ok"], out["incl_status"] = ctx.check_inclination(m["segments"])
    for k, yaw in enumerate((0.4, -1.1)):
        ctx.run_polygon_footprint(FOOTPRINT, yaw)
        layers(f"polygon{k}", ("traversability_x", "traversability_rot"))
    out["poly_ok"], out["poly_trav"] = ctx.polygons_traversable(m["polygons"])
    hull = ctx.polygon_untraversable_hull(4.0 * FOOTPRINT + np.array(POS))
    out["hull_ok"], out["hull_trav"], out["hull"] = np.array([hull[0]]), np.array([hull[1]]), hull[2]
    ctx.set_check_robot_inclination(True)
    for k, v in enumerate(ctx.check_polygon_footprint_paths(m["poses"], np.hstack([FOOTPRINT, np.zeros((4, 1))]))):
        out[f"polygon_paths{k}"] = v
    for k, v in enumerate(ctx.check_footprint_paths(m["paths"])):
        out[f"paths{k}"] = v
    ctx.set_check_robot_inclination(False)
    got = ctx.check_footprint_paths_radius(m["paths"], m["radii"], offset=0.15, want_stats=True)
    assert got[3]["n_radius_classes"] == 20
    for k, v in enumerate(got[:3]):
        out[f"paths_radius{k}"] = v
    for k, (h, w) in enumerate(((8, 8), (8, 8), (24, 16), (24, 16))):  # both slots, then both grown
        t = np.empty((w, h), np.float32)
        ctx.download_tile_async("traversability", 0, 3, 5, t)
        ctx.sync()
        out[f"tile{k}"] = t
    # the three layer filters in place on a layer nothing above reads again: the copy of the input each of them reads
    ctx.run_radius_filter("mean", 1.5 * RES, "traversability_slope")
    ctx.run_window_expression("mean(traversability_slope)", dict(window_size=3), "traversability_slope")
    ctx.run_median_fill(None, "traversability_slope")
    layers("filters_in_place", ("traversability_slope",))
    return out


def assert_identical(got, want, ctx):
    assert got.keys() == want.keys()
    for k in want:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes(), f"{ctx}: {k} differs from the fresh context's"


@pytest.fixture(scope="module")
def fresh(capi, oracle):
    """The same calls on a fresh context of each geometry, once."""
    te_p = to_te_params(capi, params(oracle))
    out = {}
    for shape in (SMALL, LARGE):
        with capi.Context(0) as ctx:
            out[shape] = run_round(capi, ctx, shape, te_p)
    return out


def test_every_buffer_exists_regrows_and_is_released(capi, oracle, fresh):
    op = params(oracle)
    te_p = to_te_params(capi, op)
    assert len(tie_offsets(op.step_radius1, RES)) == 4 and len(tie_offsets(op.step_radius2, RES)) == 4  # (+-2, 0), (0, +-2): the tie scratch
    with capi.Context(0) as ctx:
        for n, shape in enumerate((SMALL, LARGE, SMALL)):
            got = run_round(capi, ctx, shape, te_p)
            tag = f"round {n + 1}, {shape[0]} x {shape[1]}"
            assert_identical(got, fresh[shape], tag)
            g = oracle.geom(shape[0], shape[1], RES, POS)
            want = oracle.chain(g, op, got["image/elevation"])
            assert sparse_march(got["image/elevation"])  # (the hole queue)
            for chain in ("chain", "generic", "chain_again"):
                print(tag, chain, assert_layers_match({k: got[f"{chain}/{k}"] for k in OUT_LAYERS}, want, ctx=f"{tag}: {chain} against the oracle"))
            assert np.isnan(got["image/elevation"]).sum() == 2
