"""The sums of the circular footprint pass on traversability layers whose values leave [0, 1], against the oracle's
isTraversable on the layers the device holds (the three score layers are downloaded, the traversability layer is the one the
test wrote or the device combined: the sum pass alone is under test, as tests/test_polygon.py does it for the polygon pass).

Two of the five sum routes (te_fp_route.h) store T' + 4096 U per cell and take the count of untraversable cells back out of the
disc sum; that is right only while every |T'| and every disc's |sum T'| stay below 2048.  The families below cross that
limit through every door the C-ABI has: layers from outside (te_upload_layer, te_run_expression, te_device_ptr) in other
units, negative and mixed-sign layers, single huge cells, a large fp_default, and layers the chain itself wrote with
plain weights (the sum instead of the mean of the scores).  The fixed-point routes are driven at saturation: every cell at
the cap, the largest discs, every exponent k from 23 down to its floor 17 and the first cap beyond.

The library does not say which kernel it launched: every case's route and k are pinned on the CPU by the named case of the
same name in tests/cpu/fp_route_check.cpp (tests/test_fp_route.py, tests/footprint_value_cases.py).

Tolerances: TOL * max(1, M) with M the largest |finite value| or |fp_default| entering the sums (test_gpu_round3's precedent:
4e-5 for values reaching 4); NaN patterns equal; cells the oracle gives 0 exactly 0; a constant layer's unblocked discs
bit for bit the constant; fixed point: 2^-(k+1) + 2^-23 |want|, the bound the kernels' comments derive.

The boundary pair (sum_just_below_2048, sum_just_above_2048; fv_bound_below_reach18, fv_bound_above_reach18) marks where a
packed sum turns wrong: below it the double kernels may be planned, from it on they must not be.

The route of any reach takes a disc's runs as differences of one prefix sum per map column, so its error follows the whole
column's sum of |values|, not the disc's (include/travgpu.h, te_run_footprint): test_small_values_below_a_large_head_of_the_column
holds a magnitude ratio of 1e6 within every column to that model.
"""
import ctypes
import math

import numpy as np
import pytest

from tests import footprint_value_cases as fv
from tests.helpers import TOL, to_te_params

pytestmark = pytest.mark.gpu

FILTER_CELLS = 3  # radius of the filter discs, tie-free


@pytest.fixture(scope="module")
def capi():
    from traversability_estimation_amd import capi
    capi.load()
    assert capi.device_count() >= 1
    return capi


_ELEV = {}


def elevation(kind, rows, cols):
    """(cols, rows) float32: 'boxes' a gentle plane with three boxes, 'flat' a level map with one box, 'plane' a constant
    gradient with one box; each with a small block of unobserved cells."""
    key = (kind, rows, cols)
    if key not in _ELEV:
        from traversability_estimation_amd import synth
        i = np.arange(rows, dtype=np.float64)[None, :]
        j = np.arange(cols, dtype=np.float64)[:, None]
        if kind == "boxes":
            e = synth.with_steps((0.001 * i + 0.0005 * j).astype(np.float32), 3, seed=5, height=(0.25, 0.4))
        else:
            e = ((0.004 * i + 0.002 * j) if kind == "plane" else np.zeros((cols, rows))).astype(np.float32)
            e[12:17, 8:14] += np.float32(0.3)
        e[52:55, 30:34] = np.nan
        _ELEV[key] = np.ascontiguousarray(e)
    return _ELEV[key]


def params(oracle, geo, **over):
    from traversability_estimation_amd import synth
    r = synth.benchmark_radius(FILTER_CELLS, fv.RES)
    rad, off = fv.radii(geo)
    return oracle.default_params(normals_radius=r, rough_radius=r, step_radius1=r, step_radius2=r, fp_radius=rad, fp_offset=off, **over)


def dilate(mask, q):
    """Cells within squared distance q (in cells) of a set cell; nothing wraps around the border."""
    cols, rows = mask.shape
    n = int(math.sqrt(q))
    pad = np.pad(mask, n)
    out = np.zeros_like(mask)
    for a in range(-n, n + 1):
        for b in range(-n, n + 1):
            if a * a + b * b <= q:
                out |= pad[n + b:n + b + cols, n + a:n + a + rows]
    return out


def disc_classes(oracle, g, op, elev, layers, geo, nan_cells):
    """(discs that surely hold an untraversable cell, discs that surely hold none, discs that surely hold a NaN cell, discs
    that surely hold none) -- 'surely': a radius one cell inside / outside the footprint's."""
    rows, cols = g.rows, g.cols
    _, memo = oracle.footprint(g, op, elev, layers, want_memo=True)
    untrav = np.zeros(rows * cols, bool)
    for m in memo.values():
        untrav |= (m == 0)
    untrav = untrav.reshape(cols, rows)
    rc = sum(fv.GEOS[geo][:2])
    inner, outer = (rc - 1.0) ** 2, (rc + 1.0) ** 2
    return (dilate(untrav, inner).reshape(-1), ~dilate(untrav, outer).reshape(-1), dilate(nan_cells, inner).reshape(-1),
            ~dilate(nan_cells, outer).reshape(-1), untrav)


def run_device(capi, op, elev, rows, cols, writer=None, any_reach=False, region=None):
    """The footprint layer and the four layers the sum pass read, as the device holds them.  writer: called with the context
    behind a chain without the footprint flag, writes the traversability layer; None: the chain's own layer, footprint flag."""
    with capi.Context(0) as ctx:
        ctx.set_params(to_te_params(capi, op))
        ctx.set_geometry(rows, cols, 1, fv.RES, fv.POS)
        if any_reach:
            ctx.set_option(capi.OPT_FP_ANY_REACH, 1)
        ctx.upload_elevation(elev)
        if writer is None:
            ctx.run_chain(capi.RUN_FOOTPRINT)
        else:
            ctx.run_chain(0)
            writer(ctx)
            ctx.run_footprint()
        if region is not None:
            r0, c0, h, w, tile = region
            ctx.upload_tile(np.ascontiguousarray(tile), 0, r0, c0)
            ctx.run_chain_region(0, r0, c0, h, w, flags=capi.RUN_FOOTPRINT)
        ctx.sync()
        names = ("traversability_slope", "traversability_step", "traversability_roughness", "traversability", "traversability_footprint")
        return {k: ctx.download(k) for k in names}


def check(name, got, want, bound):
    """NaN patterns equal, the oracle's zeros exactly zero, every other cell within `bound` (a number or one per cell)."""
    got, want = np.asarray(got, np.float32).reshape(-1), np.asarray(want, np.float32).reshape(-1)
    gn, wn = np.isnan(got), np.isnan(want)
    both = ~gn & ~wn
    err = np.zeros(got.shape, np.float64)
    err[both] = np.abs(got[both].astype(np.float64) - want[both].astype(np.float64))
    bound = np.broadcast_to(np.asarray(bound, np.float64), got.shape)
    worst = int(np.argmax(err - bound))
    print(f"{name}: max|d| = {err.max():.3g} (bound there {bound[int(np.argmax(err))]:.3g}), NaN pattern differs in {int((gn != wn).sum())} cells, "
          f"{int(((want == 0) & (got != 0)).sum())} of {int((want == 0).sum())} zeros not zero, {int((err > bound).sum())} cells beyond the bound "
          f"(cell {worst}: got {got[worst]!r}, want {want[worst]!r})")
    assert not (gn != wn).any(), f"{name}: NaN pattern"
    assert not ((want == 0) & (got != 0)).any(), f"{name}: a disc the oracle gives 0"
    assert not (err > bound).any(), f"{name}: {int((err > bound).sum())} cells, max|d| {err.max():.3g}"


# ---- layers from outside -----------------------------------------------------------------------------------------------------
# family -> (rng, shape, geo, untraversable cells) -> (layer, M, fp_default or None, the constant or None)
def _const(c):
    return lambda rng, shape, geo, untrav: (np.full(shape, c, np.float32), abs(c), None, np.float32(c))


def _spikes(rng, shape, geo, untrav):
    """0.5 everywhere; single cells of 5000 and -5000, one pair two cells from an untraversable cell (a disc with one
    untraversable cell and a sum below -2048) and one pair in the open: the per-cell limit."""
    t = np.full(shape, 0.5, np.float32)
    js, is_ = np.nonzero(untrav)
    j, i = int(js[0]), int(is_[0])
    t[min(j + 2, shape[0] - 1), i] = 5000.0
    t[j, min(i + 2, shape[1] - 1)] = -5000.0
    t[shape[0] - 9, shape[1] - 11] = 5000.0
    t[shape[0] - 20, shape[1] - 30] = -5000.0
    return t, 5000.0, None, None


def _boundary(sign):
    def make(rng, shape, geo, untrav):
        c = np.float32(0.5 * fv.K_UOFF / fv.disc_cells(geo) * (1.0 + sign * 1e-3))  # the largest disc sums to 2048 -+ 2
        return np.full(shape, c, np.float32), float(c), None, c
    return make


FAMILIES = {
    "const_100": _const(100.0),
    "uniform_0_1e4": lambda rng, shape, geo, untrav: (rng.uniform(0.0, 1e4, shape).astype(np.float32), 1e4, None, None),
    "const_1e6": _const(1e6),
    "uniform_m50_0": lambda rng, shape, geo, untrav: (rng.uniform(-50.0, 0.0, shape).astype(np.float32), 50.0, None, None),
    "mixed_pm1e3": lambda rng, shape, geo, untrav: (rng.uniform(-1e3, 1e3, shape).astype(np.float32), 1e3, None, None),
    "spikes_pm5000": _spikes,
    "unit_default_50": lambda rng, shape, geo, untrav: (rng.uniform(0.0, 1.0, shape).astype(np.float32), 50.0, 50.0, None),
    "sum_just_below_2048": _boundary(-1),
    "sum_just_above_2048": _boundary(+1),
}
EXT_GEOS = ("r5", "r9", "reach18", "tie15", "rows48")


def external_case(capi, oracle, geo, family, any_reach, write=None):
    rows, cols = fv.GEOS[geo][3:]
    elev = elevation("boxes", rows, cols)
    g = oracle.geom(rows, cols, fv.RES, fv.POS)
    nan_cells = np.isnan(elev)
    op0 = params(oracle, geo)
    scores = oracle.chain(g, op0, elev)
    untrav = disc_classes(oracle, g, op0, elev, scores, geo, nan_cells)[4]
    t, M, default, const = FAMILIES[family](np.random.default_rng(17), (cols, rows), geo, untrav)
    t[nan_cells] = np.nan  # unobserved cells: fp_default enters the sums
    op = params(oracle, geo, **({} if default is None else {"fp_default": default}))
    M = max(M, abs(op.fp_default))
    got = run_device(capi, op, elev, rows, cols, writer=write(t) if write else (lambda ctx: ctx.upload_layer("traversability", t)),
                     any_reach=any_reach)
    if write is None:
        assert np.array_equal(got["traversability"].view(np.uint32), t.reshape(-1).view(np.uint32))
    want = oracle.footprint(g, op, elev, got)
    blocked, clear, nan_in, nan_out, _ = disc_classes(oracle, g, op, elev, got, geo, nan_cells)
    assert blocked.any() and clear.any() and nan_in.any() and (clear & nan_out).any(), "blocked, unblocked and NaN-touching discs all occur"
    assert (blocked & nan_in).any() or (clear & nan_in).any()
    name = f"fv_ext_{geo}{'_def50' if default else ''}{'_any' if any_reach else ''} {family}"
    if const is not None:  # an unblocked disc of a constant layer: the mean IS the constant (sums of k * c are exact in double)
        exact = clear & nan_out
        assert np.array_equal(want[exact].view(np.uint32), np.full(int(exact.sum()), const, np.float32).view(np.uint32))
        bad = got["traversability_footprint"][exact].view(np.uint32) != const.view(np.uint32)
        print(f"{name}: {int(bad.sum())} of {int(exact.sum())} unblocked discs are not the constant bit for bit")
        assert not bad.any(), f"{name}: unblocked discs of a constant layer"
    check(name, got["traversability_footprint"], want, TOL * max(1.0, M))
    return got["traversability_footprint"]


@pytest.mark.parametrize("any_reach", [False, True], ids=["routed", "any_reach"])
@pytest.mark.parametrize("family", list(FAMILIES))
@pytest.mark.parametrize("geo", EXT_GEOS)
def test_uploaded_layer(capi, oracle, geo, family, any_reach):
    """CPU-pinned as fv_ext_<geo>, fv_ext_<geo>_def50 (family unit_default_50) and fv_ext_<geo>_any (the control)."""
    assert f"fv_ext_{geo}" in fv.PLANNED and f"fv_ext_{geo}_def50" in fv.PLANNED and f"fv_ext_{geo}_any" in fv.PLANNED
    external_case(capi, oracle, geo, family, any_reach)


@pytest.mark.parametrize("geo", ["r9", "reach18"])
def test_small_values_below_a_large_head_of_the_column(capi, oracle, geo):
    """Uniform values in [0, 1] with 1e6 in row 0 of every column, uploaded (routes: fv_ext_<geo>, the route of any reach).
    Every disc further down a column is a sum of small values taken as differences of prefixes near 1e6.  The bound is the
    error model include/travgpu.h states, worked out for this map: a prefix entry is the end of at most 14 additions (a
    64-wide scan of 6 steps and the carry, two chunks of 96 rows), a run two entries and a subtraction, the disc's 2 reach + 1
    runs as many additions more -- under 32 roundings of 2^-53 A per run, A the largest column's sum of |values| -- and the
    mean is that over at least one cell, plus one float32 ulp between two roundings of nearly the same number.  TOL * M would
    be 10 here and would hold nothing; a prefix kept in float would miss this bound by five orders of magnitude."""
    rows, cols = fv.GEOS[geo][3:]
    elev = elevation("boxes", rows, cols)
    g = oracle.geom(rows, cols, fv.RES, fv.POS)
    op = params(oracle, geo)
    t = np.random.default_rng(23).uniform(0.0, 1.0, (cols, rows)).astype(np.float32)
    t[:, 0] = 1e6
    t[np.isnan(elev)] = np.nan
    got = run_device(capi, op, elev, rows, cols, writer=lambda ctx: ctx.upload_layer("traversability", t))
    assert np.array_equal(got["traversability"].view(np.uint32), t.reshape(-1).view(np.uint32))
    want = oracle.footprint(g, op, elev, got)
    A = np.where(np.isfinite(t), np.abs(t), abs(op.fp_default)).astype(np.float64).sum(axis=1).max()
    reach = int(sum(fv.GEOS[geo][:2]))
    assert 1e6 < A < 1e6 + rows and reach in (9, 18)
    small = np.nan_to_num(np.asarray(want, np.float64).reshape(-1), nan=np.inf)
    assert ((small > 0.0) & (small < 1.0)).sum() > rows * cols // 4  # (means of small values below the head: what is under test)
    bound = (2 * reach + 1) * 2.0 ** -48 * A + 2.0 ** -23 * np.abs(np.nan_to_num(np.asarray(want, np.float64).reshape(-1)))
    check(f"fv_ext_{geo} head of 1e6", got["traversability_footprint"], want, bound)


def _hip_memcpy_to_device(dst, host):
    """A plain hipMemcpy (host to device) through the HIP runtime the library itself is linked against: the symbol is looked
    up from libtravgpu.so's own handle (dlsym searches a library and what it depends on), never by a runtime's file name,
    so no second runtime can come into the process.  No torch."""
    from traversability_estimation_amd import capi
    hip = ctypes.CDLL(capi.LIB_PATH)  # (already loaded by capi.load(): the same handle)
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    hip.hipMemcpy.restype = ctypes.c_int
    assert hip.hipMemcpy(ctypes.c_void_p(dst), host.ctypes.data_as(ctypes.c_void_p), host.nbytes, 1) == 0


@pytest.mark.parametrize("geo", ["r9", "tie15"])
def test_three_writers_of_the_same_layer(capi, oracle, geo):
    """100 * traversability_slope written by te_run_expression, the same values by te_upload_layer and by a hipMemcpy through
    te_device_ptr: three contexts, one footprint layer, the oracle's on those values (routes: fv_ext_<geo>)."""
    rows, cols = fv.GEOS[geo][3:]
    elev = elevation("boxes", rows, cols)
    g = oracle.geom(rows, cols, fv.RES, fv.POS)
    op = params(oracle, geo)
    by_expr = run_device(capi, op, elev, rows, cols, writer=lambda ctx: ctx.run_expression("100 * traversability_slope"))
    t = by_expr["traversability"].copy()
    assert np.nanmax(t) > 90.0 and np.isnan(t).any()  # (the slope score of the gentle plane is 0.98)
    want = oracle.footprint(g, op, elev, by_expr)
    check(f"fv_ext_{geo} expression", by_expr["traversability_footprint"], want, TOL * 100.0)
    by_upload = run_device(capi, op, elev, rows, cols, writer=lambda ctx: ctx.upload_layer("traversability", t))

    def through_pointer(ctx):
        ctx.sync()
        ptr, nbytes = ctx.device_ptr("traversability")
        assert nbytes >= t.nbytes
        _hip_memcpy_to_device(ptr, t)

    by_pointer = run_device(capi, op, elev, rows, cols, writer=through_pointer)
    for other in (by_upload, by_pointer):
        assert np.array_equal(other["traversability"].view(np.uint32), t.view(np.uint32))
        assert np.array_equal(other["traversability_footprint"].view(np.uint32), by_expr["traversability_footprint"].view(np.uint32))


# ---- layers the chain wrote with plain weights ----------------------------------------------------------------------------------
# CPU case -> (geometry, map, overrides of the default parameters)
CHAIN_CASES = {
    "fv_w1111_r15": ("r15", "flat", dict(w_scale=1.0, w_slope=1.0, w_step=1.0, w_rough=1.0)),        # the sum of the scores
    "fv_w1_10_r9": ("r9", "boxes", dict(w_scale=1.0, w_slope=10.0, w_step=10.0, w_rough=10.0)),
    "fv_wneg_r9": ("r9", "boxes", dict(w_scale=1.0, w_slope=1.0, w_step=1.0, w_rough=-1.0)),         # no bound
    "fv_def50_chain_r5": ("r5", "boxes", dict(fp_default=50.0)),
    "fv_wdefault_r15": ("r15", "flat", {}),                                                            # keep their kernels
    "fv_wdefault_r9": ("r9", "boxes", {}),
    "fv_bound_below_reach18": ("reach18", "flat", dict(w_scale=1.88 / 3.0)),                           # 1085 cells: 2039.8
    "fv_bound_above_reach18": ("reach18", "flat", dict(w_scale=1.89 / 3.0)),                           # 2050.7
}


def chain_bound(op):
    return max(1.0, abs(op.w_scale) * (abs(op.w_slope) + abs(op.w_step) + abs(op.w_rough)), abs(op.fp_default))


@pytest.mark.parametrize("case", list(CHAIN_CASES))
def test_chain_written_layer_with_plain_weights(capi, oracle, case):
    assert case in fv.PLANNED
    geo, kind, over = CHAIN_CASES[case]
    rows, cols = fv.GEOS[geo][3:]
    elev = elevation(kind, rows, cols)
    g = oracle.geom(rows, cols, fv.RES, fv.POS)
    op = params(oracle, geo, **over)
    got = run_device(capi, op, elev, rows, cols)
    want = oracle.footprint(g, op, elev, got)
    blocked, clear, nan_in, _, _ = disc_classes(oracle, g, op, elev, got, geo, np.isnan(elev))
    assert blocked.any() and clear.any() and nan_in.any()
    check(case, got["traversability_footprint"], want, TOL * chain_bound(op))


def test_chain_written_sum_of_scores_on_a_batch_of_two_maps(capi, oracle):
    """fv_w1111_r15_batch2: the flat map and the map with three boxes side by side."""
    geo, (rows, cols) = "r15", fv.GEOS["r15"][3:]
    op = params(oracle, geo, w_scale=1.0)
    g = oracle.geom(rows, cols, fv.RES, fv.POS)
    maps = [elevation("flat", rows, cols), elevation("boxes", rows, cols)]
    with capi.Context(0) as ctx:
        ctx.set_params(to_te_params(capi, op))
        ctx.set_geometry(rows, cols, 2, fv.RES, fv.POS)
        ctx.upload_elevation(np.concatenate([m.reshape(-1) for m in maps]))
        ctx.run_chain(capi.RUN_FOOTPRINT)
        ctx.sync()
        names = ("traversability_slope", "traversability_step", "traversability_roughness", "traversability", "traversability_footprint")
        got = {k: ctx.download(k).reshape(2, -1) for k in names}
    for b in range(2):
        layers = {k: np.ascontiguousarray(v[b]) for k, v in got.items()}
        check(f"fv_w1111_r15_batch2 map {b}", layers["traversability_footprint"], oracle.footprint(g, op, maps[b], layers), TOL * 3.0)


def test_chain_written_sum_of_scores_through_a_region_run(capi, oracle):
    """fv_w1111_r15_region: te_run_chain_region(TE_RUN_FOOTPRINT) over an odd-origin rectangle computes its own bound."""
    geo, (rows, cols) = "r15", fv.GEOS["r15"][3:]
    op = params(oracle, geo, w_scale=1.0)
    g = oracle.geom(rows, cols, fv.RES, fv.POS)
    elev = elevation("flat", rows, cols).copy()
    r0, c0, h, w = 21, 17, 31, 27
    tile = elev[c0:c0 + w, r0:r0 + h].copy()
    tile[5:9, 7:12] += np.float32(0.35)  # a box in the rectangle: untraversable cells, spiral walks
    got = run_device(capi, op, elev, rows, cols, region=(r0, c0, h, w, tile))
    elev[c0:c0 + w, r0:r0 + h] = tile
    want = oracle.footprint(g, op, elev, got)
    blocked, clear, _, _, _ = disc_classes(oracle, g, op, elev, got, geo, np.isnan(elev))
    assert blocked.any() and clear.any()
    check("fv_w1111_r15_region", got["traversability_footprint"], want, TOL * 3.0)


# ---- fixed point at saturation -----------------------------------------------------------------------------------------------
def saturation_case(capi, oracle, case, geo, kind, over):
    route, k = fv.PLANNED[case]
    rows, cols = fv.GEOS[geo][3:]
    elev = elevation(kind, rows, cols)
    g = oracle.geom(rows, cols, fv.RES, fv.POS)
    op = params(oracle, geo, **over)
    got = run_device(capi, op, elev, rows, cols)
    want = oracle.footprint(g, op, elev, got)
    blocked, clear, nan_in, _, _ = disc_classes(oracle, g, op, elev, got, geo, np.isnan(elev))
    assert blocked.any() and clear.any() and nan_in.any()  # (a blocked disc among saturated cells: the sticky flag, the count field)
    cap = max(op.w_scale * 3.0, op.fp_default)
    if kind == "flat":
        t = got["traversability"]
        assert (t[np.isfinite(t)] == np.float32(op.w_scale * 3.0)).mean() > 0.8  # every score is 1: every cell at the weights' cap
    if route in ("slide4", "slide5"):
        assert k == fv.fp_fixed_k(fv.SAT[geo][0], fv.fixed_cap(op.w_scale * 3.0, op.fp_default), fv.SAT[geo][1])
        bound = 2.0 ** -(k + 1) + 2.0 ** -23 * np.abs(want.astype(np.float64))
    else:
        bound = TOL * max(1.0, cap)
    check(f"{case} ({route}, k = {k})", got["traversability_footprint"], want, bound)


@pytest.mark.parametrize("k", range(23, 15, -1))
@pytest.mark.parametrize("geo", list(fv.SAT))
def test_fixed_point_at_saturation(capi, oracle, geo, k):
    """fv_<geo>_k<k>: the flat map, w_scale the largest float that still gives k (16: the first that does not -- the pass
    leaves the fixed-point route), weights 1 1 1, fp_default at the cap."""
    s = fv.sat_scale(geo, k)
    saturation_case(capi, oracle, f"fv_{geo}_k{k}", geo, "flat", dict(w_scale=s, fp_default=s * 3.0))


@pytest.mark.parametrize("geo", list(fv.SAT))
def test_fixed_point_with_the_default_as_the_cap(capi, oracle, geo):
    """fv_<geo>_defcap: a layer at 0.3, fp_default at the k = 17 cap, unobserved cells."""
    saturation_case(capi, oracle, f"fv_{geo}_defcap", geo, "flat", dict(w_scale=float(np.float32(0.1)), fp_default=fv.sat_scale(geo, 17) * 3.0))


@pytest.mark.parametrize("geo", list(fv.SAT))
def test_fixed_point_on_a_constant_gradient(capi, oracle, geo):
    """fv_<geo>_k17's plan on a plane: every interior cell has the same value, with a fraction at 2^-17 -- the worst
    systematic rounding."""
    s = fv.sat_scale(geo, 17)
    saturation_case(capi, oracle, f"fv_{geo}_k17", geo, "plane", dict(w_scale=s, fp_default=s * 3.0))
