"""The case table of tests/test_gpu_beside_prefetch.py: one row for every entry point that takes the context's lock with
`beside_prefetch = true` (csrc/te_ctx.h: CtxLock) and touches a layer -- how it is called through capi.Context, the layers it
reads, the layers it writes and what shows its result.  tests/test_beside_prefetch_table.py scans csrc/*.hip for those lock
constructions and holds the table complete: a new entry point that runs beside a prefetch fails there until it has a row.

Shape: one map of 1536 x 1200 cells at 0.05 m, 7.03 MiB a layer -- above HostStager::kMinBytes = 4 MiB (csrc/te_internal.h;
csrc/te_stage.hip: `bytes < kMinBytes` takes the plain hipMemcpyAsync), so every whole-layer transfer is staged in chunks of
kChunk = 8 MiB through the page-locked ring, the path a prefetch takes on its own thread.  te_prefetch_layers takes at most 8
layers; every prefetch here sends 8.

Layers are named as capi names them; u0 .. u15 are the sixteen user layers every context of these tests adds first, so that
their ids are 15 .. 30 in every context (u15: id 30, the top bit the 32-bit masks use).
"""
import zlib

import numpy as np

ROWS, COLS, RES = 1536, 1200, 0.05
LAYER_BYTES = ROWS * COLS * 4
STAGING_THRESHOLD_BYTES = 4 << 20  # HostStager::kMinBytes
assert LAYER_BYTES > STAGING_THRESHOLD_BYTES
N_PREFETCH = 8                     # te_prefetch_layers: n <= 8
USER = ["u%d" % k for k in range(16)]
TOP_USER, TOP_USER_ID = "u15", 30
RECT = (37, 53, 1001, 777)         # row0, col0, h, w of every region form: odd origin, no multiple of a tile, most of the map

E, SL, ST, RO, T = "elevation", "traversability_slope", "traversability_step", "traversability_roughness", "traversability"
NX, NY, NZ, RS = "surface_normal_x", "surface_normal_y", "surface_normal_z", "robot_slope"


def std_dev(x):
    """the nested standard deviation of tests/window_expression_cases.py over the window of layer `x` (a window expression names its input layer)"""
    return f"sqrt(sumOfFinites(square({x} - meanOfFinites({x}))) ./ numberOfFinites({x}))"


# entry points that run beside a prefetch and touch no layer: no row
NO_LAYER = {
    "te_set_params": "writes the context's parameters and tables, no layer",
    "te_get_params": "reads the context's parameters, no layer",
    "te_add_layer": "a new name has no memory yet: it touches no layer",
    "te_layer_id": "looks a name up in the table of user names",
    "te_layer_name": "looks an id up in the table of user names",
}


def params(capi):
    """Windows of three and two cells (at the defaults a 0.05 m map has single-cell step windows: the step layer is 1 wherever
    the elevation is valid, whatever the elevation) and critical values the inputs below stay under, so that no score saturates."""
    from traversability_estimation_amd import synth
    r3, r2 = synth.benchmark_radius(3, RES), synth.benchmark_radius(2, RES)
    return capi.default_params(normals_radius=r3, rough_radius=r3, step_radius1=r3, step_radius2=r2, slope_critical=1.0, rough_critical=0.5)


_content = {}
SMALL = (160, 120)  # rows, cols: the shape tests/test_beside_prefetch_table.py checks the OLD / NEW preconditions at on the CPU


def start_of(shape):
    """te_run_reachable's start cell (row, col) on a map of `shape`"""
    return (shape[0] // 2, shape[1] // 2)


def content(kind, layer, seed, shape=(ROWS, COLS)):
    """The (cols, rows) float32 contents of `layer`: value kind `kind`, OLD and NEW differing in `seed` alone.  Cached, never
    written to.  shape: (rows, cols), the GPU tests' by default."""
    key = (kind, layer, seed, tuple(shape))
    if key not in _content:
        a = _make(kind, zlib.crc32(layer.encode()) % 100000 * 10 + seed, seed, *shape)
        a.setflags(write=False)
        _content[key] = a
    return _content[key]


def _ring(a, start, half, thick=2):
    """a NaN wall around the start cell: the box a reachable call cannot leave"""
    r, c = start
    a[c - half:c + half + 1, r - half:r - half + thick] = np.nan
    a[c - half:c + half + 1, r + half - thick + 1:r + half + 1] = np.nan
    a[c - half:c - half + thick, r - half:r + half + 1] = np.nan
    a[c + half - thick + 1:c + half + 1, r - half:r + half + 1] = np.nan


def _make(kind, s, seed, rows, cols):
    from traversability_estimation_amd import synth
    rng = np.random.default_rng(s)
    fr, fc = rows / ROWS, cols / COLS  # (the blocks below are placed on the GPU tests' shape and scaled to any other)
    if kind == "noise":       # uniform in [0, 1), cell by cell independent: fillers, thresholds, scores
        return rng.random((cols, rows), dtype=np.float32)
    if kind == "normal_z":    # acos of it stays under slope_critical
        return (np.float32(0.6) + np.float32(0.4) * rng.random((cols, rows), dtype=np.float32)).astype(np.float32)
    if kind == "normal_xy":   # near-vertical normals: the roughness stays far from its critical value
        return (np.float32(0.1) * (rng.random((cols, rows), dtype=np.float32) - np.float32(0.5))).astype(np.float32)
    if kind == "stepped":
        # StepFilter's score is 1 where no cell of the second window steps more than step_critical (0.12 m) and 0 where four do:
        # nearly two-valued.  An odd seed is flat ground (1 almost everywhere), an even one steep (0 almost everywhere).
        return np.ascontiguousarray(synth.perlin_elevation(rows, cols, seed=s, amplitude=0.02 if seed % 2 else 6.0), np.float32)
    t = synth.with_steps(synth.perlin_elevation(rows, cols, seed=s, amplitude=0.12), 8, seed=s + 7)
    if kind == "terrain":
        return np.ascontiguousarray(t, np.float32)
    if kind == "holed":       # median fill, cloud: invalid cells, scattered and in a block
        t = synth.with_holes(t, 0.01, seed=s + 1)
        t[int((100 + 10 * seed) * fc):int((140 + 10 * seed) * fc), int(300 * fr):int(380 * fr)] = np.nan
    elif kind == "seeds":     # distance with NaN seeds: about 11 cells to the nearest one
        t = synth.with_holes(t, 0.002, seed=s + 1)
        t[int((500 + 100 * seed) * fc):int((520 + 100 * seed) * fc), int(700 * fr):int(760 * fr)] = np.nan
    elif kind == "blocked":   # components: the free cells are one large component whose size differs with the seed
        t = synth.with_holes(t, 0.03 + 0.02 * seed, seed=s + 1)
    elif kind == "walled":    # reachable: scattered blocked cells, and under an even seed a wall around the start cell
        t = synth.with_holes(t, 0.02, seed=s + 1)
        r, c = start_of((rows, cols))
        t[c - 3:c + 4, r - 3:r + 4] = 0.0
        if seed % 2 == 0:
            _ring(t, (r, c), max(6, int(20 * min(fr, fc))))
    else:
        raise KeyError(kind)
    return np.ascontiguousarray(t, np.float32)


class Row:
    """name: the test id.  entry: the exported te_* name.  call(ctx, capi): makes the call; a read-only row returns what it
    downloaded (an array, bytes, or a list of them), a writing row returns None (a region form returns the rectangle it wrote:
    `and None`) and its result is the download of `writes`.
    reads / writes: the layers the call's contract names (travgpu.h).  may_write: layers the call may use as scratch (never
    prefetched beside it as bystanders, never compared).  kinds: the value kind of a read layer (default "noise").  base: layers
    that hold fixed contents before the call -- the output of a region form outside its rectangle.  region: the row writes RECT
    (grown by the call's reach) only.  options: te_set_option pairs set on every context of the row.  tol: compared with
    assert_layers_match at its default tolerance (te_run_filter, as the issue asks) instead of bit for bit.  long_call: the
    call is the slowest the library has (situation 4).  fill_mask: the call leaves a fill mask (situation 3)."""

    def __init__(self, name, entry, call, reads=(), writes=(), may_write=(), kinds=None, base=(), region=False, options=(), tol=False, long_call=False,
                 fill_mask=False, result_is_layer=True):
        self.name, self.entry, self.call = name, entry, call
        self.reads, self.writes, self.may_write = tuple(reads), tuple(writes), tuple(may_write)
        self.kinds = dict(kinds or {})
        self.base, self.region, self.options, self.tol = tuple(base), region, tuple(options), tol
        self.long_call, self.fill_mask = long_call, fill_mask
        self.result_is_layer = result_is_layer  # (a read-only row whose result is one whole layer in [cols][rows] order)

    @property
    def touches(self):
        return tuple(dict.fromkeys(self.reads + self.writes + self.may_write + self.base))

    def kind(self, layer):
        return self.kinds.get(layer, "noise")


def _fill(capi, **over):
    return capi.default_median_fill_params(**over)


def _win(capi, w):
    return capi.window_expr_params(window_size=w)


def _submap_args():
    # a request of about 60 % of each side around a point off the centre
    return (3.1, -2.3), (0.6 * ROWS * RES, 0.6 * COLS * RES)


def _msg_info(capi):
    return capi.TeMsgInfo()


def _removed(ctx, capi, layer):
    """te_remove_layer, then what shows it: the id comes back for a new name, without contents."""
    lid = ctx.layer_id(layer)
    ctx.remove_layer(layer)
    again = ctx.add_layer("again")
    try:
        ctx.download("again")
        code = 0
    except capi.TeError as e:
        code = e.code
    assert again == lid and code == capi.TE_ERR_NOT_READY, (lid, again, code)
    return np.array([lid, again, code], np.int32)


CUT = ("lower", 0.6, 0.25)  # ThresholdFilter on "noise": six cells in ten are replaced
D_ARGS = ("below", -10.0, 40.5 * RES)  # te_run_distance: no value is a seed, every NaN is (nan_is_seed); the cap reaches 40 cells
C_ARGS = ("below", -10.0)             # te_run_components / te_run_reachable: blocked = NaN

ROWS_TABLE = [
    # ---- te_run_filter: the five plugins, the normals once more under the raster method ----
    Row("filter-slope", "te_run_filter", lambda c, k: c.run_filter("slope"), reads=(NZ,), writes=(SL,), kinds={NZ: "normal_z"}, tol=True),
    Row("filter-step", "te_run_filter", lambda c, k: c.run_filter("step"), reads=(E,), writes=(ST,), kinds={E: "stepped"}, tol=True),
    Row("filter-roughness", "te_run_filter", lambda c, k: c.run_filter("roughness"), reads=(E, NX, NY, NZ), writes=(RO,),
        kinds={E: "terrain", NX: "normal_xy", NY: "normal_xy", NZ: "normal_z"}, tol=True),
    Row("filter-combine", "te_run_filter", lambda c, k: c.run_filter("combine"), reads=(SL, ST, RO), writes=(T,), tol=True),
    Row("filter-normals", "te_run_filter", lambda c, k: c.run_filter("normals"), reads=(E,), writes=(NX, NY, NZ), may_write=(SL, RO), kinds={E: "terrain"}, tol=True),
    Row("filter-normals-raster", "te_run_filter", lambda c, k: c.run_filter("normals"), reads=(E,), writes=(NX, NY, NZ), may_write=(SL, RO), kinds={E: "terrain"},
        options=(("OPT_NORMALS_ALGORITHM", 1),), tol=True),
    # ---- median fill ----
    Row("median-fill", "te_run_median_fill", lambda c, k: c.run_median_fill(_fill(k), RS, "u1"), reads=(RS,), writes=("u1",), kinds={RS: "holed"}, fill_mask=True),
    Row("median-fill-in-place", "te_run_median_fill", lambda c, k: c.run_median_fill(_fill(k, filter_existing_values=1, existing_value_radius=0.05), "u2", "u2"),
        reads=("u2",), writes=("u2",), kinds={"u2": "holed"}, fill_mask=True),
    Row("median-fill-region", "te_run_median_fill_region", lambda c, k: c.run_median_fill_region(_fill(k, filter_existing_values=1, existing_value_radius=0.05), RS, ST, 0, *RECT) and None,
        reads=(RS,), writes=(ST,), kinds={RS: "holed"}, base=(ST,), region=True),
    # ---- mean / minimum in a radius ----
    Row("radius-mean", "te_run_radius_filter", lambda c, k: c.run_radius_filter("mean", 0.16, "u0", RO), reads=("u0",), writes=(RO,)),
    Row("radius-min-in-place", "te_run_radius_filter", lambda c, k: c.run_radius_filter("min", 0.11, SL, SL), reads=(SL,), writes=(SL,)),
    Row("radius-mean-region", "te_run_radius_filter_region", lambda c, k: c.run_radius_filter_region("mean", 0.16, ST, "u3", 0, *RECT) and None,
        reads=(ST,), writes=("u3",), base=("u3",), region=True),
    # ---- window expressions ----
    Row("window-mean5", "te_run_window_expression", lambda c, k: c.run_window_expression(f"meanOfFinites({RO})", _win(k, 5), RO, T), reads=(RO,), writes=(T,)),
    Row("window-range3-in-place", "te_run_window_expression", lambda c, k: c.run_window_expression("maxOfFinites(u4) - minOfFinites(u4)", _win(k, 3), "u4", "u4"),
        reads=("u4",), writes=("u4",)),
    Row("window-std21-reader", "te_run_window_expression", lambda c, k: c.run_window_expression(std_dev(ST), _win(k, 21), ST, "u5"), reads=(ST,), writes=("u5",),
        long_call=True),
    Row("window-std21-writer", "te_run_window_expression", lambda c, k: c.run_window_expression(std_dev("u6"), _win(k, 21), "u6", SL), reads=("u6",), writes=(SL,),
        long_call=True),
    Row("window-mean5-region", "te_run_window_expression_region", lambda c, k: c.run_window_expression_region(f"meanOfFinites({T})", _win(k, 5), T, RO, 0, *RECT) and None,
        reads=(T,), writes=(RO,), base=(RO,), region=True),
    # ---- distance ----
    Row("distance", "te_run_distance", lambda c, k: c.run_distance(*D_ARGS, T, "u7", nan_is_seed=True), reads=(T,), writes=("u7",), kinds={T: "seeds"}),
    Row("distance-in-place", "te_run_distance", lambda c, k: c.run_distance(*D_ARGS, RO, RO, nan_is_seed=True), reads=(RO,), writes=(RO,), kinds={RO: "seeds"}),
    Row("distance-region", "te_run_distance_region", lambda c, k: c.run_distance_region(*D_ARGS, "u8", ST, 0, *RECT, nan_is_seed=True) and None, reads=("u8",), writes=(ST,),
        kinds={"u8": "seeds"}, base=(ST,), region=True),
    # ---- connected regions ----
    Row("components", "te_run_components", lambda c, k: c.run_components(*C_ARGS, 4, T, SL, nan_is_seed=True), reads=(T,), writes=(SL,), kinds={T: "blocked"}),
    Row("components-in-place-top-user", "te_run_components", lambda c, k: c.run_components(*C_ARGS, 8, TOP_USER, TOP_USER, nan_is_seed=True),
        reads=(TOP_USER,), writes=(TOP_USER,), kinds={TOP_USER: "blocked"}),
    Row("reachable", "te_run_reachable", lambda c, k: c.run_reachable(*C_ARGS, [start_of((ROWS, COLS))], 4, RS, "u9", nan_is_seed=True), reads=(RS,), writes=("u9",),
        kinds={RS: "walled"}),
    # ---- expressions ----
    Row("expression", "te_run_expression", lambda c, k: c.run_expression(f"0.5 * {SL} + {RO} .* {RO}"), reads=(SL, RO), writes=(T,)),
    Row("expression-region", "te_run_expression_region", lambda c, k: c.run_expression_region(f"{ST} - 2 * {RS}", 0, *RECT), reads=(ST, RS), writes=(T,),
        base=(T,), region=True),
    Row("layer-expression-user-in-user-out", "te_run_layer_expression", lambda c, k: c.run_layer_expression(f"u10 .* {SL} + 1", "u11"), reads=("u10", SL),
        writes=("u11",)),
    Row("layer-expression-top-user-in", "te_run_layer_expression", lambda c, k: c.run_layer_expression(f"sqrt({TOP_USER}) + {ST}", RO), reads=(TOP_USER, ST),
        writes=(RO,)),
    Row("layer-expression-in-place", "te_run_layer_expression", lambda c, k: c.run_layer_expression(f"{SL} .* {SL} + {ST}", SL), reads=(SL, ST), writes=(SL,)),
    Row("layer-expression-thresholds", "te_run_layer_expression_thresholds", lambda c, k: c.run_layer_expression(f"{RO} + u12", TOP_USER, [("upper", 1.2, 2.0)]),
        reads=(RO, "u12"), writes=(TOP_USER,)),
    Row("layer-expression-region", "te_run_layer_expression_region", lambda c, k: c.run_layer_expression_region(f"2 * u13 - {SL}", ST, 0, *RECT),
        reads=("u13", SL), writes=(ST,), base=(ST,), region=True),
    Row("layer-expression-thresholds-region", "te_run_layer_expression_thresholds_region",
        lambda c, k: c.run_layer_expression_region(f"{T} + {RO}", "u14", 0, *RECT, thresholds=[("lower", 0.5, -1.0)]), reads=(T, RO), writes=("u14",),
        base=("u14",), region=True),
    # ---- ThresholdFilter, DuplicationFilter ----
    Row("threshold", "te_run_threshold", lambda c, k: c.run_threshold(RO, *CUT), reads=(RO,), writes=(RO,)),
    Row("threshold-top-user", "te_run_threshold", lambda c, k: c.run_threshold(TOP_USER, *CUT), reads=(TOP_USER,), writes=(TOP_USER,)),
    Row("threshold-region", "te_run_threshold_region", lambda c, k: c.run_threshold_region(ST, *CUT, 0, *RECT), reads=(ST,), writes=(ST,), region=True),
    Row("copy-layer", "te_copy_layer", lambda c, k: c.copy_layer(SL, "u1"), reads=(SL,), writes=("u1",)),
    Row("copy-layer-from-user", "te_copy_layer", lambda c, k: c.copy_layer("u2", T), reads=("u2",), writes=(T,)),
    # ---- read-only rows: downloads (several layers: one record per cell, so that a change of one layer changes every record;
    # a serialised message holds one layer) ----
    Row("download", "te_download_layer", lambda c, k: c.download(ST), reads=(ST,)),
    Row("download-top-user", "te_download_layer", lambda c, k: c.download(TOP_USER), reads=(TOP_USER,)),
    Row("download-circular", "te_download_layer_circular", lambda c, k: c.download_layer_circular(RO, (5, 3)), reads=(RO,), result_is_layer=False),
    # (te_download_msg takes the plain lock for the geometry before its helper takes the one beside a prefetch: it always joins,
    # so this row cannot expose a mask; it is here because the scan finds the helper)
    Row("download-msg", "te_download_msg", lambda c, k: c.download_msg(_msg_info(k), {"a": "u3"}), reads=("u3",), result_is_layer=False),
    Row("occupancy", "te_download_occupancy", lambda c, k: np.ascontiguousarray(c.download_occupancy([T, "u4"], 0.0, 1.0).T), reads=(T, "u4"), result_is_layer=False),
    Row("occupancy-msg", "te_download_occupancy_msg", lambda c, k: c.download_occupancy_msg(_msg_info(k), RO, 0.0, 1.0), reads=(RO,), result_is_layer=False),
    Row("cloud", "te_download_cloud", lambda c, k: c.download_cloud([RS, T], RS).copy(), reads=(RS, T), kinds={RS: "holed", T: "holed"}, result_is_layer=False),
    Row("cloud-msg", "te_download_cloud_msg", lambda c, k: c.download_cloud_msg(_msg_info(k), {"z": "u5"}, "u5"), reads=("u5",),
        kinds={"u5": "holed"}, result_is_layer=False),
    Row("submap", "te_download_submap", lambda c, k: np.stack(list(c.download_submap(*_submap_args(), [SL, "u6"])[1].values()), -1).reshape(-1, 2), reads=(SL, "u6"),
        result_is_layer=False),
    Row("submap-msg", "te_download_submap_msg", lambda c, k: c.download_submap_msg(_msg_info(k), *_submap_args(), {"a": RO})[1], reads=(RO,), result_is_layer=False),
    # ---- te_remove_layer: the layer's memory is released, which a prefetch into it must not outlive.  What this row holds: the
    # call succeeds beside a prefetch of its layer and of others, the id comes back empty, the bystanders arrive whole.  What it
    # cannot see: a missed join is a write into released memory, which no download shows. ----
    Row("remove-layer", "te_remove_layer", lambda c, k: _removed(c, k, "u7"), writes=("u7",), result_is_layer=False),
]

BY_NAME = {r.name: r for r in ROWS_TABLE}
assert len(BY_NAME) == len(ROWS_TABLE)


def entries():
    return {r.entry for r in ROWS_TABLE}
