"""The shapes, radii, holes and normal layers of tests/test_gpu_plugin_filters.py and tests/test_plugin_filter_ref.py, kept
apart from them so that tests/test_chain_route.py can check -- without a GPU -- that every case lands on the route it claims.
Routes are named as tests/cpu/chain_route_check.cpp prints them.

Shapes are the smallest at which these kernels can still go wrong: 70 x 37 and 130 x 33 cut workgroups and tiles both ways and
still hold a 16-cell disc; the marches need 64 rows (64 x 40 against 63 x 40); 5 x 7, 3 x 200 and 200 x 3 are narrower than
the disc; 40 x 33 runs as a batch of three maps -- all NaN, the case's map, another terrain with another hole pattern."""
import collections

import numpy as np

RES = 0.05
STEP_TIE_RES = 0.04  # the default 0.04 m step windows are whole cells here
FILTER_STEP, FILTER_ROUGHNESS, FILTER_NORMALS = 2, 3, 5  # TE_FILTER_*
PAST_32 = 33.5  # cells: beyond the discs of te_disc.h, served under TE_OPT_FILTER_ANY_RADIUS only

# cells: the filter's radii in cells (step: both windows; roughness, normals: one).  any_option: TE_OPT_FILTER_ANY_RADIUS.
# route: what plan_filter_route gives -- step: (height pass, score pass); roughness and normals: the normals kernel.
Case = collections.namedtuple("Case", "name filter rows cols batch res cells generic any_option route")


def _step(name, rows, cols, res, r1, r2, route, batch=1, generic=False, any_option=0):
    return Case(name, FILTER_STEP, rows, cols, batch, res, (r1, r2), generic, any_option, route)


def _one(filter_, name, rows, cols, r, route, batch=1, generic=False, any_option=0):
    return Case(name, filter_, rows, cols, batch, RES, (r,), generic, any_option, route)


SMALL, GENERIC = ("k_step_small",) * 2, ("generic",) * 2
STEP = [
    _step("single cell", 70, 37, RES, 0.0, 0.0, SMALL),
    _step("tie 1", 130, 33, STEP_TIE_RES, 1, 1, SMALL),
    _step("tie 2", 70, 37, STEP_TIE_RES, 2, 2, SMALL),
    _step("tie 2 narrow", 5, 7, STEP_TIE_RES, 2, 2, SMALL),
    _step("2.5", 70, 37, RES, 2.5, 2.5, ("march<5>",) * 2),
    _step("5.4", 130, 33, RES, 5.4, 5.4, ("march<29>",) * 2),
    _step("5.4 then 2.5", 70, 37, RES, 5.4, 2.5, ("march<29>", "march<5>")),
    _step("2.5 rows 64", 64, 40, RES, 2.5, 2.5, ("march<5>",) * 2),
    _step("2.5 rows 63", 63, 40, RES, 2.5, 2.5, GENERIC),
    _step("2.5 cols 3", 200, 3, RES, 2.5, 2.5, ("march<5>",) * 2),
    _step("5.4 rows 3", 3, 200, RES, 5.4, 5.4, GENERIC),
    _step("tie 3", 70, 37, STEP_TIE_RES, 3, 3, ("RAW<8>+ties",) * 2),
    _step("tie 5", 130, 33, STEP_TIE_RES, 5, 5, ("RAW<20>+ties",) * 2),
    _step("tie 3 rows 63", 63, 40, STEP_TIE_RES, 3, 3, GENERIC),
    _step("2.5 generic flag", 70, 37, RES, 2.5, 2.5, GENERIC, generic=True),
    _step("past 32 then 2.5", 70, 70, RES, PAST_32, 2.5, ("any", "march<5>"), any_option=1),
    _step("2.5 batch", 40, 33, RES, 2.5, 2.5, GENERIC, batch=3),
    _step("5.4 batch rows 70", 70, 37, RES, 5.4, 5.4, ("march<29>",) * 2, batch=3),
]

ROUGHNESS = [_one(FILTER_ROUGHNESS, *c) for c in (
    ("3.6", 70, 37, 3.6, "k_normals_slide"),
    ("5.4", 130, 33, 5.4, "k_normals_slide"),
    ("9.2", 64, 40, 9.2, "k_normals_slide"),
    ("5.4 rows 63", 63, 40, 5.4, "k_normals_slide"),
    ("11.3", 70, 37, 11.3, "k_normals_slide<R>"),
    ("16.2", 130, 33, 16.2, "k_normals_slide<R>"),
    ("tie 1", 70, 37, 1, "k_normals"),
    ("tie 2", 130, 33, 2, "k_normals"),
    ("tie 3", 64, 40, 3, "k_normals"),
    ("tie 5", 70, 37, 5, "k_normals"),
    ("3.6 on 5 x 7", 5, 7, 3.6, "k_normals"),
    ("3.6 on 3 x 200", 3, 200, 3.6, "k_normals"),
    ("3.6 on 200 x 3", 200, 3, 3.6, "k_normals"),
)] + [
    _one(FILTER_ROUGHNESS, "5.4 generic flag", 70, 37, 5.4, "k_normals", generic=True),
    _one(FILTER_ROUGHNESS, "past 32", 70, 70, PAST_32, "any", any_option=1),
    _one(FILTER_ROUGHNESS, "3.6 batch", 40, 33, 3.6, "k_normals_slide", batch=3),
    _one(FILTER_ROUGHNESS, "tie 3 batch", 40, 33, 3, "k_normals", batch=3),
]

NORMALS = [_one(FILTER_NORMALS, *c) for c in (
    ("tie 1", 70, 37, 1, "k_normals_small-CROSS"),
    ("5.4", 130, 33, 5.4, "k_normals3-KEEP-dense"),
    ("tie 5", 70, 37, 5, "k_normals3-KEEP-TIES"),
    ("11.3", 70, 37, 11.3, "k_normals_slide<R>"),
    ("tie 5 rows 63", 63, 40, 5, "k_normals"),
)]

ALL = STEP + ROUGHNESS + NORMALS

# the normal layers handed to the roughness plugin
NORMAL_KINDS = ["own",         # the oracle's normals of the same map and radius
                "tilted",      # random unit vectors up to about 30 degrees off z, valid on every cell: also over invalid centres
                "short",       # the same vectors at length 0.5 (the reference does not normalise its input)
                "long",        # ... and at length 2
                "horizontal",  # nz = 0 exactly
                "nan_nx",      # 3 % NaN in surface_normal_x alone: the one layer the reference tests, those cells are NaN
                "nan_ny",      # NaN in surface_normal_y alone under a finite nx: NaN arithmetic, a false comparison, score 0
                "void"]        # tilted normals over a map that is unobserved but for isolated cells: windows of one point (score
#                                0) and of none (score 1), every valid normal but a few over an invalid centre


def case_id(c):
    return "%s-%dx%dx%d" % (c.name.replace(" ", "_"), c.rows, c.cols, c.batch)


def radius(c, k=0):
    return c.cells[k] * c.res


def terrain(rows, cols, seed, amplitude=0.12):
    """Rolling ground with kerbs and a little noise, float32 of shape (cols, rows)."""
    rng = np.random.default_rng(seed)
    j, i = np.mgrid[0:cols, 0:rows].astype(np.float64)
    z = amplitude * (np.sin(i / 7.0 + rng.uniform(0, 6)) + np.cos(j / 5.0 + rng.uniform(0, 6))) + rng.normal(0.0, amplitude / 12.0, (cols, rows))
    for _ in range(3):
        a, b = int(rng.integers(0, cols)), int(rng.integers(0, rows))
        z[a:a + max(2, cols // 5), b:b + max(2, rows // 6)] += rng.uniform(0.08, 0.3)
    return z.astype(np.float32)


def punch(e, seed, pattern="speckle+block"):
    """2 % speckle and one unobserved block (about a sixth of each side); "inf+rows": 4 % invalid cells of all three kinds and
    two unobserved rows.  Returns a copy."""
    rng = np.random.default_rng(seed)
    e = e.copy()
    cols, rows = e.shape
    if pattern == "speckle+block":
        e[rng.random(e.shape) < 0.02] = np.nan
        a, b = cols // 3, rows // 4
        e[a:a + max(1, cols // 6), b:b + max(1, rows // 6)] = np.nan
    elif pattern == "inf+rows":
        bad = rng.random(e.shape)
        e[bad < 0.04] = np.nan
        e[bad < 0.025] = np.inf
        e[bad < 0.0125] = -np.inf
        e[cols // 2:cols // 2 + 2, :] = np.nan
    else:
        raise KeyError(pattern)
    return e


def void(e, R):
    """`e` unobserved but for isolated cells more than R cells apart (as far as the map allows)."""
    cols, rows = e.shape
    out = np.full_like(e, np.nan)
    step = int(R) + 2
    for a in range(cols // 4, cols, 2 * step):
        for b in range(rows // 4, rows, 2 * step):
            out[a, b] = e[a, b]
    return out


def elevation(c, seed=0, kind=None):
    """[batch] flat float32 maps of case c.  A single map is the case's map; of a batch of three, map 0 is all NaN, map 1 is the
    case's map and map 2 another terrain with another hole pattern.  kind "void": see NORMAL_KINDS."""
    base = 1000 * (ALL.index(c) + 1) + 17 * seed
    # (the step filter sees gentle ground between its kerbs: a window of five cells stays below the critical step height there)
    amplitude = 0.02 if c.filter == FILTER_STEP else 0.12
    own = punch(terrain(c.rows, c.cols, base, amplitude), base + 1)
    if kind == "void":
        own = void(terrain(c.rows, c.cols, base, amplitude), np.ceil(max(c.cells)))
    if c.batch == 1:
        return [own.reshape(-1)]
    assert c.batch == 3
    other = punch(terrain(c.rows, c.cols, base + 2, amplitude=1.5 * amplitude), base + 3, "inf+rows")
    return [np.full(c.rows * c.cols, np.nan, np.float32), own.reshape(-1), other.reshape(-1)]


def tilted(n, rng):
    v = rng.normal(size=(n, 3)) * np.array([0.25, 0.25, 0.0]) + np.array([0.0, 0.0, 1.0])
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    return [np.ascontiguousarray(v[:, k], dtype=np.float32) for k in range(3)]


def normals(kind, elev, own, seed):
    """(nx, ny, nz) of kind `kind` for one flat map; own: the oracle's normals of it (a callable, asked only for "own").  An
    all-NaN map gets all-NaN normals whatever the kind."""
    n = elev.size
    if not np.isfinite(elev).any():
        return [np.full(n, np.nan, np.float32) for _ in range(3)]
    rng = np.random.default_rng(seed)
    if kind == "own":
        return [np.array(a, np.float32) for a in own()]
    nx, ny, nz = tilted(n, rng)
    if kind == "short":
        nx, ny, nz = nx * np.float32(0.5), ny * np.float32(0.5), nz * np.float32(0.5)
    elif kind == "long":
        nx, ny, nz = nx * np.float32(2), ny * np.float32(2), nz * np.float32(2)
    elif kind == "horizontal":
        t = rng.uniform(0.0, 2.0 * np.pi, n)
        nx, ny, nz = np.cos(t).astype(np.float32), np.sin(t).astype(np.float32), np.zeros(n, np.float32)
    elif kind == "nan_nx":
        nx[rng.random(n) < 0.03] = np.nan
    elif kind == "nan_ny":
        ny[rng.random(n) < 0.03] = np.nan
    elif kind not in ("tilted", "void"):
        raise KeyError(kind)
    return [nx, ny, nz]


SLOPE_SHAPE = (70, 37)
SLOPE_BATCH_SHAPE = (40, 33)


def slope_values(crit):
    """surface_normal_z values no chain would write beside the ones it does: the ends of acos' domain and just beyond, zeros of
    both signs and a denormal, cos(crit) as float32 with its two neighbours, and the non-finite ones."""
    one, c = np.float32(1), np.float32(np.cos(crit))
    up, down = np.float32(np.inf), np.float32(-np.inf)
    return np.array([1.0, np.nextafter(one, np.float32(0)), np.nextafter(one, np.float32(2)), 2.0, -1.0, np.nextafter(-one, np.float32(-2)),
                     0.0, -0.0, 1e-40, c, np.nextafter(c, up), np.nextafter(c, down), np.nan, np.inf, -np.inf], np.float32)


def slope_layers(crit):
    """{name: (rows, cols, [flat maps])}: the value table repeated across a layer, a random layer over [-1, 1], and a batch of
    three -- the table (from another phase), random values, all NaN."""
    table = slope_values(crit)
    rows, cols = SLOPE_SHAPE
    rng = np.random.default_rng(4242)
    rb, cb = SLOPE_BATCH_SHAPE
    return {"table": (rows, cols, [np.resize(table, rows * cols)]),
            "random": (rows, cols, [rng.uniform(-1.0, 1.0, rows * cols).astype(np.float32)]),
            "batch": (rb, cb, [np.resize(np.roll(table, 4), rb * cb), rng.uniform(-1.0, 1.0, rb * cb).astype(np.float32),
                               np.full(rb * cb, np.nan, np.float32)])}


def hole_facts(maps):
    """(share of invalid cells, clustered) of the uploaded batch as the upload counts them: runs in memory order; clustered when
    the runs average 8 cells or more."""
    bad = ~np.isfinite(np.concatenate([np.asarray(m).reshape(-1) for m in maps]))
    invalid = int(bad.sum())
    runs = int(bad[0]) + int((bad[1:] & ~bad[:-1]).sum())
    return invalid / bad.size, invalid > 0 and runs * 8 <= invalid


def route_line(c):
    """The case as tests/cpu/chain_route_check.cpp's `filter` mode reads it: rows cols batch res filter radius-cells (two numbers;
    the second is the step filter's second window, otherwise unused) generic any hole-share clustered."""
    share, clustered = hole_facts(elevation(c))
    return "%d %d %d %r %d %r %r %d %d %r %d" % (c.rows, c.cols, c.batch, c.res, c.filter, float(c.cells[0]), float(c.cells[-1]), c.generic,
                                                 c.any_option == 2, share, clustered)


def route_words(c):
    return " ".join(c.route) if c.filter == FILTER_STEP else c.route
