"""te_run_distance on the device, through capi, against its definition as a brute-force loop (tests/ref_py/distance_ref.py).  The
layer is defined bit for bit, so every comparison is array_equal on the bit patterns and no tolerance is involved anywhere, on
both routes of the second pass (TE_OPT_DISTANCE_ROUTE 1: tiled wherever it fits, 2: the route of any reach);
te_distance_stats shows which one ran.  Shapes, caps and inputs: tests/distance_cases.py (tests/test_distance_plan.py checks on
the CPU that each of them takes the route claimed here).  The wavefront's bookkeeping in pass 1 -- halos of several chunks, a
mask per lane, the search behind the segment -- has no check outside the GPU: the tall cases and the tall region cases below
are that check (DESIGN.md section 4.11 lists them)."""
import numpy as np
import pytest

from tests import distance_cases as K
from tests.ref_py import distance_ref as D
from tests.ref_py import expression_ref as E
from tests.ref_py import pointwise_ref as P

pytestmark = pytest.mark.gpu

IN, OUT = "traversability", "traversability_roughness"
MARK = np.float32(-77.25)
CLAIMS = {(r, c, reach, opt): claim for (r, c, reach, opt, claim) in K.ROUTE_CLAIMS}


@pytest.fixture(scope="module")
def capi():
    from traversability_estimation_amd import build, capi
    build.build_lib()
    return capi


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def to_device(maps):
    return np.ascontiguousarray(np.stack([m.T for m in maps]), np.float32).reshape(-1)


def from_device(flat, batch, rows, cols):
    return flat.reshape(batch, cols, rows).transpose(0, 2, 1)


_MAPS, _D2 = {}, {}


def maps_of(rows, cols):
    if (rows, cols) not in _MAPS:
        _MAPS[(rows, cols)] = K.maps(rows, cols, 1000 * rows + cols)
    return _MAPS[(rows, cols)]


def squared(maps, mode):
    """[batch] d2 of every cell; computed once per input and mode, never changed (the cap does not enter)."""
    key = (tuple(m.tobytes() for m in maps), maps[0].shape, mode)
    if key not in _D2:
        d2 = [D.squared_cells(D.seeds(m, mode, K.THRESHOLD)) for m in maps]
        for a in d2:
            a.setflags(write=False)
        _D2[key] = d2
    return _D2[key]


def reference(maps, mode, max_distance):
    return np.stack([D.from_squared(d2, max_distance, K.RES) for d2 in squared(maps, mode)])


_D2_ONE = {}


def squared_of(a, mode, threshold=K.THRESHOLD):
    """d2 of every cell of one map: computed once per set of seeds (the modes of a designed map share theirs), the short axis
    first (the definition is symmetric in the axes, and its loop runs over the first one), never changed."""
    seed = D.seeds(a, mode, threshold)
    key = (seed.shape, seed.tobytes())
    if key not in _D2_ONE:
        d2 = np.ascontiguousarray(D.squared_cells(seed.T).T) if seed.shape[0] > seed.shape[1] else D.squared_cells(seed)
        d2.setflags(write=False)
        _D2_ONE[key] = d2
    return _D2_ONE[key]


def definition(maps, mode, max_distance, threshold=K.THRESHOLD, res=K.RES):
    return np.stack([D.from_squared(squared_of(a, mode, threshold), max_distance, res) for a in maps])


def context(capi, rows, cols, batch, maps=None, route=0, res=K.RES):
    ctx = capi.Context(0)
    ctx.set_params(capi.default_params())
    ctx.set_geometry(rows, cols, batch, res)
    ctx.set_option(capi.OPT_DISTANCE_ROUTE, route)
    if maps is not None:
        ctx.upload_layer(IN, to_device(maps))
    return ctx


def differing(got, want):
    bad = np.argwhere(bits(got) != bits(want))
    return [(tuple(int(v) for v in b), float(got[tuple(b)]), float(want[tuple(b)])) for b in bad[:6]], len(bad)


@pytest.mark.parametrize("mode", K.MODES)
@pytest.mark.parametrize("rows,cols", K.SHAPES)
def test_every_cell_on_both_routes(capi, rows, cols, mode):
    maps = maps_of(rows, cols)
    assert not D.seeds(maps[-1], K.BELOW, K.THRESHOLD).any()  # one map of the batch is empty under BELOW
    for route in (1, 2):
        with context(capi, rows, cols, K.BATCH, maps, route) as ctx:
            for reach in K.REACHES + [K.ABOVE_THE_DIAGONAL]:
                md = K.cap_for(reach)
                want = reference(maps, mode, md)
                ctx.run_distance(mode, K.THRESHOLD, md, IN, OUT)
                got = from_device(ctx.download(OUT), K.BATCH, rows, cols)
                first, n = differing(got, want)
                assert n == 0, f"mode {mode} route {route} {(rows, cols)} reach {reach}: {n} cells differ, (map, i, j), got, want: {first}"
                assert not np.isnan(got).any()
                tiled, any_reach = ctx.distance_stats()
                blocks = K.BATCH * -(-rows // 64) * -(-cols // 64)
                assert (tiled, any_reach) == ((blocks, 0) if CLAIMS[(rows, cols, reach, route)] == "tiled" else (0, blocks)), (reach, route)
            ctx.run_distance(mode, K.THRESHOLD, md, IN, OUT)  # a second run: the same bits
            assert np.array_equal(bits(from_device(ctx.download(OUT), K.BATCH, rows, cols)), bits(want))
            # the input is as it was
            assert np.array_equal(bits(from_device(ctx.download(IN), K.BATCH, rows, cols)), bits(np.stack(maps)))
    if mode == K.BELOW:  # the map without a seed holds the cap everywhere
        assert (reference(maps, mode, K.cap_for(3))[-1] == np.float32(K.cap_for(3))).all()


@pytest.mark.parametrize("route", (1, 2))
def test_in_place_user_layers_and_batch_sub_ranges(capi, route):
    rows, cols = 70, 37
    maps = maps_of(rows, cols)
    for reach in (3, 40):
        md, mode = K.cap_for(reach), K.BELOW | K.NAN_IS_SEED
        want = reference(maps, mode, md)
        with context(capi, rows, cols, K.BATCH, maps, route) as ctx:
            # a user layer as output, then as input
            ctx.add_layer("clearance"), ctx.add_layer("raw")
            ctx.run_distance(mode, K.THRESHOLD, md, IN, "clearance")
            assert np.array_equal(bits(from_device(ctx.download("clearance"), K.BATCH, rows, cols)), bits(want))
            ctx.upload_layer("raw", to_device(maps))
            ctx.run_distance("below", K.THRESHOLD, md, "raw", OUT, nan_is_seed=True)
            assert np.array_equal(bits(from_device(ctx.download(OUT), K.BATCH, rows, cols)), bits(want))
            # in place equals out of place
            ctx.run_distance(mode, K.THRESHOLD, md, "raw")
            assert np.array_equal(bits(from_device(ctx.download("raw"), K.BATCH, rows, cols)), bits(want))
            # one map of the batch: the others of out_layer are left alone
            ctx.upload_layer(OUT, np.full(K.BATCH * rows * cols, MARK, np.float32))
            ctx.run_distance(mode, K.THRESHOLD, md, IN, OUT, map0=1, nmaps=1)
            got = from_device(ctx.download(OUT), K.BATCH, rows, cols)
            assert np.array_equal(bits(got[1]), bits(want[1])) and (got[0] == MARK).all() and (got[2] == MARK).all()
            assert ctx.distance_stats()[0 if CLAIMS[(rows, cols, reach, route)] == "tiled" else 1] == 2 * 1


@pytest.mark.parametrize("route", (1, 2))
@pytest.mark.parametrize("reach", K.REGION_REACHES)
def test_region_equals_the_whole_map_call(capi, route, reach):
    rows, cols = K.REGION_SHAPE
    maps = maps_of(rows, cols)
    md, mode, m = K.cap_for(reach), K.BELOW, 1
    rng = np.random.default_rng(reach)
    with context(capi, rows, cols, K.BATCH, maps, route) as ctx, context(capi, rows, cols, K.BATCH, None, route) as fresh:
        ctx.run_distance(mode, K.THRESHOLD, md, IN, OUT)
        now = [a.copy() for a in maps]
        for (r0, c0, h, w) in K.rects(rows, cols):
            # new seeds and new free cells inside the rectangle only
            tile = np.where(rng.random((h, w)) < 0.3, np.float32(0.1), np.float32(0.9)).astype(np.float32)
            now[m][r0:r0 + h, c0:c0 + w] = tile
            ctx.upload_layer_tile(IN, np.ascontiguousarray(tile.T), m, r0, c0)
            i0, j0, i1, j1 = max(0, r0 - reach), max(0, c0 - reach), min(rows, r0 + h + reach), min(cols, c0 + w + reach)
            before = from_device(ctx.download(OUT), K.BATCH, rows, cols).copy()
            poisoned = before.copy()
            outside = np.ones((rows, cols), bool)
            outside[i0:i1, j0:j1] = False
            # (a cell outside out_rect holds a marker: the call must not write it, not even its old value)
            poisoned[m][outside] = MARK
            ctx.upload_layer(OUT, to_device(list(poisoned)))
            rect = ctx.run_distance_region(mode, K.THRESHOLD, md, IN, OUT, m, r0, c0, h, w)
            assert rect == (i0, j0, i1 - i0, j1 - j0), (rect, (r0, c0, h, w))
            got = from_device(ctx.download(OUT), K.BATCH, rows, cols).copy()
            assert (got[m][outside] == MARK).all(), (r0, c0, h, w)
            blocks = -(-(i1 - i0) // 64) * -(-(j1 - j0) // 64)
            assert ctx.distance_stats() == ((blocks, 0) if route == 1 else (0, blocks))
            got[m][outside] = before[m][outside]
            ctx.upload_layer(OUT, to_device(list(got)))
            # the whole layer equals a fresh whole-map call, and that equals the definition
            fresh.upload_layer(IN, to_device(now))
            fresh.run_distance(mode, K.THRESHOLD, md, IN, OUT)
            whole = from_device(fresh.download(OUT), K.BATCH, rows, cols)
            first, n = differing(got, whole)
            assert n == 0, f"route {route} reach {reach} rectangle {(r0, c0, h, w)}: {n} cells differ: {first}"
        assert np.array_equal(bits(whole), bits(np.stack([D.distance(a, mode, K.THRESHOLD, md, K.RES) for a in now])))


@pytest.mark.parametrize("mode", K.MODES)
@pytest.mark.parametrize("rows,cols,reach,opt,claim,lds,seg_chunks,p1_segs", K.TALL_CASES)
def test_every_cell_of_the_tall_cases(capi, rows, cols, reach, opt, claim, lds, seg_chunks, p1_segs, mode):
    """Several segments per column, halos of several chunks, a mask in every lane, the tile at the LDS limit and the route by plan
    on either side of its reach (tests/distance_cases.py: TALL_CASES), under the option the case names."""
    md = K.cap_for(reach)
    blocks = K.BATCH * -(-rows // 64) * -(-cols // 64)
    with context(capi, rows, cols, K.BATCH, None, opt) as ctx:
        for n, maps in enumerate(K.tall_batches(rows, cols, reach, seg_chunks, mode, 1000 * rows + cols)):
            if n == 0:
                assert not D.seeds(maps[-1], K.BELOW, K.THRESHOLD).any()  # one map of the batch is empty under BELOW
            want = definition(maps, mode, md)
            ctx.upload_layer(IN, to_device(maps))
            ctx.run_distance(mode, K.THRESHOLD, md, IN, OUT)
            got = from_device(ctx.download(OUT), K.BATCH, rows, cols)
            first, bad = differing(got, want)
            assert bad == 0, f"mode {mode} option {opt} {(rows, cols)} reach {reach} batch {n}: {bad} cells differ, (map, i, j), got, want: {first}"
            assert not np.isnan(got).any()
            assert ctx.distance_stats() == ((blocks, 0) if claim == "tiled" else (0, blocks)), (reach, opt)
            ctx.run_distance(mode, K.THRESHOLD, md, IN, OUT)  # a second run: the same bits
            assert np.array_equal(bits(from_device(ctx.download(OUT), K.BATCH, rows, cols)), bits(want))
            # the input is as it was
            assert np.array_equal(bits(from_device(ctx.download(IN), K.BATCH, rows, cols)), bits(np.stack(maps)))


def region_tile(rng, h, w):
    """New cells of a rectangle: seeds of either mode, free cells and NaN cells (few of each in a large rectangle, so that the
    definition stays quick)."""
    p = 0.15 if h * w < 1000 else 0.01
    u = rng.random((h, w))
    return np.where(u < p, np.float32(0.1), np.where(u < 2 * p, np.float32(0.9), np.where(u < 3 * p, np.float32(np.nan), np.float32(K.THRESHOLD)))).astype(np.float32)


@pytest.mark.parametrize("mode", K.MODES)
@pytest.mark.parametrize("option", (0, 1))
@pytest.mark.parametrize("name", sorted(K.REGION_TALL))
def test_region_on_a_tall_map_in_every_mode(capi, name, option, mode):
    """The region form where g starts inside a chunk, its pre-halo is cut by `in`, and a region holds more than one segment
    (tests/distance_cases.py: REGION_TALL), on the first and the last map of the batch."""
    case = K.REGION_TALL[name]
    (rows, cols), reach = case["shape"], case["reach"]
    md = K.cap_for(reach)
    tiled = option == 1 or reach <= 64
    rng = np.random.default_rng(reach + mode)
    now = [a.copy() for a in K.region_base(name, mode)]
    with context(capi, rows, cols, K.BATCH, now, option) as ctx, context(capi, rows, cols, K.BATCH, None, option) as fresh:
        ctx.run_distance(mode, K.THRESHOLD, md, IN, OUT)
        for m in (0, K.BATCH - 1):
            for (r0, c0, h, w), _claim in case["rects"]:
                tile = region_tile(rng, h, w)
                now[m][r0:r0 + h, c0:c0 + w] = tile
                ctx.upload_layer_tile(IN, np.ascontiguousarray(tile.T), m, r0, c0)
                i0, j0, i1, j1 = max(0, r0 - reach), max(0, c0 - reach), min(rows, r0 + h + reach), min(cols, c0 + w + reach)
                before = from_device(ctx.download(OUT), K.BATCH, rows, cols).copy()
                poisoned = before.copy()
                outside = np.ones((rows, cols), bool)
                outside[i0:i1, j0:j1] = False
                poisoned[m][outside] = MARK  # (the call must not write a cell outside out_rect, not even its old value)
                ctx.upload_layer(OUT, to_device(list(poisoned)))
                rect = ctx.run_distance_region(mode, K.THRESHOLD, md, IN, OUT, m, r0, c0, h, w)
                assert rect == (i0, j0, i1 - i0, j1 - j0), (rect, (r0, c0, h, w))
                got = from_device(ctx.download(OUT), K.BATCH, rows, cols).copy()
                assert (got[m][outside] == MARK).all(), (m, r0, c0, h, w)
                blocks = -(-(i1 - i0) // 64) * -(-(j1 - j0) // 64)
                assert ctx.distance_stats() == ((blocks, 0) if tiled else (0, blocks))
                got[m][outside] = before[m][outside]
                ctx.upload_layer(OUT, to_device(list(got)))
                # the whole layer equals a fresh whole-map call, and that equals the definition
                fresh.upload_layer(IN, to_device(now))
                fresh.run_distance(mode, K.THRESHOLD, md, IN, OUT)
                whole = from_device(fresh.download(OUT), K.BATCH, rows, cols)
                first, bad = differing(got, whole)
                assert bad == 0, f"{name} option {option} mode {mode} map {m} rectangle {(r0, c0, h, w)}: {bad} cells differ: {first}"
            first, bad = differing(whole, definition(now, mode, md))
            assert bad == 0, f"{name} option {option} mode {mode} after map {m}: {bad} cells differ from the definition: {first}"
        assert np.array_equal(bits(from_device(ctx.download(IN), K.BATCH, rows, cols)), bits(np.stack(now)))


@pytest.mark.parametrize("option", (0, 1))
def test_a_region_call_first_sizes_the_scratch(capi, option):
    """On a fresh context the first distance call is a region call: the scratch of pass 1 is sized by the region.  A whole-map call
    grows it; the same region call then reads its g at another column height than the one left behind."""
    case = K.REGION_TALL["A"]
    (rows, cols), reach, mode, m = case["shape"], case["reach"], K.BELOW | K.NAN_IS_SEED, 0
    (r0, c0, h, w), claim = case["rects"][0]
    i0, j0, oh, ow = claim["out"]
    md = K.cap_for(reach)
    now = [a.copy() for a in K.region_base("A", mode)]
    now[m][r0:r0 + h, c0:c0 + w] = region_tile(np.random.default_rng(5), h, w)
    want = definition(now, mode, md)
    outside = np.ones((K.BATCH, rows, cols), bool)
    outside[m, i0:i0 + oh, j0:j0 + ow] = False
    with context(capi, rows, cols, K.BATCH, now, option) as ctx:
        for step in ("region first", "whole map", "region again"):
            if step == "whole map":
                ctx.run_distance(mode, K.THRESHOLD, md, IN, OUT)
                got = from_device(ctx.download(OUT), K.BATCH, rows, cols)
                first, bad = differing(got, want)
            else:
                ctx.upload_layer(OUT, np.full(K.BATCH * rows * cols, MARK, np.float32))
                assert ctx.run_distance_region(mode, K.THRESHOLD, md, IN, OUT, m, r0, c0, h, w) == claim["out"]
                got = from_device(ctx.download(OUT), K.BATCH, rows, cols)
                assert (got[outside] == MARK).all(), step
                first, bad = differing(np.where(outside, want, got), want)
            assert bad == 0, f"{step}, option {option}: {bad} cells differ from the definition: {first}"


@pytest.mark.parametrize("route", (1, 2))
def test_values_at_the_edges_of_the_comparison_and_of_the_cap(capi, route):
    """Other resolutions; thresholds 0.0, -0.25 and 0.1 (a double) on cells around them -- both zeros, subnormals, the smallest
    normals, infinities, NaN, the float neighbours of the threshold; and caps that are ties in cells (max_distance = k * res and
    res * sqrt(k)): the definition's cap_cells says on which side each falls.  tests/test_distance_ref.py holds the inputs to that."""
    rows, cols = K.EDGE_SHAPE
    seed = 1000 * rows + cols
    tie_maps = K.tie_maps(seed)

    def check(ctx, maps, mode, threshold, md, res, what):
        want = definition(maps, mode, md, threshold, res)
        ctx.upload_layer(IN, to_device(maps))
        ctx.run_distance(mode, threshold, md, IN, OUT)
        got = from_device(ctx.download(OUT), K.BATCH, rows, cols)
        first, bad = differing(got, want)
        assert bad == 0, f"route {route} {what}: {bad} cells differ, (map, i, j), got, want: {first}"
        assert not np.isnan(got).any()

    for res in K.EDGE_RESOLUTIONS + [K.RES]:
        with context(capi, rows, cols, K.BATCH, None, route, res) as ctx:
            if res != K.RES:
                md = K.cap_for(K.EDGE_REACH, res)
                assert D.cap_cells(md, res)[1] == K.EDGE_REACH
                for mode in K.MODES:
                    check(ctx, maps_of(rows, cols), mode, K.THRESHOLD, md, res, f"res {res} mode {mode}")
            else:
                for threshold, pool in K.EDGE_POOLS:
                    for mode in K.MODES:
                        check(ctx, K.edge_maps(threshold, pool, mode, seed), mode, threshold, K.cap_for(K.EDGE_REACH), res, f"threshold {threshold} mode {mode}")
            ties = [(f"{k} * res", k * res) for k in K.TIE_CELLS] + [(f"res * sqrt({k})", res * float(np.sqrt(np.float64(k)))) for k in K.TIE_SQUARES]
            for name, md in ties:
                check(ctx, tie_maps, K.BELOW, K.THRESHOLD, md, res, f"res {res} cap {name} = {md!r}: cap2 {D.cap_cells(md, res)[0]}")


def test_refusals(capi):
    rows, cols = 70, 37
    maps = maps_of(rows, cols)
    with context(capi, rows, cols, K.BATCH, maps) as ctx:
        absent = ctx.add_layer("absent")
        tin, tout = capi.LAYERS[IN], capi.LAYERS[OUT]
        for call, code, words in [
                (lambda: ctx.run_distance(K.BELOW, 0.5, 0.0, IN, OUT), capi.TE_ERR_BAD_PARAM, "max_distance must be finite and positive"),
                (lambda: ctx.run_distance(K.BELOW, 0.5, -1.0, IN, OUT), capi.TE_ERR_BAD_PARAM, "max_distance must be finite and positive"),
                (lambda: ctx.run_distance(K.BELOW, 0.5, np.nan, IN, OUT), capi.TE_ERR_BAD_PARAM, "max_distance must be finite and positive"),
                (lambda: ctx.run_distance(K.BELOW, 0.5, np.inf, IN, OUT), capi.TE_ERR_BAD_PARAM, "max_distance must be finite and positive"),
                (lambda: ctx.run_distance(K.BELOW, 0.5, 32768 * K.RES, IN, OUT), capi.TE_ERR_BAD_PARAM, "more than 32767 cells"),
                (lambda: ctx.run_distance(0, 0.5, 1.0, IN, OUT), capi.TE_ERR_INVALID_ARG, "mode 0"),
                (lambda: ctx.run_distance(3, 0.5, 1.0, IN, OUT), capi.TE_ERR_INVALID_ARG, "mode 3"),
                (lambda: ctx.run_distance(K.BELOW | 8, 0.5, 1.0, IN, OUT), capi.TE_ERR_INVALID_ARG, "mode 9"),
                (lambda: ctx.run_distance(K.NAN_IS_SEED, 0.5, 1.0, IN, OUT), capi.TE_ERR_INVALID_ARG, "mode 4"),
                (lambda: ctx.run_distance(K.BELOW, np.nan, 1.0, IN, OUT), capi.TE_ERR_BAD_PARAM, "threshold must be finite"),
                (lambda: ctx.run_distance(K.BELOW, np.inf, 1.0, IN, OUT), capi.TE_ERR_BAD_PARAM, "threshold must be finite"),
                (lambda: ctx.run_distance(K.BELOW, 0.5, 1.0, absent, OUT), capi.TE_ERR_NOT_READY, f"the input layer {absent} does not exist yet"),
                (lambda: ctx.run_distance(K.BELOW, 0.5, 1.0, 40, OUT), capi.TE_ERR_INVALID_ARG, "bad input layer 40"),
                (lambda: ctx.run_distance(K.BELOW, 0.5, 1.0, IN, 40), capi.TE_ERR_INVALID_ARG, "bad output layer 40"),
                (lambda: ctx.run_distance(K.BELOW, 0.5, 1.0, IN, OUT, K.BATCH, 1), capi.TE_ERR_INVALID_ARG, f"maps [{K.BATCH},{K.BATCH + 1}) of batch {K.BATCH}"),
                (lambda: ctx.run_distance_region(K.BELOW, 0.5, 1.0, IN, IN, 0, 0, 0, 4, 4), capi.TE_ERR_INVALID_ARG, f"in_layer == out_layer ({tin})"),
                (lambda: ctx.run_distance_region(K.BELOW, 0.5, 1.0, IN, OUT, 0, rows - 3, 0, 4, 4), capi.TE_ERR_INVALID_ARG,
                 f"rectangle ({rows - 3},0)+(4,4) outside {rows}x{cols}"),
                (lambda: ctx.run_distance_region(K.BELOW, 0.5, 1.0, IN, OUT, 0, 0, 0, 0, 4), capi.TE_ERR_INVALID_ARG, "rectangle (0,0)+(0,4)"),
                (lambda: ctx.run_distance_region(K.BELOW, 0.5, 1.0, IN, OUT, K.BATCH, 0, 0, 4, 4), capi.TE_ERR_INVALID_ARG, f"map {K.BATCH} of batch {K.BATCH}"),
                (lambda: ctx.run_distance_region(K.BELOW, 0.5, 1.0, absent, OUT, 0, 0, 0, 4, 4), capi.TE_ERR_NOT_READY, f"the input layer {absent} does not exist yet"),
                (lambda: ctx.run_distance_region(K.BELOW, 0.5, 0.0, IN, OUT, 0, 0, 0, 4, 4), capi.TE_ERR_BAD_PARAM, "max_distance must be finite and positive"),
                (lambda: ctx.time_distance_samples(K.BELOW, 0.5, 1.0, IN, IN, 0, 1), capi.TE_ERR_INVALID_ARG, "in_layer == out_layer")]:
            with pytest.raises(capi.TeError) as e:
                call()
            assert e.value.code == code and words in str(e.value), (str(e.value), words)
        with pytest.raises(capi.TeError) as e:  # no call has succeeded yet
            ctx.distance_stats()
        assert e.value.code == capi.TE_ERR_NOT_READY
        assert tout != tin
        # the context is as it was: the next call runs
        ctx.run_distance(K.BELOW, 0.5, 1.0, IN, OUT)
        assert sum(ctx.distance_stats()) == K.BATCH * 2
    with capi.Context(0) as bare:
        with pytest.raises(capi.TeError) as e:
            bare.run_distance(K.BELOW, 0.5, 1.0, IN, OUT)
        assert e.value.code == capi.TE_ERR_NOT_READY and "geometry not set" in str(e.value)


def test_clearance_into_a_cost(capi):
    """te_run_distance on traversability below 0.5 into a user layer, then 1 - clearance ./ 0.5 with its threshold into a cost layer."""
    rows, cols = 70, 37
    maps = maps_of(rows, cols)
    steps = [("lower", 0.0, 0.0)]
    with context(capi, rows, cols, K.BATCH, maps) as ctx:
        ctx.add_layer("clearance"), ctx.add_layer("cost")
        ctx.run_distance("below", 0.5, 0.5, IN, "clearance")
        ctx.run_layer_expression("1 - clearance ./ 0.5", "cost", thresholds=steps)
        got = ctx.download("cost").reshape(K.BATCH, cols, rows)
    clearance = np.stack([D.distance(m, D.BELOW, 0.5, 0.5, K.RES).T for m in maps])
    # (every operation of the expression rounds to float32; expression_ref evaluates the same text over a name it knows)
    cost = np.float32(1.0) - clearance / np.float32(0.5)
    assert np.array_equal(bits(cost), bits(E.evaluate("1 - traversability ./ 0.5", {"traversability": clearance})))
    want = P.thresholds(cost, steps)
    assert np.array_equal(bits(got), bits(want))
    assert (got == 1.0).any() and (got == 0.0).any() and ((got > 0.0) & (got < 1.0)).any()
