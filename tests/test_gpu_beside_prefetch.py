"""Calls that run beside a prefetch (CtxLock with beside_prefetch = true, csrc/te_ctx.h): WHEN their kernels read and write.

te_prefetch_layers uploads whole layers on its own thread and stream; a call that passes `true` joins it only if its `touches`
mask meets the prefetch's.  A mask that leaves out a layer the kernel reads or writes is a race no value test sees.  For every
row of tests/beside_prefetch_cases.py (tests/test_beside_prefetch_table.py keeps that table complete) four situations:

  1  the call reads a layer the prefetch writes: its result is that of the NEW contents, in every cell, three rounds running
  2  the call writes a layer the prefetch writes: afterwards the layer holds the call's result, not the prefetched values
  3  the call touches none of the prefetched layers: its result is right, the eight layers arrive bit for bit, and the
     context's cached state is that of a plain upload (a chain on the prefetched elevation, the median fill's mask)
  4  the prefetch starts behind a call that is still reading or writing its layer (the ev0 wait of te_prefetch_layers)

The yardstick of every case is the quiet run: the same call in a fresh context after plain uploads and a sync, no prefetch
anywhere, compared bit for bit (te_run_filter: assert_layers_match at its default tolerance).  Every prefetch sends 8 layers
from pageable arrays with the layer under test last, so that it arrives several milliseconds after a launch that missed the
join -- in situation 4 first, where the collision is at the start.  Before the racing part each case asserts that a stale or
mixed read could not pass: the quiet results on OLD and on NEW differ in more than half of the cells the call writes or
downloads, and a written layer differs from the prefetched values in as many.

Measured (MI355X, recorded, not asserted; test_the_window_is_real prints both): the 8-layer prefetch alone takes 2.8 to 3.0 ms of
host time from te_prefetch_layers to the return of te_wait_prefetch (the first of a context, which starts the worker thread and
the staging ring: 15 to 20 ms); from te_prefetch_layers to the return of te_run_radius_filter beside it 0.05 ms.  With the
`touches` argument of te_run_radius_filter and of te_run_distance_region cleared in a scratch build, situation 1 fails in round 0:
radius-mean in 1843199 of 1843200 cells, distance-region in 770729 of the 777777 cells of its rectangle.
Situation 4, on a warm prefetcher: the nested standard deviation at window 21 takes 4.1 ms alone; its launch returns after
0.02 ms, te_prefetch_layers 0.1 ms later, te_wait_prefetch 6.5 to 6.8 ms after the launch returned (the call, then the
transfer).  In a scratch build without the ev0 record / wait of te_prefetch_layers all four cases fail: the reader's output
differs from the quiet run in 1403813 of 1843200 cells, the written layer does not hold the prefetched values.

The tile transfers (te_upload_layer_tile, te_download_tile) take the lock without `beside_prefetch`: they always join, and have
no row."""
import time

import numpy as np
import pytest

from tests import beside_prefetch_cases as cases
from tests.beside_prefetch_cases import COLS, E, N_PREFETCH, RECT, ROWS, ROWS_TABLE
from tests.helpers import OUT_LAYERS, assert_layers_match, compare_layer

pytestmark = pytest.mark.gpu
OLD, NEW = 1, 2
FILLER_SEED = 7


@pytest.fixture(scope="module")
def capi():
    from traversability_estimation_amd import capi
    capi.load()
    assert capi.device_count() >= 1, "no MI355X visible"
    return capi


def open_ctx(capi, row):
    ctx = capi.Context(0)
    ctx.set_params(cases.params(capi))
    ctx.set_geometry(ROWS, COLS, 1, cases.RES)
    for k, u in enumerate(cases.USER):
        assert ctx.add_layer(u) == capi.LAYER_COUNT + k
    for name, value in (row.options if row is not None else ()):
        ctx.set_option(getattr(capi, name), value)
    return ctx


def value(row, layer, seed):
    return cases.content(row.kind(layer) if layer in row.reads else "noise", layer, seed)


def filler(layer):
    return cases.content("terrain" if layer == E else "noise", layer, FILLER_SEED)


def bystanders(row, n, elevation=False):
    """n layers the row does not name: the elevation first if asked for and free, then user layers"""
    free = ([E] if elevation and E not in row.touches else []) + [u for u in cases.USER if u not in row.touches]
    return free[:n]


BASE = 99


def put(ctx, row, held, base=BASE):
    """the row's fixed contents (seed `base`) and its read layers as `held` = {layer: seed}"""
    for layer in row.base:
        ctx.upload_layer(layer, cases.content("noise", layer, base))
    for layer, seed in held.items():
        ctx.upload_layer(layer, value(row, layer, seed))


def result_of(ctx, row, returned):
    """what shows the call's result, as {name: array}"""
    if returned is None:
        return {w: ctx.download(w) for w in row.writes}
    items = returned if isinstance(returned, list) else [returned]
    return {"result%d" % k: np.frombuffer(v, np.uint8) if isinstance(v, (bytes, bytearray)) else np.asarray(v) for k, v in enumerate(items)}


_quiet = {}


def quiet(capi, row, held, base=BASE):
    """The yardstick, once per (row, contents): a fresh context, plain uploads, a sync, the call, its result (and fill mask)."""
    key = (row.name, tuple(sorted(held.items())), base if row.base else BASE)
    if key not in _quiet:
        with open_ctx(capi, row) as ctx:
            put(ctx, row, held, base)
            ctx.sync()
            res = result_of(ctx, row, row.call(ctx, capi))
            ctx.sync()
            if row.fill_mask:
                res["fill_mask"] = ctx.download_fill_mask(0)
        for v in res.values():
            v.setflags(write=False)
        _quiet[key] = res
    return _quiet[key]


def cells_of(row, name, a):
    """the cells a comparison counts, as rows of a 2-D array of unsigned integers: a float layer cell by cell (a region row:
    the cells of RECT), records of up to 8 values record by record, the bytes of a message in groups of four from its end (its layers are its
    tail), anything else element by element"""
    a = np.ascontiguousarray(a)
    if a.dtype == np.float32 and a.size == ROWS * COLS and (name in row.writes or row.result_is_layer):
        a = a.reshape(COLS, ROWS)
        if row.region:
            r0, c0, h, w = RECT
            a = np.ascontiguousarray(a[c0:c0 + w, r0:r0 + h])
        return a.view(np.uint32).reshape(-1, 1)
    if a.ndim == 2 and a.shape[-1] <= 8:  # records: a cloud's points, the cells of several layers side by side
        return a.view(np.dtype("u%d" % a.dtype.itemsize))
    if a.dtype == np.uint8:  # (result_of: a serialised message)
        b = a.reshape(-1)
        return b[b.size % 4:].reshape(-1, 4)
    return a.reshape(-1, 1).view(np.dtype("u%d" % a.dtype.itemsize))


def differing(row, name, a, b):
    """(cells that differ, cells) of two results of one kind; records one of them lacks all count as differing.  A row compared
    at a tolerance counts the cells that differ by more than it (or in being NaN): what its comparison would refuse."""
    if row.tol:
        n_bad, _, _ = compare_layer(name, a, b)
        return n_bad, np.asarray(a).size
    ca, cb = cells_of(row, name, a), cells_of(row, name, b)
    n = min(len(ca), len(cb))
    return int((ca[:n] != cb[:n]).any(axis=1).sum()) + abs(len(ca) - len(cb)), max(len(ca), len(cb))


def assert_distinct(row, a, b, what):
    """the precondition: in more than half of the cells"""
    bad, total = 0, 0
    for name in a:
        if name == "fill_mask":
            continue
        d, n = differing(row, name, a[name], b[name])
        bad, total = bad + d, total + n
    print(f"{row.name}: {what}: {bad} of {total} cells differ")
    assert total > 0 and 2 * bad > total, f"{row.name}: {what} differ in {bad} of {total} cells only: a stale read could pass"


def assert_same(row, got, want, what):
    if row.tol:
        assert_layers_match(got, want, layers=list(want), ctx=f"{row.name}: {what}")
        return
    for name in want:
        a, b = np.asarray(got[name]), np.asarray(want[name])
        assert a.shape == b.shape and a.dtype == b.dtype, (row.name, what, name, a.shape, b.shape)
        if not np.array_equal(a.view(np.uint8), b.view(np.uint8)):
            d, n = differing(row, name, a, b)
            raise AssertionError(f"{row.name}: {what}: {name} differs from the quiet run in {d} of {n} cells")


def bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).reshape(-1).view(np.uint32), np.ascontiguousarray(b, np.float32).reshape(-1).view(np.uint32))


def ids(pairs):
    return [f"{r.name}-{layer}" for r, layer in pairs]


READS = [(r, layer) for r in ROWS_TABLE for layer in r.reads]
WRITES = [(r, layer) for r in ROWS_TABLE for layer in r.writes]
LONG = [(r, layer) for r in ROWS_TABLE if r.long_call for layer in dict.fromkeys(r.reads + r.writes)]


@pytest.mark.parametrize("row, layer", READS, ids=ids(READS))
def test_1_a_call_that_reads_a_prefetched_layer_sees_the_new_contents(capi, row, layer):
    held = {r: OLD for r in row.reads}
    want = {OLD: quiet(capi, row, held), NEW: quiet(capi, row, {**held, layer: NEW})}
    assert_distinct(row, want[OLD], want[NEW], f"the quiet results on OLD and NEW {layer}")
    if layer in row.writes:  # in place: the prefetch must not land on the result either
        assert_distinct(row, {layer: want[NEW][layer]}, {layer: value(row, layer, NEW)}, f"the quiet result and NEW {layer}")
    others = bystanders(row, N_PREFETCH - 1)
    with open_ctx(capi, row) as ctx:
        put(ctx, row, held)
        ctx.sync()
        nxt = NEW
        for rnd in range(3):  # (a race does not lose every time)
            if rnd:  # as the quiet run had them: the fixed contents of a region form's output, an operand the call rewrote in place
                put(ctx, row, {r: OLD for r in row.reads if r in row.writes and r != layer})
            ctx.prefetch_layers({**{b: filler(b) for b in others}, layer: value(row, layer, nxt)})
            got = result_of(ctx, row, row.call(ctx, capi))
            ctx.wait_prefetch()
            assert_same(row, got, {k: v for k, v in want[nxt].items() if k != "fill_mask"}, f"round {rnd}, beside a prefetch of {layer}")
            nxt = OLD if nxt == NEW else NEW


@pytest.mark.parametrize("row, layer", WRITES, ids=ids(WRITES))
def test_2_a_call_that_writes_a_prefetched_layer_is_the_last_writer(capi, row, layer):
    held = {r: OLD for r in row.reads}
    sent = value(row, layer, NEW)
    effective = {**held, layer: NEW} if layer in row.reads else held  # in place: the call reads what the prefetch brought
    # (a region form writes its rectangle alone: outside it the layer keeps what the prefetch brought, so the quiet run starts
    # from those values)
    want = {k: v for k, v in quiet(capi, row, effective, base=NEW).items() if k != "fill_mask"}
    if layer in want:
        assert_distinct(row, {layer: want[layer]}, {layer: sent}, f"the quiet result and the prefetched {layer}")
    others = bystanders(row, N_PREFETCH - 1)
    with open_ctx(capi, row) as ctx:
        put(ctx, row, held)
        ctx.sync()
        ctx.prefetch_layers({**{b: filler(b) for b in others}, layer: sent})
        returned = row.call(ctx, capi)
        ctx.wait_prefetch()
        ctx.sync()
        assert_same(row, result_of(ctx, row, returned), want, f"after a prefetch of {layer}, which the call writes")
        for b in others:
            assert bits_equal(ctx.download(b), filler(b)), (row.name, b)


SCRATCH = [(r, layer) for r in ROWS_TABLE for layer in r.may_write]


@pytest.mark.parametrize("row, layer", SCRATCH, ids=ids(SCRATCH))
def test_2_a_call_is_the_last_writer_of_a_layer_it_uses_as_scratch(capi, row, layer):
    """A layer outside the call's contract that its kernels may write on the way (te_run_filter(TE_FILTER_NORMALS): the slope
    and the roughness; filter_layers names both).  Whether this route writes it is read off a quiet call first: the layer held
    noise, and either still does or holds the call's own values.  Behind a prefetch of it the same holds in the same order:
    a call that writes the layer joins first and is the last writer -- the layer holds the call's own values, not the prefetched
    ones --, a call that leaves it alone (the raster method) leaves the prefetched values whole."""
    held = {r: OLD for r in row.reads}
    before, sent = cases.content("noise", layer, OLD), cases.content("noise", layer, NEW)
    with open_ctx(capi, row) as ctx:
        put(ctx, row, held)
        ctx.upload_layer(layer, before)
        ctx.sync()
        row.call(ctx, capi)
        ctx.sync()
        own = ctx.download(layer)
        writes_it = not bits_equal(own, before)
        if writes_it:
            d, n = differing(row, layer, own, sent)
            assert 2 * d > n, f"{row.name}: the call's own {layer} and the prefetched one differ in {d} of {n} cells only"
        ctx.prefetch_layers({**{b: filler(b) for b in bystanders(row, N_PREFETCH - 1)}, layer: sent})
        row.call(ctx, capi)
        ctx.wait_prefetch()
        ctx.sync()
        got = ctx.download(layer)
    print(f"{row.name}: the call {'writes' if writes_it else 'leaves'} {layer}")
    if writes_it:
        n_bad, _, _ = compare_layer(layer, got, own)
        assert n_bad == 0, f"{row.name}: {layer} does not hold the call's own values behind a prefetch of it: {n_bad} cells"
    else:
        assert bits_equal(got, sent), f"{row.name}: {layer}, which the call leaves alone, does not hold the prefetched values"


@pytest.mark.parametrize("row", ROWS_TABLE, ids=[r.name for r in ROWS_TABLE])
def test_3_a_call_that_touches_no_prefetched_layer_runs_beside_it(capi, row):
    held = {r: OLD for r in row.reads}
    want = quiet(capi, row, held)
    sent = bystanders(row, N_PREFETCH, elevation=True)
    assert len(sent) == N_PREFETCH
    with open_ctx(capi, row) as ctx:
        put(ctx, row, held)
        ctx.sync()
        ctx.prefetch_layers({b: filler(b) for b in sent})
        got = result_of(ctx, row, row.call(ctx, capi))
        ctx.wait_prefetch()
        assert_same(row, got, {k: v for k, v in want.items() if k != "fill_mask"}, "beside a prefetch of other layers")
        if row.fill_mask:
            assert np.array_equal(ctx.download_fill_mask(0), want["fill_mask"]), row.name
        for b in sent:
            assert bits_equal(ctx.download(b), filler(b)), (row.name, b)
        if E in sent:  # the state a prefetched elevation leaves is the state a plain upload leaves
            ctx.run_chain(0)
            ctx.sync()
            chain = {k: ctx.download(k) for k in OUT_LAYERS}
            ref = chain_of_a_plain_upload(capi, row)
            for k in OUT_LAYERS:
                assert bits_equal(chain[k], ref[k]), (row.name, k)


_chain = {}


def chain_of_a_plain_upload(capi, row):
    if row.options not in _chain:
        with open_ctx(capi, row) as ctx:
            ctx.upload_elevation(filler(E))
            ctx.run_chain(0)
            ctx.sync()
            _chain[row.options] = {k: ctx.download(k) for k in OUT_LAYERS}
    return _chain[row.options]


@pytest.mark.parametrize("row, layer", LONG, ids=ids(LONG))
def test_4_a_prefetch_waits_for_a_call_that_still_uses_its_layer(capi, row, layer):
    """The slowest call the library has (the nested standard deviation at window 21: profiles/window_expression_bench.json) is
    queued and not waited for; a prefetch of the layer it reads, or writes, follows at once, that layer FIRST in the list.
    The context's prefetcher is warm: a first prefetch starts its thread, its stream and its page-locked ring, which takes
    longer than the call runs, so one of bystanders is sent and waited for before.  Recorded: the call's own duration (queued
    and waited for, host clock) and the time from its return to the return of te_wait_prefetch."""
    held = {r: OLD for r in row.reads}
    want = quiet(capi, row, held)
    sent = value(row, layer, NEW)
    if layer in row.reads:
        assert_distinct(row, want, quiet(capi, row, {**held, layer: NEW}), f"the quiet results on OLD and NEW {layer}")
    else:
        assert_distinct(row, {layer: want[layer]}, {layer: sent}, f"the quiet result and the prefetched {layer}")
    others = bystanders(row, N_PREFETCH)
    with open_ctx(capi, row) as ctx:
        put(ctx, row, held)
        ctx.prefetch_layers({b: filler(b) for b in others})
        ctx.wait_prefetch()
        ctx.sync()
        t0 = time.perf_counter()
        row.call(ctx, capi)  # (once alone: its duration; the same inputs, so the racing call below writes the same values)
        ctx.sync()
        alone = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        row.call(ctx, capi)
        t1 = time.perf_counter()
        ctx.prefetch_layers({layer: sent, **{b: filler(b) for b in others[:N_PREFETCH - 1]}})
        t2 = time.perf_counter()
        ctx.wait_prefetch()
        t3 = time.perf_counter()
        ctx.sync()
        print(f"WINDOW {row.name}, prefetch of {layer}: the call alone {alone:.3f} ms; its launch returns after {(t1 - t0) * 1e3:.3f} ms, "
              f"te_prefetch_layers after {(t2 - t1) * 1e3:.3f} ms more, te_wait_prefetch {(t3 - t1) * 1e3:.3f} ms after the launch returned")
        assert bits_equal(ctx.download(layer), sent), f"{row.name}: {layer} does not hold the prefetched values"
        if layer in row.reads and layer not in row.writes:
            assert_same(row, result_of(ctx, row, None), want, f"the reader of {layer}, a prefetch of it right behind")


def test_the_window_is_real(capi):
    """Recorded, not asserted: the host time of the 8-layer prefetch alone, and in a second run the host time from
    te_prefetch_layers to the return of a racing call's launch (a call that does not join: situation 3's)."""
    row = cases.BY_NAME["radius-mean"]
    sent = bystanders(row, N_PREFETCH, elevation=True)
    layers = {b: filler(b) for b in sent}
    alone, launch = [], []
    with open_ctx(capi, row) as ctx:
        put(ctx, row, {r: OLD for r in row.reads})
        ctx.sync()
        for k in range(4):
            t0 = time.perf_counter()
            ctx.prefetch_layers(layers)
            ctx.wait_prefetch()
            alone.append((time.perf_counter() - t0) * 1e3)
        for k in range(4):
            t0 = time.perf_counter()
            ctx.prefetch_layers(layers)
            row.call(ctx, capi)
            launch.append((time.perf_counter() - t0) * 1e3)
            ctx.wait_prefetch()
            ctx.sync()
    print(f"WINDOW prefetch of {N_PREFETCH} layers of {cases.LAYER_BYTES / 2 ** 20:.2f} MiB, alone, ms: {['%.3f' % v for v in alone]}")
    print(f"WINDOW te_prefetch_layers to the return of te_run_radius_filter beside it, ms: {['%.3f' % v for v in launch]}")
    assert min(alone) > 0 and min(launch) > 0
