"""The case table of tests/beside_prefetch_cases.py is complete: every exported te_* entry point that takes the context's lock
with `beside_prefetch = true` has a row there, or is listed as touching no layer.  Found by reading csrc/*.hip: a CtxLock whose
second argument is `true`, the function around it, and -- where that is a helper shared by several entry points -- the te_*
functions of the same file that call it."""
import glob
import os
import re

import numpy as np

from tests import beside_prefetch_cases as cases

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "traversability_estimation_amd", "csrc")
LOCK = re.compile(r"\bCtxLock\s+\w+\s*\(\s*\w+\s*,\s*(?:/\*.*?\*/\s*)?true\b")
# a function definition at the start of a line: its name is the last identifier before the parameter list
DEFINITION = re.compile(r"^(?:static\s+|inline\s+|extern\s+\"C\"\s+)*[A-Za-z_][\w:<>\*&\s]*?\b(\w+)\s*\([^;{}]*\)\s*(?:const\s*)?\{", re.M)


def definitions(text):
    """[(name, start of the body, end of the body)] of the functions defined at the start of a line"""
    out = []
    for m in DEFINITION.finditer(text):
        depth, k = 0, m.end() - 1
        while k < len(text):
            depth += {"{": 1, "}": -1}.get(text[k], 0)
            if depth == 0:
                break
            k += 1
        out.append((m.group(1), m.end(), k))
    return out


def beside_prefetch_entries():
    found, sites = set(), 0
    for path in sorted(glob.glob(os.path.join(CSRC, "*.hip"))):
        with open(path) as f:
            text = f.read()
        defs = definitions(text)
        for lock in LOCK.finditer(text):
            sites += 1
            owners = [name for name, a, b in defs if a <= lock.start() < b]
            assert owners, (path, text[lock.start():lock.start() + 80])
            todo, seen = [owners[-1]], set()
            while todo:  # a shared helper: the functions of this file that call it, down to the exported names
                name = todo.pop()
                if name in seen:
                    continue
                seen.add(name)
                if name.startswith("te_"):
                    found.add(name)
                    continue
                callers = [n for n, a, b in defs if n != name and re.search(r"\b%s\s*\(" % re.escape(name), text[a:b])]
                assert callers, f"{os.path.basename(path)}: nothing in the file calls {name}, which runs beside a prefetch"
                todo += callers
    return found, sites


def test_every_entry_point_that_runs_beside_a_prefetch_has_a_row():
    found, sites = beside_prefetch_entries()
    assert sites >= 31, sites  # (the scan still finds the lock constructions: 31 when this was written)
    with open(os.path.join(os.path.dirname(CSRC), "..", "include", "travgpu.h")) as f:
        header = f.read()
    for name in found:
        assert re.search(r"\b%s\s*\(" % name, header), f"{name} is not declared in include/travgpu.h"
    table = cases.entries()
    assert not (table & set(cases.NO_LAYER)), table & set(cases.NO_LAYER)
    assert found == table | set(cases.NO_LAYER), {"without a row": sorted(found - table - set(cases.NO_LAYER)),
                                                  "rows of calls that always join": sorted((table | set(cases.NO_LAYER)) - found)}


def test_the_scan_follows_the_shared_helpers():
    found, _ = beside_prefetch_entries()
    for name in ("te_run_layer_expression", "te_run_layer_expression_thresholds", "te_run_layer_expression_region", "te_run_layer_expression_thresholds_region",
                 "te_run_components", "te_run_reachable", "te_download_layer_circular", "te_download_msg"):
        assert name in found, name
    for name in ("te_run_chain", "te_sync", "te_upload_layer", "te_upload_layer_tile", "te_download_tile", "te_wait_prefetch"):
        assert name not in found, name


def test_the_table_is_consistent():
    assert cases.LAYER_BYTES > cases.STAGING_THRESHOLD_BYTES
    with open(os.path.join(CSRC, "te_internal.h")) as f:
        assert re.search(r"kMinBytes\s*=\s*\(size_t\)4\s*<<\s*20", f.read()), "HostStager::kMinBytes is no longer 4 MiB: see beside_prefetch_cases.py"
    names = set(cases.USER) | {cases.E, cases.SL, cases.ST, cases.RO, cases.T, cases.NX, cases.NY, cases.NZ, cases.RS}
    for r in cases.ROWS_TABLE:
        assert set(r.touches) <= names, r.name
        assert r.reads or r.writes, r.name
        assert set(r.base) <= set(r.writes), r.name
        # eight bystanders must be left for a prefetch the row does not touch
        assert len([u for u in cases.USER if u not in r.touches]) >= cases.N_PREFETCH, r.name
    assert any(cases.TOP_USER in r.reads for r in cases.ROWS_TABLE) and any(cases.TOP_USER in r.writes for r in cases.ROWS_TABLE)
    assert cases.USER.index(cases.TOP_USER) + 15 == cases.TOP_USER_ID
    for f in ("slope", "step", "roughness", "combine", "normals"):
        assert "filter-" + f in cases.BY_NAME
    assert cases.BY_NAME["filter-normals-raster"].options == (("OPT_NORMALS_ALGORITHM", 1),)


def _half_differ(a, b):
    a, b = np.asarray(a), np.asarray(b)
    same = (a == b) | ((a != a) & (b != b)) if a.dtype.kind == "f" else a == b
    n = int((~same).sum())
    assert 2 * n > a.size, (n, a.size)
    return n


def test_old_and_new_differ_in_more_than_half_of_the_cells_on_the_references():
    """What the CPU can show of the GPU tests' precondition: on cases.SMALL, with the references of tests/ref_py, the result on
    OLD and the result on NEW differ in more than half of the cells for the rows whose outputs are few-valued or capped -- the
    distance, the components, the reachable cells, the threshold, the occupancy, the median fill.  (The references take
    (rows, cols); the contents are [cols][rows].)  The GPU tests assert the same at their own shape before they race."""
    from tests.ref_py import components_ref, distance_ref, median_fill_ref, occupancy_ref, pointwise_ref
    rows, cols = cases.SMALL
    old_new = lambda kind, layer: [cases.content(kind, layer, seed, cases.SMALL).T for seed in (1, 2)]
    mode = distance_ref.BELOW | distance_ref.NAN_IS_SEED
    kind, threshold, cap = cases.D_ARGS
    assert kind == "below" and cases.C_ARGS == ("below", threshold)
    _half_differ(*[distance_ref.distance(a, mode, threshold, cap, cases.RES) for a in old_new("seeds", cases.T)])
    _half_differ(*[components_ref.sizes(a, mode, threshold, 4) for a in old_new("blocked", cases.T)])
    _half_differ(*[components_ref.sizes(a, mode, threshold, 8) for a in old_new("blocked", cases.TOP_USER)])
    reach = [components_ref.reachable(a, mode, threshold, 4, [cases.start_of(cases.SMALL)]) for a in old_new("walled", cases.RS)]
    assert reach[0].mean() > 0.9 and reach[1].mean() < 0.1  # (OLD: the open map; NEW: the box around the start)
    _half_differ(*reach)
    cut = [pointwise_ref.threshold(a, *cases.CUT) for a in old_new("noise", cases.RO)]
    _half_differ(*cut)
    _half_differ(cut[1], old_new("noise", cases.RO)[1])  # in place: the result differs from what the prefetch brought
    _half_differ(*[occupancy_ref.to_occupancy(a, 0.0, 1.0) for a in old_new("noise", cases.T)])
    _half_differ(*[median_fill_ref.median_fill(a, cases.RES, filter_existing_values=True, existing_value_radius=0.05)[0] for a in old_new("holed", "u2")])
