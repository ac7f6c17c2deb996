"""The offset table of te_run_polygon_footprint and the inside test of every polygon kernel (csrc/te_polygon_table.h) on the
CPU: tests/cpu/polygon_table_check.cpp walks the table as k_polygon_footprint_table does, for every centre cell of small
maps on three geometries (origin near zero, origin 500 m away, resolution 0.01), against polygon_bbox plus polygon_inside --
the cells and their order, no run cell outside, no unlisted cell inside, every LDS index inside the tile, Quad::inside equal to
polygon_inside -- for a few hundred random polygons and for every footprint of tests/polygon_cases.py; plain and, as a
stand-alone program, under the sanitizers.  And every case of tests/polygon_cases.py takes the kernel it claims, with the
spans and the tile it claims: what the GPU tests rely on to reach both sides of the table's two limits."""
import os
import subprocess

import pytest

from tests import polygon_cases as K
from tests.conftest import ROOT

SRC = os.path.join(ROOT, "tests", "cpu", "polygon_table_check.cpp")
INC = os.path.join(ROOT, "traversability_estimation_amd", "csrc")


def build(tmp, flags):
    exe = str(tmp / "polygon_table_check")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off"] + flags + ["-I", INC, SRC, "-o", exe], check=True, timeout=300)
    return exe


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return build(tmp_path_factory.mktemp("polygon_table"), ["-O2"])


def out(exe, *args):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    return r.stdout.strip()


def checks(text):
    last = text.splitlines()[-1].split()
    assert last[1:] == ["checks,", "0", "failed", "checks"], text[-2000:]
    return int(last[0])


def test_check_program(exe):
    assert checks(out(exe)) > 10 ** 7


@pytest.mark.parametrize("name", [c["name"] for c in K.CASES])
def test_the_table_of_every_case_walks_the_cells_of_the_inside_test(exe, name):
    c = K.case(name)
    text = out(exe, "check", *K.route_args(c))
    # per geometry: both polygons of a table case are walked; of a per-cell case, the ones that fit (of the others the
    # program checks that the refusal names a limit: one check per polygon and geometry)
    want = sum(p[0] == "fits" for p in c["polygons"])
    assert int(text.splitlines()[0].split()[0]) == 3 * want
    assert checks(text) > (1000 if want else 5)


def test_check_program_under_the_sanitizers(tmp_path):
    """One build, as a stand-alone program: the random polygons and every case."""
    exe = build(tmp_path, ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    assert checks(out(exe)) > 10 ** 7
    for c in K.CASES:
        assert checks(out(exe, "check", *K.route_args(c))) > 5, c["name"]


def route(exe, c):
    lines = out(exe, "route", *K.route_args(c)).splitlines()
    polys = []
    for line in lines[:2]:
        f = line.split()
        polys.append(dict(kernel=f[0], why=f[1], di_span=int(f[2]), dj_span=int(f[3]), n_rows=int(f[4]), n_uncertain=int(f[5]), tile=int(f[6])))
    return polys, lines[2].split()[1]


@pytest.mark.parametrize("name", [c["name"] for c in K.CASES])
def test_every_case_takes_the_kernel_it_claims(exe, name):
    c = K.case(name)
    polys, kernel = route(exe, c)
    assert kernel == c["kernel"]
    for got, (why, di_span, dj_span, tile) in zip(polys, c["polygons"]):
        assert (got["why"], got["di_span"], got["dj_span"]) == (why, di_span, dj_span), got
        assert got["kernel"] == ("table" if why == "fits" else "percell")
        if why != "span":  # (a box beyond 255 offsets is refused before the used part, and with it the tile, is known)
            assert got["tile"] == tile == (255 + di_span) * dj_span * 8
        assert (got["tile"] <= 65536) == (why == "fits") or why == "span"
    assert (kernel == "table") == all(p[0] == "fits" for p in c["polygons"])


def test_the_limit_cases_sit_on_both_sides_of_both_limits(exe):
    """lds_fits is the largest square tile and long_y the largest tile there is; long_x has the largest row index; each has its
    neighbour on the other side."""
    def spans(name):
        return route(exe, K.case(name))[0][0]
    fit, over = spans("lds_fits"), spans("lds_over")
    assert fit["di_span"] == fit["dj_span"] == 28 and 65536 - fit["tile"] < (255 + 28) * 8  # within one row of the limit
    assert over["di_span"] == over["dj_span"] == 29 and over["why"] == "tile"
    assert spans("long_y")["tile"] == 65536 and spans("long_y")["di_span"] == 1 and spans("long_y_over")["why"] == "tile"
    assert spans("long_y_3")["di_span"] == 3 and (255 + 3) * 32 * 8 > 65536 >= spans("long_y_3")["tile"]
    x = spans("long_x")
    assert x["di_span"] == 251 >= 248 and x["n_rows"] == 251 and x["kernel"] == "table"
    assert spans("long_x_252")["why"] == spans("long_x_over")["why"] == "span"
    assert spans("long_x_252")["di_span"] == 256  # the box, one beyond the limit: the first footprint that does not fit
    mixed = route(exe, K.case("yaw_mixed"))
    assert [p["kernel"] for p in mixed[0]] == ["table", "percell"] and mixed[1] == "percell"
