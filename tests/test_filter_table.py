"""te_disc_table.h on the CPU: the filter discs of any radius (te_filter_any.hip).  The table is the disc the oracle's
CircleIterator visits -- runs counted inside the map, tie offsets decided per centre with isInside's own formula -- at
several centres and map origins for radii of 0.3 to 125 cells, and it is build_disc's disc for every radius build_disc
(te_disc.h, the function the library ships) accepts (a sweep in tests/cpu/disc_table_check.cpp)."""
import os
import subprocess

import pytest

from tests.conftest import ROOT


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("disc_table") / "disc_table_check"
    src = os.path.join(ROOT, "tests", "cpu", "disc_table_check.cpp")
    inc = os.path.join(ROOT, "traversability_estimation_amd", "csrc")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-I", inc, src, "-o", str(out)], check=True,
                   timeout=300)
    return str(out)


def table(exe, radius, res):
    lines = subprocess.run([exe, repr(radius), repr(res)], capture_output=True, text=True, timeout=60, check=True).stdout.split("\n")
    R, reach, npoints, n_ties = (int(v) for v in lines[0].split())
    hw = [int(v) for v in lines[1].split()]
    tv = [int(v) for v in lines[2].split()]
    assert len(hw) == R + 1 and len(tv) == 2 * n_ties
    return dict(R=R, reach=reach, npoints=npoints, hw=hw, ties=list(zip(tv[0::2], tv[1::2])))


def count_at(t, g, i, j, radius):
    """cells of the disc around (i, j) inside the map: the runs clipped, the ties with CircleIterator::isInside's arithmetic"""
    n = 0
    for dj in range(-t["R"], t["R"] + 1):
        if 0 <= j + dj < g.cols:
            h = t["hw"][abs(dj)]
            n += max(0, min(i + h, g.rows - 1) - max(i - h, 0) + 1)
    ax = g.pos_x + (0.5 * g.len_x - 0.5 * g.res)
    ay = g.pos_y + (0.5 * g.len_y - 0.5 * g.res)
    cx, cy = ax + g.res * float(-i), ay + g.res * float(-j)
    for di, dj in t["ties"]:
        if 0 <= i + di < g.rows and 0 <= j + dj < g.cols:
            dx = (ax + g.res * float(-(i + di))) - cx
            dy = (ay + g.res * float(-(j + dj))) - cy
            n += 1 if dx * dx + dy * dy <= radius * radius else 0
    return n


# radii in cells: fractional, whole-cell (tie) radii, and ones with many tie offsets (25 and 50: 20, 65 and 85: 36, 125: 28)
CELLS = [0.3, 1.0, 2.5, 9.0, 20.3, 25.0, 32.7, 33.0, 40.0, 47.9, 50.0, 65.0, 80.4, 85.0, 120.0, 125.0]


@pytest.mark.parametrize("cells", CELLS)
def test_table_is_the_oracle_circle(exe, oracle, cells):
    for res, (rows, cols), pos in ((0.01, (300, 280), (0.0, 0.0)), (0.02, (261, 300), (1.37, -2.11)), (0.03, (290, 251), (-5.5, 3.25))):
        radius = cells * res
        t = table(exe, radius, res)
        g = oracle.geom(rows, cols, res, pos)
        centres = {(0, 0), (rows - 1, cols - 1), (rows // 2, cols // 2), (3, cols // 3), (rows // 3, cols - 2), (rows - 7, 11)}
        for ci, cj in sorted(centres):
            assert count_at(t, g, ci, cj, radius) == oracle.circle_count(g, ci, cj, radius), (cells, res, ci, cj)


@pytest.mark.parametrize("cells,n_ties", [(25.0, 20), (50.0, 20), (65.0, 36), (85.0, 36), (125.0, 28), (40.0, 12), (40.3, 0)])
def test_tie_offsets(exe, cells, n_ties):
    t = table(exe, cells * 0.01, 0.01)
    assert len(t["ties"]) == n_ties, t["ties"]
    q = round(cells * cells) if cells == int(cells) else None
    for di, dj in t["ties"]:
        assert q is not None and di * di + dj * dj == q
    assert len(set(t["ties"])) == len(t["ties"])
    # nested runs, the tie at the end of a run never inside it, npoints the cells of the runs
    assert all(a >= b for a, b in zip(t["hw"], t["hw"][1:]))
    for di, dj in t["ties"]:
        assert abs(dj) > t["R"] or abs(di) > t["hw"][abs(dj)]
    assert t["npoints"] == sum((1 if b == 0 else 2) * (2 * h + 1) for b, h in enumerate(t["hw"]))
    assert t["reach"] == max([t["R"], t["hw"][0]] + [max(abs(a), abs(b)) for a, b in t["ties"]])


def test_agrees_with_build_disc(exe):
    checked, bad = (int(v) for v in subprocess.run([exe, "sweep"], capture_output=True, text=True, timeout=300, check=True).stdout.split())
    assert checked > 10000 and bad == 0, (checked, bad)
