"""The cases of tests/test_gpu_footprint_values.py: what each one feeds the route plan of the circular footprint pass, and
the route and the fixed-point exponent k it must be planned for.  tests/cpu/fp_route_check.cpp holds the same inputs as
named cases (compiled from te_fp_route.h, the header the library routes with) and tests/test_fp_route.py compares what it
prints with PLANNED below -- the library does not report the kernel it launched, so this is where a GPU case's route is pinned.
No GPU, no library: plain values."""
import math

TF = 1.0 + 1e-6  # synth.benchmark_radius: a radius just above a whole number of cells is tie-free
ROWS, COLS, RES, POS = 96, 80, 0.05, (1.5, -2.0)
K_UOFF = 4096.0  # te_fp_route.h kFpUOff, for the boundary family; tests/test_fp_route.py holds it to the header's value

# footprint geometries: name -> (fp_radius in cells, fp_offset in cells, tie radius, rows, cols)
GEOS = {
    "r5": (3.0, 2.0, False, ROWS, COLS),        # tie-free: k_fp_slide3's inputs
    "r9": (6.0, 3.0, False, ROWS, COLS),
    "reach18": (12.0, 6.5, None, ROWS, COLS),   # 18.5 cells: the general kernel's inputs
    "tie15": (10.0, 5.0, True, ROWS, COLS),     # a whole-cell tie radius
    "rows48": (6.0, 3.0, False, 48, COLS),      # narrower than a wavefront
    "r15": (10.0, 5.0, False, ROWS, COLS),      # tie-free, 709 cells
    "sat5": (10.0, math.sqrt(250.0) - 10.0, False, ROWS, COLS),  # k_fp_slide5's largest disc: Q = 250, 793 cells
    "sat4_15": (10.0, 5.0, True, ROWS, COLS),
    "sat4_16": (10.0, 6.0, True, ROWS, COLS),
}


def radii(geo, res=RES):
    """(fp_radius, fp_offset) in metres, as the GPU tests and the oracle take them."""
    rad, off, tie = GEOS[geo][:3]
    f = TF if tie is False else 1.0
    return rad * res * f, off * res * f


def disc_cells(geo):
    """Cells of the whole disc, those on the circle of a tie radius included."""
    rad, off, tie = GEOS[geo][:3]
    q = (rad + off) ** 2 * (1.0 + 1e-9)
    n = int(rad + off) + 1
    return sum(1 for a in range(-n, n + 1) for b in range(-n, n + 1) if a * a + b * b <= q)


def fp_fixed_k(cells, cap, limit):
    """te_fp_route.h fp_fixed_k, restated (tests/test_fp_route.py holds it to the harness's printed k)."""
    k = 23
    while k >= 0 and cells * (cap * 2.0 ** k + 1.0) >= limit:
        k -= 1
    return k


def fixed_cap(tcap, default):
    return max(tcap, default) * (1.0 + 1e-6) + 1e-12


# fixed point at saturation: geometry -> (cells of fp_fixed_k, limit, the largest float w_scale with k = 17 under the weights
# 1 1 1, the next float: the first with k = 16)
SAT = {
    "sat5": (793, 2.0 ** 27, float.fromhex("0x1.b8c2a2p-2"), float.fromhex("0x1.b8c2a4p-2")),
    "sat4_15": (31, 2.0 ** 24, float.fromhex("0x1.6057d4p+0"), float.fromhex("0x1.6057d6p+0")),
    "sat4_16": (33, 2.0 ** 24, float.fromhex("0x1.4afd28p+0"), float.fromhex("0x1.4afd2ap+0")),
}


def sat_scale(geo, k):
    """w_scale of case fv_<geo>_k<k>: the largest float that still gives k (23 .. 17), the first that gives 16."""
    s17, s16 = SAT[geo][2:]
    return s16 if k == 16 else s17 * 2.0 ** (17 - k)


# name -> (route, k): what the harness must print for the case of that name (k = -1 off the fixed-point routes)
PLANNED = {}
for _g in ("r5", "r9", "reach18", "tie15", "rows48"):
    PLANNED[f"fv_ext_{_g}"] = ("any", -1)        # no bound: never a kernel that packs the count into the sum
    PLANNED[f"fv_ext_{_g}_def50"] = ("any", -1)
    PLANNED[f"fv_ext_{_g}_any"] = ("any", -1)    # TE_OPT_FP_ANY_REACH: the control
PLANNED.update({
    "fv_w1111_r15": ("any", -1),            # 709 cells x 3 = 2127 >= 2048 (k would be 15: no fixed point either)
    "fv_w1111_r15_batch2": ("any", -1),
    "fv_w1111_r15_region": ("any", -1),
    "fv_w1_10_r9": ("any", -1),             # 253 cells x 30
    "fv_wneg_r9": ("any", -1),              # a negative weight: no bound
    "fv_def50_chain_r5": ("any", -1),       # 81 cells x 50
    "fv_wdefault_r15": ("slide5", 17),      # the default weights keep their kernels
    "fv_wdefault_r9": ("slide5", 19),
    "fv_bound_below_reach18": ("general", -1),  # 1085 cells x 1.88 = 2039.8
    "fv_bound_above_reach18": ("any", -1),      # 1085 cells x 1.89 = 2050.7
})
for _g in SAT:
    for _k in range(23, 16, -1):
        PLANNED[f"fv_{_g}_k{_k}"] = ("slide5" if _g == "sat5" else "slide4", _k)
    PLANNED[f"fv_{_g}_defcap"] = ("slide5" if _g == "sat5" else "slide4", 17)
PLANNED["fv_sat5_k16"] = ("slide3", -1)     # the pass leaves the fixed-point route: 793 x 1.2913 = 1024 keeps the double kernel
PLANNED["fv_sat4_15_k16"] = ("any", -1)     # 709 x 4.129 = 2927: no packed sum either
PLANNED["fv_sat4_16_k16"] = ("any", -1)
