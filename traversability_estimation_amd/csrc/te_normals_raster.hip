// te_normals_raster.hip -- gridMapFilters/NormalVectorsFilter, `algorithm: raster` (TE_OPT_NORMALS_ALGORITHM = 1): the normal
// of a cell from the finite differences of its four neighbours, one pass over the elevation that writes
// surface_normal_{x,y,z} and, in the chain form, traversability_slope (SlopeFilter::update, SlopeFilter.cpp:59-88, on the
// float32 surface_normal_z it has just stored).  The contract is restated in include/travgpu.h (grid_map_filters is not in
// the reference tree); tests/ref_py/raster_normals_ref.py is its numpy form and the kernel is held to it bit for bit.
//
// Built with -ffp-contract=off and without fast-math: every operation below is one separately rounded double, the division
// and the square root are the compiler's IEEE expansions (v_div_scale / v_div_fmas / v_div_fixup, and the corrected
// v_rsq_f64 iteration).
//
// Shape of the kernel, and why:
//   - One cell per thread, a wavefront on 64 consecutive rows i of one column j (i is the fast axis of the column-major
//     layer), a workgroup of 4 wavefronts on 4 neighbouring columns.  Per cell the pass moves 4 B in and 16 B out; what a
//     thread DOES per cell is three double divisions, a double square root and, with the slope, a double acos and a fourth
//     division -- several hundred VALU instructions.  The kernel is therefore not paced by how wide its loads are:
//     64 lanes x 4 B is a whole 256 B request per wave-instruction, the shape MI355X_MICROARCH.md measures at the full
//     streaming store rate (6.0 - 6.2 TB/s for one dword per lane), and many resident waves (no LDS, few registers) hide
//     the latency.  More cells per thread would only lengthen the dependent double chains per wave.  Measured
//     (tools/raster_normals_bench.py, 4096^2): 0.091 ms for the normals alone, 2.1 x what its 16 B per cell cost at the rate
//     of a device copy -- the arithmetic, not the memory, is what is left.
//   - The five values of a cell are five scalar loads.  t and b are the addresses next to c, in the same or the adjacent
//     128 B line the wave has just requested; l and r are the same rows of the two neighbouring columns, which the other
//     wavefronts of the workgroup (and the next workgroup along j) read as their c: HBM sees each elevation once, the
//     rest is served by the L1 / L2.  16 B vector loads are no option: a column starts at j * rows * 4 bytes, which no
//     vector width divides for odd `rows`.
//   - No LDS, no tables.  Every load is bounds-checked against the map (the outermost line of cells is never visited, so
//     an interior cell's neighbours are all inside it): nothing is read outside a map, not even the slab's guard rows.
//   - Offsets are 64-bit (size_t): maps above 2^32 bytes per layer need no refusal.  The batch is the slowest part of the
//     flattened block index.
#include "te_cell.h"
#include "te_internal.h"

namespace te {
namespace fast {

namespace {

constexpr int kRasterRows = 64;  // cells of a block along i: one wavefront
constexpr int kRasterCols = 4;   // ... along j: one wavefront each

// One direction: lo / hi the neighbours towards smaller / larger index, c the centre.  false: no gradient.
__device__ __forceinline__ bool raster_gradient(double lo, double c, double hi, double res, double& g) {
  const bool flo = __builtin_isfinite(lo), fhi = __builtin_isfinite(hi);
  if (flo && fhi) {
    g = (hi - lo) / (2.0 * res);
    return true;
  }
  if (!__builtin_isfinite(c)) return false;
  if (flo) {
    g = (c - lo) / res;
    return true;
  }
  if (fhi) {
    g = (hi - c) / res;
    return true;
  }
  return false;
}

template <bool SLOPE>
__global__ __launch_bounds__(kRasterRows* kRasterCols) void k_normals_raster(int rows, int cols, int nbx, int nby, double res, int axis,
                                                                              double slope_crit, const float* __restrict__ elev,
                                                                              float* __restrict__ onx, float* __restrict__ ony,
                                                                              float* __restrict__ onz, float* __restrict__ slope) {
  // (uniform: one division per block, not per cell)
  const unsigned b = blockIdx.x;
  const unsigned per_map = (unsigned)nbx * (unsigned)nby;
  const unsigned map = b / per_map, bm = b - map * per_map;
  const unsigned by = bm / (unsigned)nbx, bx = bm - by * (unsigned)nbx;
  const int i = (int)bx * kRasterRows + (int)threadIdx.x;
  const int j = (int)by * kRasterCols + (int)threadIdx.y;
  if (i >= rows || j >= cols) return;
  const size_t o = ((size_t)map * (size_t)cols + (size_t)j) * (size_t)rows + (size_t)i;
  const float qnan = __builtin_nanf("");
  float nf[3] = {qnan, qnan, qnan};
  if (i >= 1 && i < rows - 1 && j >= 1 && j < cols - 1) {  // (all four neighbours lie inside the map)
    const size_t R = (size_t)rows;
    const double c = (double)elev[o], t = (double)elev[o - 1], bt = (double)elev[o + 1], l = (double)elev[o - R], r = (double)elev[o + R];
    double gx, gy;
    if (raster_gradient(t, c, bt, res, gx) && raster_gradient(l, c, r, res, gy)) {
      const double xx = gx * gx, yy = gy * gy;
      const double s = xx + yy;
      const double norm = sqrt(s + 1.0);
      double n0 = gx / norm, n1 = gy / norm, n2 = 1.0 / norm;
      const double on_axis = axis == 0 ? n0 : (axis == 1 ? n1 : n2);
      if (on_axis < 0.0) {
        n0 = -n0;
        n1 = -n1;
        n2 = -n2;
      }
      nf[0] = (float)n0;
      nf[1] = (float)n1;
      nf[2] = (float)n2;
    }
  }
  onx[o] = nf[0];
  ony[o] = nf[1];
  onz[o] = nf[2];
  if (SLOPE) slope[o] = __builtin_isfinite(nf[2]) ? slope_score(nf[2], slope_crit) : qnan;  // SlopeFilter.cpp:71-81
}

}  // namespace

// k_normals_raster on every cell of every map; slope: the chain form (nullptr: the normals alone)
hipError_t normals_raster(const Geo& g, int axis, double slope_crit, const float* elev, float* nx, float* ny, float* nz, float* slope,
                          hipStream_t s) {
  const long long nbx = ((long long)g.rows + kRasterRows - 1) / kRasterRows, nby = ((long long)g.cols + kRasterCols - 1) / kRasterCols;
  const long long blocks = nbx * nby * (long long)g.batch;
  if (g.rows <= 0 || g.cols <= 0 || g.batch <= 0 || blocks > 0x7fffffffll) return hipErrorInvalidValue;
  const dim3 grid((unsigned)blocks), blk(kRasterRows, kRasterCols);
  if (slope)
    hipLaunchKernelGGL(k_normals_raster<true>, grid, blk, 0, s, g.rows, g.cols, (int)nbx, (int)nby, g.res, axis, slope_crit, elev, nx, ny, nz, slope);
  else
    hipLaunchKernelGGL(k_normals_raster<false>, grid, blk, 0, s, g.rows, g.cols, (int)nbx, (int)nby, g.res, axis, slope_crit, elev, nx, ny, nz,
                       (float*)nullptr);
  return hipGetLastError();
}

}  // namespace fast
}  // namespace te
