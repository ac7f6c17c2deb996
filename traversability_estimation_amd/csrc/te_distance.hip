// te_distance.hip -- the two passes of te_run_distance (include/travgpu.h).  Per-cell arithmetic: te_distance.h; rectangles, route
// and launch geometry: te_distance_plan.h.  Layers are column-major: cell (i, j) of a map is element j * rows + i, so a
// wavefront's 64 lanes always hold 64 consecutive rows of one column and every access below is 64 consecutive elements.
// No atomics and no waits between workgroups; the batch rides on blockIdx.z.
#include "te_distance_launch.h"

namespace te {
namespace distance {

namespace {

// Pass 1.  One wavefront per segment of a column: it walks its rows in chunks of 64 -- the R rows before the segment, the
// segment, then the rows behind it until the first seed -- and takes the seeds of a chunk as a ballot.  Lane c keeps the mask of
// the segment's c-th chunk and the distance from its first row to the last seed before it; the way back hands every chunk
// the first seed behind it, and column_nearest settles the cell.  Every cell of the input is read once per wavefront.
__global__ __launch_bounds__(kThreads) void k_distance_columns(Plan p, const float* __restrict__ in_all, uint16_t* __restrict__ g_all, int mode, float threshold) {
  const int lane = threadIdx.x & (kLanes - 1), wave = threadIdx.x / kLanes;
  int i0, i1, j;
  if (!p1_unit(p, blockIdx.x, wave, &i0, &i1, &j)) return;  // (the whole wavefront)
  const float* __restrict__ in = in_all + ((size_t)blockIdx.z * p.cols + j) * (size_t)p.rows;
  const size_t gh = (size_t)region::height(p.g);
  uint16_t* __restrict__ g = g_all + (size_t)blockIdx.z * p.g_cells + (size_t)(j - p.g.j0) * gh;
  const int sat = p.R + 1;
  // rows of the input this column may be read at: [low, high), inside the map
  const long long low = (long long)i0 - p.R > p.in.i0 ? (long long)i0 - p.R : p.in.i0, high = p.in.i1;

  long long last = -(1ll << 40);  // row of the last seed seen
  for (long long row0 = i0 - ((i0 - low + kLanes - 1) / kLanes) * kLanes; row0 < i0; row0 += kLanes) {
    const long long row = row0 + lane;
    const unsigned long long m = __ballot(row >= low && is_seed(in[row >= low ? row : low], mode, threshold));
    if (m) last = row0 + 63 - __builtin_clzll(m);
  }
  const int nown = (i1 - i0 + kLanes - 1) / kLanes;  // <= kMaxSegChunks
  unsigned long long my_mask = 0;
  int my_before = kNone;
  for (int c = 0; c < nown; ++c) {
    const long long row0 = (long long)i0 + (long long)c * kLanes, row = row0 + lane;
    // (the rows of the last chunk behind i1 are the first rows of the halo)
    const unsigned long long m = __ballot(row < high && is_seed(in[row < high ? row : high - 1], mode, threshold));
    const long long d = row0 - last;
    if (lane == c) my_mask = m, my_before = d < kNone ? (int)d : kNone;
    if (m) last = row0 + 63 - __builtin_clzll(m);
  }
  long long next = 1ll << 40;  // row of the first seed behind the chunk in hand
  for (long long row0 = (long long)i0 + (long long)nown * kLanes; row0 < high && row0 < (long long)i1 + p.R; row0 += kLanes) {
    const long long row = row0 + lane;
    const unsigned long long m = __ballot(row < high && is_seed(in[row < high ? row : high - 1], mode, threshold));
    if (m) {
      next = row0 + __builtin_ctzll(m);
      break;
    }
  }
  for (int c = nown - 1; c >= 0; --c) {
    const long long row0 = (long long)i0 + (long long)c * kLanes, row = row0 + lane;
    const unsigned long long m = __shfl(my_mask, c);
    const int before = __shfl(my_before, c);
    const long long d = next - (row0 + kLanes - 1);
    const int v = column_nearest(m, lane, before, d < kNone ? (int)d : kNone, sat);
    if (row < i1) g[row - p.g.i0] = (uint16_t)v;
    if (m) next = row0 + __builtin_ctzll(m);
  }
}

// Pass 2.  A workgroup owns a tile of 64 rows x 64 columns of out; lane l of wavefront w owns row l of it and the columns
// w, w + 4, ... .  kTiled: the tile's rows of g, with R columns on either side, are staged in LDS as [column][64 rows] first.
template <bool kTiled>
__global__ __launch_bounds__(kThreads) void k_distance_rows(Plan p, const uint16_t* __restrict__ g_all, float* __restrict__ out_all, double res, float beyond) {
  extern __shared__ uint16_t lds_g[];
  const int lane = threadIdx.x & (kLanes - 1), wave = threadIdx.x / kLanes;
  int i0, j0, c0, c1;
  p2_tile(p, blockIdx.x, &i0, &j0);
  p2_columns(p, j0, &c0, &c1);
  const int i = i0 + lane;
  const bool row_ok = i < p.out.i1;
  const size_t gh = (size_t)region::height(p.g);  // (the rows of g are those of out)
  const uint16_t* __restrict__ g = g_all + (size_t)blockIdx.z * p.g_cells + (size_t)(row_ok ? i - p.g.i0 : 0);
  if (kTiled) {
    for (int c = c0 + wave; c < c1; c += kWaves) lds_g[(size_t)(c - c0) * kTI + lane] = row_ok ? g[(size_t)(c - p.g.j0) * gh] : (uint16_t)0;
    __syncthreads();
  }
  if (!row_ok) return;
  float* __restrict__ out = out_all + (size_t)blockIdx.z * (size_t)p.rows * (size_t)p.cols + (size_t)i;
  for (int k = 0; k < kCellsPerLane; ++k) {
    int ci, j;
    if (!p2_cell(p, i0, j0, wave, lane, k, &ci, &j)) break;
    const int lo = j - c0 < p.R ? j - c0 : p.R, hi = c1 - 1 - j < p.R ? c1 - 1 - j : p.R;
    const uint32_t d2 = kTiled ? row_min(&lds_g[(size_t)(j - c0) * kTI + lane], (ptrdiff_t)kTI, lo, hi, p.cap2 + 1u)
                               : row_min(g + (size_t)(j - p.g.j0) * gh, (ptrdiff_t)gh, lo, hi, p.cap2 + 1u);
    out[(size_t)j * (size_t)p.rows] = value_of(d2, p.cap2, res, beyond);
  }
}

}  // namespace

hipError_t launch(const Plan& p, const Args& a, int passes, hipStream_t stream, unsigned long long counts[2]) {
  if (counts) counts[0] = counts[1] = 0;
  if (a.nmaps <= 0) return hipSuccess;
  const region::Rect& o = p.out;
  if (!p.fits || a.nmaps > 65535 || o.i0 < 0 || o.j0 < 0 || o.i0 >= o.i1 || o.j0 >= o.j1 || o.i1 > p.rows || o.j1 > p.cols) return hipErrorInvalidValue;
  const dim3 block(kThreads);
  if (passes & kPass1)
    hipLaunchKernelGGL(k_distance_columns, dim3((unsigned)p.p1_blocks, 1, (unsigned)a.nmaps), block, 0, stream, p, a.in, a.g, a.mode, a.threshold);
  if (passes & kPass2) {
    const dim3 grid((unsigned)p.p2_blocks, 1, (unsigned)a.nmaps);
    if (p.route == kRouteTiled)
      hipLaunchKernelGGL(k_distance_rows<true>, grid, block, p.lds_bytes, stream, p, a.g, a.out, a.res, a.beyond);
    else
      hipLaunchKernelGGL(k_distance_rows<false>, grid, block, 0, stream, p, a.g, a.out, a.res, a.beyond);
    if (counts) counts[p.route == kRouteTiled ? 0 : 1] = p.p2_blocks * (unsigned long long)a.nmaps;
  }
  return hipGetLastError();
}

}  // namespace distance
}  // namespace te
