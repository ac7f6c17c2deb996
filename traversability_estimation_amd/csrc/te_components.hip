// te_components.hip -- the launches of te_run_components / te_run_reachable (include/travgpu.h).  Per-run and union routines:
// te_components.h; tiles, seams and grids: te_components_plan.h.  Layers are column-major: cell (i, j) of a map is element
// j * rows + i, so a wavefront's 64 lanes hold 64 consecutive rows of one column.
// No workgroup waits for another one, no launch depends on what the map holds, and the only atomics are integer ones.  What
// workgroups share inside one launch -- the labels in the seam pass and in flatten, the counts, the four totals -- is touched
// through Atomic<agent> alone; plain loads read what an earlier launch wrote.  The batch rides on blockIdx.z.
#include "te_components.h"
#include "te_components_launch.h"

namespace te {
namespace components {

namespace {

using Lds = Atomic<__HIP_MEMORY_SCOPE_WORKGROUP>;
using Dev = Atomic<__HIP_MEMORY_SCOPE_AGENT>;
constexpr int kColsPerWave = kTJ / kWaves;

// Tile pass.  One workgroup labels one tile in LDS: a wavefront takes every fourth column, its ballot is the column's mask.
// Out: the label of every cell (the smallest linear index of its tile-local component, kBlocked for a blocked cell) and its
// count (the cells of the tile-local component at that smallest cell, 0 elsewhere).
__global__ __launch_bounds__(kThreads) void k_components_tile(Plan p, const float* __restrict__ in_all, uint32_t* __restrict__ L_all, uint32_t* __restrict__ S_all,
                                                              int mode, float threshold, int connectivity) {
  __shared__ uint32_t lab[kTJ * kLanes];
  __shared__ uint32_t cnt[kTJ * kLanes];
  __shared__ unsigned long long msk[kTJ];
  const int lane = threadIdx.x & (kLanes - 1), wave = threadIdx.x / kLanes;
  int i0, j0;
  tile_origin(p, blockIdx.x, &i0, &j0);
  const size_t map = (size_t)blockIdx.z * (size_t)p.cells;
  const float* __restrict__ in = in_all + map;
  const int i = i0 + lane;
  const bool row_ok = lane < p.ti && i < p.rows;
  const int nc = p.cols - j0 < p.tj ? p.cols - j0 : p.tj;
  for (int c = wave; c < nc; c += kWaves) {
    const float v = row_ok ? in[(size_t)(j0 + c) * (size_t)p.rows + (size_t)i] : 0.0f;
    const unsigned long long m = __ballot(row_ok && is_free(v, mode, threshold));
    if (lane == 0) msk[c] = m;
    lab[c * kLanes + lane] = tile_first_label(m, c, lane);
    cnt[c * kLanes + lane] = 0;
  }
  __syncthreads();
  for (int c = wave < 1 ? wave + kWaves : wave; c < nc; c += kWaves) tile_unite_lane<Lds>(lab, c, lane, msk[c], msk[c - 1], connectivity);
  __syncthreads();
  uint32_t root[kColsPerWave];
#pragma unroll
  for (int k = 0; k < kColsPerWave; ++k) {
    const int c = wave + k * kWaves;
    root[k] = kBlocked;
    if (c >= nc) continue;
    const unsigned long long m = msk[c];
    const uint32_t t = lab[c * kLanes + lane];
    if (t == kBlocked) continue;
    root[k] = find<Lds>(lab, t);
    // one add per run of the column, with its length
    if ((run_starts(m) >> lane) & 1ull) Lds::fetch_add(&cnt[root[k]], (uint32_t)run_length(m, lane));
  }
  __syncthreads();
  if (!row_ok) return;
  uint32_t* __restrict__ L = L_all + map;
  uint32_t* __restrict__ S = S_all + map;
#pragma unroll
  for (int k = 0; k < kColsPerWave; ++k) {
    const int c = wave + k * kWaves;
    if (c >= nc) continue;
    const size_t x = (size_t)(j0 + c) * (size_t)p.rows + (size_t)i;
    const uint32_t r = root[k];
    L[x] = r == kBlocked ? kBlocked : (uint32_t)((size_t)(j0 + (int)(r / kLanes)) * (size_t)p.rows + (size_t)(i0 + (int)(r % kLanes)));
    S[x] = cnt[c * kLanes + lane];
  }
}

// Seam pass: one thread per seam cell
__global__ __launch_bounds__(kThreads) void k_components_seams(Plan p, uint32_t* L_all, int connectivity) {
  const unsigned long long u = (unsigned long long)blockIdx.x * kThreads + threadIdx.x;
  if (u >= p.seam_cells) return;
  uint32_t* L = L_all + (size_t)blockIdx.z * (size_t)p.cells;
  bool col_seam;
  int i, j;
  seam_cell(p, u, &col_seam, &i, &j);
  if (col_seam)
    seam_col_cell<Dev>(L, p.rows, p.ti, i, j, connectivity);
  else
    seam_row_cell<Dev>(L, p.rows, p.cols, p.tj, i, j, connectivity);
}

// Flatten + count: one thread per cell
__global__ __launch_bounds__(kThreads) void k_components_flatten(Plan p, uint32_t* L_all, uint32_t* S_all) {
  const unsigned long long x = (unsigned long long)blockIdx.x * kThreads + threadIdx.x;
  if (x >= p.cells) return;
  const size_t map = (size_t)blockIdx.z * (size_t)p.cells;
  flatten_cell<Dev>(L_all + map, S_all + map, (uint32_t)x);
}

// The starts of te_run_reachable: a flag at the root of every start on a free cell (one map)
__global__ __launch_bounds__(kThreads) void k_components_starts(Starts s, const uint32_t* __restrict__ L, uint32_t* S) {
  const int k = threadIdx.x;
  if (k >= s.n) return;
  const uint32_t r = L[s.cell[k]];
  if (r != kBlocked) Dev::fetch_or(S + r, kFlag);
}

// Write, and the four totals: components (roots), free cells, the largest component, cells written 1.0f
template <bool kReach>
__global__ __launch_bounds__(kThreads) void k_components_write(Plan p, const uint32_t* __restrict__ L_all, const uint32_t* __restrict__ S_all, float* __restrict__ out_all,
                                                               unsigned long long* counts) {
  __shared__ uint32_t acc[4];
  if (threadIdx.x < 4) acc[threadIdx.x] = 0;
  __syncthreads();
  const size_t map = (size_t)blockIdx.z * (size_t)p.cells;
  const uint32_t* __restrict__ L = L_all + map;
  const uint32_t* __restrict__ S = S_all + map;
  float* __restrict__ out = out_all + map;
  uint32_t n_roots = 0, n_free = 0, largest = 0, n_ones = 0;
  const unsigned long long stride = (unsigned long long)gridDim.x * kThreads;
  for (unsigned long long x = (unsigned long long)blockIdx.x * kThreads + threadIdx.x; x < p.cells; x += stride) {
    const uint32_t t = L[x];
    const float v = kReach ? reach_value(t, S) : size_value(t, S);
    out[x] = v;
    if (t == kBlocked) continue;
    ++n_free;
    if (kReach && v != 0.0f) ++n_ones;
    if (t == (uint32_t)x) {
      ++n_roots;
      const uint32_t n = S[t] & ~kFlag;
      largest = n > largest ? n : largest;
    }
  }
  if (n_roots) Lds::fetch_add(&acc[0], n_roots);
  if (n_free) Lds::fetch_add(&acc[1], n_free);
  if (largest) __hip_atomic_fetch_max(&acc[2], largest, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  if (n_ones) Lds::fetch_add(&acc[3], n_ones);
  __syncthreads();
  if (threadIdx.x == 0) {
    if (acc[0]) __hip_atomic_fetch_add(counts + 0, (unsigned long long)acc[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (acc[1]) __hip_atomic_fetch_add(counts + 1, (unsigned long long)acc[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (acc[2]) __hip_atomic_fetch_max(counts + 2, (unsigned long long)acc[2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (acc[3]) __hip_atomic_fetch_add(counts + 3, (unsigned long long)acc[3], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

}  // namespace

hipError_t launch(const Plan& p, const Args& a, const Starts* starts, hipStream_t stream) {
  if (a.nmaps <= 0) return hipSuccess;
  if (!p.fits || a.nmaps > 65535 || p.ti != kTI || p.tj != kTJ || (starts && (a.nmaps != 1 || starts->n < 1 || starts->n > kMaxStarts))) return hipErrorInvalidValue;
  if (starts)
    for (int k = 0; k < starts->n; ++k)
      if (starts->cell[k] >= p.cells) return hipErrorInvalidValue;
  uint32_t* const L = (uint32_t*)a.scratch;
  uint32_t* const S = L + (size_t)p.cells * (size_t)a.nmaps;
  const dim3 block(kThreads);
  const unsigned z = (unsigned)a.nmaps;
  hipError_t e = hipMemsetAsync(a.counts, 0, 4 * sizeof(unsigned long long), stream);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_components_tile, dim3((unsigned)p.tile_blocks, 1, z), block, 0, stream, p, a.in, L, S, a.mode, a.threshold, a.connectivity);
  if (p.seam_blocks) hipLaunchKernelGGL(k_components_seams, dim3((unsigned)p.seam_blocks, 1, z), block, 0, stream, p, L, a.connectivity);
  hipLaunchKernelGGL(k_components_flatten, dim3((unsigned)p.flat_blocks, 1, z), block, 0, stream, p, L, S);
  if (starts) {
    hipLaunchKernelGGL(k_components_starts, dim3(1), block, 0, stream, *starts, (const uint32_t*)L, S);
    hipLaunchKernelGGL(k_components_write<true>, dim3(p.write_blocks, 1, z), block, 0, stream, p, (const uint32_t*)L, (const uint32_t*)S, a.out, a.counts);
  } else {
    hipLaunchKernelGGL(k_components_write<false>, dim3(p.write_blocks, 1, z), block, 0, stream, p, (const uint32_t*)L, (const uint32_t*)S, a.out, a.counts);
  }
  return hipGetLastError();
}

}  // namespace components
}  // namespace te
