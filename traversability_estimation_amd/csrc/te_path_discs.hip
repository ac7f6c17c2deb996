// te_path_discs.hip -- circular path checks at each path's own radius, evaluated on demand (te_check_footprint_paths_radius).
//
// checkCircularFootprintPath (TraversabilityMap.cpp:345-462) takes path.radius from every FootprintPath and calls
// isTraversable(centre, radius + 0.15, .., radius) at the centres the path visits; with traversability_footprint all-NaN
// (computeTraversability leaves it so) every centre takes the on-demand branch (:679-736): one SpiralIterator walk, memoised.
// Three kernels on the context's stream do the same for a batch of paths with mixed radii, without a footprint layer:
//
//   k_pd_visit  one thread per path: the enumeration of te_path_visit.h (LineIt, pos_to_index of te_geom.h).  Every visited
//               centre gives a key (radius class, cell), inserted into an open-addressing table of 64-bit keys with atomicCAS;
//               the first insertion of a key appends its slot to the work list.  This table is the memo of the call: a disc
//               is evaluated once however many paths visit it.  Its size follows the number of visits, not the map.
//   k_pd_discs  one wavefront per listed disc (persistent grid): the spiral table of the disc's radius class (te_fp_table.h:
//               the tables and ties of the footprint pass at any reach), 64 entries per trip.  Every lane tests the
//               untraversable mask of its entry, a ballot finds the first untraversable entry in iterator order, the entries
//               before it are summed in double (invalid cells count as traversabilityDefault_).  Then the reference's three
//               outcomes: 0 (radiusMin == 0, or the cell within radiusMin: :694-704), the factor-scaled mean (:705-711), the
//               plain mean (:732-735), rounded to float as the memo store does (static_cast<float>) and kept beside the key.
//               (The lanes add their own entries and the wavefront's partial sums are folded at the end: the association of
//               the double sum differs from the serial one, by a few ulp of double before the rounding to float.)
//   k_pd_paths  one thread per path: the walk k_check_circular_paths does (te_path_walk.h: one body for both) with every
//               centre's value looked up by its key instead of read from a layer.
// The mask is the whole-map isTraversableForFilters mask of k_fp_mask (te_footprint.hip): it does not depend on the radius.
// Not covered: publishPolygons, and the untraversable polygon of the on-demand branch (the hull at :729).
#include "te_geom.h"
#include "te_internal.h"
#include "te_path_visit.h"
#include "te_path_walk.h"

namespace te {
namespace {

constexpr int kLanes = 64;
constexpr int kWavesPerBlock = 4;

struct DevGeom {  // te_path_visit.h's G on the device
  Geo g;
  using Line = LineIt;
  __device__ __forceinline__ bool inside(double x, double y) const { return pos_inside(g, x, y); }
  __device__ __forceinline__ bool to_index(double x, double y, int& i, int& j) const { return pos_to_index(g, x, y, i, j); }
};

__device__ __forceinline__ float qnanf() { return __builtin_nanf(""); }

// slot of `key`, inserting it if it is new (then the slot joins the work list); a full table or list sets the overflow flag
__device__ __forceinline__ void insert_key(const PathDiscScratch& s, uint64_t key) {
  unsigned long long* keys = reinterpret_cast<unsigned long long*>(s.keys);
  uint64_t h = pv::hash_key(key) & s.mask;
  for (uint64_t probe = 0; probe <= s.mask; ++probe) {
    const unsigned long long prev = atomicCAS(&keys[h], (unsigned long long)pv::kEmptyKey, (unsigned long long)key);
    if (prev == (unsigned long long)pv::kEmptyKey) {
      const unsigned at = atomicAdd(&s.counters[kPdDiscs], 1u);
      if (at < s.list_cap)
        s.list[at] = (unsigned)h;
      else
        atomicOr(&s.counters[kPdOverflow], 1u);
      return;
    }
    if (prev == (unsigned long long)key) return;
    h = (h + 1) & s.mask;
  }
  atomicOr(&s.counters[kPdOverflow], 1u);
}

// the value kept for `key` (every key a path looks up was inserted by k_pd_visit; NaN if it was not)
__device__ __forceinline__ double lookup_key(const PathDiscScratch& s, uint64_t key) {
  uint64_t h = pv::hash_key(key) & s.mask;
  for (uint64_t probe = 0; probe <= s.mask; ++probe) {
    const uint64_t k = s.keys[h];
    if (k == key) return (double)s.vals[h];
    if (k == pv::kEmptyKey) break;
    h = (h + 1) & s.mask;
  }
  return (double)qnanf();
}

__global__ __launch_bounds__(256) void k_pd_visit(Geo g, PathDiscScratch s, int n_paths, const int* __restrict__ pose_offset,
                                                  const double* __restrict__ pose_xy, const int* __restrict__ path_class) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n_paths) return;
  const int p0 = pose_offset[k], n = pose_offset[k + 1] - p0;
  const unsigned cls = (unsigned)path_class[k];
  const DevGeom G{g};
  unsigned visits = 0;
  pv::visit_path(G, n, pose_xy + 2 * (size_t)p0, [&](int i, int j) {
    // (to_index accepted the ends of the line, so its cells lie inside the map)
    insert_key(s, pv::pack_key(cls, i, j, g.rows));
    ++visits;
  });
  if (visits) atomicAdd(&s.counters[kPdVisits], visits);
}

__global__ __launch_bounds__(kLanes* kWavesPerBlock) void k_pd_discs(Geo g, PathDiscScratch s, const PathDiscClass* __restrict__ classes,
                                                                   const float* __restrict__ trav, const uint8_t* __restrict__ untrav,
                                                                   double def) {
  const int lane = threadIdx.x & (kLanes - 1);
  const unsigned wave = blockIdx.x * kWavesPerBlock + threadIdx.x / kLanes;
  const unsigned n_waves = gridDim.x * kWavesPerBlock;
  unsigned n_discs = s.counters[kPdDiscs];
  n_discs = n_discs < s.list_cap ? n_discs : s.list_cap;
  for (unsigned d = wave; d < n_discs; d += n_waves) {  // (uniform per wavefront)
    const unsigned slot = s.list[d];
    const uint64_t key = s.keys[slot];
    const PathDiscClass c = classes[pv::key_class(key)];
    const uint64_t cell = pv::key_cell(key);
    const int jc = (int)(cell / (uint64_t)g.rows), ic = (int)(cell - (uint64_t)jc * (uint64_t)g.rows);
    double acc = 0.0;
    int cnt = 0;
    float out = qnanf();
    bool blocked = false;
    for (int k0 = 0; k0 < c.n_spiral; k0 += kLanes) {
      const int k = k0 + lane;
      int4 e = make_int4(0, 0, 0, 0);
      if (k < c.n_spiral) e = c.spiral[k];
      const int ii = ic + e.x, jj = jc + e.y;
      bool in = k < c.n_spiral && ii >= 0 && ii < g.rows && jj >= 0 && jj < g.cols;
      if (in && e.w) {  // on the circle: SpiralIterator::isInside per centre
        const double dx = cell_x(g, ii) - cell_x(g, ic), dy = cell_y(g, jj) - cell_y(g, jc);
        in = dx * dx + dy * dy <= c.r2;
      }
      double v = 0.0;
      bool u = false;
      if (in) {
        const size_t o = (size_t)jj * g.rows + ii;
        const float tv = trav[o];
        v = __builtin_isfinite(tv) ? (double)tv : def;  // :719-724
        u = untrav[o] != 0;
      }
      const unsigned long long bm = __ballot(in && u);
      if (bm != 0ull) {  // the first untraversable cell in iterator order
        blocked = true;
        const int first = __builtin_ctzll(bm);
        const double ru = (double)__shfl(e.z, first) * g.res;  // getCurrentRadius()
        if (c.rmin == 0.0 || ru <= c.rmin) {                   // :694-704
          out = 0.0f;
        } else {  // :705-711
          const bool before = in && lane < first;
          acc += before ? v : 0.0;
          cnt += __popcll(__ballot(before));
#pragma unroll
          for (int sh = 32; sh >= 1; sh >>= 1) acc += __shfl_xor(acc, sh);
          const double factor = ((ru - c.rmin) / (c.rmax - c.rmin) + 1.0) / 2.0;
          out = (float)(acc * (factor / cnt));
        }
        break;
      }
      acc += in ? v : 0.0;
      cnt += __popcll(__ballot(in));
    }
    if (!blocked) {  // :732-735 (the centre is a cell of the map: cnt >= 1)
#pragma unroll
      for (int sh = 32; sh >= 1; sh >>= 1) acc += __shfl_xor(acc, sh);
      out = (float)(acc / (double)cnt);
    }
    if (lane == 0) s.vals[slot] = out;
  }
}

__global__ __launch_bounds__(256) void k_pd_paths(Geo g, PathDiscScratch s, double fp_default, const float* __restrict__ robot_slope,
                                                  int n_paths, const int* __restrict__ pose_offset, const double* __restrict__ pose_xy,
                                                  const int* __restrict__ path_class, unsigned char* __restrict__ is_safe,
                                                  double* __restrict__ traversability, int* __restrict__ status) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n_paths) return;
  const int p0 = pose_offset[k], n = pose_offset[k + 1] - p0;
  const unsigned cls = (unsigned)path_class[k];
  unsigned char safe;
  double out;
  int st;
  check_circular_path(g, robot_slope, fp_default, n, pose_xy + 2 * (size_t)p0,
                      [&](int i, int j) { return lookup_key(s, pv::pack_key(cls, i, j, g.rows)); }, safe, out, st);
  is_safe[k] = safe;
  traversability[k] = out;
  status[k] = st;
}

}  // namespace

hipError_t launch_path_discs(const Geo& g, const PathDiscScratch& s, const PathDiscClass* classes, const float* trav, const uint8_t* untrav,
                             double fp_default, const float* robot_slope, int n_paths, const int* pose_offset, const double* pose_xy,
                             const int* path_class, unsigned char* is_safe, double* traversability, int* status, hipStream_t stream) {
  if (n_paths <= 0) return hipSuccess;
  const dim3 per_path((unsigned)((n_paths + 255) / 256));
  hipLaunchKernelGGL(k_pd_visit, per_path, dim3(256), 0, stream, g, s, n_paths, pose_offset, pose_xy, path_class);
  // persistent grid: a wavefront per listed disc up to eight blocks per compute unit, the rest in turns
  const unsigned want = (s.list_cap + kWavesPerBlock - 1) / kWavesPerBlock, most = (unsigned)device_cus() * 8u;
  const unsigned blocks = want < most ? (want > 0 ? want : 1u) : most;
  hipLaunchKernelGGL(k_pd_discs, dim3(blocks), dim3(kLanes * kWavesPerBlock), 0, stream, g, s, classes, trav, untrav, fp_default);
  hipLaunchKernelGGL(k_pd_paths, per_path, dim3(256), 0, stream, g, s, fp_default, robot_slope, n_paths, pose_offset, pose_xy, path_class,
                     is_safe, traversability, status);
  return hipGetLastError();
}

}  // namespace te
