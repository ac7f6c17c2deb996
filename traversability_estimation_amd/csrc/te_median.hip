// te_median.hip -- the kernels of te_run_median_fill (include/travgpu.h: MedianFillFilter), gfx950.
//
//   mask passes      bytes, one lane per cell: k_mask_valid (finite cells), k_mask_morph (one 3x3 erosion or dilation, cells
//                    outside the map do not vote), k_mask_or (the window OR along one axis; two launches make the square).
//   k_median_tile    the hot path: one workgroup per 64 x 16 tile.  It stages the tile and a halo of r cells as keys in LDS,
//                    copies through every cell that keeps its value, compacts the cells that need a median into an LDS list
//                    (ballot + prefix, in a fixed order), and then whole wavefronts take cells from that list: each lane selects
//                    one cell's median by bisection over the 32 key bits (te_median.h), every step a count over its window in
//                    LDS.  One kernel for every r the plan gives it (te_median_plan.h); r arrives as an argument.
//   k_median_any     every other window: k_any_count / k_any_scan / k_any_list compact the cells that need a median into a
//                    list in memory order (a count per 256 cells, one workgroup scans the counts, the cells are written at
//                    their offsets), and one wavefront per listed cell strides over the clamped window in global memory; the
//                    counts are wave-wide ballots.  Same bisection, same result.
// No atomics, no floating-point arithmetic on the values: the output is a function of the input alone.
//
// Region form (te_run_median_fill_region; the rectangles: te_region_plan.h): the k_*_rect mask passes run one lane per cell
// of the rectangle their stage is planned on, in map coordinates on the same scratch; k_median_tile takes the origin of its
// tile grid and the end of the cells it owns (the whole-map launch passes the map's), and the general route compacts the
// cells of the rectangle alone (k_any_count / k_any_list with RECT).  Nothing in a region launch is sized by the map.
//
// Bounds: every global index is formed from a cell (i, j) with 0 <= i < rows, 0 <= j < cols checked where it is formed, and
// a map index below nmaps; LDS indices lie in the staged rectangle because a listed cell is a tile cell and rr <= r.
#include "te_median.h"
#include "te_median_launch.h"

namespace te {
namespace median {
namespace {

constexpr int kMaskBlock = 256;

__device__ __forceinline__ unsigned lane_id() { return threadIdx.x & 63u; }

__global__ __launch_bounds__(kMaskBlock) void k_mask_valid(const float* __restrict__ in, uint8_t* __restrict__ v, size_t total) {
  const size_t idx = (size_t)blockIdx.x * kMaskBlock + threadIdx.x;
  if (idx < total) v[idx] = finite_bits(float_bits(in[idx])) ? 1 : 0;
}

// erode: a cell stays set if all of its in-map 3x3 neighbours are set; dilate: a cell is set if any of them is
__device__ __forceinline__ uint8_t morph_cell(const uint8_t* __restrict__ s, int rows, int cols, int i, int j, int erode) {
  const int i0 = i > 0 ? i - 1 : 0, i1 = i < rows - 1 ? i + 1 : rows - 1;
  const int j0 = j > 0 ? j - 1 : 0, j1 = j < cols - 1 ? j + 1 : cols - 1;
  int all = 1, any = 0;
  for (int jj = j0; jj <= j1; ++jj)
    for (int ii = i0; ii <= i1; ++ii) {
      const int b = s[(size_t)jj * rows + ii] != 0;
      all &= b;
      any |= b;
    }
  return (uint8_t)(erode ? all : any);
}
__global__ __launch_bounds__(kMaskBlock) void k_mask_morph(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int rows, int cols,
                                                           size_t total, int erode) {
  const size_t idx = (size_t)blockIdx.x * kMaskBlock + threadIdx.x;
  if (idx >= total) return;
  const size_t cells = (size_t)rows * cols;
  const size_t cell = idx % cells;
  dst[idx] = morph_cell(src + (idx - cell), rows, cols, (int)(cell % rows), (int)(cell / rows), erode);
}

// OR of s over [x - r, x + r] clamped, x the row index (along_rows) or the column index
__device__ __forceinline__ uint8_t or_cell(const uint8_t* __restrict__ s, int rows, int cols, int i, int j, int r, int along_rows) {
  int any = 0;
  if (along_rows) {
    const int i0 = i > r ? i - r : 0, i1 = (rows - 1 - i > r) ? i + r : rows - 1;
    const uint8_t* const col = s + (size_t)j * rows;
    for (int ii = i0; ii <= i1 && !any; ++ii) any = col[ii] != 0;
  } else {
    const int j0 = j > r ? j - r : 0, j1 = (cols - 1 - j > r) ? j + r : cols - 1;
    for (int jj = j0; jj <= j1 && !any; ++jj) any = s[(size_t)jj * rows + i] != 0;
  }
  return (uint8_t)any;
}
__global__ __launch_bounds__(kMaskBlock) void k_mask_or(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int rows, int cols, size_t total,
                                                        int r, int along_rows) {
  const size_t idx = (size_t)blockIdx.x * kMaskBlock + threadIdx.x;
  if (idx >= total) return;
  const size_t cells = (size_t)rows * cols;
  const size_t cell = idx % cells;
  dst[idx] = or_cell(src + (idx - cell), rows, cols, (int)(cell % rows), (int)(cell / rows), r, along_rows);
}

// The same passes over one rectangle of one map (te_region_plan.h), one lane per cell of `q`, which lies in the map: src
// and dst are that map's bytes, indexed by map cell.  what: 0 V of `in`, 1 an erosion, 2 a dilation, 3 / 4 the OR along the
// rows / the columns.
__global__ __launch_bounds__(kMaskBlock) void k_mask_rect(const float* __restrict__ in, const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int rows,
                                                          int cols, region::Rect q, int what, int r) {
  const size_t k = (size_t)blockIdx.x * kMaskBlock + threadIdx.x;
  if (k >= region::cells(q)) return;
  int i, j;
  region::cell_of(q, k, &i, &j);
  if (i < 0 || i >= rows || j < 0 || j >= cols) return;  // (never: q lies in the map)
  const size_t g = (size_t)j * rows + i;
  uint8_t v;
  if (what == 0)
    v = finite_bits(float_bits(in[g])) ? 1 : 0;
  else if (what <= 2)
    v = morph_cell(src, rows, cols, i, j, what == 1);
  else
    v = or_cell(src, rows, cols, i, j, r, what == 3);
  dst[g] = v;
}

// what a cell does, from its value and its mask byte: 0 keeps its value, 1 takes the median of its window
__device__ __forceinline__ bool needs_median(uint32_t bits, uint8_t should_fill, int r_exist) {
  return should_fill && (!finite_bits(bits) || r_exist >= 0);
}

__global__ __launch_bounds__(kTileThreads) void k_median_tile(const float* __restrict__ in, float* __restrict__ out, const uint8_t* __restrict__ mask,
                                                              int rows, int cols, int tiles_x, int tiles_y, int r, int r_fill, int r_exist,
                                                              int oi0, int oj0, int i_end, int j_end) {
  extern __shared__ uint32_t s_keys[];  // [h][w], w along the rows; then the list
  __shared__ int s_cnt[16];
  const int w = kTileRows + 2 * r, h = kTileCols + 2 * r;
  uint16_t* const s_list = (uint16_t*)(s_keys + (size_t)w * h);
  const size_t cells = (size_t)rows * cols;
  const unsigned b = blockIdx.x;
  const int tx = (int)(b % (unsigned)tiles_x), ty = (int)((b / (unsigned)tiles_x) % (unsigned)tiles_y);
  const size_t map = b / ((unsigned)tiles_x * (unsigned)tiles_y);
  in += map * cells;
  out += map * cells;
  mask += map * cells;
  const int tid = (int)threadIdx.x;

  // the tile and its halo as keys; cells outside the map hold kNoKey like every cell that is not finite
  const int gi0 = oi0 + tx * kTileRows - r, gj0 = oj0 + ty * kTileCols - r;
  for (int e = tid; e < w * h; e += kTileThreads) {
    const int li = e % w, lj = e / w;
    const int gi = gi0 + li, gj = gj0 + lj;
    uint32_t key = kNoKey;
    if (gi >= 0 && gi < rows && gj >= 0 && gj < cols) key = float_key(in[(size_t)gj * rows + gi]);
    s_keys[e] = key;
  }

  // every lane owns four tile cells (row li, columns wave + 4 q): copy through, or vote for the list
  const int li = tid & 63, wave = tid >> 6;
  const int gi = oi0 + tx * kTileRows + li;  // (the tile grid starts at (oi0, oj0) and owns cells below (i_end, j_end) <= (rows, cols))
  unsigned long long votes[4];
  bool need[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int lj = wave + 4 * q;
    const int gj = oj0 + ty * kTileCols + lj;
    need[q] = false;
    if (gi < i_end && gj < j_end) {
      const size_t g = (size_t)gj * rows + gi;
      const float v = in[g];
      need[q] = needs_median(float_bits(v), mask[g], r_exist);
      if (!need[q]) out[g] = v;
    }
    votes[q] = __ballot(need[q]);
    if (lane_id() == 0) s_cnt[q * 4 + wave] = __popcll(votes[q]);
  }
  __syncthreads();
  int total = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int slot = q * 4 + wave;
    int base = 0;
    for (int s = 0; s < 16; ++s) {
      base += s < slot ? s_cnt[s] : 0;
      if (q == 0) total += s_cnt[s];
    }
    if (need[q]) s_list[base + __popcll(votes[q] & ((1ull << lane_id()) - 1ull))] = (uint16_t)((wave + 4 * q) * kTileRows + li);
  }
  __syncthreads();

  // whole wavefronts over the list, whatever the hole pattern was
  for (int e = tid; e < total; e += kTileThreads) {
    const int c = s_list[e];
    const int ci = c % kTileRows, cj = c / kTileRows;
    const uint32_t centre = s_keys[(size_t)(cj + r) * w + (ci + r)];
    const int rr = centre != kNoKey ? r_exist : r_fill;  // (a finite cell is listed only with r_exist >= 0)
    const uint32_t* const win = s_keys + (size_t)(cj + r - rr) * w + (ci + r - rr);
    const int side = 2 * rr + 1;
    const float m = median([&](uint32_t p) {
      unsigned n = 0;
      for (int dj = 0; dj < side; ++dj) {
        const uint32_t* const line = win + (size_t)dj * w;
        for (int di = 0; di < side; ++di) n += line[di] < p ? 1u : 0u;
      }
      return n;
    });
    out[(size_t)(oj0 + ty * kTileCols + cj) * rows + (oi0 + tx * kTileRows + ci)] = m;
  }
}

// ---- the general route, one map per launch ----

// copies through the cells that keep their value and counts the others per 256 cells
// (RECT: `cells` are those of the rectangle q of the map, rows fastest, and a cell's index in the layer comes from q)
template <bool RECT>
__device__ __forceinline__ size_t any_cell(size_t idx, int rows, const region::Rect& q) {
  if (!RECT) return idx;
  int i, j;
  region::cell_of(q, idx, &i, &j);
  return (size_t)j * rows + i;
}
template <bool RECT>
__global__ __launch_bounds__(kAnyBlock) void k_any_count(const float* __restrict__ in, float* __restrict__ out, const uint8_t* __restrict__ mask,
                                                         size_t cells, int r_exist, unsigned* __restrict__ counts, int rows, region::Rect q) {
  __shared__ int s_cnt[kAnyBlock / 64];
  const size_t idx = (size_t)blockIdx.x * kAnyBlock + threadIdx.x;
  bool need = false;
  if (idx < cells) {
    const size_t g = any_cell<RECT>(idx, rows, q);
    const float v = in[g];
    need = needs_median(float_bits(v), mask[g], r_exist);
    if (!need) out[g] = v;
  }
  const unsigned long long votes = __ballot(need);
  if (lane_id() == 0) s_cnt[threadIdx.x >> 6] = __popcll(votes);
  __syncthreads();
  if (threadIdx.x == 0) counts[blockIdx.x] = (unsigned)(s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3]);
}

// counts[0 .. n) -> their exclusive prefix sums, counts[n] = the total; one workgroup
__global__ __launch_bounds__(kAnyBlock) void k_any_scan(unsigned* __restrict__ counts, size_t n) {
  __shared__ unsigned s[2][kAnyBlock];
  __shared__ unsigned s_carry;
  const int tid = (int)threadIdx.x;
  if (tid == 0) s_carry = 0;
  __syncthreads();
  for (size_t base = 0; base < n; base += kAnyBlock) {
    const size_t k = base + tid;
    const unsigned v = k < n ? counts[k] : 0u;
    int cur = 0;
    s[0][tid] = v;
    __syncthreads();
    for (int d = 1; d < kAnyBlock; d <<= 1) {
      const unsigned t = s[cur][tid] + (tid >= d ? s[cur][tid - d] : 0u);
      s[cur ^ 1][tid] = t;
      cur ^= 1;
      __syncthreads();
    }
    const unsigned carry = s_carry;
    if (k < n) counts[k] = carry + s[cur][tid] - v;
    __syncthreads();
    if (tid == kAnyBlock - 1) s_carry = carry + s[cur][tid];
    __syncthreads();
  }
  if (tid == 0) counts[n] = s_carry;
}

// the cells that need a median, in memory order
template <bool RECT>
__global__ __launch_bounds__(kAnyBlock) void k_any_list(const float* __restrict__ in, const uint8_t* __restrict__ mask, size_t cells, int r_exist,
                                                        const unsigned* __restrict__ offsets, unsigned* __restrict__ list, int rows, region::Rect q) {
  __shared__ int s_cnt[kAnyBlock / 64];
  const size_t idx = (size_t)blockIdx.x * kAnyBlock + threadIdx.x;
  const size_t g = idx < cells ? any_cell<RECT>(idx, rows, q) : 0;
  const bool need = idx < cells && needs_median(float_bits(in[g]), mask[g], r_exist);
  const unsigned long long votes = __ballot(need);
  const int wave = (int)(threadIdx.x >> 6);
  if (lane_id() == 0) s_cnt[wave] = __popcll(votes);
  __syncthreads();
  if (!need) return;
  unsigned pos = offsets[blockIdx.x];
  for (int k = 0; k < wave; ++k) pos += (unsigned)s_cnt[k];
  pos += (unsigned)__popcll(votes & ((1ull << lane_id()) - 1ull));
  if (pos < cells) list[pos] = (unsigned)g;  // (pos < the total <= cells: the prefix sums say so)
}

// one wavefront per listed cell; n_list: the total behind the counts
__global__ __launch_bounds__(kAnyBlock) void k_median_any(const float* __restrict__ in, float* __restrict__ out, int rows, int cols,
                                                          const unsigned* __restrict__ list, const unsigned* __restrict__ n_list, int r_fill,
                                                          int r_exist) {
  const size_t cells = (size_t)rows * cols;
  const size_t n = *n_list < cells ? *n_list : cells;
  const size_t waves = (size_t)gridDim.x * (kAnyBlock / 64);
  const unsigned lane = lane_id();
  for (size_t e = (size_t)blockIdx.x * (kAnyBlock / 64) + (threadIdx.x >> 6); e < n; e += waves) {  // (wave-uniform)
    const size_t cell = list[e];
    if (cell >= cells) continue;
    const int i = (int)(cell % rows), j = (int)(cell / rows);
    const int rr = finite_bits(float_bits(in[cell])) ? r_exist : r_fill;
    const int i0 = i > rr ? i - rr : 0, i1 = (rows - 1 - i > rr) ? i + rr : rows - 1;
    const int j0 = j > rr ? j - rr : 0, j1 = (cols - 1 - j > rr) ? j + rr : cols - 1;
    const unsigned wh = (unsigned)(i1 - i0 + 1);
    const size_t wn = (size_t)wh * (size_t)(j1 - j0 + 1);
    const float m = median([&](uint32_t p) {
      unsigned cnt = 0;
      for (size_t t0 = 0; t0 < wn; t0 += 64) {  // (wave-uniform trip count: every lane reaches every ballot)
        const size_t t = t0 + lane;
        bool hit = false;
        if (t < wn) {
          const size_t dj = t / wh, di = t - dj * wh;
          hit = float_key(in[((size_t)j0 + dj) * rows + ((size_t)i0 + di)]) < p;
        }
        cnt += (unsigned)__popcll(__ballot(hit));
      }
      return cnt;
    });
    if (lane == 0) out[cell] = m;
  }
}

unsigned blocks_of(size_t total, int block) { return (unsigned)((total + block - 1) / block); }

}  // namespace

hipError_t launch(const Args& a, const Plan& p, hipStream_t stream) {
  const size_t cells = (size_t)a.rows * a.cols, total = cells * (size_t)a.nmaps;
  if (total == 0 || (total + kMaskBlock - 1) / kMaskBlock > 0x7fffffffull) return hipErrorInvalidValue;
  const unsigned mb = blocks_of(total, kMaskBlock);
  // V, then k erosions and k dilations between the two scratch masks (no launch at all for k = 0), then the square OR
  hipLaunchKernelGGL(k_mask_valid, dim3(mb), dim3(kMaskBlock), 0, stream, a.in, a.tmp[0], total);
  int cur = 0;
  for (int k = 0; k < 2 * a.iterations; ++k) {
    hipLaunchKernelGGL(k_mask_morph, dim3(mb), dim3(kMaskBlock), 0, stream, a.tmp[cur], a.tmp[cur ^ 1], a.rows, a.cols, total, k < a.iterations ? 1 : 0);
    cur ^= 1;
  }
  hipLaunchKernelGGL(k_mask_or, dim3(mb), dim3(kMaskBlock), 0, stream, a.tmp[cur], a.tmp[cur ^ 1], a.rows, a.cols, total, a.r_fill, 1);
  hipLaunchKernelGGL(k_mask_or, dim3(mb), dim3(kMaskBlock), 0, stream, a.tmp[cur ^ 1], a.mask, a.rows, a.cols, total, a.r_fill, 0);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;

  if (p.route == kRouteTile) {
    hipLaunchKernelGGL(k_median_tile, dim3((unsigned)p.blocks), dim3(kTileThreads), p.lds_bytes, stream, a.in, a.out, a.mask, a.rows, a.cols, p.tiles_x,
                       p.tiles_y, p.r, a.r_fill, a.r_exist, 0, 0, a.rows, a.cols);
    return hipGetLastError();
  }
  const size_t nb = any_blocks(cells);
  if (nb > 0x7fffffffull) return hipErrorInvalidValue;
  const size_t want_waves = cells < 8192 ? cells : 8192;  // (the list is at most `cells` long; a grid-stride loop takes the rest)
  const unsigned any_grid = (unsigned)((want_waves + kAnyBlock / 64 - 1) / (kAnyBlock / 64));
  const region::Rect whole = {0, 0, a.rows, a.cols};
  for (int m = 0; m < a.nmaps; ++m) {
    const float* const in = a.in + (size_t)m * cells;
    float* const out = a.out + (size_t)m * cells;
    const uint8_t* const mask = a.mask + (size_t)m * cells;
    hipLaunchKernelGGL(k_any_count<false>, dim3((unsigned)nb), dim3(kAnyBlock), 0, stream, in, out, mask, cells, a.r_exist, a.any_counts, a.rows, whole);
    hipLaunchKernelGGL(k_any_scan, dim3(1), dim3(kAnyBlock), 0, stream, a.any_counts, nb);
    hipLaunchKernelGGL(k_any_list<false>, dim3((unsigned)nb), dim3(kAnyBlock), 0, stream, in, mask, cells, a.r_exist, a.any_counts, a.any_list, a.rows, whole);
    hipLaunchKernelGGL(k_median_any, dim3(any_grid), dim3(kAnyBlock), 0, stream, in, out, a.rows, a.cols, a.any_list, a.any_counts + nb, a.r_fill, a.r_exist);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

// One map: a.in / a.out / a.mask / a.tmp point at that map's cells (a.nmaps is not read); every launch is sized by a
// rectangle of p.
hipError_t launch_region(const Args& a, const RegionPlan& p, hipStream_t stream) {
  const region::Rect out = p.out;
  if (region::cells(out) == 0 || out.i0 < 0 || out.j0 < 0 || out.i1 > a.rows || out.j1 > a.cols) return hipErrorInvalidValue;
  const auto mask_pass = [&](const uint8_t* src, uint8_t* dst, const region::Rect& q, int what) {
    hipLaunchKernelGGL(k_mask_rect, dim3(blocks_of(region::cells(q), kMaskBlock)), dim3(kMaskBlock), 0, stream, a.in, src, dst, a.rows, a.cols, q, what, a.r_fill);
  };
  mask_pass(nullptr, a.tmp[0], mask_stage_rect(p, 0), 0);
  int cur = 0;
  for (int k = 0; k < 2 * a.iterations; ++k) {
    mask_pass(a.tmp[cur], a.tmp[cur ^ 1], mask_stage_rect(p, k + 1), k < a.iterations ? 1 : 2);
    cur ^= 1;
  }
  mask_pass(a.tmp[cur], a.tmp[cur ^ 1], row_or_rect(p), 3);
  mask_pass(a.tmp[cur ^ 1], a.mask, out, 4);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;

  if (p.k.route == kRouteTile) {
    hipLaunchKernelGGL(k_median_tile, dim3((unsigned)p.k.blocks), dim3(kTileThreads), p.k.lds_bytes, stream, a.in, a.out, a.mask, a.rows, a.cols, p.k.tiles_x,
                       p.k.tiles_y, p.k.r, a.r_fill, a.r_exist, out.i0, out.j0, out.i1, out.j1);
    return hipGetLastError();
  }
  const size_t oc = region::cells(out), nb = p.any_blocks;
  if (nb > 0x7fffffffull) return hipErrorInvalidValue;
  const size_t want_waves = oc < 8192 ? oc : 8192;
  const unsigned any_grid = (unsigned)((want_waves + kAnyBlock / 64 - 1) / (kAnyBlock / 64));
  hipLaunchKernelGGL(k_any_count<true>, dim3((unsigned)nb), dim3(kAnyBlock), 0, stream, a.in, a.out, a.mask, oc, a.r_exist, a.any_counts, a.rows, out);
  hipLaunchKernelGGL(k_any_scan, dim3(1), dim3(kAnyBlock), 0, stream, a.any_counts, nb);
  hipLaunchKernelGGL(k_any_list<true>, dim3((unsigned)nb), dim3(kAnyBlock), 0, stream, a.in, a.mask, oc, a.r_exist, a.any_counts, a.any_list, a.rows, out);
  hipLaunchKernelGGL(k_median_any, dim3(any_grid), dim3(kAnyBlock), 0, stream, a.in, a.out, a.rows, a.cols, a.any_list, a.any_counts + nb, a.r_fill, a.r_exist);
  return hipGetLastError();
}

}  // namespace median
}  // namespace te
