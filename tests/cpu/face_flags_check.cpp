// face_flags_check.cpp -- the face flags of an elevation layer from the header the library builds and reads them with
// (te_face_flags.h), checked against the mask kernel's own tile test.  tests/test_face_flags.py.
//
//   face_flags_check <rows> <cols> <batch> <crit_step> <in> <out>
//     in:  elevation, then the step score layer: 2 x batch x rows x cols float32, cell (i, j) of map m at m*rows*cols + j*rows + i
//     out: the flag bytes (face_flag_bytes), then hit' per cell (batch x rows x cols bytes)
//
// Before it writes, for every tile of k_fp_mask<MY>, MY in {4, 8, 32} (64 x MY cells, halo MH = 3; restated here as
// te_footprint.hip computes it: t_key = elevation where the step score is 0, NaN elsewhere and outside the map; t_kl on the tile
// rows 1 .. MTH-2 and columns 1 .. MTW-2 from the NaN-ignoring 3x3 minimum of t_key):
//   soundness   tile_has_kl  =>  some flag of the tile is set (face_tile_clear is false);
//   tightness   with the step score 0 in every cell of the tile's reach, tile_has_kl <=> some flag of the tile is set.
// Exit status 1 and a line on stderr for a violation.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "te_face_flags.h"

namespace {

constexpr int MX = 64, MH = 3, MTW = MX + 2 * MH;

// tile_has_kl of the tile at (i0, j0) of map e / s (s == nullptr: the step score is 0 everywhere)
bool tile_has_kl(const float* e, const float* s, int rows, int cols, int i0, int j0, int MY, double crit) {
  const int MTH = MY + 2 * MH;
  std::vector<float> t_elev((size_t)MTW * MTH), t_key((size_t)MTW * MTH);
  for (int lb = 0; lb < MTH; ++lb)
    for (int la = 0; la < MTW; ++la) {
      const int a = i0 - MH + la, b = j0 - MH + lb;
      const bool in = a >= 0 && a < rows && b >= 0 && b < cols;
      const size_t o = in ? (size_t)b * rows + a : 0;
      t_elev[(size_t)lb * MTW + la] = in ? e[o] : NAN;
      t_key[(size_t)lb * MTW + la] = (in && (s == nullptr || s[o] == 0.0f)) ? e[o] : NAN;
    }
  for (int r = 1; r <= MTH - 2; ++r)
    for (int c = 1; c <= MTW - 2; ++c) {
      float m = NAN;
      for (int dr = -1; dr <= 1; ++dr)
        for (int dc = -1; dc <= 1; ++dc) m = std::fmin(m, t_key[(size_t)(r + dr) * MTW + c + dc]);  // (fmin ignores NaN, like v_min3_f32)
      if ((double)m < (double)t_elev[(size_t)r * MTW + c] - crit) return true;
    }
  return false;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 7) return 2;
  const int rows = std::atoi(argv[1]), cols = std::atoi(argv[2]), batch = std::atoi(argv[3]);
  const double crit = std::atof(argv[4]);
  if (rows <= 0 || cols <= 0 || batch <= 0) return 2;
  const size_t per = (size_t)rows * cols, n = per * batch;
  std::vector<float> elev(n), step(n);
  FILE* f = std::fopen(argv[5], "rb");
  if (!f || std::fread(elev.data(), sizeof(float), n, f) != n || std::fread(step.data(), sizeof(float), n, f) != n) return 2;
  std::fclose(f);

  std::vector<uint8_t> flags(te::face_flag_bytes(rows, cols, batch)), hit(n);
  te::face_flags_host(elev.data(), rows, cols, batch, crit, flags.data(), hit.data());

  int bad = 0;
  for (int m = 0; m < batch; ++m)
    for (int MY : {4, 8, 32})
      for (int j0 = 0; j0 < cols; j0 += MY)
        for (int i0 = 0; i0 < rows; i0 += MX) {
          const bool clear = te::face_tile_clear(flags.data(), rows, cols, m, i0, j0, MY);
          const bool kl = tile_has_kl(elev.data() + m * per, step.data() + m * per, rows, cols, i0, j0, MY, crit);
          const bool kl_all = tile_has_kl(elev.data() + m * per, nullptr, rows, cols, i0, j0, MY, crit);
          if (kl && clear) {
            std::fprintf(stderr, "unsound: map %d, MY %d, tile (%d, %d) has a lower step neighbour and clear flags\n", m, MY, i0, j0);
            ++bad;
          }
          if (kl_all == clear) {
            std::fprintf(stderr, "not tight: map %d, MY %d, tile (%d, %d): step 0 everywhere gives tile_has_kl = %d, flags clear = %d\n", m, MY, i0,
                         j0, (int)kl_all, (int)clear);
            ++bad;
          }
        }
  if (bad) return 1;

  f = std::fopen(argv[6], "wb");
  if (!f || std::fwrite(flags.data(), 1, flags.size(), f) != flags.size() || std::fwrite(hit.data(), 1, n, f) != n) return 2;
  std::fclose(f);
  return 0;
}
