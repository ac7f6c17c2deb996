// te_median.h -- the exact selection behind te_run_median_fill (include/travgpu.h): plain C++ that compiles for the host and
// the device.  The kernels (te_median.hip) and the CPU harness (tests/cpu/median_select_check.cpp) compile THIS text.
//
//   float_key   the order-preserving map from a float32 to a 32-bit unsigned key: every bit of a negative is flipped, the
//               sign bit of a non-negative is set.  Finite values land in [0x00800000, 0xff7fffff] and compare as unsigned
//               exactly as the floats compare (-0.0 sorts just below +0.0: the one place where the key order is finer than
//               the float order).  +-inf and NaN map to kNoKey = 0xffffffff, which no finite value maps to and which is
//               above every finite key: a count of "keys below a pivot" never counts one.
//   key_float   the inverse on finite keys, bit for bit.
//   select      the key at sorted index `rank` of a bag of keys that is given only through below(p) = the number of its
//               keys < p: the largest p with below(p) <= rank, built from the top bit down (below is monotone).  32 calls.
//               Duplicates need no care: the key at index rank is v  <=>  below(v) <= rank < below(v + 1).
//   median      the contract's median of a window: n = its finite values = below(kNoKey); none: NaN; otherwise the value at
//               index n / 2 of the sorted values -- the upper median, what std::nth_element(b, b + n / 2, e) leaves there.
// Selection has no rounding: the result is one of the inputs, and it cannot depend on the order the window is visited in.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define TE_MEDIAN_HD __host__ __device__ inline
#else
#define TE_MEDIAN_HD inline
#endif

namespace te {
namespace median {

constexpr uint32_t kNoKey = 0xffffffffu;
constexpr uint32_t kNanBits = 0x7fc00000u;  // the NaN a window without a finite value yields

TE_MEDIAN_HD uint32_t float_bits(float v) {
  uint32_t b;
  __builtin_memcpy(&b, &v, sizeof(b));
  return b;
}
TE_MEDIAN_HD float bits_float(uint32_t b) {
  float v;
  __builtin_memcpy(&v, &b, sizeof(v));
  return v;
}
TE_MEDIAN_HD bool finite_bits(uint32_t b) { return (b & 0x7f800000u) != 0x7f800000u; }

TE_MEDIAN_HD uint32_t float_key(float v) {
  const uint32_t b = float_bits(v);
  if (!finite_bits(b)) return kNoKey;
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
// (of a finite key)
TE_MEDIAN_HD float key_float(uint32_t k) { return bits_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// below(p): the number of keys < p, for any p.  rank < below(kNoKey).
template <class Below>
TE_MEDIAN_HD uint32_t select(Below&& below, uint32_t rank) {
  uint32_t p = 0;
  for (uint32_t bit = 0x80000000u; bit; bit >>= 1)
    if ((uint32_t)below(p | bit) <= rank) p |= bit;
  return p;
}

template <class Below>
TE_MEDIAN_HD float median(Below&& below) {
  const uint32_t n = (uint32_t)below(kNoKey);
  if (n == 0) return bits_float(kNanBits);
  return key_float(select(below, n / 2));
}

// the bag as an array (the CPU harness; the kernels count over LDS or with a whole wavefront)
TE_MEDIAN_HD uint32_t count_below(const uint32_t* keys, int n, uint32_t p) {
  uint32_t c = 0;
  for (int k = 0; k < n; ++k) c += keys[k] < p ? 1u : 0u;
  return c;
}

}  // namespace median
}  // namespace te
