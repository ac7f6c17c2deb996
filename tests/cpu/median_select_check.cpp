// CPU check of the selection the median-fill kernels instantiate (traversability_estimation_amd/csrc/te_median.h): the same
// header, compiled for the host, plain and under the sanitizers (tests/test_median_select.py).
//   - float_key: the unsigned order of the keys is the float order on a ladder of negatives, denormals, +-0 and +-FLT_MAX;
//     +-inf and NaN (quiet, signalling, both signs, any payload) give kNoKey, which no finite value gives; key_float inverts
//     float_key bit for bit;
//   - median: against std::nth_element(b, b + n / 2, e) over the finite values, on random bags of 1 .. 225 values drawn from
//     1 .. 8 distinct ones (ties dominate), with non-finite values mixed in; a bag without a finite value gives NaN.
//   median_select_check [n_random seed]
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <random>
#include <vector>

#include "te_median.h"

using namespace te::median;

namespace {

int g_failed = 0;
#define CHECK(cond, ...)              \
  do {                                \
    if (!(cond)) {                    \
      ++g_failed;                     \
      if (g_failed <= 20) {           \
        printf("FAILED %s: ", #cond); \
        printf(__VA_ARGS__);          \
        printf("\n");                 \
      }                               \
    }                                 \
  } while (0)

float median_of(const std::vector<float>& bag) {
  std::vector<uint32_t> keys(bag.size());
  for (size_t k = 0; k < bag.size(); ++k) keys[k] = float_key(bag[k]);
  return median([&](uint32_t p) { return count_below(keys.data(), (int)keys.size(), p); });
}

void check_keys() {
  // strictly ascending floats
  const float ladder[] = {-FLT_MAX, -1e30f, -1e6f, -2.5f, -1.0f, -1e-6f, -FLT_MIN, -bits_float(0x007fffffu), -bits_float(1u), 0.0f,
                          bits_float(1u), bits_float(0x007fffffu), FLT_MIN, 1e-6f, 1.0f / 255.0f, 1.0f, 2.5f, 1e6f, 1e30f, FLT_MAX};
  const int n = (int)(sizeof(ladder) / sizeof(ladder[0]));
  for (int a = 0; a < n; ++a) {
    CHECK(float_key(ladder[a]) != kNoKey, "ladder[%d]", a);
    CHECK(float_bits(key_float(float_key(ladder[a]))) == float_bits(ladder[a]), "round trip of ladder[%d]", a);
    for (int b = 0; b < n; ++b)
      CHECK((float_key(ladder[a]) < float_key(ladder[b])) == (ladder[a] < ladder[b]), "order of ladder[%d], ladder[%d]", a, b);
  }
  // -0.0 sorts just below +0.0, above every negative
  CHECK(float_key(-0.0f) + 1 == float_key(0.0f), "the zeros");
  CHECK(float_key(-bits_float(1u)) < float_key(-0.0f), "the largest negative and -0.0");
  CHECK(float_bits(key_float(float_key(-0.0f))) == 0x80000000u, "round trip of -0.0");
  // the smallest and largest finite keys leave room for the sentinel
  CHECK(float_key(-FLT_MAX) == 0x00800000u && float_key(FLT_MAX) == 0xff7fffffu, "the ends: %08x %08x", float_key(-FLT_MAX), float_key(FLT_MAX));
  const uint32_t not_finite[] = {0x7f800000u, 0xff800000u, 0x7fc00000u, 0xffc00000u, 0x7f800001u, 0xff800001u, 0x7fffffffu, 0xffffffffu, 0x7fa00000u};
  for (uint32_t b : not_finite) CHECK(float_key(bits_float(b)) == kNoKey, "%08x", b);
  // every exponent, a few mantissas: round trip, and neighbours in float order are neighbours in key order
  for (uint32_t e = 0; e < 255; ++e)
    for (uint32_t m : {0u, 1u, 0x400000u, 0x7fffffu})
      for (uint32_t s : {0u, 0x80000000u}) {
        const uint32_t b = s | (e << 23) | m;
        CHECK(float_bits(key_float(float_key(bits_float(b)))) == b, "round trip of %08x", b);
      }
}

void check_random(int n_sets, unsigned seed) {
  std::mt19937 rng(seed);
  const float pool[] = {0.0f, 1.0f / 255.0f, 2.0f / 255.0f, 254.0f / 255.0f, 1.0f, -3.5f, 1e6f, 1e-6f, -1e-6f, bits_float(3u), -bits_float(3u),
                        FLT_MAX, -FLT_MAX, 17.25f, -17.25f, 0.5f};
  const float junk[] = {NAN, INFINITY, -INFINITY, bits_float(0xffc00001u)};
  const int n_pool = (int)(sizeof(pool) / sizeof(pool[0]));
  for (int s = 0; s < n_sets; ++s) {
    const int n = 1 + (int)(rng() % 225), distinct = 1 + (int)(rng() % 8);
    float vals[8];
    for (int k = 0; k < distinct; ++k) vals[k] = pool[rng() % n_pool];
    const unsigned junk_in = rng() % 4;  // one set in four has no junk; otherwise about one value in junk_in + 2 is junk
    std::vector<float> bag((size_t)n), finite;
    for (int k = 0; k < n; ++k) {
      const bool j = junk_in != 0 && rng() % (junk_in + 2) == 0;
      bag[(size_t)k] = j ? junk[rng() % 4] : vals[rng() % (unsigned)distinct];
      if (!j) finite.push_back(bag[(size_t)k]);
    }
    const float got = median_of(bag);
    if (finite.empty()) {
      CHECK(float_bits(got) == kNanBits, "set %d: no finite value, got %08x", s, float_bits(got));
      continue;
    }
    std::nth_element(finite.begin(), finite.begin() + (long)(finite.size() / 2), finite.end());
    const float want = finite[finite.size() / 2];
    // (the pool holds one zero, so equal floats are equal bits)
    CHECK(float_bits(got) == float_bits(want), "set %d of %d values (%d distinct): got %g (%08x), want %g (%08x)", s, n, distinct, (double)got,
          float_bits(got), (double)want, float_bits(want));
  }
  // a bag of nothing but junk, and the named small cases
  CHECK(float_bits(median_of({NAN, INFINITY, -INFINITY})) == kNanBits, "junk only");
  CHECK(median_of({2.0f, 1.0f}) == 2.0f, "n = 2 takes the larger");
  CHECK(median_of({3.0f, 1.0f, 2.0f}) == 2.0f, "n = 3");
  CHECK(median_of({4.0f, 1.0f, 3.0f, 2.0f}) == 3.0f, "n = 4 takes the upper median");
  CHECK(median_of({5.0f}) == 5.0f, "n = 1");
  CHECK(median_of({1.0f, NAN, INFINITY, 7.0f, 7.0f}) == 7.0f, "junk is not counted");
}

}  // namespace

int main(int argc, char** argv) {
  const int n = argc > 1 ? atoi(argv[1]) : 100000;
  const unsigned seed = argc > 2 ? (unsigned)atoi(argv[2]) : 1u;
  check_keys();
  check_random(n, seed);
  printf("%d random sets, %d failed checks\n", n, g_failed);
  return g_failed ? 1 : 0;
}
