// Stand-alone driver of csrc/two_plane.hpp (its pure part) for tests/test_two_plane_cpu.py.  No input.  Prints
//   exp <bit pattern, hex> <scale exponent>    for all 256 exponent fields x mantissa all-zeros / all-ones x sign clear / set
//                                              (the test compares them with tests/two_plane_refs.py)
//   ok <property>                              for every property of the rule that holds, checked here exhaustively
//   FAIL <property> <where>                    for the first violation of one (exit status 1)
// The bounds of the properties follow from the rule itself: a float with exponent field e has 2^(e - 127) <= |x| < 2^(e - 126)
// and k = 141 - e, so 2^14 <= |x| 2^k < 2^15 wherever the exponent is not clamped.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <initializer_list>

#include "two_plane.hpp"

static float as_float(uint32_t b) {
  float f;
  memcpy(&f, &b, 4);
  return f;
}

static int failures = 0;
static void fail(const char* what, long a, long b) {
  printf("FAIL %s at %ld %ld\n", what, a, b);
  ++failures;
}
template <class F>
static void property(const char* name, F body) {
  const int before = failures;
  body(name);
  if (failures == before) printf("ok %s\n", name);
}

int main() {
  for (uint32_t e = 0; e < 256; ++e)
    for (uint32_t mant : {0u, 0x7fffffu})
      for (uint32_t sign : {0u, 0x80000000u}) {
        const uint32_t bits = sign | (e << 23) | mant;
        printf("exp %08x %d\n", bits, mml::scale_exp_of(bits));
      }

  property("pow2_bits", [](const char* name) {
    for (int k = -126; k <= 127; ++k)
      if (as_float(mml::pow2_bits(k)) != ldexpf(1.f, k)) return fail(name, k, 0);
  });
  property("scale_exp_range", [](const char* name) {
    for (uint32_t e = 0; e < 256; ++e)
      for (uint32_t mant : {0u, 0x7fffffu}) {
        const uint32_t bits = (e << 23) | mant;
        const int k = mml::scale_exp_of(bits);
        if (k != mml::scale_exp_of(bits | 0x80000000u)) return fail(name, e, 1);
        if (e == 255) {
          if (k != 0) return fail(name, e, 2);
        } else if (e < 31) {
          if (k != 110) return fail(name, e, 3);
        } else if (e > 251) {
          if (k != -110) return fail(name, e, 4);
        } else {
          // (a power of two times a float, the product far from fp32's ends: exact)
          const float y = as_float(bits) * as_float(mml::pow2_bits(k));
          if (mant ? !(y < 32768.f) : !(y >= 16384.f)) return fail(name, e, 5);
        }
      }
  });
  property("row_gives_way", [](const char* name) {
    for (int kA = -110; kA <= 110; ++kA)
      for (int kB = -110; kB <= 110; ++kB) {
        const int r = mml::row_gives_way(kA, kB), sum = kA + kB;
        const int want = sum > 126 ? 126 - kB : (sum < -126 ? -126 - kB : kA);  // unchanged, or the nearest that fits
        if (abs(r + kB) > 126 || r != want) return fail(name, kA, kB);
      }
  });
  property("both_give_way", [](const char* name) {
    for (int kA = -110; kA <= 110; ++kA)
      for (int kB = -110; kB <= 110; ++kB) {
        const mml::ScalePair g = mml::both_give_way(kA, kB);
        const int a = g.row, b = g.col;
        const int sum = kA + kB, da = a - kA, db = b - kB;
        if (abs(a + b) > 126) return fail(name, kA, kB);
        if (abs(sum) <= 126) {
          if (da != 0 || db != 0) return fail(name, kA, kB);
          continue;
        }
        // both move towards the range, no further than its edge; the row operand's step is the column's or one more
        const int dir = sum > 126 ? -1 : 1;
        if (da * dir < 0 || db * dir < 0 || abs(a + b) != 126) return fail(name, kA, kB);
        if (abs(da) - abs(db) != 0 && abs(da) - abs(db) != 1) return fail(name, kA, kB);
      }
  });
  return failures ? 1 : 0;
}
