// 64-bit fixed point of the LDS row fold (scatter_fold.hpp: the insert and the flush that scatter_fold_kernel and
// scatter_pool_fold_kernel share): every gradient value of a workgroup is scaled by 2^(150 + shift - emax), emax = the
// largest exponent the workgroup holds, and summed with integer LDS atomics -- the chunk sum does not depend on the
// order of the addends.
#pragma once
#include "common.hpp"

namespace mml {
#ifdef __HIPCC__
__device__ __forceinline__ long long to_fixed(float x, int emax, const int shift = 28) {
  const unsigned u = __float_as_uint(x);
  int e = (int)((u >> 23) & 0xffu);
  if (e == 255) return 0;             // Inf / NaN: added to the table row directly (scatter_fold_kernel), not folded
  unsigned m = u & 0x7fffffu;
  if (e) m |= 0x800000u; else e = 1;  // subnormal
  const int sh = e - emax + shift;    // <= shift: x = m * 2^(e - 150) in units of 2^(emax - 150 - shift)
  long long v;
  if (sh >= 0) v = (long long)m << sh;
  else if (sh > -25) v = ((long long)m + (1ll << (-sh - 1))) >> (-sh);
  else v = 0;
  return (u >> 31) ? -v : v;
}

__device__ __forceinline__ float from_fixed(long long v, int emax, const int shift = 28) {
  return (float)ldexp((double)v, emax - 150 - shift);  // int64 -> f64 is exact below 2^53 and rounds once above; one rounding to f32
}
#endif
}  // namespace mml
