// The scale rule of the two-plane fp16 arithmetic, stated once.  planes_cut_kernel (gemm.hip) cuts the weights with it;
// gemm.hip, gemm_panel.hip, gemm_ws.hip, gemm_os.hip, gemm_nt.hip and tower_head.hip scale the operand they cut
// themselves with it and combine the two -- fp32-equivalent results need the SAME rule on both sides.  The pure part
// (no HIP, nothing dereferenced) builds with a plain C++ compiler: tests/two_plane_driver.cpp holds it against the numpy
// statement (tests/two_plane_refs.py) and against its own properties without a GPU (tests/test_two_plane_cpu.py).
// oracle/cabi_cpu.c keeps an independent C restatement on purpose; the same test holds the two to each other.
//
// The rule: an operand whose magnitudes are bounded by a slot's value A is multiplied by s = 2^k before it is cut into
// h = rne16(x s), l = rne16(x s - h), with k such that |x| 2^k < 2^15 for every |x| <= A.
//   * 2^15: fp16's largest finite value is 65 504 < 2^16, and rne16 of a value just below 2^15 may round UP to 2^15:
//     one binade of room keeps h finite whatever the rounding does.
//   * 141: a finite fp32 with exponent field e is below 2^(e - 126), so k = 15 - (e - 126).  Only the field
//     enters: mantissa and sign of the bound do not matter.
//   * Inf / NaN (e = 255): k = 0.  They reach the result whatever the scale.
//   * +-110: 2^k and 2^-k are built as bit patterns (pow2_bits), which takes 127 +- k inside 1 .. 254 -- an empty or
//     all-zero tensor (e = 0) asks for 141.  Zeros stay zeros at 2^110; a bound below 2^-95 (e < 31) is scaled short
//     of 2^15 and loses leading bits of the planes; a bound of 2^125 or more (e > 251) is not brought below 2^15 and
//     its largest values may overflow fp16 -- in the last three binades before fp32 itself ends.
// The epilogue multiplies the accumulator by ONE fp32 number 2^-(kA + kB), so kA + kB has to stay inside +-126 too; two
// clamped exponents can add up to +-220.  row_gives_way / both_give_way bring the sum back (which one applies depends
// on whether the column operand's planes already exist).  gemm_ws.hip, gemm_panel.hip and tower_head.hip do NOT clamp
// the sum: they form the inverse as the product 2^-kA 2^-kB of two in-range powers, which under- or overflows as fp32
// does where the kernels above give way.
#pragma once
#include <stdint.h>

#include "../../include/mmlrec.h"

#ifdef __HIPCC__
#define MML_TP_FN __host__ __device__ __forceinline__
#else
#define MML_TP_FN inline
#endif

namespace mml {

// the scale exponent of a magnitude bit pattern (the largest word of a slot, or any |x| as bits)
MML_TP_FN int scale_exp_of(uint32_t bits) {
  const int e = (int)((bits >> 23) & 0xffu);  // |x| < 2^(e - 126)
  if (e == 255) return 0;
  const int k = 141 - e;
  return k > 110 ? 110 : (k < -110 ? -110 : k);
}

// 2^k as an fp32 bit pattern, -126 <= k <= 127
MML_TP_FN uint32_t pow2_bits(int k) { return (uint32_t)(127 + k) << 23; }

// Pre-cut weights: the planes are what they are (cut with kB), so where kA + kB leaves +-126 the row operand alone
// gives way.  Returns the row operand's exponent.
MML_TP_FN int row_gives_way(int kA, const int kB) {
  if (kA + kB > 126) kA = 126 - kB;
  if (kA + kB < -126) kA = -126 - kB;
  return kA;
}

// Both operands cut in the kernel: where kA + kB leaves +-126 -- two operands below 2^-48, whose products fp32 can
// barely hold -- both scales give way equally; the row operand takes the odd unit.
// (By value and returned as a pair: with reference parameters hipcc orders a few scalar instructions of gemm.hip and
// gemm_nt.hip differently.)
struct ScalePair { int row, col; };
MML_TP_FN ScalePair both_give_way(int kA, int kB) {
  const int over = kA + kB - 126, under = -126 - (kA + kB);
  if (over > 0) { kA -= (over + 1) >> 1; kB -= over >> 1; }
  if (under > 0) { kA += (under + 1) >> 1; kB += under >> 1; }
  return {kA, kB};
}

#ifdef __HIPCC__
// A magnitude slot is MML_AMAX_WORDS consecutive words; producers atomicMax the bit pattern of |x| into ANY of them
// (which one is picked from the workgroup / wave number, so that thousands of same-address atomics do not serialise
// at the memory side), consumers take the largest.
__device__ __forceinline__ uint32_t amax_slot(const uint32_t* p) {
  uint32_t m = 0;
#pragma unroll
  for (int i = 0; i < MML_AMAX_WORDS; ++i) m = p[i] > m ? p[i] : m;
  return m;
}
__device__ __forceinline__ float pow2f(int k) { return __uint_as_float(pow2_bits(k)); }
#endif

}  // namespace mml
