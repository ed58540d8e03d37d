// f16x3.hpp — shared pieces of the f16x3-emulated fp32 GEMM (fusion_f16x3.hip k_fusion_rows_f16x3): a round-to-nearest split
// of SCALED fp32 values into two half-precision terms, the sibling of x6.hpp's three-way bfloat16 split.
//
// A half-precision term holds 11 significand bits, so two terms (plus the sign of the second) cover fp32's 24 where three
// bfloat16 terms (8 bits each) are needed: three products per 16 k — a_l b_h, a_h b_l, a_h b_h, the O(2^-22) a_l b_l
// dropped — instead of x6's six, on an MFMA of the same cycle count.  What half precision does not have is fp32's exponent
// range (normal numbers from 2^-14 to 65504), so every row of either operand is multiplied by its own power of two first:
//
//   scale exponent  s = 14 - e,  e = the exponent of the row's largest finite magnitude (2^e <= max |x| < 2^(e+1)), so that the
//                   scaled maximum lies in [2^14, 2^15) and rounds to at most 2^15;  s is clamped to [-126, 127] (a row whose
//                   maximum is an fp32 subnormal gets 2^127 — finite, its values end below 2) and is 0 for an all-zero row;
//   xs = x * 2^s    exact (a power of two) unless xs underflows fp32's normal range, which takes an element 2^140 below its
//                   row's maximum;
//   h = rn16(xs)    round to nearest even,  |xs - h| <= 2^-11 |xs|;
//   l = rn16(xs - (float)h)   the subtraction is exact in fp32 (Sterbenz / the difference is a multiple of ulp32(xs) below
//                   2^12 of them); l is exact when that difference needs <= 11 bits, else rounded by <= one ulp32(xs):
//                   |xs - (h + l)| <= 2^-23 |xs| for every element whose l is a normal half, i.e. |xs| >= 2^-2 — within
//                   2^16 of its row's maximum.
// The product is un-scaled with ldexp by -(s_row + s_column): exact.
//
// Elements far below their row's maximum.  Below 2^-16 of the maximum l becomes a half-precision subnormal (spacing 2^-24 in
// the scaled domain: an ABSOLUTE error of 2^-25 * 2^-s, i.e. 2^-40 of the row's maximum, no longer relative to the element);
// below 2^-28 of it h is subnormal as well, and below 2^-39 the element rounds to zero.  The conversions and
// v_mfma_f32_32x32x16_f16 honour half-precision subnormals — measured on the MI355X, not assumed
// (tests/test_gpu_fusion_f16x3.py::test_fusion_pair_f16x3_keeps_subnormal_terms: a term that is 2^-16 after scaling gives
// its exact product) — so these are the bounds.  An error that is relative to the ROW's maximum where x6's is
// relative to the ELEMENT is the contract: with exact accumulation the emulation alone gives up to ~1e-5 of sum |a||w| at
// 2^26 of dynamic range inside the rows where x6 gives 4e-7 (measured on the kernel on such operands: 4.9e-7 vs 8.5e-7 on
// 2880 outputs, 1e-7 of the output's scale either way).
//
// Non-finite inputs.  The row maximum ignores NaN; a row that holds +-Inf has e = 128 and s = -114: Inf stays Inf in h and
// l = Inf - Inf = NaN, so an Inf operand turns its output row / column into NaN exactly as in x6.hpp; the finite elements of
// such a row are scaled 2^-114 and mostly vanish.  NaN stays NaN.
// YOLAT_STRICT_FP32=1 selects the fp32-input MFMA kernels instead (x6.hpp), YOLAT_FUSION_F16X3=0 the bf16x6 ones.
#pragma once
#include "base.hpp"

typedef _Float16 fh_f16x8 __attribute__((ext_vector_type(8)));

namespace {
// scale exponent of a row whose largest finite magnitude is m (m >= 0)
__host__ __device__ __forceinline__ int fh_scale_exp(float m) {
  unsigned u;
  __builtin_memcpy(&u, &m, 4);
  u &= 0x7fffffffu;
  if (u == 0u) return 0;
  const int s = 14 - ((int)(u >> 23) - 127);
  return s > 127 ? 127 : s;                              // (s >= -114: the exponent field is at most 255)
}
// 2^s for s in [-126, 127]
__host__ __device__ __forceinline__ float fh_pow2(int s) {
  const unsigned u = (unsigned)(s + 127) << 23;
  float f;
  __builtin_memcpy(&f, &u, 4);
  return f;
}
// two-term half-precision split of 8 SCALED fp32 values (|x| <= 2^15): h = rn16(x), l = rn16(x - h)
__device__ __forceinline__ void fh_split8(const float x[8], fh_f16x8& h, fh_f16x8& l) {
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const _Float16 hi = (_Float16)x[i];
    h[i] = hi;
    l[i] = (_Float16)(x[i] - (float)hi);
  }
}
}  // namespace
