// The MXFP4 rule of the 4-bit decoder weights (mx4.hip; tests/mx4_cases.py is the same rule in torch): OCP e2m1 codes plus one E8M0
// power-of-two scale per run of 32 consecutive K elements of a weight row.
//   amax = max |x_i| (fp32) ; amax == 0: e = 0 ; else e = the smallest integer with amax <= 6 * 2^e, read from amax's bits: with
//   amax = m * 2^q, 1 <= m < 2: e = q - 2 if m <= 1.5, else q - 1 ; e clamped to [-126, 127] ; scale byte = e + 127, in [1, 254]
//   code_i = sign << 3 | idx, idx = the index in {0, 0.5, 1, 1.5, 2, 3, 4, 6} nearest to |x_i| / 2^e (exact), ties to the EVEN index;
//   the sign of x is kept, also on a zero.  Nothing is clamped: |x_i| / 2^e <= 6 by construction (kv8_rule.h's "no clamp" habit; the
//   OCP floor rule would saturate (6, 8)).
//   A run with a non-finite element: scale byte 0xFF, codes 0.  The kernels read a scale byte as the float (byte << 23), so 0xFF is
//   +inf and 0 * inf = NaN: such a run makes its output non-finite, never a finite wrong number.
//   x^_i = grid[idx] * (+-1) * 2^e.
// Layout: byte j of a code row holds element 2 j in bits 0-3 and element 2 j + 1 in bits 4-7, the order in which
// v_cvt_scalef32_pk_bf16_fp4 unpacks the byte its byte_sel names.
#pragma once
#include "vita_common.h"
#include "kv8_rule.h"

constexpr int kMx4Block = 32;        // K elements that share a scale (host side: ops.MX4_BLOCK)

// max |x| of a run as bf16 bits (kv8_absmax_bits: integer order, NaN above inf) -> the scale byte
__device__ __forceinline__ unsigned mx4_scale_byte(const unsigned absmax_bits) {
  if (absmax_bits >= 0x7f80u) return 0xffu;                            // inf or NaN in the run
  if (absmax_bits == 0u) return 127u;
  const int q = (int)(absmax_bits >> 7) - 127;                         // a bf16 subnormal reads as q = -127: clamped below
  int e = (absmax_bits & 0x7fu) <= 0x40u ? q - 2 : q - 1;              // m <= 1.5 ?
  e = e < -126 ? -126 : e;                                             // e <= 126 as it is
  return (unsigned)(e + 127);
}
__device__ __forceinline__ float mx4_scale_f32(const unsigned byte) { return __uint_as_float(byte << 23); }

// one bf16 (low 16 bits of h) -> its 4-bit code under the scale 2^e, inv = 2^-e (a normal fp32 for every e the rule gives)
__device__ __forceinline__ unsigned mx4_encode1(const unsigned h, const float inv) {
  const float v = __uint_as_float((h & 0x7fffu) << 16) * inv;          // |x| / 2^e, exact
  const unsigned idx = (unsigned)(v > 0.25f) + (unsigned)(v >= 0.75f) + (unsigned)(v > 1.25f) + (unsigned)(v >= 1.75f) +
                       (unsigned)(v > 2.5f) + (unsigned)(v >= 3.5f) + (unsigned)(v > 5.0f);
  return ((h >> 12) & 8u) | idx;
}
// 8 bf16 of one lane -> 8 codes in one word (element i in bits 4 i .. 4 i + 3)
__device__ __forceinline__ unsigned mx4_encode8(const u32x4 x, const unsigned scale_byte) {
  if (scale_byte == 0xffu) return 0u;
  const float inv = __uint_as_float((254u - scale_byte) << 23);        // 2^-(byte - 127)
  unsigned c = 0u;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    c |= mx4_encode1(x[j] & 0xffffu, inv) << (8 * j);
    c |= mx4_encode1(x[j] >> 16, inv) << (8 * j + 4);
  }
  return c;
}
// 8 codes of one word -> four packed bf16 pairs (exact: the grid values themselves, the scale stays outside)
__device__ __forceinline__ void mx4_decode8(const unsigned w, unsigned* p) {
  p[0] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, 1.0f, 0));
  p[1] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, 1.0f, 1));
  p[2] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, 1.0f, 2));
  p[3] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, 1.0f, 3));
}
