// The MXFP8 rule of the opt-in prefill GEMMs (mx8.hip; tests/mx8_rule.py is the same rule in torch): OCP e4m3fn codes plus one E8M0
// power-of-two scale per run of 32 consecutive K elements of a row, the operand format of v_mfma_scale_f32_16x16x128_f8f6f4.
//   amax = max |x_i| ; amax == 0: e = 0 ; else e = the smallest integer with amax <= 448 * 2^e, read from amax's bits: with
//   amax = m * 2^q, 1 <= m < 2: e = q - 8 if m <= 1.75, else q - 7 ; e clamped to [-126, 127] ; scale byte = e + 127, in [1, 254]
//   code_i = e4m3fn_rne(x_i / 2^e): the division is exact (a power of two, the quotient a normal or zero fp32), the sign of x is kept,
//   also on a zero.  Nothing is clamped: |x_i| / 2^e <= 448 by construction (kv8_rule.h's encoder and its "no clamp" habit).
//   A run with a non-finite element: scale byte 0xFF AND every code 0x7F (e4m3fn NaN).  tools/hwprobe/mx8_map.hip
//   (profiles/r27_mx8_map.txt) settled what the instruction does with either; the NaN codes are what makes every output that reads
//   the run NaN, never a finite wrong number, and the 0xFF scale marks the run for readers that look at scales alone.
//   x^_i = f32(code_i) * 2^e.
// Layout: codes [rows, K] one byte each (row stride in bytes), scales [rows, K / 32] bytes dense.
#pragma once
#include "vita_common.h"
#include "kv8_rule.h"

constexpr int kMx8Block = 32;        // K elements that share a scale (host side: ops.MX8_BLOCK)

// max |x| of a run as bf16 bits (kv8_absmax_bits: integer order, NaN above inf) -> the scale byte
__device__ __forceinline__ unsigned mx8_scale_byte(const unsigned absmax_bits) {
  if (absmax_bits >= 0x7f80u) return 0xffu;                            // inf or NaN in the run
  if (absmax_bits == 0u) return 127u;
  const int q = (int)(absmax_bits >> 7) - 127;                         // a bf16 subnormal reads as q = -127: clamped below
  int e = (absmax_bits & 0x7fu) <= 0x60u ? q - 8 : q - 7;              // m <= 1.75 ?
  e = e < -126 ? -126 : e;                                             // e <= 120 as it is
  return (unsigned)(e + 127);
}
// 8 bf16 of one lane -> 8 codes (element i in byte i)
__device__ __forceinline__ u32x2 mx8_encode8(const u32x4 x, const unsigned scale_byte) {
  if (scale_byte == 0xffu) return u32x2{0x7f7f7f7fu, 0x7f7f7f7fu};
  return kv8_encode8(x, __uint_as_float(scale_byte << 23));            // x / 2^e, IEEE division by a power of two: exact
}
