// The e4m3 quantisation rule of the FP8 KV cache (kv8.hip) and of the FP8 decoder weights (w8.hip), on 8 bf16 values per lane:
//   amax = max |x_i| over the run that shares a scale ; s = amax > 0 ? amax / 448 : 1 ; c_i = e4m3fn_rne(x_i / s) ; x^_i = f32(c_i) * s
// fp32, IEEE division, no clamp.  The run is a K or V head row of 128 elements there, 128 consecutive K elements of a weight row here;
// the lanes of a run combine their kv8_absmax_bits with an integer maximum.  tests/kv8_cases.py is the same rule in torch.
#pragma once
#include "vita_common.h"

// |x| as integers orders like the floats and puts every NaN above inf: the maximum is exact and carries a NaN through.
__device__ __forceinline__ unsigned kv8_absmax_bits(const u32x4 a) {
  unsigned m = 0u;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    m = max(m, a[j] & 0x7fffu);
    m = max(m, (a[j] >> 16) & 0x7fffu);
  }
  return m;
}
__device__ __forceinline__ float kv8_scale(unsigned absmax_bits) {
  const float amax = __uint_as_float(absmax_bits << 16);
  return amax > 0.f ? amax / 448.0f : 1.0f;
}
__device__ __forceinline__ u32x2 kv8_encode8(const u32x4 x, const float s) {
  u32x2 c;
#pragma unroll
  for (int w = 0; w < 2; ++w) {
    int v = 0;
    v = __builtin_amdgcn_cvt_pk_fp8_f32(bf16lo_to_f32(x[2 * w]) / s, bf16hi_to_f32(x[2 * w]) / s, v, false);
    v = __builtin_amdgcn_cvt_pk_fp8_f32(bf16lo_to_f32(x[2 * w + 1]) / s, bf16hi_to_f32(x[2 * w + 1]) / s, v, true);
    c[w] = (unsigned)v;
  }
  return c;
}
// The rule for reading a cache row back as bf16 (vita_kv8_load; the one-pass extend behind an FP8 cache): x~_i = bf16_rne(f32(c_i) * s),
// one fp32 multiply rounded to fp32, then one RNE conversion to bf16.  Non-finite stays non-finite: a NaN code or a NaN scale gives NaN,
// an inf scale inf (or NaN on a zero code).  In torch: (codes.float() * scales[..., None]).to(torch.bfloat16).
__device__ __forceinline__ u32x4 kv8_readback8(const u32x2 c, const float s) {
  u32x4 x;
#pragma unroll
  for (int w = 0; w < 2; ++w) {
    const auto lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)c[w], false);
    const auto hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)c[w], true);
    x[2 * w] = pack_bf16x2(lo[0] * s, lo[1] * s);
    x[2 * w + 1] = pack_bf16x2(hi[0] * s, hi[1] * s);
  }
  return x;
}
// 4 codes of one word -> two packed bf16 pairs (exact)
__device__ __forceinline__ void kv8_decode4(const unsigned w, unsigned& p0, unsigned& p1) {
  const auto lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, false);
  const auto hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, true);
  p0 = pack_bf16x2(lo[0], lo[1]);
  p1 = pack_bf16x2(hi[0], hi[1]);
}
