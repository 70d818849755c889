// FP8 (OCP e4m3fn) decoder weights for the cached token step: the quantiser that runs once per weight, the
// single-token GEMV over codes + scales and its form for the 2 .. 8 rows of the multi-row steps (the body MXFP4 shares: qgemv.h,
// with the format's facts in W8Format below).  The rule is the KV cache's
// (kv8_rule.h, tests/kv8_cases.py), applied to every run of 128 consecutive K elements of one weight row W[n, 128 b .. 128 b + 127]:
// codes [N, K] (1 byte, row stride in bytes), scales [N, K / 128] fp32 dense, 0.516 of the bf16 bytes.  Every e4m3 value is a bf16
// value, so the dot product is decode.hip's v_dot2_f32_bf16 on the codes; a block's scale multiplies the lane's finished 16-element
// partial, and nothing is rounded to bf16 in front of the epilogue.
#include "vita_common.h"
#include "kv8_rule.h"
#include "qgemv.h"

#include <math.h>

namespace {

constexpr int kW8Block = 128;        // K elements that share a scale (host side: ops.W8_BLOCK)

// ---- quantiser: item = (row n, block b); its 16 lanes hold 8 elements each, as kv8_store_kernel ------------------------------------
__global__ __launch_bounds__(256) void w8_quantize_kernel(const bf16_t* __restrict__ W, int64_t ldw, int64_t N, int nblk,
                                                          unsigned char* __restrict__ codes, int64_t ldc,
                                                          float* __restrict__ scales) {
  const int sub = threadIdx.x & 15;
  const int64_t items = N * nblk;
  for (int64_t it = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 4; it < items; it += ((int64_t)gridDim.x * blockDim.x) >> 4) {
    const int64_t n = it / nblk;
    const int b = (int)(it - n * nblk);
    const u32x4 x = *reinterpret_cast<const u32x4*>(W + n * ldw + b * kW8Block + sub * 8);
    unsigned m = kv8_absmax_bits(x);
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) m = max(m, (unsigned)__shfl_xor((int)m, o));
    const float s = kv8_scale(m);
    *reinterpret_cast<u32x2*>(codes + n * ldc + b * kW8Block + sub * 8) = kv8_encode8(x, s);
    if (sub == 0) scales[it] = s;
  }
}

// ---- y[N] = epilogue(dequant(codes, scales)[N,K] . norm(x)[K]) ----------------------------------------------------------------------
// A row is half the bytes it has in bf16, so one wave streams TWO code rows, which keeps as many 16-byte loads in flight per wave
// as gemv_kernel has: outputs 2 w and 2 w + 1, or SWIGLU's gate and up rows of output w.  A lane loads 16 codes as one 16-byte
// vector, so 8 neighbouring lanes cover one scale block and a wave pass covers 1024 columns; the block's scale is one more
// (broadcast) 4-byte load per vector.  Per 16 bytes of codes: 8 v_cvt_pk_f32_fp8 + 8 v_cvt_pk_bf16_f32 + 8 v_dot2 + 2 for the
// scale = 26 VALU instructions, against 16 bytes every ~34 lane-cycles that HBM delivers per CU: the kernel stays HBM-bound.
// NORM: gemv_kernel's rstd (gemv_rstd) and gemv_norm_x, so the normalised x has the bits it has on the bf16 path.
// Rows behind N (an odd N's second row recomputes row N - 1 and stores nothing) and columns behind K are never read.
// w8_dot16 = w8_decode16 (16 codes -> 8 packed bf16 pairs) + qgemv_dot16p (the eight chained dot2 from 0): qgemv.h's body decodes a
// vector once and runs the chain once per input row.
__device__ __forceinline__ void w8_decode16(const u32x4 c, unsigned (&p)[8]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) kv8_decode4(c[j], p[2 * j], p[2 * j + 1]);
}
__device__ __forceinline__ float w8_dot16(const u32x4 c, const u32x4 xa, const u32x4 xb) {
  unsigned p[8];
  w8_decode16(c, p);
  return qgemv_dot16p(p, xa, xb);
}

template <int EPI, bool NORM>
__global__ __launch_bounds__(256) void gemv_w8_kernel(const bf16_t* __restrict__ x, const unsigned char* __restrict__ codes,
                                                      int64_t ldc, const float* __restrict__ scales, bf16_t* __restrict__ y,
                                                      int64_t N, int64_t K, const bf16_t* __restrict__ bias,
                                                      const bf16_t* __restrict__ R, const bf16_t* __restrict__ gamma, float eps) {
  constexpr bool SW = EPI == VITA_EPI_SWIGLU;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t w = (int64_t)blockIdx.x * 4 + wave;
  const int64_t n0 = SW ? w : 2 * w;                                   // first output of this wave
  if (n0 >= N) return;
  const int64_t r0 = n0;                                               // the two code rows
  const int64_t r1 = SW ? n0 + N : (n0 + 1 < N ? n0 + 1 : N - 1);
  const int nvec = (int)(K >> 4), nblk = (int)(K >> 7);
  const u32x4* xr = reinterpret_cast<const u32x4*>(x);
  const u32x4* gr = reinterpret_cast<const u32x4*>(gamma);
  float rstd = 1.f;
  if (NORM) rstd = gemv_rstd(xr, (int)(K >> 3), lane, K, eps);
  const u32x4* c0 = reinterpret_cast<const u32x4*>(codes + r0 * ldc);
  const u32x4* c1 = reinterpret_cast<const u32x4*>(codes + r1 * ldc);
  const float* s0p = scales + r0 * nblk;
  const float* s1p = scales + r1 * nblk;
  float a0 = 0.f, a1 = 0.f;
#pragma unroll 4
  for (int v = lane; v < nvec; v += 64) {
    const u32x4 cv0 = c0[v], cv1 = c1[v];
    const float sc0 = s0p[v >> 3], sc1 = s1p[v >> 3];
    u32x4 xa = xr[2 * v], xb = xr[2 * v + 1];
    if (NORM) {
      xa = gemv_norm_x(xa, rstd, gr[2 * v]);
      xb = gemv_norm_x(xb, rstd, gr[2 * v + 1]);
    }
    a0 += w8_dot16(cv0, xa, xb) * sc0;
    a1 += w8_dot16(cv1, xa, xb) * sc1;
  }
  const float t0 = wave_reduce_sum(a0);
  const float t1 = wave_reduce_sum(a1);
  if (lane != 0) return;
  if (SW) {
    y[n0] = gemv_epilogue<EPI>(t0, t1, 0.f, 0.f);
  } else {
    y[n0] = gemv_epilogue<EPI>(t0, 0.f, GEMV_ELEM(VITA_EPI_BIAS, bias, n0), GEMV_ELEM(VITA_EPI_RESIDUAL, R, n0));
    if (n0 + 1 < N)
      y[n0 + 1] = gemv_epilogue<EPI>(t1, 0.f, GEMV_ELEM(VITA_EPI_BIAS, bias, n0 + 1), GEMV_ELEM(VITA_EPI_RESIDUAL, R, n0 + 1));
  }
}

template <int EPI, bool NORM>
void launch_gemv_w8(const void* x, const void* codes, int64_t ldc, const void* scales, void* y, int64_t N, int64_t K, const void* bias,
                    const void* R, const void* gamma, float eps, hipStream_t st) {
  const int64_t waves = EPI == VITA_EPI_SWIGLU ? N : (N + 1) / 2;
  hipLaunchKernelGGL((gemv_w8_kernel<EPI, NORM>), dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, st, (const bf16_t*)x,
                     (const unsigned char*)codes, ldc, (const float*)scales, (bf16_t*)y, N, K, (const bf16_t*)bias, (const bf16_t*)R,
                     (const bf16_t*)gamma, eps);
}

// ---- y[b][N] = epilogue(dequant(codes, scales)[N,K] . x[b][K]) for b < rows <= 8: the multi-row decode steps on FP8 weights --------
// gemv_rows_kernel's promise on gemv_w8_kernel's arithmetic, by qgemv.h's body: it walks K exactly as gemv_w8_kernel does (lane stride
// 64 over the vectors, the chain from 0, acc += partial * scale, wave_reduce_sum, gemv_epilogue), so row b has the bits of
// vita_gemv_w8 on row b.  No folded RMSNorm: a wave would redo every row's ~40 VALU instructions per 8 elements for the few code
// rows it owns; the steps normalise once with vita_rmsnorm_fwd.  A wave owns 2 code rows at R = 2 as gemv_w8_kernel,
// 4 at R = 4 and 8, which halves the x bytes (R x 32 per lane and vector, from L1 / L2) that go with a byte of codes.
struct W8Format {
  using codes_t = u32x4;
  using scale_t = float;
  using held_t = float;
  static constexpr int kScaleShift = 7, kVecShift = 3;
  static constexpr int code_rows(int R) { return R == 2 ? 2 : 4; }
  static __device__ __forceinline__ void decode16(const u32x4 c, unsigned (&p)[8]) { w8_decode16(c, p); }
  static __device__ __forceinline__ float scale_f32(const float s) { return s; }
  static __device__ __forceinline__ float accumulate(const float acc, const float dot, const float scale) { return acc + dot * scale; }
  // K a multiple of the block, code rows of K bytes at a 16-byte stride from a 16-byte aligned base
  static bool codes_unsupported(const void* codes, int64_t ldc_bytes, int64_t K) {
    return (K & (kW8Block - 1)) || K >= (int64_t(1) << 31) || (ldc_bytes & 15) || ldc_bytes < K || ((uintptr_t)codes & 15);
  }
  static constexpr uintptr_t kScaleAlign = 3;                          // fp32 scales
  static constexpr int kRowsBelowOne = VITA_ERR_INVALID_ARG;
};

template <int EPI, int R>
__global__ __launch_bounds__(256) void gemv_rows_w8_kernel(const bf16_t* __restrict__ x, int64_t ldx, int rows,
                                                           const unsigned char* __restrict__ codes, int64_t ldc,
                                                           const float* __restrict__ scales, bf16_t* __restrict__ y, int64_t ldy,
                                                           int64_t N, int64_t K, const bf16_t* __restrict__ bias,
                                                           const bf16_t* __restrict__ Res, int64_t ldr) {
  qgemv_body<W8Format, EPI, R, false>(x, ldx, rows, codes, ldc, scales, y, ldy, N, K, bias, Res, ldr, nullptr, 0.f);
}

}  // namespace

extern "C" int vita_w8_quantize(const void* W, int64_t ldw, int64_t N, int64_t K, void* codes, int64_t ldc_bytes, void* scales,
                                void* stream) {
  if (!W || !codes || !scales || N <= 0 || K <= 0) return VITA_ERR_INVALID_ARG;
  // not W8Format::codes_unsupported: the quantiser has no 32-bit K (N K <= 2^40 is its bound)
  if ((K & (kW8Block - 1)) || (ldw & 7) || ldw < K || (ldc_bytes & 15) || ldc_bytes < K ||
      (((uintptr_t)W | (uintptr_t)codes) & 15) || ((uintptr_t)scales & 3) || N > (int64_t(1) << 40) / K)
    return VITA_ERR_UNSUPPORTED;
  const int64_t items = N * (K / kW8Block);                              // 16 lanes each, 16 per workgroup
  const unsigned blocks = (unsigned)((items + 15) / 16 < 4096 ? (items + 15) / 16 : 4096);
  hipLaunchKernelGGL(w8_quantize_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)W, ldw, N,
                     (int)(K / kW8Block), (unsigned char*)codes, ldc_bytes, (float*)scales);
  return vita_check_launch();
}

extern "C" int vita_gemv_w8(const void* x, const void* codes, int64_t ldc_bytes, const void* scales, void* y, int64_t N, int64_t K,
                            int epilogue, const void* bias, const void* R, const void* gamma, float eps, void* stream) {
  const int rc = qgemv_refusal<W8Format>(x, codes, ldc_bytes, scales, y, N, K, epilogue, bias, R, gamma, eps);
  if (rc != VITA_OK) return rc;
  return qgemv_dispatch_norm(epilogue, gamma != nullptr, [&](auto e, auto norm) {
    launch_gemv_w8<decltype(e)::value, decltype(norm)::value>(x, codes, ldc_bytes, scales, y, N, K, bias, R, gamma, norm ? eps : 0.f,
                                                              (hipStream_t)stream);
  });
}

extern "C" int vita_gemv_rows_w8(const void* x, int64_t ldx, int rows, const void* codes, int64_t ldc_bytes, const void* scales, void* y,
                                 int64_t ldy, int64_t N, int64_t K, int epilogue, const void* bias, const void* R, int64_t ldr,
                                 void* stream) {
  const int rc = qgemv_rows_refusal<W8Format>(x, ldx, rows, codes, ldc_bytes, scales, y, ldy, N, K, epilogue, bias, R, ldr);
  if (rc != VITA_OK) return rc;
  return qgemv_dispatch_rows(epilogue, rows, [&](auto e, auto r) {
    constexpr int E = decltype(e)::value, RR = decltype(r)::value;
    hipLaunchKernelGGL((gemv_rows_w8_kernel<E, RR>), dim3(qgemv_blocks<W8Format, E, RR>(N)), dim3(256), 0, (hipStream_t)stream,
                       (const bf16_t*)x, ldx, rows, (const unsigned char*)codes, ldc_bytes, (const float*)scales, (bf16_t*)y, ldy, N, K,
                       (const bf16_t*)bias, (const bf16_t*)R, ldr);
  });
}
