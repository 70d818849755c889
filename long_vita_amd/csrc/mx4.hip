// MXFP4 (OCP e2m1 codes + one E8M0 scale per 32 K elements) decoder weights for the cached token step: the quantiser
// that runs once per weight, the single-token GEMV over codes + scales and its form for the 2 .. 8 rows of the multi-row steps (both
// the body FP8's multi-row kernel shares: qgemv.h, with the format's facts in Mx4Format below).  The
// rule and the nibble order are mx4_rule.h's (tests/mx4_cases.py): codes [N, K / 2] (row stride in bytes), scales [N, K / 32] bytes
// dense, 0.266 of the bf16 bytes.  Every e2m1 value is a bf16 value: v_cvt_scalef32_pk_bf16_fp4 turns a byte into a packed bf16 pair
// (scale operand 1.0), the dot product is decode.hip's v_dot2_f32_bf16 on the pairs, and a run's scale (a power of two, exact)
// multiplies the lane's finished 16-element partial in fp32: nothing is rounded to bf16 in front of the epilogue.
#include "vita_common.h"
#include "mx4_rule.h"
#include "qgemv.h"

#include <math.h>

namespace {

// ---- quantiser: item = (row n, run b); its 4 lanes hold 8 elements each and share the maximum by __shfl_xor -------------------------
__global__ __launch_bounds__(256) void mx4_quantize_kernel(const bf16_t* __restrict__ W, int64_t ldw, int64_t N, int nblk,
                                                           unsigned char* __restrict__ codes, int64_t ldc,
                                                           unsigned char* __restrict__ scales) {
  const int sub = threadIdx.x & 3;
  const int64_t items = N * nblk;
  for (int64_t it = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 2; it < items; it += ((int64_t)gridDim.x * blockDim.x) >> 2) {
    const int64_t n = it / nblk;
    const int b = (int)(it - n * nblk);
    const u32x4 x = *reinterpret_cast<const u32x4*>(W + n * ldw + b * kMx4Block + sub * 8);
    unsigned m = kv8_absmax_bits(x);
#pragma unroll
    for (int o = 1; o < 4; o <<= 1) m = max(m, (unsigned)__shfl_xor((int)m, o));
    const unsigned sb = mx4_scale_byte(m);
    *reinterpret_cast<unsigned*>(codes + n * ldc + b * (kMx4Block / 2) + sub * 4) = mx4_encode8(x, sb);
    if (sub == 0) scales[it] = (unsigned char)sb;
  }
}

// ---- y[b][N] = epilogue(dequant(codes, scales)[N,K] . norm(x[b])[K]), b < rows <= R ------------------------------------------------
// qgemv.h's body for the single-token kernel (R = 1, optional folded RMSNorm) and the multi-row kernel (R = 2, 4, 8, no norm), so that
// row b of the latter has the bits of the former on row b by construction (acc = fma(partial, scale, acc)).
// What was chosen and why.  A code row is a quarter of its bf16 bytes, so a wave streams FOUR code rows (outputs 4 w .. 4 w + 3, or
// SWIGLU's gate and up rows of outputs 2 w and 2 w + 1) and a lane takes 8 bytes = 16 codes of each: 32 bytes of codes in flight
// per lane and pass, what gemv_w8_kernel has with 2 rows x 16 bytes, and the x vectors (xa, xb) of a pass are gemv_w8_kernel's.
// 8 bytes, not 16: K = 5120 is 320 vectors of 16 codes = 5 full wave passes, where 160 vectors of 32 codes would leave half the
// wave idle in the third pass (K = 13824: 13.5 against 6.75 passes, the same 96 %).  The price is that two neighbouring lanes load
// the same scale byte and each scales its own partial: per 16 bytes of codes 16 conversions + 16 dot2 + 2 x (shift + fma) = 36
// VALU instructions for 32 elements, against gemv_w8_kernel's 26 for 16.  The scale multiplies the partial rather than riding on
// the conversion: 0 * inf = NaN is then IEEE's word for a non-finite run, not a property of the conversion's scale operand.
struct Mx4Format {
  using codes_t = u32x2;
  using scale_t = unsigned char;
  using held_t = unsigned;
  static constexpr int kScaleShift = 5, kVecShift = 1;
  static constexpr int code_rows(int) { return 4; }
  static __device__ __forceinline__ void decode16(const u32x2 c, unsigned (&p)[8]) {
    mx4_decode8(c[0], &p[0]);
    mx4_decode8(c[1], &p[4]);
  }
  static __device__ __forceinline__ float scale_f32(const unsigned byte) { return mx4_scale_f32(byte); }
  static __device__ __forceinline__ float accumulate(const float acc, const float dot, const float scale) {
    return __builtin_fmaf(dot, scale, acc);
  }
  // K a multiple of the run, code rows of K / 2 bytes at a 16-byte stride from a 16-byte aligned base
  static bool codes_unsupported(const void* codes, int64_t ldc_bytes, int64_t K) {
    return (K & (kMx4Block - 1)) || K >= (int64_t(1) << 31) || (ldc_bytes & 15) || ldc_bytes < K / 2 || ((uintptr_t)codes & 15);
  }
  static constexpr uintptr_t kScaleAlign = 0;                          // scale bytes
  static constexpr int kRowsBelowOne = VITA_ERR_UNSUPPORTED;
};

template <int EPI, bool NORM>
__global__ __launch_bounds__(256) void gemv_mx4_kernel(const bf16_t* __restrict__ x, const unsigned char* __restrict__ codes,
                                                       int64_t ldc, const unsigned char* __restrict__ scales, bf16_t* __restrict__ y,
                                                       int64_t N, int64_t K, const bf16_t* __restrict__ bias,
                                                       const bf16_t* __restrict__ R, const bf16_t* __restrict__ gamma, float eps) {
  qgemv_body<Mx4Format, EPI, 1, NORM>(x, 0, 1, codes, ldc, scales, y, 0, N, K, bias, R, 0, gamma, eps);
}

template <int EPI, int R>
__global__ __launch_bounds__(256) void gemv_rows_mx4_kernel(const bf16_t* __restrict__ x, int64_t ldx, int rows,
                                                            const unsigned char* __restrict__ codes, int64_t ldc,
                                                            const unsigned char* __restrict__ scales, bf16_t* __restrict__ y,
                                                            int64_t ldy, int64_t N, int64_t K, const bf16_t* __restrict__ bias,
                                                            const bf16_t* __restrict__ Res, int64_t ldr) {
  qgemv_body<Mx4Format, EPI, R, false>(x, ldx, rows, codes, ldc, scales, y, ldy, N, K, bias, Res, ldr, nullptr, 0.f);
}

}  // namespace

extern "C" int vita_mx4_quantize(const void* W, int64_t ldw, int64_t N, int64_t K, void* codes, int64_t ldc_bytes, void* scales,
                                 void* stream) {
  if (!W || !codes || !scales || N <= 0 || K <= 0) return VITA_ERR_INVALID_ARG;
  if (Mx4Format::codes_unsupported(codes, ldc_bytes, K) || (ldw & 7) || ldw < K || ((uintptr_t)W & 15) || N > (int64_t(1) << 40) / K)
    return VITA_ERR_UNSUPPORTED;
  const int64_t items = N * (K / kMx4Block);                             // 4 lanes each, 64 per workgroup
  const unsigned blocks = (unsigned)((items + 63) / 64 < 4096 ? (items + 63) / 64 : 4096);
  hipLaunchKernelGGL(mx4_quantize_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)W, ldw, N,
                     (int)(K / kMx4Block), (unsigned char*)codes, ldc_bytes, (unsigned char*)scales);
  return vita_check_launch();
}

extern "C" int vita_gemv_mx4(const void* x, const void* codes, int64_t ldc_bytes, const void* scales, void* y, int64_t N, int64_t K,
                             int epilogue, const void* bias, const void* R, const void* gamma, float eps, void* stream) {
  const int rc = qgemv_refusal<Mx4Format>(x, codes, ldc_bytes, scales, y, N, K, epilogue, bias, R, gamma, eps);
  if (rc != VITA_OK) return rc;
  return qgemv_dispatch_norm(epilogue, gamma != nullptr, [&](auto e, auto norm) {
    constexpr int E = decltype(e)::value;
    hipLaunchKernelGGL((gemv_mx4_kernel<E, decltype(norm)::value>), dim3(qgemv_blocks<Mx4Format, E, 1>(N)), dim3(256), 0,
                       (hipStream_t)stream, (const bf16_t*)x, (const unsigned char*)codes, ldc_bytes, (const unsigned char*)scales,
                       (bf16_t*)y, N, K, (const bf16_t*)bias, (const bf16_t*)R, (const bf16_t*)gamma, norm ? eps : 0.f);
  });
}

extern "C" int vita_gemv_rows_mx4(const void* x, int64_t ldx, int rows, const void* codes, int64_t ldc_bytes, const void* scales, void* y,
                                  int64_t ldy, int64_t N, int64_t K, int epilogue, const void* bias, const void* R, int64_t ldr,
                                  void* stream) {
  const int rc = qgemv_rows_refusal<Mx4Format>(x, ldx, rows, codes, ldc_bytes, scales, y, ldy, N, K, epilogue, bias, R, ldr);
  if (rc != VITA_OK) return rc;
  return qgemv_dispatch_rows(epilogue, rows, [&](auto e, auto r) {
    constexpr int E = decltype(e)::value, RR = decltype(r)::value;
    hipLaunchKernelGGL((gemv_rows_mx4_kernel<E, RR>), dim3(qgemv_blocks<Mx4Format, E, RR>(N)), dim3(256), 0, (hipStream_t)stream,
                       (const bf16_t*)x, ldx, rows, (const unsigned char*)codes, ldc_bytes, (const unsigned char*)scales, (bf16_t*)y, ldy,
                       N, K, (const bf16_t*)bias, (const bf16_t*)R, ldr);
  });
}

