// MXFP4 (OCP e2m1 codes + one E8M0 scale per 32 K elements) decoder weights for the cached token step: the quantiser
// that runs once per weight, the single-token GEMV over codes + scales and its form for the 2 .. 8 rows of the multi-row steps.  The
// rule and the nibble order are mx4_rule.h's (tests/mx4_cases.py): codes [N, K / 2] (row stride in bytes), scales [N, K / 32] bytes
// dense, 0.266 of the bf16 bytes.  Every e2m1 value is a bf16 value: v_cvt_scalef32_pk_bf16_fp4 turns a byte into a packed bf16 pair
// (scale operand 1.0), the dot product is decode.hip's v_dot2_f32_bf16 on the pairs, and a run's scale (a power of two, exact)
// multiplies the lane's finished 16-element partial in fp32: nothing is rounded to bf16 in front of the epilogue.
#include "vita_common.h"
#include "mx4_rule.h"

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
// One body for the single-token kernel (R = 1, optional folded RMSNorm) and the multi-row kernel (R = 2, 4, 8, no norm), so that row
// b of the latter has the bits of the former on row b by construction: every (input row, code row) pair keeps an fp32 accumulator
// that walks K the same way (lane stride 64 over the 16-code vectors, eight chained dot2 from 0, acc = fma(partial, scale, acc),
// wave_reduce_sum, gemv_epilogue).
// What was chosen and why.  A code row is a quarter of its bf16 bytes, so a wave streams FOUR code rows (outputs 4 w .. 4 w + 3, or
// SWIGLU's gate and up rows of outputs 2 w and 2 w + 1) and a lane takes 8 bytes = 16 codes of each: 32 bytes of codes in flight
// per lane and pass, what gemv_w8_kernel has with 2 rows x 16 bytes, and the x vectors (xa, xb) of a pass are gemv_w8_kernel's.
// 8 bytes, not 16: K = 5120 is 320 vectors of 16 codes = 5 full wave passes, where 160 vectors of 32 codes would leave half the
// wave idle in the third pass (K = 13824: 13.5 against 6.75 passes, the same 96 %).  The price is that two neighbouring lanes load
// the same scale byte and each scales its own partial: per 16 bytes of codes 16 conversions + 16 dot2 + 2 x (shift + fma) = 36
// VALU instructions for 32 elements, against gemv_w8_kernel's 26 for 16.  The scale multiplies the partial rather than riding on
// the conversion: 0 * inf = NaN is then IEEE's word for a non-finite run, not a property of the conversion's scale operand.
// The loads are placed by hand as in gemv_rows_w8_kernel (sched_barrier: nothing is scheduled across it): per vector the x vectors
// (L1 / L2; gamma with them) are issued and fly under the decode of the codes that were issued one vector earlier; then the codes
// and scale bytes of the NEXT vector (HBM) are issued and fly under all the dot products of this one.  Behind the last vector the
// same codes are loaded again: never a column behind K.  R = rows rounded up: surplus rows recompute row rows - 1 and are not
// stored; outputs behind N recompute output N - 1 and are not stored.  Code rows behind N (2 N), columns behind K and input rows
// behind rows - 1 are never read.
__device__ __forceinline__ float mx4_dot16p(const unsigned (&p)[8], const u32x4 xa, const u32x4 xb) {
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j) s = dot2_bf16(xa[j], p[j], s);
#pragma unroll
  for (int j = 0; j < 4; ++j) s = dot2_bf16(xb[j], p[4 + j], s);
  return s;
}

template <int EPI, int R, bool NORM>
__device__ __forceinline__ void mx4_gemv_body(const bf16_t* __restrict__ x, int64_t ldx, int rows,
                                              const unsigned char* __restrict__ codes, int64_t ldc,
                                              const unsigned char* __restrict__ scales, bf16_t* __restrict__ y, int64_t ldy, int64_t N,
                                              int64_t K, const bf16_t* __restrict__ bias, const bf16_t* __restrict__ Res, int64_t ldr,
                                              const bf16_t* __restrict__ gamma, float eps) {
  static_assert(!NORM || R == 1, "the folded RMSNorm is the single-token kernel's");
  constexpr bool SW = EPI == VITA_EPI_SWIGLU;
  constexpr int CR = 4, NSUB = SW ? 2 : 1, NOUT = CR / NSUB;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t n0 = ((int64_t)blockIdx.x * 4 + wave) * NOUT;          // first output of this wave
  if (n0 >= N) return;
  const int nvec = (int)(K >> 4), nblk = (int)(K >> 5);
  const u32x4* xr[R];
#pragma unroll
  for (int b = 0; b < R; ++b) xr[b] = reinterpret_cast<const u32x4*>(x + (int64_t)(b < rows ? b : rows - 1) * ldx);
  const u32x4* gr = reinterpret_cast<const u32x4*>(gamma);
  float rstd = 1.f;
  if (NORM) rstd = gemv_rstd(xr[0], (int)(K >> 3), lane, K, eps);
  const u32x2* cp[NOUT][NSUB];
  const unsigned char* sp[NOUT][NSUB];
  float acc[NOUT][NSUB][R];
#pragma unroll
  for (int o = 0; o < NOUT; ++o) {
    const int64_t n = (n0 + o < N) ? n0 + o : N - 1;                   // clamp: tail outputs recompute output N - 1
#pragma unroll
    for (int s = 0; s < NSUB; ++s) {
      const int64_t r = n + s * N;                                     // SWIGLU: s = 1 is the "up" row
      cp[o][s] = reinterpret_cast<const u32x2*>(codes + r * ldc);
      sp[o][s] = scales + r * nblk;
#pragma unroll
      for (int b = 0; b < R; ++b) acc[o][s][b] = 0.f;
    }
  }
  u32x2 cv[NOUT][NSUB];
  unsigned sc[NOUT][NSUB];
  const auto load_codes = [&](const int v) {
#pragma unroll
    for (int o = 0; o < NOUT; ++o) {
#pragma unroll
      for (int s = 0; s < NSUB; ++s) {
        cv[o][s] = cp[o][s][v];
        sc[o][s] = sp[o][s][v >> 1];
      }
    }
  };
  if (lane < nvec) load_codes(lane);
  for (int v = lane; v < nvec; v += 64) {
    u32x4 xa[R], xb[R];
#pragma unroll
    for (int b = 0; b < R; ++b) xa[b] = xr[b][2 * v], xb[b] = xr[b][2 * v + 1];
    u32x4 ga, gb;
    if (NORM) ga = gr[2 * v], gb = gr[2 * v + 1];
    __builtin_amdgcn_sched_barrier(0);
    unsigned p[NOUT][NSUB][8];
    float scv[NOUT][NSUB];
#pragma unroll
    for (int o = 0; o < NOUT; ++o) {
#pragma unroll
      for (int s = 0; s < NSUB; ++s) {
        mx4_decode8(cv[o][s][0], &p[o][s][0]);
        mx4_decode8(cv[o][s][1], &p[o][s][4]);
        scv[o][s] = mx4_scale_f32(sc[o][s]);
      }
    }
    __builtin_amdgcn_sched_barrier(0);
    load_codes(v + 64 < nvec ? v + 64 : v);
    __builtin_amdgcn_sched_barrier(0);
    if (NORM) {
      xa[0] = gemv_norm_x(xa[0], rstd, ga);
      xb[0] = gemv_norm_x(xb[0], rstd, gb);
    }
#pragma unroll
    for (int b = 0; b < R; ++b) {
#pragma unroll
      for (int o = 0; o < NOUT; ++o) {
#pragma unroll
        for (int s = 0; s < NSUB; ++s) acc[o][s][b] = __builtin_fmaf(mx4_dot16p(p[o][s], xa[b], xb[b]), scv[o][s], acc[o][s][b]);
      }
    }
  }
#pragma unroll
  for (int o = 0; o < NOUT; ++o) {
#pragma unroll
    for (int b = 0; b < R; ++b) {
      const float t0 = wave_reduce_sum(acc[o][0][b]);
      const float t1 = SW ? wave_reduce_sum(acc[o][NSUB - 1][b]) : 0.f;
      const int64_t n = n0 + o;
      if (lane != 0 || n >= N || b >= rows) continue;
      y[(int64_t)b * ldy + n] = gemv_epilogue<EPI>(t0, t1, GEMV_ELEM(VITA_EPI_BIAS, bias, n), GEMV_ELEM(VITA_EPI_RESIDUAL, Res, (int64_t)b * ldr + n));
    }
  }
}

template <int EPI, bool NORM>
__global__ __launch_bounds__(256) void gemv_mx4_kernel(const bf16_t* __restrict__ x, const unsigned char* __restrict__ codes,
                                                       int64_t ldc, const unsigned char* __restrict__ scales, bf16_t* __restrict__ y,
                                                       int64_t N, int64_t K, const bf16_t* __restrict__ bias,
                                                       const bf16_t* __restrict__ R, const bf16_t* __restrict__ gamma, float eps) {
  mx4_gemv_body<EPI, 1, NORM>(x, 0, 1, codes, ldc, scales, y, 0, N, K, bias, R, 0, gamma, eps);
}

template <int EPI, int R>
__global__ __launch_bounds__(256) void gemv_rows_mx4_kernel(const bf16_t* __restrict__ x, int64_t ldx, int rows,
                                                            const unsigned char* __restrict__ codes, int64_t ldc,
                                                            const unsigned char* __restrict__ scales, bf16_t* __restrict__ y,
                                                            int64_t ldy, int64_t N, int64_t K, const bf16_t* __restrict__ bias,
                                                            const bf16_t* __restrict__ Res, int64_t ldr) {
  mx4_gemv_body<EPI, R, false>(x, ldx, rows, codes, ldc, scales, y, ldy, N, K, bias, Res, ldr, nullptr, 0.f);
}

// workgroups of 4 waves, NOUT outputs per wave
template <int EPI>
unsigned mx4_blocks(int64_t N) {
  constexpr int NOUT = EPI == VITA_EPI_SWIGLU ? 2 : 4;
  return (unsigned)(((N + NOUT - 1) / NOUT + 3) / 4);
}

template <int EPI, bool NORM>
void launch_gemv_mx4(const void* x, const void* codes, int64_t ldc, const void* scales, void* y, int64_t N, int64_t K, const void* bias,
                     const void* R, const void* gamma, float eps, hipStream_t st) {
  hipLaunchKernelGGL((gemv_mx4_kernel<EPI, NORM>), dim3(mx4_blocks<EPI>(N)), dim3(256), 0, st, (const bf16_t*)x,
                     (const unsigned char*)codes, ldc, (const unsigned char*)scales, (bf16_t*)y, N, K, (const bf16_t*)bias,
                     (const bf16_t*)R, (const bf16_t*)gamma, eps);
}

template <int EPI>
void launch_gemv_rows_mx4(const void* x, int64_t ldx, int rows, const void* codes, int64_t ldc, const void* scales, void* y, int64_t ldy,
                          int64_t N, int64_t K, const void* bias, const void* R, int64_t ldr, hipStream_t st) {
#define VITA_GRMX4(RR)                                                                                                          \
  hipLaunchKernelGGL((gemv_rows_mx4_kernel<EPI, RR>), dim3(mx4_blocks<EPI>(N)), dim3(256), 0, st, (const bf16_t*)x, ldx, rows,  \
                     (const unsigned char*)codes, ldc, (const unsigned char*)scales, (bf16_t*)y, ldy, N, K, (const bf16_t*)bias, \
                     (const bf16_t*)R, ldr);
  if (rows <= 2) { VITA_GRMX4(2) } else if (rows <= 4) { VITA_GRMX4(4) } else { VITA_GRMX4(8) }
#undef VITA_GRMX4
}

// K a multiple of the run, code rows of K / 2 bytes at a 16-byte stride from a 16-byte aligned base
bool mx4_codes_unsupported(const void* codes, int64_t ldc_bytes, int64_t K) {
  return (K & (kMx4Block - 1)) || K >= (int64_t(1) << 31) || (ldc_bytes & 15) || ldc_bytes < K / 2 || ((uintptr_t)codes & 15);
}

}  // namespace

extern "C" int vita_mx4_quantize(const void* W, int64_t ldw, int64_t N, int64_t K, void* codes, int64_t ldc_bytes, void* scales,
                                 void* stream) {
  if (!W || !codes || !scales || N <= 0 || K <= 0) return VITA_ERR_INVALID_ARG;
  if (mx4_codes_unsupported(codes, ldc_bytes, K) || (ldw & 7) || ldw < K || ((uintptr_t)W & 15) || N > (int64_t(1) << 40) / K)
    return VITA_ERR_UNSUPPORTED;
  const int64_t items = N * (K / kMx4Block);                             // 4 lanes each, 64 per workgroup
  const unsigned blocks = (unsigned)((items + 63) / 64 < 4096 ? (items + 63) / 64 : 4096);
  hipLaunchKernelGGL(mx4_quantize_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)W, ldw, N,
                     (int)(K / kMx4Block), (unsigned char*)codes, ldc_bytes, (unsigned char*)scales);
  return vita_check_launch();
}

extern "C" int vita_gemv_mx4(const void* x, const void* codes, int64_t ldc_bytes, const void* scales, void* y, int64_t N, int64_t K,
                             int epilogue, const void* bias, const void* R, const void* gamma, float eps, void* stream) {
  if (!x || !codes || !scales || !y || N <= 0 || K <= 0) return VITA_ERR_INVALID_ARG;
  if ((epilogue == VITA_EPI_BIAS && !bias) || (epilogue == VITA_EPI_RESIDUAL && !R)) return VITA_ERR_INVALID_ARG;
  if (gamma && !(eps >= 0.f)) return VITA_ERR_INVALID_ARG;
  if (mx4_codes_unsupported(codes, ldc_bytes, K) || (((uintptr_t)x | (uintptr_t)gamma) & 15))       // 16-byte x and gamma vectors
    return VITA_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
#define VITA_GMX4(E)                                                                                      \
  case E:                                                                                                 \
    if (gamma) launch_gemv_mx4<E, true>(x, codes, ldc_bytes, scales, y, N, K, bias, R, gamma, eps, st);   \
    else launch_gemv_mx4<E, false>(x, codes, ldc_bytes, scales, y, N, K, bias, R, nullptr, 0.f, st);      \
    break;
  switch (epilogue) {
    VITA_GMX4(VITA_EPI_NONE) VITA_GMX4(VITA_EPI_BIAS) VITA_GMX4(VITA_EPI_RESIDUAL) VITA_GMX4(VITA_EPI_SWIGLU)
    default: return VITA_ERR_UNSUPPORTED;
  }
#undef VITA_GMX4
  return vita_check_launch();
}

extern "C" int vita_gemv_rows_mx4(const void* x, int64_t ldx, int rows, const void* codes, int64_t ldc_bytes, const void* scales, void* y,
                                  int64_t ldy, int64_t N, int64_t K, int epilogue, const void* bias, const void* R, int64_t ldr,
                                  void* stream) {
  if (!x || !codes || !scales || !y || N <= 0 || K <= 0) return VITA_ERR_INVALID_ARG;
  if ((epilogue == VITA_EPI_BIAS && !bias) || (epilogue == VITA_EPI_RESIDUAL && (!R || ldr < N))) return VITA_ERR_INVALID_ARG;
  if (rows < 1 || rows > 8 || mx4_codes_unsupported(codes, ldc_bytes, K) || (ldx & 7) || ldx < K || ldy < N || ((uintptr_t)x & 15))
    return VITA_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
#define VITA_GRMX4E(E) \
  case E: launch_gemv_rows_mx4<E>(x, ldx, rows, codes, ldc_bytes, scales, y, ldy, N, K, bias, R, ldr, st); break;
  switch (epilogue) {
    VITA_GRMX4E(VITA_EPI_NONE) VITA_GRMX4E(VITA_EPI_BIAS) VITA_GRMX4E(VITA_EPI_RESIDUAL) VITA_GRMX4E(VITA_EPI_SWIGLU)
    default: return VITA_ERR_UNSUPPORTED;
  }
#undef VITA_GRMX4E
  return vita_check_launch();
}
