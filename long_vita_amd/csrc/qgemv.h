// The one GEMV body over quantised decoder weights, shared by w8.hip (FP8: e4m3 codes + one fp32 scale per 128 K) and
// mx4.hip (MXFP4: e2m1 codes + one E8M0 byte per 32 K), and the host side's argument checks and dispatch that go with it.  What a
// format is, is written once, as a traits struct F next to its decode helpers (W8Format, Mx4Format):
//   codes_t            a lane's 16 codes of one code row as one vector load (u32x4 / u32x2)
//   scale_t, held_t    a scale in memory, and in the register that waits for its vector's turn (float, float / unsigned char, unsigned)
//   kScaleShift        log2 of the K elements per scale (7 / 5); kVecShift: log2 of the 16-code vectors per scale (3 / 1)
//   code_rows(R)       code rows a wave streams (R == 2 ? 2 : 4 / 4)
//   decode16           16 codes -> 8 packed bf16 pairs, exact;  scale_f32: held_t -> float;  accumulate(acc, dot, scale)
//   codes_unsupported, kScaleAlign, kRowsBelowOne    what the host entries refuse, and with which code (below)
#pragma once
#include "vita_common.h"

#include <type_traits>

// the eight chained dot2 from 0 over a decoded vector: the partial a scale multiplies
__device__ __forceinline__ float qgemv_dot16p(const unsigned (&p)[8], const u32x4 xa, const u32x4 xb) {
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j) s = dot2_bf16(xa[j], p[j], s);
#pragma unroll
  for (int j = 0; j < 4; ++j) s = dot2_bf16(xb[j], p[4 + j], s);
  return s;
}

// ---- y[b][N] = epilogue(dequant(codes, scales)[N,K] . norm(x[b])[K]), b < rows <= R ------------------------------------------------
// R = 1 with an optional folded RMSNorm (gemv_kernel's gemv_rstd and gemv_norm_x) is a single-token kernel, R = 2, 4, 8 without one a
// multi-row kernel.  A wave reads each of its code rows and their scales ONCE for all input rows and decodes a 16-code vector to
// packed bf16 once; every (input row, code row) pair keeps an fp32 accumulator of its own that walks K the same way for every R:
// lane stride 64 over the vectors, qgemv_dot16p, F::accumulate, wave_reduce_sum, gemv_epilogue.  So row b of a multi-row kernel has
// the bits of the format's single-token kernel on row b (FP8's is gemv_w8_kernel, which walks K in these steps).  A wave owns
// F::code_rows(R) code rows; SWIGLU: the gate and up rows of half as many outputs.  R = rows rounded up to 2, 4 or 8: the surplus
// rows recompute row rows - 1 and are not stored; outputs behind N recompute output N - 1 and are not stored.  Code rows behind N
// (2 N), columns behind K and input rows behind rows - 1 are never read.
// The loads are placed by hand (sched_barrier: nothing is scheduled across it), because left alone hipcc sinks every load to its
// first use to save registers and waits for each in turn.  Loads come back in issue order, so per vector: the x vectors of all
// rows (L1 / L2; gamma with them) are issued and fly under the decode of the codes, which were issued one vector earlier; then the
// codes and scales of the NEXT vector (HBM) are issued last and fly under all the dot products of this one.  Behind the last vector
// the same codes are loaded again: never a column behind K.  The order of the arithmetic is not touched.
template <class F, int EPI, int R, bool NORM>
__device__ __forceinline__ void qgemv_body(const bf16_t* __restrict__ x, int64_t ldx, int rows, const unsigned char* __restrict__ codes,
                                           int64_t ldc, const typename F::scale_t* __restrict__ scales, bf16_t* __restrict__ y,
                                           int64_t ldy, int64_t N, int64_t K, const bf16_t* __restrict__ bias,
                                           const bf16_t* __restrict__ Res, int64_t ldr, const bf16_t* __restrict__ gamma, float eps) {
  static_assert(!NORM || R == 1, "the folded RMSNorm is the single-token kernel's");
  using codes_t = typename F::codes_t;
  constexpr bool SW = EPI == VITA_EPI_SWIGLU;
  constexpr int CR = F::code_rows(R), NSUB = SW ? 2 : 1, NOUT = CR / NSUB;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t n0 = ((int64_t)blockIdx.x * 4 + wave) * NOUT;          // first output of this wave
  if (n0 >= N) return;
  const int nvec = (int)(K >> 4), nblk = (int)(K >> F::kScaleShift);
  const u32x4* xr[R];
#pragma unroll
  for (int b = 0; b < R; ++b) xr[b] = reinterpret_cast<const u32x4*>(x + (int64_t)(b < rows ? b : rows - 1) * ldx);
  const u32x4* gr = reinterpret_cast<const u32x4*>(gamma);
  float rstd = 1.f;
  if constexpr (NORM) rstd = gemv_rstd(xr[0], (int)(K >> 3), lane, K, eps);
  const codes_t* cp[NOUT][NSUB];
  const typename F::scale_t* sp[NOUT][NSUB];
  float acc[NOUT][NSUB][R];
#pragma unroll
  for (int o = 0; o < NOUT; ++o) {
    const int64_t n = (n0 + o < N) ? n0 + o : N - 1;                   // clamp: tail outputs recompute output N - 1
#pragma unroll
    for (int s = 0; s < NSUB; ++s) {
      const int64_t r = n + s * N;                                     // SWIGLU: s = 1 is the "up" row
      cp[o][s] = reinterpret_cast<const codes_t*>(codes + r * ldc);
      sp[o][s] = scales + r * nblk;
#pragma unroll
      for (int b = 0; b < R; ++b) acc[o][s][b] = 0.f;
    }
  }
  codes_t cv[NOUT][NSUB];
  typename F::held_t sc[NOUT][NSUB];
  const auto load_codes = [&](const int v) {
#pragma unroll
    for (int o = 0; o < NOUT; ++o) {
#pragma unroll
      for (int s = 0; s < NSUB; ++s) {
        cv[o][s] = cp[o][s][v];
        sc[o][s] = sp[o][s][v >> F::kVecShift];
      }
    }
  };
  if (lane < nvec) load_codes(lane);
  for (int v = lane; v < nvec; v += 64) {
    u32x4 xa[R], xb[R];
#pragma unroll
    for (int b = 0; b < R; ++b) xa[b] = xr[b][2 * v], xb[b] = xr[b][2 * v + 1];
    u32x4 ga, gb;
    if constexpr (NORM) ga = gr[2 * v], gb = gr[2 * v + 1];
    __builtin_amdgcn_sched_barrier(0);
    unsigned p[NOUT][NSUB][8];
    float scv[NOUT][NSUB];
#pragma unroll
    for (int o = 0; o < NOUT; ++o) {
#pragma unroll
      for (int s = 0; s < NSUB; ++s) {
        F::decode16(cv[o][s], p[o][s]);
        scv[o][s] = F::scale_f32(sc[o][s]);
      }
    }
    __builtin_amdgcn_sched_barrier(0);
    load_codes(v + 64 < nvec ? v + 64 : v);
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (NORM) {
      xa[0] = gemv_norm_x(xa[0], rstd, ga);
      xb[0] = gemv_norm_x(xb[0], rstd, gb);
    }
#pragma unroll
    for (int b = 0; b < R; ++b) {
#pragma unroll
      for (int o = 0; o < NOUT; ++o) {
#pragma unroll
        for (int s = 0; s < NSUB; ++s) acc[o][s][b] = F::accumulate(acc[o][s][b], qgemv_dot16p(p[o][s], xa[b], xb[b]), scv[o][s]);
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

// ---- host side ---------------------------------------------------------------------------------------------------------------------
// workgroups of 4 waves over N outputs for a kernel of the body
template <class F, int EPI, int R>
unsigned qgemv_blocks(int64_t N) {
  constexpr int NOUT = F::code_rows(R) / (EPI == VITA_EPI_SWIGLU ? 2 : 1);
  return (unsigned)(((N + NOUT - 1) / NOUT + 3) / 4);
}

template <int V>
using qgemv_int = std::integral_constant<int, V>;

// the epilogues a GEMV has: launch(qgemv_int<EPI>) for one of them, then the launch's status; any other is VITA_ERR_UNSUPPORTED
template <class Launch>
int qgemv_dispatch(int epilogue, Launch&& launch) {
  switch (epilogue) {
    case VITA_EPI_NONE: launch(qgemv_int<VITA_EPI_NONE>{}); break;
    case VITA_EPI_BIAS: launch(qgemv_int<VITA_EPI_BIAS>{}); break;
    case VITA_EPI_RESIDUAL: launch(qgemv_int<VITA_EPI_RESIDUAL>{}); break;
    case VITA_EPI_SWIGLU: launch(qgemv_int<VITA_EPI_SWIGLU>{}); break;
    default: return VITA_ERR_UNSUPPORTED;
  }
  return vita_check_launch();
}
// single token: launch(qgemv_int<EPI>, std::bool_constant<NORM>), NORM = a gamma was given
template <class Launch>
int qgemv_dispatch_norm(int epilogue, bool norm, Launch&& launch) {
  return qgemv_dispatch(epilogue, [&](auto e) {
    if (norm) launch(e, std::true_type{});
    else launch(e, std::false_type{});
  });
}
// multi-row: launch(qgemv_int<EPI>, qgemv_int<R>), R = rows rounded up to 2, 4 or 8
template <class Launch>
int qgemv_dispatch_rows(int epilogue, int rows, Launch&& launch) {
  return qgemv_dispatch(epilogue, [&](auto e) {
    if (rows <= 2) launch(e, qgemv_int<2>{});
    else if (rows <= 4) launch(e, qgemv_int<4>{});
    else launch(e, qgemv_int<8>{});
  });
}

// What vita_gemv_<F> and vita_gemv_rows_<F> refuse before anything is launched; VITA_OK: go on to the dispatch, which refuses the
// epilogue.  Per format: F::codes_unsupported (K a multiple of the block and below 2^31, the code rows' stride and base),
// F::kScaleAlign (the scale pointer's alignment mask: 3 for fp32 scales, 0 for bytes) and F::kRowsBelowOne, the code for rows < 1,
// on which the two formats' entries disagree and their tests pin both.
template <class F>
int qgemv_refusal(const void* x, const void* codes, int64_t ldc_bytes, const void* scales, const void* y, int64_t N, int64_t K,
                  int epilogue, const void* bias, const void* R, const void* gamma, float eps) {
  if (!x || !codes || !scales || !y || N <= 0 || K <= 0) return VITA_ERR_INVALID_ARG;
  if ((epilogue == VITA_EPI_BIAS && !bias) || (epilogue == VITA_EPI_RESIDUAL && !R)) return VITA_ERR_INVALID_ARG;
  if (gamma && !(eps >= 0.f)) return VITA_ERR_INVALID_ARG;
  if (F::codes_unsupported(codes, ldc_bytes, K) || (((uintptr_t)x | (uintptr_t)gamma) & 15) || ((uintptr_t)scales & F::kScaleAlign))
    return VITA_ERR_UNSUPPORTED;                                       // 16-byte x and gamma vectors
  return VITA_OK;
}
template <class F>
int qgemv_rows_refusal(const void* x, int64_t ldx, int rows, const void* codes, int64_t ldc_bytes, const void* scales, const void* y,
                       int64_t ldy, int64_t N, int64_t K, int epilogue, const void* bias, const void* R, int64_t ldr) {
  if (!x || !codes || !scales || !y || N <= 0 || K <= 0) return VITA_ERR_INVALID_ARG;
  if (rows < 1 && F::kRowsBelowOne == VITA_ERR_INVALID_ARG) return VITA_ERR_INVALID_ARG;
  if ((epilogue == VITA_EPI_BIAS && !bias) || (epilogue == VITA_EPI_RESIDUAL && (!R || ldr < N))) return VITA_ERR_INVALID_ARG;
  if (rows < 1 || rows > 8 || F::codes_unsupported(codes, ldc_bytes, K) || (ldx & 7) || ldx < K || ldy < N || ((uintptr_t)x & 15) ||
      ((uintptr_t)scales & F::kScaleAlign))
    return VITA_ERR_UNSUPPORTED;
  return VITA_OK;
}
