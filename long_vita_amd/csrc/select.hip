// Token choice on the device: transformers' RepetitionPenaltyLogitsProcessor -> TemperatureLogitsWarper -> TopKLogitsWarper ->
// TopPLogitsWarper -> multinomial (greedy: arg-max of the penalised scores), in the order `generate` applies them for the checkpoint's
// generation_config.json (H/models/long_vita_qwen2_intern/generation_config.json:4-12; tools/inference_long_vita.py:820-826,868).
//
// One workgroup of 1024 threads per row of bf16 logits.  Pass A turns the logits into fp32 scores (penalty, temperature), stores them in the
// workspace and finds the arg-max.  The k-th largest score and the top-p cut are both found by an 8-bit radix select over order-preserving
// 32-bit keys of the scores: four passes, each one an LDS histogram of the digit below the prefix found so far, weighted 1 (top-k) or by
// the token's mass (top-p).  Masses are exp(x - max) * 2^40 as 64-bit integers: their sums are exact and independent of the order of the
// LDS atomics, so every decision is bit-reproducible; the inverse CDF is an exact integer prefix scan in id order.  A mass is at most
// 2^40, so a row of up to 2^23 columns sums below 2^63: the launcher refuses more.
#include "vita_common.h"
#include <math.h>

namespace {

typedef unsigned long long u64;
constexpr int SEL_THREADS = 1024, SEL_WAVES = SEL_THREADS / 64;
constexpr int64_t SEL_MAX_COLS = 1 << 23;                 // cols * 2^40 (every mass at its maximum) stays below 2^63
// The histogram is [bin][copy]: the high bits of scores are nearly all alike, so the lanes of a wave mostly hit ONE bin and would serialise
// on one address.  Counts (top-k) are 32-bit with 32 copies, lane l adding to copy l & 31: the 32 lanes of a half-wave always fall on 32
// different banks, whatever their bins.  Masses (top-p) are 64-bit with 16 copies in the same 32 KiB.
constexpr int HIST_BINS = 256, MASS_COPIES = 16, COUNT_COPIES = 32;

struct SelShared {
  u64 hist[HIST_BINS * MASS_COPIES];                      // or unsigned [HIST_BINS * COUNT_COPIES]
  u64 bins[HIST_BINS];
  u64 wave_mass[SEL_WAVES];
  unsigned wave_cnt[SEL_WAVES];
  float red_x[SEL_WAVES];
  int red_i[SEL_WAVES];
  u64 pick_above, pick_target;
  unsigned pick_digit;
};

// order-preserving: a > b as floats (finite, -0 canonicalised to +0)  <=>  key(a) > key(b) as unsigned
__device__ __forceinline__ unsigned score_key(float x) {
  const unsigned u = __float_as_uint(x);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
// exp(x - max) in (0, 1] as 2^-40 fixed point (the scaling by a power of two is exact; the conversion truncates)
__device__ __forceinline__ u64 score_mass(float x, float mx) { return (u64)(expf(x - mx) * 1099511627776.f); }

__device__ __forceinline__ u64 shfl_up_u64(u64 v, int d) {
  const unsigned lo = __shfl_up((unsigned)v, d, 64), hi = __shfl_up((unsigned)(v >> 32), d, 64);
  return ((u64)hi << 32) | lo;
}
__device__ __forceinline__ u64 shfl_u64(u64 v, int lane) {
  const unsigned lo = __shfl((unsigned)v, lane, 64), hi = __shfl((unsigned)(v >> 32), lane, 64);
  return ((u64)hi << 32) | lo;
}
__device__ __forceinline__ u64 wave_incl_scan_u64(u64 v, int lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const u64 o = shfl_up_u64(v, d);
    if (lane >= d) v += o;
  }
  return v;
}

// f(v, x[8]) for the score vectors v = first, first + stride, ... < v_end
template <class F>
__device__ __forceinline__ void for_each_score_vec(const float* __restrict__ sc, int first, int v_end, int stride, F&& f) {
  for (int v = first; v < v_end; v += stride) {
    const f32x4 lo = *reinterpret_cast<const f32x4*>(sc + (int64_t)v * 8), hi = *reinterpret_cast<const f32x4*>(sc + (int64_t)v * 8 + 4);
    const float x[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    f(v, x);
  }
}

// The digit d with above(d) < target <= above(d) + bins[d], above(d) = the sum of the bins of all higher digits, into sh.pick_digit /
// sh.pick_above.  top_p > 0: the target is the top-p cut ceil(top_p * total) of this histogram's total, left in sh.pick_target.
// Called by the whole block behind a barrier that completed the histogram; ends with a barrier.
__device__ void hist_pick(SelShared& sh, u64 target, float top_p, bool mass) {
  const int t = threadIdx.x;
  if (t < HIST_BINS) {
    u64 s = 0;
    if (mass) {
#pragma unroll
      for (int c = 0; c < MASS_COPIES; ++c) s += sh.hist[t * MASS_COPIES + c];
    } else {
      const unsigned* cnt = reinterpret_cast<const unsigned*>(sh.hist);
#pragma unroll
      for (int c = 0; c < COUNT_COPIES; ++c) s += cnt[t * COUNT_COPIES + c];
    }
    sh.bins[t] = s;
  }
  if (t == 0) { sh.pick_digit = 0; sh.pick_above = 0; sh.pick_target = target; }
  __syncthreads();
  if (t < 64) {
    u64 b[4], s = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) { b[j] = sh.bins[HIST_BINS - 1 - (4 * t + j)]; s += b[j]; }
    const u64 incl = wave_incl_scan_u64(s, t);
    const u64 total = shfl_u64(incl, 63);
    if (top_p > 0.f) {                                   // a token stays iff the mass above it is < top_p * total: integer mass < ceil(.)
      const double cut = ceil((double)top_p * (double)total);
      target = cut >= (double)total ? total : (u64)cut;
      if (target < 1) target = 1;
      if (t == 0) sh.pick_target = target;
    }
    u64 a = incl - s;
    if (a < target && target <= incl) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (target <= a + b[j]) { sh.pick_digit = HIST_BINS - 1 - (4 * t + j); sh.pick_above = a; break; }
        a += b[j];
      }
    }
  }
  __syncthreads();
}

// The key v of the score with  W(keys > v) < target <= W(keys >= v)  among the scores with key >= lo_key, W = the count (top_p == 0) or
// the summed mass (top_p > 0, target = ceil(top_p * total mass)).
__device__ unsigned radix_select(const float* __restrict__ sc, int nv, unsigned lo_key, float mx, u64 target, float top_p, SelShared& sh) {
  const int t = threadIdx.x;
  const bool mass = top_p > 0.f;
  u64 prefix = 0;
  for (int shift = 24; shift >= 0; shift -= 8) {
    for (int i = t; i < HIST_BINS * MASS_COPIES; i += SEL_THREADS) sh.hist[i] = 0;
    __syncthreads();
    unsigned* cnt = reinterpret_cast<unsigned*>(sh.hist);
    for_each_score_vec(sc, t, nv, SEL_THREADS, [&](int, const float* x) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const unsigned key = score_key(x[j]);
        if (key >= lo_key && ((u64)key >> (shift + 8)) == prefix) {
          const unsigned digit = (key >> shift) & 255u;
          if (mass) atomicAdd(&sh.hist[digit * MASS_COPIES + (t & (MASS_COPIES - 1))], score_mass(x[j], mx));
          else atomicAdd(&cnt[digit * COUNT_COPIES + (t & (COUNT_COPIES - 1))], 1u);
        }
      }
    });
    __syncthreads();
    hist_pick(sh, target, shift == 24 ? top_p : 0.f, mass);
    target = sh.pick_target - sh.pick_above;
    prefix = (prefix << 8) | sh.pick_digit;
  }
  return (unsigned)prefix;
}

__global__ __launch_bounds__(SEL_THREADS) void select_token_kernel(const bf16_t* __restrict__ logits, int64_t ld, int cols,
                                                                   uint8_t* __restrict__ seen, float penalty, int do_sample,
                                                                   float temperature, int top_k, float top_p, const float* __restrict__ u,
                                                                   int64_t* __restrict__ token_out, int32_t* __restrict__ kept_out,
                                                                   int mark_chosen, float* __restrict__ scores) {
  __shared__ SelShared sh;
  const int t = threadIdx.x, lane = t & 63, wid = t >> 6, nv = cols >> 3;
  const int64_t row = blockIdx.x;
  const bf16_t* lrow = logits + row * ld;
  float* sc = scores + row * (int64_t)cols;
  uint8_t* srow = seen ? seen + row * (int64_t)cols : nullptr;
  const bool penal = srow && penalty != 1.f;
  const bool seen8 = (reinterpret_cast<uintptr_t>(srow) & 7) == 0;

  // ---- pass A: scores and their arg-max (ties: the lowest id) -------------------------------------------------------------------------
  float best = -INFINITY;
  int best_i = 0x7fffffff;
  for (int v = t; v < nv; v += SEL_THREADS) {
    const u32x4 w = *reinterpret_cast<const u32x4*>(lrow + (int64_t)v * 8);
    u64 sbits = 0;
    if (penal) {
      if (seen8) {
        sbits = *reinterpret_cast<const u64*>(srow + (int64_t)v * 8);
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) sbits |= (u64)srow[(int64_t)v * 8 + j] << (8 * j);
      }
    }
    float x[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float f = (j & 1) ? bf16hi_to_f32(w[j >> 1]) : bf16lo_to_f32(w[j >> 1]);
      if ((sbits >> (8 * j)) & 0xffu) f = f < 0.f ? f * penalty : f / penalty;
      if (do_sample) f = f / temperature;
      if (f == 0.f) f = 0.f;                             // -0 and +0 are one score: one key
      x[j] = f;
      if (f > best) { best = f; best_i = v * 8 + j; }    // ids ascend within a thread: the first maximum stays
    }
    if (do_sample) vita_store_row8(sc + (int64_t)v * 8, x);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float ox = __shfl_xor(best, off, 64);
    const int oi = __shfl_xor(best_i, off, 64);
    if (ox > best || (ox == best && oi < best_i)) { best = ox; best_i = oi; }
  }
  if (lane == 0) { sh.red_x[wid] = best; sh.red_i[wid] = best_i; }
  __syncthreads();                                       // also orders the score stores before the passes that read them
#pragma unroll
  for (int i = 0; i < SEL_WAVES; ++i) {
    const float ox = sh.red_x[i];
    const int oi = sh.red_i[i];
    if (ox > best || (ox == best && oi < best_i)) { best = ox; best_i = oi; }
  }
  if (!do_sample) {
    if (t == 0) {
      token_out[row] = best_i;
      if (kept_out) kept_out[row] = 1;
      if (mark_chosen && srow) srow[best_i] = 1;
    }
    return;
  }

  // ---- the cut: kept = { key >= cut } -----------------------------------------------------------------------------------------------
  unsigned cut = 0;
  if (top_k > 0 && top_k < cols) cut = radix_select(sc, nv, 0u, best, (u64)top_k, 0.f, sh);
  if (top_p > 0.f && top_p < 1.f) cut = radix_select(sc, nv, cut, best, 0, top_p, sh);

  // ---- the draw: the first kept token, in ascending id, whose inclusive mass prefix exceeds u * Z -----------------------------------------
  // wave w owns the ids of vectors [w * seg, (w + 1) * seg): first every wave sums its segment, then the one wave that holds the crossing
  // scans its segment again
  const int seg = (nv + SEL_WAVES - 1) / SEL_WAVES, v0 = wid * seg, v1 = min(nv, v0 + seg);
  u64 msum = 0;
  unsigned cnt = 0;
  for_each_score_vec(sc, v0 + lane, v1, 64, [&](int, const float* x) {
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (score_key(x[j]) >= cut) { msum += score_mass(x[j], best); ++cnt; }
  });
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    msum += ((u64)__shfl_xor((unsigned)(msum >> 32), off, 64) << 32) | __shfl_xor((unsigned)msum, off, 64);
    cnt += __shfl_xor(cnt, off, 64);
  }
  if (lane == 0) { sh.wave_mass[wid] = msum; sh.wave_cnt[wid] = cnt; }
  __syncthreads();
  u64 z = 0;
  unsigned kept = 0;
#pragma unroll
  for (int i = 0; i < SEL_WAVES; ++i) { z += sh.wave_mass[i]; kept += sh.wave_cnt[i]; }
  u64 resid = (u64)((double)u[row] * (double)z);         // prefix > u * Z  <=>  prefix > floor(u * Z): the prefixes are integers
  if (resid >= z) resid = z - 1;                          // z >= 2^40: the arg-max is always kept and has mass 2^40
  int wstar = 0;
  for (; wstar < SEL_WAVES - 1; ++wstar) {
    if (resid < sh.wave_mass[wstar]) break;
    resid -= sh.wave_mass[wstar];
  }
  if (wid != wstar) return;
  u64 running = 0;
  for (int base = v0; base < v1; base += 64) {           // 64 consecutive vectors per step: ids ascend with the lane
    const int v = base + lane;
    u64 m[8], s = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) m[j] = 0;
    if (v < v1) {
      const f32x4 lo = *reinterpret_cast<const f32x4*>(sc + (int64_t)v * 8), hi = *reinterpret_cast<const f32x4*>(sc + (int64_t)v * 8 + 4);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float x = j < 4 ? lo[j & 3] : hi[j & 3];
        if (score_key(x) >= cut) m[j] = score_mass(x, best);
        s += m[j];
      }
    }
    const u64 incl = wave_incl_scan_u64(s, lane);
    const u64 hit = __ballot(running + incl > resid);
    if (hit) {
      if (lane == __ffsll((long long)hit) - 1) {
        u64 a = running + incl - s;
        int tok = v * 8;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          a += m[j];
          if (a > resid) { tok = v * 8 + j; break; }
        }
        token_out[row] = tok;
        if (kept_out) kept_out[row] = (int32_t)kept;
        if (mark_chosen && srow) srow[tok] = 1;
      }
      return;
    }
    running += shfl_u64(incl, 63);
  }
}

__global__ __launch_bounds__(256) void token_seen_mark_kernel(const int64_t* __restrict__ ids, int64_t n, uint8_t* __restrict__ seen,
                                                              int64_t vocab, int32_t* __restrict__ err_flag) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t id = ids[i];
    if (id >= 0 && id < vocab) seen[id] = 1;
    else if (err_flag) atomicExch(err_flag, 1);
  }
}

}  // namespace

extern "C" int vita_token_seen_mark(const int64_t* ids, int64_t n, uint8_t* seen, int64_t vocab, int32_t* err_flag, void* stream) {
  if (!ids || !seen || n < 0 || vocab <= 0) return VITA_ERR_INVALID_ARG;
  if (n == 0) return VITA_OK;
  const int64_t blocks = (n + 255) / 256;
  hipLaunchKernelGGL(token_seen_mark_kernel, dim3((unsigned)(blocks > 1024 ? 1024 : blocks)), dim3(256), 0, (hipStream_t)stream, ids, n,
                     seen, vocab, err_flag);
  return vita_check_launch();
}

extern "C" int64_t vita_select_token_workspace_bytes(int64_t rows, int64_t cols) {
  return rows > 0 && cols > 0 ? rows * cols * (int64_t)sizeof(float) : 0;    // the fp32 scores of every row
}

extern "C" int vita_select_token(const void* logits, int64_t ld, int64_t rows, int64_t cols, uint8_t* seen, float repetition_penalty,
                                 int do_sample, float temperature, int top_k, float top_p, const float* u, int64_t* token_out,
                                 int32_t* kept_out, int mark_chosen, void* workspace, int64_t workspace_bytes, void* stream) {
  if (!logits || !token_out || !workspace || rows < 0 || cols <= 0 || ld < cols) return VITA_ERR_INVALID_ARG;
  if (!(repetition_penalty > 0.f) || !isfinite(repetition_penalty)) return VITA_ERR_INVALID_ARG;
  if (do_sample && (!u || !(temperature > 0.f) || !isfinite(temperature))) return VITA_ERR_INVALID_ARG;
  if (!isfinite(top_p)) return VITA_ERR_INVALID_ARG;
  if (workspace_bytes < vita_select_token_workspace_bytes(rows, cols)) return VITA_ERR_INVALID_ARG;
  if ((cols & 7) || (ld & 7) || cols > SEL_MAX_COLS || rows > 0x7fffffffll) return VITA_ERR_UNSUPPORTED;
  if ((reinterpret_cast<uintptr_t>(logits) & 15) || (reinterpret_cast<uintptr_t>(workspace) & 15)) return VITA_ERR_UNSUPPORTED;
  if (rows == 0) return VITA_OK;
  hipLaunchKernelGGL(select_token_kernel, dim3((unsigned)rows), dim3(SEL_THREADS), 0, (hipStream_t)stream, (const bf16_t*)logits, ld,
                     (int)cols, seen, repetition_penalty, do_sample ? 1 : 0, temperature, top_k, top_p, u, token_out, kept_out,
                     mark_chosen, (float*)workspace);
  return vita_check_launch();
}
