// Beam-search candidates (M/inference/text_generation/generation.py:283-471; the scoring of :356-376 and beam_candidates :454-471
// without sampling): of all rows x cols continuations of the live beams, the n_out best by
//   score = log_softmax(logit / temperature)[col] + beam_scores[row],
// sorted by descending score, equal scores by ascending flat index row * cols + col.  The reference sorts the whole [rows * vocab]
// array on the device and reads 2 * beam_size entries back one .item() at a time; here two small launches leave the 2 * beam_size
// (index, score) pairs for ONE copy to the host.
//
// Inside a row the score is a monotone function of the logit, so the row's best n_out are its n_out largest logits:
//   beam_cand_block_kernel : grid (blocks, rows).  A workgroup owns a contiguous range of one row: max and sum of exp of the range
//                            (fp32 on the bf16 logits), and its n_out largest logits, lowest column first among equals — found by
//                            n_out passes over the range (L2-resident), each taking the best entry strictly behind the last one.
//   beam_cand_final_kernel : one workgroup.  Folds the ranges' statistics into each row's max and log-sum, scores the
//                            rows x blocks x n_out survivors and takes the n_out best of them the same way.
#include "vita_common.h"

#include <math.h>

namespace {

constexpr int kCandMaxOut = 16;
constexpr int kCandMaxRows = 16;
constexpr int kCandMaxBlocks = 64;
constexpr int kCandMinChunk = 2048;
constexpr int64_t kCandMaxCols = int64_t(1) << 23;

inline int cand_blocks(int64_t cols) {
  const int64_t n = (cols + kCandMinChunk - 1) / kCandMinChunk;
  return (int)(n < 1 ? 1 : (n > kCandMaxBlocks ? kCandMaxBlocks : n));
}

// total order of the candidates: higher value first, equal values by lower index
__device__ __forceinline__ bool cand_before(float va, long long ia, float vb, long long ib) {
  return va > vb || (va == vb && ia < ib);
}

// the first (value, index) of the workgroup in that order; every thread gets it.  red_v / red_i: 4 entries of LDS each.
__device__ __forceinline__ void block_first(float& v, long long& i, float* red_v, long long* red_i) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float ov = __shfl_xor(v, off, 64);
    const long long oi = __shfl_xor(i, off, 64);
    if (cand_before(ov, oi, v, i)) { v = ov; i = oi; }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();                                       // protect red_* from the previous use
  if (lane == 0) { red_v[wave] = v; red_i[wave] = i; }
  __syncthreads();
  v = red_v[0]; i = red_i[0];
#pragma unroll
  for (int w = 1; w < 4; ++w)
    if (cand_before(red_v[w], red_i[w], v, i)) { v = red_v[w]; i = red_i[w]; }
}

__device__ __forceinline__ float load_logit(const bf16_t* row, int c) {
  const float v = bf16_to_f32(row[c]);
  return v != v ? -INFINITY : v;                          // a NaN logit ranks last
}

constexpr long long kNoIndex = 0x7fffffffffffffffLL;

__global__ __launch_bounds__(256) void beam_cand_block_kernel(const bf16_t* __restrict__ logits, int64_t ld, int cols, int chunk,
                                                              int n_out, float temperature, float* __restrict__ stat_m,
                                                              float* __restrict__ stat_s, float* __restrict__ cand_v,
                                                              int* __restrict__ cand_c) {
  __shared__ float red_v[4];
  __shared__ long long red_i[4];
  __shared__ float red_f[16];
  const int blk = blockIdx.x, r = blockIdx.y, nblk = gridDim.x, t = threadIdx.x;
  const bf16_t* row = logits + (int64_t)r * ld;
  const int c0 = blk * chunk, c1 = min(cols, c0 + chunk);
  // statistics of the range: max of x = logit / temperature, sum of exp(x - max)
  float vmax = -INFINITY;
  for (int c = c0 + t; c < c1; c += 256) vmax = fmaxf(vmax, load_logit(row, c));
  {
    long long dummy = 0;
    float v = vmax;
    // reuse the ordered reduction for the max (the index plays no part)
    block_first(v, dummy, red_v, red_i);
    vmax = v;
  }
  const float xmax = vmax / temperature;
  float s = 0.f;
  if (vmax > -INFINITY)
    for (int c = c0 + t; c < c1; c += 256) s += expf(load_logit(row, c) / temperature - xmax);
  s = block_reduce_sum(s, red_f);
  if (t == 0) { stat_m[r * nblk + blk] = xmax; stat_s[r * nblk + blk] = s; }
  // the n_out largest logits of the range, lowest column first among equals
  float pv = INFINITY;
  long long pi = -1;
  for (int k = 0; k < n_out; ++k) {
    float bv = -INFINITY;
    long long bi = kNoIndex;
    for (int c = c0 + t; c < c1; c += 256) {
      const float v = load_logit(row, c);
      if (cand_before(pv, pi, v, c) && cand_before(v, c, bv, bi)) { bv = v; bi = c; }
    }
    block_first(bv, bi, red_v, red_i);
    if (t == 0) {
      const int64_t e = ((int64_t)r * nblk + blk) * n_out + k;
      cand_v[e] = bv;
      cand_c[e] = bi == kNoIndex ? -1 : (int)bi;
    }
    pv = bv; pi = bi;                                     // exhausted range: (-inf, no index) — nothing lies behind it
  }
}

__global__ __launch_bounds__(256) void beam_cand_final_kernel(const float* __restrict__ stat_m, const float* __restrict__ stat_s,
                                                              const float* __restrict__ cand_v, const int* __restrict__ cand_c,
                                                              const float* __restrict__ beam_scores, int rows, int cols, int nblk,
                                                              int n_out, float temperature, long long* __restrict__ idx_out,
                                                              float* __restrict__ score_out) {
  __shared__ float red_v[4];
  __shared__ long long red_i[4];
  __shared__ float row_m[kCandMaxRows], row_logs[kCandMaxRows], row_bs[kCandMaxRows];
  const int t = threadIdx.x;
  if (t < rows) {                                         // fold the ranges' (max, sum) of row t: at most 64 of them
    float M = -INFINITY;
    for (int b = 0; b < nblk; ++b) M = fmaxf(M, stat_m[t * nblk + b]);
    float S = 0.f;
    for (int b = 0; b < nblk; ++b) {
      const float m = stat_m[t * nblk + b];
      if (m > -INFINITY) S += stat_s[t * nblk + b] * expf(m - M);
    }
    row_m[t] = M;
    row_logs[t] = logf(S);
    row_bs[t] = beam_scores[t];
  }
  __syncthreads();
  const int per_row = nblk * n_out, total = rows * per_row;
  float pv = INFINITY;
  long long pi = -1;
  for (int k = 0; k < n_out; ++k) {
    float bv = -INFINITY;
    long long bi = kNoIndex;
    for (int e = t; e < total; e += 256) {
      const int c = cand_c[e];
      if (c < 0) continue;
      const int r = e / per_row;
      float sc = (cand_v[e] / temperature - row_m[r]) - row_logs[r] + row_bs[r];
      if (sc != sc) sc = -INFINITY;
      const long long flat = (long long)r * cols + c;
      if (cand_before(pv, pi, sc, flat) && cand_before(sc, flat, bv, bi)) { bv = sc; bi = flat; }
    }
    block_first(bv, bi, red_v, red_i);
    if (t == 0) { idx_out[k] = bi == kNoIndex ? -1 : bi; score_out[k] = bv; }
    pv = bv; pi = bi;
  }
}

bool cand_shape_ok(int64_t rows, int64_t cols) { return rows >= 1 && rows <= kCandMaxRows && cols >= 1 && cols <= kCandMaxCols; }

}  // namespace

extern "C" int64_t vita_beam_candidates_workspace_bytes(int64_t rows, int64_t cols) {
  if (!cand_shape_ok(rows, cols)) return 0;
  return rows * cand_blocks(cols) * (int64_t)(2 + 2 * kCandMaxOut) * (int64_t)sizeof(float);
}

extern "C" int vita_beam_candidates(const void* logits, int64_t ld, int64_t rows, int64_t cols, const float* beam_scores,
                                    float temperature, int n_out, int64_t* idx_out, float* score_out, void* workspace,
                                    int64_t workspace_bytes, void* stream) {
  if (!logits || !beam_scores || !idx_out || !score_out || !workspace || rows < 1 || cols < 1 || n_out < 1) return VITA_ERR_INVALID_ARG;
  if (!(temperature > 0.f) || !(temperature < INFINITY)) return VITA_ERR_INVALID_ARG;
  if (cols > kCandMaxCols || rows > kCandMaxRows || n_out > kCandMaxOut) return VITA_ERR_UNSUPPORTED;
  if ((int64_t)n_out > rows * cols || ld < cols) return VITA_ERR_INVALID_ARG;
  if (workspace_bytes < vita_beam_candidates_workspace_bytes(rows, cols) || ((uintptr_t)workspace & 15)) return VITA_ERR_INVALID_ARG;
  const int nblk = cand_blocks(cols);
  const int chunk = (int)((cols + nblk - 1) / nblk);
  float* stat_m = (float*)workspace;
  float* stat_s = stat_m + rows * nblk;
  float* cand_v = stat_s + rows * nblk;
  int* cand_c = (int*)(cand_v + rows * nblk * kCandMaxOut);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(beam_cand_block_kernel, dim3((unsigned)nblk, (unsigned)rows), dim3(256), 0, st, (const bf16_t*)logits, ld, (int)cols,
                     chunk, n_out, temperature, stat_m, stat_s, cand_v, cand_c);
  int rc = vita_check_launch();
  if (rc != VITA_OK) return rc;
  hipLaunchKernelGGL(beam_cand_final_kernel, dim3(1), dim3(256), 0, st, (const float*)stat_m, (const float*)stat_s, (const float*)cand_v,
                     (const int*)cand_c, beam_scores, (int)rows, (int)cols, nblk, n_out, temperature, (long long*)idx_out, score_out);
  return vita_check_launch();
}
