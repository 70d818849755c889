// Prompt-lookup speculative decoding on the device (tools/inference_long_vita.py:820-826,868: greedy, repetition_penalty 1.05, up to 1024
// new tokens behind a long prompt): the draft rule of transformers' PromptLookupCandidateGenerator.get_candidates on the device history,
// and the greedy acceptance of one verify pass.  Nothing here synchronises with the host.
//
// vita_ngram_draft.  A window hist[i : i + g] that equals the suffix hist[n - g : n] ENDS at e = i + g.  For every end e the thread
// counts m(e), the tokens in front of e that agree with the tokens in front of n (at most G' = min(G, n - 1)); e then is a match for
// every g <= m(e).  Larger g beats smaller g and, at one g, the leftmost i wins, so the answer is the minimum of the 64-bit key
// (G - m(e)) << 40 | (e - m(e)) over the ends 1 <= e < min(n, max_total) with m(e) >= 1: an order-independent minimum.  Stage one:
// up to 256 workgroups walk the ends once (one coalesced pass over the history for all g) and each stores its minimum with a plain
// store; stage two: one workgroup reduces those, cuts the continuation and writes it.  No atomics, no initialised workspace.
// An entry of hist is only ever compared or copied: it never forms an address.
//
// vita_draft_verify.  One workgroup of 1024 threads per row takes the arg-max of the row's penalised fp32 scores exactly as
// select_token_kernel's greedy pass does (select.hip), the penalised ids being seen U {draft[0 .. row - 1]}, and parks it in
// record[2 + row]; one wave then scans the rows: accepted prefix, eos cut, history, byte map, record.
#include "vita_common.h"
#include <math.h>

namespace {

typedef unsigned long long u64;
constexpr int NG_THREADS = 256, NG_MAX_BLOCKS = 256, NG_MAX_DRAFT = 7, NG_MAX_EOS = 8;
constexpr u64 NG_NONE = ~0ull;
constexpr int DV_THREADS = 1024, DV_WAVES = DV_THREADS / 64, DV_MIN_ROWS = 2, DV_MAX_ROWS = 8;
constexpr int64_t DV_MAX_COLS = 1 << 23;                   // vita_select_token's limit

__device__ __forceinline__ int64_t clamp_len(const int32_t* n_hist, int64_t hist_cap) {
  const int64_t n = *n_hist;
  return n < 0 ? 0 : (n > hist_cap ? hist_cap : n);
}

__device__ __forceinline__ u64 wave_min_u64(u64 v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const u64 o = ((u64)__shfl_xor((unsigned)(v >> 32), off, 64) << 32) | __shfl_xor((unsigned)v, off, 64);
    if (o < v) v = o;
  }
  return v;
}

__device__ __forceinline__ u64 block_min_u64(u64 v, u64* red) {   // NG_THREADS threads; every thread gets the minimum
  v = wave_min_u64(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  u64 r = red[0];
#pragma unroll
  for (int i = 1; i < NG_THREADS / 64; ++i) r = red[i] < r ? red[i] : r;
  return r;
}

__global__ __launch_bounds__(NG_THREADS) void ngram_scan_kernel(const int64_t* __restrict__ hist, int64_t hist_cap,
                                                                const int32_t* __restrict__ n_hist, int max_ngram, int64_t max_total,
                                                                u64* __restrict__ part) {
  __shared__ u64 red[NG_THREADS / 64];
  const int64_t n = clamp_len(n_hist, hist_cap);
  const int64_t geff = n - 1 < (int64_t)max_ngram ? n - 1 : (int64_t)max_ngram;     // min(G, n - 1)
  const int64_t e_end = n < max_total ? n : max_total;                               // ends e < min(n, max_total)
  u64 best = NG_NONE;
  if (geff >= 1) {
    const int64_t last = hist[n - 1];
    for (int64_t e = 1 + (int64_t)blockIdx.x * NG_THREADS + threadIdx.x; e < e_end; e += (int64_t)gridDim.x * NG_THREADS) {
      if (hist[e - 1] != last) continue;
      int64_t m = 1;
      const int64_t lim = e < geff ? e : geff;
      while (m < lim && hist[e - 1 - m] == hist[n - 1 - m]) ++m;
      const u64 key = ((u64)(max_ngram - m) << 40) | (u64)(e - m);
      if (key < best) best = key;
    }
  }
  best = block_min_u64(best, red);
  if (threadIdx.x == 0) part[blockIdx.x] = best;
}

__global__ __launch_bounds__(NG_THREADS) void ngram_finish_kernel(const int64_t* __restrict__ hist, int64_t hist_cap,
                                                                  const int32_t* __restrict__ n_hist, int max_ngram, int num_draft,
                                                                  int64_t max_total, const int64_t* __restrict__ eos, int n_eos,
                                                                  const u64* __restrict__ part, int n_part,
                                                                  int64_t* __restrict__ draft_out, int32_t* __restrict__ n_draft_out) {
  __shared__ u64 red[NG_THREADS / 64];
  const u64 key = block_min_u64((int)threadIdx.x < n_part ? part[threadIdx.x] : NG_NONE, red);
  if (threadIdx.x != 0) return;
  const int64_t n = clamp_len(n_hist, hist_cap);
  int n_out = 0;
  if (key != NG_NONE && max_total != n + 1) {
    const int64_t g = (int64_t)max_ngram - (int64_t)(key >> 40), i = (int64_t)(key & ((1ull << 40) - 1));
    const int64_t start = i + g;
    int64_t end = start + num_draft;
    if (end > n) end = n;
    if (end > max_total) end = max_total;
    for (int64_t j = start; j < end; ++j) {
      const int64_t id = hist[j];
      bool stop = false;
      for (int q = 0; q < n_eos; ++q) stop |= eos[q] == id;
      if (stop) break;                                     // cut in front of the first eos id; the search does not go on
      draft_out[n_out++] = id;
    }
  }
  for (int j = n_out; j < num_draft; ++j) draft_out[j] = -1;
  *n_draft_out = n_out;
}

__global__ __launch_bounds__(DV_THREADS) void draft_rows_kernel(const bf16_t* __restrict__ logits, int64_t ld, int cols,
                                                                const uint8_t* __restrict__ seen, float penalty,
                                                                const int64_t* __restrict__ draft, int64_t* __restrict__ record) {
  __shared__ float red_x[DV_WAVES];
  __shared__ int red_i[DV_WAVES];
  const int t = threadIdx.x, lane = t & 63, wid = t >> 6, nv = cols >> 3, row = blockIdx.x;
  const bf16_t* lrow = logits + (int64_t)row * ld;
  const bool penal = penalty != 1.f;
  const bool seen8 = (reinterpret_cast<uintptr_t>(seen) & 7) == 0;
  // the drafts in front of this row, as ids of this row's columns; one outside [0, cols) penalises nothing
  int did[NG_MAX_DRAFT];
#pragma unroll
  for (int j = 0; j < NG_MAX_DRAFT; ++j) {
    did[j] = -1;
    if (j < row) {
      const int64_t d = draft[j];
      if (d >= 0 && d < cols) did[j] = (int)d;
    }
  }
  float best = -INFINITY;
  int best_i = 0x7fffffff;
  for (int v = t; v < nv; v += DV_THREADS) {
    const u32x4 w = *reinterpret_cast<const u32x4*>(lrow + (int64_t)v * 8);
    u64 sbits = 0;
    if (penal) {
      if (seen) {
        if (seen8) {
          sbits = *reinterpret_cast<const u64*>(seen + (int64_t)v * 8);
        } else {
#pragma unroll
          for (int j = 0; j < 8; ++j) sbits |= (u64)seen[(int64_t)v * 8 + j] << (8 * j);
        }
      }
#pragma unroll
      for (int j = 0; j < NG_MAX_DRAFT; ++j)
        if ((did[j] >> 3) == v) sbits |= 0xffull << (8 * (did[j] & 7));             // did = -1: -1 >> 3 = -1, never a vector
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float f = (j & 1) ? bf16hi_to_f32(w[j >> 1]) : bf16lo_to_f32(w[j >> 1]);
      if ((sbits >> (8 * j)) & 0xffu) f = f < 0.f ? f * penalty : f / penalty;
      if (f == 0.f) f = 0.f;                               // -0 and +0 are one score
      if (f > best) { best = f; best_i = v * 8 + j; }      // ids ascend within a thread: the first maximum stays
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float ox = __shfl_xor(best, off, 64);
    const int oi = __shfl_xor(best_i, off, 64);
    if (ox > best || (ox == best && oi < best_i)) { best = ox; best_i = oi; }
  }
  if (lane == 0) { red_x[wid] = best; red_i[wid] = best_i; }
  __syncthreads();
  if (t == 0) {
#pragma unroll
    for (int i = 0; i < DV_WAVES; ++i) {
      const float ox = red_x[i];
      const int oi = red_i[i];
      if (ox > best || (ox == best && oi < best_i)) { best = ox; best_i = oi; }
    }
    if (best_i >= cols) best_i = 0;                        // no score above -inf (all -inf or NaN): id 0, an id that may index hist / seen
    record[2 + row] = best_i;
  }
}

__global__ __launch_bounds__(64) void draft_scan_kernel(int t, int cols, uint8_t* __restrict__ seen, const int64_t* __restrict__ draft,
                                                        const int64_t* __restrict__ eos, int n_eos, int64_t* __restrict__ hist,
                                                        int64_t hist_cap, int32_t* __restrict__ n_hist, int64_t* __restrict__ record) {
  if (threadIdx.x != 0) return;
  int64_t a[DV_MAX_ROWS];
  for (int i = 0; i < t; ++i) a[i] = record[2 + i];
  int n_acc = 0;
  while (n_acc < t - 1 && draft[n_acc] == a[n_acc]) ++n_acc;
  int n_emit = n_acc + 1, stop = 0;
  for (int i = 0; i <= n_acc && !stop; ++i)
    for (int q = 0; q < n_eos; ++q)
      if (eos[q] == a[i]) { n_emit = i + 1; stop = 1; break; }   // cut BEHIND the first eos among the emitted tokens
  const int64_t n = clamp_len(n_hist, hist_cap);
  for (int i = 0; i < n_emit; ++i) {
    if (n + i < hist_cap) hist[n + i] = a[i];
    if (seen && a[i] >= 0 && a[i] < cols) seen[a[i]] = 1;
  }
  *n_hist = (int32_t)(n + n_emit < hist_cap ? n + n_emit : hist_cap);
  record[0] = n_emit;
  record[1] = stop;
  for (int i = 0; i < t; ++i) record[2 + i] = i < n_emit ? a[i] : -1;
}

}  // namespace

extern "C" int64_t vita_ngram_draft_workspace_bytes(int64_t hist_cap) {
  (void)hist_cap;
  return NG_MAX_BLOCKS * (int64_t)sizeof(u64);             // one partial minimum per workgroup of stage one
}

extern "C" int vita_ngram_draft(const int64_t* hist, int64_t hist_cap, const int32_t* n_hist, int max_ngram, int num_draft,
                                int64_t max_total, const int64_t* eos, int n_eos, int64_t* draft_out, int32_t* n_draft_out,
                                void* workspace, int64_t workspace_bytes, void* stream) {
  if (!hist || !n_hist || !draft_out || !n_draft_out || !workspace || (!eos && n_eos > 0)) return VITA_ERR_INVALID_ARG;
  if (num_draft < 1 || max_ngram < 1 || n_eos < 0 || hist_cap < 0) return VITA_ERR_INVALID_ARG;
  if (workspace_bytes < vita_ngram_draft_workspace_bytes(hist_cap)) return VITA_ERR_INVALID_ARG;
  if (num_draft > NG_MAX_DRAFT || n_eos > NG_MAX_EOS) return VITA_ERR_UNSUPPORTED;
  if (max_ngram > (1 << 20)) return VITA_ERR_UNSUPPORTED;                           // G - g sits above bit 40 of the key
  if (hist_cap >= (int64_t(1) << 31) || (reinterpret_cast<uintptr_t>(workspace) & 7)) return VITA_ERR_UNSUPPORTED;   // *n_hist is int32
  int64_t blocks = (hist_cap + NG_THREADS - 1) / NG_THREADS;
  blocks = blocks < 1 ? 1 : (blocks > NG_MAX_BLOCKS ? NG_MAX_BLOCKS : blocks);
  u64* part = (u64*)workspace;
  hipLaunchKernelGGL(ngram_scan_kernel, dim3((unsigned)blocks), dim3(NG_THREADS), 0, (hipStream_t)stream, hist, hist_cap, n_hist,
                     max_ngram, max_total, part);
  hipLaunchKernelGGL(ngram_finish_kernel, dim3(1), dim3(NG_THREADS), 0, (hipStream_t)stream, hist, hist_cap, n_hist, max_ngram, num_draft,
                     max_total, eos, n_eos, part, (int)blocks, draft_out, n_draft_out);
  return vita_check_launch();
}

extern "C" int vita_draft_verify(const void* logits, int64_t ld, int t, int64_t cols, uint8_t* seen, float repetition_penalty,
                                 const int64_t* draft, const int64_t* eos, int n_eos, int64_t* hist, int64_t hist_cap, int32_t* n_hist,
                                 int64_t* record, void* stream) {
  if (!logits || !draft || !hist || !n_hist || !record || (!eos && n_eos > 0)) return VITA_ERR_INVALID_ARG;
  if (cols <= 0 || ld < cols || n_eos < 0 || hist_cap < 0) return VITA_ERR_INVALID_ARG;
  if (!(repetition_penalty > 0.f) || !isfinite(repetition_penalty)) return VITA_ERR_INVALID_ARG;
  if (t < DV_MIN_ROWS || t > DV_MAX_ROWS || n_eos > NG_MAX_EOS) return VITA_ERR_UNSUPPORTED;
  if ((cols & 7) || (ld & 7) || cols > DV_MAX_COLS || (reinterpret_cast<uintptr_t>(logits) & 15)) return VITA_ERR_UNSUPPORTED;
  if (hist_cap >= (int64_t(1) << 31)) return VITA_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(draft_rows_kernel, dim3((unsigned)t), dim3(DV_THREADS), 0, (hipStream_t)stream, (const bf16_t*)logits, ld, (int)cols,
                     (const uint8_t*)seen, repetition_penalty, draft, record);
  hipLaunchKernelGGL(draft_scan_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, t, (int)cols, seen, draft, eos, n_eos, hist, hist_cap,
                     n_hist, record);
  return vita_check_launch();
}
