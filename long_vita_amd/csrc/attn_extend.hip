// Flash attention of t NEW query rows against a KV cache that already holds their keys ("extend": a follow-up turn or a prefill
// chunk behind a cached context).  gfx950, head_dim 128, bf16 I/O, fp32 statistics, GQA.
//
// Geometry: query row i sits at position q_pos0 + i.  Cache rows [0, n_full) are visible to every row; row k >= n_full sits at
// position key_pos0 + (k - n_full) * key_pos_step and is visible iff that position <= the row's.  Positions of the appended rows
// ascend, so a row sees exactly the keys [0, lim] with lim = n_full + floor((pos - key_pos0) / step) (n_full - 1 when pos < key_pos0,
// never beyond n_keys - 1): ONE integer per lane decides every mask, and only tiles that reach beyond the smallest lim of a wave
// evaluate it.
//
// Shares attn_fwd8.h's tile body with flash_fwd_kernel (attn.hip): 8 waves x 32 rows, 64-key K/V tiles staged by LDS-DMA with the bank
// swizzle on the source address, S^T = K Q^T / O^T = V^T P^T on v_mfma_f32_32x32x16_bf16, the online-softmax step, the bf16 / lse
// epilogue.  What is this kernel's own:
//   * the 256 rows of a workgroup are STACKED (row, query head of the kv group) pairs, row-major: stacked index s = row * G + head.
//     One K/V tile read serves all G heads of the group, and a 16-row follow-up fills 80 of 256 MFMA rows instead of 16;
//   * the keys are cut into n_splits ranges of whole tiles (blocks = kv head x query tile x split) so that a short follow-up behind
//     a long context still fills the chip; every split writes un-normalised fp32 partials (m, l in the log2 domain, o) and
//     extend_merge_kernel forms the bf16 context and the natural-log lse.  One split writes the result directly;
//   * the mask by one limit per lane, the tile maximum rounded up to an integer under quant_m, and two bf16 terms of P when all
//     stacked rows fit one query tile.
// decode_attn_merge_kernel (decode.hip) is not reused: it writes a dense [heads][128] context and no lse; this merge writes through
// row / head strides and one workgroup handles four (row, head) pairs.
//
// Reference behaviour restated: H/models/long_vita_qwen2_intern/modeling_long_vita.py:150-202 (q_len > 1 behind a DynamicCache:
// cache_position = arange(past_seen, past_seen + s), causal mask over past + new keys) and the cached decode loop
// M/inference/text_generation/generation.py:127-131 fed more than one token.
#include "attn_fwd8.h"

namespace {

using fwd8::KVT;             // keys per tile
using fwd8::QTILE;           // stacked query rows per workgroup (8 waves x 32)
constexpr int D = 128;
constexpr int kMaxSplits = 64;
constexpr int kTargetBlocks = 512;      // two rounds of one workgroup per CU (256 CUs)
constexpr int kMinTilesPerSplit = 4;

struct ExtArgs {
  const bf16_t* q; int64_t q_rs, q_gs, q_hs;
  const bf16_t* k; const bf16_t* v; int64_t kv_rs, kv_gs;
  bf16_t* o; int64_t o_rs, o_hs;
  float* lse;                    // [heads][t] or null
  float* pm; float* pl; float* po;   // partials [n_splits][heads][t] (x 128 for po); unused with one split
  int t, G, n_kv_heads, n_q_tiles;
  int n_keys, n_full;
  int64_t q_pos0, key_pos0, key_pos_step;
  int n_splits, tiles_per_split;
  int quant_m;                   // running max kept on integers (log2 domain): see the kernel's main loop
  int partial_out;               // write the fp32 partials even with one split (the beam step merges them with its tail partial)
  float scale_log2e;
  // the segment launch alone (flash_extend_kernel<., true>, vita_prefix_extend_attn_fwd): see segment_args
  const bf16_t* const* tail_ptrs; const int* seg;
  int n_seg, seg_max_count, tail_cap;
};

// ---- the segment launch: up to 8 continuation rows b, each with count_b NEW tokens behind tail0_b rows of its own tail ---------------
// seg [n_seg][3] (int32, device) = (first query row, count, tail0).  Every triple is clamped before it forms an address: first into
// [0, t], tail0 into [0, tail_cap], count into [0, min(seg_max_count, t - first, tail_cap - tail0)].
struct Segment { int first, count, tail0; };
__device__ __forceinline__ Segment clamped_segment(const ExtArgs& p, int b) {
  Segment s = {p.seg[3 * b], p.seg[3 * b + 1], p.seg[3 * b + 2]};
  s.first = min(max(s.first, 0), p.t);
  s.tail0 = min(max(s.tail0, 0), p.tail_cap);
  s.count = min(min(max(s.count, 0), p.seg_max_count), min(p.t - s.first, p.tail_cap - s.tail0));
  return s;
}
// The launch's arguments (t = all query rows, n_splits = the part the launch writes, kv strides = the tails') as those of segment sg
// alone: its queries against its tail, rows [0, tail0) visible to all of them and the diagonal behind.  A segment with count > 0 reads
// its entry of tail_ptrs; nothing else does.
__device__ __forceinline__ ExtArgs segment_args(const ExtArgs& p, int b, const Segment& sg) {
  ExtArgs s = p;
  s.q = p.q + (int64_t)sg.first * p.q_rs;
  s.k = p.tail_ptrs[2 * b]; s.v = p.tail_ptrs[2 * b + 1];
  s.t = sg.count;
  s.n_full = sg.tail0; s.n_keys = sg.tail0 + sg.count;
  s.q_pos0 = 0; s.key_pos0 = 0; s.key_pos_step = 1;
  return s;
}
// Query rows no segment names get the merge's neutral element in the launch's part (the blocks behind the last segment)
__device__ __forceinline__ void fill_unnamed_rows(const ExtArgs& p, int block, int n_blocks) {
  const int64_t heads = (int64_t)p.n_kv_heads * p.G, n_rec = heads * p.t;
  for (int64_t i = (int64_t)block * 512 + threadIdx.x; i < n_rec; i += (int64_t)n_blocks * 512) {
    const int row = (int)(i % p.t);
    bool named = false;
    for (int b = 0; b < p.n_seg; ++b) {
      const Segment sg = clamped_segment(p, b);
      named = named || (row >= sg.first && row < sg.first + sg.count);
    }
    if (named) continue;
    const int64_t rec = (int64_t)p.n_splits * n_rec + i;
    p.pm[rec] = -1.0e30f; p.pl[rec] = 0.f;
    for (int d = 0; d < 128; d += 4) *reinterpret_cast<f32x4*>(p.po + rec * 128 + d) = f32x4{0.f, 0.f, 0.f, 0.f};
  }
}

// last visible key of query row i (-1: none)
__device__ __forceinline__ int last_visible_key(const ExtArgs& p, int i) {
  const int64_t pos = p.q_pos0 + i;
  int64_t lim = (int64_t)p.n_full - 1;
  if (pos >= p.key_pos0) lim = (int64_t)p.n_full + (pos - p.key_pos0) / p.key_pos_step;
  if (lim > (int64_t)p.n_keys - 1) lim = (int64_t)p.n_keys - 1;
  return (int)lim;
}

// SPLIT_P: two bf16 terms of P (attn_fwd8.h's pv_phase) — the precision of the decode kernels' fp32 p.  With random V the 2^-9 rounding
// of a single bf16 p is the largest error of the whole kernel (it does not average out: the error sum has the size of the output sum).
// Used when all stacked rows fit ONE query tile (t * G <= 256: a launch that streams K/V once, the decode kernels' regime); it costs
// 16 more MFMAs per tile (48 instead of 32).  Longer launches keep the prefill kernels' single bf16 term.
// SEG: the segment launch, grid (kv head, query tile of the longest segment, segment b — and one more index for fill_unnamed_rows).  A
// workgroup runs this same body on segment_args; its partial goes to part n_splits of the LAUNCH's records, at row first_b + i.
template <bool SPLIT_P, bool SEG = false>
__global__ __launch_bounds__(512, 2) void flash_extend_kernel(ExtArgs launch) {
  ExtArgs seg_args;
  int seg_first = 0;
  if constexpr (SEG) {
    const int b = blockIdx.z;
    if (b == launch.n_seg) { fill_unnamed_rows(launch, blockIdx.y * gridDim.x + blockIdx.x, gridDim.x * gridDim.y); return; }
    const Segment sg = clamped_segment(launch, b);
    if ((int)blockIdx.y * QTILE >= sg.count * launch.G) return;          // an idle row (count 0) among them
    seg_args = segment_args(launch, b, sg);
    seg_first = sg.first;
  }
  const ExtArgs& p = SEG ? seg_args : launch;
  using T = fwd8::Tile<D>;
  constexpr int DS = T::DS, DB = T::DB, SLOTB = T::SLOTB;

  extern __shared__ __attribute__((aligned(16))) char smem[];  // [2][K tile | V tile]
  const unsigned lds0 = (unsigned)(uintptr_t)(lds_char*)smem;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int hi = lane >> 5, l31 = lane & 31;

  // ---- work decomposition: block = (kv head, key split, query tile), late (long) query tiles first -----------------------------
  int bid = blockIdx.x;
  const int kvh = bid % p.n_kv_heads; bid /= p.n_kv_heads;
  const int split = SEG ? 0 : bid % p.n_splits;
  const int qt = SEG ? (int)blockIdx.y : p.n_q_tiles - 1 - bid / p.n_splits;
  const int G = p.G;
  const int n_stack = p.t * G;                                  // stacked rows of this kv group
  const int s_wg = qt * QTILE, s_wave = s_wg + wave * 32;
  const int s_mine = s_wave + l31;
  const bool live = s_mine < n_stack;
  const int s_c = live ? s_mine : n_stack - 1;
  const int my_row = s_c / G, my_hq = s_c - my_row * G;
  const int my_lim = last_visible_key(p, my_row);
  // wave- and workgroup-uniform limits (the limit ascends with the stacked index)
  const int wg_lim = last_visible_key(p, (min(s_wg + QTILE, n_stack) - 1) / G);
  const bool wave_live = s_wave < n_stack;
  const int wave_lim = wave_live ? last_visible_key(p, (min(s_wave + 32, n_stack) - 1) / G) : -1;
  const int wave_min_lim = wave_live ? last_visible_key(p, s_wave / G) : -1;
  const float scale_log2e = p.scale_log2e;

  const int j_begin = split * p.tiles_per_split;
  const int j_end = min(j_begin + p.tiles_per_split, wg_lim >= 0 ? wg_lim / KVT + 1 : 0);

  // ---- Q fragments (B operand of S^T = K Q^T): lane = (stacked row l31, k-slot half hi) -----------------------------------------
  bf16x8 qf[DS];
  {
    const bf16_t* qp = p.q + (int64_t)my_row * p.q_rs + (int64_t)kvh * p.q_gs + (int64_t)my_hq * p.q_hs + hi * 8;
#pragma unroll
    for (int ds = 0; ds < DS; ++ds) qf[ds] = *reinterpret_cast<const bf16x8*>(qp + ds * 16);
  }

  unsigned koff[DS], voff[DB];                      // per-lane LDS read offsets of the K and V^T fragments
  fwd8::frag_offsets<D>(lane, koff, voff);

  f32x16 o_acc[DB];
#pragma unroll
  for (int i = 0; i < DB; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) o_acc[i][r] = 0.f;
  float m_run = -1.0e30f, l_run = 0.f;

  const bf16_t* kbase = p.k + (int64_t)kvh * p.kv_gs;
  const bf16_t* vbase = p.v + (int64_t)kvh * p.kv_gs;

  fwd8::DmaLane<D> dma;
  fwd8::dma_lane_init<D>(dma, wave, lane, p.kv_rs, p.kv_rs);
  auto dma_tile = [&](int j, unsigned sl) __attribute__((always_inline)) {
    const int64_t row0 = (int64_t)j * KVT;
    // rows of the cache behind row0 (>= 1, an int: n_keys is one): nothing past n_keys is ever read
    fwd8::dma_tile<D>(dma, wave, kbase + row0 * p.kv_rs, vbase + row0 * p.kv_rs, p.kv_rs, p.kv_rs, p.n_keys - j * KVT, sl);
  };

  // ---- main loop: tile j in LDS slot (j - j_begin) & 1, tile j + 1 lands under its MFMA work ---------------------------------------
  f32x16 s0, s1;
  if (j_begin < j_end) dma_tile(j_begin, lds0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  int slot = 0;
  for (int j = j_begin; j < j_end; ++j) {
    if (j + 1 < j_end) dma_tile(j + 1, lds0 + (slot ^ 1) * SLOTB);
    const unsigned sl = lds0 + slot * SLOTB;
    const int k0 = j * KVT;
    if (k0 <= wave_lim) {                               // wave-uniform: some row of this wave sees a key of the tile
      fwd8::qk_phase<D>(sl, koff, qf, s0, s1);
      if (k0 + KVT - 1 > wave_min_lim) {                // the tile reaches past the n_full / diagonal / n_keys limit of some row
        const int lim = my_lim - k0;                    // key <= lim visible
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int key = (r & 3) + 8 * (r >> 2) + 4 * hi;
          if (key > lim) s0[r] = -INFINITY;
          if (key + 32 > lim) s1[r] = -INFINITY;
        }
      }
      // quant_m (every launch whose shape is split over the keys): the running max moves on INTEGERS of the log2 domain.  Two histories
      // of a row (one split or many, wherever the cuts fall) then differ by whole powers of two in every p = 2^(s - m): bf16(p) is the
      // same mantissa, the rescales are exact, and the splits compose to the unsplit result up to fp32 summation order.  With a real-valued
      // max the two bf16 roundings of p are unrelated and split and unsplit results sit 2.8e-3 apart (each 2.2e-3 from the exact one).
      // Unsplit shapes keep the real-valued max: the prefill kernel's arithmetic on the same rows.
      float m_tile = fwd8::tile_row_max(s0, s1) * scale_log2e;
      if (p.quant_m) m_tile = ceilf(m_tile);
      fwd8::softmax_step<D>(m_tile, scale_log2e, s0, s1, m_run, l_run, o_acc);
      fwd8::pv_phase<D, SPLIT_P ? 2 : 1>(sl, voff, s0, s1, o_acc);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");    // this wave's DMA pieces have landed
    __syncthreads();
    slot ^= 1;
  }

  // ---- epilogue ------------------------------------------------------------------------------------------------------------------------
  const float l_tot = swap32_sum(l_run);
  if (!live) return;
  const int head = kvh * G + my_hq;
  if (p.n_splits == 1 && !p.partial_out) {
    fwd8::store_row_bf16<D>(p.o + (int64_t)my_row * p.o_rs + (int64_t)head * p.o_hs, o_acc, l_tot > 0.f ? 1.0f / l_tot : 0.f, hi);
    if (p.lse && hi == 0) p.lse[(int64_t)head * p.t + my_row] = fwd8::lse_natural(m_run, l_tot);
  } else {
    const int64_t rec = SEG ? ((int64_t)launch.n_splits * (p.n_kv_heads * G) + head) * launch.t + seg_first + my_row
                            : ((int64_t)split * (p.n_kv_heads * G) + head) * p.t + my_row;
    float* po = p.po + rec * D;
#pragma unroll
    for (int db = 0; db < DB; ++db) {
#pragma unroll
      for (int rg = 0; rg < 4; ++rg) {
        const f32x4 w = {o_acc[db][rg * 4 + 0], o_acc[db][rg * 4 + 1], o_acc[db][rg * 4 + 2], o_acc[db][rg * 4 + 3]};
        *reinterpret_cast<f32x4*>(po + 32 * db + 8 * rg + 4 * hi) = w;
      }
    }
    if (hi == 0) { p.pm[rec] = m_run; p.pl[rec] = l_tot; }
  }
}

// ---- merge of the key splits: one wave per (head, row); lane p < n_splits holds part p's statistics, every lane two columns ------------
__global__ __launch_bounds__(256) void extend_merge_kernel(const float* __restrict__ pm, const float* __restrict__ pl,
                                                           const float* __restrict__ po, int n_splits, int64_t n_rec, int t,
                                                           bf16_t* __restrict__ out, int64_t o_rs, int64_t o_hs, float* __restrict__ lse) {
  const int lane = threadIdx.x & 63;
  const int64_t rec = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);       // head * t + row
  if (rec >= n_rec) return;
  const bool has = lane < n_splits;
  const float m = has ? pm[(int64_t)lane * n_rec + rec] : -1.0e30f;       // an empty part carries m = -1e30, l = 0
  float M = m;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) M = fmaxf(M, __shfl_xor(M, o));
  const float w = has ? __builtin_amdgcn_exp2f(m - M) : 0.f;
  const float L = wave_reduce_sum(has ? pl[(int64_t)lane * n_rec + rec] * w : 0.f);
  float a0 = 0.f, a1 = 0.f;
  for (int s = 0; s < n_splits; ++s) {
    const float ws = __shfl(w, s);
    const float2 v = *reinterpret_cast<const float2*>(po + ((int64_t)s * n_rec + rec) * D + 2 * lane);
    a0 += v.x * ws;
    a1 += v.y * ws;
  }
  const float inv = L > 0.f ? 1.0f / L : 0.f;
  const int64_t head = rec / t, row = rec - head * t;
  *reinterpret_cast<unsigned*>(out + row * o_rs + head * o_hs + 2 * lane) = pack_bf16x2(a0 * inv, a1 * inv);
  if (lse && lane == 0) lse[rec] = L > 0.f ? (M + log2f(L)) * 0.69314718055994530942f : -INFINITY;
}

// The split count: a function of the shapes only (and, under VITA_DEBUG, of VITA_ATTN_EXTEND_SPLITS — the tests force 1 and the maximum).
// The smallest count that gives the launch kTargetBlocks workgroups, every split at least kMinTilesPerSplit key tiles.
int extend_splits(int64_t t, int n_q_heads, int64_t n_keys, bool allow_override = true) {
  const int64_t key_tiles = (n_keys + KVT - 1) / KVT;
  const int64_t cap = key_tiles < kMaxSplits ? (key_tiles < 1 ? 1 : key_tiles) : kMaxSplits;
  int64_t splits;
  const char* e = vita_dev_getenv("VITA_ATTN_EXTEND_SPLITS");
  if (allow_override && e && atoi(e) > 0) {
    splits = atoi(e);
  } else {
    const int64_t blocks = (t * n_q_heads + QTILE - 1) / QTILE;     // 256-row tiles of the stacked (row, head) pairs, all kv groups
    splits = (kTargetBlocks + blocks - 1) / blocks;
    const int64_t by_len = key_tiles / kMinTilesPerSplit;
    if (splits > by_len) splits = by_len;
  }
  if (splits > cap) splits = cap;
  if (splits < 1) splits = 1;
  const int64_t per = (key_tiles + splits - 1) / splits;           // whole tiles per split; drop splits that would start past the end
  return per > 0 ? (int)((key_tiles + per - 1) / per) : 1;
}

bool extend_shape_ok(int64_t t, int n_q_heads, int64_t n_keys) { return t > 0 && n_q_heads > 0 && n_keys > 0; }

// ---- beam search (M/inference/text_generation/generation.py:283-471): the B beams of one request share the prompt --------------------
// Query row b = beam b.  The prefix rows [0, L) of the cache shard are common to all beams: flash_extend_kernel<true> runs with t = B,
// n_full = n_keys = L — every key visible to every row, the (beam, head) pairs of a kv group stacked on the MFMA rows — so a workgroup
// reads each prefix K / V tile once for all beams, and leaves its fp32 partials.  A beam's own generated tokens live in the tail cache
// [tail_cap][B][kv groups][128]: step s of slot j is row s * B + j, and beam b's key of step s is slot anc[b][s].  beam_tail_kernel
// (VALU, decode_attn_partial_kernel's lane layout: 16 lanes per 256-byte row, 4 rows per wave instruction, 4 row loads in flight)
// gives one workgroup to each (beam, kv group) and writes one more partial, part index n_splits; extend_merge_kernel folds all of them.
// Every table entry is clamped into [0, B) before it forms an address.
constexpr int kBeamMax = 8;
constexpr int kBeamMaxSplits = kMaxSplits - 1;          // extend_merge_kernel: one lane per part, the tail partial is one of them

// The tail pass of ONE (row, kv group) — the key loop, the softmax step, the cross-wave fold and the partial record — has one owner:
// beam_tail_kernel and prefix_batch_tail_kernel (grid: row b x kv group g) run these statements and differ only in how a key index
// becomes an address: make_key_off(b, g, sub) is called once, where the loop's invariants are formed, and returns key_off(key), the
// element offset of key < n_keys — its 128-wide row of this group, the lane's 8 elements — behind kt / vt.  n_keys <= 0 writes the
// merge's neutral element and reads neither kt / vt nor anything key_off names.
template <int QPG, class MakeKeyOff>
__device__ __forceinline__ void tail_partial_body(const bf16_t* __restrict__ q, int64_t q_rs, int64_t q_gs, int64_t q_hs,
                                                  const bf16_t* __restrict__ kt, const bf16_t* __restrict__ vt, int n_keys,
                                                  MakeKeyOff make_key_off, int B, float scale_log2, float* __restrict__ pm,
                                                  float* __restrict__ pl, float* __restrict__ po, int64_t part_base) {
  constexpr int ITS = 4;                                  // K / V row loads in flight per lane
  constexpr int kWaveKeys = ITS * 4;
  __shared__ float wm[4][QPG], wl[4][QPG];
  __shared__ float wo[4][QPG][D];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int sub = lane & 15, kq = lane >> 4;
  const int b = blockIdx.x, g = blockIdx.y;
  const int64_t rec0 = part_base + (int64_t)g * QPG * B + b;          // record of head h: rec0 + h * B
  if (n_keys <= 0) {                                      // no key of its own yet: the merge's neutral element
    if (t < QPG) { pm[rec0 + (int64_t)t * B] = -1.0e30f; pl[rec0 + (int64_t)t * B] = 0.f; }
    if (t < D)
      for (int h = 0; h < QPG; ++h) po[(rec0 + (int64_t)h * B) * D + t] = 0.f;
    return;
  }
  unsigned qp[QPG][4];
#pragma unroll
  for (int h = 0; h < QPG; ++h) {
    const u32x4 qv = *reinterpret_cast<const u32x4*>(q + b * q_rs + g * q_gs + h * q_hs + sub * 8);
#pragma unroll
    for (int j = 0; j < 4; ++j) qp[h][j] = qv[j];
  }
  float mrun[QPG], lrun[QPG], acc[QPG][8];
#pragma unroll
  for (int h = 0; h < QPG; ++h) {
    mrun[h] = -INFINITY;
    lrun[h] = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[h][i] = 0.f;
  }
  const auto key_off = make_key_off(b, g, sub);

  for (int key0 = wave * kWaveKeys; key0 < n_keys; key0 += 4 * kWaveKeys) {
    u32x4 kr[ITS], vr[ITS];
#pragma unroll
    for (int it = 0; it < ITS; ++it) {
      const int key = key0 + it * 4 + kq;
      kr[it] = u32x4{0u, 0u, 0u, 0u};
      vr[it] = u32x4{0u, 0u, 0u, 0u};
      if (key < n_keys) {
        const int64_t off = key_off(key);
        kr[it] = *reinterpret_cast<const u32x4*>(kt + off);
        vr[it] = *reinterpret_cast<const u32x4*>(vt + off);
      }
    }
    float p[QPG][ITS];
#pragma unroll
    for (int h = 0; h < QPG; ++h) {
      float tm = -INFINITY;
#pragma unroll
      for (int it = 0; it < ITS; ++it) {
        float sv = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) sv = dot2_bf16(qp[h][j], kr[it][j], sv);
        sv = row16_allreduce_sum(sv) * scale_log2;
        sv = (key0 + it * 4 + kq < n_keys) ? sv : -INFINITY;
        p[h][it] = sv;
        tm = fmaxf(tm, sv);
      }
      tm = fmaxf(tm, __shfl_xor(tm, 16));
      tm = fmaxf(tm, __shfl_xor(tm, 32));                  // finite: key0 < n_keys
      const float mnew = fmaxf(mrun[h], tm);
      const float alpha = __builtin_amdgcn_exp2f(mrun[h] - mnew);        // exp2(-inf) = 0 on the first tile
      mrun[h] = mnew;
      float ls = 0.f;
#pragma unroll
      for (int it = 0; it < ITS; ++it) {
        p[h][it] = __builtin_amdgcn_exp2f(p[h][it] - mnew);
        ls += p[h][it];
      }
      lrun[h] = lrun[h] * alpha + ls;
#pragma unroll
      for (int i = 0; i < 8; ++i) acc[h][i] *= alpha;
    }
#pragma unroll
    for (int it = 0; it < ITS; ++it) {
      float vf[8];
#pragma unroll
      for (int i = 0; i < 4; ++i) { vf[2 * i] = bf16lo_to_f32(vr[it][i]); vf[2 * i + 1] = bf16hi_to_f32(vr[it][i]); }
#pragma unroll
      for (int h = 0; h < QPG; ++h)
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[h][i] += p[h][it] * vf[i];
    }
  }
#pragma unroll
  for (int h = 0; h < QPG; ++h) {
    float l = lrun[h];
    l += __shfl_xor(l, 16);
    l += __shfl_xor(l, 32);
    if (lane == 0) { wm[wave][h] = mrun[h]; wl[wave][h] = l; }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      float v = acc[h][i];
      v += __shfl_xor(v, 16);
      v += __shfl_xor(v, 32);
      if (kq == 0) wo[wave][h][sub * 8 + i] = v;
    }
  }
  __syncthreads();
  if (t < D) {
#pragma unroll
    for (int h = 0; h < QPG; ++h) {
      const float M = fmaxf(fmaxf(wm[0][h], wm[1][h]), fmaxf(wm[2][h], wm[3][h]));   // finite: wave 0 had a tile
      float L = 0.f, O = 0.f;
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        const float f = (wm[w][h] == -INFINITY) ? 0.f : __builtin_amdgcn_exp2f(wm[w][h] - M);
        L += wl[w][h] * f;
        O += wo[w][h][t] * f;
      }
      po[(rec0 + (int64_t)h * B) * D + t] = O;
      if (t == 0) { pm[rec0 + (int64_t)h * B] = M; pl[rec0 + (int64_t)h * B] = L; }
    }
  }
}

template <int QPG>
__global__ __launch_bounds__(256) void beam_tail_kernel(const bf16_t* __restrict__ q, int64_t q_rs, int64_t q_gs, int64_t q_hs,
                                                        const bf16_t* __restrict__ kt, const bf16_t* __restrict__ vt,
                                                        const int* __restrict__ anc, int64_t tail_cap, int B, int n_gen,
                                                        float scale_log2, float* __restrict__ pm, float* __restrict__ pl,
                                                        float* __restrict__ po, int64_t part_base) {
  const int G = gridDim.y;
  auto make_key_off = [=](int b, int g, int sub) __attribute__((always_inline)) {
    const int64_t slot_stride = (int64_t)G * D, step_stride = (int64_t)B * slot_stride;
    const int* my_anc = anc + (int64_t)b * tail_cap;
    const int64_t goff = (int64_t)g * D + sub * 8;
    return [=](int key) __attribute__((always_inline)) {
      int slot = my_anc[key];
      slot = slot < 0 ? 0 : (slot >= B ? B - 1 : slot);              // a corrupt table gives wrong numbers, never a stray address
      return (int64_t)key * step_stride + (int64_t)slot * slot_stride + goff;
    };
  };
  tail_partial_body<QPG>(q, q_rs, q_gs, q_hs, kt, vt, n_gen, make_key_off, B, scale_log2, pm, pl, po, part_base);
}

// ---- several continuations of one prefilled prompt (M/inference/text_generation/generation.py:33-280 at batch_size > 1, the rows
// sharing their first prefix_len tokens).  The prefix pass is the beams': query row b = continuation b.  Row b's own tokens live in a
// tail of its own, [tail_cap][kv groups][128] behind tail_ptrs[b] = {K base, V base} (the table of decode_attn_batch_partial_kernel),
// and it holds min(max(tail_lens[b], 0), tail_cap) of them: the length is read on the device, clamped before it bounds an address,
// and an idle row (length <= 0) reads neither its table entry nor its tail.
template <int QPG>
__global__ __launch_bounds__(256) void prefix_batch_tail_kernel(const bf16_t* __restrict__ q, int64_t q_rs, int64_t q_gs, int64_t q_hs,
                                                                const bf16_t* const* __restrict__ tail_ptrs, int64_t tail_rs,
                                                                int64_t tail_gs, const int* __restrict__ tail_lens, int tail_cap,
                                                                int B, float scale_log2, float* __restrict__ pm,
                                                                float* __restrict__ pl, float* __restrict__ po, int64_t part_base) {
  const int b = blockIdx.x;
  int n = tail_lens[b];
  n = n < 0 ? 0 : (n > tail_cap ? tail_cap : n);
  const bf16_t* kt = n > 0 ? tail_ptrs[2 * b] : nullptr;
  const bf16_t* vt = n > 0 ? tail_ptrs[2 * b + 1] : nullptr;
  auto make_key_off = [=](int, int g, int sub) __attribute__((always_inline)) {
    const int64_t goff = (int64_t)g * tail_gs + sub * 8;
    return [=](int key) __attribute__((always_inline)) { return (int64_t)key * tail_rs + goff; };
  };
  tail_partial_body<QPG>(q, q_rs, q_gs, q_hs, kt, vt, n, make_key_off, B, scale_log2, pm, pl, po, part_base);
}

// key splits of the prefix pass: extend_splits' rule for t = B rows (a function of the shapes only), at most kBeamMaxSplits
int beam_splits(int n_beams, int n_q_heads, int64_t prefix_len) {
  int splits = extend_splits(n_beams, n_q_heads, prefix_len, false);
  if (splits > kBeamMaxSplits) {
    const int64_t key_tiles = (prefix_len + KVT - 1) / KVT;
    const int64_t per = (key_tiles + kBeamMaxSplits - 1) / kBeamMaxSplits;
    splits = (int)((key_tiles + per - 1) / per);
  }
  return splits;
}

constexpr int kPrefixExtendMaxTokens = 1 << 15;         // query rows of one ragged pass (vita_prefix_extend_attn_fwd)

bool beam_shape_ok(int n_beams, int n_q_heads, int64_t prefix_len, int max_rows = kBeamMax) {
  return n_beams >= 1 && n_beams <= max_rows && n_q_heads > 0 && prefix_len > 0 && prefix_len <= 0x7fffffffLL - 256;
}

}  // namespace

extern "C" size_t vita_flash_attn_extend_workspace_bytes(int64_t t, int n_q_heads, int64_t n_keys) {
  if (!extend_shape_ok(t, n_q_heads, n_keys)) return 0;
  const int splits = extend_splits(t, n_q_heads, n_keys);
  return splits == 1 ? 0 : (size_t)splits * (size_t)n_q_heads * (size_t)t * (D + 2) * sizeof(float);
}

extern "C" int vita_flash_attn_extend_fwd(const vita_attn_extend_params* p, void* stream) {
  if (!p || !p->q || !p->k_cache || !p->v_cache || !p->out) return VITA_ERR_INVALID_ARG;
  if (!extend_shape_ok(p->t, p->n_q_heads, p->n_keys) || p->n_kv_heads <= 0 || p->n_q_heads % p->n_kv_heads) return VITA_ERR_INVALID_ARG;
  if (p->n_full < 0 || p->n_full > p->n_keys || p->key_pos_step < 1 || p->q_pos0 < 0 || p->key_pos0 < 0) return VITA_ERR_INVALID_ARG;
  // the running max is max(score) * scale: the scale must be positive (and finite); distinct cache rows need a positive row stride
  if (!(p->softmax_scale > 0.f) || !(p->softmax_scale < INFINITY) || p->kv_row_stride <= 0) return VITA_ERR_INVALID_ARG;
  if (p->head_dim != D) return VITA_ERR_UNSUPPORTED;
  if (p->n_keys > 0x7fffffffLL - 256 || p->t * (int64_t)p->n_q_heads > 0x7fffff00LL || p->q_pos0 + p->t > (int64_t(1) << 40))
    return VITA_ERR_UNSUPPORTED;
  const int64_t strides[] = {p->q_row_stride, p->q_group_stride, p->q_head_stride, p->kv_row_stride, p->kv_group_stride,
                             p->out_row_stride, p->out_head_stride};
  for (int64_t s : strides)
    if (s & 7) return VITA_ERR_UNSUPPORTED;            // 16-byte vector loads / LDS-DMA pieces
  if (p->kv_row_stride * KVT > 0x7fffffffLL) return VITA_ERR_UNSUPPORTED;   // 32-bit lane offsets inside a tile
  const uintptr_t bases = (uintptr_t)p->q | (uintptr_t)p->k_cache | (uintptr_t)p->v_cache | (uintptr_t)p->out;
  if (bases & 15) return VITA_ERR_UNSUPPORTED;         // 16-byte vector loads / LDS-DMA pieces start at the bases
  if ((uintptr_t)p->lse & 3) return VITA_ERR_UNSUPPORTED;   // word stores

  ExtArgs a;
  a.q = (const bf16_t*)p->q; a.q_rs = p->q_row_stride; a.q_gs = p->q_group_stride; a.q_hs = p->q_head_stride;
  a.k = (const bf16_t*)p->k_cache; a.v = (const bf16_t*)p->v_cache; a.kv_rs = p->kv_row_stride; a.kv_gs = p->kv_group_stride;
  a.o = (bf16_t*)p->out; a.o_rs = p->out_row_stride; a.o_hs = p->out_head_stride;
  a.lse = p->lse;
  a.t = (int)p->t; a.G = p->n_q_heads / p->n_kv_heads; a.n_kv_heads = p->n_kv_heads;
  a.n_q_tiles = (int)((p->t * a.G + QTILE - 1) / QTILE);
  a.n_keys = (int)p->n_keys; a.n_full = (int)p->n_full;
  a.q_pos0 = p->q_pos0; a.key_pos0 = p->key_pos0; a.key_pos_step = p->key_pos_step;
  a.n_splits = extend_splits(p->t, p->n_q_heads, p->n_keys);
  const int64_t key_tiles = (p->n_keys + KVT - 1) / KVT;
  a.tiles_per_split = (int)((key_tiles + a.n_splits - 1) / a.n_splits);
  a.quant_m = extend_splits(p->t, p->n_q_heads, p->n_keys, false) > 1;      // by shape, whatever the developer switch forces
  a.partial_out = 0;
  a.scale_log2e = p->softmax_scale * LOG2E;
  const int64_t n_rec = (int64_t)p->n_q_heads * p->t;
  a.pm = a.pl = a.po = nullptr;
  if (a.n_splits > 1) {
    const size_t need = (size_t)a.n_splits * (size_t)n_rec * (D + 2) * sizeof(float);
    if (!p->workspace || p->workspace_bytes < need || ((uintptr_t)p->workspace & 15)) return VITA_ERR_INVALID_ARG;
    a.po = (float*)p->workspace;                                   // [splits][heads][t][128], then m and l [splits][heads][t]
    a.pm = a.po + (int64_t)a.n_splits * n_rec * D;
    a.pl = a.pm + (int64_t)a.n_splits * n_rec;
  }
  const int64_t nblocks = (int64_t)a.n_kv_heads * a.n_q_tiles * a.n_splits;
  if (nblocks > 0x7fffffff) return VITA_ERR_UNSUPPORTED;

  constexpr int lds = 2 * 2 * KVT * D * 2;
  static std::atomic<unsigned long long> attr_set{0};
  vita_device_once(attr_set, [&] {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&flash_extend_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&flash_extend_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
  });
  hipStream_t st = (hipStream_t)stream;
  if (a.n_q_tiles == 1) hipLaunchKernelGGL(flash_extend_kernel<true>, dim3((unsigned)nblocks), dim3(512), lds, st, a);
  else hipLaunchKernelGGL(flash_extend_kernel<false>, dim3((unsigned)nblocks), dim3(512), lds, st, a);
  int rc = vita_check_launch();
  if (rc != VITA_OK || a.n_splits == 1) return rc;
  hipLaunchKernelGGL(extend_merge_kernel, dim3((unsigned)((n_rec + 3) / 4)), dim3(256), 0, st, a.pm, a.pl, a.po, a.n_splits, n_rec, a.t,
                     a.o, a.o_rs, a.o_hs, a.lse);
  return vita_check_launch();
}

extern "C" size_t vita_beam_attn_workspace_bytes(int n_beams, int n_q_heads, int64_t prefix_len) {
  if (!beam_shape_ok(n_beams, n_q_heads, prefix_len)) return 0;
  return (size_t)(beam_splits(n_beams, n_q_heads, prefix_len) + 1) * (size_t)n_q_heads * (size_t)n_beams * (D + 2) * sizeof(float);
}

namespace {

// What vita_beam_attn_fwd and vita_prefix_batch_attn_fwd share: B query rows in the mixed QKV buffer, one read-only prefix, a tail
// partial behind the prefix splits.  The checks of the common arguments (the entry's own stand between the two), the prefix launch
// and the merge each have one owner.
struct PrefixArgs {
  const void* q; int64_t q_rs, q_gs, q_hs;
  const void *k, *v; int64_t kv_rs, kv_gs, prefix_len;
  int n_rows, n_q_heads, n_kv_heads, head_dim;
  float scale;
  void *out, *ws; size_t ws_bytes;
};

int prefix_args_invalid(const PrefixArgs& p) {
  if (!p.q || !p.k || !p.v || !p.out || !p.ws) return VITA_ERR_INVALID_ARG;
  if (p.n_rows < 1 || p.n_q_heads <= 0 || p.n_kv_heads <= 0 || p.n_q_heads % p.n_kv_heads || p.prefix_len <= 0) return VITA_ERR_INVALID_ARG;
  // positive and finite, read off the bits: this file is compiled with -fno-honor-nans, which folds a NaN away from float compares
  unsigned scale_bits;
  __builtin_memcpy(&scale_bits, &p.scale, sizeof scale_bits);
  if (scale_bits == 0u || scale_bits >= 0x7f800000u || p.kv_rs <= 0) return VITA_ERR_INVALID_ARG;
  return VITA_OK;
}

int prefix_args_unsupported(const PrefixArgs& p, int max_rows = kBeamMax) {
  if (p.head_dim != D || p.n_q_heads / p.n_kv_heads > 8 || !beam_shape_ok(p.n_rows, p.n_q_heads, p.prefix_len, max_rows))
    return VITA_ERR_UNSUPPORTED;
  const int64_t strides[] = {p.q_rs, p.q_gs, p.q_hs, p.kv_rs, p.kv_gs};
  for (int64_t s : strides)
    if (s & 7) return VITA_ERR_UNSUPPORTED;            // 16-byte vector loads / LDS-DMA pieces
  if (p.kv_rs * KVT > 0x7fffffffLL) return VITA_ERR_UNSUPPORTED;   // 32-bit lane offsets inside a tile
  const uintptr_t bases = (uintptr_t)p.q | (uintptr_t)p.k | (uintptr_t)p.v | (uintptr_t)p.out | (uintptr_t)p.ws;
  return (bases & 15) ? VITA_ERR_UNSUPPORTED : VITA_OK;
}

// flash_extend_kernel over the prefix, every key visible to every row (<true> while the stacked rows fit one query tile: the beams
// and the batched step always, a ragged pass of n_rows * G <= 256); the partials stay in the workspace, one more part kept free behind
// the splits for the tail pass
int prefix_pass(const PrefixArgs& p, ExtArgs& a, hipStream_t st) {
  a.q = (const bf16_t*)p.q; a.q_rs = p.q_rs; a.q_gs = p.q_gs; a.q_hs = p.q_hs;
  a.k = (const bf16_t*)p.k; a.v = (const bf16_t*)p.v; a.kv_rs = p.kv_rs; a.kv_gs = p.kv_gs;
  a.o = (bf16_t*)p.out; a.o_rs = (int64_t)p.n_q_heads * D; a.o_hs = D;
  a.lse = nullptr;
  a.t = p.n_rows; a.G = p.n_q_heads / p.n_kv_heads; a.n_kv_heads = p.n_kv_heads;
  a.n_q_tiles = (p.n_rows * a.G + QTILE - 1) / QTILE;            // 1 for B <= 8 rows (B * qpg <= 64 stacked rows)
  a.n_keys = (int)p.prefix_len; a.n_full = (int)p.prefix_len;   // every prefix key is visible to every row
  a.q_pos0 = 0; a.key_pos0 = 0; a.key_pos_step = 1;
  a.n_splits = beam_splits(p.n_rows, p.n_q_heads, p.prefix_len);
  const int64_t key_tiles = (p.prefix_len + KVT - 1) / KVT;
  a.tiles_per_split = (int)((key_tiles + a.n_splits - 1) / a.n_splits);
  a.quant_m = 1;                                                // the partials are always merged: see the kernel's main loop
  a.partial_out = 1;
  a.scale_log2e = p.scale * LOG2E;
  const int64_t n_rec = (int64_t)p.n_q_heads * p.n_rows;
  const int n_parts = a.n_splits + 1;
  const size_t need = (size_t)n_parts * (size_t)n_rec * (D + 2) * sizeof(float);
  if (p.ws_bytes < need) return VITA_ERR_INVALID_ARG;
  a.po = (float*)p.ws;                                          // [parts][heads][B][128], then m and l [parts][heads][B]
  a.pm = a.po + (int64_t)n_parts * n_rec * D;
  a.pl = a.pm + (int64_t)n_parts * n_rec;

  constexpr int lds = 2 * 2 * KVT * D * 2;
  static std::atomic<unsigned long long> attr_set{0};
  vita_device_once(attr_set, [&] {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&flash_extend_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&flash_extend_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
  });
  const dim3 grid((unsigned)(p.n_kv_heads * a.n_q_tiles * a.n_splits));
  if (a.n_q_tiles == 1) hipLaunchKernelGGL(flash_extend_kernel<true>, grid, dim3(512), lds, st, a);
  else hipLaunchKernelGGL(flash_extend_kernel<false>, grid, dim3(512), lds, st, a);
  return vita_check_launch();
}

int prefix_merge(const ExtArgs& a, hipStream_t st) {
  const int64_t n_rec = (int64_t)a.n_kv_heads * a.G * a.t;
  hipLaunchKernelGGL(extend_merge_kernel, dim3((unsigned)((n_rec + 3) / 4)), dim3(256), 0, st, a.pm, a.pl, a.po, a.n_splits + 1, n_rec,
                     a.t, a.o, a.o_rs, a.o_hs, (float*)nullptr);
  return vita_check_launch();
}

}  // namespace

extern "C" int vita_beam_attn_fwd(const void* q, int64_t q_row_stride, int64_t q_group_stride, int64_t q_head_stride,
                                  const void* k_cache, const void* v_cache, int64_t kv_row_stride, int64_t kv_group_stride,
                                  int64_t prefix_len, const void* k_tail, const void* v_tail, int64_t tail_cap,
                                  const int32_t* ancestry, int n_beams, int n_gen, int n_q_heads, int n_kv_heads, int head_dim,
                                  float softmax_scale, void* out, void* workspace, size_t workspace_bytes, void* stream) {
  const PrefixArgs p = {q, q_row_stride, q_group_stride, q_head_stride, k_cache, v_cache, kv_row_stride, kv_group_stride, prefix_len,
                        n_beams, n_q_heads, n_kv_heads, head_dim, softmax_scale, out, workspace, workspace_bytes};
  int rc = prefix_args_invalid(p);
  if (rc != VITA_OK) return rc;
  if (n_gen < 0 || tail_cap < 0 || n_gen > tail_cap || (n_gen > 0 && (!k_tail || !v_tail || !ancestry))) return VITA_ERR_INVALID_ARG;
  rc = prefix_args_unsupported(p);
  if (rc != VITA_OK) return rc;
  if (((uintptr_t)k_tail | (uintptr_t)v_tail) & 15) return VITA_ERR_UNSUPPORTED;
  if ((uintptr_t)ancestry & 3) return VITA_ERR_UNSUPPORTED;

  ExtArgs a;
  hipStream_t st = (hipStream_t)stream;
  rc = prefix_pass(p, a, st);
  if (rc != VITA_OK) return rc;
  const dim3 tgrid((unsigned)n_beams, (unsigned)n_kv_heads);
  const float sl2 = softmax_scale * LOG2E;
  const int64_t part_base = (int64_t)a.n_splits * n_q_heads * n_beams;
#define VITA_BEAM_TAIL(Q)                                                                                                         \
  case Q:                                                                                                                         \
    hipLaunchKernelGGL(beam_tail_kernel<Q>, tgrid, dim3(256), 0, st, a.q, a.q_rs, a.q_gs, a.q_hs, (const bf16_t*)k_tail,           \
                       (const bf16_t*)v_tail, (const int*)ancestry, tail_cap, n_beams, n_gen, sl2, a.pm, a.pl, a.po, part_base);  \
    break;
  switch (a.G) {
    VITA_BEAM_TAIL(1) VITA_BEAM_TAIL(2) VITA_BEAM_TAIL(3) VITA_BEAM_TAIL(4) VITA_BEAM_TAIL(5) VITA_BEAM_TAIL(6) VITA_BEAM_TAIL(7)
    VITA_BEAM_TAIL(8)
  }
#undef VITA_BEAM_TAIL
  rc = vita_check_launch();
  if (rc != VITA_OK) return rc;
  return prefix_merge(a, st);
}

extern "C" size_t vita_prefix_batch_attn_workspace_bytes(int n_rows, int n_q_heads, int64_t prefix_len) {
  return vita_beam_attn_workspace_bytes(n_rows, n_q_heads, prefix_len);       // the same parts: the prefix splits and one tail partial
}

extern "C" int vita_prefix_batch_attn_fwd(const void* q, int64_t q_row_stride, int64_t q_group_stride, int64_t q_head_stride,
                                          const void* k_cache, const void* v_cache, int64_t kv_row_stride, int64_t kv_group_stride,
                                          int64_t prefix_len, const void* tail_ptrs, int64_t tail_row_stride,
                                          int64_t tail_group_stride, const int32_t* tail_lens, int tail_cap, int n_rows, int n_q_heads,
                                          int n_kv_heads, int head_dim, float softmax_scale, void* out, void* workspace,
                                          size_t workspace_bytes, void* stream) {
  const PrefixArgs p = {q, q_row_stride, q_group_stride, q_head_stride, k_cache, v_cache, kv_row_stride, kv_group_stride, prefix_len,
                        n_rows, n_q_heads, n_kv_heads, head_dim, softmax_scale, out, workspace, workspace_bytes};
  int rc = prefix_args_invalid(p);
  if (rc != VITA_OK) return rc;
  if (!tail_ptrs || !tail_lens || tail_cap < 0 || tail_row_stride < 0 || tail_group_stride < 0) return VITA_ERR_INVALID_ARG;
  rc = prefix_args_unsupported(p);
  if (rc != VITA_OK) return rc;
  if ((tail_row_stride | tail_group_stride) & 7) return VITA_ERR_UNSUPPORTED;          // 16-byte vector loads of the tail rows
  if (((uintptr_t)tail_ptrs & 7) || ((uintptr_t)tail_lens & 3)) return VITA_ERR_UNSUPPORTED;

  ExtArgs a;
  hipStream_t st = (hipStream_t)stream;
  rc = prefix_pass(p, a, st);
  if (rc != VITA_OK) return rc;
  const dim3 tgrid((unsigned)n_rows, (unsigned)n_kv_heads);
  const float sl2 = softmax_scale * LOG2E;
  const int64_t part_base = (int64_t)a.n_splits * n_q_heads * n_rows;
#define VITA_PREFIX_TAIL(Q)                                                                                                        \
  case Q:                                                                                                                          \
    hipLaunchKernelGGL(prefix_batch_tail_kernel<Q>, tgrid, dim3(256), 0, st, a.q, a.q_rs, a.q_gs, a.q_hs,                           \
                       (const bf16_t* const*)tail_ptrs, tail_row_stride, tail_group_stride, (const int*)tail_lens, tail_cap,       \
                       n_rows, sl2, a.pm, a.pl, a.po, part_base);                                                                  \
    break;
  switch (a.G) {
    VITA_PREFIX_TAIL(1) VITA_PREFIX_TAIL(2) VITA_PREFIX_TAIL(3) VITA_PREFIX_TAIL(4) VITA_PREFIX_TAIL(5) VITA_PREFIX_TAIL(6)
    VITA_PREFIX_TAIL(7) VITA_PREFIX_TAIL(8)
  }
#undef VITA_PREFIX_TAIL
  rc = vita_check_launch();
  if (rc != VITA_OK) return rc;
  return prefix_merge(a, st);
}

// ---- a ragged pass behind the shared prefix: count_b new tokens of every continuation row b in one launch set ------------------------
// The prefix pass with t = n_tokens query rows, the segment launch of flash_extend_kernel for every row's new tokens over its own
// tail (part n_splits), the merge.  Both launches take two bf16 terms of P while n_tokens * G <= 256, one beyond (SPLIT_P's rule).
extern "C" size_t vita_prefix_extend_attn_workspace_bytes(int64_t n_tokens, int n_q_heads, int64_t prefix_len) {
  if (n_tokens > kPrefixExtendMaxTokens || !beam_shape_ok((int)n_tokens, n_q_heads, prefix_len, kPrefixExtendMaxTokens)) return 0;
  return (size_t)(beam_splits((int)n_tokens, n_q_heads, prefix_len) + 1) * (size_t)n_q_heads * (size_t)n_tokens * (D + 2) * sizeof(float);
}

extern "C" int vita_prefix_extend_attn_fwd(const void* q, int64_t q_row_stride, int64_t q_group_stride, int64_t q_head_stride,
                                           const void* k_cache, const void* v_cache, int64_t kv_row_stride, int64_t kv_group_stride,
                                           int64_t prefix_len, const void* tail_ptrs, int64_t tail_row_stride,
                                           int64_t tail_group_stride, int tail_cap, const int32_t* segments, int n_rows,
                                           int64_t n_tokens, int max_count, int n_q_heads, int n_kv_heads, int head_dim,
                                           float softmax_scale, void* out, void* workspace, size_t workspace_bytes, void* stream) {
  if (n_tokens < 1) return VITA_ERR_INVALID_ARG;
  if (n_tokens > kPrefixExtendMaxTokens) return VITA_ERR_UNSUPPORTED;
  const PrefixArgs p = {q, q_row_stride, q_group_stride, q_head_stride, k_cache, v_cache, kv_row_stride, kv_group_stride, prefix_len,
                        (int)n_tokens, n_q_heads, n_kv_heads, head_dim, softmax_scale, out, workspace, workspace_bytes};
  int rc = prefix_args_invalid(p);
  if (rc != VITA_OK) return rc;
  if (!tail_ptrs || !segments || n_rows < 1 || max_count < 0 || tail_cap < 0 || tail_row_stride <= 0 || tail_group_stride < 0)
    return VITA_ERR_INVALID_ARG;
  if (workspace_bytes < vita_prefix_extend_attn_workspace_bytes(n_tokens, n_q_heads, prefix_len)) return VITA_ERR_INVALID_ARG;
  rc = prefix_args_unsupported(p, kPrefixExtendMaxTokens);
  if (rc != VITA_OK) return rc;
  if (n_rows > kBeamMax) return VITA_ERR_UNSUPPORTED;
  if ((tail_row_stride | tail_group_stride) & 7) return VITA_ERR_UNSUPPORTED;          // LDS-DMA pieces of the tail rows
  if (tail_row_stride * KVT > 0x7fffffffLL) return VITA_ERR_UNSUPPORTED;               // 32-bit lane offsets inside a tile
  if (((uintptr_t)tail_ptrs & 7) || ((uintptr_t)segments & 3)) return VITA_ERR_UNSUPPORTED;

  ExtArgs a;
  hipStream_t st = (hipStream_t)stream;
  rc = prefix_pass(p, a, st);
  if (rc != VITA_OK) return rc;
  ExtArgs s = a;                                                  // t = n_tokens and n_splits = the part to write stay the launch's
  s.kv_rs = tail_row_stride; s.kv_gs = tail_group_stride;
  s.tail_ptrs = (const bf16_t* const*)tail_ptrs; s.seg = (const int*)segments;
  s.n_seg = n_rows; s.tail_cap = tail_cap;
  s.seg_max_count = (int)(max_count < n_tokens ? max_count : n_tokens);
  s.n_q_tiles = s.seg_max_count > 0 ? (s.seg_max_count * a.G + QTILE - 1) / QTILE : 1;
  s.tiles_per_split = (tail_cap + KVT - 1) / KVT + 1;             // one split: every tile of a tail
  constexpr int lds = 2 * 2 * KVT * D * 2;
  static std::atomic<unsigned long long> attr_set{0};
  vita_device_once(attr_set, [&] {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&flash_extend_kernel<true, true>), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&flash_extend_kernel<false, true>), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
  });
  const dim3 sgrid((unsigned)n_kv_heads, (unsigned)s.n_q_tiles, (unsigned)n_rows + 1);
  if (a.n_q_tiles == 1) hipLaunchKernelGGL((flash_extend_kernel<true, true>), sgrid, dim3(512), lds, st, s);
  else hipLaunchKernelGGL((flash_extend_kernel<false, true>), sgrid, dim3(512), lds, st, s);
  rc = vita_check_launch();
  if (rc != VITA_OK) return rc;
  return prefix_merge(a, st);
}
