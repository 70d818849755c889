// Flash attention forward for gfx950 (MI355X): online softmax, bf16 I/O, fp32 statistics.
// head_dim 128 (LLM: causal GQA 40:8, zig-zag context-parallel chunk geometry), 96 (SigLIP) and 64 (ViT, non-causal, 1025 tokens):
// the kernel for every geometry attn64.hip / attn64v.hip refuse.  Bound: MFMA; algorithmic work 4 * d flop per visible (q, k) pair.
//
// Structure (one workgroup = 8 waves = 256 query rows of ONE query head; KV tile = 64 keys).  The tile body is attn_fwd8.h's, shared
// with flash_extend_kernel (attn_extend.hip): LDS-DMA of the K|V slot, S^T = K Q^T, the online-softmax step, O^T = V^T P^T with one
// bf16 term of P, the bf16 / lse epilogue.  This file owns:
//   * the double-buffered walk: the DMA of tile t+1 is issued before tile t is computed and lands in the other LDS slot under its
//     MFMA work; one s_waitcnt + barrier per tile.
//   * Sequence geometry is chunked (see vita_attn_params): causal visibility is decided per (query chunk id, key chunk id) pair,
//     element masks (diagonal, ragged last chunk, packed segments) are only evaluated on the tiles that need them.
//   * Workgroup order: kv head = block id % n_kv_heads (= the XCD when n_kv_heads = 8, so one XCD's L2 serves one kv head's K/V
//     stream to all its concurrently running query tiles), query tiles heaviest-first so the causal tail is short.
//
// Reference behaviour restated: M/core/transformer/dot_product_attention.py:186-289 (unfused
// math: softmax(QK^T / sqrt(d)) V with GQA repeat :171-175), :312-329 (ViT, non-causal),
// :374-390 (LLM causal).  Zig-zag chunk ownership: M/training/utils.py:329-341.
#include "attn_args.h"
#include "attn_fwd8.h"
#include <stdlib.h>
#include <type_traits>

namespace {

using fwd8::KVT;
using fwd8::QTILE;

// One kv tile position of the iteration space (all fields wave-uniform -> SGPRs).
struct TileIt {
  int c, j, n;        // chunk, tile inside chunk, tiles to visit in this chunk; c == n_kv_chunks -> end
  int rows;           // valid rows of chunk c
  int diag;           // CAUSAL and chunk c is the query tile's own chunk
  int64_t crow;       // first row of chunk c in the K/V buffers
};

// One variant is built: K/V through the LDS-DMA, K-fragment reads pinned QK_AHEAD = 3 k-steps ahead (attn_fwd8.h).  The register-staging
// path (global_load -> VGPR -> ds_write_b128, loads two tiles ahead), the other QK_AHEAD settings and the shader-clock TIMING
// instrumentation were template parameters nobody instantiated; r14 deleted them with a same-box A / B of every instance family
// (profiles/r14_kernel_bodies_ab.txt; register counts unchanged, profiles/r14_kernel_bodies_isa.txt).
// Measured and dropped: a 3-slot "staggered" schedule (waves 4..7 half a tile behind waves 0..3): 0 to -3 %;
// s_setprio around the MFMA clusters: -2 %; a 4-wave x 64-row variant with one wave per SIMD and compiler-allocated AGPRs: -19 %; an
// in-wave software-pipelined 4-wave x 32-row kernel (exp of tile t between the MFMAs of tile t+1, 4-slot ring): -35 % (LDS-bound;
// see DESIGN.md 4.1, git history).
template <int D, bool CAUSAL>
__global__ __launch_bounds__(512, 2) void flash_fwd_kernel(AttnArgs p) {
  using T = fwd8::Tile<D>;
  constexpr int DS = T::DS, DB = T::DB, SLOTB = T::SLOTB;

  extern __shared__ __attribute__((aligned(16))) char smem[];  // [2][K tile | V tile]
  // LDS byte address of the ring (32-bit); fragment reads use  VGPR(lane offset + slot base) + imm
  const unsigned lds0 = (unsigned)(uintptr_t)(lds_char*)smem;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // provably wave-uniform
  const int hi = lane >> 5, l31 = lane & 31;

  // ---- work decomposition -------------------------------------------------------------------
  const QTileId wg = decode_q_tile(p, blockIdx.x, p.tiles_per_q_chunk);
  const int kvh = wg.kvh, hq = wg.hq, head = wg.head, b = wg.b, qc = wg.qc, qti = wg.qti;
  const int gq = p.q_gid[qc];
  const int q_rows_in_chunk = (qc == p.n_q_chunks - 1) ? p.q_valid : p.chunk_len;
  const int q_off_wg = qti * QTILE;                 // offset of this tile inside its chunk
  const int q_off = q_off_wg + wave * 32;           // this wave's first row inside the chunk
  const int my_q = q_off + l31;                     // this lane's row inside the chunk
  const bool q_live = my_q < q_rows_in_chunk;
  const int64_t q_local_row = (int64_t)qc * p.chunk_len + (q_live ? my_q : q_rows_in_chunk - 1);
  const int q_last_wg = min(q_off_wg + QTILE, q_rows_in_chunk) - 1;  // last valid row of the WG
  const float scale_log2e = p.scale_log2e;
  // packed sequences (block-diagonal causal, single chunk): a query only sees keys >= the first row of its segment.
  // seg_start is non-decreasing, so the workgroup starts at the tile of its first row's segment and only the tiles
  // below its last row's segment start need the extra element mask.
  const int my_start = p.seg_start ? p.seg_start[q_local_row] : 0;
  const int wg_first_start = p.seg_start ? p.seg_start[(int64_t)qc * p.chunk_len + q_off_wg] : 0;
  const int wg_last_start = p.seg_start ? p.seg_start[(int64_t)qc * p.chunk_len + q_last_wg] : 0;

  // ---- Q fragments (B operand of S^T = K Q^T): lane = (query row l31, k-slot half hi) --------
  bf16x8 qf[DS];
  {
    const bf16_t* qp = p.q + (int64_t)b * p.q_bs + q_local_row * p.q_rs + (int64_t)kvh * p.q_gs + (int64_t)hq * p.q_hs + hi * 8;
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

  const bf16_t* kbase = p.k + (int64_t)b * p.k_bs + (int64_t)kvh * p.k_hs;
  const bf16_t* vbase = p.v + (int64_t)b * p.v_bs + (int64_t)kvh * p.v_hs;

  // ---- tile iterator ------------------------------------------------------------------------------
  auto enter_chunk = [&](TileIt& t) __attribute__((always_inline)) {   // skip chunks with nothing to visit
    while (t.c < p.n_kv_chunks) {
      t.rows = (t.c == p.n_kv_chunks - 1) ? p.kv_valid : p.chunk_len;
      const int all = (t.rows + KVT - 1) / KVT;
      const int gk = p.kv_gid[t.c];
      t.diag = CAUSAL && gk == gq;
      t.n = (!CAUSAL || gk < gq) ? all : (gk > gq ? 0 : min(all, q_last_wg / KVT + 1));
      if (t.n > 0) { t.crow = p.kv_row[t.c]; t.j = wg_first_start / KVT; return; }
      ++t.c;
    }
  };
  auto advance = [&](TileIt& t) __attribute__((always_inline)) {
    if (++t.j == t.n) { ++t.c; enter_chunk(t); }
  };

  fwd8::DmaLane<D> dma;
  fwd8::dma_lane_init<D>(dma, wave, lane, p.k_rs, p.v_rs);
  auto dma_tile = [&](const TileIt& t, unsigned sl) __attribute__((always_inline)) {
    const int64_t row0 = t.crow + (int64_t)t.j * KVT;
    // wave-uniform bases + 32-bit lane offsets; valid rows in this tile = t.rows - t.j * KVT (>= 1)
    fwd8::dma_tile<D>(dma, wave, kbase + row0 * p.k_rs, vbase + row0 * p.v_rs, p.k_rs, p.v_rs, t.rows - t.j * KVT, sl);
  };

  // ---- this kernel's element mask of one tile: diagonal, ragged end of the chunk, packed segment start ----------------------------
  f32x16 s0, s1;
  auto mask_tile = [&](int kv_off, bool diag, int kv_rows) __attribute__((always_inline)) {
    const bool need_mask = (diag && kv_off + KVT - 1 > q_off) || (kv_off + KVT > kv_rows) || (kv_off < wg_last_start);
    if (need_mask) {
      const int lim_c = diag ? (my_q - kv_off) : 0x7fffffff;        // key <= lim_c visible
      const int lim = min(lim_c, kv_rows - kv_off - 1);              // key <= .. valid
      const int lo = my_start - kv_off;                              // key >= lo: same packed segment
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int key = (r & 3) + 8 * (r >> 2) + 4 * hi;
        if (key > lim || key < lo) s0[r] = -INFINITY;
        if (key + 32 > lim || key + 32 < lo) s1[r] = -INFINITY;
      }
    }
  };

  // ---- prologue: tile 0 -> LDS slot 0 ---------------------------------------------------------------
  TileIt cur;
  cur.c = 0; cur.j = 0; cur.n = 0; cur.rows = 0; cur.diag = 0; cur.crow = 0;
  enter_chunk(cur);
  TileIt nx1 = cur;                                   // tile t+1
  if (cur.c < p.n_kv_chunks) {
    dma_tile(cur, lds0);
    advance(nx1);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  int slot = 0;
  while (cur.c < p.n_kv_chunks) {
    const bool has_n1 = nx1.c < p.n_kv_chunks;
    TileIt nx2 = nx1;
    // tile t+1 -> the other LDS slot (every wave finished reading it before the last barrier)
    if (has_n1) {
      dma_tile(nx1, lds0 + (slot ^ 1) * SLOTB);        // lands under this tile's MFMA work
      advance(nx2);
    }
    const unsigned sl = lds0 + slot * SLOTB;
    const int kv_off = cur.j * KVT;                  // tile offset inside its chunk
    // wave-uniform skip: the whole tile lies after this wave's last query row
    const bool skip = cur.diag && kv_off > q_off + 31;
    if (!skip) {
      fwd8::qk_phase<D>(sl, koff, qf, s0, s1);
      mask_tile(kv_off, cur.diag, cur.rows);
      fwd8::softmax_step<D>(fwd8::tile_row_max(s0, s1) * scale_log2e, scale_log2e, s0, s1, m_run, l_run, o_acc);
      fwd8::pv_phase<D, 1>(sl, voff, s0, s1, o_acc);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's DMA pieces have landed
    __syncthreads();
    slot ^= 1;
    cur = nx1;
    nx1 = nx2;
  }

  // ---- epilogue ----------------------------------------------------------------------------------
  const float l_tot = swap32_sum(l_run);
  const float inv = l_tot > 0.f ? 1.0f / l_tot : 0.f;
  if (q_live) {
    const int64_t orow = (int64_t)qc * p.chunk_len + my_q;
    fwd8::store_row_bf16<D>(p.o + (int64_t)b * p.o_bs + orow * p.o_rs + (int64_t)kvh * p.o_gs + (int64_t)hq * p.o_hs, o_acc, inv, hi);
    if (p.lse && hi == 0) p.lse[((int64_t)b * p.n_q_heads + head) * p.n_q_rows + orow] = fwd8::lse_natural(m_run, l_tot);
  }
}

template <int D, bool CAUSAL>
int launch_attn(const AttnArgs& a, int64_t nblocks, hipStream_t st) {
  constexpr int lds = fwd8::Tile<D>::LDS_BYTES;
  static std::atomic<unsigned long long> attr_set{0};
  vita_device_once(attr_set, [&] {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&flash_fwd_kernel<D, CAUSAL>), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
  });
  hipLaunchKernelGGL((flash_fwd_kernel<D, CAUSAL>), dim3((unsigned)nblocks), dim3(512), lds, st, a);
  return vita_check_launch();
}

}  // namespace

// ---- merge of two attention partials over disjoint key sets (context parallelism: own chunks first, remote chunks after the gather)
//   lse = log(exp(lse_a) + exp(lse_b)),  O = O_a exp(lse_a - lse) + O_b exp(lse_b - lse);  a part that saw no key has lse = -inf.
// HBM-bound: one thread per (row, head, 16-byte piece of d = 128); O_a / lse_a are updated in place.
namespace {
__global__ __launch_bounds__(256) void attn_merge_kernel(bf16_t* __restrict__ oa, int64_t oa_rs, int64_t oa_hs, float* __restrict__ lse_a,
                                                         const bf16_t* __restrict__ ob, int64_t ob_rs, int64_t ob_hs,
                                                         const float* __restrict__ lse_b, int64_t rows, int heads) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int piece = (int)(idx & 15);
  const int64_t rh = idx >> 4;
  if (rh >= rows * heads) return;
  const int64_t row = rh / heads;
  const int h = (int)(rh % heads);
  const float la = lse_a[(int64_t)h * rows + row], lb = lse_b[(int64_t)h * rows + row];
  const float mx = fmaxf(la, lb);
  float wa = 1.f, wb = 0.f, l = la;
  if (mx > -INFINITY) {
    const float ea = __expf(la - mx), eb = __expf(lb - mx);
    const float inv = 1.0f / (ea + eb);
    wa = ea * inv; wb = eb * inv;
    l = mx + __logf(ea + eb);
  }
  u32x4* pa = reinterpret_cast<u32x4*>(oa + row * oa_rs + (int64_t)h * oa_hs + piece * 8);
  const u32x4 a = *pa, bq = *reinterpret_cast<const u32x4*>(ob + row * ob_rs + (int64_t)h * ob_hs + piece * 8);
  u32x4 r;
#pragma unroll
  for (int j = 0; j < 4; ++j)
    r[j] = pack_bf16x2(bf16lo_to_f32(a[j]) * wa + bf16lo_to_f32(bq[j]) * wb, bf16hi_to_f32(a[j]) * wa + bf16hi_to_f32(bq[j]) * wb);
  *pa = r;
  if (piece == 0) lse_a[(int64_t)h * rows + row] = l;
}
}  // namespace

extern "C" int vita_attn_merge(void* o_a, int64_t oa_row_stride, int64_t oa_head_stride, float* lse_a, const void* o_b,
                               int64_t ob_row_stride, int64_t ob_head_stride, const float* lse_b, int64_t rows, int heads,
                               int head_dim, void* stream) {
  if (!o_a || !o_b || !lse_a || !lse_b || rows < 0 || heads <= 0) return VITA_ERR_INVALID_ARG;
  if (head_dim != 128) return VITA_ERR_UNSUPPORTED;
  if ((oa_row_stride & 7) || (oa_head_stride & 7) || (ob_row_stride & 7) || (ob_head_stride & 7)) return VITA_ERR_UNSUPPORTED;
  if (rows == 0) return VITA_OK;
  const int64_t n = rows * heads * 16;
  hipLaunchKernelGGL(attn_merge_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (bf16_t*)o_a, oa_row_stride,
                     oa_head_stride, lse_a, (const bf16_t*)o_b, ob_row_stride, ob_head_stride, lse_b, rows, heads);
  return vita_check_launch();
}

// win_tiles == nullptr: the full launch.  Otherwise n_win distinct 256-row query tiles of a plain causal single-chunk geometry: the grid
// holds those tiles' workgroups only, each decoding to the workgroup the full launch runs for its tile (AttnArgs::win_qt)
static int flash_attn_fwd_impl(const vita_attn_params* p, const int32_t* win_tiles, int n_win, void* stream) {
  if (!p || !p->q || !p->k || !p->v || !p->o) return VITA_ERR_INVALID_ARG;
  if (p->batch <= 0 || p->n_q_heads <= 0 || p->n_kv_heads <= 0 || p->chunk_len <= 0 ||
      p->n_q_chunks <= 0 || p->n_kv_chunks <= 0 || !p->q_chunk_gid || !p->kv_chunk_gid ||
      !p->kv_chunk_row)
    return VITA_ERR_INVALID_ARG;
  if (p->head_dim != 64 && p->head_dim != 96 && p->head_dim != 128) return VITA_ERR_UNSUPPORTED;
  if (p->n_q_heads % p->n_kv_heads) return VITA_ERR_INVALID_ARG;
  if (p->n_q_chunks > kMaxChunks || p->n_kv_chunks > kMaxChunks) return VITA_ERR_UNSUPPORTED;
  if (p->chunk_len > 0x7fffff00LL) return VITA_ERR_UNSUPPORTED;
  if (p->q_valid <= 0 || p->q_valid > p->chunk_len || p->kv_valid <= 0 || p->kv_valid > p->chunk_len)
    return VITA_ERR_INVALID_ARG;
  // partial chunks only for single-chunk geometry; multi-chunk needs whole 64-key tiles
  if (p->n_q_chunks > 1 && p->q_valid != p->chunk_len) return VITA_ERR_UNSUPPORTED;
  if (p->n_kv_chunks > 1 && (p->kv_valid != p->chunk_len || p->chunk_len % KVT)) return VITA_ERR_UNSUPPORTED;
  const int64_t strides[] = {p->q_batch_stride, p->q_row_stride, p->q_head_stride, p->k_batch_stride,
                             p->k_row_stride, p->k_head_stride, p->v_batch_stride, p->v_row_stride,
                             p->v_head_stride, p->q_group_stride};
  for (int64_t s : strides)
    if (s & 7) return VITA_ERR_UNSUPPORTED;          // 16-byte vector loads
  if ((p->o_batch_stride & 3) || (p->o_row_stride & 3) || (p->o_head_stride & 3) || (p->o_group_stride & 3)) return VITA_ERR_UNSUPPORTED;
  // every kernel reads q 16 bytes at a time (bf16x8 loads) and k / v in 16-byte LDS-DMA pieces, stores lse and reads the segment table as
  // 4-byte words; the general kernel stores o 8 bytes at a time (the 64-row kernels 16: their _eligible() hands an output that is only
  // 8-byte aligned to the general one).  Refused here, before anything is launched.
  if (((uintptr_t)p->q | (uintptr_t)p->k | (uintptr_t)p->v) & 15) return VITA_ERR_UNSUPPORTED;
  if ((uintptr_t)p->o & 7) return VITA_ERR_UNSUPPORTED;
  if (((uintptr_t)p->lse | (uintptr_t)p->q_seg_start) & 3) return VITA_ERR_UNSUPPORTED;

  AttnArgs a;
  a.q = (const bf16_t*)p->q; a.q_bs = p->q_batch_stride; a.q_rs = p->q_row_stride; a.q_hs = p->q_head_stride;
  a.q_gs = vita_group_stride(p->q_group_stride, p->q_head_stride, p->n_q_heads / p->n_kv_heads);
  a.k = (const bf16_t*)p->k; a.k_bs = p->k_batch_stride; a.k_rs = p->k_row_stride; a.k_hs = p->k_head_stride;
  a.v = (const bf16_t*)p->v; a.v_bs = p->v_batch_stride; a.v_rs = p->v_row_stride; a.v_hs = p->v_head_stride;
  a.o = (bf16_t*)p->o; a.o_bs = p->o_batch_stride; a.o_rs = p->o_row_stride; a.o_hs = p->o_head_stride;
  a.o_gs = vita_group_stride(p->o_group_stride, p->o_head_stride, p->n_q_heads / p->n_kv_heads);
  a.lse = p->lse;
  a.batch = p->batch; a.n_q_heads = p->n_q_heads; a.n_kv_heads = p->n_kv_heads;
  a.chunk_len = (int)p->chunk_len; a.q_valid = (int)p->q_valid; a.kv_valid = (int)p->kv_valid;
  a.n_q_chunks = p->n_q_chunks; a.n_kv_chunks = p->n_kv_chunks;
  a.tiles_per_q_chunk = (int)((p->chunk_len + QTILE - 1) / QTILE);
  a.n_q_rows = (int)((int64_t)(p->n_q_chunks - 1) * p->chunk_len + p->q_valid);
  a.scale_log2e = p->softmax_scale * LOG2E;
  a.seg_start = p->q_seg_start;
  if (p->q_seg_start && (p->n_q_chunks != 1 || p->n_kv_chunks != 1 || !p->causal || p->batch != 1)) return VITA_ERR_UNSUPPORTED;
  vita_copy_chunk_tables(a, p);
  for (int i = 0; i < p->n_q_chunks; ++i) a.q_order[i] = i;
  // heaviest (largest global chunk id) first
  for (int i = 1; i < p->n_q_chunks; ++i)
    for (int j = i; j > 0 && a.q_gid[a.q_order[j]] > a.q_gid[a.q_order[j - 1]]; --j) {
      const int t = a.q_order[j]; a.q_order[j] = a.q_order[j - 1]; a.q_order[j - 1] = t;
    }
  int64_t nblocks = (int64_t)p->batch * p->n_q_heads * p->n_q_chunks * a.tiles_per_q_chunk;
  if (nblocks > 0x7fffffff) return VITA_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  a.win_n = 0;
  if (win_tiles) {
    if (n_win <= 0) return VITA_ERR_INVALID_ARG;
    if (!p->causal || p->n_q_chunks != 1 || p->n_kv_chunks != 1 || p->head_dim != 128 || n_win > kMaxWindowTiles) return VITA_ERR_UNSUPPORTED;
    // heaviest (last) tile first, as the full launch orders them; position of tile t in that order = tiles - 1 - t
    for (int i = 0; i < n_win; ++i) {
      const int t = win_tiles[i];
      if (t < 0 || t >= a.tiles_per_q_chunk) return VITA_ERR_INVALID_ARG;
      int j = i;
      for (; j > 0 && a.win_qt[j - 1] > a.tiles_per_q_chunk - 1 - t; --j) a.win_qt[j] = a.win_qt[j - 1];
      a.win_qt[j] = a.tiles_per_q_chunk - 1 - t;
    }
    for (int i = 1; i < n_win; ++i)
      if (a.win_qt[i] == a.win_qt[i - 1]) return VITA_ERR_INVALID_ARG;          // a tile listed twice
    a.win_n = n_win;
    nblocks = (int64_t)p->batch * p->n_q_heads * n_win;
    // the kernel the full launch picks for this geometry, or none
    if (vita_attn64_eligible(a, p->head_dim, true)) return vita_attn64_launch(a, nblocks, st);
    return launch_attn<128, true>(a, nblocks, st);
  }
  // d = 128 causal with whole 256-row / 64-key tiles: the 4 x 64-row in-wave-pipelined kernel (attn64.hip)
  if (vita_attn64_eligible(a, p->head_dim, p->causal != 0)) return vita_attn64_launch(a, nblocks, st);
  // d = 64 non-causal (the vision towers): the same structure at head size 64, ragged rows / keys (attn64v.hip)
  if (vita_attn64v_eligible(a, p->head_dim, p->causal != 0)) return vita_attn64v_launch(a, st);
  if (p->head_dim == 128) return p->causal ? launch_attn<128, true>(a, nblocks, st) : launch_attn<128, false>(a, nblocks, st);
  if (p->head_dim == 96) return p->causal ? launch_attn<96, true>(a, nblocks, st) : launch_attn<96, false>(a, nblocks, st);
  return p->causal ? launch_attn<64, true>(a, nblocks, st) : launch_attn<64, false>(a, nblocks, st);
}

extern "C" int vita_flash_attn_fwd(const vita_attn_params* p, void* stream) { return flash_attn_fwd_impl(p, nullptr, 0, stream); }

extern "C" int vita_flash_attn_fwd_window(const vita_attn_params* p, const int32_t* q_tiles, int n_q_tiles, void* stream) {
  if (!q_tiles) return VITA_ERR_INVALID_ARG;
  return flash_attn_fwd_impl(p, q_tiles, n_q_tiles, stream);
}
