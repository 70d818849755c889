// The tile body of the 8-wave x 32-row forward attention kernels, written once: flash_fwd_kernel (attn.hip) and flash_extend_kernel
// (attn_extend.hip) include it, nobody else.  One workgroup = 8 waves = 256 query rows; a K|V ring slot holds 64 keys.
//   * K and V tiles go HBM/L2 -> LDS with the LDS-DMA (global_load_lds_dwordx4).  The DMA writes lane-linear, so attn_tile.h's bank
//     swizzles are applied to the per-lane SOURCE address (the same involution as on the fragment reads): no staging VGPRs.
//   * S^T = K Q^T (v_mfma_f32_32x32x16_bf16): a lane owns ONE query row (lane & 31) and 32 of the 64 keys, so row max and row sum
//     are in-lane reductions plus one v_permlane32_swap.  Accumulator register r of s0 is key (r & 3) + 8 (r >> 2) + 4 hi, s1 32 more.
//   * O^T = V^T P^T: the P^T operand is the packed S^T accumulator (any consistent assignment of keys to MFMA k-slots is valid, the
//     contraction is a sum), the V^T operand comes from the row-major V tile through ds_read_b64_tr_b16.
// What a kernel keeps: its work decomposition, its tile walk, its element mask, what it does to the tile maximum, its fp32 epilogue.
// Every helper takes the kernel's named locals by reference and is inlined: nothing here says which kernel calls it.
#pragma once
#include "attn_tile.h"

namespace fwd8 {

constexpr int QTILE = 256;   // query rows per workgroup (8 waves x 32)
constexpr int KVT = 64;      // keys per tile
constexpr int QK_AHEAD = 3;  // K-fragment reads pinned that many k-steps ahead of their MFMAs

template <int D>
struct Tile {
  static constexpr int DS = D / 16;              // QK^T k-steps
  static constexpr int DB = D / 32;              // O^T row blocks
  static constexpr int ROWB = D * 2;             // bytes per K/V row
  static constexpr int TILEB = KVT * ROWB;       // bytes per K (or V) tile
  static constexpr int SLOTB = 2 * TILEB;        // bytes per ring slot (K tile | V tile)
  static constexpr int SLOTS = ROWB / 16;        // 16-byte slots per row
  static constexpr int LDS_BYTES = 2 * SLOTB;    // the two-slot ring (dynamic LDS of a launch)
  // LDS-DMA: wave w issues pieces q = 0 .. PIECES - 1 of K and of V; piece (w, q) = rows (w PIECES + q) RPP .. of the tile (1 KiB),
  // lane i lands at byte 16 i of the piece.  d = 96: a piece is 5 1/3 rows and an operand 12 pieces; the 24 pieces of a slot are
  // dealt three per wave (waves 0 .. 3 K, 4 .. 7 V) and lane i of piece x fills the 16-byte unit u = 64 x + i = (row u / 12,
  // physical slot u % 12).
  static constexpr bool D96 = D == 96;
  static constexpr int PIECES = D96 ? 3 : TILEB / 1024 / 8;   // wave-instructions per operand per wave (d = 96: of ITS operand)
  static constexpr int RPP = 1024 / ROWB;                     // tile rows per 1-KiB piece (d = 96: unused)
};

// ---- per-lane LDS read offsets (everything else is a compile-time immediate) -----------------------------------------------------------
// K fragment (A operand): row l31 (+32), 16-byte slot 2 ds + hi.  V^T fragment of O^T row block db: attn_tile.h's transposed-read lane map
template <int D>
__device__ __forceinline__ void frag_offsets(int lane, unsigned (&koff)[D / 16], unsigned (&voff)[D / 32]) {
  const int hi = lane >> 5, l31 = lane & 31;
#pragma unroll
  for (int ds = 0; ds < D / 16; ++ds) koff[ds] = frag_off<D>(l31, 2 * ds + hi);
  const int key_l = tr_lane_row(lane);
#pragma unroll
  for (int db = 0; db < D / 32; ++db) {
    const int col = tr_lane_col(lane, db);
    voff[db] = Tile<D>::TILEB + tr_off<D>(key_l, col >> 4, (col & 15) * 2);
  }
}

// ---- LDS-DMA of one 64-key K|V slot ----------------------------------------------------------------------------------------------------
// This lane's pieces: the tile row it fills, the LOGICAL slot whose data must land at its physical slot (inverse of the read swizzles),
// and both as 32-bit source offsets (elements) from the tile's first row.
template <int D>
struct DmaLane {
  unsigned dk_off[Tile<D>::PIECES], dv_off[Tile<D>::PIECES];
  int d_row[Tile<D>::PIECES], d_ks[Tile<D>::PIECES], d_vs[Tile<D>::PIECES];
};
template <int D>
__device__ __forceinline__ void dma_lane_init(DmaLane<D>& m, const int& wave, int lane, const int64_t& k_rs, const int64_t& v_rs) {
  using T = Tile<D>;
#pragma unroll
  for (int q = 0; q < T::PIECES; ++q) {
    const int unit = (T::D96 ? (wave & 3) * T::PIECES + q : 0) * 64 + lane;
    const int row = T::D96 ? unit / T::SLOTS : (wave * T::PIECES + q) * T::RPP + lane / T::SLOTS;   // tile row this lane fills
    const int ps = T::D96 ? unit % T::SLOTS : lane % T::SLOTS;                                     // physical 16-byte slot in the row
    m.d_ks[q] = frag_slot_inv<D>(row, ps);
    m.d_vs[q] = tr_slot_inv<D>(row, ps);
    m.d_row[q] = row;
    m.dk_off[q] = (unsigned)(row * k_rs + m.d_ks[q] * 8);
    m.dv_off[q] = (unsigned)(row * v_rs + m.d_vs[q] * 8);
  }
}
// Issue one tile: kp / vp = its first K / V row (wave-uniform), left = valid rows behind them (>= 1), sl = LDS address of the slot.
// Rows past `left` are clamped to left - 1: nothing behind the last valid row is read, the element mask hides the copies.
template <int D>
__device__ __forceinline__ void dma_tile(const DmaLane<D>& m, const int& wave, const bf16_t* kp, const bf16_t* vp, const int64_t& k_rs,
                                         const int64_t& v_rs, const int left, unsigned sl) {
  using T = Tile<D>;
  if constexpr (T::D96) {                              // this wave's three pieces of ITS operand
    const bool v_wave = wave >= 4;
    const bf16_t* xp = v_wave ? vp : kp;
    const int64_t rs = v_wave ? v_rs : k_rs;
    const unsigned dst = sl + (v_wave ? T::TILEB : 0) + (wave & 3) * T::PIECES * 1024;
#pragma unroll
    for (int q = 0; q < T::PIECES; ++q) {
      const int row = m.d_row[q] < left ? m.d_row[q] : left - 1;
      __builtin_amdgcn_global_load_lds((gvoid*)(xp + (int64_t)row * rs + (v_wave ? m.d_vs[q] : m.d_ks[q]) * 8),
                                       (lvoid*)(uintptr_t)(dst + q * 1024), 16, 0, 0);
    }
  } else if (left >= KVT) {
#pragma unroll
    for (int q = 0; q < T::PIECES; ++q) {
      const int piece = wave * T::PIECES + q;
      __builtin_amdgcn_global_load_lds((gvoid*)(kp + m.dk_off[q]), (lvoid*)(uintptr_t)(sl + piece * 1024), 16, 0, 0);
      __builtin_amdgcn_global_load_lds((gvoid*)(vp + m.dv_off[q]), (lvoid*)(uintptr_t)(sl + T::TILEB + piece * 1024), 16, 0, 0);
    }
  } else {                                             // padded tail
#pragma unroll
    for (int q = 0; q < T::PIECES; ++q) {
      const int piece = wave * T::PIECES + q;
      const int row = m.d_row[q] < left ? m.d_row[q] : left - 1;
      __builtin_amdgcn_global_load_lds((gvoid*)(kp + (int64_t)row * k_rs + m.d_ks[q] * 8),
                                       (lvoid*)(uintptr_t)(sl + piece * 1024), 16, 0, 0);
      __builtin_amdgcn_global_load_lds((gvoid*)(vp + (int64_t)row * v_rs + m.d_vs[q] * 8),
                                       (lvoid*)(uintptr_t)(sl + T::TILEB + piece * 1024), 16, 0, 0);
    }
  }
}

// ---- S^T = K Q^T of the slot at LDS address sl: 2 x DS MFMAs into s0 (keys 0 .. 31) / s1 (keys 32 .. 63) -------------------------------
template <int D>
__device__ __forceinline__ void qk_phase(unsigned sl, const unsigned (&koff)[D / 16], const bf16x8 (&qf)[D / 16], f32x16& s0, f32x16& s1) {
  constexpr int DS = Tile<D>::DS;
#pragma unroll
  for (int r = 0; r < 16; ++r) { s0[r] = 0.f; s1[r] = 0.f; }
  bf16x8 ka[DS], kb[DS];
#pragma unroll
  for (int ds = 0; ds < DS; ++ds) {
    const unsigned a = sl + koff[ds];
    ka[ds] = *(lds_bf16x8*)(uintptr_t)(a);
    kb[ds] = *(lds_bf16x8*)(uintptr_t)(a + 32 * Tile<D>::ROWB);
  }
#pragma unroll
  for (int ds = 0; ds < DS; ++ds) {
    s0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ka[ds], qf[ds], s0, 0, 0, 0);
    s1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kb[ds], qf[ds], s1, 0, 0, 0);
  }
  // pin the issue order: K fragments run QK_AHEAD k-steps ahead of the MFMAs that consume them
  __builtin_amdgcn_sched_group_barrier(0x100, 2 * QK_AHEAD, 0);
#pragma unroll
  for (int ds = 0; ds < DS; ++ds) {
    __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
    if (ds + QK_AHEAD < DS) __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
  }
}

// ---- online softmax, log2 domain ------------------------------------------------------------------------------------------------------
// the row's largest (masked, unscaled) score of the tile
__device__ __forceinline__ float tile_row_max(const f32x16& s0, const f32x16& s1) {
  float mx = fmaxf(s0[0], s1[0]);
#pragma unroll
  for (int r = 1; r < 16; ++r) mx = fmaxf(fmaxf(s0[r], s1[r]), mx);
  return swap32_max(mx);
}
// m_tile = the tile's maximum, already scaled (and whatever else the caller did to it): new running max, the exponentials in place of
// the scores, the rescale of l_run and o_acc (skipped when no lane of the wave moved its max)
template <int D>
__device__ __forceinline__ void softmax_step(const float m_tile, const float& scale_log2e, f32x16& s0, f32x16& s1, float& m_run, float& l_run,
                                             f32x16 (&o_acc)[D / 32]) {
  const float m_new = fmaxf(m_run, m_tile);
  const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
  m_run = m_new;
  float psum = 0.f;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    s0[r] = __builtin_amdgcn_exp2f(fmaf(s0[r], scale_log2e, -m_new));
    s1[r] = __builtin_amdgcn_exp2f(fmaf(s1[r], scale_log2e, -m_new));
    psum += s0[r] + s1[r];
  }
  l_run = l_run * alpha + psum;
  if (!__all(alpha == 1.0f)) {
#pragma unroll
    for (int i = 0; i < D / 32; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) o_acc[i][r] *= alpha;
  }
}

// ---- O^T += V^T P^T -----------------------------------------------------------------------------------------------------------------------
// P^T operand: step t uses registers 8 (t & 1) .. of block t >> 1 (the V^T fragment uses the same key <-> k-slot assignment).
// P_TERMS = 2: the probabilities enter as TWO bf16 terms, p = hi + lo (lo = bf16(p - hi)), so the product carries ~16 bits of p
// instead of 8; one V^T fragment read serves both terms.
template <int D, int P_TERMS>
__device__ __forceinline__ void pv_phase(unsigned sl, const unsigned (&voff)[D / 32], const f32x16& s0, const f32x16& s1,
                                         f32x16 (&o_acc)[D / 32]) {
  static_assert(P_TERMS == 1 || P_TERMS == 2, "one or two bf16 terms of P");
  constexpr int DB = Tile<D>::DB, ROWB = Tile<D>::ROWB;
  bf16x8 pf[4];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    pf[0][j] = (__bf16)s0[j];
    pf[1][j] = (__bf16)s0[8 + j];
    pf[2][j] = (__bf16)s1[j];
    pf[3][j] = (__bf16)s1[8 + j];
  }
  bf16x8 pl[4];
  if (P_TERMS == 2) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      pl[0][j] = (__bf16)(s0[j] - (float)pf[0][j]);
      pl[1][j] = (__bf16)(s0[8 + j] - (float)pf[1][j]);
      pl[2][j] = (__bf16)(s1[j] - (float)pf[2][j]);
      pl[3][j] = (__bf16)(s1[8 + j] - (float)pf[3][j]);
    }
  }
  unsigned va[DB];
#pragma unroll
  for (int db = 0; db < DB; ++db) va[db] = sl + voff[db];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
#pragma unroll
    for (int db = 0; db < DB; ++db) {
      const unsigned vp = va[db] + 16 * t * ROWB;
      const s16x4 a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(uintptr_t)(vp));
      const s16x4 c = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(uintptr_t)(vp + 8 * ROWB));
      typedef __attribute__((ext_vector_type(8))) short s16x8;
      const s16x8 ac = __builtin_shufflevector(a, c, 0, 1, 2, 3, 4, 5, 6, 7);
      o_acc[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, ac), pf[t], o_acc[db], 0, 0, 0);
      if (P_TERMS == 2) o_acc[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, ac), pl[t], o_acc[db], 0, 0, 0);
    }
  }
}

// ---- epilogue: the lane's row of O as bf16 (op = the row's first column), and its natural-log lse --------------------------------------
template <int D>
__device__ __forceinline__ void store_row_bf16(bf16_t* op, const f32x16 (&o_acc)[D / 32], const float inv, int hi) {
#pragma unroll
  for (int db = 0; db < D / 32; ++db) {
#pragma unroll
    for (int rg = 0; rg < 4; ++rg) {
      const int d = 32 * db + 8 * rg + 4 * hi;
      u32x2 w = {pack_bf16x2(o_acc[db][rg * 4 + 0] * inv, o_acc[db][rg * 4 + 1] * inv),
                 pack_bf16x2(o_acc[db][rg * 4 + 2] * inv, o_acc[db][rg * 4 + 3] * inv)};
      *reinterpret_cast<u32x2*>(op + d) = w;
    }
  }
}
__device__ __forceinline__ float lse_natural(float m_run, float l_tot) {      // m_run in the log2 domain; a row that saw no key: -inf
  return l_tot > 0.f ? (m_run + log2f(l_tot)) * 0.69314718055994530942f : -INFINITY;
}

}  // namespace fwd8
