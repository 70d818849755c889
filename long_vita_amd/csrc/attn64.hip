// Flash attention forward, d = 128, causal, whole tiles: 4 waves x 64 query rows, one wave per SIMD (gfx950 / MI355X).
// The fast path of vita_flash_attn_fwd for the LLM prefill (plain causal and the zig-zag context-parallel chunk tables);
// attn.hip keeps every other geometry (d = 64 ViT, non-causal, ragged tails, packed samples).
//
// Why a second structure (tools/hwprobe/attn_ladder.hip, attn64.hip; profiles/r02_hwprobe_*): with 32 query rows per wave every
// K / V^T fragment read from LDS feeds ONE MFMA and two waves share a SIMD, where they hide only half of each other's VALU time;
// with 64 rows per wave a fragment feeds two MFMAs and the only way to overlap the softmax with the matrix pipe is inside one
// instruction stream — so this kernel is an in-wave software pipeline:
//   * one workgroup = 4 waves = 256 query rows of ONE query head; a wave owns 64 rows = two 32-row blocks qb; 64-key tiles
//   * register classes: O^T (2 x 4 x 16 = 128 registers) lives in AGPRs and is touched by MFMAs only (inline asm, "+a"); the
//     Q fragments (64) are pinned in AGPRs and read from there as MFMA B operands; S^T (two tiles in flight, 2 x 64) comes
//     from builtin MFMAs in VGPR form (this file is compiled with -mllvm -amdgpu-mfma-vgpr-form=1) so the softmax reads it
//     without accumulator moves; -fno-slp-vectorize keeps the fp32 softmax math out of v_pk_* (it shares the matrix datapath)
//   * phase 1: 32 MFMAs  S(t+1) = K(t+1) Q^T  ||  exp2 / row sum / bf16 pack of the last 8 - NF2 P fragments of tile t
//     phase 2: 32 MFMAs  O += V(t)^T P(t)^T   ||  the first NF2 P fragments of tile t+1
//     NF2 = 4: one exp half-unit behind every MFMA, two fma + two exp2 behind the even ones, two adds + one pack behind the odd
//     ones (phase 1 ends two slots early: make_deal1); sched_barrier(0) in front of and behind every MFMA keeps the order (left
//     alone, the scheduler hoists a slot's filler in front of its MFMA and two MFMAs issue back to back)
//   * the SEAMS between the phases hold a branch and nothing else (r26; before, stamped: 223 and 265 cycles per tile beyond the MFMA
//     slot, of about 2900, profiles/r26_attn_seams.txt): whatever a phase needs before its first MFMA is done inside the phase
//     before it.  The S phase reads the P V phase's first three V^T fragments in front of its MFMAs 29 and 31 and makes the
//     acceptance compare (and the mask flag of the tile being multiplied) in front of MFMA 31, into ONE scalar, so that one s_cmp
//     and one branch separate the last S MFMA from the first P V MFMA; the fragments stay live across the out-of-line path.  The
//     P V phase moves the tile walk on and builds the next trip's DMA descriptors in two of its sum-and-pack gaps, holds the tile's
//     barrier in front of its MFMA 29 and reads the next S phase's first three K fragments behind it: the loop's back edge is the
//     other seam.  The prologue and the peeled last trip keep the plain order.  Bit-identical to the kernel before (the arithmetic,
//     its order inside every half-unit and the order of the row-sum adds are untouched; tests/test_attn64_seams_gpu.py holds the
//     digests).  Same-box A / B, 7 rounds: 128K 134.50 -> 131.00 ms (- 2.6 %, parent's spread 0.12 ms), 32K 8.585 -> 8.320, 16K 2.173
//     -> 2.134 (profiles/r26_attn_seams_ab.txt; what each step gave alone, and that the barrier and the walk pay only next to the
//     closed S -> P V seam: HISTORY §4.1)
//   * OPTIMISTIC running maximum (r12) on top of the LAZY one (r02: the maximum, and with it O and l, only moves when some row of
//     the wave exceeds it by more than 2^THR, THR = 8, so P <= 2^8 instead of <= 1 — bf16 / fp32 have the range, the relative
//     rounding of P is unchanged — and the 400-instruction accumulator rescale leaves the steady state).  Tile 0 gets its true row
//     maxima in the prologue; from then on the steady state takes NO maxima: a tile is exponentiated against the running maximum
//     as it stands, and ONE compare per row block and tile, on the row sum that is computed anyway, accepts it: l_tile <= 2^THR
//     proves every p <= 2^THR, which is all the lazy rule asks.  Only a tile that fails takes its true maxima, out of line, and
//     applies the lazy rule to them; if the maxima move, l and the accumulators are rescaled and the tile is exponentiated again.
//     The maxima move exactly when and where they did with 32 max3 steps, two swaps and a decision on every tile: the results
//     are bit-identical to that kernel's.  Same-box A / B against it: 128K 145.7 -> 135.0 ms, 32K 9.24 -> 8.71, 16K 2.40 -> 2.25
//     (profiles/r12_attn_optimistic_ab.txt)
//   * K / V tiles HBM/L2 -> LDS by LDS-DMA (buffer_load ... lds: SGPR descriptor re-based per tile + the lane's 32-bit offset,
//     no address VALU), separate K and V rings of two 16 KiB slots, one barrier per tile (inside the P V phase); attn_tile.h's frag / tr layouts
//     (conflict-free ds_read_b128 / ds_read_b64_tr_b16), the swizzle applied to the DMA's per-lane SOURCE address
//   * masks: a tile of the diagonal chunk that reaches past the workgroup's first row is masked element-wise for every wave
//     (tiles wholly past a wave's rows come out as exp2(-inf) = 0: no per-wave control flow in the pipeline)
// Reference behaviour restated: M/core/transformer/dot_product_attention.py:186-289,374-390; zig-zag chunk ownership
// M/training/utils.py:329-341.
#include "attn_args.h"
#include <stdlib.h>

namespace {

constexpr int D = 128, KVT = 64, QTILE = 256, ROWB = D * 2, TILEB = KVT * ROWB;     // 16 KiB per K (or V) tile
constexpr int LDS_K = 0, LDS_V = 2 * TILEB;                                         // K ring [2] | V ring [2]
constexpr int NF2 = 4;                                                               // P fragments of tile t+1 done in phase 2
constexpr int THR = 8;                                                               // lazy running maximum, log2 units
constexpr float ACCEPT_MAX = (float)(1 << THR);                                      // a lane's row sum <= 2^THR: none of its p exceeds 2^THR

// ---- filler schedule: the 64 exp half-units of a tile dealt to the 2 x 32 MFMA slots -------------------------------------------------
// half 0: two fma + two exp2 (1 + 1 + 2 + 2), half 1: two row-sum adds + one bf16 pack (3).  Phase 2 (P V of tile t) carries half-units
// 0 .. 8 NF2 - 1 of tile t+1, dealt by cumulative issue cost (make_map: a unit goes to the slot its weight's midpoint falls in; with
// NF2 = 4 that is ONE half-unit per slot, half 0 behind the even MFMAs and half 1 behind the odd ones: no gap holds more than 24 cycles
// of VALU issue, and the gaps in front of the even MFMAs, with their LDS reads, hold 12).  Phase 1 (S of tile t+1) carries half-units
// 8 NF2 .. 63 of tile t and ENDS TWO SLOTS EARLY (make_deal1).
struct SlotMap { int first[33]; };
constexpr int half_w(int h) { return (h & 1) ? 3 : 6; }
constexpr SlotMap make_map(int h0, int n) {
  SlotMap m{};
  int tot = 0;
  for (int u = 0; u < n; ++u) tot += half_w(h0 + u);
  int acc = 0, u = 0;
  for (int s = 0; s < 32; ++s) {
    m.first[s] = u;
    while (u < n && (2 * acc + half_w(h0 + u)) * 32 <= 2 * tot * (s + 1)) { acc += half_w(h0 + u); ++u; }
  }
  m.first[32] = n;
  return m;
}
// Phase 1: half-units 32 .. 63, up to two per slot; w picks the pair of exp2 temporaries.  Slots 0 .. 21 and 28, 29 hold one, in order.
// Half-units 54 .. 57 and 58 .. 61 are dealt over three slots each as (exp2 pair A | exp2 pair B | sums and packs of A and B): 8 + 24,
// 8 + 24 and 8 + 2 x 12.5 cycles of issue, the doubled slots being 24 and 27, whose gaps carry neither a DMA piece nor a K read.  The
// tile's last row-sum add is behind MFMA 29, slots 30 and 31 are free: the acceptance compare is issued in front of MFMA 31.  The adds
// into l_tile keep the order of the half-units, so the sums are the ones a one-per-slot deal gives.
struct Deal { int n[32]; int h[32][2]; int w[32][2]; };
constexpr Deal make_deal1() {
  Deal d{};
  for (int s = 0; s < 22; ++s) { d.n[s] = 1; d.h[s][0] = 32 + s; }
  const int at[2] = {22, 25};
  for (int k = 0; k < 2; ++k) {
    const int s = at[k], u = 32 + s + k;                      // u even: the exp2 half of pair A
    d.n[s] = 1; d.h[s][0] = u;
    d.n[s + 1] = 1; d.h[s + 1][0] = u + 2; d.w[s + 1][0] = 1;
    d.n[s + 2] = 2; d.h[s + 2][0] = u + 1; d.h[s + 2][1] = u + 3; d.w[s + 2][1] = 1;
  }
  d.n[28] = 1; d.h[28][0] = 62;
  d.n[29] = 1; d.h[29][0] = 63;
  return d;
}

// One barrier per tile (rings of two slots).  (Rings of four slots, TWO tiles between barriers and the DMAs of tiles t+2 .. t+4 issued
// at the start of a pair, were measured in r03 and r06: no gain.)
// PACKED (r03): packed samples (p.seg_start: first key row of each query row's segment, non-decreasing; one chunk).  The workgroup
// starts at the (even) tile of its first row's segment, and a tile that begins before the segment of the wave's LAST row gets a
// second arithmetic mask (key >= seg_start[row]); rows whose segment starts later see such tiles as all-masked: P = 0, the running
// maximum stays at its initial -1e30; its first visible key then gives exp2(s + 1e30) = inf, the tile fails the acceptance and the
// rare path rescales the (zero) state by exp2(-1e30 - m) = 0.
template <bool PACKED>
__global__ __launch_bounds__(256, 1) void flash_fwd64_kernel(AttnArgs p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const unsigned lds0 = (unsigned)(uintptr_t)(lds_char*)smem;
  const int tid = threadIdx.x, lane = tid & 63, hi = lane >> 5, l31 = lane & 31;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

  // ---- work decomposition (decode_q_tile: kv head = block id % n_kv_heads = the XCD for 8 kv heads; heaviest query tiles first) ----
  const QTileId wg = decode_q_tile(p, blockIdx.x, p.tiles_per_q_chunk);
  const int kvh = wg.kvh, hq = wg.hq, head = wg.head, b = wg.b, qc = wg.qc, qti = wg.qti;
  const int gq = p.q_gid[qc];
  const int q_off_wg = qti * QTILE;                 // offset of this workgroup inside its chunk
  const int q_off = q_off_wg + wave * 64;           // this wave's first row inside the chunk
  const float scale_log2e = p.scale_log2e;
  // packed samples: first tile to visit, the per-lane segment starts of the wave's rows, and the largest of them (wave-uniform)
  int seg_j0 = 0, seg_lo[2] = {0, 0}, seg_lo_max = 0;
  if constexpr (PACKED) {
    const int* ss = p.seg_start + (int64_t)qc * p.chunk_len;
    seg_j0 = (ss[q_off_wg] / KVT) & ~1;                          // even: the pipeline consumes tiles in pairs
    seg_lo[0] = ss[q_off + l31]; seg_lo[1] = ss[q_off + 32 + l31];
    seg_lo_max = __builtin_amdgcn_readfirstlane(ss[q_off + 63]);
  }

  // ---- Q fragments (B operand of S^T = K Q^T): block qb, k-step ds: row q_off + 32 qb + l31, d = 16 ds + 8 hi .. + 7 ----------
  bf16x8 qf[2][8];
  {
    const bf16_t* qp = p.q + (int64_t)b * p.q_bs + ((int64_t)qc * p.chunk_len + q_off + l31) * p.q_rs + (int64_t)kvh * p.q_gs +
                       (int64_t)hq * p.q_hs + hi * 8;
#pragma unroll
    for (int qb = 0; qb < 2; ++qb)
#pragma unroll
      for (int ds = 0; ds < 8; ++ds) qf[qb][ds] = *reinterpret_cast<const bf16x8*>(qp + (int64_t)32 * qb * p.q_rs + ds * 16);
  }
#pragma unroll
  for (int qb = 0; qb < 2; ++qb)
#pragma unroll
    for (int ds = 0; ds < 8; ++ds) asm volatile("" : "+a"(qf[qb][ds]));      // live in AGPRs from here on

  // ---- LDS fragment offsets (attn_tile.h: K frag layout, V tr layout) ---------------------------------------------------------
  unsigned koff[8], voff[4];
#pragma unroll
  for (int ds = 0; ds < 8; ++ds) koff[ds] = frag_off<D>(l31, 2 * ds + hi);       // + 32 kb rows: immediate
  const int key_l = tr_lane_row(lane);
#pragma unroll
  for (int db = 0; db < 4; ++db) {
    const int col = tr_lane_col(lane, db);
    voff[db] = tr_off<D>(key_l, col >> 4, (col & 15) * 2);
  }
  // ---- LDS-DMA: wave w moves pieces 4w .. 4w+3 (1 KiB = 4 rows) of K and of V; swizzle on the SOURCE address ---------------
  unsigned dk_off[4], dv_off[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int row = (wave * 4 + q) * 4 + (lane >> 4), ps = lane & 15;
    const int ks = frag_slot_inv<D>(row, ps);
    const int vs = tr_slot_inv<D>(row, ps);
    dk_off[q] = (unsigned)((row * p.k_rs + ks * 8) * 2);     // bytes inside the tile (64 rows x row stride < 2^32)
    dv_off[q] = (unsigned)((row * p.v_rs + vs * 8) * 2);
  }
  const char* kbase = (const char*)(p.k + (int64_t)b * p.k_bs + (int64_t)kvh * p.k_hs);
  const char* vbase = (const char*)(p.v + (int64_t)b * p.v_bs + (int64_t)kvh * p.v_hs);
  // LDS address of this wave's first piece in K / V ring slot 0.  The descriptor is re-based on the tile's first row: no
  // 4 GiB limit on the K / V buffers, no address VALU.  `opaque` keeps the 16 piece addresses from being hoisted into 16 SGPRs.
  const unsigned lds_kw = lds0 + LDS_K + wave * 4096, lds_vw = lds0 + LDS_V + wave * 4096;
  // issued from inline asm (vita_lds_dma16, vita_common.h): through the builtin, hipcc put an `s_waitcnt vmcnt(0)` in front of the first
  // V^T read of every P.V phase — the next tile's DMA, issued one phase earlier, was waited for in the middle of the current tile
  auto dma_k = [&](const TileIt& t, int slot) __attribute__((always_inline)) {
    const vita_rsrc_t r = vita_make_rsrc_uniform(t.kp);
    unsigned base = lds_kw;
    asm volatile("" : "+s"(base));
#pragma unroll
    for (int q = 0; q < 4; ++q) vita_lds_dma16(r, dk_off[q], base + slot * TILEB + q * 1024);
  };
  auto dma_v = [&](const TileIt& t, int slot) __attribute__((always_inline)) {
    const vita_rsrc_t r = vita_make_rsrc_uniform(t.vp);
    unsigned base = lds_vw;
    asm volatile("" : "+s"(base));
#pragma unroll
    for (int q = 0; q < 4; ++q) vita_lds_dma16(r, dv_off[q], base + slot * TILEB + q * 1024);
  };

  // r05: ONE piece at a time, for the spread issue inside the S = K Q^T phase: an LDS-DMA instruction holds the
  // issuing wave for ~60 cycles (MI355X_MICROARCH.md), a 32 x 32 x 16 MFMA keeps the matrix pipe busy for 32 — eight of them in a burst at
  // the top of a tile, right behind the barrier, are ~480 cycles with nothing in the pipe; one behind every fourth MFMA hides half of each.
  // Same-box A / B: 128K 147.5 - 148.0 -> 144.8 - 145.9 ms (- 1.5 ... 1.8 %), 32K - 1.7 %, 16K - 3 % (the chip returns about half of a cycle
  // saving as time: it is power-limited).  Reading the P V phase's first two V^T fragments a phase early on top of it: no further gain.
  auto dma_piece = [&](const vita_rsrc_t& r, const unsigned* off, unsigned lds_w, int slot, int q) __attribute__((always_inline)) {
    unsigned base = lds_w;
    asm volatile("" : "+s"(base));
    vita_lds_dma16(r, off[q], base + slot * TILEB + q * 1024);
  };

  // ---- tile iterator (attn_tile.h) ----------------------------------------------------------------------------------------------
  const CausalTileWalk<PACKED, AttnArgs> walk(p, kbase, vbase, gq, q_off_wg, seg_j0);
  const int n_tiles = walk.count();                  // a multiple of 4 (chunk_len % 256 == 0); PACKED: even, >= 4: seg_start[row] <= row
  if (n_tiles == 0) {
    // a launch over REMOTE chunks only (context parallelism: the rank's own chunks are attended to before the gather lands,
    // dot_product_attention.forward_cp): these rows see none of them -> O = 0, lse = -inf, the merge ignores this part
    const u32x2 z = {0u, 0u};
#pragma unroll
    for (int qb = 0; qb < 2; ++qb) {
      const int64_t orow = (int64_t)qc * p.chunk_len + q_off + 32 * qb + l31;
      bf16_t* op = p.o + (int64_t)b * p.o_bs + orow * p.o_rs + (int64_t)kvh * p.o_gs + (int64_t)hq * p.o_hs;
#pragma unroll
      for (int i = 0; i < 16; ++i) *reinterpret_cast<u32x2*>(op + 8 * i + 4 * hi) = z;
      if (p.lse && hi == 0) p.lse[((int64_t)b * p.n_q_heads + head) * p.n_q_rows + orow] = -INFINITY;
    }
    return;
  }

  // ---- state ----------------------------------------------------------------------------------------------------------
  f32x16 o[2][4];                                    // O^T[qb][db]: d = 32 db + (r & 3) + 8 (r >> 2) + 4 hi, row 32 qb + l31 (AGPRs)
#pragma unroll
  for (int qb = 0; qb < 2; ++qb)
#pragma unroll
    for (int db = 0; db < 4; ++db)
#pragma unroll
      for (int r = 0; r < 16; ++r) o[qb][db][r] = 0.f;
#pragma unroll
  for (int qb = 0; qb < 2; ++qb)
#pragma unroll
    for (int db = 0; db < 4; ++db) asm volatile("" : "+a"(o[qb][db]));
  f32x16 sb[2][2][2];                                // S^T[parity][qb][kb]: key 32 kb + (r & 3) + 8 (r >> 2) + 4 hi
  unsigned pk[2][2][4][4];                           // packed P^T[parity][qb][frag f][4 dwords]; frag f = regs 8 (f & 1) .. of kb = f >> 1
  float m_run[2] = {-1.0e30f, -1.0e30f}, l_run[2] = {0.f, 0.f}, m_neg[2];
  // r04: the 32 probabilities a lane holds of a tile are summed into l_tile first and folded into l_run ONCE per tile.  Adding them one
  // by one stagnates on very long rows: beyond ~2 M visible keys l_run's ulp reaches the size of a single p (p ~ 2^-8 of the row
  // maximum, l_run ~ 5e4 -> ulp 4e-3), the small ones are rounded away and O / l comes out too large — 1.5e-2 at 13 M keys
  // (tools/bench_maxseq.py: one CP = 8 rank at S = 16.8 M); a tile's partial sum is 32 x larger than its terms
  float l_tile[2] = {0.f, 0.f};
  float ea[2] = {0.f, 0.f}, eb[2] = {0.f, 0.f};                      // two pairs of exp2 results (Deal)

  constexpr SlotMap MAP2 = make_map(0, 8 * NF2);
  constexpr Deal DEAL1 = make_deal1();
  static_assert(NF2 == 4, "make_deal1 deals half-units 32 .. 63");

  // exp half-units (64 per tile): h -> fragment g = h >> 3 (need order of P V: g = 2 f + qb), element pair pr = (h >> 1) & 3;
  // half 0: the two fma + exp2 of the pair, half 1: row sum, bf16 pack (an exp2 result is never consumed by the next instruction)
  auto exp_half = [&](int par, int h, int w = 0) __attribute__((always_inline)) {
    const int g = h >> 3, pr = (h >> 1) & 3, qb = g & 1, f = g >> 1, kb = f >> 1, r = 8 * (f & 1) + 2 * pr;
    if ((h & 1) == 0) {
      ea[w] = __builtin_amdgcn_exp2f(fmaf(sb[par][qb][kb][r], scale_log2e, m_neg[qb]));
      eb[w] = __builtin_amdgcn_exp2f(fmaf(sb[par][qb][kb][r + 1], scale_log2e, m_neg[qb]));
    } else {
      l_tile[qb] += ea[w];
      l_tile[qb] += eb[w];
      pk[par][qb][f][pr] = pack_bf16x2(ea[w], eb[w]);
      asm volatile("" :: "v"(pk[par][qb][f][pr]), "v"(l_tile[qb]));                            // computed HERE (no sinking past the phase)
    }
  };
  // true row maxima of S(par) (after the masks), log2 units.  Only the prologue (tile 0) and the slow path of `accept` come here.
  auto row_max = [&](int par, float* mx) __attribute__((always_inline)) {
#pragma unroll
    for (int qb = 0; qb < 2; ++qb) {
      float m = fmaxf(sb[par][qb][0][0], sb[par][qb][1][0]);
#pragma unroll
      for (int r = 1; r < 16; ++r) m = fmaxf(fmaxf(sb[par][qb][0][r], sb[par][qb][1][r]), m);
      mx[qb] = swap32_max(m) * scale_log2e;
    }
  };
  // the running maxima move up to mx; returns alpha = exp2(old - new) per row block
  auto raise_max = [&](const float* mx, float* alpha) __attribute__((always_inline)) {
#pragma unroll
    for (int qb = 0; qb < 2; ++qb) {
      const float m_new = fmaxf(m_run[qb], mx[qb]);
      alpha[qb] = __builtin_amdgcn_exp2f(m_run[qb] - m_new);
      m_run[qb] = m_new;
      m_neg[qb] = -m_new;
    }
  };
  auto k_frag = [&](unsigned kslot, int i) __attribute__((always_inline)) {        // i = 2 ds + kb
    return *(lds_bf16x8*)(uintptr_t)(kslot + koff[i >> 1] + (i & 1) * 32 * ROWB);
  };
  auto v_frag = [&](unsigned vslot, int i) __attribute__((always_inline)) {        // i = 4 t + db
    const unsigned va = vslot + voff[i & 3] + 16 * (i >> 2) * ROWB;
    const s16x4 a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(uintptr_t)(va));
    const s16x4 c = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(uintptr_t)(va + 8 * ROWB));
    typedef __attribute__((ext_vector_type(8))) short s16x8;
    const s16x8 ac = __builtin_shufflevector(a, c, 0, 1, 2, 3, 4, 5, 6, 7);
    return __builtin_bit_cast(bf16x8, ac);
  };
  // S(buffer `dst`) = K(kslot) Q^T: slot = 4 ds + 2 kb + qb; K fragment (kb, ds) read two fragments ahead (ring of four).
  // FILL (every S phase but the prologue's): the exp half-units 8 NF2 .. 63 of tile `par` go behind the MFMAs; the first three K
  // fragments are in kr_pre already; in front of MFMAs 29 and 31 the first three V^T fragments of tile `par` (in its V ring slot since the
  // barrier before) are read for the P V phase, and in front of MFMA 31 the phase decides what follows it (`slow`)
  vita_rsrc_t rk_next = vita_make_rsrc_uniform(kbase), rv_next = rk_next;     // descriptors of the tiles being fetched (spread issue)
  bool spread_k = false, spread_v = false;
  int spread_k_slot = 0, spread_v_slot = 0;
  bf16x8 kr_pre[3], vr_pre[3];                       // the next phase's first three fragments, read before the seam in front of it
  auto needs_mask = [&](const TileIt& t) __attribute__((always_inline)) { return t.diag && t.j * KVT + KVT - 1 > q_off_wg; };
  auto seg_masked = [&](const TileIt& t) __attribute__((always_inline)) { return PACKED && t.j * KVT < seg_lo_max; };
  int nx1_masked = 0;                                // tile nx1 takes a mask (wave-uniform; kept with nx1)
  unsigned long long slow = 0;                       // tile t fails the acceptance, or tile t+1 needs a mask (wave-uniform)
  TileIt nx1, nx2;
  auto next_masked = [&]() __attribute__((always_inline)) { return needs_mask(nx1) || seg_masked(nx1); };
  auto qk_phase = [&](int dst, unsigned kslot, bool fill, int par) __attribute__((always_inline)) {
    const unsigned vslot = lds0 + LDS_V + par * TILEB;
    bf16x8 kr[4];
    if (fill) { kr[0] = kr_pre[0]; kr[1] = kr_pre[1]; kr[2] = kr_pre[2]; }
    else { kr[0] = k_frag(kslot, 0); kr[1] = k_frag(kslot, 1); }
#pragma unroll
    for (int s = 0; s < 32; ++s) {
      const int i = s >> 1, qb = s & 1, ds = i >> 1, kb = i & 1;
      if (fill && (s & 3) == 2) {                    // pieces 0 .. 3 of K in front of MFMAs 2, 6, 10, 14; of V in front of 18, 22, 26, 30:
        const int q = s >> 2;                        // the gaps that carry a sum-and-pack half-unit (12 cycles of VALU issue)
        if (q < 4) { if (spread_k) dma_piece(rk_next, dk_off, lds_kw, spread_k_slot, q); }
        else if (spread_v) dma_piece(rv_next, dv_off, lds_vw, spread_v_slot, q - 4);
      }
      if (qb == 0 && i + 2 < 16 && !(fill && i == 0)) kr[(i + 2) & 3] = k_frag(kslot, i + 2);
      if (fill && s == 29) vr_pre[0] = v_frag(vslot, 0);
      if (fill && s == 31) {
        vr_pre[1] = v_frag(vslot, 1); vr_pre[2] = v_frag(vslot, 2);
        // the acceptance of tile `par` (its last row-sum add is behind MFMA 29) and the mask flag of the tile being multiplied, in one
        // scalar: two v_cmp into lane masks and two s_or HERE, one s_cmp and one branch behind the last MFMA (the two ballots are
        // separate on purpose: a ballot of `a || b` goes through a v_cndmask and a second v_cmp)
        slow = __builtin_amdgcn_ballot_w64(!(l_tile[0] <= ACCEPT_MAX)) | __builtin_amdgcn_ballot_w64(!(l_tile[1] <= ACCEPT_MAX)) |
               (unsigned long long)(unsigned)nx1_masked;
        asm volatile("" : "+s"(slow));
      }
      if (fill) __builtin_amdgcn_sched_barrier(0);   // DMA piece and K reads in FRONT of the slot's MFMA: they share the gap of the slot before
      if (ds == 0) {
        f32x16 z;
#pragma unroll
        for (int r = 0; r < 16; ++r) z[r] = 0.f;
        sb[dst][qb][kb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kr[i & 3], qf[qb][ds], z, 0, 0, 0);
      } else {
        sb[dst][qb][kb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kr[i & 3], qf[qb][ds], sb[dst][qb][kb], 0, 0, 0);
      }
      if (fill) {
        __builtin_amdgcn_sched_barrier(0);           // the slot's filler goes BEHIND its MFMA
#pragma unroll
        for (int u = 0; u < DEAL1.n[s]; ++u) exp_half(par, DEAL1.h[s][u], DEAL1.w[s][u]);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  };
  // the rest of tile `par`'s softmax without a next tile to multiply (last tile)
  auto finish_sm = [&](int par) __attribute__((always_inline)) {
#pragma unroll
    for (int u = 8 * NF2; u < 64; ++u) exp_half(par, u);
  };
  // O += V(vslot)^T P(par)^T  ||  (has_next) the first NF2 fragments of tile par ^ 1; the first three V^T fragments are in vr_pre.
  // EARLY (a loop trip: another S phase follows and its K tile was fetched in this trip): the phase holds the tile's barrier and
  // everything the next S phase needs before its first MFMA, so that the seam between the two holds the loop's branch and nothing else:
  //   behind MFMAs 5 and 9 (sum-and-pack gaps)  the tile walk moves on (at a chunk end through the chunk tables, where it stands)
  //                                             and the two DMA descriptors and the mask flag of the next trip are made, in SGPRs
  //   in front of MFMA 29                       s_waitcnt vmcnt(0) lgkmcnt(0) + s_barrier.  What the barrier waits for is over by
  //                                             then: every wave's reads of V(t) (the last one is issued in front of MFMA 26; the
  //                                             lgkmcnt(0) sees it back) and of K(t+1) (the S phase), and this wave's pieces of K(t+2) /
  //                                             V(t+1) (issued in the S phase).  The DMAs that refill the two slots are issued in the
  //                                             NEXT S phase, behind the barrier, as before.
  //   behind the barrier, in front of 29 and 30 the first three K fragments of K(t+2), from the ring slot this trip filled
  auto pv_phase = [&](int par, unsigned vslot, bool has_next, bool early) __attribute__((always_inline)) {
    const unsigned kslot_next = lds0 + LDS_K + par * TILEB;
    bf16x8 vr[4];
    if (has_next) { vr[0] = vr_pre[0]; vr[1] = vr_pre[1]; vr[2] = vr_pre[2]; }
    else { vr[0] = v_frag(vslot, 0); vr[1] = v_frag(vslot, 1); }
#pragma unroll
    for (int s = 0; s < 32; ++s) {
      const int i = s >> 1, qb = s & 1, t = i >> 2, db = i & 3;
      if (qb == 0 && i + 2 < 16 && !(has_next && i == 0)) vr[(i + 2) & 3] = v_frag(vslot, i + 2);
      if (early && s == 29) {
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        kr_pre[0] = k_frag(kslot_next, 0);
      }
      if (early && s == 30) { kr_pre[1] = k_frag(kslot_next, 1); kr_pre[2] = k_frag(kslot_next, 2); }
      const u32x4 pw = {pk[par][qb][t][0], pk[par][qb][t][1], pk[par][qb][t][2], pk[par][qb][t][3]};
      const bf16x8 pf = __builtin_bit_cast(bf16x8, pw);
      asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, %0" : "+a"(o[qb][db]) : "v"(vr[i & 3]), "v"(pf));
      __builtin_amdgcn_sched_barrier(0);             // the slot's filler goes BEHIND its MFMA (left alone, half 0 is hoisted in front of it)
      if (has_next) {
#pragma unroll
        for (int u = MAP2.first[s]; u < MAP2.first[s + 1]; ++u) exp_half(par ^ 1, u);
      }
      if (early && s == 5) { nx1 = nx2; walk.advance(nx2); }      // (behind the last tile the walk ends: no table is read past its end)
      if (early && s == 9) {
        rk_next = vita_make_rsrc_uniform(nx2.kp); rv_next = vita_make_rsrc_uniform(nx1.vp);
        asm volatile("" : "+s"(rk_next), "+s"(rv_next));          // made HERE, not where the first piece goes out
        nx1_masked = __builtin_amdgcn_readfirstlane((int)next_masked());
        asm volatile("" : "+s"(nx1_masked));
      }
      __builtin_amdgcn_sched_barrier(0);
    }
  };
  // causal mask of a diagonal-chunk tile (kv_off = its offset inside the chunk) in buffer `par`.  Pure VALU arithmetic
  // (s += min(lim - key, 0) * 3e38: exp2 of it is 0, a running maximum never sees it) — compare-and-select would park 64
  // lane masks in SGPR pairs and the per-register key constants in VGPRs, and that pressure spills into the steady state.
  auto mask_tile = [&](int par, int kv_off) __attribute__((always_inline)) {
#pragma unroll
    for (int qb = 0; qb < 2; ++qb) {
      const int base = q_off + 32 * qb + l31 - kv_off - 4 * hi;                 // key <= lim visible; key = const(kb, r) + 4 hi
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int kc = 32 * kb + (r & 3) + 8 * (r >> 2);
          const float pen = fminf((float)(base - kc), 0.0f);
          sb[par][qb][kb][r] = fmaf(pen, 3.0e38f, sb[par][qb][kb][r]);
        }
    }
  };
  // packed samples: keys before a row's segment start (key >= seg_lo visible), same arithmetic
  auto seg_mask_tile = [&](int par, int kv_off) __attribute__((always_inline)) {
#pragma unroll
    for (int qb = 0; qb < 2; ++qb) {
      const int base = kv_off + 4 * hi - seg_lo[qb];
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int kc = 32 * kb + (r & 3) + 8 * (r >> 2);
          const float pen = fminf((float)(base + kc), 0.0f);
          sb[par][qb][kb][r] = fmaf(pen, 3.0e38f, sb[par][qb][kb][r]);
        }
    }
  };
  // Acceptance of tile `par`, after its last exp half-unit and before its P V phase.  The half-units used the running maxima as they
  // stood (OPTIMISTIC: no maxima are taken in the steady state).  Probabilities are non-negative, so a lane's sum l_tile <= 2^THR
  // proves each of its 32 p <= 2^THR: the lazy rule (move the maxima when some row of the wave exceeds its own by more than 2^THR)
  // would have left the tile alone, and it is accepted as it is.  A lane that fails (inf included: a row still at -1e30 meeting its
  // first visible key) sends the whole wave out of line: true maxima from S(par), which is intact up to here, and the lazy rule
  // itself.  If no row exceeds its maximum by 2^THR (a sum of many p, none of them large) the tile stands as computed.  Otherwise
  // the RARE path: the maxima move, l and O *= alpha (every P V MFMA of the tile before has been issued), all 64 half-units again.
  // The maxima therefore move on exactly the tiles, and to exactly the values, of the lazy rule: results are bit for bit its results.
  // In a loop trip the test itself is made inside the S phase (`slow`, qk_phase) and accept_slow is entered out of line with the P V
  // phase's first three V^T fragments in registers; it repeats the test, since `slow` also stands for a tile that only needs a mask.
  auto accept_slow = [&](int par) __attribute__((always_inline)) {
    if (__builtin_expect(__any(!(l_tile[0] <= ACCEPT_MAX) || !(l_tile[1] <= ACCEPT_MAX)), 0)) {
      float mx[2];
      row_max(par, mx);
      if (__any((mx[1] > m_run[1] + (float)THR) || (mx[0] > m_run[0] + (float)THR))) {
        float alpha[2];
        raise_max(mx, alpha);
        // (the accumulators are operands of the wait: the compiler may not read them above it)
        asm volatile("s_nop 15\n\ts_nop 15" : "+a"(o[0][0]), "+a"(o[0][1]), "+a"(o[0][2]), "+a"(o[0][3]), "+a"(o[1][0]), "+a"(o[1][1]), "+a"(o[1][2]), "+a"(o[1][3]));                       // asm MFMA -> accumulator read
#pragma unroll
        for (int qb = 0; qb < 2; ++qb) {
          l_run[qb] *= alpha[qb];
          l_tile[qb] = 0.f;
#pragma unroll
          for (int db = 0; db < 4; ++db) {
#pragma unroll
            for (int r = 0; r < 16; ++r) o[qb][db][r] *= alpha[qb];
            asm volatile("" : "+a"(o[qb][db]));
          }
        }
        asm volatile("s_nop 7" ::: "memory");                                     // accumulator write -> asm MFMA read
#pragma unroll
        for (int h = 0; h < 64; ++h) exp_half(par, h);
      }
    }
  };
  auto fold_tile = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int qb = 0; qb < 2; ++qb) {
      l_run[qb] += l_tile[qb];
      l_tile[qb] = 0.f;
    }
  };
  auto accept = [&](int par) __attribute__((always_inline)) { accept_slow(par); fold_tile(); };
  auto masks = [&](const TileIt& t, int par) __attribute__((always_inline)) {          // wave-uniform conditions
    if (needs_mask(t)) mask_tile(par, t.j * KVT);
    if constexpr (PACKED) {
      if (seg_masked(t)) seg_mask_tile(par, t.j * KVT);
    }
  };

  // ---- prologue: K(0), V(0), K(1) -> LDS; S(0); the start of its softmax -----------------------------------------------------
  TileIt cur;
  walk.begin(cur);
  nx1 = cur;
  walk.advance(nx1);
  dma_k(cur, 0); dma_v(cur, 0);
  dma_k(nx1, 1);                                     // n_tiles >= 4
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  qk_phase(0, lds0 + LDS_K, false, 0);
  __syncthreads();                                  // every wave has read K(0): its ring slot may be refilled
  masks(cur, 0);
  {
    float mx0[2], alpha0[2];                         // tile 0 gets its true maxima (O and l are zero: nothing to rescale)
    row_max(0, mx0);
    raise_max(mx0, alpha0);
  }
#pragma unroll
  for (int u = 0; u < 8 * NF2; ++u) exp_half(0, u);

  // ---- main loop: two tiles per trip (the S / P buffer parity is a compile-time constant); n_tiles is a multiple of 4 ----------
  // full(par): tile t sits in buffer par; K(t+2) -> K ring slot par, V(t+1) -> V ring slot par ^ 1; S(t+1) -> buffer par ^ 1.  On entry
  // nx1 / nx2 are tiles t+1 / t+2, rk_next / rv_next the descriptors of K(t+2) / V(t+1), nx1_masked the mask flag of tile t+1 and
  // kr_pre the first three fragments of K(t+1): a loop trip (more_k) leaves all of that behind for the next one from inside its P V
  // phase, barrier included; the peeled trip has no S phase to prepare and keeps its barrier behind the phase.
  // The two seams of a trip: S(t+1) -> P V(t) is ONE scalar compare and branch (`slow`, fragments in vr_pre); P V(t) -> S(t+2) is the
  // loop's own branch (fragments in kr_pre).
  auto full = [&](int par, bool more_k) __attribute__((always_inline)) {
    // K(t+2) and V(t+1) go out one piece at a time inside the S phase (K(t) in that slot was last read before the previous barrier)
    spread_k = more_k; spread_k_slot = par;
    spread_v = true; spread_v_slot = par ^ 1;
    qk_phase(par ^ 1, lds0 + LDS_K + (par ^ 1) * TILEB, true, par);
    if (__builtin_expect(slow != 0, 0)) { accept_slow(par); masks(nx1, par ^ 1); }
    fold_tile();
    pv_phase(par, lds0 + LDS_V + par * TILEB, true, more_k);
    if (!more_k) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
    }
  };
  // what the first trip finds ready (K(1) is in ring slot 1 since the prologue's first barrier)
  kr_pre[0] = k_frag(lds0 + LDS_K + TILEB, 0); kr_pre[1] = k_frag(lds0 + LDS_K + TILEB, 1); kr_pre[2] = k_frag(lds0 + LDS_K + TILEB, 2);
  nx2 = nx1;
  walk.advance(nx2);                                 // n_tiles >= 4
  rk_next = vita_make_rsrc_uniform(nx2.kp); rv_next = vita_make_rsrc_uniform(nx1.vp);
  nx1_masked = __builtin_amdgcn_readfirstlane((int)next_masked());
  for (int t = 0; t + 2 < n_tiles; t += 2) {
    full(0, true);
    full(1, true);
  }
  full(0, false);
  finish_sm(1);                                      // last tile: the rest of its softmax, then P V
  accept(1);
  pv_phase(1, lds0 + LDS_V + TILEB, false, false);

  // ---- epilogue: O[row][head][d] = O^T / l, lse ------------------------------------------------------------------------------
  asm volatile("s_nop 15\n\ts_nop 15" : "+a"(o[0][0]), "+a"(o[0][1]), "+a"(o[0][2]), "+a"(o[0][3]), "+a"(o[1][0]), "+a"(o[1][1]), "+a"(o[1][2]), "+a"(o[1][3]));
#pragma unroll
  for (int qb = 0; qb < 2; ++qb) {
    const float l_tot = swap32_sum(l_run[qb]);
    const float inv = l_tot > 0.f ? 1.0f / l_tot : 0.f;
    const int64_t orow = (int64_t)qc * p.chunk_len + q_off + 32 * qb + l31;
    bf16_t* op = p.o + (int64_t)b * p.o_bs + orow * p.o_rs + (int64_t)kvh * p.o_gs + (int64_t)hq * p.o_hs;
#pragma unroll
    for (int db = 0; db < 4; ++db) store_row_block32(op + 32 * db, o[qb][db], inv, hi);       // two 16-byte stores per block (r06)
    if (p.lse && hi == 0) {
      const float lse = l_tot > 0.f ? (m_run[qb] + log2f(l_tot)) * 0.69314718055994530942f : -INFINITY;
      p.lse[((int64_t)b * p.n_q_heads + head) * p.n_q_rows + orow] = lse;
    }
  }
}

}  // namespace

bool vita_attn64_eligible(const AttnArgs& a, int head_dim, bool causal) {
  if (head_dim != 128 || !causal) return false;
  if (a.seg_start && (a.n_q_chunks != 1 || a.n_kv_chunks != 1 || a.batch != 1)) return false;     // packed samples: one chunk (CP = 1)
  if (a.chunk_len % QTILE || a.q_valid != a.chunk_len || a.kv_valid != a.chunk_len) return false;
  // 16-byte output stores (r06)
  if (((uintptr_t)a.o & 15) || (a.o_rs & 7) || (a.o_hs & 7) || (a.o_gs & 7) || (a.o_bs & 7)) return false;
  // a tile's 64 rows x row stride must fit the 32-bit lane offset of the DMA
  if (a.k_rs * 2 * KVT >= (1ll << 31) || a.v_rs * 2 * KVT >= (1ll << 31)) return false;
  // (a query chunk sees whole chunks, its own up to the diagonal, or nothing: the tile count is 0 or a multiple of 4)
  const char* e = vita_dev_getenv("VITA_ATTN64");
  return !(e && e[0] == '0');
}

int vita_attn64_launch(const AttnArgs& a, int64_t nblocks, hipStream_t st) {
  static std::atomic<unsigned long long> attr_set{0};
  vita_device_once(attr_set, [&] {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&flash_fwd64_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize, 4 * TILEB);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&flash_fwd64_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, 4 * TILEB);
  });
  if (a.seg_start) hipLaunchKernelGGL((flash_fwd64_kernel<true>), dim3((unsigned)nblocks), dim3(256), 4 * TILEB, st, a);
  else hipLaunchKernelGGL((flash_fwd64_kernel<false>), dim3((unsigned)nblocks), dim3(256), 4 * TILEB, st, a);
  return vita_check_launch();
}
