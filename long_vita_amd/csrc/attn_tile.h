// What the attention kernels must agree on, written once: the swizzled LDS layouts of a K / V / Q / dO tile (and their inverses, which
// the LDS-DMA applies to its SOURCE address: the DMA writes lane-linear), the lane map of the transposed read, the decode of a block id
// into a query tile, and the causal walk over whole 64-key tiles.  A read formula and a DMA formula that disagree give wrong numbers
// with no fault, so the bank-conflict arguments are static_asserts here, not comments in nine files.
// Users: attn.hip, attn64.hip, attn64v.hip, attn_extend.hip, attn_bwd.hip, attn_bwd64.hip, attn_bwd_kv64.hip, attn_bwd_kvp.hip.
#pragma once
#include "vita_common.h"
#include <type_traits>

constexpr int kMaxChunks = 32;                          // chunk-table entries of AttnArgs / BwdArgs
constexpr float LOG2E = 1.44269504088896340736f;

typedef __attribute__((address_space(3))) char lds_char;
typedef __attribute__((address_space(3))) const bf16x8 lds_bf16x8;
typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
typedef __attribute__((address_space(3))) u32x4 lds_u32x4;
typedef __attribute__((address_space(3))) const f32x4 lds_f32x4;
typedef __attribute__((address_space(3))) void lvoid;
typedef __attribute__((address_space(1))) const void gvoid;

// max / sum over the two lanes (l, l + 32) that share a query row of a 32 x 32 accumulator
__device__ __forceinline__ float swap32_max(float x) {
  const unsigned xi = __float_as_uint(x);
  auto r = __builtin_amdgcn_permlane32_swap(xi, xi, false, false);
  return fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
}
__device__ __forceinline__ float swap32_sum(float x) {
  const unsigned xi = __float_as_uint(x);
  auto r = __builtin_amdgcn_permlane32_swap(xi, xi, false, false);
  return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}

// ---- LDS layouts of a [rows][D] bf16 tile (row = 2 D bytes = D / 8 slots of 16 bytes; the bank period is 256 bytes) ----------------------
// Every layout is a per-row map of logical to physical position, its inverse, and the byte offset it gives:
//   frag  rows read as ds_read_b128 fragments, 16 consecutive rows x one logical slot per pass
//   tr    rows read by ds_read_b64_tr_b16, a 32-lane half touching 4 rows x 64 bytes; the unit that moves is the 32-byte chunk
//   dual  (D = 128) one image that serves both reads
#define TILE_FN __host__ __device__ __forceinline__ constexpr

// d = 96 (a head size of 72 zero-padded): a row is 192 bytes = 12 slots = 3/4 of a bank period, so an XOR does not fit.  The frag layout
// ROTATES the slot by (row >> 2) & 3 mod 12: rows r .. r + 3 start 0, 12, 8, 4 units into the period, the rotation of rows r + 4 k fills
// each group of four.  The tr layout needs nothing: 192 = -64 mod 256 puts rows r .. r + 3 in four different 64-byte windows as they are.
template <int D> TILE_FN int frag_slot(int row, int slot) {                     // logical -> physical 16-byte slot
  return D == 128 ? (slot ^ (row & 15)) : D == 96 ? (slot + ((row >> 2) & 3)) % 12 : (slot ^ ((row >> 1) & 7));
}
template <int D> TILE_FN int frag_slot_inv(int row, int ps) {                   // physical -> logical: the DMA's source slot
  return D == 128 ? (ps ^ (row & 15)) : D == 96 ? (ps + 12 - ((row >> 2) & 3)) % 12 : (ps ^ ((row >> 1) & 7));
}
template <int D> TILE_FN int frag_off(int row, int slot) { return row * (2 * D) + (frag_slot<D>(row, slot) << 4); }

template <int D> TILE_FN int tr_chunk(int row, int chunk) {                     // logical -> physical 32-byte chunk (its own inverse)
  return D == 128 ? (chunk ^ ((row & 3) << 1)) : D == 96 ? chunk : (chunk ^ (row & 2));
}
template <int D> TILE_FN int tr_slot_inv(int row, int ps) {                     // physical 16-byte slot -> logical: the DMA's source slot
  return D == 128 ? ((((ps >> 1) ^ ((row & 3) << 1)) << 1) | (ps & 1)) : D == 96 ? ps : ((((ps >> 1) ^ (row & 2)) << 1) | (ps & 1));
}
template <int D> TILE_FN int tr_off(int row, int chunk, int b) { return row * (2 * D) + (tr_chunk<D>(row, chunk) << 5) + b; }

// dual use, D = 128: 16-byte slots XOR-ed with dual_key(row).  16 consecutive rows get 16 different keys (frag reads); rows 4 k .. 4 k + 3
// differ in the key's upper two bits, which pick the 64-byte window (transposed reads).  An XOR: the map is its own inverse.
TILE_FN int dual_key(int row) { return ((row & 3) << 2) | ((row >> 2) & 3); }
TILE_FN int dual_slot(int row, int slot) { return slot ^ dual_key(row); }
TILE_FN int dual_off(int row, int slot) { return row * 256 + (dual_slot(row, slot) << 4); }

// ds_read_b64_tr_b16: inside a 16-lane group, lane i supplies the 8-byte piece (row i >> 2, columns 4 (i & 3) ..) of a [4 rows][16 d] block;
// group g covers rows 4 (g >> 1) .. and the columns 16 (g & 1) .. of the 32-column block db.  A second read 8 rows down completes 16 rows.
TILE_FN int tr_lane_row(int lane) {
  const int g16 = lane >> 4, i16 = lane & 15;
  return 4 * (g16 >> 1) + (i16 >> 2);
}
TILE_FN int tr_lane_col(int lane, int db) {
  const int g16 = lane >> 4, i16 = lane & 15;
  return 32 * db + 16 * (g16 & 1) + 4 * (i16 & 3);
}

// ---- the comments' arguments as compile-time facts (rows 0 .. 63: every kernel's tile; the formulas repeat every 16 rows) ------------------
namespace tile_check {
constexpr int kRows = 64;
template <int D> constexpr bool frag_inverts() {        // a permutation of the row's slots, and frag_slot_inv undoes it
  for (int row = 0; row < kRows; ++row)
    for (int s = 0; s < D / 8; ++s) {
      const int ps = frag_slot<D>(row, s);
      if (ps < 0 || ps >= D / 8 || frag_slot_inv<D>(row, ps) != s || frag_slot<D>(row, frag_slot_inv<D>(row, s)) != s) return false;
    }
  return true;
}
template <int D> constexpr bool tr_inverts() {          // the same for the 16-byte slots of the tr layout
  for (int row = 0; row < kRows; ++row)
    for (int s = 0; s < D / 8; ++s) {
      const int ps = (tr_chunk<D>(row, s >> 1) << 1) | (s & 1);
      if (ps < 0 || ps >= D / 8 || tr_slot_inv<D>(row, ps) != s || tr_chunk<D>(row, tr_chunk<D>(row, s >> 1)) != (s >> 1)) return false;
    }
  return true;
}
constexpr bool dual_inverts() {
  for (int row = 0; row < kRows; ++row)
    for (int s = 0; s < 16; ++s) {
      const int ps = dual_slot(row, s);
      if (ps < 0 || ps >= 16 || dual_slot(row, ps) != s) return false;
    }
  return true;
}
// one logical slot across ANY 16 consecutive rows lands in 16 different 16-byte units of the 256-byte bank period
template <class Off> constexpr bool frag_conflict_free(Off off, int slots) {
  for (int r0 = 0; r0 + 16 <= kRows; ++r0)
    for (int s = 0; s < slots; ++s) {
      unsigned seen = 0;
      for (int r = r0; r < r0 + 16; ++r) seen |= 1u << ((off(r, s) >> 4) & 15);
      if (seen != 0xffffu) return false;
    }
  return true;
}
// the four rows 4 k .. 4 k + 3 that a 32-lane half of a transposed read touches, at one logical 64-byte window w of the row, land in four
// different 64-byte windows of the bank period, and each row's 64 bytes stay inside one window
template <class Off> constexpr bool tr_conflict_free(Off off64, int windows) {     // off64(row, w, i): byte offset of 16-byte piece i of window w
  for (int r0 = 0; r0 < kRows; r0 += 4)
    for (int w = 0; w < windows; ++w) {
      unsigned seen = 0;
      for (int r = r0; r < r0 + 4; ++r) {
        for (int i = 1; i < 4; ++i)
          if ((off64(r, w, i) >> 6) != (off64(r, w, 0) >> 6)) return false;
        seen |= 1u << ((off64(r, w, 0) >> 6) & 3);
      }
      if (seen != 0xfu) return false;
    }
  return true;
}
static_assert(frag_inverts<128>() && frag_inverts<96>() && frag_inverts<64>(), "frag layout: slot map and DMA source slot disagree");
static_assert(tr_inverts<128>() && tr_inverts<96>() && tr_inverts<64>(), "tr layout: chunk map and DMA source slot disagree");
static_assert(dual_inverts(), "dual layout: not an involution on the row's 16 slots");
static_assert(frag_conflict_free([](int r, int s) { return frag_off<128>(r, s); }, 16), "frag layout, d = 128: ds_read_b128 bank conflict");
static_assert(frag_conflict_free([](int r, int s) { return frag_off<64>(r, s); }, 8), "frag layout, d = 64: ds_read_b128 bank conflict");
static_assert(frag_conflict_free([](int r, int s) { return frag_off<96>(r, s); }, 12), "frag layout, d = 96: (12 row + rotated slot) mod 16 is not a permutation over 16 rows");
static_assert(frag_conflict_free([](int r, int s) { return dual_off(r, s); }, 16), "dual layout: ds_read_b128 bank conflict");
static_assert(tr_conflict_free([](int r, int w, int i) { return tr_off<128>(r, 2 * w + (i >> 1), (i & 1) * 16); }, 4), "tr layout, d = 128: ds_read_b64_tr_b16 bank conflict");
static_assert(tr_conflict_free([](int r, int w, int i) { return tr_off<96>(r, 2 * w + (i >> 1), (i & 1) * 16); }, 3), "tr layout, d = 96: ds_read_b64_tr_b16 bank conflict");
static_assert(tr_conflict_free([](int r, int w, int i) { return tr_off<64>(r, 2 * w + (i >> 1), (i & 1) * 16); }, 2), "tr layout, d = 64: ds_read_b64_tr_b16 bank conflict");
static_assert(tr_conflict_free([](int r, int w, int i) { return dual_off(r, 4 * w + i); }, 4), "dual layout: ds_read_b64_tr_b16 bank conflict");
}  // namespace tile_check
#undef TILE_FN

// ---- block id -> query tile: kv head innermost (= the XCD when there are 8 kv heads, so one XCD's L2 serves one kv head's K / V stream to
// all its concurrently running query tiles), then the query head of the group, then the 256-row query tiles heaviest first.  The forward
// (AttnArgs) orders chunks by global id (q_order), has a batch above the tiles and, in a windowed launch (win_n > 0), workgroups for the
// listed tiles only, each decoding to the workgroup the full launch runs for its tile; the backward (BwdArgs) takes chunks last to first.
struct AttnArgs;
struct QTileId { int kvh, hq, head, b, qc, qti; };   // kv head, query head in its group, query head, batch, chunk (buffer order), tile in chunk
template <class Args>
__device__ __forceinline__ QTileId decode_q_tile(const Args& p, int bid, const int tiles_per_chunk) {
  QTileId t;
  const int G = p.n_q_heads / p.n_kv_heads;
  t.kvh = bid % p.n_kv_heads; bid /= p.n_kv_heads;
  t.hq = bid % G; bid /= G;
  t.head = t.kvh * G + t.hq;
  if constexpr (std::is_same<Args, AttnArgs>::value) {
    const int n_q_tiles = p.n_q_chunks * tiles_per_chunk;
    const int n_launched = p.win_n ? p.win_n : n_q_tiles;
    const int qt_order = p.win_n ? p.win_qt[bid % n_launched] : bid % n_launched;
    t.b = bid / n_launched;
    t.qc = p.q_order[qt_order / tiles_per_chunk];
    t.qti = tiles_per_chunk - 1 - qt_order % tiles_per_chunk;
  } else {
    t.b = 0;
    t.qc = p.n_q_chunks - 1 - bid / tiles_per_chunk;
    t.qti = tiles_per_chunk - 1 - bid % tiles_per_chunk;
  }
  return t;
}

// ---- the causal walk of a 256-row query tile over whole 64-key tiles (chunk_len % 256 == 0): a key chunk with a smaller global id is
// visible whole, the tile's own chunk up to the tile's last row, a later chunk not at all.  All fields wave-uniform -> SGPRs.
// The walk REFERS to the kernel's own kbase / vbase / gq / q_off_wg / seg_j0 (named locals that outlive it), as the lambdas it replaces
// captured them: with copies the compiler allocated the packed attn64 instance one SGPR differently.
struct TileIt {
  int c, j, n;        // chunk, tile inside chunk, tiles to visit in this chunk; c == n_kv_chunks: end
  int diag;           // chunk c is the query tile's own chunk
  const char* kp;     // first K / V row of the tile (running pointers: one 64-bit add per tile, no multiplies in the loop)
  const char* vp;
};
template <bool PACKED, class Args>
struct CausalTileWalk {
  static constexpr int KVT = 64, QTILE = 256;
  const Args& p;
  const char* const& kbase; const char* const& vbase;    // the kv head's first K / V row
  const int& gq; const int& q_off_wg;                    // global id of the query tile's chunk, the tile's first row inside it
  const int& seg_j0;                                     // PACKED: first tile to visit (the tile of the first row's segment start)
  int tiles_per_chunk, k_tile_bytes, v_tile_bytes;

  __device__ __forceinline__ CausalTileWalk(const Args& p_, const char* const& kbase_, const char* const& vbase_, const int& gq_,
                                            const int& q_off_wg_, const int& seg_j0_)
      : p(p_), kbase(kbase_), vbase(vbase_), gq(gq_), q_off_wg(q_off_wg_), seg_j0(seg_j0_), tiles_per_chunk(p_.chunk_len / KVT),
        k_tile_bytes((int)(p_.k_rs * 2 * KVT)), v_tile_bytes((int)(p_.v_rs * 2 * KVT)) {}
  __device__ __forceinline__ int visible(int gk) const {             // tiles the query tile sees of a key chunk with global id gk
    return gk < gq ? tiles_per_chunk : (gk > gq ? 0 : q_off_wg / KVT + QTILE / KVT);
  }
  __device__ __forceinline__ void enter(TileIt& t) const {           // skip chunks with nothing to visit
    while (t.c < p.n_kv_chunks) {
      const int gk = p.kv_gid[t.c];
      t.diag = gk == gq;
      t.n = visible(gk);
      if (t.n > 0) {
        const int64_t crow = p.kv_row[t.c] + (PACKED ? seg_j0 * KVT : 0);
        t.kp = kbase + crow * p.k_rs * 2;
        t.vp = vbase + crow * p.v_rs * 2;
        t.j = PACKED ? seg_j0 : 0;                   // (t.n stays the absolute end: tiles seg_j0 .. t.n - 1)
        return;
      }
      ++t.c;
    }
  }
  __device__ __forceinline__ void begin(TileIt& t) const {           // the first tile of the walk
    t.c = 0; t.j = 0; t.n = 0; t.diag = 0; t.kp = kbase; t.vp = vbase;
    enter(t);
  }
  __device__ __forceinline__ void advance(TileIt& t) const {
    t.kp += k_tile_bytes;
    t.vp += v_tile_bytes;
    if (++t.j == t.n) { ++t.c; enter(t); }
  }
  __device__ __forceinline__ int count() const {                     // tiles of the whole walk: 0 or a multiple of 4 (PACKED: less seg_j0)
    int n = 0;
    for (int c = 0; c < p.n_kv_chunks; ++c) n += visible(p.kv_gid[c]);
    if constexpr (PACKED) n -= seg_j0;
    return n;
  }
};

// ---- host side of the two C entry points ------------------------------------------------------------------------------------------------
// stride between the first query heads of two kv groups: 0 means the heads of a group are contiguous
inline int64_t vita_group_stride(int64_t group_stride, int64_t head_stride, int heads_per_group) {
  return group_stride ? group_stride : head_stride * heads_per_group;
}
template <class Args, class Params> inline void vita_copy_chunk_tables(Args& a, const Params* p) {
  for (int i = 0; i < p->n_q_chunks; ++i) a.q_gid[i] = p->q_chunk_gid[i];
  for (int i = 0; i < p->n_kv_chunks; ++i) { a.kv_gid[i] = p->kv_chunk_gid[i]; a.kv_row[i] = p->kv_chunk_row[i]; }
}
