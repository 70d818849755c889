// MXFP8 (OCP e4m3fn codes + one E8M0 scale per 32 K elements) for the opt-in prefill GEMMs: the quantiser that runs once
// per weight and once per activation matrix per linear, and the tile GEMM over two quantised operands on the block-scaled matrix
// instruction v_mfma_scale_f32_16x16x128_f8f6f4.  The rule is mx8_rule.h's (tests/mx8_rule.py): codes [rows, K] one byte each (row
// stride in bytes), scales [rows, K / 32] bytes dense.
//
// The instruction's maps (tools/hwprobe/mx8_map.hip, profiles/r27_mx8_map.txt), lane l, r = l & 15, q = l >> 4: operand registers 0-3
// hold K 16 q .. + 15 and registers 4-7 hold K 64 + 16 q .. + 15 of row (column) r; byte 0 of the lane's scale register scales row
// (column) r, K 32 q .. + 31 — the run q, which is NOT the lane's own 32 elements; D[4 q + j][r] as for every 16 x 16 form.
//
// gemm_mx8_kernel (one workgroup = WM x WN waves = one BM x BN output tile, one K-step = 128 elements = one MFMA per 16 x 16 block):
//   * a code tile is [rows][128] bytes, the bf16 tile kernel's 128-byte rows: staged HBM -> LDS by 16-byte LDS-DMA, two stages, one
//     barrier per K-step; the swizzle sits on the per-lane SOURCE address and is mirrored on the ds_read_b128 side:
//     physical 16-B slot = logical slot ^ ((row >> 1) & 7).  A fragment is the two slots q and q + 4 of row r (2 x ds_read_b128); the
//     four 16-lane groups a ds_read_b128 is served in each hold rows 0 .. 15 once, with q's low bit = r3 ^ r2 (or its complement),
//     and the swizzle makes the 16 (128-byte half, slot) pairs of a group distinct: conflict-free;
//   * the scale bytes of a K-step are 4 bytes per row: each stage carries them behind its code tiles as [rows][4], filled by 4-byte
//     LDS-DMA (one wave-instruction per 64 rows, straight from scales[row][4 kt .. + 3]), and a lane reads the byte the instruction
//     wants from it — row r, run q — with one ds_read_u8 per 16-row block: no VALU work, no register shuffles;
//   * the weight fragment is the MFMA's first operand and the activation fragment its second, so a lane ends up with four consecutive
//     output columns of one row: 8-byte bias / residual loads and bf16 stores;
//   * every output element is one chain of K / 128 MFMAs in ascending k on a zero accumulator, whatever the tile, the wave or M: a
//     row's bits do not depend on M or on the tile the row falls in, by construction (both tile shapes run the same chain).
//   Ragged M: source rows are clamped to M - 1 (their products land in rows the epilogue does not store).
//   Resources (hipcc -Rpass-analysis=kernel-resource-usage, no scratch in any instantiation):
//     <256,256,2,4>: 8 waves, 216 - 220 VGPR, 0 AGPR, 2 waves per SIMD, 133 KiB LDS (2 x (64 KiB codes + 2 KiB scales)): one workgroup per CU
//     <128,128,2,2>: 4 waves, 148 - 152 VGPR, 0 AGPR, 66 KiB LDS: two workgroups per CU (ragged or small problems)
//     mx8_quantize_kernel: 32 VGPR, no LDS
#include "vita_common.h"
#include "mx8_rule.h"

namespace {

typedef __attribute__((address_space(3))) void lds_void;
typedef __attribute__((address_space(3))) const u32x4 lds_u32x4;
typedef __attribute__((address_space(3))) const unsigned char lds_u8;
typedef __attribute__((address_space(3))) char lds_char;
typedef __attribute__((address_space(1))) const void gbl_cvoid;
typedef int i32x8 __attribute__((ext_vector_type(8)));

// ---- quantiser: item = (row, run); its 4 lanes hold 8 elements each and share the maximum by __shfl_xor ------------------------------
__global__ __launch_bounds__(256) void mx8_quantize_kernel(const bf16_t* __restrict__ X, int64_t ldx, int64_t rows, int nblk,
                                                           unsigned char* __restrict__ codes, int64_t ldc,
                                                           unsigned char* __restrict__ scales) {
  const int sub = threadIdx.x & 3;
  const int64_t items = rows * nblk;
  for (int64_t it = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 2; it < items; it += ((int64_t)gridDim.x * blockDim.x) >> 2) {
    const int64_t r = it / nblk;
    const int b = (int)(it - r * nblk);
    const u32x4 x = *reinterpret_cast<const u32x4*>(X + r * ldx + b * kMx8Block + sub * 8);
    unsigned m = kv8_absmax_bits(x);
#pragma unroll
    for (int o = 1; o < 4; o <<= 1) m = max(m, (unsigned)__shfl_xor((int)m, o));
    const unsigned sb = mx8_scale_byte(m);
    *reinterpret_cast<u32x2*>(codes + r * ldc + b * kMx8Block + sub * 8) = mx8_encode8(x, sb);
    if (sub == 0) scales[it] = (unsigned char)sb;
  }
}

struct Mx8Args {
  const unsigned char* A; int64_t lda; const unsigned char* As;      // activation codes [M][K], scales [M][K / 32]
  const unsigned char* W; int64_t ldw; const unsigned char* Ws;      // weight codes [N (2 N)][K], scales
  bf16_t* C; int64_t ldc;
  int64_t M, N, K;                                                    // N = output columns (SWIGLU: W has 2 N rows)
  const bf16_t* bias; const bf16_t* R; int64_t ldr;
  int tiles_m, tiles_n;
};

constexpr int BKB = 128;                                              // bytes (= elements) of a code row per K-step

// physical slot = logical slot ^ swz(row): see the header comment
__device__ __forceinline__ int swz(int row) { return (row >> 1) & 7; }

__device__ __forceinline__ void unpack4(const u32x2 v, float (&f)[4]) {
  f[0] = bf16lo_to_f32(v[0]); f[1] = bf16hi_to_f32(v[0]); f[2] = bf16lo_to_f32(v[1]); f[3] = bf16hi_to_f32(v[1]);
}

// four consecutive output columns n .. n + 3 of row m; the rounding chains are vita_gemm_bf16's (include/vita_hip.h)
template <int EPI>
__device__ __forceinline__ void store_quad(const Mx8Args& p, const f32x4 v, const f32x4 up, int64_t m, int64_t n) {
  float o[4] = {v[0], v[1], v[2], v[3]};
  if (EPI == VITA_EPI_SWIGLU) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float g = bf16_round(o[j]);
      const float u = bf16_round(up[j]);
      o[j] = bf16_round(g / (1.0f + __expf(-g))) * u;
    }
  }
  if ((EPI == VITA_EPI_BIAS || EPI == VITA_EPI_RESIDUAL) && p.bias) {
    float b[4];
    unpack4(*reinterpret_cast<const u32x2*>(p.bias + n), b);
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] += b[j];
  }
  if (EPI == VITA_EPI_RESIDUAL) {
    float r[4];
    unpack4(*reinterpret_cast<const u32x2*>(p.R + m * p.ldr + n), r);
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = bf16_round(o[j]) + r[j];
  }
  const u32x2 w = {pack_bf16x2(o[0], o[1]), pack_bf16x2(o[2], o[3])};
  *reinterpret_cast<u32x2*>(p.C + m * p.ldc + n) = w;
}

template <int EPI, int BM, int BN, int WM, int WN>
__global__ __launch_bounds__(64 * WM * WN, 2) void gemm_mx8_kernel(Mx8Args p) {
  constexpr int NW = WM * WN;
  constexpr int TM = BM / WM, TN = BN / WN;          // per-wave tile
  constexpr int MI = TM / 16, NI = TN / 16;          // 16 x 16 blocks per wave
  constexpr int A_BYTES = BM * BKB, W_BYTES = BN * BKB, SC_OFF = A_BYTES + W_BYTES, STAGE = SC_OFF + (BM + BN) * 4;
  constexpr int QA = BM / 8 / NW, QW = BN / 8 / NW;  // 1-KiB DMA pieces per wave per operand
  constexpr int SP = (BM + BN) / 64;                 // 256-byte scale pieces per stage: piece sp is wave sp % NW's
  static_assert(EPI != VITA_EPI_SWIGLU || NI % 2 == 0, "SwiGLU pairs 16-column blocks (gate, up) of a wave");
  static_assert(SP <= NW, "at most one scale piece per wave");

  extern __shared__ __attribute__((aligned(16))) char smem[];
  const unsigned lds0 = (unsigned)(uintptr_t)(lds_char*)smem;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WN, wn = wave % WN;

  // ---- XCD-aware, grouped tile order (gemm.hip's) ---------------------------------------------------------------------------------
  const int nwg = p.tiles_m * p.tiles_n;
  int pid;
  {
    const int bid = blockIdx.x, xcd = bid & 7, q = nwg >> 3, r = nwg & 7;
    pid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
  }
  constexpr int GROUP_M = (BM == 256) ? 4 : 8;
  const int per_group = GROUP_M * p.tiles_n;
  const int group = pid / per_group;
  const int first_m = group * GROUP_M;
  const int gsz = min(p.tiles_m - first_m, GROUP_M);
  const int in_group = pid - group * per_group;
  const int tm = first_m + in_group % gsz;
  const int tn = in_group / gsz;
  const int64_t m0 = (int64_t)tm * BM;
  const int64_t n0 = (int64_t)tn * (EPI == VITA_EPI_SWIGLU ? BN / 2 : BN);      // output-column origin

  // W row behind tile row lr.  SWIGLU: 16-row blocks alternate gate / up of the same 16 output columns
  auto w_row = [&](int lr) __attribute__((always_inline)) {
    if (EPI == VITA_EPI_SWIGLU) {
      const int blk = lr >> 4;
      int64_t oc = n0 + (blk >> 1) * 16 + (lr & 15);
      oc = oc < p.N ? oc : p.N - 1;
      return ((blk & 1) ? p.N : 0) + oc;
    }
    const int64_t g = n0 + lr;
    return g < p.N ? g : p.N - 1;
  };

  // ---- DMA sources: a wave-instruction moves 8 tile rows (1 KiB); lane -> (row rbase + lane / 8, physical slot lane & 7) ----------
  const unsigned char* a_src[QA];
  const unsigned char* w_src[QW];
#pragma unroll
  for (int q = 0; q < QA; ++q) {
    const int lr = (wave * QA + q) * 8 + (lane >> 3);
    int64_t g = m0 + lr;
    g = g < p.M ? g : p.M - 1;
    a_src[q] = p.A + g * p.lda + (((lane & 7) ^ swz(lr)) << 4);
  }
#pragma unroll
  for (int q = 0; q < QW; ++q) {
    const int lr = (wave * QW + q) * 8 + (lane >> 3);
    w_src[q] = p.W + w_row(lr) * p.ldw + (((lane & 7) ^ swz(lr)) << 4);
  }
  // scale piece `wave` (if < SP): 64 rows x 4 bytes; pieces 0 .. BM / 64 - 1 are A's, the rest W's
  const int64_t nblk = p.K >> 5;
  const unsigned char* s_src = nullptr;
  if (wave < SP) {
    const int lr = wave * 64 + lane;
    if (lr < BM) {
      int64_t g = m0 + lr;
      g = g < p.M ? g : p.M - 1;
      s_src = p.As + g * nblk;
    } else {
      s_src = p.Ws + w_row(lr - BM) * nblk;
    }
  }
  auto stage = [&](unsigned sl) __attribute__((always_inline)) {
#pragma unroll
    for (int q = 0; q < QA; ++q) {
      __builtin_amdgcn_global_load_lds((gbl_cvoid*)a_src[q], (lds_void*)(uintptr_t)(sl + (wave * QA + q) * 1024), 16, 0, 0);
      a_src[q] += BKB;
    }
#pragma unroll
    for (int q = 0; q < QW; ++q) {
      __builtin_amdgcn_global_load_lds((gbl_cvoid*)w_src[q], (lds_void*)(uintptr_t)(sl + A_BYTES + (wave * QW + q) * 1024), 16, 0, 0);
      w_src[q] += BKB;
    }
    if (wave < SP) {
      __builtin_amdgcn_global_load_lds((gbl_cvoid*)s_src, (lds_void*)(uintptr_t)(sl + SC_OFF + wave * 256), 4, 0, 0);
      s_src += 4;
    }
  };

  // ---- per-lane fragment offsets: row l & 15 of the wave's first block (+ 16-row blocks as immediates), slots q and q + 4 -------------
  const int fr = lane & 15, fq = lane >> 4;
  const unsigned fa0 = (wm * TM + fr) * BKB + ((fq ^ swz(fr)) << 4);
  const unsigned fa1 = (wm * TM + fr) * BKB + (((fq + 4) ^ swz(fr)) << 4);
  const unsigned fw0 = A_BYTES + (wn * TN + fr) * BKB + ((fq ^ swz(fr)) << 4);
  const unsigned fw1 = A_BYTES + (wn * TN + fr) * BKB + (((fq + 4) ^ swz(fr)) << 4);
  const unsigned fsa = SC_OFF + (wm * TM + fr) * 4 + fq;
  const unsigned fsw = SC_OFF + (BM + wn * TN + fr) * 4 + fq;

  f32x4 acc[NI][MI];
#pragma unroll
  for (int i = 0; i < NI; ++i)
#pragma unroll
    for (int j = 0; j < MI; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nk = (int)(p.K / BKB);
  stage(lds0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  for (int t = 0; t < nk; ++t) {
    const unsigned cur = lds0 + (t & 1) * STAGE;
    if (t + 1 < nk) stage(lds0 + ((t + 1) & 1) * STAGE);
    i32x8 wf[NI];
    int ws[NI];
#pragma unroll
    for (int ni = 0; ni < NI; ++ni) {
      const u32x4 lo = *(lds_u32x4*)(uintptr_t)(cur + fw0 + ni * 16 * BKB);
      const u32x4 hi = *(lds_u32x4*)(uintptr_t)(cur + fw1 + ni * 16 * BKB);
      wf[ni] = i32x8{(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3], (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
      ws[ni] = *(lds_u8*)(uintptr_t)(cur + fsw + ni * 64);
    }
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) {
      const u32x4 lo = *(lds_u32x4*)(uintptr_t)(cur + fa0 + mi * 16 * BKB);
      const u32x4 hi = *(lds_u32x4*)(uintptr_t)(cur + fa1 + mi * 16 * BKB);
      const i32x8 af = i32x8{(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3], (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
      const int as = *(lds_u8*)(uintptr_t)(cur + fsa + mi * 64);
#pragma unroll
      for (int ni = 0; ni < NI; ++ni)
        acc[ni][mi] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(wf[ni], af, acc[ni][mi], 0, 0, 0, ws[ni], 0, as);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }

  // ---- epilogue: the lane holds columns 4 (l >> 4) .. + 3 of block ni for row l & 15 of block mi ----------------------------------
#pragma unroll
  for (int mi = 0; mi < MI; ++mi) {
    const int64_t m = m0 + wm * TM + mi * 16 + fr;
    if (m >= p.M) continue;
    if (EPI == VITA_EPI_SWIGLU) {
#pragma unroll
      for (int pi = 0; pi < NI / 2; ++pi) {
        const int64_t n = n0 + (wn * (NI / 2) + pi) * 16 + fq * 4;
        if (n < p.N) store_quad<EPI>(p, acc[2 * pi][mi], acc[2 * pi + 1][mi], m, n);
      }
    } else {
#pragma unroll
      for (int ni = 0; ni < NI; ++ni) {
        const int64_t n = n0 + wn * TN + ni * 16 + fq * 4;
        if (n < p.N) store_quad<EPI>(p, acc[ni][mi], acc[ni][mi], m, n);
      }
    }
  }
}

template <int EPI, int BM, int BN, int WM, int WN>
int launch_mx8_cfg(Mx8Args a, hipStream_t st) {
  constexpr int lds = 2 * ((BM + BN) * BKB + (BM + BN) * 4);
  const int64_t tm = (a.M + BM - 1) / BM;
  const int64_t bn_out = EPI == VITA_EPI_SWIGLU ? BN / 2 : BN;
  const int64_t tn = (a.N + bn_out - 1) / bn_out;
  if (tm * tn > 0x7fffffff) return VITA_ERR_UNSUPPORTED;
  a.tiles_m = (int)tm; a.tiles_n = (int)tn;
  static std::atomic<unsigned long long> attr_set{0};
  vita_device_once(attr_set, [&] {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&gemm_mx8_kernel<EPI, BM, BN, WM, WN>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, lds);
  });
  hipLaunchKernelGGL((gemm_mx8_kernel<EPI, BM, BN, WM, WN>), dim3((unsigned)(tm * tn)), dim3(64 * WM * WN), lds, st, a);
  return vita_check_launch();
}

// The 256 x 256 tile where it fills the chip with whole tiles (N a multiple of its width), the 128 x 128 tile everywhere else.  Both run
// the same per-element chain, so the choice moves no bit.
template <int EPI>
int launch_mx8(const Mx8Args& a, hipStream_t st) {
  const int64_t bn_out = EPI == VITA_EPI_SWIGLU ? 128 : 256;
  const bool big = a.N % bn_out == 0 && ((a.M + 255) / 256) * (a.N / bn_out) >= 192;
  return big ? launch_mx8_cfg<EPI, 256, 256, 2, 4>(a, st) : launch_mx8_cfg<EPI, 128, 128, 2, 2>(a, st);
}

}  // namespace

extern "C" int vita_mx8_quantize(const void* X, int64_t ldx, int64_t rows, int64_t K, void* codes, int64_t ldc_bytes, void* scales,
                                 void* stream) {
  if (!X || !codes || !scales || rows <= 0 || K <= 0) return VITA_ERR_INVALID_ARG;
  if ((K & (kMx8Block - 1)) || K >= (int64_t(1) << 31) || (ldc_bytes & 15) || ldc_bytes < K || ((uintptr_t)codes & 15) || (ldx & 7) ||
      ldx < K || ((uintptr_t)X & 15) || rows > (int64_t(1) << 40) / K)
    return VITA_ERR_UNSUPPORTED;
  const int64_t items = rows * (K / kMx8Block);                          // 4 lanes each, 64 per workgroup
  const unsigned blocks = (unsigned)((items + 63) / 64 < 8192 ? (items + 63) / 64 : 8192);
  hipLaunchKernelGGL(mx8_quantize_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)X, ldx, rows,
                     (int)(K / kMx8Block), (unsigned char*)codes, ldc_bytes, (unsigned char*)scales);
  return vita_check_launch();
}

extern "C" int vita_gemm_mx8(const void* A_codes, int64_t lda_bytes, const void* A_scales, const void* W_codes, int64_t ldw_bytes,
                             const void* W_scales, void* C, int64_t ldc, int64_t M, int64_t N, int64_t K, int epilogue,
                             const void* bias, const void* R, int64_t ldr, void* stream) {
  if (!A_codes || !A_scales || !W_codes || !W_scales || !C || M <= 0 || N <= 0 || K <= 0) return VITA_ERR_INVALID_ARG;
  if (epilogue != VITA_EPI_NONE && epilogue != VITA_EPI_BIAS && epilogue != VITA_EPI_RESIDUAL && epilogue != VITA_EPI_SWIGLU)
    return VITA_ERR_INVALID_ARG;
  if (epilogue == VITA_EPI_BIAS && !bias) return VITA_ERR_INVALID_ARG;
  if (epilogue == VITA_EPI_RESIDUAL && !R) return VITA_ERR_INVALID_ARG;
  if ((K % BKB) || (N % 128)) return VITA_ERR_UNSUPPORTED;
  if (K >= (int64_t(1) << 31) || N >= (int64_t(1) << 30) || M >= (int64_t(1) << 31)) return VITA_ERR_UNSUPPORTED;
  if ((lda_bytes & 15) || lda_bytes < K || (ldw_bytes & 15) || ldw_bytes < K || ((uintptr_t)A_codes & 15) || ((uintptr_t)W_codes & 15) ||
      ((uintptr_t)A_scales & 3) || ((uintptr_t)W_scales & 3))
    return VITA_ERR_UNSUPPORTED;
  if ((ldc & 3) || ldc < N || ((uintptr_t)C & 7)) return VITA_ERR_UNSUPPORTED;
  const bool reads_bias = (epilogue == VITA_EPI_BIAS || epilogue == VITA_EPI_RESIDUAL) && bias;
  if (reads_bias && ((uintptr_t)bias & 7)) return VITA_ERR_UNSUPPORTED;
  if (epilogue == VITA_EPI_RESIDUAL && ((ldr & 3) || ldr < N || ((uintptr_t)R & 7))) return VITA_ERR_UNSUPPORTED;
  Mx8Args a;
  a.A = (const unsigned char*)A_codes; a.lda = lda_bytes; a.As = (const unsigned char*)A_scales;
  a.W = (const unsigned char*)W_codes; a.ldw = ldw_bytes; a.Ws = (const unsigned char*)W_scales;
  a.C = (bf16_t*)C; a.ldc = ldc; a.M = M; a.N = N; a.K = K;
  a.bias = (const bf16_t*)bias; a.R = (const bf16_t*)R; a.ldr = ldr;
  a.tiles_m = a.tiles_n = 0;
  hipStream_t st = (hipStream_t)stream;
  switch (epilogue) {
    case VITA_EPI_NONE: return launch_mx8<VITA_EPI_NONE>(a, st);
    case VITA_EPI_BIAS: return launch_mx8<VITA_EPI_BIAS>(a, st);
    case VITA_EPI_RESIDUAL: return launch_mx8<VITA_EPI_RESIDUAL>(a, st);
    default: return launch_mx8<VITA_EPI_SWIGLU>(a, st);
  }
}
