// FP8 (OCP e4m3fn) KV cache for the cached decode: the quantising store, the split decode attention over codes +
// scales, and the de-quantising load that hands rows back as bf16 (x~_i = bf16_rne(f32(c_i) * s), kv8_rule.h) to the one-pass extend
// of a follow-up turn, whose attention kernel reads bf16 K / V.  One rule for every kernel here and for tests/kv8_cases.py, per K or V head row x[0..127] (bf16, K after
// RoPE) of one (cache row, kv group):
//   amax = max |x_i| (a NaN in the row makes amax NaN) ; s = amax > 0 ? amax / 448 : 1 ; c_i = e4m3fn_rne(x_i / s) ; x^_i = f32(c_i) * s
// fp32, IEEE division, no clamp: x / s reaches at most 448 (1 + 2^-23), which rounds to 448; a non-finite element leaves non-finite
// de-quantised values in its row (NaN: s = 1 and the element's code is NaN; inf: s = inf, 0 * inf and NaN * inf).
// Every e4m3 value is a bf16 value, so the attention below is decode.hip's arithmetic on codes: s_k multiplies the finished dot
// product, s_v multiplies p in front of P.V; (m, l, O) partials, split geometry and the neutral element are decode.hip's, and
// vita_decode_attn_merge takes them as they are.
#include "vita_common.h"
#include "kv8_rule.h"

#include <math.h>

namespace {

// ---- quantising store: item = (row r, group g, K or V); its 16 lanes hold 8 elements each ------------------------------------------
// rows outside [row0, row0 + rows) are not touched; a row0 (host or device) that would leave the cache writes nothing.
__global__ __launch_bounds__(256) void kv8_store_kernel(const bf16_t* __restrict__ k_src, const bf16_t* __restrict__ v_src,
                                                        int64_t src_row_stride, int64_t src_group_stride, int64_t rows, int groups,
                                                        unsigned char* __restrict__ kc, unsigned char* __restrict__ vc,
                                                        int64_t code_row_stride, int64_t code_group_stride,
                                                        float* __restrict__ ks, float* __restrict__ vs, int64_t scale_row_stride,
                                                        int64_t scale_group_stride, int64_t row0, const int64_t* __restrict__ row0_dev,
                                                        int64_t capacity) {
  if (row0_dev) row0 = *row0_dev;
  if (row0 < 0 || row0 + rows > capacity) return;
  const int sub = threadIdx.x & 15;
  const int64_t items = rows * groups * 2;
  for (int64_t it = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 4; it < items; it += ((int64_t)gridDim.x * blockDim.x) >> 4) {
    const int kv = (int)(it & 1);
    const int g = (int)((it >> 1) % groups);
    const int64_t r = (it >> 1) / groups;
    const bf16_t* src = (kv ? v_src : k_src) + r * src_row_stride + (int64_t)g * src_group_stride + sub * 8;
    const u32x4 x = *reinterpret_cast<const u32x4*>(src);
    unsigned m = kv8_absmax_bits(x);
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) m = max(m, (unsigned)__shfl_xor((int)m, o));
    const float s = kv8_scale(m);
    const u32x2 c = kv8_encode8(x, s);
    *reinterpret_cast<u32x2*>((kv ? vc : kc) + (row0 + r) * code_row_stride + (int64_t)g * code_group_stride + sub * 8) = c;
    if (sub == 0) (kv ? vs : ks)[(row0 + r) * scale_row_stride + (int64_t)g * scale_group_stride] = s;
  }
}

// ---- de-quantising load: the store's mirror, item = (row r, group g, K or V) on 16 lanes x 8 elements ------------------------------
// one 8-byte code load + one broadcast 4-byte scale load, kv8_readback8, one 16-byte store: 132 B in and 256 B out per item, HBM-bound.
// Nothing outside rows [0, rows) is read or written, the padding between rows and groups included.
__global__ __launch_bounds__(256) void kv8_load_kernel(const unsigned char* __restrict__ kc, const unsigned char* __restrict__ vc,
                                                       int64_t code_row_stride, int64_t code_group_stride,
                                                       const float* __restrict__ ks, const float* __restrict__ vs,
                                                       int64_t scale_row_stride, int64_t scale_group_stride, int64_t rows, int groups,
                                                       bf16_t* __restrict__ k_dst, bf16_t* __restrict__ v_dst, int64_t dst_row_stride,
                                                       int64_t dst_group_stride) {
  const int sub = threadIdx.x & 15;
  const int64_t items = rows * groups * 2;
  for (int64_t it = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 4; it < items; it += ((int64_t)gridDim.x * blockDim.x) >> 4) {
    const int kv = (int)(it & 1);
    const int g = (int)((it >> 1) % groups);
    const int64_t r = (it >> 1) / groups;
    const u32x2 c = *reinterpret_cast<const u32x2*>((kv ? vc : kc) + r * code_row_stride + (int64_t)g * code_group_stride + sub * 8);
    const float s = (kv ? vs : ks)[r * scale_row_stride + (int64_t)g * scale_group_stride];
    *reinterpret_cast<u32x4*>((kv ? v_dst : k_dst) + r * dst_row_stride + (int64_t)g * dst_group_stride + sub * 8) = kv8_readback8(c, s);
  }
}

// ---- RoPE of the new token's q and k heads (in place in the mixed qkv row) + quantised append of its K / V ---------------------------
// decode.hip's rope_append_kernel with the rule behind the rotation: the 8 lanes of one head (two 8-wide vectors each) share the maximum.
__global__ __launch_bounds__(256) void rope_append_kv8_kernel(bf16_t* __restrict__ mixed, int groups, int qpg, int head_dim,
                                                              const bf16_t* __restrict__ cos_tab, const bf16_t* __restrict__ sin_tab,
                                                              unsigned char* __restrict__ kc, unsigned char* __restrict__ vc,
                                                              int64_t code_row_stride, int64_t code_group_stride,
                                                              float* __restrict__ ks, float* __restrict__ vs, int64_t scale_row_stride,
                                                              int64_t scale_group_stride, int append_row) {
  const int half = head_dim >> 1, nv = half >> 3, hpg = qpg + 2;       // head_dim 128: nv = 8, a head's lanes are 8 aligned neighbours
  const int total = groups * hpg * nv;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const int vi = i % nv, h = (i / nv) % hpg, g = i / (nv * hpg);
    bf16_t* p = mixed + ((int64_t)g * hpg + h) * head_dim + vi * 8;
    u32x4 x1 = *reinterpret_cast<const u32x4*>(p);
    u32x4 x2 = *reinterpret_cast<const u32x4*>(p + half);
    if (h <= qpg) {
      const u32x4 c = *reinterpret_cast<const u32x4*>(cos_tab + vi * 8);
      const u32x4 s = *reinterpret_cast<const u32x4*>(sin_tab + vi * 8);
      rope_rotate8(x1, x2, c, s, 1.0f);
      *reinterpret_cast<u32x4*>(p) = x1;
      *reinterpret_cast<u32x4*>(p + half) = x2;
    }
    if (h >= qpg && append_row >= 0) {                                 // h is the same in the 8 lanes of a head: they are all here
      unsigned m = max(kv8_absmax_bits(x1), kv8_absmax_bits(x2));
#pragma unroll
      for (int o = 1; o < 8; o <<= 1) m = max(m, (unsigned)__shfl_xor((int)m, o));
      const float s = kv8_scale(m);
      const bool is_k = h == qpg;
      unsigned char* o8 = (is_k ? kc : vc) + (int64_t)append_row * code_row_stride + (int64_t)g * code_group_stride + vi * 8;
      *reinterpret_cast<u32x2*>(o8) = kv8_encode8(x1, s);
      *reinterpret_cast<u32x2*>(o8 + half) = kv8_encode8(x2, s);
      if (vi == 0) (is_k ? ks : vs)[(int64_t)append_row * scale_row_stride + (int64_t)g * scale_group_stride] = s;
    }
  }
}

// ---- decode attention, stage 1, on codes + scales ----------------------------------------------------------------------------------
// decode.hip's decode_attn_partial_kernel: the same split geometry, lane map (16 lanes per row, lane sub owns dims 8 sub .. 8 sub + 7,
// now one 8-byte load), rows in flight, online softmax and end-of-kernel merge.  Per row one more broadcast 4-byte load per tensor:
// its scale, fetched with the row.  Codes are converted with v_cvt_pk_f32_fp8 and repacked to bf16 pairs for v_dot2_f32_bf16.
// The launch is VALU-bound at qpg >= 4 (profiles/r15_kv8.jsonl), so the loop spends no instruction it can save: no branch around
// the loads (a key behind the range reads the range's last row and gets probability 0), 32-bit row strides (one v_mad_u64_u32 per
// address), the K scale folded into the softmax scale once per row.  Four-row tiles at 3 waves per SIMD were 35 % slower at qpg 5.
constexpr int kDecKeys = 128;        // as decode.hip (host side: ops.DECODE_KEYS_PER_TILE)

template <int QPG>
__global__ __launch_bounds__(256, 2) void decode_attn_partial_kv8_kernel(
    const bf16_t* __restrict__ q, int64_t q_group_stride, int64_t q_head_stride, const unsigned char* __restrict__ kc,
    const unsigned char* __restrict__ vc, int64_t code_row_stride, int64_t code_group_stride, const float* __restrict__ ks,
    const float* __restrict__ vs, int64_t scale_row_stride, int64_t scale_group_stride, int len, const int* __restrict__ len_dev,
    float scale_log2, float* __restrict__ pm, float* __restrict__ pl, float* __restrict__ po) {
  constexpr int D = 128;
  constexpr int ITS = QPG >= 7 ? 4 : 8;                   // K/V row loads in flight per lane (register budget)
  constexpr int kWaveKeys = ITS * 4;
  __shared__ float wm[4][QPG], wl[4][QPG];
  __shared__ float wo[4][QPG][D];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int sub = lane & 15, kq = lane >> 4;
  const int blk = blockIdx.x, g = blockIdx.y;
  const int H = gridDim.y * QPG;
  if (len_dev) len = min(len, *len_dev);                  // row count kept on the device (graph replay)
  const int ntiles = (len + kDecKeys - 1) / kDecKeys;
  const int tiles_per_wg = (ntiles + (int)gridDim.x - 1) / (int)gridDim.x;
  const int key_begin = blk * tiles_per_wg * kDecKeys;
  const int key_end = min(len, key_begin + tiles_per_wg * kDecKeys);
  if (key_begin >= len) {                                 // empty split: neutral element of the merge
    if (t < QPG) { pm[(int64_t)blk * H + g * QPG + t] = -INFINITY; pl[(int64_t)blk * H + g * QPG + t] = 0.f; }
    if (t < D)
      for (int h = 0; h < QPG; ++h) po[((int64_t)blk * H + g * QPG + h) * D + t] = 0.f;
    return;
  }

  unsigned qp[QPG][4];                                    // packed bf16 pairs, consumed by v_dot2_f32_bf16
#pragma unroll
  for (int h = 0; h < QPG; ++h) {
    const u32x4 qv = *reinterpret_cast<const u32x4*>(q + g * q_group_stride + h * q_head_stride + sub * 8);
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
  const unsigned char* kbase = kc + g * code_group_stride + sub * 8;
  const unsigned char* vbase = vc + g * code_group_stride + sub * 8;
  const float* ksbase = ks + g * scale_group_stride;
  const float* vsbase = vs + g * scale_group_stride;
  const unsigned crs = (unsigned)code_row_stride, srs = (unsigned)scale_row_stride;      // < 2^31: checked by the launcher

  for (int key0 = key_begin + wave * kWaveKeys; key0 < key_end; key0 += 4 * kWaveKeys) {
    u32x2 kr[ITS], vr[ITS];
    float ksc[ITS], vsc[ITS];
#pragma unroll
    for (int it = 0; it < ITS; ++it) {
      // a key behind the range reads the range's last row instead (no branch around the loads, nothing read outside the rows the
      // launch owns); its score is set to -inf below, so p = 0 and the row adds 0 * v
      const int key = min(key0 + it * 4 + kq, key_end - 1);
      const uint64_t coff = (uint64_t)(unsigned)key * crs, soff = (uint64_t)(unsigned)key * srs;     // one v_mad_u64_u32 each
      kr[it] = *reinterpret_cast<const u32x2*>(kbase + coff);
      vr[it] = *reinterpret_cast<const u32x2*>(vbase + coff);
      ksc[it] = ksbase[soff] * scale_log2;
      vsc[it] = vsbase[soff];
    }
    float sc[QPG][ITS];
#pragma unroll
    for (int it = 0; it < ITS; ++it) {
      unsigned kp[4];
      kv8_decode4(kr[it][0], kp[0], kp[1]);
      kv8_decode4(kr[it][1], kp[2], kp[3]);
#pragma unroll
      for (int h = 0; h < QPG; ++h) {
        float sv = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) sv = dot2_bf16(qp[h][j], kp[j], sv);
        sc[h][it] = sv;
      }
    }
    float p[QPG][ITS];
#pragma unroll
    for (int h = 0; h < QPG; ++h) {
      float tm = -INFINITY;
#pragma unroll
      for (int it = 0; it < ITS; ++it) {
        float sv = row16_allreduce_sum(sc[h][it]) * ksc[it];
        sv = (key0 + it * 4 + kq < key_end) ? sv : -INFINITY;
        p[h][it] = sv;
        tm = fmaxf(tm, sv);
      }
      tm = fmaxf(tm, __shfl_xor(tm, 16));
      tm = fmaxf(tm, __shfl_xor(tm, 32));                  // finite: key0 < key_end
      const float mnew = fmaxf(mrun[h], tm);
      const float alpha = __builtin_amdgcn_exp2f(mrun[h] - mnew);        // exp2(-inf) = 0 on the first tile
      mrun[h] = mnew;
      float ls = 0.f;
#pragma unroll
      for (int it = 0; it < ITS; ++it) {
        p[h][it] = __builtin_amdgcn_exp2f(p[h][it] - mnew);
        ls += p[h][it];
      }
      lrun[h] = lrun[h] * alpha + ls;                      // this row-group's keys only; summed over kq at the end
#pragma unroll
      for (int i = 0; i < 8; ++i) acc[h][i] *= alpha;
    }
#pragma unroll
    for (int it = 0; it < ITS; ++it) {
      float vf[8];
#pragma unroll
      for (int w = 0; w < 2; ++w) {
        const auto lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)vr[it][w], false);
        const auto hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)vr[it][w], true);
        vf[4 * w] = lo[0]; vf[4 * w + 1] = lo[1]; vf[4 * w + 2] = hi[0]; vf[4 * w + 3] = hi[1];
      }
#pragma unroll
      for (int h = 0; h < QPG; ++h) {
        const float ps = p[h][it] * vsc[it];
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[h][i] += ps * vf[i];
      }
    }
  }
  // wave result: sum the 4 row-groups (lanes sub, sub+16, sub+32, sub+48 hold the same dims)
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
      po[((int64_t)blk * H + g * QPG + h) * D + t] = O;
      // A non-finite K / V row makes L and O NaN.  vita_decode_attn_merge writes O / L only where L > 0 and 0 elsewhere, which
      // would turn that NaN into a zero context: a NaN sum goes out as +inf, so that the merge divides and the NaN of O shows.
      if (t == 0) { pm[(int64_t)blk * H + g * QPG + h] = M; pl[(int64_t)blk * H + g * QPG + h] = (L == L) ? L : INFINITY; }
    }
  }
}

bool kv8_cache_ok(const void* kc, const void* vc, int64_t code_row_stride, int64_t code_group_stride, const void* ks, const void* vs,
                  int* rc) {
  if (!kc || !vc || !ks || !vs) { *rc = VITA_ERR_INVALID_ARG; return false; }
  if ((code_row_stride & 7) || (code_group_stride & 7) || (((uintptr_t)kc | (uintptr_t)vc) & 7) ||
      (((uintptr_t)ks | (uintptr_t)vs) & 3)) {                          // 8-byte code vectors, 4-byte scales
    *rc = VITA_ERR_UNSUPPORTED;
    return false;
  }
  return true;
}

}  // namespace

extern "C" int vita_kv8_store(const void* k_src, const void* v_src, int64_t src_row_stride, int64_t src_group_stride, int64_t rows,
                              int groups, int head_dim, void* k_codes, void* v_codes, int64_t code_row_stride,
                              int64_t code_group_stride, void* k_scales, void* v_scales, int64_t scale_row_stride,
                              int64_t scale_group_stride, int64_t row0, const void* row0_dev, int64_t capacity, void* stream) {
  if (!k_src || !v_src || rows <= 0 || groups <= 0 || capacity <= 0) return VITA_ERR_INVALID_ARG;
  int rc = VITA_OK;
  if (!kv8_cache_ok(k_codes, v_codes, code_row_stride, code_group_stride, k_scales, v_scales, &rc)) return rc;
  if (!row0_dev && (row0 < 0 || row0 + rows > capacity)) return VITA_ERR_INVALID_ARG;
  if (rows > capacity) return VITA_ERR_INVALID_ARG;
  if (head_dim != 128 || (src_row_stride & 7) || (src_group_stride & 7) || (((uintptr_t)k_src | (uintptr_t)v_src) & 15) ||
      (((uintptr_t)row0_dev) & 7) || rows * groups > (int64_t(1) << 40))
    return VITA_ERR_UNSUPPORTED;
  const int64_t items = rows * groups * 2;                               // 16 lanes each, 16 per workgroup
  const unsigned blocks = (unsigned)((items + 15) / 16 < 4096 ? (items + 15) / 16 : 4096);
  hipLaunchKernelGGL(kv8_store_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)k_src, (const bf16_t*)v_src,
                     src_row_stride, src_group_stride, rows, groups, (unsigned char*)k_codes, (unsigned char*)v_codes,
                     code_row_stride, code_group_stride, (float*)k_scales, (float*)v_scales, scale_row_stride, scale_group_stride,
                     row0, (const int64_t*)row0_dev, capacity);
  return vita_check_launch();
}

extern "C" int vita_kv8_load(const void* k_codes, const void* v_codes, int64_t code_row_stride, int64_t code_group_stride,
                             const void* k_scales, const void* v_scales, int64_t scale_row_stride, int64_t scale_group_stride,
                             int64_t rows, int groups, int head_dim, void* k_dst, void* v_dst, int64_t dst_row_stride,
                             int64_t dst_group_stride, void* stream) {
  if (!k_dst || !v_dst || rows <= 0 || groups <= 0) return VITA_ERR_INVALID_ARG;
  int rc = VITA_OK;
  if (!kv8_cache_ok(k_codes, v_codes, code_row_stride, code_group_stride, k_scales, v_scales, &rc)) return rc;
  if (head_dim != 128 || (dst_row_stride & 7) || (dst_group_stride & 7) || (((uintptr_t)k_dst | (uintptr_t)v_dst) & 15) ||
      rows > (int64_t(1) << 40) || rows * groups > (int64_t(1) << 40))
    return VITA_ERR_UNSUPPORTED;
  const int64_t items = rows * groups * 2;                               // 16 lanes each, 16 per workgroup
  const unsigned blocks = (unsigned)((items + 15) / 16 < 4096 ? (items + 15) / 16 : 4096);
  hipLaunchKernelGGL(kv8_load_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const unsigned char*)k_codes,
                     (const unsigned char*)v_codes, code_row_stride, code_group_stride, (const float*)k_scales, (const float*)v_scales,
                     scale_row_stride, scale_group_stride, rows, groups, (bf16_t*)k_dst, (bf16_t*)v_dst, dst_row_stride,
                     dst_group_stride);
  return vita_check_launch();
}

extern "C" int vita_decode_attn_partial_kv8(const void* q, int64_t q_group_stride, int64_t q_head_stride, const void* k_codes,
                                            const void* v_codes, int64_t code_row_stride, int64_t code_group_stride,
                                            const void* k_scales, const void* v_scales, int64_t scale_row_stride,
                                            int64_t scale_group_stride, int len, const void* len_dev, int n_splits, int groups,
                                            int qpg, int head_dim, float softmax_scale, void* part_m, void* part_l, void* part_o,
                                            void* stream) {
  if (!q || !part_m || !part_l || !part_o || len <= 0 || groups <= 0 || n_splits <= 0) return VITA_ERR_INVALID_ARG;
  int rc = VITA_OK;
  if (!kv8_cache_ok(k_codes, v_codes, code_row_stride, code_group_stride, k_scales, v_scales, &rc)) return rc;
  if (head_dim != 128 || qpg < 1 || qpg > 8 || (q_group_stride & 7) || (q_head_stride & 7) || ((uintptr_t)q & 15) ||
      ((uintptr_t)len_dev & 3) || code_row_stride < 0 || code_row_stride >= (int64_t(1) << 31) || scale_row_stride < 0 ||
      scale_row_stride >= (int64_t(1) << 31))                             // the kernel multiplies rows by 32-bit strides
    return VITA_ERR_UNSUPPORTED;
  dim3 grid((unsigned)n_splits, (unsigned)groups), block(256);
  hipStream_t st = (hipStream_t)stream;
  const float sl2 = softmax_scale * 1.4426950408889634f;
#define VITA_DEC8(Q)                                                                                                            \
  case Q:                                                                                                                       \
    hipLaunchKernelGGL(decode_attn_partial_kv8_kernel<Q>, grid, block, 0, st, (const bf16_t*)q, q_group_stride, q_head_stride,  \
                       (const unsigned char*)k_codes, (const unsigned char*)v_codes, code_row_stride, code_group_stride,        \
                       (const float*)k_scales, (const float*)v_scales, scale_row_stride, scale_group_stride, len,               \
                       (const int*)len_dev, sl2, (float*)part_m, (float*)part_l, (float*)part_o);                               \
    break;
  switch (qpg) {
    VITA_DEC8(1) VITA_DEC8(2) VITA_DEC8(3) VITA_DEC8(4) VITA_DEC8(5) VITA_DEC8(6) VITA_DEC8(7) VITA_DEC8(8)
  }
#undef VITA_DEC8
  return vita_check_launch();
}

// the fused layer entry's second kernel (decode.hip: vita_decode_layer_attn_kv8); arguments checked by the caller
int vita_kv8_rope_append(void* qkv, int groups, int qpg, int head_dim, const void* cos_tab, const void* sin_tab,
                         const vita_kv8_cache* c, int append_row, hipStream_t stream) {
  hipLaunchKernelGGL(rope_append_kv8_kernel, dim3(4), dim3(256), 0, stream, (bf16_t*)qkv, groups, qpg, head_dim,
                     (const bf16_t*)cos_tab, (const bf16_t*)sin_tab, (unsigned char*)c->k_codes, (unsigned char*)c->v_codes,
                     c->code_row_stride, c->code_group_stride, (float*)c->k_scales, (float*)c->v_scales, c->scale_row_stride,
                     c->scale_group_stride, append_row);
  return vita_check_launch();
}
