// mx8_map — operand and scale maps of v_mfma_scale_f32_16x16x128_f8f6f4 with e4m3 operands (gfx950), pinned with exact integer data.
//
//   hipcc --offload-arch=gfx950 -O3 mx8_map.hip -o bin/mx8_map && bin/mx8_map > profiles/r27_mx8_map.txt
//
// One wave per case.  The kernel hands lane l (r = l & 15, q = l >> 4) the bytes  X[r][16 q .. + 15]  in registers 0-3 and
// X[r][64 + 16 q .. + 15]  in registers 4-7 of each operand, and the lane's own 32-bit scale word.  (The first version of this probe
// handed out X[r][32 q .. + 31], "4 K lanes x 32 K elements per lane" read as one contiguous run: T1 passed — any K permutation
// shared by A and B does — and T2 showed a lane's scale reaching only 16 of those 32 elements.)  Everything else is decided on the host:
//   T1  data map   one-hot A (code 1.0) at every (row, k) against an asymmetric integer B, all scales 1: D must be row `row` = B[:, k]
//   T2  scale map  A = 1.0 on one 32-block, B = 1.0; the scale word of ONE lane doubled: which (row / column, block) doubles?
//   T3  both       dense small integers, a distinct power-of-two scale per (row, block) on both sides, exact against the host sum
//   T4  scale byte 0xFF, 0x00 and 0xFE; which byte of the scale word op_sel 0..3 reads
//   T5  e4m3 NaN codes 0x7F / 0xFF against finite and zero partners
//   T6  summation  2^24 + 31 ones - 2^24 inside one instruction, and against the C input: what survives?
// Exit status 0 = the hypothesis holds in T1-T3.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>

typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

struct Case {
  uint8_t a[16][128];     // A[row][k]
  uint8_t b[16][128];     // B[col][k]
  uint32_t sa[64], sb[64];   // scale word of lane l, as the instruction sees it
  float c[16][16];
  float d[16][16];
  int opsel;
};

template <int OPSEL>
__device__ f32x4 mfma(i32x8 a, i32x8 b, f32x4 c, int sa, int sb) {
  return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, c, 0, 0, OPSEL, sa, OPSEL, sb);
}

__global__ __launch_bounds__(64) void probe(Case* cases) {
  Case& cs = cases[blockIdx.x];
  const int l = threadIdx.x, r = l & 15, q = l >> 4;
  i32x8 a, b;
  for (int j = 0; j < 8; ++j) {
    const int k = (j < 4 ? 16 * q : 64 + 16 * q - 16) + 4 * j;
    a[j] = *reinterpret_cast<const int*>(&cs.a[r][k]);
    b[j] = *reinterpret_cast<const int*>(&cs.b[r][k]);
  }
  f32x4 c;
  for (int j = 0; j < 4; ++j) c[j] = cs.c[4 * q + j][r];       // C / D: column = lane & 15, row = 4 (lane >> 4) + j
  const int sa = (int)cs.sa[l], sb = (int)cs.sb[l];
  f32x4 d;
  switch (cs.opsel) {
    case 1: d = mfma<1>(a, b, c, sa, sb); break;
    case 2: d = mfma<2>(a, b, c, sa, sb); break;
    case 3: d = mfma<3>(a, b, c, sa, sb); break;
    default: d = mfma<0>(a, b, c, sa, sb); break;
  }
  for (int j = 0; j < 4; ++j) cs.d[4 * q + j][r] = d[j];
}

// e4m3fn code of an exactly representable normal value (or zero)
static uint8_t e4m3(float v) {
  if (v == 0.f) return 0;
  const uint8_t s = v < 0 ? 0x80 : 0;
  int e;
  const float m = frexpf(fabsf(v), &e);      // |v| = m 2^e, 0.5 <= m < 1
  const int mant = (int)(m * 16.f) - 8;      // 3 bits behind the leading one
  return s | (uint8_t)((e - 1 + 7) << 3) | (uint8_t)mant;
}
static void unit(Case& c) {
  memset(&c, 0, sizeof c);
  for (int l = 0; l < 64; ++l) c.sa[l] = c.sb[l] = 127;
}
static int bval(int n, int k) { return (k * 7 + n * 3 + (k >> 5)) % 17 - 8; }     // asymmetric, |.| <= 8

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__); return 2; } } while (0)

int main() {
  std::vector<Case> cs;
  // ---- T1 ----
  const int t1 = (int)cs.size();
  for (int r = 0; r < 16; ++r)
    for (int k = 0; k < 128; ++k) {
      Case c; unit(c);
      c.a[r][k] = e4m3(1.f);
      for (int n = 0; n < 16; ++n) for (int kk = 0; kk < 128; ++kk) c.b[n][kk] = e4m3((float)bval(n, kk));
      cs.push_back(c);
    }
  // ---- T2: side 0 = A scale word of lane l doubled, side 1 = B ----
  const int t2 = (int)cs.size();
  for (int side = 0; side < 2; ++side)
    for (int l = 0; l < 64; ++l)
      for (int blk = 0; blk < 4; ++blk) {
        Case c; unit(c);
        for (int r = 0; r < 16; ++r) for (int k = 32 * blk; k < 32 * blk + 32; ++k) { c.a[r][k] = e4m3(1.f); c.b[r][k] = e4m3(1.f); }
        (side ? c.sb : c.sa)[l] = 128;
        cs.push_back(c);
      }
  // ---- T3 ----
  const int t3 = (int)cs.size();
  for (int rep = 0; rep < 4; ++rep) {
    Case c; unit(c);
    uint32_t s = 12345u + rep;
    for (int r = 0; r < 16; ++r) for (int k = 0; k < 128; ++k) {
      s = s * 1664525u + 1013904223u; c.a[r][k] = e4m3((float)((int)((s >> 16) % 9) - 4));
      s = s * 1664525u + 1013904223u; c.b[r][k] = e4m3((float)((int)((s >> 16) % 9) - 4));
    }
    for (int l = 0; l < 64; ++l) {
      const int r = l & 15, q = l >> 4;
      c.sa[l] = 127 + (r * 3 + q + rep) % 7 - 3;
      c.sb[l] = 127 + (r + 2 * q + rep) % 5 - 2;
    }
    for (int r = 0; r < 16; ++r) for (int n = 0; n < 16; ++n) c.c[r][n] = (float)(r - 2 * n);
    cs.push_back(c);
  }
  // ---- T4: A = B = 1.0 on block 0 only, so row / column 0 reads the scale of lane 0 (if T2 says so) ----
  const int t4 = (int)cs.size();
  const char* t4name[] = {"sa[lane 0] = 0xFF", "sb[lane 0] = 0xFF", "sa[lane 0] = 0xFF, A row 0 all zero", "sa[lane 0] = 0x00", "sa[lane 0] = 0xFE",
                          "sa = sb = 0xFE everywhere", "sa word 0x83828180 op_sel 0", "op_sel 1", "op_sel 2", "op_sel 3",
                          "sa[lane 0] = 0x1FF (bits above the byte)"};
  for (int v = 0; v < 11; ++v) {
    Case c; unit(c);
    for (int r = 0; r < 16; ++r) for (int k = 0; k < 32; ++k) { c.a[r][k] = e4m3(1.f); c.b[r][k] = e4m3(1.f); }
    if (v == 0) c.sa[0] = 0xFF;
    if (v == 1) c.sb[0] = 0xFF;
    if (v == 2) { c.sa[0] = 0xFF; memset(c.a[0], 0, 128); }
    if (v == 3) c.sa[0] = 0;
    if (v == 4) c.sa[0] = 0xFE;
    if (v == 5) for (int l = 0; l < 64; ++l) c.sa[l] = c.sb[l] = 0xFE;
    if (v >= 6 && v <= 9) { for (int l = 0; l < 64; ++l) { c.sa[l] = 0x83828180u; c.sb[l] = 0x7F7F7F7Fu; } c.opsel = v - 6; }
    if (v == 10) c.sa[0] = 0x1FF;
    cs.push_back(c);
  }
  // ---- T5 ----
  const int t5 = (int)cs.size();
  const char* t5name[] = {"A[0][0] = 0x7F, B = 1.0", "A[0][0] = 0xFF, B = 1.0", "A[0][0] = 0x7F, B[:, 0] = 0", "A[0][0] = 0x7F, B all zero",
                          "A row 0 block 0 all 0x7F, B all zero", "B[0][0] = 0x7F, A = 1.0"};
  for (int v = 0; v < 6; ++v) {
    Case c; unit(c);
    for (int r = 0; r < 16; ++r) for (int k = 0; k < 32; ++k) { c.a[r][k] = e4m3(1.f); c.b[r][k] = e4m3(1.f); }
    if (v == 0 || v == 2 || v == 3) c.a[0][0] = 0x7F;
    if (v == 1) c.a[0][0] = 0xFF;
    if (v == 2) for (int n = 0; n < 16; ++n) c.b[n][0] = 0;
    if (v == 3 || v == 4) memset(c.b, 0, sizeof c.b);
    if (v == 4) memset(c.a[0], 0x7F, 32);
    if (v == 5) c.b[0][0] = 0x7F;
    cs.push_back(c);
  }
  // ---- T6: row 0: +2^24 at k = 0 (block 0), 31 ones in block 1, -2^24 at k = 96 (block 3); row 1: the same with the big pair adjacent ----
  const int t6 = (int)cs.size();
  for (int v = 0; v < 3; ++v) {
    Case c; unit(c);
    for (int n = 0; n < 16; ++n) for (int k = 0; k < 128; ++k) c.b[n][k] = e4m3(1.f);
    for (int r = 0; r < 16; ++r) {
      c.a[r][0] = e4m3(1.f);
      for (int k = 32; k < 63; ++k) c.a[r][k] = e4m3(1.f);
      if (v == 0) c.a[r][96] = e4m3(-1.f);
    }
    for (int l = 0; l < 16; ++l) c.sa[l] = 127 + 24;
    for (int l = 48; l < 64; ++l) c.sa[l] = 127 + 24;
    if (v == 1) for (int r = 0; r < 16; ++r) for (int n = 0; n < 16; ++n) c.c[r][n] = -16777216.f;   // the big negative term as C
    if (v == 2) {                                                                                 // C = 2^24, 31 ones only
      for (int r = 0; r < 16; ++r) { c.a[r][0] = 0; for (int n = 0; n < 16; ++n) c.c[r][n] = 16777216.f; }
    }
    cs.push_back(c);
  }

  Case* dev;
  CK(hipMalloc(&dev, cs.size() * sizeof(Case)));
  CK(hipMemcpy(dev, cs.data(), cs.size() * sizeof(Case), hipMemcpyHostToDevice));
  probe<<<(unsigned)cs.size(), 64>>>(dev);
  CK(hipDeviceSynchronize());
  CK(hipMemcpy(cs.data(), dev, cs.size() * sizeof(Case), hipMemcpyDeviceToHost));
  CK(hipFree(dev));

  printf("v_mfma_scale_f32_16x16x128_f8f6f4, e4m3 x e4m3; lane l (r = l & 15, q = l >> 4) is handed X[r][16 q .. + 15] (registers 0-3), X[r][64 + 16 q .. + 15] (registers 4-7) and its own scale word\n\n");
  int bad1 = 0;
  for (int r = 0; r < 16; ++r) for (int k = 0; k < 128; ++k) {
    const Case& c = cs[t1 + r * 128 + k];
    for (int rr = 0; rr < 16; ++rr) for (int n = 0; n < 16; ++n) {
      const float want = rr == r ? (float)bval(n, k) : 0.f;
      if (c.d[rr][n] != want) { if (bad1 < 8) printf("  T1 mismatch: one-hot (%d, %d): D[%d][%d] = %g, want %g\n", r, k, rr, n, c.d[rr][n], want); ++bad1; }
    }
  }
  printf("T1 data map: 2048 one-hot positions x 256 outputs, mismatches: %d  -> %s\n", bad1,
         bad1 ? "HYPOTHESIS FAILS" : "registers 0-3 of lane l hold K 16 q .. + 15, registers 4-7 K 64 + 16 q .. + 15 of row (column) l & 15, for A and for B (up to a K permutation inside a scale run, which T2 / T3 cannot see either); D[4 q + j][l & 15]");

  int bad2 = 0;
  for (int side = 0; side < 2; ++side)
    for (int l = 0; l < 64; ++l) {
      int hit_blk = -1, hit_idx = -1, nhit = 0;
      for (int blk = 0; blk < 4; ++blk) {
        const Case& c = cs[t2 + (side * 64 + l) * 4 + blk];
        for (int r = 0; r < 16; ++r) for (int n = 0; n < 16; ++n) {
          const int idx = side ? n : r;
          if (c.d[r][n] == 64.f) { if (hit_blk != blk || hit_idx != idx) { hit_blk = blk; hit_idx = idx; } ++nhit; }
          else if (c.d[r][n] != 32.f) { if (bad2 < 8) printf("  T2 odd value %g (side %d lane %d block %d D[%d][%d])\n", c.d[r][n], side, l, blk, r, n); ++bad2; }
        }
      }
      const bool ok = nhit == 16 && hit_blk == (l >> 4) && hit_idx == (l & 15);
      if (!ok) { ++bad2; printf("  T2 %s scale of lane %2d: %d outputs doubled, last (%s %d, block %d)\n", side ? "B" : "A", l, nhit, side ? "column" : "row", hit_idx, hit_blk); }
    }
  printf("T2 scale map: 2 x 64 lanes x 4 blocks, deviations: %d  -> %s\n", bad2,
         bad2 ? "HYPOTHESIS FAILS" : "byte 0 of lane l's scale word scales row (column) l & 15, K 32 q .. 32 q + 31: NOT the lane's own elements");

  int bad3 = 0;
  for (int rep = 0; rep < 4; ++rep) {
    const Case& c = cs[t3 + rep];
    auto dec = [](uint8_t x) { const int e = (x >> 3) & 15, m = x & 7; const float v = e ? ldexpf(1.f + m / 8.f, e - 7) : ldexpf(m / 8.f, -6); return (x & 0x80) ? -v : v; };
    for (int r = 0; r < 16; ++r) for (int n = 0; n < 16; ++n) {
      double s = c.c[r][n];
      for (int k = 0; k < 128; ++k)
        s += (double)dec(c.a[r][k]) * dec(c.b[n][k]) * ldexp(1.0, (int)c.sa[(k >> 5) * 16 + r] - 127 + (int)c.sb[(k >> 5) * 16 + n] - 127);
      if ((double)c.d[r][n] != s) { if (bad3 < 8) printf("  T3 mismatch rep %d D[%d][%d] = %g, want %g\n", rep, r, n, c.d[r][n], s); ++bad3; }
    }
  }
  printf("T3 dense integers, distinct scales per (row, block), C input: 4 x 256 outputs, mismatches: %d\n\n", bad3);

  printf("T4 scale bytes (A = B = 1.0 on block 0, all other scales 2^0; D[0][0] reads lane 0's scale, D[1][1] does not; plain value 32)\n");
  for (int v = 0; v < 11; ++v) {
    const Case& c = cs[t4 + v];
    printf("  %-44s D[0][0] = %-12g D[0][1] = %-12g D[1][0] = %-12g D[1][1] = %g\n", t4name[v], c.d[0][0], c.d[0][1], c.d[1][0], c.d[1][1]);
  }
  printf("\nT5 e4m3 NaN codes (A = B = 1.0 on block 0; plain value 32)\n");
  for (int v = 0; v < 6; ++v) {
    const Case& c = cs[t5 + v];
    printf("  %-44s D[0][0] = %-12g D[0][1] = %-12g D[1][0] = %-12g D[1][1] = %g\n", t5name[v], c.d[0][0], c.d[0][1], c.d[1][0], c.d[1][1]);
  }
  printf("\nT6 summation inside one instruction\n");
  printf("  2^24 (k = 0) + 31 ones (k = 32 .. 62) - 2^24 (k = 96), C = 0:   D[0][0] = %g   (exact 31; an fp32 chain in k order gives 0)\n", cs[t6].d[0][0]);
  printf("  2^24 (k = 0) + 31 ones, C = -2^24:                             D[0][0] = %g   (exact 31)\n", cs[t6 + 1].d[0][0]);
  printf("  31 ones, C = +2^24:                                            D[0][0] - 2^24 = %g   (exact 31; fp32 adds of 1 give 0)\n",
         (double)cs[t6 + 2].d[0][0] - 16777216.0);
  return (bad1 || bad2 || bad3) ? 1 : 0;
}
