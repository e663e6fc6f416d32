// 3x3 stride-1 'SAME' convolution + bias + leaky_relu: Winograd F(2x2,3x3) with FLOAT32 operands split into TWO fp16 terms,
// three fp16 MFMA products per 16 k (m4d_wino6.hip's tiling, DMA scheme and epilogue; six bf16 products there).
//
// A float32 value scaled by a power of two into fp16's range is hi + lo with hi = fp16(x), lo = fp16(x - hi) (round to nearest,
// 11 + 11 significant bits; x - hi is exact in float32).  a * b = ah bh + ah bl + al bh + al bl: the dropped al bl is about
// 2^-22 |a b|, and an fp16 x fp16 product is exact in the matrix core's float32 accumulator.  Three v_mfma_f32_32x32x16_f16
// (same rate as the bf16 form) instead of six, half the B-fragment traffic, and the split of the A operand takes four
// v_fma_mix instructions per element pair (scale, convert, residual in one rounding each) instead of eleven.
//   Scales.  fp16 has 5 exponent bits, so every operand is scaled first, by a power of two (exact) that is uniform over K.
//   Each Winograd position is a GEMM of its own; in position (r, c) row m (one Winograd tile) is scaled by 2^s, s from the
//   largest finite |d| over ALL input channels of the four input pixels that V[r][c] = (B^T d B)[r][c] combines (|V| <= 4 max|d|,
//   so |2^s V| < 2^15) -- per position, not per 4x4 patch, so that an output pixel's error follows the inputs of its own 3x3
//   window, as in a float32 Winograd kernel (a patch-wide scale lost small pixels next to a 2^40 larger neighbour).  Column n
//   (one output channel) is scaled by 2^t_n on the host (pack_conv_weights_winof16, |2^t_n U| < 2^15).  The epilogue multiplies
//   each accumulator by 2^-s (v_ldexp, exact) before the output transform and by 2^-t_n after it.  The per-pixel maxima come
//   from a scan of the tile's whole halo at the start of the unit, issued behind the prologue's DMAs (raw halo of chunk 0 and
//   the first B fragments do not depend on it).  An Inf / NaN among a position's inputs makes that position non-finite
//   whatever the scale (hi = Inf, lo = Inf - Inf), as in the bf16 split: the scan clamps to the largest finite value so that
//   the scale itself stays finite.  In a chain of these layers the scan is a second pass over 18 x 18 x Cin floats per unit for
//   values the producing layer held in registers: with pm_out its epilogue leaves one word per pixel and 64-channel group, and
//   with pm_in the next layer reads those 324 x ceil(Cin/64) words instead (m4d_conv3x3_winof16_bias_act_pm; same scales, same
//   bits).
// Everything else as m4d_wino6.hip: 8 waves, two per SIMD, a 16x16-pixel x 64-cout unit per workgroup, raw halo and B
// fragments by LDS-DMA with hand-counted vmcnt waits (now 1 raw + 2 fragment pieces per wave and position), the first and the
// last chunk peeled, HALF units for a last cout group of <= 32 channels, XCD tile mapping, the staggered first round.
// Deterministic: fixed summation order, no atomics, and every scale depends on the image's own data only.
#include <cstdlib>
#include "m4d_common.h"
#include "../../include/m4depth_hip.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef int i32x4 __attribute__((ext_vector_type(4)));

struct WinoF16Args {
  const float* x; const unsigned char* wu; const short* wexp; const float* bias; float* out;
  const unsigned* pm_in;        // [b][h][w][ceil(Cin/64)] pixel maxima of x as its producer wrote them, or null: scan the halo
  unsigned* pm_out;             // [b][h][w][CoutPad/64] pixel maxima of out for the next layer, or null
  int b, h, w, Cin, Cout, CoutPad, n_chunks, tiles_x, tiles_y;
  float slope;
  int phases;                   // power of two <= 32
  int stagger;                  // > 0: the first-round workgroups start up to this many 100-MHz ticks apart (m4d_wino6.hip)
};

constexpr int kT = 16, kH = kT + 2;              // output tile, halo (pixels)
constexpr int kJ = 10;                           // raw halo layout of m4d_wino6.hip: [row][column parity][column / 2][quad + pad]
constexpr int kPix = 5;
constexpr int kRow = 2 * kJ * kPix;
constexpr int kRawUsed = kH * kRow;
constexpr int kRawDma = 29;
constexpr int kRawK = 4;
constexpr int kRawSlots = kRawDma * 64;
constexpr int kFrag = 4 * 1024;                  // B fragments per position: 2 N-tiles x 2 parts x 1 KB
constexpr int kBRingBytes = 4 * kFrag;           // per position row: a ring of 4 positions
constexpr int kBRingOff = 2 * kRawSlots * 16;    // byte offset of the B rings in LDS
constexpr int kEpiBytes = (4 * 4 * 2 * 32 * 36 + 32) * 4;     // epilogue staging (aliases the raw halo and the rings)
constexpr int kPmOff = kEpiBytes;                // halo pixel maxima [kH * kH] (bits of a finite float >= 0), kept past the epilogue
constexpr int kTsOff = kPmOff + kH * kH * 4;     // -s of every (position, tile) [16][64]
constexpr int kLdsBytes = kTsOff + 16 * 64 * 4;
static_assert(kBRingOff + 4 * kBRingBytes <= kEpiBytes, "the K loop's LDS lies inside the epilogue's");
static_assert(kLdsBytes <= 160 * 1024, "LDS budget of one CU");

// (v0, v1) x 2^s -> packed fp16 hi and lo, each conversion rounded once (v_fma_mix: a * b + c with f32 / f16 sources):
// hi = fp16(2^s v), lo = fp16(2^s v - hi).  Four VALU instructions per pair.
__device__ __forceinline__ void split2_pair(float v0, float v1, float S, unsigned& hi, unsigned& lo) {
  asm("v_fma_mixlo_f16 %0, %1, %2, 0" : "=v"(hi) : "v"(v0), "v"(S));
  asm("v_fma_mixhi_f16 %0, %1, %2, 0" : "+v"(hi) : "v"(v1), "v"(S));
  asm("v_fma_mixlo_f16 %0, %1, %2, -%3 op_sel_hi:[0,0,1]" : "=v"(lo) : "v"(v0), "v"(S), "v"(hi));
  asm("v_fma_mixhi_f16 %0, %1, %2, -%3 op_sel:[0,0,1] op_sel_hi:[0,0,1]" : "+v"(lo) : "v"(v1), "v"(S), "v"(hi));
}

__device__ __forceinline__ float max3_abs(float m, float a, float b) {      // max(m, |a|, |b|); NaN operands are dropped
  asm("v_max3_f32 %0, %0, |%1|, |%2|" : "+v"(m) : "v"(a), "v"(b));
  return m;
}

__global__ void __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2, 2)))
conv3x3_winof16_kernel(const WinoF16Args a) {
  extern __shared__ __align__(16) float lds[];
  asm volatile("" : : "s"(a.x), "s"(a.wu), "s"(a.out), "s"(a.bias));
  if (a.stagger > 0 && blockIdx.y == 0 && blockIdx.x < 256) {
    const unsigned phase = (blockIdx.x >> 3) & (unsigned)(a.phases - 1);
    const unsigned long long t_end = wall_clock64() + (unsigned long long)(phase * (unsigned)a.stagger) / (unsigned)a.phases;
    for (int spin = 0; spin < 512 && wall_clock64() < t_end; ++spin) __builtin_amdgcn_s_sleep(16);   // (bounded: a delay, never a hang)
  }
  float4* raw = reinterpret_cast<float4*>(lds);                      // [2][kRawSlots]
  unsigned* pm = reinterpret_cast<unsigned*>(reinterpret_cast<unsigned char*>(lds) + kPmOff);
  int* ts = reinterpret_cast<int*>(reinterpret_cast<unsigned char*>(lds) + kTsOff);
  const unsigned lds_base = (unsigned)(size_t)(__attribute__((address_space(3))) float*)lds;

  const int t = threadIdx.x, lane = t & 63;
  const int wv = __builtin_amdgcn_readfirstlane(t >> 6);
  const int pr = wv & 3, mt = wv >> 2;                               // position row, M-tile (waves r and r + 4 share a SIMD)
  const int m = lane & 31, kh = lane >> 5;
  const int n_tiles = a.tiles_x * a.tiles_y, n_groups = a.CoutPad / 64;
  int tile, ng;
  {
    const int L = blockIdx.x;
    if ((n_tiles & 7) == 0) {                                        // the cout groups of one pixel tile on one XCD
      const int xcd = L & 7, idx = L >> 3;
      tile = xcd * (n_tiles >> 3) + idx / n_groups;
      ng = idx % n_groups;
    } else {
      tile = L / n_groups;
      ng = L % n_groups;
    }
  }
  const int tile_y = (tile / a.tiles_x) * kT, tile_x = (tile % a.tiles_x) * kT;
  const int bi = blockIdx.y;
  const int n = a.n_chunks, last = n - 1;
  const float* ximg = a.x + (long long)bi * a.h * a.w * a.Cin;

  // ---- raw halo by LDS-DMA (m4d_wino6.hip)
  i32x4 rsrc;
  {
    const unsigned long long xa = (unsigned long long)ximg;
    rsrc[0] = __builtin_amdgcn_readfirstlane((int)(xa & 0xffffffffull));
    rsrc[1] = __builtin_amdgcn_readfirstlane((int)((xa >> 32) & 0xffffull));
    rsrc[2] = a.h * a.w * a.Cin * 4;
    rsrc[3] = 0x00020000;
  }
  unsigned rvoff[kRawK];
#pragma unroll
  for (int k = 0; k < kRawK; ++k) {
    const int i = min(wv + 8 * k, kRawDma - 1);
    const int s = i * 64 + lane;
    const int pix = s / kPix, q = s - pix * kPix;
    const int hy = pix / (2 * kJ), r2 = pix - hy * (2 * kJ);
    const int e = r2 / kJ, j = r2 - e * kJ;
    const int hx = 2 * j + e;
    const int gy = tile_y - 1 + hy, gx = tile_x - 1 + hx;
    const bool ok = s < kRawUsed && q < 4 && j < 9 && gy >= 0 && gy < a.h && gx >= 0 && gx < a.w;
    rvoff[k] = ok ? (unsigned)(((gy * a.w + gx) * a.Cin + q * 4) * 4) : 0x80000000u;
  }
  auto raw_dma = [&](int chunk, int buf, int k) {
    const int i = min(wv + 8 * k, kRawDma - 1);
    const unsigned lds_dst = lds_base + (unsigned)((buf * kRawSlots + i * 64) * 16);
    asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tbuffer_load_dwordx4 %0, %2, %3 offen lds"
                 : : "v"(rvoff[k]), "s"(lds_dst), "s"(rsrc), "s"(chunk * 64) : "memory", "m0");
  };

  const int ra = pr == 0 ? 0 : (pr == 2 ? 2 : 1);
  const int rb_ = pr == 0 ? 2 : (pr == 1 ? 2 : (pr == 2 ? 1 : 3));
  const float sgn = pr == 1 ? 1.f : -1.f;
  const int ty0 = m >> 3, tx = m & 7;
  const int src0 = (8 * mt + 2 * ty0) * kRow + tx * kPix + 2 * kh;

  float tv[4][8];
  auto read_t = [&](const float4* rbuf, int c0) {
#pragma unroll
    for (int qq = 0; qq < 2; ++qq)
#pragma unroll
      for (int cc = 0; cc < 2; ++cc) {
        const int c = c0 + 2 * cc;
        const int s = src0 + qq + ((c & 1) * kJ + (c >> 1)) * kPix;
        const float4 da = rbuf[s + ra * kRow], db = rbuf[s + rb_ * kRow];
        tv[c][4 * qq + 0] = __builtin_fmaf(sgn, db.x, da.x);
        tv[c][4 * qq + 1] = __builtin_fmaf(sgn, db.y, da.y);
        tv[c][4 * qq + 2] = __builtin_fmaf(sgn, db.z, da.z);
        tv[c][4 * qq + 3] = __builtin_fmaf(sgn, db.w, da.w);
      }
  };
  float Sc[4];                                     // 2^s of this lane's tile (row m of M-tile mt) at positions (pr, 0..3)
  // A operands of position (pr, c), element pair e -> one packed word of the hi and of the lo fp16x8 operand
  auto gen_pair = [&](int c, int e, u32x4 (&A)[2]) {
    float v[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int ch = 2 * e + h;
      v[h] = c == 0 ? tv[0][ch] - tv[2][ch] : c == 1 ? tv[1][ch] + tv[2][ch] : c == 2 ? tv[2][ch] - tv[1][ch] : tv[1][ch] - tv[3][ch];
    }
    unsigned p_hi, p_lo;
    split2_pair(v[0], v[1], Sc[c], p_hi, p_lo);
    A[0][e] = p_hi; A[1][e] = p_lo;
  };

  // ---- B operands: wu[chunk][N-group][16 positions][2 N-tiles][2 parts][64 lanes][8 fp16]; 4 KB per position, wave (pr, mt)
  // fetches N-tile mt's two fragments
  const long long w_pos = kFrag;
  const long long w_chunk = (long long)n_groups * 16 * w_pos;
  const unsigned char* wc = a.wu + ((long long)ng * 16 + 4 * pr) * w_pos;
  const unsigned bring = lds_base + (unsigned)(kBRingOff + pr * kBRingBytes);
  const unsigned char* bring_p = reinterpret_cast<const unsigned char*>(lds) + kBRingOff + pr * kBRingBytes;
  const unsigned bl = (unsigned)lane * 16u;
  const bool half = __builtin_amdgcn_readfirstlane(ng * 64 + 32 >= a.Cout ? 1 : 0) != 0;
  const unsigned bl_dma = (half && mt == 1) ? 0u : bl + (unsigned)mt * 2048u;
  auto b_dma = [&](const unsigned char* gsrc, int slot) {
    asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\t"
                 "global_load_lds_dwordx4 %0, %2\n\tglobal_load_lds_dwordx4 %0, %2 offset:1024"
                 : : "v"(bl_dma), "s"(bring + (unsigned)(slot * kFrag) + (unsigned)mt * 2048u), "s"(gsrc) : "memory", "m0");
  };
  f16x8 B0[2][2], B1[2];                           // B hi (double buffered) and lo per N-tile
  auto frag = [&](int slot, int nt, int part) {
    return *reinterpret_cast<const f16x8*>(bring_p + slot * kFrag + (nt * 2 + part) * 1024 + bl);
  };
#define M4D_WF_WAIT(nn) asm volatile("s_waitcnt vmcnt(" #nn ") lgkmcnt(0)" ::: "memory")

  f32x16 acc[4][2];

  // ---- prologue: raw(0), B(0), B(1), B(2), raw(1), B(3) by DMA (the K loop's vmcnt order, m4d_wino6.hip), then the scan
#pragma unroll
  for (int k = 0; k < kRawK; ++k) raw_dma(0, 0, k);
  b_dma(wc, 0);
  b_dma(wc + w_pos, 1);
  b_dma(wc + 2 * w_pos, 2);
#pragma unroll
  for (int k = 0; k < kRawK; ++k) raw_dma(min(1, last), 1, k);
  b_dma(wc + 3 * w_pos, 3);
  static_assert(kRawK == 4, "the vmcnt counts below assume 4 raw-halo pieces + 2 fragment pieces per position");

  // ---- row scales.  Per halo pixel the largest |x| over all Cin: 8 lanes per pixel (128 contiguous bytes per pixel and load),
  // pixels t / 8 + 64 r; pixels outside the image (and past the halo) count as 0.  Then per tile the maximum over its 4x4 patch.
  //   pm_in: the layer that wrote x left these maxima beside it (its epilogue, below), one word per pixel and group of 64
  // channels -- thread p takes halo pixel p's, and x itself is read by the DMAs only.  The scales use the exponent field of a
  // maximum alone, so the two sources need not agree on a denormal maximum (a scan may flush it to 0; exponent 0 either way).
  if (a.pm_in) {
    if (t < kH * kH) {
      const int hy = t / kH, hx = t - hy * kH;
      const int gy = tile_y - 1 + hy, gx = tile_x - 1 + hx;
      const int G = (a.Cin + 63) >> 6;
      unsigned u = 0u;
      if (gy >= 0 && gy < a.h && gx >= 0 && gx < a.w) {
        const unsigned* q = a.pm_in + (((long long)bi * a.h + gy) * a.w + gx) * G;
        for (int g = 0; g < G; ++g) u = max(u, q[g]);
      }
      pm[t] = min(u, 0x7f7fffffu);                 // (as written; the bound keeps a scale finite whatever the caller hands in)
    }
  } else {
    const int g = t & 7, p0 = t >> 3, nq = a.Cin >> 2;
    constexpr int kR = (kH * kH + 63) / 64;        // 6
    int poff[kR];
    bool pv[kR];
    float mx[kR];
#pragma unroll
    for (int r = 0; r < kR; ++r) {
      const int p = p0 + 64 * r, hy = p / kH, hx = p - hy * kH;
      const int gy = tile_y - 1 + hy, gx = tile_x - 1 + hx;
      pv[r] = p < kH * kH && gy >= 0 && gy < a.h && gx >= 0 && gx < a.w;
      poff[r] = pv[r] ? (gy * a.w + gx) * a.Cin : 0;                // (a pixel inside the image either way: no masked loads)
      mx[r] = 0.f;
    }
#pragma unroll 2
    for (int q = g; q < nq; q += 8) {
#pragma unroll
      for (int r = 0; r < kR; ++r) {
        const float4 v = *reinterpret_cast<const float4*>(ximg + poff[r] + 4 * q);
        mx[r] = max3_abs(max3_abs(mx[r], v.x, v.y), v.z, v.w);
      }
    }
#pragma unroll
    for (int r = 0; r < kR; ++r) {
      unsigned u = pv[r] ? min(__float_as_uint(mx[r]), 0x7f7fffffu) : 0u;   // Inf -> the largest finite float
      u = max(u, (unsigned)__builtin_amdgcn_update_dpp(0, (int)u, 0x141, 0xf, 0xf, false));   // row_half_mirror
      u = max(u, (unsigned)__builtin_amdgcn_update_dpp(0, (int)u, 0xb1, 0xf, 0xf, false));    // quad_perm [1,0,3,2]
      u = max(u, (unsigned)__builtin_amdgcn_update_dpp(0, (int)u, 0x4e, 0xf, 0xf, false));    // quad_perm [2,3,0,1]
      const int p = p0 + 64 * r;
      if (g == 0 && p < kH * kH) pm[p] = u;
    }
  }
  __syncthreads();
  {
    // this lane's tile: halo rows 2 (4 mt + ty0) + (ra, rb) feed position row pr; columns 2 tx + (0, 2), (1, 2), (1, 2), (1, 3)
    // feed positions c = 0 .. 3 (V = B^T d B).  The scale of position (pr, c) comes from those four pixels only, so that an output
    // pixel's error follows the inputs of its own 3x3 window, as in a float32 Winograd kernel.
    const unsigned* row = pm + 2 * (4 * mt + ty0) * kH + 2 * tx;
    unsigned cm[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) cm[j] = max(row[ra * kH + j], row[rb_ * kH + j]);
    const unsigned um[4] = {max(cm[0], cm[2]), max(cm[1], cm[2]), max(cm[1], cm[2]), max(cm[1], cm[3])};
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      // max < 2^(E - 126) with E the biased exponent: s = 139 - E keeps 2^s max < 2^13; all-zero / denormal inputs -> 2^126
      const int s = min(139 - (int)(um[c] >> 23), 126);
      Sc[c] = __uint_as_float((unsigned)(s + 127) << 23);
      if (kh == 0) ts[(pr * 4 + c) * 64 + mt * 32 + m] = -s;
    }
  }
  M4D_WF_WAIT(0);
  __syncthreads();
  u32x4 A[2][2];                                   // [ring][part]: packed fp16 pairs

  auto pin_a = [&](u32x4 (&X)[2]) {
#pragma unroll
    for (int part = 0; part < 2; ++part) asm volatile("" : "+v"(X[part]));
  };
  auto pin_t = [&](int c0) {
#pragma unroll
    for (int cc = 0; cc < 2; ++cc)
#pragma unroll
      for (int e = 0; e < 8; ++e) asm volatile("" : "+v"(tv[c0 + 2 * cc][e]));
  };
#define M4D_WF_MFMA(c, ap, bv)                                                                                         \
  _Pragma("unroll") for (int nt = 0; nt < NTL; ++nt)                                                                   \
    acc[c][nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, A[(c) & 1][ap]), bv[nt], acc[c][nt], 0, 0, 0);
#define M4D_WF_MFMA0(c, ap, bv)                                                                                        \
  _Pragma("unroll") for (int nt = 0; nt < NTL; ++nt)                                                                   \
    acc[c][nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, A[(c) & 1][ap]), bv[nt],             \
                                                        FIRST ? f32x16{} : acc[c][nt], 0, 0, 0);
#define M4D_WF_PIPE(valu)                                                                                              \
  _Pragma("unroll") for (int i_ = 0; i_ < NTL; ++i_) {                                                                 \
    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                                                                 \
    __builtin_amdgcn_sched_group_barrier(0x002, (valu) * (2 / NTL), 0);                                                \
  }
  // One position = three blocks of NTL MFMAs (the small product first: A lo x B hi, then A hi x B lo, A hi x B hi), each followed
  // by one DMA slot.  B lo is refilled for the next position after block 1 (its last use), B hi is double buffered.
#define M4D_WF_BLOCK0(c, cn, next_slot, valu, NEXT)                                                                    \
  if (NEXT) { B0[((c) & 1) ^ 1][0] = frag(next_slot, 0, 0); if (NTL == 2) B0[((c) & 1) ^ 1][1] = frag(next_slot, 1, 0);    \
              gen_pair(cn, 0, A[((c) & 1) ^ 1]); gen_pair(cn, 1, A[((c) & 1) ^ 1]); }                                    \
  M4D_WF_MFMA0(c, 1, B0[(c) & 1])                                                                                      \
  if (NEXT) { asm volatile("" : "+v"(A[((c) & 1) ^ 1][0][0]), "+v"(A[((c) & 1) ^ 1][0][1]),                              \
                                "+v"(A[((c) & 1) ^ 1][1][0]), "+v"(A[((c) & 1) ^ 1][1][1])); M4D_WF_PIPE(valu) }        \
  __builtin_amdgcn_sched_barrier(0);
#define M4D_WF_BLOCK1(c, cn, valu, NEXT)                                                                               \
  if (NEXT) { gen_pair(cn, 2, A[((c) & 1) ^ 1]); }                                                                     \
  M4D_WF_MFMA(c, 0, B1)                                                                                                \
  if (NEXT) { asm volatile("" : "+v"(A[((c) & 1) ^ 1][0][2]), "+v"(A[((c) & 1) ^ 1][1][2])); M4D_WF_PIPE(valu) }        \
  __builtin_amdgcn_sched_barrier(0);
#define M4D_WF_BLOCK2(c, cn, next_slot, valu, NEXT)                                                                    \
  if (NEXT) { B1[0] = frag(next_slot, 0, 1); if (NTL == 2) B1[1] = frag(next_slot, 1, 1);                                \
              gen_pair(cn, 3, A[((c) & 1) ^ 1]); }                                                                     \
  M4D_WF_MFMA(c, 0, B0[(c) & 1])                                                                                       \
  if (NEXT) { pin_a(A[((c) & 1) ^ 1]); M4D_WF_PIPE(valu) }                                                             \
  __builtin_amdgcn_sched_barrier(0);

  // Per position: barrier; one raw piece and this wave's half of B four positions ahead; then vmcnt(N) leaves exactly the DMAs
  // of this and the previous position in flight (N = 2 x 3).
  auto k_loop = [&](auto ntl_tag) __attribute__((always_inline)) {
  constexpr int NTL = decltype(ntl_tag)::value;
  asm volatile("" ::: "memory");
  read_t(raw, 0);
  read_t(raw, 1);
#pragma unroll
  for (int nt = 0; nt < NTL; ++nt) { B0[0][nt] = frag(0, nt, 0); B1[nt] = frag(0, nt, 1); }
#pragma unroll
  for (int e = 0; e < 4; ++e) gen_pair(0, e, A[0]);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  // LAST chunk (peeled): no DMA.  In flight at its entry, oldest first: (n-2, 2)[3] (n-2, 3)[3] -> position 0 ends with
  // vmcnt(3) (slot 2, read by position 1, landed), position 1 with vmcnt(0) (slot 3).
  auto chunk_body = [&](int chunk, auto first_tag, auto last_tag) __attribute__((always_inline)) {
    constexpr bool FIRST = decltype(first_tag)::value != 0, LAST = decltype(last_tag)::value != 0;
    const unsigned char* wn = chunk < last ? wc + w_chunk : wc;
    const int rnext_c = min(chunk + 2, last);
    const float4* rnext = raw + ((chunk + 1) & 1) * kRawSlots;
    // position 0
    __builtin_amdgcn_s_barrier();
    M4D_WF_BLOCK0(0, 1, 1, 2, true)
    if (!LAST) raw_dma(rnext_c, chunk & 1, 0);
    M4D_WF_BLOCK1(0, 1, 1, true)
    if (!LAST) b_dma(wn, 0);
    M4D_WF_BLOCK2(0, 1, 1, 1, true)
    if (!LAST) M4D_WF_WAIT(6);
    else M4D_WF_WAIT(3);
    // position 1
    __builtin_amdgcn_s_barrier();
    M4D_WF_BLOCK0(1, 2, 2, 2, true)
    if (!LAST) raw_dma(rnext_c, chunk & 1, 1);
    M4D_WF_BLOCK1(1, 2, 1, true)
    if (!LAST) b_dma(wn + w_pos, 1);
    M4D_WF_BLOCK2(1, 2, 2, 1, true)
    if (!LAST) M4D_WF_WAIT(6);
    else M4D_WF_WAIT(0);
    // position 2: columns 0, 2 of t(chunk + 1)
    __builtin_amdgcn_s_barrier();
    M4D_WF_BLOCK0(2, 3, 3, 2, true)
    if (!LAST) { raw_dma(rnext_c, chunk & 1, 2); read_t(rnext, 0); }
    M4D_WF_BLOCK1(2, 3, 5, true)
    if (!LAST) { b_dma(wn + 2 * w_pos, 2); pin_t(0); }
    M4D_WF_BLOCK2(2, 3, 3, 5, true)
    if (!LAST) M4D_WF_WAIT(6);
    else asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    // position 3: columns 1, 3 of t(chunk + 1)
    __builtin_amdgcn_s_barrier();
    M4D_WF_BLOCK0(3, 0, 0, 2, !LAST)
    if (!LAST) { raw_dma(rnext_c, chunk & 1, 3); read_t(rnext, 1); }
    M4D_WF_BLOCK1(3, 0, 5, !LAST)
    if (!LAST) { b_dma(wn + 3 * w_pos, 3); pin_t(1); }
    M4D_WF_BLOCK2(3, 0, 0, 5, !LAST)
    if (!LAST) M4D_WF_WAIT(6);
    if (!LAST) wc = wn;
  };
  chunk_body(0, m4d_int<1>{}, m4d_int<0>{});     // (a single-chunk layer, Cin = 16, ends here with surplus fetches)
  if (n > 1) {
    for (int chunk = 1; chunk < last; ++chunk) chunk_body(chunk, m4d_int<0>{}, m4d_int<0>{});
    chunk_body(last, m4d_int<0>{}, m4d_int<1>{});
  }
  };
  if (half) k_loop(m4d_int<1>{}); else k_loop(m4d_int<2>{});
#undef M4D_WF_MFMA
#undef M4D_WF_MFMA0
#undef M4D_WF_BLOCK0
#undef M4D_WF_BLOCK1
#undef M4D_WF_BLOCK2
#undef M4D_WF_PIPE
  M4D_WF_WAIT(0);                                  // no DMA may land in LDS once the epilogue reuses it
#undef M4D_WF_WAIT
  __syncthreads();

  // ---- 2^-s per (position, tile) on the accumulators, output transform (m4d_wino6.hip), then 2^-t_n, bias, leaky_relu
  const int cq16 = half ? (t & 7) : (t & 15);
  const int co = ng * 64 + 4 * cq16;
  float bs[4];
  int wt[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) { bs[e] = a.bias[min(co + e, a.Cout - 1)]; wt[e] = a.wexp[co + e]; }
  constexpr int kMS = 36;
  constexpr int kRbMT = 4 * 2 * 32 * kMS;
  constexpr int kRbSkew = 32;
  float* Rb = lds;
  {
    // accumulator register r holds tile row (r & 3) + 8 (r >> 2) + 4 kh of M-tile mt: four consecutive tiles per ds_read_b128
    int4 ne[4][4];                                 // [position c][r >> 2]
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) ne[c][g4] = *reinterpret_cast<const int4*>(ts + (pr * 4 + c) * 64 + mt * 32 + 8 * g4 + 4 * kh);
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
      if (nt == 1 && half) break;
#pragma unroll
      for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int4 q = ne[c][r >> 2];
          const int ex = (r & 3) == 0 ? q.x : (r & 3) == 1 ? q.y : (r & 3) == 2 ? q.z : q.w;
          acc[c][nt][r] = __builtin_ldexpf(acc[c][nt][r], ex);
        }
    }
  }
#pragma unroll
  for (int nt = 0; nt < 2; ++nt) {
    if (nt == 1 && half) break;
    float* rbuf = Rb + (nt * 2 + mt) * kRbMT + nt * kRbSkew;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float m0 = acc[0][nt][r], m1 = acc[1][nt][r], m2 = acc[2][nt][r], m3 = acc[3][nt][r];
      const int trow = (r & 3) + 8 * (r >> 2) + 4 * kh;
      rbuf[((pr * 2 + 0) * 32 + trow) * kMS + m] = (m0 + m1) + m2;
      rbuf[((pr * 2 + 1) * 32 + trow) * kMS + m] = (m1 - m2) - m3;
    }
  }
  __syncthreads();
  float* oimg = a.out + (long long)bi * a.h * a.w * a.Cout;
  const bool vec_ok = (a.Cout & 3) == 0;
  const bool whole = tile_x + kT <= a.w && tile_y + kT <= a.h;
  const bool fast = whole && vec_ok && ng * 64 + (half ? 32 : 64) <= a.Cout;
  const int ont = cq16 >> 3, cq = cq16 & 7;
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    if (it == 1 && half) break;
    const int tl = half ? (t >> 3) & 31 : (t >> 4) & 31, omt = half ? (t >> 8) : it;
    const float* rbuf = Rb + (ont * 2 + omt) * kRbMT + ont * kRbSkew;
    const int tg = omt * 32 + tl;
    const int ty2 = tg >> 3, tx2 = tg & 7;
    float4 rv[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int k = 0; k < 2; ++k) rv[i][k] = *reinterpret_cast<const float4*>(rbuf + ((i * 2 + k) * 32 + tl) * kMS + 4 * cq);
    float y[2][2][4];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const float* r0 = reinterpret_cast<const float*>(&rv[0][k]); const float* r1 = reinterpret_cast<const float*>(&rv[1][k]);
      const float* r2 = reinterpret_cast<const float*>(&rv[2][k]); const float* r3 = reinterpret_cast<const float*>(&rv[3][k]);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int ex = -wt[e];
        const float v0 = __builtin_ldexpf((r0[e] + r1[e]) + r2[e], ex) + bs[e];
        const float v1 = __builtin_ldexpf((r1[e] - r2[e]) - r3[e], ex) + bs[e];
        y[k][0][e] = v0 > 0.f ? v0 : v0 * a.slope;
        y[k][1][e] = v1 > 0.f ? v1 : v1 * a.slope;
      }
    }
    const int ox = tile_x + 2 * tx2, oy = tile_y + 2 * ty2;
    if (a.pm_out) {
      // The maxima the next layer's scan would find, from the values as stored: per pixel the largest finite |y| over this
      // group's real channels (NaN counts as 0, Inf as the largest finite float; a padded channel carries a clamped bias and
      // does not count).  The 16 lanes (8 in a half unit) that hold a tile's channels are neighbours: reduced by DPP as in the
      // scan.  One plain store per pixel and group; every pixel of the image belongs to exactly one unit per group.
      // v_max3 drops NaN operands (the stored values are results of arithmetic: quiet), as in the scan; the four pixels' DPP
      // chains are issued side by side.
      const bool allv = ng * 64 + (half ? 32 : 64) <= a.Cout;        // (workgroup-uniform) no padded channel in this unit
      unsigned pu[2][2];
#pragma unroll
      for (int k = 0; k < 2; ++k)
#pragma unroll
        for (int l = 0; l < 2; ++l) {
          float v[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = (allv || co + e < a.Cout) ? y[k][l][e] : 0.f;
          pu[k][l] = min(__float_as_uint(max3_abs(max3_abs(0.f, v[0], v[1]), v[2], v[3])), 0x7f7fffffu);
        }
#define M4D_WF_PMAX(ctrl)                                                                                              \
  _Pragma("unroll") for (int k = 0; k < 2; ++k) _Pragma("unroll") for (int l = 0; l < 2; ++l)                            \
    pu[k][l] = max(pu[k][l], (unsigned)__builtin_amdgcn_update_dpp(0, (int)pu[k][l], ctrl, 0xf, 0xf, false));
      M4D_WF_PMAX(0x141)                           // row_half_mirror
      M4D_WF_PMAX(0xb1)                            // quad_perm [1,0,3,2]
      M4D_WF_PMAX(0x4e)                            // quad_perm [2,3,0,1]
      if (!half) { M4D_WF_PMAX(0x140) }            // row_mirror
#undef M4D_WF_PMAX
      if (cq16 == 0) {
        unsigned* pp = a.pm_out + (((long long)bi * a.h + oy) * a.w + ox) * n_groups + ng;
#pragma unroll
        for (int l = 0; l < 2; ++l)
#pragma unroll
          for (int k = 0; k < 2; ++k)
            if (ox + k < a.w && oy + l < a.h) pp[((long long)l * a.w + k) * n_groups] = pu[k][l];
      }
    }
    float* op = oimg + ((long long)oy * a.w + ox) * a.Cout + co;
    if (fast) {
#pragma unroll
      for (int l = 0; l < 2; ++l)
#pragma unroll
        for (int k = 0; k < 2; ++k) m4d_store16(op + ((long long)l * a.w + k) * a.Cout, y[k][l][0], y[k][l][1], y[k][l][2], y[k][l][3]);
    } else if (co < a.Cout) {
#pragma unroll
      for (int l = 0; l < 2; ++l)
#pragma unroll
        for (int k = 0; k < 2; ++k)
          if (ox + k < a.w && oy + l < a.h) {
            float* o2 = op + ((long long)l * a.w + k) * a.Cout;
            if (vec_ok && co + 3 < a.Cout) m4d_store16(o2, y[k][l][0], y[k][l][1], y[k][l][2], y[k][l][3]);
            else { for (int e = 0; e < 4; ++e) if (co + e < a.Cout) o2[e] = y[k][l][e]; }
          }
    }
  }
}

}  // namespace

extern "C" int m4d_conv3x3_winof16_bias_act_pm(const float* x, const void* wuh, const float* bias, int b, int h, int w,
                                               int Cin, int Cout, int CoutPad, float slope, float* out,
                                               const unsigned* pm_in, unsigned* pm_out,
                                               int stagger_us, int stagger_phases, void* stream) {
  M4D_CHECK_ARG(x && wuh && bias && out && b > 0 && h > 0 && w > 0 && Cin >= 16 && Cout > 0);
  M4D_CHECK_ARG(CoutPad % 64 == 0 && CoutPad >= Cout && Cin % 16 == 0);
  M4D_CHECK_ARG(((((uintptr_t)x) & 15u) == 0) && ((((uintptr_t)wuh) & 15u) == 0));
  M4D_CHECK_ARG((long long)h * w * Cin * 4 < (1ll << 31));                              // one image = one buffer descriptor
  M4D_CHECK_ARG(stagger_us >= 0 && stagger_us <= 1000);
  M4D_CHECK_ARG(stagger_us == 0 || (stagger_phases >= 1 && stagger_phases <= 32 && !(stagger_phases & (stagger_phases - 1))));
  M4D_CHECK_ARG(((((uintptr_t)pm_in) & 3u) == 0) && ((((uintptr_t)pm_out) & 3u) == 0));
  M4D_CHECK_ARG(!pm_out || (CoutPad - Cout < 64 && (const void*)pm_out != (const void*)pm_in));   // one word per real cout group
  WinoF16Args a;
  a.pm_in = pm_in; a.pm_out = pm_out;
  a.x = x; a.wu = reinterpret_cast<const unsigned char*>(wuh); a.bias = bias; a.out = out;
  a.b = b; a.h = h; a.w = w; a.Cin = Cin; a.Cout = Cout; a.CoutPad = CoutPad; a.n_chunks = Cin / 16; a.slope = slope;
  // the per-cout exponents t_n follow the fragments: [CoutPad] int16
  a.wexp = reinterpret_cast<const short*>(a.wu + (long long)a.n_chunks * (CoutPad / 64) * 16 * kFrag);
  a.tiles_x = (w + kT - 1) / kT; a.tiles_y = (h + kT - 1) / kT;
  a.stagger = stagger_us * 100;
  a.phases = stagger_us > 0 ? stagger_phases : 1;
  const dim3 grid((unsigned)(a.tiles_x * a.tiles_y * (CoutPad / 64)), (unsigned)b);
  M4D_LDS_OPT_IN(&conv3x3_winof16_kernel);
  m4d_launch(conv3x3_winof16_kernel, grid, dim3(512), (size_t)kLdsBytes, (hipStream_t)stream, a);
  return M4D_LAUNCH_RESULT();
}

extern "C" int m4d_conv3x3_winof16_bias_act_ks(const float* x, const void* wuh, const float* bias, int b, int h, int w,
                                               int Cin, int Cout, int CoutPad, float slope, float* out,
                                               int stagger_us, int stagger_phases, void* stream) {
  return m4d_conv3x3_winof16_bias_act_pm(x, wuh, bias, b, h, w, Cin, Cout, CoutPad, slope, out, nullptr, nullptr, stagger_us,
                                         stagger_phases, stream);
}
