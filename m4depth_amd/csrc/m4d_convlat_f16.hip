// The latency-first small-map convolution of m4d_convlat.hip (tiling, K split over waves and workgroups, weight fragments
// straight into MFMA operand registers, partial-sum slabs finished by the consumer while it stages, K sub-slices added in wave
// order through LDS) with float32 operands scaled by powers of two and split into TWO fp16 terms: three
// v_mfma_f32_32x32x16_f16 products per 16 k instead of six bf16 ones, two weight parts per lane and chunk instead of three
// (18 x 16 B instead of 27 x 16 B).  The split is m4d_wino_f16.hip's: hi = fp16(2^s x), lo = fp16(2^s x - hi), the dropped
// lo x lo product about 2^-22 |a b|.
//   Scales.  B column n (one output channel) is scaled by 2^t_n on the host (pack_conv_weights_lat_f16, |2^t_n w| < 2^15).
//   A row m (one output pixel) is scaled by 2^s_m, s_m from the largest finite |x| over that pixel's 3x3 window and the wave's
//   channels of the round (clamped: Inf / NaN count as the largest finite float), so that each output's error follows its
//   own window (a tile-wide scale loses small pixels next to a much larger neighbour).  The halo is shared by the nine taps and
//   every tap reads it under another row's scale, so it stays float32 in LDS and is split where an A fragment is read: four
//   v_fma_mix per element pair.  The per-halo-pixel maxima are taken while the halo is committed (one quad of lanes per pixel
//   and chunk), the 3x3 maxima of a lane's rows after the barrier the round has anyway.  Each round (up to two chunks per wave)
//   accumulates on its own; its sums are multiplied by 2^-(s_m + t_n) (v_ldexp, exact) and added to the running float32 sums,
//   so what leaves a wave -- into the in-workgroup reduction or a partial slab -- is unscaled: the slab format
//   (network_ops.PartialAct) is the bf16x3 kernel's, and any consumer of it works unchanged.
//   Inf / NaN inside a window make that output non-finite (hi = Inf, lo = Inf - Inf), as in the bf16 split.
// Stride 1 and the cout-groups x K-sub-slices form only (the stride-2 and M-over-waves forms are not dispatched by default and
// stay on m4d_convlat.hip).  Deterministic: fixed summation order, no atomics, and every scale depends on the data only; every
// M-tile count with the same (kw, s_out) gives the same bits.
#include <cstdlib>
#include "m4d_common.h"
#include "m4d_convlat.h"
#include "../../include/m4depth_hip.h"

namespace {

typedef _Float16 lat_f16x8 __attribute__((ext_vector_type(8)));
typedef unsigned lat_u32x4 __attribute__((ext_vector_type(4)));

constexpr int kRowF = 20;                           // floats per staged halo pixel and chunk: 16 channels + 4 (LDS bank spread)
constexpr int kFragF16 = 18 * 1024;                 // bytes of one (group, chunk): [9 taps][2 parts][64 lanes][8] fp16

// (v0, v1) x S -> packed fp16 hi and lo, each rounded once (m4d_wino_f16.hip)
__device__ __forceinline__ void lat_split2_pair(float v0, float v1, float S, unsigned& hi, unsigned& lo) {
  asm("v_fma_mixlo_f16 %0, %1, %2, 0" : "=v"(hi) : "v"(v0), "v"(S));
  asm("v_fma_mixhi_f16 %0, %1, %2, 0" : "+v"(hi) : "v"(v1), "v"(S));
  asm("v_fma_mixlo_f16 %0, %1, %2, -%3 op_sel_hi:[0,0,1]" : "=v"(lo) : "v"(v0), "v"(S), "v"(hi));
  asm("v_fma_mixhi_f16 %0, %1, %2, -%3 op_sel:[0,0,1] op_sel_hi:[0,0,1]" : "+v"(lo) : "v"(v1), "v"(S), "v"(hi));
}

// |v| as the bits of a finite float (Inf / NaN -> the largest finite one): orders like the magnitudes
__device__ __forceinline__ unsigned lat_abs_bits(float v) { return min(__float_as_uint(v) & 0x7fffffffu, 0x7f7fffffu); }

// Stage `n_st` chunks (first chunk c0) of the halo as lat_stage of m4d_convlat.hip does (slabs in slab order, the producer's
// bias + leaky_relu, zero outside the map), but float32, [chunk][pixel][kRowF] in LDS, and the largest |x| of every
// (chunk, pixel) into pm[chunk][pixel].  The four lanes of a (chunk, pixel) are one aligned quad.
template <int SIN, int HW, int HP>
__device__ __forceinline__ void lat_stage_f16(const LatArgs& a, float* halo, unsigned* pm, int t, int bi, int gy0, int gx0, int c0,
                                              int n_st) {
  constexpr int IB = SIN >= 3 ? 2 : 4;
  const int n_items = n_st * HP * 4;
  for (int base = 0; base < n_items; base += 256 * IB) {
    float4 v[IB][SIN];
    int item[IB], ch[IB];
    bool ok[IB];
#pragma unroll
    for (int i = 0; i < IB; ++i) {
      const int idx = base + i * 256 + t;
      const int idc = min(idx, n_items - 1);
      const int j = idc / (HP * 4), rem = idc - j * (HP * 4);
      const int hp = rem >> 2, q = rem & 3;
      const int gy = gy0 + hp / HW, gx = gx0 + hp % HW;
      ch[i] = (c0 + j) * 16 + 4 * q;
      ok[i] = idx < n_items && gy >= 0 && gy < a.h && gx >= 0 && gx < a.w && ch[i] < a.Cin;
      item[i] = idx < n_items ? idx >> 2 : -1;                       // = j * HP + hp
      const long long off = (((long long)bi * a.h + min(max(gy, 0), a.h - 1)) * a.w + min(max(gx, 0), a.w - 1)) * a.Cin
                            + min(ch[i], a.Cin - 4);
#pragma unroll
      for (int s = 0; s < SIN; ++s) v[i][s] = *reinterpret_cast<const float4*>(a.x + s * a.x_slab + off);
    }
#pragma unroll
    for (int i = 0; i < IB; ++i) {
      float e[4] = {v[i][0].x, v[i][0].y, v[i][0].z, v[i][0].w};
#pragma unroll
      for (int s = 1; s < SIN; ++s) { e[0] += v[i][s].x; e[1] += v[i][s].y; e[2] += v[i][s].z; e[3] += v[i][s].w; }
      if (a.x_bias != nullptr) {
        const float4 bb = *reinterpret_cast<const float4*>(a.x_bias + min(ch[i], a.Cin - 4));
        const float bv[4] = {bb.x, bb.y, bb.z, bb.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) { const float u = e[k] + bv[k]; e[k] = u > 0.f ? u : u * a.x_slope; }
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) e[k] = ok[i] ? e[k] : 0.f;
      unsigned u = max(max(lat_abs_bits(e[0]), lat_abs_bits(e[1])), max(lat_abs_bits(e[2]), lat_abs_bits(e[3])));
      u = max(u, (unsigned)__builtin_amdgcn_update_dpp(0, (int)u, 0xb1, 0xf, 0xf, false));    // quad_perm [1,0,3,2]
      u = max(u, (unsigned)__builtin_amdgcn_update_dpp(0, (int)u, 0x4e, 0xf, 0xf, false));    // quad_perm [2,3,0,1]
      if (item[i] >= 0) {
        *reinterpret_cast<float4*>(halo + item[i] * kRowF + 4 * (t & 3)) = make_float4(e[0], e[1], e[2], e[3]);
        if ((t & 3) == 0) pm[item[i]] = u;
      }
    }
  }
}

template <int MTX, int MTY>
__global__ void __launch_bounds__(256, 1)
conv3x3_lat_f16_kernel(const LatArgs a) {
  extern __shared__ __align__(16) float lds_dyn[];
  constexpr int MT = MTX * MTY;
  constexpr int TW = 8 * MTX, TH = 4 * MTY, HW = TW + 2, HP = HW * (TH + 2);   // output tile, input halo (stride 1)
  constexpr int kChunkF = HP * kRowF;
  const int t = threadIdx.x, lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int cgw = 1 << a.cgw_log2, kw = 4 >> a.cgw_log2;
  const int cg = wave & (cgw - 1), ks = wave >> a.cgw_log2;
  const int bx = blockIdx.x, by = blockIdx.y, bz = blockIdx.z;
  const int tiles = a.tiles_x * a.tiles_y;
  const int bi = bx / tiles, tile = bx - bi * tiles;
  const int ty0 = (tile / a.tiles_x) * TH, tx0 = (tile % a.tiles_x) * TW;
  const int g = by * cgw + cg;
  const bool active = g < a.n_groups;
  const int c_begin = bz * a.chunks_per_slice;
  const int c_end = min(a.n_chunks, c_begin + a.chunks_per_slice);
  const int n_slice = max(c_end - c_begin, 0);
  const int rounds = (n_slice + kw - 1) / kw;
  const int n = lane & 31, kh = lane >> 5;
  const int co = g * 32 + n;
  float* halo = lds_dyn;                              // [2 kw][HP][kRowF]
  unsigned* pm = reinterpret_cast<unsigned*>(lds_dyn + 2 * kw * kChunkF);     // [2 kw][HP]
  int* ts = reinterpret_cast<int*>(pm + 2 * kw * HP) + wave * MT * 32;        // this wave's -s_m: [MT][32]
  // epilogue operands first: nothing at the end of the launch waits for memory
  const float my_bias = (a.s_out == 1 && active && co < a.Cout) ? a.bias[co] : 0.f;
  const int gc = min(g, a.n_groups - 1);
  const int my_t = reinterpret_cast<const short*>(a.wp + (long long)a.n_groups * a.n_chunks * kFragF16)[gc * 32 + n];

  lat_f32x16 acc[MT];
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[m][r] = 0.f;

  const unsigned char* wg = a.wp + ((long long)gc * a.n_chunks) * kFragF16 + lane * 16;

  for (int r0 = 0; r0 < rounds; r0 += 2) {
    // ---- this wave's weight fragments of up to two chunks, straight into MFMA operand registers
    float4 bq[2][2][9];
    bool valid[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int c = c_begin + (r0 + q) * kw + ks;
      valid[q] = active && (r0 + q) < rounds && c < c_end;
      const unsigned char* wc = wg + (long long)min(c, a.n_chunks - 1) * kFragF16;
      if (valid[q]) {
#pragma unroll
        for (int p = 0; p < 2; ++p)
#pragma unroll
          for (int tp = 0; tp < 9; ++tp) bq[q][p][tp] = *reinterpret_cast<const float4*>(wc + (tp * 2 + p) * 1024);
      }
    }
    // ---- the workgroup's halo of the same chunks, float32, and its per-pixel maxima
    const int c0 = c_begin + r0 * kw;
    const int n_st = min(2 * kw, c_end - c0);
    switch (a.s_in) {
      case 1: lat_stage_f16<1, HW, HP>(a, halo, pm, t, bi, ty0 - 1, tx0 - 1, c0, n_st); break;
      case 2: lat_stage_f16<2, HW, HP>(a, halo, pm, t, bi, ty0 - 1, tx0 - 1, c0, n_st); break;
      case 3: lat_stage_f16<3, HW, HP>(a, halo, pm, t, bi, ty0 - 1, tx0 - 1, c0, n_st); break;
      default: lat_stage_f16<4, HW, HP>(a, halo, pm, t, bi, ty0 - 1, tx0 - 1, c0, n_st); break;
    }
    __syncthreads();
    if (valid[0]) {                                   // (valid[1] implies valid[0])
      // ---- row scales of this round: 2^s_m from the 3x3 window of pixel m over this wave's chunks
      float Sc[MT];
#pragma unroll
      for (int m = 0; m < MT; ++m) {
        const int my = m / MTX, mx = m % MTX;
        const int hp0 = (my * 4 + (n >> 3)) * HW + mx * 8 + (n & 7);
        unsigned um = 0;
#pragma unroll
        for (int q = 0; q < 2; ++q) {
          if (valid[q]) {
            const unsigned* pq = pm + (q * kw + ks) * HP + hp0;
#pragma unroll
            for (int tp = 0; tp < 9; ++tp) um = max(um, pq[(tp / 3) * HW + tp % 3]);
          }
        }
        // max < 2^(E - 126), E the biased exponent: s = 139 - E keeps 2^s max < 2^13; all-zero / denormal windows -> 2^126
        const int s = min(139 - (int)(um >> 23), 126);
        Sc[m] = __uint_as_float((unsigned)(s + 127) << 23);
        if (kh == 0) ts[m * 32 + n] = -s;
      }
      lat_f32x16 part[MT];
#pragma unroll
      for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) part[m][r] = 0.f;
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        if (valid[q]) {
          const float* ac = halo + (q * kw + ks) * kChunkF + kh * 8;
#pragma unroll
          for (int tp = 0; tp < 9; ++tp) {
            const lat_f16x8 bh = __builtin_bit_cast(lat_f16x8, bq[q][0][tp]);
            const lat_f16x8 bl = __builtin_bit_cast(lat_f16x8, bq[q][1][tp]);
#pragma unroll
            for (int m = 0; m < MT; ++m) {
              const int my = m / MTX, mx = m % MTX;
              const float* ap = ac + ((my * 4 + (n >> 3) + tp / 3) * HW + mx * 8 + (n & 7) + tp % 3) * kRowF;
              const float4 x0 = *reinterpret_cast<const float4*>(ap);
              const float4 x1 = *reinterpret_cast<const float4*>(ap + 4);
              unsigned ah[4], al[4];
              lat_split2_pair(x0.x, x0.y, Sc[m], ah[0], al[0]);
              lat_split2_pair(x0.z, x0.w, Sc[m], ah[1], al[1]);
              lat_split2_pair(x1.x, x1.y, Sc[m], ah[2], al[2]);
              lat_split2_pair(x1.z, x1.w, Sc[m], ah[3], al[3]);
              const lat_f16x8 h = __builtin_bit_cast(lat_f16x8, lat_u32x4{ah[0], ah[1], ah[2], ah[3]});
              const lat_f16x8 l = __builtin_bit_cast(lat_f16x8, lat_u32x4{al[0], al[1], al[2], al[3]});
              part[m] = __builtin_amdgcn_mfma_f32_32x32x16_f16(h, bl, part[m], 0, 0, 0);      // small products first
              part[m] = __builtin_amdgcn_mfma_f32_32x32x16_f16(l, bh, part[m], 0, 0, 0);
              part[m] = __builtin_amdgcn_mfma_f32_32x32x16_f16(h, bh, part[m], 0, 0, 0);
            }
          }
        }
      }
      // ---- unscale (2^-(s_m + t_n), exact) and add to the running sums; register r holds row (r & 3) + 8 (r >> 2) + 4 kh
#pragma unroll
      for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
          const int4 ne = *reinterpret_cast<const int4*>(ts + m * 32 + 8 * g4 + 4 * kh);
          acc[m][4 * g4 + 0] += __builtin_ldexpf(part[m][4 * g4 + 0], ne.x - my_t);
          acc[m][4 * g4 + 1] += __builtin_ldexpf(part[m][4 * g4 + 1], ne.y - my_t);
          acc[m][4 * g4 + 2] += __builtin_ldexpf(part[m][4 * g4 + 2], ne.z - my_t);
          acc[m][4 * g4 + 3] += __builtin_ldexpf(part[m][4 * g4 + 3], ne.w - my_t);
        }
    }
    if (r0 + 2 < rounds) __syncthreads();             // the next stage overwrites the halo
  }
  // ---- K sub-slices of the workgroup's waves, added in wave order through LDS (m4d_convlat.hip)
  if (kw > 1) {
    __syncthreads();                                  // the reduction buffer aliases the halo
    float* red = lds_dyn;                             // [kw - 1][cgw][MT][16][64]
    if (ks > 0) {
#pragma unroll
      for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) red[((((ks - 1) * cgw + cg) * MT + m) * 16 + r) * 64 + lane] = acc[m][r];
    }
    __syncthreads();
    if (ks == 0) {
      for (int k = 1; k < kw; ++k)
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[m][r] += red[((((k - 1) * cgw + cg) * MT + m) * 16 + r) * 64 + lane];
    }
  }
  if (ks == 0 && active && co < a.Cout) {
    float* op = a.out + bz * a.out_slab + (long long)bi * a.oh * a.ow * a.Cout + co;
    const bool final_out = a.s_out == 1;
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      const int my = m / MTX, mx = m % MTX;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int mr = (r & 3) + 8 * (r >> 2) + 4 * kh;
        const int oy = ty0 + my * 4 + (mr >> 3), ox = tx0 + mx * 8 + (mr & 7);
        if (oy < a.oh && ox < a.ow) {
          float v = acc[m][r];
          if (final_out) { v += my_bias; v = v > 0.f ? v : v * a.slope; }
          op[((long long)oy * a.ow + ox) * a.Cout] = v;
        }
      }
    }
  }
}

template <int MTX, int MTY>
int lat_f16_launch(const LatArgs& a, int kw, hipStream_t s) {
  constexpr int HP = (8 * MTX + 2) * (4 * MTY + 2), MT = MTX * MTY;
  const int cgw = 4 / kw;
  const size_t lds_a = (size_t)2 * kw * HP * (kRowF + 1) * 4 + 4 * MT * 32 * 4;      // halo + pixel maxima + the waves' -s_m
  const size_t lds_r = (size_t)(kw - 1) * cgw * MT * 16 * 64 * 4;
  const size_t lds = lds_a > lds_r ? lds_a : lds_r;
  M4D_CHECK_ARG(lds <= 160 * 1024);
  if (lds > 64 * 1024) M4D_LDS_OPT_IN(&conv3x3_lat_f16_kernel<MTX, MTY>);
  const dim3 grid((unsigned)(a.b * a.tiles_x * a.tiles_y), (unsigned)((a.n_groups + cgw - 1) / cgw), (unsigned)a.s_out);
  m4d_launch(conv3x3_lat_f16_kernel<MTX, MTY>, grid, dim3(256), lds, s, a);
  return 0;
}

}  // namespace

extern "C" int m4d_conv3x3_lat_f16(const float* x, int s_in, long long x_slab_floats, const float* x_bias, float x_slope,
                                   const void* wp, const float* bias, int b, int h, int w, int Cin, int Cout, float slope,
                                   int mt, int kw, int s_out, float* out, long long out_slab_floats, void* stream) {
  M4D_CHECK_ARG(mt == 1 || mt == 2 || mt == 4);       // (no M-over-waves form)
  M4D_CHECK_ARG((((uintptr_t)wp) & 15u) == 0);
  LatArgs a;
  const int rc = lat_make_args(a, kw, x, s_in, x_slab_floats, x_bias, x_slope, wp, bias, b, h, w, Cin, Cout, 1, slope, mt, s_out,
                               out, out_slab_floats);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  const int rl = mt == 1 ? lat_f16_launch<1, 1>(a, kw, s) : mt == 2 ? lat_f16_launch<1, 2>(a, kw, s) : lat_f16_launch<2, 2>(a, kw, s);
  if (rl) return rl;
  return M4D_LAUNCH_RESULT();
}
