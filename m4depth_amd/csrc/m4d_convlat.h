// LatArgs and the argument checks shared by the latency-first small-map convolutions: m4d_convlat.hip (float32 operands as
// three bf16 terms) and m4d_convlat_f16.hip (two fp16 terms after power-of-two scales).  Both accept the same configurations.
#pragma once
#include "m4d_common.h"

namespace {

typedef float lat_f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 lat_bf16x8 __attribute__((ext_vector_type(8)));

struct LatArgs {
  const float* x; long long x_slab; int s_in;       // input: s_in partial slabs (>= 1), x_slab floats apart
  const float* x_bias; float x_slope;               // the PRODUCER's bias / leaky-relu slope, applied while staging; nullptr = x is final
  const unsigned char* wp;                          // pack_conv_weights_lat: [group][chunk][tap][part][lane][8] bf16
  const float* bias; float slope;                   // this layer's epilogue, applied only when s_out == 1
  float* out; long long out_slab; int s_out;        // s_out K slices = gridDim.z; slice z -> out + z * out_slab (raw partial sums)
  int b, h, w, Cin, Cout, n_chunks, n_groups, tiles_x, tiles_y;
  int cgw_log2, chunks_per_slice;                   // waves = (1 << cgw_log2) cout groups x (4 >> cgw_log2) K sub-slices
  int oh, ow, pad_y, pad_x;                         // output size; TF 'SAME' pad before (1 at stride 1; 0 or 1 at stride 2)
};

constexpr int kLatRow = 24;                         // floats per staged halo pixel and chunk: 3 parts x 16 bf16 = 96 bytes

}  // namespace

// argument checks + LatArgs of one layer (kw: 1 for the M-over-waves form)
static int lat_make_args(LatArgs& a, int& kw, const float* x, int s_in, long long x_slab_floats, const float* x_bias, float x_slope,
                         const void* wp, const float* bias, int b, int h, int w, int Cin, int Cout, int stride, float slope,
                         int mt, int s_out, float* out, long long out_slab_floats) {
  M4D_CHECK_ARG(x && wp && bias && out && b > 0 && h > 0 && w > 0 && (stride == 1 || stride == 2));
  M4D_CHECK_ARG(Cin >= 16 && Cin % 4 == 0 && Cout >= 1);
  const int oh = (h + stride - 1) / stride, ow = (w + stride - 1) / stride;
  M4D_CHECK_ARG(s_in >= 1 && s_in <= 4 && (s_in == 1 || x_slab_floats >= (long long)b * h * w * Cin));
  M4D_CHECK_ARG(s_out >= 1 && (s_out == 1 || out_slab_floats >= (long long)b * oh * ow * Cout));
  M4D_CHECK_ARG((mt == 1 || mt == 2 || mt == 4 || mt == 8) && (kw == 1 || kw == 2 || kw == 4));   // mt 8 = "M over waves" (kw unused)
  if (mt == 8) kw = 1;
  a.x = x; a.x_slab = x_slab_floats; a.s_in = s_in; a.x_bias = x_bias; a.x_slope = x_slope;
  a.wp = reinterpret_cast<const unsigned char*>(wp); a.bias = bias; a.slope = slope;
  a.out = out; a.out_slab = out_slab_floats; a.s_out = s_out;
  a.b = b; a.h = h; a.w = w; a.Cin = Cin; a.Cout = Cout; a.oh = oh; a.ow = ow;
  // TF 'SAME': total pad = max((out - 1) * stride + 3 - in, 0), before = total / 2
  a.pad_y = ((oh - 1) * stride + 3 - h > 0 ? (oh - 1) * stride + 3 - h : 0) / 2;
  a.pad_x = ((ow - 1) * stride + 3 - w > 0 ? (ow - 1) * stride + 3 - w : 0) / 2;
  a.n_chunks = (Cin + 15) / 16; a.n_groups = (Cout + 31) / 32;
  M4D_CHECK_ARG(s_out <= a.n_chunks);
  a.cgw_log2 = kw == 1 ? 2 : (kw == 2 ? 1 : 0);
  a.chunks_per_slice = (a.n_chunks + s_out - 1) / s_out;
  M4D_CHECK_ARG((long long)(s_out - 1) * a.chunks_per_slice < a.n_chunks);     // no empty K slice
  const int mtx = mt >= 4 ? 2 : 1, mty = mt >= 2 ? 2 : 1;
  a.tiles_x = (ow + 8 * mtx - 1) / (8 * mtx); a.tiles_y = (oh + 4 * mty - 1) / (4 * mty);
  // LDS: two staged rounds of kw chunks each
  const size_t lds_a = (size_t)2 * kw * ((8 * mtx - 1) * stride + 3) * ((4 * mty - 1) * stride + 3) * kLatRow * 4;
  M4D_CHECK_ARG(lds_a <= 160 * 1024);
  return 0;
}
