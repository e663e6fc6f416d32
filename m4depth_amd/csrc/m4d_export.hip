// Data back end: the mirror of m4d_data.hip.  One launch turns the depth estimate of a frame batch into what goes to disk --
// the datasets' own 16-bit encodings (KITTI uint16 = depth * 256; Mid-Air uint16 = float16 bits of 512 / depth, the formats
// m4d_decode_depth_resize reads) and ready-to-save RGB8 panels (image, colourised estimate / ground truth / relative error)
// stacked vertically -- so that 2 bytes per pixel (+ 3 per panel) cross PCIe instead of the float32 map, and the host only
// compresses.  One IEEE float32 rounding per operation in the order written in include/m4depth_hip.h: a numpy restatement
// agrees bit for bit (-ffp-contract=off, correctly rounded division; rintf = round half to even = np.rint).
//
// Mapping: one lane = a run of kRun consecutive pixels of one row; a full, aligned run is read with 16-byte loads and written
// with 8-byte (depth16) / 3 x 4-byte (one panel's 12 bytes) stores, a ragged row end or a misaligned run (odd widths, views)
// goes through guarded element accesses.  The colour table sits in LDS as one packed word per entry.
#include "m4d_common.h"
#include "../../include/m4depth_hip.h"

namespace {

constexpr int kRun = 4;
constexpr int kLut = 257;                                     // 256 colours + the invalid colour

inline int grid1d(long long n) { long long g = (n + 255) / 256; return (int)(g > 65535 ? 65535 : (g < 1 ? 1 : g)); }

struct PanelKinds { int k[4]; };

__device__ __forceinline__ bool valid_depth(float d) { return isfinite(d) && d > 0.0f; }

// n (0..4) floats from p, the rest `fill`; one 16-byte load when all four are there and p allows it
__device__ __forceinline__ void load_run(const float* __restrict__ p, int n, float fill, float (&v)[kRun]) {
  if (n == kRun && (((uintptr_t)p) & 15u) == 0) {
    typedef float f32x4 __attribute__((ext_vector_type(4)));
    const f32x4 q = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p));    // read once: streamed past the caches
    v[0] = q[0]; v[1] = q[1]; v[2] = q[2]; v[3] = q[3];
  } else {
#pragma unroll
    for (int e = 0; e < kRun; ++e) v[e] = e < n ? p[e] : fill;
  }
}

__device__ __forceinline__ unsigned kitti16(float d) {
  return valid_depth(d) ? (unsigned)fminf(fmaxf(rintf(d * 256.0f), 1.0f), 65535.0f) : 0u;
}
__device__ __forceinline__ unsigned midair16(float d) {
  if (!valid_depth(d)) return 0x7C00u;
  return (unsigned)__half_as_ushort(__float2half_rn(512.0f / d));        // an overflowing quotient is +Inf = 0x7C00 too
}
__device__ __forceinline__ int depth_index(float d, float inv_far, float inv_span) {
  if (!valid_depth(d)) return 256;
  const float t = (1.0f / d - inv_far) / inv_span;
  return (int)rintf(fminf(fmaxf(t, 0.0f), 1.0f) * 255.0f);
}
__device__ __forceinline__ int error_index(float est, float gt, float err_max) {
  if (!(valid_depth(est) && valid_depth(gt))) return 256;
  const float r = (fabsf(est - gt) / gt) / err_max;
  return (int)rintf(fminf(r, 1.0f) * 255.0f);
}
__device__ __forceinline__ unsigned rgb_byte(float v) {                    // fmaxf(NaN, 0) = 0: a NaN channel is black
  return (unsigned)rintf(fminf(fmaxf(v, 0.0f), 1.0f) * 255.0f);
}

__global__ void __launch_bounds__(256)
depth_export_kernel(const float* __restrict__ est, long long est_stride, const float* __restrict__ gt, long long gt_stride,
                    const float* __restrict__ rgb, long long rgb_stride, int h, int w, int runs_per_row, long long total_runs,
                    int format, uint16_t* __restrict__ depth16, int n_panels, PanelKinds kinds,
                    const uint8_t* __restrict__ lut, float near, float far, float err_max, uint8_t* __restrict__ panels) {
  __shared__ unsigned s_lut[kLut];                            // r | g << 8 | b << 16
  bool need_gt = false, need_rgb = false, need_lut = false;
  for (int p = 0; p < n_panels; ++p) {
    need_rgb |= kinds.k[p] == 0;
    need_gt |= kinds.k[p] >= 2;
    need_lut |= kinds.k[p] != 0;
  }
  if (need_lut) {
    for (int i = threadIdx.x; i < kLut; i += blockDim.x)
      s_lut[i] = (unsigned)lut[i * 3] | ((unsigned)lut[i * 3 + 1] << 8) | ((unsigned)lut[i * 3 + 2] << 16);
    __syncthreads();
  }
  const float inv_far = 1.0f / far;
  const float inv_span = 1.0f / near - inv_far;

  for (long long run = (long long)blockIdx.x * blockDim.x + threadIdx.x; run < total_runs;
       run += (long long)gridDim.x * blockDim.x) {
    const int x0 = (int)(run % runs_per_row) * kRun;
    const long long row = run / runs_per_row;                 // image * h + y
    const int y = (int)(row % h);
    const long long img = row / h;
    const int n = min(kRun, w - x0);
    const long long pix = (long long)y * w + x0;              // inside the image

    float e[kRun], g[kRun];
    load_run(est + img * est_stride + pix, n, 0.0f, e);
    if (need_gt) load_run(gt + img * gt_stride + pix, n, 0.0f, g);

    if (format != 0) {
      unsigned q[kRun];
#pragma unroll
      for (int i = 0; i < kRun; ++i) q[i] = format == 1 ? kitti16(e[i]) : midair16(e[i]);
      uint16_t* o = depth16 + row * w + x0;
      const unsigned lo = q[0] | (q[1] << 16), hi = q[2] | (q[3] << 16);
      if (n == kRun && (((uintptr_t)o) & 7u) == 0) {
        *reinterpret_cast<uint2*>(o) = make_uint2(lo, hi);
      } else if (n == kRun && (((uintptr_t)o) & 3u) == 0) {
        reinterpret_cast<unsigned*>(o)[0] = lo;
        reinterpret_cast<unsigned*>(o)[1] = hi;
      } else {
#pragma unroll
        for (int i = 0; i < kRun; ++i) if (i < n) o[i] = (uint16_t)q[i];
      }
    }

    float c[3][kRun];                                          // the run's 12 colour floats, as three 16-byte pieces
    if (need_rgb) {
      const float* src = rgb + img * rgb_stride + pix * 3;
#pragma unroll
      for (int k = 0; k < 3; ++k) load_run(src + k * kRun, min(max(3 * n - k * kRun, 0), kRun), 0.0f, c[k]);
    }

    for (int p = 0; p < n_panels; ++p) {
      const int kind = kinds.k[p];
      unsigned col[kRun];                                      // r | g << 8 | b << 16 of each pixel
#pragma unroll
      for (int i = 0; i < kRun; ++i) {
        if (kind == 0) {
          const int f = 3 * i;                                 // compile-time after unrolling
          col[i] = rgb_byte(c[f / kRun][f % kRun]) | (rgb_byte(c[(f + 1) / kRun][(f + 1) % kRun]) << 8) |
                   (rgb_byte(c[(f + 2) / kRun][(f + 2) % kRun]) << 16);
        } else {
          const int idx = kind == 1 ? depth_index(e[i], inv_far, inv_span)
                        : kind == 2 ? depth_index(g[i], inv_far, inv_span) : error_index(e[i], g[i], err_max);
          col[i] = s_lut[idx];
        }
      }
      uint8_t* o = panels + (((img * n_panels + p) * h + y) * (long long)w + x0) * 3;
      if (n == kRun && (((uintptr_t)o) & 3u) == 0) {
        unsigned* o4 = reinterpret_cast<unsigned*>(o);
        o4[0] = col[0] | (col[1] << 24);
        o4[1] = (col[1] >> 8) | (col[2] << 16);
        o4[2] = (col[2] >> 16) | (col[3] << 8);
      } else {
#pragma unroll
        for (int i = 0; i < kRun; ++i) {
          if (i < n) {
            o[3 * i] = (uint8_t)col[i];
            o[3 * i + 1] = (uint8_t)(col[i] >> 8);
            o[3 * i + 2] = (uint8_t)(col[i] >> 16);
          }
        }
      }
    }
  }
}

}  // namespace

extern "C" int m4d_depth_export(const float* est, long long est_stride, const float* gt, long long gt_stride, const float* rgb,
                                long long rgb_stride, int b, int h, int w, int format, uint16_t* depth16, int n_panels,
                                const int* panel_kinds, const uint8_t* lut, float near, float far, float err_max,
                                uint8_t* panels, void* stream) {
  M4D_CHECK_ARG(est && b > 0 && h > 0 && w > 0);
  M4D_CHECK_ARG(format >= 0 && format <= 2 && n_panels >= 0 && n_panels <= 4);
  M4D_CHECK_ARG(format != 0 || n_panels > 0);                 // something to write
  M4D_CHECK_ARG(format == 0 || depth16);
  M4D_CHECK_ARG(near > 0.0f && far > near && err_max > 0.0f);
  const long long per_image = (long long)h * w;
  M4D_CHECK_ARG(est_stride >= per_image && (!gt || gt_stride >= per_image) && (!rgb || rgb_stride >= 3 * per_image));
  M4D_CHECK_ARG(((((uintptr_t)est) | ((uintptr_t)gt) | ((uintptr_t)rgb)) & 3u) == 0 && (((uintptr_t)depth16) & 1u) == 0);
  PanelKinds kinds = {{0, 0, 0, 0}};
  if (n_panels > 0) {
    M4D_CHECK_ARG(panel_kinds && panels);
    for (int p = 0; p < n_panels; ++p) {
      const int k = panel_kinds[p];
      M4D_CHECK_ARG(k >= 0 && k <= 3);
      M4D_CHECK_ARG(k != 0 || rgb);
      M4D_CHECK_ARG(k == 0 || lut);
      M4D_CHECK_ARG(k < 2 || gt);
      kinds.k[p] = k;
    }
  }
  const int runs_per_row = (w + kRun - 1) / kRun;
  const long long total_runs = (long long)b * h * runs_per_row;
  m4d_launch(depth_export_kernel, dim3(grid1d(total_runs)), dim3(256), 0, (hipStream_t)stream, est, est_stride, gt, gt_stride,
             rgb, rgb_stride, h, w, runs_per_row, total_runs, format, depth16, n_panels, kinds, lut, near, far, err_max, panels);
  return M4D_LAUNCH_RESULT();
}
