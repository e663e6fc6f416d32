// Data front end for a user's own recording (dataloaders/recording.py): lens undistortion fused with the cast and resize
// that m4d_data.hip does for the benchmark datasets.  The network assumes a pinhole camera (get_coords_2d, reproject), so
// the loader picks a pinhole OUTPUT camera and every output pixel is looked up in the distorted source frame:
//   m4d_undistort_map        once per recording: output pixel -> source index coordinates (u, v), or (-1, -1) = no source
//   m4d_decode_rgb8_remap    per frame batch: u8 -> /255 -> bilinear at (u, v), the Axis / lerp2 arithmetic of m4d_data.hip
//   m4d_decode_depth16_remap per frame batch: uint16 -> nearest at (u, v) -> * inv_scale
// The host still uploads only the decoder's raw frame.  One IEEE rounding per operation in the order include/m4depth_hip.h
// states (tests/recording_ref.py restates it in numpy): the radtan and pinhole maps and both samplers are bit-exact.
#include "m4d_common.h"
#include "../../include/m4depth_hip.h"

namespace {

inline int grid1d(long long n) { long long g = (n + 255) / 256; return (int)(g > 65535 ? 65535 : (g < 1 ? 1 : g)); }

struct Camera { float fx, fy, cx, cy; };
struct Distortion { float k[5]; };

template <int MODEL>
__global__ void __launch_bounds__(256)
undistort_map_kernel(Distortion d, Camera src, Camera dst, int ih, int iw, int ow, long long total, float2* __restrict__ map) {
  const float u_max = (float)iw - 0.5f, v_max = (float)ih - 0.5f;
  for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (long long)gridDim.x * blockDim.x) {
    const int col = (int)(idx % ow);
    const int row = (int)(idx / ow);
    const float x = (((float)col + 0.5f) - dst.cx) / dst.fx;
    const float y = (((float)row + 0.5f) - dst.cy) / dst.fy;
    float xd = x, yd = y;
    if (MODEL == 1) {                                         // radtan (OpenCV / Kalibr): k1 k2 p1 p2 k3
      const float k1 = d.k[0], k2 = d.k[1], p1 = d.k[2], p2 = d.k[3], k3 = d.k[4];
      const float r2 = x * x + y * y;
      const float rad = 1.0f + r2 * (k1 + r2 * (k2 + r2 * k3));
      xd = x * rad + ((((2.0f * p1) * x) * y) + p2 * (r2 + (2.0f * x) * x));
      yd = y * rad + (p1 * (r2 + (2.0f * y) * y) + (((2.0f * p2) * x) * y));
    } else if (MODEL == 2) {                                  // equidistant (OpenCV fisheye / Kalibr): k1..k4
      const float r = sqrtf(x * x + y * y);
      const float th = atanf(r);
      const float th2 = th * th;
      const float thd = th * (1.0f + th2 * (d.k[0] + th2 * (d.k[1] + th2 * (d.k[2] + th2 * d.k[3]))));
      const float s = r > 1e-8f ? thd / r : 1.0f;
      xd = x * s;
      yd = y * s;
    }
    const float u = (xd * src.fx + src.cx) - 0.5f;
    const float v = (yd * src.fy + src.cy) - 0.5f;
    // NaN fails every comparison, +-Inf the range: both end as "no source"
    const bool ok = u >= -0.5f && u <= u_max && v >= -0.5f && v <= v_max;
    map[idx] = ok ? make_float2(u, v) : make_float2(-1.0f, -1.0f);
  }
}

struct Axis { int lo, hi; float lerp; };
__device__ __forceinline__ Axis remap_axis(float src, int in_n) {          // half_pixel_axis of m4d_data.hip after its first line
  const float fl = floorf(src), top = (float)(in_n - 1);        // clamped as floats: the cast never sees a value off the int range
  Axis a;
  a.lo = (int)fminf(fmaxf(fl, 0.0f), top);
  a.hi = (int)fminf(fmaxf(ceilf(src), 0.0f), top);
  a.lerp = src - fl;
  return a;
}
__device__ __forceinline__ float lerp2(float tl, float tr, float bl, float br, float xl, float yl) {
  const float top = tl + (tr - tl) * xl;
  const float bot = bl + (br - bl) * xl;
  return top + (bot - top) * yl;
}
// valid coordinates are >= -0.5 and finite; (-1, -1) is the map's "no source", a NaN or an infinity is treated like it
__device__ __forceinline__ bool has_source(float2 uv) {
  return uv.x >= -0.5f && uv.y >= -0.5f && uv.x < INFINITY && uv.y < INFINITY;
}

// One thread = one output pixel, all three channels: one 8-byte map load (coalesced), four 3-byte gathers, 12 bytes out.
__global__ void __launch_bounds__(256)
rgb8_remap_kernel(const uint8_t* __restrict__ img, const float2* __restrict__ map, int ih, int iw, long long per_out,
                  long long total, float* __restrict__ out) {
  for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (long long)gridDim.x * blockDim.x) {
    const long long n = idx / per_out;
    const float2 uv = map[idx - n * per_out];
    float r = 0.0f, g = 0.0f, b = 0.0f;
    if (has_source(uv)) {
      const uint8_t* p = img + n * ih * iw * 3;
      const Axis xa = remap_axis(uv.x, iw), ya = remap_axis(uv.y, ih);
      const uint8_t* tl = p + ((long long)ya.lo * iw + xa.lo) * 3;
      const uint8_t* tr = p + ((long long)ya.lo * iw + xa.hi) * 3;
      const uint8_t* bl = p + ((long long)ya.hi * iw + xa.lo) * 3;
      const uint8_t* br = p + ((long long)ya.hi * iw + xa.hi) * 3;
      r = lerp2((float)tl[0] / 255.0f, (float)tr[0] / 255.0f, (float)bl[0] / 255.0f, (float)br[0] / 255.0f, xa.lerp, ya.lerp);
      g = lerp2((float)tl[1] / 255.0f, (float)tr[1] / 255.0f, (float)bl[1] / 255.0f, (float)br[1] / 255.0f, xa.lerp, ya.lerp);
      b = lerp2((float)tl[2] / 255.0f, (float)tr[2] / 255.0f, (float)bl[2] / 255.0f, (float)br[2] / 255.0f, xa.lerp, ya.lerp);
    }
    float* o = out + idx * 3;
    o[0] = r; o[1] = g; o[2] = b;
  }
}

__global__ void __launch_bounds__(256)
depth16_remap_kernel(const uint16_t* __restrict__ raw, const float2* __restrict__ map, float inv_scale, int ih, int iw,
                     long long per_out, long long total, float* __restrict__ out) {
  for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (long long)gridDim.x * blockDim.x) {
    const long long n = idx / per_out;
    const float2 uv = map[idx - n * per_out];
    float v = 0.0f;
    if (has_source(uv)) {
      const int xi = (int)fminf(fmaxf(floorf(uv.x + 0.5f), 0.0f), (float)(iw - 1));
      const int yi = (int)fminf(fmaxf(floorf(uv.y + 0.5f), 0.0f), (float)(ih - 1));
      const uint16_t q = raw[n * ih * iw + (long long)yi * iw + xi];
      v = q != 0 ? (float)q * inv_scale : 0.0f;
    }
    out[idx] = v;
  }
}

}  // namespace

extern "C" int m4d_undistort_map(int model, const float* dist, const float src_cam[4], const float out_cam[4], int ih, int iw,
                                 int oh, int ow, float* map, void* stream) {
  M4D_CHECK_ARG(model >= 0 && model <= 2 && src_cam && out_cam && map && ih > 0 && iw > 0 && oh > 0 && ow > 0);
  M4D_CHECK_ARG(model == 0 || dist);
  M4D_CHECK_ARG((((uintptr_t)map) & 7u) == 0);
  Distortion d = {{0.f, 0.f, 0.f, 0.f, 0.f}};
  for (int i = 0; i < (model == 1 ? 5 : model == 2 ? 4 : 0); ++i) d.k[i] = dist[i];
  const Camera src = {src_cam[0], src_cam[1], src_cam[2], src_cam[3]};
  const Camera dst = {out_cam[0], out_cam[1], out_cam[2], out_cam[3]};
  const long long total = (long long)oh * ow;
  float2* m = reinterpret_cast<float2*>(map);
  if (model == 0)
    m4d_launch(undistort_map_kernel<0>, dim3(grid1d(total)), dim3(256), 0, (hipStream_t)stream, d, src, dst, ih, iw, ow, total, m);
  else if (model == 1)
    m4d_launch(undistort_map_kernel<1>, dim3(grid1d(total)), dim3(256), 0, (hipStream_t)stream, d, src, dst, ih, iw, ow, total, m);
  else
    m4d_launch(undistort_map_kernel<2>, dim3(grid1d(total)), dim3(256), 0, (hipStream_t)stream, d, src, dst, ih, iw, ow, total, m);
  return M4D_LAUNCH_RESULT();
}

extern "C" int m4d_decode_rgb8_remap(const uint8_t* images, const float* map, int n, int ih, int iw, int oh, int ow, float* out,
                                     void* stream) {
  M4D_CHECK_ARG(images && map && out && n > 0 && ih > 0 && iw > 0 && oh > 0 && ow > 0);
  M4D_CHECK_ARG((((uintptr_t)map) & 7u) == 0 && (((uintptr_t)out) & 3u) == 0);
  const long long per_out = (long long)oh * ow, total = per_out * n;
  m4d_launch(rgb8_remap_kernel, dim3(grid1d(total)), dim3(256), 0, (hipStream_t)stream, images,
             reinterpret_cast<const float2*>(map), ih, iw, per_out, total, out);
  return M4D_LAUNCH_RESULT();
}

extern "C" int m4d_decode_depth16_remap(const uint16_t* raw, const float* map, float inv_scale, int n, int ih, int iw, int oh,
                                        int ow, float* out, void* stream) {
  M4D_CHECK_ARG(raw && map && out && n > 0 && ih > 0 && iw > 0 && oh > 0 && ow > 0);
  M4D_CHECK_ARG((((uintptr_t)raw) & 1u) == 0 && (((uintptr_t)map) & 7u) == 0 && (((uintptr_t)out) & 3u) == 0);
  const long long per_out = (long long)oh * ow, total = per_out * n;
  m4d_launch(depth16_remap_kernel, dim3(grid1d(total)), dim3(256), 0, (hipStream_t)stream, raw,
             reinterpret_cast<const float2*>(map), inv_scale, ih, iw, per_out, total, out);
  return M4D_LAUNCH_RESULT();
}
