// Training summaries (main.py --log_dir): one launch turns the maps a TensorBoard image summary shows -- the last frame's
// image, the re-projected previous image, the ground-truth log depth and every pyramid level's estimate, each at its own
// resolution -- into uint8 images, so that only bytes leave the device and the host only compresses
// (m4depth_network.py:401-415; the float -> uint8 rule is the one written in include/m4depth_hip.h).  One IEEE float32
// rounding per operation (-ffp-contract=off).
//
// Mapping: an image of a map is a flat run of h*w*c floats -> as many bytes.  One lane = kRun consecutive elements of one
// image: one 16-byte load and one packed 4-byte store when both addresses allow it, guarded element accesses otherwise (the
// ragged end of an image, an odd-sized image behind the first, a view at an odd offset).  Every map owns a contiguous range of
// workgroups, so the per-map lookup is uniform over the workgroup; the descriptors travel by value in the kernel arguments.
#include "m4d_common.h"
#include "../../include/m4depth_hip.h"

#include <algorithm>
#include <utility>

namespace {

constexpr int kRun = 4;
constexpr int kMaxMaps = 16;
constexpr int kThreads = 256;
constexpr float kLog200 = 5.29831737f;                        // the float32 nearest to ln 200

struct SummaryMaps {
  const float* src[kMaxMaps];
  long long stride[kMaxMaps];                                 // floats between images
  long long out_offset[kMaxMaps];
  long long elems[kMaxMaps];                                  // h * w * c: floats of an image = bytes of its output
  unsigned first_block[kMaxMaps + 1];                         // map m owns workgroups first_block[m] .. first_block[m+1]
  int kind[kMaxMaps];
};

// convert_image_dtype(float32 -> uint8, saturate=True): scale by 255.5, saturate, truncate
__device__ __forceinline__ unsigned quantize(float v) {
  if (v != v) return 0u;
  const float t = v * 255.5f;
  if (t < 0.0f) return 0u;
  if (t >= 255.0f) return 255u;
  return (unsigned)t;
}
__device__ __forceinline__ unsigned to_byte(float v, int kind) {
  if (kind == 1) v = logf(fminf(fmaxf(v, 1.0f), 200.0f)) / kLog200;      // fmaxf(NaN, 1) = 1: a NaN depth is black
  return quantize(v);
}

__global__ void __launch_bounds__(kThreads)
summary_images_kernel(SummaryMaps maps, int n_maps, int n, uint8_t* __restrict__ out) {
  int m = 0;
  while (m + 1 < n_maps && blockIdx.x >= maps.first_block[m + 1]) ++m;       // uniform over the workgroup
  const long long elems = maps.elems[m];
  const long long runs_per_image = (elems + kRun - 1) / kRun;
  const long long run = (long long)(blockIdx.x - maps.first_block[m]) * kThreads + threadIdx.x;
  if (run >= runs_per_image * n) return;
  const long long img = run / runs_per_image;
  const long long e0 = (run - img * runs_per_image) * kRun;
  const int cnt = (int)min((long long)kRun, elems - e0);
  const int kind = maps.kind[m];
  const float* __restrict__ p = maps.src[m] + img * maps.stride[m] + e0;
  uint8_t* __restrict__ o = out + maps.out_offset[m] + img * elems + e0;

  float v[kRun];
  if (cnt == kRun && (((uintptr_t)p) & 15u) == 0) {
    typedef float f32x4 __attribute__((ext_vector_type(4)));
    const f32x4 q = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p));      // read once
    v[0] = q[0]; v[1] = q[1]; v[2] = q[2]; v[3] = q[3];
  } else {
#pragma unroll
    for (int e = 0; e < kRun; ++e) v[e] = e < cnt ? p[e] : 0.0f;
  }
  unsigned b[kRun];
#pragma unroll
  for (int e = 0; e < kRun; ++e) b[e] = to_byte(v[e], kind);
  if (cnt == kRun && (((uintptr_t)o) & 3u) == 0) {
    *reinterpret_cast<unsigned*>(o) = b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24);
  } else {
#pragma unroll
    for (int e = 0; e < kRun; ++e) if (e < cnt) o[e] = (uint8_t)b[e];
  }
}

}  // namespace

extern "C" int m4d_summary_images(int n_maps, const float* const* src, const long long* stride, const int* h, const int* w,
                                  const int* c, const int* kind, const long long* out_offset, int n, uint8_t* out,
                                  void* stream) {
  M4D_CHECK_ARG(n_maps >= 1 && n_maps <= kMaxMaps && n >= 1);
  M4D_CHECK_ARG(src && stride && h && w && c && kind && out_offset && out);
  SummaryMaps maps = {};
  std::pair<long long, long long> ranges[kMaxMaps];           // [begin, end) of every map's output bytes
  unsigned long long blocks = 0;
  for (int m = 0; m < n_maps; ++m) {
    M4D_CHECK_ARG(src[m] && (((uintptr_t)src[m]) & 3u) == 0);
    M4D_CHECK_ARG(h[m] > 0 && w[m] > 0 && (c[m] == 1 || c[m] == 3) && (kind[m] == 0 || kind[m] == 1));
    const long long elems = (long long)h[m] * w[m] * c[m];
    M4D_CHECK_ARG(stride[m] >= elems && out_offset[m] >= 0);
    maps.src[m] = src[m];
    maps.stride[m] = stride[m];
    maps.out_offset[m] = out_offset[m];
    maps.elems[m] = elems;
    maps.kind[m] = kind[m];
    maps.first_block[m] = (unsigned)blocks;
    const unsigned long long runs = (unsigned long long)((elems + kRun - 1) / kRun) * (unsigned long long)n;
    blocks += (runs + kThreads - 1) / kThreads;
    M4D_CHECK_ARG(blocks <= 0x7FFFFFFFull);
    ranges[m] = {out_offset[m], out_offset[m] + elems * n};
  }
  for (int m = n_maps; m <= kMaxMaps; ++m) maps.first_block[m] = (unsigned)blocks;
  std::sort(ranges, ranges + n_maps);
  for (int m = 1; m < n_maps; ++m) M4D_CHECK_ARG(ranges[m].first >= ranges[m - 1].second);
  m4d_launch(summary_images_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream, maps, n_maps, n, out);
  return M4D_LAUNCH_RESULT();
}
