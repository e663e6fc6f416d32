// Point-cloud export: the depth estimate of a frame batch as dense lists of coloured 3-D vertices, in the camera frame or in
// the frame of the trajectory's first camera (include/m4depth_hip.h: m4d_pose_accumulate, m4d_depth_cloud).
//
// The work is a stream compaction whose output order is fixed (raster order), so that the buffer is deterministic:
//   launch 1 (cloud_count_kernel)  one workgroup = kChunk consecutive candidates of one sample (the pixels of the `step`
//            lattice in raster order); it writes how many of them are kept to workspace[sample][workgroup];
//   launch 2 (cloud_write_kernel)  the same mapping; a workgroup sums the counts of the workgroups before it in its sample
//            (plain loads of what launch 1 finished writing: no workgroup waits on another), ranks its own kept candidates
//            with one wave64 ballot + a popcount of the lower lanes (v_mbcnt) per wave and the waves' totals through LDS,
//            and stores each vertex with one 16-byte store.  The last workgroup of a sample writes counts[sample].
// No atomics, no ordering between workgroups of a launch.  The prefix in launch 2 is quadratic in the workgroups of a sample
// (workgroup k reads k ints); at 384 x 1280 with step 1 that is 1920 workgroups reading at most 7.5 KB each from L2.  It is
// meant for camera frames, so a map of more than kMaxCap = 2^24 candidates (4096 x 4096; 65536 workgroups, the last of which
// reads 256 KB) is refused rather than served slowly: beyond that the prefix wants a scan of its own.
#include "m4d_common.h"
#include "../../include/m4depth_hip.h"

namespace {

constexpr int kChunk = 256;                                   // candidates per workgroup = threads per workgroup
constexpr int kWaves = kChunk / 64;
constexpr long long kMaxCap = 1LL << 24;                      // candidates per sample: bounds the quadratic prefix

struct CloudArgs {
  const float* depth; long long depth_stride;
  const float* rgb; long long rgb_stride;
  const float* cam_f; const float* cam_c; const double* pose;
  int h, w, step, cw, cap, nblk;
  float near, far;
};

// candidate k of the sample -> its pixel and depth; whether it is kept
__device__ __forceinline__ bool cloud_candidate(const CloudArgs& a, int s, int k, int& row, int& col, float& d) {
  if (k >= a.cap) return false;
  row = (k / a.cw) * a.step;
  col = (k % a.cw) * a.step;
  d = a.depth[s * a.depth_stride + (long long)row * a.w + col];
  return isfinite(d) && d >= a.near && d <= a.far;
}

__device__ __forceinline__ unsigned cloud_byte(float v) {     // m4d_depth_export's rgb rule; fmaxf(NaN, 0) = 0
  return (unsigned)rintf(fminf(fmaxf(v, 0.0f), 1.0f) * 255.0f);
}

__global__ void __launch_bounds__(kChunk)
cloud_count_kernel(CloudArgs a, int* __restrict__ workspace) {
  __shared__ int s_wave[kWaves];
  const int s = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int row, col; float d;
  const bool keep = cloud_candidate(a, s, blockIdx.x * kChunk + threadIdx.x, row, col, d);
  const unsigned long long mask = __ballot(keep);
  if (lane == 0) s_wave[wave] = __popcll(mask);
  __syncthreads();
  if (threadIdx.x == 0) {
    int n = 0;
#pragma unroll
    for (int i = 0; i < kWaves; ++i) n += s_wave[i];
    workspace[(long long)s * a.nblk + blockIdx.x] = n;
  }
}

__global__ void __launch_bounds__(kChunk)
cloud_write_kernel(CloudArgs a, const int* __restrict__ workspace, uint4* __restrict__ vertices, int* __restrict__ counts) {
  __shared__ int s_wave[kWaves], s_before[kWaves];
  const int s = blockIdx.y, blk = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;

  int before = 0;                                             // kept candidates of the workgroups before this one
  const int* ws = workspace + (long long)s * a.nblk;
  for (int i = threadIdx.x; i < blk; i += kChunk) before += ws[i];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) before += __shfl_down(before, off, 64);

  int row = 0, col = 0; float d = 0.0f;
  const bool keep = cloud_candidate(a, s, blk * kChunk + threadIdx.x, row, col, d);
  const unsigned long long mask = __ballot(keep);
  const int rank = __builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
  if (lane == 0) { s_wave[wave] = __popcll(mask); s_before[wave] = before; }
  __syncthreads();
  int base = 0, total = 0;
#pragma unroll
  for (int i = 0; i < kWaves; ++i) {
    base += s_before[i];
    if (i < wave) base += s_wave[i];
    total += s_wave[i];
  }
  if (threadIdx.x == 0 && blk == a.nblk - 1) {
    int all = total;
#pragma unroll
    for (int i = 0; i < kWaves; ++i) all += s_before[i];
    counts[s] = all;
  }
  if (!keep) return;

  const float fx = a.cam_f[s * 2], fy = a.cam_f[s * 2 + 1], cx = a.cam_c[s * 2], cy = a.cam_c[s * 2 + 1];
  float x = ((((float)col + 0.5f) - cx) / fx) * d;            // get_coords_2d's operand order, then * depth
  float y = ((((float)row + 0.5f) - cy) / fy) * d;
  float z = d;
  if (a.pose) {                                               // Rw X + tw in float64, one rounding to float32
    const double* p = a.pose + s * 7;
    double r[9];
    m4d_rot64(p, r);
    const double X = x, Y = y, Z = z;
    x = (float)(((r[0] * X + r[1] * Y) + r[2] * Z) + p[4]);
    y = (float)(((r[3] * X + r[4] * Y) + r[5] * Z) + p[5]);
    z = (float)(((r[6] * X + r[7] * Y) + r[8] * Z) + p[6]);
  }
  const float* c = a.rgb + s * a.rgb_stride + ((long long)row * a.w + col) * 3;
  const unsigned rgba = cloud_byte(c[0]) | (cloud_byte(c[1]) << 8) | (cloud_byte(c[2]) << 16) | 0xFF000000u;
  vertices[(long long)s * a.cap + (base + rank)] =
      make_uint4(__float_as_uint(x), __float_as_uint(y), __float_as_uint(z), rgba);
}

// one lane = one sample
__global__ void __launch_bounds__(64)
pose_accumulate_kernel(const unsigned char* __restrict__ reset, int force_all, const float* __restrict__ rot,
                       const float* __restrict__ trans, int b, double* __restrict__ pose) {
  const int s = blockIdx.x * 64 + threadIdx.x;
  if (s >= b) return;
  double* p = pose + s * 7;
  if (force_all || (reset && reset[s])) {
    p[0] = 1.0; p[1] = 0.0; p[2] = 0.0; p[3] = 0.0; p[4] = 0.0; p[5] = 0.0; p[6] = 0.0;
    return;
  }
  double w = rot[s * 4], x = rot[s * 4 + 1], y = rot[s * 4 + 2], z = rot[s * 4 + 3];
  const double n = sqrt(((w * w + x * x) + y * y) + z * z);
  w /= n; x /= n; y /= n; z /= n;
  const double pw = p[0], px = p[1], py = p[2], pz = p[3];
  const double t0 = trans[s * 3], t1 = trans[s * 3 + 1], t2 = trans[s * 3 + 2];
  double r[9];                                                // tw <- R(p) t + tw
  m4d_rot64(p, r);
  p[4] = ((r[0] * t0 + r[1] * t1) + r[2] * t2) + p[4];
  p[5] = ((r[3] * t0 + r[4] * t1) + r[5] * t2) + p[5];
  p[6] = ((r[6] * t0 + r[7] * t1) + r[8] * t2) + p[6];
  // Rw <- Rw R: the Hamilton product p q, renormalised
  double rw = ((pw * w - px * x) - py * y) - pz * z;
  double rx = ((pw * x + px * w) + py * z) - pz * y;
  double ry = ((pw * y - px * z) + py * w) + pz * x;
  double rz = ((pw * z + px * y) - py * x) + pz * w;
  const double m = sqrt(((rw * rw + rx * rx) + ry * ry) + rz * rz);
  p[0] = rw / m; p[1] = rx / m; p[2] = ry / m; p[3] = rz / m;
}

inline bool cloud_geometry(int b, int h, int w, int step, long long& cw, long long& cap, long long& nblk) {
  if (b <= 0 || h <= 0 || w <= 0 || step < 1) return false;
  cw = (w + (long long)step - 1) / step;
  cap = ((h + (long long)step - 1) / step) * cw;
  nblk = (cap + kChunk - 1) / kChunk;
  return cap <= kMaxCap && b <= 65535;                        // (candidate indices stay ints;) b is the grid's y
}

}  // namespace

extern "C" long long m4d_depth_cloud_workspace_ints(int b, int h, int w, int step) {
  long long cw, cap, nblk;
  return cloud_geometry(b, h, w, step, cw, cap, nblk) ? b * nblk : 0;
}

extern "C" int m4d_pose_accumulate(const unsigned char* reset, int force_all, const float* rot, const float* trans, int b,
                                   double* pose, void* stream) {
  M4D_CHECK_ARG(rot && trans && pose && b > 0);
  M4D_CHECK_ARG(((((uintptr_t)rot) | ((uintptr_t)trans)) & 3u) == 0 && (((uintptr_t)pose) & 7u) == 0);
  m4d_launch(pose_accumulate_kernel, dim3((unsigned)((b + 63) / 64)), dim3(64), 0, (hipStream_t)stream, reset, force_all, rot,
             trans, b, pose);
  return M4D_LAUNCH_RESULT();
}

extern "C" int m4d_depth_cloud(const float* depth, long long depth_stride, const float* rgb, long long rgb_stride,
                               const float* cam_f, const float* cam_c, const double* pose, int b, int h, int w, int step,
                               float near, float far, void* vertices, int* counts, int* workspace, void* stream) {
  long long cw, cap, nblk;
  M4D_CHECK_ARG(depth && rgb && cam_f && cam_c && vertices && counts && workspace);
  M4D_CHECK_ARG(cloud_geometry(b, h, w, step, cw, cap, nblk));
  M4D_CHECK_ARG(far > near);                                  // false for a NaN bound
  const long long per_image = (long long)h * w;
  M4D_CHECK_ARG(depth_stride >= per_image && rgb_stride >= 3 * per_image);
  M4D_CHECK_ARG(((((uintptr_t)depth) | ((uintptr_t)rgb) | ((uintptr_t)cam_f) | ((uintptr_t)cam_c) | ((uintptr_t)counts) |
                  ((uintptr_t)workspace)) & 3u) == 0);
  M4D_CHECK_ARG((((uintptr_t)pose) & 7u) == 0 && (((uintptr_t)vertices) & 15u) == 0);
  const CloudArgs a = {depth, depth_stride, rgb, rgb_stride, cam_f, cam_c, pose, h, w, step, (int)cw, (int)cap, (int)nblk,
                       near, far};
  const dim3 grid((unsigned)nblk, (unsigned)b);
  m4d_launch(cloud_count_kernel, grid, dim3(kChunk), 0, (hipStream_t)stream, a, workspace);
  m4d_launch(cloud_write_kernel, grid, dim3(kChunk), 0, (hipStream_t)stream, a, (const int*)workspace, (uint4*)vertices, counts);
  return M4D_LAUNCH_RESULT();
}
