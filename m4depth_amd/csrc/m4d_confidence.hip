// Multi-view depth check: a pixel of the current estimate is confirmed by an earlier frame of its trajectory when its 3-D
// point, projected into that frame, lands on a surface that frame estimated too and that surface projects back onto the pixel
// (include/m4depth_hip.h: m4d_depth_views).  The forward-backward reprojection test of multi-view stereo fusion.
//
// One launch.  A thread owns four consecutive pixels of the flattened map (one dword of counts, 16 bytes of depth_f and of the
// ring copy when the geometry allows vector stores; the element path otherwise).  The relative transforms of the views (12
// doubles each) are computed once per workgroup by its first `a` threads and staged in LDS; a pixel then does about 65 float64
// operations per view, four of them divisions, and four gathered taps.  The ring slot written (`head`) is never one of the
// slots read, so no workgroup waits on another; no atomics, no zero-fill: every output element has exactly one writer.
#include "m4d_common.h"
#include "../../include/m4depth_hip.h"

namespace {

constexpr int kThreads = 256;
constexpr int kPerThread = 4;
constexpr int kMaxViews = 8;
constexpr long long kMaxPixels = 1LL << 24;

struct ViewsArgs {
  const float* depth; long long depth_stride;
  const float* cam_f; const float* cam_c; const double* pose;
  const unsigned char* reset; int force_all;
  int b, h, w, hw, views, head;
  float* ring_depth; double* ring_pose;
  const int* age_in; int* age_out;
  float tol_px, tol_rel; int min_views;
  unsigned char* n_views; float* depth_f;
};

template <bool kVec>
__global__ void __launch_bounds__(kThreads)
depth_views_kernel(ViewsArgs a) {
  __shared__ double s_t[kMaxViews][12];                       // per view: Rr (row-major), tr
  const int s = blockIdx.y, K = a.views, slots = K + 1;
  const bool fresh = a.force_all || (a.reset && a.reset[s]);
  const int age = fresh ? 0 : min(max(a.age_in[s], 0), K);

  if ((int)threadIdx.x < age) {                               // view j = threadIdx.x + 1
    const int slot = (a.head + slots - ((int)threadIdx.x + 1)) % slots;
    const double* pk = a.ring_pose + ((long long)slot * a.b + s) * 7;
    const double* pc = a.pose + s * 7;
    double rk[9], rc[9];
    m4d_rot64(pk, rk);
    m4d_rot64(pc, rc);
    double* t = s_t[threadIdx.x];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j)                             // Rr = R(qk)^T R(qc)
        t[i * 3 + j] = (rk[i] * rc[j] + rk[3 + i] * rc[3 + j]) + rk[6 + i] * rc[6 + j];
    const double d0 = pc[4] - pk[4], d1 = pc[5] - pk[5], d2 = pc[6] - pk[6];
#pragma unroll
    for (int i = 0; i < 3; ++i) t[9 + i] = (rk[i] * d0 + rk[3 + i] * d1) + rk[6 + i] * d2;   // tr = R(qk)^T (tc - tk)
  }
  if (blockIdx.x == 0) {                                      // the sample's state: one writer each
    if (threadIdx.x < 7) a.ring_pose[((long long)a.head * a.b + s) * 7 + threadIdx.x] = a.pose[s * 7 + threadIdx.x];
    if (threadIdx.x == 7) a.age_out[s] = min(age + 1, K);
  }
  __syncthreads();

  const int p0 = (blockIdx.x * kThreads + (int)threadIdx.x) * kPerThread;
  if (p0 >= a.hw) return;
  const float fx = a.cam_f[s * 2], fy = a.cam_f[s * 2 + 1], cx = a.cam_c[s * 2], cy = a.cam_c[s * 2 + 1];
  const double fxd = fx, fyd = fy, cxd = cx, cyd = cy;
  const double tol2 = (double)a.tol_px * (double)a.tol_px, rel = a.tol_rel;
  const double umax = (double)(a.w - 1), vmax = (double)(a.h - 1);
  const float* src = a.depth + s * a.depth_stride;
  const long long plane = (long long)a.b * a.hw;

  float d[kPerThread];
  if (kVec) {
    const float4 v = *reinterpret_cast<const float4*>(src + p0);
    d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
  } else {
#pragma unroll
    for (int e = 0; e < kPerThread; ++e) d[e] = p0 + e < a.hw ? src[p0 + e] : 0.0f;
  }

  unsigned n[kPerThread];
#pragma unroll
  for (int e = 0; e < kPerThread; ++e) {
    n[e] = 0;
    const float de = d[e];
    if (p0 + e >= a.hw || !(isfinite(de) && de > 0.0f)) continue;
    const int row = (p0 + e) / a.w, col = (p0 + e) - row * a.w;
    const double xc = (((float)col + 0.5f) - cx) / fx * de;   // float32: m4d_depth_cloud's operand order
    const double yc = (((float)row + 0.5f) - cy) / fy * de;
    const double zc = de;
    for (int j = 0; j < age; ++j) {
      const double* t = s_t[j];
      const double X = ((t[0] * xc + t[1] * yc) + t[2] * zc) + t[9];
      const double Y = ((t[3] * xc + t[4] * yc) + t[5] * zc) + t[10];
      const double Z = ((t[6] * xc + t[7] * yc) + t[8] * zc) + t[11];
      if (!(Z > 0.0)) continue;
      const double u = ((fxd * X) / Z + cxd) - 0.5, v = ((fyd * Y) / Z + cyd) - 0.5;
      if (!(u >= 0.0 && u <= umax && v >= 0.0 && v <= vmax)) continue;        // false for NaN
      const float u32 = (float)u, v32 = (float)v;
      const int x0 = max(min((int)floorf(u32), a.w - 2), 0), y0 = max(min((int)floorf(v32), a.h - 2), 0);
      const float ax = u32 - (float)x0, ay = v32 - (float)y0;
      const int slot = (a.head + slots - (j + 1)) % slots;
      const float* img = a.ring_depth + (long long)slot * plane + (long long)s * a.hw + ((long long)y0 * a.w + x0);
      const float d00 = img[0], d01 = img[1], d10 = img[a.w], d11 = img[a.w + 1];
      if (!(isfinite(d00) && d00 > 0.0f && isfinite(d01) && d01 > 0.0f && isfinite(d10) && d10 > 0.0f && isfinite(d11) && d11 > 0.0f))
        continue;
      const float top = d00 + ax * (d01 - d00), bot = d10 + ax * (d11 - d10);
      const double dk = top + ay * (bot - top);
      const double e0 = (((u + 0.5) - cxd) / fxd) * dk - t[9];
      const double e1 = (((v + 0.5) - cyd) / fyd) * dk - t[10];
      const double e2 = dk - t[11];
      const double bx = (t[0] * e0 + t[3] * e1) + t[6] * e2;                  // Yc = Rr^T (Yk - tr)
      const double by = (t[1] * e0 + t[4] * e1) + t[7] * e2;
      const double bz = (t[2] * e0 + t[5] * e1) + t[8] * e2;
      if (!(bz > 0.0)) continue;
      const double du = (((fxd * bx) / bz + cxd) - 0.5) - (double)col;
      const double dv = (((fyd * by) / bz + cyd) - 0.5) - (double)row;
      if (du * du + dv * dv < tol2 && fabs(bz - zc) < rel * zc) ++n[e];
    }
  }

  float* ring = a.ring_depth + (long long)a.head * plane + (long long)s * a.hw;
  unsigned char* nv = a.n_views + (long long)s * a.hw;
  float* df = a.depth_f ? a.depth_f + (long long)s * a.hw : nullptr;
  const float qnan = __uint_as_float(0x7FC00000u);
  if (kVec) {
    *reinterpret_cast<unsigned*>(nv + p0) = n[0] | (n[1] << 8) | (n[2] << 16) | (n[3] << 24);
    m4d_store16(ring + p0, d[0], d[1], d[2], d[3]);
    if (df)
      m4d_store16(df + p0, (int)n[0] >= a.min_views ? d[0] : qnan, (int)n[1] >= a.min_views ? d[1] : qnan,
                  (int)n[2] >= a.min_views ? d[2] : qnan, (int)n[3] >= a.min_views ? d[3] : qnan);
  } else {
#pragma unroll
    for (int e = 0; e < kPerThread; ++e) {
      if (p0 + e >= a.hw) break;
      nv[p0 + e] = (unsigned char)n[e];
      ring[p0 + e] = d[e];
      if (df) df[p0 + e] = (int)n[e] >= a.min_views ? d[e] : qnan;
    }
  }
}

inline bool views_geometry(int b, int h, int w, int views) {
  return b >= 1 && b <= 65535 && h >= 2 && w >= 2 && (long long)h * w <= kMaxPixels && views >= 1 && views <= kMaxViews;
}

}  // namespace

extern "C" long long m4d_depth_views_ring_floats(int b, int h, int w, int views) {
  return views_geometry(b, h, w, views) ? (long long)(views + 1) * b * h * w : -1;
}

extern "C" int m4d_depth_views(const float* depth, long long depth_stride, const float* cam_f, const float* cam_c,
                               const double* pose, const unsigned char* reset, int force_all, int b, int h, int w, int views,
                               int head, float* ring_depth, double* ring_pose, const int* age_in, int* age_out, float tol_px,
                               float tol_rel, int min_views, unsigned char* n_views, float* depth_f, void* stream) {
  M4D_CHECK_ARG(depth && cam_f && cam_c && pose && ring_depth && ring_pose && age_in && age_out && n_views);
  M4D_CHECK_ARG(views_geometry(b, h, w, views));
  M4D_CHECK_ARG(head >= 0 && head <= views && min_views >= 1 && min_views <= views);
  M4D_CHECK_ARG(tol_px > 0.0f && tol_rel > 0.0f);            // false for NaN
  M4D_CHECK_ARG(age_in != age_out);
  const long long hw = (long long)h * w;
  M4D_CHECK_ARG(depth_stride >= hw);
  M4D_CHECK_ARG(((((uintptr_t)depth) | ((uintptr_t)cam_f) | ((uintptr_t)cam_c) | ((uintptr_t)ring_depth) | ((uintptr_t)age_in) |
                  ((uintptr_t)age_out) | ((uintptr_t)depth_f)) & 3u) == 0);
  M4D_CHECK_ARG(((((uintptr_t)pose) | ((uintptr_t)ring_pose)) & 7u) == 0);
  const ViewsArgs a = {depth, depth_stride, cam_f, cam_c, pose, reset, force_all, b, h, w, (int)hw, views, head, ring_depth,
                       ring_pose, age_in, age_out, tol_px, tol_rel, min_views, n_views, depth_f};
  // four pixels per thread leave as 16-byte / 4-byte stores when every image starts on such a boundary
  const bool vec = hw % 4 == 0 && depth_stride % 4 == 0 &&
                   ((((uintptr_t)depth) | ((uintptr_t)ring_depth) | ((uintptr_t)depth_f)) & 15u) == 0 &&
                   (((uintptr_t)n_views) & 3u) == 0;
  const dim3 grid((unsigned)((hw + kThreads * kPerThread - 1) / (kThreads * kPerThread)), (unsigned)b);
  if (vec) m4d_launch(depth_views_kernel<true>, grid, dim3(kThreads), 0, (hipStream_t)stream, a);
  else     m4d_launch(depth_views_kernel<false>, grid, dim3(kThreads), 0, (hipStream_t)stream, a);
  return M4D_LAUNCH_RESULT();
}
