// Pieces the photometric loss (m4d_photo.hip) and the reprojection-consistency score (m4d_consistency.hip) share: the warp
// query of reproject on a predicted depth, and the SSIM + L1 error over a 3x3 window from tiles in LDS.  One definition each,
// so both carry the same bits (-ffp-contract=off: one IEEE rounding per float operation, in the order written here).
#pragma once
#include "m4d_common.h"

constexpr int kPhotoTile = 16;
constexpr double kPhotoC1 = 0.01 * 0.01, kPhotoC2 = 0.03 * 0.03;

// combined_mat = diag(fx,fy,1) @ [R|t] as in reproject_flow_kernel (m4d_geometry.hip): the same sequential dot products
__device__ __forceinline__ void m4d_photo_matrix(const M4dMotion& m, float M[3][4]) {
  const float T[3][4] = {{m.r00, m.r01, m.r02, m.tx}, {m.r10, m.r11, m.r12, m.ty}, {m.r20, m.r21, m.r22, m.tz}};
  const float P[3][3] = {{m.fx, 0.f, 0.f}, {0.f, m.fy, 0.f}, {0.f, 0.f, 1.f}};
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      float acc = P[r][0] * T[0][c];
      acc = acc + P[r][1] * T[1][c];
      acc = acc + P[r][2] * T[2][c];
      M[r][c] = acc;
    }
}

// reproject's query of pixel (i, j) with raw depth `draw`: the projected point pr, the query (qx, qy), its bilinear cell and
// alphas, and validity = Pz > 0, query inside [0, w-1] x [0, h-1], depth finite
struct M4dPhotoQuery {
  float ux, uy, pr[3], qx, qy, ax, ay;
  int x0, y0;
  bool ok;
};
__device__ __forceinline__ M4dPhotoQuery m4d_photo_query(const M4dMotion& m, const float M[3][4], int i, int j, float draw, int h,
                                                         int w) {
  M4dPhotoQuery q;
  const float d = fminf(fmaxf(draw, 0.01f), 200.0f);
  const float mx = ((float)i + 0.5f) - m.cx;
  const float my = ((float)j + 0.5f) - m.cy;
  q.ux = mx / m.fx; q.uy = my / m.fy;
  const float pos0 = q.ux * d, pos1 = q.uy * d, pos2 = 1.0f * d;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    float acc = M[r][0] * pos0;
    acc = acc + M[r][1] * pos1;
    acc = acc + M[r][2] * pos2;
    q.pr[r] = acc + M[r][3] * 1.0f;
  }
  const float px = q.pr[0] / q.pr[2], py = q.pr[1] / q.pr[2];
  q.qy = (float)j + (py - my);                               // dense_image_warp.py:244 on reproject's flow
  q.qx = (float)i + (px - mx);
  m4d_bilinear_axis(q.qy, h, q.y0, q.ay);
  m4d_bilinear_axis(q.qx, w, q.x0, q.ax);
  q.ok = q.pr[2] > 0.0f && q.qx >= 0.0f && q.qx <= (float)(w - 1) && q.qy >= 0.0f && q.qy <= (float)(h - 1) && isfinite(draw);
  return q;
}

// window sums of one channel at LDS position `at` (row pitch S pixels, 3 floats per pixel)
struct WinStats { double mx, my, n1, n2, d1, d2; };
template <int S>
__device__ __forceinline__ WinStats win_stats(const float* __restrict__ x, const float* __restrict__ y, int at, int c) {
  double sx = 0.0, sy = 0.0, sxx = 0.0, syy = 0.0, sxy = 0.0;
#pragma unroll
  for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
    for (int dx = -1; dx <= 1; ++dx) {
      const int k = (at + dy * S + dx) * 3 + c;
      const double a = (double)x[k], b = (double)y[k];
      sx += a; sy += b; sxx += a * a; syy += b * b; sxy += a * b;
    }
  WinStats s;
  s.mx = sx / 9.0; s.my = sy / 9.0;
  const double vx = sxx / 9.0 - s.mx * s.mx, vy = syy / 9.0 - s.my * s.my, cxy = sxy / 9.0 - s.mx * s.my;
  s.n1 = 2.0 * s.mx * s.my + kPhotoC1; s.n2 = 2.0 * cxy + kPhotoC2;
  s.d1 = s.mx * s.mx + s.my * s.my + kPhotoC1; s.d2 = vx + vy + kPhotoC2;
  return s;
}

template <int S>
__device__ __forceinline__ double photo_error(const float* __restrict__ x, const float* __restrict__ y, int at) {
  double pe = 0.0;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const WinStats s = win_stats<S>(x, y, at, c);
    const double ssim = (s.n1 * s.n2) / (s.d1 * s.d2);
    pe += 0.85 * (1.0 - ssim) / 2.0 + 0.15 * fabs((double)x[at * 3 + c] - (double)y[at * 3 + c]);
  }
  return pe / 3.0;
}
