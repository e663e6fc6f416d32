// Pose refinement by direct photometric alignment (include/m4depth_hip.h, "Pose refinement").
// Gauss-Newton on the grey residual of the current frame sampled at the reprojection of the previous frame's pixels with the
// previous frame's estimated depth; the query is m4d_photo_query (m4d_photo_common.h) on the float32 rounding of the pose, so
// the half-pixel and clamp conventions are those of the photometric loss and the consistency score.
//
// One iteration = two launches.  align_sums_kernel: 16x16 level pixels per workgroup, one pixel per thread, the 29 terms of
// the normal equations per pixel in float32 arithmetic, promoted to double, reduced by wave64 shuffles and across the four
// waves through LDS in a fixed order, one 29-value partial per tile.  align_finish_kernel: one wave per sample folds the
// partials in index order, lane 0 solves the damped 6x6 system by Cholesky in double and updates the pose.  No atomics, no
// zero-fill, no host read: the same bits every run, and sample s of a batch is the launch on sample s alone.
#include "m4d_common.h"
#include "m4d_photo_common.h"
#include "../../include/m4depth_hip.h"

namespace {

constexpr int kTile = kPhotoTile;
constexpr int kSums = 29;          // H upper triangle row-major (21), b (6), cost, N
constexpr int kState = 64;         // doubles per sample at the head of the workspace (the layout of the header)
enum { S_A = 0, S_a = 9, S_XI = 12, S_COST0 = 18, S_COST1 = 19, S_COVER = 20, S_ITERS = 21, S_BAD = 22, S_STRIDE = 23, S_SUMS = 32 };

struct Quat { double w, x, y, z; };

__device__ __forceinline__ Quat load_unit_quat(const float* __restrict__ rot, int bi) {
  Quat q = {(double)rot[bi * 4 + 0], (double)rot[bi * 4 + 1], (double)rot[bi * 4 + 2], (double)rot[bi * 4 + 3]};
  const double n = sqrt(((q.w * q.w + q.x * q.x) + q.y * q.y) + q.z * q.z);
  q.w /= n; q.x /= n; q.y /= n; q.z /= n;
  return q;
}

__device__ __forceinline__ void quat_matrix(const Quat& q, double R[9]) {
  R[0] = 1.0 - 2.0 * (q.y * q.y + q.z * q.z); R[1] = 2.0 * (q.x * q.y - q.w * q.z); R[2] = 2.0 * (q.x * q.z + q.w * q.y);
  R[3] = 2.0 * (q.x * q.y + q.w * q.z); R[4] = 1.0 - 2.0 * (q.x * q.x + q.z * q.z); R[5] = 2.0 * (q.y * q.z - q.w * q.x);
  R[6] = 2.0 * (q.x * q.z - q.w * q.y); R[7] = 2.0 * (q.y * q.z + q.w * q.x); R[8] = 1.0 - 2.0 * (q.x * q.x + q.y * q.y);
}

// (A, a) = (R^T, -R^T t), xi_acc = 0, no iteration run yet
__global__ void __launch_bounds__(64)
align_begin_kernel(const float* __restrict__ rot, const float* __restrict__ trans, int b, double* __restrict__ state) {
  const int bi = blockIdx.x * 64 + threadIdx.x;
  if (bi >= b) return;
  double* st = state + (long long)bi * kState;
  double R[9];
  quat_matrix(load_unit_quat(rot, bi), R);
  const double t[3] = {(double)trans[bi * 3 + 0], (double)trans[bi * 3 + 1], (double)trans[bi * 3 + 2]};
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int c = 0; c < 3; ++c) st[S_A + r * 3 + c] = R[c * 3 + r];
    st[S_a + r] = -((R[0 * 3 + r] * t[0] + R[1 * 3 + r] * t[1]) + R[2 * 3 + r] * t[2]);
  }
  for (int k = S_XI; k < kState; ++k) st[k] = 0.0;
}

__device__ __forceinline__ float grey(const float* __restrict__ p) { return ((p[0] + p[1]) + p[2]) / 3.0f; }

__global__ void __launch_bounds__(256)
align_sums_kernel(const float* __restrict__ cur, long long cur_stride, const float* __restrict__ prev, long long prev_stride,
                  const float* __restrict__ est_prev, long long est_stride, const float* __restrict__ cam_f,
                  const float* __restrict__ cam_c, const unsigned char* __restrict__ reset,
                  const unsigned char* __restrict__ active, int W, int hl, int wl, int s, float huber,
                  const double* __restrict__ state, double* __restrict__ partial) {
  __shared__ double red[kSums][4];
  const int bi = blockIdx.z;
  // a sample its masks rule out: nothing of it is read, and the finish launch does not read its partials
  if (!active[bi] || reset[bi]) return;
  const double* st = state + (long long)bi * kState;
  M4dMotion m;
  m.r00 = (float)st[0]; m.r01 = (float)st[1]; m.r02 = (float)st[2];
  m.r10 = (float)st[3]; m.r11 = (float)st[4]; m.r12 = (float)st[5];
  m.r20 = (float)st[6]; m.r21 = (float)st[7]; m.r22 = (float)st[8];
  m.tx = (float)st[9]; m.ty = (float)st[10]; m.tz = (float)st[11];
  const float fs = (float)s;                                      // a power of two: the level camera is exact
  m.fx = cam_f[bi * 2 + 0] / fs; m.fy = cam_f[bi * 2 + 1] / fs;
  m.cx = cam_c[bi * 2 + 0] / fs; m.cy = cam_c[bi * 2 + 1] / fs;
  m.stx = 0.f; m.sty = 0.f;
  float M[3][4];
  m4d_photo_matrix(m, M);
  const int i = blockIdx.x * kTile + threadIdx.x % kTile, j = blockIdx.y * kTile + threadIdx.x / kTile;
  double acc[kSums];
#pragma unroll
  for (int k = 0; k < kSums; ++k) acc[k] = 0.0;
  if (i < wl && j < hl) {
    const float* I = cur + (long long)bi * cur_stride;
    const float* Ip = prev + (long long)bi * prev_stride;
    const float draw = est_prev[(long long)bi * est_stride + (long long)(j * s + s / 2) * W + (i * s + s / 2)];
    const M4dPhotoQuery q = m4d_photo_query(m, M, i, j, draw, hl, wl);
    if (q.ok) {
      const float d = fminf(fmaxf(draw, 0.01f), 200.0f);
      const float X0 = q.ux * d, X1 = q.uy * d, X2 = d;
      const float Yx = ((m.r00 * X0 + m.r01 * X1) + m.r02 * X2) + m.tx;
      const float Yy = ((m.r10 * X0 + m.r11 * X1) + m.r12 * X2) + m.ty;
      const float Yz = ((m.r20 * X0 + m.r21 * X1) + m.r22 * X2) + m.tz;
      const float* c0 = I + ((long long)q.y0 * wl + q.x0) * 3;   // 0 <= y0 <= hl-2, 0 <= x0 <= wl-2 for every query
      const float tl = grey(c0), tr = grey(c0 + 3), bl = grey(c0 + (long long)wl * 3), br = grey(c0 + (long long)wl * 3 + 3);
      const float r = m4d_lerp2(tl, tr, bl, br, q.ax, q.ay) - grey(Ip + ((long long)j * wl + i) * 3);
      const float gx = (1.0f - q.ay) * (tr - tl) + q.ay * (br - bl);
      const float gy = (1.0f - q.ax) * (bl - tl) + q.ax * (br - tr);
      const float gfx = gx * m.fx, gfy = gy * m.fy;
      float J[6];
      J[0] = gfx / Yz;
      J[1] = gfy / Yz;
      J[2] = -((gfx * Yx + gfy * Yy) / (Yz * Yz));
      J[3] = Yy * J[2] - Yz * J[1];
      J[4] = Yz * J[0] - Yx * J[2];
      J[5] = Yx * J[1] - Yy * J[0];
      const float ar = fabsf(r);
      const double wh = (double)(ar <= huber ? 1.0f : huber / ar), rd = (double)r;
      int k = 0;
#pragma unroll
      for (int a = 0; a < 6; ++a) {
        const double wj = wh * (double)J[a];
#pragma unroll
        for (int c = a; c < 6; ++c) acc[k++] = wj * (double)J[c];
        acc[21 + a] = wj * rd;
      }
      acc[27] = wh * rd * rd;
      acc[28] = 1.0;
    }
  }
#pragma unroll
  for (int k = 0; k < kSums; ++k) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc[k] += __shfl_down(acc[k], o);
  }
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < kSums; ++k) red[k][threadIdx.x >> 6] = acc[k];
  }
  __syncthreads();
  if (threadIdx.x < kSums) {
    const long long blk = ((long long)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    partial[kSums * blk + threadIdx.x] = ((red[threadIdx.x][0] + red[threadIdx.x][1]) + red[threadIdx.x][2]) + red[threadIdx.x][3];
  }
}

// exp of a rotation vector (Rodrigues), series below 1e-4 rad
__device__ __forceinline__ void rodrigues(const double w[3], double E[9]) {
  const double t2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2], t = sqrt(t2);
  double ka, kb;
  if (t < 1e-4) { ka = 1.0 - t2 / 6.0; kb = 0.5 - t2 / 24.0; }
  else { ka = sin(t) / t; kb = (1.0 - cos(t)) / t2; }
  E[0] = 1.0 - kb * (w[1] * w[1] + w[2] * w[2]); E[1] = kb * w[0] * w[1] - ka * w[2]; E[2] = kb * w[0] * w[2] + ka * w[1];
  E[3] = kb * w[0] * w[1] + ka * w[2]; E[4] = 1.0 - kb * (w[0] * w[0] + w[2] * w[2]); E[5] = kb * w[1] * w[2] - ka * w[0];
  E[6] = kb * w[0] * w[2] - ka * w[1]; E[7] = kb * w[1] * w[2] + ka * w[0]; E[8] = 1.0 - kb * (w[0] * w[0] + w[1] * w[1]);
}

// one wave per sample: lane t sums the sample's partials t, t + 64, ... in index order, a shuffle tree, lane 0 solves
__global__ void __launch_bounds__(64)
align_finish_kernel(const double* __restrict__ partial, int nblk, const unsigned char* __restrict__ reset,
                    const unsigned char* __restrict__ active, int hl, int wl, int s, double damping, double prior_t,
                    double prior_r, double* __restrict__ state) {
  const int bi = blockIdx.x;
  double* st = state + (long long)bi * kState;
  if (!active[bi] || reset[bi] || st[S_BAD] != 0.0) return;      // wave-uniform
  double sum[kSums];
#pragma unroll
  for (int k = 0; k < kSums; ++k) sum[k] = 0.0;
  const double* p = partial + (long long)bi * nblk * kSums;
  for (int t = threadIdx.x; t < nblk; t += 64)
#pragma unroll
    for (int k = 0; k < kSums; ++k) sum[k] += p[kSums * t + k];
#pragma unroll
  for (int k = 0; k < kSums; ++k) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum[k] += __shfl_down(sum[k], o);
  }
  if (threadIdx.x != 0) return;
#pragma unroll
  for (int k = 0; k < kSums; ++k) st[S_SUMS + k] = sum[k];
  const double n = sum[28];
  bool ok = n >= 1.0;
  const double cost = sum[27] / n;
  if (st[S_STRIDE] != (double)s) { st[S_STRIDE] = (double)s; st[S_COST0] = cost; }    // the first iteration of a level
  st[S_COST1] = cost;
  st[S_COVER] = n / ((double)hl * (double)wl);
  // (H/N + mu diag(H/N) + W) delta = -(b/N + W xi_acc)
  double L[6][6], rhs[6];
  {
    int k = 0;
    for (int a = 0; a < 6; ++a)
      for (int c = a; c < 6; ++c) { L[c][a] = sum[k++] / n; }
  }
  for (int a = 0; a < 6; ++a) {
    const double wp = a < 3 ? prior_t : prior_r;
    rhs[a] = -(sum[21 + a] / n + wp * st[S_XI + a]);
    L[a][a] = (L[a][a] + damping * L[a][a]) + wp;
  }
#pragma unroll
  for (int c = 0; c < 6; ++c) {                                    // Cholesky in place: the lower triangle of L
    double d = L[c][c];
    for (int k = 0; k < c; ++k) d -= L[c][k] * L[c][k];
    if (!(d > 0.0) || !isfinite(d)) ok = false;            // the rest runs on and is discarded
    d = sqrt(d);
    L[c][c] = d;
    for (int r = c + 1; r < 6; ++r) {
      double v = L[r][c];
      for (int k = 0; k < c; ++k) v -= L[r][k] * L[c][k];
      L[r][c] = v / d;
    }
  }
  double delta[6];
  if (ok) {
    for (int r = 0; r < 6; ++r) {
      double v = rhs[r];
      for (int k = 0; k < r; ++k) v -= L[r][k] * delta[k];
      delta[r] = v / L[r][r];
    }
    for (int r = 5; r >= 0; --r) {
      double v = delta[r];
      for (int k = r + 1; k < 6; ++k) v -= L[k][r] * delta[k];
      delta[r] = v / L[r][r];
    }
    for (int r = 0; r < 6; ++r) ok = ok && isfinite(delta[r]);
  }
  if (!ok || !isfinite(cost)) { st[S_BAD] = 1.0; return; }
  double E[9], A[9], a[3];
  rodrigues(delta + 3, E);
  for (int k = 0; k < 9; ++k) A[k] = st[S_A + k];
  for (int k = 0; k < 3; ++k) a[k] = st[S_a + k];
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) st[S_A + r * 3 + c] = (E[r * 3 + 0] * A[0 * 3 + c] + E[r * 3 + 1] * A[1 * 3 + c]) + E[r * 3 + 2] * A[2 * 3 + c];
    st[S_a + r] = ((E[r * 3 + 0] * a[0] + E[r * 3 + 1] * a[1]) + E[r * 3 + 2] * a[2]) + delta[r];
  }
  for (int r = 0; r < 6; ++r) st[S_XI + r] += delta[r];
  st[S_ITERS] += 1.0;
}

__device__ __forceinline__ float finite_or_zero(double v) { return isfinite(v) ? (float)v : 0.f; }

__global__ void __launch_bounds__(64)
align_end_kernel(const float* __restrict__ rot, const float* __restrict__ trans, const unsigned char* __restrict__ reset,
                 const unsigned char* __restrict__ active, int b, double min_cover, double cap_t, double cap_r,
                 const double* __restrict__ state, float* __restrict__ rot_out, float* __restrict__ trans_out,
                 float* __restrict__ rows) {
  const int bi = blockIdx.x * 64 + threadIdx.x;
  if (bi >= b) return;
  const double* st = state + (long long)bi * kState;
  const float q_in[4] = {rot[bi * 4 + 0], rot[bi * 4 + 1], rot[bi * 4 + 2], rot[bi * 4 + 3]};
  const float t_in[3] = {trans[bi * 3 + 0], trans[bi * 3 + 1], trans[bi * 3 + 2]};
  float* row = rows + (long long)bi * 8;
  const bool live = active[bi] && !reset[bi];
  bool applied = false;
  float q_new[4] = {0.f, 0.f, 0.f, 0.f}, t_new[3] = {0.f, 0.f, 0.f};
  double dt = 0.0, angle = 0.0;
  if (live) {
    // R' = A^T, t' = -A^T a
    double R[9], t[3];
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 3; ++c) R[r * 3 + c] = st[S_A + c * 3 + r];
      t[r] = -((st[S_A + 0 * 3 + r] * st[S_a + 0] + st[S_A + 1 * 3 + r] * st[S_a + 1]) + st[S_A + 2 * 3 + r] * st[S_a + 2]);
    }
    Quat q;
    const double tr = R[0] + R[4] + R[8];
    if (tr > 0.0) {
      const double k = sqrt(tr + 1.0) * 2.0;
      q.w = 0.25 * k; q.x = (R[7] - R[5]) / k; q.y = (R[2] - R[6]) / k; q.z = (R[3] - R[1]) / k;
    } else if (R[0] > R[4] && R[0] > R[8]) {
      const double k = sqrt(1.0 + R[0] - R[4] - R[8]) * 2.0;
      q.w = (R[7] - R[5]) / k; q.x = 0.25 * k; q.y = (R[1] + R[3]) / k; q.z = (R[2] + R[6]) / k;
    } else if (R[4] > R[8]) {
      const double k = sqrt(1.0 + R[4] - R[0] - R[8]) * 2.0;
      q.w = (R[2] - R[6]) / k; q.x = (R[1] + R[3]) / k; q.y = 0.25 * k; q.z = (R[5] + R[7]) / k;
    } else {
      const double k = sqrt(1.0 + R[8] - R[0] - R[4]) * 2.0;
      q.w = (R[3] - R[1]) / k; q.x = (R[2] + R[6]) / k; q.y = (R[5] + R[7]) / k; q.z = 0.25 * k;
    }
    double n = sqrt(((q.w * q.w + q.x * q.x) + q.y * q.y) + q.z * q.z);
    if (q.w < 0.0) n = -n;
    q.w /= n; q.x /= n; q.y /= n; q.z /= n;
    // the rotation between R' and R: q' conj(q0)
    const Quat q0 = load_unit_quat(rot, bi);
    const double rw = ((q.w * q0.w + q.x * q0.x) + q.y * q0.y) + q.z * q0.z;
    const double rx = ((-q.w * q0.x + q.x * q0.w) - q.y * q0.z) + q.z * q0.y;
    const double ry = ((-q.w * q0.y + q.x * q0.z) + q.y * q0.w) - q.z * q0.x;
    const double rz = ((-q.w * q0.z - q.x * q0.y) + q.y * q0.x) + q.z * q0.w;
    angle = 2.0 * atan2(sqrt((rx * rx + ry * ry) + rz * rz), fabs(rw));
    const double e0 = t[0] - (double)t_in[0], e1 = t[1] - (double)t_in[1], e2 = t[2] - (double)t_in[2];
    dt = sqrt((e0 * e0 + e1 * e1) + e2 * e2);
    q_new[0] = (float)q.w; q_new[1] = (float)q.x; q_new[2] = (float)q.y; q_new[3] = (float)q.z;
    t_new[0] = (float)t[0]; t_new[1] = (float)t[1]; t_new[2] = (float)t[2];
    bool fin = isfinite(dt) && isfinite(angle);
    for (int k = 0; k < 4; ++k) fin = fin && isfinite(q_new[k]);
    for (int k = 0; k < 3; ++k) fin = fin && isfinite(t_new[k]);
    applied = fin && st[S_BAD] == 0.0 && st[S_ITERS] >= 1.0 && st[S_COVER] >= min_cover && st[S_COST1] < st[S_COST0] &&
              dt <= cap_t && angle <= cap_r;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) rot_out[bi * 4 + k] = applied ? q_new[k] : q_in[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) trans_out[bi * 3 + k] = applied ? t_new[k] : t_in[k];
  row[0] = live ? finite_or_zero(st[S_COST0]) : 0.f;
  row[1] = live ? finite_or_zero(st[S_COST1]) : 0.f;
  row[2] = live ? finite_or_zero(st[S_COVER]) : 0.f;
  row[3] = live ? finite_or_zero(dt) : 0.f;
  row[4] = live ? finite_or_zero(angle) : 0.f;
  row[5] = live ? (float)st[S_ITERS] : 0.f;
  row[6] = applied ? 1.f : 0.f;
  row[7] = 0.f;
}

inline bool align_dims_ok(int b, int h, int w) {
  return b > 0 && b <= 65535 && h >= 3 && w >= 3 && (long long)h * w <= (1LL << 24) && h <= 65535 * kTile;
}
inline int align_tiles(int h, int w) { return ((h + kTile - 1) / kTile) * ((w + kTile - 1) / kTile); }
inline bool aligned8(const void* p) { return (((uintptr_t)p) & 7u) == 0; }

}  // namespace

extern "C" long long m4d_pose_align_workspace_bytes(int b, int h, int w) {
  if (!align_dims_ok(b, h, w)) return -1;
  return ((long long)b * kState + (long long)b * align_tiles(h, w) * kSums) * (long long)sizeof(double);
}

extern "C" int m4d_pose_align_begin(const float* rot, int rot_c, const float* trans, int b, int h, int w, void* workspace,
                                    void* stream) {
  M4D_CHECK_ARG(rot && trans && workspace && rot_c == 4 && align_dims_ok(b, h, w) && aligned8(workspace));
  m4d_launch(align_begin_kernel, dim3((b + 63) / 64), dim3(64), 0, (hipStream_t)stream, rot, trans, b, (double*)workspace);
  return M4D_LAUNCH_RESULT();
}

extern "C" int m4d_pose_align_iterate(const float* cur, long long cur_stride, const float* prev, long long prev_stride,
                                      const float* est_prev, long long est_prev_stride, const float* cam_f, const float* cam_c,
                                      const unsigned char* reset, const unsigned char* active, int b, int h, int w, int s,
                                      float huber, float damping, float prior_t, float prior_r, void* workspace, void* stream) {
  M4D_CHECK_ARG(cur && prev && est_prev && cam_f && cam_c && reset && active && workspace && aligned8(workspace));
  M4D_CHECK_ARG(align_dims_ok(b, h, w) && s >= 1 && (s & (s - 1)) == 0 && h % s == 0 && w % s == 0 && h / s >= 3 && w / s >= 3);
  M4D_CHECK_ARG(huber > 0.f && damping >= 0.f && prior_t >= 0.f && prior_r >= 0.f);
  const int hl = h / s, wl = w / s;
  const long long hwl = (long long)hl * wl;
  M4D_CHECK_ARG(cur_stride >= 3 * hwl && prev_stride >= 3 * hwl && est_prev_stride >= (long long)h * w);
  hipStream_t st = (hipStream_t)stream;
  double* state = (double*)workspace;
  double* partial = state + (long long)b * kState;
  const dim3 grid((wl + kTile - 1) / kTile, (hl + kTile - 1) / kTile, b);       // never more tiles than align_tiles(h, w)
  m4d_launch(align_sums_kernel, grid, dim3(256), 0, st, cur, cur_stride, prev, prev_stride, est_prev, est_prev_stride, cam_f, cam_c,
             reset, active, w, hl, wl, s, huber, (const double*)state, partial);
  m4d_launch(align_finish_kernel, dim3(b), dim3(64), 0, st, (const double*)partial, align_tiles(hl, wl), reset, active, hl, wl, s,
             (double)damping, (double)prior_t, (double)prior_r, state);
  return M4D_LAUNCH_RESULT();
}

extern "C" int m4d_pose_align_end(const float* rot, int rot_c, const float* trans, const unsigned char* reset,
                                  const unsigned char* active, int b, int h, int w, float min_cover, float cap_t, float cap_r,
                                  const void* workspace, float* rot_out, float* trans_out, float* rows8, void* stream) {
  M4D_CHECK_ARG(rot && trans && reset && active && workspace && rot_out && trans_out && rows8 && rot_c == 4);
  M4D_CHECK_ARG(align_dims_ok(b, h, w) && aligned8(workspace) && min_cover >= 0.f && cap_t >= 0.f && cap_r >= 0.f);
  m4d_launch(align_end_kernel, dim3((b + 63) / 64), dim3(64), 0, (hipStream_t)stream, rot, trans, reset, active, b, (double)min_cover,
             (double)cap_t, (double)cap_r, (const double*)workspace, rot_out, trans_out, rows8);
  return M4D_LAUNCH_RESULT();
}
