// Reprojection consistency: a label-free score of the full-resolution estimate (include/m4depth_hip.h, "Reprojection
// consistency").  Per sample: the previous image is warped into the current frame with the ESTIMATED
// depth (the query of m4d_photo_warp_fwd, m4d_photo_common.h: the same bits) and compared with the current image (SSIM + L1,
// the pe of m4d_photo.hip), and the estimate's projected depth Pz is compared with the previous frame's estimate sampled at the
// query (Bian et al., NeurIPS 2019).
//
// One fused pass and a finish launch, no intermediate in HBM: 16x16-pixel tiles, 256 threads.  The staging loop runs over the
// 18x18 pixels of the tile plus its 1-pixel halo, does the warp query and the bilinear samples per pixel and leaves `warped`,
// `cur`, `prev` and the valid byte in LDS (3 x 3888 + 324 bytes, about 12 KB: the workgroup count per CU is not LDS-limited);
// the geometric term is summed there for the tile's own pixels only (the halo belongs to the neighbours).  Then every thread
// computes its two window errors from LDS.  The halo costs 324 / 256 of the warp work -- the price of not writing a [B,H,W,3]
// map and launching again.  Block partials in double, wave64 shuffles, a fixed-order finish per sample, no atomics, no
// zero-fill: the same bits every run, and row s of a batch is the row of a launch on sample s alone.
#include "m4d_common.h"
#include "m4d_photo_common.h"
#include "../../include/m4depth_hip.h"

namespace {

constexpr int kTile = kPhotoTile;
constexpr int kSums = 6;          // sum_M pe_w, sum_M pe_id, #{pe_w < pe_id}, N, sum_G g, Ng

__global__ void __launch_bounds__(256)
consistency_kernel(const float* __restrict__ est, long long est_stride, const float* __restrict__ est_prev,
                   long long est_prev_stride, const float* __restrict__ cur, long long cur_stride, const float* __restrict__ prev,
                   long long prev_stride, const float* __restrict__ rot, int rot_c, const float* __restrict__ trans,
                   const float* __restrict__ cam_f, const float* __restrict__ cam_c, const unsigned char* __restrict__ reset,
                   const unsigned char* __restrict__ active, int h, int w, double* __restrict__ partial) {
  constexpr int HALO = 1, S = kTile + 2 * HALO;
  __shared__ float s_w[S * S * 3], s_c[S * S * 3], s_p[S * S * 3];
  __shared__ unsigned char s_v[S * S];
  __shared__ double red[kSums][4];
  const int bi = blockIdx.z;
  // a sample its masks rule out: nothing of it is read (its previous-frame buffers may hold another trajectory or nothing),
  // and the finish launch does not read its partials
  if (!active[bi] || reset[bi]) return;
  const int x0 = blockIdx.x * kTile, y0 = blockIdx.y * kTile;
  const M4dMotion m = m4d_load_motion(rot, rot_c, trans, cam_f, cam_c, bi);
  float M[3][4];
  m4d_photo_matrix(m, M);
  const float* D = est + (long long)bi * est_stride;
  const float* Dp = est_prev + (long long)bi * est_prev_stride;
  const float* I = cur + (long long)bi * cur_stride;
  const float* Ip = prev + (long long)bi * prev_stride;
  double a_g = 0.0, a_ng = 0.0;
  for (int k = threadIdx.x; k < S * S; k += 256) {
    const int ly = k / S, lx = k % S;
    const int gy = y0 - HALO + ly, gx = x0 - HALO + lx;
    const bool in = gy >= 0 && gy < h && gx >= 0 && gx < w;
    bool ok = false;
    float wv[3] = {0.f, 0.f, 0.f}, cv[3] = {0.f, 0.f, 0.f}, pv[3] = {0.f, 0.f, 0.f};
    if (in) {
      const long long o = (long long)gy * w + gx;
      const M4dPhotoQuery q = m4d_photo_query(m, M, gx, gy, D[o], h, w);
      ok = q.ok;
      const long long cell = (long long)q.y0 * w + q.x0;         // 0 <= y0 <= h-2, 0 <= x0 <= w-2 for every query, NaN included
      const float* s = Ip + cell * 3;
      const long long rs = (long long)w * 3;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        wv[c] = m4d_lerp2(s[c], s[3 + c], s[rs + c], s[rs + 3 + c], q.ax, q.ay);
        cv[c] = I[o * 3 + c];
        pv[c] = Ip[o * 3 + c];
      }
      // the geometric term: the tile's own pixels only, never the halo
      if (ok && ly >= HALO && ly < HALO + kTile && lx >= HALO && lx < HALO + kTile) {
        const float tl = Dp[cell], tr = Dp[cell + 1], bl = Dp[cell + w], br = Dp[cell + w + 1];
        if (isfinite(tl) && isfinite(tr) && isfinite(bl) && isfinite(br) && tl > 0.f && tr > 0.f && bl > 0.f && br > 0.f) {
          const float dq = m4d_lerp2(tl, tr, bl, br, q.ax, q.ay);
          const double pz = (double)q.pr[2], dd = (double)dq;
          a_g += fabs(pz - dd) / (pz + dd);
          a_ng += 1.0;
        }
      }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) { s_w[k * 3 + c] = wv[c]; s_c[k * 3 + c] = cv[c]; s_p[k * 3 + c] = pv[c]; }
    s_v[k] = ok ? 1 : 0;
  }
  __syncthreads();
  const int tx = threadIdx.x % kTile, ty = threadIdx.x / kTile;
  const int gx = x0 + tx, gy = y0 + ty;
  const int at = (ty + HALO) * S + (tx + HALO);
  double a[kSums] = {0.0, 0.0, 0.0, 0.0, a_g, a_ng};
  bool on = gx >= 1 && gx <= w - 2 && gy >= 1 && gy <= h - 2;
  if (on) {
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
      for (int dx = -1; dx <= 1; ++dx) on = on && s_v[at + dy * S + dx] != 0;
  }
  if (on) {
    const double pe_w = photo_error<S>(s_w, s_c, at), pe_id = photo_error<S>(s_p, s_c, at);
    a[0] = pe_w; a[1] = pe_id; a[2] = pe_w < pe_id ? 1.0 : 0.0; a[3] = 1.0;
  }
#pragma unroll
  for (int i = 0; i < kSums; ++i) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) a[i] += __shfl_down(a[i], o);
  }
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int i = 0; i < kSums; ++i) red[i][threadIdx.x >> 6] = a[i];
  }
  __syncthreads();
  if (threadIdx.x < kSums) {
    const long long blk = ((long long)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    partial[kSums * blk + threadIdx.x] = ((red[threadIdx.x][0] + red[threadIdx.x][1]) + red[threadIdx.x][2]) + red[threadIdx.x][3];
  }
}

// one workgroup per sample: lane t sums the sample's partials t, t + 256, ... in index order, then a fixed halving tree
__global__ void __launch_bounds__(256)
consistency_finish_kernel(const double* __restrict__ partial, int nblk, const unsigned char* __restrict__ reset,
                          const unsigned char* __restrict__ active, int h, int w, float* __restrict__ rows,
                          unsigned char* __restrict__ counted) {
  __shared__ double sh[kSums][256];
  const int bi = blockIdx.x;
  const bool live = active[bi] && !reset[bi];                      // workgroup-uniform
  double s[kSums] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (live) {
    const double* p = partial + (long long)bi * nblk * kSums;
    for (int k = threadIdx.x; k < nblk; k += 256)
#pragma unroll
      for (int i = 0; i < kSums; ++i) s[i] += p[kSums * k + i];
  }
#pragma unroll
  for (int i = 0; i < kSums; ++i) sh[i][threadIdx.x] = s[i];
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (threadIdx.x < off)
      for (int i = 0; i < kSums; ++i) sh[i][threadIdx.x] += sh[i][threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const double n = sh[3][0], ng = sh[5][0];
    const bool ok = live && n > 0.0 && ng > 0.0;
    float* r = rows + (long long)bi * 6;
    r[0] = ok ? (float)(sh[0][0] / n) : 0.f;
    r[1] = ok ? (float)(sh[1][0] / n) : 0.f;
    r[2] = ok ? (float)(sh[2][0] / n) : 0.f;
    r[3] = ok ? (float)(sh[4][0] / ng) : 0.f;
    r[4] = ok ? (float)(n / ((double)(h - 2) * (double)(w - 2))) : 0.f;
    r[5] = ok ? (float)(ng / ((double)h * (double)w)) : 0.f;
    counted[bi] = ok ? 1 : 0;
  }
}

inline bool consistency_dims_ok(int b, int h, int w) {
  return b > 0 && b <= 65535 && h >= 3 && w >= 3 && (long long)h * w <= (1LL << 24) && h <= 65535 * kTile;   // grid y, z
}
inline int consistency_tiles(int h, int w) { return ((h + kTile - 1) / kTile) * ((w + kTile - 1) / kTile); }

}  // namespace

extern "C" long long m4d_consistency_workspace_bytes(int b, int h, int w) {
  if (!consistency_dims_ok(b, h, w)) return -1;
  return (long long)b * consistency_tiles(h, w) * kSums * (long long)sizeof(double);
}

extern "C" int m4d_consistency_per_sample(const float* est, long long est_stride, const float* est_prev, long long est_prev_stride,
                                          const float* cur, long long cur_stride, const float* prev, long long prev_stride,
                                          const float* rot, int rot_c, const float* trans, const float* cam_f, const float* cam_c,
                                          const unsigned char* reset, const unsigned char* active, int b, int h, int w,
                                          void* workspace, float* rows6, unsigned char* counted, void* stream) {
  M4D_CHECK_ARG(est && est_prev && cur && prev && rot && trans && cam_f && cam_c && reset && active && workspace && rows6 && counted);
  M4D_CHECK_ARG(consistency_dims_ok(b, h, w) && (rot_c == 3 || rot_c == 4) && (((uintptr_t)workspace) & 7u) == 0);
  const long long hw = (long long)h * w;
  M4D_CHECK_ARG(est_stride >= hw && est_prev_stride >= hw && cur_stride >= 3 * hw && prev_stride >= 3 * hw);
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((w + kTile - 1) / kTile, (h + kTile - 1) / kTile, b);
  m4d_launch(consistency_kernel, grid, dim3(256), 0, s, est, est_stride, est_prev, est_prev_stride, cur, cur_stride, prev,
             prev_stride, rot, rot_c, trans, cam_f, cam_c, reset, active, h, w, (double*)workspace);
  m4d_launch(consistency_finish_kernel, dim3(b), dim3(256), 0, s, (const double*)workspace, consistency_tiles(h, w), reset, active,
             h, w, rows6, counted);
  return M4D_LAUNCH_RESULT();
}
