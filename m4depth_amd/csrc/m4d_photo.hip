// Photometric reprojection loss: training without ground-truth depth ("Photometric loss").
//
// Per pyramid level and frame t >= 1 the previous frame's image is warped into the current one with the PREDICTED depth
// (the query of depth_operations.reproject: reproject_flow_kernel + interp_bilinear_kernel, same device functions, same
// operation order, so `warped` carries reproject's bits) and compared with the current image:
//   pe(a, b)   = 0.85 (1 - SSIM(a, b)) / 2 + 0.15 |a - b|, mean over the 3 channels, SSIM over the 3x3 window with
//                sigma^2 = mean(x^2) - mu^2, sigma_xy = mean(xy) - mu_x mu_y, C1 = 0.01^2, C2 = 0.03^2, no clipping;
//   M(p)       = p interior (1 <= y <= h-2, 1 <= x <= w-2), all 9 window pixels valid, and (auto-masking, optional)
//                pe(warped, cur)(p) < pe(prev, cur)(p);   valid = Pz > 0, query inside [0, w-1] x [0, h-1], depth finite;
//   photo      = sum M pe(warped, cur) / max(N, 1), N = sum M;
//   smooth     = [sum_{x<w-1} |ld(y,x+1) - ld(y,x)| exp(-mean_c |cur(y,x+1) - cur(y,x)|) + the same along y] / (b h w),
//                ld = log(clip(depth, 0.01, 200));
//   term       = photo + lambda smooth            (Monodepth2: Godard et al., ICCV 2019, eq. 2-5, single source frame).
// The backward is a pure gather: every pixel q sums the derivative of the (at most 9) masked windows it lies in, times
// dwarp = d warped / d clip(depth) of the forward, plus the smoothness term; the mask and N are the forward's.
//
// Structure: 16x16-pixel tiles, 256 threads, `warped`, `cur`, validity / mask and log depth of the tile plus its halo in LDS
// (1 pixel forward, 2 pixels backward: the windows of the 3x3 neighbours), window statistics and sums in double (the maps are
// small; float32's cancellation in mean(x^2) - mu^2 against C2 = 9e-4 would otherwise be the largest error of the loss).
// No atomics, no memset: block partials in double, wave64 shuffles, one fixed-order finish -- the same bits every run.
#include "m4d_common.h"
#include "m4d_photo_common.h"
#include "../../include/m4depth_hip.h"

namespace {

constexpr int kTile = kPhotoTile;

// ---- image pyramid: 2x2 mean, ((a + b) + (c + d)) * 0.25 with a, b on the upper row ---------------------------------------
__global__ void __launch_bounds__(256)
pyramid_box_kernel(const float* __restrict__ in, int oh, int ow, long long total, float* __restrict__ out) {
  for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
    const int c = (int)(idx % 3);
    long long r = idx / 3;
    const int x = (int)(r % ow); r /= ow;
    const int y = (int)(r % oh);
    const long long ni = r / oh;
    const long long iw3 = 2LL * ow * 3;
    const float* p = in + (ni * 2 * oh + 2 * y) * iw3 + 2LL * x * 3 + c;
    out[idx] = ((p[0] + p[3]) + (p[iw3] + p[iw3 + 3])) * 0.25f;
  }
}

// ---- warp: reproject's query, the bilinear sample, its derivative w.r.t. the clipped depth, validity ----------------------
__global__ void __launch_bounds__(256)
photo_warp_fwd_kernel(const float* __restrict__ depth, const float* __restrict__ rot, int rot_c, const float* __restrict__ trans,
                      const float* __restrict__ cam_f, const float* __restrict__ cam_c, const float* __restrict__ prev, int h, int w,
                      float* __restrict__ warped, float* __restrict__ dwarp, unsigned char* __restrict__ valid) {
  const int bi = blockIdx.y;
  const M4dMotion m = m4d_load_motion(rot, rot_c, trans, cam_f, cam_c, bi);
  float M[3][4];
  m4d_photo_matrix(m, M);
  const int hw = h * w;
  const float* img = prev + (long long)bi * hw * 3;
  for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < hw; p += gridDim.x * blockDim.x) {
    const int i = p % w, j = p / w;
    const long long o = (long long)bi * hw + p;
    const float draw = depth[o];
    const M4dPhotoQuery q = m4d_photo_query(m, M, i, j, draw, h, w);
    const float ux = q.ux, uy = q.uy, qx = q.qx, qy = q.qy, ax = q.ax, ay = q.ay;
    const float* pr = q.pr;
    const int x0 = q.x0, y0 = q.y0;
    float dpr[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) dpr[r] = (M[r][0] * ux + M[r][1] * uy) + M[r][2];        // d pr[r] / d d
    // an axis whose alpha was clamped carries no gradient (the gradient of clip outside its bounds; NaN: none)
    const float ry = qy - (float)y0, rx = qx - (float)x0;
    const bool gy_on = ry >= 0.0f && ry <= 1.0f, gx_on = rx >= 0.0f && rx <= 1.0f;
    const float pz2 = pr[2] * pr[2];
    const float dqx = (dpr[0] * pr[2] - pr[0] * dpr[2]) / pz2;
    const float dqy = (dpr[1] * pr[2] - pr[1] * dpr[2]) / pz2;
    const bool ok = q.ok;
    const float* s = img + ((long long)y0 * w + x0) * 3;
    const long long rs = (long long)w * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float tl = s[c], tr = s[3 + c], bl = s[rs + c], br = s[rs + 3 + c];
      warped[o * 3 + c] = m4d_lerp2(tl, tr, bl, br, ax, ay);
      const float dwx = gx_on ? (1.0f - ay) * (tr - tl) + ay * (br - bl) : 0.0f;
      const float dwy = gy_on ? (1.0f - ax) * (bl - tl) + ax * (br - tr) : 0.0f;
      dwarp[o * 3 + c] = ok ? dwx * dqx + dwy * dqy : 0.0f;    // never read where invalid (no masked window holds the pixel)
    }
    valid[o] = ok ? 1 : 0;
  }
}

// ---- shared pieces of the loss kernels -----------------------------------------------------------------------------------
__device__ __forceinline__ float clip_depth(float d) { return fminf(fmaxf(d, 0.01f), 200.0f); }

// win_stats / photo_error: m4d_photo_common.h
__device__ __forceinline__ double edge_weight(const float* __restrict__ cur, int a, int b) {
  const double d = (fabs((double)cur[b * 3] - (double)cur[a * 3]) + fabs((double)cur[b * 3 + 1] - (double)cur[a * 3 + 1]))
                   + fabs((double)cur[b * 3 + 2] - (double)cur[a * 3 + 2]);
  return exp(-(d / 3.0));
}

// ---- forward: per-pixel error, mask, block partials (sum M pe, N, sum smooth) ----------------------------------------------
__global__ void __launch_bounds__(256)
photo_loss_fwd_kernel(const float* __restrict__ depth, const float* __restrict__ warped, const unsigned char* __restrict__ valid,
                      const float* __restrict__ cur, const float* __restrict__ prev, int h, int w, int automask,
                      unsigned char* __restrict__ mask, double* __restrict__ partial) {
  constexpr int HALO = 1, S = kTile + 2 * HALO;
  __shared__ float s_w[S * S * 3], s_c[S * S * 3], s_p[S * S * 3];
  __shared__ double s_ld[S * S];
  __shared__ unsigned char s_v[S * S];
  __shared__ double red[3][4];
  const int bi = blockIdx.z, x0 = blockIdx.x * kTile, y0 = blockIdx.y * kTile;
  const long long base = (long long)bi * h * w;
  for (int k = threadIdx.x; k < S * S; k += 256) {
    const int gy = y0 - HALO + k / S, gx = x0 - HALO + k % S;
    const bool in = gy >= 0 && gy < h && gx >= 0 && gx < w;
    const long long o = base + (long long)gy * w + gx;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      s_w[k * 3 + c] = in ? warped[o * 3 + c] : 0.f;
      s_c[k * 3 + c] = in ? cur[o * 3 + c] : 0.f;
      s_p[k * 3 + c] = in ? prev[o * 3 + c] : 0.f;
    }
    s_v[k] = in ? valid[o] : 0;
    s_ld[k] = in ? log((double)clip_depth(depth[o])) : 0.0;
  }
  __syncthreads();
  const int tx = threadIdx.x % kTile, ty = threadIdx.x / kTile;
  const int gx = x0 + tx, gy = y0 + ty;
  const int at = (ty + HALO) * S + (tx + HALO);
  double s_pe = 0.0, s_n = 0.0, s_sm = 0.0;
  if (gx < w && gy < h) {
    bool on = gx >= 1 && gx <= w - 2 && gy >= 1 && gy <= h - 2;
    if (on) {
#pragma unroll
      for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) on = on && s_v[at + dy * S + dx] != 0;
    }
    if (on) {
      const double pe_w = photo_error<S>(s_w, s_c, at);
      if (automask) on = pe_w < photo_error<S>(s_p, s_c, at);
      if (on) { s_pe = pe_w; s_n = 1.0; }
    }
    mask[base + (long long)gy * w + gx] = on ? 1 : 0;
    if (gx < w - 1) s_sm += fabs(s_ld[at + 1] - s_ld[at]) * edge_weight(s_c, at, at + 1);
    if (gy < h - 1) s_sm += fabs(s_ld[at + S] - s_ld[at]) * edge_weight(s_c, at, at + S);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { s_pe += __shfl_down(s_pe, o); s_n += __shfl_down(s_n, o); s_sm += __shfl_down(s_sm, o); }
  if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = s_pe; red[1][threadIdx.x >> 6] = s_n; red[2][threadIdx.x >> 6] = s_sm; }
  __syncthreads();
  if (threadIdx.x < 3) {
    const long long blk = ((long long)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    partial[3 * blk + threadIdx.x] = ((red[threadIdx.x][0] + red[threadIdx.x][1]) + red[threadIdx.x][2]) + red[threadIdx.x][3];
  }
}

// one workgroup: lane t sums partials t, t + 256, ... in index order, then a fixed halving tree; out = (term, photo, smooth, N)
__global__ void __launch_bounds__(256)
photo_loss_finish_kernel(const double* __restrict__ partial, long long nblk, double pixels, float lambda, float* __restrict__ out) {
  __shared__ double sh[3][256];
  double s[3] = {0.0, 0.0, 0.0};
  for (long long k = threadIdx.x; k < nblk; k += 256) { s[0] += partial[3 * k]; s[1] += partial[3 * k + 1]; s[2] += partial[3 * k + 2]; }
  sh[0][threadIdx.x] = s[0]; sh[1][threadIdx.x] = s[1]; sh[2][threadIdx.x] = s[2];
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (threadIdx.x < off)
      for (int k = 0; k < 3; ++k) sh[k][threadIdx.x] += sh[k][threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const double n = sh[1][0];
    const double photo = sh[0][0] / (n > 1.0 ? n : 1.0);
    const double smooth = sh[2][0] / pixels;
    out[0] = (float)(photo + (double)lambda * smooth);
    out[1] = (float)photo;
    out[2] = (float)smooth;
    out[3] = (float)n;
  }
}

// ---- backward: gather over the masked windows a pixel lies in ---------------------------------------------------------------
__global__ void __launch_bounds__(256)
photo_loss_bwd_kernel(const float* __restrict__ depth, const float* __restrict__ warped, const float* __restrict__ dwarp,
                      const float* __restrict__ cur, const unsigned char* __restrict__ mask, const float* __restrict__ out4,
                      const float* __restrict__ g_out, int h, int w, float lambda, double pixels, float* __restrict__ g_depth) {
  constexpr int HALO = 2, S = kTile + 2 * HALO, S1 = kTile + 2;
  __shared__ float s_w[S * S * 3], s_c[S * S * 3];
  __shared__ double s_ld[S * S];
  __shared__ unsigned char s_m[S * S];
  __shared__ double s_st[S1 * S1 * 3 * 6];         // (mu_x, mu_y, n1, n2, 1/d1, 1/d2) per channel of every window centre
  const int bi = blockIdx.z, x0 = blockIdx.x * kTile, y0 = blockIdx.y * kTile;
  const long long base = (long long)bi * h * w;
  for (int k = threadIdx.x; k < S * S; k += 256) {
    const int gy = y0 - HALO + k / S, gx = x0 - HALO + k % S;
    const bool in = gy >= 0 && gy < h && gx >= 0 && gx < w;
    const long long o = base + (long long)gy * w + gx;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      s_w[k * 3 + c] = in ? warped[o * 3 + c] : 0.f;
      s_c[k * 3 + c] = in ? cur[o * 3 + c] : 0.f;
    }
    s_m[k] = in ? mask[o] : 0;
    s_ld[k] = in ? log((double)clip_depth(depth[o])) : 0.0;
  }
  __syncthreads();
  // a masked pixel is interior, so its window lies inside the image and inside the 2-pixel halo
  for (int k = threadIdx.x; k < S1 * S1; k += 256) {
    const int at = (k / S1 + 1) * S + (k % S1 + 1);
    if (s_m[at]) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const WinStats s = win_stats<S>(s_w, s_c, at, c);
        double* st = s_st + (k * 3 + c) * 6;
        st[0] = s.mx; st[1] = s.my; st[2] = s.n1; st[3] = s.n2; st[4] = 1.0 / s.d1; st[5] = 1.0 / s.d2;
      }
    }
  }
  __syncthreads();
  const int tx = threadIdx.x % kTile, ty = threadIdx.x / kTile;
  const int gx = x0 + tx, gy = y0 + ty;
  if (gx >= w || gy >= h) return;
  const int at = (ty + HALO) * S + (tx + HALO);
  const long long o = base + (long long)gy * w + gx;
  double acc[3] = {0.0, 0.0, 0.0};
#pragma unroll
  for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
    for (int dx = -1; dx <= 1; ++dx) {
      const int p = at + dy * S + dx;
      if (!s_m[p]) continue;
      const int k = (ty + 1 + dy) * S1 + (tx + 1 + dx);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const double* st = s_st + (k * 3 + c) * 6;
        const double xq = (double)s_w[at * 3 + c], yq = (double)s_c[at * 3 + c];
        const double inv = st[4] * st[5];
        const double ssim = st[2] * st[3] * inv;
        const double dssim = (2.0 / 9.0) * ((st[1] * st[3] + st[2] * (yq - st[1])) * inv
                                            - ssim * (st[0] * st[4] + (xq - st[0]) * st[5]));
        double d = -0.425 * dssim;
        if (dy == 0 && dx == 0) {
          const double e = xq - yq;
          d += 0.15 * (e > 0.0 ? 1.0 : (e < 0.0 ? -1.0 : 0.0));
        }
        acc[c] += d;
      }
    }
  const double n = (double)out4[3];
  double g = ((acc[0] * (double)dwarp[o * 3] + acc[1] * (double)dwarp[o * 3 + 1]) + acc[2] * (double)dwarp[o * 3 + 2])
             / (3.0 * (n > 1.0 ? n : 1.0));
  // smoothness: the (up to) four differences the pixel's log depth enters
  double sm = 0.0;
  const double ld = s_ld[at];
  if (gx < w - 1) { const double e = s_ld[at + 1] - ld; sm -= (e > 0.0 ? 1.0 : (e < 0.0 ? -1.0 : 0.0)) * edge_weight(s_c, at, at + 1); }
  if (gx > 0)     { const double e = ld - s_ld[at - 1]; sm += (e > 0.0 ? 1.0 : (e < 0.0 ? -1.0 : 0.0)) * edge_weight(s_c, at - 1, at); }
  if (gy < h - 1) { const double e = s_ld[at + S] - ld; sm -= (e > 0.0 ? 1.0 : (e < 0.0 ? -1.0 : 0.0)) * edge_weight(s_c, at, at + S); }
  if (gy > 0)     { const double e = ld - s_ld[at - S]; sm += (e > 0.0 ? 1.0 : (e < 0.0 ? -1.0 : 0.0)) * edge_weight(s_c, at - S, at); }
  const float draw = depth[o];
  const bool inside = draw >= 0.01f && draw <= 200.0f;         // clip passes inside its bounds (m4d_loss_level_bwd)
  g += (double)lambda * sm / (pixels * (double)clip_depth(draw));
  g_depth[o] = inside ? (float)((double)g_out[0] * g) : 0.0f;
}

// ---- full-resolution terms and the minimum over two sources ("Full resolution, two sources") ---------
// U_s: bilinear upsampling with half-pixel centres and edge clamp; one axis of output index Y over n input samples
__device__ __forceinline__ void hp_axis(int Y, int n, float s, int& i0, int& i1, float& a) {
  const float src = fmaxf(((float)Y + 0.5f) / s - 0.5f, 0.0f);     // exact in float32: s is a power of two
  const int fl = (int)floorf(src);
  i0 = fl < n - 1 ? fl : n - 1;
  i1 = i0 + 1 < n - 1 ? i0 + 1 : n - 1;
  a = src - (float)i0;
}

__global__ void __launch_bounds__(256)
upsample_hp_fwd_kernel(const float* __restrict__ x, int h, int w, int si, long long total, float* __restrict__ out) {
  const int H = h * si, W = w * si;
  const float s = (float)si;
  for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
    const int X = (int)(idx % W);
    long long r = idx / W;
    const int Y = (int)(r % H);
    const float* p = x + (r / H) * h * w;
    int y0, y1, x0, x1;
    float ay, ax;
    hp_axis(Y, h, s, y0, y1, ay);
    hp_axis(X, w, s, x0, x1, ax);
    out[idx] = m4d_lerp2(p[y0 * w + x0], p[y0 * w + x1], p[y1 * w + x0], p[y1 * w + x1], ax, ay);
  }
}

// the weight with which fine index Y reads coarse index ci along one axis: (1 - a) from the lower tap, a from the upper one,
// both where the clamp folds them onto the same sample
__device__ __forceinline__ double hp_weight(int Y, int ci, int n, float s) {
  int i0, i1;
  float a;
  hp_axis(Y, n, s, i0, i1, a);
  return (i0 == ci ? 1.0 - (double)a : 0.0) + (i1 == ci ? (double)a : 0.0);
}
// the fine indices whose stencil can hold coarse index ci: [lo, hi], at most 2 s of them
__device__ __forceinline__ void hp_span(int ci, int si, int N, int& lo, int& hi) {
  lo = ci * si - si / 2;
  hi = ci * si + si + si / 2 - 1;
  if (lo < 0) lo = 0;
  if (hi > N - 1) hi = N - 1;
}

// U_s^T, s <= 4: one thread per coarse pixel, at most 64 values in row-major order
__global__ void __launch_bounds__(256)
upsample_hp_bwd_thread_kernel(const float* __restrict__ g_out, int h, int w, int si, long long total, float* __restrict__ g_x) {
  const int H = h * si, W = w * si;
  const float s = (float)si;
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const int cx = (int)(idx % w);
  const long long r = idx / w;
  const int cy = (int)(r % h);
  const float* g = g_out + (r / h) * H * W;
  int ylo, yhi, xlo, xhi;
  hp_span(cy, si, H, ylo, yhi);
  hp_span(cx, si, W, xlo, xhi);
  double acc = 0.0;
  for (int Y = ylo; Y <= yhi; ++Y) {
    const double wy = hp_weight(Y, cy, h, s);
    for (int X = xlo; X <= xhi; ++X) acc += wy * hp_weight(X, cx, w, s) * (double)g[(long long)Y * W + X];
  }
  g_x[idx] = (float)acc;
}

// U_s^T, s >= 8: one wave per coarse pixel (256 .. 16384 values): lane l sums values l, l + 64, ... of the row-major window
// in double, then the fixed shuffle tree
__global__ void __launch_bounds__(256)
upsample_hp_bwd_wave_kernel(const float* __restrict__ g_out, int h, int w, int si, long long total, float* __restrict__ g_x) {
  const int H = h * si, W = w * si;
  const float s = (float)si;
  const long long idx = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (idx >= total) return;                                        // wave-uniform
  const int lane = threadIdx.x & 63;
  const int cx = (int)(idx % w);
  const long long r = idx / w;
  const int cy = (int)(r % h);
  const float* g = g_out + (r / h) * H * W;
  int ylo, yhi, xlo, xhi;
  hp_span(cy, si, H, ylo, yhi);
  hp_span(cx, si, W, xlo, xhi);
  const int nx = xhi - xlo + 1, n = (yhi - ylo + 1) * nx;
  double acc = 0.0;
  for (int k = lane; k < n; k += 64) {
    const int Y = ylo + k / nx, X = xlo + k % nx;
    acc += hp_weight(Y, cy, h, s) * hp_weight(X, cx, w, s) * (double)g[(long long)Y * W + X];
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o);
  if (lane == 0) g_x[idx] = (float)acc;
}

// ---- identity error: min over the present sources of pe(source, cur), the auto-mask's right-hand side ------------------------
__global__ void __launch_bounds__(256)
photo_identity_kernel(const float* __restrict__ cur, const float* __restrict__ src0, const float* __restrict__ src1, int h, int w,
                      float* __restrict__ pe_id) {
  constexpr int HALO = 1, S = kTile + 2 * HALO;
  __shared__ float s_c[S * S * 3], s_0[S * S * 3], s_1[S * S * 3];
  const int bi = blockIdx.z, x0 = blockIdx.x * kTile, y0 = blockIdx.y * kTile;
  const long long base = (long long)bi * h * w;
  for (int k = threadIdx.x; k < S * S; k += 256) {
    const int gy = y0 - HALO + k / S, gx = x0 - HALO + k % S;
    const bool in = gy >= 0 && gy < h && gx >= 0 && gx < w;
    const long long o = base + (long long)gy * w + gx;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      s_c[k * 3 + c] = in ? cur[o * 3 + c] : 0.f;
      s_0[k * 3 + c] = in ? src0[o * 3 + c] : 0.f;
      s_1[k * 3 + c] = (in && src1) ? src1[o * 3 + c] : 0.f;
    }
  }
  __syncthreads();
  const int tx = threadIdx.x % kTile, ty = threadIdx.x / kTile;
  const int gx = x0 + tx, gy = y0 + ty;
  if (gx >= w || gy >= h) return;
  const int at = (ty + HALO) * S + (tx + HALO);
  double id = 0.0;
  if (gx >= 1 && gx <= w - 2 && gy >= 1 && gy <= h - 2) {
    id = photo_error<S>(s_0, s_c, at);
    if (src1) {
      const double e = photo_error<S>(s_1, s_c, at);
      if (e < id) id = e;
    }
  }
  pe_id[base + (long long)gy * w + gx] = (float)id;
}

// ---- forward over up to two sources: per-pixel minimum, selection, block partials (sum M m, N, sum smooth) ------------------
__global__ void __launch_bounds__(256)
photo_min_fwd_kernel(const float* __restrict__ depth, const float* __restrict__ warped0, const unsigned char* __restrict__ valid0,
                     const float* __restrict__ warped1, const unsigned char* __restrict__ valid1, const float* __restrict__ cur,
                     const float* __restrict__ pe_id, int h, int w, unsigned char* __restrict__ sel, double* __restrict__ partial) {
  constexpr int HALO = 1, S = kTile + 2 * HALO;
  __shared__ float s_w0[S * S * 3], s_w1[S * S * 3], s_c[S * S * 3];
  __shared__ double s_ld[S * S];
  __shared__ unsigned char s_v0[S * S], s_v1[S * S];
  __shared__ double red[3][4];
  const int bi = blockIdx.z, x0 = blockIdx.x * kTile, y0 = blockIdx.y * kTile;
  const long long base = (long long)bi * h * w;
  for (int k = threadIdx.x; k < S * S; k += 256) {
    const int gy = y0 - HALO + k / S, gx = x0 - HALO + k % S;
    const bool in = gy >= 0 && gy < h && gx >= 0 && gx < w;
    const bool in1 = in && warped1;
    const long long o = base + (long long)gy * w + gx;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      s_w0[k * 3 + c] = in ? warped0[o * 3 + c] : 0.f;
      s_w1[k * 3 + c] = in1 ? warped1[o * 3 + c] : 0.f;
      s_c[k * 3 + c] = in ? cur[o * 3 + c] : 0.f;
    }
    s_v0[k] = in ? valid0[o] : 0;
    s_v1[k] = in1 ? valid1[o] : 0;
    s_ld[k] = in ? log((double)clip_depth(depth[o])) : 0.0;
  }
  __syncthreads();
  const int tx = threadIdx.x % kTile, ty = threadIdx.x / kTile;
  const int gx = x0 + tx, gy = y0 + ty;
  const int at = (ty + HALO) * S + (tx + HALO);
  double s_pe = 0.0, s_n = 0.0, s_sm = 0.0;
  if (gx < w && gy < h) {
    const long long o = base + (long long)gy * w + gx;
    int choice = 0;
    double m = 0.0;
    if (gx >= 1 && gx <= w - 2 && gy >= 1 && gy <= h - 2) {
      bool ok0 = true, ok1 = warped1 != nullptr;
#pragma unroll
      for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
          ok0 = ok0 && s_v0[at + dy * S + dx] != 0;
          ok1 = ok1 && s_v1[at + dy * S + dx] != 0;
        }
      if (ok0) { m = photo_error<S>(s_w0, s_c, at); choice = 1; }
      if (ok1) {
        const double e = photo_error<S>(s_w1, s_c, at);
        if (choice == 0 || e < m) { m = e; choice = 2; }            // a tie keeps the previous frame
      }
      if (choice && pe_id && !(m < (double)pe_id[o])) choice = 0;
    }
    if (choice) { s_pe = m; s_n = 1.0; }
    sel[o] = (unsigned char)choice;
    if (gx < w - 1) s_sm += fabs(s_ld[at + 1] - s_ld[at]) * edge_weight(s_c, at, at + 1);
    if (gy < h - 1) s_sm += fabs(s_ld[at + S] - s_ld[at]) * edge_weight(s_c, at, at + S);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { s_pe += __shfl_down(s_pe, o); s_n += __shfl_down(s_n, o); s_sm += __shfl_down(s_sm, o); }
  if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = s_pe; red[1][threadIdx.x >> 6] = s_n; red[2][threadIdx.x >> 6] = s_sm; }
  __syncthreads();
  if (threadIdx.x < 3) {
    const long long blk = ((long long)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    partial[3 * blk + threadIdx.x] = ((red[threadIdx.x][0] + red[threadIdx.x][1]) + red[threadIdx.x][2]) + red[threadIdx.x][3];
  }
}

// ---- backward over up to two sources: one gather ------------------------------------------------------------------------------
// Per selected window centre and channel the derivative of -0.425 SSIM w.r.t. a window pixel (x_q, y_q) of the selected source
// is affine in (x_q, y_q): A + B y_q + C x_q with
//   k = -0.425 * 2/9, A = k [ mu_y (n2 - n1) / (d1 d2) - SSIM mu_x (1/d1 - 1/d2) ], B = k n1 / (d1 d2), C = -k SSIM / d2,
// the same expression as photo_loss_bwd_kernel's regrouped, so the tile keeps 3 doubles per channel instead of 6 (23 KB, 41 KB
// of LDS in all: three workgroups per CU at full resolution instead of two).
__global__ void __launch_bounds__(256)
photo_min_bwd_kernel(const float* __restrict__ depth, const float* __restrict__ warped0, const float* __restrict__ dwarp0,
                     const float* __restrict__ warped1, const float* __restrict__ dwarp1, const float* __restrict__ cur,
                     const unsigned char* __restrict__ sel, const float* __restrict__ out4, const float* __restrict__ g_out, int h,
                     int w, float lambda, double pixels, float* __restrict__ g_depth) {
  constexpr int HALO = 2, S = kTile + 2 * HALO, S1 = kTile + 2;
  __shared__ float s_w0[S * S * 3], s_w1[S * S * 3], s_c[S * S * 3];
  __shared__ double s_ld[S * S];
  __shared__ unsigned char s_m[S * S];
  __shared__ double s_st[S1 * S1 * 3 * 3];
  const int bi = blockIdx.z, x0 = blockIdx.x * kTile, y0 = blockIdx.y * kTile;
  const long long base = (long long)bi * h * w;
  for (int k = threadIdx.x; k < S * S; k += 256) {
    const int gy = y0 - HALO + k / S, gx = x0 - HALO + k % S;
    const bool in = gy >= 0 && gy < h && gx >= 0 && gx < w;
    const bool in1 = in && warped1;
    const long long o = base + (long long)gy * w + gx;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      s_w0[k * 3 + c] = in ? warped0[o * 3 + c] : 0.f;
      s_w1[k * 3 + c] = in1 ? warped1[o * 3 + c] : 0.f;
      s_c[k * 3 + c] = in ? cur[o * 3 + c] : 0.f;
    }
    unsigned char m = in ? sel[o] : 0;
    if (m > 2 || (m == 2 && !warped1)) m = 0;                      // a byte that names no present source selects nothing
    s_m[k] = m;
    s_ld[k] = in ? log((double)clip_depth(depth[o])) : 0.0;
  }
  __syncthreads();
  // a selected pixel is interior, so its window lies inside the image and inside the 2-pixel halo
  for (int k = threadIdx.x; k < S1 * S1; k += 256) {
    const int at = (k / S1 + 1) * S + (k % S1 + 1);
    if (s_m[at]) {
      const float* x = s_m[at] == 2 ? s_w1 : s_w0;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const WinStats s = win_stats<S>(x, s_c, at, c);
        const double i1 = 1.0 / s.d1, i2 = 1.0 / s.d2, inv = i1 * i2, ssim = s.n1 * s.n2 * inv;
        const double kk = -0.425 * (2.0 / 9.0);
        double* st = s_st + (k * 3 + c) * 3;
        st[0] = kk * (s.my * (s.n2 - s.n1) * inv - ssim * s.mx * (i1 - i2));
        st[1] = kk * s.n1 * inv;
        st[2] = -kk * ssim * i2;
      }
    }
  }
  __syncthreads();
  const int tx = threadIdx.x % kTile, ty = threadIdx.x / kTile;
  const int gx = x0 + tx, gy = y0 + ty;
  if (gx >= w || gy >= h) return;
  const int at = (ty + HALO) * S + (tx + HALO);
  const long long o = base + (long long)gy * w + gx;
  double acc0[3] = {0.0, 0.0, 0.0}, acc1[3] = {0.0, 0.0, 0.0};
#pragma unroll
  for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
    for (int dx = -1; dx <= 1; ++dx) {
      const int p = at + dy * S + dx;
      const int m = s_m[p];
      if (!m) continue;
      const int k = (ty + 1 + dy) * S1 + (tx + 1 + dx);
      const float* x = m == 2 ? s_w1 : s_w0;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const double* st = s_st + (k * 3 + c) * 3;
        const double xq = (double)x[at * 3 + c], yq = (double)s_c[at * 3 + c];
        double d = st[0] + st[1] * yq + st[2] * xq;
        if (dy == 0 && dx == 0) {
          const double e = xq - yq;
          d += 0.15 * (e > 0.0 ? 1.0 : (e < 0.0 ? -1.0 : 0.0));
        }
        if (m == 2) acc1[c] += d; else acc0[c] += d;
      }
    }
  const double n = (double)out4[3];
  double g = (acc0[0] * (double)dwarp0[o * 3] + acc0[1] * (double)dwarp0[o * 3 + 1]) + acc0[2] * (double)dwarp0[o * 3 + 2];
  if (dwarp1) g += (acc1[0] * (double)dwarp1[o * 3] + acc1[1] * (double)dwarp1[o * 3 + 1]) + acc1[2] * (double)dwarp1[o * 3 + 2];
  g /= 3.0 * (n > 1.0 ? n : 1.0);
  double sm = 0.0;
  const double ld = s_ld[at];
  if (gx < w - 1) { const double e = s_ld[at + 1] - ld; sm -= (e > 0.0 ? 1.0 : (e < 0.0 ? -1.0 : 0.0)) * edge_weight(s_c, at, at + 1); }
  if (gx > 0)     { const double e = ld - s_ld[at - 1]; sm += (e > 0.0 ? 1.0 : (e < 0.0 ? -1.0 : 0.0)) * edge_weight(s_c, at - 1, at); }
  if (gy < h - 1) { const double e = s_ld[at + S] - ld; sm -= (e > 0.0 ? 1.0 : (e < 0.0 ? -1.0 : 0.0)) * edge_weight(s_c, at, at + S); }
  if (gy > 0)     { const double e = ld - s_ld[at - S]; sm += (e > 0.0 ? 1.0 : (e < 0.0 ? -1.0 : 0.0)) * edge_weight(s_c, at - S, at); }
  const float draw = depth[o];
  const bool inside = draw >= 0.01f && draw <= 200.0f;
  g += (double)lambda * sm / (pixels * (double)clip_depth(draw));
  g_depth[o] = inside ? (float)((double)g_out[0] * g) : 0.0f;
}

inline bool photo_dims_ok(int b, int h, int w) {
  return b > 0 && h >= 3 && w >= 3 && (long long)b * h * w <= (1LL << 24);     // N travels as a float: exact up to 2^24
}
inline long long photo_blocks(int b, int h, int w) {
  return (long long)b * ((h + kTile - 1) / kTile) * ((w + kTile - 1) / kTile);
}

}  // namespace

extern "C" long long m4d_image_pyramid_floats(int n, int H, int W, int levels) {
  if (n <= 0 || H <= 0 || W <= 0 || levels < 1 || levels > 16 || H % (1 << levels) != 0 || W % (1 << levels) != 0) return -1;
  long long total = 0;
  for (int i = 1; i <= levels; ++i) total += (long long)n * (H >> i) * (W >> i) * 3;
  return total;
}

extern "C" int m4d_image_pyramid_box(const float* image, int n, int H, int W, int levels, float* out, void* stream) {
  M4D_CHECK_ARG(image && out && m4d_image_pyramid_floats(n, H, W, levels) > 0);
  const float* src = image;
  float* dst = out;
  for (int i = 1; i <= levels; ++i) {
    const int oh = H >> i, ow = W >> i;
    const long long total = (long long)n * oh * ow * 3;
    long long g = (total + 255) / 256;
    m4d_launch(pyramid_box_kernel, dim3((unsigned)(g > 8192 ? 8192 : g)), dim3(256), 0, (hipStream_t)stream, src, oh, ow, total, dst);
    src = dst;
    dst += total;
  }
  return M4D_LAUNCH_RESULT();
}

extern "C" int m4d_photo_warp_fwd(const float* depth, const float* rot, int rot_c, const float* trans, const float* cam_f,
                                  const float* cam_c, const float* prev, int b, int h, int w, float* warped, float* dwarp,
                                  unsigned char* valid, void* stream) {
  M4D_CHECK_ARG(depth && rot && trans && cam_f && cam_c && prev && warped && dwarp && valid);
  M4D_CHECK_ARG(photo_dims_ok(b, h, w) && (rot_c == 3 || rot_c == 4));
  int gx = m4d_blocks((long long)h * w, 256);
  if (gx > 4096) gx = 4096;
  m4d_launch(photo_warp_fwd_kernel, dim3(gx, b), dim3(256), 0, (hipStream_t)stream, depth, rot, rot_c, trans, cam_f, cam_c, prev,
             h, w, warped, dwarp, valid);
  return M4D_LAUNCH_RESULT();
}

extern "C" long long m4d_photo_workspace_bytes(int b, int h, int w) {
  if (!photo_dims_ok(b, h, w)) return -1;
  return photo_blocks(b, h, w) * 3 * (long long)sizeof(double);
}

extern "C" int m4d_photo_loss_fwd(const float* depth, const float* warped, const unsigned char* valid, const float* cur,
                                  const float* prev, int b, int h, int w, float lambda, int automask, void* workspace,
                                  float* out4, unsigned char* mask, void* stream) {
  M4D_CHECK_ARG(depth && warped && valid && cur && prev && workspace && out4 && mask);
  M4D_CHECK_ARG(photo_dims_ok(b, h, w) && (((uintptr_t)workspace) & 7u) == 0);
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((w + kTile - 1) / kTile, (h + kTile - 1) / kTile, b);
  m4d_launch(photo_loss_fwd_kernel, grid, dim3(256), 0, s, depth, warped, valid, cur, prev, h, w, automask, mask,
             (double*)workspace);
  m4d_launch(photo_loss_finish_kernel, dim3(1), dim3(256), 0, s, (const double*)workspace, photo_blocks(b, h, w),
             (double)b * h * w, lambda, out4);
  return M4D_LAUNCH_RESULT();
}

extern "C" int m4d_photo_loss_bwd(const float* depth, const float* warped, const float* dwarp, const float* cur,
                                  const unsigned char* mask, const float* out4, const float* g_out, int b, int h, int w,
                                  float lambda, float* g_depth, void* stream) {
  M4D_CHECK_ARG(depth && warped && dwarp && cur && mask && out4 && g_out && g_depth);
  M4D_CHECK_ARG(photo_dims_ok(b, h, w));
  const dim3 grid((w + kTile - 1) / kTile, (h + kTile - 1) / kTile, b);
  m4d_launch(photo_loss_bwd_kernel, grid, dim3(256), 0, (hipStream_t)stream, depth, warped, dwarp, cur, mask, out4, g_out, h, w,
             lambda, (double)b * h * w, g_depth);
  return M4D_LAUNCH_RESULT();
}

// ---- full resolution, two sources -----------------------------------------------------------------------------------------------
namespace {
inline bool upsample_dims_ok(int b, int h, int w, int s) {
  if (b <= 0 || h < 1 || w < 1 || s < 2 || s > 64 || (s & (s - 1)) != 0) return false;
  const long long H = (long long)h * s, W = (long long)w * s;
  return H <= (1 << 24) && W <= (1 << 24) && (long long)b * H <= (1LL << 24) && (long long)b * H * W <= (1LL << 24);
}
}  // namespace

extern "C" int m4d_upsample_hp_fwd(const float* x, int b, int h, int w, int s, float* out, void* stream) {
  M4D_CHECK_ARG(x && out && upsample_dims_ok(b, h, w, s));
  const long long total = (long long)b * h * s * w * s;
  long long g = (total + 255) / 256;
  m4d_launch(upsample_hp_fwd_kernel, dim3((unsigned)(g > 8192 ? 8192 : g)), dim3(256), 0, (hipStream_t)stream, x, h, w, s, total, out);
  return M4D_LAUNCH_RESULT();
}

extern "C" int m4d_upsample_hp_bwd(const float* g_out, int b, int h, int w, int s, float* g_x, void* stream) {
  M4D_CHECK_ARG(g_out && g_x && upsample_dims_ok(b, h, w, s));
  const long long total = (long long)b * h * w;
  if (s <= 4)
    m4d_launch(upsample_hp_bwd_thread_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, g_out, h, w, s,
               total, g_x);
  else
    m4d_launch(upsample_hp_bwd_wave_kernel, dim3((unsigned)((total + 3) / 4)), dim3(256), 0, (hipStream_t)stream, g_out, h, w, s, total,
               g_x);
  return M4D_LAUNCH_RESULT();
}

extern "C" int m4d_photo_identity_fwd(const float* cur, const float* src0, const float* src1, int b, int h, int w, float* pe_id,
                                      void* stream) {
  M4D_CHECK_ARG(cur && src0 && pe_id && photo_dims_ok(b, h, w));
  const dim3 grid((w + kTile - 1) / kTile, (h + kTile - 1) / kTile, b);
  m4d_launch(photo_identity_kernel, grid, dim3(256), 0, (hipStream_t)stream, cur, src0, src1, h, w, pe_id);
  return M4D_LAUNCH_RESULT();
}

extern "C" long long m4d_photo_min_workspace_bytes(int b, int h, int w) { return m4d_photo_workspace_bytes(b, h, w); }

extern "C" int m4d_photo_min_fwd(const float* depth, const float* warped0, const unsigned char* valid0, const float* warped1,
                                 const unsigned char* valid1, const float* cur, const float* pe_id, int b, int h, int w,
                                 float lambda, void* workspace, float* out4, unsigned char* sel, void* stream) {
  M4D_CHECK_ARG(depth && warped0 && valid0 && cur && workspace && out4 && sel && (warped1 != nullptr) == (valid1 != nullptr));
  M4D_CHECK_ARG(photo_dims_ok(b, h, w) && (((uintptr_t)workspace) & 7u) == 0);
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((w + kTile - 1) / kTile, (h + kTile - 1) / kTile, b);
  m4d_launch(photo_min_fwd_kernel, grid, dim3(256), 0, s, depth, warped0, valid0, warped1, valid1, cur, pe_id, h, w, sel,
             (double*)workspace);
  m4d_launch(photo_loss_finish_kernel, dim3(1), dim3(256), 0, s, (const double*)workspace, photo_blocks(b, h, w),
             (double)b * h * w, lambda, out4);
  return M4D_LAUNCH_RESULT();
}

extern "C" int m4d_photo_min_bwd(const float* depth, const float* warped0, const float* dwarp0, const float* warped1,
                                 const float* dwarp1, const float* cur, const unsigned char* sel, const float* out4,
                                 const float* g_out, int b, int h, int w, float lambda, float* g_depth, void* stream) {
  M4D_CHECK_ARG(depth && warped0 && dwarp0 && cur && sel && out4 && g_out && g_depth && (warped1 != nullptr) == (dwarp1 != nullptr));
  M4D_CHECK_ARG(photo_dims_ok(b, h, w));
  const dim3 grid((w + kTile - 1) / kTile, (h + kTile - 1) / kTile, b);
  m4d_launch(photo_min_bwd_kernel, grid, dim3(256), 0, (hipStream_t)stream, depth, warped0, dwarp0, warped1, dwarp1, cur, sel, out4,
             g_out, h, w, lambda, (double)b * h * w, g_depth);
  return M4D_LAUNCH_RESULT();
}
