// Two small fused reductions that the reference runs as a dozen (DINL) / ~50 (metrics)
// separate TF ops, and that PyTorch would run as as many tiny kernels:
//   * DomainNormalization (m4depth_network.py:44-48) fused with the leaky_relu that follows it
//     at encoder level 0 (:82-84): two deterministic two-stage reductions (mean, then the
//     two-pass variance TF computes) and ONE apply pass, instead of ~12 passes over the
//     largest activation of the network ([b,H,W,16]);
//   * the 7 depth metrics of metrics.py in one pass over (gt, est).
// Partial sums are combined in a fixed order (no atomics): results are run-to-run identical.  The DINL statistics are summed
// in double from the first add on: a frame whose mean dwarfs its spread, or a flat frame (an all-zero one included), keeps
// its digits, and the mean of a constant channel is exact, so its variance is exactly 0.
#include <type_traits>
#include "m4d_common.h"
#include "../../include/m4depth_hip.h"

namespace {

constexpr int kDinlMaxBlocks = 512;
// Workspace of the DINL entry points, per image: kDinlMaxBlocks x C double partials, then mean [b][C], var [b][C] (floats)
__host__ __device__ constexpr long long dinl_partial_floats(int b, int C) { return 2LL * b * kDinlMaxBlocks * C; }

// pass 0: sum x ; pass 1: sum (x - mean)^2, per (batch, channel); C % 4 == 0, C/4 divides 256
__global__ void __launch_bounds__(256)
dinl_partial_kernel(const float* __restrict__ x, const float* __restrict__ mean, int hw, int C, int pass,
                    double* __restrict__ partial) {
  __shared__ double sh[4][256];
  const int bi = blockIdx.y;
  const int c4n = C >> 2;
  const int ppi = 256 / c4n;                       // pixels per block iteration
  const int c4 = threadIdx.x % c4n, po = threadIdx.x / c4n;
  const float* xb = x + (long long)bi * hw * C;
  float4 m = make_float4(0.f, 0.f, 0.f, 0.f);
  if (pass == 1) m = *reinterpret_cast<const float4*>(mean + bi * C + c4 * 4);
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  for (int p = blockIdx.x * ppi + po; p < hw; p += gridDim.x * ppi) {
    float4 v = *reinterpret_cast<const float4*>(xb + (long long)p * C + c4 * 4);
    if (pass == 1) {
      v.x = v.x - m.x; v.y = v.y - m.y; v.z = v.z - m.z; v.w = v.w - m.w;
      v.x = v.x * v.x; v.y = v.y * v.y; v.z = v.z * v.z; v.w = v.w * v.w;
    }
    acc[0] += (double)v.x; acc[1] += (double)v.y; acc[2] += (double)v.z; acc[3] += (double)v.w;
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) sh[e][threadIdx.x] = acc[e];
  __syncthreads();
  if (po == 0) {                                   // fixed-order combine of the ppi partials of this channel group
    double* pp = partial + ((long long)bi * gridDim.x + blockIdx.x) * C + c4 * 4;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      double s = sh[e][c4];
      for (int r = 1; r < ppi; ++r) s += sh[e][r * c4n + c4];
      pp[e] = s;
    }
  }
}

// 256 lanes: lane (j, c) sums every (256/C)-th partial of channel c, then the 256/C sub-sums are
// combined in index order -- a fixed summation tree, so the result is run-to-run identical.
__global__ void __launch_bounds__(256)
dinl_finalize_kernel(const double* __restrict__ partial, int nblk, int C, int hw, float* __restrict__ out) {
  __shared__ double sh[256];
  const int bi = blockIdx.x;
  const int c = threadIdx.x % C, j = threadIdx.x / C, nj = 256 / C;
  double s = 0.0;
  for (int k = j; k < nblk; k += nj) s += partial[((long long)bi * nblk + k) * C + c];
  sh[threadIdx.x] = s;
  __syncthreads();
  if (j == 0) {
    for (int r = 1; r < nj; ++r) s += sh[r * C + c];
    out[bi * C + c] = (float)(s / (double)hw);
  }
}

template <int C>
__global__ void __launch_bounds__(256)
dinl_apply_kernel(const float* __restrict__ x, const float* __restrict__ mean, const float* __restrict__ var,
                  const float* __restrict__ scale, const float* __restrict__ bias, int hw, int w, float slope,
                  float* __restrict__ out, int out_h, int out_w, int off_y, int off_x) {
  const int bi = blockIdx.y;
  float mu[C], dv[C], sc[C], bs[C];
#pragma unroll
  for (int c = 0; c < C; ++c) {
    mu[c] = mean[bi * C + c];
    dv[c] = var[bi * C + c] + 1e-12f;              // (x - mean) / (var + 1e-12): variance, not std (:47)
    sc[c] = scale[c];
    bs[c] = bias[c];
  }
  for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < hw; p += gridDim.x * blockDim.x) {
    const float* px = x + ((long long)bi * hw + p) * C;
    float n[C];
    float ss = 0.f;
#pragma unroll
    for (int c = 0; c < C; c += 4) {
      const float4 v = *reinterpret_cast<const float4*>(px + c);
      n[c] = (v.x - mu[c]) / dv[c]; n[c + 1] = (v.y - mu[c + 1]) / dv[c + 1];
      n[c + 2] = (v.z - mu[c + 2]) / dv[c + 2]; n[c + 3] = (v.w - mu[c + 3]) / dv[c + 3];
    }
#pragma unroll
    for (int c = 0; c < C; ++c) ss = ss + n[c] * n[c];
    const float inv = 1.0f / sqrtf(fmaxf(ss, 1e-12f));                    // tf.math.l2_normalize
    float* po = out + (((long long)bi * out_h + (p / w + off_y)) * out_w + (p % w + off_x)) * C;   // dense or padded target
#pragma unroll
    for (int c = 0; c < C; c += 4) {
      float4 o;
      o.x = sc[c] * (n[c] * inv) + bs[c]; o.y = sc[c + 1] * (n[c + 1] * inv) + bs[c + 1];
      o.z = sc[c + 2] * (n[c + 2] * inv) + bs[c + 2]; o.w = sc[c + 3] * (n[c + 3] * inv) + bs[c + 3];
      o.x = o.x > 0.f ? o.x : o.x * slope; o.y = o.y > 0.f ? o.y : o.y * slope;
      o.z = o.z > 0.f ? o.z : o.z * slope; o.w = o.w > 0.f ? o.w : o.w * slope;
      *reinterpret_cast<float4*>(po + c) = o;
    }
  }
}

// ---- encoder level 0, first convolution: 3 -> 16 channels, stride 1, + bias, + the DINL mean partial sums ------
// K = 27 is far too small for the matrix cores and the layer writes the largest activation of the network
// ([b,H,W,16]) once; a direct convolution with the 27 x 16 weights read through the scalar cache.  The
// workgroup also leaves the per-channel sums of its outputs for the DINL mean (same partial layout as
// dinl_partial_kernel pass 0), which saves one full read of that activation.
template <int C>
__global__ void __launch_bounds__(256)
enc_head_conv_kernel(const float* __restrict__ img, const float* __restrict__ w27, const float* __restrict__ bias,
                     int h, int w, int bsz, long long stride_b, long long stride_t,
                     float* __restrict__ out, double* __restrict__ partial) {
  __shared__ double sh[4][C];
  const int bi = blockIdx.y;
  const int hw = h * w;
  // image bi = frame (bi / bsz) of sequence (bi % bsz): the frames of a [b,T,H,W,3] batch are encoded in one launch,
  // frame-major, straight from the sequence tensor (no stacking copy)
  const float* ib = img + (long long)(bi % bsz) * stride_b + (long long)(bi / bsz) * stride_t;
  float* ob = out + (long long)bi * hw * C;
  double csum[C];
#pragma unroll
  for (int c = 0; c < C; ++c) csum[c] = 0.0;
  for (int p = blockIdx.x * 256 + threadIdx.x; p < hw; p += gridDim.x * 256) {
    const int y = p / w, x = p - y * w;
    typedef float f2 __attribute__((ext_vector_type(2)));         // packed v_pk_mul_f32 / v_pk_add_f32: two channels per op
    f2 acc2[C / 2];
#pragma unroll
    for (int c = 0; c < C / 2; ++c) acc2[c] = (f2){0.f, 0.f};
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
      const int yy = y + ky - 1;
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
        const int xx = x + kx - 1;
        const bool in = yy >= 0 && yy < h && xx >= 0 && xx < w;
        const float* px = ib + ((long long)(in ? yy : y) * w + (in ? xx : x)) * 3;
        const float v0 = in ? px[0] : 0.f, v1 = in ? px[1] : 0.f, v2 = in ? px[2] : 0.f;
        const f2* wt = reinterpret_cast<const f2*>(w27 + (ky * 3 + kx) * 3 * C);   // HWIO: [tap][cin][cout], uniform -> scalar loads
#pragma unroll
        for (int c = 0; c < C / 2; ++c)
          acc2[c] = ((acc2[c] + (f2){v0, v0} * wt[c]) + (f2){v1, v1} * wt[C / 2 + c]) + (f2){v2, v2} * wt[C + c];
      }
    }
    float acc[C];
#pragma unroll
    for (int c = 0; c < C / 2; ++c) { acc[2 * c] = acc2[c].x; acc[2 * c + 1] = acc2[c].y; }
#pragma unroll
    for (int c = 0; c < C; c += 4) {
      float4 o = make_float4(acc[c] + bias[c], acc[c + 1] + bias[c + 1], acc[c + 2] + bias[c + 2], acc[c + 3] + bias[c + 3]);
      *reinterpret_cast<float4*>(ob + (long long)p * C + c) = o;
      csum[c] += (double)o.x; csum[c + 1] += (double)o.y; csum[c + 2] += (double)o.z; csum[c + 3] += (double)o.w;
    }
  }
  // fixed-order reduction: butterfly inside the wave, then the 4 waves in index order
#pragma unroll
  for (int c = 0; c < C; ++c) {
    double v = csum[c];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6][c] = v;
  }
  __syncthreads();
  if (threadIdx.x < C)
    partial[((long long)bi * gridDim.x + blockIdx.x) * C + threadIdx.x] =
        ((sh[0][threadIdx.x] + sh[1][threadIdx.x]) + sh[2][threadIdx.x]) + sh[3][threadIdx.x];
}

// ---- metrics.py in one pass ---------------------------------------------------------
constexpr int kMetricSums = 9;
constexpr int kMetricBlocks = 512;

__global__ void __launch_bounds__(256)
metrics_partial_kernel(const float* __restrict__ gt_raw, const float* __restrict__ est_raw, long long n, float max_d,
                       double* __restrict__ partial, long long per_image, long long gt_image_stride) {
  // gt image j starts at gt_raw + j * gt_image_stride (the last frame of a [b,T,H,W,1] sequence batch, read in place:
  // m4depth_network.py:455); element i of the dense walk = (image i / per_image, offset i % per_image), kept incrementally --
  // same elements per thread in the same order as the dense form, so the sums are the same bits
  float s[kMetricSums];
#pragma unroll
  for (int k = 0; k < kMetricSums; ++k) s[k] = 0.f;
  const long long step = (long long)gridDim.x * blockDim.x;
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  long long img = i / per_image, off = i - img * per_image;
  for (; i < n; i += step) {
    const float gt = fminf(fmaxf(gt_raw[img * gt_image_stride + off], 0.0f), max_d);               // m4depth_network.py:465-467
    off += step;
    while (off >= per_image) { off -= per_image; ++img; }
    const float est = fminf(fmaxf(est_raw[i], 0.001f), max_d);
    const bool m = gt > 1e-6f;                                            // metrics.py:3-5
    const float diff = gt - est;
    const float lg = logf(gt + 1e-6f), le = logf(est + 1e-6f);
    const bool m2 = lg > 1e-6f;                                           // RMSE_log masks on the LOG (metrics.py:24-28)
    const float th = fmaxf(gt / est, est / gt);
    if (m) {
      s[0] += 1.0f;
      s[1] += fabsf(diff) / (gt + 1e-6f);
      s[2] += diff * diff / (gt + 1e-6f);
      s[3] += diff * diff;
      s[6] += th < 1.25f ? 1.0f : 0.0f;
      s[7] += th < 1.5625f ? 1.0f : 0.0f;
      s[8] += th < 1.953125f ? 1.0f : 0.0f;
    }
    if (m2) { s[4] += 1.0f; s[5] += (lg - le) * (lg - le); }
  }
  __shared__ double sh[4][kMetricSums];
#pragma unroll
  for (int k = 0; k < kMetricSums; ++k) {
    double v = (double)s[k];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);             // fixed tree: deterministic
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6][k] = v;
  }
  __syncthreads();
  if (threadIdx.x < kMetricSums)
    partial[(long long)blockIdx.x * kMetricSums + threadIdx.x] =
        ((sh[0][threadIdx.x] + sh[1][threadIdx.x]) + sh[2][threadIdx.x]) + sh[3][threadIdx.x];
}

__global__ void __launch_bounds__(kMetricSums * 32)
metrics_finalize_kernel(const double* __restrict__ partial, int nblk, float* __restrict__ out7,
                        float* __restrict__ total7, float count, float* __restrict__ mean7) {
  __shared__ double sub[kMetricSums * 32];
  __shared__ double tot[kMetricSums];
  const int q = threadIdx.x % kMetricSums, j = threadIdx.x / kMetricSums;    // 32 sub-sums per quantity
  double s = 0.0;
  for (int k = j; k < nblk; k += 32) s += partial[(long long)k * kMetricSums + q];
  sub[threadIdx.x] = s;
  __syncthreads();
  if (j == 0) {
    for (int r = 1; r < 32; ++r) s += sub[r * kMetricSums + q];               // fixed order
    tot[q] = s;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const double cnt = tot[0] > 1.0 ? tot[0] : 1.0, cnt2 = tot[4] > 1.0 ? tot[4] : 1.0;
    out7[0] = (float)(tot[1] / cnt);                 // AbsRel
    out7[1] = (float)(tot[2] / cnt);                 // SqRel
    out7[2] = sqrtf((float)(tot[3] / cnt));          // RMSE
    out7[3] = sqrtf((float)(tot[5] / cnt2));         // RMSE_log
    out7[4] = (float)(tot[6] / cnt);                 // Delta1..3
    out7[5] = (float)(tot[7] / cnt);
    out7[6] = (float)(tot[8] / cnt);
    if (total7) {                                    // Keras Mean (metrics.py): total += per-batch value; result = total / count
#pragma unroll
      for (int i = 0; i < 7; ++i) {
        const float t = total7[i] + out7[i];
        total7[i] = t;
        if (mean7) mean7[i] = t / count;
      }
    }
  }
}

// ---- the same metrics per sample of a batch (batched streaming evaluation) -----------------------------------------
// Sample s = blockIdx.y is scored alone, with the block partition and per-thread element order m4d_depth_metrics uses for
// one image of n floats (gridDim.x = min(ceil(n / 256), kMetricBlocks)): its float partials, their double combine and the
// finalize below are those of metrics_partial_kernel / metrics_finalize_kernel, so row s is the same bits as a call on
// image s by itself.  Partials: [b][gridDim.x][kMetricSums] doubles.
__global__ void __launch_bounds__(256)
metrics_partial_ps_kernel(const float* __restrict__ gt_raw, long long gt_stride, const float* __restrict__ est_raw,
                          long long est_stride, long long n, float max_d, double* __restrict__ partial) {
  const float* gt_img = gt_raw + (long long)blockIdx.y * gt_stride;
  const float* est_img = est_raw + (long long)blockIdx.y * est_stride;
  float s[kMetricSums];
#pragma unroll
  for (int k = 0; k < kMetricSums; ++k) s[k] = 0.f;
  const long long step = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += step) {
    const float gt = fminf(fmaxf(gt_img[i], 0.0f), max_d);
    const float est = fminf(fmaxf(est_img[i], 0.001f), max_d);
    const bool m = gt > 1e-6f;
    const float diff = gt - est;
    const float lg = logf(gt + 1e-6f), le = logf(est + 1e-6f);
    const bool m2 = lg > 1e-6f;
    const float th = fmaxf(gt / est, est / gt);
    if (m) {
      s[0] += 1.0f;
      s[1] += fabsf(diff) / (gt + 1e-6f);
      s[2] += diff * diff / (gt + 1e-6f);
      s[3] += diff * diff;
      s[6] += th < 1.25f ? 1.0f : 0.0f;
      s[7] += th < 1.5625f ? 1.0f : 0.0f;
      s[8] += th < 1.953125f ? 1.0f : 0.0f;
    }
    if (m2) { s[4] += 1.0f; s[5] += (lg - le) * (lg - le); }
  }
  __shared__ double sh[4][kMetricSums];
#pragma unroll
  for (int k = 0; k < kMetricSums; ++k) {
    double v = (double)s[k];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6][k] = v;
  }
  __syncthreads();
  if (threadIdx.x < kMetricSums)
    partial[((long long)blockIdx.y * gridDim.x + blockIdx.x) * kMetricSums + threadIdx.x] =
        ((sh[0][threadIdx.x] + sh[1][threadIdx.x]) + sh[2][threadIdx.x]) + sh[3][threadIdx.x];
}

// one workgroup per sample: the fixed-order finalize of metrics_finalize_kernel into rows[s][7], and the counting flag
// counted[s] = active[s] && !new_traj[s] (the masks are read here, never by the host)
__global__ void __launch_bounds__(kMetricSums * 32)
metrics_finalize_ps_kernel(const double* __restrict__ partial, int nblk, const unsigned char* __restrict__ new_traj,
                           const unsigned char* __restrict__ active, float* __restrict__ rows, unsigned char* __restrict__ counted) {
  __shared__ double sub[kMetricSums * 32];
  __shared__ double tot[kMetricSums];
  const int smp = blockIdx.x;
  const double* pp = partial + (long long)smp * nblk * kMetricSums;
  const int q = threadIdx.x % kMetricSums, j = threadIdx.x / kMetricSums;
  double s = 0.0;
  for (int k = j; k < nblk; k += 32) s += pp[(long long)k * kMetricSums + q];
  sub[threadIdx.x] = s;
  __syncthreads();
  if (j == 0) {
    for (int r = 1; r < 32; ++r) s += sub[r * kMetricSums + q];
    tot[q] = s;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const double cnt = tot[0] > 1.0 ? tot[0] : 1.0, cnt2 = tot[4] > 1.0 ? tot[4] : 1.0;
    float* out7 = rows + (long long)smp * 7;
    out7[0] = (float)(tot[1] / cnt);
    out7[1] = (float)(tot[2] / cnt);
    out7[2] = sqrtf((float)(tot[3] / cnt));
    out7[3] = sqrtf((float)(tot[5] / cnt2));
    out7[4] = (float)(tot[6] / cnt);
    out7[5] = (float)(tot[7] / cnt);
    out7[6] = (float)(tot[8] / cnt);
    counted[smp] = (active[smp] != 0 && new_traj[smp] == 0) ? 1 : 0;
  }
}


// ---- encoder level 0 WITHOUT its [b,H,W,16] intermediate (m4d_enc_level0_fwd) ------------------------------------------
// The head of the network (m4depth_network.py:79-87 with DINL) is conv3x3(RGB, 3 -> 16) -> DomainNormalization ->
// leaky_relu -> conv3x3 stride 2 (16 -> 16).  The 16-channel full-resolution map (63 MB for two 384x1280 frames) was
// written once and read twice (two-pass variance, then the stride-2 convolution: ~190 us for two frames).  K = 27 is small
// but not too small for v_mfma_f32_16x16x4_f32 (16 pixels x 16 channels, 7 k-steps = 224 cycles per SIMD): the first
// convolution is cheap enough to be RECOMPUTED from the RGB image (12 MB) in every pass -- sum, squared deviations,
// and the fused pass that normalises the recomputed map in LDS and convolves it with stride 2.
typedef float f32x4 __attribute__((ext_vector_type(4)));

// Per-lane operands of the 3 -> 16 convolution as 16x16x4 MFMAs: lane (i = lane & 15, g = lane >> 4) supplies
// A[pixel i][k = 4 s + g] and B[k][cout i] in step s; k = (ky * 3 + kx) * 3 + channel = ky * 9 + (kx * 3 + channel), so the
// A element sits koff[s] = ky * row_stride + k % 9 floats after the window's top-left RGB value.  k = 27 (s = 6, g = 3) is
// padding: zero weight.
__device__ __forceinline__ void enc0_lane_setup(const float* __restrict__ w27, int lane, int row_stride, int (&koff)[7], float (&wb)[7]) {
  const int j = lane & 15, g = lane >> 4;
#pragma unroll
  for (int s = 0; s < 7; ++s) {
    const int k = 4 * s + g;
    const bool valid = k < 27;
    const int kk = valid ? k : 0;
    koff[s] = (kk / 9) * row_stride + kk % 9;
    wb[s] = valid ? w27[k * 16 + j] : 0.f;
  }
}
// window_base = &tile[window top-left of pixel i of this lane]; returns rows 4 g .. 4 g + 3 (pixels) of column j (cout)
__device__ __forceinline__ f32x4 enc0_conv1(const float* window_base, const int (&koff)[7], const float (&wb)[7]) {
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int s = 0; s < 7; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(window_base[koff[s]], wb[s], acc, 0, 0, 0);
  return acc;
}

constexpr int kE0TW = 128, kE0TH = 8;              // statistics tile (pixels)
constexpr int kE0RS = (kE0TW + 2) * 3;             // floats per staged RGB row (390)

// The shift of the single-pass statistics (enc0_stats_kernel below): conv1 + bias at the image's centre pixel.  On a typical frame it is one
// sample of the very distribution whose moments are taken, and var = S2 / n - (S1 / n)^2 cancels little.  On a frame whose
// centre is unlike the rest (a flat or dark frame with a bright centre, a grey one with a black centre) (mean - K)^2 exceeds the
// variance by up to ~n: the sums are therefore taken in double from the first add on (y - K of two floats is exact in double),
// and the cancellation costs ~n x 1e-16 instead of every digit.  Evaluated with the same expression by the statistics kernel
// and by its finalisation.
// In two halves, so that a caller can put the loads beside its other loads: enc0_shift_load requests the 27 weights of
// channel j and the 27 RGB values of the centre window with independent loads (a tap outside the image reads pixel 0 instead
// and is skipped below), enc0_shift_sum is the multiply-add chain in tap order -- one memory round trip, not one per tap.
__device__ __forceinline__ void enc0_shift_load(const float* __restrict__ ib, const float* __restrict__ w27, int h, int w, int j,
                                                float (&sw)[27], float (&sp)[27]) {
  const int cy = h / 2, cx = w / 2;
#pragma unroll
  for (int ky = 0; ky < 3; ++ky)
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) {
      const int gy = cy + ky - 1, gx = cx + kx - 1;
      const bool ok = !(gy < 0 || gy >= h || gx < 0 || gx >= w);
      const long long base = ok ? ((long long)gy * w + gx) * 3 : 0LL;
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        sw[(ky * 3 + kx) * 3 + ch] = w27[((ky * 3 + kx) * 3 + ch) * 16 + j];
        sp[(ky * 3 + kx) * 3 + ch] = ib[base + ch];
      }
    }
}
__device__ __forceinline__ float enc0_shift_sum(float bias_j, const float (&sw)[27], const float (&sp)[27], int h, int w) {
  const int cy = h / 2, cx = w / 2;
  float y = bias_j;
#pragma unroll
  for (int ky = 0; ky < 3; ++ky)
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) {
      const int gy = cy + ky - 1, gx = cx + kx - 1;
      const bool ok = !(gy < 0 || gy >= h || gx < 0 || gx >= w);
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) y = ok ? y + sw[(ky * 3 + kx) * 3 + ch] * sp[(ky * 3 + kx) * 3 + ch] : y;
    }
  return y;
}

constexpr int kE0TE = (kE0TH + 2) * kE0RS;         // staged floats per statistics tile (3900)
constexpr int kE0NL = (kE0TE + 255) / 256;         // ... per thread (16)
static_assert(kE0RS > 256 && kE0RS < 512, "enc0_tile_load: thread t starts in row 0 and crosses at most one row end per step of 256");
// Element idx = t + 256 i of the tile at (y0, x0) -> v[i], every load requested before the first is waited for: (row, column) of
// idx advance by 256 without a division, and an element outside the image (or past the tile's end) reads the nearest pixel
// inside -- no branch stands between two loads.  Returns the mask of the elements inside the image (bit i); enc0_tile_store applies it, so that
// nothing touches v[] -- and waits for the loads -- between the two calls.
__device__ __forceinline__ unsigned enc0_tile_load(const float* __restrict__ ib, int h, int w, int y0, int x0, int t, float (&v)[kE0NL]) {
  const int row3 = w * 3, gy0 = y0 - 1, gc0 = (x0 - 1) * 3;
  int r = 0, cc = t;
  unsigned mask = 0u;
#pragma unroll
  for (int i = 0; i < kE0NL; ++i) {
    const int gy = gy0 + r, gxc = gc0 + cc;
    const bool in = r < kE0TH + 2 && gy >= 0 && gy < h && gxc >= 0 && gxc < row3;
    v[i] = ib[(long long)min(max(gy, 0), h - 1) * row3 + min(max(gxc, 0), row3 - 1)];
    mask |= in ? 1u << i : 0u;
    cc += 256;
    if (cc >= kE0RS) { cc -= kE0RS; ++r; }
  }
  return mask;
}
__device__ __forceinline__ void enc0_tile_store(float* __restrict__ tile, int t, const float (&v)[kE0NL], unsigned mask) {
#pragma unroll
  for (int i = 0; i < kE0NL; ++i)
    if (t + 256 * i < kE0TE) tile[t + 256 * i] = (mask >> i & 1u) ? v[i] : 0.f;
}

// BOTH moments of conv1 + bias in one pass -- S1 = sum (y - K), S2 = sum (y - K)^2 with the per-image, per-channel shift K of
// enc0_shift_load / enc0_shift_sum -- double partials [image][block][32] (16 x S1, 16 x S2), finished by enc0_moments_finalize_kernel: the level-0
// statistics are TWO dependent launches (round 5 took four: RGB totals, analytic mean, squared deviations, finalisation; slower,
// profiles/r06_enc0_single_pass_ab.txt, and retired).  A workgroup walks tiles blockIdx.x, + gridDim.x, ...  Every sum is a double,
// per lane, through the butterfly and the workgroup combine, in a fixed order.
// (`unused` was the mean of the retired two-pass variance; it stays in the signature because dropping it moves the kernel's other
//  arguments, which changes the kernel's code and belongs in a measured change.)
__global__ void __launch_bounds__(256)
enc0_stats_kernel(const float* __restrict__ img, const float* __restrict__ w27, const float* __restrict__ bias,
                  const float* __restrict__ unused, int h, int w, int bsz, long long stride_b, long long stride_t,
                  int tiles_x, int n_tiles, double* __restrict__ partial) {
  __shared__ float tile[2][kE0TE];                 // 2 x 15.6 KB: the next tile is staged while this one is consumed
  __shared__ double sh[2][4][16];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int j = lane & 15, g = lane >> 4;
  const int bi = blockIdx.y;
  const float* ib = img + (long long)(bi % bsz) * stride_b + (long long)(bi / bsz) * stride_t;
  // one round trip to memory for everything the first tile needs: its pixels, the lane's weights, and the shift's operands
  float v[kE0NL];
  int ti = blockIdx.x;
  unsigned vmask = 0u;
  if (ti < n_tiles) vmask = enc0_tile_load(ib, h, w, (ti / tiles_x) * kE0TH, (ti % tiles_x) * kE0TW, t, v);
  float sw[27], sp[27];
  enc0_shift_load(ib, w27, h, w, j, sw, sp);
  int koff[7]; float wb[7];
  enc0_lane_setup(w27, lane, kE0RS, koff, wb);
  const float bias_j = bias[j];
  const double shift_j = (double)enc0_shift_sum(bias_j, sw, sp, h, w);
  double csum = 0.0, csum2 = 0.0;
  if (ti < n_tiles) enc0_tile_store(tile[0], t, v, vmask);
  __syncthreads();
  int cur = 0;
  for (; ti < n_tiles; ti += gridDim.x) {
    const int y0 = (ti / tiles_x) * kE0TH, x0 = (ti % tiles_x) * kE0TW;
    const int tn = ti + gridDim.x;
    const bool more = tn < n_tiles;                // (the same in every thread of the workgroup)
    if (more) vmask = enc0_tile_load(ib, h, w, (tn / tiles_x) * kE0TH, (tn % tiles_x) * kE0TW, t, v);   // in flight during the MFMAs below
    const float* tb = tile[cur];
    // A tile that lies inside the image whole (every tile of a 384 x 1280 frame) takes the copy of this code whose per-pixel
    // "inside the image" test is folded away: the kernel is bound by its VALU instructions, and that is a third of the sums'.
    // (Rolled to four chains at a time: unrolled further, the scheduler keeps all sixteen results of a tile live beside the staged
    //  registers, and the kernel no longer fits four workgroups per CU.)
    auto tile_sums = [&](auto whole) {
      constexpr bool kWhole = decltype(whole)::value;
#pragma unroll 1
      for (int rr = 0; rr < 2; ++rr) {
        const int yl = 2 * wv + rr;
#pragma unroll 4
        for (int ct = 0; ct < kE0TW / 16; ++ct) {
          const float* wnd = tb + yl * kE0RS + 3 * (16 * ct + j);
          const f32x4 acc = enc0_conv1(wnd, koff, wb);
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const bool valid = kWhole || (y0 + yl < h && x0 + 16 * ct + 4 * g + r < w);
            const float v1 = acc[r] + bias_j;
            const double d = valid ? (double)v1 - shift_j : 0.0;
            csum += d;
            csum2 = fma(d, d, csum2);
          }
        }
      }
    };
    if (y0 + kE0TH <= h && x0 + kE0TW <= w) tile_sums(std::true_type{}); else tile_sums(std::false_type{});
    if (more) {
      enc0_tile_store(tile[cur ^ 1], t, v, vmask);
      __syncthreads();                             // the other buffer is complete, and this one is consumed: the only barrier per tile
    }
    cur ^= 1;
  }
  csum += __shfl_xor(csum, 16);                    // the four pixel groups of a channel: fixed butterfly
  csum += __shfl_xor(csum, 32);
  csum2 += __shfl_xor(csum2, 16);
  csum2 += __shfl_xor(csum2, 32);
  if (lane < 16) { sh[0][wv][lane] = csum; sh[1][wv][lane] = csum2; }
  __syncthreads();
  constexpr int NQ = 32;                           // 16 x S1, 16 x S2
  if (t < NQ) {
    const int q = t >> 4, c = t & 15;
    partial[((long long)bi * gridDim.x + blockIdx.x) * NQ + t] = ((sh[q][0][c] + sh[q][1][c]) + sh[q][2][c]) + sh[q][3][c];
  }
}

// mean = K + S1 / n, var = S2 / n - (S1 / n)^2 (the biased variance of tf.math.reduce_variance) from the double partials above,
// added in block order by a fixed tree: run-to-run identical.  One workgroup per image; thread (c, j): channel c
// (32 columns: 16 x S1, 16 x S2), every 8th block from j.
__global__ void __launch_bounds__(256)
enc0_moments_finalize_kernel(const float* __restrict__ img, const double* __restrict__ partial, int nblk, const float* __restrict__ w27,
                             const float* __restrict__ bias, int h, int w, int bsz, long long stride_b, long long stride_t,
                             float* __restrict__ mean, float* __restrict__ var) {
  __shared__ double sh[256];
  const int bi = blockIdx.x, t = threadIdx.x;
  const int c = t & 31, j = t >> 5;
  // (the kernel is a latency chain on the head of the step: the shift's operands -- every thread takes those of channel t & 15,
  //  threads 0..15 use the result -- and all of a thread's partials are requested together, before the first add: one round trip;
  //  a partial past the last block reads element 0 and becomes 0 by a select)
  const float* ib0 = img + (long long)(bi % bsz) * stride_b + (long long)(bi / bsz) * stride_t;
  float sw[27], sp[27];
  enc0_shift_load(ib0, w27, h, w, t & 15, sw, sp);
  const float sbias = bias[t & 15];
  double pv[32];
  const int cnt = (nblk - j + 7) / 8;
#pragma unroll
  for (int i = 0; i < 32; ++i) {
    const double x = partial[i < cnt ? ((long long)bi * nblk + j + 8 * i) * 32 + c : 0LL];
    pv[i] = i < cnt ? x : 0.0;
  }
  const float shift = enc0_shift_sum(sbias, sw, sp, h, w);
  double s = 0.0;
#pragma unroll
  for (int i = 0; i < 32; ++i) s += pv[i];                         // block order j, j + 8, ...: fixed
  sh[t] = s;
  __syncthreads();
  if (t < 32) {
    for (int r = 1; r < 8; ++r) s += sh[r * 32 + t];
    sh[t] = s;
  }
  __syncthreads();
  if (t < 16) {
    const double n = (double)h * (double)w;
    const double m1 = sh[t] / n, m2 = sh[16 + t] / n;
    mean[bi * 16 + t] = (float)((double)shift + m1);
    const double v = m2 - m1 * m1;
    var[bi * 16 + t] = (float)(v > 0.0 ? v : 0.0);
  }
}

constexpr int kF0OW = 16, kF0OH = 8;               // stride-2 output tile
constexpr int kF0CW = 2 * kF0OW + 1, kF0CH = 2 * kF0OH + 1;   // conv1 region it needs: 33 x 17 (TF 'SAME' on an even size pads bottom / right)
constexpr int kF0RW = kF0CW + 2, kF0RH = kF0CH + 2;            // RGB region 35 x 19
constexpr int kF0RS = kF0RW * 3;                   // floats per staged RGB row (105)
constexpr int kF0NS = 17;                          // floats per normalised pixel in LDS (16 + 1: stride-2 reads conflict-free)
constexpr int kF0NP = kF0CW * kF0CH;               // 561 conv1 pixels

// conv1 recomputed on the 33x17 region, + bias, DomainNormalization, leaky_relu(dn_slope) -> LDS (zero outside the
// image: the stride-2 convolution's padding), then conv3x3 stride 2 (16 -> 16) + bias + leaky_relu(slope) -> out.
__global__ void __launch_bounds__(256)
enc0_fused_kernel(const float* __restrict__ img, const float* __restrict__ w27, const float* __restrict__ bias1,
                  const float* __restrict__ mean, const float* __restrict__ var, const float* __restrict__ dn_scale,
                  const float* __restrict__ dn_bias, float dn_slope, const float* __restrict__ w2, const float* __restrict__ bias2,
                  float slope, int h, int w, int oh, int ow, int pad_y, int pad_x, int bsz, long long stride_b, long long stride_t,
                  int tiles_x, float* __restrict__ out) {
  __shared__ float rgb[kF0RH * kF0RS];             // 8 KB
  __shared__ float nrm[kF0NP * kF0NS];             // 38 KB
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int j = lane & 15, g = lane >> 4;
  const int bi = blockIdx.y;
  const float* ib = img + (long long)(bi % bsz) * stride_b + (long long)(bi / bsz) * stride_t;
  const int oy0 = (blockIdx.x / tiles_x) * kF0OH, ox0 = (blockIdx.x % tiles_x) * kF0OW;
  const int cy0 = 2 * oy0 - pad_y, cx0 = 2 * ox0 - pad_x;   // conv1 region origin (image coordinates; TF 'SAME': pad_before = 0 on even sizes, 1 on odd)
  // staging: every load of the kernel -- the thread's 8 RGB elements idx = t + 256 i, the lane's weights of both convolutions,
  // the statistics -- is requested before the first is waited for; (row, column) of idx advance without a division, and an
  // element outside the image (or past the region's end) reads pixel 0 and becomes 0 by a select
  constexpr int kNL = (kF0RH * kF0RS + 255) / 256, kStep = 256 - 2 * kF0RS;
  static_assert(kStep >= 0 && kStep < kF0RS && 3 * kF0RS > 256, "the row / column walk below");
  float sv[kNL];
  {
    const int row3 = w * 3, gy0 = cy0 - 1, gc0 = (cx0 - 1) * 3;
    int r = (t >= kF0RS) + (t >= 2 * kF0RS), cc = t - r * kF0RS;
#pragma unroll
    for (int i = 0; i < kNL; ++i) {
      const int gy = gy0 + r, gxc = gc0 + cc;
      const bool in = r < kF0RH && gy >= 0 && gy < h && gxc >= 0 && gxc < row3;
      const float x = ib[in ? (long long)gy * row3 + gxc : 0LL];
      sv[i] = in ? x : 0.f;
      r += 2; cc += kStep;
      if (cc >= kF0RS) { cc -= kF0RS; ++r; }
    }
  }
  int koff[7]; float wb[7];
  enc0_lane_setup(w27, lane, kF0RS, koff, wb);
  const float bias_j = bias1[j];
  __shared__ float s_mu[16], s_dv[16], s_sc[16], s_bs[16];
  const float st_mu = mean[bi * 16 + (t & 15)], st_var = var[bi * 16 + (t & 15)], st_sc = dn_scale[t & 15], st_bs = dn_bias[t & 15];
  float wb2[36];                                   // B operand of the second convolution: k = tap * 16 + channel = 4 s + g
#pragma unroll
  for (int s = 0; s < 36; ++s) wb2[s] = w2[(4 * s + g) * 16 + j];
  const float bias2_j = bias2[j];
#pragma unroll
  for (int i = 0; i < kNL; ++i)
    if (t + 256 * i < kF0RH * kF0RS) rgb[t + 256 * i] = sv[i];
  if (t < 16) {
    s_mu[t] = st_mu;
    s_dv[t] = 1.0f / (st_var + 1e-12f);            // (x - mean) / (var + 1e-12): variance, not std (:47), as a multiply
    s_sc[t] = st_sc; s_bs[t] = st_bs;
  }
  __syncthreads();
  // ---- phase 1a: conv1 + bias of the 561 region pixels as 36 tiles of 16 (pixel p = 16 tile + i, row-major), 9 per wave -> LDS:
  // three tiles at a time on three accumulators (a chain is 7 dependent MFMAs: three chains interleaved keep the pipe busy);
  // only tile 35 is ragged (pixel 560 alone), the other 35 store unconditionally
  static_assert((kF0NP + 15) / 16 == 36 && kF0NP > 16 * 35, "nine 16-pixel tiles per wave, the last one of wave 3 ragged");
#pragma unroll 1                                   // (unrolled, the nine accumulators cost a workgroup per CU)
  for (int it = 0; it < 9; it += 3) {
    const float* wa[3];
#pragma unroll
    for (int u = 0; u < 3; ++u) {
      const int pa = min(16 * (wv + 4 * (it + u)) + j, kF0NP - 1);   // this lane's A pixel of tile u
      const int ay = pa / kF0CW, ax = pa - ay * kF0CW;
      wa[u] = rgb + ay * kF0RS + 3 * ax;
    }
    f32x4 c0 = {0.f, 0.f, 0.f, 0.f}, c1 = c0, c2 = c0;
#pragma unroll
    for (int s = 0; s < 7; ++s) {
      c0 = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[0][koff[s]], wb[s], c0, 0, 0, 0);
      c1 = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[1][koff[s]], wb[s], c1, 0, 0, 0);
      c2 = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[2][koff[s]], wb[s], c2, 0, 0, 0);
    }
    float* n0 = nrm + (16 * (wv + 4 * it) + 4 * g) * kF0NS + j;      // accumulator row r -> pixel 16 tile + 4 g + r
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      n0[r * kF0NS] = c0[r] + bias_j;
      n0[(64 + r) * kF0NS] = c1[r] + bias_j;
    }
    if (it < 6 || wv < 3) {
#pragma unroll
      for (int r = 0; r < 4; ++r) n0[(128 + r) * kF0NS] = c2[r] + bias_j;
    } else {                                       // tile 35
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (16 * 35 + 4 * g + r < kF0NP) n0[(128 + r) * kF0NS] = c2[r] + bias_j;
    }
  }
  __syncthreads();
  // ---- phase 1b: DomainNormalization + leaky_relu per pixel, in place (one thread per pixel: the 1/sqrt once, not per channel)
  for (int p = t; p < kF0NP; p += 256) {
    const int py = p / kF0CW, px = p - py * kF0CW;
    const bool inside = cy0 + py >= 0 && cy0 + py < h && cx0 + px >= 0 && cx0 + px < w;
    float* q = nrm + p * kF0NS;
    float n[16];
    float ss = 0.f;
#pragma unroll
    for (int c = 0; c < 16; ++c) { n[c] = (q[c] - s_mu[c]) * s_dv[c]; ss = ss + n[c] * n[c]; }
    const float inv = 1.0f / sqrtf(fmaxf(ss, 1e-12f));                      // tf.math.l2_normalize
#pragma unroll
    for (int c = 0; c < 16; ++c) {
      float o = s_sc[c] * (n[c] * inv) + s_bs[c];
      o = o > 0.f ? o : o * dn_slope;
      q[c] = inside ? o : 0.f;                     // outside the image: the zero padding of the stride-2 convolution
    }
  }
  __syncthreads();
  // ---- phase 2: 8 rows of 16 stride-2 outputs, 2 rows per wave; A[pixel i][k]: pixel (2 oy + ky, 2 i + kx), channel
  // (the two rows' chains of 36 alternate on two accumulators, and the A operands of step s + 2 are read from LDS while step s
  //  multiplies: one row after the other, every second MFMA waited for an LDS read issued just before it)
  constexpr int kS2 = 36;
  const float* base2 = nrm + ((4 * wv) * kF0CW + 2 * j) * kF0NS + g;
  auto a2 = [&](int rr, int s) {
    const int tap = s >> 2, ky = tap / 3, kx = tap - 3 * ky;
    return base2[((2 * rr + ky) * kF0CW + kx) * kF0NS + 4 * (s & 3)];
  };
  f32x4 acc2[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
  float xa[2][2] = {{a2(0, 0), a2(1, 0)}, {a2(0, 1), a2(1, 1)}};
#pragma unroll
  for (int s = 0; s < kS2; ++s) {
    const float x0 = xa[s & 1][0], x1 = xa[s & 1][1];
    if (s + 2 < kS2) { xa[s & 1][0] = a2(0, s + 2); xa[s & 1][1] = a2(1, s + 2); }
    acc2[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(x0, wb2[s], acc2[0], 0, 0, 0);
    acc2[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(x1, wb2[s], acc2[1], 0, 0, 0);
    __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);            // two LDS reads (step s + 2)
    __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);            // two MFMAs (step s)
  }
#pragma unroll
  for (int rr = 0; rr < 2; ++rr) {
    const int oyl = 2 * wv + rr;
    const f32x4 acc = acc2[rr];
    const int oy = oy0 + oyl;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int ox = ox0 + 4 * g + r;
      if (oy < oh && ox < ow) {
        float v = acc[r] + bias2_j;
        v = v > 0.f ? v : v * slope;
        out[(((long long)bi * oh + oy) * ow + ox) * 16 + j] = v;
      }
    }
  }
}

}  // namespace

extern "C" long long m4d_dinl_workspace_floats(int b, int C) {
  return dinl_partial_floats(b, C) + 2LL * b * C;
}

extern "C" int m4d_dinl_fwd(const float* x, const float* scale, const float* bias, int b, int h, int w, int C,
                            float slope, float* workspace, float* out, void* stream) {
  return m4d_dinl_fwd_padded(x, scale, bias, b, h, w, C, slope, workspace, out, h, w, 0, 0, stream);
}

extern "C" int m4d_dinl_fwd_padded(const float* x, const float* scale, const float* bias, int b, int h, int w, int C,
                                   float slope, float* workspace, float* out, int out_h, int out_w, int off_y,
                                   int off_x, void* stream) {
  M4D_CHECK_ARG(x && scale && bias && workspace && out && b > 0 && h > 0 && w > 0);
  M4D_CHECK_ARG(off_y >= 0 && off_x >= 0 && off_y + h <= out_h && off_x + w <= out_w);
  M4D_CHECK_ARG(C == 16 || C == 32);               // the reference applies DINL to encoder level 0 only (16 channels)
  M4D_CHECK_ARG(((((uintptr_t)x | (uintptr_t)out | (uintptr_t)workspace)) & 15u) == 0);
  hipStream_t s = (hipStream_t)stream;
  const int hw = h * w;
  const int ppi = 256 / (C / 4);
  int nblk = (hw + ppi * 8 - 1) / (ppi * 8);
  if (nblk > kDinlMaxBlocks) nblk = kDinlMaxBlocks;
  double* partial = reinterpret_cast<double*>(workspace);
  float* mean = workspace + dinl_partial_floats(b, C);
  float* var = mean + (long long)b * C;
  m4d_launch(dinl_partial_kernel, dim3(nblk, b), dim3(256), 0, s, x, (const float*)nullptr, hw, C, 0, partial);
  m4d_launch(dinl_finalize_kernel, dim3(b), dim3(256), 0, s, (const double*)partial, nblk, C, hw, mean);
  m4d_launch(dinl_partial_kernel, dim3(nblk, b), dim3(256), 0, s, x, (const float*)mean, hw, C, 1, partial);
  m4d_launch(dinl_finalize_kernel, dim3(b), dim3(256), 0, s, (const double*)partial, nblk, C, hw, var);
  int gx = m4d_blocks(hw, 256);
  if (gx > 2048) gx = 2048;
  if (C == 16) m4d_launch(dinl_apply_kernel<16>, dim3(gx, b), dim3(256), 0, s, x, mean, var, scale, bias, hw, w, slope, out, out_h, out_w, off_y, off_x);
  else m4d_launch(dinl_apply_kernel<32>, dim3(gx, b), dim3(256), 0, s, x, mean, var, scale, bias, hw, w, slope, out, out_h, out_w, off_y, off_x);
  return M4D_LAUNCH_RESULT();
}

extern "C" int m4d_enc_head_fwd(const float* images, int bsz, long long stride_b, long long stride_t,
                                const float* w_hwio, const float* bias, int b, int h, int w, int C,
                                float* workspace, float* raw_out, void* stream) {
  M4D_CHECK_ARG(images && w_hwio && bias && workspace && raw_out && b > 0 && h > 0 && w > 0);
  M4D_CHECK_ARG(C == 16);                            // encoder level 0 of the reference (m4depth_network.py:59)
  M4D_CHECK_ARG(bsz > 0 && b % bsz == 0 && stride_b >= 0 && stride_t >= 0);
  M4D_CHECK_ARG(((((uintptr_t)raw_out | (uintptr_t)workspace)) & 15u) == 0);
  hipStream_t s = (hipStream_t)stream;
  const int hw = h * w;
  int nblk = (hw + 256 * 8 - 1) / (256 * 8);       // (4x more, smaller workgroups: same kernel time, slower finalize)
  if (nblk > kDinlMaxBlocks) nblk = kDinlMaxBlocks;
  if (nblk < 1) nblk = 1;
  double* partial = reinterpret_cast<double*>(workspace);
  float* mean = workspace + dinl_partial_floats(b, C);
  float* var = mean + (long long)b * C;
  m4d_launch(enc_head_conv_kernel<16>, dim3(nblk, b), dim3(256), 0, s, images, w_hwio, bias, h, w, bsz, stride_b, stride_t,
                     raw_out, partial);
  m4d_launch(dinl_finalize_kernel, dim3(b), dim3(256), 0, s, (const double*)partial, nblk, C, hw, mean);
  const int ppi = 256 / (C / 4);
  int nblk2 = (hw + ppi * 8 - 1) / (ppi * 8);
  if (nblk2 > kDinlMaxBlocks) nblk2 = kDinlMaxBlocks;
  m4d_launch(dinl_partial_kernel, dim3(nblk2, b), dim3(256), 0, s, (const float*)raw_out, (const float*)mean, hw, C, 1, partial);
  m4d_launch(dinl_finalize_kernel, dim3(b), dim3(256), 0, s, (const double*)partial, nblk2, C, hw, var);
  return M4D_LAUNCH_RESULT();
}

// The statistics passes (mean, variance of conv1's output per image and channel) and the fused pass, as separate entry points:
// the statistics of EVERY frame of a sequence can then be taken in the first encoder batch's launches (m4d_enc_level0_stats over
// all frames), off the later batch's dependency chain.  m4d_enc_level0_fwd = the two on one batch.
extern "C" int m4d_enc_level0_stats(const float* images, int bsz, long long stride_b, long long stride_t,
                                    const float* w1_hwio, const float* bias1, int b, int h, int w, float* workspace,
                                    float* mean, float* var, void* stream) {
  M4D_CHECK_ARG(images && w1_hwio && bias1 && workspace && mean && var);
  M4D_CHECK_ARG(b > 0 && h > 0 && w > 0 && bsz > 0 && b % bsz == 0 && stride_b >= 0 && stride_t >= 0);
  M4D_CHECK_ARG((((uintptr_t)workspace) & 7u) == 0);
  hipStream_t s = (hipStream_t)stream;
  const int tiles_x = (w + kE0TW - 1) / kE0TW, n_tiles = tiles_x * ((h + kE0TH - 1) / kE0TH);
  double* partial = reinterpret_cast<double*>(workspace);
  // 32 doubles per block in the workspace of m4d_dinl_workspace_floats -> at most 256 blocks per image; BALANCED: every workgroup
  // the same number of tiles (384x1280: 480 tiles -> 240 workgroups of exactly two, not 224 of two + 32 of one)
  const int cap = kDinlMaxBlocks / 2, per = (n_tiles + cap - 1) / cap;
  const int nb2 = (n_tiles + per - 1) / per;
  m4d_launch(enc0_stats_kernel, dim3(nb2, b), dim3(256), 0, s, images, w1_hwio, bias1, (const float*)nullptr, h, w, bsz,
             stride_b, stride_t, tiles_x, n_tiles, partial);
  m4d_launch(enc0_moments_finalize_kernel, dim3(b), dim3(256), 0, s, images, (const double*)partial, nb2, w1_hwio, bias1, h, w, bsz,
             stride_b, stride_t, mean, var);
  return M4D_LAUNCH_RESULT();
}

extern "C" int m4d_enc_level0_apply(const float* images, int bsz, long long stride_b, long long stride_t,
                                    const float* w1_hwio, const float* bias1, const float* mean, const float* var,
                                    const float* dn_scale, const float* dn_bias, float dn_slope, const float* w2_hwio,
                                    const float* bias2, float slope, int b, int h, int w, float* out, void* stream) {
  M4D_CHECK_ARG(images && w1_hwio && bias1 && mean && var && dn_scale && dn_bias && w2_hwio && bias2 && out);
  M4D_CHECK_ARG(b > 0 && h > 0 && w > 0 && bsz > 0 && b % bsz == 0 && stride_b >= 0 && stride_t >= 0);
  const int oh = (h + 1) / 2, ow = (w + 1) / 2;
  const int ftx = (ow + kF0OW - 1) / kF0OW, fty = (oh + kF0OH - 1) / kF0OH;
  const int tot_y = (oh - 1) * 2 + 3 - h, tot_x = (ow - 1) * 2 + 3 - w;                 // TF 'SAME' total padding
  const int pad_y = (tot_y > 0 ? tot_y : 0) / 2, pad_x = (tot_x > 0 ? tot_x : 0) / 2;
  m4d_launch(enc0_fused_kernel, dim3(ftx * fty, b), dim3(256), 0, (hipStream_t)stream, images, w1_hwio, bias1, mean,
                     var, dn_scale, dn_bias, dn_slope, w2_hwio, bias2, slope, h, w, oh, ow, pad_y, pad_x, bsz, stride_b,
                     stride_t, ftx, out);
  return M4D_LAUNCH_RESULT();
}

extern "C" int m4d_enc_level0_fwd(const float* images, int bsz, long long stride_b, long long stride_t,
                                   const float* w1_hwio, const float* bias1, const float* dn_scale, const float* dn_bias,
                                   float dn_slope, const float* w2_hwio, const float* bias2, float slope,
                                   int b, int h, int w, float* workspace, float* out, void* stream) {
  M4D_CHECK_ARG(workspace && b > 0);
  float* mean = workspace + dinl_partial_floats(b, 16);
  float* var = mean + (long long)b * 16;
  const int rc = m4d_enc_level0_stats(images, bsz, stride_b, stride_t, w1_hwio, bias1, b, h, w, workspace, mean, var, stream);
  if (rc != 0) return rc;
  return m4d_enc_level0_apply(images, bsz, stride_b, stride_t, w1_hwio, bias1, mean, var, dn_scale, dn_bias, dn_slope, w2_hwio,
                              bias2, slope, b, h, w, out, stream);
}

extern "C" long long m4d_metrics_workspace_bytes(void) { return (long long)kMetricBlocks * kMetricSums * sizeof(double); }

extern "C" int m4d_depth_metrics_strided(const float* gt, long long per_image, long long gt_image_stride, const float* est,
                                         long long n, float max_d, void* workspace, float* out7, float* total7, float count,
                                         float* mean7, void* stream) {
  M4D_CHECK_ARG(gt && est && workspace && out7 && n > 0 && per_image > 0 && gt_image_stride >= per_image && n % per_image == 0);
  M4D_CHECK_ARG(!mean7 || (total7 && count > 0.f));
  hipStream_t s = (hipStream_t)stream;
  long long g = (n + 255) / 256;
  const int nblk = (int)(g < kMetricBlocks ? g : kMetricBlocks);
  m4d_launch(metrics_partial_kernel, dim3(nblk), dim3(256), 0, s, gt, est, n, max_d, (double*)workspace, per_image, gt_image_stride);
  m4d_launch(metrics_finalize_kernel, dim3(1), dim3(kMetricSums * 32), 0, s, (const double*)workspace, nblk, out7, total7, count, mean7);
  return M4D_LAUNCH_RESULT();
}

extern "C" int m4d_depth_metrics(const float* gt, const float* est, long long n, float max_d, void* workspace,
                                 float* out7, float* total7, float count, float* mean7, void* stream) {
  return m4d_depth_metrics_strided(gt, n, n, est, n, max_d, workspace, out7, total7, count, mean7, stream);
}

extern "C" long long m4d_metrics_per_sample_workspace_bytes(int b) {
  return b > 0 ? (long long)b * kMetricBlocks * kMetricSums * sizeof(double) : 0;
}

extern "C" int m4d_depth_metrics_per_sample(const float* gt, long long gt_stride, const float* est, long long est_stride,
                                            int b, long long per_image, float max_d, const unsigned char* new_traj,
                                            const unsigned char* active, void* workspace, float* rows, unsigned char* counted,
                                            void* stream) {
  M4D_CHECK_ARG(gt && est && new_traj && active && workspace && rows && counted);
  M4D_CHECK_ARG(b > 0 && b <= 65535 && per_image > 0 && gt_stride >= per_image && est_stride >= per_image);
  hipStream_t s = (hipStream_t)stream;
  long long g = (per_image + 255) / 256;
  const int nblk = (int)(g < kMetricBlocks ? g : kMetricBlocks);              // the partition of m4d_depth_metrics(n = per_image)
  m4d_launch(metrics_partial_ps_kernel, dim3(nblk, b), dim3(256), 0, s, gt, gt_stride, est, est_stride, per_image, max_d,
             (double*)workspace);
  m4d_launch(metrics_finalize_ps_kernel, dim3(b), dim3(kMetricSums * 32), 0, s, (const double*)workspace, nblk, new_traj, active,
             rows, counted);
  return M4D_LAUNCH_RESULT();
}
