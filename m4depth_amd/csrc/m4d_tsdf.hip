// TSDF surface meshes: the depth estimates of a trajectory fused into a truncated signed distance field on a hashed voxel grid
// (Curless & Levoy 1996; Niessner et al. 2013) and a naive-surface-nets extraction, on the device
// (include/m4depth_hip.h: m4d_tsdf_allocate, m4d_tsdf_integrate, m4d_tsdf_extract_vertices, m4d_tsdf_extract_faces, m4d_tsdf_clear).
//
// State: per sample four statistics words, then -- structure of arrays -- the keys of a hashed voxel grid (m4d_voxel_hash.h, the
// voxel map's table) and the 24-byte records behind them.  The per-frame pass over the table streams the keys only and touches
// the records of the voxels the frame sees.
//   allocate : one thread per pixel walks its ray over the truncation band and claims the keys (agent-scope load + compare-and-
//              swap); a claim writes the key only.  The SET of keys does not depend on the schedule.
//   integrate: every slot has one thread; the owner of a record is the only thread that touches it, so the float32 sum S is the
//              same for every schedule.  The only atomic is one add per workgroup on the `updates` statistic.
//   extract  : one thread per slot looks its neighbours up with a read-only probe; records leave through a wave ballot and one
//              atomic add per wave on a count word.  The host orders them.
//   raycast  : one thread per pixel marches its ray through the field, coarse to fine, with the read-only probe, and writes the
//              depth of the first front-face zero crossing (m4d_tsdf_raycast): the volume rendered back into a frame.
//   render   : the raycast with a trilinear sample of the field and, at the hit, the interpolant's gradient as a normal, the
//              blended colour and a shaded RGB8 picture (m4d_tsdf_render).
#include "m4d_voxel_hash.h"
#include "../../include/m4depth_hip.h"

namespace {

constexpr int kChunk = 256;
constexpr int kStats = 4;                                     // occupied, dropped_range, dropped_full, updates
constexpr int kRecWords = 3;                                  // 24 bytes: float S, uint32 n, sr, sg, sb, nc
constexpr long long kMaxPixels = 1LL << 24;
constexpr unsigned kIntegrateBlocks = 1024;                  // workgroups per sample of the integrate pass, at most

struct TsdfRec { float S; unsigned n, sr, sg, sb, nc; };
static_assert(sizeof(TsdfRec) == 24, "record layout");

__device__ __forceinline__ u64* ts_keys(u64* state, int b, int s, int log2_slots) {
  return state + (long long)b * kStats + ((long long)s << log2_slots);
}
__device__ __forceinline__ TsdfRec* ts_recs(u64* state, int b, int s, int log2_slots) {
  return (TsdfRec*)(state + (long long)b * kStats + ((long long)b << log2_slots)) + ((long long)s << log2_slots);
}

__device__ __forceinline__ bool ts_pose_finite(const double* p) {
  bool ok = true;
#pragma unroll
  for (int i = 0; i < 7; ++i) ok = ok && isfinite(p[i]);
  return ok;
}

__device__ __forceinline__ bool ts_cell(double x, double voxel, unsigned& cell) { return vh_cell_of(floor(x / voxel), cell); }

__device__ __forceinline__ unsigned ts_byte(float v) {        // m4d_depth_export's rgb rule; fmaxf(NaN, 0) = 0
  return (unsigned)rintf(fminf(fmaxf(v, 0.0f), 1.0f) * 255.0f);
}

struct FrameArgs {
  const float* depth; long long depth_stride;
  const float* rgb; long long rgb_stride;
  const float* cam_f; const float* cam_c; const double* pose;
  int h, w, trunc;
  float near, far, voxel;
};

// kSkip: a thread does not probe again for the key it has just claimed (consecutive samples of a ray often share a voxel)
template <bool kSkip>
__global__ void __launch_bounds__(kChunk)
tsdf_allocate_kernel(FrameArgs a, u64* __restrict__ state, int b, int log2_slots) {
  __shared__ unsigned s_range[kChunk / 64], s_full[kChunk / 64];
  const int s = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long px = (long long)blockIdx.x * kChunk + threadIdx.x;
  const double* p = a.pose + s * 7;
  if (!ts_pose_finite(p)) return;                              // the whole workgroup: s is its sample
  float d = 0.0f;
  bool active = px < (long long)a.h * a.w;
  if (active) {
    d = a.depth[s * a.depth_stride + px];
    active = isfinite(d) && d >= a.near && d <= a.far;
  }
  const int row = (int)(px / a.w), col = (int)(px % a.w);
  const float fx = a.cam_f[s * 2], fy = a.cam_f[s * 2 + 1], cx = a.cam_c[s * 2], cy = a.cam_c[s * 2 + 1];
  const double ax = (double)((((float)col + 0.5f) - cx) / fx), ay = (double)((((float)row + 0.5f) - cy) / fy);
  double r[9];
  m4d_rot64(p, r);
  const double voxel = (double)a.voxel, hv = voxel * 0.5;
  u64* stats = state + (long long)s * kStats;
  u64* keys = ts_keys(state, b, s, log2_slots);
  u64 last = kEmpty;
  unsigned n_range = 0, n_full = 0;
  for (int k = -2 * a.trunc; active && k <= 2 * a.trunc; ++k) {
    const double z = (double)d + (double)k * hv;
    if (!(z > 0.0)) continue;
    const double X = ax * z, Y = ay * z;
    const double wx = ((r[0] * X + r[1] * Y) + r[2] * z) + p[4];
    const double wy = ((r[3] * X + r[4] * Y) + r[5] * z) + p[5];
    const double wz = ((r[6] * X + r[7] * Y) + r[8] * z) + p[6];
    unsigned ix, iy, iz;
    if (!(ts_cell(wx, voxel, ix) && ts_cell(wy, voxel, iy) && ts_cell(wz, voxel, iz))) { ++n_range; continue; }
    const u64 key = vh_pack(ix, iy, iz);
    if (kSkip && key == last) continue;
    if (vh_claim<1>(keys, key, log2_slots, stats + 0)) last = key; else ++n_full;
  }
  // the drop counters of a workgroup leave as one add each (a full table drops every sample of every ray)
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) { n_range += __shfl_down(n_range, off, 64); n_full += __shfl_down(n_full, off, 64); }
  if (lane == 0) { s_range[wave] = n_range; s_full[wave] = n_full; }
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned range = 0, full = 0;
#pragma unroll
    for (int i = 0; i < kChunk / 64; ++i) { range += s_range[i]; full += s_full[i]; }
    if (range) VH_ADD(stats + 1, range);
    if (full) VH_ADD(stats + 2, full);
  }
}

// A workgroup walks the slots blockIdx.x * kChunk + threadIdx.x + i * gridDim.x * kChunk: consecutive lanes read consecutive keys,
// the sample's rotation is formed once per thread, and the records a workgroup updated are summed through LDS into ONE atomic
// add on the sample's `updates` word (one add per wave made the launch wait on that single address: 65 536 of them, 0.8 ms).
__global__ void __launch_bounds__(kChunk)
tsdf_integrate_kernel(FrameArgs a, u64* __restrict__ state, int b, int log2_slots) {
  __shared__ unsigned s_upd[kChunk / 64];
  const int s = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const double* p = a.pose + s * 7;
  if (!ts_pose_finite(p)) return;                              // the whole workgroup: s is its sample
  double r[9];
  m4d_rot64(p, r);
  const double voxel = (double)a.voxel;
  const float T = (float)((double)a.trunc * voxel);
  const double fx = (double)a.cam_f[s * 2], fy = (double)a.cam_f[s * 2 + 1];
  const double cx = (double)a.cam_c[s * 2], cy = (double)a.cam_c[s * 2 + 1];
  const double t0 = p[4], t1 = p[5], t2 = p[6];
  const u64* keys = ts_keys(state, b, s, log2_slots);
  TsdfRec* recs = ts_recs(state, b, s, log2_slots);
  const long long slots = 1ll << log2_slots, stride = (long long)gridDim.x * kChunk;
  unsigned updated = 0;
  for (long long slot = (long long)blockIdx.x * kChunk + threadIdx.x; slot < slots; slot += stride) {
    const u64 key = keys[slot];
    if (key == kEmpty) continue;
    const double D0 = ((double)vh_cell(key, 0) + 0.5) * voxel - t0;
    const double D1 = ((double)vh_cell(key, 1) + 0.5) * voxel - t1;
    const double D2 = ((double)vh_cell(key, 2) + 0.5) * voxel - t2;
    const double X0 = (r[0] * D0 + r[3] * D1) + r[6] * D2;                      // R^T (centre - t)
    const double X1 = (r[1] * D0 + r[4] * D1) + r[7] * D2;
    const double z = (r[2] * D0 + r[5] * D1) + r[8] * D2;
    if (!(z > 0.0)) continue;
    const double u = (fx * X0) / z + cx, v = (fy * X1) / z + cy;
    if (!(u >= 0.0 && u < (double)a.w && v >= 0.0 && v < (double)a.h)) continue;      // NaN fails
    const int col = (int)floor(u), row = (int)floor(v);
    const long long px = (long long)row * a.w + col;
    const float d = a.depth[s * a.depth_stride + px];
    if (!(isfinite(d) && d >= a.near && d <= a.far)) continue;
    const float sdf = (float)((double)d - z);
    if (!(sdf >= -T)) continue;
    TsdfRec* rec = recs + slot;
    rec->S = rec->S + fminf(sdf, T) / T;
    rec->n = rec->n + 1u;
    if (sdf <= T) {
      const float* c = a.rgb + s * a.rgb_stride + px * 3;
      rec->sr += ts_byte(c[0]); rec->sg += ts_byte(c[1]); rec->sb += ts_byte(c[2]);
      rec->nc += 1u;
    }
    ++updated;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) updated += __shfl_down(updated, off, 64);
  if (lane == 0) s_upd[wave] = updated;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned all = 0;
#pragma unroll
    for (int i = 0; i < kChunk / 64; ++i) all += s_upd[i];
    if (all) VH_ADD(state + (long long)s * kStats + 3, all);
  }
}

__global__ void __launch_bounds__(kChunk)
tsdf_vertices_kernel(const u64* __restrict__ keys, const TsdfRec* __restrict__ recs, int log2_slots, unsigned min_frames,
                     float voxel_f, u64* __restrict__ keys_out, uint4* __restrict__ vertices_out, long long out_cap,
                     u64* __restrict__ count) {
  const long long slot = (long long)blockIdx.x * kChunk + threadIdx.x;
  bool keep = false;
  u64 key = kEmpty;
  float D[8];
  u64 sr = 0, sg = 0, sb = 0, nc = 0;
  unsigned n_min = 0xFFFFFFFFu;
  if (slot < (1ll << log2_slots)) {
    key = keys[slot];
    if (key != kEmpty) {
      const unsigned cx = vh_biased(key, 0), cy = vh_biased(key, 1), cz = vh_biased(key, 2);
      bool valid = cx < kCellMax && cy < kCellMax && cz < kCellMax;
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        D[c] = 0.0f;
        if (!valid) continue;
        long long at = slot;
        if (c) {
          const u64 other = vh_pack(cx + (c & 1), cy + ((c >> 1) & 1), cz + ((c >> 2) & 1));
          at = vh_find(keys, other, log2_slots);
        }
        if (at < 0) { valid = false; continue; }
        const TsdfRec r = recs[at];
        if (r.n < min_frames || r.n == 0u) { valid = false; continue; }
        D[c] = r.S / (float)r.n;
        sr += r.sr; sg += r.sg; sb += r.sb; nc += r.nc;
        n_min = r.n < n_min ? r.n : n_min;
      }
      if (valid) {
        int inside = 0;
#pragma unroll
        for (int c = 0; c < 8; ++c) inside += D[c] < 0.0f ? 1 : 0;
        keep = inside > 0 && inside < 8;
      }
    }
  }
  const long long at = vh_place(keep, count);
  if (at < 0 || at >= out_cap) return;
  float sum[3] = {0.0f, 0.0f, 0.0f};
  int crossings = 0;
#pragma unroll
  for (int axis = 0; axis < 3; ++axis) {
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      if (c & (1 << axis)) continue;
      const float Da = D[c], Db = D[c | (1 << axis)];
      if ((Da < 0.0f) == (Db < 0.0f)) continue;
      const float t = Da / (Da - Db);
#pragma unroll
      for (int i = 0; i < 3; ++i) sum[i] = sum[i] + (i == axis ? t : (float)((c >> i) & 1));
      ++crossings;
    }
  }
  const double voxel = (double)voxel_f;
  float pos[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const float local = sum[i] / (float)crossings;
    pos[i] = (float)((((double)vh_cell(key, i) + 0.5) + (double)local) * voxel);
  }
  unsigned r = 0, g = 0, bl = 0;
  if (nc) { r = (unsigned)((2 * sr + nc) / (2 * nc)); g = (unsigned)((2 * sg + nc) / (2 * nc)); bl = (unsigned)((2 * sb + nc) / (2 * nc)); }
  const unsigned alpha = n_min > 255u ? 255u : n_min;
  keys_out[at] = key;
  vertices_out[at] = make_uint4(__float_as_uint(pos[0]), __float_as_uint(pos[1]), __float_as_uint(pos[2]),
                                r | (g << 8) | (bl << 16) | (alpha << 24));
}

__global__ void __launch_bounds__(kChunk)
tsdf_faces_kernel(const u64* __restrict__ keys, const TsdfRec* __restrict__ recs, int log2_slots, unsigned min_frames,
                  u64* __restrict__ quads_out, long long out_cap, u64* __restrict__ count) {
  const long long slot = (long long)blockIdx.x * kChunk + threadIdx.x;
  u64 key = kEmpty;
  bool valid = false, in_k = false;
  unsigned cell[3] = {0, 0, 0};
  if (slot < (1ll << log2_slots)) {
    key = keys[slot];
    if (key != kEmpty) {
      const TsdfRec r = recs[slot];
      valid = r.n >= min_frames && r.n > 0u;
      if (valid) in_k = r.S / (float)r.n < 0.0f;
      cell[0] = vh_biased(key, 0); cell[1] = vh_biased(key, 1); cell[2] = vh_biased(key, 2);
    }
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) {                                // no early return: every lane takes part in the three ballots
    const int bx = (a + 1) % 3, cx = (a + 2) % 3;
    const u64 ea = 1ull << (42 - 21 * a), eb = 1ull << (42 - 21 * bx), ec = 1ull << (42 - 21 * cx);
    bool emit = false;
    if (valid && cell[a] < kCellMax && cell[bx] >= 1u && cell[cx] >= 1u) {
      const long long at = vh_find(keys, key + ea, log2_slots);
      if (at >= 0) {
        const TsdfRec r = recs[at];
        if (r.n >= min_frames && r.n > 0u) emit = (r.S / (float)r.n < 0.0f) != in_k;
      }
    }
    const long long at = vh_place(emit, count);
    if (at < 0 || at >= out_cap) continue;
    u64* q = quads_out + at * 5;
    const u64 c0 = key, c1 = key - eb, c2 = key - eb - ec, c3 = key - ec;
    q[0] = (u64)a | (in_k ? 0ull : 4ull);
    if (in_k) { q[1] = c0; q[2] = c1; q[3] = c2; q[4] = c3; }
    else      { q[1] = c3; q[2] = c2; q[3] = c1; q[4] = c0; }
  }
}

__global__ void __launch_bounds__(kChunk)
tsdf_clear_kernel(u64* __restrict__ state, const unsigned char* __restrict__ mask, int b, int log2_slots) {
  const int s = blockIdx.y;
  if (mask && !mask[s]) return;
  const long long slots = 1ll << log2_slots;
  u64* keys = ts_keys(state, b, s, log2_slots);
  u64* recs = (u64*)ts_recs(state, b, s, log2_slots);
  const long long stride = (long long)gridDim.x * kChunk;
  for (long long i = (long long)blockIdx.x * kChunk + threadIdx.x; i < slots; i += stride) {
    keys[i] = kEmpty;
    recs[i * kRecWords] = 0ull; recs[i * kRecWords + 1] = 0ull; recs[i * kRecWords + 2] = 0ull;
  }
  if (blockIdx.x == 0 && threadIdx.x < kStats) state[(long long)s * kStats + threadIdx.x] = 0ull;
}

struct RayArgs {
  const float* cam_f; const float* cam_c; const double* pose;
  const float* guide; long long guide_stride;
  const float* fill; long long fill_stride;
  float* out; long long out_stride;
  u64* hits;
  int h, w, trunc, window;
  unsigned min_frames;
  float near, far, voxel;
};

// One thread per pixel marches its ray through the volume: the state is only read.  Per sample of the ray: three float64
// divisions for the cell, one dependent 8-byte key load per probe trip, then the first 8 bytes (S, n) of the 24-byte record.
// kTile : a wave is an 8x8 pixel tile (a workgroup 16x16) instead of 64 consecutive pixels of the raster: neighbouring rays end at
//         similar depths, so the trip counts of a wave agree more.
// kReuse: a sample whose key equals the previous sample's takes that sample's answer without a probe (half-voxel steps share
//         voxels, and the fine walk starts on the coarse sample it backed up from).
template <bool kTile, bool kReuse>
__global__ void __launch_bounds__(kChunk)
tsdf_raycast_kernel(RayArgs a, const u64* __restrict__ state, int b, int log2_slots) {
  __shared__ unsigned s_hits[kChunk / 64];
  const int s = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int row, col;
  if (kTile) {
    const int tiles_x = (a.w + 15) >> 4;
    row = (int)(blockIdx.x / tiles_x) * 16 + (wave >> 1) * 8 + (lane >> 3);
    col = (int)(blockIdx.x % tiles_x) * 16 + (wave & 1) * 8 + (lane & 7);
  } else {
    const long long at = (long long)blockIdx.x * kChunk + threadIdx.x;
    row = (int)(at / a.w); col = (int)(at % a.w);
  }
  const bool active = row < a.h && col < a.w;
  const long long px = (long long)row * a.w + col;
  const float miss = active && a.fill ? a.fill[s * a.fill_stride + px] : __uint_as_float(0x7FC00000u);
  const double* p = a.pose + s * 7;
  if (!ts_pose_finite(p)) {                                    // the whole workgroup: s is its sample
    if (active) a.out[s * a.out_stride + px] = miss;
    return;
  }
  bool hit = false;
  float result = miss;
  if (active) {
    const float fx = a.cam_f[s * 2], fy = a.cam_f[s * 2 + 1], cx = a.cam_c[s * 2], cy = a.cam_c[s * 2 + 1];
    const double ax = (double)((((float)col + 0.5f) - cx) / fx), ay = (double)((((float)row + 0.5f) - cy) / fy);
    double r[9];
    m4d_rot64(p, r);
    const double voxel = (double)a.voxel, hv = voxel * 0.5;
    const int K2 = 2 * a.trunc;
    double z_lo = (double)a.near, z_hi = (double)a.far;
    if (a.guide) {
      const float g = a.guide[s * a.guide_stride + px];
      if (isfinite(g) && g >= a.near && g <= a.far) {
        const double Wd = ((double)a.window * (double)a.trunc) * voxel;
        z_lo = fmax((double)a.near, (double)g - Wd);
        z_hi = fmin((double)a.far, (double)g + Wd);
      }
    }
    const long long n_max = (long long)floor((z_hi - z_lo) / hv);
    const u64* keys = state + (long long)b * kStats + ((long long)s << log2_slots);
    const TsdfRec* recs = (const TsdfRec*)(state + (long long)b * kStats + ((long long)b << log2_slots)) + ((long long)s << log2_slots);
    long long i = 0;
    int run = 0;
    bool fine = false, have_prev = false, last_known = false;
    float prev = 0.0f, last_D = 0.0f;
    u64 last = kEmpty;
    for (long long trip = 0; trip < 2 * (n_max + 1) && i <= n_max; ++trip) {   // every position: once coarse, once fine, at most
      const double z = z_lo + (double)i * hv;
      const double X = ax * z, Y = ay * z;
      const double wx = ((r[0] * X + r[1] * Y) + r[2] * z) + p[4];
      const double wy = ((r[3] * X + r[4] * Y) + r[5] * z) + p[5];
      const double wz = ((r[6] * X + r[7] * Y) + r[8] * z) + p[6];
      unsigned ix, iy, iz;
      bool known = false;
      float D = 0.0f;
      if (ts_cell(wx, voxel, ix) && ts_cell(wy, voxel, iy) && ts_cell(wz, voxel, iz)) {
        const u64 key = vh_pack(ix, iy, iz);
        if (kReuse && key == last) {
          known = last_known; D = last_D;
        } else {
          const long long at = vh_find(keys, key, log2_slots);
          if (at >= 0) {
            const uint2 sn = *(const uint2*)(recs + at);       // S and n: the first 8 of the record's 24 bytes
            if (sn.y >= a.min_frames && sn.y > 0u) { known = true; D = __uint_as_float(sn.x) / (float)sn.y; }
          }
          last = key; last_known = known; last_D = D;
        }
      }
      if (!fine) {
        if (!known) { i += K2; continue; }
        i = i == 0 ? 0 : i - K2 + 1;                           // just after the last unknown coarse position
        fine = true; run = 0; have_prev = false;
        continue;
      }
      if (!known) {
        have_prev = false;
        if (++run == K2) { fine = false; i += K2; } else { i += 1; }
        continue;
      }
      run = 0;
      if (have_prev && prev >= 0.0f && D < 0.0f) {
        const double z_prev = z_lo + (double)(i - 1) * hv;
        result = (float)(z_prev + hv * (double)(prev / (prev - D)));
        hit = true;
        break;
      }
      prev = D; have_prev = true; i += 1;
    }
    a.out[s * a.out_stride + px] = result;
  }
  if (!a.hits) return;                                         // uniform
  unsigned n_hit = hit ? 1u : 0u;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) n_hit += __shfl_down(n_hit, off, 64);
  if (lane == 0) s_hits[wave] = n_hit;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned all = 0;
#pragma unroll
    for (int i = 0; i < kChunk / 64; ++i) all += s_hits[i];
    if (all) VH_ADD(a.hits + s, all);
  }
}

// the refusals of m4d_tsdf_raycast, which m4d_tsdf_render shares, and the launch's arguments
inline int ts_ray_args(const void* state, int b, int log2_slots, const float* cam_f, const float* cam_c, const double* pose, int h,
                       int w, float near, float far, float voxel, int trunc, int min_frames, const float* guide,
                       long long guide_stride, int window, const float* fill, long long fill_stride, float* depth_out,
                       long long out_stride, void* hits, RayArgs& a) {
  M4D_CHECK_ARG(state && cam_f && cam_c && pose && depth_out);
  M4D_CHECK_ARG(vh_geometry(b, log2_slots) && h >= 1 && w >= 1 && (long long)h * w <= kMaxPixels);
  M4D_CHECK_ARG(far > near && near > 0.0f && voxel > 0.0f && voxel < __builtin_inff() && trunc >= 2 && trunc <= 8);
  M4D_CHECK_ARG(min_frames >= 1 && (!guide || window >= 1));
  M4D_CHECK_ARG(((double)far - (double)near) / ((double)voxel * 0.5) <= 1048576.0);      // the march's constant bound
  const long long image = (long long)h * w;
  M4D_CHECK_ARG(out_stride >= image && (!guide || guide_stride >= image) && (!fill || fill_stride >= image));
  M4D_CHECK_ARG(((((uintptr_t)cam_f) | ((uintptr_t)cam_c) | ((uintptr_t)guide) | ((uintptr_t)fill) | ((uintptr_t)depth_out)) & 3u) == 0);
  M4D_CHECK_ARG(((((uintptr_t)state) | ((uintptr_t)pose) | ((uintptr_t)hits)) & 7u) == 0);
  a = {cam_f, cam_c, pose, guide, guide_stride, fill, fill_stride, depth_out, out_stride, (u64*)hits,
       h, w, trunc, guide ? window : 0, (unsigned)min_frames, near, far, voxel};
  return 0;
}

template <bool kTile, bool kReuse>
int ts_raycast(const void* state, int b, int log2_slots, const float* cam_f, const float* cam_c, const double* pose, int h, int w,
               float near, float far, float voxel, int trunc, int min_frames, const float* guide, long long guide_stride,
               int window, const float* fill, long long fill_stride, float* depth_out, long long out_stride, void* hits,
               void* stream) {
  RayArgs a;
  if (int e = ts_ray_args(state, b, log2_slots, cam_f, cam_c, pose, h, w, near, far, voxel, trunc, min_frames, guide, guide_stride,
                          window, fill, fill_stride, depth_out, out_stride, hits, a)) return e;
  const long long image = (long long)h * w;
  const long long groups = kTile ? (long long)((w + 15) / 16) * ((h + 15) / 16) : (image + kChunk - 1) / kChunk;
  m4d_launch(tsdf_raycast_kernel<kTile, kReuse>, dim3((unsigned)groups, (unsigned)b), dim3(kChunk), 0, (hipStream_t)stream, a,
             (const u64*)state, b, log2_slots);
  return M4D_LAUNCH_RESULT();
}

// ---- m4d_tsdf_render: the raycast with a trilinear sample and, at the hit, the normal and the colour -------------------------------

struct RenderArgs {
  RayArgs ray;
  float* normal; long long normal_stride;
  float* colour; long long colour_stride;
  unsigned char* view; long long view_stride;
};

__device__ __forceinline__ float ts_lerp(float a, float b, float t) { return a + t * (b - a); }

__device__ __forceinline__ float ts_tri(const float* v, const float* fr) {         // x, then y, then z
  const float x00 = ts_lerp(v[0], v[1], fr[0]), x10 = ts_lerp(v[2], v[3], fr[0]);
  const float x01 = ts_lerp(v[4], v[5], fr[0]), x11 = ts_lerp(v[6], v[7], fr[0]);
  return ts_lerp(ts_lerp(x00, x10, fr[1]), ts_lerp(x01, x11, fr[1]), fr[2]);
}

// the rest of vh_find's sequence after a first slot that held another key: trips 1 .. kProbe - 1
__device__ __forceinline__ long long ts_find_on(const u64* __restrict__ keys, u64 key, int log2_slots, u64 first) {
  const u64 slots = 1ull << log2_slots;
  u64 slot = (first + 1) & (slots - 1);
  for (int i = 1; i < kProbe; ++i) {
    const u64 cur = keys[slot];
    if (cur == key) return (long long)slot;
    if (cur == kEmpty) return -1;
    slot = (slot + 1) & (slots - 1);
  }
  return -1;
}

// The eight corners of the base cell `base` (a packed key whose three indices are below kCellMax: no carry): v[c] = S / n of the
// KNOWN ones, at[c] their slots (-1: no key); returns the mask of the KNOWN corners.
// kTogether: the eight first-slot key loads are issued together, then the eight (S, n) loads -- eight independent reads pay one
//            memory latency where eight probes back to back pay sixteen; only a corner whose first slot holds another key walks on.
template <bool kTogether>
__device__ __forceinline__ unsigned ts_corners(const u64* __restrict__ keys, const TsdfRec* __restrict__ recs, u64 base,
                                               int log2_slots, unsigned min_frames, float* v, long long* at) {
  uint2 sn[8];
  if (kTogether) {
    u64 key[8], slot[8], cur[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      key[c] = base + ((u64)(c & 1) << 42) + ((u64)((c >> 1) & 1) << 21) + (u64)(c >> 2);
      slot[c] = vh_slot_of(key[c], log2_slots);
    }
#pragma unroll
    for (int c = 0; c < 8; ++c) cur[c] = keys[slot[c]];
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      at[c] = cur[c] == key[c] ? (long long)slot[c] : -1;
      if (cur[c] != key[c] && cur[c] != kEmpty) at[c] = ts_find_on(keys, key[c], log2_slots, slot[c]);
    }
#pragma unroll
    for (int c = 0; c < 8; ++c) sn[c] = *(const uint2*)(recs + (at[c] < 0 ? 0 : at[c]));   // slot 0 exists: no branch around a load
  } else {
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const u64 key = base + ((u64)(c & 1) << 42) + ((u64)((c >> 1) & 1) << 21) + (u64)(c >> 2);
      at[c] = vh_find(keys, key, log2_slots);
      sn[c] = make_uint2(0u, 0u);
      if (at[c] >= 0) sn[c] = *(const uint2*)(recs + at[c]);
    }
  }
  unsigned mask = 0;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const bool known = at[c] >= 0 && sn[c].y >= min_frames && sn[c].y > 0u;
    v[c] = known ? __uint_as_float(sn[c].x) / (float)sn[c].y : 0.0f;
    mask |= known ? 1u << c : 0u;
  }
  return mask;
}

// g = q - 0.5 per axis -> the base cell as a packed key and the fractions; false when a corner would leave [-2^20, 2^20)
__device__ __forceinline__ bool ts_base(const double* q, u64& base, float* fr) {
  double fl[3];
  bool ok = true;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const double g = q[j] - 0.5;
    fl[j] = floor(g);
    fr[j] = (float)(g - fl[j]);
    ok = ok && fl[j] >= -(double)kHalf && fl[j] <= (double)(kHalf - 2);            // NaN fails
  }
  if (ok) base = vh_pack((unsigned)((int)fl[0] + kHalf), (unsigned)((int)fl[1] + kHalf), (unsigned)((int)fl[2] + kHalf));
  return ok;
}

// which corner of the base cell the nearest voxel floor(q) is
__device__ __forceinline__ int ts_nearest_corner(const double* q, u64 base) {
  int idx = 0;
#pragma unroll
  for (int j = 0; j < 3; ++j) idx |= ((int)floor(q[j]) + kHalf != (int)vh_biased(base, j) ? 1 : 0) << j;
  return idx;
}

__device__ __forceinline__ void ts_mean_colour(const TsdfRec* rec, float* m, bool& have) {
  const uint2* words = (const uint2*)rec;                      // sr sg | sb nc: the 16 bytes behind S and n
  const uint2 a = words[1], b = words[2];
  have = b.y > 0u;
  m[0] = ((float)a.x / (float)b.y) / 255.0f; m[1] = ((float)a.y / (float)b.y) / 255.0f; m[2] = ((float)b.x / (float)b.y) / 255.0f;
}

// kInterp  : fine-mode samples blend the eight voxels around them (never the coarse ones: they only look for known space)
// kTogether: ts_corners' form
// kKeep    : the corners stay in registers while the base cell does not change (half-voxel steps mostly stay in one)
template <bool kInterp, bool kTogether, bool kKeep>
__global__ void __launch_bounds__(kChunk)
tsdf_render_kernel(RenderArgs ra, const u64* __restrict__ state, int b, int log2_slots) {
  __shared__ unsigned s_hits[kChunk / 64];
  const RayArgs& a = ra.ray;
  const int s = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int tiles_x = (a.w + 15) >> 4;
  const int row = (int)(blockIdx.x / tiles_x) * 16 + (wave >> 1) * 8 + (lane >> 3);
  const int col = (int)(blockIdx.x % tiles_x) * 16 + (wave & 1) * 8 + (lane & 7);
  const bool active = row < a.h && col < a.w;
  const long long px = (long long)row * a.w + col;
  const float nan32 = __uint_as_float(0x7FC00000u);
  const float miss = active && a.fill ? a.fill[s * a.fill_stride + px] : nan32;
  const double* p = a.pose + s * 7;
  const bool extra = ra.normal || ra.colour || ra.view;       // uniform
  bool hit = false;
  float result = miss;
  float nrm[3] = {nan32, nan32, nan32}, colr[3] = {nan32, nan32, nan32};
  unsigned pix[3] = {0u, 0u, 0u};
  if (active && ts_pose_finite(p)) {                           // the pose: the whole workgroup's, s is its sample
    const float fx = a.cam_f[s * 2], fy = a.cam_f[s * 2 + 1], cx = a.cam_c[s * 2], cy = a.cam_c[s * 2 + 1];
    const double ax = (double)((((float)col + 0.5f) - cx) / fx), ay = (double)((((float)row + 0.5f) - cy) / fy);
    double r[9];
    m4d_rot64(p, r);
    const double voxel = (double)a.voxel, hv = voxel * 0.5;
    const int K2 = 2 * a.trunc;
    double z_lo = (double)a.near, z_hi = (double)a.far;
    if (a.guide) {
      const float g = a.guide[s * a.guide_stride + px];
      if (isfinite(g) && g >= a.near && g <= a.far) {
        const double Wd = ((double)a.window * (double)a.trunc) * voxel;
        z_lo = fmax((double)a.near, (double)g - Wd);
        z_hi = fmin((double)a.far, (double)g + Wd);
      }
    }
    const long long n_max = (long long)floor((z_hi - z_lo) / hv);
    const u64* keys = state + (long long)b * kStats + ((long long)s << log2_slots);
    const TsdfRec* recs = (const TsdfRec*)(state + (long long)b * kStats + ((long long)b << log2_slots)) + ((long long)s << log2_slots);
    long long i = 0;
    int run = 0;
    bool fine = false, have_prev = false, last_known = false;
    float prev = 0.0f, last_D = 0.0f;
    u64 last = kEmpty, kept = kEmpty;
    float v[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    unsigned mask = 0;
    double z_star = 0.0;
    for (long long trip = 0; trip < 2 * (n_max + 1) && i <= n_max; ++trip) {   // every position: once coarse, once fine, at most
      const double z = z_lo + (double)i * hv;
      const double X = ax * z, Y = ay * z;
      const double q[3] = {(((r[0] * X + r[1] * Y) + r[2] * z) + p[4]) / voxel, (((r[3] * X + r[4] * Y) + r[5] * z) + p[5]) / voxel,
                           (((r[6] * X + r[7] * Y) + r[8] * z) + p[6]) / voxel};
      bool known = false, sampled = false;
      float D = 0.0f;
      if (kInterp && fine) {                                   // the nearest voxel is one of the corners: no probe of its own
        u64 base;
        float fr[3];
        if (ts_base(q, base, fr)) {
          if (!(kKeep && base == kept)) {
            long long at[8];
            mask = ts_corners<kTogether>(keys, recs, base, log2_slots, a.min_frames, v, at);
            kept = base;
          }
          const int idx = ts_nearest_corner(q, base);
          known = (mask >> idx) & 1u;
#pragma unroll
          for (int c = 0; c < 8; ++c) D = c == idx ? v[c] : D;
          if (known && mask == 0xFFu) D = ts_tri(v, fr);
          sampled = true;
        }
      }
      unsigned ix, iy, iz;
      if (!sampled && vh_cell_of(floor(q[0]), ix) && vh_cell_of(floor(q[1]), iy) && vh_cell_of(floor(q[2]), iz)) {
        const u64 key = vh_pack(ix, iy, iz);
        if (key == last) {
          known = last_known; D = last_D;
        } else {
          const long long at = vh_find(keys, key, log2_slots);
          if (at >= 0) {
            const uint2 sn = *(const uint2*)(recs + at);       // S and n: the first 8 of the record's 24 bytes
            if (sn.y >= a.min_frames && sn.y > 0u) { known = true; D = __uint_as_float(sn.x) / (float)sn.y; }
          }
          last = key; last_known = known; last_D = D;
        }
      }
      if (!fine) {
        if (!known) { i += K2; continue; }
        i = i == 0 ? 0 : i - K2 + 1;                           // just after the last unknown coarse position
        fine = true; run = 0; have_prev = false;
        continue;
      }
      if (!known) {
        have_prev = false;
        if (++run == K2) { fine = false; i += K2; } else { i += 1; }
        continue;
      }
      run = 0;
      if (have_prev && prev >= 0.0f && D < 0.0f) {
        const double z_prev = z_lo + (double)(i - 1) * hv;
        z_star = z_prev + hv * (double)(prev / (prev - D));
        result = (float)z_star;
        hit = true;
        break;
      }
      prev = D; have_prev = true; i += 1;
    }
    if (hit && extra) {                                        // once per pixel: the surface point's corners, with their slots
      const double X = ax * z_star, Y = ay * z_star;
      const double q[3] = {(((r[0] * X + r[1] * Y) + r[2] * z_star) + p[4]) / voxel,
                           (((r[3] * X + r[4] * Y) + r[5] * z_star) + p[5]) / voxel,
                           (((r[6] * X + r[7] * Y) + r[8] * z_star) + p[6]) / voxel};
      u64 base = 0;
      float fr[3];
      long long at[8];
      const bool based = ts_base(q, base, fr);
      mask = based ? ts_corners<kTogether>(keys, recs, base, log2_slots, a.min_frames, v, at) : 0u;
      bool have_n = false;
      if (mask == 0xFFu) {
        const float gx = ts_lerp(ts_lerp(v[1] - v[0], v[3] - v[2], fr[1]), ts_lerp(v[5] - v[4], v[7] - v[6], fr[1]), fr[2]);
        const float gy = ts_lerp(ts_lerp(v[2] - v[0], v[3] - v[1], fr[0]), ts_lerp(v[6] - v[4], v[7] - v[5], fr[0]), fr[2]);
        const float gz = ts_lerp(ts_lerp(v[4] - v[0], v[5] - v[1], fr[0]), ts_lerp(v[6] - v[2], v[7] - v[3], fr[0]), fr[1]);
        const double G0 = (double)gx, G1 = (double)gy, G2 = (double)gz;
        const double c0 = (r[0] * G0 + r[3] * G1) + r[6] * G2, c1 = (r[1] * G0 + r[4] * G1) + r[7] * G2;
        const double c2 = (r[2] * G0 + r[5] * G1) + r[8] * G2;
        const double len = sqrt((c0 * c0 + c1 * c1) + c2 * c2);
        if (len > 0.0) { nrm[0] = (float)(c0 / len); nrm[1] = (float)(c1 / len); nrm[2] = (float)(c2 / len); have_n = true; }
      }
      bool have_c = false;
      if (ra.colour || ra.view) {
        if (mask == 0xFFu) {
          float m[3][8];
          bool all = true;
#pragma unroll
          for (int c = 0; c < 8; ++c) {
            float mc[3];
            bool have;
            ts_mean_colour(recs + at[c], mc, have);
            all = all && have;
            m[0][c] = mc[0]; m[1][c] = mc[1]; m[2][c] = mc[2];
          }
          if (all) {
#pragma unroll
            for (int k = 0; k < 3; ++k) colr[k] = ts_tri(m[k], fr);
            have_c = true;
          }
        }
        if (!have_c) {                                         // the nearest voxel of the surface point
          long long near_at = -1;
          bool near_known = false;
          if (based) {
            const int idx = ts_nearest_corner(q, base);
            near_known = (mask >> idx) & 1u;
#pragma unroll
            for (int c = 0; c < 8; ++c) near_at = c == idx ? at[c] : near_at;
          } else {
            unsigned ix, iy, iz;
            if (vh_cell_of(floor(q[0]), ix) && vh_cell_of(floor(q[1]), iy) && vh_cell_of(floor(q[2]), iz)) {
              near_at = vh_find(keys, vh_pack(ix, iy, iz), log2_slots);
              if (near_at >= 0) {
                const uint2 sn = *(const uint2*)(recs + near_at);
                near_known = sn.y >= a.min_frames && sn.y > 0u;
              }
            }
          }
          if (near_known) {
            float mc[3];
            ts_mean_colour(recs + near_at, mc, have_c);
            if (have_c) { colr[0] = mc[0]; colr[1] = mc[1]; colr[2] = mc[2]; }
          }
        }
      }
      float shade = 1.0f;
      if (have_n) {
        const double vl = sqrt((ax * ax + ay * ay) + 1.0);
        const double dot = (((double)nrm[0] * ax + (double)nrm[1] * ay) + (double)nrm[2]) / vl;
        shade = (float)(0.25 + 0.75 * fmax(0.0, -dot));
      }
#pragma unroll
      for (int k = 0; k < 3; ++k) pix[k] = ts_byte((have_c ? colr[k] : 0.5f) * shade);
    }
  }
  if (active) {
    a.out[s * a.out_stride + px] = result;
    if (ra.normal) { float* o = ra.normal + s * ra.normal_stride + px * 3; o[0] = nrm[0]; o[1] = nrm[1]; o[2] = nrm[2]; }
    if (ra.colour) { float* o = ra.colour + s * ra.colour_stride + px * 3; o[0] = colr[0]; o[1] = colr[1]; o[2] = colr[2]; }
    if (ra.view) {
      unsigned char* o = ra.view + s * ra.view_stride + px * 3;
      o[0] = (unsigned char)pix[0]; o[1] = (unsigned char)pix[1]; o[2] = (unsigned char)pix[2];
    }
  }
  if (!a.hits) return;                                         // uniform
  unsigned n_hit = hit ? 1u : 0u;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) n_hit += __shfl_down(n_hit, off, 64);
  if (lane == 0) s_hits[wave] = n_hit;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned all = 0;
#pragma unroll
    for (int i = 0; i < kChunk / 64; ++i) all += s_hits[i];
    if (all) VH_ADD(a.hits + s, all);
  }
}

template <bool kTogether, bool kKeep>
int ts_render(const void* state, int b, int log2_slots, const float* cam_f, const float* cam_c, const double* pose, int h, int w,
              float near, float far, float voxel, int trunc, int min_frames, const float* guide, long long guide_stride, int window,
              const float* fill, long long fill_stride, int interp, float* depth_out, long long out_stride, float* normal_out,
              long long normal_stride, float* colour_out, long long colour_stride, uint8_t* view_out, long long view_stride,
              void* hits, void* stream) {
  RenderArgs ra;
  if (int e = ts_ray_args(state, b, log2_slots, cam_f, cam_c, pose, h, w, near, far, voxel, trunc, min_frames, guide, guide_stride,
                          window, fill, fill_stride, depth_out, out_stride, hits, ra.ray)) return e;
  const long long rgb = 3LL * h * w;
  M4D_CHECK_ARG(interp >= 0 && interp <= 1);
  M4D_CHECK_ARG((!normal_out || normal_stride >= rgb) && (!colour_out || colour_stride >= rgb) && (!view_out || view_stride >= rgb));
  M4D_CHECK_ARG(((((uintptr_t)normal_out) | ((uintptr_t)colour_out)) & 3u) == 0);
  ra.normal = normal_out; ra.normal_stride = normal_stride;
  ra.colour = colour_out; ra.colour_stride = colour_stride;
  ra.view = view_out; ra.view_stride = view_stride;
  const dim3 grid((unsigned)((long long)((w + 15) / 16) * ((h + 15) / 16)), (unsigned)b);
  if (interp) m4d_launch(tsdf_render_kernel<true, kTogether, kKeep>, grid, dim3(kChunk), 0, (hipStream_t)stream, ra, (const u64*)state, b, log2_slots);
  else m4d_launch(tsdf_render_kernel<false, true, true>, grid, dim3(kChunk), 0, (hipStream_t)stream, ra, (const u64*)state, b,
                  log2_slots);                                 // the nearest march looks up no corners: one form of it
  return M4D_LAUNCH_RESULT();
}

inline int ts_frame_args(const float* depth, long long depth_stride, const float* rgb, long long rgb_stride, const float* cam_f,
                         const float* cam_c, const double* pose, int b, int h, int w, float near, float far, float voxel,
                         int trunc, const void* state, int log2_slots, bool want_rgb, FrameArgs& a) {
  M4D_CHECK_ARG(depth && cam_f && cam_c && pose && state && (rgb || !want_rgb));
  M4D_CHECK_ARG(vh_geometry(b, log2_slots) && h >= 1 && w >= 1 && (long long)h * w <= kMaxPixels);
  M4D_CHECK_ARG(far > near && voxel > 0.0f && voxel < __builtin_inff() && trunc >= 2 && trunc <= 8);
  M4D_CHECK_ARG(depth_stride >= (long long)h * w && (!want_rgb || rgb_stride >= 3LL * h * w));
  M4D_CHECK_ARG(((((uintptr_t)depth) | ((uintptr_t)rgb) | ((uintptr_t)cam_f) | ((uintptr_t)cam_c)) & 3u) == 0);
  M4D_CHECK_ARG(((((uintptr_t)pose) | ((uintptr_t)state)) & 7u) == 0);
  a = {depth, depth_stride, rgb, rgb_stride, cam_f, cam_c, pose, h, w, trunc, near, far, voxel};
  return 0;
}

template <bool kSkip>
int ts_allocate(const float* depth, long long depth_stride, const float* cam_f, const float* cam_c, const double* pose, int b,
                int h, int w, float near, float far, float voxel, int trunc, void* state, int log2_slots, void* stream) {
  FrameArgs a;
  if (int e = ts_frame_args(depth, depth_stride, nullptr, 0, cam_f, cam_c, pose, b, h, w, near, far, voxel, trunc, state,
                            log2_slots, false, a)) return e;
  const dim3 grid((unsigned)(((long long)h * w + kChunk - 1) / kChunk), (unsigned)b);
  m4d_launch(tsdf_allocate_kernel<kSkip>, grid, dim3(kChunk), 0, (hipStream_t)stream, a, (u64*)state, b, log2_slots);
  return M4D_LAUNCH_RESULT();
}

}  // namespace

extern "C" long long m4d_tsdf_state_words(int b, int log2_slots) {
  return vh_geometry(b, log2_slots) ? (long long)b * (kStats + ((long long)(1 + kRecWords) << log2_slots)) : -1;
}

extern "C" int m4d_tsdf_allocate(const float* depth, long long depth_stride, const float* cam_f, const float* cam_c,
                                 const double* pose, int b, int h, int w, float near, float far, float voxel, int trunc,
                                 void* state, int log2_slots, void* stream) {
  return ts_allocate<true>(depth, depth_stride, cam_f, cam_c, pose, b, h, w, near, far, voxel, trunc, state, log2_slots, stream);
}

#if M4D_EXPERIMENTS
// every sample of a ray probes the table: the form the per-thread key skip was measured against (tools/bench_tsdf_mesh.py)
extern "C" int m4d_tsdf_allocate_plain(const float* depth, long long depth_stride, const float* cam_f, const float* cam_c,
                                       const double* pose, int b, int h, int w, float near, float far, float voxel, int trunc,
                                       void* state, int log2_slots, void* stream) {
  return ts_allocate<false>(depth, depth_stride, cam_f, cam_c, pose, b, h, w, near, far, voxel, trunc, state, log2_slots, stream);
}
#endif

extern "C" int m4d_tsdf_integrate(const float* depth, long long depth_stride, const float* rgb, long long rgb_stride,
                                  const float* cam_f, const float* cam_c, const double* pose, int b, int h, int w, float near,
                                  float far, float voxel, int trunc, void* state, int log2_slots, void* stream) {
  FrameArgs a;
  if (int e = ts_frame_args(depth, depth_stride, rgb, rgb_stride, cam_f, cam_c, pose, b, h, w, near, far, voxel, trunc, state,
                            log2_slots, true, a)) return e;
  const unsigned blocks = vh_slot_blocks(log2_slots, kChunk);
  m4d_launch(tsdf_integrate_kernel, dim3(blocks > kIntegrateBlocks ? kIntegrateBlocks : blocks, (unsigned)b), dim3(kChunk), 0,
             (hipStream_t)stream, a, (u64*)state, b, log2_slots);
  return M4D_LAUNCH_RESULT();
}

extern "C" int m4d_tsdf_extract_vertices(const void* state, int b, int log2_slots, int s, int min_frames, float voxel,
                                         void* keys_out, void* vertices_out, long long out_cap, void* count, void* stream) {
  M4D_CHECK_ARG(state && keys_out && vertices_out && count);
  M4D_CHECK_ARG(vh_geometry(b, log2_slots) && s >= 0 && s < b && min_frames >= 1 && out_cap >= 1);
  M4D_CHECK_ARG(voxel > 0.0f && voxel < __builtin_inff());
  M4D_CHECK_ARG(((((uintptr_t)state) | ((uintptr_t)keys_out) | ((uintptr_t)count)) & 7u) == 0 &&
                (((uintptr_t)vertices_out) & 15u) == 0);
  const u64* base = (const u64*)state + (long long)b * kStats;
  const u64* keys = base + ((long long)s << log2_slots);
  const TsdfRec* recs = (const TsdfRec*)(base + ((long long)b << log2_slots)) + ((long long)s << log2_slots);
  m4d_launch(tsdf_vertices_kernel, dim3(vh_slot_blocks(log2_slots, kChunk)), dim3(kChunk), 0, (hipStream_t)stream, keys, recs,
             log2_slots, (unsigned)min_frames, voxel, (u64*)keys_out, (uint4*)vertices_out, out_cap, (u64*)count);
  return M4D_LAUNCH_RESULT();
}

extern "C" int m4d_tsdf_extract_faces(const void* state, int b, int log2_slots, int s, int min_frames, void* quads_out,
                                      long long out_cap, void* count, void* stream) {
  M4D_CHECK_ARG(state && quads_out && count);
  M4D_CHECK_ARG(vh_geometry(b, log2_slots) && s >= 0 && s < b && min_frames >= 1 && out_cap >= 1);
  M4D_CHECK_ARG(((((uintptr_t)state) | ((uintptr_t)quads_out) | ((uintptr_t)count)) & 7u) == 0);
  const u64* base = (const u64*)state + (long long)b * kStats;
  const u64* keys = base + ((long long)s << log2_slots);
  const TsdfRec* recs = (const TsdfRec*)(base + ((long long)b << log2_slots)) + ((long long)s << log2_slots);
  m4d_launch(tsdf_faces_kernel, dim3(vh_slot_blocks(log2_slots, kChunk)), dim3(kChunk), 0, (hipStream_t)stream, keys, recs,
             log2_slots, (unsigned)min_frames, (u64*)quads_out, out_cap, (u64*)count);
  return M4D_LAUNCH_RESULT();
}

extern "C" int m4d_tsdf_clear(void* state, const unsigned char* mask, int b, int log2_slots, void* stream) {
  M4D_CHECK_ARG(state && vh_geometry(b, log2_slots) && (((uintptr_t)state) & 7u) == 0);
  const long long per_sample = ((1ll << log2_slots) + kChunk - 1) / kChunk;
  const dim3 grid((unsigned)(per_sample > 2048 ? 2048 : per_sample), (unsigned)b);
  m4d_launch(tsdf_clear_kernel, grid, dim3(kChunk), 0, (hipStream_t)stream, (u64*)state, mask, b, log2_slots);
  return M4D_LAUNCH_RESULT();
}

// the product form: 8x8 pixel tiles per wave, no probe for a key the previous sample had (tools/bench_tsdf_raycast.py)
extern "C" int m4d_tsdf_raycast(const void* state, int b, int log2_slots, const float* cam_f, const float* cam_c,
                                const double* pose, int h, int w, float near, float far, float voxel, int trunc, int min_frames,
                                const float* guide, long long guide_stride, int window, const float* fill, long long fill_stride,
                                float* depth_out, long long out_stride, void* hits, void* stream) {
  return ts_raycast<true, true>(state, b, log2_slots, cam_f, cam_c, pose, h, w, near, far, voxel, trunc, min_frames, guide,
                                guide_stride, window, fill, fill_stride, depth_out, out_stride, hits, stream);
}

// the product form: the eight corners probed together and kept while the base cell stays (tools/bench_tsdf_raycast.py)
extern "C" int m4d_tsdf_render(const void* state, int b, int log2_slots, const float* cam_f, const float* cam_c,
                               const double* pose, int h, int w, float near, float far, float voxel, int trunc, int min_frames,
                               const float* guide, long long guide_stride, int window, const float* fill, long long fill_stride,
                               int interp, float* depth_out, long long out_stride, float* normal_out, long long normal_stride,
                               float* colour_out, long long colour_stride, uint8_t* view_out, long long view_stride, void* hits,
                               void* stream) {
  return ts_render<true, true>(state, b, log2_slots, cam_f, cam_c, pose, h, w, near, far, voxel, trunc, min_frames, guide,
                               guide_stride, window, fill, fill_stride, interp, depth_out, out_stride, normal_out, normal_stride,
                               colour_out, colour_stride, view_out, view_stride, hits, stream);
}

#if M4D_EXPERIMENTS
// the forms the two devices were measured against; variant bit 0 = corners probed together, bit 1 = corners kept (0 = plain)
extern "C" int m4d_tsdf_render_plain(int variant, const void* state, int b, int log2_slots, const float* cam_f, const float* cam_c,
                                     const double* pose, int h, int w, float near, float far, float voxel, int trunc,
                                     int min_frames, const float* guide, long long guide_stride, int window, const float* fill,
                                     long long fill_stride, int interp, float* depth_out, long long out_stride, float* normal_out,
                                     long long normal_stride, float* colour_out, long long colour_stride, uint8_t* view_out,
                                     long long view_stride, void* hits, void* stream) {
#define TS_RENDER_FORM(together, keep)                                                                                       \
  ts_render<together, keep>(state, b, log2_slots, cam_f, cam_c, pose, h, w, near, far, voxel, trunc, min_frames, guide,      \
                            guide_stride, window, fill, fill_stride, interp, depth_out, out_stride, normal_out, normal_stride, \
                            colour_out, colour_stride, view_out, view_stride, hits, stream)
  switch (variant) {
    case 0: return TS_RENDER_FORM(false, false);
    case 1: return TS_RENDER_FORM(true, false);
    case 2: return TS_RENDER_FORM(false, true);
    case 3: return TS_RENDER_FORM(true, true);
  }
#undef TS_RENDER_FORM
  return (int)hipErrorInvalidValue;
}
#endif

#if M4D_EXPERIMENTS
// the forms the two choices were measured against; variant bit 0 = 8x8 tiles, bit 1 = key reuse (0 = the plain kernel)
extern "C" int m4d_tsdf_raycast_plain(int variant, const void* state, int b, int log2_slots, const float* cam_f,
                                      const float* cam_c, const double* pose, int h, int w, float near, float far, float voxel,
                                      int trunc, int min_frames, const float* guide, long long guide_stride, int window,
                                      const float* fill, long long fill_stride, float* depth_out, long long out_stride,
                                      void* hits, void* stream) {
#define TS_RAYCAST_FORM(tile, reuse)                                                                                         \
  ts_raycast<tile, reuse>(state, b, log2_slots, cam_f, cam_c, pose, h, w, near, far, voxel, trunc, min_frames, guide,        \
                          guide_stride, window, fill, fill_stride, depth_out, out_stride, hits, stream)
  switch (variant) {
    case 0: return TS_RAYCAST_FORM(false, false);
    case 1: return TS_RAYCAST_FORM(true, false);
    case 2: return TS_RAYCAST_FORM(false, true);
    case 3: return TS_RAYCAST_FORM(true, true);
  }
#undef TS_RAYCAST_FORM
  return (int)hipErrorInvalidValue;
}
#endif
