// TSDF surface meshes: the depth estimates of a trajectory fused into a truncated signed distance field on a hashed voxel grid
// (Curless & Levoy 1996; Niessner et al. 2013) and a naive-surface-nets extraction, on the device
// (include/m4depth_hip.h: m4d_tsdf_allocate, m4d_tsdf_integrate, m4d_tsdf_extract_vertices, m4d_tsdf_extract_faces, m4d_tsdf_clear).
//
// State: per sample four statistics words, then -- structure of arrays -- the keys of an open-addressing table (linear probing,
// the voxel map's key packing, hash, probe bound and 3/4 rule) and the 24-byte records behind them.  The per-frame pass over the
// table streams the keys only and touches the records of the voxels the frame sees.
//   allocate : one thread per pixel walks its ray over the truncation band and claims the keys (agent-scope load + compare-and-
//              swap); a claim writes the key only.  The SET of keys does not depend on the schedule.
//   integrate: every slot has one thread; the owner of a record is the only thread that touches it, so the float32 sum S is the
//              same for every schedule.  The only atomic is one add per workgroup on the `updates` statistic.
//   extract  : one thread per slot looks its neighbours up with a read-only probe; records leave through a wave ballot and one
//              atomic add per wave on a count word.  The host orders them.
// No loop depends on what the table holds (kProbe trips at most), nothing waits for another thread.
#include "m4d_common.h"
#include "../../include/m4depth_hip.h"

namespace {

typedef unsigned long long u64;

constexpr int kChunk = 256;
constexpr int kStats = 4;                                     // occupied, dropped_range, dropped_full, updates
constexpr int kRecWords = 3;                                  // 24 bytes: float S, uint32 n, sr, sg, sb, nc
constexpr int kProbe = 128;
constexpr u64 kEmpty = ~0ull;
constexpr int kHalf = 1 << 20;
constexpr unsigned kCellMax = (1u << 21) - 1u;                // the largest biased cell index
constexpr long long kMaxPixels = 1LL << 24;
constexpr unsigned kIntegrateBlocks = 1024;                  // workgroups per sample of the integrate pass, at most

#define TS_LOAD(p) __hip_atomic_load((p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#define TS_ADD(p, v) __hip_atomic_fetch_add((p), (u64)(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)

struct TsdfRec { float S; unsigned n, sr, sg, sb, nc; };
static_assert(sizeof(TsdfRec) == 24, "record layout");

__device__ __forceinline__ u64 ts_slot_of(u64 key, int log2_slots) {
  return (key * 0x9E3779B97F4A7C15ull) >> (64 - log2_slots);
}

__device__ __forceinline__ u64* ts_keys(u64* state, int b, int s, int log2_slots) {
  return state + (long long)b * kStats + ((long long)s << log2_slots);
}
__device__ __forceinline__ TsdfRec* ts_recs(u64* state, int b, int s, int log2_slots) {
  return (TsdfRec*)(state + (long long)b * kStats + ((long long)b << log2_slots)) + ((long long)s << log2_slots);
}

// R(q) as get_rot_mat writes it, float64 (m4d_depth_cloud's expressions)
struct Rot { double r[3][3]; };
__device__ __forceinline__ Rot ts_rot(const double* p) {
  const double qw = p[0], qx = p[1], qy = p[2], qz = p[3];
  const double tx = 2.0 * qx, ty = 2.0 * qy, tz = 2.0 * qz;
  const double twx = tx * qw, twy = ty * qw, twz = tz * qw;
  const double txx = tx * qx, txy = ty * qx, txz = tz * qx;
  const double tyy = ty * qy, tyz = tz * qy, tzz = tz * qz;
  Rot m;
  m.r[0][0] = 1.0 - (tyy + tzz); m.r[0][1] = txy - twz; m.r[0][2] = txz + twy;
  m.r[1][0] = txy + twz; m.r[1][1] = 1.0 - (txx + tzz); m.r[1][2] = tyz - twx;
  m.r[2][0] = txz - twy; m.r[2][1] = tyz + twx; m.r[2][2] = 1.0 - (txx + tyy);
  return m;
}

__device__ __forceinline__ bool ts_pose_finite(const double* p) {
  bool ok = true;
#pragma unroll
  for (int i = 0; i < 7; ++i) ok = ok && isfinite(p[i]);
  return ok;
}

__device__ __forceinline__ bool ts_cell(double x, double voxel, unsigned& cell) {
  const double fl = floor(x / voxel);
  if (!(fl >= -(double)kHalf && fl < (double)kHalf)) return false;
  cell = (unsigned)((int)fl + kHalf);
  return true;
}

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
  const Rot m = ts_rot(p);
  const double voxel = (double)a.voxel, hv = voxel * 0.5;
  u64* stats = state + (long long)s * kStats;
  u64* keys = ts_keys(state, b, s, log2_slots);
  const u64 slots = 1ull << log2_slots, limit = slots - (slots >> 2);
  u64 last = kEmpty;
  unsigned n_range = 0, n_full = 0;
  for (int k = -2 * a.trunc; active && k <= 2 * a.trunc; ++k) {
    const double z = (double)d + (double)k * hv;
    if (!(z > 0.0)) continue;
    const double X = ax * z, Y = ay * z;
    const double wx = ((m.r[0][0] * X + m.r[0][1] * Y) + m.r[0][2] * z) + p[4];
    const double wy = ((m.r[1][0] * X + m.r[1][1] * Y) + m.r[1][2] * z) + p[5];
    const double wz = ((m.r[2][0] * X + m.r[2][1] * Y) + m.r[2][2] * z) + p[6];
    unsigned ix, iy, iz;
    if (!(ts_cell(wx, voxel, ix) && ts_cell(wy, voxel, iy) && ts_cell(wz, voxel, iz))) { ++n_range; continue; }
    const u64 key = ((u64)ix << 42) | ((u64)iy << 21) | (u64)iz;
    if (kSkip && key == last) continue;
    u64 slot = ts_slot_of(key, log2_slots);
    bool found = false;
    for (int i = 0; i < kProbe; ++i) {
      u64* q = keys + slot;
      u64 cur = TS_LOAD(q);
      if (cur == kEmpty) {
        if (TS_LOAD(stats + 0) >= limit) break;               // three quarters full: empty slots are no longer claimed
        u64 expected = kEmpty;
        if (__hip_atomic_compare_exchange_strong(q, &expected, key, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                 __HIP_MEMORY_SCOPE_AGENT)) {
          TS_ADD(stats + 0, 1);
          cur = key;
        } else {
          cur = expected;
        }
      }
      if (cur == key) { found = true; break; }
      slot = (slot + 1) & (slots - 1);
    }
    if (found) last = key; else ++n_full;
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
    if (range) TS_ADD(stats + 1, range);
    if (full) TS_ADD(stats + 2, full);
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
  const Rot m = ts_rot(p);
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
    const double D0 = ((double)((int)(key >> 42) - kHalf) + 0.5) * voxel - t0;
    const double D1 = ((double)((int)((key >> 21) & 0x1FFFFFull) - kHalf) + 0.5) * voxel - t1;
    const double D2 = ((double)((int)(key & 0x1FFFFFull) - kHalf) + 0.5) * voxel - t2;
    const double X0 = (m.r[0][0] * D0 + m.r[1][0] * D1) + m.r[2][0] * D2;
    const double X1 = (m.r[0][1] * D0 + m.r[1][1] * D1) + m.r[2][1] * D2;
    const double z = (m.r[0][2] * D0 + m.r[1][2] * D1) + m.r[2][2] * D2;
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
    if (all) TS_ADD(state + (long long)s * kStats + 3, all);
  }
}

// the slot of `key` in the table, or -1: the insertion's probe sequence, read-only; it ends at an empty slot
__device__ __forceinline__ long long ts_find(const u64* __restrict__ keys, u64 key, int log2_slots) {
  const u64 slots = 1ull << log2_slots;
  u64 slot = ts_slot_of(key, log2_slots);
  for (int i = 0; i < kProbe; ++i) {
    const u64 cur = keys[slot];
    if (cur == key) return (long long)slot;
    if (cur == kEmpty) return -1;
    slot = (slot + 1) & (slots - 1);
  }
  return -1;
}

// wave ballot + one atomic add per wave: the place of this lane's record, or -1 when it has none
__device__ __forceinline__ long long ts_place(bool keep, u64* count) {
  const int lane = threadIdx.x & 63;
  const u64 mask = __ballot(keep);
  if (!mask) return -1;
  const int first = __builtin_ctzll(mask);
  const int rank = __builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
  u64 base = 0;
  if (lane == first) base = TS_ADD(count, __popcll(mask));
  base = __shfl(base, first, 64);
  return keep ? (long long)base + rank : -1;
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
      const unsigned cx = (unsigned)(key >> 42), cy = (unsigned)((key >> 21) & 0x1FFFFFull), cz = (unsigned)(key & 0x1FFFFFull);
      bool valid = cx < kCellMax && cy < kCellMax && cz < kCellMax;
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        D[c] = 0.0f;
        if (!valid) continue;
        long long at = slot;
        if (c) {
          const u64 other = ((u64)(cx + (c & 1)) << 42) | ((u64)(cy + ((c >> 1) & 1)) << 21) | (u64)(cz + ((c >> 2) & 1));
          at = ts_find(keys, other, log2_slots);
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
  const long long at = ts_place(keep, count);
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
    const int cell = (int)((key >> (42 - 21 * i)) & 0x1FFFFFull) - kHalf;
    const float local = sum[i] / (float)crossings;
    pos[i] = (float)((((double)cell + 0.5) + (double)local) * voxel);
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
      cell[0] = (unsigned)(key >> 42); cell[1] = (unsigned)((key >> 21) & 0x1FFFFFull); cell[2] = (unsigned)(key & 0x1FFFFFull);
    }
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) {                                // no early return: every lane takes part in the three ballots
    const int bx = (a + 1) % 3, cx = (a + 2) % 3;
    const u64 ea = 1ull << (42 - 21 * a), eb = 1ull << (42 - 21 * bx), ec = 1ull << (42 - 21 * cx);
    bool emit = false;
    if (valid && cell[a] < kCellMax && cell[bx] >= 1u && cell[cx] >= 1u) {
      const long long at = ts_find(keys, key + ea, log2_slots);
      if (at >= 0) {
        const TsdfRec r = recs[at];
        if (r.n >= min_frames && r.n > 0u) emit = (r.S / (float)r.n < 0.0f) != in_k;
      }
    }
    const long long at = ts_place(emit, count);
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

inline bool ts_geometry(int b, int log2_slots) { return b >= 1 && b <= 65535 && log2_slots >= 6 && log2_slots <= 26; }

inline int ts_frame_args(const float* depth, long long depth_stride, const float* rgb, long long rgb_stride, const float* cam_f,
                         const float* cam_c, const double* pose, int b, int h, int w, float near, float far, float voxel,
                         int trunc, const void* state, int log2_slots, bool want_rgb, FrameArgs& a) {
  M4D_CHECK_ARG(depth && cam_f && cam_c && pose && state && (rgb || !want_rgb));
  M4D_CHECK_ARG(ts_geometry(b, log2_slots) && h >= 1 && w >= 1 && (long long)h * w <= kMaxPixels);
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

inline unsigned ts_slot_blocks(int log2_slots) { return (unsigned)(((1ll << log2_slots) + kChunk - 1) / kChunk); }

}  // namespace

extern "C" long long m4d_tsdf_state_words(int b, int log2_slots) {
  return ts_geometry(b, log2_slots) ? (long long)b * (kStats + ((long long)(1 + kRecWords) << log2_slots)) : -1;
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
  const unsigned blocks = ts_slot_blocks(log2_slots);
  m4d_launch(tsdf_integrate_kernel, dim3(blocks > kIntegrateBlocks ? kIntegrateBlocks : blocks, (unsigned)b), dim3(kChunk), 0,
             (hipStream_t)stream, a, (u64*)state, b, log2_slots);
  return M4D_LAUNCH_RESULT();
}

extern "C" int m4d_tsdf_extract_vertices(const void* state, int b, int log2_slots, int s, int min_frames, float voxel,
                                         void* keys_out, void* vertices_out, long long out_cap, void* count, void* stream) {
  M4D_CHECK_ARG(state && keys_out && vertices_out && count);
  M4D_CHECK_ARG(ts_geometry(b, log2_slots) && s >= 0 && s < b && min_frames >= 1 && out_cap >= 1);
  M4D_CHECK_ARG(voxel > 0.0f && voxel < __builtin_inff());
  M4D_CHECK_ARG(((((uintptr_t)state) | ((uintptr_t)keys_out) | ((uintptr_t)count)) & 7u) == 0 &&
                (((uintptr_t)vertices_out) & 15u) == 0);
  const u64* base = (const u64*)state + (long long)b * kStats;
  const u64* keys = base + ((long long)s << log2_slots);
  const TsdfRec* recs = (const TsdfRec*)(base + ((long long)b << log2_slots)) + ((long long)s << log2_slots);
  m4d_launch(tsdf_vertices_kernel, dim3(ts_slot_blocks(log2_slots)), dim3(kChunk), 0, (hipStream_t)stream, keys, recs, log2_slots,
             (unsigned)min_frames, voxel, (u64*)keys_out, (uint4*)vertices_out, out_cap, (u64*)count);
  return M4D_LAUNCH_RESULT();
}

extern "C" int m4d_tsdf_extract_faces(const void* state, int b, int log2_slots, int s, int min_frames, void* quads_out,
                                      long long out_cap, void* count, void* stream) {
  M4D_CHECK_ARG(state && quads_out && count);
  M4D_CHECK_ARG(ts_geometry(b, log2_slots) && s >= 0 && s < b && min_frames >= 1 && out_cap >= 1);
  M4D_CHECK_ARG(((((uintptr_t)state) | ((uintptr_t)quads_out) | ((uintptr_t)count)) & 7u) == 0);
  const u64* base = (const u64*)state + (long long)b * kStats;
  const u64* keys = base + ((long long)s << log2_slots);
  const TsdfRec* recs = (const TsdfRec*)(base + ((long long)b << log2_slots)) + ((long long)s << log2_slots);
  m4d_launch(tsdf_faces_kernel, dim3(ts_slot_blocks(log2_slots)), dim3(kChunk), 0, (hipStream_t)stream, keys, recs, log2_slots,
             (unsigned)min_frames, (u64*)quads_out, out_cap, (u64*)count);
  return M4D_LAUNCH_RESULT();
}

extern "C" int m4d_tsdf_clear(void* state, const unsigned char* mask, int b, int log2_slots, void* stream) {
  M4D_CHECK_ARG(state && ts_geometry(b, log2_slots) && (((uintptr_t)state) & 7u) == 0);
  const long long per_sample = ((1ll << log2_slots) + kChunk - 1) / kChunk;
  const dim3 grid((unsigned)(per_sample > 2048 ? 2048 : per_sample), (unsigned)b);
  m4d_launch(tsdf_clear_kernel, grid, dim3(kChunk), 0, (hipStream_t)stream, (u64*)state, mask, b, log2_slots);
  return M4D_LAUNCH_RESULT();
}
