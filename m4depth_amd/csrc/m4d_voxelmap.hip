// Voxel maps: the per-frame point clouds of a trajectory merged into one vertex per occupied voxel, on the device
// (include/m4depth_hip.h: m4d_voxel_map_integrate, m4d_voxel_map_extract, m4d_voxel_map_clear).
//
// State: one hashed voxel grid per sample (m4d_voxel_hash.h), records of kRec = 10 unsigned 64-bit words (key, n, sx, sy, sz,
// sr, sg, sb, last_stamp, frames) behind four statistics words per sample.  Every accumulator is an integer, so the sums do
// not depend on the order in which threads arrive and the table's CONTENT is the same for every schedule -- only the slot a key
// lives in may differ, and the extraction's order is made the key order on the host.
//
// Integrate: one thread per vertex.  Raster-order neighbours often share a voxel, so the lanes of a wave first sum the
// contributions of every run of consecutive lanes with one key (a segmented shuffle reduction on two packed words), and only
// the head lane of a run probes the table and issues the atomics: 9 atomics per run instead of per vertex.  Integer sums: the
// bits cannot change.  kCombine = false is the one-vertex-one-probe form it was measured against.
#include "m4d_voxel_hash.h"
#include "../../include/m4depth_hip.h"

namespace {

constexpr int kChunk = 256;                                   // vertices per workgroup = threads per workgroup
constexpr int kWaves = kChunk / 64;
constexpr int kRec = 10;                                      // words of a table record
constexpr int kStats = 4;                                     // observations, dropped_range, dropped_full, occupied
constexpr long long kMaxCap = 1LL << 24;                      // m4d_depth_cloud's bound on the vertices of a sample

// one coordinate -> voxel index + 2^20 and the offset bin 0..255; false = out of range
__device__ __forceinline__ bool vm_axis(float x, double voxel, unsigned& cell, unsigned& off) {
  const double g = (double)x / voxel;
  const double fl = floor(g);
  if (!vh_cell_of(fl, cell)) return false;
  const int o = (int)floor((g - fl) * 256.0);                 // g - fl rounds to 1.0 for a tiny negative g: bin 255
  off = (unsigned)(o > 255 ? 255 : o);
  return true;
}

template <bool kCombine>
__global__ void __launch_bounds__(kChunk)
voxel_integrate_kernel(const uint4* __restrict__ vertices, const int* __restrict__ counts, int cap, float voxel_f,
                       u64 stamp, u64* __restrict__ state, int b, int log2_slots) {
  __shared__ unsigned s_obs[kWaves], s_range[kWaves];
  const int s = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int k = blockIdx.x * kChunk + threadIdx.x;
  int count = counts[s];
  count = count < 0 ? 0 : (count > cap ? cap : count);
  const bool in = k < count;

  u64 key = kEmpty, pa = 0, pb = 0;                           // pa = ox | oy << 16 | oz << 32 | n << 48, pb = r | g << 16 | b << 32
  bool ok = false;
  if (in) {
    const uint4 v = vertices[(long long)s * cap + k];
    const float x = __uint_as_float(v.x), y = __uint_as_float(v.y), z = __uint_as_float(v.z);
    unsigned cx = 0, cy = 0, cz = 0, ox = 0, oy = 0, oz = 0;
    const double voxel = (double)voxel_f;
    ok = isfinite(x) && isfinite(y) && isfinite(z) && vm_axis(x, voxel, cx, ox) && vm_axis(y, voxel, cy, oy) &&
         vm_axis(z, voxel, cz, oz);
    if (ok) {
      key = vh_pack(cx, cy, cz);
      pa = (u64)ox | ((u64)oy << 16) | ((u64)oz << 32) | (1ull << 48);
      pb = (u64)(v.w & 0xFFu) | ((u64)((v.w >> 8) & 0xFFu) << 16) | ((u64)((v.w >> 16) & 0xFFu) << 32);
    }
  }
  const u64 m_in = __ballot(in), m_bad = __ballot(in && !ok);
  if (lane == 0) { s_obs[wave] = __popcll(m_in); s_range[wave] = __popcll(m_bad); }

  bool head = ok;
  if (kCombine) {
    // runs of consecutive lanes with one key: the head of a run ends up with the run's sums (at most 64 * 255 per field)
    const u64 before = __shfl_up(key, 1, 64);
    const bool starts = lane == 0 || before != key;           // dropped lanes carry kEmpty and form runs of their own kind
    const u64 heads = __ballot(starts);
    const u64 above = lane == 63 ? 0ull : heads & ~((2ull << lane) - 1ull);
    const int end = above ? __builtin_ctzll(above) : 64;      // first lane of the next run
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const u64 qa = __shfl_down(pa, off, 64), qb = __shfl_down(pb, off, 64);
      if (lane + off < end) { pa += qa; pb += qb; }
    }
    head = ok && starts;
  }

  u64* stats = state + (long long)s * kStats;
  if (head) {
    u64* table = state + (long long)b * kStats + ((long long)s << log2_slots) * kRec;
    u64* rec = vh_claim<kRec>(table, key, log2_slots, stats + 3);
    const u64 n = pa >> 48;
    if (rec) {
      VH_ADD(rec + 1, n);
      VH_ADD(rec + 2, pa & 0xFFFFu);
      VH_ADD(rec + 3, (pa >> 16) & 0xFFFFu);
      VH_ADD(rec + 4, (pa >> 32) & 0xFFFFu);
      VH_ADD(rec + 5, pb & 0xFFFFu);
      VH_ADD(rec + 6, (pb >> 16) & 0xFFFFu);
      VH_ADD(rec + 7, (pb >> 32) & 0xFFFFu);
      const u64 old = __hip_atomic_fetch_max(rec + 8, stamp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (old < stamp) VH_ADD(rec + 9, 1);
    } else {
      VH_ADD(stats + 2, n);                                   // the probe ran out, or the table is full
    }
  }

  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned obs = 0, range = 0;
#pragma unroll
    for (int i = 0; i < kWaves; ++i) { obs += s_obs[i]; range += s_range[i]; }
    if (obs) VH_ADD(stats + 0, obs);
    if (range) VH_ADD(stats + 1, range);
  }
}

// one thread per slot of sample s; the qualifying records leave in the order the waves arrive
__global__ void __launch_bounds__(kChunk)
voxel_extract_kernel(const u64* __restrict__ table, int log2_slots, u64 min_frames, float voxel_f,
                     u64* __restrict__ keys_out, uint4* __restrict__ vertices_out, long long out_cap,
                     u64* __restrict__ count) {
  const long long slot = (long long)blockIdx.x * kChunk + threadIdx.x;
  const u64* rec = table + slot * kRec;
  bool keep = false;
  u64 key = kEmpty;
  if (slot < (1ll << log2_slots)) {
    key = rec[0];
    keep = key != kEmpty && rec[1] > 0 && rec[9] >= min_frames;
  }
  const long long at = vh_place(keep, count);
  if (at < 0 || at >= out_cap) return;                        // the count still says how many there were
  const u64 n = rec[1];
  const double voxel = (double)voxel_f, dn = (double)n;
  float p[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    p[a] = (float)(((double)vh_cell(key, a) + ((double)rec[2 + a] / dn + 0.5) / 256.0) * voxel);
  }
  const unsigned r = (unsigned)((2 * rec[5] + n) / (2 * n)), g = (unsigned)((2 * rec[6] + n) / (2 * n)),
                 bl = (unsigned)((2 * rec[7] + n) / (2 * n));
  const u64 frames = rec[9];
  const unsigned alpha = frames > 255 ? 255u : (unsigned)frames;
  keys_out[at] = key;
  vertices_out[at] = make_uint4(__float_as_uint(p[0]), __float_as_uint(p[1]), __float_as_uint(p[2]),
                                r | (g << 8) | (bl << 16) | (alpha << 24));
}

__global__ void __launch_bounds__(kChunk)
voxel_clear_kernel(u64* __restrict__ state, const unsigned char* __restrict__ mask, int b, int log2_slots) {
  const int s = blockIdx.y;
  if (mask && !mask[s]) return;
  const long long words = (1ll << log2_slots) * kRec;
  u64* table = state + (long long)b * kStats + (long long)s * words;
  const long long stride = (long long)gridDim.x * kChunk;
  for (long long i = (long long)blockIdx.x * kChunk + threadIdx.x; i < words; i += stride)
    table[i] = (i % kRec == 0) ? kEmpty : 0ull;
  if (blockIdx.x == 0 && threadIdx.x < kStats) state[(long long)s * kStats + threadIdx.x] = 0ull;
}

template <bool kCombine>
int vm_integrate(const void* vertices, const int* counts, int b, int cap, float voxel, long long stamp, void* state,
                 int log2_slots, void* stream) {
  M4D_CHECK_ARG(vertices && counts && state);
  M4D_CHECK_ARG(vh_geometry(b, log2_slots) && cap >= 1 && cap <= kMaxCap);
  M4D_CHECK_ARG(voxel > 0.0f && voxel < __builtin_inff() && stamp >= 1);
  M4D_CHECK_ARG((((uintptr_t)vertices) & 15u) == 0 && (((uintptr_t)counts) & 3u) == 0 && (((uintptr_t)state) & 7u) == 0);
  const dim3 grid((unsigned)((cap + kChunk - 1) / kChunk), (unsigned)b);
  m4d_launch(voxel_integrate_kernel<kCombine>, grid, dim3(kChunk), 0, (hipStream_t)stream, (const uint4*)vertices, counts, cap,
             voxel, (u64)stamp, (u64*)state, b, log2_slots);
  return M4D_LAUNCH_RESULT();
}

}  // namespace

extern "C" long long m4d_voxel_map_state_words(int b, int log2_slots) {
  return vh_geometry(b, log2_slots) ? (long long)b * (kStats + ((long long)kRec << log2_slots)) : -1;
}

extern "C" int m4d_voxel_map_integrate(const void* vertices, const int* counts, int b, int cap, float voxel, long long stamp,
                                       void* state, int log2_slots, void* stream) {
  return vm_integrate<true>(vertices, counts, b, cap, voxel, stamp, state, log2_slots, stream);
}

#if M4D_EXPERIMENTS
// the one-vertex-one-probe form the in-wave combining was measured against (tools/bench_voxel_map.py)
extern "C" int m4d_voxel_map_integrate_uncombined(const void* vertices, const int* counts, int b, int cap, float voxel,
                                                  long long stamp, void* state, int log2_slots, void* stream) {
  return vm_integrate<false>(vertices, counts, b, cap, voxel, stamp, state, log2_slots, stream);
}
#endif

extern "C" int m4d_voxel_map_extract(const void* state, int b, int log2_slots, int s, int min_frames, float voxel,
                                     void* keys_out, void* vertices_out, long long out_cap, void* count, void* stream) {
  M4D_CHECK_ARG(state && keys_out && vertices_out && count);
  M4D_CHECK_ARG(vh_geometry(b, log2_slots) && s >= 0 && s < b && min_frames >= 1 && out_cap >= 1);
  M4D_CHECK_ARG(voxel > 0.0f && voxel < __builtin_inff());
  M4D_CHECK_ARG(((((uintptr_t)state) | ((uintptr_t)keys_out) | ((uintptr_t)count)) & 7u) == 0 &&
                (((uintptr_t)vertices_out) & 15u) == 0);
  const u64* table = (const u64*)state + (long long)b * kStats + ((long long)s << log2_slots) * kRec;
  m4d_launch(voxel_extract_kernel, dim3(vh_slot_blocks(log2_slots, kChunk)), dim3(kChunk), 0, (hipStream_t)stream, table,
             log2_slots, (u64)min_frames, voxel, (u64*)keys_out, (uint4*)vertices_out, out_cap, (u64*)count);
  return M4D_LAUNCH_RESULT();
}

extern "C" int m4d_voxel_map_clear(void* state, const unsigned char* mask, int b, int log2_slots, void* stream) {
  M4D_CHECK_ARG(state && vh_geometry(b, log2_slots) && (((uintptr_t)state) & 7u) == 0);
  const long long per_sample = ((1ll << log2_slots) * kRec + kChunk - 1) / kChunk;
  const dim3 grid((unsigned)(per_sample > 2048 ? 2048 : per_sample), (unsigned)b);
  m4d_launch(voxel_clear_kernel, grid, dim3(kChunk), 0, (hipStream_t)stream, (u64*)state, mask, b, log2_slots);
  return M4D_LAUNCH_RESULT();
}
