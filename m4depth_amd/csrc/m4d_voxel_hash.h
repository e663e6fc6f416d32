// The hashed voxel grid of m4d_voxelmap.hip and m4d_tsdf.hip: one open-addressing table per sample, linear probing.
//   key     three cell indices floor(x / voxel) + 2^20, 21 bits each, x in the top bits; kEmpty = all ones is no key (a valid
//           key stays below 2^63)
//   slot    Fibonacci hashing: the top log2_slots bits of key * 2^64 / phi
//   claim   an insertion walks at most kProbe slots from there; an empty one is claimed by compare-and-swap unless the sample's
//           `occupied` counter has reached 3/4 of the slots.  Keys are read and claimed with relaxed agent-scope atomics only
//           (a sample's table is touched by workgroups on every XCD).  WHICH keys a table holds does not depend on the schedule
//           as long as it neither fills nor exhausts a probe; the slot a key lives in may.
// No loop depends on what the table holds (kProbe trips at most), nothing waits for another thread.
#pragma once
#include "m4d_common.h"

namespace {

typedef unsigned long long u64;

constexpr int kProbe = 128;                                   // probe trips of one insertion or lookup: the constant bound
constexpr u64 kEmpty = ~0ull;
constexpr int kHalf = 1 << 20;                                // voxel indices live in [-2^20, 2^20)
constexpr unsigned kCellMax = (1u << 21) - 1u;                // the largest biased cell index

#define VH_LOAD(p) __hip_atomic_load((p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#define VH_ADD(p, v) __hip_atomic_fetch_add((p), (u64)(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)

__device__ __forceinline__ u64 vh_pack(unsigned cx, unsigned cy, unsigned cz) {
  return ((u64)cx << 42) | ((u64)cy << 21) | (u64)cz;
}
__device__ __forceinline__ unsigned vh_biased(u64 key, int axis) {              // the biased cell index, axis 0 = x
  return (unsigned)((key >> (42 - 21 * axis)) & 0x1FFFFFull);
}
__device__ __forceinline__ int vh_cell(u64 key, int axis) { return (int)vh_biased(key, axis) - kHalf; }

__device__ __forceinline__ u64 vh_slot_of(u64 key, int log2_slots) {
  return (key * 0x9E3779B97F4A7C15ull) >> (64 - log2_slots);
}

// fl = floor(x / voxel), computed by the caller -> the biased cell index; false = out of range (NaN included)
__device__ __forceinline__ bool vh_cell_of(double fl, unsigned& cell) {
  if (!(fl >= -(double)kHalf && fl < (double)kHalf)) return false;
  cell = (unsigned)((int)fl + kHalf);
  return true;
}

// insert-or-find: the slot of `key` -- the address of its key word -- in a table whose keys are kStride words apart, or nullptr:
// the probe ran out, or the table is three quarters full and empty slots are no longer claimed.  A fresh claim writes the key
// only and counts in *occupied.
template <int kStride>
__device__ __forceinline__ u64* vh_claim(u64* keys, u64 key, int log2_slots, u64* occupied) {
  const u64 slots = 1ull << log2_slots, limit = slots - (slots >> 2);
  u64 slot = vh_slot_of(key, log2_slots);
  u64* at = nullptr;
  for (int i = 0; i < kProbe; ++i) {
    u64* p = keys + slot * kStride;
    u64 cur = VH_LOAD(p);
    if (cur == kEmpty) {
      if (VH_LOAD(occupied) >= limit) break;
      u64 expected = kEmpty;
      if (__hip_atomic_compare_exchange_strong(p, &expected, key, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                               __HIP_MEMORY_SCOPE_AGENT)) {
        VH_ADD(occupied, 1);
        cur = key;
      } else {
        cur = expected;                                       // somebody else's claim: maybe of this very key
      }
    }
    if (cur == key) { at = p; break; }
    slot = (slot + 1) & (slots - 1);
  }
  return at;
}

// the slot of `key` in a table nobody writes, or -1: the insertion's probe sequence, read-only; it ends at an empty slot
__device__ __forceinline__ long long vh_find(const u64* __restrict__ keys, u64 key, int log2_slots) {
  const u64 slots = 1ull << log2_slots;
  u64 slot = vh_slot_of(key, log2_slots);
  for (int i = 0; i < kProbe; ++i) {
    const u64 cur = keys[slot];
    if (cur == key) return (long long)slot;
    if (cur == kEmpty) return -1;
    slot = (slot + 1) & (slots - 1);
  }
  return -1;
}

// wave ballot + one atomic add per wave: the place of this lane's record in an output list, or -1 when it has none
__device__ __forceinline__ long long vh_place(bool keep, u64* count) {
  const int lane = threadIdx.x & 63;
  const u64 mask = __ballot(keep);
  if (!mask) return -1;
  const int first = __builtin_ctzll(mask);
  const int rank = __builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
  u64 base = 0;
  if (lane == first) base = VH_ADD(count, __popcll(mask));
  base = __shfl(base, first, 64);
  return keep ? (long long)base + rank : -1;
}

inline bool vh_geometry(int b, int log2_slots) { return b >= 1 && b <= 65535 && log2_slots >= 6 && log2_slots <= 26; }

// workgroups of `threads` that give every slot of one sample's table a thread
inline unsigned vh_slot_blocks(int log2_slots, int threads) { return (unsigned)(((1ll << log2_slots) + threads - 1) / threads); }

}  // namespace
