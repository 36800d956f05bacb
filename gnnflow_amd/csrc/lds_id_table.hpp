// The probing of a row's LDS table keyed by the 64-bit neighbour id, shared by the readers that
// hash a row's two windows (common_neighbors.hip, neighbor_cooccurrence.hip, pair_sequence.hip).
// Each file keeps its own table struct, whose slots differ (20 bytes with pa, 16 without); what
// is shared is how a slot is found: open addressing, linear probing, `cap` slots in use (a power of two, shift =
// 64 - log2(cap)), the empty mark -1, which no neighbour is.  A table type T has `int64_t key[]`
// with at least cap elements, all kIdEmpty before the first claim.
//
// A probe loop runs at most cap trips and then gives the key up instead of spinning.  That cannot
// happen where the caller keeps the load at or below 1/2: with at most cap / 2 keys in cap slots a
// probe sequence meets the key itself or an empty slot first, and no slot is ever emptied while
// keys are claimed.
#pragma once

#include <cstdint>

#include <hip/hip_runtime.h>

namespace gf {

constexpr int kIdTableWave = 64;
constexpr int64_t kIdEmpty = -1;

// TPR threads work on a row.  One wave: its LDS operations complete in order, the fence is for the
// compiler.  Several waves: a barrier, which every wave of the workgroup has to reach the same
// number of times.
template <int TPR>
__device__ __forceinline__ void phase_end() {
  if constexpr (TPR == kIdTableWave) {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
  } else {
    __syncthreads();
  }
}

__device__ __forceinline__ uint32_t home_slot(int64_t z, uint32_t shift) {
  return static_cast<uint32_t>((static_cast<uint64_t>(z) * 0x9E3779B97F4A7C15ull) >> shift);
}

// the slot of key z, claimed if z is new; cap when the table is full (it never is: header comment)
template <class T>
__device__ __forceinline__ uint32_t claim(T& tb, int64_t z, uint32_t cap, uint32_t shift) {
  uint32_t h = home_slot(z, shift);
  for (uint32_t i = 0; i < cap; ++i) {
    const unsigned long long seen =
        atomicCAS(reinterpret_cast<unsigned long long*>(&tb.key[h]),
                  static_cast<unsigned long long>(kIdEmpty), static_cast<unsigned long long>(z));
    if (seen == static_cast<unsigned long long>(kIdEmpty) ||
        seen == static_cast<unsigned long long>(z))
      return h;
    h = (h + 1) & (cap - 1);
  }
  return cap;
}

// the slot that holds key z; cap if none does (a claimed key is always found)
template <class T>
__device__ __forceinline__ uint32_t find(const T& tb, int64_t z, uint32_t cap, uint32_t shift) {
  uint32_t h = home_slot(z, shift);
  for (uint32_t i = 0; i < cap; ++i) {
    const int64_t k = tb.key[h];
    if (k == z) return h;
    if (k == kIdEmpty) break;
    h = (h + 1) & (cap - 1);
  }
  return cap;
}

}  // namespace gf
