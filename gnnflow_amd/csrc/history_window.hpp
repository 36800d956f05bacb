// "The edges of a node strictly before t", resolved on the device over one node's segment of the
// temporal edge store (edge_store.hpp: a contiguous, chronologically sorted run per node).
// Shared by hist_negatives.hip and seen_mask.hip, so that both mean the same thing by "strictly
// before" and "live".
#pragma once

#include <cstdint>

#include <hip/hip_runtime.h>

#include "edge_store.hpp"

namespace gf {

// elements of the ascending run ts[0:n) that are < t (float <: a NaN t gives 0)
__device__ __forceinline__ uint32_t count_before(const float* __restrict__ ts, uint32_t n,
                                                 float t) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;      // < n
    if (ts[mid] < t) lo = mid + 1; else hi = mid;
  }
  return lo;
}

}  // namespace gf
