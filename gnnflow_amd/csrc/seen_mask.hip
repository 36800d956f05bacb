// Which candidates has each source already met: for row i with source s = src[i] and time
// t = ts[i], and a candidate list of C node ids (any order, duplicates allowed),
//
//   considered = the window of s at (t, no lower end, max_history), as history_window.hpp
//                defines it; empty: the row stays zero
//   mask[i, p / 64] |= 1 << (p % 64)       for every p with cand_ids[p] == r.dst, r considered
//
// The candidates arrive sorted with the permutation that sorted them (sorted_ids, perm), so that
// a destination is found with one lower bound and its duplicates are the equal entries behind it.
//
// A wave takes a row at a time, four rows per workgroup, rows past the grid limit grid-strided.
// All lanes resolve the window together (the same addresses: one request), then stride over the
// n records, one 32-byte record per lane.  Plain loads, no waiting on another workgroup, no LDS;
// atomicOr on the mask's 64-bit words is the only atomic, and OR is commutative and idempotent:
// the same inputs give the same bits.  The cost is the records read: a hub with 10^6 earlier
// edges is 10^6 record reads and lower bounds for its row, by one wave; max_history bounds it.
#include "seen_mask.hpp"
#include "common.hpp"
#include "history_window.hpp"

namespace gf {
namespace {

using namespace wave_per_row;      // kThreads, kWave, kWaves, kMaxGrid

struct SeenArgs {
  StoreView store;
  const int64_t* src;
  const float* ts;
  uint64_t rows;
  const int64_t* sorted_ids;
  const int64_t* perm;
  uint32_t C, W;
  uint32_t max_history;      // 0: the whole history
  unsigned long long* mask;  // [rows, W]
};

// first j in [0, n) with ids[j] >= x, n if none
__device__ __forceinline__ uint32_t lower_bound(const int64_t* __restrict__ ids, uint32_t n,
                                                int64_t x) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;      // < n
    if (ids[mid] < x) lo = mid + 1; else hi = mid;
  }
  return lo;
}

__global__ void __launch_bounds__(kThreads) seen_mask_kernel(const SeenArgs a) {
  const uint32_t lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
  const uint64_t step = static_cast<uint64_t>(gridDim.x) * kWaves;
  for (uint64_t row = static_cast<uint64_t>(blockIdx.x) * kWaves + wave; row < a.rows;
       row += step) {                                          // uniform over the wave
    const Window win = window_of(a.store, a.src[row], a.ts[row], nullptr, 0, a.max_history);
    if (win.n == 0) continue;
    unsigned long long* const out = a.mask + row * a.W;
    for (uint32_t x = lane; x < win.n; x += kWave) {
      const int64_t d = win.seg[x].dst;
      for (uint32_t j = lower_bound(a.sorted_ids, a.C, d); j < a.C && a.sorted_ids[j] == d; ++j) {
        const int64_t p = a.perm[j];
        if (p < 0 || p >= static_cast<int64_t>(a.C)) continue;      // not a permutation: no bit
        const unsigned long long bit = 1ull << (p & 63);
        // a repeated destination finds its bit set: bits are only ever set, so a stale 0 costs
        // one redundant OR and a 1 is final
        if (!(out[p >> 6] & bit)) atomicOr(out + (p >> 6), bit);      // p >> 6 < W
      }
    }
  }
}

}  // namespace

void seen_mask(const GraphView& g, const int64_t* d_src, const float* d_ts, size_t num_rows,
               const int64_t* d_sorted_ids, const int64_t* d_perm, size_t num_cand,
               size_t max_history, uint64_t* d_mask, int device, hipStream_t stream) {
  const std::string w("seen_mask");
  GF_REQUIRE(num_cand >= 1, w + ": needs at least one candidate");
  GF_REQUIRE(num_cand < (size_t{1} << 31), w + ": 2^31 candidates or more");
  GF_REQUIRE(num_rows < (size_t{1} << 31), w + ": 2^31 rows or more");
  if (num_rows == 0) return;
  GF_REQUIRE(d_src && d_ts, w + ": null src or ts");
  GF_REQUIRE(d_sorted_ids && d_perm, w + ": null sorted_ids or perm");
  GF_REQUIRE(d_mask != nullptr, w + ": null mask");
  const StoreView store = store_view(g);
  if (store.table_len == 0) return;      // no history: every row stays zero
  const uint32_t C = static_cast<uint32_t>(num_cand);
  SeenArgs a = {store, d_src, d_ts, num_rows, d_sorted_ids, d_perm, C, (C + 63) / 64,
                history_bound(max_history), reinterpret_cast<unsigned long long*>(d_mask)};
  DeviceGuard dg(device);
  seen_mask_kernel<<<strided_grid(num_rows, kWaves, kMaxGrid), dim3(kThreads), 0, stream>>>(a);
  GF_HIP(hipGetLastError());
}

}  // namespace gf
