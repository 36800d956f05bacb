// Has this pair interacted before, how often, and when last: for row i with source s = src[i],
// destination d = dst[i], time t = ts[i] and, when `since` is given, lower end lo = since[i],
//
//   considered  = the window of s at (t, lo, max_history), as history_window.hpp defines it
//   count[i]    = #{considered records with .dst == d}
//   p           = the largest pool position among them
//   last_ts[i]  = nbr_pool[p].ts,  -inf when count == 0
//   last_eid[i] = nbr_pool[p].eid, -1   when count == 0
//
// Every row's three outputs are written, the rows without a considered edge too.
//
// A wave takes a row at a time, four rows per workgroup, rows past the grid limit grid-strided.
// All lanes resolve the window together (the same addresses: one request), then stride over the
// n records, one 32-byte record per lane, of which .dst is read.  A lane keeps its match count
// and its largest matching index; the wave sums the one and takes the maximum of the other with
// cross-lane shuffles, integers both: the result does not depend on the lane order.  Lane 0 reads
// .ts / .eid of the winner and stores the three values.  Plain loads and stores, no LDS, no
// atomics, no waiting on another workgroup.  The cost is the records read: a hub with 10^6
// earlier edges is 10^6 record reads for its row, by one wave; max_history and since are what
// bound it.
#include "pair_history.hpp"
#include "common.hpp"
#include "history_window.hpp"

namespace gf {
namespace {

using namespace wave_per_row;      // kThreads, kWave, kWaves, kMaxGrid

struct PairArgs {
  StoreView store;           // without a node: every row gets the empty answer
  const int64_t* src;
  const int64_t* dst;
  const float* ts;
  const float* since;        // nullptr: no lower end
  uint64_t rows;
  uint32_t max_history;      // 0: the whole window
  int64_t* count;
  float* last_ts;
  int64_t* last_eid;
};

__global__ void __launch_bounds__(kThreads) pair_history_kernel(const PairArgs a) {
  const uint32_t lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
  const uint64_t step = static_cast<uint64_t>(gridDim.x) * kWaves;
  for (uint64_t row = static_cast<uint64_t>(blockIdx.x) * kWaves + wave; row < a.rows;
       row += step) {                                          // uniform over the wave
    const Window win = window_of(a.store, a.src[row], a.ts[row], a.since, row, a.max_history);
    const EdgePair* const seg = win.seg;
    const uint32_t n = win.n;
    // n is the same in every lane: the wave takes the branches below as one
    uint32_t cnt = 0, best = 0;      // best: 1 + the largest matching index, 0 for none (n < 2^32)
    if (n != 0) {
      const int64_t d = a.dst[row];
      for (uint32_t x = lane; x < n; x += kWave) {
        if (seg[x].dst == d) {
          ++cnt;
          best = x + 1;      // x ascends
        }
      }
      for (int o = kWave / 2; o > 0; o >>= 1) {
        cnt += __shfl_xor(cnt, o);
        const uint32_t other = __shfl_xor(best, o);
        best = other > best ? other : best;
      }
    }
    if (lane == 0) {
      a.count[row] = static_cast<int64_t>(cnt);
      a.last_ts[row] = cnt ? seg[best - 1].ts : __uint_as_float(0xFF800000u);      // -inf
      a.last_eid[row] = cnt ? seg[best - 1].eid : int64_t{-1};
    }
  }
}

}  // namespace

void pair_history(const GraphView& g, const int64_t* d_src, const int64_t* d_dst,
                  const float* d_ts, const float* d_since, size_t num_rows, size_t max_history,
                  int64_t* d_count, float* d_last_ts, int64_t* d_last_eid, int device,
                  hipStream_t stream) {
  const std::string w("pair_history");
  GF_REQUIRE(num_rows < (size_t{1} << 31), w + ": 2^31 rows or more");
  if (num_rows == 0) return;
  GF_REQUIRE(d_src && d_dst && d_ts, w + ": null src, dst or ts");
  GF_REQUIRE(d_count && d_last_ts && d_last_eid, w + ": null count, last_ts or last_eid");
  PairArgs a = {store_view(g), d_src, d_dst, d_ts, d_since, num_rows, history_bound(max_history),
                d_count, d_last_ts, d_last_eid};
  DeviceGuard dg(device);
  pair_history_kernel<<<strided_grid(num_rows, kWaves, kMaxGrid), dim3(kThreads), 0, stream>>>(a);
  GF_HIP(hipGetLastError());
}

}  // namespace gf
