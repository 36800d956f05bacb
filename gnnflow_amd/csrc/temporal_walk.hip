// Backward-in-time random walks over the temporal edge store (edge_store.hpp: one contiguous,
// chronologically sorted run per node).  Walk (i, w), w < W, starts at v_0 = src[i], t_0 = ts[i];
// nodes[i, w, 0] = src[i] always, and for step j = 0 .. L - 1:
//
//   seg[0 .. n) = the window of v_j at (t_j, no lower end, max_history), as history_window.hpp
//          defines it                                                 n == 0: the walk has ended
//   u_a  = gf_philox4x32_10_first(seed ^ (GF_WALK_SEED_TAG + a), tid, (epoch << 8) + j)   a < recency
//   x    = max over a of ((uint64(u_a) * n) >> 32)                    0 <= x < n
//   r    = seg[x]
//   nodes[i, w, j + 1] = r.dst;  eids[i, w, j] = r.eid;  times[i, w, j] = r.ts
//   v_{j+1} = r.dst;  t_{j+1} = r.ts              tid = (first_row + i) * W + w  (wraps)
//
// Every slot from the step a walk ends on holds nodes = -1, eids = -1, times = 0, so the kernel
// writes every element of the three outputs.  The window is resolved again at every step, and its
// bounds test is what checks a record's dst before it indexes the table as the next v; time
// strictly decreases along a walk.
//
// One lane per walk, consecutive lanes consecutive w of one root: a walk is a chain of up to 3 L
// dependent random reads (node entry, timestamp search, one 32-byte record), so the kernel lives
// on the number of walks in flight, and step 0's node entry and search are the same addresses for
// the lanes of a root: one request per wave while a root fills it.  A workgroup is one wave:
// walks share nothing, and a small call spreads over more CUs that way.  Plain loads and stores,
// no atomics, no LDS, no waiting on another workgroup.
//
// The outputs are written per lane, not staged in LDS.  A walk's rows are (L + 1) * 8, L * 8 and
// L * 4 bytes and the rows of a wave's 64 walks are adjacent, so over the L steps the wave writes
// three contiguous ranges in full, which the L2 merges into whole lines before they leave for
// HBM; a staged form needs 20 L + 8 bytes of LDS per lane (41 KB per wave at L = 32) and would
// bound the waves per CU, the one thing a latency-bound chain needs.
#include "temporal_walk.hpp"
#include "common.hpp"
#include "history_window.hpp"

#include "../../include/gnnflow_rng.h"

namespace gf {
namespace {

constexpr int kThreads = 64;              // one wave
// 8 waves per SIMD on 256 CUs: what can be resident at once; walks past kMaxGrid * kThreads
// are grid-strided
constexpr uint32_t kMaxGrid = 8192;

static_assert(kWalkMaxLength == GF_WALK_MAX_LENGTH && kWalkMaxRecency == GF_WALK_MAX_RECENCY,
              "gnnflow_hip.h and temporal_walk.hpp disagree on the walk limits");

struct WalkArgs {
  StoreView store;           // without a node: every walk ends on step 0
  const int64_t* src;
  const float* ts;
  uint64_t walks;            // B * W < 2^31
  uint32_t W, L, recency;
  uint32_t max_history;      // 0: the whole history
  uint64_t seed, epoch, first_row;
  int64_t* nodes;            // [walks, L + 1]
  int64_t* eids;             // [walks, L]
  float* times;              // [walks, L]
};

__global__ void __launch_bounds__(kThreads) temporal_walk_kernel(const WalkArgs a) {
  const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kThreads;
  for (uint64_t g = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x; g < a.walks;
       g += stride) {
    const uint64_t i = g / a.W;                                // < B
    const uint64_t w = g - i * a.W;                            // < W
    const uint64_t tid = (a.first_row + i) * a.W + w;          // wraps mod 2^64
    int64_t v = a.src[i];
    float t = a.ts[i];
    int64_t* const nodes = a.nodes + g * (a.L + 1);            // g * (L + 1) + j < walks * (L + 1)
    int64_t* const eids = a.eids + g * a.L;                    // g * L + j < walks * L
    float* const times = a.times + g * a.L;
    nodes[0] = v;
    bool alive = true;
    for (uint32_t j = 0; j < a.L; ++j) {
      int64_t nd = -1, ne = -1;
      float nt = 0.0f;
      // v is a record's dst from step 1 on: window_of checks it before it indexes the table
      const Window win = alive ? window_of(a.store, v, t, nullptr, 0, a.max_history)
                               : Window{nullptr, 0};
      alive = win.n != 0;
      if (alive) {
        const uint64_t call = (a.epoch << 8) + j;              // wraps mod 2^64
        uint32_t x = 0;
        for (uint32_t p = 0; p < a.recency; ++p) {
          const uint64_t u = gf_philox4x32_10_first(
              a.seed ^ (GF_WALK_SEED_TAG + static_cast<uint64_t>(p)), tid, call);
          const uint32_t xp = static_cast<uint32_t>((u * win.n) >> 32);      // < n
          x = xp > x ? xp : x;
        }
        const EdgePair* const r = win.seg + x;                 // x < n: inside the window
        nd = r->dst;
        ne = r->eid;
        nt = r->ts;
        v = nd;
        t = nt;
      }
      nodes[j + 1] = nd;                                       // j + 1 <= L
      eids[j] = ne;                                            // j < L
      times[j] = nt;
    }
  }
}

}  // namespace

void temporal_walks(const GraphView& g, const int64_t* d_src, const float* d_ts, size_t num_rows,
                    size_t num_walks, size_t length, size_t recency, size_t max_history,
                    uint64_t seed, uint64_t epoch, uint64_t first_row, int64_t* d_nodes,
                    int64_t* d_eids, float* d_times, int device, hipStream_t stream) {
  const std::string w("temporal_walks");
  GF_REQUIRE(length >= 1 && length <= kWalkMaxLength, w + ": length outside [1, 32]");
  GF_REQUIRE(num_walks >= 1 && num_walks < (size_t{1} << 16), w + ": num_walks outside [1, 65535]");
  GF_REQUIRE(recency >= 1 && recency <= kWalkMaxRecency, w + ": recency outside [1, 8]");
  GF_REQUIRE(num_rows < (size_t{1} << 31) && num_rows * num_walks < (size_t{1} << 31),
             w + ": 2^31 walks or more");
  if (num_rows == 0) return;
  GF_REQUIRE(d_src && d_ts, w + ": null src or ts");
  GF_REQUIRE(d_nodes && d_eids && d_times, w + ": null nodes, eids or times");
  const uint64_t walks = static_cast<uint64_t>(num_rows) * num_walks;
  WalkArgs a = {store_view(g), d_src, d_ts, walks, static_cast<uint32_t>(num_walks),
                static_cast<uint32_t>(length), static_cast<uint32_t>(recency),
                history_bound(max_history), seed, epoch, first_row, d_nodes, d_eids, d_times};
  DeviceGuard dg(device);
  temporal_walk_kernel<<<strided_grid(walks, kThreads, kMaxGrid), dim3(kThreads), 0, stream>>>(a);
  GF_HIP(hipGetLastError());
}

}  // namespace gf
