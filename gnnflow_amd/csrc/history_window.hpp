// "The edges of a node strictly before t": the one statement of the history window that the
// edge-history readers share (hist_negatives.hip, seen_mask.hip, pair_history.hip,
// temporal_walk.hip, common_neighbors.hip with temporal_degree, neighbor_cooccurrence.hip,
// neighbor_aggregate.hip, neighbor_sequence.hip, pair_sequence.hip).  The store keeps one
// contiguous, chronologically sorted run per node (edge_store.hpp); for node v, time t, optional
// lower end lo and bound H (max_history, 0: none):
//
//   e  = table[v]                 v < 0, v >= table_len, e.size == 0: the window is empty
//   c  = #{x in ts_pool[e.start .. e.start + e.size) : x < t}        float <: NaN t gives 0
//   c0 = lo given ? min(c, #{x : x < lo}) : 0                        float <: NaN lo gives 0
//   n  = H ? min(c - c0, H) : c - c0
//   considered = nbr_pool[e.start + c - n .. e.start + c)            lo <= ts < t, the newest n,
//                                                                    oldest first
//
// The upper end is exclusive: an edge at t itself (a tie) is not considered, and a NaN t considers
// nothing.  The lower end is inclusive, and a NaN lo is no lower end; lo > t gives c0 = c, an
// empty window.  H applies after lo.  "Live" is what the node's entry spans now: edges that
// offload_old_blocks took are gone, and on a store built with reverse edges a node's run also
// holds the edges that pointed at it.  The last_ts_bits shortcut (t later than the node's newest
// edge: c = e.size) is the search's answer without the search.
//
// Inside the run: count_before returns at most e.size, so c0 <= c <= e.size and n <= c - c0 <= c;
// the considered records start at e.start + (c - n) >= e.start and end at e.start + c <=
// e.start + e.size.  A reader that indexes seg[0 .. n) stays inside the node's run.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>

#include <hip/hip_runtime.h>

#include "edge_store.hpp"

namespace gf {

// What the readers use of a GraphView; the leading member of each reader's argument struct.
struct StoreView {
  const NodeEntry* table;
  uint64_t table_len;        // 0: a store without a node, every window is empty
  const float* ts_pool;
  const EdgePair* nbr_pool;
};

// the only place that decides a store is empty
inline StoreView store_view(const GraphView& g) {
  const bool empty = g.table_len == 0 || g.table == nullptr || g.ts_pool == nullptr ||
                     g.nbr_pool == nullptr;
  return {g.table, empty ? 0 : g.table_len, g.ts_pool, g.nbr_pool};
}

// H of a caller's max_history: a node's run holds fewer than 2^32 edges, a larger bound is no bound
inline uint32_t history_bound(size_t max_history) {
  return max_history > 0xFFFFFFFFull ? 0u : static_cast<uint32_t>(max_history);
}

// workgroups for `items` (rows, walks, elements) taken `per_group` at a time; the items past
// `max_groups` workgroups are grid-strided by the kernel
inline dim3 strided_grid(uint64_t items, uint32_t per_group, uint32_t max_groups) {
  const uint64_t groups = (items + per_group - 1) / per_group;
  return dim3(static_cast<uint32_t>(std::min<uint64_t>(groups, max_groups)));
}

// The geometry of the readers in which a wave takes a row at a time (seen_mask.hip,
// pair_history.hip, neighbor_aggregate.hip, neighbor_sequence.hip), which launch
// strided_grid(rows, kWaves, kMaxGrid) workgroups of kThreads.  The other readers have their own.
namespace wave_per_row {
constexpr int kThreads = 256;
constexpr int kWave = 64;
constexpr int kWaves = kThreads / kWave;      // rows a workgroup works on at a time
constexpr uint32_t kMaxGrid = 4096;           // rows past kMaxGrid * kWaves are grid-strided
}  // namespace wave_per_row

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

// e, c and c0 of node v's window at time t; the lower end is since[row], none when since is
// nullptr.  false, with c = c0 = 0 and e not set, for a node without a window: e is read only
// after a true return.
[[nodiscard]] __device__ __forceinline__ bool window_counts(const StoreView& s, int64_t v,
                                                            float t, const float* since,
                                                            uint64_t row, NodeEntry& e,
                                                            uint32_t& c, uint32_t& c0) {
  c = c0 = 0;
  if (v < 0 || static_cast<uint64_t>(v) >= s.table_len) return false;
  e = s.table[v];
  if (e.size == 0) return false;
  const float* const run = s.ts_pool + e.start;
  c = t > __uint_as_float(e.last_ts_bits) ? e.size : count_before(run, e.size, t);   // <= e.size
  if (since != nullptr && c != 0) {
    c0 = count_before(run, e.size, since[row]);
    if (c0 > c) c0 = c;
  }
  return true;
}

struct Window {
  const EdgePair* seg;       // seg[0 .. n) are the considered records, oldest first
  uint32_t n;                // 0: seg is not to be read (nullptr for a node without a window)
};

// the considered records of node v; max_history == 0: no bound
__device__ __forceinline__ Window window_of(const StoreView& s, int64_t v, float t,
                                            const float* since, uint64_t row,
                                            uint32_t max_history) {
  NodeEntry e;
  uint32_t c, c0;
  Window w = {nullptr, 0};
  if (window_counts(s, v, t, since, row, e, c, c0)) {
    w.n = c - c0;
    if (max_history && max_history < w.n) w.n = max_history;
    w.seg = s.nbr_pool + e.start + (c - w.n);      // inside the run: header comment
  }
  return w;
}

}  // namespace gf
