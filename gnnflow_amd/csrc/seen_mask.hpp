// seen_mask.hip: which of C candidate nodes has each of B sources already met — one bit per
// (source, candidate), set where an edge of the source strictly before the row's time leads to
// the candidate.  The history comes from the node's segment of the temporal edge store.
// Contract: include/gnnflow_hip.h (gf_graph_seen_mask).
#pragma once

#include <cstddef>
#include <cstdint>

#include <hip/hip_runtime.h>

#include "edge_store.hpp"

namespace gf {

// ORs into d_mask [num_rows, ceil(num_cand / 64)] (zeroed by the caller) bit perm[j] of row i for
// every j with sorted_ids[j] == the dst of one of the newest max_history (0: all) edges of
// d_src[i] before d_ts[i].  d_sorted_ids ascending, d_perm its positions in the caller's order,
// both [num_cand].  `g` is the view of the store at the time of the call.
void seen_mask(const GraphView& g, const int64_t* d_src, const float* d_ts, size_t num_rows,
               const int64_t* d_sorted_ids, const int64_t* d_perm, size_t num_cand,
               size_t max_history, uint64_t* d_mask, int device, hipStream_t stream);

}  // namespace gf
