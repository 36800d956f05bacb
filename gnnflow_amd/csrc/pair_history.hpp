// pair_history.hip: did this (source, destination) pair interact before the row's time, how
// often, and when last — three scalars per row, read from the source's segment of the temporal
// edge store.  The question EdgeBank asks, and the usual hand-made pair features.
// Contract: include/gnnflow_hip.h (gf_graph_pair_history).
#pragma once

#include <cstddef>
#include <cstdint>

#include <hip/hip_runtime.h>

#include "edge_store.hpp"

namespace gf {

// For row i: among the newest max_history (0: all) edges of d_src[i] with
// d_since[i] <= ts < d_ts[i] (d_since == nullptr: no lower end), d_count[i] = those that lead to
// d_dst[i], d_last_ts[i] / d_last_eid[i] = timestamp and edge id of the latest of them in the
// store's order (-inf / -1 when there is none).  Every element of the three outputs is written.
// `g` is the view of the store at the time of the call.
void pair_history(const GraphView& g, const int64_t* d_src, const int64_t* d_dst,
                  const float* d_ts, const float* d_since, size_t num_rows, size_t max_history,
                  int64_t* d_count, float* d_last_ts, int64_t* d_last_eid, int device,
                  hipStream_t stream);

}  // namespace gf
