// neighbor_aggregate.hip: the sum or the mean of the feature rows of the nodes a node met, and of
// the edges it met them over, inside its history window -- GraphMixer's node encoder and the
// windowed mean-pooling baseline.  The only edge-history reader that touches a feature row.
// Contract: include/gnnflow_hip.h (gf_graph_neighbor_aggregate).
#pragma once

#include <cstddef>
#include <cstdint>

#include <hip/hip_runtime.h>

#include "edge_store.hpp"

namespace gf {

constexpr size_t kAggregateMaxWidth = 1024;      // GF_AGG_MAX_WIDTH

// For row i: over the newest max_history (0: all) edges of d_nodes[i] with
// d_since[i] <= ts < d_ts[i] (d_since == nullptr: no lower end), oldest first, d_count[i] = their
// number n, d_node_out[i, :] = the float32 sum in that order of d_node_feats[record.dst, :] and
// d_edge_out[i, :] that of d_edge_feats[record.eid, :], divided once by float(n) when `mean`
// (zeros when n == 0).  An id without a row in its table (negative, >= node_rows / edge_rows) adds
// a zero row and still counts.  A table is absent as (nullptr, width 0) and its output is then not
// written; at least one is given, of width 1 .. kAggregateMaxWidth, row-major and contiguous.
// Every element of d_count and of the outputs of the given tables is written.  `g` is the view of
// the store at the time of the call.
void neighbor_aggregate(const GraphView& g, const int64_t* d_nodes, const float* d_ts,
                        const float* d_since, size_t num_rows, size_t max_history,
                        const float* d_node_feats, size_t node_rows, size_t dn,
                        const float* d_edge_feats, size_t edge_rows, size_t de, bool mean,
                        int64_t* d_count, float* d_node_out, float* d_edge_out, int device,
                        hipStream_t stream);

}  // namespace gf
