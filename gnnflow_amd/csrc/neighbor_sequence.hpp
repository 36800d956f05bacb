// neighbor_sequence.hip: a node's newest interactions as one padded sequence of node id, edge id,
// time and time delta, and optionally the finished [edge features | node features | time encoding]
// tokens of the sequence-based temporal models (GraphMixer's link encoder, DyGFormer, TCL) -- the
// per-node reader, where neighbor_cooccurrence.hip reads the two ends of a pair.
// Contract: include/gnnflow_hip.h (gf_graph_neighbor_sequence).
#pragma once

#include <cstddef>
#include <cstdint>

#include <hip/hip_runtime.h>

#include "edge_store.hpp"

namespace gf {

constexpr size_t kSeqMaxLength = 512;      // GF_SEQ_MAX_LENGTH
constexpr size_t kSeqMaxWidth = 1024;      // GF_SEQ_MAX_WIDTH

// For row i, over the newest `length` edges of d_nodes[i] with d_since[i] <= ts < d_ts[i]
// (d_since == nullptr: no lower end), oldest first, n of them: d_lengths[i] = n; for p < n
// d_out_nodes / d_eids / d_times [i, p] are the record's dst, eid and ts and d_delta_t[i, p] =
// d_ts[i] - ts (one float32 subtraction); for p >= n they are -1, -1, 0, 0.  d_tokens[i, p, :] =
// [d_edge_feats[eid, :] | d_node_feats[dst, :] | cosf(d_weight[j] * delta_t + d_bias[j])], a table
// part zero for an id without a row (negative, >= edge_rows / node_rows), and all of it +0.0 for
// p >= n.  A part is absent as (nullptr, width 0); d_tokens is written when a part is given.
// Widths are 1 .. kSeqMaxWidth, 1 <= length <= kSeqMaxLength.  Every element of the outputs is
// written.  `g` is the view of the store at the time of the call.
void neighbor_sequence(const GraphView& g, const int64_t* d_nodes, const float* d_ts,
                       const float* d_since, size_t num_rows, size_t length,
                       const float* d_edge_feats, size_t edge_rows, size_t de,
                       const float* d_node_feats, size_t node_rows, size_t dn,
                       const float* d_weight, const float* d_bias, size_t dim_time,
                       int32_t* d_lengths, int64_t* d_out_nodes, int64_t* d_eids, float* d_times,
                       float* d_delta_t, float* d_tokens, int device, hipStream_t stream);

}  // namespace gf
