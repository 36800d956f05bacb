// pair_sequence.hip: everything DyGFormer concatenates for a pair, finished, from one launch --
// neighbor_cooccurrence.hip's two padded sequences with the self slot and their co-occurrence
// counts, the time deltas, and the node-feature, edge-feature and time-encoding channels of every
// slot as three separate contiguous tensors (the model patches and projects each channel on its
// own).  The pair reader with features, where neighbor_sequence.hip is the per-node one.
// Contract: include/gnnflow_hip.h (gf_graph_pair_sequence).
#pragma once

#include <cstddef>
#include <cstdint>

#include <hip/hip_runtime.h>

#include "edge_store.hpp"

namespace gf {

constexpr size_t kPairSeqMaxLength = 512;      // GF_PAIRSEQ_MAX_LENGTH
constexpr size_t kPairSeqMaxWidth = 1024;      // GF_PAIRSEQ_MAX_WIDTH

// d_lengths, d_nodes, d_eids, d_times and d_counts are neighbor_cooccurrence's with include_self
// (neighbor_cooccurrence.hpp), L = length in 2 .. kPairSeqMaxLength.  d_delta_t[i, side, p] =
// d_ts[i] - d_times[i, side, p] on a filled slot (the self slot: d_ts[i] - d_ts[i]), +0.0 in the
// padding.  On a filled slot d_node_out[i, side, p, :] = d_node_feats[d_nodes[i, side, p], :],
// d_edge_out = d_edge_feats[d_eids[i, side, p], :] (zeros for an id without a row: negative, >=
// node_rows / edge_rows; the self slot's eid is -1) and d_time_out[.., j] = cosf(d_weight[j] *
// delta_t + d_bias[j]); every element of a padded slot is +0.0.  A part is absent as (nullptr,
// width 0) and its output is then not touched; widths are 1 .. kPairSeqMaxWidth.  Every element
// of the six planes and of the outputs of the given parts is written.  `g` is the view of the
// store at the time of the call.
void pair_sequence(const GraphView& g, const int64_t* d_src, const int64_t* d_dst,
                   const float* d_ts, const float* d_since, size_t num_rows, size_t length,
                   const float* d_node_feats, size_t node_rows, size_t dn,
                   const float* d_edge_feats, size_t edge_rows, size_t de, const float* d_weight,
                   const float* d_bias, size_t dim_time, int32_t* d_lengths, int64_t* d_nodes,
                   int64_t* d_eids, float* d_times, float* d_delta_t, int32_t* d_counts,
                   float* d_node_out, float* d_edge_out, float* d_time_out, int device,
                   hipStream_t stream);

}  // namespace gf
