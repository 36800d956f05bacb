// neighbor_cooccurrence.hip: the pair inputs of the sequence-based temporal models (DyGFormer,
// GraphMixer) -- the most recent interactions of both ends of a pair as two padded sequences of
// node id, edge id and time, and for every element of either sequence how often that node occurs
// in the source's sequence and how often in the destination's (DyGFormer's neighbour
// co-occurrence encoding).
// Contract: include/gnnflow_hip.h (gf_graph_neighbor_cooccurrence).
#pragma once

#include <cstddef>
#include <cstdint>

#include <hip/hip_runtime.h>

#include "edge_store.hpp"

namespace gf {

constexpr size_t kCoocMaxLength = 512;      // GF_COOC_MAX_LENGTH

// For row i, with self = include_self ? 1 : 0 and H = length - self >= 1: seq(v) = [v if self] +
// the destinations of the newest H edges of v with d_since[i] <= ts < d_ts[i] (d_since == nullptr:
// no lower end), oldest first.  Side 0 is d_src[i]'s, side 1 d_dst[i]'s.  d_lengths[i, side] =
// |seq|; d_nodes / d_eids / d_times [i, side, :] = the sequence's nodes, edge ids (-1 for the self
// slot) and times (d_ts[i] for the self slot), then -1 / -1 / 0; d_counts[i, side, p, 0 / 1] = how
// often d_nodes[i, side, p] occurs in side 0's / side 1's sequence, 0 for a negative node and in
// the padding.  Every element of the five outputs is written.  1 + self <= length <=
// kCoocMaxLength.  `g` is the view of the store at the time of the call.
void neighbor_cooccurrence(const GraphView& g, const int64_t* d_src, const int64_t* d_dst,
                           const float* d_ts, const float* d_since, size_t num_rows,
                           size_t length, bool include_self, int32_t* d_lengths,
                           int64_t* d_nodes, int64_t* d_eids, float* d_times, int32_t* d_counts,
                           int device, hipStream_t stream);

}  // namespace gf
