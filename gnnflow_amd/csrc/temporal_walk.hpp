// temporal_walk.hip: backward-in-time random walks over the temporal edge store — W walks of L
// steps from each of B roots, every step to an edge of the current node strictly before the
// current time.  walk_positions.hip: the position-count ("anonymous") encoding of such walks.
// Contracts: include/gnnflow_hip.h (gf_graph_temporal_walks, gf_walk_position_counts).
#pragma once

#include <cstddef>
#include <cstdint>

#include <hip/hip_runtime.h>

#include "edge_store.hpp"

namespace gf {

constexpr size_t kWalkMaxLength = 32;          // GF_WALK_MAX_LENGTH
constexpr size_t kWalkMaxRecency = 8;          // GF_WALK_MAX_RECENCY
constexpr size_t kWalkMaxRefEntries = 4096;    // GF_WALK_MAX_REF_ENTRIES

// Writes d_nodes [num_rows, num_walks, length + 1], d_eids and d_times [num_rows, num_walks,
// length], every element: walk (i, w) starts at d_src[i] at time d_ts[i] and takes, per step, one
// of the newest max_history (0: all) edges of its node before its time, the maximum of `recency`
// Philox draws; from the step it ends on its slots hold -1, -1 and 0.  `g` is the view of the
// store at the time of the call.
void temporal_walks(const GraphView& g, const int64_t* d_src, const float* d_ts, size_t num_rows,
                    size_t num_walks, size_t length, size_t recency, size_t max_history,
                    uint64_t seed, uint64_t epoch, uint64_t first_row, int64_t* d_nodes,
                    int64_t* d_eids, float* d_times, int device, hipStream_t stream);

// d_out [rows, walks, len1, ref_len1] (int32) = how often d_nodes[i, w, j] (int64 [rows, walks,
// len1]) stands at position p of the ref_walks walks d_ref[i] (int64 [rows, ref_walks, ref_len1]);
// a negative node counts nothing.
void walk_position_counts(const int64_t* d_nodes, const int64_t* d_ref, size_t rows, size_t walks,
                          size_t len1, size_t ref_walks, size_t ref_len1, int32_t* d_out,
                          int device, hipStream_t stream);

}  // namespace gf
