// hist_negatives.hip: historical negatives for batches that batch_stream.hip has assembled —
// destinations the source interacted with strictly before the edge's time, drawn by Philox
// from the node's segment of the temporal edge store.  Contract: include/gnnflow_hip.h
// (gf_batch_hist_negatives).
#pragma once

#include <cstddef>
#include <cstdint>

#include <hip/hip_runtime.h>

#include "edge_store.hpp"

namespace gf {

constexpr int kHistNegAttempts = 4;      // draws per slot before the random negative is kept

// Overwrites the first hist_ratio negative planes of num_batches assembled batches (borders
// and slices as batch_assemble_many) where a historical negative exists.  `g` is the view of
// the store at the time of the call.
void batch_hist_negatives(const GraphView& g, const int64_t* d_src, const int64_t* d_dst,
                          const float* d_time, size_t num_rows, const int64_t* d_borders,
                          size_t num_batches, size_t max_batch_rows, size_t neg_ratio,
                          size_t hist_ratio, uint64_t seed, uint64_t epoch, uint64_t first_row,
                          int64_t* d_roots, size_t capacity, uint64_t* d_filled, int device,
                          hipStream_t stream);

}  // namespace gf
