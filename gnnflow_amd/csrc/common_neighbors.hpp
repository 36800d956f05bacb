// common_neighbors.hip: which nodes have both ends of a pair met before the row's time — the
// intersection of two time-windowed histories of the temporal edge store, as a set, with how often
// each side met each common node; and temporal_degree, the size of one node's window.  The inputs
// of the neighbour-overlap baselines (common neighbours, Jaccard, Adamic-Adar, resource
// allocation, preferential attachment) and of common-neighbour models.
// Contract: include/gnnflow_hip.h (gf_graph_common_neighbors, gf_graph_temporal_degree).
#pragma once

#include <cstddef>
#include <cstdint>

#include <hip/hip_runtime.h>

#include "edge_store.hpp"

namespace gf {

constexpr size_t kCnMaxHistory = 512;      // GF_CN_MAX_HISTORY; max_common has the same bound

// For row i: A = the newest max_history edges of d_src[i] with d_since[i] <= ts < d_ts[i]
// (d_since == nullptr: no lower end), B the same of d_dst[i].  d_n_src / d_n_dst = |A|, |B|;
// d_u_src / d_u_dst = distinct non-negative destinations in A, B; d_common = those in both;
// d_nodes[i, :] = the common ones, the one the source met most recently first, the first
// min(common, max_common), then -1; d_cnt_src / d_cnt_dst [i, :] = how often A, B hold that node,
// 0 in the padding.  Every element of the eight outputs is written.  1 <= max_history <=
// kCnMaxHistory, max_common <= kCnMaxHistory.  `g` is the view of the store at the time of the
// call.
void common_neighbors(const GraphView& g, const int64_t* d_src, const int64_t* d_dst,
                      const float* d_ts, const float* d_since, size_t num_rows,
                      size_t max_history, size_t max_common, int32_t* d_n_src, int32_t* d_n_dst,
                      int32_t* d_u_src, int32_t* d_u_dst, int32_t* d_common, int64_t* d_nodes,
                      int32_t* d_cnt_src, int32_t* d_cnt_dst, int device, hipStream_t stream);

// d_out[i] = the number of live edges of d_nodes[i] with d_since[i] <= ts < d_ts[i] (d_since ==
// nullptr: no lower end); 0 for a node that is negative, past the node table or without live edges.
void temporal_degree(const GraphView& g, const int64_t* d_nodes, const float* d_ts,
                     const float* d_since, size_t num, int64_t* d_out, int device,
                     hipStream_t stream);

}  // namespace gf
