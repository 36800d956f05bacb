// extern "C" entry points of include/gnnflow_hip.h over EdgeStore: gf_graph_* and the one
// batch call that reads the store, gf_batch_hist_negatives.
#include "capi_handles.hpp"
#include "common_neighbors.hpp"
#include "hist_negatives.hpp"
#include "neighbor_aggregate.hpp"
#include "neighbor_cooccurrence.hpp"
#include "neighbor_sequence.hpp"
#include "pair_history.hpp"
#include "pair_sequence.hpp"
#include "seen_mask.hpp"
#include "temporal_walk.hpp"

extern "C" {

int gf_graph_create(gf_graph** out, size_t initial_pool_size, size_t maximum_pool_size,
                    int mem_resource_type, size_t minium_block_size,
                    size_t blocks_to_preallocate, int insertion_policy, int device,
                    int adaptive_block_size) {
  return guarded([&] {
    GF_REQUIRE(out != nullptr, "gf_graph_create: null out");
    *out = new gf_graph(initial_pool_size, maximum_pool_size, mem_resource_type,
                        minium_block_size, blocks_to_preallocate, insertion_policy, device,
                        adaptive_block_size != 0);
  });
}
int gf_graph_destroy(gf_graph* g) { return destroy_handle(g); }
int gf_graph_add_edges(gf_graph* g, const int64_t* src, const int64_t* dst, const float* ts,
                       const int64_t* eids, size_t n) {
  return guarded([&] { GF_G(g); g->impl.add_edges(src, dst, ts, eids, n); });
}
int gf_graph_offload_old_blocks(gf_graph* g, float timestamp, int to_file, size_t* num_blocks) {
  return guarded([&] {
    GF_G(g);
    size_t n = g->impl.offload_old_blocks(timestamp, to_file != 0);
    if (num_blocks) *num_blocks = n;
  });
}
int gf_graph_num_vertices(const gf_graph* g, size_t* out) {
  return guarded([&] { GF_G(g); *out = g->impl.num_nodes(); });
}
int gf_graph_num_source_vertices(const gf_graph* g, size_t* out) {
  return guarded([&] { GF_G(g); *out = g->impl.num_src_nodes(); });
}
int gf_graph_num_edges(const gf_graph* g, size_t* out) {
  return guarded([&] { GF_G(g); *out = g->impl.num_edges(); });
}
int gf_graph_max_vertex_id(const gf_graph* g, int64_t* out) {
  return guarded([&] { GF_G(g); *out = g->impl.max_node_id(); });
}
int gf_graph_ids_fit_u32(const gf_graph* g, int* out) {
  return guarded([&] { GF_G(g); *out = g->impl.ids_fit_u32() ? 1 : 0; });
}
int gf_graph_out_degree(const gf_graph* g, const int64_t* nodes, size_t n, size_t* out) {
  return guarded([&] { GF_G(g); g->impl.out_degree(nodes, n, out); });
}
int gf_graph_nodes(const gf_graph* g, int64_t* out, size_t capacity, size_t* count) {
  return guarded([&] { GF_G(g); *count = g->impl.nodes(out, capacity, false); });
}
int gf_graph_src_nodes(const gf_graph* g, int64_t* out, size_t capacity, size_t* count) {
  return guarded([&] { GF_G(g); *count = g->impl.nodes(out, capacity, true); });
}
int gf_graph_edges(const gf_graph* g, int64_t* out, size_t capacity, size_t* count) {
  return guarded([&] { GF_G(g); *count = g->impl.edges(out, capacity); });
}
int gf_graph_get_temporal_neighbors(const gf_graph* g, int64_t node, int64_t* dst, float* ts,
                                    int64_t* eids, size_t capacity, size_t* count) {
  return guarded([&] { GF_G(g); *count = g->impl.get_temporal_neighbors(node, dst, ts, eids, capacity); });
}
int gf_graph_avg_linked_list_length(const gf_graph* g, float* out) {
  return guarded([&] { GF_G(g); *out = g->impl.avg_linked_list_length(); });
}
int gf_graph_memory_usage(const gf_graph* g, float* out) {
  return guarded([&] { GF_G(g); *out = g->impl.graph_mem_usage(); });
}
int gf_graph_metadata_memory_usage(const gf_graph* g, float* out) {
  return guarded([&] { GF_G(g); *out = g->impl.metadata_mem_usage(); });
}
int gf_graph_device(const gf_graph* g, int* out) {
  return guarded([&] { GF_G(g); *out = g->impl.device(); });
}
// reads the store's view NOW: ordered against add_edges / offload_old_blocks by the caller
int gf_batch_hist_negatives(const gf_graph* g, const int64_t* d_src, const int64_t* d_dst,
                            const float* d_time, size_t num_rows, const int64_t* d_borders,
                            size_t num_batches, size_t max_batch_rows, size_t neg_ratio,
                            size_t hist_ratio, uint64_t seed, uint64_t epoch, uint64_t first_row,
                            int64_t* d_roots, size_t capacity, uint64_t* d_filled, int device,
                            void* stream) {
  return guarded([&] {
    GF_G(g);
    gf::batch_hist_negatives(g->impl.view(), d_src, d_dst, d_time, num_rows, d_borders,
                             num_batches, max_batch_rows, neg_ratio, hist_ratio, seed, epoch,
                             first_row, d_roots, capacity, d_filled, device, as_stream(stream));
  });
}
// reads the store's view NOW, as gf_batch_hist_negatives does
int gf_graph_seen_mask(const gf_graph* g, const int64_t* d_src, const float* d_ts, size_t num_rows,
                       const int64_t* d_sorted_ids, const int64_t* d_perm, size_t num_cand,
                       size_t max_history, uint64_t* d_mask, int device, void* stream) {
  return guarded([&] {
    GF_G(g);
    gf::seen_mask(g->impl.view(), d_src, d_ts, num_rows, d_sorted_ids, d_perm, num_cand,
                  max_history, d_mask, device, as_stream(stream));
  });
}
// reads the store's view NOW, as gf_batch_hist_negatives does
int gf_graph_pair_history(const gf_graph* g, const int64_t* d_src, const int64_t* d_dst,
                          const float* d_ts, const float* d_since, size_t num_rows,
                          size_t max_history, int64_t* d_count, float* d_last_ts,
                          int64_t* d_last_eid, int device, void* stream) {
  return guarded([&] {
    GF_G(g);
    gf::pair_history(g->impl.view(), d_src, d_dst, d_ts, d_since, num_rows, max_history, d_count,
                     d_last_ts, d_last_eid, device, as_stream(stream));
  });
}
// reads the store's view NOW, as gf_batch_hist_negatives does
int gf_graph_common_neighbors(const gf_graph* g, const int64_t* d_src, const int64_t* d_dst,
                              const float* d_ts, const float* d_since, size_t num_rows,
                              size_t max_history, size_t max_common, int32_t* d_n_src,
                              int32_t* d_n_dst, int32_t* d_u_src, int32_t* d_u_dst,
                              int32_t* d_common, int64_t* d_nodes, int32_t* d_cnt_src,
                              int32_t* d_cnt_dst, int device, void* stream) {
  return guarded([&] {
    GF_G(g);
    gf::common_neighbors(g->impl.view(), d_src, d_dst, d_ts, d_since, num_rows, max_history,
                         max_common, d_n_src, d_n_dst, d_u_src, d_u_dst, d_common, d_nodes,
                         d_cnt_src, d_cnt_dst, device, as_stream(stream));
  });
}
// reads the store's view NOW, as gf_batch_hist_negatives does
int gf_graph_temporal_degree(const gf_graph* g, const int64_t* d_nodes, const float* d_ts,
                             const float* d_since, size_t num, int64_t* d_out, int device,
                             void* stream) {
  return guarded([&] {
    GF_G(g);
    gf::temporal_degree(g->impl.view(), d_nodes, d_ts, d_since, num, d_out, device,
                        as_stream(stream));
  });
}
// reads the store's view NOW, as gf_batch_hist_negatives does
int gf_graph_neighbor_cooccurrence(const gf_graph* g, const int64_t* d_src, const int64_t* d_dst,
                                   const float* d_ts, const float* d_since, size_t num_rows,
                                   size_t length, int include_self, int32_t* d_lengths,
                                   int64_t* d_nodes, int64_t* d_eids, float* d_times,
                                   int32_t* d_counts, int device, void* stream) {
  return guarded([&] {
    GF_G(g);
    gf::neighbor_cooccurrence(g->impl.view(), d_src, d_dst, d_ts, d_since, num_rows, length,
                              include_self != 0, d_lengths, d_nodes, d_eids, d_times, d_counts,
                              device, as_stream(stream));
  });
}
// reads the store's view NOW, as gf_batch_hist_negatives does
int gf_graph_neighbor_aggregate(const gf_graph* g, const int64_t* d_nodes, const float* d_ts,
                                const float* d_since, size_t num_rows, size_t max_history,
                                const float* d_node_feats, size_t node_rows, size_t dn,
                                const float* d_edge_feats, size_t edge_rows, size_t de, int mean,
                                int64_t* d_count, float* d_node_out, float* d_edge_out,
                                int device, void* stream) {
  return guarded([&] {
    GF_G(g);
    gf::neighbor_aggregate(g->impl.view(), d_nodes, d_ts, d_since, num_rows, max_history,
                           d_node_feats, node_rows, dn, d_edge_feats, edge_rows, de, mean != 0,
                           d_count, d_node_out, d_edge_out, device, as_stream(stream));
  });
}
// reads the store's view NOW, as gf_batch_hist_negatives does
int gf_graph_neighbor_sequence(const gf_graph* g, const int64_t* d_nodes, const float* d_ts,
                               const float* d_since, size_t num_rows, size_t length,
                               const float* d_edge_feats, size_t edge_rows, size_t de,
                               const float* d_node_feats, size_t node_rows, size_t dn,
                               const float* d_weight, const float* d_bias, size_t dim_time,
                               int32_t* d_lengths, int64_t* d_out_nodes, int64_t* d_eids,
                               float* d_times, float* d_delta_t, float* d_tokens, int device,
                               void* stream) {
  return guarded([&] {
    GF_G(g);
    gf::neighbor_sequence(g->impl.view(), d_nodes, d_ts, d_since, num_rows, length, d_edge_feats,
                          edge_rows, de, d_node_feats, node_rows, dn, d_weight, d_bias, dim_time,
                          d_lengths, d_out_nodes, d_eids, d_times, d_delta_t, d_tokens, device,
                          as_stream(stream));
  });
}
// reads the store's view NOW, as gf_batch_hist_negatives does
int gf_graph_pair_sequence(const gf_graph* g, const int64_t* d_src, const int64_t* d_dst,
                           const float* d_ts, const float* d_since, size_t num_rows,
                           size_t length, const float* d_node_feats, size_t node_rows, size_t dn,
                           const float* d_edge_feats, size_t edge_rows, size_t de,
                           const float* d_weight, const float* d_bias, size_t dim_time,
                           int32_t* d_lengths, int64_t* d_nodes, int64_t* d_eids, float* d_times,
                           float* d_delta_t, int32_t* d_counts, float* d_node_out,
                           float* d_edge_out, float* d_time_out, int device, void* stream) {
  return guarded([&] {
    GF_G(g);
    gf::pair_sequence(g->impl.view(), d_src, d_dst, d_ts, d_since, num_rows, length,
                      d_node_feats, node_rows, dn, d_edge_feats, edge_rows, de, d_weight, d_bias,
                      dim_time, d_lengths, d_nodes, d_eids, d_times, d_delta_t, d_counts,
                      d_node_out, d_edge_out, d_time_out, device, as_stream(stream));
  });
}
// reads the store's view NOW, as gf_batch_hist_negatives does
int gf_graph_temporal_walks(const gf_graph* g, const int64_t* d_src, const float* d_ts,
                            size_t num_rows, size_t num_walks, size_t length, size_t recency,
                            size_t max_history, uint64_t seed, uint64_t epoch, uint64_t first_row,
                            int64_t* d_nodes, int64_t* d_eids, float* d_times, int device,
                            void* stream) {
  return guarded([&] {
    GF_G(g);
    gf::temporal_walks(g->impl.view(), d_src, d_ts, num_rows, num_walks, length, recency,
                       max_history, seed, epoch, first_row, d_nodes, d_eids, d_times, device,
                       as_stream(stream));
  });
}

}  // extern "C"
