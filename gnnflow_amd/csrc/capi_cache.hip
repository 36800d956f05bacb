// extern "C" entry points of include/gnnflow_hip.h over FeatureCache and the row kernels:
// gf_cache_*, gf_debug_lru_*, gf_pull_*, gf_gather_rows*, gf_memory_*.
#include "capi_handles.hpp"
#include "enqueue_worker.hpp"

namespace {

// What a job of the asynchronous fetch calls works on.  It runs after the call has returned, so
// it takes a copy of the caller's descriptors.
struct FetchJob {
  gf::FeatureCache *node, *edge;
  std::vector<gf_fetch_desc> descs;
  hipStream_t stream;
};
inline FetchJob fetch_job(gf_cache* node_cache, gf_cache* edge_cache, const gf_fetch_desc* descs,
                          size_t n, void* stream, const uint64_t* ticket, const char* null_ticket,
                          const char* null_descs) {
  GF_REQUIRE(ticket != nullptr, null_ticket);
  GF_REQUIRE(descs != nullptr || n == 0, null_descs);
  return FetchJob{cache_or_null(node_cache), cache_or_null(edge_cache),
                  std::vector<gf_fetch_desc>(descs, descs + n), as_stream(stream)};
}

}  // namespace

extern "C" {

int gf_cache_create(gf_cache** out, size_t num_ids, size_t capacity, size_t dim,
                    const float* d_feats, int device) {
  return guarded([&] {
    GF_REQUIRE(out != nullptr, "gf_cache_create: null out");
    *out = new gf_cache(num_ids, capacity, dim, d_feats, device);
  });
}
int gf_cache_destroy(gf_cache* c) { return destroy_handle(c); }
int gf_cache_set_policy(gf_cache* c, int policy) {
  return guarded([&] { GF_C(c); c->impl.set_policy(policy); });
}
int gf_cache_reset_order(gf_cache* c, void* stream) {
  return guarded([&] { GF_C(c); c->impl.reset_order(as_stream(stream)); });
}
int gf_cache_init_ids(gf_cache* c, const int64_t* d_ids, size_t n, void* stream) {
  return guarded([&] { GF_C(c); c->impl.init_ids(d_ids, n, as_stream(stream)); });
}
int gf_cache_init(gf_cache* c, void* stream) {
  return guarded([&] { GF_C(c); c->impl.init(as_stream(stream)); });
}
int gf_cache_resize(gf_cache* c, size_t new_num_ids, size_t new_capacity, const float* d_feats,
                    void* stream) {
  return guarded([&] {
    GF_C(c);
    c->impl.resize(new_num_ids, new_capacity, d_feats, as_stream(stream));
  });
}
int gf_cache_fetch(gf_cache* c, const int64_t* d_ids, size_t n, float* d_out, int update,
                   uint32_t* d_stats, void* stream) {
  return guarded([&] {
    GF_C(c);
    c->impl.fetch(d_ids, n, d_out, update != 0, d_stats, as_stream(stream));
  });
}
int gf_cache_init_rows(gf_cache* c, const int64_t* d_ids, size_t n, const float* d_rows,
                       void* stream) {
  return guarded([&] {
    GF_C(c);
    GF_REQUIRE(d_rows != nullptr || n == 0, "cache: null rows");
    c->impl.init_ids(d_ids, n, as_stream(stream), d_rows);
  });
}
int gf_cache_probe(gf_cache* c, const int64_t* d_ids, size_t n, int32_t* d_slot, void* stream) {
  return guarded([&] { GF_C(c); c->impl.probe(d_ids, n, d_slot, as_stream(stream)); });
}
int gf_cache_fetch_pulled(gf_cache* c, const int64_t* d_ids, size_t n, float* d_out, int update,
                          uint32_t* d_stats, const float* d_miss_rows,
                          const uint32_t* d_miss_index, void* stream) {
  return guarded([&] {
    GF_C(c);
    c->impl.fetch_pulled(d_ids, n, d_out, update != 0, d_stats, d_miss_rows, d_miss_index,
                         as_stream(stream));
  });
}
int gf_cache_fetch_blocks_pulled(gf_cache* node_cache, gf_cache* edge_cache,
                                 const gf_fetch_pulled_desc* descs, size_t n, void* stream) {
  return guarded([&] {
    gf::fetch_blocks_pulled(cache_or_null(node_cache), cache_or_null(edge_cache), descs, n,
                            as_stream(stream));
  });
}
int gf_cache_fetch_blocks(gf_cache* node_cache, gf_cache* edge_cache, const gf_fetch_desc* descs,
                          size_t n, void* stream) {
  return guarded([&] {
    gf::fetch_blocks(cache_or_null(node_cache), cache_or_null(edge_cache), descs, n, as_stream(stream));
  });
}
int gf_cache_fetch_blocks_async(gf_cache* node_cache, gf_cache* edge_cache,
                                const gf_fetch_desc* descs, size_t n, void* stream,
                                uint64_t* ticket) {
  return guarded([&] {
    FetchJob j = fetch_job(node_cache, edge_cache, descs, n, stream, ticket,
                           "fetch_blocks_async: null ticket", "fetch_blocks_async: null descriptors");
    *ticket = gf::EnqueueWorker::get().submit([j = std::move(j)]() {
      gf::fetch_blocks(j.node, j.edge, j.descs.data(), j.descs.size(), j.stream);
    });
  });
}
int gf_cache_prefetch_blocks(gf_cache* node_cache, gf_cache* edge_cache,
                             const gf_fetch_desc* descs, size_t n, void* stream, int* issued) {
  return guarded([&] {
    const bool did = gf::prefetch_blocks(cache_or_null(node_cache), cache_or_null(edge_cache),
                                         descs, n, as_stream(stream));
    if (issued) *issued = did ? 1 : 0;
  });
}
int gf_cache_prefetch_blocks_async(gf_cache* node_cache, gf_cache* edge_cache,
                                   const gf_fetch_desc* descs, size_t n, void* stream,
                                   uint64_t* ticket) {
  return guarded([&] {
    FetchJob j = fetch_job(node_cache, edge_cache, descs, n, stream, ticket,
                           "prefetch_blocks_async: null ticket",
                           "prefetch_blocks_async: null descriptors");
    *ticket = gf::EnqueueWorker::get().submit([j = std::move(j)]() {
      gf::prefetch_blocks(j.node, j.edge, j.descs.data(), j.descs.size(), j.stream);
    });
  });
}
int gf_cache_fetch_announce_async(gf_cache* node_cache, gf_cache* edge_cache,
                                  const gf_fetch_desc* descs, size_t n, void* stream,
                                  const gf_fetch_desc* next_descs, size_t next_n,
                                  const gf_block* next_blocks, size_t next_layers,
                                  size_t next_snapshots, void* prefetch_stream, uint64_t* ticket) {
  return guarded([&] {
    const char* no_ticket = "fetch_announce_async: null ticket";
    const char* no_descs = "fetch_announce_async: null descriptors";
    FetchJob now = fetch_job(node_cache, edge_cache, descs, n, stream, ticket, no_ticket, no_descs);
    FetchJob next = fetch_job(node_cache, edge_cache, next_descs, next_n, prefetch_stream, ticket,
                              no_ticket, no_descs);
    if (next_blocks != nullptr) {
      const size_t L = next_layers, NS = next_snapshots;
      GF_REQUIRE(L >= 1 && NS >= 1, "fetch_announce_async: empty block array");
      for (size_t s = 0; next.node && s < NS; ++s) {   // mfgs[0]: the last sampled layer
        const gf_block& b = next_blocks[(L - 1) * NS + s];
        if (b.num_src_nodes)
          next.descs.push_back(gf_fetch_desc{0, 1, b.all_nodes, b.num_src_nodes, nullptr, nullptr});
      }
      for (size_t i = 0; next.edge && i < L * NS; ++i) {
        const gf_block& b = next_blocks[i];
        if (b.num_edges)
          next.descs.push_back(gf_fetch_desc{1, 1, b.eids, b.num_edges, nullptr, nullptr});
      }
    }
    *ticket = gf::EnqueueWorker::get().submit([now = std::move(now), next = std::move(next)]() {
      gf::fetch_blocks(now.node, now.edge, now.descs.data(), now.descs.size(), now.stream);
      gf::prefetch_blocks(next.node, next.edge, next.descs.data(), next.descs.size(), next.stream);
    });
  });
}
int gf_cache_fetch_wait(uint64_t ticket) {   // (a fetch ticket is the fetch lane's bare sequence)
  return gf::wait_ticket(gf::make_ticket(0, ticket));
}
int gf_cache_set_row_mirror(gf_cache* c, int on) {
  return guarded([&] { GF_C(c); c->impl.set_row_mirror(on != 0); });
}
int gf_cache_set_staging(gf_cache* c, size_t generations, size_t rows_per_generation) {
  return guarded([&] { GF_C(c); c->impl.set_staging(generations, rows_per_generation); });
}
int gf_cache_set_staging_lag(gf_cache* c, size_t lag) {
  return guarded([&] { GF_C(c); c->impl.set_staging_lag(lag); });
}
int gf_cache_invalidate_staging(gf_cache* c) {
  return guarded([&] { GF_C(c); c->impl.invalidate_staging(); });
}
int gf_cache_staging_state(gf_cache* c, uint64_t* out) {
  return guarded([&] {
    GF_C(c);
    GF_REQUIRE(out != nullptr, "gf_cache_staging_state: null output");
    c->impl.staging_state(out);
  });
}
int gf_cache_slot_ids(const gf_cache* c, int64_t* out, size_t capacity) {
  return guarded([&] { GF_C(c); c->impl.slot_ids(out, capacity); });
}
int gf_cache_mem_bytes(const gf_cache* c, size_t* out) {
  return guarded([&] { GF_C(c); *out = c->impl.mem_bytes(); });
}
int gf_cache_lru_state(const gf_cache* c, uint64_t out[7]) {
  return guarded([&] {
    GF_C(c);
    GF_REQUIRE(out != nullptr, "gf_cache_lru_state: null output");
    c->impl.lru_state(out);
  });
}
int gf_debug_lru_trace_enable(gf_cache* c, int on) {
  return guarded([&] { GF_C(c); c->impl.lru_trace_enable(on != 0); });
}
int gf_debug_lru_trace(gf_cache* c, uint64_t* out, size_t capacity_words, size_t* words) {
  return guarded([&] {
    GF_C(c);
    GF_REQUIRE(out != nullptr && words != nullptr, "gf_debug_lru_trace: null output");
    *words = c->impl.lru_trace_read(out, capacity_words);
  });
}

// ---- sharded features: pull rounds -------------------------------------------------------------
int gf_pull_count(const gf_pull_desc* descs, size_t n, int world_size, uint32_t* d_counts,
                  int device, void* stream) {
  return guarded([&] {
    GF_REQUIRE(descs != nullptr && n >= 1 && n <= 4, "gf_pull_count: 1..4 contexts");
    gf::FeatureCache* caches[4] = {nullptr, nullptr, nullptr, nullptr};
    for (size_t i = 0; i < n; ++i) caches[i] = cache_or_null(descs[i].cache);
    gf::pull_count(descs, n, world_size, caches, d_counts, device, as_stream(stream));
  });
}
int gf_pull_scatter(const gf_pull_desc* descs, size_t n, int world_size, uint32_t* d_counts,
                    uint32_t* d_cursor, int device, void* stream) {
  return guarded([&] {
    GF_REQUIRE(descs != nullptr && n >= 1 && n <= 4, "gf_pull_scatter: 1..4 contexts");
    gf::FeatureCache* caches[4] = {nullptr, nullptr, nullptr, nullptr};
    for (size_t i = 0; i < n; ++i) caches[i] = cache_or_null(descs[i].cache);
    gf::pull_scatter(descs, n, world_size, caches, d_counts, d_cursor, device, as_stream(stream));
  });
}
int gf_pull_session_create(gf_pull_session** out, gf_comm* comm, int device) {
  return guarded([&] {
    GF_REQUIRE(out != nullptr, "gf_pull_session_create: null output");
    *out = new gf_pull_session(comm ? &comm->impl : nullptr, device);
    (*out)->ordered = comm != nullptr && !comm->loopback && comm->ipc == nullptr;
  });
}
int gf_pull_session_destroy(gf_pull_session* s) { return destroy_handle(s); }
int gf_pull_round(gf_pull_session* s, gf_cache* node_cache, gf_cache* edge_cache,
                  const gf_pull_ctx* ctxs, size_t n, int flag, int* any_flag, uint64_t* rows_pulled,
                  uint64_t* bytes_sent, uint32_t* d_error_flag, void* stream) {
  gf::FeatureCache* nc = cache_or_null(node_cache);
  gf::FeatureCache* ec = cache_or_null(edge_cache);
  hipStream_t st = as_stream(stream);
  if (s != nullptr && s->ordered) {
    // The sampler's chains (collectives on the lanes' communicators) are issued by the fetch
    // lane's enqueue thread, this round's collectives (on the session's communicator) would be
    // issued by the caller's: two threads, no common order across ranks — RCCL kernels of
    // different communicators that share a hardware queue could then wait for each other.  The
    // round therefore takes its place in that thread's queue and the caller waits for it.
    gf::PullSession* impl = &s->impl;
    const int lane = gf::kCollectiveLane;
    return gf::wait_ticket(gf::make_ticket(lane, gf::EnqueueWorker::get(lane).submit([=]() {
      impl->round(nc, ec, ctxs, n, flag, any_flag, rows_pulled, bytes_sent, d_error_flag, st);
    })));
  }
  return guarded([&] {
    GF_REQUIRE(s != nullptr, "null pull session");
    s->impl.round(nc, ec, ctxs, n, flag, any_flag, rows_pulled, bytes_sent, d_error_flag, st);
  });
}

// ---- rows by id, TGN memory ----------------------------------------------------------------------
int gf_gather_rows(const float* d_feats, size_t num_rows, size_t dim, const int64_t* d_ids,
                   size_t n, float* d_out, int device, void* stream) {
  return guarded([&] {
    gf::gather_rows(d_feats, num_rows, dim, d_ids, n, d_out, device, as_stream(stream));
  });
}
int gf_gather_rows_indexed(const float* d_rows, size_t num_local_rows, size_t dim,
                           const int32_t* d_index, size_t num_ids, const int64_t* d_ids, size_t n,
                           float* d_out, uint32_t* d_flag, int device, void* stream) {
  return guarded([&] {
    gf::gather_rows_indexed(d_rows, num_local_rows, dim, d_index, num_ids, d_ids, n, d_out, d_flag,
                            device, as_stream(stream));
  });
}
int gf_memory_prepare_input(const float* d_node_memory, const float* d_node_memory_ts,
                            const float* d_mailbox, const float* d_mailbox_ts, size_t num_nodes,
                            size_t dim_memory, size_t dim_mail, const int64_t* d_ids, size_t n,
                            float* d_mem, float* d_mem_ts, float* d_mail_ts, float* d_mem_input,
                            int device, void* stream) {
  return guarded([&] {
    const float* tables[4] = {d_node_memory, d_mailbox, d_node_memory_ts, d_mailbox_ts};
    const size_t dims[4] = {dim_memory, dim_mail, 1, 1};
    float* outs[4] = {d_mem, d_mem_input, d_mem_ts, d_mail_ts};
    gf::gather_rows_multi(tables, dims, outs, 4, num_nodes, d_ids, n, device, as_stream(stream));
  });
}
int gf_memory_update(float* d_node_memory, float* d_node_memory_ts, float* d_mailbox,
                     float* d_mailbox_ts, size_t num_nodes, size_t dim_memory, size_t dim_edge,
                     const int64_t* d_nid, const float* d_memory, const float* d_ts,
                     const float* d_edge_feats, size_t n, int neg_sample_ratio,
                     uint64_t* d_win_mail, uint64_t* d_win_mem, uint64_t epoch, int device,
                     void* stream) {
  return guarded([&] {
    gf::memory_update(d_node_memory, d_node_memory_ts, d_mailbox, d_mailbox_ts, num_nodes,
                      dim_memory, dim_edge, d_nid, d_memory, d_ts, d_edge_feats, n,
                      neg_sample_ratio, reinterpret_cast<unsigned long long*>(d_win_mail),
                      reinterpret_cast<unsigned long long*>(d_win_mem), epoch, device,
                      as_stream(stream));
  });
}

}  // extern "C"
