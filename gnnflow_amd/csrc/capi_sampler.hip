// extern "C" entry points of include/gnnflow_hip.h over Sampler: gf_sampler_* (plain, padded,
// the chained part_* protocol, partitioned, over a communicator, grouped) and gf_partition_*.
#include "capi_handles.hpp"
#include "enqueue_worker.hpp"
#include "partition.hpp"

namespace {

// The calling thread begins a sample itself only while every sample in flight on the sampler was
// begun that way: a begin of its own would overtake the ones still queued on an enqueue thread.
inline void require_sync_begins(const gf_sampler* s, const char* msg) {
  GF_REQUIRE(s->begin_tickets.empty() || s->begin_tickets.back() == 0, msg);
}

// `narrow_ids` of the shared-chain entry points: bit 0 = 12-byte reply records; bits 8..23 = the
// compact reply slots' edge fill in 1/1000 (0: the fixed records travel)
inline bool flag_narrow(int f) { return (f & 1) != 0; }
inline double flag_edge_fill(int f) { return ((f >> 8) & 0xFFFF) / 1000.0; }
// bit 1: layer l + 1 does not request layer l's roots again (most-recent, equal fanouts)
inline bool flag_reuse(int f) { return (f & 2) != 0; }

// the group's samples as the sampler takes them (checked)
std::vector<gf::Sampler::GroupSample> group_samples(gf_comm* c, const gf_group_sample* samples,
                                                    int m) {
  (void)c;   // null: one rank, nothing to exchange
  GF_REQUIRE(samples != nullptr, "null samples");
  GF_REQUIRE(m >= 1 && m <= GF_PART_GROUP_MAX, "group: 1..4 samples");
  std::vector<gf::Sampler::GroupSample> gs(m);
  for (int j = 0; j < m; ++j) {
    GF_S(samples[j].sampler);
    gs[j] = gf::Sampler::GroupSample{&samples[j].sampler->impl, samples[j].d_roots,
                                     samples[j].d_root_ts, samples[j].num_roots, samples[j].d_out,
                                     samples[j].out_bytes};
  }
  return gs;
}

}  // namespace

extern "C" {

int gf_sampler_create(gf_sampler** out, gf_graph* g, const uint32_t* fanouts, size_t num_layers,
                      int sampling_policy, uint32_t num_snapshots, float snapshot_time_window,
                      int prop_time, uint64_t seed) {
  return guarded([&] {
    GF_REQUIRE(out != nullptr, "gf_sampler_create: null out");
    GF_G(g);
    GF_REQUIRE(fanouts != nullptr, "gf_sampler_create: null fanouts");
    *out = new gf_sampler(&g->impl, fanouts, num_layers, sampling_policy, num_snapshots,
                          snapshot_time_window, prop_time != 0, seed);
  });
}
int gf_sampler_destroy(gf_sampler* s) { return destroy_handle(s); }
int gf_sampler_output_bytes(const gf_sampler* s, size_t num_roots, size_t* bytes) {
  return guarded([&] { GF_S(s); *bytes = s->impl.output_bytes(num_roots); });
}
int gf_sampler_layer_output_bytes(const gf_sampler* s, size_t num_roots, uint32_t layer,
                                  size_t* bytes) {
  return guarded([&] {
    GF_S(s);
    GF_REQUIRE(layer < s->impl.num_layers(), "layer out of range");
    *bytes = s->impl.layer_output_bytes(num_roots, layer);
  });
}
int gf_sampler_sample(gf_sampler* s, const int64_t* d_roots, const float* d_root_ts,
                      size_t num_roots, void* d_out, size_t out_bytes, gf_block* blocks,
                      void* stream) {
  return guarded([&] {
    GF_S(s);
    GF_REQUIRE(s->begin_tickets.empty(), "sample: asynchronous samples are still in flight");
    s->impl.sample(d_roots, d_root_ts, num_roots, d_out, out_bytes, blocks, as_stream(stream));
  });
}
int gf_sampler_sample_begin(gf_sampler* s, const int64_t* d_roots, const float* d_root_ts,
                            size_t num_roots, void* d_out, size_t out_bytes, void* stream) {
  return guarded([&] {
    GF_S(s);
    require_sync_begins(s, "sample_begin: earlier samples were begun through the enqueue thread");
    s->impl.sample_begin(d_roots, d_root_ts, num_roots, d_out, out_bytes, as_stream(stream));
    s->begin_tickets.push_back(0);
  });
}
int gf_sampler_sample_begin_async(gf_sampler* s, const int64_t* d_roots, const float* d_root_ts,
                                  size_t num_roots, void* d_out, size_t out_bytes,
                                  void* stream) {
  return guarded([&] {
    GF_S(s);
    GF_REQUIRE(s->begin_tickets.size() < gf::Sampler::kMaxInFlight,
               "sample_begin_async: too many samples in flight on this sampler");
    gf::Sampler* impl = &s->impl;
    hipStream_t st = as_stream(stream);
    const int lane = s->plain_lane;
    s->begin_tickets.push_back(gf::make_ticket(lane, gf::EnqueueWorker::get(lane).submit(
        [impl, d_roots, d_root_ts, num_roots, d_out, out_bytes, st]() {
          impl->sample_begin(d_roots, d_root_ts, num_roots, d_out, out_bytes, st);
        })));
  });
}
int gf_sampler_set_enqueue_lane(gf_sampler* s, int lane) {
  return guarded([&] {
    GF_S(s);
    GF_REQUIRE(lane == 1 || lane == 2, "gf_sampler_set_enqueue_lane: lane must be 1 or 2");
    GF_REQUIRE(s->begin_tickets.empty(), "gf_sampler_set_enqueue_lane: samples are in flight");
    s->plain_lane = lane;
  });
}
int gf_sampler_call_counter(const gf_sampler* s, uint64_t* out) {
  return guarded([&] {
    GF_S(s);
    GF_REQUIRE(out != nullptr, "gf_sampler_call_counter: null output");
    *out = s->impl.call_counter();
  });
}
int gf_sampler_set_call_counter(gf_sampler* s, uint64_t value, int through_enqueue_thread) {
  return guarded([&] {
    GF_S(s);
    gf::Sampler* impl = &s->impl;
    if (through_enqueue_thread) {
      // (jobs of the sampling lane run in submission order: the begin submitted next sees it)
      gf::EnqueueWorker::get(s->plain_lane).submit([impl, value]() { impl->set_call_counter(value); });
    } else {
      require_sync_begins(
          s, "set_call_counter: samples begun through the enqueue thread are in flight");
      impl->set_call_counter(value);
    }
  });
}
int gf_sampler_sample_end(gf_sampler* s, gf_block* blocks) {
  if (s && !s->begin_tickets.empty()) {
    const uint64_t t = s->begin_tickets.front();
    s->begin_tickets.pop_front();
    if (t) {   // begun through the enqueue thread: wait for the enqueue of THIS sample
      const int rc = gf::wait_ticket(t);
      if (rc != GF_OK) return rc;
    }
  }
  return guarded([&] { GF_S(s); s->impl.sample_end(blocks); });
}
int gf_sampler_sample_layer(gf_sampler* s, const int64_t* d_roots, const float* d_root_ts,
                            size_t num_roots, uint32_t layer, uint32_t snapshot, void* d_out,
                            size_t out_bytes, gf_block* block, void* stream) {
  return guarded([&] {
    GF_S(s);
    s->impl.sample_layer(d_roots, d_root_ts, num_roots, layer, snapshot, d_out, out_bytes, block,
                         as_stream(stream));
  });
}
int gf_sampler_sample_host(gf_sampler* s, const int64_t* nodes, const float* ts,
                           size_t num_roots, gf_block* blocks) {
  return guarded([&] { GF_S(s); s->impl.sample_host(nodes, ts, num_roots, blocks); });
}
int gf_sampler_sample_layer_host(gf_sampler* s, const int64_t* nodes, const float* ts,
                                 size_t num_roots, uint32_t layer, uint32_t snapshot,
                                 gf_block* block) {
  return guarded([&] {
    GF_S(s);
    s->impl.sample_layer_host(nodes, ts, num_roots, layer, snapshot, block);
  });
}
void gf_host_blocks_free(gf_block* blocks, size_t n) {
  if (!blocks) return;
  for (size_t i = 0; i < n; ++i) {
    free(blocks[i].all_nodes);
    free(blocks[i].all_timestamps);
    free(blocks[i].delta_timestamps);
    free(blocks[i].eids);
    free(blocks[i].row);
    free(blocks[i].col);
    blocks[i] = gf_block{};
  }
}

// ---- partitioned sampling: plan, padded layers, the chained part_* protocol ------------------
int gf_partition_scratch_bytes(size_t num_roots, int world_size, size_t* out) {
  return guarded([&] {
    GF_REQUIRE(out != nullptr, "gf_partition_scratch_bytes: null output");
    GF_REQUIRE(world_size >= 1, "partition: world size must be >= 1");
    *out = gf::partition_scratch_bytes(num_roots, world_size);
  });
}
int gf_partition_plan(const int64_t* d_nodes, const float* d_ts, size_t num_roots, int world_size,
                      int rank, int64_t* d_requests, uint32_t* d_pos, uint64_t* d_counts,
                      void* d_scratch, size_t scratch_bytes, int device, void* stream) {
  return guarded([&] {
    gf::partition_plan(d_nodes, d_ts, num_roots, world_size, rank, d_requests, d_pos, d_counts,
                       d_scratch, scratch_bytes, device, as_stream(stream));
  });
}
int gf_sampler_sample_layer_padded(gf_sampler* s, const int64_t* d_requests, size_t n,
                                   uint32_t layer, uint32_t snapshot, int64_t* d_out,
                                   void* stream) {
  return guarded([&] {
    GF_S(s);
    s->impl.sample_layer_padded(d_requests, n, layer, snapshot, d_out, as_stream(stream));
  });
}
int gf_sampler_merge_padded(gf_sampler* s, const int64_t* d_roots, const float* d_ts, size_t n,
                            uint32_t layer, const int64_t* d_replies, const uint32_t* d_pos,
                            void* d_out, size_t out_bytes, gf_block* block, void* stream) {
  return guarded([&] {
    GF_S(s);
    s->impl.merge_padded(d_roots, d_ts, n, layer, d_replies, d_pos, d_out, out_bytes, block,
                         as_stream(stream));
  });
}
int gf_sampler_part_layout(const gf_sampler* s, size_t num_roots, uint32_t layer, int world_size,
                           gf_part_layout* out) {
  return guarded([&] {
    GF_S(s);
    GF_REQUIRE(world_size >= 1 && world_size <= 64, "partition: world size must be 1..64");
    s->impl.part_layout(std::max<size_t>(num_roots, 1), layer, world_size, 0.0, 0, out);
  });
}
int gf_sampler_part_layout_slotted(const gf_sampler* s, size_t num_roots, uint32_t layer,
                                   int world_size, double slack, size_t slot_roots,
                                   gf_part_layout* out) {
  return guarded([&] {
    GF_S(s);
    GF_REQUIRE(world_size >= 1 && world_size <= 64, "partition: world size must be 1..64");
    GF_REQUIRE(slack > 0.0, "part_layout_slotted: slack must be positive");
    s->impl.part_layout(std::max<size_t>(num_roots, 1), layer, world_size, slack, slot_roots, out);
  });
}
int gf_sampler_part_group_slot(const gf_sampler* s, size_t num_roots, uint32_t layer,
                               int world_size, double slack, size_t slot_roots, int narrow,
                               double edge_fill, uint64_t* out) {
  return guarded([&] {
    GF_S(s);
    GF_REQUIRE(out != nullptr, "part_group_slot: null output");
    GF_REQUIRE(world_size >= 1 && world_size <= 64, "partition: world size must be 1..64");
    GF_REQUIRE(slack > 0.0, "part_group_slot: slack must be positive");
    GF_REQUIRE(layer < s->impl.num_layers(), "layer out of range");
    gf::Sampler::GroupLayout lay;
    const size_t R[1] = {std::max<size_t>(num_roots, 1)};
    s->impl.group_layout(R, 1, layer, world_size, slack, slot_roots, (narrow & 1) != 0, edge_fill,
                         &lay, (narrow & 2) != 0);
    const size_t rb = (narrow & 1) ? 12 : 24;
    out[0] = lay.stride;
    out[1] = edge_fill > 0.0 ? lay.cslot : lay.stride * s->impl.fanout(layer) * rb;
    out[2] = lay.edge_cap;
    out[3] = lay.off_bytes;
  });
}
int gf_sampler_part_begin(gf_sampler* s, const int64_t* d_roots, const float* d_root_ts,
                          size_t num_roots, void* d_out, size_t out_bytes, int world_size,
                          int rank, void* stream) {
  return guarded([&] {
    GF_S(s);
    require_sync_begins(s, "part_begin: earlier samples were begun through the enqueue thread");
    s->impl.part_begin(d_roots, d_root_ts, num_roots, d_out, out_bytes, world_size, rank, 0.0, 0,
                       as_stream(stream));
  });
}
int gf_sampler_part_begin_slotted(gf_sampler* s, const int64_t* d_roots, const float* d_root_ts,
                                  size_t num_roots, void* d_out, size_t out_bytes, int world_size,
                                  int rank, double slack, size_t slot_roots, void* stream) {
  return guarded([&] {
    GF_S(s);
    GF_REQUIRE(slack > 0.0, "part_begin_slotted: slack must be positive");
    require_sync_begins(s, "part_begin: earlier samples were begun through the enqueue thread");
    s->impl.part_begin(d_roots, d_root_ts, num_roots, d_out, out_bytes, world_size, rank, slack,
                       slot_roots, as_stream(stream));
  });
}
int gf_sampler_part_serve(gf_sampler* s, uint32_t layer, uint32_t snapshot, void* d_ws,
                          size_t ws_bytes) {
  return guarded([&] { GF_S(s); s->impl.part_serve(layer, snapshot, d_ws, ws_bytes); });
}
int gf_sampler_part_overflowed(const gf_sampler* s, int* out) {
  return guarded([&] {
    GF_REQUIRE(s != nullptr && out != nullptr, "part_overflowed: null argument");
    *out = s->impl.last_overflow() ? 1 : 0;
  });
}
int gf_sampler_part_plan_own(gf_sampler* s, uint32_t layer, uint32_t snapshot, void* d_ws,
                             size_t ws_bytes, int phases) {
  return guarded([&] {
    GF_S(s);
    GF_REQUIRE(phases >= 1 && phases <= 3, "part_plan_own: phases must be 1, 2 or 3");
    s->impl.part_plan_own(layer, snapshot, d_ws, ws_bytes, phases);
  });
}
int gf_sampler_part_merge(gf_sampler* s, uint32_t layer, uint32_t snapshot, void* d_ws,
                          size_t ws_bytes) {
  return guarded([&] { GF_S(s); s->impl.part_merge(layer, snapshot, d_ws, ws_bytes); });
}
int gf_sampler_part_commit(gf_sampler* s) {
  return guarded([&] {
    GF_S(s);
    s->impl.part_commit();
    s->begin_tickets.push_back(0);
  });
}
int gf_sampler_part_abort(gf_sampler* s) {
  return guarded([&] { GF_S(s); s->impl.part_abort(); });
}
int gf_sampler_sample_partitioned(gf_sampler* s, const int64_t* d_roots, const float* d_root_ts,
                                  size_t num_roots, void* d_out, size_t out_bytes, void* d_ws,
                                  size_t ws_bytes, void* stream) {
  return guarded([&] {
    GF_S(s);
    require_sync_begins(
        s, "sample_partitioned: earlier samples were begun through the enqueue thread");
    s->impl.sample_partitioned(d_roots, d_root_ts, num_roots, d_out, out_bytes, d_ws, ws_bytes,
                               as_stream(stream));
    s->begin_tickets.push_back(0);
  });
}
int gf_sampler_sample_partitioned_async(gf_sampler* s, const int64_t* d_roots,
                                        const float* d_root_ts, size_t num_roots, void* d_out,
                                        size_t out_bytes, void* d_ws, size_t ws_bytes,
                                        void* stream) {
  return guarded([&] {
    GF_S(s);
    GF_REQUIRE(s->begin_tickets.size() < gf::Sampler::kMaxInFlight,
               "sample_partitioned_async: too many samples in flight on this sampler");
    gf::Sampler* impl = &s->impl;
    hipStream_t st = as_stream(stream);
    s->begin_tickets.push_back(gf::make_ticket(1, gf::EnqueueWorker::get(1).submit(
        [impl, d_roots, d_root_ts, num_roots, d_out, out_bytes, d_ws, ws_bytes, st]() {
          impl->sample_partitioned(d_roots, d_root_ts, num_roots, d_out, out_bytes, d_ws,
                                   ws_bytes, st);
        })));
  });
}

// ---- partitioned sampling over a communicator: one sample, a group of up to four -------------
int gf_sampler_sample_partitioned_comm(gf_sampler* s, gf_comm* c, const int64_t* d_roots,
                                       const float* d_root_ts, size_t num_roots, void* d_out,
                                       size_t out_bytes, void* d_ws, size_t ws_bytes, double slack,
                                       size_t slot_roots, int overlap, void* stream) {
  return guarded([&] {
    GF_REQUIRE(s != nullptr && c != nullptr, "null sampler / communicator handle");
    require_sync_begins(
        s, "sample_partitioned_comm: earlier samples were begun through the enqueue thread");
    s->impl.sample_partitioned_slotted(d_roots, d_root_ts, num_roots, d_out, out_bytes, d_ws,
                                       ws_bytes, slack, slot_roots, c->impl, overlap != 0,
                                       as_stream(stream));
    s->begin_tickets.push_back(0);
  });
}
int gf_sampler_sample_partitioned_comm_async(gf_sampler* s, gf_comm* c, const int64_t* d_roots,
                                             const float* d_root_ts, size_t num_roots, void* d_out,
                                             size_t out_bytes, void* d_ws, size_t ws_bytes,
                                             double slack, size_t slot_roots, int overlap,
                                             void* stream) {
  return guarded([&] {
    GF_REQUIRE(s != nullptr && c != nullptr, "null sampler / communicator handle");
    GF_REQUIRE(!c->loopback, "sample_partitioned_comm_async: a loopback communicator's ranks are "
                             "threads; one enqueue thread cannot serve them (use the synchronous call)");
    GF_REQUIRE(s->begin_tickets.size() < gf::Sampler::kMaxInFlight,
               "sample_partitioned_comm_async: too many samples in flight on this sampler");
    gf::Sampler* impl = &s->impl;
    gf::Exchange* comm = &c->impl;
    hipStream_t st = as_stream(stream);
    const bool ov = overlap != 0;
    // The chain of a sample over a communicator is ~11 stream operations, collectives among
    // them, and the pipelined loop is bound by the host time of issuing them.  Two issuing
    // threads slow each other down here (measured, one rank over RCCL, 3 lanes: the chain's
    // issue time 40 us with one thread for chains AND fetches, 63-83 us with a thread each;
    // step 53 vs 72-84 us), so the chains share the fetch lane's thread.  It also keeps ONE
    // global order of everything that is enqueued, on every rank.
    const int lane = gf::kCollectiveLane;
    s->begin_tickets.push_back(gf::make_ticket(lane, gf::EnqueueWorker::get(lane).submit(
        [impl, comm, d_roots, d_root_ts, num_roots, d_out, out_bytes, d_ws, ws_bytes, slack,
         slot_roots, ov, st]() {
          impl->sample_partitioned_slotted(d_roots, d_root_ts, num_roots, d_out, out_bytes, d_ws,
                                           ws_bytes, slack, slot_roots, *comm, ov, st);
        })));
  });
}
int gf_sampler_part_group_ws_bytes(const gf_sampler* s, const size_t* roots, int m, int world_size,
                                   double slack, size_t slot_roots, int narrow_ids,
                                   size_t* bytes) {
  return guarded([&] {
    GF_REQUIRE(s != nullptr && roots != nullptr && bytes != nullptr,
               "part_group_ws_bytes: null argument");
    GF_REQUIRE(m >= 1 && m <= GF_PART_GROUP_MAX, "group: 1..4 samples");
    GF_REQUIRE(world_size >= 1 && world_size <= 32, "group: world size must be 1..32");
    size_t R[GF_PART_GROUP_MAX];
    for (int j = 0; j < m; ++j) R[j] = std::max<size_t>(roots[j], 1);
    *bytes = (slack > 0.0 && s->impl.group_ok(R, m))
                 ? gf::Sampler::group_ws_bytes(s->impl, R, m, world_size, slack, slot_roots,
                                               flag_narrow(narrow_ids), flag_edge_fill(narrow_ids),
                                               flag_reuse(narrow_ids))
                 : 0;
  });
}
int gf_sampler_sample_partitioned_comm_group(gf_comm* c, const gf_group_sample* samples, int m,
                                             void* d_ws, size_t ws_bytes, double slack,
                                             size_t slot_roots, int force_overflow,
                                             int narrow_ids, void* stream) {
  return guarded([&] {
    const auto gs = group_samples(c, samples, m);
    for (int j = 0; j < m; ++j)
      require_sync_begins(
          samples[j].sampler,
          "sample_partitioned_comm_group: earlier samples were begun through the enqueue thread");
    gf::Sampler::sample_partitioned_group(gs.data(), m, d_ws, ws_bytes, slack, slot_roots,
                                          c ? &c->impl : nullptr, as_stream(stream),
                                          static_cast<unsigned>(force_overflow),
                                          flag_narrow(narrow_ids), flag_edge_fill(narrow_ids),
                                          flag_reuse(narrow_ids));
    for (int j = 0; j < m; ++j) samples[j].sampler->begin_tickets.push_back(0);
  });
}
int gf_sampler_sample_partitioned_comm_group_async(gf_comm* c, const gf_group_sample* samples,
                                                   int m, void* d_ws, size_t ws_bytes,
                                                   double slack, size_t slot_roots,
                                                   int force_overflow, int narrow_ids,
                                                   void* stream) {
  return guarded([&] {
    auto gs = group_samples(c, samples, m);
    GF_REQUIRE(!c || !c->loopback, "sample_partitioned_comm_group_async: a loopback "
                                   "communicator's ranks are threads (use the synchronous call)");
    for (int j = 0; j < m; ++j)
      GF_REQUIRE(samples[j].sampler->begin_tickets.size() < gf::Sampler::kMaxInFlight,
                 "sample_partitioned_comm_group_async: too many samples in flight on a sampler");
    gf::Exchange* comm = c ? &c->impl : nullptr;
    hipStream_t st = as_stream(stream);
    // no communicator, no collective: the sampling lane's thread, like the plain sampler's
    const int lane = c ? gf::kCollectiveLane : 1;
    // ONE job for all samples of the group: every sampler's ticket is this job's
    const uint64_t t = gf::make_ticket(lane, gf::EnqueueWorker::get(lane).submit(
        [gs = std::move(gs), m, d_ws, ws_bytes, slack, slot_roots, comm, st, force_overflow,
         narrow_ids]() {
          gf::Sampler::sample_partitioned_group(gs.data(), m, d_ws, ws_bytes, slack, slot_roots,
                                                comm, st, static_cast<unsigned>(force_overflow),
                                                flag_narrow(narrow_ids), flag_edge_fill(narrow_ids),
                                                flag_reuse(narrow_ids));
        }));
    for (int j = 0; j < m; ++j) samples[j].sampler->begin_tickets.push_back(t);
  });
}

}  // extern "C"
