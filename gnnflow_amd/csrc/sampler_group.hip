// ---- two samples in ONE chain ---------------------------------------------------------------
// The slotted chain of a sample is ~11 stream operations, and at batch 600 its throughput is
// bound by the host thread that issues them (measured: 3-6 us each), not by the GPU.  Up to
// kMaxGroup = 4 consecutive batches therefore SHARE their launches and exchanges: sample j of
// m runs through its own sampler (clones on the same graph: own output, counters, publish
// record), all write their requests into one buffer — owner q's rows of sample j into slot
// m q + j, so the buffer is P runs of m slots and ONE equal-split all-to-all moves them all —,
// the received slots (m P of them, served alike) and the m own shares are sampled by one
// launch, one exchange brings the replies back, one launch merges all, one publishes all: 11
// operations per m samples.  Conditions (else the caller issues single chains): one snapshot,
// every layer of every sample within the fused plan / fused merge limits (<= 32 768 roots,
// fanout <= 256).  Layout of the shared workspace of layer l, rows of 16 B (requests) and
// fanout x 24 B (replies):  [m P slots of `stride` rows | own share 0 | ... | own share m-1].
#include "sampler_ctx.hpp"
#include "partition.hpp"

#include <chrono>
#include <cmath>

namespace gf {

size_t Sampler::group_ws_bytes(const Sampler& a, const size_t* R, int m, int world, double slack,
                               size_t slot_roots, bool narrow, double edge_fill, bool reuse_roots) {
  size_t total = 0;
  for (size_t l = 0; l < a.fanouts_.size(); ++l) {
    GroupLayout lay;
    a.group_layout(R, m, static_cast<uint32_t>(l), world, slack, slot_roots, narrow, edge_fill, &lay,
                   reuse_roots);
    total += lay.total;
  }
  return total;
}

bool Sampler::group_ok(const size_t* R, int m) const {
  if (num_snapshots_ != 1 || m < 1 || m > kMaxGroup) return false;
  for (size_t l = 0; l < fanouts_.size(); ++l) {
    if (fanouts_[l] > kEmitThreads) return false;
    for (int j = 0; j < m; ++j) {
      const size_t bound = root_bound(std::max<size_t>(R[j], 1), l);
      if (bound > kSmallRoots || bound > kPlanJobsMaxRoots) return false;
    }
  }
  return true;
}

void Sampler::group_layout(const size_t* R, int m, uint32_t layer, int world, double slack,
                           size_t slot_roots, bool narrow, double edge_fill,
                           GroupLayout* out, bool reuse_roots) const {
  GF_REQUIRE(m >= 1 && m <= kMaxGroup, "group layout: 1..4 samples");
  gf_part_layout one;
  part_layout(std::max<size_t>(R[0], 1), layer, world, slack, slot_roots, &one,
              layer_reuses_roots(reuse_roots, layer));   // slot stride
  const size_t F = fanouts_[layer];
  const size_t slot_rows = static_cast<size_t>(m) * world * one.slot_stride;
  size_t bound[kMaxGroup], rows = slot_rows;
  for (int j = 0; j < m; ++j) {
    bound[j] = root_bound(std::max<size_t>(R[j], 1), layer);
    out->own[j] = rows;
    rows += bound[j];
  }
  GF_REQUIRE(rows < 0xFFFFFFFFull, "group layout: more than 2^32-1 request rows");
  out->stride = one.slot_stride;
  out->slot_rows = slot_rows;
  size_t at = 0;
  const size_t rb = narrow ? 12 : 24;   // bytes per reply slot
  out->requests = at; at = align_up(at + rows * 16, 256);
  out->replies = at;  at = align_up(at + rows * F * rb, 256);
  out->inbox = at;    at = align_up(at + slot_rows * 16, 256);
  out->served = at;   at = align_up(at + slot_rows * F * rb, 256);
  for (int j = 0; j < m; ++j) { out->counts[j] = at; at = align_up(at + static_cast<size_t>(world) * 8, 256); }
  for (int j = 0; j < m; ++j) { out->pos[j] = at; at = align_up(at + bound[j] * 4, 256); }
  // first edge of every root in the merged block (+ the total): what the NEXT layer needs to
  // take the edges of the roots it does not request again from this block
  for (int j = 0; j < m; ++j) { out->first[j] = at; at = align_up(at + (bound[j] + 1) * 4, 256); }
  out->edge_cap = out->cslot = out->row_cnt = out->cserved = out->creplies = out->off_bytes = 0;
  if (edge_fill > 0.0) {
    // compact reply slot: offsets [0] = its edges, [r] = edges of the rows before row r
    // (1 <= r < stride), [stride] = "a slot of this sender overflowed"; then the edges.  The
    // first layer's roots are the batch itself — most of them have edges — while deeper layers
    // thin out: layer l gets the share edge_fill^(l / (L - 1)) of its fixed records (1 for the
    // first layer, edge_fill for the last).  16-bit offsets while the capacity allows.
    const size_t L = fanouts_.size();
    const double f = L > 1 ? std::pow(edge_fill, static_cast<double>(layer) / (L - 1)) : 1.0;
    const size_t cap = static_cast<size_t>(
        std::ceil(f * static_cast<double>((one.slot_stride - 1) * F)));
    out->edge_cap = std::max<size_t>(cap, F);
    out->off_bytes = out->edge_cap < 65535 ? 2 : 4;
    out->cslot = align_up(out->off_bytes * (one.slot_stride + 1), 16) + align_up(out->edge_cap * rb, 16);
    const size_t slots = static_cast<size_t>(m) * world;
    out->row_cnt = at;  at = align_up(at + slot_rows * 4, 256);
    out->cserved = at;  at = align_up(at + slots * out->cslot, 256);
    out->creplies = at; at = align_up(at + slots * out->cslot, 256);
  }
  out->total = at;
}

void Sampler::sample_partitioned_group(const GroupSample* gs, int m, void* d_ws, size_t ws_bytes,
                                       double slack, size_t slot_roots, Exchange* ex,
                                       hipStream_t stream, unsigned force_overflow, bool narrow,
                                       double edge_fill, bool reuse_roots) {
  GF_REQUIRE(gs != nullptr && m >= 1 && m <= kMaxGroup, "sample_partitioned_group: 1..4 samples");
  Sampler& a = *gs[0].s;
  size_t Rin[kMaxGroup];
  for (int j = 0; j < m; ++j) {
    GF_REQUIRE(gs[j].s != nullptr, "sample_partitioned_group: null sampler");
    for (int k = 0; k < j; ++k)
      GF_REQUIRE(gs[j].s != gs[k].s, "sample_partitioned_group: the samples need a sampler each");
    const Sampler& b = *gs[j].s;
    GF_REQUIRE(a.graph_ == b.graph_ && a.fanouts_ == b.fanouts_ && a.policy_ == b.policy_ &&
                   a.num_snapshots_ == b.num_snapshots_ && a.window_ == b.window_ &&
                   a.prop_time_ == b.prop_time_ && a.seed_ == b.seed_,
               "sample_partitioned_group: the samplers differ");
    Rin[j] = gs[j].R;
  }
  GF_REQUIRE(slack > 0.0, "sample_partitioned_group: slack must be positive");
  GF_REQUIRE(a.group_ok(Rin, m), "sample_partitioned_group: these samples cannot share a chain");
  DeviceGuard dg(a.graph_->device());
  const size_t L = a.fanouts_.size();
  // ex == null: ONE rank and nothing to exchange (every root is its own): the same chain
  // without its two all-to-alls and without the inbox job
  const int P = ex ? ex->world() : 1, me = ex ? ex->rank() : 0;
  using clk = std::chrono::steady_clock;
  auto t_prev = clk::now();
  auto lap = [&](int stage) {
    const auto t = clk::now();
    part_host_add(stage,
                  std::chrono::duration_cast<std::chrono::nanoseconds>(t - t_prev).count());
    t_prev = t;
  };
  int begun = 0;
  auto abort_all = [&]() { for (int j = 0; j < begun; ++j) gs[j].s->part_abort(); };
  try {
    for (; begun < m; ++begun) {
      const GroupSample& g = gs[begun];
      g.s->part_begin(g.d_roots, g.d_ts, g.R, g.d_out, g.out_bytes, P, me, slack, slot_roots,
                      stream);
    }
  } catch (...) {
    abort_all();
    throw;
  }
  lap(0);
  try {
    char* w = static_cast<char*>(d_ws);
    size_t off = 0;
    size_t Rs[kMaxGroup];
    for (int j = 0; j < m; ++j) Rs[j] = gs[j].s->part_.Rs;
    const uint32_t* first_prev[kMaxGroup] = {nullptr, nullptr, nullptr, nullptr};
    for (size_t l = 0; l < L; ++l) {
      // Layer l's first roots ARE layer l - 1's roots, with the same timestamps (all_nodes =
      // roots ++ neighbours): with most-recent sampling and the same fanout their k most recent
      // neighbours are what the previous block already holds, so they are neither bucketed nor
      // requested nor sampled again — the merge copies their edges out of the previous block
      // (the reference requests every root of every layer, dist_sampler.py:174-186).
      const bool reuse = a.layer_reuses_roots(reuse_roots, l);
      GroupLayout lay;
      a.group_layout(Rs, m, static_cast<uint32_t>(l), P, slack, slot_roots, narrow, edge_fill, &lay,
                     reuse_roots);
      GF_REQUIRE(off + lay.total <= ws_bytes, "sample_partitioned_group: workspace too small");
      const size_t rb = narrow ? 12 : 24;
      char* base = w + off;
      const uint32_t F = a.fanouts_[l], stride = static_cast<uint32_t>(lay.stride);
      int64_t* requests = reinterpret_cast<int64_t*>(base + lay.requests);
      int64_t* replies = reinterpret_cast<int64_t*>(base + lay.replies);
      const int64_t* roots[kMaxGroup]; const float* ts[kMaxGroup]; const uint64_t* d_R[kMaxGroup];
      uint64_t R_host[kMaxGroup];
      size_t bound = 0;
      for (int j = 0; j < m; ++j) {
        Sampler& s = *gs[j].s;
        s.part_roots(static_cast<uint32_t>(l), 0, &roots[j], &ts[j], &d_R[j], &R_host[j]);
        bound = std::max(bound, l == 0 ? s.part_.R : s.root_bound(s.part_.Rs, l));
      }
      // 1. all plans
      PlanJob pj[kMaxGroup];
      for (int j = 0; j < m; ++j) {
        pj[j] = PlanJob{roots[j], ts[j], d_R[j], R_host[j], requests,
                        reinterpret_cast<uint32_t*>(base + lay.pos[j]),
                        reinterpret_cast<uint64_t*>(base + lay.counts[j]),
                        gs[j].s->part_overflow(), l == 0 ? 1 : 0, static_cast<uint32_t>(m),
                        static_cast<uint32_t>(j), static_cast<uint32_t>(lay.own[j]),
                        (force_overflow >> j) & 1u};
        if (reuse) {
          const int64_t* r_; const float* t_;
          gs[j].s->part_roots(static_cast<uint32_t>(l - 1), 0, &r_, &t_, &pj[j].d_skip,
                              &pj[j].skip_host);
        }
      }
      partition_plan_jobs(pj, m, bound, P, me, stride, a.graph_->device(), stream);
      lap(1);
      // 2. every sample's request slots out
      if (ex) ex->all_to_all(requests, base + lay.inbox, static_cast<size_t>(m) * stride * 16, stream);
      lap(2);
      // 3. the received slots (of all samples, served alike) and the own shares
      const uint64_t n_inbox = ex ? lay.slot_rows : 0;
      const size_t n_max = std::max<size_t>(n_inbox, bound);
      // group width by the roots there really are (<= the layer's bound per sample), not by the
      // slot rows, most of which are empty: a latency chain wants the 16-lane search
      // (layer 1 of the batch-600 pair: 9.3 -> see profiles/README.md round 4)
      // ... and by ALL the roots of the launch: m samples' layers together no longer fit the
      // GPU with 16 lanes per root, and the launch shares the GPU with the other lanes' chains
      // and the fetch kernels, so roots in flight per wave count for more than search rounds:
      // 2 lanes per root from 4 096 roots on (batch 600, 4 samples per chain, one rank over
      // RCCL: 56.7 us per step with 16 lanes, 50.7 with 4, 46.8 with 2, 43.8 with 2 also for
      // the 7 200-root first layer; profiles/README.md round 4)
      constexpr int kChainWidth = 2;
      constexpr size_t kChainSmall = 4096;
      const int width = static_cast<size_t>(m) * bound > kChainSmall ? kChainWidth : a.search_group_;
      const unsigned grid = capped_grid(n_max, kSearchThreads / width, 256 * 8);
      const PaddedCommon pc{0, 1, a.window_, F, a.policy_ == GF_SAMPLING_POLICY_UNIFORM ? 1 : 0,
                            a.prop_time_ ? 1 : 0, a.seed_, narrow ? 1 : 0};
      PaddedJobs jobs;
      jobs.j[0] = PaddedJob{reinterpret_cast<const int64_t*>(base + lay.inbox), n_inbox, a.calls_++,
                            reinterpret_cast<int64_t*>(base + lay.served), nullptr, nullptr, 0,
                            nullptr, nullptr, stride, static_cast<uint32_t>(m * P),
                            a.part_overflow()};
      jobs.j[0].m = static_cast<uint32_t>(m);
      for (int j = 0; j < m; ++j) jobs.j[0].d_overflow_of[j] = gs[j].s->part_overflow();
      const bool compact = ex != nullptr && lay.edge_cap > 0;
      if (compact) jobs.j[0].row_cnt = reinterpret_cast<uint32_t*>(base + lay.row_cnt);
      for (int j = 0; j < m; ++j) {
        PaddedJob& own = jobs.j[1 + j];
        own = PaddedJob{requests, 0, gs[j].s->calls_++, replies,
                        reinterpret_cast<const uint64_t*>(base + lay.counts[j]) + me, d_R[j],
                        R_host[j], nullptr, nullptr, stride, static_cast<uint32_t>(m * P), nullptr};
        own.own_skip = lay.own[j];
      }
      {
        ProfileScope ps(kProfSearch, stream);
        launch_padded_group(width, grid, 1 + m, stream, view_for(a.graph_, bound), pc, jobs);
        GF_HIP(hipGetLastError());
      }
      lap(3);
      // 4. the replies back: the sampled edges packed per slot (compact), or the fixed slots
      if (compact) {
        if (!a.part_ticket_.data()) {
          a.part_ticket_.reserve(256);
          GF_HIP(hipMemsetAsync(a.part_ticket_.data(), 0, 256, stream));
        }
        if (++a.part_tag_ == 0) ++a.part_tag_;   // (a zeroed ticket must never look current)
        launch_reply_compact(
            CompactArgs{reinterpret_cast<const int64_t*>(base + lay.inbox), base + lay.served,
                        reinterpret_cast<const uint32_t*>(base + lay.row_cnt), base + lay.cserved,
                        a.part_ticket_.as<unsigned long long>(), stride, F,
                        static_cast<uint32_t>(m), static_cast<uint32_t>(P),
                        static_cast<uint32_t>(lay.edge_cap), static_cast<uint32_t>(lay.cslot),
                        narrow ? 1u : 0u, static_cast<uint32_t>(lay.off_bytes), a.part_tag_},
            static_cast<unsigned>(m * P), stream);
        GF_HIP(hipGetLastError());
        ex->all_to_all(base + lay.cserved, base + lay.creplies, static_cast<size_t>(m) * lay.cslot, stream);
      } else if (ex) {
        ex->all_to_all(base + lay.served, replies, static_cast<size_t>(m) * stride * F * rb, stream);
      }
      lap(4);
      // 5. all merges
      MergeJobs mj;
      for (int j = 0; j < m; ++j) {
        Sampler& s = *gs[j].s;
        uint64_t* cslot = s.part_counts() + 2 * l;
        const BlockPtrs& out = s.part_.slot->ptrs[l];
        mj.j[j] = MergeJob{roots[j], ts[j], d_R[j], R_host[j], replies,
                           reinterpret_cast<const uint32_t*>(base + lay.pos[j]),
                           static_cast<uint32_t>(lay.slot_rows),
                           reinterpret_cast<uint64_t*>(s.ws_.as<char>()), next_merge_tag(),
                           s.part_overflow(), out.all_nodes, out.all_ts, out.dt, out.eids, out.row,
                           out.col, cslot, cslot + 1, (l + 1 < L) ? cslot + 2 : nullptr};
        if (compact) {
          mj.j[j].crep = base + lay.creplies;
          mj.j[j].cslot = static_cast<uint32_t>(lay.cslot);
          mj.j[j].edge_cap = static_cast<uint32_t>(lay.edge_cap);
          mj.j[j].m = static_cast<uint32_t>(m);
          mj.j[j].jidx = static_cast<uint32_t>(j);
          mj.j[j].off_bytes = static_cast<uint32_t>(lay.off_bytes);
        }
        mj.j[j].first_out = reinterpret_cast<uint32_t*>(base + lay.first[j]);
        if (reuse) {
          const int64_t* r_; const float* t_;
          s.part_roots(static_cast<uint32_t>(l - 1), 0, &r_, &t_, &mj.j[j].d_R_prev,
                       &mj.j[j].R_prev_host);
          const BlockPtrs& pb = s.part_.slot->ptrs[l - 1];
          mj.j[j].first_prev = first_prev[j];
          mj.j[j].nodes_prev = pb.all_nodes;
          mj.j[j].ts_prev = pb.all_ts;
          mj.j[j].dt_prev = pb.dt;
          mj.j[j].eids_prev = pb.eids;
        }
        first_prev[j] = reinterpret_cast<const uint32_t*>(base + lay.first[j]);
      }
      {
        ProfileScope ps(kProfEmit, stream);
        const unsigned egrid = static_cast<unsigned>(
            (static_cast<uint64_t>(std::max<size_t>(bound, 1)) * F + kEmitThreads - 1) /
            kEmitThreads);
        launch_merge_fused_group(mj, egrid, m, F, stride, narrow ? (a.prop_time_ ? 2 : 1) : 0,
                                 stream);
        GF_HIP(hipGetLastError());
      }
      lap(5);
      off += lay.total;
    }
    PublishGroup pg;
    for (int j = 0; j < m; ++j) gs[j].s->part_commit_prepare(pg.p[j]);
    launch_publish_group(pg, m, stream);
    GF_HIP(hipGetLastError());
    for (int j = 0; j < m; ++j) gs[j].s->part_commit_finish();
    lap(6);
    part_host_add(7, static_cast<uint64_t>(m));   // samples
  } catch (...) {
    abort_all();
    throw;
  }
}

}  // namespace gf
