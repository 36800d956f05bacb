// Temporal neighbour sampling on MI355X (gfx950).
//
// Replaces gnnflow/csrc/sampling_kernels.cu (SampleLayerRecentKernel :11-107,
// SampleLayerUniformKernel :109-273), the thrust::remove_if compaction
// (temporal_sampler.cu:191-204) and the host-side result assembly
// (temporal_sampler.cu:236-274) with three launches per (layer, snapshot), all
// device resident:
//
//   1. search : one 16-lane group per root (4 lanes in large layers).  Resolves the root's time
//               window ONCE (the reference repeats the block walk and both binary
//               searches in each of the F slot threads) with a group-wide k-ary
//               search over the node's flat timestamp segment: every round the
//               group's lanes probe GROUP pivots in parallel and a ballot/popcount
//               picks the sub-range, so a window over 4096 edges is found in 2
//               dependent memory round trips at GROUP=64 instead of 12.
//   2. scan   : exclusive prefix sum of the per-root valid-slot counts (wave
//               shuffles + LDS), which gives every root its base in the compacted
//               output and the layer's edge count S (and R' = R + S, the next
//               layer's root count, which never leaves HBM).
//   3. emit   : one thread per (root, slot): reads the selected edge (one 32 B
//               {dst, eid, ts} record = one DRAM sector) and writes the final MFG
//               arrays (all_nodes, all_timestamps, delta_timestamps, eids, row, col)
//               directly at base[root] + slot, i.e. already compacted, root-major,
//               newest first — the order thrust's stable remove_if leaves.
//
// Equivalence with the reference's per-block case analysis
// (sampling_kernels.cu:55-86): for chronologically ingested edges the union over
// blocks of [LowerBound(start), LowerBound(end)) equals
// [lower_bound(start), lower_bound(end)) on the node's concatenated sequence, and
// "j-th most recent, spilling to the previous block" (:88-92) is index
// end-1-j on that sequence.  tests/ proves it against the block-walking oracle.
#include "sampler_ctx.hpp"
#include "partition.hpp"

#include <sched.h>

#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>

namespace gf {

// ---- host driver -------------------------------------------------------------------
Sampler::Sampler(EdgeStore* graph, const uint32_t* fanouts, size_t num_layers, int policy,
                 uint32_t num_snapshots, float window, bool prop_time, uint64_t seed)
    : graph_(graph),
      fanouts_(fanouts, fanouts + num_layers),
      policy_(policy),
      num_snapshots_(num_snapshots),
      window_(window),
      prop_time_(prop_time),
      seed_(seed) {
  GF_REQUIRE(graph != nullptr, "sampler: null graph");
  GF_REQUIRE(num_layers > 0, "sampler: fanouts must not be empty");
  for (uint32_t f : fanouts_) GF_REQUIRE(f > 0, "sampler: fanout must be positive");
  GF_REQUIRE(policy == GF_SAMPLING_POLICY_RECENT || policy == GF_SAMPLING_POLICY_UNIFORM,
             "sampler: invalid sampling policy");
  GF_REQUIRE(num_snapshots >= 1, "sampler: num_snapshots must be >= 1");
  search_group_ = group_width_from_env("GNNFLOW_SEARCH_GROUP", 16);
  large_group_ = group_width_from_env("GNNFLOW_SEARCH_GROUP_LARGE", 4);
  {
    const char* v = std::getenv("GNNFLOW_SAMPLER_HYBRID_SEARCH");   // tests
    hybrid_search_ = !(v && std::atoi(v) == 0);
  }
  DeviceGuard dg(graph_->device());
  for (InFlight& f : ring_) GF_HIP(hipEventCreateWithFlags(&f.done, hipEventDisableTiming));
  rec_words_ = 2 + 2 * num_layers * num_snapshots;   // flag, {R, S} per block, overflow
  h_counts_.reserve(kMaxInFlight * rec_words_ * sizeof(uint64_t));
  std::memset(h_counts_.data(), 0, kMaxInFlight * rec_words_ * sizeof(uint64_t));
  h_layer_counts_.reserve(2 * sizeof(uint64_t));
  // (own_stream_ — the stream of the host-array entry points — is created on first use: every
  // stream a process creates shifts the hardware-queue placement of the ones created after it,
  // and a pipelined loop clones its sampler per lane)
}

Sampler::~Sampler() {
  for (InFlight& f : ring_) {
    if (f.done) {
      (void)hipEventSynchronize(f.done);
      (void)hipEventDestroy(f.done);
    }
  }
  if (own_stream_) {
    (void)hipStreamSynchronize(own_stream_);
    (void)hipStreamDestroy(own_stream_);
  }
}

size_t Sampler::root_bound(size_t R, size_t layer) const {
  size_t b = R;
  for (size_t l = 0; l < layer; ++l) b += b * fanouts_[l];
  return b;
}

// Per-block carve of the output buffer; every array 16-byte aligned.
size_t Sampler::layer_output_bytes(size_t Rb, size_t layer) const {
  const size_t F = fanouts_[layer], Sb = Rb * F;
  return align_up((Rb + Sb) * 8, 16) + align_up((Rb + Sb) * 4, 16) + align_up(Sb * 4, 16) +
         3 * align_up(Sb * 8, 16);
}

Sampler::BlockPtrs Sampler::carve(char* p, size_t Rb, uint32_t F) const {
  const size_t Sb = Rb * F;
  BlockPtrs b;
  b.all_nodes = reinterpret_cast<int64_t*>(p); p += align_up((Rb + Sb) * 8, 16);
  b.eids = reinterpret_cast<int64_t*>(p);      p += align_up(Sb * 8, 16);
  b.row = reinterpret_cast<int64_t*>(p);       p += align_up(Sb * 8, 16);
  b.col = reinterpret_cast<int64_t*>(p);       p += align_up(Sb * 8, 16);
  b.all_ts = reinterpret_cast<float*>(p);      p += align_up((Rb + Sb) * 4, 16);
  b.dt = reinterpret_cast<float*>(p);
  return b;
}

size_t Sampler::output_bytes(size_t R) const {
  size_t total = 0;
  for (size_t l = 0; l < fanouts_.size(); ++l)
    total += num_snapshots_ * layer_output_bytes(root_bound(R, l), l);
  return total;
}

void Sampler::reserve_workspace(size_t Rb, size_t num_blocks, hipStream_t stream) {
  if (Rb <= ws_roots_ && num_blocks <= ws_blocks_) return;
  ws_roots_ = std::max(ws_roots_, Rb);
  ws_blocks_ = std::max(ws_blocks_, num_blocks);
  size_t bytes = align_up(ws_roots_ * 8, 16) + 3 * align_up(ws_roots_ * 4, 16) +
                 ws_blocks_ * 2 * sizeof(uint64_t) + 64;
  // kernels of earlier samples may still be queued on `stream` with the old workspace: it
  // is retired behind an event and freed later (stream-ordered swap, no stall)
  retired_.collect();
  DeviceBuffer fresh;
  fresh.reserve(bytes, 0, stream);
  // the first array doubles as the fused merge's granules: no stale tag in fresh memory
  GF_HIP(hipMemsetAsync(fresh.data(), 0, align_up(ws_roots_ * 8, 16), stream));
  std::swap(ws_, fresh);
  retired_.retire(std::move(fresh), stream);
}

// TemporalSampler::Sample, temporal_sampler.cu:279-305 — split in two so a caller can
// overlap the sampling of batch i+1 (on its own stream) with other work on batch i:
// begin() enqueues every kernel plus the size read-back and returns; end() waits on the
// completion event and reports the block sizes.
void Sampler::sample_begin(const int64_t* d_roots, const float* d_ts, size_t R, void* d_out,
                           size_t out_bytes, hipStream_t stream) {
  const size_t L = fanouts_.size(), NS = num_snapshots_;
  InFlight* slot;
  {
    std::lock_guard<std::mutex> lk(ring_mu_);
    GF_REQUIRE(ring_count_ < kMaxInFlight, "sample_begin: too many samples in flight on this sampler");
    if (ring_count_ > 0) {
      const InFlight& newest = ring_[(ring_head_ + ring_count_ - 1) % kMaxInFlight];
      GF_REQUIRE(newest.roots == 0 || R == 0 || newest.stream == stream,
                 "sample_begin: samples in flight on one sampler must share a stream");
    }
    slot = &ring_[(ring_head_ + ring_count_) % kMaxInFlight];
  }
  // (only this thread begins samples: the slot stays free until ring_count_ is bumped below)
  slot->ptrs.assign(L * NS, BlockPtrs{});
  slot->roots = R;
  slot->by_event = false;
  slot->stream = stream;
  if (R == 0) {  // temporal_sampler.cu:107-114
    calls_ += L * NS;
    std::lock_guard<std::mutex> lk(ring_mu_);
    ++ring_count_;
    return;
  }
  GF_REQUIRE(d_roots && d_ts && d_out, "sample: null device pointer");
  GF_REQUIRE(out_bytes >= output_bytes(R), "sample: output buffer too small");
  DeviceGuard dg(graph_->device());
  reserve_workspace(root_bound(R, L - 1), L * NS, stream);
  uint64_t* d_counts = reinterpret_cast<uint64_t*>(
      ws_.as<char>() + align_up(ws_roots_ * 8, 16) + 3 * align_up(ws_roots_ * 4, 16));

  std::vector<BlockPtrs>& ptrs = slot->ptrs;
  char* p = static_cast<char*>(d_out);
  for (size_t l = 0; l < L; ++l) {
    const size_t Rb = root_bound(R, l);
    for (size_t s = 0; s < NS; ++s) {
      ptrs[l * NS + s] = carve(p, Rb, fanouts_[l]);
      p += layer_output_bytes(Rb, l);
    }
  }
  slot->seq = ++publish_seq_;
  uint64_t* rec = h_counts_.as<uint64_t>() + (slot->seq % kMaxInFlight) * rec_words_;
  *reinterpret_cast<volatile uint64_t*>(rec) = 0;   // this record's publish is pending
  Publish pub;
  pub.d_counts = d_counts;
  pub.h_counts = rec + 1;   // word 0 is the sequence flag
  pub.h_flag = rec;
  pub.seq = slot->seq;
  pub.num_words = static_cast<uint32_t>(L * NS * 2);
  // No publish kernel: the sample's LAST kernel copies the sizes to pinned memory and the host
  // polls the stream's event for completion — one launch less per sample on the sampling
  // stream (round 4, seven same-box pairs: 32.6-32.8 us per step against 33.0-33.7, and none of
  // the occasional 36-37 us runs against a publish kernel and its flag)
  slot->by_event = true;
  for (size_t l = 0; l < L; ++l) {
    const size_t Rb = root_bound(R, l);
    for (size_t s = 0; s < NS; ++s) {
      const size_t b = l * NS + s;
      uint64_t* cslot = d_counts + 2 * b;
      // the next layer of the same snapshot reads its root count R + S from next_R
      uint64_t* next_R = (l + 1 < L) ? cslot + 2 * NS : nullptr;
      const Publish last = (b + 1 == L * NS) ? pub : Publish{};
      if (l == 0) {
        enqueue_layer(d_roots, d_ts, Rb, nullptr, R, l, s, ptrs[b], cslot, next_R, stream, last);
      } else {
        const BlockPtrs& prev = ptrs[(l - 1) * NS + s];
        enqueue_layer(prev.all_nodes, prev.all_ts, Rb, cslot, 0, l, s, ptrs[b], cslot, next_R,
                      stream, last);
      }
    }
  }
  GF_HIP(hipEventRecord(slot->done, stream));
  std::lock_guard<std::mutex> lk(ring_mu_);
  ++ring_count_;
}

size_t Sampler::in_flight() const {
  std::lock_guard<std::mutex> lk(ring_mu_);
  return ring_count_;
}

void Sampler::sample_end(gf_block* blocks) {
  const size_t L = fanouts_.size(), NS = num_snapshots_;
  GF_REQUIRE(blocks != nullptr, "sample: null blocks array");
  InFlight* slot;
  {
    std::lock_guard<std::mutex> lk(ring_mu_);
    GF_REQUIRE(ring_count_ > 0, "sample_end: no sample in flight");
    slot = &ring_[ring_head_];
  }
  auto pop = [&] {
    std::lock_guard<std::mutex> lk(ring_mu_);
    ring_head_ = (ring_head_ + 1) % kMaxInFlight;
    --ring_count_;
  };
  if (slot->roots == 0) {
    for (size_t b = 0; b < L * NS; ++b) std::memset(&blocks[b], 0, sizeof(gf_block));
    last_overflow_ = false;
    pop();
    return;
  }
  DeviceGuard dg(graph_->device());
  // spin on the pinned sequence word (sub-microsecond reaction); fall back to the event
  // if the kernel has not published after a generous number of polls
  const uint64_t* rec = h_counts_.as<uint64_t>() + (slot->seq % kMaxInFlight) * rec_words_;
  volatile const uint64_t* flag = rec;
  bool seen = false;
  if (slot->by_event) {   // completion = the event behind the sample's last kernel
    for (uint64_t spin = 0;; ++spin) {
      const hipError_t q = hipEventQuery(slot->done);
      if (q == hipSuccess) break;
      if (q != hipErrorNotReady) { pop(); GF_HIP(q); }
      if (spin > 4096 && (spin & 63) == 0) sched_yield();
    }
    seen = true;
  }
  for (uint64_t spin = 0; !seen && spin < (1ull << 26); ++spin) {
    if (*flag == slot->seq) { seen = true; break; }
    __builtin_ia32_pause();
    // a short pure spin covers the usual few microseconds; beyond that give the core away
    // (8 ranks per node each have a spinner and an enqueue thread)
    if (spin > 4096 && (spin & 63) == 0) sched_yield();
  }
  if (!seen) {
    const hipError_t e = hipEventSynchronize(slot->done);
    if (e != hipSuccess) { pop(); GF_HIP(e); }
  }
  __atomic_thread_fence(__ATOMIC_ACQUIRE);
  const uint64_t* hc = rec + 1;
  for (size_t b = 0; b < L * NS; ++b) {
    gf_block& o = blocks[b];
    o.all_nodes = slot->ptrs[b].all_nodes;
    o.all_timestamps = slot->ptrs[b].all_ts;
    o.delta_timestamps = slot->ptrs[b].dt;
    o.eids = slot->ptrs[b].eids;
    o.row = slot->ptrs[b].row;
    o.col = slot->ptrs[b].col;
    o.num_dst_nodes = hc[2 * b];
    o.num_edges = hc[2 * b + 1];
    o.num_src_nodes = o.num_dst_nodes + o.num_edges;
  }
  last_overflow_ = hc[2 * L * NS] != 0;
  pop();
}

void Sampler::sample(const int64_t* d_roots, const float* d_ts, size_t R, void* d_out,
                     size_t out_bytes, gf_block* blocks, hipStream_t stream) {
  GF_REQUIRE(blocks != nullptr, "sample: null blocks array");
  sample_begin(d_roots, d_ts, R, d_out, out_bytes, stream);
  sample_end(blocks);
}

// TemporalSampler::SampleLayer, temporal_sampler.cu:97-277
void Sampler::sample_layer(const int64_t* d_roots, const float* d_ts, size_t R, uint32_t layer,
                           uint32_t snapshot, void* d_out, size_t out_bytes, gf_block* block,
                           hipStream_t stream) {
  GF_REQUIRE(layer < fanouts_.size(), "sample_layer: layer out of range");
  GF_REQUIRE(snapshot < num_snapshots_, "sample_layer: snapshot out of range");
  GF_REQUIRE(block != nullptr, "sample_layer: null block");
  if (R == 0) {
    std::memset(block, 0, sizeof(gf_block));
    calls_++;
    return;
  }
  GF_REQUIRE(d_roots && d_ts && d_out, "sample_layer: null device pointer");
  GF_REQUIRE(out_bytes >= layer_output_bytes(R, layer), "sample_layer: output buffer too small");
  DeviceGuard dg(graph_->device());
  reserve_workspace(R, 2, stream);
  uint64_t* d_counts = reinterpret_cast<uint64_t*>(
      ws_.as<char>() + align_up(ws_roots_ * 8, 16) + 3 * align_up(ws_roots_ * 4, 16));
  BlockPtrs ptrs = carve(static_cast<char*>(d_out), R, fanouts_[layer]);
  enqueue_layer(d_roots, d_ts, R, nullptr, R, layer, snapshot, ptrs, d_counts, nullptr, stream,
                Publish{});
  GF_HIP(hipMemcpyAsync(h_layer_counts_.data(), d_counts, 2 * sizeof(uint64_t),
                        hipMemcpyDeviceToHost, stream));
  GF_HIP(hipStreamSynchronize(stream));
  const uint64_t* hc = h_layer_counts_.as<uint64_t>();
  block->all_nodes = ptrs.all_nodes;
  block->all_timestamps = ptrs.all_ts;
  block->delta_timestamps = ptrs.dt;
  block->eids = ptrs.eids;
  block->row = ptrs.row;
  block->col = ptrs.col;
  block->num_dst_nodes = hc[0];
  block->num_edges = hc[1];
  block->num_src_nodes = hc[0] + hc[1];
}

std::atomic<uint64_t> g_part_host_ns[8];
void part_host_add(int stage, uint64_t v) {
  g_part_host_ns[stage].fetch_add(v, std::memory_order_relaxed);
}

// ---- partitioned sampling, chained on the device ------------------------------------------
// part_begin -> for every (layer, snapshot): part_plan_own, [the caller's exchange: request
// all-to-all-v, sample_layer_padded for what it received, reply all-to-all-v], part_merge ->
// part_commit.  Every kernel takes the layer's root count from device memory (it is the
// previous layer's R + S), so nothing is read back between the layers; part_commit publishes
// the block sizes like sample_begin does and sample_end() returns them.  With one rank there
// is no exchange and sample_partitioned() issues the whole chain in one call.
void Sampler::part_layout(size_t R0, uint32_t layer, int world_size, double slack,
                          size_t slot_roots, gf_part_layout* out, bool skip_prev) const {
  GF_REQUIRE(layer < fanouts_.size(), "part_layout: layer out of range");
  GF_REQUIRE(out != nullptr, "part_layout: null output");
  GF_REQUIRE(slack >= 0.0, "part_layout: negative slack");
  const size_t Rb = root_bound(R0, layer), F = fanouts_[layer];
  // slotted form (slack > 0): per-peer capacity = the even share of the worst-case root count
  // times `slack`, never more than the layer can have; rows = P slots of (header + cap) + the
  // own share's region.  The capacity follows from `slot_roots` — the batch size every rank
  // agreed on — not from this rank's own R0: the slots must have the same size on all ranks.
  size_t stride = 0, rows = Rb;
  if (slack > 0.0) {
    // (skip_prev: the layer's first roots — the previous layer's — are not requested again, so
    // the slots hold at most the roots that are new in this layer)
    const size_t Sb = root_bound(std::max<size_t>(slot_roots, 1), layer) -
                      ((skip_prev && layer > 0) ? root_bound(std::max<size_t>(slot_roots, 1), layer - 1) : 0);
    const double share = std::ceil(static_cast<double>(Sb) * slack / world_size);
    const size_t cap = std::max<size_t>(1, std::min<size_t>(Sb, static_cast<size_t>(share)));
    stride = cap + 1;
    rows = static_cast<size_t>(world_size) * stride + Rb;
    GF_REQUIRE(rows < 0xFFFFFFFFull, "part_layout: more than 2^32-1 request rows");
  }
  out->root_bound = Rb;
  out->requests = 0;
  out->replies = rows * 16;
  out->counts = out->replies + rows * F * 24;
  out->pos = out->counts + align_up(static_cast<size_t>(world_size) * 8, 16);
  out->scratch = align_up(out->pos + Rb * 4, 16);
  out->scratch_bytes = partition_scratch_bytes(Rb, world_size);
  size_t end = align_up(out->scratch + out->scratch_bytes, 256);
  out->slot_stride = stride;
  out->inbox = out->served = 0;
  if (stride) {
    const size_t slots = static_cast<size_t>(world_size) * stride;
    out->inbox = end;
    out->served = align_up(out->inbox + slots * 16, 256);
    end = align_up(out->served + slots * F * 24, 256);
  }
  out->total = end;
}

void Sampler::part_begin(const int64_t* d_roots, const float* d_ts, size_t R, void* d_out,
                         size_t out_bytes, int world_size, int rank, double slack,
                         size_t slot_roots, hipStream_t stream) {
  const size_t L = fanouts_.size(), NS = num_snapshots_;
  GF_REQUIRE(!part_.active, "part_begin: a partitioned sample is already being built");
  GF_REQUIRE(world_size >= 1 && rank >= 0 && rank < world_size, "part_begin: bad rank / world");
  GF_REQUIRE(R == 0 || (d_roots && d_ts), "part_begin: null device pointer");
  // layers chain through worst-case-sized blocks even when this rank has no root of its own
  // (R = 0): it still plans, serves the other ranks' requests and merges empty blocks
  const size_t Rs = std::max<size_t>(R, 1);
  GF_REQUIRE(d_out && out_bytes >= output_bytes(Rs), "part_begin: output buffer too small");
  InFlight* slot;
  {
    std::lock_guard<std::mutex> lk(ring_mu_);
    GF_REQUIRE(ring_count_ < kMaxInFlight, "part_begin: too many samples in flight on this sampler");
    slot = &ring_[(ring_head_ + ring_count_) % kMaxInFlight];
  }
  DeviceGuard dg(graph_->device());
  // root_of[] is indexed by request ROW: the slotted form has more rows than roots
  gf_part_layout last;
  part_layout(Rs, static_cast<uint32_t>(L - 1), world_size, slack, slot_roots, &last);
  reserve_workspace(std::max(root_bound(Rs, L - 1), last.replies / 16), L * NS, stream);
  slot->ptrs.assign(L * NS, BlockPtrs{});
  slot->roots = Rs;          // never the "R = 0 short-circuit" record: sizes come from the device
  slot->by_event = false;    // a partitioned sample publishes through its publish kernel
  slot->stream = stream;
  char* p = static_cast<char*>(d_out);
  for (size_t l = 0; l < L; ++l) {
    const size_t Rb = root_bound(Rs, l);
    for (size_t s = 0; s < NS; ++s) {
      slot->ptrs[l * NS + s] = carve(p, Rb, fanouts_[l]);
      p += layer_output_bytes(Rb, l);
    }
  }
  part_ = PartState{};
  part_.active = true;
  part_.slot = slot;
  part_.d_roots = d_roots;
  part_.d_ts = d_ts;
  part_.R = R;
  part_.Rs = Rs;
  part_.world = world_size;
  part_.rank = rank;
  part_.slack = slack;
  part_.slot_roots = slot_roots;
  part_.stream = stream;
}

// the sample-wide "a slot overflowed somewhere" word: behind the block counters
uint32_t* Sampler::part_overflow() const {
  return reinterpret_cast<uint32_t*>(part_counts() + 2 * ws_blocks_);
}

// Scratch of the chained merge in the sampler's workspace (ordered by the stream like the rest
// of it): rec_cnt[i] = valid slots of root i, root_of[row] = root of a request / reply row
// (the workspace's `base` array, which the fused merge does not need).
uint32_t* Sampler::part_rec_cnt() const {
  return reinterpret_cast<uint32_t*>(ws_.as<char>() + align_up(ws_roots_ * 8, 16));
}
uint32_t* Sampler::part_root_of() const {
  return reinterpret_cast<uint32_t*>(ws_.as<char>() + align_up(ws_roots_ * 8, 16) +
                                     align_up(ws_roots_ * 4, 16));
}
// Layers that take the fused merge get their own share's counts from the sampling kernel.
bool Sampler::part_own_counts(size_t root_bound) const {
  return root_bound <= kSmallRoots && root_bound > 0;
}

// Slotted form, layers of <= kSmallRoots roots: the merge is ONE launch (merge_slots_fused_kernel);
// neither the per-root counts nor root_of[] are needed then.  Other layers: the count + emit pair.
bool Sampler::part_fused_merge(size_t root_bound, uint32_t fanout) const {
  return part_.slack > 0.0 && part_own_counts(root_bound) && fanout <= kEmitThreads &&
         (root_bound * fanout + kEmitThreads - 1) / kEmitThreads <= ws_roots_;
}

uint64_t* Sampler::part_counts() const {
  return reinterpret_cast<uint64_t*>(ws_.as<char>() + align_up(ws_roots_ * 8, 16) +
                                     3 * align_up(ws_roots_ * 4, 16));
}

// roots of (layer, snapshot): the caller's for layer 0, else the previous layer's block
void Sampler::part_roots(uint32_t layer, uint32_t snapshot, const int64_t** roots,
                         const float** ts, const uint64_t** d_R, uint64_t* R_host) const {
  const size_t NS = num_snapshots_;
  if (layer == 0) {
    *roots = part_.d_roots;
    *ts = part_.d_ts;
    *d_R = nullptr;
    *R_host = part_.R;
  } else {
    const BlockPtrs& prev = part_.slot->ptrs[(layer - 1) * NS + snapshot];
    *roots = prev.all_nodes;
    *ts = prev.all_ts;
    *d_R = part_counts() + 2 * (layer * NS + snapshot);   // written by the previous merge
    *R_host = 0;
  }
}

// the publish record of the sample being built (its pinned words are reset here)
void Sampler::part_commit_prepare(Publish& pub) {
  GF_REQUIRE(part_.active, "part_commit: no partitioned sample is being built");
  const size_t L = fanouts_.size(), NS = num_snapshots_;
  InFlight* slot = part_.slot;
  part_.active = false;
  slot->seq = ++publish_seq_;
  uint64_t* rec = h_counts_.as<uint64_t>() + (slot->seq % kMaxInFlight) * rec_words_;
  *reinterpret_cast<volatile uint64_t*>(rec) = 0;
  pub.d_counts = part_counts();
  pub.h_counts = rec + 1;
  pub.h_flag = rec;
  pub.seq = slot->seq;
  pub.num_words = static_cast<uint32_t>(L * NS * 2);
  pub.d_extra = part_.slack > 0.0 ? part_overflow() : nullptr;
}

void Sampler::part_commit_finish() {
  GF_HIP(hipEventRecord(part_.slot->done, part_.stream));
  std::lock_guard<std::mutex> lk(ring_mu_);
  ++ring_count_;
}

void Sampler::part_commit() {
  DeviceGuard dg(graph_->device());
  Publish pub;
  part_commit_prepare(pub);
  launch_publish(pub, part_.stream);
  GF_HIP(hipGetLastError());
  part_commit_finish();
}

void Sampler::part_abort() { part_.active = false; }

// one rank: no exchange — the whole chain in one call (begin form: sample_end() completes it)
void Sampler::sample_partitioned(const int64_t* d_roots, const float* d_ts, size_t R, void* d_out,
                                 size_t out_bytes, void* d_ws, size_t ws_bytes,
                                 hipStream_t stream) {
  DeviceGuard dg(graph_->device());   // once for the chain: the steps' own guards then find it set
  const size_t L = fanouts_.size(), NS = num_snapshots_;
  part_begin(d_roots, d_ts, R, d_out, out_bytes, 1, 0, 0.0, 0, stream);
  try {
    char* w = static_cast<char*>(d_ws);
    size_t off = 0;
    for (size_t l = 0; l < L; ++l) {
      gf_part_layout lay;
      part_layout(part_.Rs, static_cast<uint32_t>(l), 1, 0.0, 0, &lay);
      for (size_t s = 0; s < NS; ++s) {
        GF_REQUIRE(off + lay.total <= ws_bytes, "sample_partitioned: workspace too small");
        part_plan_own(static_cast<uint32_t>(l), static_cast<uint32_t>(s), w + off, lay.total, 3);
        part_merge(static_cast<uint32_t>(l), static_cast<uint32_t>(s), w + off, lay.total);
        off += lay.total;
      }
    }
    part_commit();
  } catch (...) {
    part_abort();
    throw;
  }
}

// several ranks: plan -> request slots out (equal split) -> own share + serve -> reply slots back
// -> merge, per (layer, snapshot), all enqueued by this one call (dist.py issues the same chain
// step by step when the exchange has to go through torch.distributed)
void Sampler::sample_partitioned_slotted(const int64_t* d_roots, const float* d_ts, size_t R,
                                         void* d_out, size_t out_bytes, void* d_ws,
                                         size_t ws_bytes, double slack, size_t slot_roots,
                                         Exchange& ex, bool overlap, hipStream_t stream) {
  const size_t L = fanouts_.size(), NS = num_snapshots_;
  GF_REQUIRE(slack > 0.0, "sample_partitioned_slotted: slack must be positive");
  DeviceGuard dg(graph_->device());   // once for the chain: the steps' own guards then find it set
  // host time of the issuing thread per stage (gf_debug_part_host_us): the chain is ~13 stream
  // operations issued by ONE thread, which is what bounds its throughput at batch 600
  using clk = std::chrono::steady_clock;
  auto t_prev = clk::now();
  auto lap = [&](int stage) {
    const auto t = clk::now();
    g_part_host_ns[stage].fetch_add(
        std::chrono::duration_cast<std::chrono::nanoseconds>(t - t_prev).count(),
        std::memory_order_relaxed);
    t_prev = t;
  };
  part_begin(d_roots, d_ts, R, d_out, out_bytes, ex.world(), ex.rank(), slack, slot_roots, stream);
  lap(0);
  try {
    char* w = static_cast<char*>(d_ws);
    size_t off = 0;
    for (size_t l = 0; l < L; ++l) {
      gf_part_layout lay;
      part_layout(part_.Rs, static_cast<uint32_t>(l), part_.world, slack, slot_roots, &lay);
      const size_t slot_rows = lay.slot_stride;
      const size_t F = fanouts_[l];
      for (size_t s = 0; s < NS; ++s) {
        GF_REQUIRE(off + lay.total <= ws_bytes, "sample_partitioned_slotted: workspace too small");
        char* b = w + off;
        const uint32_t li = static_cast<uint32_t>(l), si = static_cast<uint32_t>(s);
        part_plan_own(li, si, b, lay.total, 1);
        lap(1);
        if (overlap) {
          ex.all_to_all_forked(b + lay.requests, b + lay.inbox, slot_rows * 16, stream);
          part_plan_own(li, si, b, lay.total, 2);
          ex.join(stream);
        } else {
          ex.all_to_all(b + lay.requests, b + lay.inbox, slot_rows * 16, stream);
        }
        lap(2);
        part_serve(li, si, b, lay.total, /*with_own=*/!overlap);
        lap(3);
        if (overlap) {   // one communicator, one stream: the reply exchange goes there too
          ex.all_to_all_forked(b + lay.served, b + lay.replies, slot_rows * F * 24, stream);
          ex.join(stream);
        } else {
          ex.all_to_all(b + lay.served, b + lay.replies, slot_rows * F * 24, stream);
        }
        lap(4);
        part_merge(li, si, b, lay.total);
        lap(5);
        off += lay.total;
      }
    }
    part_commit();
    lap(6);
    g_part_host_ns[7].fetch_add(1, std::memory_order_relaxed);   // samples
  } catch (...) {
    part_abort();
    throw;
  }
}

// Host time the issuing thread spent per stage of the slotted chain since the last reset:
// out[0..6] = begin, plan, request exchange, serve, reply exchange, merge, commit (us, summed
// over all samples), out[7] = samples.
void part_host_us(double out[8], bool reset) {
  for (int i = 0; i < 8; ++i) {
    const uint64_t v = reset ? g_part_host_ns[i].exchange(0) : g_part_host_ns[i].load();
    out[i] = i < 7 ? v / 1e3 : static_cast<double>(v);
  }
}

// Copies device-resident blocks into freshly malloc'ed host arrays
// (api.cc:17-24 vec2npy copies likewise).
void Sampler::to_host_blocks(const gf_block* dev, gf_block* host, size_t n, hipStream_t stream) {
  auto dup = [&](const void* d, size_t bytes) -> void* {
    void* h = std::malloc(bytes ? bytes : 1);
    if (!h) throw std::bad_alloc();
    if (bytes) GF_HIP(hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, stream));
    return h;
  };
  for (size_t b = 0; b < n; ++b) {
    const gf_block& d = dev[b];
    gf_block& h = host[b];
    h.num_dst_nodes = d.num_dst_nodes;
    h.num_src_nodes = d.num_src_nodes;
    h.num_edges = d.num_edges;
    h.all_nodes = static_cast<int64_t*>(dup(d.all_nodes, d.num_src_nodes * 8));
    h.all_timestamps = static_cast<float*>(dup(d.all_timestamps, d.num_src_nodes * 4));
    h.delta_timestamps = static_cast<float*>(dup(d.delta_timestamps, d.num_edges * 4));
    h.eids = static_cast<int64_t*>(dup(d.eids, d.num_edges * 8));
    h.row = static_cast<int64_t*>(dup(d.row, d.num_edges * 8));
    h.col = static_cast<int64_t*>(dup(d.col, d.num_edges * 8));
  }
  GF_HIP(hipStreamSynchronize(stream));
}

void Sampler::sample_host(const int64_t* nodes, const float* ts, size_t R, gf_block* blocks) {
  const size_t nb = fanouts_.size() * num_snapshots_;
  if (R == 0) {
    // R = 0 short-circuit (temporal_sampler.cu:107-114): empty arrays, 0 nodes
    calls_ += nb;
    for (size_t b = 0; b < nb; ++b) {
      std::memset(&blocks[b], 0, sizeof(gf_block));
      blocks[b].all_nodes = static_cast<int64_t*>(std::malloc(1));
      blocks[b].all_timestamps = static_cast<float*>(std::malloc(1));
      blocks[b].delta_timestamps = static_cast<float*>(std::malloc(1));
      blocks[b].eids = static_cast<int64_t*>(std::malloc(1));
      blocks[b].row = static_cast<int64_t*>(std::malloc(1));
      blocks[b].col = static_cast<int64_t*>(std::malloc(1));
    }
    return;
  }
  GF_REQUIRE(nodes && ts, "sample: null input array");
  DeviceGuard dg(graph_->device());
  const size_t in_bytes = align_up(R * 8, 16) + align_up(R * 4, 16);
  const size_t out_bytes = output_bytes(R);
  if (!own_stream_) GF_HIP(hipStreamCreateWithFlags(&own_stream_, hipStreamNonBlocking));
  host_io_.reserve(in_bytes + out_bytes, 0, own_stream_);
  char* d = host_io_.as<char>();
  int64_t* d_nodes = reinterpret_cast<int64_t*>(d);
  float* d_ts = reinterpret_cast<float*>(d + align_up(R * 8, 16));
  GF_HIP(hipMemcpyAsync(d_nodes, nodes, R * 8, hipMemcpyHostToDevice, own_stream_));
  GF_HIP(hipMemcpyAsync(d_ts, ts, R * 4, hipMemcpyHostToDevice, own_stream_));
  std::vector<gf_block> dev(nb);
  sample(d_nodes, d_ts, R, d + in_bytes, out_bytes, dev.data(), own_stream_);
  to_host_blocks(dev.data(), blocks, nb, own_stream_);
}

void Sampler::sample_layer_host(const int64_t* nodes, const float* ts, size_t R, uint32_t layer,
                                uint32_t snapshot, gf_block* block) {
  GF_REQUIRE(layer < fanouts_.size(), "sample_layer: layer out of range");
  GF_REQUIRE(snapshot < num_snapshots_, "sample_layer: snapshot out of range");
  if (R == 0) {
    calls_++;
    std::memset(block, 0, sizeof(gf_block));
    block->all_nodes = static_cast<int64_t*>(std::malloc(1));
    block->all_timestamps = static_cast<float*>(std::malloc(1));
    block->delta_timestamps = static_cast<float*>(std::malloc(1));
    block->eids = static_cast<int64_t*>(std::malloc(1));
    block->row = static_cast<int64_t*>(std::malloc(1));
    block->col = static_cast<int64_t*>(std::malloc(1));
    return;
  }
  GF_REQUIRE(nodes && ts, "sample_layer: null input array");
  DeviceGuard dg(graph_->device());
  const size_t in_bytes = align_up(R * 8, 16) + align_up(R * 4, 16);
  const size_t out_bytes = layer_output_bytes(R, layer);
  if (!own_stream_) GF_HIP(hipStreamCreateWithFlags(&own_stream_, hipStreamNonBlocking));
  host_io_.reserve(in_bytes + out_bytes, 0, own_stream_);
  char* d = host_io_.as<char>();
  int64_t* d_nodes = reinterpret_cast<int64_t*>(d);
  float* d_ts = reinterpret_cast<float*>(d + align_up(R * 8, 16));
  GF_HIP(hipMemcpyAsync(d_nodes, nodes, R * 8, hipMemcpyHostToDevice, own_stream_));
  GF_HIP(hipMemcpyAsync(d_ts, ts, R * 4, hipMemcpyHostToDevice, own_stream_));
  gf_block dev;
  sample_layer(d_nodes, d_ts, R, layer, snapshot, d + in_bytes, out_bytes, &dev, own_stream_);
  to_host_blocks(&dev, block, 1, own_stream_);
}

}  // namespace gf
