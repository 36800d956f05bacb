// The owner's half of partitioned sampling: search + select in ONE launch into a fixed
// `fanout` slots per request row, so the output size follows from the row count and nothing is
// read back.  One job per launch, the inbox and the own share as a pair, or a group's five.
#include "sampler_ctx.hpp"
#include "partition.hpp"

#include "../../include/gnnflow_rng.h"

namespace gf {

namespace {

// d_own != null: "this rank's own share" of a chained partitioned layer — the last *d_own
// of the layer's R request rows (R = *d_total, or total_host), counts still on the device.
// root_of / rec_cnt (own share only): the number of valid slots of every row goes straight
// to its root's counter, so the merge does not have to read the rows back to count them.
// stride != 0: the slotted layout (partition.hip).  Own share: it starts at row
// world * stride.  Otherwise `req` is the INBOX of an equal-split exchange — `world` slots of
// `stride` rows, row 0 of a slot its header {rows that follow, flags} — and only the rows
// a header announces are served (reply row = request row); a sender's overflow flag is
// folded into this rank's word, so every rank learns of it in the same exchange.
template <int GROUP>
__device__ inline void padded_job(const GraphView& g, const PaddedCommon& c, const PaddedJob& j) {
  const int64_t* __restrict__ req = j.req;
  int64_t* __restrict__ out = j.out;
  const uint32_t* __restrict__ root_of = j.root_of;
  uint64_t n = j.n;
  const uint32_t fanout = c.fanout, stride = j.stride;
  uint32_t* __restrict__ out32 = reinterpret_cast<uint32_t*>(j.out);
  if (j.d_own) {
    n = *j.d_own;
    const uint64_t skip = stride ? (j.own_skip ? j.own_skip : static_cast<uint64_t>(j.world) * stride)
                                 : (j.d_total ? *j.d_total : j.total_host) - n;
    req += 2 * skip;
    if (c.narrow) out32 += skip * fanout * 3;   // rows of fanout x 12 B
    else out += skip * fanout * 3;              // rows of fanout x 24 B
    if (root_of) root_of += skip;
  }
  constexpr int kGroupsPerBlock = kSearchThreads / GROUP;
  const int lane = threadIdx.x % GROUP;
  const int group_in_wave = (threadIdx.x % 64) / GROUP;
  const uint64_t group = static_cast<uint64_t>(blockIdx.x) * kGroupsPerBlock + threadIdx.x / GROUP;
  const uint64_t num_groups = static_cast<uint64_t>(gridDim.x) * kGroupsPerBlock;
  const bool inbox = stride && !j.d_own;
  for (uint64_t r = group; r < n; r += num_groups) {
    if (inbox) {
      const uint64_t q = r / stride, jj = r - q * stride;
      if (jj == 0) {
        if (lane == 0 && (req[2 * r + 1] & 1))
          atomicOr(j.m ? j.d_overflow_of[q % j.m] : j.d_overflow, 1u);
        continue;
      }
      const uint64_t rows = static_cast<uint64_t>(req[2 * q * stride]);
      if (jj - 1 >= min(rows, static_cast<uint64_t>(stride - 1))) continue;
    }
    const int64_t nid = req[2 * r];
    const float t = __uint_as_float(static_cast<uint32_t>(static_cast<uint64_t>(req[2 * r + 1])));
    float start, end;
    time_window(t, c.snapshot_idx, c.num_snapshots, c.window, &start, &end);
    uint64_t end_off = 0;
    uint32_t n_cand = 0;
    if (nid >= 0 && static_cast<uint64_t>(nid) < g.table_len) {
      const NodeEntry e = g.table[nid];
      if (e.size > 0) {
        uint32_t lo, hi;
        window_bounds<GROUP>(g, e, start, end, lane, group_in_wave, &lo, &hi);
        n_cand = hi > lo ? hi - lo : 0;
        end_off = e.start + hi;
      }
    }
    const uint32_t valid = valid_slots(n_cand, fanout, c.uniform);
    if (j.rec_cnt && lane == 0) j.rec_cnt[root_of[r]] = valid;
    if (j.row_cnt && lane == 0) j.row_cnt[r] = valid;
    for (uint32_t k = lane; k < fanout; k += GROUP) {
      const uint64_t slot = r * fanout + k;
      if (c.narrow) {
        uint32_t* o = out32 + slot * 3;
        if (k < valid) {
          const uint32_t pick = c.uniform ? gf_philox4x32_10_first(c.seed, slot, j.call) % n_cand : k;
          const EdgePair nb = g.nbr_pool[end_off - 1 - pick];
          o[0] = static_cast<uint32_t>(nb.dst);
          o[1] = static_cast<uint32_t>(nb.eid);
          o[2] = __float_as_uint(nb.ts);
        } else {
          o[0] = 0xFFFFFFFFu;
          o[1] = 0xFFFFFFFFu;
          o[2] = 0xFFFFFFFFu;
        }
        continue;
      }
      int64_t* o = out + slot * 3;
      if (k < valid) {
        const uint32_t pick = c.uniform ? gf_philox4x32_10_first(c.seed, slot, j.call) % n_cand : k;
        const uint64_t e = end_off - 1 - pick;
        const EdgePair nb = g.nbr_pool[e];
        const float ets = nb.ts;
        o[0] = nb.dst;
        o[1] = nb.eid;
        o[2] = pack_f32_pair(c.prop_time ? t : ets, t - ets);
      } else {
        o[0] = -1;
        o[1] = -1;
        o[2] = -1;
      }
    }
  }
}

template <int GROUP>
__global__ __launch_bounds__(kSearchThreads) void sample_padded_kernel(
    GraphView g, const int64_t* __restrict__ req, uint64_t n, uint32_t snapshot_idx,
    uint32_t num_snapshots, float window, uint32_t fanout, int uniform, int prop_time,
    uint64_t seed, uint64_t call, int64_t* __restrict__ out,
    const uint64_t* __restrict__ d_own, const uint64_t* __restrict__ d_total,
    uint64_t total_host, const uint32_t* __restrict__ root_of, uint32_t* __restrict__ rec_cnt,
    uint32_t stride, uint32_t world, uint32_t* __restrict__ d_overflow) {
  const PaddedCommon c{snapshot_idx, num_snapshots, window, fanout, uniform, prop_time, seed};
  padded_job<GROUP>(g, c, PaddedJob{req, n, call, out, d_own, d_total, total_host, root_of, rec_cnt,
                                    stride, world, d_overflow});
}

// Two jobs in one launch (blockIdx.y): the requests this rank received AND its own share —
// one launch and one kernel boundary less per layer when the exchange runs in the sampling
// stream (nothing to overlap the own share with).
template <int GROUP>
__global__ __launch_bounds__(kSearchThreads) void sample_padded_pair_kernel(
    GraphView g, PaddedCommon c, PaddedJob a, PaddedJob b) {
  if (blockIdx.y == 0) padded_job<GROUP>(g, c, a);
  else padded_job<GROUP>(g, c, b);
}
// ... and up to five: the shared inbox of m <= 4 samples and their own shares
template <int GROUP>
__global__ __launch_bounds__(kSearchThreads) void sample_padded_group_kernel(
    GraphView g, PaddedCommon c, PaddedJobs jobs) {
  padded_job<GROUP>(g, c, jobs.j[blockIdx.y]);
}

template <typename... Args>
void launch_padded(int width, unsigned grid, hipStream_t stream, Args... args) {
  switch (width) {
    case 2: sample_padded_kernel<2><<<dim3(grid), dim3(kSearchThreads), 0, stream>>>(args...); break;
    case 4: sample_padded_kernel<4><<<dim3(grid), dim3(kSearchThreads), 0, stream>>>(args...); break;
    case 8: sample_padded_kernel<8><<<dim3(grid), dim3(kSearchThreads), 0, stream>>>(args...); break;
    default: sample_padded_kernel<16><<<dim3(grid), dim3(kSearchThreads), 0, stream>>>(args...); break;
  }
}

void launch_padded_pair(int width, unsigned grid, hipStream_t stream, const GraphView& g,
                        const PaddedCommon& c, const PaddedJob& a, const PaddedJob& b) {
  const dim3 gr(grid, 2), bl(kSearchThreads);
  switch (width) {
    case 2: sample_padded_pair_kernel<2><<<gr, bl, 0, stream>>>(g, c, a, b); break;
    case 4: sample_padded_pair_kernel<4><<<gr, bl, 0, stream>>>(g, c, a, b); break;
    case 8: sample_padded_pair_kernel<8><<<gr, bl, 0, stream>>>(g, c, a, b); break;
    default: sample_padded_pair_kernel<16><<<gr, bl, 0, stream>>>(g, c, a, b); break;
  }
}

}  // namespace

void launch_padded_group(int width, unsigned grid, int jobs_n, hipStream_t stream,
                         const GraphView& g, const PaddedCommon& c, const PaddedJobs& jobs) {
  const dim3 gr(grid, static_cast<unsigned>(jobs_n)), bl(kSearchThreads);
  switch (width) {
    case 2: sample_padded_group_kernel<2><<<gr, bl, 0, stream>>>(g, c, jobs); break;
    case 4: sample_padded_group_kernel<4><<<gr, bl, 0, stream>>>(g, c, jobs); break;
    case 8: sample_padded_group_kernel<8><<<gr, bl, 0, stream>>>(g, c, jobs); break;
    default: sample_padded_group_kernel<16><<<gr, bl, 0, stream>>>(g, c, jobs); break;
  }
}

// ---- partitioned sampling ------------------------------------------------------------
void Sampler::sample_layer_padded(const int64_t* d_requests, size_t n, uint32_t layer,
                                  uint32_t snapshot, int64_t* d_out, hipStream_t stream) {
  GF_REQUIRE(layer < fanouts_.size(), "sample_layer_padded: layer out of range");
  GF_REQUIRE(snapshot < num_snapshots_, "sample_layer_padded: snapshot out of range");
  const uint64_t call = calls_++;
  if (n == 0) return;
  GF_REQUIRE(d_requests && d_out, "sample_layer_padded: null device pointer");
  const uint32_t F = fanouts_[layer];
  GF_REQUIRE(static_cast<uint64_t>(n) * F < 0xFFFFFFFFull,
             "sampler: more than 2^32-1 slots in one layer");
  DeviceGuard dg(graph_->device());
  const GraphView gv = view_for(graph_, n);
  const int uniform = policy_ == GF_SAMPLING_POLICY_UNIFORM;
  const int width = n > kSmallRoots ? large_group_ : search_group_;
  const unsigned grid = capped_grid(n, kSearchThreads / width, 256 * 8);
  ProfileScope ps(kProfSearch, stream);
  launch_padded(width, grid, stream, gv, d_requests, static_cast<uint64_t>(n), snapshot,
                num_snapshots_, window_, F, uniform, prop_time_ ? 1 : 0, seed_, call, d_out,
                static_cast<const uint64_t*>(nullptr), static_cast<const uint64_t*>(nullptr),
                static_cast<uint64_t>(0), static_cast<const uint32_t*>(nullptr),
                static_cast<uint32_t*>(nullptr), 0u, 0u, static_cast<uint32_t*>(nullptr));
  GF_HIP(hipGetLastError());
}

void Sampler::part_plan_own(uint32_t layer, uint32_t snapshot, void* d_ws, size_t ws_bytes,
                            int phases) {
  GF_REQUIRE(part_.active, "part_plan_own: no partitioned sample is being built");
  GF_REQUIRE(layer < fanouts_.size() && snapshot < num_snapshots_, "part_plan_own: out of range");
  gf_part_layout lay;
  part_layout(part_.Rs, layer, part_.world, part_.slack, part_.slot_roots, &lay);
  GF_REQUIRE(d_ws && ws_bytes >= lay.total, "part_plan_own: workspace too small");
  DeviceGuard dg(graph_->device());
  char* w = static_cast<char*>(d_ws);
  const int64_t* roots; const float* ts; const uint64_t* d_R; uint64_t R_host;
  part_roots(layer, snapshot, &roots, &ts, &d_R, &R_host);
  hipStream_t stream = part_.stream;
  const size_t Rb = lay.root_bound;
  const uint32_t stride = static_cast<uint32_t>(lay.slot_stride);
  uint64_t* d_counts = reinterpret_cast<uint64_t*>(w + lay.counts);
  if (!(phases & 1)) {
    // planned by an earlier call
  } else if (layer == 0 && part_.R == 0 && !stride) {
    GF_HIP(hipMemsetAsync(d_counts, 0, part_.world * sizeof(uint64_t), stream));
  } else {
    // slotted: the sample's first plan STORES the overflow word (the workspace is shared by
    // the samples in flight on this stream), the later ones only raise it
    partition_plan_dev(roots, ts, d_R, layer == 0 ? part_.R : Rb, part_.world, part_.rank,
                       reinterpret_cast<int64_t*>(w + lay.requests),
                       reinterpret_cast<uint32_t*>(w + lay.pos), d_counts, w + lay.scratch,
                       lay.scratch_bytes, graph_->device(), stream,
                       (part_own_counts(layer == 0 ? part_.R : Rb) &&
                        !part_fused_merge(layer == 0 ? part_.R : Rb, fanouts_[layer]))
                           ? part_root_of() : nullptr,
                       stride, stride ? part_overflow() : nullptr,
                       layer == 0 && snapshot == 0 ? 1 : 0);
  }
  if (!(phases & 2)) return;
  // this rank's own share: the last counts[rank] request rows (slotted: the rows from
  // world * stride on); the kernel takes the count from the device, so with one rank nothing
  // is read back, and with several the caller issues it right after starting the request
  // exchange, which it then overlaps
  const uint64_t call = calls_++;
  const uint32_t F = fanouts_[layer];
  const size_t n_bound = layer == 0 ? part_.R : Rb;
  if (n_bound) {
    const int width = n_bound > kSmallRoots ? large_group_ : search_group_;
    const unsigned grid = capped_grid(n_bound, kSearchThreads / width, 256 * 8);
    ProfileScope ps(kProfSearch, stream);
    launch_padded(width, grid, stream, view_for(graph_, n_bound),
                  reinterpret_cast<const int64_t*>(w + lay.requests), static_cast<uint64_t>(0),
                  snapshot, num_snapshots_, window_, F, policy_ == GF_SAMPLING_POLICY_UNIFORM ? 1 : 0,
                  prop_time_ ? 1 : 0, seed_, call, reinterpret_cast<int64_t*>(w + lay.replies),
                  static_cast<const uint64_t*>(d_counts + part_.rank), d_R,
                  static_cast<uint64_t>(R_host), static_cast<const uint32_t*>(part_root_of()),
                  (part_own_counts(n_bound) && !part_fused_merge(n_bound, F))
                      ? part_rec_cnt() : static_cast<uint32_t*>(nullptr),
                  stride, static_cast<uint32_t>(part_.world), static_cast<uint32_t*>(nullptr));
    GF_HIP(hipGetLastError());
  }
}

// Slotted form: serves the request inbox (what the equal-split exchange delivered: one slot per
// rank) from this rank's shard into `served`, reply row = request row; the caller sends
// `served` back slot for slot into the prefix of the reply buffer.
void Sampler::part_serve(uint32_t layer, uint32_t snapshot, void* d_ws, size_t ws_bytes,
                         bool with_own) {
  GF_REQUIRE(part_.active, "part_serve: no partitioned sample is being built");
  GF_REQUIRE(layer < fanouts_.size() && snapshot < num_snapshots_, "part_serve: out of range");
  gf_part_layout lay;
  part_layout(part_.Rs, layer, part_.world, part_.slack, part_.slot_roots, &lay);
  GF_REQUIRE(lay.slot_stride, "part_serve: the sample was not begun in the slotted form");
  GF_REQUIRE(d_ws && ws_bytes >= lay.total, "part_serve: workspace too small");
  DeviceGuard dg(graph_->device());
  char* w = static_cast<char*>(d_ws);
  hipStream_t stream = part_.stream;
  const uint64_t call = calls_++;
  const uint32_t F = fanouts_[layer];
  const uint32_t stride = static_cast<uint32_t>(lay.slot_stride);
  const uint64_t n = static_cast<uint64_t>(part_.world) * stride;
  GF_REQUIRE(n * F < 0xFFFFFFFFull, "sampler: more than 2^32-1 slots in one layer");
  if (with_own) {
    // the received requests and this rank's own share in ONE launch (part_plan_own phase 2 is
    // then not called for this layer)
    const int64_t* roots; const float* ts; const uint64_t* d_R; uint64_t R_host;
    part_roots(layer, snapshot, &roots, &ts, &d_R, &R_host);
    const size_t n_bound = layer == 0 ? part_.R : lay.root_bound;
    const uint64_t call_own = calls_++;
    const size_t n_max = std::max<size_t>(n, n_bound);
    // width by the layer's roots, not by the (mostly empty) slot rows
    const size_t n_real = std::max<size_t>(lay.root_bound, n_bound);
    const int width = n_real > kSmallRoots ? large_group_ : search_group_;
    const unsigned grid = capped_grid(n_max, kSearchThreads / width, 256 * 8);
    uint64_t* d_counts = reinterpret_cast<uint64_t*>(w + lay.counts);
    const PaddedCommon pc{snapshot, num_snapshots_, window_, F,
                          policy_ == GF_SAMPLING_POLICY_UNIFORM ? 1 : 0, prop_time_ ? 1 : 0, seed_};
    const PaddedJob serve{reinterpret_cast<const int64_t*>(w + lay.inbox), n, call,
                          reinterpret_cast<int64_t*>(w + lay.served), nullptr, nullptr, 0, nullptr,
                          nullptr, stride, static_cast<uint32_t>(part_.world), part_overflow()};
    const PaddedJob own{reinterpret_cast<const int64_t*>(w + lay.requests), 0, call_own,
                        reinterpret_cast<int64_t*>(w + lay.replies), d_counts + part_.rank, d_R,
                        R_host, part_root_of(),
                        (part_own_counts(n_bound) && !part_fused_merge(n_bound, F))
                            ? part_rec_cnt() : nullptr, stride,
                        static_cast<uint32_t>(part_.world), nullptr};
    ProfileScope ps(kProfSearch, stream);
    launch_padded_pair(width, grid, stream, view_for(graph_, n_real), pc, serve, own);
    GF_HIP(hipGetLastError());
    return;
  }
  const int width = n > kSmallRoots ? large_group_ : search_group_;
  const unsigned grid = capped_grid(n, kSearchThreads / width, 256 * 8);
  ProfileScope ps(kProfSearch, stream);
  launch_padded(width, grid, stream, view_for(graph_, n),
                reinterpret_cast<const int64_t*>(w + lay.inbox), n, snapshot, num_snapshots_,
                window_, F, policy_ == GF_SAMPLING_POLICY_UNIFORM ? 1 : 0, prop_time_ ? 1 : 0,
                seed_, call, reinterpret_cast<int64_t*>(w + lay.served),
                static_cast<const uint64_t*>(nullptr), static_cast<const uint64_t*>(nullptr),
                static_cast<uint64_t>(0), static_cast<const uint32_t*>(nullptr),
                static_cast<uint32_t*>(nullptr), stride, static_cast<uint32_t>(part_.world),
                part_overflow());
  GF_HIP(hipGetLastError());
}

}  // namespace gf
