// ---- planning a pull from sharded feature tables -------------------------------------------
// Cache(distributed=True) (reference: cache.py:288-313,351-388 probe the cache, `unique` the
// missed ids and pull their rows from the owning machine's KVStore, kvstore.py:285-339).  Here
// the owners are the GPUs of the node.  Per fetch round, for up to kMaxCtx contexts (a node
// block, an edge block, cache-free target rows) in the same launches:
//   claim    every missed row claims its id (atomicMax(map[id], -(row + 1)): the lowest row
//            wins — the same claim the gather makes, which it will find settled);
//   count    the rows that TRAVEL — the winners, and every row of a cache-free context — per
//            owner(key) = splitmix64(key) mod P (key: the node id; for edge rows the edge's
//            source node);
//   (the caller exchanges the counts, reads them back — the round's one host synchronisation —
//    and derives the owner-major offsets)
//   scatter  the travelling ids into the compact owner-major send buffer; req_pos[row] = the
//            position of the row's id = the index of its row in the pulled rows, which arrive
//            in the same order.
#include "feature_cache_ctx.hpp"

#include <algorithm>
#include <vector>

namespace gf {

namespace {

__device__ inline int64_t pull_key(const PullCtx& c, uint32_t i) {
  if (!c.key_base) return c.ids[i];
  return c.key_base[c.key_index ? c.key_index[i] : static_cast<int64_t>(i)];
}

__global__ __launch_bounds__(256) void pull_claim_kernel(PullRound r) {
  const PullCtx& c = r.c[blockIdx.y];
  if (!c.map) return;
  const uint32_t stride = gridDim.x * blockDim.x;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < c.n; i += stride) {
    const int64_t id = c.ids[i];
    if (id < 0 || static_cast<uint64_t>(id) >= c.num_ids) continue;
    if (c.map[id] < 0) atomicMax(&c.map[id], -static_cast<int32_t>(i + 1));
  }
}

// does row i travel, and to whom (P = it does not)
__device__ inline uint32_t pull_owner(const PullCtx& c, uint32_t i, OwnerDiv od) {
  if (i >= c.n) return od.P;
  const int64_t id = c.ids[i];
  if (id < 0 || static_cast<uint64_t>(id) >= c.num_ids) return od.P;
  if (c.map && c.map[id] != -static_cast<int32_t>(i + 1)) return od.P;   // hit, or not the winner
  return owner_of(pull_key(c, i), od);
}

template <bool kScatter>
__global__ __launch_bounds__(256) void pull_bucket_kernel(PullRound r) {
  const PullCtx& c = r.c[blockIdx.y];
  const uint32_t P = r.od.P;
  const int lane = threadIdx.x & 63;
  __shared__ uint32_t s_off[64];
  if (kScatter) {   // first send position per owner: the exclusive prefix of the counts
    if (threadIdx.x == 0) {
      uint32_t at = 0;
      for (uint32_t q = 0; q < P; ++q) { s_off[q] = at; at += c.counts[q * c.cstride]; }
    }
    __syncthreads();
  }
  const uint32_t stride = gridDim.x * blockDim.x;
  const uint32_t rounds = (c.n + stride - 1) / stride;   // uniform trip count (ballots inside)
  for (uint32_t k = 0; k < rounds; ++k) {
    const uint32_t i = k * stride + blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t o = pull_owner(c, i, r.od);
    for (uint32_t q = 0; q < P; ++q) {
      const unsigned long long m = __ballot(o == q);
      if (!m) continue;                                   // wave-uniform
      if (!kScatter) {
        if (lane == 0) atomicAdd(&c.counts[q * c.cstride], static_cast<uint32_t>(__popcll(m)));
      } else {
        uint32_t base = 0;
        const int leader = __ffsll(static_cast<long long>(m)) - 1;
        if (lane == leader) base = atomicAdd(&c.cursor[q], static_cast<uint32_t>(__popcll(m)));
        base = __shfl(base, leader, 64);
        if (o == q) {
          const uint32_t at = s_off[q] + base + __popcll(m & ((1ull << lane) - 1ull));
          c.send_ids[at] = c.ids[i];
          c.req_pos[i] = at;
        }
      }
    }
  }
}

}  // namespace

// ---- sharded feature tables: plan, serve, fetch (kernels above: "planning a pull") ---------
namespace {
PullRound make_pull_round(const gf_pull_desc* descs, size_t n, int world, FeatureCache* const* caches,
                          uint32_t* d_counts, uint32_t* d_cursor, size_t* max_rows,
                          uint32_t cstride = 1) {
  GF_REQUIRE(descs != nullptr && n >= 1 && n <= static_cast<size_t>(kMaxCtx),
             "pull: 1..4 contexts per round");
  GF_REQUIRE(world >= 1 && world <= 64, "pull: world size must be 1..64");
  PullRound r;
  std::memset(&r, 0, sizeof(r));
  r.count = static_cast<int>(n);
  r.od = owner_div(static_cast<uint32_t>(world));
  *max_rows = 0;
  for (size_t i = 0; i < n; ++i) {
    const gf_pull_desc& d = descs[i];
    GF_REQUIRE(d.n == 0 || d.d_ids != nullptr, "pull: null ids");
    GF_REQUIRE(d.n < 0x7FFFFFFFull, "pull: more than 2^31-1 rows in one block");
    PullCtx& c = r.c[i];
    c.ids = d.d_ids;
    c.n = static_cast<uint32_t>(d.n);
    c.key_base = d.d_key_base;
    c.key_index = d.d_key_index;
    c.map = caches[i] ? caches[i]->pull_map() : nullptr;
    c.num_ids = caches[i] ? caches[i]->num_ids() : d.num_ids;
    c.counts = cstride == 1 ? d_counts + i * world : d_counts + i;   // [ctx][owner] | [owner][ctx]
    c.cstride = cstride;
    c.cursor = d_cursor ? d_cursor + i * world : nullptr;
    c.send_ids = d.d_send_ids;
    c.req_pos = d.d_req_pos;
    *max_rows = std::max(*max_rows, d.n);
  }
  return r;
}
inline unsigned pull_grid(size_t rows) {
  return static_cast<unsigned>(std::max<size_t>(1, std::min<size_t>((rows + 255) / 256, 2048)));
}
}  // namespace

void pull_count(const gf_pull_desc* descs, size_t n, int world, FeatureCache* const* caches,
                uint32_t* d_counts, int device, hipStream_t stream) {
  GF_REQUIRE(d_counts != nullptr, "pull_count: null counts");
  DeviceGuard dg(device);
  size_t rows;
  PullRound r = make_pull_round(descs, n, world, caches, d_counts, nullptr, &rows);
  GF_HIP(hipMemsetAsync(d_counts, 0, n * world * sizeof(uint32_t), stream));
  if (rows == 0) return;
  const dim3 grid(pull_grid(rows), static_cast<unsigned>(n));
  pull_claim_kernel<<<grid, dim3(256), 0, stream>>>(r);
  pull_bucket_kernel<false><<<grid, dim3(256), 0, stream>>>(r);
  GF_HIP(hipGetLastError());
}

void pull_scatter(const gf_pull_desc* descs, size_t n, int world, FeatureCache* const* caches,
                  uint32_t* d_counts, uint32_t* d_cursor, int device, hipStream_t stream) {
  GF_REQUIRE(d_counts && d_cursor, "pull_scatter: null counts / cursor");
  DeviceGuard dg(device);
  size_t rows;
  PullRound r = make_pull_round(descs, n, world, caches, d_counts, d_cursor, &rows);
  for (size_t i = 0; i < n; ++i)
    GF_REQUIRE(descs[i].n == 0 || (descs[i].d_send_ids && descs[i].d_req_pos),
               "pull_scatter: null send / position buffer");
  GF_HIP(hipMemsetAsync(d_cursor, 0, n * world * sizeof(uint32_t), stream));
  if (rows == 0) return;
  const dim3 grid(pull_grid(rows), static_cast<unsigned>(n));
  pull_bucket_kernel<true><<<grid, dim3(256), 0, stream>>>(r);
  GF_HIP(hipGetLastError());
}

// the owner's side: out[i,:] = rows[index[ids[i]],:]
void gather_rows_indexed(const float* d_rows, size_t num_local_rows, size_t dim,
                         const int32_t* d_index, size_t num_ids, const int64_t* d_ids, size_t n,
                         float* d_out, uint32_t* d_flag, int device, hipStream_t stream) {
  if (n == 0) return;
  GF_REQUIRE(d_rows && d_index && d_ids && d_out && d_flag, "gather_rows_indexed: null pointer");
  GF_REQUIRE(dim > 0 && num_local_rows > 0, "gather_rows_indexed: empty shard");
  DeviceGuard dg(device);
  Round r;
  r.count = 1;
  r.c[0] = plain_ctx(d_rows, num_ids, dim, d_ids, n, d_out);
  r.c[0].remap = d_index;
  r.c[0].flag = d_flag;
  launch_round(r, stream);
}

// All fetches of one fetch_feature() call over sharded tables, rounds as in fetch_blocks: the
// pulled rows stand in for the local table, a missed row finds its own through the claim the
// plan settled (Ctx::req_pos).
void fetch_blocks_pulled(FeatureCache* node, FeatureCache* edge, const gf_fetch_pulled_desc* descs,
                         size_t n, hipStream_t stream) {
  GF_REQUIRE(descs != nullptr || n == 0, "fetch_blocks_pulled: null descriptors");
  std::vector<const gf_fetch_pulled_desc*> nodes, edges;
  for (size_t i = 0; i < n; ++i) {
    const gf_fetch_pulled_desc& d = descs[i];
    GF_REQUIRE(d.kind == 0 || d.kind == 1, "fetch_blocks_pulled: kind must be 0 (node) or 1 (edge)");
    GF_REQUIRE((d.kind == 0 ? node : edge) == nullptr || (d.kind == 0 ? node : edge)->mirror_,
               "fetch_blocks_pulled: pulled rows need the row mirror");
    if (d.n == 0) continue;
    GF_REQUIRE(d.d_pulled_rows && d.d_req_pos, "fetch_blocks_pulled: null pulled rows");
    GF_REQUIRE((d.kind == 0 ? node : edge) != nullptr, "fetch_blocks_pulled: block without its cache");
    (d.kind == 0 ? nodes : edges).push_back(&d);
  }
  const int device = node ? node->device() : (edge ? edge->device() : 0);
  DeviceGuard dg(device);
  size_t max_node_rows = 0, max_edge_rows = 0;
  for (const auto* d : nodes) max_node_rows = std::max(max_node_rows, d->n);
  for (const auto* d : edges) max_edge_rows = std::max(max_edge_rows, d->n);
  if (node && max_node_rows) node->reserve_workspace(max_node_rows, stream);
  if (edge && max_edge_rows) edge->reserve_workspace(max_edge_rows, stream);
  const size_t rounds = std::max(nodes.size(), edges.size());
  for (size_t i = 0; i < rounds; ++i) {
    Round r;
    r.count = 0;
    auto add = [&](FeatureCache* fc, const gf_fetch_pulled_desc& d) {
      Ctx& c = r.c[r.count++];
      fc->prepare(d.d_ids, d.n, d.d_out, d.update != 0, d.d_stats, &c, stream);
      c.miss_rows = d.d_pulled_rows;
      c.req_pos = d.d_req_pos;
      c.inst_from_table = 0;   // the missed rows are the pulled ones, not a local table's
      if (c.vec4 && (reinterpret_cast<uintptr_t>(d.d_pulled_rows) & 15u)) {
        c.vec4 = 0;
        c.dimv = static_cast<uint32_t>(fc->dim_);
        set_odd4(c, fc->dim_, fc->policy_ == GF_CACHE_LRU || !d.update || fc->capacity_ == 0);
      }
    };
    if (i < nodes.size()) add(node, *nodes[i]);
    if (i < edges.size()) add(edge, *edges[i]);
    launch_round(r, stream);
  }
}

// out[i,:] = rows[pos[i],:] — the cache-free context of a pull round (every row travelled;
// req_pos is its place among the pulled rows)
namespace {
__global__ void rows_by_pos_kernel(const float* __restrict__ rows, const uint32_t* __restrict__ pos,
                                   uint32_t n, uint32_t dim, float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const uint32_t nwaves = (gridDim.x * blockDim.x) >> 6;
  for (uint32_t i = wave; i < n; i += nwaves) {
    const float* s = rows + static_cast<uint64_t>(pos[i]) * dim;
    float* o = out + static_cast<uint64_t>(i) * dim;
    for (uint32_t c = lane; c < dim; c += 64) o[c] = s[c];
  }
}
}  // namespace

// One fetch round over sharded tables as ONE native call: plan -> count exchange -> the round's
// host synchronisation -> scatter -> ids out -> serve -> rows back -> fetch (the stages
// Cache._pull_round issues one by one when the exchange has to go through torch.distributed).
PullSession::PullSession(Exchange* ex, int device) : ex_(ex), device_(device) {}

void PullSession::round(FeatureCache* node, FeatureCache* edge, const gf_pull_ctx* ctxs, size_t n,
                        int flag, int* any_flag, uint64_t* rows_pulled, uint64_t* bytes_sent,
                        uint32_t* d_error_flag, hipStream_t st) {
  GF_REQUIRE(ctxs != nullptr && n >= 1 && n <= static_cast<size_t>(kMaxCtx),
             "pull round: 1..4 contexts");
  GF_REQUIRE(d_error_flag != nullptr, "pull round: null error flag");
  DeviceGuard dg(device_);
  const int P = ex_ ? ex_->world() : 1, me = ex_ ? ex_->rank() : 0;
  const size_t W = n + 1;   // words per owner: the contexts' counts + this rank's flag
  // buffers
  gf_pull_desc descs[kMaxCtx];
  FeatureCache* caches[kMaxCtx] = {nullptr, nullptr, nullptr, nullptr};
  for (size_t k = 0; k < n; ++k) {
    const gf_pull_ctx& c = ctxs[k];
    GF_REQUIRE(c.kind >= 0 && c.kind <= 2, "pull round: bad kind");
    GF_REQUIRE(c.dim > 0 && c.d_shard_rows && c.d_shard_index, "pull round: bad shard");
    caches[k] = c.kind == 0 ? node : (c.kind == 1 ? edge : nullptr);
    GF_REQUIRE(c.kind == 2 || caches[k] != nullptr, "pull round: block without its cache");
    send_ids_[k].reserve(std::max<size_t>(c.pull.n, 1) * 8, 0, st);
    req_pos_[k].reserve(std::max<size_t>(c.pull.n, 1) * 4, 0, st);
    // sized BEFORE the round's first exchange from what is known now (at most pull.n rows leave;
    // about as many arrive when the ids spread evenly), doubling: in the steady state no
    // hipMalloc / hipFree — a device-wide synchronisation — sits between two collectives
    pulled_[k].reserve(std::max<size_t>(c.pull.n, 1) * c.dim * 4, 0, st);
    got_[k].reserve(std::max<size_t>(c.pull.n, 1) * 8, 0, st);
    served_[k].reserve(std::max<size_t>(c.pull.n, 1) * c.dim * 4, 0, st);
    descs[k] = c.pull;
    descs[k].cache = nullptr;   // caches[] carries it
    descs[k].d_send_ids = send_ids_[k].as<int64_t>();
    descs[k].d_req_pos = req_pos_[k].as<uint32_t>();
  }
  counts_.reserve((2 * P * W + n * P) * 4, 0, st);
  h_counts_.reserve(2 * P * W * 4);
  uint32_t* d_counts = counts_.as<uint32_t>();        // [P][W] own, then [P][W] received
  uint32_t* d_recv = d_counts + P * W;
  uint32_t* d_cursor = d_recv + P * W;
  // 1. claims + per-owner counts, owner-major so that row q goes to rank q as it is
  size_t rows;
  PullRound r = make_pull_round(descs, n, P, caches, d_counts, nullptr, &rows,
                                static_cast<uint32_t>(W));
  GF_HIP(hipMemsetAsync(d_counts, 0, P * W * 4, st));
  if (rows) {
    const dim3 grid(pull_grid(rows), static_cast<unsigned>(n));
    pull_claim_kernel<<<grid, dim3(256), 0, st>>>(r);
    pull_bucket_kernel<false><<<grid, dim3(256), 0, st>>>(r);
    GF_HIP(hipGetLastError());
  }
  if (flag)   // this rank's flag rides in word n of every owner's row (any non-zero value)
    GF_HIP(hipMemset2DAsync(d_counts + n, W * 4, 1, 4, P, st));
  if (ex_) ex_->all_to_all(d_counts, d_recv, W * 4, st);
  else GF_HIP(hipMemcpyAsync(d_recv, d_counts, P * W * 4, hipMemcpyDeviceToDevice, st));
  // 2. the round's one host synchronisation
  uint32_t* h = h_counts_.as<uint32_t>();
  GF_HIP(hipMemcpyAsync(h, d_counts, 2 * P * W * 4, hipMemcpyDeviceToHost, st));
  GF_HIP(hipStreamSynchronize(st));
  const uint32_t* hs = h;             // hs[q * W + k]: rows of context k this rank sends to q
  const uint32_t* hr = h + P * W;     // hr[q * W + k]: rows rank q asks this rank for
  int any = flag ? 1 : 0;
  for (int q = 0; q < P; ++q) any |= hr[q * W + n] ? 1 : 0;
  if (any_flag) *any_flag = any;
  // 3. ids into the compact owner-major send buffers
  r = make_pull_round(descs, n, P, caches, d_counts, d_cursor, &rows, static_cast<uint32_t>(W));
  GF_HIP(hipMemsetAsync(d_cursor, 0, n * P * 4, st));
  if (rows) {
    pull_bucket_kernel<true><<<dim3(pull_grid(rows), static_cast<unsigned>(n)), dim3(256), 0, st>>>(r);
    GF_HIP(hipGetLastError());
  }
  std::vector<size_t> sb(P), so(P), rb(P), ro(P);
  gf_fetch_pulled_desc fd[kMaxCtx];
  size_t nf = 0;
  // a skewed round (more rows asked of this rank than it asks for itself): grow for every
  // context now, before the first of the id / row exchanges
  for (size_t k = 0; k < n; ++k) {
    size_t n_recv = 0;
    for (int q = 0; q < P; ++q) n_recv += hr[q * W + k];
    got_[k].reserve(std::max<size_t>(n_recv, 1) * 8, 0, st);
    served_[k].reserve(std::max<size_t>(n_recv, 1) * ctxs[k].dim * 4, 0, st);
  }
  for (size_t k = 0; k < n; ++k) {
    const gf_pull_ctx& c = ctxs[k];
    size_t n_send = 0, n_recv = 0;
    for (int q = 0; q < P; ++q) { n_send += hs[q * W + k]; n_recv += hr[q * W + k]; }
    GF_REQUIRE(n_send <= std::max<size_t>(c.pull.n, 1), "pull round: more rows claimed than asked");
    auto exchange = [&](const void* send, void* recv, size_t row_bytes, bool back) {
      // forward: this rank's ids to their owners; back: the owners' rows to the requesters
      size_t a = 0, b = 0;
      for (int q = 0; q < P; ++q) {
        const size_t s_rows = back ? hr[q * W + k] : hs[q * W + k];
        const size_t r_rows = back ? hs[q * W + k] : hr[q * W + k];
        sb[q] = s_rows * row_bytes; so[q] = a; a += sb[q];
        rb[q] = r_rows * row_bytes; ro[q] = b; b += rb[q];
      }
      // every rank makes every call, whatever its own sizes are: a transport may synchronise
      // the ranks inside it
      if (ex_) ex_->all_to_all_v(send, sb.data(), so.data(), recv, rb.data(), ro.data(), st);
      else if (a) GF_HIP(hipMemcpyAsync(recv, send, a, hipMemcpyDeviceToDevice, st));
    };
    // 4. ids out, served by their owners, rows back
    exchange(send_ids_[k].data(), got_[k].data(), 8, false);
    if (n_recv)
      gather_rows_indexed(c.d_shard_rows, c.shard_rows, c.dim, c.d_shard_index, c.pull.num_ids,
                          got_[k].as<int64_t>(), n_recv, served_[k].as<float>(), d_error_flag,
                          device_, st);
    exchange(served_[k].data(), pulled_[k].data(), c.dim * 4, true);
    if (rows_pulled) rows_pulled[k] = n_send - hs[me * W + k];
    if (bytes_sent)
      bytes_sent[k] = 8 * (n_send - hs[me * W + k]) + 4 * c.dim * (n_recv - hr[me * W + k]);
    // 5. the fetch itself
    if (c.pull.n == 0) continue;
    GF_REQUIRE(c.d_out != nullptr, "pull round: null output");
    if (c.kind == 2) {
      const unsigned grid = static_cast<unsigned>(std::min<size_t>((c.pull.n + 3) / 4, 2048));
      rows_by_pos_kernel<<<dim3(grid), dim3(256), 0, st>>>(
          pulled_[k].as<float>(), req_pos_[k].as<uint32_t>(), static_cast<uint32_t>(c.pull.n),
          static_cast<uint32_t>(c.dim), c.d_out);
      GF_HIP(hipGetLastError());
      continue;
    }
    gf_fetch_pulled_desc& f = fd[nf++];
    f.kind = c.kind;
    f.update = c.update;
    f.d_ids = c.pull.d_ids;
    f.n = c.pull.n;
    f.d_out = c.d_out;
    f.d_stats = c.d_stats;
    f.d_pulled_rows = pulled_[k].as<float>();
    f.d_req_pos = req_pos_[k].as<uint32_t>();
  }
  if (nf) fetch_blocks_pulled(node, edge, fd, nf, st);
}

}  // namespace gf
