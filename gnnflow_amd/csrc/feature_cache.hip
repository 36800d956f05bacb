// Fused feature gather + LRU replacement on MI355X.
//
// Reference behaviour restated (gnnflow/cache/cache.py:255-400, lru_cache.py:121-201),
// per block of ids:
//   out[i,:] = cache_buffer[map[id_i]] if id_i is cached else feats[id_i]
//   hit ratio = #cached / n
//   if update and any miss: count -= 1 for every slot; hit slots -> 0; the
//   k = min(#unique missed ids, capacity) slots with the smallest count are
//   evicted and refilled with the missed ids' rows.
// The reference spends ~10 ATen launches, a host round trip for the missed rows
// (unique -> CPU index_select -> pinned -> H2D) and a topk over the whole capacity
// on every block.  Here a *round* of up to three independent blocks (one node-cache
// block, one edge-cache block, one cache-free gather) is the gather launch plus the update of
// the caches that missed — LRU, the policy on the hot path: one launch; LFU / FIFO: three —
// none of which waits for the host; each kernel takes the round's contexts by value and
// blockIdx.y selects the context, so the node and edge caches advance in the same launches.
// The parts, each a translation unit of its own around feature_cache_ctx.hpp:
//   gather.hip         the gather (the kernel that moves ~all the bytes)
//   cache_lru.hip      LRU: the eviction order as a list (two launches; cache_lru_fused.hip:
//                      one) or a queue (cache_lru_queue.hip), the host side of that list
//   cache_select.hip   LFU / FIFO: histogram select of the victims
//   cache_staging.hip  staging ring for host-resident tables
//   cache_pull.hip     sharded feature tables: plan, serve, fetch
// This file holds the host class and issues the rounds.
// All bookkeeping kernels return at once for a context whose block had no miss (the
// reference skips update_*_cache then too, cache.py:318); a hit only changes replacement
// state if the block also had a miss, exactly as in the reference.
#include "feature_cache_ctx.hpp"

#include <algorithm>
#include <cstring>
#include <vector>

namespace gf {

namespace {

__global__ void cache_fill_kernel(int32_t* map, uint64_t num_ids, int64_t* slot_id,
                                  uint32_t* stamp, uint32_t* touched, uint64_t capacity,
                                  int identity, uint32_t stamp0) {
  const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < num_ids;
       i += stride)
    map[i] = (identity && i < capacity) ? static_cast<int32_t>(i) : kAbsent;
  for (uint64_t s = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; s < capacity;
       s += stride) {
    slot_id[s] = identity ? static_cast<int64_t>(s) : -1;
    stamp[s] = stamp0;
    touched[s] = 0;
  }
}

// slot of every id (>= 0: cached there, -1: not cached, -2: out of range): what a caller
// that pulls missed rows from their owners needs to know before the fetch
__global__ void cache_probe_kernel(const int64_t* __restrict__ ids, uint64_t n,
                                   const int32_t* __restrict__ map, uint64_t num_ids,
                                   int32_t* __restrict__ slot) {
  const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n;
       i += stride) {
    const int64_t id = ids[i];
    int32_t v = -2;
    if (id >= 0 && static_cast<uint64_t>(id) < num_ids) {
      v = map ? map[id] : kAbsent;
      if (v < 0) v = -1;
    }
    slot[i] = v;
  }
}

inline bool pointer_on_device(const void* p) {
  hipPointerAttribute_t attr;
  std::memset(&attr, 0, sizeof(attr));
  if (hipPointerGetAttributes(&attr, p) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  return attr.type == hipMemoryTypeDevice;
}

}  // namespace

// Issues one round: the gather for every context, then (if any context updates its cache)
// the updates of the LRU contexts and of the LFU / FIFO contexts.
void launch_round(Round& r, hipStream_t stream) {
  if (r.count == 0) return;
  launch_gather(r, stream);
  bool any_update = false, only_fused = true;
  for (int i = 0; i < r.count; ++i) {
    any_update = any_update || r.c[i].update;
    only_fused = only_fused && (!r.c[i].update || (r.c[i].policy == GF_CACHE_LRU && r.c[i].fused));
  }
  if (!any_update) return;
  // the LRU slot of the profile: ONE fused launch carries its own dispatch events (the clock
  // rocprofv3 reads: begin / end of the dispatch); several launches sit between two stream events
  ProfileScope ps(only_fused ? -1 : kProfLru, stream);
  launch_lru_update(r, stream, only_fused);
  launch_select_update(r, stream);
}

FeatureCache::FeatureCache(size_t num_ids, size_t capacity, size_t dim, const float* d_feats,
                           int device)
    : num_ids_(num_ids), capacity_(capacity), dim_(dim), feats_(d_feats), device_(device) {
  GF_REQUIRE(dim > 0, "cache: dim must be positive");
  GF_REQUIRE(d_feats != nullptr, "cache: null feature table");
  GF_REQUIRE(capacity <= num_ids, "cache: capacity larger than the id space");
  GF_REQUIRE(capacity < 0x7FFFFFFFull, "cache: capacity must be < 2^31");
  DeviceGuard dg(device_);
  lru_fuse_spins_from_env(device_);
  table_on_device_ = pointer_on_device(d_feats);
  buffer_.reserve(std::max<size_t>(capacity * dim * sizeof(float), 16), 0, nullptr, true);
  map_.reserve(std::max<size_t>(num_ids * sizeof(int32_t), 16));
  slot_id_.reserve(std::max<size_t>(capacity * sizeof(int64_t), 16));
  stamp_.reserve(std::max<size_t>(capacity * sizeof(uint32_t), 16));
  touched_.reserve(std::max<size_t>(capacity * sizeof(uint32_t), 16));
  state_.reserve(kRing * sizeof(Counters), 0, nullptr, true);
  fifo_ptr_.reserve(16);
  qstate_.reserve(sizeof(QueueState));
  rewind_fifo(nullptr);
  cache_fill_kernel<<<dim3(1024), dim3(256), 0, nullptr>>>(
      map_.as<int32_t>(), num_ids_, slot_id_.as<int64_t>(), stamp_.as<uint32_t>(),
      touched_.as<uint32_t>(), capacity_, 0, 0u);
  GF_HIP(hipGetLastError());
  init_queue(nullptr);
  GF_HIP(hipMemsetAsync(buffer_.data(), 0, buffer_.bytes(), nullptr));
  GF_HIP(hipMemsetAsync(state_.data(), 0, state_.bytes(), nullptr));
  GF_HIP(hipStreamSynchronize(nullptr));
}

FeatureCache::~FeatureCache() {
  for (hipEvent_t e : stage_events_)
    if (e) (void)hipEventDestroy(e);
}

// diagnostics: stamps of the one-launch list update (gf_debug_lru_trace)
void FeatureCache::lru_trace_enable(bool on) {
  DeviceGuard dg(device_);
  GF_HIP(hipDeviceSynchronize());
  if (!on) { trace_.release(); return; }
  trace_.reserve((kGatherTraceBase + 8 * kGatherTraceWgs) * sizeof(unsigned long long));
  GF_HIP(hipMemset(trace_.data(), 0, trace_.bytes()));
}
size_t FeatureCache::lru_trace_read(uint64_t* out, size_t capacity_words) {
  if (!trace_.data()) return 0;
  DeviceGuard dg(device_);
  GF_HIP(hipDeviceSynchronize());
  const size_t words = std::min(capacity_words, trace_.bytes() / sizeof(unsigned long long));
  GF_HIP(hipMemcpy(out, trace_.data(), words * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  return words;
}

// Cache.init_cache (cache.py:175-195) / LRUCache.reset (lru_cache.py:91-105)
void FeatureCache::init(hipStream_t stream) {
  DeviceGuard dg(device_);
  cache_fill_kernel<<<dim3(1024), dim3(256), 0, stream>>>(
      map_.as<int32_t>(), num_ids_, slot_id_.as<int64_t>(), stamp_.as<uint32_t>(),
      touched_.as<uint32_t>(), capacity_, 1,
      policy_ == GF_CACHE_LFU ? 1u : 0u);   // LFUCache.init_cache: count += 1 (lfu_cache.py:80-84)
  GF_HIP(hipGetLastError());
  epoch_ = 0;
  rewind_fifo(stream);
  init_queue(stream);
  if (capacity_ && mirror_)
    GF_HIP(hipMemcpyAsync(buffer_.data(), feats_, capacity_ * dim_ * sizeof(float),
                          hipMemcpyDefault, stream));
}

// FIFOCache.reset (fifo_cache.py:70-75) rewinds the rotation pointer and keeps the cached
// ids: with install-epoch stamps that is "all slots equally old" -> refill from slot 0.
// LFUCache.reset (lfu_cache.py:86-118) re-initialises and then zeroes the use counts.
void FeatureCache::reset_order(hipStream_t stream) {
  DeviceGuard dg(device_);
  if (capacity_) {
    GF_HIP(hipMemsetAsync(stamp_.data(), 0, capacity_ * sizeof(uint32_t), stream));
    GF_HIP(hipMemsetAsync(touched_.data(), 0, capacity_ * sizeof(uint32_t), stream));
  }
  epoch_ = 0;
  rewind_fifo(stream);
}

// cache_*_pointer = capacity - 1 (fifo_cache.py:63-69): the next refill starts at slot 0
void FeatureCache::rewind_fifo(hipStream_t stream) {
  GF_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(fifo_ptr_.data()),
                           capacity_ ? static_cast<int>(capacity_ - 1) : 0, 1, stream));
}

void FeatureCache::set_policy(int policy) {
  GF_REQUIRE(policy == GF_CACHE_LRU || policy == GF_CACHE_LFU || policy == GF_CACHE_FIFO,
             "cache: unknown replacement policy");
  if (policy == policy_) return;
  policy_ = policy;
  // the per-slot words mean different things per policy (LRU: queue position / hit claim)
  DeviceGuard dg(device_);
  if (capacity_) {
    GF_HIP(hipMemsetAsync(stamp_.data(), 0, capacity_ * sizeof(uint32_t), nullptr));
    GF_HIP(hipMemsetAsync(touched_.data(), 0, capacity_ * sizeof(uint32_t), nullptr));
  }
  init_queue(nullptr);
  GF_HIP(hipStreamSynchronize(nullptr));
  if (policy_ != GF_CACHE_LRU) {   // only LRU keeps a queue
    queue_.release();
    queue_alt_.release();
    qpos_.release();
    wsnap_.release();
    qbits_.release();
    compact_.release();
    queue_form_ = false;
  }
}

namespace {
__global__ void cache_install_ids_kernel(const int64_t* __restrict__ ids, uint64_t n,
                                         uint64_t num_ids, uint32_t dim,
                                         const float* __restrict__ feats,
                                         const float* __restrict__ rows, int32_t* map,
                                         int64_t* slot_id, float* buffer) {
  const int lane = threadIdx.x & 63;
  const uint64_t wave = (static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x) >> 6;
  const uint64_t nwaves = (static_cast<uint64_t>(gridDim.x) * blockDim.x) >> 6;
  for (uint64_t s = wave; s < n; s += nwaves) {
    const int64_t id = ids[s];
    if (id < 0 || static_cast<uint64_t>(id) >= num_ids) continue;
    if (lane == 0) { map[id] = static_cast<int32_t>(s); slot_id[s] = id; }
    for (uint32_t c = lane; buffer && c < dim; c += 64)
      buffer[s * dim + c] = rows ? rows[s * dim + c] : feats[static_cast<uint64_t>(id) * dim + c];
  }
}
}  // namespace

// GNNLabStaticCache.init_cache (gnnlab_static_cache.py:87-168): slot i holds ids[i]
void FeatureCache::init_ids(const int64_t* d_ids, size_t n, hipStream_t stream,
                            const float* d_rows) {
  GF_REQUIRE(n <= capacity_, "cache: more ids than slots");
  GF_REQUIRE(d_ids != nullptr || n == 0, "cache: null id list");
  DeviceGuard dg(device_);
  cache_fill_kernel<<<dim3(1024), dim3(256), 0, stream>>>(
      map_.as<int32_t>(), num_ids_, slot_id_.as<int64_t>(), stamp_.as<uint32_t>(),
      touched_.as<uint32_t>(), capacity_, 0, 0u);
  epoch_ = 0;
  rewind_fifo(stream);
  init_queue(stream);
  if (n) {
    const unsigned grid = static_cast<unsigned>(std::min<size_t>((n + 3) / 4, 4096));
    cache_install_ids_kernel<<<dim3(grid), dim3(256), 0, stream>>>(
        d_ids, n, num_ids_, static_cast<uint32_t>(dim_), feats_, d_rows, map_.as<int32_t>(),
        slot_id_.as<int64_t>(), mirror_ ? buffer_.as<float>() : nullptr);
  }
  GF_HIP(hipGetLastError());
}

// Cache.resize (cache.py:197-221): grow the id space / capacity, keep the contents
void FeatureCache::resize(size_t new_num_ids, size_t new_capacity, const float* d_feats,
                          hipStream_t stream) {
  GF_REQUIRE(new_num_ids >= num_ids_ && new_capacity >= capacity_,
             "cache: resize can only grow");
  GF_REQUIRE(new_capacity <= new_num_ids && new_capacity < 0x7FFFFFFFull,
             "cache: invalid capacity");
  DeviceGuard dg(device_);
  if (d_feats) {
    feats_ = d_feats;
    table_on_device_ = pointer_on_device(d_feats);
    GF_REQUIRE(mirror_ || table_on_device_,
               "cache: a table in host memory needs the row mirror (gf_cache_set_row_mirror)");
  }
  if (policy_ == GF_CACHE_LRU && new_capacity > capacity_) compact_queue(stream);   // dense list
  if (new_num_ids > num_ids_) {
    DeviceBuffer nmap;
    nmap.reserve(new_num_ids * sizeof(int32_t));
    std::vector<int32_t> tail(new_num_ids - num_ids_, kAbsent);  // new ids start uncached
    GF_HIP(hipMemcpyAsync(nmap.data(), map_.data(), num_ids_ * sizeof(int32_t),
                          hipMemcpyDeviceToDevice, stream));
    GF_HIP(hipMemcpyAsync(nmap.as<int32_t>() + num_ids_, tail.data(),
                          tail.size() * sizeof(int32_t), hipMemcpyHostToDevice, stream));
    GF_HIP(hipStreamSynchronize(stream));
    std::swap(map_, nmap);
  }
  if (new_capacity > capacity_) {
    if (mirror_)
      buffer_.reserve(new_capacity * dim_ * sizeof(float), capacity_ * dim_ * sizeof(float),
                      stream, true);
    DeviceBuffer nid, nst, ntc;
    nid.reserve(new_capacity * sizeof(int64_t));
    nst.reserve(new_capacity * sizeof(uint32_t));
    ntc.reserve(new_capacity * sizeof(uint32_t));
    std::vector<int64_t> empty_ids(new_capacity - capacity_, -1);
    GF_HIP(hipMemcpyAsync(nid.data(), slot_id_.data(), capacity_ * sizeof(int64_t),
                          hipMemcpyDeviceToDevice, stream));
    GF_HIP(hipMemcpyAsync(nid.as<int64_t>() + capacity_, empty_ids.data(),
                          empty_ids.size() * sizeof(int64_t), hipMemcpyHostToDevice, stream));
    GF_HIP(hipMemsetAsync(nst.data(), 0, new_capacity * sizeof(uint32_t), stream));
    GF_HIP(hipMemcpyAsync(nst.data(), stamp_.data(), capacity_ * sizeof(uint32_t),
                          hipMemcpyDeviceToDevice, stream));
    GF_HIP(hipMemsetAsync(ntc.data(), 0, new_capacity * sizeof(uint32_t), stream));
    GF_HIP(hipMemcpyAsync(ntc.data(), touched_.data(), capacity_ * sizeof(uint32_t),
                          hipMemcpyDeviceToDevice, stream));
    GF_HIP(hipStreamSynchronize(stream));
    std::swap(slot_id_, nid);
    std::swap(stamp_, nst);
    std::swap(touched_, ntc);
  }
  const size_t old_capacity = capacity_;
  num_ids_ = new_num_ids;
  capacity_ = new_capacity;
  ws_rows_ = 0;   // tile arrays depend on the capacity
  if (staging()) {   // new table, more ids: the ring starts over
    const size_t gens = stage_gens_, rows = stage_cap_;
    if (table_on_device_) set_staging(0, 0);
    else set_staging(gens, rows);
  }
  if (policy_ == GF_CACHE_LRU && new_capacity > old_capacity) grow_queue(old_capacity, stream);
}

void FeatureCache::reserve_workspace(size_t n, hipStream_t stream) {
  retired_.collect();
  if (n <= ws_rows_ && ws_.data()) return;
  ws_rows_ = std::max(ws_rows_, n);
  const size_t tiles = (capacity_ + kTile - 1) / kTile + 1;
  size_t bytes = (kBins1 + kBins2) * sizeof(uint32_t) + 4 * align_up(ws_rows_ * 4, 16) +
                 align_up(ws_rows_ * 8, 16) + 2 * align_up(tiles * 4, 16) +
                 align_up((kMaxRowTiles + 1) * 4, 16) + 64;
  if (policy_ == GF_CACHE_LRU)   // staged victims per list tile / queue chunk, chunk counts
    bytes += 2 * align_up(stage_entries(ws_rows_, capacity_) * 4, 256) +
             align_up((victim_chunks(ws_rows_) + 2) * 4, 256) + 256 +
             2 * align_up(fuse_stage_entries(ws_rows_, capacity_) * 8, 256);
  // Kernels already queued on `stream` may still use the old scratch: it is retired behind
  // an event on that stream and freed once the event has completed — a stream-ordered swap,
  // no device-wide stall when a larger block arrives mid-run.
  DeviceBuffer fresh;
  fresh.reserve(bytes, 0, stream);
  std::swap(ws_, fresh);
  retired_.retire(std::move(fresh), stream);
}

// Fills the device context of one block fetch and advances this cache's host-side state
// (epoch, counter ring).  The caller launches the round.
void FeatureCache::prepare(const int64_t* d_ids, size_t n, float* d_out, bool update,
                           uint32_t* d_stats, Ctx* ctx_out, hipStream_t stream) {
  GF_REQUIRE(d_ids && d_out, "cache fetch: null pointer");
  reserve_workspace(n, stream);
  const size_t tiles = (capacity_ + kTile - 1) / kTile;
  Ctx& c = *ctx_out;
  std::memset(&c, 0, sizeof(c));
  char* p = ws_.as<char>();
  c.hist1 = reinterpret_cast<uint32_t*>(p);         p += kBins1 * sizeof(uint32_t);
  c.hist2 = reinterpret_cast<uint32_t*>(p);         p += kBins2 * sizeof(uint32_t);
  c.slot_of_row = reinterpret_cast<int32_t*>(p);    p += align_up(ws_rows_ * 4, 16);
  c.rep_flag = reinterpret_cast<uint32_t*>(p);      p += align_up(ws_rows_ * 4, 16);
  c.rep_rank = reinterpret_cast<uint32_t*>(p);      p += align_up(ws_rows_ * 4, 16);
  c.rep_row = reinterpret_cast<uint32_t*>(p);       p += align_up(ws_rows_ * 4, 16);
  c.rep_id = reinterpret_cast<int64_t*>(p);         p += align_up(ws_rows_ * 8, 16);
  c.tile_tie = reinterpret_cast<uint32_t*>(p);      p += align_up((tiles + 1) * 4, 16);
  c.tile_old = reinterpret_cast<uint32_t*>(p);      p += align_up((tiles + 1) * 4, 16);
  c.row_tile_sum = reinterpret_cast<uint32_t*>(p);  p += align_up((kMaxRowTiles + 1) * 4, 16);
  char* qscratch = reinterpret_cast<char*>(align_up(reinterpret_cast<uintptr_t>(p), 256));
  c.ids = d_ids;
  c.n = static_cast<uint32_t>(n);
  c.vec4 = vec4_ok(dim_, mirror_ ? buffer_.data() : feats_, feats_, d_out) ? 1 : 0;
  c.dimv = static_cast<uint32_t>(c.vec4 ? dim_ / 4 : dim_);
  c.inst_from_table = table_on_device_ ? 1 : 0;
  set_odd4(c, dim_, policy_ == GF_CACHE_LRU || !update || capacity_ == 0);
  c.tile_rows = pick_tile_rows(n);
  c.out = d_out;
  c.feats = feats_;
  c.num_ids = num_ids_;
  c.map = capacity_ ? map_.as<int32_t>() : nullptr;
  c.cache_buf = mirror_ ? buffer_.as<float>() : nullptr;
  c.slot_id = slot_id_.as<int64_t>();
  c.stamp = stamp_.as<uint32_t>();
  c.touched = touched_.as<uint32_t>();
  c.capacity = static_cast<uint32_t>(capacity_);
  c.update = (update && capacity_ > 0) ? 1 : 0;
  c.policy = policy_;
  c.fifo_ptr = fifo_ptr_.as<uint32_t>();
  c.epoch_new = c.update ? ++epoch_ : epoch_;
  c.ctr = state_.as<Counters>() + (ring_pos_ % kRing);
  c.ctr_next = state_.as<Counters>() + ((ring_pos_ + 1) % kRing);
  ring_pos_++;
  c.stats = d_stats;
  if (c.update && policy_ == GF_CACHE_LRU) fill_lru_ctx(c, n, qscratch, stream);
}

// One block of Cache.fetch_feature (cache.py:269-323 / :326-400)
void FeatureCache::fetch(const int64_t* d_ids, size_t n, float* d_out, bool update,
                         uint32_t* d_stats, hipStream_t stream) {
  if (n == 0) return;
  DeviceGuard dg(device_);
  Round r;
  r.count = 1;
  hipEvent_t seen[2];
  int num_seen = 0;
  stage_sync(stream, seen, &num_seen);
  prepare(d_ids, n, d_out, update, d_stats, &r.c[0], stream);
  stage_fill(&r.c[0]);
  launch_round(r, stream);
  stage_round_done();
}

// Cache(distributed=True): the slots of a block's ids, so that the caller can pull the
// missed rows from their owners ...
void FeatureCache::probe(const int64_t* d_ids, size_t n, int32_t* d_slot, hipStream_t stream) {
  if (n == 0) return;
  GF_REQUIRE(d_ids && d_slot, "cache probe: null pointer");
  DeviceGuard dg(device_);
  const unsigned grid = static_cast<unsigned>(std::min<size_t>((n + 255) / 256, 4096));
  cache_probe_kernel<<<dim3(grid), dim3(256), 0, stream>>>(
      d_ids, n, capacity_ ? map_.as<int32_t>() : nullptr, num_ids_, d_slot);
  GF_HIP(hipGetLastError());
}

// ... and the block's fetch with those rows standing in for the local feature table
void FeatureCache::fetch_pulled(const int64_t* d_ids, size_t n, float* d_out, bool update,
                                uint32_t* d_stats, const float* d_miss_rows,
                                const uint32_t* d_miss_index, hipStream_t stream) {
  if (n == 0) return;
  GF_REQUIRE(d_miss_rows && d_miss_index, "cache fetch: null pulled rows");
  GF_REQUIRE(mirror_, "cache fetch: pulled rows need the row mirror (gf_cache_set_row_mirror)");
  DeviceGuard dg(device_);
  Round r;
  r.count = 1;
  prepare(d_ids, n, d_out, update, d_stats, &r.c[0], stream);
  r.c[0].miss_rows = d_miss_rows;
  r.c[0].miss_index = d_miss_index;
  r.c[0].inst_from_table = 0;   // the missed rows are the pulled ones, not the local table's
  if (r.c[0].vec4 && (reinterpret_cast<uintptr_t>(d_miss_rows) & 15u)) {
    r.c[0].vec4 = 0;
    r.c[0].dimv = static_cast<uint32_t>(dim_);
    set_odd4(r.c[0], dim_, policy_ == GF_CACHE_LRU || !update || capacity_ == 0);
  }
  launch_round(r, stream);
}

void FeatureCache::gather_plain(const int64_t* d_ids, size_t n, float* d_out,
                                hipStream_t stream) {
  gather_rows(feats_, num_ids_, dim_, d_ids, n, d_out, device_, stream);
}

// All feature fetches of one fetch_feature() call (cache.py:255-413).  The node cache and
// the edge cache are independent, so round i carries the i-th node block AND the i-th edge
// block (the edge blocks must stay ordered: each sees the LRU state the previous one left);
// cache-free gathers ride in the first round.  Every round is the same few launches whatever
// the number of contexts in it.
void fetch_blocks(FeatureCache* node, FeatureCache* edge, const gf_fetch_desc* descs, size_t n,
                  hipStream_t stream) {
  GF_REQUIRE(descs != nullptr || n == 0, "fetch_blocks: null descriptors");
  std::vector<const gf_fetch_desc*> nodes, edges, plain;
  for (size_t i = 0; i < n; ++i) {
    const gf_fetch_desc& d = descs[i];
    GF_REQUIRE(d.kind >= 0 && d.kind <= 2, "fetch_blocks: bad kind");
    if (d.n == 0) continue;
    if (d.kind == 0) {
      GF_REQUIRE(node != nullptr, "fetch_blocks: node block without a node cache");
      nodes.push_back(&d);
    } else {
      GF_REQUIRE(edge != nullptr, "fetch_blocks: edge block without an edge cache");
      (d.kind == 1 ? edges : plain).push_back(&d);
    }
  }
  const int device = node ? node->device() : (edge ? edge->device() : 0);
  DeviceGuard dg(device);
  // size each cache's scratch for its largest block up front: no reallocation (and device
  // synchronisation) between the rounds of one fetch
  size_t max_node_rows = 0, max_edge_rows = 0;
  for (const gf_fetch_desc* d : nodes) max_node_rows = std::max(max_node_rows, d->n);
  for (const gf_fetch_desc* d : edges) max_edge_rows = std::max(max_edge_rows, d->n);
  if (node && max_node_rows) node->reserve_workspace(max_node_rows, stream);
  if (edge && max_edge_rows) edge->reserve_workspace(max_edge_rows, stream);
  {   // host-resident tables: rows pulled ahead of this fetch must have landed
    hipEvent_t seen[2];
    int num_seen = 0;
    if (node) node->stage_sync(stream, seen, &num_seen);
    if (edge) edge->stage_sync(stream, seen, &num_seen);
  }
  auto done = [&] {
    if (node) node->stage_round_done();
    if (edge) edge->stage_round_done();
  };
  size_t pi = 0;
  const size_t rounds = std::max(nodes.size(), edges.size());
  for (size_t i = 0; i < rounds; ++i) {
    Round r;
    r.count = 0;
    if (i < nodes.size()) {
      const gf_fetch_desc& d = *nodes[i];
      node->prepare(d.d_ids, d.n, d.d_out, d.update != 0, d.d_stats, &r.c[r.count], stream);
      node->stage_fill(&r.c[r.count++]);
    }
    if (i < edges.size()) {
      const gf_fetch_desc& d = *edges[i];
      edge->prepare(d.d_ids, d.n, d.d_out, d.update != 0, d.d_stats, &r.c[r.count], stream);
      edge->stage_fill(&r.c[r.count++]);
    }
    while (pi < plain.size() && r.count < kMaxCtx) {
      const gf_fetch_desc& d = *plain[pi++];
      r.c[r.count] = plain_ctx(edge->feats_, edge->num_ids_, edge->dim_, d.d_ids, d.n, d.d_out);
      edge->stage_fill(&r.c[r.count++]);
    }
    launch_round(r, stream);
    done();
  }
  while (pi < plain.size()) {   // cache-free gathers that did not fit into a round
    Round r;
    r.count = 0;
    while (pi < plain.size() && r.count < kMaxCtx) {
      const gf_fetch_desc& d = *plain[pi++];
      r.c[r.count] = plain_ctx(edge->feats_, edge->num_ids_, edge->dim_, d.d_ids, d.n, d.d_out);
      edge->stage_fill(&r.c[r.count++]);
    }
    launch_round(r, stream);
    done();
  }
}

void FeatureCache::slot_ids(int64_t* out, size_t capacity) const {
  GF_REQUIRE(out != nullptr && capacity >= capacity_, "slot_ids: output too small");
  if (!capacity_) return;
  DeviceGuard dg(device_);
  GF_HIP(hipDeviceSynchronize());
  GF_HIP(hipMemcpy(out, slot_id_.data(), capacity_ * sizeof(int64_t), hipMemcpyDeviceToHost));
}

void FeatureCache::lru_state(uint64_t out[7]) const {
  for (int i = 0; i < 7; ++i) out[i] = 0;
  if (policy_ != GF_CACHE_LRU || !capacity_) return;
  DeviceGuard dg(device_);
  GF_HIP(hipDeviceSynchronize());
  QueueState qs;
  GF_HIP(hipMemcpy(&qs, qstate_.data(), sizeof(qs), hipMemcpyDeviceToHost));
  out[0] = queue_form_ ? 1 : 0;
  out[1] = queue_cap_;
  out[2] = qs.head;
  out[3] = qs.tail;
  out[4] = compactions_;
  out[5] = list_form_updates_;
  out[6] = qs.lone_walks;
}

size_t FeatureCache::mem_bytes() const {
  return (mirror_ ? capacity_ * dim_ * sizeof(float) : 0) + num_ids_ * sizeof(int32_t) +
         capacity_ * (sizeof(int64_t) + 2 * sizeof(uint32_t));
}

// The cached rows' copy in HBM (`buffer`).  With the feature table itself in HBM a hit and a miss
// are the same bytes at the same distance: without the mirror the slots hold ids only, every
// row is read from the table, an install moves nothing — the replacement state (what the
// reference's protocol lets a caller observe: hit ratios, which ids are cached) is unchanged.
void FeatureCache::set_row_mirror(bool on) {
  DeviceGuard dg(device_);
  GF_HIP(hipDeviceSynchronize());
  GF_REQUIRE(on || table_on_device_, "cache: only a table in device memory can do without the row mirror");
  if (on == mirror_) return;
  mirror_ = on;
  if (!on) { buffer_.release(); return; }
  buffer_.reserve(std::max<size_t>(capacity_ * dim_ * sizeof(float), 16), 0, nullptr, true);
  // the rows of the ids cached right now
  if (capacity_) {
    std::vector<int64_t> ids(capacity_);
    GF_HIP(hipMemcpy(ids.data(), slot_id_.data(), capacity_ * sizeof(int64_t), hipMemcpyDeviceToHost));
    for (size_t s2 = 0; s2 < capacity_; ++s2)
      if (ids[s2] >= 0)
        GF_HIP(hipMemcpy(buffer_.as<float>() + s2 * dim_, feats_ + static_cast<size_t>(ids[s2]) * dim_,
                         dim_ * sizeof(float), hipMemcpyDefault));
  }
}

}  // namespace gf
