// EdgeStore implementation, all but add_edges (edge_store_ingest.hip): lifetime, pools and
// fences, the node table, offload, accessors.  See edge_store.hpp for the layout; reference
// lines are cited on each function that restates reference behaviour.
#include "edge_store_internal.hpp"
#include "ingest_sort.hpp"

#include <sys/mman.h>

#include <chrono>
#include <cstdio>
#include <fstream>

namespace gf {

namespace {
// ---- kernels -------------------------------------------------------------------
// fence_l[g] = ts_pool[(g + 1) * 16^l - 1] for every block that ends below `live` (after the
// pools were reallocated: the fence buffer is new)
__global__ void rebuild_fences_kernel(const float* __restrict__ ts_pool, uint64_t live,
                                      FenceView fence) {
  const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
  const uint64_t first = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  for (uint32_t l = 0; l < fence.levels; ++l) {
    const uint32_t shift = 4 * (l + 1);
    const uint64_t blocks = live >> shift;
    for (uint64_t g = first; g < blocks; g += stride)
      fence.base[fence.off[l] + g] = ts_pool[((g + 1) << shift) - 1];
  }
}

__global__ void update_nodes_kernel(const int64_t* __restrict__ ids,
                                    const NodeEntry* __restrict__ entries, size_t n,
                                    NodeEntry* __restrict__ table) {
  size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i < n) table[ids[i]] = entries[i];
}

struct RangeDesc { uint64_t start, count, out; };

__global__ void gather_ranges_kernel(const RangeDesc* __restrict__ ranges, size_t nranges,
                                     const float* __restrict__ ts_pool,
                                     const EdgePair* __restrict__ nbr_pool,
                                     int64_t* __restrict__ o_dst, int64_t* __restrict__ o_eid,
                                     float* __restrict__ o_ts) {
  for (size_t r = blockIdx.x; r < nranges; r += gridDim.x) {
    RangeDesc rd = ranges[r];
    for (uint64_t i = threadIdx.x; i < rd.count; i += blockDim.x) {
      EdgePair p = nbr_pool[rd.start + i];
      o_dst[rd.out + i] = p.dst;
      o_eid[rd.out + i] = p.eid;
      o_ts[rd.out + i] = ts_pool[rd.start + i];
    }
  }
}

}  // namespace

// ---- lifetime -------------------------------------------------------------------
EdgeStore::EdgeStore(size_t initial_pool_size, size_t maximum_pool_size,
                     int mem_resource_type, size_t minimum_block_size,
                     size_t /*blocks_to_preallocate*/, int insertion_policy, int device,
                     bool adaptive_block_size)
    : initial_pool_size_(initial_pool_size),
      maximum_pool_size_(maximum_pool_size),
      minimum_block_size_(minimum_block_size),
      mem_resource_type_(mem_resource_type),
      insertion_policy_(insertion_policy),
      device_(device),
      adaptive_(adaptive_block_size),
      free_lists_(64) {
  GF_REQUIRE(mem_resource_type >= GF_MEM_CUDA && mem_resource_type <= GF_MEM_SHARED,
             "invalid memory resource type");
  GF_REQUIRE(insertion_policy == GF_INSERTION_POLICY_INSERT ||
                 insertion_policy == GF_INSERTION_POLICY_REPLACE,
             "invalid insertion policy");
  GF_REQUIRE(maximum_pool_size >= initial_pool_size,
             "maximum_pool_size must be >= initial_pool_size");
  int count = 0;
  GF_HIP(hipGetDeviceCount(&count));
  GF_REQUIRE(device >= 0 && device < count, "invalid device id");
  DeviceGuard dg(device_);
  GF_HIP(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking));
}

EdgeStore::~EdgeStore() {
  if (stream_) {
    (void)hipStreamSynchronize(stream_);
    (void)hipStreamDestroy(stream_);
  }
}

GraphView EdgeStore::view() const {
  GraphView v;
  v.table = table_.as<NodeEntry>();
  v.table_len = any_node_ ? max_node_id_ + 1 : 0;
  v.ts_pool = ts_pool_.as<float>();
  v.nbr_pool = nbr_pool_.as<EdgePair>();
  v.fence = fence_view_;
  v.nonneg_ts = negative_ts_.load(std::memory_order_relaxed) ? 0 : 1;
  return v;
}

// (Re)allocates the fence levels for a pool of `cap` elements and fills them from the first
// `live` elements of ts_pool_.  Called when the pools grow: rare, and one strided pass.
void EdgeStore::rebuild_fences(uint64_t cap, uint64_t live) {
  FenceView f{nullptr, {0}, 0};
  uint64_t total = 0;
  for (uint32_t l = 0; l < kFenceMaxLevels; ++l) {
    const uint64_t n = cap >> (4 * (l + 1));
    if (n == 0) break;
    f.off[l] = total;
    total += align_up(n, 64);   // every level starts on a 256-byte boundary
    f.levels = l + 1;
  }
  if (f.levels == 0) { fence_view_ = f; return; }
  total += 64;   // a whole aligned window of 16 fences is readable behind the last level
  // ingest kernels queued earlier hold the old view: they are on stream_, and so is this.
  // A sample() enqueued on ANOTHER stream before this add_edges may still be running with the
  // old view (callers order add_edges against sample(), SURVEY 8(b) "Threading" — the
  // reference: wait_for_all_updates_to_finish — but a sample that was merely ENQUEUED earlier
  // is legitimate): the previous generation of the fences therefore stays allocated until the
  // next growth instead of being freed here.
  DeviceBuffer fresh;
  fresh.reserve(total * sizeof(float), 0, stream_);
  GF_HIP(hipStreamSynchronize(stream_));
  std::swap(fence_, fresh);
  std::swap(fence_prev_, fresh);   // `fresh` now holds the generation before the previous one
  f.base = fence_.as<float>();
  fence_view_ = f;
  if (live >= 16) {
    const unsigned grid = static_cast<unsigned>(std::min<uint64_t>(((live >> 4) + 255) / 256, 4096));
    rebuild_fences_kernel<<<dim3(std::max(grid, 1u)), dim3(256), 0, stream_>>>(
        ts_pool_.as<float>(), live, f);
    GF_HIP(hipGetLastError());
  }
}

// ---- bookkeeping ----------------------------------------------------------------
// dynamic_graph.cu:140-147 AddNodes
namespace {
constexpr size_t kHugePage = size_t(2) << 20;
inline size_t huge_rounded(size_t bytes) { return (bytes + kHugePage - 1) / kHugePage * kHugePage; }
}  // namespace

void* huge_zeroed_alloc(size_t bytes) {
  const size_t rounded = huge_rounded(bytes);
  char* raw = static_cast<char*>(mmap(nullptr, rounded + kHugePage, PROT_READ | PROT_WRITE,
                                      MAP_PRIVATE | MAP_ANONYMOUS, -1, 0));
  if (raw == MAP_FAILED) throw std::bad_alloc();
  char* p = reinterpret_cast<char*>((reinterpret_cast<uintptr_t>(raw) + kHugePage - 1) /
                                    kHugePage * kHugePage);
  if (p > raw) (void)munmap(raw, static_cast<size_t>(p - raw));
  const size_t tail = static_cast<size_t>(raw + rounded + kHugePage - (p + rounded));
  if (tail) (void)munmap(p + rounded, tail);
  (void)madvise(p, rounded, MADV_HUGEPAGE);
  return p;
}

void huge_free(void* p, size_t bytes) {
  if (p) (void)munmap(p, huge_rounded(bytes));
}

void NodeTable::resize(size_t n) {
  if (n <= size_) return;
  const size_t have = chunks_.size(), want = (n + kChunk - 1) >> kShift;
  chunks_.resize(want, nullptr);
  parallel_for(want - have, 1, [&](size_t c0, size_t c1) {
    for (size_t c = c0; c < c1; ++c) {
      NodeState* chunk = static_cast<NodeState*>(huge_zeroed_alloc(kChunk * sizeof(NodeState)));
      for (size_t i = 0; i < kChunk; ++i) new (chunk + i) NodeState();
      chunks_[have + c] = chunk;
    }
  });
  size_ = n;
}

NodeTable::~NodeTable() {
  for (NodeState* chunk : chunks_) {
    if (!chunk) continue;
    for (size_t i = 0; i < kChunk; ++i) chunk[i].~NodeState();
    huge_free(chunk, kChunk * sizeof(NodeState));
  }
}

void EdgeStore::add_nodes(int64_t max_node) {
  size_t need = static_cast<size_t>(max_node) + 1;
  if (any_node_ && need <= nodes_.size()) return;
  nodes_.resize(need);
  if (need > seen_.capacity()) seen_.reserve(need + need / 4);
  seen_.resize(need, 0);
  if (need > table_cap_) {
    size_t cap = table_cap_ ? table_cap_ : 1024;
    while (cap < need) cap *= 2;
    table_.reserve(cap * sizeof(NodeEntry), table_cap_ * sizeof(NodeEntry), stream_,
                   /*zero_new=*/true);
    table_cap_ = table_.bytes() / sizeof(NodeEntry);
  }
  max_node_id_ = static_cast<size_t>(max_node);
  any_node_ = true;
}

// `if (--edges_[eid] == 0) edges_.erase(eid)` (dynamic_graph.cu:393-397)
void EdgeStore::drop_eid(int64_t eid) {
  if (eid >= 0 && static_cast<uint64_t>(eid) < eid_dense_.size()) {
    uint32_t& c = eid_dense_[eid];
    if (c > 0 && --c == 0) num_live_eids_--;
    return;
  }
  auto it = eid_sparse_.find(eid);
  if (it != eid_sparse_.end() && --it->second == 0) {
    eid_sparse_.erase(it);
    num_live_eids_--;
  }
}

void EdgeStore::seg_free(uint64_t start, uint64_t cap) {
  free_lists_[log2_exact(cap)].push_back(start);
}

void EdgeStore::ensure_pool(uint64_t elems) {
  if (elems <= pool_elems_) return;
  uint64_t cap = pool_elems_ ? pool_elems_ : std::max<uint64_t>(initial_pool_size_ / kBlockSpace, 1024);
  if (nbr_pool_.in_place() && ts_pool_.in_place()) {
    // growing in place costs nothing but the mapping: a quarter of headroom instead of doubling
    // (at 1.3 G edges doubling left 160 GB of HBM in use for 47 GB of edges)
    cap = std::max(cap, elems + elems / 4);
  } else {
    while (cap < elems) cap *= 2;
  }
  // the whole used prefix [0, old bump) is preserved across the reallocation
  uint64_t keep = std::min<uint64_t>(pool_elems_, bump_);
  if (!pools_ready_) {
    // address ranges for the most the pools may ever hold: power-of-two segments can take up
    // to ~4x the live edges; capped at 64 G elements
    const uint64_t max_elems = std::min<uint64_t>(
        std::max<uint64_t>(16 * (maximum_pool_size_ / kBlockSpace + 1), cap), uint64_t(1) << 36);
    ts_pool_.init(max_elems * sizeof(float), device_);
    nbr_pool_.init(max_elems * sizeof(EdgePair), device_);
    pools_ready_ = true;
  }
  const auto t0 = std::chrono::steady_clock::now();
  ts_pool_.reserve(cap * sizeof(float), keep * sizeof(float), stream_);
  const auto t1 = std::chrono::steady_clock::now();
  nbr_pool_.reserve(cap * sizeof(EdgePair), keep * sizeof(EdgePair), stream_);
  const auto t2 = std::chrono::steady_clock::now();
  if (std::getenv("GNNFLOW_INGEST_PROFILE"))
    std::fprintf(stderr, "ensure_pool: %llu -> %llu elems (keep %llu): ts %.1f ms, nbr %.1f ms\n",
                 (unsigned long long)pool_elems_, (unsigned long long)cap, (unsigned long long)keep,
                 std::chrono::duration<double, std::milli>(t1 - t0).count(),
                 std::chrono::duration<double, std::milli>(t2 - t1).count());
  pool_elems_ = cap;
  rebuild_fences(cap, keep);
}

void EdgeStore::upload_entries(const std::vector<int64_t>& ids) {
  if (ids.empty()) return;
  const size_t k = ids.size();
  pinned_.reserve(k * (sizeof(int64_t) + sizeof(NodeEntry)));
  int64_t* h_ids = pinned_.as<int64_t>();
  NodeEntry* h_ent = reinterpret_cast<NodeEntry*>(h_ids + k);
  parallel_for(k, 1 << 15, [&](size_t i0, size_t i1) {
    for (size_t i = i0; i < i1; ++i) {
      if (i + 16 < i1) __builtin_prefetch(&nodes_[ids[i + 16]], 0, 1);
      h_ids[i] = ids[i];
      h_ent[i] = node_entry(nodes_[ids[i]]);
    }
  });
  publish_entries(pinned_, k);
}

// entries prepared by the caller in pinned memory: int64 ids[k] followed by NodeEntry[k]
void EdgeStore::publish_entries(const PinnedBuffer& prepared, size_t k) {
  if (k == 0) return;
  const size_t bytes = k * (sizeof(int64_t) + sizeof(NodeEntry));
  staging_.reserve(bytes, 0, stream_);
  GF_HIP(hipMemcpyAsync(staging_.data(), prepared.data(), bytes, hipMemcpyHostToDevice, stream_));
  int64_t* d_ids = staging_.as<int64_t>();
  NodeEntry* d_ent = reinterpret_cast<NodeEntry*>(d_ids + k);
  update_nodes_kernel<<<dim3((k + 255) / 256), dim3(256), 0, stream_>>>(
      d_ids, d_ent, k, table_.as<NodeEntry>());
  GF_HIP(hipGetLastError());
  GF_HIP(hipStreamSynchronize(stream_));
}

// ---- DynamicGraph::OffloadOldBlocks, dynamic_graph.cu:382-411 --------------------
size_t EdgeStore::offload_old_blocks(float timestamp, bool to_file) {
  DeviceGuard dg(device_);
  struct Dropped { int64_t node; uint64_t out; std::vector<LogicalBlock> blocks; };
  std::vector<RangeDesc> ranges;
  std::vector<Dropped> dropped;
  std::vector<int64_t> touched;
  uint64_t total = 0;
  size_t num_blocks = 0;
  for (size_t v = 0; v < nodes_.size(); ++v) {
    if (!(seen_[v] & 1)) continue;
    NodeState& st = nodes_[v];
    // blocks are chronological, so the blocks with end_ts < t form a prefix
    uint64_t k = 0;
    Dropped d{static_cast<int64_t>(v), total, {}};
    while (st.num_blocks() > 0 && st.blocks[st.first_block].end_ts < timestamp) {
      const LogicalBlock& b = st.blocks[st.first_block];
      k += b.size;
      logical_bytes_ -= b.capacity * kBlockSpace;
      logical_blocks_--;
      d.blocks.push_back(b);
      st.first_block++;
      num_blocks++;
    }
    if (d.blocks.empty()) continue;
    if (k > 0) ranges.push_back({st.seg_start + st.live_off, k, total});
    total += k;
    st.live_off += k;
    st.live_size -= k;
    if (st.num_blocks() == 0) {
      st.blocks.clear();
      st.first_block = 0;
      if (st.live_size == 0 && st.seg_cap) {
        seg_free(st.seg_start, st.seg_cap);
        st.seg_start = st.seg_cap = st.live_off = 0;
      }
    }
    dropped.push_back(std::move(d));
    touched.push_back(static_cast<int64_t>(v));
  }
  if (total > 0) {
    size_t rbytes = align_up(ranges.size() * sizeof(RangeDesc), 16);
    size_t o_dst = rbytes, o_eid = o_dst + total * 8, o_ts = o_eid + total * 8,
           bytes = o_ts + total * 4;
    pinned_.reserve(bytes);
    staging_.reserve(bytes, 0, stream_);
    std::memcpy(pinned_.data(), ranges.data(), ranges.size() * sizeof(RangeDesc));
    GF_HIP(hipMemcpyAsync(staging_.data(), pinned_.data(), rbytes, hipMemcpyHostToDevice, stream_));
    char* d = staging_.as<char>();
    unsigned grid = static_cast<unsigned>(std::min<size_t>(ranges.size(), 4096));
    gather_ranges_kernel<<<dim3(grid), dim3(256), 0, stream_>>>(
        reinterpret_cast<RangeDesc*>(d), ranges.size(), ts_pool_.as<float>(),
        nbr_pool_.as<EdgePair>(), reinterpret_cast<int64_t*>(d + o_dst),
        reinterpret_cast<int64_t*>(d + o_eid), reinterpret_cast<float*>(d + o_ts));
    GF_HIP(hipGetLastError());
    GF_HIP(hipMemcpyAsync(pinned_.as<char>() + o_dst, d + o_dst, bytes - o_dst,
                          hipMemcpyDeviceToHost, stream_));
    GF_HIP(hipStreamSynchronize(stream_));
    const int64_t* h_dst = reinterpret_cast<const int64_t*>(pinned_.as<char>() + o_dst);
    const int64_t* h_eid = reinterpret_cast<const int64_t*>(pinned_.as<char>() + o_eid);
    const float* h_ts = reinterpret_cast<const float*>(pinned_.as<char>() + o_ts);
    for (uint64_t i = 0; i < total; ++i) drop_eid(h_eid[i]);
    if (to_file) {
      // temporal_block_allocator.cu:182-221 SaveToFile record layout
      for (const Dropped& dr : dropped) {
        uint64_t off = dr.out;
        NodeState& st = nodes_[dr.node];
        for (const LogicalBlock& b : dr.blocks) {
          std::string name = "temporal_block_" + std::to_string(dr.node) + "-" +
                             std::to_string(st.saved_blocks++) + ".bin";
          std::ofstream f(name, std::ios::out | std::ios::binary);
          if (!f) throw Error(GF_ERR_IO, "cannot open " + name);
          uint64_t size = b.size, cap = b.capacity, null_ptr = 0;
          f.write(reinterpret_cast<const char*>(&size), 8);
          f.write(reinterpret_cast<const char*>(&cap), 8);
          f.write(reinterpret_cast<const char*>(&b.start_ts), 4);
          f.write(reinterpret_cast<const char*>(&b.end_ts), 4);
          f.write(reinterpret_cast<const char*>(h_dst + off), 8 * b.size);
          f.write(reinterpret_cast<const char*>(h_ts + off), 4 * b.size);
          f.write(reinterpret_cast<const char*>(h_eid + off), 8 * b.size);
          f.write(reinterpret_cast<const char*>(&null_ptr), 8);  // prev
          f.write(reinterpret_cast<const char*>(&null_ptr), 8);  // next
          off += b.size;
        }
      }
    }
  }
  upload_entries(touched);
  return num_blocks;
}

// ---- accessors: dynamic_graph.cu:289-380 -----------------------------------------
void EdgeStore::out_degree(const int64_t* nodes, size_t n, size_t* out) const {
  for (size_t i = 0; i < n; ++i) {
    GF_REQUIRE(nodes[i] >= 0 && static_cast<size_t>(nodes[i]) < nodes_.size(),
               "out_degree: vertex id out of range");
    out[i] = nodes_[nodes[i]].num_edges;
  }
}

size_t EdgeStore::nodes(int64_t* out, size_t cap, bool src_only) const {
  size_t k = 0;
  const uint8_t bit = src_only ? 2 : 1;
  for (size_t v = 0; v < seen_.size(); ++v) {
    if (!(seen_[v] & bit)) continue;
    if (out && k < cap) out[k] = static_cast<int64_t>(v);
    k++;
  }
  return k;
}

size_t EdgeStore::edges(int64_t* out, size_t cap) const {
  size_t k = 0;
  for (size_t e = 0; e < eid_dense_.size(); ++e) {
    if (!eid_dense_[e]) continue;
    if (out && k < cap) out[k] = static_cast<int64_t>(e);
    k++;
  }
  for (const auto& kv : eid_sparse_) {
    if (out && k < cap) out[k] = kv.first;
    k++;
  }
  return k;
}

size_t EdgeStore::get_temporal_neighbors(int64_t node, int64_t* dst, float* ts,
                                         int64_t* eids, size_t cap) const {
  if (node < 0 || static_cast<size_t>(node) >= nodes_.size()) return 0;
  const NodeState& st = nodes_[node];
  size_t n = st.live_size;
  if (!dst || n == 0) return n;
  GF_REQUIRE(cap >= n, "get_temporal_neighbors: output arrays too small");
  DeviceGuard dg(device_);
  std::vector<float> h_ts(n);
  std::vector<EdgePair> h_nb(n);
  uint64_t s = st.seg_start + st.live_off;
  GF_HIP(hipMemcpy(h_ts.data(), ts_pool_.as<float>() + s, n * sizeof(float), hipMemcpyDeviceToHost));
  GF_HIP(hipMemcpy(h_nb.data(), nbr_pool_.as<EdgePair>() + s, n * sizeof(EdgePair), hipMemcpyDeviceToHost));
  for (size_t i = 0; i < n; ++i) {  // newest first
    dst[i] = h_nb[n - 1 - i].dst;
    eids[i] = h_nb[n - 1 - i].eid;
    ts[i] = h_ts[n - 1 - i];
  }
  return n;
}

float EdgeStore::avg_linked_list_length() const {
  float sum = 0;
  for (size_t v = 0; v < nodes_.size(); ++v)
    if (seen_[v] & 1) sum += static_cast<float>(nodes_[v].num_blocks());
  return sum / static_cast<float>(num_nodes_);
}

float EdgeStore::metadata_mem_usage() const {
  // sizeof(TemporalBlock) * #blocks + sizeof(DoublyLinkedList) * table size
  // (dynamic_graph.cu:370-380), with this layout's 16-byte table entries
  return static_cast<float>(64 * logical_blocks_ +
                            sizeof(NodeEntry) * (any_node_ ? max_node_id_ + 1 : 0));
}

}  // namespace gf
