// EdgeStore::add_edges (DynamicGraph::AddEdges, dynamic_graph.cu:77-138): host-side ingest
// planning, phase by phase, + the HIP kernels that write the edges.  See edge_store.hpp for the
// layout; reference lines are cited on each function that restates reference behaviour.
#include "edge_store_internal.hpp"
#include "ingest_sort.hpp"

#include <chrono>
#include <cstdio>
#include <numeric>
#include <string>

namespace gf {

namespace {

constexpr size_t kIngestChunk = 1 << 23; // edges per staging upload

// ---- kernels -------------------------------------------------------------------
// Append a sorted batch: edge i goes to pool element dest[i].  Writes are 4 B + 16 B
// per edge; within one source node dest[] is consecutive, so stores coalesce.
__global__ void scatter_edges_kernel(const uint64_t* __restrict__ dest,
                                     const int64_t* __restrict__ dst,
                                     const int64_t* __restrict__ eid,
                                     const float* __restrict__ ts, size_t n,
                                     float* __restrict__ ts_pool,
                                     EdgePair* __restrict__ nbr_pool, FenceView fence) {
  size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n;
       i += stride) {
    uint64_t d = dest[i];
    ts_pool[d] = ts[i];
    fence_store(fence, d, ts[i]);
    EdgePair p;
    p.dst = dst[i];
    p.eid = eid[i];
    p.ts = ts[i];
    p.pad[0] = p.pad[1] = p.pad[2] = 0;
    nbr_pool[d] = p;
  }
}

struct MoveDesc { uint64_t src, dst, count; };

// Relocate full segments (source and destination never overlap: the destination
// is a fresh segment and frees are deferred to the end of the ingest call).
__global__ void move_segments_kernel(const MoveDesc* __restrict__ moves, size_t nmoves,
                                     float* __restrict__ ts_pool,
                                     EdgePair* __restrict__ nbr_pool, FenceView fence) {
  for (size_t m = blockIdx.x; m < nmoves; m += gridDim.x) {
    MoveDesc mv = moves[m];
    for (uint64_t i = threadIdx.x; i < mv.count; i += blockDim.x) {
      const float t = ts_pool[mv.src + i];
      ts_pool[mv.dst + i] = t;
      fence_store(fence, mv.dst + i, t);
      nbr_pool[mv.dst + i] = nbr_pool[mv.src + i];
    }
  }
}

// ---- the batch between phases ----------------------------------------------------
// GNNFLOW_INGEST_PROFILE=1: per-phase host time of add_edges on stderr
struct PhaseTimer {
  bool on;
  std::chrono::steady_clock::time_point t0;
  const char* names[12];
  double us[12];
  int k = 0;
  PhaseTimer() : on(std::getenv("GNNFLOW_INGEST_PROFILE") != nullptr),
                 t0(std::chrono::steady_clock::now()) {}
  void mark(const char* name) {
    if (!on || k >= 12) return;
    auto t1 = std::chrono::steady_clock::now();
    names[k] = name;
    us[k++] = std::chrono::duration<double, std::micro>(t1 - t0).count();
    t0 = t1;
  }
  void report(size_t n) {
    if (!on) return;
    double tot = 0;
    for (int i = 0; i < k; ++i) tot += us[i];
    std::fprintf(stderr, "add_edges n=%zu %.1f ms (%.1f M edges/s):", n, tot / 1e3, n / tot);
    for (int i = 0; i < k; ++i) std::fprintf(stderr, " %s %.1f", names[i], us[i] / 1e3);
    std::fprintf(stderr, "\n");
  }
};

struct Group { int64_t v; size_t begin, end; };
// the runs of equal source: a host vector (host ordering), or a view of the device
// ordering's group table in pinned memory (no 6.5 M-element vector to build per chunk)
struct GroupList {
  std::vector<Group> host;
  const uint32_t* src = nullptr;
  const uint32_t* start = nullptr;
  size_t n = 0;
  size_t size() const { return src ? n : host.size(); }
  Group operator[](size_t g) const {
    return src ? Group{static_cast<int64_t>(src[g]), start[g], start[g + 1]} : host[g];
  }
  void push_back(const Group& g) { host.push_back(g); }
};

struct Joiner { std::thread t; ~Joiner() { if (t.joinable()) t.join(); } };

// The per-group passes of add_edges walk `nodes_` in increasing vertex order but with gaps:
// nearly every group is a cache miss on its NodeState (its newest block sits inline in it).
// Software prefetch: the NodeState of the group 16 ahead.
inline void prefetch_groups(const NodeTable& nodes, const GroupList& groups, size_t g,
                            size_t g_end) {
  if (g + 16 < g_end) {
    const size_t v = static_cast<size_t>(groups[g + 16].v);
    if (v < nodes.size()) __builtin_prefetch(&nodes[v], 1, 1);
  }
}

// The segment decision: the power-of-two capacity of the larger segment a vertex (null: never
// seen) needs before it takes `cnt` more edges, 0 when they fit the one it has.
inline uint64_t grown_segment_cap(const NodeState* st, size_t cnt, uint64_t min_phys) {
  const uint64_t need = (st ? st->live_size : 0) + cnt;
  if (st && st->seg_cap != 0 && st->live_off + need <= st->seg_cap) return 0;
  return pow2_ceil(need < min_phys ? min_phys : need);
}

// why validate_batch rejects a group
__attribute__((noinline)) std::string group_error(int code, int64_t v, float t, float last_ts) {
  if (code == GF_ERR_INVALID_ARGUMENT) return "add_edges: more than 2^32-1 live edges on one vertex";
  return "add_edges: vertex " + std::to_string(v) + " got an edge at t=" + std::to_string(t) +
         " older than its newest stored edge t=" + std::to_string(last_ts);
}

}  // namespace

struct EdgeStore::IngestBatch {
  const int64_t *src, *dst, *eids;   // the call's arguments
  const float* ts;
  size_t n;
  PhaseTimer pt;
  int64_t max_node = 0;              // scan
  // order: `groups` are the runs of equal source in (source, timestamp, input position) order
  // and `s_ts` the timestamps in it; everything after the ordering works per GROUP
  bool on_device = false;
  GroupList groups;
  std::vector<uint32_t> perm;        // host path only
  std::vector<float> s_ts_vec;
  const float* s_ts = nullptr;
  // plan
  uint64_t min_phys = 1;             // smallest physical segment
  std::vector<Move> moves;
  std::vector<std::pair<uint64_t, uint64_t>> deferred_free;
  std::vector<uint64_t> dest;        // host path: per-edge destinations for the staging copy
  size_t new_nodes = 0, new_srcs = 0;   // added to the counters once the helper has joined
};

// ---- block policy: dynamic_graph.cu:206-287 AddEdgesForOneNode -------------------
struct EdgeStore::BlockStep {
  size_t fill;       // edges that go into the tail block (after `tail_cap` took effect)
  size_t open_cap;   // capacity of the block to open for the rest, 0: none
  size_t tail_cap;   // replace policy: the tail's new capacity, 0: it keeps its own
};

// (the pool limit is checked for the whole batch before anything is mutated, validate_batch;
// the byte / block counters are accumulated per thread and applied by the caller)
struct EdgeStore::BlockDelta {
  size_t bytes = 0, blocks = 0;   // (a step never shrinks anything: both only grow)
  void count(const BlockStep& s, const LogicalBlock* tail) {
    if (s.open_cap) { bytes += s.open_cap * kBlockSpace; blocks++; }
    if (s.tail_cap) bytes += (s.tail_cap - tail->capacity) * kBlockSpace;
  }
};

// What the reference does with `cnt` (> 0) more edges of a vertex whose newest block is `tail`
// (null: no live block) — a pure function of its arguments and the store's configuration.
inline EdgeStore::BlockStep EdgeStore::block_step(const LogicalBlock* tail, uint64_t num_edges,
                                                  uint64_t num_insertions, size_t cnt) const {
  // temporal_block_allocator.cu:83-88,134-149 (AlignUp in AllocateInternal)
  auto clamped = [&](size_t x) { return x < minimum_block_size_ ? minimum_block_size_ : x; };
  if (!tail) return {0, clamped(cnt), 0};                       // case 1: empty list
  if (tail->size + cnt <= tail->capacity) return {cnt, 0, 0};   // case 3: fits in the tail
  if (insertion_policy_ != GF_INSERTION_POLICY_INSERT)          // case 2: tail overflows
    return {cnt, 0, clamped(tail->size + cnt)};                 //   replace: Reallocate(size + n)
  const size_t fill = tail->capacity - tail->size, num = cnt - fill;
  const size_t avg = num_insertions == 0 ? num : num_edges / num_insertions;
  return {fill, clamped(adaptive_ ? pow2_ceil(std::max(num, avg)) : num), 0};
}

// block_step applied to the block headers + utils.cu:33-63 CopyEdgesToBlock (headers only: the
// bytes live in the node's flat segment).
void EdgeStore::simulate_blocks(NodeState& st, const float* ts, size_t n, BlockDelta* delta) {
  auto copy_to = [&](LogicalBlock& b, size_t start_idx, size_t cnt) {
    b.size += cnt;
    b.start_ts = std::min(b.start_ts, ts[start_idx]);
    b.end_ts = ts[start_idx + cnt - 1];
  };
  LogicalBlock* tail = st.num_blocks() ? &st.blocks.back() : nullptr;
  const BlockStep s = block_step(tail, st.num_edges, st.num_insertions, n);
  delta->count(s, tail);
  if (s.tail_cap) tail->capacity = s.tail_cap;
  if (s.fill) copy_to(*tail, 0, s.fill);
  if (s.open_cap) {   // AllocateInternal header init
    st.blocks.push_back({0, s.open_cap, std::numeric_limits<float>::max(), 0});
    copy_to(st.blocks.back(), s.fill, n - s.fill);
  }
  st.num_edges += n;
  st.num_insertions++;
}

// `edges_[eid]++` for a batch (dynamic_graph.cu:93-95; num_edges() = distinct ids).  Dense
// counters for the usual non-negative, roughly contiguous eids, grown once per batch from the
// batch's largest id; ids they do not cover (negative, or far beyond what has been inserted)
// go through a hash map.
void EdgeStore::bump_eids(const int64_t* eids, size_t n) {
  int64_t mx = -1, mn = 0;
  bool consecutive = n > 0;   // eids[i] == eids[0] + i for the whole batch (a running counter)
  {
    std::mutex mu;
    parallel_for(n, 1 << 16, [&](size_t i0, size_t i1) {
      int64_t m = -1, lo = 0;
      bool run = true;
      const int64_t base = eids[0] - 0;
      for (size_t i = i0; i < i1; ++i) {
        m = std::max(m, eids[i]);
        lo = std::min(lo, eids[i]);
        run &= eids[i] == base + static_cast<int64_t>(i);
      }
      std::lock_guard<std::mutex> lk(mu);
      mx = std::max(mx, m);
      mn = std::min(mn, lo);
      consecutive = consecutive && run;
    });
  }
  eid_max_ = std::max(eid_max_, mx);
  eid_min_ = std::min(eid_min_, mn);
  const uint64_t budget = 64 + 8 * (eids_inserted_ + n);   // dense only while reasonably full
  if (mx >= 0 && static_cast<uint64_t>(mx) >= eid_dense_.size() &&
      static_cast<uint64_t>(mx) < budget) {
    const size_t nsz = static_cast<size_t>(mx) + 1;
    eid_dense_.resize(nsz);
    for (auto it = eid_sparse_.begin(); it != eid_sparse_.end();) {   // keep "eid <
      if (it->first >= 0 && static_cast<uint64_t>(it->first) < nsz) {  // dense.size() =>
        eid_dense_[it->first] += static_cast<uint32_t>(it->second);    // counted densely"
        it = eid_sparse_.erase(it);
      } else {
        ++it;
      }
    }
  }
  const uint64_t dense = eid_dense_.size();
  std::mutex mu;
  if (consecutive && eids[0] >= 0 && static_cast<uint64_t>(eids[0]) + n <= dense) {
    // the batch's ids are one run of the dense counters: every thread owns its part of the
    // run, no locked read-modify-write (10^7 of those are ~50 ms on four threads)
    const size_t first = static_cast<size_t>(eids[0]);
    parallel_for(n, 1 << 16, [&](size_t i0, size_t i1) {
      size_t fresh = 0;
      for (size_t i = i0; i < i1; ++i) fresh += eid_dense_[first + i]++ == 0 ? 1 : 0;
      std::lock_guard<std::mutex> lk(mu);
      num_live_eids_ += fresh;
    });
    eids_inserted_ += n;
    return;
  }
  parallel_for(n, 1 << 16, [&](size_t i0, size_t i1) {
    size_t fresh = 0;
    std::vector<int64_t> sparse;
    for (size_t i = i0; i < i1; ++i) {
      const int64_t e = eids[i];
      if (e >= 0 && static_cast<uint64_t>(e) < dense) {
        if (__atomic_fetch_add(&eid_dense_[e], 1u, __ATOMIC_RELAXED) == 0) fresh++;
      } else {
        sparse.push_back(e);
      }
    }
    std::lock_guard<std::mutex> lk(mu);
    num_live_eids_ += fresh;
    for (int64_t e : sparse)
      if (eid_sparse_[e]++ == 0) num_live_eids_++;
  });
  eids_inserted_ += n;
}

// ---- add_edges, phase by phase ----------------------------------------------------
void EdgeStore::scan_batch(IngestBatch& b) {
  const int64_t* src = b.src;
  const int64_t* dst = b.dst;
  const float* ts = b.ts;
  std::mutex mu;
  bool negative = false;
  size_t first_nan = b.n;
  parallel_for(b.n, 1 << 16, [&](size_t i0, size_t i1) {
    int64_t m = 0;
    bool neg = false, nan = false;
    for (size_t i = i0; i < i1; ++i) {
      neg |= (src[i] < 0) | (dst[i] < 0);
      nan |= ts[i] != ts[i];
      m = std::max(m, std::max(src[i], dst[i]));
    }
    size_t at = i1;   // where: looked up only in a part that has one, off the loop above
    if (nan)
      for (at = i0; ts[at] == ts[at]; ++at) {}
    std::lock_guard<std::mutex> lk(mu);
    b.max_node = std::max(b.max_node, m);
    negative |= neg;
    if (nan) first_nan = std::min(first_nan, at);
  });
  GF_REQUIRE(!negative, "add_edges: negative vertex id");
  // no ordering has a place for a NaN: `<` is not an order over it, and every later search of
  // the vertex's run assumes one
  GF_REQUIRE(first_nan == b.n,
             "add_edges: NaN timestamp at position " + std::to_string(first_nan));
}

// 1. order by (source, timestamp, input position): the reference groups by
//    source in input order and stable-sorts each group by timestamp
//    (dynamic_graph.cu:105-128, utils.h:16-27).
//    Batches worth it are ordered on the device (ingest_sort.hip: radix sort + group table;
//    the per-edge permutation then never exists on the host), small ones — the online
//    600-edge ingests, where a sort launch chain would cost more than the whole call — by
//    the host counting sort.
void EdgeStore::order_on_device(IngestBatch& b) {
  if (!sorter_holder_) sorter_holder_.reset(new IngestSorter());
  unsigned node_bits = 1;
  while (node_bits < 32 && (static_cast<uint64_t>(b.max_node) >> node_bits)) ++node_bits;
  const size_t G = sorter_holder_->order(b.src, b.dst, b.ts, b.eids, b.n, node_bits, stream_);
  b.pt.mark("dsort");
  // pinned landing buffers: a pageable D2H of the 40 MB of sorted timestamps alone costs
  // more than the sort
  const size_t o_start = align_up(G * 4, 64), o_sts = o_start + align_up((G + 1) * 4, 64);
  order_pinned_.reserve(o_sts + b.n * 4);
  uint32_t* g_src = order_pinned_.as<uint32_t>();
  uint32_t* g_start = reinterpret_cast<uint32_t*>(order_pinned_.as<char>() + o_start);
  float* h_sts = reinterpret_cast<float*>(order_pinned_.as<char>() + o_sts);
  sorter_holder_->download(g_src, g_start, h_sts, stream_);
  g_start[G] = static_cast<uint32_t>(b.n);
  b.s_ts = h_sts;
  b.groups.src = g_src;
  b.groups.start = g_start;
  b.groups.n = G;
  b.pt.mark("groups");
}

void EdgeStore::order_on_host(IngestBatch& b) {
  const int64_t* src = b.src;
  const float* ts = b.ts;
  const size_t n = b.n;
  std::vector<uint32_t>& perm = b.perm;
  std::vector<float>& st = b.s_ts_vec;
  perm.resize(n);
  st.resize(n);
  const size_t table_len = static_cast<size_t>(b.max_node) + 1;
  if (table_len <= 4 * n + (1u << 16)) {
    // counting sort by source (stable), then fix up unsorted groups by time
    std::vector<uint32_t> head(table_len + 1, 0);
    for (size_t i = 0; i < n; ++i) head[src[i] + 1]++;
    for (size_t v = 0; v < table_len; ++v) head[v + 1] += head[v];
    {
      std::vector<uint32_t> cur(head.begin(), head.end() - 1);
      for (size_t i = 0; i < n; ++i) perm[cur[src[i]]++] = static_cast<uint32_t>(i);
    }
    b.pt.mark("csort");
    parallel_for(table_len, 1 << 14, [&](size_t v0, size_t v1) {
      for (size_t v = v0; v < v1; ++v) {
        const size_t a = head[v], e = head[v + 1];
        bool sorted = true;
        for (size_t k = a; k < e; ++k) {
          st[k] = ts[perm[k]];
          if (k > a && st[k] < st[k - 1]) sorted = false;
        }
        if (!sorted) {
          std::stable_sort(perm.begin() + a, perm.begin() + e,
                           [&](uint32_t x, uint32_t y) { return ts[x] < ts[y]; });
          for (size_t k = a; k < e; ++k) st[k] = ts[perm[k]];
        }
      }
    });
    b.pt.mark("tsgather");
    for (size_t v = 0; v < table_len; ++v)
      if (head[v + 1] > head[v]) b.groups.push_back({static_cast<int64_t>(v), head[v], head[v + 1]});
  } else {
    std::iota(perm.begin(), perm.end(), 0u);
    std::sort(perm.begin(), perm.end(), [&](uint32_t x, uint32_t y) {
      if (src[x] != src[y]) return src[x] < src[y];
      if (ts[x] < ts[y]) return true;
      if (ts[y] < ts[x]) return false;
      return x < y;
    });
    parallel_for(n, 1 << 16, [&](size_t k0, size_t k1) {
      for (size_t k = k0; k < k1; ++k) st[k] = ts[perm[k]];
    });
    for (size_t i = 0; i < n;) {
      const int64_t v = src[perm[i]];
      size_t j = i;
      while (j < n && src[perm[j]] == v) ++j;
      b.groups.push_back({v, i, j});
      i = j;
    }
  }
  b.s_ts = st.data();
  b.pt.mark("sort");
}

// 2. validate before mutating anything: a group's oldest new edge must not be
//    older than the node's newest stored edge (reference: CHECK_LE ->
//    abort, utils.cu:42-43; the docstring promises ValueError,
//    gnnflow/dynamic_graph.py:99-101) — and a dry run of everything that can fail later:
//    the logical block bytes the batch adds (block_step, i.e. dynamic_graph.cu:206-287
//    against the rmm pool limit) and the pool elements its new segments need (what
//    plan_segments will take: free lists first, the bump pointer for the rest).  A batch that
//    does not fit is rejected HERE — no vertex, counter, block list or allocator state has
//    been touched yet, so the graph stays exactly as it was.
void EdgeStore::validate_batch(const IngestBatch& b) {
  const GroupList& groups = b.groups;
  const float* s_ts = b.s_ts;
  const size_t G = groups.size();
  const uint64_t min_phys = b.min_phys;
  std::mutex mu;
  size_t add_bytes = 0;
  std::vector<uint64_t> demand(free_lists_.size(), 0);   // new segments per size class
  std::string first_error;
  int first_code = GF_OK;
  size_t first_at = G;
  parallel_for(G, 1 << 14, [&](size_t g0, size_t g1) {
    BlockDelta delta;
    std::vector<uint64_t> dem(free_lists_.size(), 0);
    for (size_t g = g0; g < g1; ++g) {
      prefetch_groups(nodes_, groups, g, g1);
      const Group& gr = groups[g];
      const size_t cnt = gr.end - gr.begin;
      const NodeState* st =
          static_cast<size_t>(gr.v) < nodes_.size() ? &nodes_[gr.v] : nullptr;
      if (st) {
        const int code = s_ts[gr.begin] < st->last_ts ? GF_ERR_TIMESTAMP_ORDER
                         : st->live_size + cnt >= 0xFFFFFFFFull ? GF_ERR_INVALID_ARGUMENT : GF_OK;
        if (code != GF_OK) {   // the message is built here only: off the loop's fast path
          std::lock_guard<std::mutex> lk(mu);
          if (g < first_at) {
            first_at = g;
            first_code = code;
            first_error = group_error(code, gr.v, s_ts[gr.begin], st->last_ts);
          }
          continue;
        }
      }
      const LogicalBlock* tail = st && st->num_blocks() ? &st->blocks.back() : nullptr;
      delta.count(block_step(tail, st ? st->num_edges : 0, st ? st->num_insertions : 0, cnt),
                  tail);
      if (const uint64_t cap = grown_segment_cap(st, cnt, min_phys)) dem[log2_exact(cap)]++;
    }
    std::lock_guard<std::mutex> lk(mu);
    add_bytes += delta.bytes;
    for (size_t c = 0; c < dem.size(); ++c) demand[c] += dem[c];
  });
  if (first_code != GF_OK) throw Error(first_code, first_error);
  if (logical_bytes_ + add_bytes > maximum_pool_size_) {
    throw Error(GF_ERR_OUT_OF_MEMORY,
                "maximum_pool_size exceeded: temporal blocks need " +
                    std::to_string(logical_bytes_ + add_bytes) + " bytes > " +
                    std::to_string(maximum_pool_size_) + " (batch rejected, graph unchanged)");
  }
  uint64_t extra = 0;   // what the free lists cannot serve comes off the bump pointer
  for (size_t c = 0; c < demand.size(); ++c)
    if (demand[c] > free_lists_[c].size()) extra += (demand[c] - free_lists_[c].size()) << c;
  ensure_pool(bump_ + extra);   // a failing hipMalloc also surfaces before any mutation
}

// 3. bookkeeping sets (dynamic_graph.cu:89-103): several threads, atomic test-and-set on the
//    per-vertex bytes / per-edge-id counters; they share nothing with the planning passes
//    (seen_ / eid counters vs nodes_ and the segment allocator), so big batches update them
//    on a helper thread meanwhile.
void EdgeStore::update_sets(const IngestBatch& b) {
  // A locked read-modify-write on a cold line costs ~10x a load, and after the first
  // batches nearly every vertex has been seen: test with a plain load, set only when a bit
  // is missing.  Sources are marked once per GROUP (distinct source), not once per edge:
  // by plan_blocks, which visits every group anyway.  A handful of threads here: the planning
  // passes run at the same time.
  const int64_t* dst = b.dst;
  std::mutex mu;
  parallel_for(b.n, 1 << 16, 4, [&](size_t i0, size_t i1) {
    size_t nn = 0;
    for (size_t i = i0; i < i1; ++i) {
      // random bytes of a table that is 120 MB at MAG scale: fetch ahead
      if (i + 32 < i1) __builtin_prefetch(&seen_[dst[i + 32]], 0, 1);
      uint8_t cur = __atomic_load_n(&seen_[dst[i]], __ATOMIC_RELAXED);
      if (cur & 1) continue;
      cur = __atomic_fetch_or(&seen_[dst[i]], 1, __ATOMIC_RELAXED);
      nn += !(cur & 1);
    }
    std::lock_guard<std::mutex> lk(mu);
    num_nodes_ += nn;
  });
  bump_eids(b.eids, b.n);
}

// 4. plan: logical blocks, physical segments, one base destination per group.
//    Pass A (parallel over groups — every group is another vertex): replay the block policy
//    and decide whether the vertex needs a larger segment.  Pass B (only the groups that do):
//    the segment allocator.  Pass C (parallel): bases, live ranges.
void EdgeStore::plan_blocks(IngestBatch& b) {
  const GroupList& groups = b.groups;
  const float* s_ts = b.s_ts;
  const size_t G = groups.size();
  // per-group scratch kept across calls: a fresh 52 MB std::vector per 10^7-edge chunk is an
  // mmap + 13 k page faults + munmap every time
  if (gbase_.size() < G) { gbase_.resize(G); newcap_.resize(G); }
  uint64_t* newcap = newcap_.data();   // every entry is written here
  const uint64_t min_phys = b.min_phys;
  std::mutex mu;
  parallel_for(G, 1 << 13, [&](size_t g0, size_t g1) {
    BlockDelta delta;
    size_t new_nodes = 0, new_srcs = 0;
    for (size_t g = g0; g < g1; ++g) {
      prefetch_groups(nodes_, groups, g, g1);
      const Group& gr = groups[g];
      const size_t cnt = gr.end - gr.begin;
      NodeState& st = nodes_[gr.v];
      simulate_blocks(st, s_ts + gr.begin, cnt, &delta);
      newcap[g] = grown_segment_cap(&st, cnt, min_phys);
      // bookkeeping sets, source side (dynamic_graph.cu:89-103): once per distinct source
      uint8_t cur = __atomic_load_n(&seen_[gr.v], __ATOMIC_RELAXED);
      if ((cur & 3) != 3) {
        cur = __atomic_fetch_or(&seen_[gr.v], 3, __ATOMIC_RELAXED);
        new_nodes += !(cur & 1);
        new_srcs += !(cur & 2);
      }
    }
    std::lock_guard<std::mutex> lk(mu);
    logical_bytes_ += delta.bytes;
    logical_blocks_ += delta.blocks;
    b.new_nodes += new_nodes;
    b.new_srcs += new_srcs;
  });
}

// Pass B, the segment allocator, in parallel too: the requests of one size class are ranked
// in group order (per-chunk counts, then a prefix over the chunks); the first ones take the
// class's free list from its back and the rest share one run off the bump pointer, class after
// class.  Where a segment lies is not observable, only that every vertex gets one of the right
// size.
void EdgeStore::plan_segments(IngestBatch& b) {
  const GroupList& groups = b.groups;
  const size_t G = groups.size();
  const uint64_t* newcap = newcap_.data();
  constexpr size_t kChunk = 1 << 13;
  const size_t nchunks = (G + kChunk - 1) / kChunk;
  const size_t ncls = free_lists_.size();
  std::vector<uint32_t> rank0(nchunks * ncls, 0);   // requests per (chunk, class), then ranks
  parallel_for(nchunks, 1, [&](size_t c0, size_t c1) {
    for (size_t c = c0; c < c1; ++c) {
      uint32_t* cnt = &rank0[c * ncls];
      const size_t g1 = std::min(G, (c + 1) * kChunk);
      for (size_t g = c * kChunk; g < g1; ++g)
        if (newcap[g]) cnt[log2_exact(newcap[g])]++;
    }
  });
  std::vector<uint64_t> total(ncls, 0), from_free(ncls, 0), bump_base(ncls, 0);
  for (size_t c = 0; c < nchunks; ++c)
    for (size_t k = 0; k < ncls; ++k) {
      const uint32_t here = rank0[c * ncls + k];
      rank0[c * ncls + k] = static_cast<uint32_t>(total[k]);
      total[k] += here;
    }
  uint64_t bump = bump_;
  for (size_t k = 0; k < ncls; ++k) {
    from_free[k] = std::min<uint64_t>(total[k], free_lists_[k].size());
    bump_base[k] = bump;
    bump += (total[k] - from_free[k]) << k;
  }
  std::vector<std::vector<Move>> chunk_moves(nchunks);
  std::vector<std::vector<std::pair<uint64_t, uint64_t>>> chunk_free(nchunks);
  parallel_for(nchunks, 1, [&](size_t c0, size_t c1) {
    std::vector<uint32_t> next(ncls);
    for (size_t c = c0; c < c1; ++c) {
      for (size_t k = 0; k < ncls; ++k) next[k] = rank0[c * ncls + k];
      const size_t g1 = std::min(G, (c + 1) * kChunk);
      for (size_t g = c * kChunk; g < g1; ++g) {
        if (!newcap[g]) continue;
        const int k = log2_exact(newcap[g]);
        const uint64_t j = next[k]++;
        const auto& fl = free_lists_[k];
        const uint64_t ns = j < from_free[k] ? fl[fl.size() - 1 - j]
                                             : bump_base[k] + ((j - from_free[k]) << k);
        NodeState& st = nodes_[groups[g].v];
        if (st.seg_cap) {
          if (st.live_size) chunk_moves[c].push_back({st.seg_start + st.live_off, ns, st.live_size});
          chunk_free[c].emplace_back(st.seg_start, st.seg_cap);
        }
        st.seg_start = ns;
        st.seg_cap = newcap[g];
        st.live_off = 0;
      }
    }
  });
  for (size_t k = 0; k < ncls; ++k)
    free_lists_[k].resize(free_lists_[k].size() - from_free[k]);
  bump_ = bump;
  for (size_t c = 0; c < nchunks; ++c) {
    b.moves.insert(b.moves.end(), chunk_moves[c].begin(), chunk_moves[c].end());
    b.deferred_free.insert(b.deferred_free.end(), chunk_free[c].begin(), chunk_free[c].end());
  }
}

void EdgeStore::plan_bases(IngestBatch& b) {
  const GroupList& groups = b.groups;
  const float* s_ts = b.s_ts;
  const size_t G = groups.size();
  const bool on_device = b.on_device;
  if (!on_device) b.dest.resize(b.n);
  uint64_t* dest = b.dest.data();
  uint64_t* gbase = gbase_.data();
  // the node-table entries to publish are written here, while the vertex record is in cache
  // (a separate pass over the records just to read them back cost 5 ms per 10^7 edges)
  publish_pinned_.reserve(G * (sizeof(int64_t) + sizeof(NodeEntry)));
  int64_t* pub_ids = publish_pinned_.as<int64_t>();
  NodeEntry* pub_ent = reinterpret_cast<NodeEntry*>(pub_ids + G);
  parallel_for(G, 1 << 13, [&](size_t g0, size_t g1) {
    for (size_t g = g0; g < g1; ++g) {
      if (g + 16 < g1) __builtin_prefetch(&nodes_[groups[g + 16].v], 1, 1);
      const Group& gr = groups[g];
      const size_t cnt = gr.end - gr.begin;
      NodeState& st = nodes_[gr.v];
      const uint64_t base = st.seg_start + st.live_off + st.live_size;
      gbase[g] = base;
      if (!on_device)
        for (size_t k = 0; k < cnt; ++k) dest[gr.begin + k] = base + k;
      st.live_size += cnt;
      st.last_ts = s_ts[gr.end - 1];
      if (s_ts[gr.begin] < 0.0f) negative_ts_.store(true, std::memory_order_relaxed);
      pub_ids[g] = gr.v;
      pub_ent[g] = node_entry(st);
    }
  });
  GF_REQUIRE(bump_ <= pool_elems_, "add_edges: internal error: pool smaller than planned");
}

// 5. device: relocate grown segments, then scatter the batch, then publish entries
void EdgeStore::run_device_phase(IngestBatch& b) {
  const size_t n = b.n;
  if (!b.moves.empty()) {
    size_t bytes = b.moves.size() * sizeof(MoveDesc);
    pinned_.reserve(bytes);
    staging_.reserve(bytes, 0, stream_);
    std::memcpy(pinned_.data(), b.moves.data(), bytes);
    GF_HIP(hipMemcpyAsync(staging_.data(), pinned_.data(), bytes, hipMemcpyHostToDevice, stream_));
    unsigned grid = static_cast<unsigned>(std::min<size_t>(b.moves.size(), 4096));
    move_segments_kernel<<<dim3(grid), dim3(256), 0, stream_>>>(
        staging_.as<MoveDesc>(), b.moves.size(), ts_pool_.as<float>(), nbr_pool_.as<EdgePair>(),
        fence_view_);
    GF_HIP(hipGetLastError());
    GF_HIP(hipStreamSynchronize(stream_));  // staging is reused below
  }
  if (b.on_device) {
    sorter_holder_->scatter(gbase_.data(), ts_pool_.as<float>(), nbr_pool_.as<EdgePair>(),
                            fence_view_, stream_);
    GF_HIP(hipStreamSynchronize(stream_));   // gbase_ is a host vector
  } else {
    const uint32_t* perm = b.perm.data();
    const uint64_t* dest = b.dest.data();
    const int64_t* dst = b.dst;
    const int64_t* eids = b.eids;
    const float* s_ts = b.s_ts;
    for (size_t off = 0; off < n; off += kIngestChunk) {
      size_t m = std::min(kIngestChunk, n - off);
      size_t o_dst = m * sizeof(uint64_t), o_eid = o_dst + m * sizeof(int64_t),
             o_ts = o_eid + m * sizeof(int64_t), bytes = o_ts + m * sizeof(float);
      pinned_.reserve(bytes);
      staging_.reserve(bytes, 0, stream_);
      char* h = pinned_.as<char>();
      uint64_t* h_dest = reinterpret_cast<uint64_t*>(h);
      int64_t* h_dst = reinterpret_cast<int64_t*>(h + o_dst);
      int64_t* h_eid = reinterpret_cast<int64_t*>(h + o_eid);
      float* h_ts = reinterpret_cast<float*>(h + o_ts);
      parallel_for(m, 1 << 16, [&](size_t k0, size_t k1) {
        for (size_t k = k0; k < k1; ++k) {
          const size_t p = perm[off + k];
          h_dest[k] = dest[off + k];
          h_dst[k] = dst[p];
          h_eid[k] = eids[p];
          h_ts[k] = s_ts[off + k];
        }
      });
      GF_HIP(hipMemcpyAsync(staging_.data(), h, bytes, hipMemcpyHostToDevice, stream_));
      char* d = staging_.as<char>();
      unsigned grid = static_cast<unsigned>(std::min<size_t>((m + 255) / 256, 8192));
      scatter_edges_kernel<<<dim3(grid), dim3(256), 0, stream_>>>(
          reinterpret_cast<uint64_t*>(d), reinterpret_cast<int64_t*>(d + o_dst),
          reinterpret_cast<int64_t*>(d + o_eid), reinterpret_cast<float*>(d + o_ts), m,
          ts_pool_.as<float>(), nbr_pool_.as<EdgePair>(), fence_view_);
      GF_HIP(hipGetLastError());
      GF_HIP(hipStreamSynchronize(stream_));  // the pinned chunk is refilled next
    }
  }
  b.pt.mark("device");
  // the moves above read the old segments: freed only now
  for (auto& f : b.deferred_free) seg_free(f.first, f.second);
  publish_entries(publish_pinned_, b.groups.size());  // ends with the stream sync of dynamic_graph.cu:135-137
}

void EdgeStore::add_edges(const int64_t* src, const int64_t* dst, const float* ts,
                          const int64_t* eids, size_t n) {
  GF_REQUIRE(n > 0, "add_edges: empty batch (reference: CHECK_GT(src_nodes.size(), 0))");
  GF_REQUIRE(src && dst && ts && eids, "add_edges: null array");
  GF_REQUIRE(n < 0xFFFFFFFFull, "add_edges: more than 2^32-1 edges in one call");
  DeviceGuard dg(device_);
  IngestBatch b{src, dst, eids, ts, n};
  b.min_phys = pow2_ceil(minimum_block_size_);   // (1 for a minimum of 0)
  PhaseTimer& pt = b.pt;

  scan_batch(b);
  pt.mark("scan");
  static const size_t device_sort_min = [] {
    const char* v = std::getenv("GNNFLOW_INGEST_DEVICE_SORT_MIN");   // tests: 0 = always
    return v ? static_cast<size_t>(std::atoll(v)) : (size_t(1) << 17);
  }();
  b.on_device = n >= device_sort_min && n < 0x7FFFFFFFull &&
                static_cast<uint64_t>(b.max_node) < 0xFFFFFFFFull;
  if (b.on_device) order_on_device(b); else order_on_host(b);

  validate_batch(b);
  pt.mark("validate");
  add_nodes(b.max_node);
  // Declared after everything the helper reads (the batch; the pinned group table is a
  // member), so that it is joined first, also when a later phase throws.
  Joiner sets_thread;
  if (n >= (size_t(1) << 18)) sets_thread.t = std::thread([&] { update_sets(b); });
  else update_sets(b);
  pt.mark("sets");

  plan_blocks(b);
  pt.mark("planA");
  plan_segments(b);
  pt.mark("planB");
  plan_bases(b);
  pt.mark("planC");
  run_device_phase(b);
  pt.mark("publish");
  // the bookkeeping helper shares nothing with the device phase either: joined last
  if (sets_thread.t.joinable()) sets_thread.t.join();
  num_nodes_ += b.new_nodes;
  num_src_nodes_ += b.new_srcs;
  pt.mark("join");
  pt.report(n);
}

}  // namespace gf
