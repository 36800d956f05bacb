// What the translation units of the sampler share (sample_layer.hip, sample_padded.hip,
// sample_merge.hip, sampler_group.hip, sampler.hip): the launch constants, the kernel-argument
// structs, the device helpers more than one of them uses and the launchers that cross units.
// Private to those files.
#pragma once

#include "sampler.hpp"

#include <algorithm>

namespace gf {

constexpr int kSearchThreads = 256;
constexpr int kEmitThreads = 256;
constexpr int kScanThreads = 1024;
constexpr int kScanItems = 4;  // per thread per tile
constexpr size_t kSmallRoots = 32768;  // layers up to this many roots skip the scan launch
constexpr uint32_t kGranuleSpins = 1u << 12;   // ~ a few ms of polling before a tile is recounted
constexpr size_t kLaneSearchRoots = size_t{1} << 20;   // layers from this many roots: lane-per-root pass
constexpr uint32_t kMaxHubSegs = 2048;         // = the lane pass's largest grid
constexpr int kScanTile = 4096;   // roots per tile of the parallel scan (sample_layer.hip, 2b)
constexpr int kCompactThreads = 1024;   // reply_compact_kernel's workgroup
constexpr uint64_t kGranuleCountMask = 0x3FF;      // a tile has kEmitThreads = 256 slots

// sampling_kernels.cu:28-40
__device__ inline void time_window(float root_ts, uint32_t snapshot_idx,
                                   uint32_t num_snapshots, float window, float* start,
                                   float* end) {
  if (num_snapshots == 1) {
    *start = (fabs(static_cast<double>(window)) < 1e-6) ? 0.0f : root_ts - window;
    *end = root_ts;
  } else {
    float k = static_cast<float>(num_snapshots - snapshot_idx - 1);
    *end = fmaf(-k, window, root_ts);  // nvcc contracts `t - k*w` (see oracle)
    *start = *end - window;
  }
}

template <int GROUP>
__device__ inline uint32_t group_count(bool pred, int group_in_wave) {
  unsigned long long m = __ballot(pred);
  if (GROUP == 64) return __popcll(m);
  return __popcll((m >> (group_in_wave * GROUP)) & ((1ull << GROUP) - 1ull));
}

// First index in [0, n) with ts[idx] >= x (utils.cu:96-109 LowerBound), evaluated
// cooperatively by a GROUP-lane group; every lane returns the result.
template <int GROUP>
__device__ inline uint32_t lower_bound_group(const float* __restrict__ ts, uint32_t n,
                                             float x, int lane, int group_in_wave) {
  uint32_t lo = 0, hi = n;
  while (hi - lo > GROUP) {
    uint32_t span = hi - lo;
    uint32_t stride = (span + GROUP - 1) / GROUP;
    uint32_t p = lo + lane * stride;
    bool less = (p < hi) && (ts[p] < x);
    uint32_t c = group_count<GROUP>(less, group_in_wave);
    if (c == 0) {
      hi = lo;
    } else {
      uint32_t nlo = lo + (c - 1) * stride + 1;
      uint32_t nhi = lo + c * stride;
      hi = nhi < hi ? nhi : hi;
      lo = nlo;
    }
  }
  uint32_t p = lo + lane;
  bool less = (p < hi) && (ts[p] < x);
  return lo + group_count<GROUP>(less, group_in_wave);
}

// The same lower bound over the segment [s, s + n) of the timestamp pool, through the fences
// (edge_store.hpp: fence_l[g] = ts_pool[(g + 1) * 16^l - 1], global positions): from the
// coarsest level whose blocks are smaller than the segment down to level 1, every round takes
// the (<= 17) fences whose positions lie inside the current range as pivots — they are
// CONSECUTIVE entries of the level, i.e. one or two 64-byte lines, read by the group as
// contiguous 16-byte / 4-byte loads — and narrows the range to the gap between two of them;
// the last <= 16-element gap is resolved on the timestamps themselves.  ceil(log16 n) rounds
// of one line each, where the strided k-ary search reads GROUP sectors per round
// (sample_search_kernel<4> on the 10 M-node graph: 2.4-4.6x the algorithmic bytes).
template <int GROUP>
__device__ inline uint32_t lower_bound_fenced(const GraphView& g, uint64_t s, uint32_t n, float x,
                                              int lane, int group_in_wave) {
  constexpr int V = 16 / GROUP;   // consecutive values per lane: the group covers 16 per round
  uint64_t lo = s, hi = s + n;    // the answer lies in [lo, hi]
  if (g.fence.levels == 0)   // small layers (view_for), or a pool too small for fences
    return lower_bound_group<GROUP>(g.ts_pool + s, n, x, lane, group_in_wave);
  if (n > 16) {
    int top = (31 - __clz(n - 1)) >> 2;   // coarsest level with 16^top < n
    if (top > static_cast<int>(g.fence.levels)) top = g.fence.levels;
    for (int l = top; l >= 1; --l) {
      const int shift = 4 * l;
      const float* __restrict__ F = g.fence.base + g.fence.off[l - 1];
      // fences whose position ((b + 1) << shift) - 1 lies in [lo, hi)
      uint64_t b_first = ((lo + (1ull << shift)) >> shift) - 1;
      const uint64_t b_end = hi >> shift;   // one past the last
      while (b_first < b_end) {              // at most two rounds per level
        // aligned window of 16 fences (the levels are padded: the whole window is readable)
        const uint64_t w0 = b_first & ~3ull;
        const float* __restrict__ src = F + w0 + static_cast<uint64_t>(lane) * V;
        float val[V];
        if (V == 4) {
          const float4 f = *reinterpret_cast<const float4*>(src);
          val[0] = f.x; val[1 % V] = f.y; val[2 % V] = f.z; val[3 % V] = f.w;
        } else if (V == 2) {
          const float2 f = *reinterpret_cast<const float2*>(src);
          val[0] = f.x; val[1 % V] = f.y;
        } else {
#pragma unroll
          for (int v = 0; v < V; ++v) val[v] = src[v];
        }
        uint32_t mine = 0;
#pragma unroll
        for (int v = 0; v < V; ++v) {
          const uint64_t b = w0 + static_cast<uint64_t>(lane) * V + v;
          mine += (b >= b_first && b < b_end && val[v] < x) ? 1u : 0u;
        }
        // sum over the group's lanes
        uint32_t less = mine;
#pragma unroll
        for (int d = 1; d < GROUP; d <<= 1) less += __shfl_xor(less, d, 64);
        const uint64_t seen = min(b_end, w0 + 16) - b_first;   // pivots looked at
        if (less < seen) {   // the (less)-th pivot is the first one >= x
          hi = ((b_first + less + 1) << shift) - 1;
          if (less) lo = (b_first + less) << shift;
          break;
        }
        lo = (b_first + seen) << shift;   // all of them < x
        b_first += seen;
      }
    }
  }
  // the remaining gap (<= 16 elements below a level-1 fence; a whole small segment): 16
  // consecutive timestamps per round
  const float* __restrict__ ts = g.ts_pool;
  for (;;) {
    uint32_t mine = 0;
#pragma unroll
    for (int v = 0; v < V; ++v) {
      const uint64_t p = lo + static_cast<uint64_t>(lane) * V + v;
      mine += (p < hi && ts[p] < x) ? 1u : 0u;
    }
    uint32_t less = mine;
#pragma unroll
    for (int d = 1; d < GROUP; d <<= 1) less += __shfl_xor(less, d, 64);
    const uint64_t m = min<uint64_t>(hi - lo, 16);
    if (less < m || lo + 16 >= hi) return static_cast<uint32_t>(lo + less - s);
    lo += 16;
  }
}

// The window [start, end) of one root on its node's segment, with the two shortcuts the node
// entry allows (edge_store.hpp): `end` later than the node's newest edge -> hi = size; a window
// that starts at 0 on a graph without negative timestamps -> lo = 0.  Otherwise the searches.
template <int GROUP>
__device__ inline void window_bounds(const GraphView& g, const NodeEntry& e, float start, float end,
                                     int lane, int group_in_wave, uint32_t* lo_out,
                                     uint32_t* hi_out) {
  uint32_t hi;
  if (end > __uint_as_float(e.last_ts_bits)) hi = e.size;
  else hi = lower_bound_fenced<GROUP>(g, e.start, e.size, end, lane, group_in_wave);
  uint32_t lo = 0;
  if (!(g.nonneg_ts > 0 && start <= 0.0f) && hi > 0) {
    const float first = g.ts_pool[e.start];
    if (start > first) lo = lower_bound_fenced<GROUP>(g, e.start, hi, start, lane, group_in_wave);
  }
  *lo_out = lo;
  *hi_out = hi;
}

__device__ inline uint32_t valid_slots(uint32_t n_cand, uint32_t fanout, int uniform) {
  // recent: slot j valid iff j < #candidates (sampling_kernels.cu:88-104);
  // uniform: every slot valid iff there is a candidate (:202, with replacement)
  if (uniform) return n_cand ? fanout : 0u;
  return n_cand < fanout ? n_cand : fanout;
}

// Size read-back without a memcpy + event wait: the last kernel of a sample() copies the
// per-block {R, S} words into pinned host memory and then stores the call's sequence
// number; the host spins on that word (hipEventSynchronize wakes up 10-20 us late).
struct Publish {
  const uint64_t* d_counts;   // device counts array (all blocks of this sample)
  uint64_t* h_counts;         // pinned host mirror (device-mapped)
  uint64_t* h_flag;           // pinned host sequence word
  uint64_t seq;
  uint32_t num_words;         // 0 = nothing to publish
  const uint32_t* d_extra = nullptr;   // one more word behind the counts (slot overflow), or null
};
struct PublishGroup { Publish p[4]; };

// Decoupled look-back of the one-launch kernels: the sum of the counts that the `n_before`
// workgroups before this one published as granules {tag | count} (count in the bits of `mask`).
// Every thread polls up to kLookBatch granules PER ROUND TRIP — all loads of a batch are issued
// before the first is looked at (polled one after the other, a thread's 3-5 granules cost 3-5
// dependent agent-scope loads) — and a granule that has not
// shown the tag after kGranuleSpins rounds is recomputed by `recount(b)` (termination does not
// depend on dispatch order).  Returns this THREAD's partial sum; `recounts` counts fallbacks.
constexpr int kLookBatch = 8;
template <int kBlock, typename Recount>
__device__ inline uint32_t lookback_partial(const uint64_t* granules, uint32_t n_before,
                                            uint64_t tag, uint64_t mask, unsigned int* recounts,
                                            Recount recount) {
  uint32_t part = 0;
  for (uint32_t base = 0; base < n_before; base += kLookBatch * kBlock) {   // uniform trip count
    uint64_t gr[kLookBatch];
    bool need[kLookBatch];
    bool any = false;
#pragma unroll
    for (int k = 0; k < kLookBatch; ++k) {
      need[k] = base + k * kBlock + threadIdx.x < n_before;
      any |= need[k];
    }
    for (uint32_t spins = 0; any && spins < kGranuleSpins; ++spins) {
#pragma unroll
      for (int k = 0; k < kLookBatch; ++k)
        gr[k] = need[k] ? __hip_atomic_load(&granules[base + k * kBlock + threadIdx.x],
                                            __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                        : 0ull;
      any = false;
#pragma unroll
      for (int k = 0; k < kLookBatch; ++k) {
        if (!need[k]) continue;
        if ((gr[k] & ~mask) == tag) {
          part += static_cast<uint32_t>(gr[k] & mask);
          need[k] = false;
        } else {
          any = true;
        }
      }
      if (any) __builtin_amdgcn_s_sleep(1);
    }
#pragma unroll
    for (int k = 0; k < kLookBatch; ++k) {
      if (need[k]) {
        part += recount(base + k * kBlock + threadIdx.x);
        atomicAdd(recounts, 1u);
      }
    }
  }
  return part;
}

// ---- partitioned sampling: fixed-slot replies and their merge ---------
__device__ inline int64_t pack_f32_pair(float lo, float hi) {
  return static_cast<int64_t>(static_cast<uint64_t>(__float_as_uint(lo)) |
                              (static_cast<uint64_t>(__float_as_uint(hi)) << 32));
}

// Search + select in ONE launch: with `fanout` fixed slots per root there is no compaction,
// hence no prefix sum between the two.  Same window / candidate / selection rules as
// sample_search_kernel + sample_emit_kernel; the Philox counter is the slot index.
struct PaddedCommon {
  uint32_t snapshot_idx, num_snapshots;
  float window;
  uint32_t fanout;
  int uniform, prop_time;
  uint64_t seed;
  // reply slots of 12 B {dst, eid, edge time as u32 / u32 / f32 bits; dst 0xFFFFFFFF = empty}
  // instead of 24 B {dst, eid, (out time, dt)}: the shared chains of graphs whose node and edge
  // ids fit 32 bits (half the bytes on the wire; dt and the out time are recomputed from the
  // root's time by the merge)
  int narrow = 0;
};
struct PaddedJob {
  const int64_t* req;
  uint64_t n;
  uint64_t call;             // Philox call counter of this job
  int64_t* out;
  const uint64_t* d_own;
  const uint64_t* d_total;
  uint64_t total_host;
  const uint32_t* root_of;
  uint32_t* rec_cnt;
  uint32_t stride, world;
  uint32_t* d_overflow;
  // several samples sharing one exchange (sample_partitioned_group): an own share starts at row
  // own_skip (0: world * stride); the inbox holds `world` = P x m slots, slot v belongs to
  // sample v % m and raises THAT sample's word d_overflow_of[v % m] (m = 0: d_overflow)
  uint64_t own_skip = 0;
  uint32_t m = 0;
  uint32_t* d_overflow_of[4] = {nullptr, nullptr, nullptr, nullptr};
  uint32_t* row_cnt = nullptr;   // inbox job, compact replies: valid slots of every served row
};

struct PaddedJobs { PaddedJob j[5]; };

struct MergeJob {
  const int64_t* roots;
  const float* root_ts;
  const uint64_t* d_R;
  uint64_t R_host;
  const int64_t* rep;        // the (shared) reply buffer
  const uint32_t* pos;
  uint32_t slot_rows;        // rows of the buffer that belong to slots (P x m x stride)
  uint64_t* granules;
  uint64_t tag;
  uint32_t* d_overflow;
  int64_t* all_nodes; float* all_ts; float* dt; int64_t* eids; int64_t* row; int64_t* col;
  uint64_t* out_R; uint64_t* out_S; uint64_t* next_R;
  // compact replies (null: the slots' rows are fixed-fanout rows of `rep` like the own share's):
  // the received slots, cslot bytes each — u32 [0] edges of the slot, [r] edges before row r,
  // [stride] the sender's overflow word, then the edges, edge_cap at most
  const char* crep = nullptr;
  uint32_t cslot = 0, edge_cap = 0, m = 1, jidx = 0, off_bytes = 4;
  // reuse of the previous layer (roots whose pos[] is kPosReused): root r < R_prev of this
  // layer IS root r of the previous one, same timestamp, and its edges are entries
  // [first_prev[r], first_prev[r + 1]) of the previous block; first_out[r] = this block's first
  // edge of root r (R + 1 entries), for the next layer
  const uint32_t* first_prev = nullptr;
  const uint64_t* d_R_prev = nullptr;
  uint64_t R_prev_host = 0;
  const int64_t* nodes_prev = nullptr; const float* ts_prev = nullptr;
  const float* dt_prev = nullptr; const int64_t* eids_prev = nullptr;
  uint32_t* first_out = nullptr;
};
struct MergeReuse {
  const uint32_t* first_prev; uint64_t R_prev;
  const int64_t* nodes_prev; const float* ts_prev; const float* dt_prev; const int64_t* eids_prev;
  uint32_t* first_out;
};
struct MergeJobs { MergeJob j[4]; };

struct CompactArgs {
  const int64_t* inbox;
  const void* served;
  const uint32_t* row_cnt;
  char* cserved;
  // [m] {launch tag, overflow count << 16 | slots done}: a word that carries another launch's tag
  // (a chain abandoned half-way, whatever the reason) starts over — nothing relies on a reset
  unsigned long long* ticket;
  uint32_t stride, fanout, m, world, edge_cap, cslot, narrow, off_bytes, tag;
};

inline unsigned capped_grid(uint64_t work_items, unsigned per_block, unsigned cap) {
  uint64_t g = (work_items + per_block - 1) / per_block;
  if (g < 1) g = 1;
  return static_cast<unsigned>(std::min<uint64_t>(g, cap));
}

// The fences pay where a layer is bound by memory traffic (large layers: one line per round
// instead of GROUP sectors; config 3, batch 300 k: search 538 -> 516 us).  A small layer is a
// pure latency chain with the same number of rounds either way, and the fenced search's extra
// address arithmetic made it slower (REDDIT-shaped batch 600: 6.0 -> 7.7 us per launch): small
// layers search the timestamps directly.
inline GraphView view_for(const EdgeStore* g, size_t roots) {
  GraphView v = g->view();
  if (roots <= kSmallRoots) v.fence.levels = 0;
  return v;
}

// ---- the launchers that cross units ----------------------------------------------------
// sample_layer.hip
int group_width_from_env(const char* name, int fallback);
void launch_scan(const uint32_t* rec_cnt, uint32_t* base, uint32_t* tile_scratch,
                 const uint64_t* d_R, uint64_t R_host, size_t Rb, uint32_t F, int uniform,
                 uint64_t* out_R, uint64_t* out_S, uint64_t* next_R, hipStream_t stream);
void launch_publish(const Publish& p, hipStream_t stream);
void launch_publish_group(const PublishGroup& g, int m, hipStream_t stream);
// sample_padded.hip
void launch_padded_group(int width, unsigned grid, int jobs_n, hipStream_t stream,
                         const GraphView& g, const PaddedCommon& c, const PaddedJobs& jobs);
// sample_merge.hip
void launch_merge_fused_group(const MergeJobs& jobs, unsigned grid, int m, uint32_t fanout,
                              uint32_t stride, int narrow, hipStream_t stream);
void launch_reply_compact(const CompactArgs& a, unsigned grid, hipStream_t stream);
uint64_t next_merge_tag();
// sampler.hip: adds to the per-stage host time of the issuing thread (part_host_us)
void part_host_add(int stage, uint64_t v);

}  // namespace gf
