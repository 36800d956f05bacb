// The three launches of one (layer, snapshot), all device resident (sampler.hip has the whole
// story): search resolves every root's time window once, scan turns the per-root valid-slot
// counts into each root's base in the compacted output and the layer's edge count, emit writes
// the MFG arrays at base[root] + slot.  Sampler::enqueue_layer issues them; the publish kernels
// hand a sample's block sizes to the host.
#include "sampler_ctx.hpp"

#include <cstdlib>

#include "../../include/gnnflow_rng.h"

namespace gf {

namespace {

// Stream-ordered after the last emit kernel, so every output of the sample is complete
// (and released by the kernel boundary) before the host can observe the sequence word.
__global__ void sample_publish_kernel(Publish p) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  for (uint32_t i = 0; i < p.num_words; ++i) p.h_counts[i] = p.d_counts[i];
  p.h_counts[p.num_words] = p.d_extra ? *p.d_extra : 0;
  __threadfence_system();
  *reinterpret_cast<volatile uint64_t*>(p.h_flag) = p.seq;
}

__global__ void sample_publish_group_kernel(PublishGroup g) {
  if (threadIdx.x != 0) return;
  const Publish& p = g.p[blockIdx.x];
  for (uint32_t i = 0; i < p.num_words; ++i) p.h_counts[i] = p.d_counts[i];
  p.h_counts[p.num_words] = p.d_extra ? *p.d_extra : 0;
  __threadfence_system();
  *reinterpret_cast<volatile uint64_t*>(p.h_flag) = p.seq;
}

// ---- 1. search --------------------------------------------------------------------
template <int GROUP>
__global__ __launch_bounds__(kSearchThreads) void sample_search_kernel(
    GraphView g, const int64_t* __restrict__ roots, const float* __restrict__ root_ts,
    const uint64_t* __restrict__ d_R, uint64_t R_host, uint32_t snapshot_idx,
    uint32_t num_snapshots, float window, uint64_t* __restrict__ rec_end,
    uint32_t* __restrict__ rec_cnt, uint32_t fanout, int uniform,
    uint32_t* __restrict__ wg_sum, const uint32_t* __restrict__ list,
    const uint32_t* __restrict__ seg_count, uint32_t num_segs, uint32_t seg_cap) {
  __shared__ uint32_t s_sum;
  __shared__ uint32_t seg_prefix[kMaxHubSegs + 1];
  if (wg_sum && threadIdx.x == 0) s_sum = 0;
  if (wg_sum) __syncthreads();
  // list != null: only the hubs the lane-per-root pass of a large layer left over — segment
  // s of the worklist holds seg_count[s] root indices at list[s * seg_cap ...]; every
  // workgroup builds the exclusive prefix of the counts (<= kMaxHubSegs words) in LDS and
  // finds the segment of its i-th hub by binary search, so the hubs are spread evenly over
  // the groups wherever they sat in the batch.
  uint64_t R = d_R ? *d_R : R_host;
  if (list) {
    __shared__ uint32_t wtot[kSearchThreads / 64];
    uint32_t carry = 0;
    for (uint32_t s0 = 0; s0 < num_segs; s0 += kSearchThreads) {   // uniform trip count
      const uint32_t sidx = s0 + threadIdx.x;
      const uint32_t v = sidx < num_segs ? seg_count[sidx] : 0u;
      uint32_t incl = v;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const uint32_t up = __shfl_up(incl, d, 64);
        if ((threadIdx.x & 63) >= d) incl += up;
      }
      __syncthreads();
      if ((threadIdx.x & 63) == 63) wtot[threadIdx.x >> 6] = incl;
      __syncthreads();
      uint32_t wbase = 0, tot = 0;
      for (int w = 0; w < kSearchThreads / 64; ++w) {
        if (w < (threadIdx.x >> 6)) wbase += wtot[w];
        tot += wtot[w];
      }
      if (sidx < num_segs) seg_prefix[sidx] = carry + wbase + incl - v;
      carry += tot;
    }
    if (threadIdx.x == 0) seg_prefix[num_segs] = carry;
    __syncthreads();
    R = seg_prefix[num_segs];
  }
  constexpr int kGroupsPerBlock = kSearchThreads / GROUP;
  const int lane = threadIdx.x % GROUP;
  const int group_in_wave = (threadIdx.x % 64) / GROUP;
  const uint64_t group = static_cast<uint64_t>(blockIdx.x) * kGroupsPerBlock + threadIdx.x / GROUP;
  const uint64_t num_groups = static_cast<uint64_t>(gridDim.x) * kGroupsPerBlock;
  for (uint64_t i = group; i < R; i += num_groups) {
    uint64_t r = i;
    if (list) {   // largest segment s with seg_prefix[s] <= i
      uint32_t lo_s = 0, hi_s = num_segs;
      while (hi_s - lo_s > 1) {
        const uint32_t mid = (lo_s + hi_s) >> 1;
        if (seg_prefix[mid] <= i) lo_s = mid; else hi_s = mid;
      }
      r = list[static_cast<uint64_t>(lo_s) * seg_cap + (i - seg_prefix[lo_s])];
    }
    const int64_t nid = roots[r];
    const float t = root_ts[r];
    float start, end;
    time_window(t, snapshot_idx, num_snapshots, window, &start, &end);
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
    if (lane == 0) {
      rec_end[r] = end_off;
      rec_cnt[r] = n_cand;
      if (wg_sum) atomicAdd(&s_sum, valid_slots(n_cand, fanout, uniform));
    }
  }
  // small-batch path: the grid covers every root exactly once (no striding), so
  // workgroup b owns roots [b*kGroupsPerBlock, (b+1)*kGroupsPerBlock) and publishes
  // their valid-slot total for the emit kernel's prefix
  if (wg_sum) {
    __syncthreads();
    if (threadIdx.x == 0) wg_sum[blockIdx.x] = s_sum;
  }
}

// ---- 1b. search for large layers: lane per root, then groups for the hubs ----------------
// A 16-lane group per root keeps only 4 roots per wave in flight, and a root is a chain of
// 2-7 dependent random reads (table entry -> pivots ...): at 10^5-10^7 roots per layer the
// kernel is bound by that latency, not by HBM (measured on the 10 M-node / 200 M-edge graph:
// 32 G random reads/s against > 100 G/s in the emit kernel).  On a power-law graph > 90 % of
// the roots have at most one 64-byte line of timestamps, so a first pass gives every LANE a
// root (64 table entries in flight per wave) and resolves it on the spot if its segment has
// <= kLaneDeg timestamps (all loads independent: one more round trip); the roots with longer
// segments are appended to the workgroup's own segment of a worklist (an LDS counter: one
// global atomic per wave on a shared counter would serialise at ~88 per microsecond) that a
// second launch of the cooperative k-ary search works off, evenly spread over its groups
// whatever their position in the batch.
constexpr uint32_t kLaneDeg = 16;

__global__ __launch_bounds__(kSearchThreads) void sample_search_lanes_kernel(
    GraphView g, const int64_t* __restrict__ roots, const float* __restrict__ root_ts,
    const uint64_t* __restrict__ d_R, uint64_t R_host, uint32_t snapshot_idx,
    uint32_t num_snapshots, float window, uint64_t* __restrict__ rec_end,
    uint32_t* __restrict__ rec_cnt, uint32_t* __restrict__ hub_list,
    uint32_t* __restrict__ seg_count, uint32_t seg_cap) {
  __shared__ uint32_t s_seg_n;
  if (threadIdx.x == 0) s_seg_n = 0;
  __syncthreads();
  uint32_t* seg = hub_list + static_cast<uint64_t>(blockIdx.x) * seg_cap;
  const uint64_t R = d_R ? *d_R : R_host;
  const int lane = threadIdx.x & 63;
  const uint64_t wave = (static_cast<uint64_t>(blockIdx.x) * kSearchThreads + threadIdx.x) >> 6;
  const uint64_t num_waves = (static_cast<uint64_t>(gridDim.x) * kSearchThreads) >> 6;
  const uint64_t chunks = (R + 63) / 64;
  for (uint64_t chunk = wave; chunk < chunks; chunk += num_waves) {   // wave-uniform trip count
    const uint64_t r = chunk * 64 + lane;
    const bool in = r < R;
    int64_t nid = -1;
    float start = 0.f, end = 0.f;
    if (in) {
      nid = roots[r];
      time_window(root_ts[r], snapshot_idx, num_snapshots, window, &start, &end);
    }
    NodeEntry e;
    e.start = 0;
    e.size = 0;
    if (in && nid >= 0 && static_cast<uint64_t>(nid) < g.table_len) e = g.table[nid];
    // newest edge older than the window's end and the window open at 0: nothing to read
    const bool whole = g.nonneg_ts > 0 && start <= 0.0f && e.size > 0 &&
                       end > __uint_as_float(e.last_ts_bits);
    const bool big = e.size > kLaneDeg && !whole;
    if (in && whole) {
      rec_end[r] = e.start + e.size;
      rec_cnt[r] = e.size;
    } else if (in && !big) {
      uint32_t hi = 0, lo = 0;
      if (e.size > 0) {
        const float* ts = g.ts_pool + e.start;
        float v[kLaneDeg];
        if ((e.start & 3u) == 0) {
          // 16-byte loads (segments start 64-byte aligned unless a prefix was offloaded):
          // a quarter of the L2 requests of the scalar form, which bound this pass
          const float4* t4 = reinterpret_cast<const float4*>(ts);
#pragma unroll
          for (uint32_t q = 0; q < kLaneDeg / 4; ++q) {
            const float4 x = 4 * q < e.size ? t4[q] : make_float4(0.f, 0.f, 0.f, 0.f);
            v[4 * q] = x.x; v[4 * q + 1] = x.y; v[4 * q + 2] = x.z; v[4 * q + 3] = x.w;
          }
        } else {
#pragma unroll
          for (uint32_t i = 0; i < kLaneDeg; ++i) v[i] = i < e.size ? ts[i] : 0.f;   // independent
        }
#pragma unroll
        for (uint32_t i = 0; i < kLaneDeg; ++i) {
          hi += (i < e.size && v[i] < end) ? 1u : 0u;
          lo += (i < e.size && v[i] < start) ? 1u : 0u;
        }
      }
      rec_end[r] = e.start + hi;
      rec_cnt[r] = hi > lo ? hi - lo : 0;
    }
    const unsigned long long hubs = __ballot(big);
    if (hubs) {   // append to this workgroup's segment: LDS counter, no global atomic
      uint32_t at = 0;
      if (lane == 0) at = atomicAdd(&s_seg_n, static_cast<uint32_t>(__popcll(hubs)));
      at = __shfl(at, 0, 64);
      if (big) seg[at + __popcll(hubs & ((1ull << lane) - 1ull))] = static_cast<uint32_t>(r);
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) seg_count[blockIdx.x] = s_seg_n;
}

// ---- 2. scan -----------------------------------------------------------------------
__global__ __launch_bounds__(kScanThreads) void sample_scan_kernel(
    const uint32_t* __restrict__ rec_cnt, uint32_t* __restrict__ base,
    const uint64_t* d_R, uint64_t R_host, uint32_t fanout, int uniform, uint64_t* out_R,
    uint64_t* out_S, uint64_t* next_R) {
  __shared__ uint32_t wave_sums[kScanThreads / 64];
  __shared__ uint32_t carry_s;
  const uint64_t R = d_R ? *d_R : R_host;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid == 0) carry_s = 0;
  __syncthreads();
  constexpr uint64_t kTile = static_cast<uint64_t>(kScanThreads) * kScanItems;
  for (uint64_t tile = 0; tile < R; tile += kTile) {
    uint32_t v[kScanItems];
    uint32_t local = 0;
    const uint64_t i0 = tile + static_cast<uint64_t>(tid) * kScanItems;
#pragma unroll
    for (int k = 0; k < kScanItems; ++k) {
      v[k] = (i0 + k < R) ? valid_slots(rec_cnt[i0 + k], fanout, uniform) : 0u;
      local += v[k];
    }
    // inclusive scan of `local` across the wave
    uint32_t incl = local;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      uint32_t up = __shfl_up(incl, d, 64);
      if (lane >= d) incl += up;
    }
    if (lane == 63) wave_sums[wave] = incl;
    __syncthreads();
    uint32_t wave_base = 0;
    for (int w = 0; w < wave; ++w) wave_base += wave_sums[w];
    uint32_t run = carry_s + wave_base + incl - local;
#pragma unroll
    for (int k = 0; k < kScanItems; ++k) {
      if (i0 + k < R) base[i0 + k] = run;
      run += v[k];
    }
    __syncthreads();
    if (tid == kScanThreads - 1) carry_s = run;  // last thread's run = tile total + carry
    __syncthreads();
  }
  if (tid == 0) {
    const uint64_t S = carry_s;
    *out_R = R;
    *out_S = S;
    if (next_R) *next_R = R + S;
  }
}

// ---- 2b. parallel scan for large layers --------------------------------------------
// tile = kScanTile roots.  (a) per-tile sums, (b) one workgroup scans the tile sums and
// publishes S / R', (c) every tile scans itself and adds its base.

__global__ __launch_bounds__(kScanThreads) void sample_tile_sum_kernel(
    const uint32_t* __restrict__ rec_cnt, const uint64_t* d_R, uint64_t R_host,
    uint32_t fanout, int uniform, uint32_t* __restrict__ tile_sum) {
  __shared__ uint32_t red[kScanThreads / 64];
  const uint64_t R = d_R ? *d_R : R_host;
  const uint64_t tiles = (R + kScanTile - 1) / kScanTile;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    uint32_t local = 0;
    const uint64_t i0 = tile * kScanTile + static_cast<uint64_t>(tid) * kScanItems;
#pragma unroll
    for (int k = 0; k < kScanItems; ++k)
      if (i0 + k < R) local += valid_slots(rec_cnt[i0 + k], fanout, uniform);
    for (int d = 32; d > 0; d >>= 1) local += __shfl_down(local, d, 64);
    if (lane == 0) red[wave] = local;
    __syncthreads();
    if (tid == 0) {
      uint32_t t = 0;
      for (int w = 0; w < kScanThreads / 64; ++w) t += red[w];
      tile_sum[tile] = t;
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(kScanThreads) void sample_tile_scan_kernel(
    const uint32_t* __restrict__ tile_sum, uint32_t* __restrict__ tile_base,
    const uint64_t* d_R, uint64_t R_host, uint64_t* out_R, uint64_t* out_S, uint64_t* next_R) {
  __shared__ uint32_t wave_sums[kScanThreads / 64];
  __shared__ uint32_t carry_s;
  const uint64_t R = d_R ? *d_R : R_host;
  const uint64_t tiles = (R + kScanTile - 1) / kScanTile;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid == 0) carry_s = 0;
  __syncthreads();
  for (uint64_t t0 = 0; t0 < tiles; t0 += kScanThreads) {
    const uint64_t i = t0 + tid;
    const uint32_t v = i < tiles ? tile_sum[i] : 0u;
    uint32_t incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      uint32_t up = __shfl_up(incl, d, 64);
      if (lane >= d) incl += up;
    }
    if (lane == 63) wave_sums[wave] = incl;
    __syncthreads();
    uint32_t wave_base = 0;
    for (int w = 0; w < wave; ++w) wave_base += wave_sums[w];
    const uint32_t excl = carry_s + wave_base + incl - v;
    if (i < tiles) tile_base[i] = excl;
    __syncthreads();
    if (tid == kScanThreads - 1) carry_s = excl + v;
    __syncthreads();
  }
  if (tid == 0) {
    const uint64_t S = carry_s;
    *out_R = R;
    *out_S = S;
    if (next_R) *next_R = R + S;
  }
}

__global__ __launch_bounds__(kScanThreads) void sample_tile_apply_kernel(
    const uint32_t* __restrict__ rec_cnt, const uint32_t* __restrict__ tile_base,
    const uint64_t* d_R, uint64_t R_host, uint32_t fanout, int uniform,
    uint32_t* __restrict__ base) {
  __shared__ uint32_t wave_sums[kScanThreads / 64];
  const uint64_t R = d_R ? *d_R : R_host;
  const uint64_t tiles = (R + kScanTile - 1) / kScanTile;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    uint32_t v[kScanItems], local = 0;
    const uint64_t i0 = tile * kScanTile + static_cast<uint64_t>(tid) * kScanItems;
#pragma unroll
    for (int k = 0; k < kScanItems; ++k) {
      v[k] = (i0 + k < R) ? valid_slots(rec_cnt[i0 + k], fanout, uniform) : 0u;
      local += v[k];
    }
    uint32_t incl = local;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      uint32_t up = __shfl_up(incl, d, 64);
      if (lane >= d) incl += up;
    }
    if (lane == 63) wave_sums[wave] = incl;
    __syncthreads();
    uint32_t wave_base = 0;
    for (int w = 0; w < wave; ++w) wave_base += wave_sums[w];
    uint32_t run = tile_base[tile] + wave_base + incl - local;
#pragma unroll
    for (int k = 0; k < kScanItems; ++k) {
      if (i0 + k < R) base[i0 + k] = run;
      run += v[k];
    }
    __syncthreads();
  }
}

// ---- 3. emit -----------------------------------------------------------------------
__global__ __launch_bounds__(kEmitThreads) void sample_emit_kernel(
    GraphView g, const int64_t* __restrict__ roots, const float* __restrict__ root_ts,
    const uint64_t* __restrict__ d_R, uint64_t R_host, uint32_t fanout, int uniform,
    int prop_time, uint64_t seed, uint64_t call, const uint64_t* __restrict__ rec_end,
    const uint32_t* __restrict__ rec_cnt, const uint32_t* __restrict__ base,
    int64_t* __restrict__ all_nodes, float* __restrict__ all_ts, float* __restrict__ dt,
    int64_t* __restrict__ eids, int64_t* __restrict__ row, int64_t* __restrict__ col,
    Publish pub) {
  const uint64_t R = d_R ? *d_R : R_host;
  const uint64_t total = R * fanout;
  if (pub.num_words && blockIdx.x == 0 && threadIdx.x == 0) {   // sizes: final before this launch
    for (uint32_t i = 0; i < pub.num_words; ++i) pub.h_counts[i] = pub.d_counts[i];
    pub.h_counts[pub.num_words] = 0;
  }
  // Four slots per thread and trip, every load of a stage issued before the first use: a
  // sampled edge is ONE random 32-byte record, and what bounds this kernel at large batches is
  // how many of those reads are in flight (HBM's random-access rate), not bytes.  One slot per
  // trip left each wave with a single record read outstanding between two dependent hops
  // (count / end -> record -> stores).
  const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
  const uint64_t first = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  constexpr int K = 4;
  for (uint64_t t0 = first; t0 < total; t0 += K * stride) {
    uint64_t t[K], r[K], end[K];
    uint32_t j[K], n[K], bs[K];
    float rts[K];
    bool in[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      t[k] = t0 + static_cast<uint64_t>(k) * stride;
      in[k] = t[k] < total;
      r[k] = in[k] ? t[k] / fanout : 0;
      j[k] = static_cast<uint32_t>(t[k] - r[k] * fanout);
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
      n[k] = in[k] ? rec_cnt[r[k]] : 0u;
      end[k] = in[k] ? rec_end[r[k]] : 0;
      bs[k] = in[k] ? base[r[k]] : 0u;
      rts[k] = in[k] ? root_ts[r[k]] : 0.f;
      if (in[k] && t[k] < R) {  // dst nodes come first in all_nodes / all_timestamps
        all_nodes[t[k]] = roots[t[k]];
        all_ts[t[k]] = root_ts[t[k]];
      }
    }
    EdgePair nb[K];
    bool ok[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      ok[k] = in[k] && j[k] < valid_slots(n[k], fanout, uniform);
      if (ok[k]) {
        const uint32_t pick = uniform ? gf_philox4x32_10_first(seed, t[k], call) % n[k] : j[k];
        nb[k] = g.nbr_pool[end[k] - 1 - pick];
      }
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
      if (!ok[k]) continue;
      const float ets = nb[k].ts;
      const uint64_t o = static_cast<uint64_t>(bs[k]) + j[k];
      all_nodes[R + o] = nb[k].dst;
      all_ts[R + o] = prop_time ? rts[k] : ets;
      dt[o] = rts[k] - ets;
      eids[o] = nb[k].eid;
      row[o] = static_cast<int64_t>(r[k]);
      col[o] = static_cast<int64_t>(R + o);
    }
  }
}

// ---- 2+3 fused (small batches): emit with an in-kernel prefix -----------------------
// For layers with at most kSmallRoots roots the separate scan launch is dropped: every
// emit workgroup derives the compacted base of its first root from the search kernel's
// per-workgroup sums (a few hundred to a few thousand L2-resident words), scans its own
// <= 256 roots in LDS, and the workgroup owning the last slot publishes S and R' = R + S.
__global__ __launch_bounds__(kEmitThreads) void sample_emit_prefix_kernel(
    GraphView g, const int64_t* __restrict__ roots, const float* __restrict__ root_ts,
    const uint64_t* d_R, uint64_t R_host, uint32_t fanout, int uniform, int prop_time,
    uint64_t seed, uint64_t call, const uint64_t* __restrict__ rec_end,
    const uint32_t* __restrict__ rec_cnt, const uint32_t* __restrict__ wg_sum,
    uint32_t roots_per_search_wg, int64_t* __restrict__ all_nodes, float* __restrict__ all_ts,
    float* __restrict__ dt, int64_t* __restrict__ eids, int64_t* __restrict__ row,
    int64_t* __restrict__ col, uint64_t* out_R, uint64_t* out_S, uint64_t* next_R, Publish pub) {
  __shared__ uint32_t red[kEmitThreads / 64];
  __shared__ uint32_t lbase[kEmitThreads];
  __shared__ uint32_t wave_tot[kEmitThreads / 64];
  const uint64_t R = d_R ? *d_R : R_host;
  const uint64_t total = R * fanout;
  const uint64_t t0 = static_cast<uint64_t>(blockIdx.x) * kEmitThreads;
  if (t0 >= total) return;   // uniform for the workgroup
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint64_t t_last = min(t0 + kEmitThreads - 1, total - 1);
  const uint32_t r_first = static_cast<uint32_t>(t0 / fanout);
  const uint32_t r_last = static_cast<uint32_t>(t_last / fanout);
  const uint32_t nroots = r_last - r_first + 1;   // <= kEmitThreads
  // 1. base of r_first = search-workgroup sums before it + the remainder inside its group
  const uint32_t b_first = r_first / roots_per_search_wg;
  uint32_t part = 0;
  for (uint32_t b = tid; b < b_first; b += kEmitThreads) part += wg_sum[b];
  for (uint32_t r = b_first * roots_per_search_wg + tid; r < r_first; r += kEmitThreads)
    part += valid_slots(rec_cnt[r], fanout, uniform);
  for (int d = 32; d > 0; d >>= 1) part += __shfl_down(part, d, 64);
  if (lane == 0) red[wave] = part;
  // 2. exclusive scan of this workgroup's own roots
  const uint32_t mine = tid < static_cast<int>(nroots)
                            ? valid_slots(rec_cnt[r_first + tid], fanout, uniform) : 0u;
  uint32_t incl = mine;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    uint32_t up = __shfl_up(incl, d, 64);
    if (lane >= d) incl += up;
  }
  if (lane == 63) wave_tot[wave] = incl;
  __syncthreads();
  uint32_t base = 0;
#pragma unroll
  for (int w = 0; w < kEmitThreads / 64; ++w) base += red[w];
  uint32_t wbase = 0;
  for (int w = 0; w < wave; ++w) wbase += wave_tot[w];
  lbase[tid] = base + wbase + incl - mine;
  __syncthreads();
  // 3. emit
  const uint64_t t = t0 + tid;
  if (t < total) {
    if (t < R) {
      all_nodes[t] = roots[t];
      all_ts[t] = root_ts[t];
    }
    const uint32_t r = static_cast<uint32_t>(t / fanout);
    const uint32_t j = static_cast<uint32_t>(t - static_cast<uint64_t>(r) * fanout);
    const uint32_t n = rec_cnt[r];
    if (j < valid_slots(n, fanout, uniform)) {
      const uint32_t pick = uniform ? gf_philox4x32_10_first(seed, t, call) % n : j;
      const uint64_t e = rec_end[r] - 1 - pick;
      const EdgePair nb = g.nbr_pool[e];
      const float ets = nb.ts;
      const float rts = root_ts[r];
      const uint64_t o = static_cast<uint64_t>(lbase[r - r_first]) + j;
      all_nodes[R + o] = nb.dst;
      all_ts[R + o] = prop_time ? rts : ets;
      dt[o] = rts - ets;
      eids[o] = nb.eid;
      row[o] = static_cast<int64_t>(r);
      col[o] = static_cast<int64_t>(R + o);
    }
  }
  // 4. the workgroup that owns the last slot knows the layer's edge count
  if (t_last == total - 1 && tid == static_cast<int>(nroots) - 1) {
    const uint64_t S = static_cast<uint64_t>(lbase[tid]) + mine;
    *out_R = R;
    *out_S = S;
    if (next_R) *next_R = R + S;
    // the LAST kernel of a sample also copies every block's sizes into pinned host memory (the
    // earlier blocks' are final: their kernels are complete; this block's were just written by
    // this thread); the host learns of the sample's completion from the stream's event
    for (uint32_t i = 0; i < pub.num_words; ++i) pub.h_counts[i] = pub.d_counts[i];
    if (pub.num_words) pub.h_counts[pub.num_words] = 0;
  }
}

template <typename... Args>
void launch_search(int width, unsigned grid, hipStream_t stream, Args... args) {
  switch (width) {
    case 2: sample_search_kernel<2><<<dim3(grid), dim3(kSearchThreads), 0, stream>>>(args...); break;
    case 4: sample_search_kernel<4><<<dim3(grid), dim3(kSearchThreads), 0, stream>>>(args...); break;
    case 8: sample_search_kernel<8><<<dim3(grid), dim3(kSearchThreads), 0, stream>>>(args...); break;
    default: sample_search_kernel<16><<<dim3(grid), dim3(kSearchThreads), 0, stream>>>(args...); break;
  }
}

}  // namespace

// Lanes cooperating on one root in the search kernels.  A small layer (<= 32 768 roots,
// every root in flight at once) is a pure latency chain, so it wants FEW rounds: 16 lanes,
// log16(deg) + 1 dependent reads.  A large layer is bound by how many roots the resident
// waves keep in flight, so it wants NARROW groups: 4 lanes put 16 roots in flight per wave
// and issue 40 probes per 10^7-edge segment instead of 96 (measured on the 10 M-node /
// 200 M-edge graph, profiles/).  Read when a sampler is created so tests can compare widths.
int group_width_from_env(const char* name, int fallback) {
  const char* v = std::getenv(name);
  const int g = v ? std::atoi(v) : fallback;
  return (g == 2 || g == 4 || g == 8 || g == 16) ? g : fallback;
}

// The exclusive prefix sum of the valid-slot counts: one workgroup up to 65 536 roots, tiles
// beyond (tile_scratch: the tile sums and the tile bases, 2 * tiles <= ws_roots_ words).
void launch_scan(const uint32_t* rec_cnt, uint32_t* base, uint32_t* tile_scratch,
                 const uint64_t* d_R, uint64_t R_host, size_t Rb, uint32_t F, int uniform,
                 uint64_t* out_R, uint64_t* out_S, uint64_t* next_R, hipStream_t stream) {
  if (Rb <= 65536) {
    sample_scan_kernel<<<dim3(1), dim3(kScanThreads), 0, stream>>>(
        rec_cnt, base, d_R, R_host, F, uniform, out_R, out_S, next_R);
    return;
  }
  const size_t tiles = (Rb + kScanTile - 1) / kScanTile;
  uint32_t* tile_sum = tile_scratch;
  uint32_t* tile_base = tile_scratch + tiles;
  const unsigned grid = static_cast<unsigned>(std::min<size_t>(tiles, 2048));
  sample_tile_sum_kernel<<<dim3(grid), dim3(kScanThreads), 0, stream>>>(
      rec_cnt, d_R, R_host, F, uniform, tile_sum);
  sample_tile_scan_kernel<<<dim3(1), dim3(kScanThreads), 0, stream>>>(
      tile_sum, tile_base, d_R, R_host, out_R, out_S, next_R);
  sample_tile_apply_kernel<<<dim3(grid), dim3(kScanThreads), 0, stream>>>(
      rec_cnt, tile_base, d_R, R_host, F, uniform, base);
}

void launch_publish(const Publish& p, hipStream_t stream) {
  sample_publish_kernel<<<dim3(1), dim3(64), 0, stream>>>(p);
}
void launch_publish_group(const PublishGroup& g, int m, hipStream_t stream) {
  sample_publish_group_kernel<<<dim3(static_cast<unsigned>(m)), dim3(64), 0, stream>>>(g);
}

void Sampler::enqueue_layer(const int64_t* d_roots, const float* d_ts, size_t Rb,
                            const uint64_t* d_R, uint64_t R_host, uint32_t layer,
                            uint32_t snapshot, const BlockPtrs& out, uint64_t* d_counts_slot,
                            uint64_t* next_R, hipStream_t stream, const Publish& pub) {
  const uint32_t F = fanouts_[layer];
  const int uniform = policy_ == GF_SAMPLING_POLICY_UNIFORM;
  GF_REQUIRE(static_cast<uint64_t>(Rb) * F < 0xFFFFFFFFull,
             "sampler: more than 2^32-1 slots in one layer");
  char* w = ws_.as<char>();
  uint64_t* rec_end = reinterpret_cast<uint64_t*>(w); w += align_up(ws_roots_ * 8, 16);
  uint32_t* rec_cnt = reinterpret_cast<uint32_t*>(w); w += align_up(ws_roots_ * 4, 16);
  uint32_t* base = reinterpret_cast<uint32_t*>(w);    w += align_up(ws_roots_ * 4, 16);
  uint32_t* wg_sum = reinterpret_cast<uint32_t*>(w);
  const GraphView gv = view_for(graph_, Rb);
  const uint64_t call = calls_++;
  // small layers: search publishes per-workgroup sums and emit does its own prefix.  (Search +
  // prefix + emit in ONE launch through look-back granules was built and measured: 17 us per
  // layer against 6.5 + 6 us + a 1.5 us boundary — across XCDs a count reaches its readers
  // through memory, which a kernel boundary does for free; profiles/README, round 5.)
  const bool small = Rb <= kSmallRoots;
  const unsigned roots_per_wg = kSearchThreads / search_group_;
  {
    ProfileScope ps(kProfSearch, stream);
    const unsigned grid = small ? static_cast<unsigned>((Rb + roots_per_wg - 1) / roots_per_wg)
                                : capped_grid(Rb, roots_per_wg, 256 * 8);
    if (hybrid_search_ && Rb >= kLaneSearchRoots) {
      // worklist: segment w (of the lane pass's workgroup w) can hold every root that
      // workgroup looks at; seg_count lives in the tile scratch (wg_sum), unused until the scan.
      const unsigned lgrid = capped_grid(Rb, kSearchThreads, kMaxHubSegs);
      const uint64_t chunks_per_wg = ((Rb + 63) / 64 + (lgrid * 4ull) - 1) / (lgrid * 4ull);
      const uint32_t seg_cap = static_cast<uint32_t>(chunks_per_wg * 4 * 64);
      const size_t hub_bytes = static_cast<size_t>(seg_cap) * lgrid * sizeof(uint32_t);
      if (hub_bytes > hub_buf_.bytes()) {   // stream-ordered swap, as for the workspace
        DeviceBuffer fresh;
        fresh.reserve(hub_bytes, 0, stream);
        std::swap(hub_buf_, fresh);
        retired_.retire(std::move(fresh), stream);
      }
      uint32_t* hub_list_ = hub_buf_.as<uint32_t>();
      uint32_t* seg_count = wg_sum;
      sample_search_lanes_kernel<<<dim3(lgrid), dim3(kSearchThreads), 0, stream>>>(
          gv, d_roots, d_ts, d_R, R_host, snapshot, num_snapshots_, window_, rec_end, rec_cnt,
          hub_list_, seg_count, seg_cap);
      launch_search(large_group_, capped_grid(Rb / 4, kSearchThreads / large_group_, 256 * 8),
                    stream, gv, d_roots, d_ts, nullptr, 0, snapshot, num_snapshots_, window_,
                    rec_end, rec_cnt, F, uniform, nullptr, hub_list_, seg_count, lgrid, seg_cap);
    } else if (small) {
      launch_search(search_group_, grid, stream, gv, d_roots, d_ts, d_R, R_host, snapshot,
                    num_snapshots_, window_, rec_end, rec_cnt, F, uniform, wg_sum, nullptr,
                    nullptr, 0, 0);
    } else {
      launch_search(large_group_, capped_grid(Rb, kSearchThreads / large_group_, 256 * 8), stream,
                    gv, d_roots, d_ts, d_R, R_host, snapshot, num_snapshots_, window_, rec_end,
                    rec_cnt, F, uniform, nullptr, nullptr, nullptr, 0, 0);
    }
    GF_HIP(hipGetLastError());
  }
  if (small) {
    ProfileScope ps(kProfEmit, stream);
    const unsigned grid = static_cast<unsigned>(
        (static_cast<uint64_t>(Rb) * F + kEmitThreads - 1) / kEmitThreads);
    sample_emit_prefix_kernel<<<dim3(grid), dim3(kEmitThreads), 0, stream>>>(
        gv, d_roots, d_ts, d_R, R_host, F, uniform, prop_time_ ? 1 : 0, seed_, call, rec_end,
        rec_cnt, wg_sum, roots_per_wg, out.all_nodes, out.all_ts, out.dt, out.eids, out.row,
        out.col, d_counts_slot, d_counts_slot + 1, next_R, pub);
    GF_HIP(hipGetLastError());
    return;
  }
  {
    ProfileScope ps(kProfScan, stream);
    // wg_sum doubles as the tile-sum / tile-base scratch
    launch_scan(rec_cnt, base, wg_sum, d_R, R_host, Rb, F, uniform, d_counts_slot,
                d_counts_slot + 1, next_R, stream);
    GF_HIP(hipGetLastError());
  }
  {
    ProfileScope ps(kProfEmit, stream);
    unsigned grid = capped_grid(static_cast<uint64_t>(Rb) * F, kEmitThreads, 256 * 16);
    sample_emit_kernel<<<dim3(grid), dim3(kEmitThreads), 0, stream>>>(
        gv, d_roots, d_ts, d_R, R_host, F, uniform, prop_time_ ? 1 : 0, seed_, call, rec_end,
        rec_cnt, base, out.all_nodes, out.all_ts, out.dt, out.eids, out.row, out.col, pub);
    GF_HIP(hipGetLastError());
  }
}

// gf_philox4x32_10_first evaluated ON THE DEVICE for n (seed, slot, call) triples: the uniform
// sampler's draws share include/gnnflow_rng.h with the CPU oracle, so a device-side miscompile
// of the Philox rounds would not show in HIP-vs-oracle parity; the Random123 known-answer
// vectors evaluated here would (tests/test_gpu_sampler_parity.py).
__global__ void philox_debug_kernel(const uint64_t* __restrict__ in, size_t n,
                                    uint32_t* __restrict__ out) {
  const size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i < n) out[i] = gf_philox4x32_10_first(in[3 * i], in[3 * i + 1], in[3 * i + 2]);
}
void philox_on_device(const uint64_t* d_in, size_t n, uint32_t* d_out, hipStream_t stream) {
  if (n == 0) return;
  philox_debug_kernel<<<dim3(static_cast<unsigned>((n + 255) / 256)), dim3(256), 0, stream>>>(
      d_in, n, d_out);
  GF_HIP(hipGetLastError());
}

}  // namespace gf
