// The requester's half of partitioned sampling: the replies (fixed-slot rows in owner-sorted
// order, or compact slots) become the layer's block in the ORIGINAL root order, laid out like
// sample_layer's output — count / scan / emit, count + emit with its own prefix, or the whole
// merge in one launch through look-back granules.
#include "sampler_ctx.hpp"
#include "partition.hpp"

#include <atomic>
#include <cstring>

namespace gf {

namespace {

// valid slots of root i's reply row (a prefix of the row for both policies)
__global__ void merge_count_kernel(const int64_t* __restrict__ rep, const uint32_t* __restrict__ pos,
                                   const uint64_t* __restrict__ d_R, uint64_t R_host,
                                   uint32_t fanout, uint32_t* __restrict__ rec_cnt,
                                   uint32_t stride, uint32_t world) {
  const uint64_t R = d_R ? *d_R : R_host;
  const uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= R) return;
  const uint32_t p = pos[i];
  uint32_t c = 0;
  // slotted layout: a header row stands for a root that did not fit its owner's slot
  if (!(stride && p < world * stride && p % stride == 0)) {
    const int64_t* s = rep + static_cast<uint64_t>(p) * fanout * 3;
    for (uint32_t j = 0; j < fanout; ++j) c += s[3 * j] >= 0 ? 1u : 0u;
  }
  rec_cnt[i] = c;
}

__global__ __launch_bounds__(kEmitThreads) void merge_emit_kernel(
    const int64_t* __restrict__ roots, const float* __restrict__ root_ts,
    const uint64_t* __restrict__ d_R, uint64_t R_host,
    uint32_t fanout, const int64_t* __restrict__ rep, const uint32_t* __restrict__ pos,
    const uint32_t* __restrict__ rec_cnt, const uint32_t* __restrict__ base,
    int64_t* __restrict__ all_nodes, float* __restrict__ all_ts, float* __restrict__ dt,
    int64_t* __restrict__ eids, int64_t* __restrict__ row, int64_t* __restrict__ col) {
  const uint64_t R = d_R ? *d_R : R_host;
  const uint64_t total = R * fanout;
  const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
  for (uint64_t t = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; t < total;
       t += stride) {
    if (t < R) {
      all_nodes[t] = roots[t];
      all_ts[t] = root_ts[t];
    }
    const uint64_t r = t / fanout;
    const uint32_t j = static_cast<uint32_t>(t - r * fanout);
    if (j >= rec_cnt[r]) continue;
    const int64_t* s = rep + (static_cast<uint64_t>(pos[r]) * fanout + j) * 3;
    const uint64_t packed = static_cast<uint64_t>(s[2]);
    const uint64_t o = static_cast<uint64_t>(base[r]) + j;
    all_nodes[R + o] = s[0];
    all_ts[R + o] = __uint_as_float(static_cast<uint32_t>(packed));
    dt[o] = __uint_as_float(static_cast<uint32_t>(packed >> 32));
    eids[o] = s[1];
    row[o] = static_cast<int64_t>(r);
    col[o] = static_cast<int64_t>(R + o);
  }
}

// Small layers: count + per-workgroup sums in one launch, then an emit that derives its own
// prefix from them (as sample_emit_prefix_kernel does) — two launches instead of count / scan /
// emit.  The layer's root count may be device resident and may be 0 (a rank without roots).
__global__ __launch_bounds__(kEmitThreads) void merge_count_sums_kernel(
    const int64_t* __restrict__ rep, const uint32_t* __restrict__ pos,
    const uint64_t* __restrict__ d_R, uint64_t R_host, uint32_t fanout,
    uint32_t* __restrict__ rec_cnt, uint32_t* __restrict__ wg_sum) {
  __shared__ uint32_t red[kEmitThreads / 64];
  const uint64_t R = d_R ? *d_R : R_host;
  const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kEmitThreads + threadIdx.x;
  uint32_t c = 0;
  if (i < R) {
    const int64_t* s = rep + static_cast<uint64_t>(pos[i]) * fanout * 3;
    for (uint32_t j = 0; j < fanout; ++j) c += s[3 * j] >= 0 ? 1u : 0u;
    rec_cnt[i] = c;
  }
  for (int d = 32; d > 0; d >>= 1) c += __shfl_down(c, d, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t t = 0;
    for (int w = 0; w < kEmitThreads / 64; ++w) t += red[w];
    wg_sum[blockIdx.x] = t;
  }
}

// Chained form: the own share's counts came from the sampling kernel itself; only the rows
// that arrived from other ranks — the first R - counts[rank] of the reply buffer — are read back
__global__ void merge_count_remote_kernel(const int64_t* __restrict__ rep,
                                          const uint32_t* __restrict__ root_of,
                                          const uint64_t* __restrict__ d_R, uint64_t R_host,
                                          const uint64_t* __restrict__ d_own, uint32_t fanout,
                                          uint32_t* __restrict__ rec_cnt) {
  const uint64_t R = d_R ? *d_R : R_host;
  const uint64_t n_net = R - min(R, *d_own);
  const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
  for (uint64_t row = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; row < n_net;
       row += stride) {
    const int64_t* s = rep + row * fanout * 3;
    uint32_t c = 0;
    for (uint32_t j = 0; j < fanout; ++j) c += s[3 * j] >= 0 ? 1u : 0u;
    rec_cnt[root_of[row]] = c;
  }
}

// Slotted layout: the rows that arrived from other ranks sit in `world` slots of `stride`
// rows (row 0 of a slot: the header row, never a reply); slot q holds min(counts[q], cap) rows.
// A root that did not fit its owner's slot (pos = the slot's header row) has no reply: its
// count is set to 0 here, so that the block's sizes stay within the layer's bounds while the
// overflowed sample runs to its end (it is then sampled again, dist.py).
__global__ void merge_count_slots_kernel(const int64_t* __restrict__ rep,
                                         const uint32_t* __restrict__ root_of,
                                         const uint32_t* __restrict__ pos,
                                         const uint64_t* __restrict__ d_R, uint64_t R_host,
                                         const uint64_t* __restrict__ counts, uint32_t stride,
                                         uint32_t world, uint32_t rank, uint32_t fanout,
                                         uint32_t* __restrict__ rec_cnt) {
  const uint64_t rows = static_cast<uint64_t>(world) * stride;
  const uint64_t step = static_cast<uint64_t>(gridDim.x) * blockDim.x;
  const uint64_t first = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  for (uint64_t row = first; row < rows; row += step) {
    const uint64_t q = row / stride, j = row - q * stride;
    if (j == 0 || q == rank || j - 1 >= min(counts[q], static_cast<uint64_t>(stride - 1))) continue;
    const int64_t* s = rep + row * fanout * 3;
    uint32_t c = 0;
    for (uint32_t k = 0; k < fanout; ++k) c += s[3 * k] >= 0 ? 1u : 0u;
    rec_cnt[root_of[row]] = c;
  }
  const uint64_t R = d_R ? *d_R : R_host;
  for (uint64_t i = first; i < R; i += step) {
    const uint32_t p = pos[i];
    if (p < rows && p % stride == 0) rec_cnt[i] = 0;
  }
}

__global__ __launch_bounds__(kEmitThreads) void merge_emit_prefix_kernel(
    const int64_t* __restrict__ roots, const float* __restrict__ root_ts,
    const uint64_t* __restrict__ d_R, uint64_t R_host, uint32_t fanout,
    const int64_t* __restrict__ rep, const uint32_t* __restrict__ pos,
    const uint32_t* __restrict__ rec_cnt, const uint32_t* __restrict__ wg_sum,
    int64_t* __restrict__ all_nodes, float* __restrict__ all_ts, float* __restrict__ dt,
    int64_t* __restrict__ eids, int64_t* __restrict__ row, int64_t* __restrict__ col,
    uint64_t* out_R, uint64_t* out_S, uint64_t* next_R) {
  __shared__ uint32_t red[kEmitThreads / 64];
  __shared__ uint32_t lbase[kEmitThreads];
  __shared__ uint32_t wave_tot[kEmitThreads / 64];
  const uint64_t R = d_R ? *d_R : R_host;
  const uint64_t total = R * fanout;
  if (total == 0) {   // nobody owns "the last slot": workgroup 0 reports the empty block
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      *out_R = 0;
      *out_S = 0;
      if (next_R) *next_R = 0;
    }
    return;
  }
  const uint64_t t0 = static_cast<uint64_t>(blockIdx.x) * kEmitThreads;
  if (t0 >= total) return;   // uniform for the workgroup
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint64_t t_last = min(t0 + kEmitThreads - 1, total - 1);
  const uint32_t r_first = static_cast<uint32_t>(t0 / fanout);
  const uint32_t r_last = static_cast<uint32_t>(t_last / fanout);
  const uint32_t nroots = r_last - r_first + 1;   // <= kEmitThreads
  const uint32_t b_first = r_first / kEmitThreads;   // count workgroups of kEmitThreads roots
  uint32_t part = 0;
  if (wg_sum) {
    for (uint32_t b = tid; b < b_first; b += kEmitThreads) part += wg_sum[b];
    for (uint32_t r = b_first * kEmitThreads + tid; r < r_first; r += kEmitThreads) part += rec_cnt[r];
  } else {
    // no per-workgroup sums: add up the counts of all the roots before this workgroup's
    // (coalesced, <= 128 KB out of L2: cheaper than the launch that would have summed them)
    for (uint32_t r = tid; r < r_first; r += kEmitThreads) part += rec_cnt[r];
  }
  for (int d = 32; d > 0; d >>= 1) part += __shfl_down(part, d, 64);
  if (lane == 0) red[wave] = part;
  const uint32_t mine = tid < static_cast<int>(nroots) ? rec_cnt[r_first + tid] : 0u;
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
  const uint64_t t = t0 + tid;
  if (t < total) {
    if (t < R) {
      all_nodes[t] = roots[t];
      all_ts[t] = root_ts[t];
    }
    const uint32_t r = static_cast<uint32_t>(t / fanout);
    const uint32_t j = static_cast<uint32_t>(t - static_cast<uint64_t>(r) * fanout);
    if (j < rec_cnt[r]) {
      const int64_t* s = rep + (static_cast<uint64_t>(pos[r]) * fanout + j) * 3;
      const uint64_t packed = static_cast<uint64_t>(s[2]);
      const uint64_t o = static_cast<uint64_t>(lbase[r - r_first]) + j;
      all_nodes[R + o] = s[0];
      all_ts[R + o] = __uint_as_float(static_cast<uint32_t>(packed));
      dt[o] = __uint_as_float(static_cast<uint32_t>(packed >> 32));
      eids[o] = s[1];
      row[o] = static_cast<int64_t>(r);
      col[o] = static_cast<int64_t>(R + o);
    }
  }
  if (t_last == total - 1 && tid == static_cast<int>(nroots) - 1) {
    const uint64_t S = static_cast<uint64_t>(lbase[tid]) + mine;
    *out_R = R;
    *out_S = S;
    if (next_R) *next_R = R + S;
  }
}

// Slotted layout, small layers: the whole merge in ONE launch.  The slots of the layer, in
// (root, slot) order, are compacted: thread t owns slot (r, j) = (t / fanout, t % fanout), which
// is valid iff root r has a reply row (pos[r] is not a slot's header row = the root fitted its
// owner's slot) and that row's slot j holds an edge; its place in the output is the number of
// valid slots before it.  The prefix over the workgroups' tiles travels through 8-byte granules
// {launch tag, tile count}: every workgroup publishes its tile's count with ONE relaxed
// agent-scope store before it looks at anybody else's, then adds up the granules of the tiles
// before its own (decoupled look-back; a granule is one naturally aligned sc1 store / sc1 load,
// so no fence is needed: /opt/skills/guides MI355X_MICROARCH "granule").  Tiles are dispatched in
// index order, so normally the lowest unfinished tile never waits for an undispatched one; a
// poll that does not see its granule within kGranuleSpins tries stops waiting and recounts that
// tile itself (see the look-back loop: termination does not depend on dispatch order).
// Replaces merge_count_slots_kernel + merge_emit_prefix_kernel: the chain of a sample is bound
// by the host thread that issues its launches, so one launch less per layer is ~3 us per sample.
__device__ unsigned int g_merge_recounts;          // tiles a look-back had to count itself

__device__ inline void merge_slots_fused_body(
    const int64_t* __restrict__ roots, const float* __restrict__ root_ts,
    const uint64_t* __restrict__ d_R, uint64_t R_host, uint32_t fanout,
    const int64_t* __restrict__ rep, const uint32_t* __restrict__ pos, uint32_t stride,
    uint32_t slot_rows, uint64_t* granules, uint64_t tag, uint32_t* d_overflow,
    int64_t* __restrict__ all_nodes, float* __restrict__ all_ts, float* __restrict__ dt,
    int64_t* __restrict__ eids, int64_t* __restrict__ row, int64_t* __restrict__ col,
    uint64_t* out_R, uint64_t* out_S, uint64_t* next_R, int narrow = 0,
    const char* __restrict__ crep = nullptr, uint32_t cslot = 0, uint32_t edge_cap = 0,
    uint32_t gm = 1, uint32_t gj = 0, uint32_t off_bytes = 4,
    MergeReuse reuse = MergeReuse{nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr}) {
  // narrow: 0 = 24 B reply slots; 1 = 12 B slots {dst, eid, edge time}, the out time is the
  // edge's; 2 = 12 B slots, the out time is the root's (prop_time)
  const uint32_t* __restrict__ rep32 = reinterpret_cast<const uint32_t*>(rep);
  const uint32_t cedges = (off_bytes * (stride + 1) + 15) & ~15u;   // a compact slot's edges
  auto offset_at = [&](const char* base, uint32_t i) -> uint32_t {
    return off_bytes == 2 ? reinterpret_cast<const uint16_t*>(base)[i]
                          : reinterpret_cast<const uint32_t*>(base)[i];
  };
  // where slot j of the reply row p is: null = no such edge.  Rows of the peers' slots come
  // in the compact form when `crep` is set, everything else as fixed-fanout rows of `rep`.
  auto record = [&](uint32_t p, uint32_t j) -> const void* {
    if (crep && p < slot_rows) {
      const uint32_t sl = p / stride, rw = p - sl * stride;
      const char* base = crep + static_cast<uint64_t>(sl) * cslot;
      const uint32_t lo = min(offset_at(base, rw), edge_cap);
      const uint32_t hi = min(offset_at(base, rw + 1 < stride ? rw + 1 : 0), edge_cap);
      if (j >= hi - lo) return nullptr;
      return base + cedges + static_cast<uint64_t>(lo + j) * (narrow ? 12 : 24);
    }
    if (narrow) {
      const uint32_t* q = rep32 + (static_cast<uint64_t>(p) * fanout + j) * 3;
      return q[0] != 0xFFFFFFFFu ? q : nullptr;
    }
    const int64_t* q = rep + (static_cast<uint64_t>(p) * fanout + j) * 3;
    return q[0] >= 0 ? q : nullptr;
  };
  // a sender whose compact slot overflowed says so in every slot it sends: all ranks redo
  if (crep && blockIdx.x == 0 && threadIdx.x * gm + gj < slot_rows / stride) {
    const char* base = crep + static_cast<uint64_t>(threadIdx.x * gm + gj) * cslot;
    if (offset_at(base, stride)) atomicOr(d_overflow, 1u);
  }
  __shared__ uint32_t wave_cnt[kEmitThreads / 64];
  __shared__ uint32_t red[kEmitThreads / 64];
  const uint64_t R = d_R ? *d_R : R_host;
  const uint64_t total = R * fanout;
  if (total == 0) {   // nobody owns "the last slot": workgroup 0 reports the empty block
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      *out_R = 0;
      *out_S = 0;
      if (next_R) *next_R = 0;
      if (reuse.first_out) reuse.first_out[0] = 0;
    }
    return;
  }
  const uint64_t t0 = static_cast<uint64_t>(blockIdx.x) * kEmitThreads;
  if (t0 >= total) return;   // uniform for the workgroup; no tile behind it exists either
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint64_t t = t0 + tid;
  bool valid = false;
  uint32_t r = 0;
  int64_t s0 = 0, s1 = 0;
  uint64_t packed = 0;
  if (t < total) {
    r = static_cast<uint32_t>(t / fanout);
    const uint32_t j = static_cast<uint32_t>(t - static_cast<uint64_t>(r) * fanout);
    const uint32_t p = pos[r];
    if (p == kPosReused) {
      // the previous block holds this root's edges (same root, same time, same fanout)
      const uint32_t lo = reuse.first_prev[r], hi = reuse.first_prev[r + 1];
      valid = j < hi - lo;
      if (valid) {
        const uint32_t e = lo + j;
        s0 = reuse.nodes_prev[reuse.R_prev + e];
        s1 = reuse.eids_prev[e];
        packed = static_cast<uint64_t>(
            pack_f32_pair(reuse.ts_prev[reuse.R_prev + e], reuse.dt_prev[e]));
      }
    } else if (!(p < slot_rows && p % stride == 0)) {
      const void* rec = record(p, j);
      valid = rec != nullptr;
      if (valid && narrow) {
        const uint32_t* s = static_cast<const uint32_t*>(rec);
        s0 = static_cast<int64_t>(s[0]);
        s1 = static_cast<int64_t>(s[1]);
        const float t = root_ts[r], ets = __uint_as_float(s[2]);
        packed = static_cast<uint64_t>(pack_f32_pair(narrow == 2 ? t : ets, t - ets));
      } else if (valid) {
        const int64_t* s = static_cast<const int64_t*>(rec);
        s0 = s[0];
        s1 = s[1];
        packed = static_cast<uint64_t>(s[2]);
      }
    }
  }
  const uint64_t ballot = __ballot(valid);
  const uint32_t before = static_cast<uint32_t>(__popcll(ballot & ((1ull << lane) - 1ull)));
  if (lane == 0) wave_cnt[wave] = static_cast<uint32_t>(__popcll(ballot));
  __syncthreads();
  uint32_t tile_cnt = 0, wbase = 0;
#pragma unroll
  for (int w = 0; w < kEmitThreads / 64; ++w) {
    if (w < wave) wbase += wave_cnt[w];
    tile_cnt += wave_cnt[w];
  }
  if (tid == 0)
    __hip_atomic_store(&granules[blockIdx.x], tag | tile_cnt, __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
  // look-back: the tiles before this one.  A granule that has not arrived after kGranuleSpins
  // polls is NOT waited for any longer: the thread counts that tile's valid slots itself (256
  // slots, two loads each: slow, but it depends on nobody).  Termination therefore does not
  // rest on the order in which workgroups are dispatched — with the GPU oversubscribed (several
  // such kernels of different streams or processes in flight, workgroups dealt to the XCDs
  // independently) a tile could otherwise wait for one that cannot be dispatched because its
  // XCD is full of waiters: observed with 4 rank processes sharing one GPU.
  uint32_t part = lookback_partial<kEmitThreads>(
      granules, blockIdx.x, tag, kGranuleCountMask, &g_merge_recounts, [&](uint32_t b) {
        uint32_t cnt = 0;
        const uint64_t lo = static_cast<uint64_t>(b) * kEmitThreads;
        const uint64_t hi = min(lo + kEmitThreads, total);
        for (uint64_t u = lo; u < hi; ++u) {
          const uint32_t ru = static_cast<uint32_t>(u / fanout);
          const uint32_t ju = static_cast<uint32_t>(u - static_cast<uint64_t>(ru) * fanout);
          const uint32_t pu = pos[ru];
          if (pu == kPosReused)
            cnt += ju < reuse.first_prev[ru + 1] - reuse.first_prev[ru] ? 1u : 0u;
          else if (!(pu < slot_rows && pu % stride == 0)) cnt += record(pu, ju) != nullptr ? 1u : 0u;
        }
        return cnt;
      });
  for (int d = 32; d > 0; d >>= 1) part += __shfl_down(part, d, 64);
  if (lane == 0) red[wave] = part;
  __syncthreads();
  uint32_t base = 0;
#pragma unroll
  for (int w = 0; w < kEmitThreads / 64; ++w) base += red[w];
  if (t < total) {
    if (t < R) {
      all_nodes[t] = roots[t];
      all_ts[t] = root_ts[t];
    }
    if (reuse.first_out && t % fanout == 0)   // slot 0 of root r: the edges before root r
      reuse.first_out[r] = base + wbase + before;
    if (valid) {
      const uint64_t o = static_cast<uint64_t>(base) + wbase + before;
      all_nodes[R + o] = s0;
      all_ts[R + o] = __uint_as_float(static_cast<uint32_t>(packed));
      dt[o] = __uint_as_float(static_cast<uint32_t>(packed >> 32));
      eids[o] = s1;
      row[o] = static_cast<int64_t>(r);
      col[o] = static_cast<int64_t>(R + o);
    }
  }
  if (t0 + kEmitThreads >= total && tid == 0) {   // the tile with the last slot
    const uint64_t S = static_cast<uint64_t>(base) + tile_cnt;
    *out_R = R;
    *out_S = S;
    if (next_R) *next_R = R + S;
    if (reuse.first_out) reuse.first_out[R] = static_cast<uint32_t>(S);
  }
}

__global__ __launch_bounds__(kEmitThreads) void merge_slots_fused_kernel(
    const int64_t* __restrict__ roots, const float* __restrict__ root_ts,
    const uint64_t* __restrict__ d_R, uint64_t R_host, uint32_t fanout,
    const int64_t* __restrict__ rep, const uint32_t* __restrict__ pos, uint32_t stride,
    uint32_t world, uint64_t* granules, uint64_t tag, uint32_t* d_overflow,
    int64_t* __restrict__ all_nodes, float* __restrict__ all_ts, float* __restrict__ dt,
    int64_t* __restrict__ eids, int64_t* __restrict__ row, int64_t* __restrict__ col,
    uint64_t* out_R, uint64_t* out_S, uint64_t* next_R) {
  merge_slots_fused_body(roots, root_ts, d_R, R_host, fanout, rep, pos, stride, world * stride,
                         granules, tag, d_overflow, all_nodes, all_ts, dt, eids, row, col, out_R,
                         out_S, next_R);
}

// m <= 4 samples that shared their exchange (blockIdx.y picks the job; each has its own granules)
__global__ __launch_bounds__(kEmitThreads) void merge_slots_fused_group_kernel(
    MergeJobs jobs, uint32_t fanout, uint32_t stride, int narrow) {
  const MergeJob& j = jobs.j[blockIdx.y];
  merge_slots_fused_body(j.roots, j.root_ts, j.d_R, j.R_host, fanout, j.rep, j.pos, stride,
                         j.slot_rows, j.granules, j.tag, j.d_overflow, j.all_nodes, j.all_ts, j.dt,
                         j.eids, j.row, j.col, j.out_R, j.out_S, j.next_R, narrow, j.crep, j.cslot,
                         j.edge_cap, j.m, j.jidx, j.off_bytes,
                         MergeReuse{j.first_prev, j.d_R_prev ? *j.d_R_prev : j.R_prev_host,
                                    j.nodes_prev, j.ts_prev, j.dt_prev, j.eids_prev, j.first_out});
}

// Compact replies of a shared chain: one workgroup per received request slot turns the slot's
// served rows (fixed `fanout` records each, of which a few hold an edge) into what travels back:
// u32 [0] = edges of the slot, [r] = edges of the rows before row r (1 <= r < stride),
// [stride] = "a slot of this sender overflowed its edge capacity" (written for ALL slots of the
// sample by whichever workgroup finishes last: one atomic carries the ticket and the flag), then
// the edges packed in row order.  Rows the request header does not announce hold nothing.
// (The reference ships back exactly the sampled edges of a partition,
// gnnflow/distributed/common.py:4-19, dist_sampler.py:244-314.)
__global__ __launch_bounds__(kCompactThreads) void reply_compact_kernel(CompactArgs a) {
  const uint32_t sl = blockIdx.x, tid = threadIdx.x, stride = a.stride, F = a.fanout;
  const uint64_t announced = static_cast<uint64_t>(a.inbox[2 * static_cast<uint64_t>(sl) * stride]);
  const uint32_t rows = static_cast<uint32_t>(min(announced, static_cast<uint64_t>(stride - 1)));
  char* base = a.cserved + static_cast<uint64_t>(sl) * a.cslot;
  auto put = [&](char* slot, uint32_t i, uint32_t v) {
    if (a.off_bytes == 2) reinterpret_cast<uint16_t*>(slot)[i] = static_cast<uint16_t>(min(v, 65535u));
    else reinterpret_cast<uint32_t*>(slot)[i] = v;
  };
  char* edges = base + ((a.off_bytes * (stride + 1) + 15) & ~15u);
  const uint32_t rb = a.narrow ? 12u : 24u;
  __shared__ uint32_t wsum[kCompactThreads / 64];
  __shared__ uint32_t carry;
  if (tid == 0) carry = 0;
  __syncthreads();
  for (uint32_t b0 = 1; b0 < stride; b0 += kCompactThreads) {
    const uint32_t r = b0 + tid;                         // row of the slot (row 0 is its header)
    const uint64_t grow = static_cast<uint64_t>(sl) * stride + r;
    const uint32_t cnt = (r < stride && r - 1 < rows) ? a.row_cnt[grow] : 0u;
    uint32_t incl = cnt;
    const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t up = __shfl_up(incl, d, 64);
      if (lane >= d) incl += up;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    uint32_t before = carry, total = 0;
#pragma unroll
    for (int w = 0; w < kCompactThreads / 64; ++w) {
      const uint32_t x = wsum[w];
      if (w < wave) before += x;
      total += x;
    }
    const uint32_t at = before + incl - cnt;
    if (r < stride) put(base, r, at);
    for (uint32_t k = 0; k < cnt; ++k) {
      if (at + k >= a.edge_cap) break;
      const uint32_t* src = reinterpret_cast<const uint32_t*>(
          static_cast<const char*>(a.served) + (grow * F + k) * rb);
      uint32_t* dst = reinterpret_cast<uint32_t*>(edges + static_cast<uint64_t>(at + k) * rb);
      for (uint32_t w = 0; w < rb / 4; ++w) dst[w] = src[w];
    }
    __syncthreads();
    if (tid == 0) carry += total;
    __syncthreads();
  }
  if (tid == 0) {
    const uint32_t total = carry;
    put(base, 0, total);
    const uint32_t j = sl % a.m, ovf = total > a.edge_cap ? 1u : 0u;
    const unsigned long long fresh = static_cast<unsigned long long>(a.tag) << 32;
    unsigned long long old = __hip_atomic_load(&a.ticket[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    uint32_t prev;
    for (;;) {
      const unsigned long long cur = static_cast<uint32_t>(old >> 32) == a.tag ? old : fresh;
      const unsigned long long seen = atomicCAS(&a.ticket[j], old, cur + 1u + (ovf << 16));
      if (seen == old) { prev = static_cast<uint32_t>(cur); break; }
      old = seen;
    }
    if ((prev & 0xFFFFu) == a.world - 1) {       // the last of this sample's `world` slots
      const uint32_t any = ((prev >> 16) + ovf) ? 1u : 0u;
      for (uint32_t q = 0; q < a.world; ++q)
        put(a.cserved + static_cast<uint64_t>(q * a.m + j) * a.cslot, stride, any);
    }
  }
}

}  // namespace

void launch_merge_fused_group(const MergeJobs& jobs, unsigned grid, int m, uint32_t fanout,
                              uint32_t stride, int narrow, hipStream_t stream) {
  merge_slots_fused_group_kernel<<<dim3(grid, static_cast<unsigned>(m)), dim3(kEmitThreads), 0,
                                   stream>>>(jobs, fanout, stride, narrow);
}
void launch_reply_compact(const CompactArgs& a, unsigned grid, hipStream_t stream) {
  reply_compact_kernel<<<dim3(grid), dim3(kCompactThreads), 0, stream>>>(a);
}

// Tag of the look-back granules of one fused-merge launch: unique in the PROCESS, not per
// sampler — a sampler's workspace may be memory another sampler's launches wrote granules into
// (freed and allocated again), and a stale granule must never carry a tag a later launch uses.
std::atomic<uint64_t> g_merge_epoch{0};
uint64_t next_merge_tag() { return (g_merge_epoch.fetch_add(1) + 1) << 10; }

void Sampler::merge_padded(const int64_t* d_roots, const float* d_ts, size_t R, uint32_t layer,
                           const int64_t* d_replies, const uint32_t* d_pos, void* d_out,
                           size_t out_bytes, gf_block* block, hipStream_t stream) {
  GF_REQUIRE(layer < fanouts_.size(), "merge_padded: layer out of range");
  GF_REQUIRE(block != nullptr, "merge_padded: null block");
  if (R == 0) {
    std::memset(block, 0, sizeof(gf_block));
    return;
  }
  GF_REQUIRE(d_roots && d_ts && d_replies && d_pos && d_out, "merge_padded: null device pointer");
  GF_REQUIRE(out_bytes >= layer_output_bytes(R, layer), "merge_padded: output buffer too small");
  const uint32_t F = fanouts_[layer];
  GF_REQUIRE(static_cast<uint64_t>(R) * F < 0xFFFFFFFFull,
             "sampler: more than 2^32-1 slots in one layer");
  DeviceGuard dg(graph_->device());
  reserve_workspace(R, 2, stream);
  char* w = ws_.as<char>();
  w += align_up(ws_roots_ * 8, 16);                                   // rec_end: unused here
  uint32_t* rec_cnt = reinterpret_cast<uint32_t*>(w); w += align_up(ws_roots_ * 4, 16);
  uint32_t* base = reinterpret_cast<uint32_t*>(w);    w += align_up(ws_roots_ * 4, 16);
  uint32_t* tile_scratch = reinterpret_cast<uint32_t*>(w); w += align_up(ws_roots_ * 4, 16);
  uint64_t* d_counts = reinterpret_cast<uint64_t*>(w);
  BlockPtrs out = carve(static_cast<char*>(d_out), R, F);
  merge_count_kernel<<<dim3(static_cast<unsigned>((R + 255) / 256)), dim3(256), 0, stream>>>(
      d_replies, d_pos, nullptr, R, F, rec_cnt, 0u, 0u);
  launch_scan(rec_cnt, base, tile_scratch, nullptr, R, R, F, 0, d_counts, d_counts + 1, nullptr,
              stream);
  merge_emit_kernel<<<dim3(capped_grid(static_cast<uint64_t>(R) * F, kEmitThreads, 256 * 16)),
                      dim3(kEmitThreads), 0, stream>>>(
      d_roots, d_ts, nullptr, R, F, d_replies, d_pos, rec_cnt, base, out.all_nodes, out.all_ts,
      out.dt, out.eids, out.row, out.col);
  GF_HIP(hipGetLastError());
  GF_HIP(hipMemcpyAsync(h_layer_counts_.data(), d_counts, 2 * sizeof(uint64_t),
                        hipMemcpyDeviceToHost, stream));
  GF_HIP(hipStreamSynchronize(stream));
  const uint64_t* hc = h_layer_counts_.as<uint64_t>();
  block->all_nodes = out.all_nodes;
  block->all_timestamps = out.all_ts;
  block->delta_timestamps = out.dt;
  block->eids = out.eids;
  block->row = out.row;
  block->col = out.col;
  block->num_dst_nodes = hc[0];
  block->num_edges = hc[1];
  block->num_src_nodes = hc[0] + hc[1];
}

void Sampler::part_merge(uint32_t layer, uint32_t snapshot, void* d_ws, size_t ws_bytes) {
  GF_REQUIRE(part_.active, "part_merge: no partitioned sample is being built");
  GF_REQUIRE(layer < fanouts_.size() && snapshot < num_snapshots_, "part_merge: out of range");
  gf_part_layout lay;
  part_layout(part_.Rs, layer, part_.world, part_.slack, part_.slot_roots, &lay);
  GF_REQUIRE(d_ws && ws_bytes >= lay.total, "part_merge: workspace too small");
  DeviceGuard dg(graph_->device());
  const size_t L = fanouts_.size(), NS = num_snapshots_;
  char* w = static_cast<char*>(d_ws);
  const int64_t* roots; const float* ts; const uint64_t* d_R; uint64_t R_host;
  part_roots(layer, snapshot, &roots, &ts, &d_R, &R_host);
  hipStream_t stream = part_.stream;
  const size_t Rb = layer == 0 ? part_.R : lay.root_bound;
  const uint32_t F = fanouts_[layer];
  const size_t b = layer * NS + snapshot;
  uint64_t* slot = part_counts() + 2 * b;
  uint64_t* next_R = (layer + 1 < L) ? slot + 2 * NS : nullptr;
  const BlockPtrs& out = part_.slot->ptrs[b];
  char* sw = ws_.as<char>();
  sw += align_up(ws_roots_ * 8, 16);                                   // rec_end: unused here
  uint32_t* rec_cnt = reinterpret_cast<uint32_t*>(sw); sw += align_up(ws_roots_ * 4, 16);
  uint32_t* base = reinterpret_cast<uint32_t*>(sw);    sw += align_up(ws_roots_ * 4, 16);
  uint32_t* tile_scratch = reinterpret_cast<uint32_t*>(sw);
  const int64_t* rep = reinterpret_cast<const int64_t*>(w + lay.replies);
  const uint32_t* pos = reinterpret_cast<const uint32_t*>(w + lay.pos);
  if (Rb == 0) {   // layer 0 of a rank without roots: an empty block, R = S = 0
    GF_HIP(hipMemsetAsync(slot, 0, 2 * sizeof(uint64_t), stream));
    if (next_R) GF_HIP(hipMemsetAsync(next_R, 0, sizeof(uint64_t), stream));
    return;
  }
  ProfileScope ps(kProfEmit, stream);
  if (lay.slot_stride && part_fused_merge(Rb, F)) {
    // granules: the workspace's rec_end array (8 B per root, unused by the partitioned path)
    const unsigned egrid = static_cast<unsigned>(
        (static_cast<uint64_t>(Rb) * F + kEmitThreads - 1) / kEmitThreads);
    const uint64_t tag = next_merge_tag();
    merge_slots_fused_kernel<<<dim3(egrid), dim3(kEmitThreads), 0, stream>>>(
        roots, ts, d_R, R_host, F, rep, pos, static_cast<uint32_t>(lay.slot_stride),
        static_cast<uint32_t>(part_.world), reinterpret_cast<uint64_t*>(ws_.as<char>()), tag,
        part_overflow(), out.all_nodes, out.all_ts, out.dt, out.eids, out.row, out.col, slot,
        slot + 1, next_R);
    GF_HIP(hipGetLastError());
    return;
  }
  if (part_own_counts(Rb)) {
    // rec_cnt lives in the sampler workspace; the own share's counts are already there
    // (part_plan_own phase 2), the rows received from other ranks are counted here; the emit
    // derives its own prefix from the counts (no scan launch, no per-workgroup sums)
    (void)base; (void)tile_scratch;
    if (lay.slot_stride) {
      const uint64_t* d_counts = reinterpret_cast<const uint64_t*>(w + lay.counts);
      merge_count_slots_kernel<<<dim3(capped_grid(part_.world * lay.slot_stride + Rb, 256, 1024)),
                                 dim3(256), 0, stream>>>(
          rep, part_root_of(), pos, d_R, R_host, d_counts, static_cast<uint32_t>(lay.slot_stride),
          static_cast<uint32_t>(part_.world), static_cast<uint32_t>(part_.rank), F, rec_cnt);
    } else if (part_.world > 1) {
      uint64_t* d_counts = reinterpret_cast<uint64_t*>(w + lay.counts);
      merge_count_remote_kernel<<<dim3(capped_grid(Rb, 256, 1024)), dim3(256), 0, stream>>>(
          rep, part_root_of(), d_R, R_host, d_counts + part_.rank, F, rec_cnt);
    }
    const unsigned egrid = static_cast<unsigned>(
        (static_cast<uint64_t>(Rb) * F + kEmitThreads - 1) / kEmitThreads);
    merge_emit_prefix_kernel<<<dim3(egrid), dim3(kEmitThreads), 0, stream>>>(
        roots, ts, d_R, R_host, F, rep, pos, rec_cnt, static_cast<const uint32_t*>(nullptr),
        out.all_nodes, out.all_ts, out.dt, out.eids, out.row, out.col, slot, slot + 1, next_R);
    GF_HIP(hipGetLastError());
    return;
  }
  merge_count_kernel<<<dim3(static_cast<unsigned>((Rb + 255) / 256)), dim3(256), 0, stream>>>(
      rep, pos, d_R, R_host, F, rec_cnt, static_cast<uint32_t>(lay.slot_stride),
      static_cast<uint32_t>(part_.world));
  launch_scan(rec_cnt, base, tile_scratch, d_R, R_host, Rb, F, 0, slot, slot + 1, next_R, stream);
  merge_emit_kernel<<<dim3(capped_grid(static_cast<uint64_t>(Rb) * F, kEmitThreads, 256 * 16)),
                      dim3(kEmitThreads), 0, stream>>>(
      roots, ts, d_R, R_host, F, rep, pos, rec_cnt, base, out.all_nodes, out.all_ts, out.dt,
      out.eids, out.row, out.col);
  GF_HIP(hipGetLastError());
}

// Tiles whose look-back granule did not arrive in time and were recounted by the waiting thread
// (fused merge), since the library was loaded, on the current device.
uint64_t merge_recounts() {
  unsigned int v = 0;
  GF_HIP(hipMemcpyFromSymbol(&v, HIP_SYMBOL(g_merge_recounts), sizeof(v)));
  return v;
}

}  // namespace gf
