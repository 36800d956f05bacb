// What the translation units of the LRU update share (cache_lru.hip, cache_lru_fused.hip,
// cache_lru_queue.hip): the device helpers more than one form of the update uses and the launch
// function of each form.  Private to those files; the overview is cache_lru.hip's header.
#pragma once

#include "feature_cache_ctx.hpp"

namespace gf {

// (internal linkage, as when they stood in the one translation unit: the same inlining decisions)
namespace {

// victims through the list tiles' staged entries, or the one-workgroup walk (kStageMinWant)
__device__ inline bool use_staged_victims(uint32_t stage_tiles, uint32_t missed_rows,
                                          uint32_t min_want) {
  return stage_tiles != 0 && missed_rows > min_want;
}

// Exclusive scan of one value per thread over a kWide-wide workgroup; *total gets the sum.
// Every thread calls it (barriers inside); `ws` is kWide / 64 words of LDS.
__device__ inline uint32_t wide_excl_scan(uint32_t v, uint32_t* ws, uint32_t* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t incl = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t up = __shfl_up(incl, d, 64);
    if (lane >= d) incl += up;
  }
  __syncthreads();            // ws may still be read from a previous call
  if (lane == 63) ws[wave] = incl;
  __syncthreads();
  uint32_t base = 0, sum = 0;
#pragma unroll
  for (int w = 0; w < kWide / 64; ++w) {
    const uint32_t x = ws[w];
    if (w < wave) base += x;
    sum += x;
  }
  *total = sum;
  return base + incl - v;
}

// sum of one value per thread over the workgroup (every thread calls it and gets the sum)
__device__ inline uint32_t wide_sum(uint32_t v, uint32_t* ws) {
  for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = v;
  __syncthreads();
  uint32_t sum = 0;
#pragma unroll
  for (int w = 0; w < kWide / 64; ++w) sum += ws[w];
  return sum;
}

// Queue form.  Chunks of the queue behind the head the victim walk covers for a block that missed
// `want` rows: the host sizes everything for 2 x block rows + 2 tiles (it does not know the misses);
// the device needs that much only if every row missed.  Scan, walk and install agree on it.
__device__ inline uint32_t victim_chunks_used(const Ctx& c, uint32_t want) {
  return min(c.v_chunks, (2u * want + kRowTile - 1) / kRowTile + 2u);
}

// Queue form: four consecutive queue entries from p0 (16-byte aligned); bit j of the result:
// entry p0 + j is live (qpos points at it) and its slot was not hit by this block (the
// gather marked the hit entries' positions in qbits: read densely here).
__device__ inline uint32_t victim_walk4(const Ctx& c, const uint32_t* list, uint32_t head,
                                        uint32_t tail, uint32_t p0, uint32_t* sl) {
  // the buffers are allocated 16 entries past queue_cap: a whole vector is readable
  const uint4 v = p0 < tail ? *reinterpret_cast<const uint4*>(list + p0)
                            : make_uint4(0u, 0u, 0u, 0u);
  // the four positions share one word of the hit bitmap (p0 is a multiple of 4)
  const uint32_t hitw = p0 < tail ? c.qbits[p0 >> 5] >> (p0 & 31u) : 0u;
  uint32_t qp[4], mask = 0;
  sl[0] = v.x; sl[1] = v.y; sl[2] = v.z; sl[3] = v.w;
#pragma unroll
  for (uint32_t j = 0; j < 4; ++j) {
    const bool in = p0 + j >= head && p0 + j < tail;
    if (!in) sl[j] = 0u;   // beyond the tail: not initialised
    qp[j] = c.qpos[sl[j]];
  }
#pragma unroll
  for (uint32_t j = 0; j < 4; ++j) {
    const bool in = p0 + j >= head && p0 + j < tail;
    if (in && qp[j] == p0 + j && !((hitw >> j) & 1u)) mask |= 1u << j;
  }
  return mask;
}

// workgroup-wide helpers for kBlock threads (the queue form's install kernel runs many small
// workgroups per CU; the wide_* ones above are for kWide)
template <int kBlock>
__device__ inline uint32_t block_excl_scan(uint32_t v, uint32_t* ws, uint32_t* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t incl = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t up = __shfl_up(incl, d, 64);
    if (lane >= d) incl += up;
  }
  __syncthreads();            // ws may still be read from a previous call
  if (lane == 63) ws[wave] = incl;
  __syncthreads();
  uint32_t base = 0, sum = 0;
#pragma unroll
  for (int w = 0; w < kBlock / 64; ++w) {
    const uint32_t x = ws[w];
    if (w < wave) base += x;
    sum += x;
  }
  *total = sum;
  return base + incl - v;
}

// Copies the rows a workgroup installed — inst[j] = {slot, row} — from the block's output into
// the cache, as one flat array of 16-byte vectors, kBlock threads, K loads in flight per thread
// (rows of `rowf` floats; VecT float4 for 16-byte-aligned rows, uf4 otherwise).
template <typename VecT, int K, uint32_t kBlock = kWide>
__device__ inline void copy_installed(const Ctx& c, const uint2* inst, const int64_t* inst_id,
                                      uint32_t n_inst, uint32_t rowf, int tid) {
  if (!c.cache_buf) return;   // no row mirror: the slots hold ids only
  const uint32_t total = n_inst * c.dimv;
  const bool table = c.inst_from_table != 0;
#pragma unroll 1
  for (uint32_t f0 = tid; f0 < total; f0 += K * kBlock) {
    float4 v[K];   // (an array of the under-aligned uf4 would live in scratch)
    uint32_t dj[K], dc[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const uint32_t f = f0 + k * kBlock;
      const bool ok = f < total;
      const uint32_t j = ok ? f / c.dimv : 0u, cc = ok ? f - j * c.dimv : 0u;
      const uint2 pr = inst[j];
      dj[k] = ok ? pr.x : ~0u;
      dc[k] = min(cc * 4, rowf - 4);   // odd rows: the last vector ends with the row
      const float* srow = table ? c.feats + static_cast<uint64_t>(inst_id[j]) * rowf
                                : c.out + static_cast<uint64_t>(pr.y) * rowf;
      const VecT t = *reinterpret_cast<const VecT*>(srow + dc[k]);
      v[k] = make_float4(t.x, t.y, t.z, t.w);
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
      if (dj[k] != ~0u) {
        VecT t;
        t.x = v[k].x; t.y = v[k].y; t.z = v[k].z; t.w = v[k].w;
        *reinterpret_cast<VecT*>(c.cache_buf + static_cast<uint64_t>(dj[k]) * rowf + dc[k]) = t;
      }
    }
  }
}

constexpr int kQInst = 256;   // queue form: block rows (= threads) per install workgroup

}  // namespace

// ---- the forms' launches -------------------------------------------------------------------
// launch_lru_update (cache_lru.hip) sizes them from the round's contexts and checks for launch
// errors once per chain: only the launchers that say so check themselves.
// cache_lru_fused.hip: the list form in one launch, for the round's fused contexts: `list_tiles` /
// `row_wgs` of the largest of them.  own_events: the launch carries the profile's dispatch
// events itself (launch_round; such a round has no other update, so it is never forked).  Checks.
void launch_lru_fused(const Round& r, size_t list_tiles, size_t row_wgs, hipStream_t stream,
                      bool own_events);
// cache_lru_queue.hip: what follows lru_list_scan_kernel for the round's queue-form contexts —
// the lone walk and the install; `rows` of the largest of them
void launch_lru_queue_update(const Round& r, size_t rows, hipStream_t stream);
// ... the compaction of one cache's queue, `tail_bound` entries of it, into the other buffer;
// `scratch` is laid out by compact_layout() (feature_cache_ctx.hpp).  Checks.
void launch_lru_queue_compact(uint32_t* q0, uint32_t* q1, QueueState* qs, uint32_t* qpos,
                              char* scratch, const CompactLayout& layout, size_t tail_bound,
                              uint32_t capacity, hipStream_t stream);
// ... and qpos[] of a dense list.  Checks.
void launch_lru_queue_index(const uint32_t* q0, const uint32_t* q1, const QueueState* qs,
                            uint32_t* qpos, uint32_t capacity, hipStream_t stream);

}  // namespace gf
