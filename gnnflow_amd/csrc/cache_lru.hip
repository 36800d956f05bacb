// The update of the LRU contexts of a fetch round (feature_cache.hip).
//
// LRU — the policy on the hot path — needs no selection at all: the reference's `count`
// only ever changes to "newest" (hit or install: count = 0 while all others sink by one,
// lru_cache.py:134-160), so the eviction order is a LIST, least recently refreshed slot
// first, that every update permutes in the same simple way: the slots hit by the block move
// behind the others, the first k = #distinct misses entries are the victims and go, refilled,
// to the very back.  `queue` holds that list (a permutation of the slots, double-buffered);
// no stamps, no histogram, no threshold, no atomics, and ties are resolved STABLY — slots of
// equal `count` keep their relative order, what a stable sort by `count` yields (the
// reference leaves it to torch.topk's unspecified tie-breaking).  One launch per round
// (lru_list_fused_kernel, "LRU list form in ONE launch" below) where its LDS tables fit; else,
// and with GNNFLOW_LRU_FUSED=0, the same work as two launches:
//   list scan   : row-tile workgroups rank the representatives of the distinct missed ids;
//                 list-tile workgroups count the hit slots per tile of the list; one more
//                 workgroup reads the victims off the front of the list.
//   list install: one thread per block row installs the m-th missed id in the m-th victim's
//                 slot (map / slot_id / row copy from the freshly gathered output — spread
//                 over as many workgroups as the block has rows); list-tile workgroups write
//                 the permuted list into the other buffer.
// A cache of 0.5 M slots or more keeps the same list as a queue ("LRU as a queue" below).
// All kernels return at once for a context whose block had no miss (the reference skips
// update_*_cache then too, cache.py:318); a hit only changes replacement state if the block
// also had a miss, exactly as in the reference.
#include "feature_cache_ctx.hpp"

#include <hip/hip_ext.h>

#include <algorithm>
#include <mutex>
#include <vector>

namespace gf {

namespace {

// victims through the list tiles' staged entries, or the one-workgroup walk (kStageMinWant)
__device__ inline bool use_staged_victims(uint32_t stage_tiles, uint32_t missed_rows,
                                          uint32_t min_want) {
  return stage_tiles != 0 && missed_rows > min_want;
}

// ---- LRU as a list ------------------------------------------------------------------
// (see the file header).  c.touched[slot] = epoch of the slot's last hit (plain stores by the
// gather); c.queue[0 / 1] are the two list buffers, qstate->parity says which one is current.

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

// Queue form: four consecutive queue entries from p0 (16-byte aligned); bit j of the result:
// entry p0 + j is live (qpos points at it) and its slot was not hit by this block (the
// gather marked the hit entries' positions in qbits: read densely here).
// Chunks of the queue behind the head the victim walk covers for a block that missed `want`
// rows: the host sizes everything for 2 x block rows + 2 tiles (it does not know the misses);
// the device needs that much only if every row missed.  Scan, walk and install agree on it.
__device__ inline uint32_t victim_chunks_used(const Ctx& c, uint32_t want) {
  return min(c.v_chunks, (2u * want + kRowTile - 1) / kRowTile + 2u);
}

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

// One launch, three kinds of workgroups (per context), all reading what the gather left:
//  * row workgroups   [0, row_blocks): each owns `tiles_per_wg` consecutive tiles of kRowTile
//    rows, finds the representatives of the distinct missed ids in them (the row whose claim
//    on map[id] survived the gather's atomicMax), ranks them in row order inside its span and
//    publishes the span's count;
//  * list workgroups  [row_blocks, row_blocks + list_blocks): count, per tile of kRowTile list
//    entries, the slots hit by this block (they will move behind the others);
//  * the victim workgroup (last) walks the list from its front and writes down the first
//    not-hit entries — as many as the block has missed ROWS (an upper bound of the distinct
//    missed ids, which only the next kernel knows) — and the hit entries it passes on the way
//    (the next victims if a block needs more slots than its own hits leave over).
// (8 waves per SIMD = 64 VGPRs, no spill: TWO workgroups per CU — a GDELT-shaped round launches
// 730 of them, 4 us each: 19.9 -> 15.6 us per launch)
__global__ __launch_bounds__(kWide, 8) void lru_list_scan_kernel(Round r, uint32_t row_blocks,
                                                              uint32_t list_blocks,
                                                              uint32_t victim_blocks) {
  const Ctx& c = r.c[blockIdx.y];
  if (!c.update || c.policy != GF_CACHE_LRU || c.fused) return;
  const int tid = threadIdx.x;
  __shared__ uint32_t ws[kWide / 64];
  const uint32_t parity = c.qstate->parity;
  const uint32_t* list = c.queue[parity & 1u];
  constexpr uint32_t kItems = kRowTile / kWide;
  if (blockIdx.x < row_blocks) {
    __shared__ uint32_t carry;
    const uint32_t row_tiles = (c.n + kLruRows - 1) / kLruRows;
    constexpr uint32_t kItems = kLruRows / kWide;   // shadows the list role's
    const uint32_t t_begin = blockIdx.x * c.tiles_per_wg;
    if (t_begin >= row_tiles) return;
    const uint32_t t_end = min(t_begin + c.tiles_per_wg, row_tiles);
    if (tid == 0) carry = 0;
    __syncthreads();
    for (uint32_t t = t_begin; t < t_end; ++t) {
      const uint32_t i0 = t * kLruRows + tid * kItems;
      int32_t sr[kItems];
      int64_t idv[kItems];
#pragma unroll
      for (uint32_t k = 0; k < kItems; ++k) {
        const bool ok = i0 + k < c.n;
        sr[k] = ok ? c.slot_of_row[i0 + k] : -2;
        idv[k] = ok ? c.ids[i0 + k] : 0;
      }
      if (t == t_begin && total_miss(c.ctr) == 0) return;   // uniform: nothing to update
      uint32_t fm[kItems], lm = 0;
#pragma unroll
      for (uint32_t k = 0; k < kItems; ++k) {
        fm[k] = (sr[k] == -1 && c.map[idv[k]] == -static_cast<int32_t>(i0 + k + 1)) ? 1u : 0u;
        lm += fm[k];
      }
      uint32_t tm;
      uint32_t run = carry + wide_excl_scan(lm, ws, &tm);
#pragma unroll
      for (uint32_t k = 0; k < kItems; ++k) {
        // (queue form: the gather left kRepHit | position for the rows that stand for a hit
        // slot and 0 for the others)
        if (i0 + k < c.n && (fm[k] || !c.qmode)) c.rep_flag[i0 + k] = fm[k] ? (kRepMiss | run) : 0u;
        run += fm[k];
      }
      __syncthreads();
      if (tid == 0) carry += tm;
      __syncthreads();
    }
    if (tid == 0) c.row_tile_sum[blockIdx.x] = carry;
    return;
  }
  const uint32_t cap = c.capacity;
  if (blockIdx.x < row_blocks + list_blocks) {
    if (c.qmode) {
      // queue form: the hit bitmap (set by the gather: 1/32 of the queue positions [head, tail))
      // per tile of kBitTile words — hit entries per tile, and per word a snapshot {word, hit
      // entries before it in its tile}: the rank of a hit entry among all of them = tile
      // prefix (the install kernel's LDS) + that + the bits below its own.  The words
      // themselves are cleared by the rows that set them, once the snapshot is all anyone reads.
      const uint32_t head = c.qstate->head, tail = c.qstate->tail;
      const uint32_t w_lo = head >> 5, w_hi = (tail + 31u) >> 5;
      const uint32_t t0 = w_lo / kBitTile;
      const uint32_t btiles = (w_hi + kBitTile - 1) / kBitTile - t0;
      const bool none = total_miss(c.ctr) == 0;
      for (uint32_t t = blockIdx.x - row_blocks; t < btiles; t += list_blocks) {
        const size_t wi = static_cast<size_t>(t0 + t) * kBitTile + tid * 4;   // four words per thread
        const uint4 wd = *reinterpret_cast<const uint4*>(c.qbits + wi);
        if (none) {
          // a block without a miss leaves the cache as it is (lru_cache.py: update() is only
          // called with missed ids): its hit marks are dropped
          if (wd.x | wd.y | wd.z | wd.w) *reinterpret_cast<uint4*>(c.qbits + wi) = make_uint4(0u, 0u, 0u, 0u);
          continue;
        }
        const uint32_t p0 = __popc(wd.x), p1 = __popc(wd.y), p2 = __popc(wd.z), p3 = __popc(wd.w);
        uint32_t total;
        const uint32_t b = wide_excl_scan(p0 + p1 + p2 + p3, ws, &total);
        // (only words with a bit set are ever looked up: 5-10 % of them on the GDELT-shaped step)
        uint4* sn = reinterpret_cast<uint4*>(c.wsnap + wi);
        if (wd.x | wd.y) sn[0] = make_uint4(wd.x, b, wd.y, b + p0);
        if (wd.z | wd.w) sn[1] = make_uint4(wd.z, b + p0 + p1, wd.w, b + p0 + p1 + p2);
        if (tid == 0) c.tile_tie[t] = total;
      }
      return;
    }
    const uint32_t list_tiles = (cap + kRowTile - 1) / kRowTile;
    if (blockIdx.x == row_blocks && tid == 0) c.ctr->q_parity = parity;
    bool first = true, staged = false;
    for (uint32_t t = blockIdx.x - row_blocks; t < list_tiles; t += list_blocks) {
      const uint32_t p0 = t * kRowTile + tid * kItems;
      uint32_t sl[kItems], hit[kItems], tc[kItems], local = 0;
      // the hit marks are indexed by list position: their loads do not wait for the list's
#pragma unroll
      for (uint32_t j = 0; j < kItems; ++j) tc[j] = p0 + j < cap ? c.touched[p0 + j] : 0u;
      if (first) {
        // the first tile is read from BOTH buffers while the parity word is still on its
        // way (one dependent hop less on the kernel's critical chain)
        uint32_t alt[kItems];
#pragma unroll
        for (uint32_t j = 0; j < kItems; ++j) {
          sl[j] = p0 + j < cap ? c.queue[0][p0 + j] : 0u;
          alt[j] = p0 + j < cap ? c.queue[1][p0 + j] : 0u;
        }
#pragma unroll
        for (uint32_t j = 0; j < kItems; ++j) sl[j] = (parity & 1u) ? alt[j] : sl[j];
        first = false;
        const uint32_t missed = total_miss(c.ctr);
        if (missed == 0) return;   // uniform across the launch
        staged = use_staged_victims(c.stage_tiles, missed, c.stage_min);
      } else {
#pragma unroll
        for (uint32_t j = 0; j < kItems; ++j) sl[j] = p0 + j < cap ? list[p0 + j] : 0u;
      }
#pragma unroll
      for (uint32_t j = 0; j < kItems; ++j) {
        hit[j] = (p0 + j < cap && tc[j] == c.epoch_new) ? 1u : 0u;
        local += hit[j];
      }
      uint32_t total;
      if (staged && t < c.stage_tiles) {
        // the victims come off the FRONT of the list: the first tiles leave their not-hit
        // entries packed, in list order (thread order = list order); the install kernel
        // finds the m-th one through the per-tile hit counts
        uint32_t before_hits = wide_excl_scan(local, ws, &total);
        uint32_t at_keep = t * kRowTile + tid * kItems - before_hits;   // not-hit before me
        uint32_t at_hit = t * kRowTile + before_hits;
#pragma unroll
        for (uint32_t j = 0; j < kItems; ++j) {
          if (p0 + j < cap) {
            if (!hit[j]) c.v_slot[at_keep++] = sl[j];
            else if (c.stage_hits) c.v_pos[at_hit++] = sl[j];
          }
        }
      } else {
        total = wide_sum(local, ws);
      }
      if (tid == 0) {
        c.tile_tie[t] = total;
        if (total) atomicAdd(&c.tile_old[t / kQGroup], total);   // zeroed by the gather
      }
    }
    return;
  }
  const uint32_t want = min(total_miss(c.ctr), cap);
  if (c.qmode) {
    // queue form: the victims are the first LIVE entries from the head that the block did
    // not hit (the host only chooses this form for blocks of <= capacity / 4 rows, so there
    // are always enough).  The walk is spread over the victim workgroups — one CU alone is
    // bound by its 64-line-per-instruction address rate on the two scattered loads per entry
    // (measured 27-37 us for 20 k victims) — in chunks of kRowTile entries: every chunk leaves
    // its candidates and their count (the install kernel finds the m-th of them through the
    // counts).  The chunks cover 2 * rows + 2 tiles from the head; should that not yield `want`
    // candidates (many dead entries right behind the head), lru_queue_walk_kernel walks on.
    // (No "last workgroup" ticket here: the __threadfence() it needs writes the XCD's whole
    // L2 back on this part — measured +15 us.)
    const uint32_t vb = blockIdx.x - row_blocks - list_blocks;
    const uint32_t head = c.qstate->head, tail = c.qstate->tail;
    if (vb == 0 && tid == 0) { c.ctr->q_parity = parity; c.ctr->q_head = head; c.ctr->q_tail = tail; }
    if (want == 0) return;
    const uint32_t hbase = head & ~3u, chunks = victim_chunks_used(c, want);
    for (uint32_t ch = vb; ch < chunks; ch += victim_blocks) {
      const uint32_t p0 = hbase + ch * kRowTile + tid * 4;
      uint32_t sl[4];
      const uint32_t mask = victim_walk4(c, list, head, tail, p0, sl);
      uint32_t total;
      uint32_t at = ch * kRowTile + wide_excl_scan(__popc(mask), ws, &total);
#pragma unroll
      for (uint32_t j = 0; j < 4; ++j)
        if (mask & (1u << j)) { c.v_slot[at] = sl[j]; c.v_pos[at] = p0 + j; ++at; }
      if (tid == 0) c.v_count[ch] = total;
    }
    return;
  }
  if (blockIdx.x != row_blocks + list_blocks ||
      use_staged_victims(c.stage_tiles, total_miss(c.ctr), c.stage_min)) return;
  if (want == 0) return;
  uint32_t* kept = c.rep_row;     // victims: not-hit entries from the front of the list
  uint32_t* moved = c.rep_rank;   // hit entries passed on the way
  uint32_t found = 0, found_hit = 0;
  for (uint32_t base = 0; base < cap && found < want; base += kRowTile) {
    const uint32_t p0 = base + tid * kItems;
    uint32_t sl[kItems], hit[kItems], lk = 0, lh = 0;
#pragma unroll
    for (uint32_t j = 0; j < kItems; ++j) sl[j] = p0 + j < cap ? list[p0 + j] : 0u;
#pragma unroll
    for (uint32_t j = 0; j < kItems; ++j) {
      const bool in = p0 + j < cap;
      hit[j] = in ? (c.touched[p0 + j] == c.epoch_new ? 1u : 0u) : 2u;
      lk += hit[j] == 0u;
      lh += hit[j] == 1u;
    }
    uint32_t tk, th;
    uint32_t ik = found + wide_excl_scan(lk, ws, &tk);
    uint32_t ih = found_hit + wide_excl_scan(lh, ws, &th);
#pragma unroll
    for (uint32_t j = 0; j < kItems; ++j) {
      if (hit[j] == 0u) { if (ik < want) kept[ik] = sl[j]; ++ik; }
      else if (hit[j] == 1u) { if (ih < want) moved[ih] = sl[j]; ++ih; }
    }
    found += tk;
    found_hit += th;
  }
  if (tid == 0) c.ctr->q_found = min(found, want);
}

// Queue form, between the two kernels, ONE workgroup per context: did the chunks yield enough
// victim candidates?  If not (many dead entries right behind the head) it walks on alone, tile
// by tile, and leaves what it finds as one more chunk (index v_chunks).  Leaves q_found.
__global__ __launch_bounds__(kWide) void lru_queue_walk_kernel(Round r) {
  const Ctx& c = r.c[blockIdx.y];
  if (!c.update || c.policy != GF_CACHE_LRU || !c.qmode) return;
  const int tid = threadIdx.x;
  __shared__ uint32_t ws[kWide / 64];
  const uint32_t want = min(total_miss(c.ctr), c.capacity);
  if (want == 0) return;
  const uint32_t head = c.ctr->q_head, tail = c.ctr->q_tail;
  const uint32_t chunks = victim_chunks_used(c, want);
  uint32_t sum = 0;
  for (uint32_t u = tid; u < chunks; u += kWide) sum += c.v_count[u];
  const uint32_t found0 = wide_sum(sum, ws);
  uint32_t found = found0;
  const uint32_t* list = c.queue[c.ctr->q_parity & 1u];
  const uint32_t limit = want > found0 ? want - found0 : 0u;   // <= block rows: fits behind the chunks
  bool walked = false;
  for (uint32_t base = (head & ~3u) + chunks * kRowTile; base < tail && found < want;
       base += kRowTile) {
    walked = true;
    const uint32_t p0 = base + tid * 4;
    uint32_t sl[4];
    const uint32_t mask = victim_walk4(c, list, head, tail, p0, sl);
    uint32_t total;
    uint32_t at = found - found0 + wide_excl_scan(__popc(mask), ws, &total);
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) {
      if (mask & (1u << j)) {
        if (at < limit) {
          c.v_slot[chunks * kRowTile + at] = sl[j];
          c.v_pos[chunks * kRowTile + at] = p0 + j;
        }
        ++at;
      }
    }
    found += total;
  }
  if (tid == 0) {
    c.v_count[chunks] = min(found - found0, limit);
    c.ctr->q_found = min(found, want);
    if (walked) c.qstate->lone_walks += 1u;
  }
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

// Queue form: applies the update, one thread per block row, kQInst rows per workgroup (many
// small workgroups per CU: every step is a chain of scattered word accesses, which only
// independent workgroups overlap):
//  * the m-th distinct missed id (m < k = min(#distinct misses, capacity, victims found))
//    takes the m-th victim candidate's slot — chunk through the chunk counts' prefix (LDS,
//    binary search), then map / slot_id / row copy as in the list form — and appends the
//    slot's new entry at tail + #hit entries + m; the one with m = k - 1 moves the head behind
//    its victim;
//  * the row that stands for a hit slot (the gather's kRepHit | old position) appends the
//    slot's new entry at tail + (hit entries before the old one) and clears its bitmap word;
//  * old entries die because qpos[] moves on.
constexpr int kQInst = 256;
__global__ __launch_bounds__(kQInst) void lru_queue_install_kernel(Round r) {
  const Ctx& c = r.c[blockIdx.y];
  if (!c.update || c.policy != GF_CACHE_LRU || !c.qmode) return;
  const int tid = threadIdx.x;
  const uint32_t row_chunks = (c.n + kQInst - 1) / kQInst;
  if (blockIdx.x >= row_chunks || total_miss(c.ctr) == 0) return;   // uniform
  __shared__ uint32_t ws[kQInst / 64];
  __shared__ uint32_t s_tpre[kMaxBitGroups];   // hit entries before a group of bitmap tiles
  __shared__ uint32_t s_cpre[kMaxVChunks];     // victim candidates before a chunk
  __shared__ uint2 inst[kQInst];               // {slot, row} installed by this workgroup
  __shared__ int64_t inst_id[kQInst];
  __shared__ uint32_t n_inst;
  const uint32_t cap = c.capacity;
  const uint32_t q_found = c.ctr->q_found, head = c.ctr->q_head, tail = c.ctr->q_tail;
  uint32_t* q = c.queue[c.ctr->q_parity & 1u];
  const uint32_t w_lo = head >> 5, w_hi = (tail + 31u) >> 5;
  const uint32_t t0 = w_lo / kBitTile;
  const uint32_t btiles = (w_hi + kBitTile - 1) / kBitTile - t0;
  const uint32_t G = c.q_group, ngroups = (btiles + G - 1) / G;   // <= kMaxBitGroups
  const uint32_t nchunks = victim_chunks_used(c, min(total_miss(c.ctr), cap)) + 1;   // <= kMaxVChunks
  // every independent load first: the counts of the bitmap tiles (a run of consecutive groups
  // per thread), of the victim chunks (likewise) and of the scan workgroups
  constexpr uint32_t kPerT = kMaxBitGroups / kQInst, kPerC = kMaxVChunks / kQInst;
  uint32_t tv[kPerT], cv[kPerC], tm_part = 0;
  const uint32_t per_t = (ngroups + kQInst - 1) / kQInst, per_c = (nchunks + kQInst - 1) / kQInst;
#pragma unroll
  for (uint32_t j = 0; j < kPerT; ++j) {
    const uint32_t g = tid * per_t + j;
    tv[j] = 0;
    if (j < per_t && g < ngroups)
      for (uint32_t u = g * G; u < min((g + 1) * G, btiles); ++u) tv[j] += c.tile_tie[u];
  }
#pragma unroll
  for (uint32_t j = 0; j < kPerC; ++j) {
    const uint32_t ch = tid * per_c + j;
    cv[j] = (j < per_c && ch < nchunks) ? c.v_count[ch] : 0u;
  }
  const uint32_t row_tiles = (c.n + kLruRows - 1) / kLruRows;
  const uint32_t spans = (row_tiles + c.tiles_per_wg - 1) / c.tiles_per_wg;
  const uint32_t span_rows = c.tiles_per_wg * kLruRows;
  for (uint32_t t = tid; t < spans; t += kQInst) tm_part += c.row_tile_sum[t];
  // exclusive prefixes into LDS: one workgroup scan of the runs' sums each
  uint32_t th, tm, unused;
  {
    uint32_t sum = 0;
#pragma unroll
    for (uint32_t j = 0; j < kPerT; ++j) sum += tv[j];
    uint32_t run = block_excl_scan<kQInst>(sum, ws, &th);
#pragma unroll
    for (uint32_t j = 0; j < kPerT; ++j) {
      const uint32_t g = tid * per_t + j;
      if (j < per_t && g < ngroups) s_tpre[g] = run;
      run += tv[j];
    }
  }
  {
    uint32_t sum = 0;
#pragma unroll
    for (uint32_t j = 0; j < kPerC; ++j) sum += cv[j];
    uint32_t run = block_excl_scan<kQInst>(sum, ws, &unused);
#pragma unroll
    for (uint32_t j = 0; j < kPerC; ++j) {
      const uint32_t ch = tid * per_c + j;
      if (j < per_c && ch < nchunks) s_cpre[ch] = run;
      run += cv[j];
    }
  }
  block_excl_scan<kQInst>(tm_part, ws, &tm);
  const uint32_t k = min(min(tm, cap), q_found);
  if (blockIdx.x == 0 && tid == 0) c.qstate->tail = tail + th + k;   // (head: by the last victim's row)
  for (uint32_t chunk = blockIdx.x; chunk < row_chunks; chunk += gridDim.x) {
    const uint32_t i = chunk * kQInst + tid;
    const bool in = i < c.n;
    const uint32_t code = in ? c.rep_flag[i] : 0u;
    const int64_t id = in ? c.ids[i] : 0;
    const uint32_t w = (chunk * kQInst) / span_rows;   // scan workgroup of these rows
    uint32_t pm_part = 0;
    for (uint32_t t = tid; t < w; t += kQInst) pm_part += c.row_tile_sum[t];
    uint32_t pm;
    block_excl_scan<kQInst>(pm_part, ws, &pm);
    if (tid == 0) n_inst = 0;
    __syncthreads();
    if (code & kRepMiss) {
      const uint32_t m = pm + (code & kRepRank);
      if (m < k) {
        uint32_t lo = 0, hi = nchunks;   // largest chunk with s_cpre[chunk] <= m
        while (hi - lo > 1) {
          const uint32_t mid = (lo + hi) >> 1;
          if (s_cpre[mid] <= m) lo = mid; else hi = mid;
        }
        const uint32_t at = lo * kRowTile + (m - s_cpre[lo]);
        const uint32_t slot = c.v_slot[at];
        const int64_t old = c.slot_id[slot];
        if (m == k - 1) c.qstate->head = c.v_pos[at] + 1u;
        if (old >= 0) c.map[old] = kAbsent;
        c.slot_id[slot] = id;
        c.map[id] = static_cast<int32_t>(slot);
        const uint32_t qa = tail + th + m;   // behind the hit entries, in victim order
        q[qa] = slot;
        c.qpos[slot] = qa;
        const uint32_t j = atomicAdd(&n_inst, 1u);
        inst[j] = make_uint2(slot, i);
        inst_id[j] = id;
      } else {
        c.map[id] = kAbsent;   // "we only cache the first self.capacity", lru_cache.py:127-133
      }
    } else if (code & kRepHit) {
      const uint32_t pos = code & kRepPos, wd = pos >> 5;
      const uint2 sn = c.wsnap[wd];
      const uint32_t slot = static_cast<uint32_t>(c.slot_of_row[i]);
      const uint32_t t = wd / kBitTile - t0, g = t / G;
      uint32_t rank = s_tpre[g] + sn.y + __popc(sn.x & ((1u << (pos & 31u)) - 1u));
      for (uint32_t u = g * G; u < t; ++u) rank += c.tile_tie[u];
      q[tail + rank] = slot;
      c.qpos[slot] = tail + rank;
      c.qbits[wd] = 0u;   // all zero again for the next update (rows sharing a word all store 0)
    }
    __syncthreads();
    // copy the installed rows out of the block's output, as one flat array
    if (c.vec4) {
      copy_installed<float4, 8, kQInst>(c, inst, inst_id, n_inst, c.dimv * 4, tid);
    } else if (c.odd4) {
      copy_installed<uf4, 8, kQInst>(c, inst, inst_id, n_inst, c.dim, tid);
    } else {
      const uint32_t total = c.cache_buf ? n_inst * c.dimv : 0u;
      for (uint32_t f = tid; f < total; f += kQInst) {
        const uint32_t j = f / c.dimv, cc = f - j * c.dimv;
        const uint2 pr = inst[j];
        c.cache_buf[static_cast<uint64_t>(pr.x) * c.dimv + cc] =
            c.inst_from_table ? c.feats[static_cast<uint64_t>(inst_id[j]) * c.dimv + cc]
                              : c.out[static_cast<uint64_t>(pr.y) * c.dimv + cc];
      }
    }
    __syncthreads();
  }
}

// Applies the update; two kinds of workgroups:
//  * row workgroups [0, row_blocks), one thread per block row: the m-th distinct missed id
//    (m < k = min(#distinct misses, capacity)) takes the m-th victim's slot — map / slot_id /
//    row copy from the freshly gathered output; the others give their claim on map[id] back;
//  * list workgroups rewrite the list into the other buffer: with L = not-hit entries ++ hit
//    entries (both in list order), the first k of L are the victims and go, in that order, to
//    the back; everything else moves up by k.  The last one flips the parity.
__global__ __launch_bounds__(kWide) void lru_list_install_kernel(Round r, uint32_t row_blocks,
                                                                 uint32_t list_blocks) {
  const Ctx& c = r.c[blockIdx.y];
  if (!c.update || c.policy != GF_CACHE_LRU || c.fused || c.qmode) return;
  const int tid = threadIdx.x;
  __shared__ uint32_t ws[kWide / 64];
  const uint32_t row_tiles = (c.n + kLruRows - 1) / kLruRows;
  const uint32_t spans = (row_tiles + c.tiles_per_wg - 1) / c.tiles_per_wg;
  const uint32_t cap = c.capacity;
  if (blockIdx.x < row_blocks) {
    // inst_rows block rows per workgroup, one thread each (256 for the usual blocks: ALL kWide
    // threads then copy the installed rows, so the copy of a block's ~thousands of missed rows
    // is spread over n / 256 workgroups; 1024 from 65 536 rows on, where a workgroup's fixed
    // ~10 us of dependent loads — one workgroup fits a CU — would otherwise come n / 256 / 256
    // times in a row)
    __shared__ uint2 inst[kWide];   // {slot, row} installed by this workgroup
    __shared__ int64_t inst_id[kWide];   // ... and the id (the row's place in the table)
    __shared__ uint32_t n_inst;
    __shared__ uint32_t s_keep[kMaxStageTiles], s_hitp[kMaxStageTiles], s_nonhit;
    const uint32_t span_rows = c.tiles_per_wg * kLruRows;
    const uint32_t inst_rows = c.inst_rows;
    const uint32_t chunks = (c.n + inst_rows - 1) / inst_rows;
    for (uint32_t chunk = blockIdx.x; chunk < chunks; chunk += row_blocks) {
      const uint32_t i = chunk * inst_rows + tid;
      const bool in = tid < static_cast<int>(inst_rows) && i < c.n;
      // every independent load first: the row's code and id, the span counts, the record
      const uint32_t code = in ? c.rep_flag[i] : 0u;
      const int64_t id = in ? c.ids[i] : 0;
      const uint32_t w = (chunk * inst_rows) / span_rows;   // scan workgroup of these rows
      uint32_t pm = 0, tm = 0;
      for (uint32_t t = tid; t < spans; t += kWide) {
        const uint32_t m = c.row_tile_sum[t];
        tm += m;
        if (t < w) pm += m;
      }
      const uint32_t q_found = c.ctr->q_found;
      const bool staged = use_staged_victims(c.stage_tiles, total_miss(c.ctr), c.stage_min);
      uint32_t stage_hit = 0, stage_len = 0, th_part = 0;
      if (staged && chunk == blockIdx.x) {
        // list form: hit counts of the tiles that staged their entries, and of the whole list
        if (tid < static_cast<int>(c.stage_tiles)) {
          stage_hit = c.tile_tie[tid];
          stage_len = min(kRowTile, cap - tid * kRowTile);
        }
        const uint32_t groups = ((cap + kRowTile - 1) / kRowTile + kQGroup - 1) / kQGroup;
        for (uint32_t g = tid; g < groups; g += kWide) th_part += c.tile_old[g];
      }
      if (chunk == blockIdx.x && total_miss(c.ctr) == 0) return;   // uniform
      pm = wide_sum(pm, ws);
      tm = wide_sum(tm, ws);
      if (staged && chunk == blockIdx.x) {
        uint32_t unused;
        const uint32_t th = wide_sum(th_part, ws);
        const uint32_t keep_before = wide_excl_scan(stage_len - stage_hit, ws, &unused);
        const uint32_t hit_before = wide_excl_scan(stage_hit, ws, &unused);
        if (tid < static_cast<int>(kMaxStageTiles)) {
          s_keep[tid] = keep_before;
          s_hitp[tid] = hit_before;
        }
        if (tid == 0) s_nonhit = cap - th;
      }
      if (tid == 0) n_inst = 0;
      __syncthreads();
      const uint32_t k = min(tm, cap);
      if (code & kRepMiss) {
        const uint32_t m = pm + (code & kRepRank);
        if (m < k) {
          uint32_t slot;
          int64_t old;
          if (staged) {
            // the m-th entry of (not-hit entries ++ hit entries), both in list order
            const bool keep = m < s_nonhit;
            const uint32_t x = keep ? m : m - s_nonhit;
            const uint32_t* pref = keep ? s_keep : s_hitp;
            uint32_t lo = 0, hi = c.stage_tiles;   // largest tile with pref[tile] <= x
            while (hi - lo > 1) {
              const uint32_t mid = (lo + hi) >> 1;
              if (pref[mid] <= x) lo = mid; else hi = mid;
            }
            const uint32_t at = lo * kRowTile + (x - pref[lo]);
            slot = (keep ? c.v_slot : c.v_pos)[at];
            old = c.slot_id[slot];
          } else {
            slot = m < q_found ? c.rep_row[m] : c.rep_rank[m - q_found];
            old = c.slot_id[slot];
          }
          if (old >= 0) c.map[old] = kAbsent;
          c.slot_id[slot] = id;
          c.map[id] = static_cast<int32_t>(slot);
          const uint32_t at = atomicAdd(&n_inst, 1u);
          inst[at] = make_uint2(slot, i);
          inst_id[at] = id;
        } else {
          c.map[id] = kAbsent;   // "we only cache the first self.capacity", lru_cache.py:127-133
        }
      }
      __syncthreads();
      // copy the installed rows out of the block's output, as one flat array
      const uint32_t total = n_inst * c.dimv;
      if (c.vec4) {
        if (c.inst_rows > kInstRows) copy_installed<float4, 6>(c, inst, inst_id, n_inst, c.dimv * 4, tid);
        else copy_installed<float4, 2>(c, inst, inst_id, n_inst, c.dimv * 4, tid);
      } else if (c.odd4) {
        if (c.inst_rows > kInstRows) copy_installed<uf4, 6>(c, inst, inst_id, n_inst, c.dim, tid);
        else copy_installed<uf4, 2>(c, inst, inst_id, n_inst, c.dim, tid);
      } else {
        for (uint32_t f = tid; c.cache_buf && f < total; f += kWide) {
          const uint32_t j = f / c.dimv, cc = f - j * c.dimv;
          const uint2 pr = inst[j];
          c.cache_buf[static_cast<uint64_t>(pr.x) * c.dimv + cc] =
              c.inst_from_table ? c.feats[static_cast<uint64_t>(inst_id[j]) * c.dimv + cc]
                                : c.out[static_cast<uint64_t>(pr.y) * c.dimv + cc];
        }
      }
      __syncthreads();
    }
    return;
  }
  if (blockIdx.x >= row_blocks + list_blocks) return;
  const uint32_t parity = c.ctr->q_parity;
  const uint32_t* list = c.queue[parity & 1u];
  uint32_t* next = c.queue[(parity & 1u) ^ 1u];
  // A workgroup rewrites SUB-tiles of kWide entries, one per thread (the scan kernel counted
  // the hits per tile of kRowTile = 4 sub-tiles): the rewrite's 2 x capacity scattered stores
  // — next[] nearly dense, qpos[] anywhere — are bound by the address rate of the CUs that
  // issue them, so they are spread over 4 x as many (install 11.7 -> see profiles/ with 33
  // workgroups of 4096 entries on the 134 k-slot cache).
  constexpr uint32_t kSubs = kRowTile / kWide;
  const uint32_t list_tiles = (cap + kRowTile - 1) / kRowTile;
  const uint32_t sub_tiles = (cap + kWide - 1) / kWide;
  const uint32_t groups = (list_tiles + kQGroup - 1) / kQGroup;
  // The first sub-tile's entries are read from BOTH buffers right away, together with the
  // parity word and the counts, and its hit marks (indexed by position: no need to wait for
  // the entries): two dependent hops less on the kernel's critical chain.
  const uint32_t st_first = blockIdx.x - row_blocks;
  uint32_t sl0, tc0;
  {
    const uint32_t p = st_first * kWide + tid;
    const uint32_t a0 = p < cap ? c.queue[0][p] : 0u;
    const uint32_t a1 = p < cap ? c.queue[1][p] : 0u;
    tc0 = p < cap ? c.touched[p] : 0u;
    sl0 = (parity & 1u) ? a1 : a0;
  }
  // #distinct misses and #hit slots of the whole block
  uint32_t tm = 0, th = 0;
  for (uint32_t t = tid; t < spans; t += kWide) tm += c.row_tile_sum[t];
  for (uint32_t g = tid; g < groups; g += kWide) th += c.tile_old[g];
  if (total_miss(c.ctr) == 0) return;   // block without a miss: the list stays as it is
  tm = wide_sum(tm, ws);
  th = wide_sum(th, ws);
  const uint32_t k = min(tm, cap), n_kept = cap - th;
  for (uint32_t st = st_first; st < sub_tiles; st += list_blocks) {
    const uint32_t t = st / kSubs, q = st - t * kSubs;
    const uint32_t p = st * kWide + tid;
    uint32_t sl, tc;
    if (st == st_first) {
      sl = sl0; tc = tc0;
    } else {
      sl = p < cap ? list[p] : 0u;
      tc = p < cap ? c.touched[p] : 0u;
    }
    // hit entries before this sub-tile: whole groups, the tiles of this tile's group, and
    // the sub-tiles of this tile before it (their marks, read densely)
    uint32_t before = 0;
    const uint32_t g0 = t / kQGroup;
    for (uint32_t g = tid; g < g0; g += kWide) before += c.tile_old[g];
    for (uint32_t u = g0 * kQGroup + tid; u < t; u += kWide) before += c.tile_tie[u];
    for (uint32_t j = 0; j < q; ++j) {
      const uint32_t pj = t * kRowTile + j * kWide + tid;   // < p <= cap
      before += (pj < cap && c.touched[pj] == c.epoch_new) ? 1u : 0u;
    }
    const uint32_t hit = (p < cap && tc == c.epoch_new) ? 1u : 0u;
    before = wide_sum(before, ws);
    uint32_t total;
    const uint32_t hb = before + wide_excl_scan(hit, ws, &total);   // hit entries before p
    if (p < cap) {
      const uint32_t l = hit ? n_kept + hb : p - hb;   // index in L
      const uint32_t at = l < k ? cap - k + l : l - k;
      next[at] = sl;
      c.qpos[sl] = at;   // where the next block's hits of this slot leave their mark
    }
  }
  if (blockIdx.x == row_blocks && tid == 0) c.qstate->parity = parity ^ 1u;
}

// ---- LRU list form in ONE launch ----------------------------------------------------------
// lru_list_scan_kernel + lru_list_install_kernel as one launch: what the second launch read
// from the first — counts per tile, the victims at the front of the list — travels between
// workgroups of the SAME launch: counts as 8-byte granules {launch tag, count} (one relaxed
// agent-scope store; the mechanism of merge_slots_fused_kernel, sample_merge.hip), the staged
// victims as write-through (sc1) stores that are drained (s_waitcnt vmcnt(0), workgroup
// barrier) before the tile's granule is published, and read with sc1 loads only
// (MI355X_MICROARCH, inter-workgroup visibility, "valid forms": row 1 of the table).
//
// Three kinds of workgroups, in this order of blockIdx.x — every wait is for a workgroup with
// a LOWER index, which was dispatched earlier:
//  * count  [0, cb)            a tile of kFuseTile list entries: marks read densely (they are
//                              indexed by list position), hits counted; the tiles that can
//                              hold one of the block's victims (those below `want` + hit rows)
//                              stage their not-hit entries packed in list order, each with
//                              the id it holds (the row role then needs no hop through
//                              slot_id[]); publishes {tag, #hits}.  Waits for nobody.
//  * row    [cb, cb + rb)      fuse_rows block rows: representatives of the distinct missed
//                              ids ranked in the span; publishes {tag, #representatives},
//                              looks back over the row workgroups before it (global rank m),
//                              reads every count granule (the m-th entry of not-hit ++ hit
//                              entries = the victim: tile by binary search in LDS, entry from
//                              the staging arrays), installs — map / slot_id / row copy.
//  * write  [cb + rb, …)       a tile of kFuseTile list entries: needs #distinct misses (all
//                              row granules) and the hits before it (count granules), writes
//                              the permuted list into the other buffer and qpos[]; the first
//                              one flips the parity.
// A poll that has not seen its granule after g_fuse_spins (4 096) tries stops waiting and computes the
// value itself from the kernel's immutable inputs (marks, list, claims), so termination does
// not depend on dispatch order (several such launches of different processes sharing the
// GPU can fill an XCD with waiters: DESIGN 6.1).  The one input that is NOT immutable is the
// claim map[id] == -(row + 1) of a representative, which the row role overwrites when it
// installs: a representative therefore first marks slot_of_row[row] = kRepMark (write-through,
// drained) and a recount reads the claim first, the mark second.
constexpr uint32_t kFuseSpinsDefault = 1u << 12;
// (a device word so that a test can force every wait into its recount path:
// GNNFLOW_LRU_FUSE_SPINS, read when the library loads its first cache)
__device__ uint32_t g_fuse_spins = kFuseSpinsDefault;
constexpr int32_t kRepMark = -3;              // slot_of_row[]: representative of a missed id
__device__ unsigned int g_lru_recounts;       // granules a waiter had to recompute itself

#define GF_RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

// Polls up to three granules with all loads in flight per round (a look-back granule and two
// count granules cost one round trip, not three); out[k] = the count, or ~0u for a granule
// that never showed the tag (null pointer: not wanted, 0).
__device__ inline void fuse_poll3(const unsigned long long* g0, const unsigned long long* g1,
                                  const unsigned long long* g2, uint32_t tag, uint32_t* out) {
  const unsigned long long* g[3] = {g0, g1, g2};
  bool need[3], any = false;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    need[k] = g[k] != nullptr;
    out[k] = need[k] ? ~0u : 0u;
    any |= need[k];
  }
  const uint32_t budget = g_fuse_spins;
  for (uint32_t spins = 0; any && spins < budget; ++spins) {
    unsigned long long x[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) x[k] = need[k] ? __hip_atomic_load(g[k], GF_RLX_AGENT) : 0ull;
    any = false;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      if (need[k]) {
        if (static_cast<uint32_t>(x[k] >> 32) == tag) {
          out[k] = static_cast<uint32_t>(x[k]);
          need[k] = false;
        } else {
          any = true;
        }
      }
    }
    if (any) __builtin_amdgcn_s_sleep(1);
  }
#pragma unroll
  for (int k = 0; k < 3; ++k)
    if (need[k]) atomicAdd(&g_lru_recounts, 1u);
}

__device__ inline void fuse_publish(unsigned long long* g, uint32_t tag, uint32_t value) {
  __hip_atomic_store(g, (static_cast<unsigned long long>(tag) << 32) | value, GF_RLX_AGENT);
}

__device__ inline uint32_t total_hits(const Counters* c) {
  uint32_t h = 0;
#pragma unroll
  for (int i = 0; i < kShards; ++i) h += c->shard[i].hits;
  return h;
}

// parity of the list buffer that is current DURING the launch tagged `tag`
__device__ inline uint32_t fuse_parity(const Ctx& c) {
  const unsigned long long w = *reinterpret_cast<const unsigned long long*>(c.qstate);
  const uint32_t parity = static_cast<uint32_t>(w), flip = static_cast<uint32_t>(w >> 32);
  return (flip == c.fuse_tag ? parity ^ 1u : parity) & 1u;
}

// hits in list tile t, from the marks (what a count workgroup publishes)
__device__ inline uint32_t fuse_recount_tile(const Ctx& c, uint32_t t) {
  uint32_t h = 0;
  const uint32_t lo = t * kFuseTile, hi = min(lo + kFuseTile, c.capacity);
  for (uint32_t p = lo; p < hi; ++p) h += c.touched[p] == c.epoch_new ? 1u : 0u;
  return h;
}

// representatives among the rows of row workgroup b (what it publishes)
__device__ inline uint32_t fuse_recount_rows(const Ctx& c, uint32_t b) {
  uint32_t m = 0;
  const uint32_t lo = b * c.fuse_rows, hi = min(lo + c.fuse_rows, c.n);
  for (uint32_t i = lo; i < hi; ++i) {
    const int64_t id = c.ids[i];
    if (id < 0 || static_cast<uint64_t>(id) >= c.num_ids) continue;
    // the claim first, the mark second (see above)
    const int32_t claim = __hip_atomic_load(&c.map[id], GF_RLX_AGENT);
    const int32_t sr = __hip_atomic_load(&c.slot_of_row[i], GF_RLX_AGENT);
    if (sr == kRepMark || (sr == -1 && claim == -static_cast<int32_t>(i + 1))) ++m;
  }
  return m;
}

// the x-th hit (want_hit) / not-hit entry of list tile t, walked serially (fallback of a row
// thread whose tile never published its staged entries)
__device__ inline uint32_t fuse_walk_tile(const Ctx& c, const uint32_t* list, uint32_t t,
                                          uint32_t x, bool want_hit) {
  const uint32_t lo = t * kFuseTile, hi = min(lo + kFuseTile, c.capacity);
  uint32_t seen = 0;
  for (uint32_t p = lo; p < hi; ++p) {
    const bool hit = c.touched[p] == c.epoch_new;
    if (hit == want_hit) {
      if (seen == x) return list[p];
      ++seen;
    }
  }
  return list[lo];   // unreachable: the prefix said the tile has more than x such entries
}

#define GF_STAMP(k) \
  do { if (c.trace && threadIdx.x == 0) c.trace[4 + vx * 8 + (k)] = wall_clock64(); } while (0)

__global__ __launch_bounds__(kWide) void lru_list_fused_kernel(Round r, uint32_t count_blocks,
                                                               uint32_t row_blocks,
                                                               uint32_t write_blocks) {
  // (the roles in THIS order of blockIdx.x — count, row, write — because every wait is for a
  // workgroup dispatched earlier; dispatching the row role, whose chain is the longest, first
  // saved 0.5 us of an isolated launch and cost 7 us per step in the pipelined loop, where the
  // row workgroups then spin for count workgroups that other kernels keep from starting:
  // profiles/README.md, round 6)
  // (the hot fields pinned into SGPRs here: one round of scalar loads instead of one per field
  // where it is first used — see gather_body)
  const Ctx& c = r.c[blockIdx.y];
  asm volatile("" :: "s"(c.update), "s"(c.policy), "s"(c.fused), "s"(c.trace), "s"(c.n),
               "s"(c.capacity), "s"(c.fuse_tag), "s"(c.fuse_rows), "s"(c.touched), "s"(c.queue[0]),
               "s"(c.queue[1]), "s"(c.qstate), "s"(c.ctr), "s"(c.epoch_new), "s"(c.slot_id),
               "s"(c.ids), "s"(c.map), "s"(c.slot_of_row), "s"(c.g_cnt), "s"(c.g_row),
               "s"(c.v_slot), "s"(c.v_old), "s"(c.v_pos), "s"(c.v_hold), "s"(c.qpos),
               "s"(c.num_ids), "s"(c.cache_buf));
  const uint32_t vx = blockIdx.x;
  if (!c.update || c.policy != GF_CACHE_LRU || !c.fused) return;
  const int tid = threadIdx.x;
  if (c.trace && vx == 0 && tid == 0) {
    c.trace[0] = count_blocks; c.trace[1] = row_blocks; c.trace[2] = write_blocks; c.trace[3] = c.fuse_tag;
  }
  GF_STAMP(0);
  __shared__ uint32_t ws[kWide / 64];
  const uint32_t cap = c.capacity, tag = c.fuse_tag;
  const uint32_t tiles = (cap + kFuseTile - 1) / kFuseTile;
  const uint32_t row_wgs = (c.n + c.fuse_rows - 1) / c.fuse_rows;

  if (vx < count_blocks) {
    // ---- count role ----
    bool first = true;
    uint32_t par = 0, bound = 0;
    bool stage_hits = false;
    for (uint32_t t = vx; t < tiles; t += count_blocks) {
      const uint32_t p = t * kFuseTile + tid;
      const bool in = p < cap;
      const uint32_t tc = in ? c.touched[p] : 0u;
      uint32_t sl;
      if (first) {
        // both buffers while the parity word is on its way (one dependent hop less)
        const uint32_t a0 = in ? c.queue[0][p] : 0u;
        const uint32_t a1 = in ? c.queue[1][p] : 0u;
        par = fuse_parity(c);
        const uint32_t missed = total_miss(c.ctr);
        if (missed == 0) return;   // uniform across the launch
        const uint32_t hit_rows = total_hits(c.ctr);
        const uint32_t want = min(missed, cap);
        // the m-th not-hit entry (m < want) lies below list position want + #hit entries
        bound = min(cap, want + hit_rows);
        // victims beyond the not-hit entries: only if misses + hits exceed the capacity
        stage_hits = static_cast<uint64_t>(want) + hit_rows > cap;
        sl = par ? a1 : a0;
        first = false;
      } else {
        sl = in ? c.queue[par][p] : 0u;
      }
      const bool hit = in && tc == c.epoch_new;
      const bool stage = t * kFuseTile < bound;
      if (t == vx) GF_STAMP(1);   // marks, list entries, parity and counters are in
      long long old = -1;
      if (stage && in && (!hit || stage_hits)) old = c.slot_id[sl];
      uint32_t total;
      const uint32_t hb = wide_excl_scan(hit ? 1u : 0u, ws, &total);
      if (stage && in) {
        if (!hit) {
          const uint32_t at = t * kFuseTile + (tid - hb);
          __hip_atomic_store(&c.v_slot[at], sl, GF_RLX_AGENT);
          __hip_atomic_store(&c.v_old[at], old, GF_RLX_AGENT);
        } else if (stage_hits) {
          const uint32_t at = t * kFuseTile + hb;
          __hip_atomic_store(&c.v_pos[at], sl, GF_RLX_AGENT);
          __hip_atomic_store(&c.v_hold[at], old, GF_RLX_AGENT);
        }
      }
      // every storing wave drains its write-through stores, then the barrier, then ONE lane
      // publishes
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      if (tid == 0) fuse_publish(&c.g_cnt[t], tag, total);
      if (t == vx) GF_STAMP(2);   // staged entries drained, count published
    }
    return;
  }

  __shared__ uint32_t s_keep[kFuseMaxTiles + 1], s_hitp[kFuseMaxTiles + 1];
  __shared__ uint32_t s_direct;

  if (vx < count_blocks + row_blocks) {
    // ---- row role ----
    const uint32_t b = vx - count_blocks;
    if (b >= row_wgs) return;
    __shared__ uint2 inst[kWide];        // {slot, row} installed by this workgroup
    __shared__ int64_t inst_id[kWide];
    __shared__ uint32_t n_inst;
    const uint32_t i = b * c.fuse_rows + tid;
    const bool in = tid < static_cast<int>(c.fuse_rows) && i < c.n;
    const int32_t sr = in ? c.slot_of_row[i] : -2;
    const int64_t id = in ? c.ids[i] : 0;
    const uint32_t par = fuse_parity(c);
    if (total_miss(c.ctr) == 0) return;   // uniform
    const bool fm = sr == -1 && c.map[id] == -static_cast<int32_t>(i + 1);
    if (fm) {
      // write-through and DRAINED before this workgroup stores anything else: a recount by
      // another workgroup reads the claim first, the mark second, and must find the mark once
      // the install below has overwritten the claim
      __hip_atomic_store(&c.slot_of_row[i], kRepMark, GF_RLX_AGENT);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    uint32_t cnt;
    const uint32_t rank = wide_excl_scan(fm ? 1u : 0u, ws, &cnt);
    if (tid == 0) {
      fuse_publish(&c.g_row[b], tag, cnt);
      n_inst = 0;
      s_direct = 0;
    }
    GF_STAMP(1);   // rows read (slot_of_row, ids, claims), representatives ranked and published
    // look-back over the row workgroups before this one (at most kFuseMaxRowWgs = kWide: one
    // per thread) and the hits per list tile (two per thread), all in flight together
    constexpr uint32_t kPer = kFuseMaxTiles / kWide;
    static_assert(kPer == 2 && kFuseMaxRowWgs <= kWide, "fuse_poll3: one row + two count granules");
    uint32_t pv[3];
    fuse_poll3(static_cast<uint32_t>(tid) < b ? &c.g_row[tid] : nullptr,
               tid * kPer < tiles ? &c.g_cnt[tid * kPer] : nullptr,
               tid * kPer + 1 < tiles ? &c.g_cnt[tid * kPer + 1] : nullptr, tag, pv);
    if (pv[0] == ~0u) pv[0] = fuse_recount_rows(c, tid);
    GF_STAMP(5);   // thread 0's own granules are in (diagnostics)
    const uint32_t pm = wide_sum(pv[0], ws);
    GF_STAMP(6);   // every thread's are (the sum is a barrier)
    // hits per list tile -> prefix of not-hit / hit entries per tile
    uint32_t hv[kPer], run_h = 0;
#pragma unroll
    for (uint32_t k = 0; k < kPer; ++k) {
      hv[k] = pv[1 + k];
      if (hv[k] == ~0u) {
        hv[k] = fuse_recount_tile(c, tid * kPer + k);
        s_direct = 1u;   // its staged entries may never arrive: walk the tiles instead
      }
      run_h += hv[k];
    }
    uint32_t th;
    uint32_t hb = wide_excl_scan(run_h, ws, &th);
#pragma unroll
    for (uint32_t k = 0; k < kPer; ++k) {
      const uint32_t t = tid * kPer + k;
      if (t <= tiles) {
        s_hitp[t] = hb;
        s_keep[t] = min(t * kFuseTile, cap) - hb;
      }
      hb += hv[k];
    }
    __syncthreads();
    GF_STAMP(2);   // every granule before this workgroup is in, prefixes in LDS
    const uint32_t n_kept = cap - th;
    if (fm) {
      const uint32_t m = pm + rank;
      if (m < cap) {   // "we only cache the first self.capacity", lru_cache.py:127-133
        const bool keep = m < n_kept;
        const uint32_t x = keep ? m : m - n_kept;
        const uint32_t* pref = keep ? s_keep : s_hitp;
        uint32_t lo = 0, hi = tiles;   // largest tile with pref[tile] <= x
        while (hi - lo > 1) {
          const uint32_t mid = (lo + hi) >> 1;
          if (pref[mid] <= x) lo = mid; else hi = mid;
        }
        uint32_t slot;
        long long old;
        if (s_direct) {
          slot = fuse_walk_tile(c, c.queue[par], lo, x - pref[lo], !keep);
          old = c.slot_id[slot];
        } else {
          const uint32_t at = lo * kFuseTile + (x - pref[lo]);
          slot = __hip_atomic_load(keep ? &c.v_slot[at] : &c.v_pos[at], GF_RLX_AGENT);
          old = __hip_atomic_load(keep ? &c.v_old[at] : &c.v_hold[at], GF_RLX_AGENT);
        }
        // (the mark store above has long been drained by the waits in between)
        if (old >= 0) c.map[old] = kAbsent;
        c.slot_id[slot] = id;
        c.map[id] = static_cast<int32_t>(slot);
        const uint32_t at = atomicAdd(&n_inst, 1u);
        inst[at] = make_uint2(slot, i);
        inst_id[at] = id;
      } else {
        c.map[id] = kAbsent;
      }
    }
    __syncthreads();
    GF_STAMP(3);   // victims read, map / slot_id written
    const uint32_t total = n_inst * c.dimv;
    if (c.vec4) {
      if (c.fuse_rows > kInstRows) copy_installed<float4, 6>(c, inst, inst_id, n_inst, c.dimv * 4, tid);
      else copy_installed<float4, 2>(c, inst, inst_id, n_inst, c.dimv * 4, tid);
    } else if (c.odd4) {
      if (c.fuse_rows > kInstRows) copy_installed<uf4, 6>(c, inst, inst_id, n_inst, c.dim, tid);
      else copy_installed<uf4, 2>(c, inst, inst_id, n_inst, c.dim, tid);
    } else {
      for (uint32_t f = tid; c.cache_buf && f < total; f += kWide) {
        const uint32_t j = f / c.dimv, cc = f - j * c.dimv;
        const uint2 pr = inst[j];
        c.cache_buf[static_cast<uint64_t>(pr.x) * c.dimv + cc] =
            c.inst_from_table ? c.feats[static_cast<uint64_t>(inst_id[j]) * c.dimv + cc]
                              : c.out[static_cast<uint64_t>(pr.y) * c.dimv + cc];
      }
    }
    GF_STAMP(4);   // installed rows copied
    return;
  }

  // ---- write role ----
  const uint32_t wb = vx - count_blocks - row_blocks;
  if (wb >= write_blocks || wb >= tiles) return;
  uint32_t sl0, tc0, par;
  {
    const uint32_t p = wb * kFuseTile + tid;
    const uint32_t a0 = p < cap ? c.queue[0][p] : 0u;
    const uint32_t a1 = p < cap ? c.queue[1][p] : 0u;
    tc0 = p < cap ? c.touched[p] : 0u;
    par = fuse_parity(c);
    sl0 = par ? a1 : a0;
  }
  if (total_miss(c.ctr) == 0) return;   // the list stays as it is
  // Stay off the granules' lines for ~2 us: nothing this role waits for is there before, and every
  // poll of a line slows the hand-over of the granules in it down — the row role's look-back, which
  // is the launch's critical path, completes 1.1 us earlier when the 132 write workgroups of the
  // headline's update do not poll beside it (profiles/r06_lru_hop_trace.txt; a longer nap makes
  // the late-dispatched write workgroups the tail instead: 3 / 4 / 5 us: +0.5 / +1.3 / +2.1 us)
  __builtin_amdgcn_s_sleep(32);
  __builtin_amdgcn_s_sleep(32);
  // #distinct misses of the whole block (every row granule) and the hits per tile, all in
  // flight together
  constexpr uint32_t kPer = kFuseMaxTiles / kWide;
  uint32_t pv[3];
  fuse_poll3(static_cast<uint32_t>(tid) < row_wgs ? &c.g_row[tid] : nullptr,
             tid * kPer < tiles ? &c.g_cnt[tid * kPer] : nullptr,
             tid * kPer + 1 < tiles ? &c.g_cnt[tid * kPer + 1] : nullptr, tag, pv);
  if (pv[0] == ~0u) pv[0] = fuse_recount_rows(c, tid);
  const uint32_t tm = wide_sum(pv[0], ws);
  // hits per tile -> hits before every tile
  uint32_t hv[kPer], run_h = 0;
#pragma unroll
  for (uint32_t k = 0; k < kPer; ++k) {
    hv[k] = pv[1 + k];
    if (hv[k] == ~0u) hv[k] = fuse_recount_tile(c, tid * kPer + k);
    run_h += hv[k];
  }
  uint32_t th;
  uint32_t hbt = wide_excl_scan(run_h, ws, &th);
#pragma unroll
  for (uint32_t k = 0; k < kPer; ++k) {
    const uint32_t t = tid * kPer + k;
    if (t <= tiles) s_hitp[t] = hbt;
    hbt += hv[k];
  }
  __syncthreads();
  GF_STAMP(1);   // every row and count granule is in
  const uint32_t k = min(tm, cap), n_kept = cap - th;
  const uint32_t* list = c.queue[par];
  uint32_t* next = c.queue[par ^ 1u];
  for (uint32_t t = wb; t < tiles; t += write_blocks) {
    const uint32_t p = t * kFuseTile + tid;
    uint32_t sl, tc;
    if (t == wb) {
      sl = sl0; tc = tc0;
    } else {
      sl = p < cap ? list[p] : 0u;
      tc = p < cap ? c.touched[p] : 0u;
    }
    const uint32_t hit = (p < cap && tc == c.epoch_new) ? 1u : 0u;
    uint32_t total;
    const uint32_t hb = s_hitp[t] + wide_excl_scan(hit, ws, &total);   // hit entries before p
    if (p < cap) {
      const uint32_t l = hit ? n_kept + hb : p - hb;   // index in (not-hit ++ hit entries)
      const uint32_t at = l < k ? cap - k + l : l - k;
      next[at] = sl;
      c.qpos[sl] = at;   // where the next block's hits of this slot leave their mark
    }
  }
  GF_STAMP(2);   // list tile(s) rewritten
  if (wb == 0 && tid == 0) {
    // {new parity, this launch's tag} in ONE store: fuse_parity() of a late workgroup of this
    // launch still resolves to `par`
    *reinterpret_cast<unsigned long long*>(c.qstate) =
        (static_cast<unsigned long long>(tag) << 32) | (par ^ 1u);
  }
}

// list of a freshly initialised cache: slot order; `prefix` new slots [first, first + prefix)
// go in front of the `old_n` entries of `old` (Cache.resize)
__global__ void list_fill_kernel(uint32_t* list, uint32_t first, uint32_t prefix,
                                 const uint32_t* old, uint32_t old_n) {
  const uint32_t stride = gridDim.x * blockDim.x;
  for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < prefix + old_n; j += stride)
    list[j] = j < prefix ? first + j : old[j - prefix];
}

// ---- LRU as a queue (large caches) --------------------------------------------------------
// The list passes above cost O(capacity) per update: 352 us for a 30 k-row block on a 40 M-slot
// cache (GDELT scale) against 17 us for the gather itself.  From queue_min_capacity() slots on
// (0.5 M), the SAME list is therefore kept as a queue with dead entries: `queue` holds entries
// [head, tail) (capacity * 3/2 allocated), qpos[slot] is the position of the slot's one LIVE
// entry, and an update only appends — the distinct hit slots in the order of their old entries,
// then the k victims, which are the first k live, not-hit entries from the head.  Old entries
// die because qpos[] moves on.  Reading the live entries from head to tail gives exactly the
// list of the list form, so both forms — and the oracle — make the same decisions.
//   gather       : a hit sets the bit of the slot's queue position in `qbits` (atomicOr); the
//                  row whose atomic set it stands for the slot (rep_flag = kRepHit | position).
//                  The hit slots thus come out deduplicated AND in queue order without a sort
//                  (a 7-launch device radix sort cost 35 us here), and nothing else in the
//                  update touches a per-slot hit mark
//   list scan    : row role — representatives of the distinct missed ids, as in the list form;
//                  victim role — chunks of the queue behind the head, one workgroup each, keep
//                  their live, not-hit entries (one scattered load per entry: qpos; the hit
//                  bits are read densely); bitmap role — per tile of kBitTile words (the
//                  bitmap is 1/32 of the queue: 7.5 MB at 40 M slots) the hit entries, per word
//                  a snapshot {word, hits before it in the tile}
//   queue walk   : ONE workgroup: did the chunks yield enough candidates?  If not it walks on
//                  and leaves what it finds as one more chunk
//   queue install: 256-thread workgroups, one thread per block row.  The m-th distinct missed
//                  id takes the m-th victim candidate's slot (chunk through the counts' prefix
//                  in LDS) and appends its entry at tail + hits + m; the row that stands for a
//                  hit slot appends at tail + (hit entries before its old one: tile prefix
//                  from LDS + the snapshot) and clears its bitmap word; head / tail move.
// Every step is O(block rows) and row-parallel: on the GDELT-shaped step (38 M slots, 198 k-
// row blocks) the update costs 108 us per step against 232 with round 4's position-parallel
// append (the non-empty bitmap tiles expanded serially per workgroup); profiles/README.
// When the queue's tail would pass its allocation it is compacted into the other buffer (two
// launches, O(capacity), once per ~capacity / (2 * block rows) updates); a block of more than
// capacity / 4 rows is handled by the list form on the compacted queue (its passes are no
// longer the larger term then) and qpos[] is rebuilt behind it.
struct CompactState { uint32_t parity, tail, pad[2]; };

__global__ __launch_bounds__(kWide) void lru_queue_compact_count_kernel(
    const uint32_t* q0, const uint32_t* q1, const QueueState* qs, const uint32_t* qpos,
    unsigned long long* live_bits, uint32_t* tile_cnt, uint32_t* group_sum, CompactState* st) {
  const int tid = threadIdx.x;
  __shared__ uint32_t ws[kWide / 64];
  const uint32_t parity = qs->parity, tail = qs->tail;
  const uint32_t* q = (parity & 1u) ? q1 : q0;
  if (blockIdx.x == 0 && tid == 0) { st->parity = parity; st->tail = tail; }
  constexpr uint32_t kItems = kRowTile / kWide;
  const uint32_t tiles = (tail + kRowTile - 1) / kRowTile;
  for (uint32_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    uint32_t local = 0;
#pragma unroll
    for (uint32_t j = 0; j < kItems; ++j) {
      const uint32_t p = t * kRowTile + j * kWide + tid;
      bool live = false;
      if (p < tail) live = qpos[q[p]] == p;
      const unsigned long long b = __ballot(live);
      if ((tid & 63) == 0) live_bits[p >> 6] = b;
      local += live ? 1u : 0u;
    }
    const uint32_t total = wide_sum(local, ws);
    if (tid == 0) {
      tile_cnt[t] = total;
      if (total) atomicAdd(&group_sum[t / kQGroup], total);
    }
  }
}

__global__ __launch_bounds__(kWide) void lru_queue_compact_write_kernel(
    uint32_t* q0, uint32_t* q1, QueueState* qs, uint32_t* qpos,
    const unsigned long long* live_bits, const uint32_t* tile_cnt, const uint32_t* group_sum,
    const CompactState* st, uint32_t capacity) {
  const int tid = threadIdx.x;
  __shared__ uint32_t ws[kWide / 64];
  const uint32_t parity = st->parity, tail = st->tail;
  const uint32_t* q = (parity & 1u) ? q1 : q0;
  uint32_t* next = (parity & 1u) ? q0 : q1;
  constexpr uint32_t kItems = kRowTile / kWide;
  const uint32_t tiles = (tail + kRowTile - 1) / kRowTile;
  for (uint32_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    uint32_t before = 0;
    const uint32_t g0 = t / kQGroup;
    for (uint32_t g = tid; g < g0; g += kWide) before += group_sum[g];
    for (uint32_t u = g0 * kQGroup + tid; u < t; u += kWide) before += tile_cnt[u];
    uint32_t run = wide_sum(before, ws);
#pragma unroll
    for (uint32_t j = 0; j < kItems; ++j) {
      const uint32_t p = t * kRowTile + j * kWide + tid;
      const uint32_t live = static_cast<uint32_t>((live_bits[p >> 6] >> (tid & 63)) & 1ull);
      uint32_t total;
      const uint32_t at = run + wide_excl_scan(live, ws, &total);
      if (live) {
        const uint32_t s = q[p];
        next[at] = s;
        qpos[s] = at;
      }
      run += total;
    }
  }
  if (blockIdx.x == 0 && tid == 0) {
    qs->parity = parity ^ 1u;
    qs->head = 0;
    qs->tail = capacity;   // every slot has exactly one live entry
  }
}

// qpos of a dense list (after init, resize, or a list-form update of a queue-capable cache)
__global__ void lru_queue_index_kernel(const uint32_t* q0, const uint32_t* q1,
                                       const QueueState* qs, uint32_t* qpos, uint32_t capacity) {
  const uint32_t* list = (qs->parity & 1u) ? q1 : q0;
  const uint32_t stride = gridDim.x * blockDim.x;
  for (uint32_t p = blockIdx.x * blockDim.x + threadIdx.x; p < capacity; p += stride)
    qpos[list[p]] = p;
}

// Side stream of the calling host thread for rounds that update caches of two forms (created on
// first use only: an extra stream shifts the process's hardware-queue mapping).
struct RoundFork {
  hipStream_t side = nullptr;
  hipEvent_t begin = nullptr, end = nullptr;
  int device = -1;
  ~RoundFork() {
    if (side) (void)hipStreamDestroy(side);
    if (begin) (void)hipEventDestroy(begin);
    if (end) (void)hipEventDestroy(end);
  }
};
inline RoundFork& round_fork() {
  static thread_local RoundFork f;
  return f;
}
inline bool fork_round(hipStream_t stream, hipStream_t* side) {
  RoundFork& f = round_fork();
  int dev = 0;
  GF_HIP(hipGetDevice(&dev));
  if (f.side && f.device != dev) return false;   // one device per host thread in practice
  if (!f.side) {
    GF_HIP(hipStreamCreateWithFlags(&f.side, hipStreamNonBlocking));
    GF_HIP(hipEventCreateWithFlags(&f.begin, hipEventDisableTiming));
    GF_HIP(hipEventCreateWithFlags(&f.end, hipEventDisableTiming));
    f.device = dev;
  }
  GF_HIP(hipEventRecord(f.begin, stream));
  GF_HIP(hipStreamWaitEvent(f.side, f.begin, 0));
  *side = f.side;
  return true;
}
inline void fork_done() { GF_HIP(hipEventRecord(round_fork().end, round_fork().side)); }
inline void join_round(hipStream_t stream) { GF_HIP(hipStreamWaitEvent(stream, round_fork().end, 0)); }

}  // namespace

void launch_lru_update(const Round& r, hipStream_t stream, bool own_events) {
  size_t q_scan_blocks = 0, q_rows = 0, q_cap = 0, q_bit_tiles = 0, q_victim_blocks = 1;
  size_t q_inst_blocks = 0, qq_rows = 0;
  size_t f_tiles = 0, f_rows = 0;
  bool forked = false;
  hipStream_t side = nullptr;
  for (int i = 0; i < r.count; ++i) {
    const Ctx& c = r.c[i];
    if (!c.update || c.policy != GF_CACHE_LRU) continue;
    if (c.fused) {
      f_tiles = std::max<size_t>(f_tiles, (c.capacity + kFuseTile - 1) / kFuseTile);
      f_rows = std::max<size_t>(f_rows, (c.n + c.fuse_rows - 1) / c.fuse_rows);
    } else {
      const size_t row_tiles = (c.n + kLruRows - 1) / kLruRows;
      q_scan_blocks = std::max(q_scan_blocks, (row_tiles + c.tiles_per_wg - 1) / c.tiles_per_wg);
      q_rows = std::max<size_t>(q_rows, c.n);
      if (c.qmode) {
        // queue form: bitmap tiles of kBitTile words (32 queue positions per word; the tail
        // is below 1.5 * capacity + 64)
        const size_t bit_tiles = ((size_t{c.capacity} * 3 / 2 + 128) / 32 + kBitTile - 1) / kBitTile + 1;
        q_bit_tiles = std::max(q_bit_tiles, bit_tiles);
        q_victim_blocks = std::max<size_t>(q_victim_blocks, std::min<size_t>(c.v_chunks, 1024));
        qq_rows = std::max<size_t>(qq_rows, c.n);
      } else {
        q_cap = std::max<size_t>(q_cap, c.capacity);
        q_inst_blocks = std::max<size_t>(q_inst_blocks, (c.n + c.inst_rows - 1) / c.inst_rows);
      }
    }
  }
  if (f_tiles) {   // LRU list form, one launch
    const unsigned cb = static_cast<unsigned>(std::min<size_t>(f_tiles, 1024));
    const unsigned rb = static_cast<unsigned>(std::max<size_t>(f_rows, 1));
    const unsigned wb = static_cast<unsigned>(std::min<size_t>(f_tiles, kFuseMaxTiles));
    // a round that also carries a queue-form (or two-launch) update — a small node cache beside a
    // GDELT-scale edge cache — runs this launch on a side stream, beside those launches: the
    // contexts are different caches, and both chains are bound by dependent accesses, not by CUs
    forked = q_rows != 0 && fork_round(stream, &side);
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (own_events && profile_begin(kProfLru, &e0, &e1)) {
      hipExtLaunchKernelGGL(lru_list_fused_kernel, dim3(cb + rb + wb, r.count), dim3(kWide), 0, stream,
                            e0, e1, 0, r, cb, rb, wb);
      profile_end(kProfLru, e0, e1);
    } else {
      lru_list_fused_kernel<<<dim3(cb + rb + wb, r.count), dim3(kWide), 0, forked ? side : stream>>>(
          r, cb, rb, wb);
    }
    GF_HIP(hipGetLastError());
    if (forked) fork_done();
  }
  if (q_rows) {   // LRU: list scan + list install
    const unsigned rb = static_cast<unsigned>(q_scan_blocks);
    // list workgroups: per kRowTile list entries of the list-form contexts (none: queue form
    // only); the install kernel's also append for the queue-form contexts
    const unsigned lb_list = static_cast<unsigned>(
        std::min<size_t>(std::max((q_cap + kRowTile - 1) / kRowTile, q_bit_tiles), 1024));
    // install: sub-tiles of kWide list entries per workgroup for the list-form contexts
    const unsigned lb_sub = static_cast<unsigned>(std::min<size_t>((q_cap + kWide - 1) / kWide, 1024));
    const unsigned lb = std::max<unsigned>(1, lb_sub);
    const unsigned vb = static_cast<unsigned>(q_victim_blocks);
    lru_list_scan_kernel<<<dim3(rb + lb_list + vb, r.count), dim3(kWide), 0, stream>>>(
        r, rb, lb_list, vb);
    if (q_bit_tiles) {
      lru_queue_walk_kernel<<<dim3(1, r.count), dim3(kWide), 0, stream>>>(r);
      const unsigned qb = static_cast<unsigned>(
          std::max<size_t>(1, std::min<size_t>((qq_rows + kQInst - 1) / kQInst, 16384)));
      lru_queue_install_kernel<<<dim3(qb, r.count), dim3(kQInst), 0, stream>>>(r);
    }
    if (q_inst_blocks) {
      const unsigned ib = static_cast<unsigned>(std::min<size_t>(q_inst_blocks, 4096));
      lru_list_install_kernel<<<dim3(ib + lb, r.count), dim3(kWide), 0, stream>>>(r, ib, lb);
    }
    GF_HIP(hipGetLastError());
    if (forked) join_round(stream);
  }
}

// GNNFLOW_LRU_FUSE_SPINS (tests): the polls' budget before a waiter recomputes the value
// itself — 0 sends EVERY look-back of the one-launch LRU update through its fallback
void lru_fuse_spins_from_env(int device) {
  static std::mutex mu;
  static std::vector<int> done;
  std::lock_guard<std::mutex> lk(mu);
  if (std::find(done.begin(), done.end(), device) == done.end()) {
    done.push_back(device);
    if (const char* v = std::getenv("GNNFLOW_LRU_FUSE_SPINS")) {
      const uint32_t spins = static_cast<uint32_t>(std::atoll(v));
      GF_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_fuse_spins), &spins, sizeof(spins)));
    }
  }
}

void lru_list_fill(uint32_t* list, uint32_t first, uint32_t prefix, const uint32_t* old,
                   uint32_t old_n, hipStream_t stream) {
  list_fill_kernel<<<dim3(1024), dim3(256), 0, stream>>>(list, first, prefix, old, old_n);
  GF_HIP(hipGetLastError());
}

// ---- LRU list, host side -----------------------------------------------------------------
// slot order: the order of a freshly initialised cache (every `count` equal)
void FeatureCache::init_queue(hipStream_t stream) {
  if (policy_ != GF_CACHE_LRU) return;
  queue_form_ = capacity_ >= queue_min_capacity();
  queue_cap_ = queue_form_ ? capacity_ + capacity_ / 2 + 64 : capacity_;
  const size_t bytes = (queue_cap_ + 16) * sizeof(uint32_t);   // + one 16-byte vector past the end
  queue_.reserve(bytes, 0, stream);
  queue_alt_.reserve(bytes, 0, stream);
  if (capacity_) {
    list_fill_kernel<<<dim3(1024), dim3(256), 0, stream>>>(
        queue_.as<uint32_t>(), 0u, static_cast<uint32_t>(capacity_), nullptr, 0u);
    GF_HIP(hipGetLastError());
  }
  const QueueState qs{0u, 0u, 0u, static_cast<uint32_t>(capacity_), 0u, 0u};
  GF_HIP(hipMemcpyAsync(qstate_.data(), &qs, sizeof(qs), hipMemcpyHostToDevice, stream));
  GF_HIP(hipStreamSynchronize(stream));   // qs is a stack variable
  tail_bound_ = capacity_;
  qpos_.reserve(std::max<size_t>(capacity_, 4) * sizeof(uint32_t), 0, stream);
  if (queue_form_) {
    GF_REQUIRE(queue_cap_ < (size_t{1} << 30), "LRU queue form: more than 2^30 queue positions");
    wsnap_.reserve(2 * qbits_bytes(queue_cap_), 0, stream);
    qbits_.reserve(qbits_bytes(queue_cap_), 0, stream);
    GF_HIP(hipMemsetAsync(qbits_.data(), 0, qbits_bytes(queue_cap_), stream));
    const size_t tiles = (queue_cap_ + kRowTile - 1) / kRowTile + 1;
    const size_t groups = (tiles + kQGroup - 1) / kQGroup + 1;
    compact_.reserve(align_up(tiles * (kRowTile / 64) * 8, 256) + align_up(tiles * 4, 256) +
                     align_up(groups * 4, 256) + 256, 0, stream);
  } else {
    wsnap_.release();
    qbits_.release();
    compact_.release();
  }
  index_queue(stream);
}

// qpos[] of a dense list
void FeatureCache::index_queue(hipStream_t stream) {
  if (!capacity_) return;
  lru_queue_index_kernel<<<dim3(2048), dim3(256), 0, stream>>>(
      queue_.as<uint32_t>(), queue_alt_.as<uint32_t>(), qstate_.as<QueueState>(),
      qpos_.as<uint32_t>(), static_cast<uint32_t>(capacity_));
  GF_HIP(hipGetLastError());
}

// Queue form: drops the dead entries (dense list in the other buffer, head = 0, tail = capacity)
void FeatureCache::compact_queue(hipStream_t stream) {
  if (!queue_form_ || tail_bound_ == capacity_) return;
  const size_t tiles = (tail_bound_ + kRowTile - 1) / kRowTile;
  const size_t groups = (tiles + kQGroup - 1) / kQGroup;
  char* p = compact_.as<char>();
  auto* live_bits = reinterpret_cast<unsigned long long*>(p);
  p += align_up(((queue_cap_ + kRowTile - 1) / kRowTile + 1) * (kRowTile / 64) * 8, 256);
  auto* tile_cnt = reinterpret_cast<uint32_t*>(p);
  p += align_up(((queue_cap_ + kRowTile - 1) / kRowTile + 1) * 4, 256);
  auto* group_sum = reinterpret_cast<uint32_t*>(p);
  p += align_up((((queue_cap_ + kRowTile - 1) / kRowTile + 1 + kQGroup - 1) / kQGroup + 1) * 4, 256);
  auto* st = reinterpret_cast<CompactState*>(p);
  GF_HIP(hipMemsetAsync(group_sum, 0, groups * 4, stream));
  const unsigned grid = static_cast<unsigned>(std::max<size_t>(1, std::min<size_t>(tiles, 2048)));
  lru_queue_compact_count_kernel<<<dim3(grid), dim3(kWide), 0, stream>>>(
      queue_.as<uint32_t>(), queue_alt_.as<uint32_t>(), qstate_.as<QueueState>(),
      qpos_.as<uint32_t>(), live_bits, tile_cnt, group_sum, st);
  lru_queue_compact_write_kernel<<<dim3(grid), dim3(kWide), 0, stream>>>(
      queue_.as<uint32_t>(), queue_alt_.as<uint32_t>(), qstate_.as<QueueState>(),
      qpos_.as<uint32_t>(), live_bits, tile_cnt, group_sum, st,
      static_cast<uint32_t>(capacity_));
  GF_HIP(hipGetLastError());
  tail_bound_ = capacity_;
  ++compactions_;
}

// Granules of the fused LRU list update that did not arrive within the polling budget and were
// recomputed by the waiting thread (since the library was loaded, current device).
uint64_t lru_recounts() {
  unsigned int v = 0;
  GF_HIP(hipMemcpyFromSymbol(&v, HIP_SYMBOL(g_lru_recounts), sizeof(v)));
  return v;
}

}  // namespace gf
