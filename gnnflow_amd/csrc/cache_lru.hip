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
// reference leaves it to torch.topk's unspecified tie-breaking).
// Three forms of that one update, one translation unit each around cache_lru_dev.hpp:
//   cache_lru_fused.hip  the list form in ONE launch (lru_list_fused_kernel), where its LDS
//                        tables fit: the default for caches below 0.5 M slots
//   cache_lru.hip        (this file) the list form in two launches, for lists beyond the fused
//                        kernel's tables and with GNNFLOW_LRU_FUSED=0:
//     list scan   : row-tile workgroups rank the representatives of the distinct missed ids;
//                   list-tile workgroups count the hit slots per tile of the list; one more
//                   workgroup reads the victims off the front of the list.
//     list install: one thread per block row installs the m-th missed id in the m-th victim's
//                   slot (map / slot_id / row copy from the freshly gathered output — spread
//                   over as many workgroups as the block has rows); list-tile workgroups write
//                   the permuted list into the other buffer.
//   cache_lru_queue.hip  a cache of 0.5 M slots or more keeps the same list as a queue ("LRU as
//                        a queue" there): the list scan, then its own walk and install
// This file also holds what the forms share on the host: launch_lru_update, which sends every
// context of a round to its form, and the FeatureCache members that size, fill and index the
// list buffers and fill the LRU part of a context.  (The buffer sizes themselves:
// feature_cache_ctx.hpp, lru_queue_cap() and what follows it.)
// All kernels return at once for a context whose block had no miss (the reference skips
// update_*_cache then too, cache.py:318); a hit only changes replacement state if the block
// also had a miss, exactly as in the reference.
#include "cache_lru_dev.hpp"

#include <algorithm>

namespace gf {

namespace {

// ---- LRU as a list ------------------------------------------------------------------
// (see the file header).  c.touched[slot] = epoch of the slot's last hit (plain stores by the
// gather); c.queue[0 / 1] are the two list buffers, qstate->parity says which one is current.

// The FIRST launch of both the two-launch list form (lru_list_install_kernel follows) and the
// queue form (its c.qmode branches; lru_queue_walk_kernel and lru_queue_install_kernel of
// cache_lru_queue.hip follow).
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

// list of a freshly initialised cache: slot order; `prefix` new slots [first, first + prefix)
// go in front of the `old_n` entries of `old` (Cache.resize)
__global__ void list_fill_kernel(uint32_t* list, uint32_t first, uint32_t prefix,
                                 const uint32_t* old, uint32_t old_n) {
  const uint32_t stride = gridDim.x * blockDim.x;
  for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < prefix + old_n; j += stride)
    list[j] = j < prefix ? first + j : old[j - prefix];
}
void lru_list_fill(uint32_t* list, uint32_t first, uint32_t prefix, const uint32_t* old,
                   uint32_t old_n, hipStream_t stream) {
  list_fill_kernel<<<dim3(1024), dim3(256), 0, stream>>>(list, first, prefix, old, old_n);
  GF_HIP(hipGetLastError());
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

// What launch_lru_update sizes the grids from: per form, the largest extent over the round's
// LRU contexts (every launch takes the whole round; blockIdx.y selects the context, and the
// workgroups beyond a smaller context's extent return at once).
struct LruExtents {
  // list form in one launch (c.fused)
  size_t fused_list_tiles = 0;   // tiles of kFuseTile list entries; 0: no such context
  size_t fused_row_wgs = 0;      // row workgroups, of c.fuse_rows block rows
  // every other context, list or queue form: lru_list_scan_kernel
  size_t scan_rows = 0;          // block rows; 0: no such context
  size_t scan_row_wgs = 0;       // row workgroups, of c.tiles_per_wg tiles of kLruRows block rows
  // ... of them the list form: lru_list_install_kernel
  size_t list_capacity = 0;      // entries of the longest list
  size_t list_inst_wgs = 0;      // install workgroups, of c.inst_rows block rows; 0: no such context
  // ... and the queue form (c.qmode): lru_queue_walk_kernel, lru_queue_install_kernel
  size_t queue_bit_tiles = 0;    // tiles of the hit bitmap; 0: no such context
  size_t queue_victim_wgs = 1;   // workgroups of the scan's victim walk behind the head
  size_t queue_rows = 0;         // block rows
};

LruExtents lru_extents(const Round& r) {
  LruExtents x;
  for (int i = 0; i < r.count; ++i) {
    const Ctx& c = r.c[i];
    if (!c.update || c.policy != GF_CACHE_LRU) continue;
    if (c.fused) {
      x.fused_list_tiles = std::max<size_t>(x.fused_list_tiles, (c.capacity + kFuseTile - 1) / kFuseTile);
      x.fused_row_wgs = std::max<size_t>(x.fused_row_wgs, (c.n + c.fuse_rows - 1) / c.fuse_rows);
      continue;
    }
    const size_t row_tiles = (c.n + kLruRows - 1) / kLruRows;
    x.scan_rows = std::max<size_t>(x.scan_rows, c.n);
    x.scan_row_wgs = std::max(x.scan_row_wgs, (row_tiles + c.tiles_per_wg - 1) / c.tiles_per_wg);
    if (c.qmode) {
      x.queue_bit_tiles = std::max(x.queue_bit_tiles, lru_bit_tiles(c.capacity));
      x.queue_victim_wgs = std::max<size_t>(x.queue_victim_wgs, std::min<size_t>(c.v_chunks, 1024));
      x.queue_rows = std::max<size_t>(x.queue_rows, c.n);
    } else {
      x.list_capacity = std::max<size_t>(x.list_capacity, c.capacity);
      x.list_inst_wgs = std::max<size_t>(x.list_inst_wgs, (c.n + c.inst_rows - 1) / c.inst_rows);
    }
  }
  return x;
}

void launch_list_scan(const Round& r, const LruExtents& x, hipStream_t stream) {
  const unsigned rb = static_cast<unsigned>(x.scan_row_wgs);
  // list workgroups: per kRowTile list entries of the list-form contexts, per bitmap tile of
  // the queue-form contexts
  const unsigned lb = static_cast<unsigned>(std::min<size_t>(
      std::max((x.list_capacity + kRowTile - 1) / kRowTile, x.queue_bit_tiles), 1024));
  const unsigned vb = static_cast<unsigned>(x.queue_victim_wgs);
  lru_list_scan_kernel<<<dim3(rb + lb + vb, r.count), dim3(kWide), 0, stream>>>(r, rb, lb, vb);
}

void launch_list_install(const Round& r, const LruExtents& x, hipStream_t stream) {
  const unsigned ib = static_cast<unsigned>(std::min<size_t>(x.list_inst_wgs, 4096));
  // list workgroups: sub-tiles of kWide list entries each
  const unsigned lb = std::max<unsigned>(
      1, static_cast<unsigned>(std::min<size_t>((x.list_capacity + kWide - 1) / kWide, 1024)));
  lru_list_install_kernel<<<dim3(ib + lb, r.count), dim3(kWide), 0, stream>>>(r, ib, lb);
}

}  // namespace

void launch_lru_update(const Round& r, hipStream_t stream, bool own_events) {
  const LruExtents x = lru_extents(r);
  // A round that carries a one-launch update AND a queue-form (or two-launch) one — a small node
  // cache beside a GDELT-scale edge cache — runs the one launch on a side stream, beside the
  // others: the contexts are different caches, and both chains are bound by dependent accesses,
  // not by CUs
  hipStream_t side = nullptr;
  const bool forked = x.fused_list_tiles && x.scan_rows && fork_round(stream, &side);
  if (x.fused_list_tiles) {
    launch_lru_fused(r, x.fused_list_tiles, x.fused_row_wgs, forked ? side : stream, own_events);
    if (forked) fork_done();
  }
  if (x.scan_rows) {
    launch_list_scan(r, x, stream);
    if (x.queue_bit_tiles) launch_lru_queue_update(r, x.queue_rows, stream);
    if (x.list_inst_wgs) launch_list_install(r, x, stream);
    GF_HIP(hipGetLastError());
    if (forked) join_round(stream);
  }
}

// ---- LRU list, host side -----------------------------------------------------------------
// Decides the form of a cache of `capacity` slots and reserves every buffer of its list (the
// sizes: feature_cache_ctx.hpp).  The list's contents, qstate and qpos[] are the caller's.
// old_lists == nullptr (init_queue): the buffers only ever grow, and the list form gives the
// queue-only ones back.  Else (resize): every buffer is a fresh allocation, and the two list
// buffers in use until now are handed to the caller, who still reads the current one.
void FeatureCache::alloc_queue(size_t capacity, hipStream_t stream, DeviceBuffer* old_lists) {
  const bool queue_form = capacity >= queue_min_capacity();
  const size_t queue_cap = lru_queue_cap(capacity, queue_form);
  GF_REQUIRE(!queue_form || queue_cap < (size_t{1} << 30),
             "LRU queue form: more than 2^30 queue positions");
  queue_form_ = queue_form;
  queue_cap_ = queue_cap;
  if (old_lists) {
    old_lists[0] = std::move(queue_);
    old_lists[1] = std::move(queue_alt_);
  }
  auto place = [&](DeviceBuffer& buf, size_t bytes) {
    if (!old_lists) {
      buf.reserve(bytes, 0, stream);
    } else {
      DeviceBuffer fresh;
      fresh.reserve(bytes);
      std::swap(buf, fresh);
    }
  };
  const size_t list_bytes = (queue_cap_ + 16) * sizeof(uint32_t);   // + one 16-byte vector past the end
  place(queue_, list_bytes);
  place(queue_alt_, list_bytes);
  place(qpos_, std::max<size_t>(capacity, 4) * sizeof(uint32_t));
  if (queue_form_) {
    place(wsnap_, 2 * qbits_bytes(queue_cap_));
    place(qbits_, qbits_bytes(queue_cap_));
    GF_HIP(hipMemsetAsync(qbits_.data(), 0, qbits_bytes(queue_cap_), stream));
    place(compact_, compact_layout(queue_cap_).bytes);
  } else if (!old_lists) {
    wsnap_.release();
    qbits_.release();
    compact_.release();
  }
}

// slot order: the order of a freshly initialised cache (every `count` equal)
void FeatureCache::init_queue(hipStream_t stream) {
  if (policy_ != GF_CACHE_LRU) return;
  alloc_queue(capacity_, stream, nullptr);
  if (capacity_) lru_list_fill(queue_.as<uint32_t>(), 0u, static_cast<uint32_t>(capacity_), nullptr, 0u, stream);
  const QueueState qs{0u, 0u, 0u, static_cast<uint32_t>(capacity_), 0u, 0u};
  GF_HIP(hipMemcpyAsync(qstate_.data(), &qs, sizeof(qs), hipMemcpyHostToDevice, stream));
  GF_HIP(hipStreamSynchronize(stream));   // qs is a stack variable
  tail_bound_ = capacity_;
  index_queue(stream);
}

// Cache.resize: the new (empty) slots [old_capacity, capacity_) are the first to be refilled, in
// slot order: they go to the front of the list, the old entries follow in their order
void FeatureCache::grow_queue(size_t old_capacity, hipStream_t stream) {
  QueueState qs;
  GF_HIP(hipMemcpyAsync(&qs, qstate_.data(), sizeof(qs), hipMemcpyDeviceToHost, stream));
  GF_HIP(hipStreamSynchronize(stream));
  DeviceBuffer old_lists[2];   // read by the fill below, freed on return
  alloc_queue(capacity_, stream, old_lists);
  lru_list_fill(queue_.as<uint32_t>(), static_cast<uint32_t>(old_capacity),
                static_cast<uint32_t>(capacity_ - old_capacity), old_lists[qs.parity & 1u].as<uint32_t>(),
                static_cast<uint32_t>(old_capacity), stream);
  const QueueState fresh{0u, 0u, 0u, static_cast<uint32_t>(capacity_), 0u, 0u};
  GF_HIP(hipMemcpyAsync(qstate_.data(), &fresh, sizeof(fresh), hipMemcpyHostToDevice, stream));
  GF_HIP(hipStreamSynchronize(stream));
  tail_bound_ = capacity_;
  index_queue(stream);
  GF_HIP(hipStreamSynchronize(stream));
}

// qpos[] of a dense list
void FeatureCache::index_queue(hipStream_t stream) {
  if (!capacity_) return;
  launch_lru_queue_index(queue_.as<uint32_t>(), queue_alt_.as<uint32_t>(), qstate_.as<QueueState>(),
                         qpos_.as<uint32_t>(), static_cast<uint32_t>(capacity_), stream);
}

// Queue form: drops the dead entries (dense list in the other buffer, head = 0, tail = capacity)
void FeatureCache::compact_queue(hipStream_t stream) {
  if (!queue_form_ || tail_bound_ == capacity_) return;
  launch_lru_queue_compact(queue_.as<uint32_t>(), queue_alt_.as<uint32_t>(),
                           qstate_.as<QueueState>(), qpos_.as<uint32_t>(), compact_.as<char>(),
                           compact_layout(queue_cap_), tail_bound_,
                           static_cast<uint32_t>(capacity_), stream);
  tail_bound_ = capacity_;
  ++compactions_;
}

namespace {
inline bool lru_fused_enabled() {
  const char* e = std::getenv("GNNFLOW_LRU_FUSED");   // 0: list scan + list install (A/B, tests)
  return e ? std::atoi(e) != 0 : true;
}
}  // namespace

// The LRU part of the context of a block fetch with update (FeatureCache::prepare): picks the
// form of this update and lays the LRU scratch out behind the common arrays of the workspace
// (`qscratch`; reserve_workspace sized it).  Schedules a queue compaction when one is due.
void FeatureCache::fill_lru_ctx(Ctx& c, size_t n, char* qscratch, hipStream_t stream) {
  const size_t row_tiles = (n + kLruRows - 1) / kLruRows;
  c.tiles_per_wg = static_cast<uint32_t>((row_tiles + kMaxRowTiles - 1) / kMaxRowTiles);
  c.inst_rows = n >= 65536 ? kWide : kInstRows;
  c.queue[0] = queue_.as<uint32_t>();
  c.queue[1] = queue_alt_.as<uint32_t>();
  c.qstate = qstate_.as<QueueState>();
  {
    const size_t stage = align_up(stage_entries(ws_rows_, capacity_) * 4, 256);
    c.v_slot = reinterpret_cast<uint32_t*>(qscratch);
    c.v_pos = reinterpret_cast<uint32_t*>(qscratch + stage);
    c.v_count = reinterpret_cast<uint32_t*>(qscratch + 2 * stage);
    const size_t vc = align_up((victim_chunks(ws_rows_) + 2) * 4, 256) + 256;
    const size_t fst = align_up(fuse_stage_entries(ws_rows_, capacity_) * 8, 256);
    c.v_old = reinterpret_cast<long long*>(qscratch + 2 * stage + vc);
    c.v_hold = reinterpret_cast<long long*>(qscratch + 2 * stage + vc + fst);
    // list form: the tiles at the front of the list that stage their entries
    const size_t list_tiles = (capacity_ + kRowTile - 1) / kRowTile;
    const size_t st = std::min(list_tiles, (2 * n + kRowTile - 1) / kRowTile + 2);
    // more tiles than kMaxStageTiles (the install kernel keeps the tile prefix in LDS): the
    // one-workgroup walk
    c.stage_tiles = st <= kMaxStageTiles ? static_cast<uint32_t>(st) : 0u;
    c.stage_min = kStageMinWant;
    c.stage_hits = st == list_tiles ? 1 : 0;
  }
  c.qpos = qpos_.as<uint32_t>();
  if (queue_form_) {
    if (n <= capacity_ / 4 && victim_chunks(n) + 1 <= kMaxVChunks) {
      // appends at most n entries (#distinct hit slots + #victims <= rows)
      if (tail_bound_ + n > queue_cap_) compact_queue(stream);
      tail_bound_ += n;
      c.qmode = 1;
      c.qbits = qbits_.as<uint32_t>();
      c.wsnap = wsnap_.as<uint2>();
      c.q_group = static_cast<uint32_t>((lru_bit_tiles(capacity_) + kMaxBitGroups - 1) / kMaxBitGroups);
      static const uint32_t forced_group = [] {
        const char* e = std::getenv("GNNFLOW_LRU_QUEUE_GROUP");   // tests: the > 89 M-slot path
        return e ? static_cast<uint32_t>(std::atoi(e)) : 0u;
      }();
      c.q_group = std::max(c.q_group, forced_group);
      c.v_chunks = static_cast<uint32_t>(victim_chunks(n));
      c.stage_tiles = 0;
    } else {
      // a block this large is cheaper in the list form, on the dense list (whose install
      // leaves qpos[] = the new list positions, which is what the queue form expects)
      compact_queue(stream);
      ++list_form_updates_;
    }
  }
  // list form in one launch (lru_list_fused_kernel) where its LDS tables and granule arrays fit
  // 256 block rows per row workgroup while that gives <= kFuseMaxRowWgs of them: the rows a
  // small cache installs belong to the FIRST representatives, i.e. to the first few row
  // workgroups, which then copy all of its rows (GDELT-scale node cache, 3 336 slots, 218 k-row
  // blocks: 57 us per update with 1 024 rows per workgroup — four workgroups copied 5.5 MB)
  // Without a row mirror nothing is copied, and 1 024 rows per workgroup keep the launch small
  // enough for every count and row workgroup to be resident from the start (1 024-thread
  // workgroups: one per CU; with 256 rows the headline's row workgroups entered 2.6 us into the
  // launch, behind the count workgroups — profiles/r06_lru_hop_trace.txt).
  c.fuse_rows = (n > size_t{kInstRows} * kFuseMaxRowWgs || !mirror_) ? kWide : kInstRows;
  if (!c.qmode && lru_fused_enabled() &&
      (capacity_ + kFuseTile - 1) / kFuseTile <= kFuseMaxTiles &&
      (n + c.fuse_rows - 1) / c.fuse_rows <= kFuseMaxRowWgs) {
    if (!granules_.data()) {
      granules_.reserve((kFuseMaxTiles + kFuseMaxRowWgs) * sizeof(unsigned long long), 0, stream);
      GF_HIP(hipMemsetAsync(granules_.data(), 0, granules_.bytes(), stream));
    }
    if (fuse_tag_ == 0xFFFFFFFFu) {   // the tags wrap: no granule may carry one from last time round
      GF_HIP(hipMemsetAsync(granules_.data(), 0, granules_.bytes(), stream));
      fuse_tag_ = 0;
    }
    c.fused = 1;
    c.trace = trace_.data() ? trace_.as<unsigned long long>() : nullptr;
    c.fuse_tag = ++fuse_tag_;
    c.g_cnt = granules_.as<unsigned long long>();
    c.g_row = c.g_cnt + kFuseMaxTiles;
  }
}

}  // namespace gf
