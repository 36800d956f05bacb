// The LRU list update in ONE launch (overview of the LRU units: cache_lru.hip): the only code of
// the library whose workgroups wait for each other.  Everything its protocol consists of is in
// this file — the granules, the polls and their budget (g_fuse_spins), the fallbacks that
// recompute a granule and their counter (g_lru_recounts), the kernel, its launch and the two
// host functions that reach the device words (one definition each: the library is built
// without relocatable device code).
#include "cache_lru_dev.hpp"

#include <hip/hip_ext.h>

#include <algorithm>
#include <mutex>
#include <vector>

namespace gf {

namespace {

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

// Never called.  lru_list_fused_kernel is the only caller of wide_sum() in this translation
// unit, and every call of it passes the same LDS array: the compiler then folds that array into
// wide_sum() BEFORE it inlines it (interprocedural constant propagation), and one v_lshlrev of
// the kernel comes out as an equivalent v_lshrrev — no better and no worse, but no longer the
// code the kernel had beside the other forms' kernels, whose calls passed other arrays.  This
// second caller with an unknown pointer keeps the kernel instruction-identical across the move
// (scripts/kernel_isa_diff.py); it costs a few dead instructions in the code object.
__device__ __attribute__((used)) uint32_t wide_sum_unfolded(uint32_t v, uint32_t* ws) {
  return wide_sum(v, ws);
}

}  // namespace

void launch_lru_fused(const Round& r, size_t list_tiles, size_t row_wgs, hipStream_t stream,
                      bool own_events) {
  const unsigned cb = static_cast<unsigned>(std::min<size_t>(list_tiles, 1024));
  const unsigned rb = static_cast<unsigned>(std::max<size_t>(row_wgs, 1));
  const unsigned wb = static_cast<unsigned>(std::min<size_t>(list_tiles, kFuseMaxTiles));
  hipEvent_t e0 = nullptr, e1 = nullptr;
  if (own_events && profile_begin(kProfLru, &e0, &e1)) {
    hipExtLaunchKernelGGL(lru_list_fused_kernel, dim3(cb + rb + wb, r.count), dim3(kWide), 0, stream,
                          e0, e1, 0, r, cb, rb, wb);
    profile_end(kProfLru, e0, e1);
  } else {
    lru_list_fused_kernel<<<dim3(cb + rb + wb, r.count), dim3(kWide), 0, stream>>>(r, cb, rb, wb);
  }
  GF_HIP(hipGetLastError());
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

// Granules of the fused LRU list update that did not arrive within the polling budget and were
// recomputed by the waiting thread (since the library was loaded, current device).
uint64_t lru_recounts() {
  unsigned int v = 0;
  GF_HIP(hipMemcpyFromSymbol(&v, HIP_SYMBOL(g_lru_recounts), sizeof(v)));
  return v;
}

}  // namespace gf
