// The row gather of a fetch round (feature_cache.hip): one launch for up to kMaxCtx contexts.
//
//   gather   : reads ids, probes the id->slot map, picks the source row (cache slot in
//              HBM, or the feature table — HBM or device-mapped pinned host memory) and
//              streams it to the output with 16-byte loads/stores.  A wave owns
//              `tile_rows` consecutive output rows, flattened, so its stores form one
//              contiguous run and every lane keeps 12 (direct contexts: 13) independent 16 B
//              loads in flight; tile_rows shrinks for small blocks, down to 16, so that a
//              20k-row block still spreads over >1000 waves.  It also records each row's slot,
//              marks hit slots as touched in this epoch, counts hits/misses (once per
//              workgroup, sharded) and lets every missed row claim its id with
//              atomicMax(map[id], -(row+1)) — the lowest row of each distinct missed id wins
//              (this replaces torch.unique).
//              This kernel moves ~all the bytes (2*dim*4 per row) and is the one priced
//              against the HBM roofline.
// Rounds whose contexts all have float4 rows on list-form or cache-free contexts run one of
// three lean kernels (every table in HBM / rows from wherever the probe says / staging ring);
// every other round runs the general kernel, gather_rows_any_kernel.
#include "feature_cache_ctx.hpp"

#include <hip/hip_ext.h>

#include <algorithm>
#include <type_traits>

namespace gf {

namespace {

// ---- the gather kernel -------------------------------------------------------------
// kLean: the instantiation for rounds of float4 rows on list-form / cache-free contexts
// (no queue-form hit path)
template <typename VecT, bool kOdd = false, bool kLean = false, bool kStaged = !kLean,
          bool kDirect = false>
__device__ inline void gather_body(const Ctx& kc, uint32_t bx, uint32_t grid_x) {
  // The context lives in the kernel-argument segment and the compiler loads a field where it is
  // first used: seven dependent rounds of scalar loads (each a trip to memory for a CU's first
  // wave) stood before the first id was read.  Pinning the hot fields into SGPRs HERE makes them
  // one round.
  const Ctx& c = kc;
  // (input operands: the values must be in SGPRs here — their loads are issued together before
  // this point — and stay the kernel arguments they are, pointers into GLOBAL memory; as in/out
  // operands they came back as generic pointers and every access through them was a flat one)
  if (kLean)   // (the general kernel has no scalar registers to spare, and its launches are long)
    asm volatile("" :: "s"(c.ids), "s"(c.n), "s"(c.num_ids), "s"(c.map), "s"(c.feats), "s"(c.out),
                 "s"(c.dimv), "s"(c.tile_rows), "s"(c.update), "s"(c.policy), "s"(c.touched),
                 "s"(c.qpos), "s"(c.epoch_new), "s"(c.slot_of_row), "s"(grid_x), "s"(c.dim),
                 "s"(c.ctr), "s"(c.ctr_next), "s"(c.stats), "s"(c.tile_old), "s"(c.hist1),
                 "s"(c.capacity));
  if (kLean && !kDirect)
    asm volatile("" :: "s"(c.cache_buf), "s"(c.miss_rows), "s"(c.remap), "s"(c.pmap), "s"(c.ring),
                 "s"(c.st_lo), "s"(c.st_span), "s"(c.st_mask), "s"(c.st_cap));
  if (c.n == 0) return;
  // diagnostics (scripts/gather_hop_trace.py): wave 0 of every workgroup stamps the wall clock at
  // the stages of its first tile
  unsigned long long* tr = nullptr;
  if (kLean && kDirect && c.trace && threadIdx.x == 0 && bx < kGatherTraceWgs)
    tr = c.trace + kGatherTraceBase + bx * 8u;
  if (tr) {
    tr[0] = wall_clock64();
    // where it runs: HW_ID (cu 8-11, sh 12, se 13-15 on gfx9) and XCC_ID
    tr[5] = static_cast<unsigned long long>(__builtin_amdgcn_s_getreg(4 | (31 << 11))) |
            (static_cast<unsigned long long>(__builtin_amdgcn_s_getreg(20 | (31 << 11))) << 32);
  }
  const int lane = threadIdx.x & 63;
  const uint32_t gtid = bx * kThreads + threadIdx.x;
  const uint32_t nthreads = grid_x * kThreads;
  // housekeeping for later launches: this fetch's histograms and the NEXT fetch's counter
  // record are cleared here (neither is in use by anyone else at this point)
  if (c.update && c.policy == GF_CACHE_LRU) {   // per-group hit counts of the list scan
    const uint32_t groups = ((c.capacity + kRowTile - 1) / kRowTile + kQGroup - 1) / kQGroup;
    for (uint32_t i = gtid; i < groups; i += nthreads) c.tile_old[i] = 0;
  } else if (c.update) {
    for (uint32_t i = gtid; i < kBins1 + kBins2; i += nthreads) c.hist1[i] = 0;  // hist2 follows
  }
  if (c.ctr_next) {
    uint32_t* nxt = reinterpret_cast<uint32_t*>(c.ctr_next);
    for (uint32_t i = gtid; i < kCounterWords; i += nthreads) nxt[i] = 0;
  }
  // row stride in units of VecT — or, for odd rows, in floats (rowu) with VecT at any float
  using Unit = std::conditional_t<kOdd, float, VecT>;
  constexpr uint32_t kVF = kOdd ? 4u : 1u;   // Units per VecT
  const Unit* feats = reinterpret_cast<const Unit*>(c.feats);
  const Unit* cache_buf = reinterpret_cast<const Unit*>(c.cache_buf);
  Unit* out = reinterpret_cast<Unit*>(c.out);
  const uint32_t dimv = c.dimv, tile_rows = c.tile_rows, n = c.n;
  const uint32_t rowu = kOdd ? c.dim : c.dimv;
  const uint32_t wave = gtid >> 6;
  const uint32_t num_waves = nthreads >> 6;
  const uint32_t tiles = (n + tile_rows - 1) / tile_rows;
  uint32_t acc_hits = 0, acc_miss = 0;   // wave-uniform
  uint32_t acc_host = 0;                 // rows read from the host table (staged contexts)
  // direct: every row comes from feats[id] whatever the probe says (table in HBM, no row mirror,
  // no pulled rows, no staging ring) — the probe then only feeds the counters and the marks
  // (a template parameter: the two orders in one instantiation cost 180 instead of 104 VGPRs)
  constexpr bool direct = kDirect;
  for (uint32_t tile = wave; tile < tiles; tile += num_waves) {
    const uint32_t row0 = tile * tile_rows;
    const uint32_t rows = min(tile_rows, n - row0);
    const Unit* src = nullptr;
    int32_t slot = -2;
    uint32_t hit_code = 0;
    bool from_host = false;   // staged context: the row is read from the host table after all
    int64_t id = -1;
    bool known = false;
    if (lane < static_cast<int>(rows)) {
      id = c.ids[row0 + lane];
      known = id >= 0 && static_cast<uint64_t>(id) < c.num_ids;
      if (known) {
        slot = c.map ? c.map[id] : -1;
        if (direct) src = feats + static_cast<uint64_t>(id) * rowu;
      }
    }
    if (kLean && kDirect && c.trace && tile == wave) {   // (wave-uniform; traced launches only)
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      if (tr) tr[1] = wall_clock64();   // ids (and the map values) in
    }
    uint64_t src_bits = reinterpret_cast<uint64_t>(src);
    const uint32_t total = rows * dimv;
    Unit* o = out + static_cast<uint64_t>(row0) * rowu;
    // The loop trip count is wave-uniform and every lane executes the cross-lane read:
    // ds_bpermute returns 0 for a source lane that EXEC has switched off, so the
    // row-base broadcast must never sit under a per-lane condition.
    auto load = [&](uint32_t fu, bool* valid, uint32_t* at) -> VecT {
      *valid = fu < total;
      const uint32_t r = *valid ? fu / dimv : 0u;
      const uint32_t cc = fu - r * dimv;
      // odd rows: the last vector of a row ends with the row (it overlaps its neighbour by
      // 4 - dim % 4 floats, which are simply written twice) — no scalar tail pass
      const uint32_t off = kOdd ? min(cc * kVF, rowu - kVF) : cc * kVF;
      // where it goes, in Units from the tile's first row (even rows: r * dimv + cc = fu)
      *at = kOdd ? r * rowu + off : fu;
      const Unit* s = reinterpret_cast<const Unit*>(__shfl(src_bits, r, 64));
      // An unconditional GLOBAL load (a lane with nothing to read reads the tile's first output
      // row): a load under a per-lane branch, or a flat one — the pointer went through a
      // cross-lane read and lost its address space — makes the compiler wait for ALL loads in
      // flight (s_waitcnt vmcnt(0)) wherever it needs one of them.
      const bool take = *valid && s != nullptr;
      const VecT x = global_load<VecT>(take ? s + off : o);
      return take ? x : vec_zero<VecT>();
    };
    // direct context: the first trip's row loads are issued here, right behind the map load and
    // before anything looks at its result — the chain is launch -> ids -> rows -> stores, the
    // probe (map -> marks / claims, which only the update reads) hangs off its side
    constexpr int K0 = kDirect ? 13 : 12;   // (13: a tile of 19 172-d rows still is one trip)
    VecT v0[K0];
    bool p0[K0];
    uint32_t at0[K0];
    constexpr bool early = direct;
    // K independent 16-byte loads in flight per lane, then the stores.  (12 covers a whole
    // 16-row tile of 172-d rows in one trip; measured 14.8-14.9 us per launch against 15.5-15.7
    // with 4 on the same box.)
    auto copy = [&](auto kk, uint32_t first) {
      constexpr int K = decltype(kk)::value;
      for (uint32_t base = first; base < total; base += 64 * K) {
        VecT v[K];
        bool p[K];
        uint32_t at[K];
#pragma unroll
        for (int k = 0; k < K; ++k) v[k] = load(base + lane + 64 * k, &p[k], &at[k]);
        // streaming stores: the 21 MB of output rows of a launch would otherwise sit dirty in
        // the L2s until the kernel's end-of-kernel write-back (14.1 -> 13.2 us per launch; the
        // install kernel, which reads the missed rows back, pays 0.5-1 us of that again;
        // storing only the hit rows this way was slower than either)
#pragma unroll
        for (int k = 0; k < K; ++k)
          if (p[k]) nt_store(v[k], reinterpret_cast<VecT*>(o + at[k]));
      }
    };
    if (early) {
      // ... and stored as they arrive; the probe's result is looked at behind the copy
#pragma unroll
      for (int k = 0; k < K0; ++k) v0[k] = load(lane + 64 * k, &p0[k], &at0[k]);
#pragma unroll
      for (int k = 0; k < K0; ++k)
        if (p0[k]) nt_store(v0[k], reinterpret_cast<VecT*>(o + at0[k]));
      // (rows wider than one trip covers are rare and this loop's registers count for the whole
      // kernel: four in flight keeps it at 4 waves per SIMD)
      copy(std::integral_constant<int, 4>{}, 64u * K0);
      if (kLean && c.trace && tile == wave) {
        if (tr) tr[2] = wall_clock64();   // every row of the tile in, its stores issued
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (tr) tr[3] = wall_clock64();   // stores acknowledged
      }
    }
    if (known) {
      const int32_t claim = slot;   // a missed id of a planned pull: -(representative row + 1)
      if (slot >= 0) {
        // (no row mirror — table in HBM, gf_cache_set_row_mirror: a hit is the table's row too)
        if (!direct)
          src = c.cache_buf ? cache_buf + static_cast<uint64_t>(slot) * rowu
                            : feats + static_cast<uint64_t>(id) * rowu;
        // a hit is recorded (LRU: refreshes the slot, LFU: counts a use) but takes effect
        // only if the block also misses; FIFO ignores hits (fifo_cache.py:77-161).
        if (!kLean && c.qmode) {
          // queue form: the mark is the bit of the entry's queue position; the row whose
          // atomic set it stands for the slot (it will append the slot's new entry)
          const uint32_t pos = c.qpos[slot], bit = 1u << (pos & 31u);
          const uint32_t was = atomicOr(&c.qbits[pos >> 5], bit);
          hit_code = (was & bit) ? 0u : (kRepHit | pos);
        } else if (c.update && c.policy != GF_CACHE_FIFO) {
          c.touched[c.policy == GF_CACHE_LRU ? c.qpos[slot] : slot] = c.epoch_new;
        }
      } else {
        slot = -1;
        if (direct) {
        } else if (c.miss_rows) {
          const uint32_t at = c.req_pos
              ? c.req_pos[c.map ? static_cast<uint32_t>(-(claim + 1)) : row0 + lane]
              : c.miss_index[row0 + lane];
          src = reinterpret_cast<const Unit*>(c.miss_rows) + static_cast<uint64_t>(at) * rowu;
        } else if (c.remap) {
          int32_t local = c.remap[id];
          if (local < 0) { *c.flag = 1u; local = 0; }
          src = feats + static_cast<uint64_t>(local) * rowu;
        } else {
          src = feats + static_cast<uint64_t>(id) * rowu;
          if (kStaged && c.pmap) {
            // {newest entry, the one before it}: an id that a generation running beside this
            // launch stages AGAIN is still readable where it was (the GDELT-shaped node block,
            // every id a dozen times per block, sent 7 k rows per step to the host otherwise)
            const ulonglong2 pq = reinterpret_cast<const ulonglong2*>(c.pmap)[id];
            const bool newest = static_cast<uint32_t>(pq.x >> 32) - c.st_lo <= c.st_span;
            const unsigned long long p = newest ? pq.x : pq.y;
            const uint32_t g = static_cast<uint32_t>(p >> 32);
            if (g - c.st_lo <= c.st_span)
              src = reinterpret_cast<const Unit*>(c.ring) +
                    (static_cast<uint64_t>(g & c.st_mask) * c.st_cap + static_cast<uint32_t>(p)) * rowu;
            else
              from_host = true;
          }
        }
        if (c.update) atomicMax(&c.map[id], -static_cast<int32_t>(row0 + lane + 1));
      }
    }
    if (lane < static_cast<int>(rows) && c.slot_of_row) c.slot_of_row[row0 + lane] = slot;
    acc_hits += __popcll(__ballot(slot >= 0));
    acc_miss += __popcll(__ballot(slot == -1));
    if (kStaged && c.pmap) acc_host += __popcll(__ballot(from_host));
    if (!direct) src_bits = reinterpret_cast<uint64_t>(src);
    if (!early) copy(std::integral_constant<int, 12>{}, 0u);
    // (behind the copy: the atomic's return value has long arrived)
    if (!kLean && c.qmode && lane < static_cast<int>(rows)) c.rep_flag[row0 + lane] = hit_code;
  }
  if (c.ctr) {
    __shared__ uint32_t wg_hits, wg_miss;
    if (threadIdx.x == 0) { wg_hits = 0; wg_miss = 0; }
    __syncthreads();
    if (lane == 0) {
      if (acc_hits) atomicAdd(&wg_hits, acc_hits);
      if (acc_miss) atomicAdd(&wg_miss, acc_miss);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      const int sh = bx & (kShards - 1);
      if (wg_hits) atomicAdd(&c.ctr->shard[sh].hits, wg_hits);
      if (wg_miss) atomicAdd(&c.ctr->shard[sh].n_miss, wg_miss);
      if (c.stats && wg_hits) atomicAdd(&c.stats[2 * sh], wg_hits);
    }
  }
  if (tr) tr[4] = wall_clock64();       // marks, claims and counters issued
  if (c.stats && gtid == 0) atomicAdd(&c.stats[1], n);
  if (kStaged && c.pmap && acc_host && lane == 0)
    atomicAdd(c.st_fallback, static_cast<unsigned long long>(acc_host));
  if (kStaged && c.progress && gtid == 0)
    __hip_atomic_store(c.progress, c.progress_val, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// Every kind of row and context: float4 rows, odd widths (16-byte vectors at 4-byte alignment),
// scalar rows; list-form, queue-form and cache-free contexts.
__device__ inline bool ctx_direct(const Ctx& c) {
  return !c.cache_buf && !c.miss_rows && !c.remap && !c.pmap;
}
__global__ __launch_bounds__(kThreads) void gather_rows_any_kernel(Round r) {
  const Ctx& c = r.c[blockIdx.y];
  if (c.n == 0) return;
  const uint32_t bx = blockIdx.x, gx = gridDim.x;
  if (ctx_direct(c)) {
    if (c.vec4) gather_body<float4, false, false, false, true>(c, bx, gx);
    else if (c.odd4) gather_body<uf4, true, false, false, true>(c, bx, gx);
    else gather_body<float, false, false, false, true>(c, bx, gx);
    return;
  }
  if (c.vec4) gather_body<float4>(c, bx, gx);
  else if (c.odd4) gather_body<uf4, true>(c, bx, gx);
  else gather_body<float>(c, bx, gx);
}

// The same for rounds whose contexts ALL take the float4 / list-form or cache-free
// path (launch_round picks): a third of the code and 104-128 instead of 138 VGPRs (4 waves per
// SIMD) — same-box A/B in profiles/README, round 5.  gather_rows_kernel: every context direct
// (tables in HBM, no row mirror: the headline replay); _mirror_: rows come from wherever the probe
// says (row mirror, pulled rows, remapped local rows).
// The lean kernels' grid is ONE row of workgroups, the contexts' workgroups back to back
// (first[k] = first workgroup of context k + 1, first.w = all): the dispatcher hands workgroups to
// the 256 CUs round robin and a CU moves its workgroups' rows at ~44 GB/s however many it holds —
// the launch ends with the fullest CU (profiles/r06_gather_hop_trace.txt), and in a (x, context)
// grid the contexts' unused workgroups shift the round robin so that some CUs get one more.
// (the lean kernels' one-row grid: which context a workgroup belongs to, its index there and
// that context's workgroup count)
__device__ inline uint32_t packed_ctx(const uint4& first, uint32_t* bx, uint32_t* gx) {
  const uint32_t b = blockIdx.x;
  const uint32_t y = (b >= first.x ? 1u : 0u) + (b >= first.y ? 1u : 0u) + (b >= first.z ? 1u : 0u);
  const uint32_t lo = y == 0 ? 0u : y == 1 ? first.x : y == 2 ? first.y : first.z;
  const uint32_t hi = y == 0 ? first.x : y == 1 ? first.y : y == 2 ? first.z : first.w;
  *bx = b - lo;
  *gx = hi - lo;
  return y;
}
__global__ __launch_bounds__(kThreads) void gather_rows_kernel(uint4 first, Round r) {
  uint32_t bx, gx;
  const uint32_t y = packed_ctx(first, &bx, &gx);
  gather_body<float4, false, true, false, true>(r.c[y], bx, gx);
}
__global__ __launch_bounds__(kThreads) void gather_rows_mirror_kernel(uint4 first, Round r) {
  uint32_t bx, gx;
  const uint32_t y = packed_ctx(first, &bx, &gx);
  gather_body<float4, false, true>(r.c[y], bx, gx);
}

// ... and the lean kernel for rounds over a host-resident table with a staging ring
__global__ __launch_bounds__(kThreads) void gather_rows_staged_kernel(uint4 first, Round r) {
  uint32_t bx, gx;
  const uint32_t y = packed_ctx(first, &bx, &gx);
  gather_body<float4, false, true, true>(r.c[y], bx, gx);
}

inline unsigned gather_grid_for(size_t n, uint32_t tile_rows) {
  const size_t waves = (n + tile_rows - 1) / tile_rows;
  return static_cast<unsigned>(std::max<size_t>(1, std::min<size_t>((waves + 3) / 4, 1024)));
}

}  // namespace

void launch_gather(Round& r, hipStream_t stream) {
  unsigned ggrid = 1;
  for (int i = 0; i < r.count; ++i) {
    const Ctx& c = r.c[i];
    GF_REQUIRE(c.n < 0x7FFFFFFFull, "gather: more than 2^31-1 rows in one block");
    ggrid = std::max(ggrid, gather_grid_for(c.n, c.tile_rows));
  }
  bool lean = true, staged = false, direct = true;
  for (int i = 0; i < r.count; ++i) {
    const Ctx& c = r.c[i];
    lean = lean && c.vec4 && !c.qmode;
    staged = staged || c.pmap != nullptr;
    direct = direct && !c.cache_buf && !c.miss_rows && !c.remap && !c.pmap;
  }
  if (lean && direct) {
    // Two workgroups per CU, not three: the dispatcher hands workgroups to the 256 CUs round
    // robin, and the launch ends with the CUs that received a third one (~2.3 us per further
    // workgroup: profiles/r06_gather_hop_trace.txt).  If slightly larger tiles — still one trip
    // of loads — bring the round down to 512 workgroups, take them.
    auto wgs = [&](uint32_t t) {
      size_t total = 0;
      for (int i = 0; i < r.count; ++i) total += ((r.c[i].n + t - 1) / t + 3) / 4;
      return total;
    };
    uint32_t t0 = 0, dimv = 1;
    bool same = true;
    for (int i = 0; i < r.count; ++i) {
      if (r.c[i].n == 0) continue;
      if (t0 == 0) t0 = r.c[i].tile_rows;
      same = same && (r.c[i].tile_rows == t0 || r.c[i].n <= 4u * r.c[i].tile_rows);
      dimv = std::max(dimv, r.c[i].dimv);
    }
    const uint32_t t_max = std::min<uint32_t>(64u, 13u * 64u / dimv);
    if (same && t0 == 16 && wgs(t0) > 512 && t_max > t0) {
      uint32_t t = t0 + 1;
      while (t < t_max && wgs(t) > 512) ++t;
      if (wgs(t) <= 512) {
        ggrid = 1;
        for (int i = 0; i < r.count; ++i) {
          if (r.c[i].n > 4u * r.c[i].tile_rows) r.c[i].tile_rows = t;
          ggrid = std::max(ggrid, gather_grid_for(r.c[i].n, r.c[i].tile_rows));
        }
      }
    }
  }
  hipEvent_t e0 = nullptr, e1 = nullptr;
  if (lean) {
    auto* kernel = staged ? gather_rows_staged_kernel
                 : direct ? gather_rows_kernel : gather_rows_mirror_kernel;
    uint32_t first[5] = {0, 0, 0, 0, 0};
    for (int i = 0; i < kMaxCtx; ++i)
      first[i + 1] = first[i] + (i < r.count && r.c[i].n ? gather_grid_for(r.c[i].n, r.c[i].tile_rows) : 0u);
    const uint4 f = make_uint4(first[1], first[2], first[3], first[4]);
    const unsigned total = std::max(1u, first[4]);
    if (profile_begin(kProfGather, &e0, &e1)) {
      // the events ride on the dispatch itself: its begin / end timestamps
      hipExtLaunchKernelGGL(kernel, dim3(total), dim3(kThreads), 0, stream, e0, e1, 0, f, r);
      profile_end(kProfGather, e0, e1);
    } else {
      kernel<<<dim3(total), dim3(kThreads), 0, stream>>>(f, r);
    }
  } else {
    auto* kernel = gather_rows_any_kernel;
    if (profile_begin(kProfGather, &e0, &e1)) {
      hipExtLaunchKernelGGL(kernel, dim3(ggrid, r.count), dim3(kThreads), 0, stream, e0, e1, 0, r);
      profile_end(kProfGather, e0, e1);
    } else {
      kernel<<<dim3(ggrid, r.count), dim3(kThreads), 0, stream>>>(r);
    }
  }
  GF_HIP(hipGetLastError());
}

Ctx plain_ctx(const float* feats, size_t num_rows, size_t dim, const int64_t* ids, size_t n,
              float* out) {
  Ctx c;
  std::memset(&c, 0, sizeof(c));
  c.ids = ids;
  c.n = static_cast<uint32_t>(n);
  c.vec4 = vec4_ok(dim, feats, out, out) ? 1 : 0;
  c.dimv = static_cast<uint32_t>(c.vec4 ? dim / 4 : dim);
  set_odd4(c, dim, true);
  c.tile_rows = pick_tile_rows(n);
  c.out = out;
  c.feats = feats;
  c.num_ids = num_rows;
  return c;
}

void gather_rows(const float* d_feats, size_t num_rows, size_t dim, const int64_t* d_ids,
                 size_t n, float* d_out, int device, hipStream_t stream) {
  if (n == 0) return;
  GF_REQUIRE(d_feats && d_ids && d_out, "gather_rows: null pointer");
  GF_REQUIRE(dim > 0, "gather_rows: dim must be positive");
  DeviceGuard dg(device);
  Round r;
  r.count = 1;
  r.c[0] = plain_ctx(d_feats, num_rows, dim, d_ids, n, d_out);
  launch_round(r, stream);
}

// Several cache-free gathers that share one id list (TGN memory: four tables), one launch.
void gather_rows_multi(const float* const* tables, const size_t* dims, float* const* outs,
                       size_t num_tables, size_t num_rows, const int64_t* d_ids, size_t n,
                       int device, hipStream_t stream) {
  if (n == 0 || num_tables == 0) return;
  GF_REQUIRE(num_tables <= static_cast<size_t>(kMaxCtx), "gather_rows_multi: too many tables");
  GF_REQUIRE(tables && dims && outs && d_ids, "gather_rows_multi: null pointer");
  DeviceGuard dg(device);
  Round r;
  r.count = static_cast<int>(num_tables);
  for (size_t t = 0; t < num_tables; ++t) {
    GF_REQUIRE(tables[t] && outs[t] && dims[t] > 0, "gather_rows_multi: bad table");
    r.c[t] = plain_ctx(tables[t], num_rows, dims[t], d_ids, n, outs[t]);
  }
  launch_round(r, stream);
}

}  // namespace gf
