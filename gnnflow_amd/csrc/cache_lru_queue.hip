// The LRU order of a LARGE cache, kept as a queue (overview of the LRU units: cache_lru.hip): the
// kernels that follow lru_list_scan_kernel (cache_lru.hip) in a queue-form update, the queue's
// compaction and the index of a dense list, with their launches.
#include "cache_lru_dev.hpp"

#include <algorithm>

namespace gf {

namespace {

// ---- LRU as a queue (large caches) --------------------------------------------------------
// The list passes (cache_lru.hip, cache_lru_fused.hip) cost O(capacity) per update: 352 us for a 30 k-row block on a 40 M-slot
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

static_assert(sizeof(CompactState) <= 256, "compact_layout() reserves 256 bytes for it");

}  // namespace

void launch_lru_queue_update(const Round& r, size_t rows, hipStream_t stream) {
  lru_queue_walk_kernel<<<dim3(1, r.count), dim3(kWide), 0, stream>>>(r);
  const unsigned qb = static_cast<unsigned>(
      std::max<size_t>(1, std::min<size_t>((rows + kQInst - 1) / kQInst, 16384)));
  lru_queue_install_kernel<<<dim3(qb, r.count), dim3(kQInst), 0, stream>>>(r);
}

void launch_lru_queue_compact(uint32_t* q0, uint32_t* q1, QueueState* qs, uint32_t* qpos,
                              char* scratch, const CompactLayout& layout, size_t tail_bound,
                              uint32_t capacity, hipStream_t stream) {
  const size_t tiles = (tail_bound + kRowTile - 1) / kRowTile;
  const size_t groups = (tiles + kQGroup - 1) / kQGroup;
  auto* live_bits = reinterpret_cast<unsigned long long*>(scratch + layout.live_bits);
  auto* tile_cnt = reinterpret_cast<uint32_t*>(scratch + layout.tile_cnt);
  auto* group_sum = reinterpret_cast<uint32_t*>(scratch + layout.group_sum);
  auto* st = reinterpret_cast<CompactState*>(scratch + layout.state);
  GF_HIP(hipMemsetAsync(group_sum, 0, groups * 4, stream));
  const unsigned grid = static_cast<unsigned>(std::max<size_t>(1, std::min<size_t>(tiles, 2048)));
  lru_queue_compact_count_kernel<<<dim3(grid), dim3(kWide), 0, stream>>>(q0, q1, qs, qpos, live_bits,
                                                                        tile_cnt, group_sum, st);
  lru_queue_compact_write_kernel<<<dim3(grid), dim3(kWide), 0, stream>>>(
      q0, q1, qs, qpos, live_bits, tile_cnt, group_sum, st, capacity);
  GF_HIP(hipGetLastError());
}

void launch_lru_queue_index(const uint32_t* q0, const uint32_t* q1, const QueueState* qs,
                            uint32_t* qpos, uint32_t capacity, hipStream_t stream) {
  lru_queue_index_kernel<<<dim3(2048), dim3(256), 0, stream>>>(q0, q1, qs, qpos, capacity);
  GF_HIP(hipGetLastError());
}

}  // namespace gf
