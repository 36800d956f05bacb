// What the translation units of the feature cache share (gather.hip, cache_staging.hip,
// cache_pull.hip, cache_select.hip, cache_lru*.hip, feature_cache.hip): the kernel-argument
// structs, the tile / bin / ring constants, the device helpers more than one of them uses and
// the launch function of each part.  Private to those files.
#pragma once

#include "feature_cache.hpp"
#include "owner_hash.hpp"

#include <cstdlib>
#include <cstring>

namespace gf {

constexpr int32_t kAbsent = INT32_MIN;  // map[] value of an uncached id
// gather workgroup (same-box A/B of the headline fetch, us per launch: 64 threads 23.5, 128 16.1,
// 256 13.3, 512 13.9, 1024 15.3 — profiles/r06_gather_hop_trace.txt)
constexpr int kThreads = 256;
constexpr int kWide = 1024;             // slot kernels, scans
constexpr int kFine = 2048;             // ages 0..2047: one bin each
constexpr int kBins1 = 4096;            // + 2048 coarse bins of 2048 ages each
constexpr int kBins2 = 2048;            // second level inside one coarse bin
constexpr uint32_t kAgeMax = kFine + 2048u * 2048u - 1u;
constexpr int kTile = 1024;             // slots per tile (= install workgroup)
constexpr int kRing = 32;               // per-fetch counter records
constexpr int kMaxCtx = 4;              // contexts per round
constexpr uint32_t kRowTile = 4096;     // rows per scan workgroup (kWide threads x 4)
constexpr uint32_t kMaxRowTiles = 1024; // more row tiles than this: chained single-workgroup scan
constexpr uint32_t kQGroup = 64;        // LRU: list tiles per group sum
constexpr uint32_t kInstRows = 256;     // LRU: block rows per install workgroup
// LRU: block rows per scan workgroup.  One row per thread: the row role is a handful of
// scattered loads per row, which a CU retires at ~one 64-line instruction per 64 cycles, so a
// 20 k-row block wants 20 CUs on it, not 5 (kRowTile rows per workgroup).
constexpr uint32_t kLruRows = 1024;
constexpr uint32_t kMaxStageTiles = 1024;   // LRU list form: list tiles that stage their victims
constexpr uint32_t kBitTile = 4096;         // LRU queue form: words of the hit bitmap per tile (kWide x 4)
constexpr uint32_t kMaxBitGroups = 1024;    // ... entries of the install kernel's LDS prefix over the tiles
constexpr uint32_t kMaxVChunks = 2048;      // LRU queue form: victim chunks (+ the walk's) the LDS prefix holds
// LRU list form in one launch (cache_lru_fused.hip, lru_list_fused_kernel)
constexpr uint32_t kFuseTile = kWide;         // list entries per count / write tile
constexpr uint32_t kFuseMaxTiles = 2048;      // list tiles (LDS prefix arrays): <= 2 M slots
constexpr uint32_t kFuseMaxRowWgs = 1024;     // row workgroups: <= 1 M block rows

// One record per fetch.  hits / misses are accumulated once per workgroup into one of 8
// shards that sit on separate 128-byte lines: same-address atomics retire at only
// ~88/us on MI355X, so one counter word per wave would dominate the gather itself.
constexpr int kShards = 8;
struct Shard {
  uint32_t hits;      // rows served from the cache
  uint32_t n_miss;    // rows served from the feature table
  uint32_t pad[30];
};
struct Counters {
  Shard shard[kShards];
  uint32_t n_unique;  // distinct missed ids
  uint32_t th_age;    // eviction threshold (written by the tile-count kernel)
  uint32_t th_k_tie;
  uint32_t fifo_start;  // FIFO: first slot of this block's refill arc
  uint32_t ticket;      // workgroups of the rank kernel that finished their level-2 histogram
  uint32_t q_parity;    // LRU list: buffer that is current during this update
  uint32_t q_found;     // LRU list: not-hit victims found by the list scan
  uint32_t q_head;      // LRU queue: head / tail of the queue during this update
  uint32_t q_tail;
  uint32_t pad[23];
};
constexpr uint32_t kCounterWords = sizeof(Counters) / 4;

// Everything one block fetch needs on the device.  `update` == 0: gather only.
// {parity, flip_tag} form ONE aligned 64-bit word: the fused list update flips the parity with
// a single store of {new parity, its launch tag}, so a workgroup of the same launch that starts
// late and reads the word knows from the tag that it already sees the NEW parity.
struct QueueState { uint32_t parity, flip_tag, head, tail, lone_walks, pad; };

struct Ctx {
  const int64_t* ids;
  uint32_t n;
  int vec4;                 // rows are float4-addressable
  uint32_t dimv;            // row length in float4s (vec4 / odd4) or floats
  // rows of dim % 4 != 0 floats (GDELT: 413 / 186) or misaligned bases: dimv = ceil(dim / 4)
  // 16-byte vectors at 4-byte alignment per row, the last one ending with the row (it overlaps
  // its neighbour); rows `dim` floats apart
  int odd4;
  uint32_t dim, tail;
  // the feature table is in HBM: the install kernel copies a missed row into the cache from
  // the table (read by the gather a moment ago: in L2) rather than from the streamed output
  int inst_from_table;
  uint32_t tile_rows;       // rows per wave in the gather
  uint32_t pad0;            // (keeps the offsets of the fields behind it)
  float* out;
  const float* feats;
  // sharded feature tables (Cache(distributed=True)): a missed row i is read from row
  // miss_index[i] of miss_rows — the rows the caller pulled from their owners — not from feats
  const float* miss_rows;
  const uint32_t* miss_index;
  // ... or, when the pull was planned natively (gf_pull_*): from row req_pos[rep] of miss_rows,
  // rep = the row whose claim on map[id] the plan settled (cache-free context: the row itself)
  const uint32_t* req_pos;
  // serving a shard: the table row of id is remap[id] (global id -> local row, < 0: not owned
  // -> *flag is raised and row 0 is served)
  const int32_t* remap;
  uint32_t* flag;
  // host-resident table with a staging ring ("staging ring" below): a missed id whose pmap entry
  // {generation, row} lies in [st_lo, st_lo + st_span] is read from that row of the generation's
  // region of the ring — an HBM copy of its table row pulled ahead of this launch
  const unsigned long long* pmap;
  const float* ring;
  uint32_t st_lo, st_span, st_mask, st_cap;
  uint32_t* progress;       // pinned host word: this launch stores progress_val = the number of
  uint32_t progress_val;    // ring-reading launches enqueued before it (all finished by now)
  unsigned long long* st_fallback;   // rows this cache's gathers read from the HOST table
  // diagnostics (gf_debug_lru_trace): per workgroup of the one-launch list update, 8 stamps of the
  // 100 MHz wall clock; [0 .. 3] of the buffer: count / row / write workgroups, launch tag
  unsigned long long* trace;
  uint64_t num_ids;
  int32_t* map;             // null: no cache (plain gather)
  float* cache_buf;
  int64_t* slot_id;
  uint32_t* stamp;          // LFU: use count (FIFO: install epoch; LRU: unused)
  uint32_t* touched;        // epoch of the last hit (pending until the block misses) — LRU list
                            // form: indexed by the entry's LIST POSITION (qpos[slot]), so the
                            // two list passes read it densely, next to the list itself;
                            // otherwise (queue form, LFU) by slot
  uint32_t* queue[2];       // LRU: the slots, least recently refreshed first (double buffer)
  QueueState* qstate;       // LRU: which buffer is current, device resident
  uint32_t tiles_per_wg;    // LRU: row tiles per scan workgroup (1 unless > 1M rows)
  uint32_t inst_rows;       // LRU: block rows per install workgroup (kInstRows or kWide)
  // LRU of a LARGE cache (queue form, see "LRU as a queue", cache_lru_queue.hip); qmode == 0: list form
  int qmode;                // this update appends to the queue instead of rewriting the list
  uint32_t* qpos;           // [capacity] position of the slot's live queue entry
  uint32_t* qbits;          // one bit per queue position: entry of a slot hit by this block
                            // (set by the gather; all zero between updates)
  uint2* wsnap;             // per word of qbits: {the word, hit entries before it in its tile}
  uint32_t q_group;         // bitmap tiles per entry of the install kernel's LDS prefix
  // list form: the first stage_tiles list tiles leave their not-hit entries (the victims, in
  // list order) packed per tile in v_slot and — if that is the whole list — their hit entries
  // in v_pos (the next victims when a block needs more slots than its hits leave over);
  // 0: one workgroup walks the list instead (more than kMaxStageTiles tiles needed)
  uint32_t stage_tiles;
  uint32_t stage_min;       // ... for blocks that missed more rows than this
  int stage_hits;
  uint32_t v_chunks;        // victim walk: chunks of kRowTile queue entries behind the head
  uint32_t* v_slot;         // [(v_chunks * kRowTile) + n] candidates per chunk (+ the lone walk's)
  uint32_t* v_pos;          // their queue positions
  uint32_t* v_count;        // [v_chunks + 1]
  // LRU list form, ONE launch (lru_list_fused_kernel): granules {launch tag, count} per list
  // tile / per row workgroup, and the front tiles' entries staged with the id they hold
  int fused;
  uint32_t fuse_tag;        // unique per launch and cache (never reset), > 0
  uint32_t fuse_rows;       // block rows per row workgroup (kInstRows or kWide)
  unsigned long long* g_cnt;   // [kFuseMaxTiles]
  unsigned long long* g_row;   // [kFuseMaxRowWgs]
  long long* v_old;         // id held by v_slot's entry
  long long* v_hold;        // ... by v_pos's (the hit entries)
  uint32_t capacity;
  uint32_t epoch_new;
  int update;
  int policy;               // GF_CACHE_LRU / _LFU / _FIFO
  uint32_t* fifo_ptr;       // FIFO: last refilled slot (fifo_cache.py:66-69), device resident
  int32_t* slot_of_row;
  uint32_t* rep_flag;
  uint32_t* rep_rank;
  uint32_t* rep_row;        // rank -> row of the representative
  int64_t* rep_id;          // rank -> id (saves the install kernel a dependent load)
  uint32_t* row_tile_sum;   // [ceil(n / kRowTile)] representatives per row tile
                            // (LRU: per scan workgroup)
  uint32_t* hist1;
  uint32_t* hist2;
  uint32_t* tile_tie;
  uint32_t* tile_old;
  Counters* ctr;            // this fetch's record (zeroed by the previous fetch)
  Counters* ctr_next;       // record of the next fetch on this cache: zeroed here
  uint32_t* stats;          // caller's 16-word hit statistics, may be null
};
struct Round {
  Ctx c[kMaxCtx];
  int count;
};

__device__ inline uint32_t total_miss(const Counters* c) {
  uint32_t m = 0;
#pragma unroll
  for (int i = 0; i < kShards; ++i) m += c->shard[i].n_miss;
  return m;
}

// LRU list form: a block that missed more rows than this finds its victims through the list
// tiles' staged entries; fewer (one or two trips) are cheaper for the one-workgroup walk
// (headline workload, ~5 k missed rows per block: 39.6-40.0 us per step with the walk,
// 40.4-41.0 staged; 30 k-row blocks with 15-30 k misses: 37.7 us per fetch with the walk, 29.4
// staged).  The same counter is read by both kernels, so they agree.
constexpr uint32_t kStageMinWant = 8192;

// a float4 that is only 4-byte aligned: global memory takes unaligned 16-byte accesses, a
// wave's 1 KB run then touches 9 lines instead of 8
typedef float uf4 __attribute__((ext_vector_type(4), aligned(4)));

typedef float nf4 __attribute__((ext_vector_type(4)));
__device__ inline void nt_store(float v, float* p) { __builtin_nontemporal_store(v, p); }
__device__ inline void nt_store(const float4& v, float4* p) {
  nf4 t; t.x = v.x; t.y = v.y; t.z = v.z; t.w = v.w;
  __builtin_nontemporal_store(t, reinterpret_cast<nf4*>(p));
}

// loads through a pointer known to be global memory (global_load_*, not flat_load_*)
template <typename VecT> __device__ inline VecT global_load(const void* p);
template <> __device__ inline float global_load<float>(const void* p) {
  return *(const __attribute__((address_space(1))) float*)p;
}
template <> __device__ inline uf4 global_load<uf4>(const void* p) {
  return *(const __attribute__((address_space(1))) uf4*)p;
}
template <> __device__ inline float4 global_load<float4>(const void* p) {
  const nf4 t = *(const __attribute__((address_space(1))) nf4*)p;
  return make_float4(t.x, t.y, t.z, t.w);
}

template <typename VecT> __device__ inline VecT vec_zero();
template <> __device__ inline uf4 vec_zero<uf4>() { return uf4{0.f, 0.f, 0.f, 0.f}; }
// (streaming, like the float4 rows: GDELT-shaped step 257 -> 233 us of gather per step; writing
// a tile's contiguous output as ALIGNED float4s instead changed nothing on top of that — the
// rest of the gap to 16-byte-aligned row widths, 212 us, is on the load side)
__device__ inline void nt_store(const uf4& v, uf4* p) { __builtin_nontemporal_store(v, p); }
template <> __device__ inline float vec_zero<float>() { return 0.0f; }
template <> __device__ inline float4 vec_zero<float4>() { return make_float4(0.f, 0.f, 0.f, 0.f); }

// rep_flag[row]: representative of a distinct missed id (rank among them in the low bits) /
// queue form: THE row that stands for a hit slot (the old queue position of its entry)
constexpr uint32_t kRepMiss = 1u << 31, kRepRank = kRepMiss - 1u;
constexpr uint32_t kRepHit = 1u << 30, kRepPos = kRepHit - 1u;

// gf_debug_lru_trace buffer: [0 .. 3] header, 8 stamps per workgroup of the one-launch update
// (at most 2 * 2048 list tiles + 1024 row workgroups), then 8 per workgroup of the gather launch
// before it (the traced cache's context)
constexpr uint32_t kGatherTraceBase = 4u + 8u * (2u * 2048u + 1024u);
constexpr uint32_t kGatherTraceWgs = 1024u;

// staging ring (cache_staging.hip): one block of a prefetch generation
struct StageCtx {
  const int64_t* ids;
  uint32_t n;
  const int32_t* map;          // null: cache-free context (target rows)
  uint64_t num_ids;
  unsigned long long* pmap;
  uint32_t* region_rows;       // [G] rows taken in each region
  long long* region_ids;       // [C] id staged in each row of THIS generation's region
  uint32_t gen, lo, mask, cap;
  // LRU: a CACHED id whose entry is among the first `risk` of the eviction order may be gone
  // when the fetch this prefetch works for runs (up to kStageAhead updates lie in between, each
  // taking at most its block's rows from the front) — it is staged as well.  A small cache that
  // a block turns over (the headline's node cache: 2 196 slots, ~800 installs per step) would
  // otherwise send a few hundred rows per step to the host table from inside the gather.
  const uint32_t* qpos;        // null: no such rule (LFU / FIFO, cache-free context)
  const QueueState* qstate;    // queue form: the head the positions count from
  uint32_t risk;
};
struct StageRound {
  StageCtx c[kMaxCtx];
  int count;
};

// ... and the pull of what a generation's blocks claimed
struct PullJob {
  const long long* ids;        // [cap] (-1: unused row)
  const float* feats;
  float* dst;                  // the region's first row
  uint32_t* region_rows;       // rows taken in the region (may exceed cap: the excess was dropped)
  uint32_t* next_rows;         // the next generation's counter, cleared here
  unsigned long long* pulled;  // rows pulled so far (diagnostics)
  uint32_t cap, dim, vec4;
};
struct PullJobs {
  PullJob j[2];
  int count;
};

// one context of a pull round over sharded feature tables (cache_pull.hip)
struct PullCtx {
  const int64_t* ids;
  uint32_t n;
  const int64_t* key_base;    // owner key of row i: key_base[key_index[i]] | key_base[i] | ids[i]
  const int64_t* key_index;
  int32_t* map;               // null: cache-free (every row travels)
  uint64_t num_ids;
  uint32_t* counts;           // rows per owner q at counts[q * cstride] (count: written;
  uint32_t cstride;           // scatter: read — the owner-major offsets are their prefix)
  uint32_t* cursor;           // [world] zeroed
  int64_t* send_ids;
  uint32_t* req_pos;          // [n]
};
struct PullRound {
  PullCtx c[kMaxCtx];
  int count;
  OwnerDiv od;
};

// rows that are not float4-addressable (dim % 4 != 0, or a misaligned base) still move as
// 16-byte vectors at 4-byte alignment; `allowed`: the kernels that will see
// this context know the mode (the LFU / FIFO install does not)
inline void set_odd4(Ctx& c, size_t dim, bool allowed) {
  c.dim = static_cast<uint32_t>(dim);
  c.odd4 = 0;
  c.tail = 0;
  if (c.vec4 || !allowed || dim < 8) return;
  c.odd4 = 1;
  c.dimv = static_cast<uint32_t>((dim + 3) / 4);   // the last vector overlaps its neighbour
  c.tail = static_cast<uint32_t>(dim % 4);
}

inline bool vec4_ok(size_t dim, const void* a, const void* b, const void* c) {
  auto al = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; };
  return dim % 4 == 0 && al(a) && al(b) && al(c);
}

// LRU caches of at least this many slots are kept as a queue (O(block rows) updates): a
// 30 k-row fetch with update costs 30 / 42 / 77 / 152 / 352 us in the list form at 0.13 / 1 / 4
// / 16 / 40 M slots and 45 / 45 / 49 us in the queue form at 4 / 16 / 40 M
// (profiles/r02_lru_capacity_sweep.jsonl)
// (round 5, 30 k-row blocks, one-launch list update: 23.9 / 36.3 / 48.5 / 68.8 us per fetch at
// 0.13 / 0.5 / 1 / 2 M slots; row-parallel queue form 41.6 / 36.8 / 35.0 / 34.9 / 34.5 / 37.7 at
// 0.13 / 0.5 / 1 / 2 / 16 / 40 M: they cross at ~0.5 M slots; profiles/r05_lru_capacity_sweep.txt)
inline size_t queue_min_capacity() {
  const char* v = std::getenv("GNNFLOW_LRU_QUEUE_MIN_CAPACITY");   // tuning / tests
  return v ? static_cast<size_t>(std::atoll(v)) : (size_t{1} << 19);
}

// entries per list buffer: the list itself, or the queue with room for dead entries
// (FeatureCache::alloc_queue)
inline size_t lru_queue_cap(size_t capacity, bool queue_form) {
  return queue_form ? capacity + capacity / 2 + 64 : capacity;
}

// bitmap over the queue positions, in whole tiles of kRowTile words (+ one tile)
inline size_t qbits_bytes(size_t queue_cap) {
  const size_t words = (queue_cap + 64 + 31) / 32;
  return ((words + kRowTile - 1) / kRowTile + 1) * kRowTile * sizeof(uint32_t);
}

// Queue form: tiles of kBitTile words of that bitmap (32 queue positions per word; the tail is
// below queue_cap + 64).  Of the capacity alone: the launch sizes its grid from the contexts,
// which carry the capacity and not queue_cap, and must cover what the context fill laid out.
inline size_t lru_bit_tiles(size_t capacity) {
  return ((lru_queue_cap(capacity, true) + 64) / 32 + kBitTile - 1) / kBitTile + 1;
}

// Scratch of the queue compaction (cache_lru_queue.hip), byte offsets: one live bit per queue
// position, the live entries per tile of kRowTile positions and per group of kQGroup tiles, the
// kernels' state.  FeatureCache::alloc_queue reserves `bytes`, compact_queue walks the offsets.
struct CompactLayout { size_t live_bits, tile_cnt, group_sum, state, bytes; };
inline CompactLayout compact_layout(size_t queue_cap) {
  const size_t tiles = (queue_cap + kRowTile - 1) / kRowTile + 1;
  const size_t groups = (tiles + kQGroup - 1) / kQGroup + 1;
  CompactLayout l;
  l.live_bits = 0;
  l.tile_cnt = l.live_bits + align_up(tiles * (kRowTile / 64) * 8, 256);
  l.group_sum = l.tile_cnt + align_up(tiles * 4, 256);
  l.state = l.group_sum + align_up(groups * 4, 256);
  l.bytes = l.state + 256;
  return l;
}

// chunks of kRowTile queue entries the victim walk covers behind the head: twice the rows
// of the block (at most that many victims are needed) + 2
inline size_t victim_chunks(size_t n) { return (2 * n + kRowTile - 1) / kRowTile + 2; }

// entries of the victim staging arrays: list form — the tiles at the front of the list (at most
// the whole list, at most kMaxStageTiles); queue form — the chunks behind the head
inline size_t stage_entries(size_t n, size_t capacity) {
  const size_t list_tiles = (capacity + kRowTile - 1) / kRowTile;
  const size_t list_form = std::min<size_t>(std::min(list_tiles, victim_chunks(n)), kMaxStageTiles);
  return std::max(list_form, victim_chunks(n)) * kRowTile + n;
}

// fused list update: entries of the staged front tiles (the ids they hold; the slots share
// the v_slot / v_pos arrays): at most min(capacity, rows) list positions, in whole tiles
inline size_t fuse_stage_entries(size_t n, size_t capacity) {
  return (std::min(n, capacity) / kFuseTile + 2) * kFuseTile;
}

// rows per wave: 64 for big blocks; fewer for small ones so the block still spreads
// over >= 1024 waves (4 per CU)
inline uint32_t pick_tile_rows(size_t n) {
  // measured on the batch-600 blocks (10k-30k rows): 16 rows per wave beats both 4 (more,
  // shorter waves: 17.8 us/launch) and 32 (16.7 us) at 13.8 us; aim for >= 1024 waves, but
  // never below 16 rows — a 16-row tile of 172-d rows is one trip of 11 loads per lane, and
  // the replay's mid-size blocks (5-16 k rows) ran at 8 rows per wave before: whole replay
  // 14.1-14.3 -> 13.6 us per launch (round 4, same box; 8 rows everywhere: 20.2 us)
  uint32_t t = 64;
  while (t > 16 && (n + t - 1) / t < 1024) t >>= 1;
  return t;
}

// ---- the parts ---------------------------------------------------------------------
// gather.hip: a cache-free context; the round's gather launch (fits tile_rows, picks the kernel)
Ctx plain_ctx(const float* feats, size_t num_rows, size_t dim, const int64_t* ids, size_t n,
              float* out);
void launch_gather(Round& r, hipStream_t stream);
// cache_lru.hip: the LRU contexts' update (list form in one or two launches, queue form: it
// dispatches to cache_lru_fused.hip and cache_lru_queue.hip through cache_lru_dev.hpp);
// own_events: the round's only update launch is the fused one, which then carries the profile's
// dispatch events itself
void launch_lru_update(const Round& r, hipStream_t stream, bool own_events);
void lru_fuse_spins_from_env(int device);   // cache_lru_fused.hip
// cache_select.hip: the LFU / FIFO contexts' update
void launch_select_update(const Round& r, hipStream_t stream);
// feature_cache.hip: one round — the gather, then the updates
void launch_round(Round& r, hipStream_t stream);

}  // namespace gf
