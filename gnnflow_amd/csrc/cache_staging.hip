// ---- staging ring: rows of a HOST-resident table pulled into HBM ahead of the gather ----------
// Reference: the tables live in host memory and every miss travels host -> pinned -> device inside
// fetch_feature (cache.py:288-313,381-388, utils.py:284-297).  Here the ids of batch i+1 exist
// while batch i is fetched (ReplayPipeline), so a kernel on a side stream pulls the table rows of
// the ids that are not cached into a ring in HBM — over PCIe, beside the fetch chain — and the
// gather then takes a missed row from the ring.  The ring is G regions of C rows, one region per
// prefetch GENERATION; pmap[id] = {generation, row in its region} of the newest staging of id and
// of the one before it.  A prefetch stages an id only
// if it is neither cached (nor claimed by the fetch in flight) nor staged in a generation that is
// still readable, so a row pulled for one batch (the batch's own target edges, above all: the next
// batches sample exactly those) serves the misses of the next G - D - 1 batches too.  It is a
// HINT: the cache's state (map, slots, hit counts) never depends on it, and an id the speculation
// missed — evicted by the update in between, or a region that was full — is read from the host
// table by the gather as before.  Rows are feats[ids] bit for bit either way.
#include "feature_cache_ctx.hpp"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <type_traits>

namespace gf {

namespace {

// claim: one thread per block row.  A row whose id is neither cached nor staged in a readable
// generation takes the next row of this generation's region (one atomic per wave) and settles the
// id's pmap entry with a compare-and-swap — of several rows with the same id one wins, the others'
// region rows stay unused.
__global__ __launch_bounds__(256) void stage_claim_kernel(StageRound r) {
  const StageCtx& c = r.c[blockIdx.y];
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t region = c.gen & c.mask, span = c.gen - c.lo;
  for (uint32_t base = blockIdx.x * 256u; base < c.n; base += gridDim.x * 256u) {
    const uint32_t i = base + threadIdx.x;
    long long id = -1;
    unsigned long long p = 0;
    bool want = false;
    if (i < c.n) {
      id = c.ids[i];
      if (id >= 0 && static_cast<uint64_t>(id) < c.num_ids) {
        // (a negative map value other than kAbsent is the claim of a fetch in flight; its update
        // installs the id — unless the block misses more ids than the cache has slots, a small
        // cache's every step — so it counts as absent: an id the fetch in flight misses is in
        // the ring already and costs nothing here)
        const int32_t slot = c.map ? c.map[id] : kAbsent;
        bool maybe = slot < 0;
        if (slot >= 0 && c.qpos) {
          uint32_t at = c.qpos[slot];
          if (c.qstate) at -= c.qstate->head;
          maybe = at < c.risk;
        }
        if (maybe) {
          p = c.pmap[2 * id];
          want = static_cast<uint32_t>(p >> 32) - c.lo > span;
        }
      }
    }
    const unsigned long long wm = __ballot(want);
    if (!wm) continue;
    const int leader = __ffsll(static_cast<long long>(wm)) - 1;
    uint32_t wbase = 0;
    if (static_cast<int>(lane) == leader)
      wbase = atomicAdd(&c.region_rows[region], static_cast<uint32_t>(__popcll(wm)));
    wbase = __shfl(wbase, leader, 64);
    const uint32_t pos = wbase + static_cast<uint32_t>(__popcll(wm & ((1ull << lane) - 1ull)));
    if (!want || pos >= c.cap) continue;
    const unsigned long long mine = (static_cast<unsigned long long>(c.gen) << 32) | pos;
    long long staged = -1;   // a row of the region that nobody reads is not pulled either
    for (;;) {
      // (the entry it replaces stays behind it: launches already in flight read the id there)
      c.pmap[2 * id + 1] = p;
      const unsigned long long old = atomicCAS(&c.pmap[2 * id], p, mine);
      if (old == p) { staged = id; break; }
      if (static_cast<uint32_t>(old >> 32) - c.lo <= span) break;   // another row of this id was first
      p = old;
    }
    c.region_ids[pos] = staged;
  }
}

// pull: the rows the claim kernel settled, host table -> this generation's region of the ring.
// A wave owns 8 consecutive ring rows — one contiguous run of stores — and keeps 2 16-byte loads
// per lane in flight over the host link (PCIe round trips are ~2 us: what counts is the number of
// reads in flight, which the number of waves provides — 6 per lane was 1.3 us per step slower in
// every grid shape, profiles/r06_pinned_pull_arrangements.txt — and every wave of the grid has
// its own rows; a first version that copied the winners of a 256-row tile inside the claim
// workgroup took 82 us for the 600 target rows of three workgroups).
// kOdd: rows whose width is not a multiple of 4 floats move as 16-byte vectors at 4-byte alignment,
// the last one ending with the row (as the gather's odd path: GDELT's 186-d / 413-d rows went as
// single floats at first — 256 B per load on the link)
template <typename VecT, bool kOdd, uint32_t K>
__device__ inline void stage_pull_body(const PullJob& j, uint32_t n) {
  constexpr uint32_t kRows = 8;
  using Unit = std::conditional_t<kOdd, float, VecT>;
  constexpr uint32_t kVF = kOdd ? 4u : 1u;   // Units per VecT
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = (blockIdx.x * 256u + threadIdx.x) >> 6, nwaves = gridDim.x * 4u;
  const uint32_t dimv = kOdd ? (j.dim + 3u) / 4u : j.dim / (sizeof(VecT) / sizeof(float));
  const uint32_t rowu = kOdd ? j.dim : dimv;
  const Unit* feats = reinterpret_cast<const Unit*>(j.feats);
  Unit* dst = reinterpret_cast<Unit*>(j.dst);
  for (uint32_t row0 = wave * kRows; row0 < n; row0 += nwaves * kRows) {
    const uint32_t rows = min(kRows, n - row0);
    const long long id = lane < rows ? j.ids[row0 + lane] : -1;
    const uint32_t valid = static_cast<uint32_t>(__popcll(__ballot(id >= 0)));
    if (lane == 0 && valid) atomicAdd(j.pulled, static_cast<unsigned long long>(valid));
    const uint32_t total = rows * dimv;
    Unit* o = dst + static_cast<uint64_t>(row0) * rowu;
    for (uint32_t base = 0; base < total; base += 64u * K) {
      VecT v[K];
      uint32_t at[K], ok = 0;   // (a bit per load: an array of flags went to scratch)
#pragma unroll
      for (uint32_t k = 0; k < K; ++k) {
        const uint32_t f = base + lane + 64u * k;
        const uint32_t rr = f < total ? f / dimv : 0u;
        const uint32_t cc = f - rr * dimv;
        const uint32_t off = kOdd ? min(cc * kVF, rowu - kVF) : cc;
        at[k] = rr * rowu + off;
        const long long src = __shfl(id, rr, 64);     // (every lane executes the cross-lane read)
        if (f < total && src >= 0) {
          v[k] = *reinterpret_cast<const VecT*>(feats + static_cast<uint64_t>(src) * rowu + off);
          ok |= 1u << k;
        }
      }
#pragma unroll
      for (uint32_t k = 0; k < K; ++k)
        if (ok & (1u << k)) *reinterpret_cast<VecT*>(o + at[k]) = v[k];
    }
  }
}

__global__ __launch_bounds__(256) void stage_pull_kernel(PullJobs jobs) {
  // (selected, not indexed: a dynamic index into the by-value argument sent it to scratch)
  const PullJob j = blockIdx.y == 0 ? jobs.j[0] : jobs.j[1];
  const uint32_t n = min(*j.region_rows, j.cap);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    *j.next_rows = 0u;   // (prefetch generations run in order on one stream)
  }
  // (nf4 / uf4, the clang vector types: an array of HIP's float4 went to scratch here)
  if (j.vec4) stage_pull_body<nf4, false, 2>(j, n);
  else if (j.dim >= 4u) stage_pull_body<uf4, true, 2>(j, n);
  else stage_pull_body<float, false, 6>(j, n);
}

}  // namespace

// ---- staging ring, host side ---------------------------------------------------------------
static std::atomic<uint64_t> g_stage_stream_waits{0};

void FeatureCache::set_staging(size_t generations, size_t rows_per_generation) {
  DeviceGuard dg(device_);
  GF_HIP(hipDeviceSynchronize());   // (a configuration call: nothing of this cache is in flight after it)
  if (generations == 0 || rows_per_generation == 0) {
    stage_gens_ = stage_cap_ = 0;
    ring_.release();
    pmap_.release();
    region_rows_.release();
    region_ids_.release();
    synced_gen_ = 0;
    return;
  }
  GF_REQUIRE(!table_on_device_, "staging ring: the feature table is already in device memory");
  GF_REQUIRE(generations >= 2 * kStageAhead && generations <= 64 &&
                 (generations & (generations - 1)) == 0,
             "staging ring: generations must be a power of two in 8..64");
  GF_REQUIRE(rows_per_generation < (size_t{1} << 31), "staging ring: too many rows per generation");
  stage_gens_ = static_cast<uint32_t>(generations);
  stage_cap_ = static_cast<uint32_t>(rows_per_generation);
  ring_.release();
  ring_.reserve(generations * rows_per_generation * dim_ * sizeof(float) + 16);
  pmap_.reserve(std::max<size_t>(2 * num_ids_ * sizeof(unsigned long long), 16));
  region_rows_.reserve(64 * sizeof(uint32_t) + 64);   // + rows pulled, + rows read from the host, + ticket
  region_ids_.release();
  region_ids_.reserve(rows_per_generation * sizeof(long long) + 16);
  progress_.reserve(64);
  *progress_.as<volatile uint32_t>() = 0;
  for (hipEvent_t& e : stage_events_)
    if (!e) GF_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  GF_HIP(hipMemset(pmap_.data(), 0, pmap_.bytes()));
  GF_HIP(hipMemset(region_rows_.data(), 0, region_rows_.bytes()));
  gen_issued_ = 0;
  stage_reads_ = 0;
  stage_read_pending_ = false;
  synced_gen_ = 0;
  std::memset(gen_event_, 0, sizeof(gen_event_));
  std::memset(reads_at_gen_, 0, sizeof(reads_at_gen_));
}

void FeatureCache::invalidate_staging() {
  if (!staging()) return;
  // every entry staged so far falls out of every window a later launch accepts; the regions
  // the skipped generations would have used are simply never read
  gen_issued_ += stage_gens_ + 1;
  for (uint32_t& v : reads_at_gen_) v = stage_reads_;
  DeviceGuard dg(device_);
  GF_HIP(hipDeviceSynchronize());
  GF_HIP(hipMemset(region_rows_.data(), 0, 64 * sizeof(uint32_t)));
  *progress_.as<volatile uint32_t>() = stage_reads_;   // (device idle: every launch has finished)
  synced_gen_ = gen_issued_;
  std::memset(gen_event_, 0, sizeof(gen_event_));
}

void FeatureCache::staging_state(uint64_t out[9]) {
  out[7] = static_cast<uint64_t>(stage_spin_us_);
  out[8] = g_stage_stream_waits.load(std::memory_order_relaxed);
  out[0] = stage_gens_;
  out[1] = stage_cap_;
  out[2] = gen_issued_;
  out[3] = stage_drops_;
  out[4] = 0;
  out[5] = staging() ? ring_.bytes() + pmap_.bytes() : 0;
  out[6] = 0;
  if (staging()) {
    DeviceGuard dg(device_);
    GF_HIP(hipDeviceSynchronize());
    unsigned long long v[2] = {0, 0};
    GF_HIP(hipMemcpy(v, region_rows_.as<uint32_t>() + 64, sizeof(v), hipMemcpyDeviceToHost));
    out[4] = v[0];
    out[6] = v[1];
  }
}

// The window of generations a launch may read when `issued` is the newest one: region g & mask
// is rewritten by generation g + G, and up to kStageAhead newer generations may be pulled while
// the launch runs.
static inline uint32_t stage_window_lo(uint32_t issued, uint32_t gens, uint32_t ahead) {
  const uint32_t keep = gens - ahead;   // generations issued, issued - 1, ..., issued - keep + 1
  return issued >= keep ? issued - keep + 1u : 1u;
}

// The next generation X rewrites the region of generation X - G.  Launches that may read that
// region were enqueued before generation X - kStageAhead was issued; they are known to have
// finished once a LATER ring-reading launch has started (it stores the number of such launches
// before it in `progress`).  The issuing thread waits for that — it is what keeps the host from
// running arbitrarily far ahead of the fetch stream, where a prefetch would see a cache state
// many updates old — and gives the generation up after GNNFLOW_STAGE_SPIN_US (a hint may be
// dropped; waiting for ever may not: nothing guarantees that the caller fetches again).
bool FeatureCache::stage_advance() {
  const uint32_t next = gen_issued_ + 1u;
  if (next > kStageAhead) {
    const uint32_t need = reads_at_gen_[(next - kStageAhead) & 63u];
    volatile uint32_t* progress = progress_.as<volatile uint32_t>();
    if (static_cast<int32_t>(*progress - need) < 0) {
      static const long spin_us = [] {
        const char* v = std::getenv("GNNFLOW_STAGE_SPIN_US");
        return v ? std::atol(v) : 20000L;
      }();
      bool ok = false;
      const auto t_spin = std::chrono::steady_clock::now();
      if (stage_reads_ != need && spin_us > 0) {   // (== : no later launch exists that could report)
        const auto t0 = std::chrono::steady_clock::now();
        for (uint32_t i = 0;; ++i) {
          if (static_cast<int32_t>(*progress - need) >= 0) { ok = true; break; }
          __builtin_ia32_pause();
          if ((i & 255u) == 255u &&
              std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(spin_us)) break;
        }
      }
      stage_spin_us_ += std::chrono::duration<double, std::micro>(
                            std::chrono::steady_clock::now() - t_spin).count();
      if (!ok) { ++stage_drops_; return false; }
    }
  }
  gen_issued_ = next;
  reads_at_gen_[next & 63u] = stage_reads_;
  return true;
}

// the fetch stream waits for the prefetches issued so far (one wait per distinct event)
// The newest generation a fetch issued now depends on: all but the `stage_lag_` newest.
uint32_t FeatureCache::stage_hi() const {
  return gen_issued_ > stage_lag_ ? gen_issued_ - stage_lag_ : 0u;
}

// The fetch stream waits for the pulls this fetch depends on — the generations up to stage_hi(),
// i.e. for the newest of them (the pull stream runs them in order).  An event that has completed
// by now — the usual case when the loop announces a batch two steps ahead of its fetch
// (gf_cache_set_staging_lag) — costs one query; one that has not is handed to the stream, whose
// wait for another queue's signal takes 12-20 us to resolve.
void FeatureCache::stage_sync(hipStream_t stream, hipEvent_t* seen, int* num_seen) {
  const uint32_t hi = stage_hi();
  if (!staging() || hi == 0 || hi <= synced_gen_) return;
  synced_gen_ = hi;
  hipEvent_t ev = gen_event_[hi % kStageEvents];
  if (!ev) return;
  for (int i = 0; i < *num_seen; ++i)
    if (seen[i] == ev) return;
  seen[(*num_seen)++] = ev;
  const hipError_t q = hipEventQuery(ev);
  if (q == hipSuccess) return;
  if (q != hipErrorNotReady) GF_HIP(q);
  (void)hipGetLastError();
  g_stage_stream_waits.fetch_add(1, std::memory_order_relaxed);
  GF_HIP(hipStreamWaitEvent(stream, ev, 0));
}

// Context of one block for the generation just taken (stage_advance).
bool FeatureCache::stage_begin(StageCtx* stage_ctx_out, const int64_t* d_ids, size_t n, bool cached) {
  StageCtx& c = *stage_ctx_out;
  std::memset(&c, 0, sizeof(c));
  c.ids = d_ids;
  c.n = static_cast<uint32_t>(n);
  c.map = (cached && capacity_) ? map_.as<int32_t>() : nullptr;
  c.num_ids = num_ids_;
  c.pmap = pmap_.as<unsigned long long>();
  c.region_rows = region_rows_.as<uint32_t>();
  c.region_ids = region_ids_.as<long long>();
  c.gen = gen_issued_;
  // (an id staged in one of the two oldest readable generations is staged again: its fetch is
  // issued one to three generations from now, when those have left the window)
  c.lo = std::min(gen_issued_, stage_window_lo(gen_issued_, stage_gens_, kStageAhead) + kStageAhead - 1u);
  c.mask = stage_gens_ - 1u;
  c.cap = stage_cap_;
  // (only a cache that kStageAhead blocks of this size can turn over: for a larger one the
  // entries at the front of the order are rarely among a block's hits, and the rule pulled 370
  // rows per step for the headline's edge cache — 134 k slots, 9.5 k-row blocks — to save 4)
  if (c.map && policy_ == GF_CACHE_LRU &&
      capacity_ <= size_t{kStageAhead} * n) {
    c.qpos = qpos_.as<uint32_t>();
    c.qstate = queue_form_ ? qstate_.as<QueueState>() : nullptr;
    c.risk = static_cast<uint32_t>(capacity_);
  }
  return true;
}

// ... and the pull of what its blocks claimed
void FeatureCache::stage_pull(PullJob* pull_job_out) {
  PullJob& j = *pull_job_out;
  const uint32_t region = gen_issued_ & (stage_gens_ - 1u);
  j.ids = region_ids_.as<long long>();
  j.feats = feats_;
  j.dst = ring_.as<float>() + static_cast<uint64_t>(region) * stage_cap_ * dim_;
  j.region_rows = region_rows_.as<uint32_t>() + region;
  j.next_rows = region_rows_.as<uint32_t>() + ((gen_issued_ + 1u) & (stage_gens_ - 1u));
  j.pulled = reinterpret_cast<unsigned long long*>(region_rows_.as<uint32_t>() + 64);
  j.cap = stage_cap_;
  j.dim = static_cast<uint32_t>(dim_);
  j.vec4 = vec4_ok(dim_, feats_, ring_.data(), ring_.data()) ? 1u : 0u;
}

void FeatureCache::stage_fill(Ctx* ctx_out) {
  const uint32_t hi = stage_hi();
  if (!staging() || hi == 0) return;
  Ctx& c = *ctx_out;
  if (c.miss_rows || c.remap) return;
  c.pmap = pmap_.as<unsigned long long>();
  c.ring = ring_.as<float>();
  // (the window's lower end follows the newest generation ISSUED: that one's successors are the
  // ones that may overwrite regions while this launch runs)
  c.st_lo = stage_window_lo(gen_issued_, stage_gens_, kStageAhead);
  if (hi < c.st_lo) return;
  c.st_span = hi - c.st_lo;
  c.st_mask = stage_gens_ - 1u;
  c.st_cap = stage_cap_;
  c.progress = progress_.as<uint32_t>();
  c.progress_val = stage_reads_;
  c.st_fallback = reinterpret_cast<unsigned long long*>(region_rows_.as<uint32_t>() + 66);
  stage_read_pending_ = true;
}

void FeatureCache::stage_round_done() {
  if (stage_read_pending_) {
    ++stage_reads_;
    stage_read_pending_ = false;
  }
}

// Cache.prefetch_feature: one staging generation per cache for the blocks a coming
// fetch_blocks(descs) will gather (feature_cache.hpp)
bool prefetch_blocks(FeatureCache* node, FeatureCache* edge, const gf_fetch_desc* descs, size_t n,
                     hipStream_t stream) {
  GF_REQUIRE(descs != nullptr || n == 0, "prefetch_blocks: null descriptors");
  const bool node_on = node && node->staging(), edge_on = edge && edge->staging();
  if (!node_on && !edge_on) return false;
  const int device = node ? node->device() : edge->device();
  DeviceGuard dg(device);
  bool node_use = false, edge_use = false;
  for (size_t i = 0; i < n; ++i) {
    const gf_fetch_desc& d = descs[i];
    GF_REQUIRE(d.kind >= 0 && d.kind <= 2, "prefetch_blocks: bad kind");
    if (d.n == 0) continue;
    GF_REQUIRE(d.d_ids != nullptr, "prefetch_blocks: null ids");
    GF_REQUIRE(d.n < 0x7FFFFFFFull, "prefetch_blocks: more than 2^31-1 rows in one block");
    if (d.kind == 0) node_use = node_use || node_on;
    else edge_use = edge_use || edge_on;
  }
  if (node_use) node_use = node->stage_advance();
  if (edge_use) edge_use = edge->stage_advance();
  if (!node_use && !edge_use) return false;
  size_t max_n = 0, node_rows = 0, edge_rows = 0;
  StageRound r;
  r.count = 0;
  auto flush = [&] {
    if (r.count == 0) return;
    const unsigned grid = static_cast<unsigned>(std::max<size_t>(1, std::min<size_t>((max_n + 255) / 256, 512)));
    stage_claim_kernel<<<dim3(grid, r.count), dim3(256), 0, stream>>>(r);
    GF_HIP(hipGetLastError());
    r.count = 0;
    max_n = 0;
  };
  for (size_t i = 0; i < n; ++i) {
    const gf_fetch_desc& d = descs[i];
    if (d.n == 0) continue;
    FeatureCache* c = d.kind == 0 ? (node_use ? node : nullptr) : (edge_use ? edge : nullptr);
    if (!c) continue;
    c->stage_begin(&r.c[r.count++], d.d_ids, d.n, d.kind != 2);
    max_n = std::max(max_n, d.n);
    (d.kind == 0 ? node_rows : edge_rows) += d.n;
    if (r.count == kMaxCtx) flush();
  }
  flush();
  {
    PullJobs jobs;
    jobs.count = 0;
    size_t most = 0;
    if (node_use) {
      node->stage_pull(&jobs.j[jobs.count++]);
      most = std::max(most, std::min<size_t>(node_rows, node->stage_cap_));
    }
    if (edge_use) {
      edge->stage_pull(&jobs.j[jobs.count++]);
      most = std::max(most, std::min<size_t>(edge_rows, edge->stage_cap_));
    }
    // 8 rows per wave, 4 waves per workgroup; the kernel reads the rows really claimed
    // (grid-stride: 64 workgroups = 256 waves; 192 stretched the GDELT-scale gathers beside the pull from 254 to 578 us)
    const unsigned grid = static_cast<unsigned>(std::max<size_t>(1, std::min<size_t>((most + 31) / 32, 64)));
    stage_pull_kernel<<<dim3(grid, jobs.count), dim3(256), 0, stream>>>(jobs);
    GF_HIP(hipGetLastError());
  }
  FeatureCache* lead = edge_use ? edge : node;
  hipEvent_t ev = lead->stage_events_[lead->gen_issued_ % FeatureCache::kStageEvents];
  GF_HIP(hipEventRecord(ev, stream));
  if (node_use) node->gen_event_[node->gen_issued_ % FeatureCache::kStageEvents] = ev;
  if (edge_use) edge->gen_event_[edge->gen_issued_ % FeatureCache::kStageEvents] = ev;
  return true;
}

}  // namespace gf
