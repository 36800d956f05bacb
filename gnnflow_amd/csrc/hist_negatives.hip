// Historical negatives, on the device: for the edge (s, d, t) in row g of the stream, a
// destination s interacted with STRICTLY BEFORE t that is not d, drawn from s's segment of
// the temporal edge store (edge_store.hpp: one contiguous, chronologically sorted run per
// node).  One launch goes over batches that batch_stream.hip has already assembled and
// overwrites the first Kh of their K negative planes where such a destination exists:
//
//   seg[0 .. c) = the window of s at (t, no lower end, no bound), as history_window.hpp
//          defines it                                                c == 0: the slot is kept
//   u_a  = gf_philox4x32_10_first(seed ^ (GF_HIST_NEG_SEED_TAG + a), tid, epoch)   a < 4
//   cand = seg[(uint64(u_a) * c) >> 32].dst                          tid = g * K + k  (wraps)
//   roots[2B + k*B + i] = the first cand != d;  none in four attempts: kept
//
// A kept slot holds the random draw gf_batch_assemble wrote, so no slot is undefined and the
// fall-back costs nothing.  The tag keeps these draws independent of the random ones of the
// same tid.  Everything else in roots and all of ts is not touched.
//
// A workgroup takes tiles of kTileRows rows.  Its first wave resolves the window ONCE per
// row into LDS; then all lanes take the tile's Kh x rows slots, consecutive lanes consecutive
// rows of one plane, and issue a slot's four candidate reads together: independent 32-byte
// sectors, selected afterwards.  Plain loads and stores, no waiting on another workgroup; the
// optional count of overwritten slots is reduced in the workgroup and added with one atomicAdd
// per workgroup.
#include "hist_negatives.hpp"
#include "common.hpp"
#include "history_window.hpp"

#include "../../include/gnnflow_rng.h"

namespace gf {
namespace {

constexpr int kThreads = 256;
constexpr int kWave = 64;
constexpr int kWaves = kThreads / kWave;
constexpr int kTileRows = 64;             // rows whose history one wave resolves per tile
constexpr uint32_t kMaxGridY = 2048;      // tiles past it are grid-strided

static_assert(kHistNegAttempts == GF_HIST_NEG_ATTEMPTS,
              "gnnflow_hip.h and hist_negatives.hpp disagree on the attempts");
static_assert(kTileRows <= kThreads, "one lane per row of a tile");

struct HistArgs {
  StoreView store;
  const int64_t* src;
  const int64_t* dst;
  const float* time;
  uint64_t rows;             // rows of the stream (bounds of src, dst, time)
  const int64_t* borders;
  uint32_t K, Kh;
  uint64_t seed, epoch, first_row;
  int64_t* roots;
  uint64_t capacity;         // elements roots can hold
  unsigned long long* filled;
};

__global__ void __launch_bounds__(kThreads) hist_negatives_kernel(const HistArgs a) {
  __shared__ const EdgePair* s_seg[kTileRows];
  __shared__ int64_t s_dst[kTileRows];
  __shared__ uint32_t s_c[kTileRows];
  __shared__ uint32_t s_filled[kWaves];
  // borders and slices exactly as batch_assemble_kernel: uniform over the workgroup
  const uint64_t planes = 2u + a.K;
  const int64_t b0 = a.borders[0], l = a.borders[blockIdx.x], h = a.borders[blockIdx.x + 1];
  if (b0 < 0 || l < b0 || h < l || static_cast<uint64_t>(h) > a.rows) return;
  const uint64_t lo = static_cast<uint64_t>(l), hi = static_cast<uint64_t>(h);
  const uint64_t base = (lo - static_cast<uint64_t>(b0)) * planes;
  const uint64_t B = hi - lo;
  if (B == 0 || base + planes * B > a.capacity) return;      // host: rows * planes < 2^62
  int64_t* const neg = a.roots + base + 2 * B;               // K planes of B
  const uint64_t tiles = (B + kTileRows - 1) / kTileRows;
  uint32_t filled = 0;
  for (uint64_t tile = blockIdx.y; tile < tiles; tile += gridDim.y) {
    const uint64_t i0 = tile * kTileRows;                     // < B
    const uint32_t n = B - i0 < kTileRows ? static_cast<uint32_t>(B - i0) : kTileRows;
    if (threadIdx.x < n) {
      const uint64_t row = lo + i0 + threadIdx.x;             // < hi <= rows
      const Window win = window_of(a.store, a.src[row], a.time[row], nullptr, 0, 0);
      s_seg[threadIdx.x] = win.seg;
      s_dst[threadIdx.x] = a.dst[row];
      s_c[threadIdx.x] = win.n;
    }
    __syncthreads();
    const uint32_t slots = a.Kh * n;                          // < 2^16 * 64
    for (uint32_t w = threadIdx.x; w < slots; w += kThreads) {
      const uint32_t k = w / n, r = w - k * n;                // k < Kh, r < n
      const uint64_t c = s_c[r];
      if (c == 0) continue;
      const EdgePair* const seg = s_seg[r];
      const int64_t d = s_dst[r];
      const uint64_t tid = (a.first_row + lo + i0 + r) * a.K + k;      // wraps mod 2^64
      int64_t cand[kHistNegAttempts];
#pragma unroll
      for (int t = 0; t < kHistNegAttempts; ++t) {
        const uint64_t u = gf_philox4x32_10_first(
            a.seed ^ (GF_HIST_NEG_SEED_TAG + static_cast<uint64_t>(t)), tid, a.epoch);
        cand[t] = seg[(u * c) >> 32].dst;                     // (u * c) >> 32 < c: in the window
      }
      int hit = -1;
#pragma unroll
      for (int t = kHistNegAttempts - 1; t >= 0; --t)
        if (cand[t] != d) hit = t;
      if (hit < 0) continue;
      int64_t pick = cand[0];
#pragma unroll
      for (int t = 1; t < kHistNegAttempts; ++t)
        if (hit == t) pick = cand[t];
      neg[static_cast<uint64_t>(k) * B + i0 + r] = pick;      // k * B + i0 + r < Kh * B <= K * B
      ++filled;
    }
    __syncthreads();                                          // the next tile rewrites the LDS
  }
  if (a.filled == nullptr) return;                            // uniform
#pragma unroll
  for (int off = kWave / 2; off >= 1; off >>= 1) filled += __shfl_down(filled, off, kWave);
  if (threadIdx.x % kWave == 0) s_filled[threadIdx.x / kWave] = filled;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t total = 0;
#pragma unroll
    for (int v = 0; v < kWaves; ++v) total += s_filled[v];
    if (total) atomicAdd(a.filled, static_cast<unsigned long long>(total));
  }
}

}  // namespace

void batch_hist_negatives(const GraphView& g, const int64_t* d_src, const int64_t* d_dst,
                          const float* d_time, size_t num_rows, const int64_t* d_borders,
                          size_t num_batches, size_t max_batch_rows, size_t neg_ratio,
                          size_t hist_ratio, uint64_t seed, uint64_t epoch, uint64_t first_row,
                          int64_t* d_roots, size_t capacity, uint64_t* d_filled, int device,
                          hipStream_t stream) {
  const std::string w("batch_hist_negatives");
  GF_REQUIRE(hist_ratio <= neg_ratio, w + ": hist_ratio above neg_ratio");
  GF_REQUIRE(neg_ratio < (size_t(1) << 16), w + ": neg_ratio of 65536 or more");
  GF_REQUIRE(num_rows < (size_t(1) << 44), w + ": more than 2^44 rows");
  GF_REQUIRE(num_batches < (size_t(1) << 31), w + ": 2^31 batches or more");
  if (hist_ratio == 0 || num_batches == 0) return;            // nothing to overwrite
  GF_REQUIRE(d_src && d_dst && d_time, w + ": null src, dst or time");
  GF_REQUIRE(d_borders != nullptr, w + ": null borders");
  GF_REQUIRE(d_roots != nullptr, w + ": null roots");
  const StoreView store = store_view(g);
  if (store.table_len == 0) return;      // no history: every slot keeps its random draw
  HistArgs a = {store, d_src, d_dst, d_time, num_rows, d_borders,
                static_cast<uint32_t>(neg_ratio), static_cast<uint32_t>(hist_ratio), seed, epoch,
                first_row, d_roots, capacity, reinterpret_cast<unsigned long long*>(d_filled)};
  DeviceGuard dg(device);
  const uint64_t tiles = (static_cast<uint64_t>(max_batch_rows) + kTileRows - 1) / kTileRows;
  const dim3 grid(static_cast<uint32_t>(num_batches),
                  static_cast<uint32_t>(std::min<uint64_t>(std::max<uint64_t>(tiles, 1), kMaxGridY)));
  hist_negatives_kernel<<<grid, dim3(kThreads), 0, stream>>>(a);
  GF_HIP(hipGetLastError());
}

}  // namespace gf
