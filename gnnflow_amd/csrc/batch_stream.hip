// The first stage of a training step, on the device: what the reference's utils.get_batch does
// on the host per batch (slice four columns, draw the negatives from a host RandomState,
// concatenate twice, then two pageable host-to-device copies).  Here the edge stream and the
// ascending list `dl` of distinct destinations live in HBM and one launch writes a batch:
//
//   roots[0:B]          = src[lo:hi]                  B = hi - lo
//   roots[B:2B]         = dst[lo:hi]
//   roots[2B + k*B + i] = dl[(uint64(u) * M) >> 32]   u = gf_philox4x32_10_first(seed, tid, epoch)
//   ts[j*B + i]         = time[lo + i]   j < 2 + K    tid = (first_row + lo + i) * K + k  (wraps)
//
// k-major, the layout ops.link_metrics documents.  The key of a draw is the edge's GLOBAL row,
// not its place in the batch: an edge gets the same negatives whatever the batch size, the
// random start or the rank that takes the batch.  M is read from device memory, so the set may
// grow without the host learning its size.  M == 0 or M >= 2^32 (no draw is defined): -1.
//
// A plain streaming copy plus one Philox per negative.  One work item is (plane j, four
// consecutive rows); consecutive lanes take consecutive quads of one plane, so every load and
// store of a wave is one contiguous run.  A quad moves as 16-byte loads and stores where the
// addresses allow it — decided per batch, uniformly over the workgroup — and row by row
// otherwise (an odd lo, a B that is no multiple of 4, the last, partial quad).  Every output
// address is written exactly once; no atomics, no LDS.
//
// The many-batch form takes the batch index from blockIdx.x and reads its borders from device
// memory; batch b's slices start at (2 + K) * (borders[b] - borders[0]).  A batch whose borders
// are not ascending, reach past the stream or whose slices would pass `capacity` writes nothing.
//
// The destination set is a bitmap of num_nodes bits.  dst_set_mark ORs the bit of each id in
// (atomicOr on the 64-bit word, skipped when the bit is already there) and counts ids outside
// [0, num_nodes) in a device counter.  dst_set_compact turns the bitmap into the ascending list in
// three launches: per-tile popcount, an exclusive scan of the tile counts by ONE workgroup, and
// an emit that rescans inside its tile.  No kernel waits on another workgroup.
#include "batch_stream.hpp"
#include "common.hpp"

#include "../../include/gnnflow_rng.h"

namespace gf {
namespace {

constexpr int kThreads = 256;
constexpr int kWave = 64;
constexpr int kWaves = kThreads / kWave;
constexpr uint32_t kMaxGridY = 2048;      // work past it is grid-strided

struct AssembleArgs {
  const int64_t* src;        // nullptr: negatives only
  const int64_t* dst;
  const float* time;
  uint64_t rows;             // rows of the stream (bounds of src, dst, time)
  const int64_t* borders;    // nullptr: the one batch [lo, hi)
  uint64_t lo, hi;
  uint32_t K;
  const int64_t* dl;
  const int64_t* dl_count;
  uint64_t seed, epoch, first_row;
  int64_t* roots;
  float* ts;
  uint64_t capacity;         // elements roots (and ts) can hold
};

template <bool kNegOnly>
__global__ void __launch_bounds__(kThreads) batch_assemble_kernel(const AssembleArgs a) {
  const uint64_t planes = (kNegOnly ? 0u : 2u) + a.K;
  uint64_t lo = a.lo, hi = a.hi, base = 0;
  if (a.borders) {
    const int64_t b0 = a.borders[0], l = a.borders[blockIdx.x], h = a.borders[blockIdx.x + 1];
    if (b0 < 0 || l < b0 || h < l || static_cast<uint64_t>(h) > a.rows) return;
    lo = static_cast<uint64_t>(l);
    hi = static_cast<uint64_t>(h);
    base = (lo - static_cast<uint64_t>(b0)) * planes;
  }
  const uint64_t B = hi - lo;
  if (B == 0 || base + planes * B > a.capacity) return;      // host: rows * planes < 2^62
  int64_t* const roots = a.roots + base;
  float* const ts = kNegOnly ? nullptr : a.ts + base;
  // uniform over the workgroup: which sides of a full quad move 16 bytes at a time
  const bool vec_in = !kNegOnly && aligned16(a.src + lo) && aligned16(a.dst + lo);
  const bool vec_time = !kNegOnly && aligned16(a.time + lo);
  const bool vec_roots = aligned16(roots) && (B & 1u) == 0;      // j * B + 4 q even
  const bool vec_ts = !kNegOnly && aligned16(ts) && (B & 3u) == 0;
  uint64_t M = 0;
  if (a.K) {
    const int64_t m = *a.dl_count;
    M = m > 0 && m < (int64_t(1) << 32) ? static_cast<uint64_t>(m) : 0;
  }
  const uint64_t Q = (B + 3) / 4;
  const uint64_t total = Q * planes;
  const uint64_t stride = static_cast<uint64_t>(gridDim.y) * kThreads;
  for (uint64_t w = static_cast<uint64_t>(blockIdx.y) * kThreads + threadIdx.x; w < total;
       w += stride) {
    const uint64_t j = w / Q, q = w - j * Q;
    const uint64_t i0 = q * 4;                                  // < B
    const uint32_t n = B - i0 < 4 ? static_cast<uint32_t>(B - i0) : 4u;
    const bool full = n == 4;
    int64_t r[4] = {0, 0, 0, 0};
    if (!kNegOnly && j < 2) {
      const int64_t* p = (j == 0 ? a.src : a.dst) + lo + i0;    // lo + i0 + n <= hi <= rows
      if (full && vec_in) {
        const longlong2 x = reinterpret_cast<const longlong2*>(p)[0];
        const longlong2 y = reinterpret_cast<const longlong2*>(p)[1];
        r[0] = x.x; r[1] = x.y; r[2] = y.x; r[3] = y.y;
      } else {
        for (uint32_t e = 0; e < n; ++e) r[e] = p[e];
      }
    } else {
      const uint64_t k = j - (kNegOnly ? 0u : 2u);
      for (uint32_t e = 0; e < n; ++e) {
        const uint64_t tid = (a.first_row + lo + i0 + e) * a.K + k;      // wraps mod 2^64
        const uint64_t u = gf_philox4x32_10_first(a.seed, tid, a.epoch);
        r[e] = M ? a.dl[(u * M) >> 32] : -1;                    // (u * M) >> 32 < M
      }
    }
    int64_t* const o = roots + j * B + i0;                      // j * B + i0 + n <= planes * B
    if (full && vec_roots) {
      longlong2 x, y;
      x.x = r[0]; x.y = r[1]; y.x = r[2]; y.y = r[3];
      reinterpret_cast<longlong2*>(o)[0] = x;
      reinterpret_cast<longlong2*>(o)[1] = y;
    } else {
      for (uint32_t e = 0; e < n; ++e) o[e] = r[e];
    }
    if (kNegOnly) continue;
    const float* const tp = a.time + lo + i0;
    float* const to = ts + j * B + i0;
    if (full && vec_time && vec_ts) {
      *reinterpret_cast<float4*>(to) = *reinterpret_cast<const float4*>(tp);
    } else if (full && vec_time) {
      const float4 t = *reinterpret_cast<const float4*>(tp);
      to[0] = t.x; to[1] = t.y; to[2] = t.z; to[3] = t.w;
    } else if (full && vec_ts) {
      float4 t;
      t.x = tp[0]; t.y = tp[1]; t.z = tp[2]; t.w = tp[3];
      *reinterpret_cast<float4*>(to) = t;
    } else {
      for (uint32_t e = 0; e < n; ++e) to[e] = tp[e];
    }
  }
}

uint32_t grid_y(uint64_t max_rows, uint64_t planes) {
  const uint64_t items = (max_rows + 3) / 4 * planes;
  const uint64_t blocks = (items + kThreads - 1) / kThreads;
  return static_cast<uint32_t>(std::min<uint64_t>(std::max<uint64_t>(blocks, 1), kMaxGridY));
}

void check_common(const char* who, bool neg_only, const int64_t* d_src, const int64_t* d_dst,
                  const float* d_time, size_t num_rows, size_t neg_ratio, const int64_t* d_dl,
                  const int64_t* d_dl_count, int64_t* d_roots, float* d_ts) {
  const std::string w(who);
  GF_REQUIRE(neg_ratio < (size_t(1) << 16), w + ": neg_ratio of 65536 or more");
  GF_REQUIRE(num_rows < (size_t(1) << 44), w + ": more than 2^44 rows");
  GF_REQUIRE(d_roots != nullptr, w + ": null roots");
  GF_REQUIRE(neg_ratio == 0 || (d_dl != nullptr && d_dl_count != nullptr),
             w + ": negatives asked for without a destination list and its count");
  if (neg_only) {
    GF_REQUIRE(d_dst == nullptr && d_time == nullptr && d_ts == nullptr,
               w + ": without src (negatives only) dst, time and ts must be null too");
  } else {
    GF_REQUIRE(d_src && d_dst && d_time && d_ts, w + ": null src, dst, time or ts");
  }
}

// ---- destination set --------------------------------------------------------------------
constexpr int kWordsPerThread = kDstSetTileWords / kThreads;
static_assert(kWordsPerThread * kThreads == kDstSetTileWords, "a tile is whole threads");

__global__ void __launch_bounds__(kThreads)
dst_set_mark_kernel(const int64_t* __restrict__ ids, uint64_t n, unsigned long long* bitmap,
                    uint64_t num_nodes, unsigned long long* out_of_range) {
  const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kThreads;
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x; i < n;
       i += stride) {
    const uint64_t id = static_cast<uint64_t>(ids[i]);      // a negative id is a huge one
    if (id >= num_nodes) {
      atomicAdd(out_of_range, 1ull);
      continue;
    }
    const unsigned long long bit = 1ull << (id & 63u);
    unsigned long long* const word = bitmap + (id >> 6);    // id < num_nodes: inside the bitmap
    if (!(*word & bit)) atomicOr(word, bit);
  }
}

// popcount of this thread's kWordsPerThread consecutive words of tile blockIdx.x
__device__ __forceinline__ uint32_t load_words(const uint64_t* __restrict__ bitmap,
                                               uint64_t num_words, uint64_t first,
                                               uint64_t (&w)[kWordsPerThread]) {
  uint32_t c = 0;
#pragma unroll
  for (int e = 0; e < kWordsPerThread; ++e) {
    w[e] = first + e < num_words ? bitmap[first + e] : 0ull;
    c += static_cast<uint32_t>(__popcll(w[e]));
  }
  return c;
}

__global__ void __launch_bounds__(kThreads)
dst_set_tile_count_kernel(const uint64_t* __restrict__ bitmap, uint64_t num_words,
                          uint32_t* __restrict__ tile_counts) {
  __shared__ uint32_t s[kWaves];
  uint64_t w[kWordsPerThread];
  const uint64_t first = static_cast<uint64_t>(blockIdx.x) * kDstSetTileWords +
                         static_cast<uint64_t>(threadIdx.x) * kWordsPerThread;
  uint32_t c = load_words(bitmap, num_words, first, w);
#pragma unroll
  for (int off = kWave / 2; off >= 1; off >>= 1) c += __shfl_down(c, off, kWave);
  if (threadIdx.x % kWave == 0) s[threadIdx.x / kWave] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t t = 0;
#pragma unroll
    for (int v = 0; v < kWaves; ++v) t += s[v];
    tile_counts[blockIdx.x] = t;
  }
}

// one workgroup: tile_offsets[t] = sum of tile_counts[0:t], count[0] = min(total, capacity)
__global__ void __launch_bounds__(kThreads)
dst_set_tile_scan_kernel(const uint32_t* __restrict__ tile_counts, uint64_t tiles,
                         uint64_t* __restrict__ tile_offsets, uint64_t capacity,
                         int64_t* __restrict__ count) {
  __shared__ uint64_t s[kThreads];
  const uint64_t per = (tiles + kThreads - 1) / kThreads;
  const uint64_t t0 = std::min<uint64_t>(threadIdx.x * per, tiles);
  const uint64_t t1 = std::min<uint64_t>(t0 + per, tiles);
  uint64_t own = 0;
  for (uint64_t t = t0; t < t1; ++t) own += tile_counts[t];
  s[threadIdx.x] = own;
  __syncthreads();
  uint64_t run = 0;
  for (uint32_t v = 0; v < threadIdx.x; ++v) run += s[v];
  if (threadIdx.x == kThreads - 1) {
    const uint64_t total = run + own;
    *count = static_cast<int64_t>(total < capacity ? total : capacity);
  }
  for (uint64_t t = t0; t < t1; ++t) {
    tile_offsets[t] = run;
    run += tile_counts[t];
  }
}

__global__ void __launch_bounds__(kThreads)
dst_set_emit_kernel(const uint64_t* __restrict__ bitmap, uint64_t num_words,
                    const uint64_t* __restrict__ tile_offsets, int64_t* __restrict__ ids,
                    uint64_t capacity) {
  __shared__ uint32_t s[kWaves];
  uint64_t w[kWordsPerThread];
  const uint64_t first = static_cast<uint64_t>(blockIdx.x) * kDstSetTileWords +
                         static_cast<uint64_t>(threadIdx.x) * kWordsPerThread;
  const uint32_t c = load_words(bitmap, num_words, first, w);
  const uint32_t lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
  uint32_t incl = c;      // inclusive scan over the wave
#pragma unroll
  for (int off = 1; off < kWave; off <<= 1) {
    const uint32_t up = __shfl_up(incl, off, kWave);
    if (lane >= static_cast<uint32_t>(off)) incl += up;
  }
  if (lane == kWave - 1) s[wave] = incl;
  __syncthreads();
  uint64_t pos = tile_offsets[blockIdx.x] + (incl - c);
  for (uint32_t v = 0; v < wave; ++v) pos += s[v];
#pragma unroll
  for (int e = 0; e < kWordsPerThread; ++e) {
    uint64_t x = w[e];
    const uint64_t id0 = (first + e) << 6;
    while (x) {
      const int b = __ffsll(static_cast<unsigned long long>(x)) - 1;
      if (pos < capacity) ids[pos] = static_cast<int64_t>(id0 + b);
      ++pos;
      x &= x - 1;
    }
  }
}

uint64_t words_of(size_t num_nodes) { return (static_cast<uint64_t>(num_nodes) + 63) / 64; }
uint64_t tiles_of(size_t num_nodes) {
  return (words_of(num_nodes) + kDstSetTileWords - 1) / kDstSetTileWords;
}
void check_nodes(const char* who, size_t num_nodes) {
  GF_REQUIRE(num_nodes < (size_t(1) << 40), std::string(who) + ": 2^40 nodes or more");
}

}  // namespace

void batch_assemble(const int64_t* d_src, const int64_t* d_dst, const float* d_time,
                    size_t num_rows, size_t lo, size_t hi, size_t neg_ratio, const int64_t* d_dl,
                    const int64_t* d_dl_count, uint64_t seed, uint64_t epoch, uint64_t first_row,
                    int64_t* d_roots, float* d_ts, int device, hipStream_t stream) {
  const bool neg_only = d_src == nullptr;
  GF_REQUIRE(lo <= hi && hi <= num_rows, "batch_assemble: needs lo <= hi <= num_rows");
  if (lo == hi || (neg_only && neg_ratio == 0)) return;      // nothing to write
  check_common("batch_assemble", neg_only, d_src, d_dst, d_time, num_rows, neg_ratio, d_dl,
               d_dl_count, d_roots, d_ts);
  const uint64_t planes = (neg_only ? 0 : 2) + neg_ratio;
  AssembleArgs a = {d_src, d_dst, d_time, num_rows, nullptr, lo, hi,
                    static_cast<uint32_t>(neg_ratio), d_dl, d_dl_count, seed, epoch, first_row,
                    d_roots, d_ts, planes * (hi - lo)};
  DeviceGuard dg(device);
  const dim3 grid(1, grid_y(hi - lo, planes));
  if (neg_only)
    batch_assemble_kernel<true><<<grid, dim3(kThreads), 0, stream>>>(a);
  else
    batch_assemble_kernel<false><<<grid, dim3(kThreads), 0, stream>>>(a);
  GF_HIP(hipGetLastError());
}

void batch_assemble_many(const int64_t* d_src, const int64_t* d_dst, const float* d_time,
                         size_t num_rows, const int64_t* d_borders, size_t num_batches,
                         size_t max_batch_rows, size_t neg_ratio, const int64_t* d_dl,
                         const int64_t* d_dl_count, uint64_t seed, uint64_t epoch,
                         uint64_t first_row, int64_t* d_roots, float* d_ts, size_t capacity,
                         int device, hipStream_t stream) {
  if (num_batches == 0) return;
  check_common("batch_assemble_many", false, d_src, d_dst, d_time, num_rows, neg_ratio, d_dl,
               d_dl_count, d_roots, d_ts);
  GF_REQUIRE(d_borders != nullptr, "batch_assemble_many: null borders");
  GF_REQUIRE(num_batches < (size_t(1) << 31), "batch_assemble_many: 2^31 batches or more");
  const uint64_t planes = 2 + neg_ratio;
  AssembleArgs a = {d_src, d_dst, d_time, num_rows, d_borders, 0, 0,
                    static_cast<uint32_t>(neg_ratio), d_dl, d_dl_count, seed, epoch, first_row,
                    d_roots, d_ts, capacity};
  DeviceGuard dg(device);
  const dim3 grid(static_cast<uint32_t>(num_batches), grid_y(max_batch_rows, planes));
  batch_assemble_kernel<false><<<grid, dim3(kThreads), 0, stream>>>(a);
  GF_HIP(hipGetLastError());
}

void dst_set_mark(const int64_t* d_ids, size_t n, uint64_t* d_bitmap, size_t num_nodes,
                  uint64_t* d_out_of_range, int device, hipStream_t stream) {
  check_nodes("dst_set_mark", num_nodes);
  if (n == 0) return;
  GF_REQUIRE(d_ids != nullptr && d_out_of_range != nullptr,
             "dst_set_mark: null ids or out-of-range counter");
  GF_REQUIRE(d_bitmap != nullptr || num_nodes == 0, "dst_set_mark: null bitmap");
  DeviceGuard dg(device);
  const uint64_t blocks = (n + kThreads - 1) / kThreads;
  dst_set_mark_kernel<<<dim3(static_cast<uint32_t>(std::min<uint64_t>(blocks, 2048))),
                        dim3(kThreads), 0, stream>>>(
      d_ids, n, reinterpret_cast<unsigned long long*>(d_bitmap), num_nodes,
      reinterpret_cast<unsigned long long*>(d_out_of_range));
  GF_HIP(hipGetLastError());
}

size_t dst_set_scratch_bytes(size_t num_nodes) {
  check_nodes("dst_set_scratch_bytes", num_nodes);
  return static_cast<size_t>(tiles_of(num_nodes)) * (sizeof(uint64_t) + sizeof(uint32_t));
}

void dst_set_compact(const uint64_t* d_bitmap, size_t num_nodes, int64_t* d_ids,
                     size_t ids_capacity, int64_t* d_count, void* d_scratch, size_t scratch_bytes,
                     int device, hipStream_t stream) {
  check_nodes("dst_set_compact", num_nodes);
  GF_REQUIRE(d_count != nullptr, "dst_set_compact: null count");
  const uint64_t words = words_of(num_nodes), tiles = tiles_of(num_nodes);
  GF_REQUIRE(tiles == 0 || (d_bitmap != nullptr && d_scratch != nullptr &&
                            scratch_bytes >= dst_set_scratch_bytes(num_nodes) &&
                            (reinterpret_cast<uintptr_t>(d_scratch) & 7u) == 0),
             "dst_set_compact: null bitmap, or scratch missing, misaligned or smaller than "
             "gf_dst_set_scratch_bytes() asks for");
  GF_REQUIRE(d_ids != nullptr || ids_capacity == 0, "dst_set_compact: null ids");
  uint64_t* const offsets = static_cast<uint64_t*>(d_scratch);      // tiles x 8 bytes, then
  uint32_t* const counts = reinterpret_cast<uint32_t*>(offsets + tiles);      // tiles x 4
  DeviceGuard dg(device);
  if (tiles)
    dst_set_tile_count_kernel<<<dim3(static_cast<uint32_t>(tiles)), dim3(kThreads), 0, stream>>>(
        d_bitmap, words, counts);
  dst_set_tile_scan_kernel<<<dim3(1), dim3(kThreads), 0, stream>>>(counts, tiles, offsets,
                                                                   ids_capacity, d_count);
  if (tiles && ids_capacity)
    dst_set_emit_kernel<<<dim3(static_cast<uint32_t>(tiles)), dim3(kThreads), 0, stream>>>(
        d_bitmap, words, offsets, d_ids, ids_capacity);
  GF_HIP(hipGetLastError());
}

}  // namespace gf
