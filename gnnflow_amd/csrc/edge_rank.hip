// Ranking with the edge score: B source rows against ONE shared set of C candidate rows,
//
//   score(i, c) = bias + sum_d w[d] * max(src[i, d] + cand[c, d], 0)              fp32
//
// without the [B * C, D] operand that the paired ops.edge_score would need and without storing
// the [B, C] scores.  Of the scores only two things are kept per source: the k best candidates
// and the number of candidates that beat or tie a reference score (the rank of a true destination
// is 1 + greater + equal / 2, the convention of link_metrics.hip).
//
// The score is edge_score.hip's, bit for bit.  The library is built with -ffp-contract=off, so
// that is a matter of the order of the adds alone, and edge_score.hip:10-15 fixes it: column d
// belongs to lane (d / 4) % 16, a lane sums its columns in ascending order, the 16 lanes are
// combined by the xor butterfly 8, 4, 2, 1 and bias is added last.  Here one thread owns a whole
// pair and keeps the 16 lanes' sums as 16 accumulators, acc[l] over the 4-column chunks l,
// l + 16, ..., and combines them in the butterfly's tree: (acc[l] + acc[l + 8]) for l < 8, then
// + 4, + 2, + 1.  The one difference: a NaN pre-activation src + cand makes the score NaN here,
// as torch.relu would, where edge_score's `x > 0 ? x : 0` turns it into 0; a row with a NaN in
// it therefore ranks last.  The hot loop is edge_score's arithmetic; only a sub-tile that staged
// a NaN or an infinity looks at its pairs' pre-activations again and overwrites such a score
// with NaN (NaN absorbs every later add and multiply, so that is what keeping it gives).
// Every other input gives edge_score's bits.
//
// Scoring pass.  A workgroup of 256 threads owns a tile of 32 source rows and one chunk of
// kEdgeRankChunk = 256 candidates, 8 sub-tiles of 32.  A sub-tile is 32 x 32 pairs, 2 x 2 per
// thread (64 accumulators).  The columns go through LDS 64 at a time, one round of the 16
// "lanes": 32 source rows, 32 candidate rows and 64 weights, rows padded to 68 floats so that the
// 16-byte reads of 16 different rows fall on 16 different bank slots.  A 4-column chunk costs a
// thread five 16-byte LDS reads for 2 x 2 x 4 terms.  The rows are staged with 16-byte loads when
// D % 4 == 0 and src, cand and w are 16-byte aligned and element by element otherwise; the
// arithmetic reads LDS and is the same either way.  Rows past B or C are staged as zeros and
// masked later.  Columns past D are staged as zeros, weight included; whole chunks of them are
// not added, and inside the last chunk their terms are w * relu(0 + 0) = +0, which leaves an
// accumulator as it is: it starts at +0, a sum is -0 only when both operands are, so it never is
// -0, and x + (+0) == x bit for bit for every other x, infinities and NaN included.
//
// The tile's 32 x 256 scores stay in LDS.  A wave then takes a source row at a time: each lane
// holds 4 of the row's 256 scores; `greater` and `equal` are ballots against the reference score
// (a NaN on either side compares false), and the top k are k rounds of a wave arg-max over
//
//   key = (ordered(score) << 32) | ~candidate        ordered: NaN -> 0, else the float's bits
//                                                     mapped so that unsigned order = float order
//
// so that a larger key is a better score or, among equal scores, a smaller candidate index, a
// NaN sorts below -inf, and no two candidates share a key.  A candidate that is skipped or past C
// has key 0, below everything.  The workgroup writes its counts and its k keys, descending, to
// scratch.
//
// Exclusion mask (MASKED).  exclude [B, W], W = ceil(C / 64): bit c % 64 of word [i, c / 64] set
// leaves candidate c out of row i exactly as skip[i] does.  Lane l holds candidates
// c0 + l + 64 j and c0 is a multiple of 64, so the 64 candidates of one j are one word: one
// wave-uniform load and a bit test per lane.  Bits past C are never looked at.  The unmasked
// instantiations are the code the kernel had before there was a mask.
//
// Merge pass.  One wave per source sums the chunks' counts (integers: any order) and takes the
// k largest of the chunks' lists: k rounds of "largest key below the previous one", every lane
// walking its chunks' descending lists up to the first key below it.  Key 0 is written as
// (-inf, -1).  No atomics, no floating-point sums across threads: selection under a total
// order, bit-reproducible.
#include "block_ops.hpp"
#include "common.hpp"

#include <cstdint>

namespace gf {
namespace {

constexpr int kThreads = 256;
constexpr int kWave = 64;
constexpr int kWaves = kThreads / kWave;
constexpr int kLanes = 16;                      // edge_score.hip's lanes per row
constexpr int kPass = kLanes * 4;               // columns of one round of the lanes
constexpr int kStride = kPass + 4;              // LDS row pitch: 17 slots of 16 bytes
constexpr int kTileSrc = 32;                    // source rows per workgroup
constexpr int kTileCand = 32;                   // candidates per sub-tile
constexpr int kChunk = static_cast<int>(kEdgeRankChunk);
constexpr int kSubTiles = kChunk / kTileCand;
constexpr int kPerLane = kChunk / kWave;        // scores of a row a lane holds
constexpr int kScorePitch = kChunk + 8;
static_assert(kTileSrc * kTileCand == 4 * kThreads, "2 x 2 pairs per thread");
static_assert(kChunk % kTileCand == 0 && kChunk % kWave == 0, "whole sub-tiles and lanes");
static_assert(kEdgeRankMaxK <= kEdgeRankChunk, "a chunk can fill a list");

// edge_score.hip's es_relu and term
__device__ __forceinline__ float er_relu(float x) { return x > 0.f ? x : 0.f; }
__device__ __forceinline__ float er_term(float w, float s, float p) { return w * er_relu(s + p); }

__device__ __forceinline__ bool nonfinite(float x) {
  return (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u;
}

// rows [row0, row0 + 32) x columns [col0, col0 + 64) of a [num_rows, D] matrix into a tile;
// true when this thread staged a NaN or an infinity
template <bool VEC>
__device__ __forceinline__ bool stage_rows(float (*tile)[kStride], const float* __restrict__ rows,
                                           uint32_t row0, uint32_t num_rows, uint32_t D,
                                           uint32_t col0) {
  bool bad = false;
  if (VEC) {
    for (uint32_t q = threadIdx.x; q < kTileSrc * kLanes; q += kThreads) {
      const uint32_t r = q / kLanes, v = q % kLanes;
      const uint32_t row = row0 + r, col = col0 + v * 4;
      float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
      if (row < num_rows && col < D)      // D % 4 == 0: the chunk is whole
        x = *reinterpret_cast<const float4*>(rows + static_cast<uint64_t>(row) * D + col);
      bad |= nonfinite(x.x) || nonfinite(x.y) || nonfinite(x.z) || nonfinite(x.w);
      *reinterpret_cast<float4*>(&tile[r][v * 4]) = x;
    }
  } else {
    for (uint32_t q = threadIdx.x; q < kTileSrc * kPass; q += kThreads) {
      const uint32_t r = q / kPass, e = q % kPass;
      const uint32_t row = row0 + r, col = col0 + e;
      const float x = row < num_rows && col < D ? rows[static_cast<uint64_t>(row) * D + col] : 0.f;
      bad |= nonfinite(x);
      tile[r][e] = x;
    }
  }
  return bad;
}

// One round of the 16 lanes: chunk l of the 64 staged columns goes to acc[..][..][l], its
// columns in ascending order.  width = the columns of the round that exist (64 when FULL); a
// chunk with none of them is left out, one with some takes its zero columns along.
template <bool FULL>
__device__ __forceinline__ void accumulate(float (&acc)[2][2][kLanes],
                                           const float (*s_src)[kStride],
                                           const float (*s_cand)[kStride], const float* s_w,
                                           uint32_t ts, uint32_t tc, uint32_t width) {
#pragma unroll
  for (int l = 0; l < kLanes; ++l) {
    if (!FULL && static_cast<uint32_t>(l * 4) >= width) continue;      // uniform
    const float4 wv = *reinterpret_cast<const float4*>(s_w + l * 4);
    float4 sv[2], cv[2];
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      sv[a] = *reinterpret_cast<const float4*>(&s_src[ts + 16 * a][l * 4]);
      cv[a] = *reinterpret_cast<const float4*>(&s_cand[tc + 16 * a][l * 4]);
    }
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        float t = acc[a][b][l];
        t += er_term(wv.x, sv[a].x, cv[b].x);
        t += er_term(wv.y, sv[a].y, cv[b].y);
        t += er_term(wv.z, sv[a].z, cv[b].z);
        t += er_term(wv.w, sv[a].w, cv[b].w);
        acc[a][b][l] = t;
      }
    // one chunk at a time: scheduled across chunks, the loads of all 16 are live at once
    __builtin_amdgcn_sched_barrier(0);
  }
}

// unsigned order = float order, NaN below -inf, -0 with +0
__device__ __forceinline__ uint32_t ordered(float x) {
  if (x != x) return 0u;
  if (x == 0.f) return 0x80000000u;
  const uint32_t b = __float_as_uint(x);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float unordered(uint32_t key) {
  if (key == 0u) return __uint_as_float(0x7fc00000u);
  return __uint_as_float((key & 0x80000000u) ? (key ^ 0x80000000u) : ~key);
}

__device__ __forceinline__ uint64_t wave_max(uint64_t v) {
#pragma unroll
  for (int off = kWave / 2; off >= 1; off >>= 1) {
    const uint64_t o =
        static_cast<uint64_t>(__shfl_xor(static_cast<unsigned long long>(v), off, kWave));
    v = o > v ? o : v;
  }
  return v;
}
__device__ __forceinline__ uint64_t wave_sum(uint64_t v) {
#pragma unroll
  for (int off = kWave / 2; off >= 1; off >>= 1)
    v += static_cast<uint64_t>(__shfl_xor(static_cast<unsigned long long>(v), off, kWave));
  return v;
}

// counts[(chunk * B + i) * 2 + {0, 1}] = greater, equal of source i in the chunk (null: none);
// lists[(i * chunks + chunk) * k + t] = its t-th largest key (k == 0: none)
template <bool VEC, bool MASKED>
__global__ void __launch_bounds__(kThreads)
edge_rank_score(const float* __restrict__ src, const float* __restrict__ cand,
                const float* __restrict__ w, const float* __restrict__ bias, uint32_t B,
                uint32_t C, uint32_t D, uint32_t k, uint32_t chunks,
                const float* __restrict__ ref, const int64_t* __restrict__ skip,
                const uint64_t* __restrict__ exclude, uint32_t* __restrict__ counts,
                uint64_t* __restrict__ lists) {
  __shared__ __align__(16) float s_src[kTileSrc][kStride];
  __shared__ __align__(16) float s_cand[kTileCand][kStride];
  __shared__ __align__(16) float s_w[kPass];
  __shared__ float s_score[kTileSrc][kScorePitch];
  const uint32_t chunk = blockIdx.x % chunks, tile = blockIdx.x / chunks;
  const uint32_t c0 = chunk * static_cast<uint32_t>(kChunk);      // < C
  const uint32_t i0 = tile * static_cast<uint32_t>(kTileSrc);     // < B
  const uint32_t ts = threadIdx.x / 16, tc = threadIdx.x % 16;
  const float b0 = bias[0];

  for (int sub = 0; sub < kSubTiles; ++sub) {
    const uint32_t cs = c0 + sub * kTileCand;
    if (cs >= C) break;      // uniform
    float acc[2][2][kLanes];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int l = 0; l < kLanes; ++l) acc[a][b][l] = 0.f;
    bool bad = false;
    for (uint32_t col0 = 0; col0 < D; col0 += kPass) {      // uniform
      __syncthreads();      // the round before has been read
      bad |= stage_rows<VEC>(s_src, src, i0, B, D, col0);
      bad |= stage_rows<VEC>(s_cand, cand, cs, C, D, col0);
      if (threadIdx.x < kPass) s_w[threadIdx.x] = col0 + threadIdx.x < D ? w[col0 + threadIdx.x] : 0.f;
      __syncthreads();
      const uint32_t width = D - col0;
      if (width >= kPass)
        accumulate<true>(acc, s_src, s_cand, s_w, ts, tc, kPass);
      else
        accumulate<false>(acc, s_src, s_cand, s_w, ts, tc, width);
    }
    const bool any_bad = __syncthreads_or(bad ? 1 : 0) != 0;      // uniform; rare
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        float* t = acc[a][b];      // the butterfly 8, 4, 2, 1 as lane 0 sees it
#pragma unroll
        for (int off = kLanes / 2; off >= 1; off >>= 1)
#pragma unroll
          for (int l = 0; l < off; ++l) t[l] = t[l] + t[l + off];
        float score = t[0] + b0;
        const uint32_t i = i0 + ts + 16 * a, c = cs + tc + 16 * b;
        if (any_bad && i < B && c < C) {      // a NaN pre-activation makes the score NaN
          const float* s = src + static_cast<uint64_t>(i) * D;
          const float* p = cand + static_cast<uint64_t>(c) * D;
          bool isnan = false;
          for (uint32_t d = 0; d < D; ++d) {
            const float x = s[d] + p[d];
            isnan |= x != x;
          }
          if (isnan) score = __uint_as_float(0x7fc00000u);
        }
        s_score[ts + 16 * a][sub * kTileCand + tc + 16 * b] = score;
      }
  }
  __syncthreads();

  const uint32_t lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
  for (uint32_t r = wave; r < kTileSrc; r += kWaves) {
    const uint32_t i = i0 + r;
    if (i >= B) break;      // uniform over the wave
    const int64_t skipped = skip ? skip[i] : -1;
    const float x = counts ? ref[i] : 0.f;
    const uint32_t W = (C + kWave - 1) / kWave, w0 = c0 / kWave;
    uint64_t key[kPerLane];
    uint32_t gt = 0, eq = 0;
#pragma unroll
    for (int j = 0; j < kPerLane; ++j) {
      const uint32_t cl = lane + j * kWave, c = c0 + cl;
      bool valid = c < C && static_cast<int64_t>(c) != skipped;
      if (MASKED) {      // the word of candidates c0 + 64 j ..: uniform over the wave
        const uint64_t word = w0 + j < W ? exclude[static_cast<uint64_t>(i) * W + w0 + j] : 0ull;
        valid = valid && !((word >> lane) & 1ull);
      }
      const float v = valid ? s_score[r][cl] : 0.f;      // past C the tile was never written
      key[j] = valid ? (static_cast<uint64_t>(ordered(v)) << 32) | static_cast<uint32_t>(~c) : 0ull;
      if (counts) {
        gt += static_cast<uint32_t>(__popcll(__ballot(valid && v > x)));
        eq += static_cast<uint32_t>(__popcll(__ballot(valid && v == x)));
      }
    }
    if (counts && lane == 0) {
      const uint64_t at = (static_cast<uint64_t>(chunk) * B + i) * 2;
      counts[at] = gt;
      counts[at + 1] = eq;
    }
    if (k == 0) continue;
    uint64_t* out = lists + (static_cast<uint64_t>(i) * chunks + chunk) * k;
    for (uint32_t t = 0; t < k; ++t) {
      uint64_t m = key[0];
#pragma unroll
      for (int j = 1; j < kPerLane; ++j) m = key[j] > m ? key[j] : m;
      m = wave_max(m);
      if (lane == 0) out[t] = m;
      if (m == 0ull) {      // nothing left: the rest of the list is empty
        for (uint32_t u = t + 1 + lane; u < k; u += kWave) out[u] = 0ull;
        break;
      }
#pragma unroll
      for (int j = 0; j < kPerLane; ++j) key[j] = key[j] == m ? 0ull : key[j];
    }
  }
}

__global__ void __launch_bounds__(kThreads)
edge_rank_merge(const uint32_t* __restrict__ counts, const uint64_t* __restrict__ lists,
                uint32_t B, uint32_t chunks, uint32_t k, float* __restrict__ values,
                int64_t* __restrict__ indices, int64_t* __restrict__ greater,
                int64_t* __restrict__ equal) {
  const uint32_t lane = threadIdx.x % kWave;
  const uint32_t i = blockIdx.x * static_cast<uint32_t>(kWaves) + threadIdx.x / kWave;
  if (i >= B) return;      // whole waves; no barrier below
  if (greater) {
    uint64_t gt = 0, eq = 0;
    for (uint32_t ch = lane; ch < chunks; ch += kWave) {
      const uint64_t at = (static_cast<uint64_t>(ch) * B + i) * 2;
      gt += counts[at];
      eq += counts[at + 1];
    }
    gt = wave_sum(gt);
    eq = wave_sum(eq);
    if (lane == 0) {
      greater[i] = static_cast<int64_t>(gt);
      equal[i] = static_cast<int64_t>(eq);
    }
  }
  const uint64_t* mine = lists + static_cast<uint64_t>(i) * chunks * k;
  uint64_t below = ~0ull;      // keys are distinct: the next one is the largest below the last
  for (uint32_t t = 0; t < k; ++t) {
    uint64_t m = 0ull;
    for (uint32_t ch = lane; ch < chunks; ch += kWave) {
      const uint64_t* p = mine + static_cast<uint64_t>(ch) * k;
      for (uint32_t e = 0; e < k; ++e) {      // descending: the first key below is the largest
        const uint64_t key = p[e];
        if (key < below) {
          m = key > m ? key : m;
          break;
        }
      }
    }
    m = wave_max(m);
    if (m == 0ull) {      // fewer than k candidates: (-inf, -1) to the end
      for (uint32_t u = t + lane; u < k; u += kWave) {
        values[static_cast<uint64_t>(i) * k + u] = __uint_as_float(0xff800000u);
        indices[static_cast<uint64_t>(i) * k + u] = -1;
      }
      break;
    }
    if (lane == 0) {
      values[static_cast<uint64_t>(i) * k + t] = unordered(static_cast<uint32_t>(m >> 32));
      indices[static_cast<uint64_t>(i) * k + t] = static_cast<int64_t>(~static_cast<uint32_t>(m));
    }
    below = m;
  }
}

size_t num_chunks(size_t num_cand) { return (num_cand + kEdgeRankChunk - 1) / kEdgeRankChunk; }

void check_shape(size_t num_src, size_t num_cand, size_t k) {
  GF_REQUIRE(num_cand >= 1, "edge_rank: needs at least one candidate");
  GF_REQUIRE(num_cand < (size_t{1} << 31), "edge_rank: more than 2^31 - 1 candidates");
  GF_REQUIRE(k <= kEdgeRankMaxK && k <= num_cand,
             "edge_rank: k must be at most min(num_cand, " + std::to_string(kEdgeRankMaxK) + ")");
  const size_t tiles = (num_src + kTileSrc - 1) / kTileSrc;
  GF_REQUIRE(num_src < (size_t{1} << 31) && tiles * num_chunks(num_cand) < (size_t{1} << 31),
             "edge_rank: too many (source tile, candidate chunk) pairs for one call");
}

}  // namespace

size_t edge_rank_scratch_bytes(size_t num_src, size_t num_cand, size_t k) {
  check_shape(num_src, num_cand, k);
  return num_chunks(num_cand) * num_src * (2 * sizeof(uint32_t) + k * sizeof(uint64_t));
}

void edge_rank(const float* d_src, const float* d_cand, const float* d_w, const float* d_bias,
               size_t num_src, size_t num_cand, size_t dim, size_t k, const float* d_ref_score,
               const int64_t* d_skip, const uint64_t* d_exclude, void* d_scratch,
               size_t scratch_bytes, float* d_values, int64_t* d_indices, int64_t* d_greater,
               int64_t* d_equal, int device, hipStream_t stream) {
  GF_REQUIRE(dim >= 1, "edge_rank: dim must be >= 1");
  GF_REQUIRE(dim < (size_t{1} << 30), "edge_rank: dim too large");
  check_shape(num_src, num_cand, k);
  if (num_src == 0 || (k == 0 && !d_ref_score)) return;
  GF_REQUIRE(d_src && d_cand && d_w && d_bias, "edge_rank: null src, cand, weight or bias");
  GF_REQUIRE(k == 0 || (d_values && d_indices), "edge_rank: null values or indices");
  GF_REQUIRE(!d_ref_score || (d_greater && d_equal),
             "edge_rank: a reference score needs greater and equal");
  GF_REQUIRE(d_scratch != nullptr && (reinterpret_cast<uintptr_t>(d_scratch) & 7) == 0 &&
                 scratch_bytes >= edge_rank_scratch_bytes(num_src, num_cand, k),
             "edge_rank: scratch missing, not 8-byte aligned or smaller than "
             "gf_edge_rank_scratch() asks for");
  const uint32_t B = static_cast<uint32_t>(num_src), C = static_cast<uint32_t>(num_cand),
                 D = static_cast<uint32_t>(dim), K = static_cast<uint32_t>(k);
  const uint32_t chunks = static_cast<uint32_t>(num_chunks(num_cand));
  const uint32_t tiles = (B + kTileSrc - 1) / kTileSrc;
  uint32_t* counts = static_cast<uint32_t*>(d_scratch);
  uint64_t* lists = reinterpret_cast<uint64_t*>(counts + static_cast<size_t>(chunks) * B * 2);
  const bool count = d_ref_score != nullptr;
  const bool vec = dim % 4 == 0 && aligned16(d_src) && aligned16(d_cand) && aligned16(d_w);
  const dim3 grid(tiles * chunks), block(kThreads);
  DeviceGuard dg(device);
  auto* const score = d_exclude ? (vec ? edge_rank_score<true, true> : edge_rank_score<false, true>)
                                : (vec ? edge_rank_score<true, false> : edge_rank_score<false, false>);
  score<<<grid, block, 0, stream>>>(d_src, d_cand, d_w, d_bias, B, C, D, K, chunks, d_ref_score,
                                    d_skip, d_exclude, count ? counts : nullptr, lists);
  GF_HIP(hipGetLastError());
  edge_rank_merge<<<dim3((B + kWaves - 1) / kWaves), block, 0, stream>>>(
      counts, lists, B, chunks, K, d_values, d_indices, count ? d_greater : nullptr,
      count ? d_equal : nullptr);
  GF_HIP(hipGetLastError());
}

}  // namespace gf
