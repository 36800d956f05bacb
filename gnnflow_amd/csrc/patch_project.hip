// Gather + patch Linear on the float32 matrix cores.  With r over the flattened leading
// dimensions, Q = L / P patches per row, K = P * d columns per patch and m = r * Q + q,
//
//   x[r, l, :]   = table[ids[r, l], :]                if l < lengths[r] and 0 <= ids[r, l] < rows
//                = te_cos(w[:], delta_t[r, l], b[:])  (time form) if l < lengths[r]
//                = 0                                  otherwise
//   out[m, c]    = bias[c] + sum_{k < K} x[r, q P + k / d, k % d] * weight[c, k]
//   dweight[c,k] = sum_m dout[m, c] * x[r, q P + k / d, k % d]        dbias[c] = sum_m dout[m, c]
//
// x is never stored: it exists only as tiles in LDS.  te_cos is time_encode_expr.hpp's, so a time
// row holds time_encode.hip's bits.  All arithmetic is float32; the products run on
// v_mfma_f32_16x16x4_f32 (float32 in, float32 accumulate), nothing is narrowed.
//
// The MFMA.  D[16 x 16] += A[16 x 4] * B[4 x 16] per wave: lane l supplies A[l % 16][l / 16] and
// B[l / 16][l % 16] and holds D[4 (l / 16) + v][l % 16] in the four floats v of its accumulator.
// A sum over k does not care in which order k is visited, so a block of 16 k is taken as four
// MFMAs in which lane group g = l / 16 supplies k = 4 g + s in step s: the four values a lane
// needs are then one aligned float4 in LDS (ds_read_b128), not four reads.  Both operands use the
// same mapping, which is all correctness needs.
//
// LDS.  Tiles are row-major with a stride of kStride = 68 floats (64 + 4).  The float4 operand
// read of lane (i, g) is at float i * 68 + 4 g + const: the 16 lanes served together differ in i
// alone and 68 / 4 = 17 is odd, so they fall on 16 different 16-byte bank groups; the scalar
// reads of the backward's B operand are at (4 g + s) * 68 + i, and 4 * 68 = 16 mod 64, so the 64
// lanes take 64 different banks.  A workgroup's LDS is (64 + C_pad) * 68 floats + 768 bytes of
// row bookkeeping: 35.6 KB at C_pad = 64 (four workgroups a CU), 53.0 KB at C_pad = 128 (three).
//
// Forward.  A workgroup of four waves owns 64 consecutive patches; wave w owns patches 16 w ..
// 16 w + 15 and the whole output width, C_pad / 16 <= 8 accumulator quads = 32 VGPRs.  K is walked
// in chunks of 64 columns: the chunk of the gathered A tile [64 x 64] and of weight [C_pad x 64]
// are staged, then 16 k at a time go through the MFMAs.  A workgroup owns one tile, so every
// element of weight is staged exactly once per workgroup whether it is kept resident or chunked:
// the chunk keeps the LDS small instead.  The K tail and the C tail are zeros in
// LDS; a zero row (padding, an id without a row) is written as zeros without a load.  The
// epilogue adds bias and stores c < C, one writer per element.
//
// Staging x.  The chunk's 64 columns are split into units of V floats (V = 4 when d % 4 == 0 and
// the table is 16-byte aligned -- in the forward, which stages weight by the same units, weight
// too -- else 1); a thread owns one unit column and walks the 64
// rows in steps of 256 / (64 / V).  Its column k is kept as (slot p = k / d, table column
// j = k % d) and advanced by 64, not divided.  What a row needs -- the offset of its patch's first
// slot in the planes and how many of the patch's slots are filled -- is worked out once per tile
// by 64 threads and kept in LDS.  V only changes how bytes are loaded: the tiles, the MFMA order
// and so the result's bits are the same for both.
//
// Backward.  grid = (column tiles of 64 k) x (partial rows).  A workgroup keeps dweight[C_pad x 64]
// in registers (wave w: columns 16 w .. 16 w + 15 by all quads, the forward's 32 VGPRs) and walks
// its share of the patches 64 at a time: the x tile of its own columns is re-gathered as in the
// forward, the dout tile is staged TRANSPOSED ([c][m], so that the A operand is again one float4
// over four patches), and dout^T x goes through the same MFMA.  Column tile 0 also sums dout over
// the step's patches in ascending order for dbias.  Each workgroup writes its partial row whole;
// a second launch sums the rows in ascending order.  No atomics: the same inputs give the same
// bits.
#include "patch_project.hpp"
#include "common.hpp"
#include "time_encode_expr.hpp"

#include <algorithm>
#include <string>

namespace gf {
namespace {

constexpr int kThreads = 256;
constexpr int kWave = 64;
constexpr int kTileM = 64;                 // patches of a forward tile, of a backward step
constexpr int kChunk = 64;                 // columns staged at a time; the backward's column tile
constexpr int kStride = kChunk + 4;        // floats between the rows of an LDS tile
constexpr int kMaxQuads = static_cast<int>(kPatchMaxChannels) / 16;
constexpr size_t kMinStepsPerPartialRow = 4;
constexpr int kFinishThreads = 256;

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct Geometry {
  uint32_t patches;          // R * Q < 2^31
  uint32_t Q, L, P, d;
  uint32_t K;                // P * d
  uint32_t C, quads;         // quads = ceil(C / 16)
  uint32_t hop_p, hop_j;     // kChunk / d, kChunk % d: a column 64 further on
};

// per row of a tile: where its patch starts in the [R, L] planes and how many of its slots are
// filled (<= 0: none, the row is zeros; a row past the last patch has 0)
struct RowInfo {
  int64_t base[kTileM];
  int32_t remain[kTileM];
};

// one unit of V floats from global memory: a 16-byte access or a scalar one
__device__ __forceinline__ void load_unit(const float* at, float (&v)[4]) {
  const float4 q = *reinterpret_cast<const float4*>(at);
  v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
}
__device__ __forceinline__ void load_unit(const float* at, float (&v)[1]) { v[0] = *at; }

// ---- the two row sources: V floats of slot `slot` of the planes from column j on, into v, which
// arrives zeroed.  j + V <= d.
struct TableRows {
  const int64_t* ids;
  const float* table;
  uint64_t rows;
  uint32_t d;
  template <int V>
  __device__ __forceinline__ void load(uint64_t slot, uint32_t j, float (&v)[V]) const {
    const int64_t id = ids[slot];
    if (id < 0 || static_cast<uint64_t>(id) >= rows) return;      // no row: zeros, no load
    const float* at = table + static_cast<uint64_t>(id) * d + j;
    load_unit(at, v);
  }
};

struct TimeRows {
  const float* delta_t;
  const float* w;
  const float* b;
  template <int V>
  __device__ __forceinline__ void load(uint64_t slot, uint32_t j, float (&v)[V]) const {
    const float dt = delta_t[slot];
#pragma unroll
    for (int u = 0; u < V; ++u) v[u] = te_cos(w[j + u], dt, b[j + u]);
  }
};

__device__ __forceinline__ void store_unit(float* at, const float (&v)[4]) {
  *reinterpret_cast<float4*>(at) = make_float4(v[0], v[1], v[2], v[3]);
}
__device__ __forceinline__ void store_unit(float* at, const float (&v)[1]) { at[0] = v[0]; }

// the tile's RowInfo for the patches m0 .. m0 + 63; visible after the next barrier
__device__ __forceinline__ void row_info(const Geometry& g, const int32_t* __restrict__ lengths,
                                         uint32_t m0, RowInfo& ri) {
  if (threadIdx.x >= kTileM) return;
  const uint64_t m = static_cast<uint64_t>(m0) + threadIdx.x;
  int64_t base = 0;
  int32_t remain = 0;
  if (m < g.patches) {
    const uint32_t r = static_cast<uint32_t>(m) / g.Q, q = static_cast<uint32_t>(m) % g.Q;
    int32_t len = lengths ? lengths[r] : static_cast<int32_t>(g.L);
    if (len > static_cast<int32_t>(g.L)) len = static_cast<int32_t>(g.L);
    base = static_cast<int64_t>(r) * g.L + q * g.P;             // q P + p < len <= L below
    remain = len - static_cast<int32_t>(q * g.P);
  }
  ri.base[threadIdx.x] = base;
  ri.remain[threadIdx.x] = remain;
}

// the x tile [64 x 64] of the columns whose unit this thread owns at (p, j); live: the column is
// below K.  Every element of the tile is written.
template <class Src, int V>
__device__ __forceinline__ void stage_rows(const Src& src, const RowInfo& ri, uint32_t p,
                                           uint32_t j, bool live, float* __restrict__ sx) {
  constexpr int U = kChunk / V, RP = kThreads / U;
  const uint32_t cu = threadIdx.x % U;
#pragma unroll 4
  for (uint32_t row = threadIdx.x / U; row < kTileM; row += RP) {
    float v[V];
#pragma unroll
    for (int u = 0; u < V; ++u) v[u] = 0.f;
    if (live && static_cast<int32_t>(p) < ri.remain[row])
      src.template load<V>(static_cast<uint64_t>(ri.base[row]) + p, j, v);
    store_unit(sx + row * kStride + cu * V, v);
  }
}

// weight[0 .. 16 quads, k0 .. k0 + 64) as sw[c][k - k0], zeros for c >= C and k >= K
template <int V>
__device__ __forceinline__ void stage_weight(const float* __restrict__ weight, const Geometry& g,
                                             uint32_t k0, float* __restrict__ sw) {
  constexpr int U = kChunk / V, RP = kThreads / U;
  const uint32_t cu = threadIdx.x % U, k = k0 + cu * V;
  for (uint32_t c = threadIdx.x / U; c < 16 * g.quads; c += RP) {
    float v[V];
#pragma unroll
    for (int u = 0; u < V; ++u) v[u] = 0.f;
    if (c < g.C && k < g.K) {                       // V == 4: K % 4 == 0, so k + 3 < K
      const float* at = weight + static_cast<uint64_t>(c) * g.K + k;
      load_unit(at, v);
    }
    store_unit(sw + c * kStride + cu * V, v);
  }
}

// dout[m0 .. m0 + 64, 0 .. 16 quads) transposed as sg[c][m - m0], zeros past the patches and past
// C.  A wave's lanes are 16 consecutive c by 4 consecutive m: 64-byte runs of dout, 64 banks.
__device__ __forceinline__ void stage_grad(const float* __restrict__ gout, const Geometry& g,
                                           uint32_t m0, float* __restrict__ sg) {
  const uint32_t c_lo = threadIdx.x % 16, m_lo = (threadIdx.x / 16) % 4;
  for (uint32_t idx = threadIdx.x / kWave; idx < 16 * g.quads; idx += kThreads / kWave) {
    const uint32_t m = (idx % 16) * 4 + m_lo, c = (idx / 16) * 16 + c_lo;
    const uint64_t gm = static_cast<uint64_t>(m0) + m;
    float v = 0.f;
    if (gm < g.patches && c < g.C) v = gout[gm * g.C + c];
    sg[c * kStride + m] = v;
  }
}

#define GF_PATCH_MFMA4(acc, a, b0, b1, b2, b3)                          \
  do {                                                                  \
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b0, acc, 0, 0, 0);  \
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b1, acc, 0, 0, 0);  \
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b2, acc, 0, 0, 0);  \
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b3, acc, 0, 0, 0);  \
  } while (0)

template <class Src, int V>
__global__ void __launch_bounds__(kThreads)
patch_project_fwd(const Src src, const Geometry g, const int32_t* __restrict__ lengths,
                  const float* __restrict__ weight, const float* __restrict__ bias,
                  float* __restrict__ out) {
  extern __shared__ __align__(16) float lds[];
  float* const sx = lds;                                   // [64][kStride]
  float* const sw = lds + kTileM * kStride;                // [16 quads][kStride]
  RowInfo& ri = *reinterpret_cast<RowInfo*>(sw + 16 * g.quads * kStride);
  const uint32_t m0 = blockIdx.x * kTileM;                 // < patches
  const uint32_t wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
  const uint32_t i = lane % 16, grp = lane / 16;
  row_info(g, lengths, m0, ri);

  f32x4 acc[kMaxQuads];
#pragma unroll
  for (int qd = 0; qd < kMaxQuads; ++qd) acc[qd] = f32x4{0.f, 0.f, 0.f, 0.f};

  const uint32_t cu = threadIdx.x % (kChunk / V);
  uint32_t p = cu * V / g.d, j = cu * V % g.d;             // this thread's unit column, chunk 0
  const float* const a_at = sx + (wave * 16 + i) * kStride + grp * 4;
  const float* const b_at = sw + i * kStride + grp * 4;
  for (uint32_t k0 = 0; k0 < g.K; k0 += kChunk) {
    __syncthreads();      // the row info is written; the last chunk's tiles are read
    stage_rows<Src, V>(src, ri, p, j, k0 + cu * V < g.K, sx);
    stage_weight<V>(weight, g, k0, sw);
    __syncthreads();
    const uint32_t left = g.K - k0;
    const uint32_t blocks = left >= kChunk ? kChunk / 16 : (left + 15) / 16;
    for (uint32_t kb = 0; kb < blocks; ++kb) {
      const float4 a = *reinterpret_cast<const float4*>(a_at + kb * 16);
#pragma unroll
      for (int qd = 0; qd < kMaxQuads; ++qd) {
        if (qd < static_cast<int>(g.quads)) {              // uniform
          const float4 b = *reinterpret_cast<const float4*>(b_at + qd * 16 * kStride + kb * 16);
          GF_PATCH_MFMA4(acc[qd], a, b.x, b.y, b.z, b.w);
        }
      }
    }
    j += g.hop_j;
    p += g.hop_p;
    if (j >= g.d) j -= g.d, ++p;
  }

#pragma unroll
  for (int qd = 0; qd < kMaxQuads; ++qd) {
    const uint32_t c = qd * 16 + i;
    if (qd < static_cast<int>(g.quads) && c < g.C) {
      const float bc = bias[c];
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const uint64_t m = static_cast<uint64_t>(m0) + wave * 16 + grp * 4 + v;
        if (m < g.patches) out[m * g.C + c] = acc[qd][v] + bc;
      }
    }
  }
}

// partials[y][c * (K + 1) + k]: k < K -> dweight[c, k]'s share of partial row y, k == K ->
// dbias[c]'s.  want_w false: gridDim.x == 1 and no x is gathered.
template <class Src, int V>
__global__ void __launch_bounds__(kThreads)
patch_project_bwd(const Src src, const Geometry g, const int32_t* __restrict__ lengths,
                  const float* __restrict__ gout, uint32_t steps, uint32_t steps_per_row,
                  bool want_w, bool want_b, float* __restrict__ partials) {
  extern __shared__ __align__(16) float lds[];
  float* const sx = lds;                                   // [64 patches][kStride]
  float* const sg = lds + kTileM * kStride;                // [16 quads channels][kStride]
  RowInfo& ri = *reinterpret_cast<RowInfo*>(sg + 16 * g.quads * kStride);
  const uint32_t wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
  const uint32_t i = lane % 16, grp = lane / 16;
  const uint32_t k0 = blockIdx.x * kChunk;                 // < K
  const uint32_t s0 = blockIdx.y * steps_per_row;          // < steps
  const uint32_t s1 = steps - s0 < steps_per_row ? steps : s0 + steps_per_row;
  const bool sum_bias = want_b && blockIdx.x == 0;

  f32x4 acc[kMaxQuads];
#pragma unroll
  for (int qd = 0; qd < kMaxQuads; ++qd) acc[qd] = f32x4{0.f, 0.f, 0.f, 0.f};
  float bsum = 0.f;

  const uint32_t k = k0 + threadIdx.x % (kChunk / V) * V;  // this thread's unit column, fixed
  const uint32_t p = k / g.d, j = k % g.d;
  const float* const a_at = sg + i * kStride + grp * 4;
  const float* const b_at = sx + grp * 4 * kStride + wave * 16 + i;
  for (uint32_t s = s0; s < s1; ++s) {                     // uniform over the workgroup
    const uint32_t m0 = s * kTileM;
    __syncthreads();      // the last step's tiles are read
    row_info(g, lengths, m0, ri);
    stage_grad(gout, g, m0, sg);
    __syncthreads();
    if (want_w) {
      stage_rows<Src, V>(src, ri, p, j, k < g.K, sx);
      __syncthreads();
#pragma unroll 1      // one block of operands in flight, as in the forward
      for (uint32_t mb = 0; mb < kTileM / 16; ++mb) {
        const float* const bp = b_at + mb * 16 * kStride;
        const float b0 = bp[0], b1 = bp[kStride], b2 = bp[2 * kStride], b3 = bp[3 * kStride];
#pragma unroll
        for (int qd = 0; qd < kMaxQuads; ++qd) {
          if (qd < static_cast<int>(g.quads)) {            // uniform
            const float4 a = *reinterpret_cast<const float4*>(a_at + qd * 16 * kStride + mb * 16);
            GF_PATCH_MFMA4(acc[qd], a, b0, b1, b2, b3);
          }
        }
      }
    }
    if (sum_bias && threadIdx.x < g.C)
#pragma unroll 8
      for (int m = 0; m < kTileM; ++m) bsum += sg[threadIdx.x * kStride + m];
  }

  const uint64_t width = static_cast<uint64_t>(g.K) + 1;
  float* const mine = partials + static_cast<uint64_t>(blockIdx.y) * g.C * width;
  if (want_w) {
    const uint32_t kc = k0 + wave * 16 + i;
#pragma unroll
    for (int qd = 0; qd < kMaxQuads; ++qd) {
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const uint32_t c = qd * 16 + grp * 4 + v;      // c < C implies qd < quads
        if (c < g.C && kc < g.K) mine[c * width + kc] = acc[qd][v];
      }
    }
  }
  if (sum_bias && threadIdx.x < g.C) mine[threadIdx.x * width + g.K] = bsum;
}

#undef GF_PATCH_MFMA4

// element e = c * (K + 1) + k of the partial rows, summed in ascending row order
__global__ void __launch_bounds__(kFinishThreads)
patch_project_bwd_finish(const float* __restrict__ partials, uint32_t rows, uint32_t C, uint32_t K,
                         float* __restrict__ gw, float* __restrict__ gb) {
  const uint32_t width = K + 1, total = C * width;         // <= 128 * 4097
  const uint32_t e = blockIdx.x * kFinishThreads + threadIdx.x;
  if (e >= total) return;
  const uint32_t c = e / width, k = e % width;
  float* const to = k < K ? (gw ? gw + static_cast<uint64_t>(c) * K + k : nullptr)
                          : (gb ? gb + c : nullptr);
  if (to == nullptr) return;
  float sum = 0.f;
  for (uint32_t y = 0; y < rows; ++y) sum += partials[static_cast<uint64_t>(y) * total + e];
  *to = sum;
}

size_t lds_bytes(const Geometry& g) {
  return (kTileM + 16 * g.quads) * kStride * sizeof(float) + sizeof(RowInfo);
}

size_t partial_rows(size_t num_patches, size_t channels, size_t patch_width) {
  const size_t steps = (num_patches + kTileM - 1) / kTileM;
  size_t rows = (steps + kMinStepsPerPartialRow - 1) / kMinStepsPerPartialRow;
  rows = std::min(rows, kPatchMaxPartialRows);
  rows = std::min(rows, kPatchMaxWorkspaceFloats / (channels * (patch_width + 1)));
  return std::max<size_t>(rows, 1);
}

// the checks both directions share; false = nothing to do
bool check(const std::string& w, const PatchSource& s, size_t num_rows, size_t length,
           size_t patch, size_t dim, size_t channels, Geometry* g) {
  GF_REQUIRE(dim >= 1 && dim <= kPatchMaxWidth,
             w + ": dim outside [1, " + std::to_string(kPatchMaxWidth) + "]");
  GF_REQUIRE(length >= 1 && length <= kPatchMaxLength,
             w + ": length outside [1, " + std::to_string(kPatchMaxLength) + "]");
  GF_REQUIRE(patch >= 1 && length % patch == 0, w + ": length is not a multiple of patch");
  GF_REQUIRE(patch * dim <= kPatchMaxPatchWidth,
             w + ": patch * dim above " + std::to_string(kPatchMaxPatchWidth));
  GF_REQUIRE(channels >= 1 && channels <= kPatchMaxChannels,
             w + ": channels outside [1, " + std::to_string(kPatchMaxChannels) + "]");
  const bool table = s.d_ids != nullptr || s.d_table != nullptr;
  const bool time = s.d_delta_t != nullptr || s.d_time_weight != nullptr ||
                    s.d_time_bias != nullptr;
  GF_REQUIRE(table != time, w + ": give the ids and their table, or delta_t and the time "
                                "encoder's weight and bias, not both and not neither");
  const size_t per_row = length / patch;
  GF_REQUIRE(num_rows < (size_t{1} << 31) / per_row + ((size_t{1} << 31) % per_row != 0),
             w + ": 2^31 patches or more");
  if (num_rows == 0) return false;
  if (table)
    GF_REQUIRE(s.d_ids && s.d_table, w + ": null ids or table");
  else
    GF_REQUIRE(s.d_delta_t && s.d_time_weight && s.d_time_bias,
               w + ": null delta_t, time weight or time bias");
  const uint32_t d = static_cast<uint32_t>(dim);
  *g = {static_cast<uint32_t>(num_rows * per_row), static_cast<uint32_t>(per_row),
        static_cast<uint32_t>(length), static_cast<uint32_t>(patch), d,
        static_cast<uint32_t>(patch * dim), static_cast<uint32_t>(channels),
        static_cast<uint32_t>((channels + 15) / 16), kChunk / d, kChunk % d};
  return true;
}

// float4 units: d % 4 == 0 keeps a unit inside one slot and makes K % 4 == 0
bool vec4(const PatchSource& s, size_t dim, const float* d_weight) {
  return dim % 4 == 0 && (s.d_table == nullptr || aligned16(s.d_table)) &&
         (d_weight == nullptr || aligned16(d_weight));
}

template <class Src>
void launch_fwd(bool v4, dim3 grid, size_t lds, hipStream_t stream, const Src& src,
                const Geometry& g, const int32_t* d_lengths, const float* d_weight,
                const float* d_bias, float* d_out) {
  if (v4)
    patch_project_fwd<Src, 4><<<grid, dim3(kThreads), lds, stream>>>(src, g, d_lengths, d_weight,
                                                                    d_bias, d_out);
  else
    patch_project_fwd<Src, 1><<<grid, dim3(kThreads), lds, stream>>>(src, g, d_lengths, d_weight,
                                                                    d_bias, d_out);
}

template <class Src>
void launch_bwd(bool v4, dim3 grid, size_t lds, hipStream_t stream, const Src& src,
                const Geometry& g, const int32_t* d_lengths, const float* d_grad_out,
                uint32_t steps, uint32_t steps_per_row, bool want_w, bool want_b,
                float* d_partials) {
  if (v4)
    patch_project_bwd<Src, 4><<<grid, dim3(kThreads), lds, stream>>>(
        src, g, d_lengths, d_grad_out, steps, steps_per_row, want_w, want_b, d_partials);
  else
    patch_project_bwd<Src, 1><<<grid, dim3(kThreads), lds, stream>>>(
        src, g, d_lengths, d_grad_out, steps, steps_per_row, want_w, want_b, d_partials);
}

}  // namespace

void patch_project_forward(const PatchSource& s, size_t num_rows, size_t length, size_t patch,
                           size_t dim, const float* d_weight, const float* d_bias,
                           size_t channels, float* d_out, int device, hipStream_t stream) {
  const std::string w("patch_project");
  Geometry g;
  if (!check(w, s, num_rows, length, patch, dim, channels, &g)) return;
  GF_REQUIRE(d_weight && d_bias && d_out, w + ": null weight, bias or out");
  const bool v4 = vec4(s, dim, d_weight);
  const dim3 grid((g.patches + kTileM - 1) / kTileM);
  DeviceGuard dg(device);
  if (s.d_ids)
    launch_fwd(v4, grid, lds_bytes(g), stream, TableRows{s.d_ids, s.d_table, s.table_rows, g.d}, g,
               s.d_lengths, d_weight, d_bias, d_out);
  else
    launch_fwd(v4, grid, lds_bytes(g), stream,
               TimeRows{s.d_delta_t, s.d_time_weight, s.d_time_bias}, g, s.d_lengths, d_weight,
               d_bias, d_out);
  GF_HIP(hipGetLastError());
}

size_t patch_project_backward_partial_rows(size_t num_patches, size_t channels,
                                           size_t patch_width) {
  GF_REQUIRE(channels >= 1 && channels <= kPatchMaxChannels && patch_width >= 1 &&
                 patch_width <= kPatchMaxPatchWidth,
             "patch_project backward: channels or patch width outside the limits");
  return partial_rows(num_patches, channels, patch_width);
}

void patch_project_backward(const PatchSource& s, size_t num_rows, size_t length, size_t patch,
                            size_t dim, size_t channels, const float* d_grad_out,
                            float* d_partials, size_t partial_rows_given, float* d_grad_weight,
                            float* d_grad_bias, int device, hipStream_t stream) {
  const std::string w("patch_project backward");
  Geometry g;
  if (!check(w, s, num_rows, length, patch, dim, channels, &g)) return;
  if (!d_grad_weight && !d_grad_bias) return;
  GF_REQUIRE(d_grad_out != nullptr, w + ": null gradient");
  const size_t want = partial_rows(g.patches, g.C, g.K);
  GF_REQUIRE(d_partials != nullptr && partial_rows_given >= want,
             w + ": partials buffer missing or smaller than "
                 "gf_patch_project_backward_partial_rows() asks for");
  const uint32_t steps = (g.patches + kTileM - 1) / kTileM;
  const uint32_t steps_per_row = static_cast<uint32_t>((steps + want - 1) / want);
  const uint32_t used = (steps + steps_per_row - 1) / steps_per_row;      // <= want
  const bool want_w = d_grad_weight != nullptr, want_b = d_grad_bias != nullptr;
  const bool v4 = vec4(s, dim, nullptr);
  const dim3 grid(want_w ? (g.K + kChunk - 1) / kChunk : 1, used);
  DeviceGuard dg(device);
  if (s.d_ids)
    launch_bwd(v4, grid, lds_bytes(g), stream, TableRows{s.d_ids, s.d_table, s.table_rows, g.d}, g,
               s.d_lengths, d_grad_out, steps, steps_per_row, want_w, want_b, d_partials);
  else
    launch_bwd(v4, grid, lds_bytes(g), stream,
               TimeRows{s.d_delta_t, s.d_time_weight, s.d_time_bias}, g, s.d_lengths, d_grad_out,
               steps, steps_per_row, want_w, want_b, d_partials);
  GF_HIP(hipGetLastError());
  const uint32_t total = g.C * (g.K + 1);
  patch_project_bwd_finish<<<dim3((total + kFinishThreads - 1) / kFinishThreads),
                             dim3(kFinishThreads), 0, stream>>>(d_partials, used, g.C, g.K,
                                                                d_grad_weight, d_grad_bias);
  GF_HIP(hipGetLastError());
}

}  // namespace gf
