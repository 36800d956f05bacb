// feed_forward.hip's op with both products of every pass on v_mfma_f32_16x16x32_bf16: float32
// tensors in memory, bfloat16 matrix operands, float32 sums.  bf(v) = widen(narrow(v)) (bf16.hpp):
//
//   u  = b1 + sum_c bf(x) bf(w1)                       float32, never rounded
//   h  = bf(gelu(u) w)                                 w: feed_forward.hip's Philox weight
//   y  = b2 + sum_j h bf(w2)
//   dh = sum_c bf(dy) bf(w2)      du = bf(dh w gelu'(u))
//   dx = sum_j du bf(w1)    dw1 = sum_m du bf(x)    dw2 = sum_m bf(dy) h
//   db1 = colsum du    db2 = colsum bf(dy)             both summed AFTER rounding, from the LDS tiles
//
// Neither u, h nor the mask reaches memory; the backward recomputes u and draws the mask again.
//
// Operands.  A lane l of the instruction supplies eight consecutive k of row (A) or column (B)
// l % 16 starting at 8 (l / 16), one ds_read_b128, and holds D[4 (l / 16) + v][l % 16] in its four
// accumulator floats: the accumulator layout of the float32 instruction, so bias, GELU and mask
// are applied as feed_forward.hip applies them.  EVERY operand of every product is k-contiguous
// bfloat16 in LDS; nothing is read k-strided.  Tile rows are 64 n + 8 elements apart (72 for a
// 64-column tile, C_pad + 8 for a full-width one): 16 bytes times an odd number, so the 16 lanes
// of a b128 read fall on distinct bank groups.
//
// Weights.  A pack launch ahead of each pass rounds w1 and w2 once and writes every orientation
// the pass reads into the caller's workspace, rows and columns zero-padded to multiples of 64
// (Hp, Cp): the forward W1 [Hp][Cp] and W2 [Cp][Hp]; the backward W1, W2T [Hp][Cp] and W1T
// [Cp][Hp].  Staging a weight tile is then a straight 16-byte copy with no bounds to check.  The
// padding is to 64, not to the k step of 32: a 64-row or 64-column tile never leaves its array.
//
// Forward.  One workgroup of four waves per 64 rows.  The x tile is rounded and staged ONCE, full
// width ([64][Cp + 8]); per hidden chunk of 64 the w1 chunk [64][Cp + 8] and the w2 slice
// [16 quads][72] are copied in, wave w takes u of rows 16 w .. 16 w + 15 by four quads of j over
// ceil(C / 32) steps, writes h as bfloat16 into a [64][72] tile, and y[64 x Cp] stays in up to 16
// accumulator quads across the chunks.  Two barriers a chunk.  LDS 113.7 KB at Cp = 256, 62.5 KB
// at Cp = 128.
//
// Backward, data pass.  x and dy tiles staged once, full width.  Per chunk: W1 and W2T chunks in,
// u and dh in one loop over C (two A reads, eight B reads, eight instructions a step), du to a
// [64][72] tile, the W1T slice [16 quads][72] copied over the two weight chunks, dx += du W1T.
// LDS 144.4 KB at Cp = 256, 78.8 KB at Cp = 128.
//
// Backward, weight pass.  grid = (hidden chunks) x (partial rows); the W1 and W2T chunks of the
// workgroup's hidden chunk are copied in once and stay.  Per row tile: u and dh from [64][72]
// chunks of x and dy; du and h go TRANSPOSED ([j][m]: a lane's four floats are four consecutive
// rows, one 8-byte store); then x and dy are staged transposed ([c][m]: a thread loads the same
// four columns of four consecutive rows and stores four packed 8-byte groups), and dw1[chunk x
// Cp] and dw2^T[chunk x Cp] accumulate in 2 x 16 quads.  Partial rows and the finishing launch are
// feed_forward.hip's scheme (its own copy here: that file's is private to it).  LDS 104.4 KB at
// Cp = 256, 71.7 KB at Cp = 128.
//
// Loads of x and dy are float4 when C % 4 == 0 and the bases are 16-byte aligned, scalars
// otherwise: a uniform run-time branch that changes how bytes are loaded and not one bit of the
// result.
#include "feed_forward.hpp"
#include "block_attention_common.hpp"

#include <algorithm>
#include <string>

namespace gf {
namespace {

constexpr int kWave = 64;
constexpr int kTileM = 64;                 // rows of a tile
constexpr int kChunk = 64;                 // columns of Hd (and of C in the weight pass) at a time
constexpr int kStep = 32;                  // k of one matrix instruction
constexpr int kPad = 8;                    // elements added to a tile row: its bytes / 16 are odd
constexpr int kStride = kChunk + kPad;     // elements between the rows of a 64-column tile
constexpr int kTile = kTileM * kStride;    // elements of a [64][72] tile
constexpr size_t kMinStepsPerPartialRow = 4;
constexpr int kFinishThreads = 256;
constexpr int kPackThreads = 256;
constexpr size_t kDefaultLdsLimit = 64 << 10;      // above it a kernel must be told

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

struct Geometry {
  uint64_t M, Hd, Hp;        // Hp, Cp: Hd, C rounded up to 64, the workspace's dimensions
  uint32_t C, Cp, quads;     // quads = ceil(C / 16)
  bool vec;                  // float4 loads of x and dy
};

__device__ __forceinline__ uint32_t pack2(float a, float b) {
  return static_cast<uint32_t>(narrow(a)) | static_cast<uint32_t>(narrow(b)) << 16;
}

__device__ __forceinline__ uint2 pack4(const float (&v)[4]) {
  return make_uint2(pack2(v[0], v[1]), pack2(v[2], v[3]));
}

__device__ __forceinline__ bf16x8 load8(const uint16_t* at) {      // one ds_read_b128
  return __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(at));
}

__device__ __forceinline__ f32x4 mfma(bf16x8 a, bf16x8 b, f32x4 acc) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc, 0, 0, 0);
}

// v[0 .. 4) = src[row * pitch + c ..], zeros at or past pitch; row is a row of the operand
__device__ __forceinline__ void load4(const float* __restrict__ src, uint64_t pitch, uint64_t row,
                                      uint64_t c, bool vec, float (&v)[4]) {
  const float* const at = src + row * pitch + c;
  if (vec) {                                                 // c + 3 < pitch when c < pitch
    float4 f = make_float4(0.f, 0.f, 0.f, 0.f);
    if (c < pitch) f = *reinterpret_cast<const float4*>(at);
    v[0] = f.x, v[1] = f.y, v[2] = f.z, v[3] = f.w;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = c + k < pitch ? at[k] : 0.f;
  }
}

// tile[r][0 .. width) = bf(src[(r0 + r) * pitch + c0 ..]) for r < 64, zeros where r0 + r >= rows
// or the column is at or past pitch; width a multiple of 4
__device__ __forceinline__ void stage_rows(const float* __restrict__ src, uint64_t pitch,
                                           uint64_t r0, uint64_t rows, uint32_t c0, uint32_t width,
                                           bool vec, uint16_t* __restrict__ tile, uint32_t stride) {
  const uint32_t per_row = width / 4;
  for (uint32_t e = threadIdx.x; e < kTileM * per_row; e += kThreads) {
    const uint32_t r = e / per_row, cu = e % per_row * 4;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (r0 + r < rows) load4(src, pitch, r0 + r, c0 + cu, vec, v);
    *reinterpret_cast<uint2*>(tile + r * stride + cu) = pack4(v);
  }
}

// tile[c][m] = bf(src[(r0 + m) * pitch + c0 + c]) for c, m < 64, zeros as in stage_rows: thread t
// loads columns 4 (t % 16) .. + 3 of rows 4 (t / 16) .. + 3 and stores four packed groups of rows
__device__ __forceinline__ void stage_transposed(const float* __restrict__ src, uint64_t pitch,
                                                 uint64_t r0, uint64_t rows, uint32_t c0, bool vec,
                                                 uint16_t* __restrict__ tile) {
  const uint32_t cu = threadIdx.x % 16 * 4, ru = threadIdx.x / 16 * 4;
  float v[4][4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    v[k][0] = v[k][1] = v[k][2] = v[k][3] = 0.f;
    if (r0 + ru + k < rows) load4(src, pitch, r0 + ru + k, c0 + cu, vec, v[k]);
  }
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const float col[4] = {v[0][c], v[1][c], v[2][c], v[3][c]};
    *reinterpret_cast<uint2*>(tile + (cu + c) * kStride + ru) = pack4(col);
  }
}

// tile[r][0 .. width) = src[r * pitch ..] for r < rows: packed weights, 16 bytes at a time
__device__ __forceinline__ void copy_rows(const uint16_t* __restrict__ src, uint64_t pitch,
                                          uint32_t rows, uint32_t width,
                                          uint16_t* __restrict__ tile, uint32_t stride) {
  const uint32_t per_row = width / 8;
  for (uint32_t e = threadIdx.x; e < rows * per_row; e += kThreads) {
    const uint32_t r = e / per_row, cu = e % per_row * 8;
    *reinterpret_cast<u32x4*>(tile + r * stride + cu) =
        *reinterpret_cast<const u32x4*>(src + r * pitch + cu);
  }
}

__device__ __forceinline__ uint32_t steps_of(uint64_t columns) {      // of 32 k, in a chunk
  return columns >= kChunk ? kChunk / kStep : static_cast<uint32_t>((columns + kStep - 1) / kStep);
}

// where a lane stands: its wave, its row or column i of a quad and its lane group
struct Lane {
  uint32_t wave, i, grp;
  __device__ __forceinline__ Lane()
      : wave(threadIdx.x / kWave), i(threadIdx.x % 16), grp(threadIdx.x % kWave / 16) {}
  // the lane's eight k of row `first + i` of a tile whose rows are `stride` apart
  __device__ __forceinline__ const uint16_t* at(const uint16_t* tile, uint32_t stride,
                                                uint32_t first) const {
    return tile + (first + i) * stride + grp * 8;
  }
};

template <bool DROP>
__device__ __forceinline__ float weight_of(const Dropout& dr, uint64_t counter) {
  if (!DROP) return 1.f;
  return gf_philox4x32_10_first(dr.seed, counter, 0) >= dr.threshold ? dr.scale : 0.f;
}

// CH: chunks of 64 columns the C accumulators cover (2: C <= 128, 4: C <= 256)
template <int CH, bool DROP>
__global__ void __launch_bounds__(kThreads)
feed_forward_bf16_fwd(const Geometry g, const Dropout dr, const float* __restrict__ x,
                      const uint16_t* __restrict__ W1, const float* __restrict__ b1,
                      const uint16_t* __restrict__ W2, const float* __restrict__ b2,
                      float* __restrict__ y) {
  extern __shared__ __align__(16) uint16_t lds[];
  const uint32_t sc = g.Cp + kPad;
  uint16_t* const sx = lds;                        // [64][sc]: bf(x), staged once
  uint16_t* const sw1 = sx + kTileM * sc;          // [64][sc]: W1[j0 .. j0 + 64)
  uint16_t* const sh = sw1 + kChunk * sc;          // [64][72]: the hidden chunk
  uint16_t* const sw2 = sh + kTile;                // [16 quads][72]: W2[:, j0 .. j0 + 64)
  const Lane ln;
  const uint64_t m0 = static_cast<uint64_t>(blockIdx.x) * kTileM;
  const uint32_t row = ln.wave * 16 + ln.grp * 4;            // + v: the lane's rows of the tile
  const uint32_t csteps = (g.C + kStep - 1) / kStep;

  f32x4 acc[CH * 4];
#pragma unroll
  for (int q = 0; q < CH * 4; ++q) acc[q] = f32x4{0.f, 0.f, 0.f, 0.f};

  stage_rows(x, g.C, m0, g.M, 0, g.Cp, g.vec, sx, sc);
  for (uint64_t j0 = 0; j0 < g.Hd; j0 += kChunk) {
    __syncthreads();      // the last chunk's readers are done
    copy_rows(W1 + j0 * g.Cp, g.Cp, kChunk, g.Cp, sw1, sc);
    copy_rows(W2 + j0, g.Hp, 16 * g.quads, kChunk, sw2, kStride);
    __syncthreads();
    f32x4 u[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) u[q] = f32x4{0.f, 0.f, 0.f, 0.f};
    {
      const uint16_t* const a_at = ln.at(sx, sc, ln.wave * 16);
      const uint16_t* const b_at = ln.at(sw1, sc, 0);
      for (uint32_t kb = 0; kb < csteps; ++kb) {
        const bf16x8 a = load8(a_at + kb * kStep);
#pragma unroll
        for (int q = 0; q < 4; ++q) u[q] = mfma(a, load8(b_at + q * 16 * sc + kb * kStep), u[q]);
      }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const uint64_t j = j0 + q * 16 + ln.i;
      const bool live = j < g.Hd;
      const float bj = live ? b1[j] : 0.f;
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const uint64_t m = m0 + row + v;
        float h = 0.f;      // a pad is 0 after the GELU: gelu(b1) of one would not be
        if (live && m < g.M) h = gelu(u[q][v] + bj) * weight_of<DROP>(dr, m * g.Hd + j);
        sh[(row + v) * kStride + q * 16 + ln.i] = narrow(h);
      }
    }
    __syncthreads();
    const uint32_t hsteps = steps_of(g.Hd - j0);
    const uint16_t* const a_at = ln.at(sh, kStride, ln.wave * 16);
    const uint16_t* const b_at = ln.at(sw2, kStride, 0);
    for (uint32_t kb = 0; kb < hsteps; ++kb) {
      const bf16x8 a = load8(a_at + kb * kStep);
#pragma unroll
      for (int q = 0; q < CH * 4; ++q)
        if (q < static_cast<int>(g.quads))                   // uniform
          acc[q] = mfma(a, load8(b_at + q * 16 * kStride + kb * kStep), acc[q]);
    }
  }

#pragma unroll
  for (int q = 0; q < CH * 4; ++q) {
    const uint32_t c = q * 16 + ln.i;
    if (c < g.C) {
      const float bc = b2[c];
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const uint64_t m = m0 + row + v;
        if (m < g.M) y[m * g.C + c] = acc[q][v] + bc;
      }
    }
  }
}

template <int CH, bool DROP>
__global__ void __launch_bounds__(kThreads)
feed_forward_bf16_bwd_data(const Geometry g, const Dropout dr, const float* __restrict__ x,
                           const uint16_t* __restrict__ W1, const float* __restrict__ b1,
                           const uint16_t* __restrict__ W2T, const uint16_t* __restrict__ W1T,
                           const float* __restrict__ dy, float* __restrict__ dx) {
  extern __shared__ __align__(16) uint16_t lds[];
  const uint32_t sc = g.Cp + kPad;
  uint16_t* const sx = lds;                        // [64][sc]: bf(x), staged once
  uint16_t* const sdy = sx + kTileM * sc;          // [64][sc]: bf(dy), staged once
  uint16_t* const sw1 = sdy + kTileM * sc;         // [64][sc]: W1[j0 .. j0 + 64)
  uint16_t* const sw2t = sw1 + kChunk * sc;        // [64][sc]: W2T[j0 .. j0 + 64)
  uint16_t* const sw1t = sw1;                      // [16 quads][72] over both: W1T[:, j0 .. + 64)
  uint16_t* const sd = sw2t + kChunk * sc;         // [64][72]: du
  const Lane ln;
  const uint64_t m0 = static_cast<uint64_t>(blockIdx.x) * kTileM;
  const uint32_t row = ln.wave * 16 + ln.grp * 4;
  const uint32_t csteps = (g.C + kStep - 1) / kStep;

  f32x4 acc[CH * 4];
#pragma unroll
  for (int q = 0; q < CH * 4; ++q) acc[q] = f32x4{0.f, 0.f, 0.f, 0.f};

  stage_rows(x, g.C, m0, g.M, 0, g.Cp, g.vec, sx, sc);
  stage_rows(dy, g.C, m0, g.M, 0, g.Cp, g.vec, sdy, sc);
  for (uint64_t j0 = 0; j0 < g.Hd; j0 += kChunk) {
    __syncthreads();      // the last chunk's readers of sw1t and sd are done
    copy_rows(W1 + j0 * g.Cp, g.Cp, kChunk, g.Cp, sw1, sc);
    copy_rows(W2T + j0 * g.Cp, g.Cp, kChunk, g.Cp, sw2t, sc);
    __syncthreads();
    f32x4 u[4], dh[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) u[q] = dh[q] = f32x4{0.f, 0.f, 0.f, 0.f};
    {
      const uint16_t* const x_at = ln.at(sx, sc, ln.wave * 16);
      const uint16_t* const dy_at = ln.at(sdy, sc, ln.wave * 16);
      const uint16_t* const w1_at = ln.at(sw1, sc, 0);
      const uint16_t* const w2_at = ln.at(sw2t, sc, 0);
      for (uint32_t kb = 0; kb < csteps; ++kb) {
        const bf16x8 ax = load8(x_at + kb * kStep), ady = load8(dy_at + kb * kStep);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          u[q] = mfma(ax, load8(w1_at + q * 16 * sc + kb * kStep), u[q]);
          dh[q] = mfma(ady, load8(w2_at + q * 16 * sc + kb * kStep), dh[q]);
        }
      }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const uint64_t j = j0 + q * 16 + ln.i;
      const bool live = j < g.Hd;
      const float bj = live ? b1[j] : 0.f;
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const uint64_t m = m0 + row + v;
        float du = 0.f;
        if (live && m < g.M)
          du = dh[q][v] * weight_of<DROP>(dr, m * g.Hd + j) * gelu_grad(u[q][v] + bj);
        sd[(row + v) * kStride + q * 16 + ln.i] = narrow(du);
      }
    }
    __syncthreads();      // the weight chunks are read; du is written
    copy_rows(W1T + j0, g.Hp, 16 * g.quads, kChunk, sw1t, kStride);
    __syncthreads();
    const uint32_t hsteps = steps_of(g.Hd - j0);
    const uint16_t* const a_at = ln.at(sd, kStride, ln.wave * 16);
    const uint16_t* const b_at = ln.at(sw1t, kStride, 0);
    for (uint32_t kb = 0; kb < hsteps; ++kb) {
      const bf16x8 a = load8(a_at + kb * kStep);
#pragma unroll
      for (int q = 0; q < CH * 4; ++q)
        if (q < static_cast<int>(g.quads))                   // uniform
          acc[q] = mfma(a, load8(b_at + q * 16 * kStride + kb * kStep), acc[q]);
    }
  }

#pragma unroll
  for (int q = 0; q < CH * 4; ++q) {
    const uint32_t c = q * 16 + ln.i;
    if (c < g.C) {
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const uint64_t m = m0 + row + v;
        if (m < g.M) dx[m * g.C + c] = acc[q][v];
      }
    }
  }
}

// A partial row is [dw1: Hd x C | dw2^T: Hd x C | db1: Hd | db2: C].  hidden false: only db2 is
// wanted, gridDim.x == 1 and nothing of size Hd is computed.
template <int CH, bool DROP>
__global__ void __launch_bounds__(kThreads)
feed_forward_bf16_bwd_weight(const Geometry g, const Dropout dr, const float* __restrict__ x,
                             const uint16_t* __restrict__ W1, const float* __restrict__ b1,
                             const uint16_t* __restrict__ W2T, const float* __restrict__ dy,
                             uint64_t steps, uint64_t steps_per_row, bool hidden, bool want_b2,
                             float* __restrict__ partials) {
  extern __shared__ __align__(16) uint16_t lds[];
  const uint32_t sc = g.Cp + kPad;
  uint16_t* const sw1 = lds;                       // [64][sc]: W1[j0 .. j0 + 64), staged once
  uint16_t* const sw2t = sw1 + kChunk * sc;        // [64][sc]: W2T[j0 .. j0 + 64), staged once
  uint16_t* const sa = sw2t + kChunk * sc;         // x chunk [m][c], then transposed [c][m]
  uint16_t* const sb = sa + kTile;                 // dy chunk [m][c], then transposed [c][m]
  uint16_t* const sdt = sb + kTile;                // du transposed [j][m]
  uint16_t* const sgt = sdt + kTile;               // h transposed [j][m]
  const Lane ln;
  const uint64_t j0 = static_cast<uint64_t>(blockIdx.x) * kChunk;
  const uint64_t s0 = blockIdx.y * steps_per_row;            // < steps
  const uint64_t s1 = steps - s0 < steps_per_row ? steps : s0 + steps_per_row;
  const uint32_t row = ln.wave * 16 + ln.grp * 4;
  const bool sum_b2 = want_b2 && blockIdx.x == 0 && threadIdx.x < kChunk;

  f32x4 acc1[CH * 4], acc2[CH * 4];
#pragma unroll
  for (int q = 0; q < CH * 4; ++q) acc1[q] = acc2[q] = f32x4{0.f, 0.f, 0.f, 0.f};
  float sum1 = 0.f, sum2[CH];
#pragma unroll
  for (int cq = 0; cq < CH; ++cq) sum2[cq] = 0.f;

  if (hidden) {      // read after the first barrier of the row loop
    copy_rows(W1 + j0 * g.Cp, g.Cp, kChunk, g.Cp, sw1, sc);
    copy_rows(W2T + j0 * g.Cp, g.Cp, kChunk, g.Cp, sw2t, sc);
  }
  for (uint64_t s = s0; s < s1; ++s) {                       // uniform over the workgroup
    const uint64_t m0 = s * kTileM;
    if (hidden) {
      f32x4 u[4], dh[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) u[q] = dh[q] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int cq = 0; cq < CH; ++cq) {
        if (cq * kChunk < static_cast<int>(g.C)) {           // uniform
          __syncthreads();      // the tiles' last readers are done
          stage_rows(x, g.C, m0, g.M, cq * kChunk, kChunk, g.vec, sa, kStride);
          stage_rows(dy, g.C, m0, g.M, cq * kChunk, kChunk, g.vec, sb, kStride);
          __syncthreads();
          const uint32_t csteps = steps_of(g.C - cq * kChunk);
          const uint16_t* const x_at = ln.at(sa, kStride, ln.wave * 16);
          const uint16_t* const dy_at = ln.at(sb, kStride, ln.wave * 16);
          const uint16_t* const w1_at = ln.at(sw1, sc, 0) + cq * kChunk;
          const uint16_t* const w2_at = ln.at(sw2t, sc, 0) + cq * kChunk;
          for (uint32_t kb = 0; kb < csteps; ++kb) {
            const bf16x8 ax = load8(x_at + kb * kStep), ady = load8(dy_at + kb * kStep);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              u[q] = mfma(ax, load8(w1_at + q * 16 * sc + kb * kStep), u[q]);
              dh[q] = mfma(ady, load8(w2_at + q * 16 * sc + kb * kStep), dh[q]);
            }
          }
        }
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const uint64_t j = j0 + q * 16 + ln.i;
        const bool live = j < g.Hd;
        const float bj = live ? b1[j] : 0.f;
        float du[4] = {0.f, 0.f, 0.f, 0.f}, gw[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          const uint64_t m = m0 + row + v;
          if (live && m < g.M) {
            const float uu = u[q][v] + bj, w = weight_of<DROP>(dr, m * g.Hd + j);
            gw[v] = gelu(uu) * w;
            du[v] = dh[q][v] * w * gelu_grad(uu);
          }
        }
        *reinterpret_cast<uint2*>(sdt + (q * 16 + ln.i) * kStride + row) = pack4(du);
        *reinterpret_cast<uint2*>(sgt + (q * 16 + ln.i) * kStride + row) = pack4(gw);
      }
    }
#pragma unroll
    for (int cq = 0; cq < CH; ++cq) {
      if (cq * kChunk < static_cast<int>(g.C)) {             // uniform
        __syncthreads();      // the transposed tiles are written; sa and sb are read
        if (hidden) stage_transposed(x, g.C, m0, g.M, cq * kChunk, g.vec, sa);
        stage_transposed(dy, g.C, m0, g.M, cq * kChunk, g.vec, sb);
        __syncthreads();
        if (sum_b2)
#pragma unroll 8
          for (int m = 0; m < kTileM; ++m) sum2[cq] += widen(sb[threadIdx.x * kStride + m]);
        if (hidden) {
          const uint16_t* const du_at = ln.at(sdt, kStride, ln.wave * 16);
          const uint16_t* const h_at = ln.at(sgt, kStride, ln.wave * 16);
          const uint16_t* const x_at = ln.at(sa, kStride, 0);
          const uint16_t* const dy_at = ln.at(sb, kStride, 0);
#pragma unroll
          for (int kb = 0; kb < kTileM / kStep; ++kb) {
            const bf16x8 adu = load8(du_at + kb * kStep), ah = load8(h_at + kb * kStep);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              acc1[cq * 4 + q] =
                  mfma(adu, load8(x_at + q * 16 * kStride + kb * kStep), acc1[cq * 4 + q]);
              acc2[cq * 4 + q] =
                  mfma(ah, load8(dy_at + q * 16 * kStride + kb * kStep), acc2[cq * 4 + q]);
            }
          }
        }
      }
    }
    if (hidden && threadIdx.x < kChunk)      // after a barrier that follows the transposed stores
#pragma unroll 8
      for (int m = 0; m < kTileM; ++m) sum1 += widen(sdt[threadIdx.x * kStride + m]);
  }

  const uint64_t hc = g.Hd * g.C;
  float* const mine = partials + static_cast<uint64_t>(blockIdx.y) * (2 * hc + g.Hd + g.C);
  if (hidden) {
#pragma unroll
    for (int q = 0; q < CH * 4; ++q) {
      const uint32_t c = q * 16 + ln.i;
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const uint64_t j = j0 + row + v;
        if (c < g.C && j < g.Hd) {
          mine[j * g.C + c] = acc1[q][v];
          mine[hc + j * g.C + c] = acc2[q][v];
        }
      }
    }
    if (threadIdx.x < kChunk && j0 + threadIdx.x < g.Hd) mine[2 * hc + j0 + threadIdx.x] = sum1;
  }
  if (sum_b2) {
#pragma unroll
    for (int cq = 0; cq < CH; ++cq) {
      const uint32_t c = cq * kChunk + threadIdx.x;
      if (c < g.C) mine[2 * hc + g.Hd + c] = sum2[cq];
    }
  }
}

// element e of the partial rows, summed in ascending row order into the gradient it belongs to
__global__ void __launch_bounds__(kFinishThreads)
feed_forward_bf16_bwd_finish(const float* __restrict__ partials, uint32_t rows, uint64_t Hd,
                             uint32_t C, float* __restrict__ gw1, float* __restrict__ gb1,
                             float* __restrict__ gw2, float* __restrict__ gb2) {
  const uint64_t hc = Hd * C, total = 2 * hc + Hd + C;
  for (uint64_t e = static_cast<uint64_t>(blockIdx.x) * kFinishThreads + threadIdx.x; e < total;
       e += static_cast<uint64_t>(gridDim.x) * kFinishThreads) {
    float* to = nullptr;
    if (e < hc) {
      to = gw1 ? gw1 + e : nullptr;
    } else if (e < 2 * hc) {
      const uint64_t j = (e - hc) / C, c = (e - hc) % C;
      to = gw2 ? gw2 + c * Hd + j : nullptr;
    } else if (e < 2 * hc + Hd) {
      to = gb1 ? gb1 + (e - 2 * hc) : nullptr;
    } else {
      to = gb2 ? gb2 + (e - 2 * hc - Hd) : nullptr;
    }
    if (to == nullptr) continue;      // not wanted: its part of the rows may not be written
    float sum = 0.f;
    for (uint32_t r = 0; r < rows; ++r) sum += partials[r * total + e];
    *to = sum;
  }
}

// One array of the workspace: dst[r][c] (rows_p x cols_p, zero outside rows x cols) = bf(src[r *
// cols + c]), or bf(src[c * rows + r]) when the source holds the transpose.
struct PackJob {
  const float* src;
  uint16_t* dst;
  uint64_t rows, cols, rows_p, cols_p;
  bool transposed;
};
struct PackJobs {
  PackJob job[3];
};

// blockIdx.y picks the array; consecutive threads write consecutive elements
__global__ void __launch_bounds__(kPackThreads) feed_forward_bf16_pack(const PackJobs jobs) {
  const PackJob& jb = jobs.job[blockIdx.y];
  const uint64_t total = jb.rows_p * jb.cols_p;
  for (uint64_t e = static_cast<uint64_t>(blockIdx.x) * kPackThreads + threadIdx.x; e < total;
       e += static_cast<uint64_t>(gridDim.x) * kPackThreads) {
    const uint64_t r = e / jb.cols_p, c = e % jb.cols_p;
    float v = 0.f;
    if (r < jb.rows && c < jb.cols) v = jb.src[jb.transposed ? c * jb.rows + r : r * jb.cols + c];
    jb.dst[e] = narrow(v);
  }
}

size_t round64(size_t n) { return (n + 63) / 64 * 64; }

size_t partial_rows(size_t num_rows, size_t width, size_t hidden) {
  const size_t steps = (num_rows + kTileM - 1) / kTileM;
  size_t rows = (steps + kMinStepsPerPartialRow - 1) / kMinStepsPerPartialRow;
  rows = std::min(rows, kFeedForwardMaxPartialRows);
  rows = std::min(rows, kFeedForwardMaxWorkspaceFloats / (2 * hidden * width + hidden + width));
  return std::max<size_t>(rows, 1);
}

void check_sizes(const std::string& w, size_t width, size_t hidden) {
  GF_REQUIRE(width >= 1 && width <= kFeedForwardMaxWidth,
             w + ": width outside [1, " + std::to_string(kFeedForwardMaxWidth) + "]");
  GF_REQUIRE(hidden >= 1 && hidden < (size_t{1} << 36), w + ": hidden width outside [1, 2^36)");
}

// the checks both directions share; false = nothing to do
bool check(const std::string& w, size_t num_rows, size_t width, size_t hidden, Geometry* g) {
  check_sizes(w, width, hidden);
  GF_REQUIRE(num_rows <= (size_t{1} << 36) && num_rows <= (size_t{1} << 63) / hidden,
             w + ": more than 2^36 rows, or 2^63 hidden elements or more");
  if (num_rows == 0) return false;
  *g = {num_rows, hidden, round64(hidden), static_cast<uint32_t>(width),
        static_cast<uint32_t>(round64(width)), static_cast<uint32_t>((width + 15) / 16), false};
  return true;
}

// the arrays of the workspace, in the order the pack launch fills them
struct Packed {
  uint16_t *W1, *second, *W1T;      // second: W2 [Cp][Hp] (forward) or W2T [Hp][Cp] (backward)
};

Packed pack(const std::string& w, const Geometry& g, const float* d_w1, const float* d_w2,
            bool backward, void* d_workspace, size_t bytes, hipStream_t stream) {
  GF_REQUIRE(d_workspace != nullptr && aligned16(d_workspace) &&
                 bytes >= feed_forward_bf16_workspace(g.C, g.Hd, backward),
             w + ": workspace missing, not 16-byte aligned or smaller than "
                 "gf_feed_forward_bf16_workspace() asks for");
  const uint64_t each = g.Hp * g.Cp;
  uint16_t* const base = static_cast<uint16_t*>(d_workspace);
  const Packed out{base, base + each, backward ? base + 2 * each : nullptr};
  PackJobs jobs{};
  jobs.job[0] = {d_w1, out.W1, g.Hd, g.C, g.Hp, g.Cp, false};
  if (backward) {
    jobs.job[1] = {d_w2, out.second, g.Hd, g.C, g.Hp, g.Cp, true};     // w2 is [C][Hd]
    jobs.job[2] = {d_w1, out.W1T, g.C, g.Hd, g.Cp, g.Hp, true};        // w1 is [Hd][C]
  } else {
    jobs.job[1] = {d_w2, out.second, g.C, g.Hd, g.Cp, g.Hp, false};
  }
  const uint64_t blocks = std::min<uint64_t>((each + kPackThreads - 1) / kPackThreads, 1u << 16);
  feed_forward_bf16_pack<<<dim3(static_cast<unsigned>(blocks), backward ? 3 : 2),
                           dim3(kPackThreads), 0, stream>>>(jobs);
  GF_HIP(hipGetLastError());
  return out;
}

template <class Kernel, class... Args>
void launch(Kernel kernel, dim3 grid, size_t lds, hipStream_t stream, Args... args) {
  if (lds > kDefaultLdsLimit)
    GF_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                               hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds)));
  kernel<<<grid, dim3(kThreads), lds, stream>>>(args...);
  GF_HIP(hipGetLastError());
}

// calls f.template operator()<CH, DROP>() for the instantiation of (C chunks, dropout)
template <class F>
void dispatch(const Geometry& g, bool drop, F&& f) {
  if (g.C <= 2 * kChunk)
    return drop ? f.template operator()<2, true>() : f.template operator()<2, false>();
  return drop ? f.template operator()<4, true>() : f.template operator()<4, false>();
}

struct Operands {
  const Geometry& g;
  const Dropout& dr;
  hipStream_t stream;
  const float *x, *b1;
  const Packed& w;
  size_t wide() const { return size_t{kTileM} * (g.Cp + kPad); }      // elements of a [64][sc] tile
};

struct Forward {
  const Operands& o;
  const float* b2;
  float* y;
  template <int CH, bool DROP>
  void operator()() const {
    const size_t elements = 2 * o.wide() + kTile + size_t{16} * o.g.quads * kStride;
    launch(feed_forward_bf16_fwd<CH, DROP>, dim3((o.g.M + kTileM - 1) / kTileM),
           elements * sizeof(uint16_t), o.stream, o.g, o.dr, o.x, o.w.W1, o.b1, o.w.second, b2, y);
  }
};

struct BackwardData {
  const Operands& o;
  const float* dy;
  float* dx;
  template <int CH, bool DROP>
  void operator()() const {
    launch(feed_forward_bf16_bwd_data<CH, DROP>, dim3((o.g.M + kTileM - 1) / kTileM),
           (4 * o.wide() + kTile) * sizeof(uint16_t), o.stream, o.g, o.dr, o.x, o.w.W1, o.b1,
           o.w.second, o.w.W1T, dy, dx);
  }
};

struct BackwardWeight {
  const Operands& o;
  const float* dy;
  dim3 grid;
  uint64_t steps, steps_per_row;
  bool hidden, want_b2;
  float* partials;
  template <int CH, bool DROP>
  void operator()() const {
    launch(feed_forward_bf16_bwd_weight<CH, DROP>, grid,
           (2 * o.wide() + 4 * kTile) * sizeof(uint16_t), o.stream, o.g, o.dr, o.x, o.w.W1, o.b1,
           o.w.second, dy, steps, steps_per_row, hidden, want_b2, partials);
  }
};

}  // namespace

size_t feed_forward_bf16_workspace(size_t width, size_t hidden, bool backward) {
  check_sizes("feed_forward_bf16 workspace", width, hidden);
  return (backward ? 3 : 2) * round64(hidden) * round64(width) * sizeof(uint16_t);
}

void feed_forward_bf16_forward(const float* d_x, const float* d_w1, const float* d_b1,
                               const float* d_w2, const float* d_b2, size_t num_rows,
                               size_t width, size_t hidden, float p, uint64_t seed,
                               void* d_workspace, size_t workspace_bytes, float* d_y, int device,
                               hipStream_t stream) {
  const std::string w("feed_forward_bf16");
  Geometry g;
  const Dropout dr = checked_dropout(p, seed);
  if (!check(w, num_rows, width, hidden, &g)) return;
  GF_REQUIRE(d_x && d_w1 && d_b1 && d_w2 && d_b2 && d_y, w + ": null x, weight, bias or y");
  g.vec = width % 4 == 0 && aligned16(d_x);
  DeviceGuard dg(device);
  const Packed packed = pack(w, g, d_w1, d_w2, false, d_workspace, workspace_bytes, stream);
  const Operands o{g, dr, stream, d_x, d_b1, packed};
  dispatch(g, p > 0.f, Forward{o, d_b2, d_y});
}

size_t feed_forward_bf16_backward_partial_rows(size_t num_rows, size_t width, size_t hidden) {
  Geometry g;
  check("feed_forward_bf16 backward", num_rows, width, hidden, &g);
  return partial_rows(num_rows, width, hidden);
}

void feed_forward_bf16_backward(const float* d_x, const float* d_w1, const float* d_b1,
                                const float* d_w2, size_t num_rows, size_t width, size_t hidden,
                                float p, uint64_t seed, const float* d_grad_y, void* d_workspace,
                                size_t workspace_bytes, float* d_partials,
                                size_t partial_rows_given, float* d_grad_x, float* d_grad_w1,
                                float* d_grad_b1, float* d_grad_w2, float* d_grad_b2, int device,
                                hipStream_t stream) {
  const std::string w("feed_forward_bf16 backward");
  Geometry g;
  const Dropout dr = checked_dropout(p, seed);
  if (!check(w, num_rows, width, hidden, &g)) return;
  const bool weights = d_grad_w1 || d_grad_b1 || d_grad_w2 || d_grad_b2;
  if (!d_grad_x && !weights) return;
  GF_REQUIRE(d_x && d_w1 && d_b1 && d_w2 && d_grad_y, w + ": null x, weight, bias or gradient");
  size_t want = 0;
  if (weights) {
    want = partial_rows(num_rows, width, hidden);
    GF_REQUIRE(d_partials != nullptr && partial_rows_given >= want,
               w + ": partials buffer missing or smaller than "
                   "gf_feed_forward_bf16_backward_partial_rows() asks for");
  }
  g.vec = width % 4 == 0 && aligned16(d_x) && aligned16(d_grad_y);
  DeviceGuard dg(device);
  const Packed packed = pack(w, g, d_w1, d_w2, true, d_workspace, workspace_bytes, stream);
  const Operands o{g, dr, stream, d_x, d_b1, packed};
  if (d_grad_x) dispatch(g, p > 0.f, BackwardData{o, d_grad_y, d_grad_x});
  if (!weights) return;
  const uint64_t steps = (num_rows + kTileM - 1) / kTileM;
  const uint64_t steps_per_row = (steps + want - 1) / want;
  const uint32_t used = static_cast<uint32_t>((steps + steps_per_row - 1) / steps_per_row);
  const bool hidden_wanted = d_grad_w1 || d_grad_b1 || d_grad_w2;
  const dim3 grid(hidden_wanted ? static_cast<unsigned>((hidden + kChunk - 1) / kChunk) : 1, used);
  dispatch(g, p > 0.f, BackwardWeight{o, d_grad_y, grid, steps, steps_per_row, hidden_wanted,
                                      d_grad_b2 != nullptr, d_partials});
  const uint64_t total = 2 * g.Hd * g.C + g.Hd + g.C;
  const uint64_t blocks = std::min<uint64_t>((total + kFinishThreads - 1) / kFinishThreads, 1u << 20);
  feed_forward_bf16_bwd_finish<<<dim3(static_cast<unsigned>(blocks)), dim3(kFinishThreads), 0,
                                 stream>>>(
      d_partials, used, g.Hd, g.C, d_grad_w1, d_grad_b1, d_grad_w2, d_grad_b2);
  GF_HIP(hipGetLastError());
}

}  // namespace gf
