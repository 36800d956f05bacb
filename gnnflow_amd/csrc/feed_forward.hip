// The feed-forward of a transformer block on the float32 matrix cores, with the hidden activation
// never stored.  With m < M rows, c < C columns, j < Hd hidden columns:
//
//   u[m, j] = b1[j] + sum_c x[m, c] w1[j, c]
//   g[m, j] = 0.5 u (1 + erf(u / sqrt 2))                                  torch's default GELU
//   w[m, j] = gf_philox4x32_10_first(seed, m Hd + j, 0) >= T ? 1 / (1 - p) : 0      (p > 0; else 1)
//   y[m, c] = b2[c] + sum_j (g w)[m, j] w2[c, j]
//   dh = dy w2     du = dh w g'(u)     g'(u) = 0.5 (1 + erf(u / sqrt 2)) + u exp(-u^2 / 2) / sqrt(2 pi)
//   dx = du w1     dw1 = du^T x     db1 = colsum du     dw2 = dy^T (g w)     db2 = colsum dy
//
// Neither u, g nor the mask reaches memory in either direction: the backward recomputes u from x
// and draws the mask again.  All arithmetic is float32; the products run on
// v_mfma_f32_16x16x4_f32 with patch_project.hip's operand mapping (lane group grp = l / 16
// supplies k = 4 grp + s in step s, so a k-contiguous operand is one ds_read_b128 per 16 k; the
// lane holds D[4 grp + v][l % 16] in its four accumulator floats v).
//
// Tiles.  Every LDS tile is [64][68] floats (patch_project's stride: 68 / 4 = 17 is odd, so the
// 16 lanes of a b128 read fall on 16 bank groups, and a k-strided scalar read at (4 grp + s) 68 +
// i takes 64 banks); rows are walked 64 at a time, C and Hd in chunks of 64 columns.  Row, C and
// Hd tails are zeros in LDS, and a hidden element with j >= Hd or m >= M is written as 0 after the
// GELU (gelu(b1) of a pad would not be zero), so no product meets a float that was not written.
//
// Forward.  One workgroup of four waves per 64 rows, looping over the hidden chunks.  GEMM 1: the
// x chunk and the w1 chunk are staged per 64 columns of C and wave w takes u of rows 16 w .. 16 w
// + 15 by four quads of j.  Bias, GELU and the dropout weight are applied in the accumulator
// layout -- (m, j) is known from wave, lane and quad -- and the chunk is written once over the x
// tile as the b128 A operand of GEMM 2, whose B operand is the slice w2[:, chunk] staged whole as
// [C_pad][68].  y[64 x C_pad] stays in up to 16 accumulator quads across all hidden chunks and is
// stored once with b2 added.  LDS (64 + C_pad) 272 B: 47.9 KB at C = 100 (three workgroups a CU),
// 74.0 KB at C = 200 (two), 87.0 KB at C = 256 (one).
//
// Backward, data pass.  The same grid and loop.  Per hidden chunk: u as in the forward, dh = dy
// w2[:, chunk] with the dy chunk as the A operand and the w2 chunk [c][j] read k-strided, du in
// the accumulator layout into a third tile, and dx[64 x C_pad] += du w1[chunk, :] with the w1
// chunk [j][c] read k-strided, per 64 columns of C, into 16 quads stored once.  LDS 3 tiles, 52.2
// KB (three workgroups a CU by LDS).
//
// Backward, weight pass.  grid = (hidden chunks) x (partial rows).  A workgroup keeps dw1[chunk x
// C_pad] and dw2^T[chunk x C_pad] in accumulators (wave w: hidden rows 16 w .. 16 w + 15 by all
// C quads, 2 x 16 quads) and walks its share of the row tiles: u and dh as in the data pass, then
// du and g w are stored TRANSPOSED ([j][m]: the accumulator's four floats are four consecutive
// rows, one b128 store per quad), so that both du^T x and (g w)^T dy have b128 A operands and
// read the x and dy chunks k-strided.  db1 of the chunk is summed from the transposed du tile in
// ascending row order; hidden chunk 0 also sums dy's columns for db2.  Each workgroup writes its
// part of its partial row whole ([dw1 | dw2^T | db1 | db2]); a second launch sums the rows in
// ascending order and transposes dw2.  No atomics: the same inputs give the same bits.  LDS 4
// tiles, 69.6 KB.
//
// Staging.  A tile row is loaded by float4 when the operand's pitch is a multiple of 4 and its
// base is 16-byte aligned, by scalars otherwise; the width is a uniform run-time branch (it only
// changes how bytes are loaded: the tiles, the MFMA order and so the bits are the same), which
// keeps the instantiations to (C <= 128 or not) x (dropout or not) per pass.
#include "feed_forward.hpp"
#include "block_attention_common.hpp"

#include <algorithm>
#include <cmath>
#include <string>

namespace gf {
namespace {

constexpr int kWave = 64;
constexpr int kTileM = 64;                 // rows of a tile
constexpr int kChunk = 64;                 // columns of C or Hd staged at a time
constexpr int kStride = kChunk + 4;        // floats between the rows of an LDS tile
constexpr int kTile = kTileM * kStride;    // floats of a [64][68] tile
constexpr size_t kMinStepsPerPartialRow = 4;
constexpr int kFinishThreads = 256;
constexpr size_t kDefaultLdsLimit = 64 << 10;      // above it a kernel must be told

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct Geometry {
  uint64_t M, Hd;
  uint32_t C, quads;         // quads = ceil(C / 16)
  bool vc, vh;               // float4 loads of the operands with pitch C (x, dy, w1) / Hd (w2)
};

// tile[r][0 .. 64) = src[(r0 + r) * pitch + c0 ..] for r < fill, zeros where r0 + r >= rows or
// the column is at or past pitch.  vec: pitch % 4 == 0 and src is 16-byte aligned.
__device__ __forceinline__ void stage(const float* __restrict__ src, uint64_t pitch, uint64_t r0,
                                      uint64_t rows, uint64_t c0, bool vec,
                                      float* __restrict__ tile, uint32_t fill = kTileM) {
  if (vec) {
    const uint32_t cu = threadIdx.x % 16;
    const uint64_t c = c0 + cu * 4;                          // c + 3 < pitch when c < pitch
#pragma unroll 4
    for (uint32_t r = threadIdx.x / 16; r < fill; r += kThreads / 16) {
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (r0 + r < rows && c < pitch)
        v = *reinterpret_cast<const float4*>(src + (r0 + r) * pitch + c);
      *reinterpret_cast<float4*>(tile + r * kStride + cu * 4) = v;
    }
  } else {
    const uint32_t cu = threadIdx.x % kChunk;
    const uint64_t c = c0 + cu;
#pragma unroll 4
    for (uint32_t r = threadIdx.x / kChunk; r < fill; r += kThreads / kChunk) {
      float v = 0.f;
      if (r0 + r < rows && c < pitch) v = src[(r0 + r) * pitch + c];
      tile[r * kStride + cu] = v;
    }
  }
}

#define GF_FF_MFMA4(acc, a, b0, b1, b2, b3)                             \
  do {                                                                  \
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b0, acc, 0, 0, 0);  \
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b1, acc, 0, 0, 0);  \
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b2, acc, 0, 0, 0);  \
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b3, acc, 0, 0, 0);  \
  } while (0)

__device__ __forceinline__ uint32_t blocks_of(uint64_t columns) {      // of 16, in a chunk
  return columns >= kChunk ? kChunk / 16 : static_cast<uint32_t>((columns + 15) / 16);
}

// where a lane stands: its wave, its column i of a quad and its lane group
struct Lane {
  uint32_t wave, i, grp;
  __device__ __forceinline__ Lane()
      : wave(threadIdx.x / kWave), i(threadIdx.x % 16), grp(threadIdx.x % kWave / 16) {}
  // the lane's b128 of a k-contiguous operand whose row is (16 wave + i) -- the A operand
  __device__ __forceinline__ const float* a_of(const float* tile) const {
    return tile + (wave * 16 + i) * kStride + grp * 4;
  }
  // row 4 grp, column i of a k-strided B operand
  __device__ __forceinline__ const float* b_of(const float* tile) const {
    return tile + grp * 4 * kStride + i;
  }
};

// acc[base + q][m][n] += sum_k a[m][k] b[k][16 q + n] for q < 4 over `blocks` blocks of 16 k; a_at
// = Lane::a_of(a), b_at = Lane::b_of(b)
template <int N>
__device__ __forceinline__ void product_nn(f32x4 (&acc)[N], int base, const float* a_at,
                                           const float* b_at, uint32_t blocks) {
#pragma unroll 1      // one block of operands in flight
  for (uint32_t kb = 0; kb < blocks; ++kb) {
    const float4 a = *reinterpret_cast<const float4*>(a_at + kb * 16);
    const float* const bp = b_at + kb * 16 * kStride;
#pragma unroll
    for (int q = 0; q < 4; ++q)
      GF_FF_MFMA4(acc[base + q], a, bp[16 * q], bp[kStride + 16 * q], bp[2 * kStride + 16 * q],
                  bp[3 * kStride + 16 * q]);
  }
}

// u[q][v] = sum_c x[m0 + 16 wave + 4 grp + v, c] w1[j0 + 16 q + i, c], through sx and sw
__device__ __forceinline__ void hidden_logits(const Geometry& g, const Lane& ln,
                                              const float* __restrict__ x,
                                              const float* __restrict__ w1, uint64_t m0,
                                              uint64_t j0, float* sx, float* sw, f32x4 (&u)[4]) {
  const float* const a_at = ln.a_of(sx);
  const float* const b_at = sw + ln.i * kStride + ln.grp * 4;
  for (uint32_t k0 = 0; k0 < g.C; k0 += kChunk) {
    __syncthreads();      // the tiles' last readers are done
    stage(x, g.C, m0, g.M, k0, g.vc, sx);
    stage(w1, g.C, j0, g.Hd, k0, g.vc, sw);
    __syncthreads();
    const uint32_t blocks = blocks_of(g.C - k0);
    for (uint32_t kb = 0; kb < blocks; ++kb) {
      const float4 a = *reinterpret_cast<const float4*>(a_at + kb * 16);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float4 b = *reinterpret_cast<const float4*>(b_at + q * 16 * kStride + kb * 16);
        GF_FF_MFMA4(u[q], a, b.x, b.y, b.z, b.w);
      }
    }
  }
}

// dh[q][v] = sum_c dy[m0 + 16 wave + 4 grp + v, c] w2[c, j0 + 16 q + i], through sx and sw
__device__ __forceinline__ void hidden_grad(const Geometry& g, const Lane& ln,
                                            const float* __restrict__ dy,
                                            const float* __restrict__ w2, uint64_t m0,
                                            uint64_t j0, float* sx, float* sw, f32x4 (&dh)[4]) {
  for (uint32_t c0 = 0; c0 < g.C; c0 += kChunk) {
    __syncthreads();
    stage(dy, g.C, m0, g.M, c0, g.vc, sx);
    stage(w2, g.Hd, c0, g.C, j0, g.vh, sw);                  // sw[c][j]
    __syncthreads();
    product_nn(dh, 0, ln.a_of(sx), ln.b_of(sw), blocks_of(g.C - c0));
  }
}

template <bool DROP>
__device__ __forceinline__ float weight_of(const Dropout& dr, uint64_t counter) {
  if (!DROP) return 1.f;
  return gf_philox4x32_10_first(dr.seed, counter, 0) >= dr.threshold ? dr.scale : 0.f;
}

// CH: chunks of 64 columns the C accumulators cover (2: C <= 128, 4: C <= 256)
template <int CH, bool DROP>
__global__ void __launch_bounds__(kThreads)
feed_forward_fwd(const Geometry g, const Dropout dr, const float* __restrict__ x,
                 const float* __restrict__ w1, const float* __restrict__ b1,
                 const float* __restrict__ w2, const float* __restrict__ b2,
                 float* __restrict__ y) {
  extern __shared__ __align__(16) float lds[];
  float* const sx = lds;                   // [64][kStride]: the x chunk, then the hidden chunk
  float* const sw = lds + kTile;           // [max(64, 16 quads)][kStride]: w1 chunk, w2 slice
  const Lane ln;
  const uint64_t m0 = static_cast<uint64_t>(blockIdx.x) * kTileM;
  const uint32_t row = ln.wave * 16 + ln.grp * 4;            // + v: the lane's rows of the tile

  f32x4 acc[CH * 4];
#pragma unroll
  for (int q = 0; q < CH * 4; ++q) acc[q] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (uint64_t j0 = 0; j0 < g.Hd; j0 += kChunk) {
    f32x4 u[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) u[q] = f32x4{0.f, 0.f, 0.f, 0.f};
    hidden_logits(g, ln, x, w1, m0, j0, sx, sw, u);
    __syncthreads();      // GEMM 1 has read sw; a wave's rows of sx are its own
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const uint64_t j = j0 + q * 16 + ln.i;
      const bool live = j < g.Hd;
      const float bj = live ? b1[j] : 0.f;
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const uint64_t m = m0 + row + v;
        float h = 0.f;
        if (live && m < g.M) h = gelu(u[q][v] + bj) * weight_of<DROP>(dr, m * g.Hd + j);
        sx[(row + v) * kStride + q * 16 + ln.i] = h;
      }
    }
    stage(w2, g.Hd, 0, g.C, j0, g.vh, sw, 16 * g.quads);     // sw[c][j]
    __syncthreads();
    const uint32_t blocks = blocks_of(g.Hd - j0);
    const float* const a_at = ln.a_of(sx);
    const float* const b_at = sw + ln.i * kStride + ln.grp * 4;
    for (uint32_t kb = 0; kb < blocks; ++kb) {
      const float4 a = *reinterpret_cast<const float4*>(a_at + kb * 16);
#pragma unroll
      for (int q = 0; q < CH * 4; ++q) {
        if (q < static_cast<int>(g.quads)) {                 // uniform
          const float4 b = *reinterpret_cast<const float4*>(b_at + q * 16 * kStride + kb * 16);
          GF_FF_MFMA4(acc[q], a, b.x, b.y, b.z, b.w);
        }
      }
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
feed_forward_bwd_data(const Geometry g, const Dropout dr, const float* __restrict__ x,
                      const float* __restrict__ w1, const float* __restrict__ b1,
                      const float* __restrict__ w2, const float* __restrict__ dy,
                      float* __restrict__ dx) {
  extern __shared__ __align__(16) float lds[];
  float* const sx = lds;                   // x chunk, dy chunk
  float* const sw = lds + kTile;           // w1 chunk [j][c], w2 chunk [c][j]
  float* const sd = lds + 2 * kTile;       // du [m][j]; a wave reads the rows it wrote
  const Lane ln;
  const uint64_t m0 = static_cast<uint64_t>(blockIdx.x) * kTileM;
  const uint32_t row = ln.wave * 16 + ln.grp * 4;

  f32x4 acc[CH * 4];
#pragma unroll
  for (int q = 0; q < CH * 4; ++q) acc[q] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (uint64_t j0 = 0; j0 < g.Hd; j0 += kChunk) {
    f32x4 u[4], dh[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) u[q] = dh[q] = f32x4{0.f, 0.f, 0.f, 0.f};
    hidden_logits(g, ln, x, w1, m0, j0, sx, sw, u);
    hidden_grad(g, ln, dy, w2, m0, j0, sx, sw, dh);
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
        sd[(row + v) * kStride + q * 16 + ln.i] = du;
      }
    }
    const uint32_t blocks = blocks_of(g.Hd - j0);
#pragma unroll
    for (int cq = 0; cq < CH; ++cq) {
      if (cq * kChunk < static_cast<int>(g.C)) {             // uniform
        __syncthreads();
        stage(w1, g.C, j0, g.Hd, cq * kChunk, g.vc, sw);     // sw[j][c]
        __syncthreads();
        product_nn(acc, cq * 4, ln.a_of(sd), ln.b_of(sw), blocks);
      }
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
feed_forward_bwd_weight(const Geometry g, const Dropout dr, const float* __restrict__ x,
                        const float* __restrict__ w1, const float* __restrict__ b1,
                        const float* __restrict__ w2, const float* __restrict__ dy,
                        uint64_t steps, uint64_t steps_per_row, bool hidden, bool want_b2,
                        float* __restrict__ partials) {
  extern __shared__ __align__(16) float lds[];
  float* const sx = lds;                   // x chunk
  float* const sw = lds + kTile;           // w1 / w2 chunk, then the dy chunk
  float* const sdt = lds + 2 * kTile;      // du transposed [j][m]
  float* const sgt = lds + 3 * kTile;      // g w transposed [j][m]
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

  for (uint64_t s = s0; s < s1; ++s) {                       // uniform over the workgroup
    const uint64_t m0 = s * kTileM;
    if (hidden) {
      f32x4 u[4], dh[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) u[q] = dh[q] = f32x4{0.f, 0.f, 0.f, 0.f};
      hidden_logits(g, ln, x, w1, m0, j0, sx, sw, u);
      hidden_grad(g, ln, dy, w2, m0, j0, sx, sw, dh);
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
        *reinterpret_cast<float4*>(sdt + (q * 16 + ln.i) * kStride + row) =
            make_float4(du[0], du[1], du[2], du[3]);
        *reinterpret_cast<float4*>(sgt + (q * 16 + ln.i) * kStride + row) =
            make_float4(gw[0], gw[1], gw[2], gw[3]);
      }
    }
#pragma unroll
    for (int cq = 0; cq < CH; ++cq) {
      if (cq * kChunk < static_cast<int>(g.C)) {             // uniform
        __syncthreads();      // the transposed tiles are written; sx and sw are read
        if (hidden) stage(x, g.C, m0, g.M, cq * kChunk, g.vc, sx);
        stage(dy, g.C, m0, g.M, cq * kChunk, g.vc, sw);
        __syncthreads();
        if (sum_b2)
#pragma unroll 8
          for (int m = 0; m < kTileM; ++m) sum2[cq] += sw[m * kStride + threadIdx.x];
        if (hidden) {
          product_nn(acc1, cq * 4, ln.a_of(sdt), ln.b_of(sx), kTileM / 16);
          product_nn(acc2, cq * 4, ln.a_of(sgt), ln.b_of(sw), kTileM / 16);
        }
      }
    }
    if (hidden && threadIdx.x < kChunk)      // after a barrier that follows the transposed stores
#pragma unroll 8
      for (int m = 0; m < kTileM; ++m) sum1 += sdt[threadIdx.x * kStride + m];
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

#undef GF_FF_MFMA4

// element e of the partial rows, summed in ascending row order into the gradient it belongs to
__global__ void __launch_bounds__(kFinishThreads)
feed_forward_bwd_finish(const float* __restrict__ partials, uint32_t rows, uint64_t Hd, uint32_t C,
                        float* __restrict__ gw1, float* __restrict__ gb1, float* __restrict__ gw2,
                        float* __restrict__ gb2) {
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

size_t partial_rows(size_t num_rows, size_t width, size_t hidden) {
  const size_t steps = (num_rows + kTileM - 1) / kTileM;
  size_t rows = (steps + kMinStepsPerPartialRow - 1) / kMinStepsPerPartialRow;
  rows = std::min(rows, kFeedForwardMaxPartialRows);
  rows = std::min(rows, kFeedForwardMaxWorkspaceFloats / (2 * hidden * width + hidden + width));
  return std::max<size_t>(rows, 1);
}

// the checks both directions share; false = nothing to do
bool check(const std::string& w, size_t num_rows, size_t width, size_t hidden, Geometry* g) {
  GF_REQUIRE(width >= 1 && width <= kFeedForwardMaxWidth,
             w + ": width outside [1, " + std::to_string(kFeedForwardMaxWidth) + "]");
  GF_REQUIRE(hidden >= 1 && hidden < (size_t{1} << 36), w + ": hidden width outside [1, 2^36)");
  GF_REQUIRE(num_rows <= (size_t{1} << 36) && num_rows <= (size_t{1} << 63) / hidden,
             w + ": more than 2^36 rows, or 2^63 hidden elements or more");
  if (num_rows == 0) return false;
  *g = {num_rows, hidden, static_cast<uint32_t>(width), static_cast<uint32_t>((width + 15) / 16),
        false, false};
  return true;
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
  const float *x, *w1, *b1, *w2;
};

struct Forward {
  const Operands& o;
  const float* b2;
  float* y;
  template <int CH, bool DROP>
  void operator()() const {
    const size_t rows = std::max<size_t>(kTileM, 16 * o.g.quads);
    launch(feed_forward_fwd<CH, DROP>, dim3((o.g.M + kTileM - 1) / kTileM),
           (kTileM + rows) * kStride * sizeof(float), o.stream, o.g, o.dr, o.x, o.w1, o.b1, o.w2,
           b2, y);
  }
};

struct BackwardData {
  const Operands& o;
  const float* dy;
  float* dx;
  template <int CH, bool DROP>
  void operator()() const {
    launch(feed_forward_bwd_data<CH, DROP>, dim3((o.g.M + kTileM - 1) / kTileM),
           3 * kTile * sizeof(float), o.stream, o.g, o.dr, o.x, o.w1, o.b1, o.w2, dy, dx);
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
    launch(feed_forward_bwd_weight<CH, DROP>, grid, 4 * kTile * sizeof(float), o.stream, o.g, o.dr,
           o.x, o.w1, o.b1, o.w2, dy, steps, steps_per_row, hidden, want_b2, partials);
  }
};

}  // namespace

void feed_forward_forward(const float* d_x, const float* d_w1, const float* d_b1,
                          const float* d_w2, const float* d_b2, size_t num_rows, size_t width,
                          size_t hidden, float p, uint64_t seed, float* d_y, int device,
                          hipStream_t stream) {
  const std::string w("feed_forward");
  Geometry g;
  const Dropout dr = checked_dropout(p, seed);
  if (!check(w, num_rows, width, hidden, &g)) return;
  GF_REQUIRE(d_x && d_w1 && d_b1 && d_w2 && d_b2 && d_y, w + ": null x, weight, bias or y");
  g.vc = width % 4 == 0 && aligned16(d_x) && aligned16(d_w1);
  g.vh = hidden % 4 == 0 && aligned16(d_w2);
  DeviceGuard dg(device);
  const Operands o{g, dr, stream, d_x, d_w1, d_b1, d_w2};
  dispatch(g, p > 0.f, Forward{o, d_b2, d_y});
}

size_t feed_forward_backward_partial_rows(size_t num_rows, size_t width, size_t hidden) {
  Geometry g;
  check("feed_forward backward", num_rows, width, hidden, &g);
  return partial_rows(num_rows, width, hidden);
}

void feed_forward_backward(const float* d_x, const float* d_w1, const float* d_b1,
                           const float* d_w2, size_t num_rows, size_t width, size_t hidden,
                           float p, uint64_t seed, const float* d_grad_y, float* d_partials,
                           size_t partial_rows_given, float* d_grad_x, float* d_grad_w1,
                           float* d_grad_b1, float* d_grad_w2, float* d_grad_b2, int device,
                           hipStream_t stream) {
  const std::string w("feed_forward backward");
  Geometry g;
  const Dropout dr = checked_dropout(p, seed);
  if (!check(w, num_rows, width, hidden, &g)) return;
  const bool weights = d_grad_w1 || d_grad_b1 || d_grad_w2 || d_grad_b2;
  if (!d_grad_x && !weights) return;
  GF_REQUIRE(d_x && d_w1 && d_b1 && d_w2 && d_grad_y, w + ": null x, weight, bias or gradient");
  g.vc = width % 4 == 0 && aligned16(d_x) && aligned16(d_w1) && aligned16(d_grad_y);
  g.vh = hidden % 4 == 0 && aligned16(d_w2);
  DeviceGuard dg(device);
  const Operands o{g, dr, stream, d_x, d_w1, d_b1, d_w2};
  if (d_grad_x) dispatch(g, p > 0.f, BackwardData{o, d_grad_y, d_grad_x});
  if (!weights) return;
  const size_t want = partial_rows(num_rows, width, hidden);
  GF_REQUIRE(d_partials != nullptr && partial_rows_given >= want,
             w + ": partials buffer missing or smaller than "
                 "gf_feed_forward_backward_partial_rows() asks for");
  const uint64_t steps = (num_rows + kTileM - 1) / kTileM;
  const uint64_t steps_per_row = (steps + want - 1) / want;
  const uint32_t used = static_cast<uint32_t>((steps + steps_per_row - 1) / steps_per_row);
  const bool hidden_wanted = d_grad_w1 || d_grad_b1 || d_grad_w2;
  const dim3 grid(hidden_wanted ? static_cast<unsigned>((hidden + kChunk - 1) / kChunk) : 1, used);
  dispatch(g, p > 0.f, BackwardWeight{o, d_grad_y, grid, steps, steps_per_row, hidden_wanted,
                                      d_grad_b2 != nullptr, d_partials});
  const uint64_t total = 2 * g.Hd * g.C + g.Hd + g.C;
  const uint64_t blocks = std::min<uint64_t>((total + kFinishThreads - 1) / kFinishThreads, 1u << 20);
  feed_forward_bwd_finish<<<dim3(static_cast<unsigned>(blocks)), dim3(kFinishThreads), 0,
                            stream>>>(
      d_partials, used, g.Hd, g.C, d_grad_w1, d_grad_b1, d_grad_w2, d_grad_b2);
  GF_HIP(hipGetLastError());
}

}  // namespace gf
