// The token-mixing half of a GraphMixer block on the float32 matrix cores, with nothing of the
// size of x stored besides y.  With n < N rows, k < K tokens, j < Kh hidden units, c < C columns:
//
//   mean[n,k], var[n,k] over c of x[n,k,:] (biased)     rstd = 1 / sqrt(var + eps)
//   xh = (x - mean) rstd                                 z[n,k,c] = xh gamma[c] + beta[c]
//   u[n,j,c] = b1[j] + sum_k w1[j,k] z[n,k,c]            h = gelu(u) m1[n,j,c]
//   t[n,k,c] = b2[k] + sum_j w2[k,j] h[n,j,c]            y = x + t m2[n,k,c]
//   m1 = gf_philox4x32_10_first(seed, (n C + c) Kh + j, 0) >= T ? 1 / (1 - p) : 0     (p > 0; else 1)
//   m2 = gf_philox4x32_10_first(seed, (n C + c) K  + k, 1) >= T ? 1 / (1 - p) : 0
//   dt = dy m2    dh = w2^T dt    du = dh m1 gelu'(u)    dz = w1^T du    a = dz gamma
//   dx = dy + rstd (a - mean_c a - xh mean_c (a xh))
//   dw2 = sum_{n,c} dt h^T    db2 = sum_{n,c} dt    dw1 = sum_{n,c} du z^T    db1 = sum_{n,c} du
//   dgamma = sum_{n,k} dz xh    dbeta = sum_{n,k} dz
//
// Once mean and rstd of a row n are known its columns c are independent, so tokens and hidden
// units are the M and k axes of every product and the columns are the N axis: x[n] is used as it
// lies in memory, [k][c] with c contiguous, and nothing is transposed.  The products run on
// v_mfma_f32_16x16x4_f32 with patch_project.hip's operand mapping (lane group grp = l / 16 supplies
// k = 4 grp + s in step s; the lane holds D[4 grp + v][l % 16] in its four accumulator floats v).
//
// Tiles.  Every LDS tile has rows of 64 floats at a stride of 68 (feed_forward.hip's: a b128 read
// of 16 rows falls on 16 bank groups, a k-strided scalar read on 64 banks) and 16 ceil(K / 16) or
// 16 ceil(Kh / 16) rows, not 64: a row of x is small and the kernels want several workgroups a
// CU.  The weights are staged once per workgroup as the b128 A operands (and, in the backward,
// their transposes, so that w2^T dt and w1^T du have b128 A operands too) and stay while the
// workgroup walks rows n = blockIdx.x, + gridDim.x, ...  A row is walked in chunks of 64 columns;
// wave w owns columns 16 w .. 16 w + 15 of the chunk in every product over tokens, so between the
// two GEMMs a wave reads only the columns of h it wrote.  Pad tokens, pad hidden units and pad
// columns are zeros in LDS, h and du of a pad are written as 0 after the GELU, and a wave whose
// columns lie past C writes zeros: no product meets a float that was not written.
//
// Forward.  Per row: mean and rstd of its K token rows by wave reductions (wave w: tokens w, w + 4,
// ...; the variance from the deviations), kept in LDS and written out for the backward.  Per
// chunk: z staged normalised, GEMM 1, bias + GELU + m1 in the accumulator layout into the h tile,
// GEMM 2, and y = x + (t + b2) m2 stored from the accumulator layout, 16 consecutive columns per
// token row; x is read again from memory there (the cache has it from the staging) instead of
// from a tile of its own, which would cost a fifth of the LDS.
//
// Backward.  One kernel, the same walk with dt = dy m2 staged beside z.  Per chunk: u and dh = w2^T
// dt (the same accumulator layout, so du is elementwise), h and du into two tiles, dz = w1^T du,
// and a = dz gamma, which is parked in dx while sum_c a and sum_c a xh are summed: in the lane over
// the chunks, then over the 16 lanes of a lane group, then over the four waves through LDS in wave
// order.  Once the row's chunks are through every lane finishes the elements of dx it parked (its
// own stores, so no fence is needed); holding a in registers instead (16 quads at C = 256) took
// the kernel past 256 registers and into scratch.  The parameter
// gradients are summed over the rows a workgroup walks: dw1 = du z^T and dw2 = dt h^T contract over
// c with both operands read b128 along c, their up to 16 + 16 blocks of 16 x 16 dealt to the waves
// (dw2 two waves on, so that at K = 32, Kh = 16 all four work) and kept in 4 + 4 accumulator
// quads; db1 and db2 are row sums of the du and dt tiles (thread t: row t / 4, columns 16 (t % 4)
// .. + 15, in ascending order, so the bits do not depend on how the tiles were loaded); dgamma and
// dbeta are column sums in the accumulator layout, added into two LDS vectors whose element c has
// one lane as its only writer.  Each workgroup writes one partial row [dw1 |
// dw2 | db1 | db2 | dgamma | dbeta]; a second launch sums the rows in ascending order.  No
// atomics: the same inputs give the same bits.
//
// Staging.  A row of x or dy is loaded by float4 when C is a multiple of 4 and the base is 16-byte
// aligned, by scalars otherwise: a uniform run-time branch that changes how bytes are loaded and
// nothing else.  Instantiations: dropout or not, per direction.
#include "token_mix.hpp"
#include "block_attention_common.hpp"

#include <algorithm>
#include <string>

namespace gf {
namespace {

constexpr int kWave = 64;
constexpr int kChunk = 64;                 // columns of C staged at a time
constexpr int kStride = kChunk + 4;        // floats between the rows of an LDS tile
constexpr int kMaxTokens = static_cast<int>(kTokenMixMaxTokens);
constexpr int kMaxWidth = static_cast<int>(kTokenMixMaxWidth);
constexpr size_t kRowsPerWorkgroup = 4;    // a workgroup is not started for fewer rows
constexpr size_t kForwardMaxWorkgroups = 2048;
constexpr int kFinishThreads = 256;
constexpr size_t kDefaultLdsLimit = 64 << 10;      // above it a kernel must be told
static_assert(kMaxTokens == kChunk && kMaxWidth % kChunk == 0 && kThreads == 4 * kWave,
              "a weight is one tile; four waves own the four column blocks of a chunk");

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct Geometry {
  uint64_t N;
  uint32_t K, Kh, C, KB, JB;     // KB = ceil(K / 16), JB = ceil(Kh / 16)
  bool vec;                      // float4 loads of x (and dy)
};

#define GF_TM_MFMA4(acc, a, b0, b1, b2, b3)                             \
  do {                                                                  \
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b0, acc, 0, 0, 0);  \
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b1, acc, 0, 0, 0);  \
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b2, acc, 0, 0, 0);  \
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b3, acc, 0, 0, 0);  \
  } while (0)

// where a lane stands: its wave (the column block it owns), its column i of a block, its lane group
struct Lane {
  uint32_t wave, i, grp;
  __device__ __forceinline__ Lane()
      : wave(threadIdx.x / kWave), i(threadIdx.x % 16), grp(threadIdx.x % kWave / 16) {}
};

__device__ __forceinline__ uint32_t blocks_of(uint32_t columns) {      // of 16, in a chunk
  return columns >= kChunk ? kChunk / 16 : (columns + 15) / 16;
}

// [v] = sum_k a[16 mb + 4 grp + v][k] b[k][16 wave + i] over k < 16 KBk: a is a k-contiguous tile
// of more than 16 mb rows, b a tile of 16 KBk rows
__device__ __forceinline__ f32x4 product(const float* a_tile, uint32_t mb, const float* b_tile,
                                         uint32_t KBk, const Lane& ln) {
  const float* const a_at = a_tile + (16 * mb + ln.i) * kStride + ln.grp * 4;
  const float* const b_at = b_tile + ln.grp * 4 * kStride + ln.wave * 16 + ln.i;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (uint32_t kb = 0; kb < KBk; ++kb) {
    const float4 a = *reinterpret_cast<const float4*>(a_at + kb * 16);
    const float* const bp = b_at + kb * 16 * kStride;
    GF_TM_MFMA4(acc, a, bp[0], bp[kStride], bp[2 * kStride], bp[3 * kStride]);
  }
  return acc;
}

// acc[v] += sum_c a[16 ab + 4 grp + v][c] b[16 bb + i][c] over c < 16 cblocks: both read b128
__device__ __forceinline__ void product_over_columns(f32x4& acc, const float* a_tile, uint32_t ab,
                                                     const float* b_tile, uint32_t bb,
                                                     uint32_t cblocks, const Lane& ln) {
  const float* const a_at = a_tile + (16 * ab + ln.i) * kStride + ln.grp * 4;
  const float* const b_at = b_tile + (16 * bb + ln.i) * kStride + ln.grp * 4;
  for (uint32_t cb = 0; cb < cblocks; ++cb) {
    const float4 a = *reinterpret_cast<const float4*>(a_at + cb * 16);
    const float4 b = *reinterpret_cast<const float4*>(b_at + cb * 16);
    GF_TM_MFMA4(acc, a, b.x, b.y, b.z, b.w);
  }
}

// tile[r][c] = src[r][c] of a [rows, cols] matrix, or src[c][r] of a [cols, rows] one, for r <
// fill and c < 64; zeros past rows and cols
__device__ __forceinline__ void stage_weight(const float* __restrict__ src, uint32_t rows,
                                             uint32_t cols, bool transposed, uint32_t fill,
                                             float* __restrict__ tile) {
  for (uint32_t e = threadIdx.x; e < fill * kChunk; e += kThreads) {
    const uint32_t r = e / kChunk, c = e % kChunk;
    float v = 0.f;
    if (r < rows && c < cols) v = transposed ? src[c * rows + r] : src[r * cols + c];
    tile[r * kStride + c] = v;
  }
}

// to[e] = from[e] for e < n, zeros up to `fill`
__device__ __forceinline__ void stage_vector(const float* __restrict__ from, uint32_t n,
                                             uint32_t fill, float* __restrict__ to) {
  for (uint32_t e = threadIdx.x; e < fill; e += kThreads) to[e] = e < n ? from[e] : 0.f;
}

// tile[k][0 .. 64) = f(k, c, row[k * C + c]) at c = c0 + column for k < K and c < C, zeros for the
// other k < fill and c.  vec: C % 4 == 0 and row is 16-byte aligned.
template <class F>
__device__ __forceinline__ void stage(const float* __restrict__ row, const Geometry& g,
                                      uint32_t c0, uint32_t fill, float* __restrict__ tile, F f) {
  if (g.vec) {
    const uint32_t cu = threadIdx.x % 16, c = c0 + cu * 4;   // c + 3 < C when c < C
    for (uint32_t k = threadIdx.x / 16; k < fill; k += kThreads / 16) {
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (k < g.K && c < g.C) {
        v = *reinterpret_cast<const float4*>(row + k * g.C + c);
        v = make_float4(f(k, c, v.x), f(k, c + 1, v.y), f(k, c + 2, v.z), f(k, c + 3, v.w));
      }
      *reinterpret_cast<float4*>(tile + k * kStride + cu * 4) = v;
    }
  } else {
    const uint32_t cu = threadIdx.x % kChunk, c = c0 + cu;
    for (uint32_t k = threadIdx.x / kChunk; k < fill; k += kThreads / kChunk) {
      float v = 0.f;
      if (k < g.K && c < g.C) v = f(k, c, row[k * g.C + c]);
      tile[k * kStride + cu] = v;
    }
  }
}

// sum of columns 16 part .. 16 part + 15 of a tile's row, in ascending order
__device__ __forceinline__ float row_sum16(const float* tile, uint32_t row, uint32_t part) {
  const float* const at = tile + row * kStride + part * 16;
  float s = 0.f;
#pragma unroll
  for (int c = 0; c < 16; ++c) s += at[c];
  return s;
}

template <bool DROP>
__device__ __forceinline__ float weight_of(const Dropout& dr, uint64_t counter, uint32_t call) {
  if (!DROP) return 1.f;
  return gf_philox4x32_10_first(dr.seed, counter, call) >= dr.threshold ? dr.scale : 0.f;
}

template <bool DROP>
__global__ void __launch_bounds__(kThreads)
token_mix_fwd(const Geometry g, const Dropout dr, const float eps, const float* __restrict__ x,
              const float* __restrict__ gamma, const float* __restrict__ beta,
              const float* __restrict__ w1, const float* __restrict__ b1,
              const float* __restrict__ w2, const float* __restrict__ b2, float* __restrict__ y,
              float* __restrict__ mean, float* __restrict__ rstd) {
  extern __shared__ __align__(16) float lds[];
  const uint32_t KP = 16 * g.KB, JP = 16 * g.JB;
  float* const sw1 = lds;                          // [JP][kStride]: w1[j][k]
  float* const sw2 = sw1 + JP * kStride;           // [KP][kStride]: w2[k][j]
  float* const sz = sw2 + KP * kStride;            // [KP][kStride]: z[k][c] of the chunk
  float* const sh = sz + KP * kStride;             // [JP][kStride]: h[j][c] of the chunk
  float* const sb1 = sh + JP * kStride;            // [64]
  float* const sb2 = sb1 + kMaxTokens;             // [64]
  float* const sgamma = sb2 + kMaxTokens;          // [256]
  float* const sbeta = sgamma + kMaxWidth;         // [256]
  float* const smean = sbeta + kMaxWidth;          // [64]
  float* const srstd = smean + kMaxTokens;         // [64]
  const Lane ln;
  const uint32_t lane = threadIdx.x % kWave;

  stage_weight(w1, g.Kh, g.K, false, JP, sw1);
  stage_weight(w2, g.K, g.Kh, false, KP, sw2);
  stage_vector(b1, g.Kh, kMaxTokens, sb1);
  stage_vector(b2, g.K, kMaxTokens, sb2);
  stage_vector(gamma, g.C, kMaxWidth, sgamma);
  stage_vector(beta, g.C, kMaxWidth, sbeta);

  for (uint64_t n = blockIdx.x; n < g.N; n += gridDim.x) {   // uniform over the workgroup
    const uint64_t at = n * g.K * g.C;
    const float* const xn = x + at;
    float* const yn = y + at;
    __syncthreads();      // the last row's readers of smean and srstd are done
    for (uint32_t k = ln.wave; k < g.K; k += kThreads / kWave) {
      float v[kMaxWidth / kWave], sum = 0.f, sq = 0.f;
#pragma unroll
      for (int t = 0; t < kMaxWidth / kWave; ++t) {
        const uint32_t c = lane + t * kWave;
        v[t] = c < g.C ? xn[k * g.C + c] : 0.f;
        sum += v[t];
      }
      const float m = group_sum<kWave>(sum) / static_cast<float>(g.C);
#pragma unroll
      for (int t = 0; t < kMaxWidth / kWave; ++t) {
        const float d = lane + t * kWave < g.C ? v[t] - m : 0.f;
        sq += d * d;
      }
      const float r = 1.f / sqrtf(group_sum<kWave>(sq) / static_cast<float>(g.C) + eps);
      if (lane == 0) {
        smean[k] = m;
        srstd[k] = r;
        mean[n * g.K + k] = m;
        rstd[n * g.K + k] = r;
      }
    }

    for (uint32_t c0 = 0; c0 < g.C; c0 += kChunk) {
      __syncthreads();      // smean and srstd are written; the tiles' last readers are done
      stage(xn, g, c0, KP, sz, [&](uint32_t k, uint32_t c, float v) {
        return (v - smean[k]) * srstd[k] * sgamma[c] + sbeta[c];
      });
      __syncthreads();
      const bool live = ln.wave < blocks_of(g.C - c0);       // uniform over the wave
      const uint32_t cc = ln.wave * 16 + ln.i, c = c0 + cc;
      if (live) {
#pragma unroll 1      // one quad's GELUs and draws in flight
        for (uint32_t jb = 0; jb < g.JB; ++jb) {
          const f32x4 u = product(sw1, jb, sz, g.KB, ln);
#pragma unroll
          for (int v = 0; v < 4; ++v) {
            const uint32_t j = jb * 16 + ln.grp * 4 + v;
            float h = 0.f;
            if (j < g.Kh && c < g.C)
              h = gelu(u[v] + sb1[j]) * weight_of<DROP>(dr, (n * g.C + c) * g.Kh + j, 0);
            sh[j * kStride + cc] = h;
          }
        }
      }
      __syncthreads();      // a wave reads the columns of sh it wrote; this orders its lanes
      if (live) {
#pragma unroll 1
        for (uint32_t kb = 0; kb < g.KB; ++kb) {
          const f32x4 t = product(sw2, kb, sh, g.JB, ln);
#pragma unroll
          for (int v = 0; v < 4; ++v) {
            const uint32_t k = kb * 16 + ln.grp * 4 + v;
            if (k < g.K && c < g.C)
              yn[k * g.C + c] = xn[k * g.C + c] +
                                (t[v] + sb2[k]) * weight_of<DROP>(dr, (n * g.C + c) * g.K + k, 1);
          }
        }
      }
    }
  }
}

// A partial row is [dw1: Kh x K | dw2: K x Kh | db1: Kh | db2: K | dgamma: C | dbeta: C].  params
// false: no parameter gradient is wanted and partials is not written; dx may be null.
template <bool DROP>
__global__ void __launch_bounds__(kThreads, 2)      // two waves a SIMD at the least
token_mix_bwd(const Geometry g, const Dropout dr, const float* __restrict__ x,
              const float* __restrict__ gamma, const float* __restrict__ beta,
              const float* __restrict__ w1, const float* __restrict__ b1,
              const float* __restrict__ w2, const float* __restrict__ mean,
              const float* __restrict__ rstd, const float* __restrict__ dy, const bool params,
              float* __restrict__ partials, float* __restrict__ dx) {
  extern __shared__ __align__(16) float lds[];
  const uint32_t KP = 16 * g.KB, JP = 16 * g.JB;
  float* const sw1 = lds;                          // [JP][kStride]: w1[j][k]
  float* const sw1t = sw1 + JP * kStride;          // [KP][kStride]: w1[j][k] at [k][j]
  float* const sw2t = sw1t + KP * kStride;         // [JP][kStride]: w2[k][j] at [j][k]
  float* const sz = sw2t + JP * kStride;           // [KP][kStride]: z[k][c] of the chunk
  float* const sdt = sz + KP * kStride;            // [KP][kStride]: dt[k][c]
  float* const sh = sdt + KP * kStride;            // [JP][kStride]: h[j][c]
  float* const sdu = sh + JP * kStride;            // [JP][kStride]: du[j][c]
  float* const sb1 = sdu + JP * kStride;           // [64]
  float* const sgamma = sb1 + kMaxTokens;          // [256]
  float* const sbeta = sgamma + kMaxWidth;         // [256]
  float* const sdgamma = sbeta + kMaxWidth;        // [256]: column c has one lane, its only writer
  float* const sdbeta = sdgamma + kMaxWidth;       // [256]
  float* const smean = sdbeta + kMaxWidth;         // [64]
  float* const srstd = smean + kMaxTokens;         // [64]
  float* const sred = srstd + kMaxTokens;          // [2][4 waves][64]: sum_c a, sum_c a xh
  const Lane ln;
  const uint32_t sum_row = threadIdx.x / 4, sum_part = threadIdx.x % 4;      // of row_sum16
  const uint32_t cc = ln.wave * 16 + ln.i;                   // the lane's column of a chunk
  const float inv_c = 1.f / static_cast<float>(g.C);

  stage_weight(w1, g.Kh, g.K, false, JP, sw1);
  stage_weight(w1, g.K, g.Kh, true, KP, sw1t);
  stage_weight(w2, g.Kh, g.K, true, JP, sw2t);
  stage_vector(b1, g.Kh, kMaxTokens, sb1);
  stage_vector(gamma, g.C, kMaxWidth, sgamma);
  stage_vector(beta, g.C, kMaxWidth, sbeta);
  stage_vector(gamma, 0, 2 * kMaxWidth, sdgamma);            // zeros, sdbeta too

  f32x4 dw1[4], dw2[4];      // blocks wave + 4 t of dw1, (wave + 2) % 4 + 4 t of dw2
#pragma unroll
  for (int t = 0; t < 4; ++t) dw1[t] = dw2[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  float db1 = 0.f, db2 = 0.f;

  for (uint64_t n = blockIdx.x; n < g.N; n += gridDim.x) {   // uniform over the workgroup
    const uint64_t at = n * g.K * g.C;
    const float* const xn = x + at;
    const float* const dyn = dy + at;
    float* const dxn = dx ? dx + at : nullptr;
    __syncthreads();      // the last row's readers of smean, srstd and sred are done
    if (threadIdx.x < g.K) {
      smean[threadIdx.x] = mean[n * g.K + threadIdx.x];
      srstd[threadIdx.x] = rstd[n * g.K + threadIdx.x];
    }
    f32x4 s1[4], s2[4];      // the lane's sums over c of a = dz gamma and of a xh
#pragma unroll
    for (int kb = 0; kb < 4; ++kb) s1[kb] = s2[kb] = f32x4{0.f, 0.f, 0.f, 0.f};

#pragma unroll 1
    for (uint32_t c0 = 0; c0 < g.C; c0 += kChunk) {
      const uint32_t c = c0 + cc;
      __syncthreads();      // smean and srstd are written; the tiles' last readers are done
      stage(xn, g, c0, KP, sz, [&](uint32_t k, uint32_t cs, float v) {
        return (v - smean[k]) * srstd[k] * sgamma[cs] + sbeta[cs];
      });
      stage(dyn, g, c0, KP, sdt, [&](uint32_t k, uint32_t cs, float v) {
        return v * weight_of<DROP>(dr, (n * g.C + cs) * g.K + k, 1);
      });
      __syncthreads();
      const uint32_t cblocks = blocks_of(g.C - c0);
      const bool live = ln.wave < cblocks;                   // uniform over the wave
      if (params && sum_row < g.K) db2 += row_sum16(sdt, sum_row, sum_part);
#pragma unroll 1      // one quad's GELUs and draws in flight
      for (uint32_t jb = 0; jb < g.JB; ++jb) {
        f32x4 u = {0.f, 0.f, 0.f, 0.f}, dh = u;
        if (live) {
          u = product(sw1, jb, sz, g.KB, ln);
          dh = product(sw2t, jb, sdt, g.KB, ln);
        }
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          const uint32_t j = jb * 16 + ln.grp * 4 + v;
          float h = 0.f, du = 0.f;                           // of a wave past C too
          if (live && j < g.Kh && c < g.C) {
            const float uu = u[v] + sb1[j];
            const float w = weight_of<DROP>(dr, (n * g.C + c) * g.Kh + j, 0);
            h = gelu(uu) * w;
            du = dh[v] * w * gelu_grad(uu);
          }
          sh[j * kStride + cc] = h;
          sdu[j * kStride + cc] = du;
        }
      }
      __syncthreads();      // the h and du tiles are whole
      if (live) {
        const float gam = c < g.C ? sgamma[c] : 0.f;
        float colg = 0.f, colb = 0.f;
#pragma unroll
        for (int kb = 0; kb < 4; ++kb) {
          if (kb < static_cast<int>(g.KB)) {                 // uniform
            const f32x4 dz = product(sw1t, kb, sdu, g.JB, ln);
#pragma unroll
            for (int v = 0; v < 4; ++v) {
              const uint32_t k = kb * 16 + ln.grp * 4 + v;
              const bool real = k < g.K && c < g.C;
              const float xh = real ? (xn[k * g.C + c] - smean[k]) * srstd[k] : 0.f;
              const float d = dz[v], av = d * gam;           // 0 for a pad k or c
              colb += d;
              colg += d * xh;
              s1[kb][v] += av;
              s2[kb][v] += av * xh;
              if (real && dx != nullptr) dxn[k * g.C + c] = av;      // finished below, by this lane
            }
          }
        }
        colg += __shfl_xor(colg, 16, kWave);
        colg += __shfl_xor(colg, 32, kWave);
        colb += __shfl_xor(colb, 16, kWave);
        colb += __shfl_xor(colb, 32, kWave);
        if (ln.grp == 0 && c < g.C) {
          sdgamma[c] += colg;
          sdbeta[c] += colb;
        }
      }
      if (params) {
        if (sum_row < g.Kh) db1 += row_sum16(sdu, sum_row, sum_part);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const uint32_t b1k = ln.wave + 4 * t, b2k = (ln.wave + 2) % 4 + 4 * t;
          if (b1k < g.JB * g.KB)                             // uniform over the wave
            product_over_columns(dw1[t], sdu, b1k / g.KB, sz, b1k % g.KB, cblocks, ln);
          if (b2k < g.JB * g.KB)
            product_over_columns(dw2[t], sdt, b2k / g.JB, sh, b2k % g.JB, cblocks, ln);
        }
      }
    }

    if (dx == nullptr) continue;                             // uniform
#pragma unroll
    for (int kb = 0; kb < 4; ++kb) {
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        float p1 = s1[kb][v], p2 = s2[kb][v];
#pragma unroll
        for (int off = 1; off < 16; off <<= 1) {
          p1 += __shfl_xor(p1, off, kWave);
          p2 += __shfl_xor(p2, off, kWave);
        }
        if (ln.i == 0 && kb < static_cast<int>(g.KB)) {
          const uint32_t k = kb * 16 + ln.grp * 4 + v;
          sred[ln.wave * kMaxTokens + k] = p1;
          sred[(4 + ln.wave) * kMaxTokens + k] = p2;
        }
      }
    }
    __syncthreads();
    // dx = dy + rstd (a - mean_c a - xh mean_c (a xh)): every lane finishes the a it stored
#pragma unroll 1
    for (uint32_t kq = ln.grp; kq < 4 * g.KB; kq += 4) {     // k = 16 kb + 4 grp + v, kq = k / 4
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const uint32_t k = kq * 4 + v;
        if (k >= g.K) continue;
        const float* const r1 = sred + k;
        const float* const r2 = sred + 4 * kMaxTokens + k;
        const float m1 = (r1[0] + r1[kMaxTokens] + r1[2 * kMaxTokens] + r1[3 * kMaxTokens]) * inv_c;
        const float m2 = (r2[0] + r2[kMaxTokens] + r2[2 * kMaxTokens] + r2[3 * kMaxTokens]) * inv_c;
        const float mu = smean[k], rs = srstd[k];
#pragma unroll 1
        for (uint32_t c = cc; c < g.C; c += kChunk) {
          const uint32_t e = k * g.C + c;
          const float xh = (xn[e] - mu) * rs;
          dxn[e] = dyn[e] + rs * (dxn[e] - m1 - xh * m2);
        }
      }
    }
  }

  if (!params) return;
  __syncthreads();      // sdgamma and sdbeta of the last row
  const uint32_t kk = g.K * g.Kh;
  float* const mine = partials + static_cast<uint64_t>(blockIdx.x) * (2 * kk + g.K + g.Kh + 2 * g.C);
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const uint32_t b1k = ln.wave + 4 * t, b2k = (ln.wave + 2) % 4 + 4 * t;
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      if (b1k < g.JB * g.KB) {
        const uint32_t j = b1k / g.KB * 16 + ln.grp * 4 + v, k = b1k % g.KB * 16 + ln.i;
        if (j < g.Kh && k < g.K) mine[j * g.K + k] = dw1[t][v];
      }
      if (b2k < g.JB * g.KB) {
        const uint32_t k = b2k / g.JB * 16 + ln.grp * 4 + v, j = b2k % g.JB * 16 + ln.i;
        if (k < g.K && j < g.Kh) mine[kk + k * g.Kh + j] = dw2[t][v];
      }
    }
  }
  db1 += __shfl_xor(db1, 1, kWave);
  db1 += __shfl_xor(db1, 2, kWave);
  db2 += __shfl_xor(db2, 1, kWave);
  db2 += __shfl_xor(db2, 2, kWave);
  if (sum_part == 0 && sum_row < g.Kh) mine[2 * kk + sum_row] = db1;
  if (sum_part == 0 && sum_row < g.K) mine[2 * kk + g.Kh + sum_row] = db2;
  for (uint32_t c = threadIdx.x; c < g.C; c += kThreads) {
    mine[2 * kk + g.Kh + g.K + c] = sdgamma[c];
    mine[2 * kk + g.Kh + g.K + g.C + c] = sdbeta[c];
  }
}

#undef GF_TM_MFMA4

// element e of the partial rows, summed in ascending row order into the gradient it belongs to
__global__ void __launch_bounds__(kFinishThreads)
token_mix_bwd_finish(const float* __restrict__ partials, uint32_t rows, uint32_t K, uint32_t Kh,
                     uint32_t C, float* __restrict__ gw1, float* __restrict__ gw2,
                     float* __restrict__ gb1, float* __restrict__ gb2, float* __restrict__ ggamma,
                     float* __restrict__ gbeta) {
  const uint32_t kk = K * Kh, total = 2 * kk + K + Kh + 2 * C;
  const uint32_t e = blockIdx.x * kFinishThreads + threadIdx.x;
  if (e >= total) return;
  float* to;
  if (e < kk) to = gw1 ? gw1 + e : nullptr;
  else if (e < 2 * kk) to = gw2 ? gw2 + (e - kk) : nullptr;
  else if (e < 2 * kk + Kh) to = gb1 ? gb1 + (e - 2 * kk) : nullptr;
  else if (e < 2 * kk + Kh + K) to = gb2 ? gb2 + (e - 2 * kk - Kh) : nullptr;
  else if (e < 2 * kk + Kh + K + C) to = ggamma ? ggamma + (e - 2 * kk - Kh - K) : nullptr;
  else to = gbeta ? gbeta + (e - 2 * kk - Kh - K - C) : nullptr;
  if (to == nullptr) return;
  float sum = 0.f;
#pragma unroll 16
  for (uint32_t r = 0; r < rows; ++r) sum += partials[static_cast<uint64_t>(r) * total + e];
  *to = sum;
}

size_t partial_row_floats(size_t tokens, size_t hidden, size_t width) {
  return 2 * tokens * hidden + tokens + hidden + 2 * width;
}

// workgroups of a walk over num_rows rows, each with kRowsPerWorkgroup rows or more (or all)
size_t workgroups(size_t num_rows, size_t most) {
  return std::max<size_t>(std::min((num_rows + kRowsPerWorkgroup - 1) / kRowsPerWorkgroup, most), 1);
}

size_t partial_rows(size_t num_rows, size_t tokens, size_t hidden, size_t width) {
  return workgroups(num_rows, std::min(kTokenMixMaxPartialRows,
                                       kTokenMixMaxWorkspaceFloats /
                                           partial_row_floats(tokens, hidden, width)));
}

// the checks both directions share; false = nothing to do
bool check(const std::string& w, size_t num_rows, size_t tokens, size_t hidden, size_t width,
           Geometry* g) {
  const std::string most = std::to_string(kTokenMixMaxTokens);
  GF_REQUIRE(tokens >= 1 && tokens <= kTokenMixMaxTokens, w + ": tokens outside [1, " + most + "]");
  GF_REQUIRE(hidden >= 1 && hidden <= kTokenMixMaxTokens,
             w + ": hidden width outside [1, " + most + "]");
  GF_REQUIRE(width >= 1 && width <= kTokenMixMaxWidth,
             w + ": width outside [1, " + std::to_string(kTokenMixMaxWidth) + "]");
  GF_REQUIRE(num_rows < (size_t{1} << 63) / (width * std::max(tokens, hidden)),
             w + ": 2^63 elements or more");
  if (num_rows == 0) return false;
  *g = {num_rows,
        static_cast<uint32_t>(tokens),
        static_cast<uint32_t>(hidden),
        static_cast<uint32_t>(width),
        static_cast<uint32_t>((tokens + 15) / 16),
        static_cast<uint32_t>((hidden + 15) / 16),
        false};
  return true;
}

template <class Kernel, class... Args>
void launch(Kernel kernel, size_t grid, size_t lds, hipStream_t stream, Args... args) {
  if (lds > kDefaultLdsLimit)
    GF_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                               hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds)));
  kernel<<<dim3(static_cast<unsigned>(grid)), dim3(kThreads), lds, stream>>>(args...);
  GF_HIP(hipGetLastError());
}

// bytes of LDS: `token_tiles` tiles of 16 KB rows, `hidden_tiles` of 16 JB rows, `vectors` floats
size_t lds_bytes(const Geometry& g, size_t token_tiles, size_t hidden_tiles, size_t vectors) {
  return ((token_tiles * g.KB + hidden_tiles * g.JB) * 16 * kStride + vectors) * sizeof(float);
}

}  // namespace

void token_mix_forward(const float* d_x, const float* d_gamma, const float* d_beta,
                       const float* d_w1, const float* d_b1, const float* d_w2, const float* d_b2,
                       size_t num_rows, size_t tokens, size_t hidden, size_t width, float eps,
                       float p, uint64_t seed, float* d_y, float* d_mean, float* d_rstd, int device,
                       hipStream_t stream) {
  const std::string w("token_mix");
  Geometry g;
  const Dropout dr = checked_dropout(p, seed);
  GF_REQUIRE(eps > 0.f && eps < 1e30f, w + ": eps must be positive and finite");     // NaN fails
  if (!check(w, num_rows, tokens, hidden, width, &g)) return;
  GF_REQUIRE(d_x && d_gamma && d_beta && d_w1 && d_b1 && d_w2 && d_b2 && d_y && d_mean && d_rstd,
             w + ": null x, parameter, y, mean or rstd");
  g.vec = width % 4 == 0 && aligned16(d_x);
  DeviceGuard dg(device);
  const size_t grid = workgroups(num_rows, kForwardMaxWorkgroups);
  const size_t lds = lds_bytes(g, 2, 2, 4 * kMaxTokens + 2 * kMaxWidth);
  if (p > 0.f)
    launch(token_mix_fwd<true>, grid, lds, stream, g, dr, eps, d_x, d_gamma, d_beta, d_w1, d_b1,
           d_w2, d_b2, d_y, d_mean, d_rstd);
  else
    launch(token_mix_fwd<false>, grid, lds, stream, g, dr, eps, d_x, d_gamma, d_beta, d_w1, d_b1,
           d_w2, d_b2, d_y, d_mean, d_rstd);
}

size_t token_mix_backward_partial_rows(size_t num_rows, size_t tokens, size_t hidden,
                                       size_t width) {
  Geometry g;
  check("token_mix backward", num_rows, tokens, hidden, width, &g);
  return partial_rows(num_rows, tokens, hidden, width);
}

void token_mix_backward(const float* d_x, const float* d_gamma, const float* d_beta,
                        const float* d_w1, const float* d_b1, const float* d_w2,
                        const float* d_mean, const float* d_rstd, size_t num_rows, size_t tokens,
                        size_t hidden, size_t width, float p, uint64_t seed,
                        const float* d_grad_y, float* d_partials, size_t partial_rows_given,
                        float* d_grad_x, float* d_grad_gamma, float* d_grad_beta,
                        float* d_grad_w1, float* d_grad_b1, float* d_grad_w2, float* d_grad_b2,
                        int device, hipStream_t stream) {
  const std::string w("token_mix backward");
  Geometry g;
  const Dropout dr = checked_dropout(p, seed);
  if (!check(w, num_rows, tokens, hidden, width, &g)) return;
  const bool params = d_grad_gamma || d_grad_beta || d_grad_w1 || d_grad_b1 || d_grad_w2 ||
                      d_grad_b2;
  if (!d_grad_x && !params) return;
  GF_REQUIRE(d_x && d_gamma && d_beta && d_w1 && d_b1 && d_w2 && d_mean && d_rstd && d_grad_y,
             w + ": null x, parameter, mean, rstd or gradient");
  const size_t rows = partial_rows(num_rows, tokens, hidden, width);
  GF_REQUIRE(!params || (d_partials != nullptr && partial_rows_given >= rows),
             w + ": partials buffer missing or smaller than "
                 "gf_token_mix_backward_partial_rows() asks for");
  g.vec = width % 4 == 0 && aligned16(d_x) && aligned16(d_grad_y);
  DeviceGuard dg(device);
  const size_t lds = lds_bytes(g, 3, 4, 11 * kMaxTokens + 4 * kMaxWidth);
  const bool drop = p > 0.f;
  auto run = [&](auto kernel) {
    launch(kernel, rows, lds, stream, g, dr, d_x, d_gamma, d_beta, d_w1, d_b1, d_w2, d_mean,
           d_rstd, d_grad_y, params, d_partials, d_grad_x);
  };
  drop ? run(token_mix_bwd<true>) : run(token_mix_bwd<false>);
  if (!params) return;
  const size_t total = partial_row_floats(tokens, hidden, width);
  token_mix_bwd_finish<<<dim3(static_cast<unsigned>((total + kFinishThreads - 1) / kFinishThreads)),
                         dim3(kFinishThreads), 0, stream>>>(
      d_partials, static_cast<uint32_t>(rows), g.K, g.Kh, g.C, d_grad_w1, d_grad_w2, d_grad_b1,
      d_grad_b2, d_grad_gamma, d_grad_beta);
  GF_HIP(hipGetLastError());
}

}  // namespace gf
