// Unmasked multi-head self-attention over short float32 sequences, on the float32 matrix cores.
// With r < n rows, h < H heads, i and j < S tokens, c < dh columns, q / k / v the three [H, dh]
// thirds of a qkv row (nn.MultiheadAttention's in_proj layout, read in place) and sc = 1 / sqrt(dh):
//
//   s[r,h,i,j]   = (sum_c q[r,i,h,c] k[r,j,h,c]) sc         a = softmax_j(s)        lse = log sum_j e^s
//   keep         = gf_philox4x32_10_first(seed, ((r H + h) S + i) S + j, 0) >= T    (p > 0)
//   w            = keep ? 1 / (1 - p) : 0                   (p == 0: w = 1, no Philox)
//   out[r,i,h,:] = sum_j (a w)[i,j] v[r,j,h,:]
//   dV = (a w)^T dO     dA = (dO V^T) w     dS = a (dA - sum_j a dA)     dQ = dS K sc     dK = dS^T Q sc
//
// Neither s, a nor the mask reaches memory: the forward leaves out and lse [n, H, S], the backward
// recomputes a = exp(s - lse) and draws the mask again.  All arithmetic is float32; the five
// products run on v_mfma_f32_16x16x4_f32 with patch_project.hip's operand mapping (lane group g
// supplies k = 4 g + s in step s; D[4 g + v][l % 16] in the lane's four accumulator floats).
//
// Work split.  One workgroup of four waves per (row, head): every element of out, lse and dqkv has
// one writer, so nothing is atomic and the bits repeat.  Queries go in tiles of 64, wave w owns
// queries 16 w .. 16 w + 15 of the tile against all keys: S_pad / 16 <= 8 accumulator quads; the
// kernels are instantiated for up to 4 (S <= 64) and up to 8 quads.  S in 65 .. 128 walks two
// query tiles.
//
// LDS.  dh is walked in chunks of 64 columns as patch_project walks K, so a tile is [rows][68]
// whatever dh is (68 / 4 = 17 is odd: the 16 lanes of a ds_read_b128 fall on 16 bank groups; the
// scalar reads of a k-strided operand are at (4 g + s) 68 + i, 64 banks).  X [64][68] holds the
// chunk of the tile's q or dO rows, Y [S_pad][68] the chunk of k or v.
//   forward:   X, Y and the dropped weights P [64][S_pad + 4], written once from the accumulator
//              layout and read as the A operand of P V (a b128 per 16 keys); V's chunk is the
//              k-strided B operand.  (128 + S_pad) 272 B + 256 (S_pad + 4) B: 52.2 KB at S = 64
//              (three workgroups a CU), 86 KB at S = 128.
//   backward:  X, Y and a w and dS TRANSPOSED, PT and DT [S_pad][68] ([j][i]): the accumulator's
//              four floats are four consecutive queries, so a lane stores one b128 per quad, and
//              both are then b128 A operands of dV = PT dO and dK = DT Q (wave w owns columns
//              16 w .. 16 w + 15 of the chunk by all key quads, as patch_project's backward does);
//              dQ = dS K reads DT k-strided.  (64 + 3 S_pad) 272 B: 69.6 KB at S = 64 (two
//              workgroups a CU), 121.9 KB at S = 128 (one).
// The dh and S tails are zeros in LDS, so no product ever meets a float that was not written.  Key
// columns j >= S take s = -inf (the forward) or a = 0 (the backward) and no mask word is drawn.
//
// Staging.  float4 loads when dh % 4 == 0 and qkv and out (dout) are 16-byte aligned, scalar loads
// otherwise; only the loads differ, the tiles and the order of every sum are the same.
//
// Backward registers.  dK and dV of the (row, head) stay in accumulators across the query tiles
// and the dh chunks -- 2 chunks x S_pad / 16 quads each -- and are stored once at the end; dQ of a
// tile's chunk is complete when computed and is stored at once.
//
// A dropped weight is the float 0 in P (PT), multiplied like any other: it adds exactly 0 for a
// finite v (dO), and a non-finite v[j] reaches every query, as it does in torch's dense product.
#include "sequence_attention.hpp"
#include "block_attention_common.hpp"

#include <cmath>
#include <string>

namespace gf {
namespace {

constexpr int kWave = 64;
constexpr int kTileQ = 64;                 // queries of a tile
constexpr int kChunk = 64;                 // columns of dh staged at a time
constexpr int kStride = kChunk + 4;        // floats between the rows of an LDS tile
constexpr int kDhChunks = static_cast<int>(kSeqAttentionMaxHeadDim) / kChunk;
constexpr size_t kDefaultLdsLimit = 64 << 10;      // above it a kernel must be told

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct Geometry {
  uint32_t S, H, dh;
  uint32_t jq;               // key quads, ceil(S / 16)
  uint32_t hd;               // H * dh: an out row, a third of a qkv row
  float scale;               // 1 / sqrt(dh)
};

__device__ __forceinline__ void load_unit(const float* at, float (&v)[4]) {
  const float4 q = *reinterpret_cast<const float4*>(at);
  v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
}
__device__ __forceinline__ void load_unit(const float* at, float (&v)[1]) { v[0] = *at; }
__device__ __forceinline__ void store_unit(float* at, const float (&v)[4]) {
  *reinterpret_cast<float4*>(at) = make_float4(v[0], v[1], v[2], v[3]);
}
__device__ __forceinline__ void store_unit(float* at, const float (&v)[1]) { at[0] = v[0]; }

// tile[row][0 .. 64) = src[row * pitch + c0 ..] for row < valid and columns below dh, zeros for
// the other columns and for valid <= row < fill
template <int V>
__device__ __forceinline__ void stage(const float* __restrict__ src, uint64_t pitch,
                                      uint32_t valid, uint32_t fill, uint32_t c0, uint32_t dh,
                                      float* __restrict__ tile) {
  constexpr int U = kChunk / V, RP = kThreads / U;
  const uint32_t cu = threadIdx.x % U, c = c0 + cu * V;      // V == 4: dh % 4 == 0, c + 3 < dh
#pragma unroll 4
  for (uint32_t row = threadIdx.x / U; row < fill; row += RP) {
    float v[V];
#pragma unroll
    for (int u = 0; u < V; ++u) v[u] = 0.f;
    if (c < dh && row < valid) load_unit(src + row * pitch + c, v);
    store_unit(tile + row * kStride + cu * V, v);
  }
}

#define GF_SEQ_MFMA4(acc, a0, a1, a2, a3, b0, b1, b2, b3)             \
  do {                                                                \
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b0, acc, 0, 0, 0); \
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b1, acc, 0, 0, 0); \
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a2, b2, acc, 0, 0, 0); \
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a3, b3, acc, 0, 0, 0); \
  } while (0)

// acc[qd][m][n] += sum_k a[m][k] b[16 qd + n][k] over `blocks` blocks of 16 k, both operands
// k-contiguous: a_at is the lane's row of a + 4 g, b_at the lane's row of b's quad 0 + 4 g
template <int QT>
__device__ __forceinline__ void product_nt(f32x4 (&acc)[QT], const float* a_at, const float* b_at,
                                           uint32_t quads, uint32_t blocks) {
  for (uint32_t kb = 0; kb < blocks; ++kb) {
    const float4 a = *reinterpret_cast<const float4*>(a_at + kb * 16);
#pragma unroll
    for (int qd = 0; qd < QT; ++qd) {
      if (qd < static_cast<int>(quads)) {                  // uniform
        const float4 b = *reinterpret_cast<const float4*>(b_at + qd * 16 * kStride + kb * 16);
        GF_SEQ_MFMA4(acc[qd], a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w);
      }
    }
  }
}

// acc[qd][m][n] += sum_k at[16 qd + m][k] b[k][n] over `blocks` blocks of 16 k: a_at is the lane's
// row of at's quad 0 + 4 g, b_at is b + 4 g rows + the lane's column
template <int QT>
__device__ __forceinline__ void product_tn(f32x4 (&acc)[QT], const float* a_at, const float* b_at,
                                           uint32_t quads, uint32_t blocks) {
#pragma unroll 1
  for (uint32_t kb = 0; kb < blocks; ++kb) {
    const float* const bp = b_at + kb * 16 * kStride;
    const float b0 = bp[0], b1 = bp[kStride], b2 = bp[2 * kStride], b3 = bp[3 * kStride];
#pragma unroll
    for (int qd = 0; qd < QT; ++qd) {
      if (qd < static_cast<int>(quads)) {                  // uniform
        const float4 a = *reinterpret_cast<const float4*>(a_at + qd * 16 * kStride + kb * 16);
        GF_SEQ_MFMA4(acc[qd], a.x, a.y, a.z, a.w, b0, b1, b2, b3);
      }
    }
  }
}

// o[cq][m][n] += sum_k a[m][k] b[k][16 cq + n] over `blocks` blocks of 16 k.  a is k-contiguous
// with stride a_stride when A_CONTIGUOUS (a_at: the lane's row + 4 g), else k-strided by kStride
// (a_at: a + 4 g rows + the lane's column); b_at is b + 4 g rows + the lane's column.
template <bool A_CONTIGUOUS>
__device__ __forceinline__ void product_nn(f32x4 (&o)[4], const float* a_at, const float* b_at,
                                           uint32_t cquads, uint32_t blocks) {
#pragma unroll 1
  for (uint32_t kb = 0; kb < blocks; ++kb) {
    float a0, a1, a2, a3;
    if (A_CONTIGUOUS) {
      const float4 a = *reinterpret_cast<const float4*>(a_at + kb * 16);
      a0 = a.x, a1 = a.y, a2 = a.z, a3 = a.w;
    } else {
      const float* const ap = a_at + kb * 16 * kStride;
      a0 = ap[0], a1 = ap[kStride], a2 = ap[2 * kStride], a3 = ap[3 * kStride];
    }
    const float* const bp = b_at + kb * 16 * kStride;
#pragma unroll
    for (int cq = 0; cq < 4; ++cq) {
      if (cq < static_cast<int>(cquads)) {                 // uniform
        const float* const bq = bp + cq * 16;
        GF_SEQ_MFMA4(o[cq], a0, a1, a2, a3, bq[0], bq[kStride], bq[2 * kStride], bq[3 * kStride]);
      }
    }
  }
}

#undef GF_SEQ_MFMA4

__device__ __forceinline__ uint32_t blocks_of(uint32_t columns) {      // of 16, in a chunk
  return columns >= kChunk ? kChunk / 16 : (columns + 15) / 16;
}

template <bool DROP>
__device__ __forceinline__ float weight_of(const Dropout& dr, uint64_t row_counter, uint32_t j) {
  if (!DROP) return 1.f;
  return gf_philox4x32_10_first(dr.seed, row_counter + j, 0) >= dr.threshold ? dr.scale : 0.f;
}

template <int QT, int V, bool DROP>
__global__ void __launch_bounds__(kThreads)
sequence_attention_fwd(const Geometry g, const Dropout dr, const float* __restrict__ qkv,
                       float* __restrict__ out, float* __restrict__ lse) {
  extern __shared__ __align__(16) float lds[];
  float* const sx = lds;                                   // [64][kStride]
  float* const sy = sx + kTileQ * kStride;                 // [16 jq][kStride]
  float* const sp = sy + 16 * g.jq * kStride;              // [64][ps]
  const uint32_t ps = 16 * g.jq + 4;
  const uint32_t wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
  const uint32_t i = lane % 16, grp = lane / 16;
  const uint32_t rh = blockIdx.x, r = rh / g.H, h = rh % g.H;
  const uint64_t pitch = 3ull * g.hd;
  const float* const q_at = qkv + static_cast<uint64_t>(r) * g.S * pitch + h * g.dh;
  const float* const k_at = q_at + g.hd;
  const float* const v_at = q_at + 2 * g.hd;
  float* const out_at = out + static_cast<uint64_t>(r) * g.S * g.hd + h * g.dh;

  for (uint32_t q0 = 0; q0 < g.S; q0 += kTileQ) {
    const uint32_t rows = g.S - q0 < kTileQ ? g.S - q0 : kTileQ;
    const bool active = wave * 16 < rows;                  // uniform over the wave
    f32x4 acc[QT];
#pragma unroll
    for (int qd = 0; qd < QT; ++qd) acc[qd] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (uint32_t c0 = 0; c0 < g.dh; c0 += kChunk) {
      __syncthreads();      // the tiles of the last chunk (of the last query tile) are read
      stage<V>(q_at + q0 * pitch, pitch, rows, (rows + 15) / 16 * 16, c0, g.dh, sx);
      stage<V>(k_at, pitch, g.S, 16 * g.jq, c0, g.dh, sy);
      __syncthreads();
      if (active)
        product_nt<QT>(acc, sx + (wave * 16 + i) * kStride + grp * 4, sy + i * kStride + grp * 4,
                       g.jq, blocks_of(g.dh - c0));
    }

    if (active) {
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const uint32_t local = wave * 16 + grp * 4 + v, row = q0 + local;
        float m = -INFINITY;
#pragma unroll
        for (int qd = 0; qd < QT; ++qd) {
          const uint32_t j = qd * 16 + i;
          const float s = j < g.S ? acc[qd][v] * g.scale : -INFINITY;     // qd >= jq: j >= S
          acc[qd][v] = s;
          m = fmaxf(m, s);
        }
        m = group_max<16>(m);                              // finite: column 0 is a key
        float sum = 0.f;
#pragma unroll
        for (int qd = 0; qd < QT; ++qd) {
          const float e = expf(acc[qd][v] - m);            // 0 past S
          acc[qd][v] = e;
          sum += e;
        }
        sum = group_sum<16>(sum);
        const float inv = 1.f / sum;
        if (i == 0 && row < g.S) lse[static_cast<uint64_t>(rh) * g.S + row] = m + logf(sum);
        const uint64_t counter = (static_cast<uint64_t>(rh) * g.S + row) * g.S;
#pragma unroll
        for (int qd = 0; qd < QT; ++qd) {
          const uint32_t j = qd * 16 + i;
          if (qd < static_cast<int>(g.jq)) {
            float a = acc[qd][v] * inv;
            if (DROP) a = j < g.S && row < g.S ? a * weight_of<DROP>(dr, counter, j) : 0.f;
            sp[local * ps + j] = a;
          }
        }
      }
    }

    for (uint32_t c0 = 0; c0 < g.dh; c0 += kChunk) {
      __syncthreads();      // P is written; the last chunk's tile is read
      stage<V>(v_at, pitch, g.S, 16 * g.jq, c0, g.dh, sy);
      __syncthreads();
      if (active) {
        const uint32_t cquads = blocks_of(g.dh - c0);
        f32x4 o[4];
#pragma unroll
        for (int cq = 0; cq < 4; ++cq) o[cq] = f32x4{0.f, 0.f, 0.f, 0.f};
        product_nn<true>(o, sp + (wave * 16 + i) * ps + grp * 4, sy + grp * 4 * kStride + i,
                         cquads, g.jq);
#pragma unroll
        for (int cq = 0; cq < 4; ++cq) {
          const uint32_t c = c0 + cq * 16 + i;
          if (c < g.dh) {
#pragma unroll
            for (int v = 0; v < 4; ++v) {
              const uint32_t row = q0 + wave * 16 + grp * 4 + v;
              if (row < g.S) out_at[static_cast<uint64_t>(row) * g.hd + c] = o[cq][v];
            }
          }
        }
      }
    }
  }
}

template <int QT, int V, bool DROP>
__global__ void __launch_bounds__(kThreads)
sequence_attention_bwd(const Geometry g, const Dropout dr, const float* __restrict__ qkv,
                       const float* __restrict__ lse, const float* __restrict__ gout,
                       float* __restrict__ gqkv) {
  extern __shared__ __align__(16) float lds[];
  float* const sx = lds;                                   // [64][kStride]
  float* const sy = sx + kTileQ * kStride;                 // [16 jq][kStride]
  float* const spt = sy + 16 * g.jq * kStride;             // [16 jq][kStride]: (a w)[i][j] at [j][i]
  float* const sdt = spt + 16 * g.jq * kStride;            // [16 jq][kStride]: dS[i][j] at [j][i]
  const uint32_t wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
  const uint32_t i = lane % 16, grp = lane / 16;
  const uint32_t rh = blockIdx.x, r = rh / g.H, h = rh % g.H;
  const uint64_t pitch = 3ull * g.hd;
  const uint64_t first = static_cast<uint64_t>(r) * g.S * pitch + h * g.dh;
  const float* const q_at = qkv + first;
  const float* const k_at = q_at + g.hd;
  const float* const v_at = q_at + 2 * g.hd;
  const float* const go_at = gout + static_cast<uint64_t>(r) * g.S * g.hd + h * g.dh;
  float* const gq_at = gqkv + first;

  f32x4 dk[kDhChunks][QT], dv[kDhChunks][QT];
#pragma unroll
  for (int ci = 0; ci < kDhChunks; ++ci)
#pragma unroll
    for (int qd = 0; qd < QT; ++qd) dk[ci][qd] = dv[ci][qd] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (uint32_t q0 = 0; q0 < g.S; q0 += kTileQ) {
    const uint32_t rows = g.S - q0 < kTileQ ? g.S - q0 : kTileQ;
    const uint32_t iblocks = (rows + 15) / 16;
    const bool active = wave < iblocks;                    // uniform over the wave
    const float* const a_row = sx + (wave * 16 + i) * kStride + grp * 4;
    const float* const b_row = sy + i * kStride + grp * 4;

    f32x4 acc_s[QT], acc_a[QT];
#pragma unroll
    for (int qd = 0; qd < QT; ++qd) acc_s[qd] = acc_a[qd] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (uint32_t c0 = 0; c0 < g.dh; c0 += kChunk) {       // s = q k^T
      __syncthreads();
      stage<V>(q_at + q0 * pitch, pitch, rows, iblocks * 16, c0, g.dh, sx);
      stage<V>(k_at, pitch, g.S, 16 * g.jq, c0, g.dh, sy);
      __syncthreads();
      if (active) product_nt<QT>(acc_s, a_row, b_row, g.jq, blocks_of(g.dh - c0));
    }
    for (uint32_t c0 = 0; c0 < g.dh; c0 += kChunk) {       // dO v^T
      __syncthreads();
      stage<V>(go_at + static_cast<uint64_t>(q0) * g.hd, g.hd, rows, iblocks * 16, c0, g.dh, sx);
      stage<V>(v_at, pitch, g.S, 16 * g.jq, c0, g.dh, sy);
      __syncthreads();
      if (active) product_nt<QT>(acc_a, a_row, b_row, g.jq, blocks_of(g.dh - c0));
    }


    if (active) {      // a w and dS, transposed: the lane's four floats are four queries
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const uint32_t row = q0 + wave * 16 + grp * 4 + v;
        const bool real = row < g.S;
        const float l = real ? lse[static_cast<uint64_t>(rh) * g.S + row] : 0.f;
        const uint64_t counter = (static_cast<uint64_t>(rh) * g.S + row) * g.S;
        float a[QT];
        float dot = 0.f;
#pragma unroll
        for (int qd = 0; qd < QT; ++qd) {
          const uint32_t j = qd * 16 + i;
          const bool in = real && j < g.S;                 // a padding row or column: all zeros
          a[qd] = in ? expf(acc_s[qd][v] * g.scale - l) : 0.f;
          const float w = in ? weight_of<DROP>(dr, counter, j) : 0.f;
          const float da = acc_a[qd][v] * w;
          dot += a[qd] * da;
          acc_s[qd][v] = a[qd] * w;
          acc_a[qd][v] = da;
        }
        dot = group_sum<16>(dot);
#pragma unroll
        for (int qd = 0; qd < QT; ++qd) acc_a[qd][v] = a[qd] * (acc_a[qd][v] - dot);
      }
#pragma unroll
      for (int qd = 0; qd < QT; ++qd) {
        if (qd < static_cast<int>(g.jq)) {
          const uint32_t at = (qd * 16 + i) * kStride + wave * 16 + grp * 4;
          *reinterpret_cast<f32x4*>(spt + at) = acc_s[qd];
          *reinterpret_cast<f32x4*>(sdt + at) = acc_a[qd];
        }
      }
    }

    const float* const t_row = i * kStride + grp * 4 + spt;          // PT's quad 0; DT is jq quads on
    const uint32_t dt = 16 * g.jq * kStride;
    const float* const x_col = sx + grp * 4 * kStride + wave * 16 + i;
#pragma unroll
    for (int ci = 0; ci < kDhChunks; ++ci) {
      const uint32_t c0 = ci * kChunk;
      if (c0 < g.dh) {                                     // uniform
        const uint32_t cquads = blocks_of(g.dh - c0);
        __syncthreads();      // PT and DT are written; X and Y are read
        stage<V>(go_at + static_cast<uint64_t>(q0) * g.hd, g.hd, rows, iblocks * 16, c0, g.dh, sx);
        __syncthreads();
        if (wave < cquads) product_tn<QT>(dv[ci], t_row, x_col, g.jq, iblocks);
        __syncthreads();
        stage<V>(q_at + q0 * pitch, pitch, rows, iblocks * 16, c0, g.dh, sx);
        stage<V>(k_at, pitch, g.S, 16 * g.jq, c0, g.dh, sy);
        __syncthreads();
        if (wave < cquads) product_tn<QT>(dk[ci], t_row + dt, x_col, g.jq, iblocks);
        if (active) {
          f32x4 o[4];
#pragma unroll
          for (int cq = 0; cq < 4; ++cq) o[cq] = f32x4{0.f, 0.f, 0.f, 0.f};
          product_nn<false>(o, sdt + grp * 4 * kStride + wave * 16 + i,
                            sy + grp * 4 * kStride + i, cquads, g.jq);
#pragma unroll
          for (int cq = 0; cq < 4; ++cq) {
            const uint32_t c = c0 + cq * 16 + i;
            if (c < g.dh) {
#pragma unroll
              for (int v = 0; v < 4; ++v) {
                const uint32_t row = q0 + wave * 16 + grp * 4 + v;
                if (row < g.S) gq_at[row * pitch + c] = o[cq][v] * g.scale;
              }
            }
          }
        }
      }
    }
  }

#pragma unroll
  for (int ci = 0; ci < kDhChunks; ++ci) {
    const uint32_t c = ci * kChunk + wave * 16 + i;
    if (c < g.dh) {
#pragma unroll
      for (int qd = 0; qd < QT; ++qd) {
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          const uint32_t j = qd * 16 + grp * 4 + v;
          if (j < g.S) {
            gq_at[j * pitch + g.hd + c] = dk[ci][qd][v] * g.scale;
            gq_at[j * pitch + 2 * g.hd + c] = dv[ci][qd][v];
          }
        }
      }
    }
  }
}

size_t lds_forward(const Geometry& g) {
  return ((kTileQ + 16 * g.jq) * kStride + kTileQ * (16 * g.jq + 4)) * sizeof(float);
}

size_t lds_backward(const Geometry& g) {
  return (kTileQ + 3 * 16 * g.jq) * kStride * sizeof(float);
}

// the checks both directions share; false = nothing to do
bool check(const std::string& w, size_t num_rows, size_t length, size_t heads, size_t head_dim,
           Geometry* g) {
  GF_REQUIRE(length >= 1 && length <= kSeqAttentionMaxLength,
             w + ": length outside [1, " + std::to_string(kSeqAttentionMaxLength) + "]");
  GF_REQUIRE(head_dim >= 1 && head_dim <= kSeqAttentionMaxHeadDim,
             w + ": head_dim outside [1, " + std::to_string(kSeqAttentionMaxHeadDim) + "]");
  GF_REQUIRE(heads >= 1 && heads <= kSeqAttentionMaxWidth &&
                 heads * head_dim <= kSeqAttentionMaxWidth,
             w + ": heads * head_dim outside [1, " + std::to_string(kSeqAttentionMaxWidth) + "]");
  GF_REQUIRE(num_rows < (size_t{1} << 31) / heads + ((size_t{1} << 31) % heads != 0),
             w + ": 2^31 (row, head) pairs or more");
  if (num_rows == 0) return false;
  const uint32_t dh = static_cast<uint32_t>(head_dim);
  *g = {static_cast<uint32_t>(length), static_cast<uint32_t>(heads), dh,
        static_cast<uint32_t>((length + 15) / 16), static_cast<uint32_t>(heads * head_dim),
        1.0f / sqrtf(static_cast<float>(dh))};
  return true;
}

template <class Kernel, class... Args>
void launch(Kernel kernel, size_t rows_heads, size_t lds, hipStream_t stream, Args... args) {
  if (lds > kDefaultLdsLimit)
    GF_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                               hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds)));
  kernel<<<dim3(static_cast<unsigned>(rows_heads)), dim3(kThreads), lds, stream>>>(args...);
  GF_HIP(hipGetLastError());
}

// calls f.template operator()<QT, V, DROP>() for the instantiation of (key quads, load width,
// dropout)
template <class F>
void dispatch(const Geometry& g, bool v4, bool drop, F&& f) {
  const int pick = (g.jq > 4 ? 4 : 0) + (v4 ? 2 : 0) + (drop ? 1 : 0);
  switch (pick) {
    case 0: return f.template operator()<4, 1, false>();
    case 1: return f.template operator()<4, 1, true>();
    case 2: return f.template operator()<4, 4, false>();
    case 3: return f.template operator()<4, 4, true>();
    case 4: return f.template operator()<8, 1, false>();
    case 5: return f.template operator()<8, 1, true>();
    case 6: return f.template operator()<8, 4, false>();
    default: return f.template operator()<8, 4, true>();
  }
}

struct Forward {
  const Geometry& g;
  const Dropout& dr;
  size_t rows_heads;
  hipStream_t stream;
  const float* d_qkv;
  float* d_out;
  float* d_lse;
  template <int QT, int V, bool DROP>
  void operator()() const {
    launch(sequence_attention_fwd<QT, V, DROP>, rows_heads, lds_forward(g), stream, g, dr, d_qkv,
           d_out, d_lse);
  }
};

struct Backward {
  const Geometry& g;
  const Dropout& dr;
  size_t rows_heads;
  hipStream_t stream;
  const float* d_qkv;
  const float* d_lse;
  const float* d_grad_out;
  float* d_grad_qkv;
  template <int QT, int V, bool DROP>
  void operator()() const {
    launch(sequence_attention_bwd<QT, V, DROP>, rows_heads, lds_backward(g), stream, g, dr, d_qkv,
           d_lse, d_grad_out, d_grad_qkv);
  }
};

}  // namespace

void sequence_attention_forward(const float* d_qkv, size_t num_rows, size_t length, size_t heads,
                                size_t head_dim, float p, uint64_t seed, float* d_out,
                                float* d_lse, int device, hipStream_t stream) {
  const std::string w("sequence_attention");
  Geometry g;
  const Dropout dr = checked_dropout(p, seed);
  if (!check(w, num_rows, length, heads, head_dim, &g)) return;
  GF_REQUIRE(d_qkv && d_out && d_lse, w + ": null qkv, out or lse");
  const bool v4 = head_dim % 4 == 0 && aligned16(d_qkv);      // out is stored by scalars
  DeviceGuard dg(device);
  dispatch(g, v4, p > 0.f, Forward{g, dr, num_rows * heads, stream, d_qkv, d_out, d_lse});
}

void sequence_attention_backward(const float* d_qkv, const float* d_lse, size_t num_rows,
                                 size_t length, size_t heads, size_t head_dim, float p,
                                 uint64_t seed, const float* d_grad_out, float* d_grad_qkv,
                                 int device, hipStream_t stream) {
  const std::string w("sequence_attention backward");
  Geometry g;
  const Dropout dr = checked_dropout(p, seed);
  if (!check(w, num_rows, length, heads, head_dim, &g)) return;
  GF_REQUIRE(d_qkv && d_lse && d_grad_out && d_grad_qkv,
             w + ": null qkv, lse, gradient or grad_qkv");
  const bool v4 = head_dim % 4 == 0 && aligned16(d_qkv) && aligned16(d_grad_out);
  DeviceGuard dg(device);
  dispatch(g, v4, p > 0.f,
           Backward{g, dr, num_rows * heads, stream, d_qkv, d_lse, d_grad_out, d_grad_qkv});
}

}  // namespace gf
