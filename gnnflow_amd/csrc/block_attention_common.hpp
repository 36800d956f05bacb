// What the kernels of block_attention.hip and block_gat.hip share, whatever their element type:
// the lane-group helpers, head_dot() -- the only place a dot over a head's columns is computed
// --, the dropout mask (layer_epilogue.hip draws it from here too) and the G / NC dispatch; and
// block_attention's own argument checks.  Everything sits in an unnamed namespace: each
// translation unit gets its own copy, and the kernels compile to the code they had when these
// lines were part of their files.
#pragma once

#include "bf16.hpp"
#include "block_ops.hpp"
#include "common.hpp"
#include "../../include/gnnflow_rng.h"

#include <cfloat>
#include <cstdint>

namespace gf {
namespace {

constexpr int kThreads = 256;
constexpr int kMaxChunks = 16;   // columns per lane of a 64-lane group: D <= 64 * 16

template <int G>
__device__ inline float group_sum(float v) {
#pragma unroll
  for (int off = G / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

template <int G>
__device__ inline float group_max(float v) {
#pragma unroll
  for (int off = G / 2; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
  return v;
}

// value of lane `j` of the caller's group
template <int G>
__device__ inline float group_read(float v, int j) {
  return __shfl(v, ((threadIdx.x & 63) & ~(G - 1)) + j, 64);
}

// sum_c a[c] * row[c] over the head's D columns; a[] holds the lane's columns of the other
// operand (0 past D).  The same value in every lane of the group.
template <int G, int NC, class T>
__device__ inline float head_dot(const float (&a)[NC], const T* __restrict__ row, uint32_t D,
                                 uint32_t lig) {
  float p = 0.f;
#pragma unroll
  for (int j = 0; j < NC; ++j) {
    const uint32_t c = lig + G * j;
    if (c < D) p += a[j] * widen(row[c]);
  }
  return group_sum<G>(p);
}

template <int G, int NC, class T>
__device__ inline void load_head(float (&a)[NC], const T* __restrict__ row, uint32_t D,
                                 uint32_t lig) {
#pragma unroll
  for (int j = 0; j < NC; ++j) {
    const uint32_t c = lig + G * j;
    a[j] = c < D ? widen(row[c]) : 0.f;
  }
}

__device__ inline float leaky(float z, float slope) { return z > 0.f ? z : slope * z; }

// what the dropout kernels need besides the attention's own arguments
struct Dropout {
  uint32_t threshold;   // T: kept <=> philox >= T
  float scale;          // 1 / (1 - p)
  uint64_t seed;
};

__device__ inline bool kept(const Dropout& dr, uint64_t edge, uint32_t H, uint32_t h) {
  return gf_philox4x32_10_first(dr.seed, edge * H + h, 0) >= dr.threshold;
}

struct Shape {
  const int64_t* offsets;
  uint64_t items;
  uint32_t H, D;
};

// calls f.template operator()<G, NC>() for the group size / columns per lane of a D-column head
template <class F>
void dispatch(uint32_t D, F&& f) {
  if (D <= 8) f.template operator()<8, 1>();
  else if (D <= 16) f.template operator()<16, 1>();
  else if (D <= 32) f.template operator()<32, 1>();
  else if (D <= 64) f.template operator()<64, 1>();
  else if (D <= 128) f.template operator()<64, 2>();
  else if (D <= 256) f.template operator()<64, 4>();
  else if (D <= 512) f.template operator()<64, 8>();
  else f.template operator()<64, kMaxChunks>();
}

inline unsigned grid_of(const Shape& s, int G) {
  return static_cast<unsigned>((s.items * G + kThreads - 1) / kThreads);
}

inline Shape checked_shape(const int64_t* d_offsets, size_t num_dst, size_t heads,
                           size_t head_dim) {
  GF_REQUIRE(heads >= 1 && head_dim >= 1, "block_attention: heads and head_dim must be >= 1");
  GF_REQUIRE(heads <= kBlockAttentionMaxWidth && head_dim <= kBlockAttentionMaxWidth &&
                 heads * head_dim <= kBlockAttentionMaxWidth,
             "block_attention: heads * head_dim exceeds GF_BLOCK_ATTENTION_MAX_WIDTH (1024)");
  static_assert(kBlockAttentionMaxWidth <= 64 * kMaxChunks, "a head must fit one group");
  GF_REQUIRE(d_offsets != nullptr, "block_attention: null offsets");
  // one group of up to 64 lanes per (destination, head): the grid stays below 2^31 blocks
  GF_REQUIRE(num_dst <= (size_t{1} << 32) / heads, "block_attention: too many destinations");
  return Shape{d_offsets, static_cast<uint64_t>(num_dst) * heads, static_cast<uint32_t>(heads),
               static_cast<uint32_t>(head_dim)};
}

// T and 1 / (1 - p) of the mask definition (gnnflow_hip.h); p is an fp32 value in [0, 1)
inline Dropout checked_dropout(float p, uint64_t seed) {
  GF_REQUIRE(p >= 0.f && p < 1.f, "block_attention: dropout p must be in [0, 1)");   // NaN fails
  return Dropout{static_cast<uint32_t>(static_cast<double>(p) * 4294967296.0), 1.0f / (1.0f - p),
                 seed};
}

}  // namespace
}  // namespace gf
