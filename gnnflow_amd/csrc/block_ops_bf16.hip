// The reduction kernels of block_ops.hip -- segment_reduce_fwd / _bwd, segment_max_fwd / _bwd --
// for bfloat16 source rows, outputs and gradients (carried as uint16_t): the tensors autocast
// hands dgl.nn.SAGEConv / GATConv.  One rule, the one of block_attention_bf16.hip: every bfloat16
// element is widened to float32 where it is loaded (exact), the arithmetic is the float32
// kernel's own -- the same lane-to-column map (lane, lane + 64, ...), the same loop over the
// edges of a segment, the same wave_sum -- and a bfloat16 result is rounded once, to nearest
// even, where it is stored.  Edge weights and their gradient stay float32: they are the softmax
// output, [E, heads] only.  The library is built with -ffp-contract=off and without fast-math, so
//
//   bf16 kernel(x)  ==  round_to_bf16(float32 kernel(widen(x)))      bit for bit.
//
// Gradient of the source rows.  With an explicit col a source may feed several edges and the
// float32 kernels add with atomicAdd.  A bfloat16 atomic add would round once per edge (and
// does not exist): the adds go to a caller-owned float32 scratch [num_src, dim] instead, the
// float32 kernel's own adds into the float32 kernel's own zeros, and narrow_rows rounds the
// scratch to the bfloat16 gradient in one small launch.  The sampler's layout (col null) stores
// each element once, directly in bfloat16, and needs neither scratch nor atomics.
//
// Loads are one 2-byte access per column: a lane owns the columns lane + 64 * j as in the float32
// kernels, which fixes the order of wave_sum's terms; a wave's loads are one contiguous run.
#include "bf16.hpp"
#include "block_ops.hpp"
#include "common.hpp"

#include <algorithm>
#include <cstdint>

namespace gf {
namespace {

using bf16 = uint16_t;

constexpr int kThreads = 256;
constexpr unsigned kMaxNarrowBlocks = 1u << 20;

__device__ inline float wave_sum(float v) {
  for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}

__global__ void segment_reduce_fwd_bf16(const int64_t* __restrict__ offsets, uint64_t num_dst,
                                        const int64_t* __restrict__ col,
                                        const bf16* __restrict__ src, uint32_t dim,
                                        const float* __restrict__ w, uint32_t heads, int mean,
                                        bf16* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const uint64_t d = (static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x) >> 6;
  if (d >= num_dst) return;
  const int64_t b = offsets[d], e = offsets[d + 1];
  const uint32_t per_head = w ? dim / heads : dim;
  const float scale = (mean && e > b) ? 1.f / static_cast<float>(e - b) : 1.f;
  for (uint32_t c = lane; c < dim; c += 64) {
    const uint32_t h = w ? c / per_head : 0u;
    float acc = 0.f;
    for (int64_t k = b; k < e; ++k) {
      const uint64_t s = col ? static_cast<uint64_t>(col[k]) : num_dst + static_cast<uint64_t>(k);
      const float v = widen(src[s * dim + c]);
      acc += w ? v * w[k * heads + h] : v;
    }
    out[d * dim + c] = narrow(acc * scale);
  }
}

// gsrc32 (col != null): the float32 scratch, zeroed, accumulated with atomicAdd.
// gsrc16 (col == null): the bfloat16 gradient itself, every edge's row stored once.
__global__ void segment_reduce_bwd_bf16(const int64_t* __restrict__ offsets, uint64_t num_dst,
                                        const int64_t* __restrict__ col,
                                        const bf16* __restrict__ src, uint32_t dim,
                                        const float* __restrict__ w, uint32_t heads, int mean,
                                        const bf16* __restrict__ gout, float* __restrict__ gsrc32,
                                        bf16* __restrict__ gsrc16, float* __restrict__ gw) {
  const int lane = threadIdx.x & 63;
  const uint64_t d = (static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x) >> 6;
  if (d >= num_dst) return;
  const int64_t b = offsets[d], e = offsets[d + 1];
  const uint32_t per_head = w ? dim / heads : dim;
  const float scale = (mean && e > b) ? 1.f / static_cast<float>(e - b) : 1.f;
  for (int64_t k = b; k < e; ++k) {
    const uint64_t s = col ? static_cast<uint64_t>(col[k]) : num_dst + static_cast<uint64_t>(k);
    if (gsrc32 || gsrc16) {
      for (uint32_t c = lane; c < dim; c += 64) {
        const float g = widen(gout[d * dim + c]) * scale;
        const float v = w ? g * w[k * heads + c / per_head] : g;
        if (col) atomicAdd(&gsrc32[s * dim + c], v);
        else gsrc16[s * dim + c] = narrow(v);   // every source row feeds exactly one edge
      }
    }
    if (gw) {
      for (uint32_t h = 0; h < heads; ++h) {
        float acc = 0.f;
        for (uint32_t c = h * per_head + lane; c < (h + 1) * per_head; c += 64)
          acc += widen(gout[d * dim + c]) * widen(src[s * dim + c]);
        acc = wave_sum(acc);
        if (lane == 0) gw[k * heads + h] = acc * scale;
      }
    }
  }
}

// best is an input element widened, so narrow() gives it back exactly; +0 without in-edges
__global__ void segment_max_fwd_bf16(const int64_t* __restrict__ offsets, uint64_t num_dst,
                                     const int64_t* __restrict__ col,
                                     const bf16* __restrict__ src, uint32_t dim,
                                     bf16* __restrict__ out, int64_t* __restrict__ arg) {
  const int lane = threadIdx.x & 63;
  const uint64_t d = (static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x) >> 6;
  if (d >= num_dst) return;
  const int64_t b = offsets[d], e = offsets[d + 1];
  for (uint32_t c = lane; c < dim; c += 64) {
    float best = 0.f;
    int64_t who = -1;
    for (int64_t k = b; k < e; ++k) {
      const uint64_t s = col ? static_cast<uint64_t>(col[k]) : num_dst + static_cast<uint64_t>(k);
      const float v = widen(src[s * dim + c]);
      if (who < 0 || v > best) { best = v; who = k; }
    }
    out[d * dim + c] = narrow(best);
    arg[d * dim + c] = who;
  }
}

// col != null: two destinations may pick one source, atomicAdd into the zeroed float32 scratch.
// col == null: source num_dst + k belongs to edge k alone, so (row, column) is the argmax of at
// most one destination and is stored directly: 0 + g, the float32 kernel's one add into its
// zero (which turns a -0 gradient into +0), rounded.
__global__ void segment_max_bwd_bf16(uint64_t num_dst, const int64_t* __restrict__ col,
                                     uint32_t dim, const bf16* __restrict__ gout,
                                     const int64_t* __restrict__ arg, float* __restrict__ gsrc32,
                                     bf16* __restrict__ gsrc16) {
  const uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= num_dst * dim) return;
  const int64_t k = arg[i];
  if (k < 0) return;
  const float g = widen(gout[i]);
  if (col) atomicAdd(&gsrc32[static_cast<uint64_t>(col[k]) * dim + (i % dim)], g);
  else gsrc16[(num_dst + static_cast<uint64_t>(k)) * dim + (i % dim)] = narrow(0.f + g);
}

__global__ void narrow_rows_kernel(const float* __restrict__ in, bf16* __restrict__ out,
                                   uint64_t n) {
  const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n;
       i += stride)
    out[i] = narrow(in[i]);
}

inline unsigned blocks_for(uint64_t threads) {
  return static_cast<unsigned>((threads + kThreads - 1) / kThreads);
}

}  // namespace

void narrow_rows(const float* d_in, uint16_t* d_out, size_t n, hipStream_t stream) {
  if (n == 0) return;
  GF_REQUIRE(d_in && d_out, "narrow_rows: null pointer");
  const uint64_t blocks = (static_cast<uint64_t>(n) + kThreads - 1) / kThreads;
  narrow_rows_kernel<<<dim3(static_cast<unsigned>(std::min<uint64_t>(blocks, kMaxNarrowBlocks))),
                       dim3(kThreads), 0, stream>>>(d_in, d_out, n);
  GF_HIP(hipGetLastError());
}

void segment_reduce_bf16_forward(const int64_t* d_offsets, size_t num_dst, const int64_t* d_col,
                                 const uint16_t* d_src, size_t dim, const float* d_w,
                                 size_t heads, bool mean, uint16_t* d_out, int device,
                                 hipStream_t stream) {
  if (num_dst == 0 || dim == 0) return;
  GF_REQUIRE(d_offsets && d_out, "segment_reduce: null pointer");
  GF_REQUIRE(!d_w || (heads > 0 && dim % heads == 0), "segment_reduce: dim must be a multiple of heads");
  DeviceGuard dg(device);
  segment_reduce_fwd_bf16<<<dim3(blocks_for(static_cast<uint64_t>(num_dst) * 64)), dim3(kThreads),
                            0, stream>>>(d_offsets, num_dst, d_col, d_src,
                                         static_cast<uint32_t>(dim), d_w,
                                         static_cast<uint32_t>(heads ? heads : 1), mean ? 1 : 0,
                                         d_out);
  GF_HIP(hipGetLastError());
}

void segment_reduce_bf16_backward(const int64_t* d_offsets, size_t num_dst, const int64_t* d_col,
                                  const uint16_t* d_src, size_t dim, const float* d_w,
                                  size_t heads, bool mean, const uint16_t* d_grad_out,
                                  uint16_t* d_grad_src, size_t num_src, float* d_grad_w,
                                  float* d_scratch, int device, hipStream_t stream) {
  DeviceGuard dg(device);
  const bool wanted = d_grad_src && num_src && dim;
  const bool via_scratch = wanted && d_col;
  GF_REQUIRE(!via_scratch || d_scratch, "segment_reduce backward: col needs the float32 scratch");
  if (via_scratch) {
    GF_HIP(hipMemsetAsync(d_scratch, 0, num_src * dim * sizeof(float), stream));
  } else if (wanted) {
    // the sampler layout writes every edge's row exactly once, so only the rows of the
    // destination nodes themselves are cleared
    const size_t rows = std::min(num_dst, num_src);
    if (rows) GF_HIP(hipMemsetAsync(d_grad_src, 0, rows * dim * sizeof(uint16_t), stream));
  }
  if (num_dst == 0 || dim == 0) {
    if (via_scratch) narrow_rows(d_scratch, d_grad_src, num_src * dim, stream);
    return;
  }
  GF_REQUIRE(d_offsets && d_grad_out, "segment_reduce backward: null pointer");
  GF_REQUIRE(!d_grad_w || (d_w && d_src), "segment_reduce backward: weight gradient needs w and src");
  GF_REQUIRE(!d_w || (heads > 0 && dim % heads == 0), "segment_reduce: dim must be a multiple of heads");
  segment_reduce_bwd_bf16<<<dim3(blocks_for(static_cast<uint64_t>(num_dst) * 64)), dim3(kThreads),
                            0, stream>>>(d_offsets, num_dst, d_col, d_src,
                                         static_cast<uint32_t>(dim), d_w,
                                         static_cast<uint32_t>(heads ? heads : 1), mean ? 1 : 0,
                                         d_grad_out, via_scratch ? d_scratch : nullptr,
                                         wanted && !d_col ? d_grad_src : nullptr, d_grad_w);
  GF_HIP(hipGetLastError());
  if (via_scratch) narrow_rows(d_scratch, d_grad_src, num_src * dim, stream);
}

void segment_max_bf16_forward(const int64_t* d_offsets, size_t num_dst, const int64_t* d_col,
                              const uint16_t* d_src, size_t dim, uint16_t* d_out, int64_t* d_arg,
                              int device, hipStream_t stream) {
  if (num_dst == 0 || dim == 0) return;
  GF_REQUIRE(d_offsets && d_src && d_out && d_arg, "segment_max: null pointer");
  DeviceGuard dg(device);
  segment_max_fwd_bf16<<<dim3(blocks_for(static_cast<uint64_t>(num_dst) * 64)), dim3(kThreads), 0,
                         stream>>>(d_offsets, num_dst, d_col, d_src, static_cast<uint32_t>(dim),
                                   d_out, d_arg);
  GF_HIP(hipGetLastError());
}

void segment_max_bf16_backward(size_t num_dst, const int64_t* d_col, size_t dim,
                               const uint16_t* d_grad_out, const int64_t* d_arg,
                               uint16_t* d_grad_src, size_t num_src, float* d_scratch, int device,
                               hipStream_t stream) {
  GF_REQUIRE(d_grad_src != nullptr || num_src == 0, "segment_max backward: null gradient");
  DeviceGuard dg(device);
  const bool via_scratch = d_col && num_src && dim;
  GF_REQUIRE(!via_scratch || d_scratch, "segment_max backward: col needs the float32 scratch");
  if (via_scratch) GF_HIP(hipMemsetAsync(d_scratch, 0, num_src * dim * sizeof(float), stream));
  else if (num_src && dim)
    GF_HIP(hipMemsetAsync(d_grad_src, 0, num_src * dim * sizeof(uint16_t), stream));
  if (num_dst == 0 || dim == 0) {
    if (via_scratch) narrow_rows(d_scratch, d_grad_src, num_src * dim, stream);
    return;
  }
  GF_REQUIRE(d_grad_out && d_arg, "segment_max backward: null pointer");
  segment_max_bwd_bf16<<<dim3(blocks_for(static_cast<uint64_t>(num_dst) * dim)), dim3(kThreads), 0,
                         stream>>>(num_dst, d_col, static_cast<uint32_t>(dim), d_grad_out, d_arg,
                                   via_scratch ? d_scratch : nullptr,
                                   via_scratch ? nullptr : d_grad_src);
  GF_HIP(hipGetLastError());
  if (via_scratch) narrow_rows(d_scratch, d_grad_src, num_src * dim, stream);
}

}  // namespace gf
