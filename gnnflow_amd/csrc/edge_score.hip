// Fused tail of the reference's EdgePredictor (gnnflow/models/modules/layers.py:171-197): after
// src_fc and dst_fc, the two adds, two relus and two out_fc GEMVs, as ONE launch forward and at
// most two launches backward.  fp32 throughout.
//
//   out[j]    = bias + sum_d w[d] * max(src[j mod B, d] + dst[j, d], 0)        j < M = r * B
//
// Row j of dst pairs with row j mod B of src: r = 2 is the reference's positive and negative
// half, r > 2 several negatives per positive, block after block.
//
// Forward.  16 lanes per row, 16 rows per workgroup.  Lane l owns the columns 4c .. 4c + 3 of
// the chunks c = l, l + 16, ... and sums its terms in ascending column order; the 16 lanes are
// combined by a fixed xor butterfly (8, 4, 2, 1) and bias is added last.  The chunks are loaded
// as one 16-byte access when D % 4 == 0 and src, dst and w are 16-byte aligned, element by
// element otherwise -- the same columns on the same lane either way, so the order of summation
// depends on D alone: not on M, not on the grid and not on the alignment.
//
// Backward, with g = grad_out[:, 0] and m[j,d] = (src[j mod B,d] + dst[j,d] > 0):
//
//   gdst[j,d] = m[j,d] ? g[j] * w[d] : 0                       one multiply
//   gsrc[i,d] = gdst[i,d] + gdst[i+B,d] + ... + gdst[i+(r-1)B,d]   ascending block order
//   gw[d]     = sum_j g[j] * max(src[j mod B,d] + dst[j,d], 0)
//   gbias     = sum_j g[j]
//
// Workgroup p owns the src rows [p * rows_per_wg, (p + 1) * rows_per_wg) together with all r of
// their dst rows, so gsrc and gdst are finished where they are computed.  Lanes sit over the
// D + 1 columns (column D is gbias; CX of them, RY = 256 / CX row phases), each lane accumulates
// its rows in registers in ascending order, the RY phases are summed in ascending order through
// LDS, and the workgroup writes one row [D + 1] of partials.  A second launch sums the at most
// kEdgeScoreMaxPartialRows partial rows as time_encode.hip does: 32 phases of ascending rows,
// then the phases in ascending order.  No atomics anywhere: every result is a fixed expression
// of the inputs and bit-reproducible.  Without gw and gbias there are no partials and no second
// launch.
//
// bfloat16 (T = uint16_t; bf16.hpp): src and dst rows, and their gradients, may be bfloat16
// while w, bias, g, out, gw and gbias stay float32.  Each element is widened (exact) when it is
// loaded, one kernel body does the arithmetic for both types, and gsrc and gdst are rounded
// once, to nearest even, when they are stored; the partials and the finish kernel know no T.
// The forward's 4-column chunk of a bfloat16 row is one 8-byte access when D % 4 == 0, src and
// dst are 8-byte aligned and w is 16-byte aligned.
#include "bf16.hpp"
#include "block_ops.hpp"
#include "common.hpp"

#include <cstdint>

namespace gf {
namespace {

constexpr int kThreads = 256;
constexpr int kLanes = 16;                          // lanes per row of the forward
constexpr int kRowsPerBlock = kThreads / kLanes;
constexpr int kFinishThreads = 1024;                // 32 columns x 32 row phases
constexpr size_t kMinRowsPerGroup = 8;

// the only place the pre-activation is computed, forward and backward: one add
__device__ __forceinline__ float es_pre(float s, float p) { return s + p; }
__device__ __forceinline__ float es_relu(float x) { return x > 0.f ? x : 0.f; }

// Columns c .. c + 3 of a row in one access, 16 bytes of float32 or 8 bytes of bfloat16, and
// column I of what was loaded.  A bfloat16 column is widened where it is used, not where it is
// loaded: the compiler schedules the two differently.
__device__ __forceinline__ float4 load4(const float* p) {
  return *reinterpret_cast<const float4*>(p);
}
__device__ __forceinline__ uint2 load4(const uint16_t* p) {
  return *reinterpret_cast<const uint2*>(p);
}
template <int I>
__device__ __forceinline__ float col(const float4& v) {
  return I == 0 ? v.x : I == 1 ? v.y : I == 2 ? v.z : v.w;
}
template <int I>
__device__ __forceinline__ float col(const uint2& u) {
  const uint32_t pair = I < 2 ? u.x : u.y;
  return __uint_as_float(I % 2 ? pair & 0xffff0000u : pair << 16);
}

template <class T, bool VEC>
__global__ void __launch_bounds__(kThreads)
edge_score_fwd(const T* __restrict__ src, const T* __restrict__ dst,
               const float* __restrict__ w, const float* __restrict__ bias, uint32_t B, uint32_t M,
               uint32_t D, float* __restrict__ out) {
  const uint32_t lane = threadIdx.x % kLanes;
  const uint32_t j = blockIdx.x * static_cast<uint32_t>(kRowsPerBlock) + threadIdx.x / kLanes;
  float acc = 0.f;
  if (j < M) {
    const T* s = src + static_cast<uint64_t>(j % B) * D;
    const T* p = dst + static_cast<uint64_t>(j) * D;
    for (uint32_t c = lane * 4; c < D; c += kLanes * 4) {
      if (VEC) {
        const auto sv = load4(s + c), pv = load4(p + c);
        const float4 wv = load4(w + c);
        acc += wv.x * es_relu(es_pre(col<0>(sv), col<0>(pv)));
        acc += wv.y * es_relu(es_pre(col<1>(sv), col<1>(pv)));
        acc += wv.z * es_relu(es_pre(col<2>(sv), col<2>(pv)));
        acc += wv.w * es_relu(es_pre(col<3>(sv), col<3>(pv)));
      } else {
        const uint32_t end = c + 4 < D ? c + 4 : D;
        for (uint32_t d = c; d < end; ++d)
          acc += w[d] * es_relu(es_pre(widen(s[d]), widen(p[d])));
      }
    }
  }
  // every lane of the wave takes part; rows past M carry zeros
#pragma unroll
  for (int off = kLanes / 2; off >= 1; off >>= 1) acc += __shfl_xor(acc, off, kLanes);
  if (j < M && lane == 0) out[j] = acc + bias[0];
}

// partials[p, c]: c < D -> gw[c]'s share of workgroup p's rows, c == D -> gbias's.  A null gsrc,
// gdst or partials is skipped (uniform over the grid).
template <class T, int CX>
__global__ void __launch_bounds__(kThreads)
edge_score_bwd(const T* __restrict__ src, const T* __restrict__ dst,
               const float* __restrict__ w, const float* __restrict__ g, uint32_t B, uint32_t r,
               uint32_t D, uint32_t rows_per_wg, T* __restrict__ gsrc, T* __restrict__ gdst,
               float* __restrict__ partials) {
  constexpr int RY = kThreads / CX;
  __shared__ float sp[RY][CX];
  const uint32_t cx = threadIdx.x % CX, ry = threadIdx.x / CX;
  const uint32_t i0 = blockIdx.x * rows_per_wg;
  const uint32_t i1 = B - i0 < rows_per_wg ? B : i0 + rows_per_wg;      // i0 < B
  const uint32_t width = D + 1;
  for (uint32_t c0 = 0; c0 < width; c0 += CX) {      // uniform over the workgroup
    const uint32_t c = c0 + cx;
    float acc = 0.f;
    if (c < D) {
      const float wc = w[c];
      for (uint32_t i = i0 + ry; i < i1; i += RY) {
        const float s = widen(src[static_cast<uint64_t>(i) * D + c]);
        float gs = 0.f;
        for (uint32_t k = 0; k < r; ++k) {
          const uint64_t j = i + static_cast<uint64_t>(k) * B;      // < r * B
          const float gj = g[j];
          const float x = es_pre(s, widen(dst[j * D + c]));
          const float gd = x > 0.f ? gj * wc : 0.f;
          if (gdst) gdst[j * D + c] = narrow_to<T>(gd);
          gs += gd;
          acc += gj * es_relu(x);
        }
        if (gsrc) gsrc[static_cast<uint64_t>(i) * D + c] = narrow_to<T>(gs);
      }
    } else if (c == D && partials) {
      for (uint32_t i = i0 + ry; i < i1; i += RY)
        for (uint32_t k = 0; k < r; ++k) acc += g[i + static_cast<uint64_t>(k) * B];
    }
    if (partials) {
      sp[ry][cx] = acc;
      __syncthreads();
      if (ry == 0 && c < width) {
        float t = sp[0][cx];
#pragma unroll
        for (int q = 1; q < RY; ++q) t += sp[q][cx];
        partials[static_cast<uint64_t>(blockIdx.x) * width + c] = t;
      }
      __syncthreads();
    }
  }
}

// column c of the [rows, D + 1] partials: c < D -> gw[c], c == D -> gbias
__global__ void __launch_bounds__(kFinishThreads)
edge_score_bwd_finish(const float* __restrict__ partials, uint32_t rows, uint32_t D,
                      float* __restrict__ gw, float* __restrict__ gbias) {
  __shared__ float s[32][32];
  const uint32_t cx = threadIdx.x & 31, ph = threadIdx.x >> 5;
  const uint32_t c = blockIdx.x * 32 + cx, width = D + 1;
  float acc = 0.f;
  if (c < width)
    for (uint32_t p = ph; p < rows; p += 32) acc += partials[static_cast<uint64_t>(p) * width + c];
  s[ph][cx] = acc;
  __syncthreads();
  if (ph != 0 || c >= width) return;
  float total = s[0][cx];
#pragma unroll
  for (int q = 1; q < 32; ++q) total += s[q][cx];
  if (c < D) {
    if (gw) gw[c] = total;
  } else if (gbias) {
    gbias[0] = total;
  }
}

// can four elements at p be one access?  16-byte aligned float32, 8-byte aligned bfloat16
template <class T>
bool aligned4(const T* p) { return (reinterpret_cast<uintptr_t>(p) & (4 * sizeof(T) - 1)) == 0; }

size_t partial_rows(size_t num_src) {
  const size_t groups = (num_src + kMinRowsPerGroup - 1) / kMinRowsPerGroup;
  return groups < kEdgeScoreMaxPartialRows ? groups : kEdgeScoreMaxPartialRows;
}

// the checks both directions share; false = nothing to do
bool check_shape(const char* what, size_t num_src, size_t num_dst, size_t dim) {
  GF_REQUIRE(dim >= 1, std::string(what) + ": dim must be >= 1");
  GF_REQUIRE(dim < (size_t{1} << 30), std::string(what) + ": dim too large");
  if (num_dst == 0) return false;
  GF_REQUIRE(num_src >= 1 && num_dst % num_src == 0,
             std::string(what) + ": the dst rows must be a whole number of blocks of the src rows");
  GF_REQUIRE(num_dst < (size_t{1} << 31), std::string(what) + ": more than 2^31 - 1 dst rows");
  return true;
}

template <class T>
void forward(const T* d_src, const T* d_dst, const float* d_w, const float* d_bias, size_t num_src,
             size_t num_dst, size_t dim, float* d_out, int device, hipStream_t stream) {
  if (!check_shape("edge_score", num_src, num_dst, dim)) return;
  GF_REQUIRE(d_src && d_dst && d_w && d_bias && d_out,
             "edge_score: null src, dst, weight, bias or out");
  const bool vec = dim % 4 == 0 && aligned4(d_src) && aligned4(d_dst) && aligned4(d_w);
  const uint32_t B = static_cast<uint32_t>(num_src), M = static_cast<uint32_t>(num_dst),
                 D = static_cast<uint32_t>(dim);
  const dim3 grid((M + kRowsPerBlock - 1) / kRowsPerBlock), block(kThreads);
  DeviceGuard dg(device);
  if (vec)
    edge_score_fwd<T, true><<<grid, block, 0, stream>>>(d_src, d_dst, d_w, d_bias, B, M, D, d_out);
  else
    edge_score_fwd<T, false><<<grid, block, 0, stream>>>(d_src, d_dst, d_w, d_bias, B, M, D, d_out);
  GF_HIP(hipGetLastError());
}

template <class T>
void backward(const T* d_src, const T* d_dst, const float* d_w, size_t num_src, size_t num_dst,
              size_t dim, const float* d_grad_out, float* d_partials, size_t partial_rows_given,
              T* d_grad_src, T* d_grad_dst, float* d_grad_w, float* d_grad_bias, int device,
              hipStream_t stream) {
  if (!check_shape("edge_score backward", num_src, num_dst, dim)) return;
  GF_REQUIRE(d_src && d_dst && d_w, "edge_score backward: null src, dst or weight");
  GF_REQUIRE(d_grad_out != nullptr, "edge_score backward: null gradient");
  const bool reduce = d_grad_w || d_grad_bias;
  if (!reduce && !d_grad_src && !d_grad_dst) return;
  const size_t want = partial_rows(num_src);
  GF_REQUIRE(!reduce || (d_partials != nullptr && partial_rows_given >= want),
             "edge_score backward: partials buffer missing or smaller than "
             "gf_edge_score_backward_partial_rows() asks for");
  const uint32_t B = static_cast<uint32_t>(num_src), D = static_cast<uint32_t>(dim);
  const uint32_t r = static_cast<uint32_t>(num_dst / num_src);
  const uint32_t rows_per_wg = static_cast<uint32_t>((num_src + want - 1) / want);
  const uint32_t groups = (B + rows_per_wg - 1) / rows_per_wg;      // <= want
  float* partials = reduce ? d_partials : nullptr;
  DeviceGuard dg(device);
  if (D + 1 <= 32)
    edge_score_bwd<T, 32><<<dim3(groups), dim3(kThreads), 0, stream>>>(
        d_src, d_dst, d_w, d_grad_out, B, r, D, rows_per_wg, d_grad_src, d_grad_dst, partials);
  else
    edge_score_bwd<T, 64><<<dim3(groups), dim3(kThreads), 0, stream>>>(
        d_src, d_dst, d_w, d_grad_out, B, r, D, rows_per_wg, d_grad_src, d_grad_dst, partials);
  GF_HIP(hipGetLastError());
  if (!reduce) return;
  edge_score_bwd_finish<<<dim3((D + 1 + 31) / 32), dim3(kFinishThreads), 0, stream>>>(
      d_partials, groups, D, d_grad_w, d_grad_bias);
  GF_HIP(hipGetLastError());
}

}  // namespace

size_t edge_score_backward_partial_rows(size_t num_src) { return partial_rows(num_src); }

void edge_score_forward(const float* d_src, const float* d_dst, const float* d_w,
                        const float* d_bias, size_t num_src, size_t num_dst, size_t dim,
                        float* d_out, int device, hipStream_t stream) {
  forward(d_src, d_dst, d_w, d_bias, num_src, num_dst, dim, d_out, device, stream);
}

void edge_score_backward(const float* d_src, const float* d_dst, const float* d_w, size_t num_src,
                         size_t num_dst, size_t dim, const float* d_grad_out, float* d_partials,
                         size_t partial_rows_given, float* d_grad_src, float* d_grad_dst,
                         float* d_grad_w, float* d_grad_bias, int device, hipStream_t stream) {
  backward(d_src, d_dst, d_w, num_src, num_dst, dim, d_grad_out, d_partials, partial_rows_given,
           d_grad_src, d_grad_dst, d_grad_w, d_grad_bias, device, stream);
}

void edge_score_bf16_forward(const uint16_t* d_src, const uint16_t* d_dst, const float* d_w,
                             const float* d_bias, size_t num_src, size_t num_dst, size_t dim,
                             float* d_out, int device, hipStream_t stream) {
  forward(d_src, d_dst, d_w, d_bias, num_src, num_dst, dim, d_out, device, stream);
}

void edge_score_bf16_backward(const uint16_t* d_src, const uint16_t* d_dst, const float* d_w,
                              size_t num_src, size_t num_dst, size_t dim, const float* d_grad_out,
                              float* d_partials, size_t partial_rows_given, uint16_t* d_grad_src,
                              uint16_t* d_grad_dst, float* d_grad_w, float* d_grad_bias,
                              int device, hipStream_t stream) {
  backward(d_src, d_dst, d_w, num_src, num_dst, dim, d_grad_out, d_partials, partial_rows_given,
           d_grad_src, d_grad_dst, d_grad_w, d_grad_bias, device, stream);
}

}  // namespace gf
