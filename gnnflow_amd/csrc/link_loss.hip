// The loss of a link-prediction step where ops.edge_score left the logits: what the reference
// gets from BCEWithLogitsLoss twice (scripts/offline_edge_prediction.py: criterion(pred_pos, ones)
// + criterion(pred_neg, zeros)), each way in one launch instead of a dozen.
//
// With positives x_i (i < P) and negatives y_j (j < N):
//
//   t(x)  = log1p(exp(-|x|))
//   l_pos = max(-x, 0) + t(x)                 softplus(-x): BCE with logits against label 1
//   l_neg = max( y, 0) + t(y)                 softplus( y): BCE with logits against label 0
//   loss  = (1/P) sum_i l_pos(x_i) + (1/N) sum_j l_neg(y_j)
//   dloss/dx_i = -s(-x_i) / P      dloss/dy_j = s(y_j) / N
//   s(t)  = 1 / (1 + exp(-t)) for t >= 0,  exp(t) / (1 + exp(t)) for t < 0
//
// Forward.  A term is float32 arithmetic on the float32 (or widened bfloat16) logit; the sums are
// float64.  A workgroup of kThreads = kLinkLossTile threads walks tiles of one side, thread t
// adding element t of each tile in ascending tile order, then the 64 lanes of a wave by a
// shuffle tree and the 16 waves in ascending order.  Up to kLinkLossSingleTiles tiles in all, ONE
// workgroup walks both sides and finishes: one launch.  Beyond that, workgroup b of a side's
// rows (at most kLinkLossMaxPartialRows / 2) takes the tiles b, b + rows, ... and writes one
// float64 partial, and a second launch sums the partials in index order, positives first.  The
// finish is the same code either way: loss = float32(sum_pos / P + sum_neg / N), one rounding
// to float32, then the accumulator with plain loads and stores.  No atomics anywhere: the order
// of every sum depends on P and N alone, so the same inputs give the same bits.
//
// A NaN logit makes its term, the sums and the loss NaN; an infinity follows the formulas
// (l_neg(+inf) = inf, l_neg(-inf) = 0).  A loss that is not finite adds 1 to the accumulator's
// nonfinite field and leaves the others alone, the rule of link_metrics.hip.
//
// Backward.  One launch over the P + N logits (only over the side whose gradient is asked for
// when the other pointer is null); the upstream scalar gradient is read from device memory.
// grad = -s(-x) * (g / P) and s(y) * (g / N): the positive side is never written as s(x) - 1,
// which cancels for large x.
//
// bfloat16 (the *_bf16 entry points; bf16.hpp): logits widened on load (exact), the float32
// arithmetic above in the same order, gradients rounded once, to nearest even, on store.  The
// loss is float32 and equals, bit for bit, the float32 kernels' on the widened logits.
#include "bf16.hpp"
#include "block_ops.hpp"
#include "common.hpp"

#include <cmath>
#include <cstdint>

namespace gf {
namespace {

constexpr int kThreads = static_cast<int>(kLinkLossTile);      // one element per thread and tile
constexpr int kWave = 64;
constexpr int kWaves = kThreads / kWave;
constexpr int kBwdThreads = 256;
constexpr int kFinishThreads = 256;
constexpr uint32_t kMaxSideRows = static_cast<uint32_t>(kLinkLossMaxPartialRows / 2);
static_assert(kThreads % kWave == 0 && kThreads <= 1024, "a tile is one workgroup of whole waves");
static_assert(kLinkLossMaxPartialRows <= kFinishThreads, "the finish stages a row per thread");

template <bool NEG>
__device__ __forceinline__ float loss_term(float x) {
  const float t = log1pf(expf(-fabsf(x)));      // NaN stays NaN
  const float m = NEG ? fmaxf(x, 0.f) : fmaxf(-x, 0.f);
  return m + t;
}

__device__ __forceinline__ float sigmoid(float t) {
  if (t >= 0.f) return 1.f / (1.f + expf(-t));
  const float e = expf(t);      // t < 0 or NaN
  return e / (1.f + e);
}

__device__ __forceinline__ void put(float* p, float v) { *p = v; }
__device__ __forceinline__ void put(uint16_t* p, float v) { *p = narrow(v); }

// The float64 sum of the terms of the tiles first, first + stride, ... of x[n]; the total is
// returned to thread 0 (other threads get a partial sum).  s_wave: kWaves doubles of LDS, free
// again when the call returns.  Every thread of the workgroup calls it.
template <typename T, bool NEG>
__device__ double side_sum(const T* __restrict__ x, uint32_t n, uint32_t first, uint32_t stride,
                           double* s_wave) {
  double acc = 0.0;
  for (uint64_t i = static_cast<uint64_t>(first) * kThreads + threadIdx.x; i < n;
       i += static_cast<uint64_t>(stride) * kThreads)
    acc += static_cast<double>(loss_term<NEG>(widen(x[i])));      // i < n
#pragma unroll
  for (int off = kWave / 2; off >= 1; off >>= 1) acc += __shfl_down(acc, off, kWave);
  if (threadIdx.x % kWave == 0) s_wave[threadIdx.x / kWave] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    acc = s_wave[0];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) acc += s_wave[w];
  }
  __syncthreads();
  return acc;
}

// acc: {sum_loss, sum_loss_times_P, batches, nonfinite, sum_P}; one thread calls it
__device__ __forceinline__ void finish(double sum_pos, double sum_neg, uint32_t P, uint32_t N,
                                       float* __restrict__ out, double* __restrict__ acc) {
  const float loss = static_cast<float>(sum_pos / static_cast<double>(P) +
                                        sum_neg / static_cast<double>(N));
  out[0] = loss;
  if (!acc) return;
  if (!isfinite(loss)) {
    acc[3] = acc[3] + 1.0;
    return;
  }
  acc[0] = acc[0] + static_cast<double>(loss);
  acc[1] = acc[1] + static_cast<double>(loss) * static_cast<double>(P);
  acc[2] = acc[2] + 1.0;
  acc[4] = acc[4] + static_cast<double>(P);
}

template <typename T>
__global__ void __launch_bounds__(kThreads)
link_loss_single(const T* __restrict__ pos, const T* __restrict__ neg, uint32_t P, uint32_t N,
                 float* __restrict__ out, double* __restrict__ acc) {
  __shared__ double s_wave[kWaves];
  const double sp = side_sum<T, false>(pos, P, 0, 1, s_wave);
  const double sn = side_sum<T, true>(neg, N, 0, 1, s_wave);
  if (threadIdx.x == 0) finish(sp, sn, P, N, out, acc);
}

// workgroups [0, rows_pos) walk the positives, [rows_pos, rows_pos + rows_neg) the negatives
template <typename T>
__global__ void __launch_bounds__(kThreads)
link_loss_partials(const T* __restrict__ pos, const T* __restrict__ neg, uint32_t P, uint32_t N,
                   uint32_t rows_pos, uint32_t rows_neg, double* __restrict__ partials) {
  __shared__ double s_wave[kWaves];
  const uint32_t b = blockIdx.x;      // uniform over the workgroup
  const double s = b < rows_pos ? side_sum<T, false>(pos, P, b, rows_pos, s_wave)
                                : side_sum<T, true>(neg, N, b - rows_pos, rows_neg, s_wave);
  if (threadIdx.x == 0) partials[b] = s;
}

__global__ void __launch_bounds__(kFinishThreads)
link_loss_finish(const double* __restrict__ partials, uint32_t rows_pos, uint32_t rows_neg,
                 uint32_t P, uint32_t N, float* __restrict__ out, double* __restrict__ acc) {
  __shared__ double s[kLinkLossMaxPartialRows];
  const uint32_t rows = rows_pos + rows_neg;      // <= kLinkLossMaxPartialRows
  if (threadIdx.x < rows) s[threadIdx.x] = partials[threadIdx.x];
  __syncthreads();
  if (threadIdx.x != 0) return;
  double sp = 0.0, sn = 0.0;
  for (uint32_t p = 0; p < rows_pos; ++p) sp += s[p];
  for (uint32_t p = rows_pos; p < rows; ++p) sn += s[p];
  finish(sp, sn, P, N, out, acc);
}

// the logits [lo, hi) of the concatenation pos, neg: lo = P skips the positives, hi = P the
// negatives
template <typename T>
__global__ void __launch_bounds__(kBwdThreads)
link_loss_bwd(const T* __restrict__ pos, const T* __restrict__ neg, uint32_t P, uint32_t N,
              uint64_t lo, uint64_t hi, const float* __restrict__ grad_out,
              T* __restrict__ grad_pos, T* __restrict__ grad_neg) {
  const uint64_t g = lo + static_cast<uint64_t>(blockIdx.x) * kBwdThreads + threadIdx.x;
  if (g >= hi) return;
  const float up = grad_out[0];
  if (g < P) {
    put(grad_pos + g, -sigmoid(-widen(pos[g])) * (up / static_cast<float>(P)));
  } else {
    const uint64_t j = g - P;      // < N
    put(grad_neg + j, sigmoid(widen(neg[j])) * (up / static_cast<float>(N)));
  }
}

uint32_t tiles(size_t n) { return static_cast<uint32_t>((n + kLinkLossTile - 1) / kLinkLossTile); }
uint32_t side_rows(size_t n) { return tiles(n) < kMaxSideRows ? tiles(n) : kMaxSideRows; }

void check_sizes(const char* what, size_t num_pos, size_t num_neg) {
  GF_REQUIRE(num_pos >= 1 && num_neg >= 1,
             std::string(what) + ": needs at least one positive and one negative logit");
  GF_REQUIRE(num_pos < (size_t{1} << 31) && num_neg < (size_t{1} << 31),
             std::string(what) + ": more than 2^31 - 1 logits on a side");
}

bool single(size_t num_pos, size_t num_neg) {
  return static_cast<size_t>(tiles(num_pos)) + tiles(num_neg) <= kLinkLossSingleTiles;
}

template <typename T>
void forward(const T* d_pos, const T* d_neg, size_t num_pos, size_t num_neg, double* d_partials,
             size_t partial_rows_given, float* d_out, double* d_acc, int device,
             hipStream_t stream) {
  check_sizes("link_loss", num_pos, num_neg);
  GF_REQUIRE(d_pos && d_neg && d_out, "link_loss: null pos, neg or out");
  const uint32_t P = static_cast<uint32_t>(num_pos), N = static_cast<uint32_t>(num_neg);
  if (single(num_pos, num_neg)) {
    DeviceGuard dg(device);
    link_loss_single<T><<<dim3(1), dim3(kThreads), 0, stream>>>(d_pos, d_neg, P, N, d_out, d_acc);
    GF_HIP(hipGetLastError());
    return;
  }
  const uint32_t rows_pos = side_rows(num_pos), rows_neg = side_rows(num_neg);
  GF_REQUIRE(d_partials != nullptr && partial_rows_given >= size_t{rows_pos} + rows_neg,
             "link_loss: partials buffer missing or smaller than gf_link_loss_partial_rows() "
             "asks for");
  DeviceGuard dg(device);
  link_loss_partials<T><<<dim3(rows_pos + rows_neg), dim3(kThreads), 0, stream>>>(
      d_pos, d_neg, P, N, rows_pos, rows_neg, d_partials);
  GF_HIP(hipGetLastError());
  link_loss_finish<<<dim3(1), dim3(kFinishThreads), 0, stream>>>(d_partials, rows_pos, rows_neg,
                                                                 P, N, d_out, d_acc);
  GF_HIP(hipGetLastError());
}

template <typename T>
void backward(const T* d_pos, const T* d_neg, size_t num_pos, size_t num_neg,
              const float* d_grad_out, T* d_grad_pos, T* d_grad_neg, int device,
              hipStream_t stream) {
  check_sizes("link_loss backward", num_pos, num_neg);
  GF_REQUIRE(d_pos && d_neg, "link_loss backward: null pos or neg");
  GF_REQUIRE(d_grad_out != nullptr, "link_loss backward: null gradient");
  if (!d_grad_pos && !d_grad_neg) return;
  const uint64_t lo = d_grad_pos ? 0 : num_pos;
  const uint64_t hi = d_grad_neg ? num_pos + num_neg : num_pos;      // lo < hi < 2^32
  const uint32_t groups = static_cast<uint32_t>((hi - lo + kBwdThreads - 1) / kBwdThreads);
  DeviceGuard dg(device);
  link_loss_bwd<T><<<dim3(groups), dim3(kBwdThreads), 0, stream>>>(
      d_pos, d_neg, static_cast<uint32_t>(num_pos), static_cast<uint32_t>(num_neg), lo, hi,
      d_grad_out, d_grad_pos, d_grad_neg);
  GF_HIP(hipGetLastError());
}

}  // namespace

size_t link_loss_partial_rows(size_t num_pos, size_t num_neg) {
  check_sizes("link_loss", num_pos, num_neg);
  return single(num_pos, num_neg) ? 0 : size_t{side_rows(num_pos)} + side_rows(num_neg);
}

void link_loss_forward(const float* d_pos, const float* d_neg, size_t num_pos, size_t num_neg,
                       double* d_partials, size_t partial_rows, float* d_out, double* d_acc,
                       int device, hipStream_t stream) {
  forward(d_pos, d_neg, num_pos, num_neg, d_partials, partial_rows, d_out, d_acc, device, stream);
}

void link_loss_backward(const float* d_pos, const float* d_neg, size_t num_pos, size_t num_neg,
                        const float* d_grad_out, float* d_grad_pos, float* d_grad_neg, int device,
                        hipStream_t stream) {
  backward(d_pos, d_neg, num_pos, num_neg, d_grad_out, d_grad_pos, d_grad_neg, device, stream);
}

void link_loss_bf16_forward(const uint16_t* d_pos, const uint16_t* d_neg, size_t num_pos,
                            size_t num_neg, double* d_partials, size_t partial_rows, float* d_out,
                            double* d_acc, int device, hipStream_t stream) {
  forward(d_pos, d_neg, num_pos, num_neg, d_partials, partial_rows, d_out, d_acc, device, stream);
}

void link_loss_bf16_backward(const uint16_t* d_pos, const uint16_t* d_neg, size_t num_pos,
                             size_t num_neg, const float* d_grad_out, uint16_t* d_grad_pos,
                             uint16_t* d_grad_neg, int device, hipStream_t stream) {
  backward(d_pos, d_neg, num_pos, num_neg, d_grad_out, d_grad_pos, d_grad_neg, device, stream);
}

}  // namespace gf
