// Fused time encoding: the [features | cos(w * dt + b)] rows that every temporal layer of the
// reference builds (gnnflow/models/modules/layers.py:16-42 TimeEncode, followed by torch.cat in
// layers.py:118-137 and memory_updater.py:62-65), as ONE launch forward and a deterministic
// two-launch reduction backward.  fp32 throughout.
//
//   out[i, 0:Wa]            = a[i, :]
//   out[i, Wa:Wa+Wb]        = b[i, :]
//   out[i, Wa+Wb+j], j < T  = cosf(w[j] * t[i] + bias[j])
//
// Forward.  `out` is contiguous, so it is ONE flat run of n * (Wa + Wb + T) floats: thread k
// writes chunk k of it (V = 4 floats as one 16-byte store when Wa, Wb and T are multiples of 4
// and every base pointer is 16-byte aligned -- then every row and every region starts on a
// 16-byte boundary; V = 1 otherwise).  A wave's stores are one contiguous run whatever the
// widths are, its loads from a / b are contiguous within a row, and every output address is
// written exactly once.  A chunk never straddles two regions.
//
// Backward of the time columns (no gradient flows to t; a and b take column slices of grad_out
// in Python):
//
//   gw[j]    = - sum_i g[i,j] * sinf(w[j]*t[i] + bias[j]) * t[i]
//   gbias[j] = - sum_i g[i,j] * sinf(w[j]*t[i] + bias[j])
//
// with g read in place from grad_out through a row pitch and a column offset.  te_arg()
// (time_encode_expr.hpp, shared with neighbor_sequence.hip) is the only place the argument is
// computed, forward and backward (the library is built with -ffp-contract=off and without
// fast-math: one multiply, one add), and te_cos() there the only cosine of it.  Workgroup p owns the rows
// [p * rows_per_wg, (p + 1) * rows_per_wg); lanes sit over the columns j (CX of them, RY = 256 / CX
// row phases), each lane accumulates its rows in registers in ascending order, the RY phases
// are summed in ascending order through LDS, and the workgroup writes one row [2, T] of
// partials.  A second launch sums the at most kMaxPartialRows partial rows: 32 phases of
// ascending rows each, then the phases in ascending order.  No atomics anywhere: the result is
// a fixed expression of the inputs and bit-reproducible.
//
// cosf / sinf are the precise forms: a real timestamp times the first frequency is an argument
// of 1e6 rad and more, where __cosf / __sinf are wrong in the first digit.
//
// bfloat16 (T = uint16_t; bf16.hpp).  The forward can write a bfloat16 row from the same
// float32 parts, t, w and bias: one kernel body computes every column and only the chunk's store
// knows T, rounding once to nearest even.  Rows of an odd width put every second row on a 2-byte
// boundary, so the 4-column path (one 8-byte store) is taken only when, besides the float32
// path's conditions, out is 8-byte aligned: with every width a multiple of 4 each chunk then
// starts on an 8-byte boundary.  The backward can read a bfloat16 grad_out: each element is
// widened (exact) when it is loaded, and the partials, their layout and the finish kernel know
// no T, so gw and gbias are the float32 results on the widened gradient, bit for bit.
#include "bf16.hpp"
#include "block_ops.hpp"
#include "common.hpp"
#include "time_encode_expr.hpp"

#include <cstdint>

namespace gf {
namespace {

constexpr int kThreads = 256;
constexpr int kFinishThreads = 1024;   // 32 columns x 32 row phases
constexpr size_t kMinRowsPerGroup = 16;

template <int V> struct Chunk;
template <> struct Chunk<1> {
  float v[1];
  __device__ static Chunk load(const float* p) { return Chunk{{*p}}; }
  __device__ void store(float* p) const { *p = v[0]; }
  __device__ void store(uint16_t* p) const { *p = narrow(v[0]); }
};
template <> struct Chunk<4> {
  float v[4];
  __device__ static Chunk load(const float* p) {
    const float4 x = *reinterpret_cast<const float4*>(p);
    return Chunk{{x.x, x.y, x.z, x.w}};
  }
  __device__ void store(float* p) const {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  }
  __device__ void store(uint16_t* p) const {
    const uint32_t lo = narrow(v[0]) | static_cast<uint32_t>(narrow(v[1])) << 16;
    const uint32_t hi = narrow(v[2]) | static_cast<uint32_t>(narrow(v[3])) << 16;
    *reinterpret_cast<uint2*>(p) = make_uint2(lo, hi);
  }
};

// qa, qb, qt: the widths of a, b and the time columns in chunks of V floats; chunks = n * Q.
// T is out's element type: a chunk is narrowed, if at all, when it is stored.
template <class T, int V>
__global__ void __launch_bounds__(kThreads)
time_encode_cat_fwd(const float* __restrict__ a, uint32_t qa, const float* __restrict__ b,
                    uint32_t qb, const float* __restrict__ t, const float* __restrict__ w,
                    const float* __restrict__ bias, uint32_t qt, uint32_t chunks,
                    T* __restrict__ out) {
  const uint32_t k = blockIdx.x * static_cast<uint32_t>(kThreads) + threadIdx.x;
  if (k >= chunks) return;
  const uint32_t Q = qa + qb + qt;
  const uint32_t row = k / Q;
  const uint32_t c = k - row * Q;
  Chunk<V> x;
  if (c < qa) {
    x = Chunk<V>::load(a + (static_cast<uint64_t>(row) * qa + c) * V);
  } else if (c < qa + qb) {
    x = Chunk<V>::load(b + (static_cast<uint64_t>(row) * qb + (c - qa)) * V);
  } else {
    const uint32_t j = (c - qa - qb) * V;
    const Chunk<V> wj = Chunk<V>::load(w + j), bj = Chunk<V>::load(bias + j);
    const float ti = t[row];
#pragma unroll
    for (int e = 0; e < V; ++e) x.v[e] = te_cos(wj.v[e], ti, bj.v[e]);
  }
  x.store(out + static_cast<uint64_t>(k) * V);
}

// partials[p, 0, j] = gw's share of workgroup p's rows, partials[p, 1, j] = gbias's.
// G is the gradient's element type, widened where it is loaded.
template <class G, int CX>
__global__ void __launch_bounds__(kThreads)
time_encode_bwd_partials(const float* __restrict__ t, const float* __restrict__ w,
                         const float* __restrict__ bias, uint64_t n, uint32_t T,
                         const G* __restrict__ g, uint64_t pitch, uint64_t rows_per_wg,
                         float* __restrict__ partials) {
  constexpr int RY = kThreads / CX;
  __shared__ float sw[RY][CX], sb[RY][CX];
  const uint32_t cx = threadIdx.x % CX, ry = threadIdx.x / CX;
  const uint64_t r0 = blockIdx.x * rows_per_wg;
  const uint64_t r1 = r0 + rows_per_wg < n ? r0 + rows_per_wg : n;
  float* prow = partials + static_cast<uint64_t>(blockIdx.x) * 2 * T;
  for (uint32_t j0 = 0; j0 < T; j0 += CX) {      // uniform over the workgroup
    const uint32_t j = j0 + cx;
    const bool active = j < T;
    float aw = 0.f, ab = 0.f;
    if (active) {
      const float wj = w[j], bj = bias[j];
      const G* gj = g + j;
      for (uint64_t i = r0 + ry; i < r1; i += RY) {
        const float ti = t[i];
        const float p = widen(gj[i * pitch]) * sinf(te_arg(wj, ti, bj));
        ab += p;
        aw += p * ti;
      }
    }
    sw[ry][cx] = aw;
    sb[ry][cx] = ab;
    __syncthreads();
    if (ry == 0 && active) {
      float tw = sw[0][cx], tb = sb[0][cx];
#pragma unroll
      for (int r = 1; r < RY; ++r) {
        tw += sw[r][cx];
        tb += sb[r][cx];
      }
      prow[j] = -tw;
      prow[T + j] = -tb;
    }
    __syncthreads();
  }
}

// column c of the [rows, 2 * T] partials: c < T -> gw[c], else gbias[c - T]
__global__ void __launch_bounds__(kFinishThreads)
time_encode_bwd_finish(const float* __restrict__ partials, uint32_t rows, uint32_t T,
                       float* __restrict__ gw, float* __restrict__ gbias) {
  __shared__ float s[32][32];
  const uint32_t cx = threadIdx.x & 31, ph = threadIdx.x >> 5;
  const uint32_t c = blockIdx.x * 32 + cx, width = 2 * T;
  float acc = 0.f;
  if (c < width)
    for (uint32_t p = ph; p < rows; p += 32) acc += partials[static_cast<uint64_t>(p) * width + c];
  s[ph][cx] = acc;
  __syncthreads();
  if (ph != 0 || c >= width) return;
  float total = s[0][cx];
#pragma unroll
  for (int r = 1; r < 32; ++r) total += s[r][cx];
  if (c < T) {
    if (gw) gw[c] = total;
  } else if (gbias) {
    gbias[c - T] = total;
  }
}

// can four elements at p be one store?  16-byte aligned float32, 8-byte aligned bfloat16
template <class T>
bool aligned4(const T* p) { return (reinterpret_cast<uintptr_t>(p) & (4 * sizeof(T) - 1)) == 0; }

size_t partial_rows(size_t n) {
  const size_t groups = (n + kMinRowsPerGroup - 1) / kMinRowsPerGroup;
  return groups < kTimeEncodeMaxPartialRows ? groups : kTimeEncodeMaxPartialRows;
}

template <class T>
void cat_forward(const float* d_a, size_t width_a, const float* d_b, size_t width_b,
                 const float* d_t, const float* d_w, const float* d_bias, size_t n,
                 size_t dim_time, T* d_out, int device, hipStream_t stream) {
  GF_REQUIRE(dim_time >= 1, "time_encode_cat: dim_time must be >= 1");
  if (n == 0) return;
  GF_REQUIRE(d_t && d_w && d_bias && d_out, "time_encode_cat: null t, w, bias or out");
  GF_REQUIRE((width_a == 0 || d_a) && (width_b == 0 || d_b),
             "time_encode_cat: null part of non-zero width");
  const size_t limit = size_t{1} << 32;
  GF_REQUIRE(width_a < limit && width_b < limit && dim_time < limit &&
                 width_a + width_b + dim_time < limit &&
                 n <= (limit - 1) / (width_a + width_b + dim_time),
             "time_encode_cat: more than 2^32 - 1 output elements");
  const bool vec = width_a % 4 == 0 && width_b % 4 == 0 && dim_time % 4 == 0 &&
                   aligned16(d_a) && aligned16(d_b) && aligned16(d_w) && aligned16(d_bias) &&
                   aligned4(d_out);
  const uint32_t v = vec ? 4 : 1;
  const uint32_t qa = static_cast<uint32_t>(width_a / v), qb = static_cast<uint32_t>(width_b / v),
                 qt = static_cast<uint32_t>(dim_time / v);
  const uint32_t chunks = static_cast<uint32_t>(n * (qa + qb + qt));
  const dim3 grid(static_cast<unsigned>((uint64_t{chunks} + kThreads - 1) / kThreads)),
      block(kThreads);
  DeviceGuard dg(device);
  if (vec)
    time_encode_cat_fwd<T, 4><<<grid, block, 0, stream>>>(d_a, qa, d_b, qb, d_t, d_w, d_bias, qt,
                                                          chunks, d_out);
  else
    time_encode_cat_fwd<T, 1><<<grid, block, 0, stream>>>(d_a, qa, d_b, qb, d_t, d_w, d_bias, qt,
                                                          chunks, d_out);
  GF_HIP(hipGetLastError());
}

template <class G>
void backward(const float* d_t, const float* d_w, const float* d_bias, size_t n, size_t dim_time,
              const G* d_grad_out, size_t grad_pitch, size_t grad_col, float* d_partials,
              size_t partial_rows_given, float* d_grad_w, float* d_grad_bias, int device,
              hipStream_t stream) {
  GF_REQUIRE(dim_time >= 1, "time_encode backward: dim_time must be >= 1");
  GF_REQUIRE(dim_time < (size_t{1} << 30), "time_encode backward: dim_time too large");
  if (n == 0 || (!d_grad_w && !d_grad_bias)) return;
  GF_REQUIRE(d_t && d_w && d_bias, "time_encode backward: null t, w or bias");
  GF_REQUIRE(d_grad_out != nullptr, "time_encode backward: null gradient");
  GF_REQUIRE(grad_col + dim_time <= grad_pitch,
             "time_encode backward: the time columns do not fit the gradient's row pitch");
  GF_REQUIRE(d_partials != nullptr && partial_rows_given >= partial_rows(n),
             "time_encode backward: partials buffer missing or smaller than "
             "gf_time_encode_backward_partial_rows() asks for");
  const size_t want = partial_rows(n);
  const uint64_t rows_per_wg = (n + want - 1) / want;
  const uint32_t groups = static_cast<uint32_t>((n + rows_per_wg - 1) / rows_per_wg);   // <= want
  const uint32_t T = static_cast<uint32_t>(dim_time);
  const G* g = d_grad_out + grad_col;
  DeviceGuard dg(device);
  if (T <= 32)
    time_encode_bwd_partials<G, 32><<<dim3(groups), dim3(kThreads), 0, stream>>>(
        d_t, d_w, d_bias, n, T, g, grad_pitch, rows_per_wg, d_partials);
  else
    time_encode_bwd_partials<G, 128><<<dim3(groups), dim3(kThreads), 0, stream>>>(
        d_t, d_w, d_bias, n, T, g, grad_pitch, rows_per_wg, d_partials);
  GF_HIP(hipGetLastError());
  time_encode_bwd_finish<<<dim3((2 * T + 31) / 32), dim3(kFinishThreads), 0, stream>>>(
      d_partials, groups, T, d_grad_w, d_grad_bias);
  GF_HIP(hipGetLastError());
}

}  // namespace

size_t time_encode_backward_partial_rows(size_t n) { return partial_rows(n); }

void time_encode_cat_forward(const float* d_a, size_t width_a, const float* d_b, size_t width_b,
                             const float* d_t, const float* d_w, const float* d_bias, size_t n,
                             size_t dim_time, float* d_out, int device, hipStream_t stream) {
  cat_forward(d_a, width_a, d_b, width_b, d_t, d_w, d_bias, n, dim_time, d_out, device, stream);
}

void time_encode_backward(const float* d_t, const float* d_w, const float* d_bias, size_t n,
                          size_t dim_time, const float* d_grad_out, size_t grad_pitch,
                          size_t grad_col, float* d_partials, size_t partial_rows_given,
                          float* d_grad_w, float* d_grad_bias, int device, hipStream_t stream) {
  backward(d_t, d_w, d_bias, n, dim_time, d_grad_out, grad_pitch, grad_col, d_partials,
           partial_rows_given, d_grad_w, d_grad_bias, device, stream);
}

void time_encode_cat_bf16_forward(const float* d_a, size_t width_a, const float* d_b,
                                  size_t width_b, const float* d_t, const float* d_w,
                                  const float* d_bias, size_t n, size_t dim_time, uint16_t* d_out,
                                  int device, hipStream_t stream) {
  cat_forward(d_a, width_a, d_b, width_b, d_t, d_w, d_bias, n, dim_time, d_out, device, stream);
}

void time_encode_backward_bf16(const float* d_t, const float* d_w, const float* d_bias, size_t n,
                               size_t dim_time, const uint16_t* d_grad_out, size_t grad_pitch,
                               size_t grad_col, float* d_partials, size_t partial_rows_given,
                               float* d_grad_w, float* d_grad_bias, int device,
                               hipStream_t stream) {
  backward(d_t, d_w, d_bias, n, dim_time, d_grad_out, grad_pitch, grad_col, d_partials,
           partial_rows_given, d_grad_w, d_grad_bias, device, stream);
}

}  // namespace gf
