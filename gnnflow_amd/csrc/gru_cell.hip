// Fused gates of a GRU cell behind its two GEMMs (torch.nn.GRUCell; the reference's TGN memory
// updater, gnnflow/models/modules/memory_updater.py:62-85), as ONE launch forward and ONE launch
// backward.  gi = x W_ih^T + b_ih and gh = h W_hh^T + b_hh are [N, 3H] with the gate chunks in
// torch's order r, z, n; hx is [N, H]:
//
//   r = sigma(gi_r + gh_r)     z = sigma(gi_z + gh_z)     n = tanh(gi_n + r * gh_n)
//   u = (1 - z) * n + z * hx
//   h_out[i] = u[i] (+ residual[i])      i < N
//   last[i]  = u[i]                      i < R <= N      (never the residual)
//
// The forward writes h_out and last and nothing else: no workspace and no saved gates.  The
// backward recomputes r, z, n from gi, gh and hx through the same function (gru_gates) and, from
// g = d h_out, writes whichever of these is asked for (a null pointer: not wanted):
//
//   a_n = g * (1 - z) * (1 - n * n)      a_z = g * (hx - n) * z * (1 - z)
//   a_r = a_n * gh_n * r * (1 - r)
//   d_gi = [a_r, a_z, a_n]      d_gh = [a_r, a_z, a_n * r]      d_hx = g * z
//
// Every output element is a fixed expression of the input elements of its own (row, column): no
// reduction, so the results do not depend on N, the grid, the path or the alignment, and are
// bit-reproducible.
//
// A thread owns W consecutive columns of one row: W = 4 (float32 gates) or 8 (bfloat16 gates) as
// 16-byte accesses when H % W == 0 and every base pointer is aligned for it -- the row pitches
// 3H and H and the chunk offsets H and 2H inherit the alignment --, W = 4 on bfloat16 gates as
// 8-byte gate accesses when only H % 4 == 0 holds (H = 100), and W = 1, element by element,
// otherwise.
//
// sigma(x) = 1 / (1 + expf(-x)) and tanhf are the library's accurate functions, not the fast
// intrinsics: expf overflows to +inf at x <= -89 and 1 / inf = 0, it underflows to 0 at large x
// and 1 / 1 = 1, and tanhf saturates to +-1, so no pre-activation gives a NaN or an infinity.
//
// bfloat16 (bf16.hpp): gi and gh, and d_gi and d_gh, may be bfloat16, and so may the residual,
// independently; hx, h_out, last, g and d_hx are float32 always.  Each bfloat16 element is
// widened (exact) where the float32 kernel loads it, the arithmetic and its order are the same
// instantiation's, and d_gi and d_gh are rounded once, to nearest even, when they are stored.
#include "bf16.hpp"
#include "block_ops.hpp"
#include "common.hpp"

#include <cstdint>
#include <initializer_list>

namespace gf {
namespace {

constexpr int kThreads = 256;

__device__ __forceinline__ float gru_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }

// the only place the gates are computed, forward and backward
__device__ __forceinline__ void gru_gates(float ir, float hr, float iz, float hz, float in,
                                          float hn, float& r, float& z, float& n) {
  r = gru_sigmoid(ir + hr);
  z = gru_sigmoid(iz + hz);
  n = tanhf(in + r * hn);
}

// W consecutive elements as one access of W * sizeof(T) bytes (two of 16 for 8 floats)
template <int W>
__device__ __forceinline__ void load_w(const float* p, float (&v)[W]) {
  if constexpr (W == 1) {
    v[0] = p[0];
  } else {
#pragma unroll
    for (int q = 0; q < W; q += 4) {
      const float4 t = *reinterpret_cast<const float4*>(p + q);
      v[q] = t.x, v[q + 1] = t.y, v[q + 2] = t.z, v[q + 3] = t.w;
    }
  }
}
template <int W>
__device__ __forceinline__ void load_w(const uint16_t* p, float (&v)[W]) {
  if constexpr (W == 1) {
    v[0] = widen(p[0]);
  } else if constexpr (W == 4) {
    const uint2 t = *reinterpret_cast<const uint2*>(p);
    v[0] = __uint_as_float(t.x << 16), v[1] = __uint_as_float(t.x & 0xffff0000u);
    v[2] = __uint_as_float(t.y << 16), v[3] = __uint_as_float(t.y & 0xffff0000u);
  } else {
    const uint4 t = *reinterpret_cast<const uint4*>(p);
    v[0] = __uint_as_float(t.x << 16), v[1] = __uint_as_float(t.x & 0xffff0000u);
    v[2] = __uint_as_float(t.y << 16), v[3] = __uint_as_float(t.y & 0xffff0000u);
    v[4] = __uint_as_float(t.z << 16), v[5] = __uint_as_float(t.z & 0xffff0000u);
    v[6] = __uint_as_float(t.w << 16), v[7] = __uint_as_float(t.w & 0xffff0000u);
  }
}
template <int W>
__device__ __forceinline__ void store_w(float* p, const float (&v)[W]) {
  if constexpr (W == 1) {
    p[0] = v[0];
  } else {
#pragma unroll
    for (int q = 0; q < W; q += 4)
      *reinterpret_cast<float4*>(p + q) = make_float4(v[q], v[q + 1], v[q + 2], v[q + 3]);
  }
}
__device__ __forceinline__ uint32_t pack2(float lo, float hi) {
  return static_cast<uint32_t>(narrow(lo)) | (static_cast<uint32_t>(narrow(hi)) << 16);
}
template <int W>
__device__ __forceinline__ void store_w(uint16_t* p, const float (&v)[W]) {
  if constexpr (W == 1) {
    p[0] = narrow(v[0]);
  } else if constexpr (W == 4) {
    *reinterpret_cast<uint2*>(p) = make_uint2(pack2(v[0], v[1]), pack2(v[2], v[3]));
  } else {
    *reinterpret_cast<uint4*>(p) = make_uint4(pack2(v[0], v[1]), pack2(v[2], v[3]),
                                              pack2(v[4], v[5]), pack2(v[6], v[7]));
  }
}

// work item `idx` of `items` = N * (H / W): its row and its first column
template <int W>
__device__ __forceinline__ void locate(uint64_t idx, uint64_t items, uint32_t H, uint64_t& row,
                                       uint32_t& col) {
  const uint32_t per_row = H / W;
  if (items <= 0xffffffffull) {      // uniform over the grid
    const uint32_t i = static_cast<uint32_t>(idx);
    row = i / per_row;
    col = (i % per_row) * W;
  } else {
    row = idx / per_row;
    col = static_cast<uint32_t>(idx % per_row) * W;
  }
}

// GT: the gates' type, RT: the residual's (residual may be null; last is null when R == 0)
template <typename GT, typename RT, int W>
__global__ void __launch_bounds__(kThreads)
gru_cell_fwd(const GT* __restrict__ gi, const GT* __restrict__ gh, const float* __restrict__ hx,
             const RT* __restrict__ residual, uint64_t items, uint32_t H, uint64_t R,
             float* __restrict__ out, float* __restrict__ last) {
  const uint64_t idx = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (idx >= items) return;
  uint64_t row;
  uint32_t col;
  locate<W>(idx, items, H, row, col);
  const uint64_t g0 = row * 3 * H + col, h0 = row * H + col;
  float ir[W], iz[W], in[W], hr[W], hz[W], hn[W], h[W], u[W];
  load_w<W>(gi + g0, ir);
  load_w<W>(gi + g0 + H, iz);
  load_w<W>(gi + g0 + 2 * static_cast<uint64_t>(H), in);
  load_w<W>(gh + g0, hr);
  load_w<W>(gh + g0 + H, hz);
  load_w<W>(gh + g0 + 2 * static_cast<uint64_t>(H), hn);
  load_w<W>(hx + h0, h);
#pragma unroll
  for (int q = 0; q < W; ++q) {
    float r, z, n;
    gru_gates(ir[q], hr[q], iz[q], hz[q], in[q], hn[q], r, z, n);
    u[q] = (1.f - z) * n + z * h[q];
  }
  if (row < R) store_w<W>(last + h0, u);
  if (residual) {
    float res[W];
    load_w<W>(residual + h0, res);
#pragma unroll
    for (int q = 0; q < W; ++q) u[q] = u[q] + res[q];
  }
  store_w<W>(out + h0, u);
}

// a null dgi, dgh or dhx is skipped (uniform over the grid)
template <typename GT, int W>
__global__ void __launch_bounds__(kThreads)
gru_cell_bwd(const GT* __restrict__ gi, const GT* __restrict__ gh, const float* __restrict__ hx,
             const float* __restrict__ g, uint64_t items, uint32_t H, GT* __restrict__ dgi,
             GT* __restrict__ dgh, float* __restrict__ dhx) {
  const uint64_t idx = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (idx >= items) return;
  uint64_t row;
  uint32_t col;
  locate<W>(idx, items, H, row, col);
  const uint64_t g0 = row * 3 * H + col, h0 = row * H + col;
  const uint64_t H2 = 2 * static_cast<uint64_t>(H);
  float ir[W], iz[W], in[W], hr[W], hz[W], hn[W], h[W], go[W];
  load_w<W>(gi + g0, ir);
  load_w<W>(gi + g0 + H, iz);
  load_w<W>(gi + g0 + H2, in);
  load_w<W>(gh + g0, hr);
  load_w<W>(gh + g0 + H, hz);
  load_w<W>(gh + g0 + H2, hn);
  load_w<W>(hx + h0, h);
  load_w<W>(g + h0, go);
  float ar[W], az[W], an[W], anr[W], dh[W];
#pragma unroll
  for (int q = 0; q < W; ++q) {
    float r, z, n;
    gru_gates(ir[q], hr[q], iz[q], hz[q], in[q], hn[q], r, z, n);
    an[q] = go[q] * (1.f - z) * (1.f - n * n);
    az[q] = go[q] * (h[q] - n) * z * (1.f - z);
    ar[q] = an[q] * hn[q] * r * (1.f - r);
    anr[q] = an[q] * r;
    dh[q] = go[q] * z;
  }
  if (dgi) {
    store_w<W>(dgi + g0, ar);
    store_w<W>(dgi + g0 + H, az);
    store_w<W>(dgi + g0 + H2, an);
  }
  if (dgh) {
    store_w<W>(dgh + g0, ar);
    store_w<W>(dgh + g0 + H, az);
    store_w<W>(dgh + g0 + H2, anr);
  }
  if (dhx) store_w<W>(dhx + h0, dh);
}

// null pointers are aligned to everything
bool aligned(const void* p, size_t bytes) {
  return (reinterpret_cast<uintptr_t>(p) & (bytes - 1)) == 0;
}

// the columns a thread owns: every access of W elements of a gate row (gate_size bytes each) and
// of W floats must be aligned to min(16, its size), for every base pointer given
template <typename GT>
int pick_width(size_t H, std::initializer_list<const void*> gates,
               std::initializer_list<const void*> floats, const void* residual,
               size_t residual_size) {
  for (const int W : {8, 4}) {
    if (W * sizeof(GT) > 16 || H % W != 0) continue;
    bool ok = aligned(residual, W * residual_size < 16 ? W * residual_size : 16);
    for (const void* p : gates) ok = ok && aligned(p, W * sizeof(GT));
    for (const void* p : floats) ok = ok && aligned(p, 16);
    if (ok) return W;
  }
  return 1;
}

// the checks both directions share; false = nothing to do
bool check_shape(const char* what, size_t n, size_t hidden) {
  GF_REQUIRE(hidden >= 1, std::string(what) + ": hidden must be >= 1");
  GF_REQUIRE(hidden < (size_t{1} << 30), std::string(what) + ": hidden too large");
  if (n == 0) return false;
  GF_REQUIRE(n < (size_t{1} << 31), std::string(what) + ": more than 2^31 - 1 rows");
  // one thread per element on the scalar path, 2^31 - 1 workgroups at the most
  GF_REQUIRE(n * hidden < (size_t{1} << 38), std::string(what) + ": 2^38 elements or more");
  return true;
}

dim3 grid_for(uint64_t items) {
  return dim3(static_cast<uint32_t>((items + kThreads - 1) / kThreads));
}

template <typename GT, typename RT>
void launch_fwd(const GT* gi, const GT* gh, const float* hx, const RT* residual, size_t n,
                size_t hidden, size_t num_last, float* out, float* last, hipStream_t stream) {
  const int W = pick_width<GT>(hidden, {gi, gh}, {hx, out, last}, residual, sizeof(RT));
  const uint32_t H = static_cast<uint32_t>(hidden);
  const uint64_t items = static_cast<uint64_t>(n) * (H / W), R = num_last;
  const dim3 grid = grid_for(items), block(kThreads);
  if (W == 8)
    gru_cell_fwd<GT, RT, 8><<<grid, block, 0, stream>>>(gi, gh, hx, residual, items, H, R, out,
                                                        last);
  else if (W == 4)
    gru_cell_fwd<GT, RT, 4><<<grid, block, 0, stream>>>(gi, gh, hx, residual, items, H, R, out,
                                                        last);
  else
    gru_cell_fwd<GT, RT, 1><<<grid, block, 0, stream>>>(gi, gh, hx, residual, items, H, R, out,
                                                        last);
  GF_HIP(hipGetLastError());
}

template <typename GT>
void forward(const GT* d_gi, const GT* d_gh, const float* d_hx, const void* d_residual,
             int residual_bf16, size_t n, size_t hidden, size_t num_last, float* d_out,
             float* d_last, int device, hipStream_t stream) {
  GF_REQUIRE(num_last <= n, "gru_cell: num_last exceeds the number of rows");
  GF_REQUIRE(residual_bf16 == 0 || residual_bf16 == 1, "gru_cell: residual_bf16 must be 0 or 1");
  if (!check_shape("gru_cell", n, hidden)) return;
  GF_REQUIRE(d_gi && d_gh && d_hx && d_out, "gru_cell: null gi, gh, hx or out");
  GF_REQUIRE(num_last == 0 || d_last != nullptr, "gru_cell: null last with num_last > 0");
  DeviceGuard dg(device);
  if (residual_bf16)
    launch_fwd(d_gi, d_gh, d_hx, static_cast<const uint16_t*>(d_residual), n, hidden, num_last,
               d_out, num_last ? d_last : nullptr, stream);
  else
    launch_fwd(d_gi, d_gh, d_hx, static_cast<const float*>(d_residual), n, hidden, num_last,
               d_out, num_last ? d_last : nullptr, stream);
}

template <typename GT>
void backward(const GT* d_gi, const GT* d_gh, const float* d_hx, size_t n, size_t hidden,
              const float* d_grad_out, GT* d_grad_gi, GT* d_grad_gh, float* d_grad_hx, int device,
              hipStream_t stream) {
  if (!check_shape("gru_cell backward", n, hidden)) return;
  GF_REQUIRE(d_gi && d_gh && d_hx, "gru_cell backward: null gi, gh or hx");
  GF_REQUIRE(d_grad_out != nullptr, "gru_cell backward: null gradient");
  if (!d_grad_gi && !d_grad_gh && !d_grad_hx) return;
  const int W = pick_width<GT>(hidden, {d_gi, d_gh, d_grad_gi, d_grad_gh},
                               {d_hx, d_grad_out, d_grad_hx}, nullptr, sizeof(float));
  const uint32_t H = static_cast<uint32_t>(hidden);
  const uint64_t items = static_cast<uint64_t>(n) * (H / W);
  const dim3 grid = grid_for(items), block(kThreads);
  DeviceGuard dg(device);
  if (W == 8)
    gru_cell_bwd<GT, 8><<<grid, block, 0, stream>>>(d_gi, d_gh, d_hx, d_grad_out, items, H,
                                                    d_grad_gi, d_grad_gh, d_grad_hx);
  else if (W == 4)
    gru_cell_bwd<GT, 4><<<grid, block, 0, stream>>>(d_gi, d_gh, d_hx, d_grad_out, items, H,
                                                    d_grad_gi, d_grad_gh, d_grad_hx);
  else
    gru_cell_bwd<GT, 1><<<grid, block, 0, stream>>>(d_gi, d_gh, d_hx, d_grad_out, items, H,
                                                    d_grad_gi, d_grad_gh, d_grad_hx);
  GF_HIP(hipGetLastError());
}

}  // namespace

void gru_cell_forward(const float* d_gi, const float* d_gh, const float* d_hx,
                      const void* d_residual, int residual_bf16, size_t n, size_t hidden,
                      size_t num_last, float* d_out, float* d_last, int device,
                      hipStream_t stream) {
  forward(d_gi, d_gh, d_hx, d_residual, residual_bf16, n, hidden, num_last, d_out, d_last, device,
          stream);
}

void gru_cell_backward(const float* d_gi, const float* d_gh, const float* d_hx, size_t n,
                       size_t hidden, const float* d_grad_out, float* d_grad_gi, float* d_grad_gh,
                       float* d_grad_hx, int device, hipStream_t stream) {
  backward(d_gi, d_gh, d_hx, n, hidden, d_grad_out, d_grad_gi, d_grad_gh, d_grad_hx, device,
           stream);
}

void gru_cell_bf16_forward(const uint16_t* d_gi, const uint16_t* d_gh, const float* d_hx,
                           const void* d_residual, int residual_bf16, size_t n, size_t hidden,
                           size_t num_last, float* d_out, float* d_last, int device,
                           hipStream_t stream) {
  forward(d_gi, d_gh, d_hx, d_residual, residual_bf16, n, hidden, num_last, d_out, d_last, device,
          stream);
}

void gru_cell_bf16_backward(const uint16_t* d_gi, const uint16_t* d_gh, const float* d_hx,
                            size_t n, size_t hidden, const float* d_grad_out,
                            uint16_t* d_grad_gi, uint16_t* d_grad_gh, float* d_grad_hx,
                            int device, hipStream_t stream) {
  backward(d_gi, d_gh, d_hx, n, hidden, d_grad_out, d_grad_gi, d_grad_gh, d_grad_hx, device,
           stream);
}

}  // namespace gf
