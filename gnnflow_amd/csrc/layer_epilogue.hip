// Fused epilogue of the reference's TemporalAttentionLayer (gnnflow/models/modules/layers.py:
// layer_norm(relu(dropout(w_out(rst)))) after the GEMM): dropout, relu and layer norm as ONE
// launch forward and at most two launches backward.  fp32 arithmetic throughout.
//
//   keep[r,d] = gf_philox4x32_10_first(seed, r * D + d, 0) >= T       T = uint32(double(p) * 2^32)
//   y[r,d]    = max(keep ? x[r,d] * sc : 0, 0)                         sc = 1.0f / (1.0f - p)
//   mean[r]   = sum_d y / D     var[r] = sum_d (y - mean)^2 / D     rstd[r] = 1 / sqrtf(var + eps)
//   out[r,d]  = (y - mean) * rstd * gamma[d] + beta[d]
//
// T == 0 (p == 0, where sc == 1) keeps everything without drawing.
//
// Forward.  One wave64 per row, kRows rows per workgroup, the row in registers.  Lane l owns the
// columns 4c .. 4c + 3 of the chunks c = l, l + 64, ...: NC = 4, 8 or 16 columns per lane for
// D <= 256, 512, 1024.  A chunk is one 16-byte access (8 bytes of a bfloat16 row) when D % 4 == 0
// and the pointers are aligned, element by element otherwise -- the same columns on the same lane
// either way, so the bits depend on neither.  Every sum is the lane's columns in ascending order,
// then a fixed xor butterfly over the 64 lanes.  The row is read once; the variance is a second
// pass over the registers (deviations from the mean), never E[y^2] - mean^2.  No mask is written:
// mean and rstd are, and the backward draws keep again from the seed.
//
// Backward, from mean and rstd as the forward stored them:
//
//   xhat = (y - mean) * rstd          g = grad_out * gamma
//   dy   = rstd * (g - sum_d(g) / D - xhat * (sum_d(g * xhat) / D))
//   grad_x[r,d]   = y > 0 ? dy * sc : 0             (y > 0 <=> keep and x * sc > 0)
//   grad_gamma[d] = sum_r grad_out * xhat          grad_beta[d] = sum_r grad_out
//
// Workgroup p owns the rows [p * rows_per_wg, (p + 1) * rows_per_wg); wave w of it takes the rows
// w, w + kRows, ... in ascending order, a row at a time as the forward does, and adds the row's
// terms of grad_gamma and grad_beta to its lanes' registers.  The kRows waves are summed in
// ascending order through LDS and the workgroup writes one row [2 D] of partials; a second launch
// sums the at most kLayerEpilogueMaxPartialRows partial rows as edge_score.hip does: 32 phases of
// ascending rows, then the phases in ascending order.  No atomics: every result is a fixed
// expression of the inputs and bit-reproducible.  Without grad_gamma and grad_beta there are no
// partials and no second launch, and every wave owns one row.
//
// bfloat16 (T = uint16_t; bf16.hpp): x and grad_x may be bfloat16 while everything else stays
// float32.  Each element is widened (exact) where the float32 kernel loads it, the arithmetic and
// its order are the float32 kernels' own, and grad_x is rounded once, to nearest even, on store.
#include "block_attention_common.hpp"

namespace gf {
namespace {

constexpr int kRows = kThreads / 64;                // rows (waves) per workgroup
constexpr int kFinishThreads = 1024;                // 32 columns x 32 row phases
constexpr size_t kMinRowsPerGroup = 8;

static_assert(kLayerEpilogueMaxWidth == 64 * kMaxChunks, "a row must fit one wave's registers");

// the four columns c .. c + 3 of a row; 0 past D.  VEC: D % 4 == 0, so c < D covers all four.
template <bool VEC>
__device__ inline void load4(const float* __restrict__ p, uint32_t c, uint32_t D, float (&v)[4]) {
  if (VEC) {
    float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
    if (c < D) t = *reinterpret_cast<const float4*>(p + c);
    v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = c + k < D ? p[c + k] : 0.f;
  }
}
template <bool VEC>
__device__ inline void load4(const uint16_t* __restrict__ p, uint32_t c, uint32_t D,
                             float (&v)[4]) {
  if (VEC) {
    uint2 t = make_uint2(0u, 0u);
    if (c < D) t = *reinterpret_cast<const uint2*>(p + c);
    v[0] = __uint_as_float(t.x << 16), v[1] = __uint_as_float(t.x & 0xffff0000u);
    v[2] = __uint_as_float(t.y << 16), v[3] = __uint_as_float(t.y & 0xffff0000u);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = c + k < D ? widen(p[c + k]) : 0.f;
  }
}

template <bool VEC>
__device__ inline void store4(float* __restrict__ p, uint32_t c, uint32_t D, const float (&v)[4]) {
  if (VEC) {
    if (c < D) *reinterpret_cast<float4*>(p + c) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (c + k < D) p[c + k] = v[k];
  }
}
template <bool VEC>
__device__ inline void store4(uint16_t* __restrict__ p, uint32_t c, uint32_t D,
                              const float (&v)[4]) {
  if (VEC) {
    if (c < D)
      *reinterpret_cast<uint2*>(p + c) =
          make_uint2(narrow(v[0]) | static_cast<uint32_t>(narrow(v[1])) << 16,
                     narrow(v[2]) | static_cast<uint32_t>(narrow(v[3])) << 16);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (c + k < D) p[c + k] = narrow(v[k]);
  }
}

// column of register q of lane `lane`
__device__ inline uint32_t column(uint32_t lane, int q) {
  return 4 * (lane + 64 * static_cast<uint32_t>(q / 4)) + static_cast<uint32_t>(q % 4);
}

template <int NC, bool VEC, class T>
__device__ inline void load_columns(float (&a)[NC], const T* __restrict__ row, uint32_t D,
                                    uint32_t lane) {
#pragma unroll
  for (int j = 0; j < NC / 4; ++j) {
    float v[4];
    load4<VEC>(row, 4 * (lane + 64 * j), D, v);
#pragma unroll
    for (int k = 0; k < 4; ++k) a[4 * j + k] = v[k];
  }
}

// y of the lane's columns of row r: the only place dropout and relu are computed, forward and
// backward.  0 past D.
template <int NC, bool VEC, class T>
__device__ inline void load_activated(float (&y)[NC], const T* __restrict__ x, uint32_t r,
                                      uint32_t D, uint32_t lane, const Dropout& dr) {
  const uint64_t base = static_cast<uint64_t>(r) * D;
  load_columns<NC, VEC>(y, x + base, D, lane);
#pragma unroll
  for (int q = 0; q < NC; ++q) {
    const uint32_t d = column(lane, q);
    float s = 0.f;
    if (d < D && (dr.threshold == 0 || gf_philox4x32_10_first(dr.seed, base + d, 0) >= dr.threshold))
      s = y[q] * dr.scale;
    y[q] = s > 0.f ? s : 0.f;
  }
}

template <int NC, bool VEC, class T>
__global__ void __launch_bounds__(kThreads)
layer_epilogue_fwd(const T* __restrict__ x, const float* __restrict__ gamma,
                   const float* __restrict__ beta, uint32_t R, uint32_t D, float eps, Dropout dr,
                   float* __restrict__ out, float* __restrict__ mean, float* __restrict__ rstd) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t r = blockIdx.x * static_cast<uint32_t>(kRows) + threadIdx.x / 64;
  if (r >= R) return;      // the whole wave
  float y[NC];
  load_activated<NC, VEC>(y, x, r, D, lane, dr);
  const float n = static_cast<float>(D);
  float s = 0.f;
#pragma unroll
  for (int q = 0; q < NC; ++q) s += y[q];
  const float m = group_sum<64>(s) / n;
  float ss = 0.f;
#pragma unroll
  for (int q = 0; q < NC; ++q) {
    const float dev = column(lane, q) < D ? y[q] - m : 0.f;
    ss += dev * dev;
  }
  const float rs = 1.0f / sqrtf(group_sum<64>(ss) / n + eps);
  float* o = out + static_cast<uint64_t>(r) * D;
#pragma unroll
  for (int j = 0; j < NC / 4; ++j) {
    const uint32_t c = 4 * (lane + 64 * j);
    float ga[4], be[4], v[4];
    load4<VEC>(gamma, c, D, ga);
    load4<VEC>(beta, c, D, be);
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = (y[4 * j + k] - m) * rs * ga[k] + be[k];
    store4<VEC>(o, c, D, v);
  }
  if (lane == 0) {
    mean[r] = m;
    rstd[r] = rs;
  }
}

// partials[p, c]: c < D -> grad_gamma[c]'s share of workgroup p's rows, D <= c < 2 D ->
// grad_beta[c - D]'s.  A null gx is skipped (uniform over the grid).  REDUCE: partials is not
// null; without it the kernel declares no LDS, so that a launch which needs none is not held to
// the occupancy 32 KiB per workgroup would allow at NC = 16.
template <int NC, bool VEC, bool REDUCE, class T>
__global__ void __launch_bounds__(kThreads)
layer_epilogue_bwd(const T* __restrict__ x, const float* __restrict__ gamma,
                   const float* __restrict__ mean, const float* __restrict__ rstd,
                   const float* __restrict__ go, uint32_t R, uint32_t D, Dropout dr,
                   uint32_t rows_per_wg, T* __restrict__ gx, float* __restrict__ partials) {
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x / 64;
  const uint32_t i0 = blockIdx.x * rows_per_wg;
  const uint32_t i1 = R - i0 < rows_per_wg ? R : i0 + rows_per_wg;      // i0 < R
  const float n = static_cast<float>(D);
  float gam[NC], ag[NC], ab[NC];
  load_columns<NC, VEC>(gam, gamma, D, lane);
#pragma unroll
  for (int q = 0; q < NC; ++q) ag[q] = ab[q] = 0.f;
  for (uint32_t r = i0 + wave; r < i1; r += kRows) {      // uniform over the wave
    float y[NC], g[NC];
    load_activated<NC, VEC>(y, x, r, D, lane, dr);
    load_columns<NC, VEC>(g, go + static_cast<uint64_t>(r) * D, D, lane);
    const float m = mean[r], rs = rstd[r];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int q = 0; q < NC; ++q) {
      const float xh = column(lane, q) < D ? (y[q] - m) * rs : 0.f;
      const float gg = g[q] * gam[q];
      s1 += gg;
      s2 += gg * xh;
      if (REDUCE) {
        ag[q] += g[q] * xh;
        ab[q] += g[q];
      }
    }
    const float m1 = group_sum<64>(s1) / n, m2 = group_sum<64>(s2) / n;
    if (gx) {
      T* o = gx + static_cast<uint64_t>(r) * D;
#pragma unroll
      for (int j = 0; j < NC / 4; ++j) {
        float v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int q = 4 * j + k;
          const float xh = (y[q] - m) * rs;
          const float dy = rs * (g[q] * gam[q] - m1 - xh * m2);
          v[k] = y[q] > 0.f ? dy * dr.scale : 0.f;
        }
        store4<VEC>(o, 4 * (lane + 64 * j), D, v);
      }
    }
  }
  if constexpr (REDUCE) {
    __shared__ float sp[kRows][2][64 * NC];
#pragma unroll
    for (int q = 0; q < NC; ++q) {
      const uint32_t d = column(lane, q);      // < 64 * NC
      sp[wave][0][d] = ag[q];
      sp[wave][1][d] = ab[q];
    }
    __syncthreads();
    float* prow = partials + static_cast<uint64_t>(blockIdx.x) * 2 * D;
    for (uint32_t c = threadIdx.x; c < 2 * D; c += kThreads) {
      const uint32_t which = c < D ? 0 : 1, d = c < D ? c : c - D;
      float t = sp[0][which][d];
#pragma unroll
      for (int w = 1; w < kRows; ++w) t += sp[w][which][d];
      prow[c] = t;
    }
  }
}

// column c of the [rows, 2 D] partials: c < D -> grad_gamma[c], else grad_beta[c - D]
__global__ void __launch_bounds__(kFinishThreads)
layer_epilogue_bwd_finish(const float* __restrict__ partials, uint32_t rows, uint32_t D,
                          float* __restrict__ gg, float* __restrict__ gb) {
  __shared__ float s[32][32];
  const uint32_t cx = threadIdx.x & 31, ph = threadIdx.x >> 5;
  const uint32_t c = blockIdx.x * 32 + cx, width = 2 * D;
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
    if (gg) gg[c] = total;
  } else if (gb) {
    gb[c - D] = total;
  }
}

bool aligned(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

size_t partial_rows(size_t R) {
  const size_t groups = (R + kMinRowsPerGroup - 1) / kMinRowsPerGroup;
  return groups < kLayerEpilogueMaxPartialRows ? groups : kLayerEpilogueMaxPartialRows;
}

// the checks both directions share, before any pointer is looked at
Dropout check_shape(const char* what, size_t R, size_t D, float p, uint64_t seed) {
  const std::string w(what);
  GF_REQUIRE(D >= 1, w + ": dim must be >= 1");
  GF_REQUIRE(D <= kLayerEpilogueMaxWidth,
             w + ": dim exceeds GF_LAYER_EPILOGUE_MAX_WIDTH (1024)");
  GF_REQUIRE(p >= 0.f && p < 1.f, w + ": dropout p must be in [0, 1)");      // NaN fails
  GF_REQUIRE(R < (size_t{1} << 31), w + ": more than 2^31 - 1 rows");
  return Dropout{static_cast<uint32_t>(static_cast<double>(p) * 4294967296.0), 1.0f / (1.0f - p),
                 seed};
}

template <class T>
void forward(const T* d_x, const float* d_gamma, const float* d_beta, size_t R, size_t D,
             float eps, float p, uint64_t seed, float* d_out, float* d_mean, float* d_rstd,
             int device, hipStream_t stream) {
  const Dropout dr = check_shape("layer_epilogue", R, D, p, seed);
  GF_REQUIRE(eps > 0.f, "layer_epilogue: eps must be > 0");      // NaN fails
  if (R == 0) return;
  GF_REQUIRE(d_x && d_gamma && d_beta && d_out && d_mean && d_rstd,
             "layer_epilogue: null x, gamma, beta, out, mean or rstd");
  const bool vec = D % 4 == 0 && aligned(d_x, 4 * sizeof(T)) && aligned(d_gamma, 16) &&
                   aligned(d_beta, 16) && aligned(d_out, 16);
  const uint32_t rows = static_cast<uint32_t>(R), dim = static_cast<uint32_t>(D);
  const dim3 grid((rows + kRows - 1) / kRows), block(kThreads);
  DeviceGuard dg(device);
#define GF_LE_FWD(NC, VEC)                                                                  \
  layer_epilogue_fwd<NC, VEC, T><<<grid, block, 0, stream>>>(d_x, d_gamma, d_beta, rows, dim, \
                                                             eps, dr, d_out, d_mean, d_rstd)
  if (D <= 256) { if (vec) GF_LE_FWD(4, true); else GF_LE_FWD(4, false); }
  else if (D <= 512) { if (vec) GF_LE_FWD(8, true); else GF_LE_FWD(8, false); }
  else { if (vec) GF_LE_FWD(16, true); else GF_LE_FWD(16, false); }
#undef GF_LE_FWD
  GF_HIP(hipGetLastError());
}

template <class T>
void backward(const T* d_x, const float* d_gamma, const float* d_mean, const float* d_rstd,
              size_t R, size_t D, float p, uint64_t seed, const float* d_grad_out,
              float* d_partials, size_t partial_rows_given, T* d_grad_x, float* d_grad_gamma,
              float* d_grad_beta, int device, hipStream_t stream) {
  const Dropout dr = check_shape("layer_epilogue backward", R, D, p, seed);
  const bool reduce = d_grad_gamma || d_grad_beta;
  if (R == 0) {      // empty sums
    if (!reduce) return;
    DeviceGuard dg(device);
    if (d_grad_gamma) GF_HIP(hipMemsetAsync(d_grad_gamma, 0, D * sizeof(float), stream));
    if (d_grad_beta) GF_HIP(hipMemsetAsync(d_grad_beta, 0, D * sizeof(float), stream));
    return;
  }
  GF_REQUIRE(d_x && d_gamma && d_mean && d_rstd,
             "layer_epilogue backward: null x, gamma, mean or rstd");
  GF_REQUIRE(d_grad_out != nullptr, "layer_epilogue backward: null gradient");
  if (!reduce && !d_grad_x) return;
  const size_t want = partial_rows(R);
  GF_REQUIRE(!reduce || (d_partials != nullptr && partial_rows_given >= want),
             "layer_epilogue backward: partials buffer missing or smaller than "
             "gf_layer_epilogue_backward_partial_rows() asks for");
  const bool vec = D % 4 == 0 && aligned(d_x, 4 * sizeof(T)) && aligned(d_gamma, 16) &&
                   aligned(d_grad_out, 16) && (!d_grad_x || aligned(d_grad_x, 4 * sizeof(T)));
  const uint32_t rows = static_cast<uint32_t>(R), dim = static_cast<uint32_t>(D);
  const uint32_t rows_per_wg = reduce ? static_cast<uint32_t>((R + want - 1) / want) : kRows;
  const uint32_t groups = (rows + rows_per_wg - 1) / rows_per_wg;      // <= want when reducing
  float* partials = reduce ? d_partials : nullptr;
  const dim3 grid(groups), block(kThreads);
  DeviceGuard dg(device);
#define GF_LE_BWD_R(NC, VEC, REDUCE)                                                   \
  layer_epilogue_bwd<NC, VEC, REDUCE, T><<<grid, block, 0, stream>>>(                  \
      d_x, d_gamma, d_mean, d_rstd, d_grad_out, rows, dim, dr, rows_per_wg, d_grad_x, partials)
#define GF_LE_BWD(NC, VEC) \
  do { if (reduce) GF_LE_BWD_R(NC, VEC, true); else GF_LE_BWD_R(NC, VEC, false); } while (0)
  if (D <= 256) { if (vec) GF_LE_BWD(4, true); else GF_LE_BWD(4, false); }
  else if (D <= 512) { if (vec) GF_LE_BWD(8, true); else GF_LE_BWD(8, false); }
  else { if (vec) GF_LE_BWD(16, true); else GF_LE_BWD(16, false); }
#undef GF_LE_BWD
#undef GF_LE_BWD_R
  GF_HIP(hipGetLastError());
  if (!reduce) return;
  layer_epilogue_bwd_finish<<<dim3((2 * dim + 31) / 32), dim3(kFinishThreads), 0, stream>>>(
      d_partials, groups, dim, d_grad_gamma, d_grad_beta);
  GF_HIP(hipGetLastError());
}

}  // namespace

size_t layer_epilogue_backward_partial_rows(size_t num_rows) { return partial_rows(num_rows); }

void layer_epilogue_forward(const float* d_x, const float* d_gamma, const float* d_beta,
                            size_t num_rows, size_t dim, float eps, float p, uint64_t seed,
                            float* d_out, float* d_mean, float* d_rstd, int device,
                            hipStream_t stream) {
  forward(d_x, d_gamma, d_beta, num_rows, dim, eps, p, seed, d_out, d_mean, d_rstd, device,
          stream);
}

void layer_epilogue_backward(const float* d_x, const float* d_gamma, const float* d_mean,
                             const float* d_rstd, size_t num_rows, size_t dim, float p,
                             uint64_t seed, const float* d_grad_out, float* d_partials,
                             size_t partial_rows, float* d_grad_x, float* d_grad_gamma,
                             float* d_grad_beta, int device, hipStream_t stream) {
  backward(d_x, d_gamma, d_mean, d_rstd, num_rows, dim, p, seed, d_grad_out, d_partials,
           partial_rows, d_grad_x, d_grad_gamma, d_grad_beta, device, stream);
}

void layer_epilogue_bf16_forward(const uint16_t* d_x, const float* d_gamma, const float* d_beta,
                                 size_t num_rows, size_t dim, float eps, float p, uint64_t seed,
                                 float* d_out, float* d_mean, float* d_rstd, int device,
                                 hipStream_t stream) {
  forward(d_x, d_gamma, d_beta, num_rows, dim, eps, p, seed, d_out, d_mean, d_rstd, device,
          stream);
}

void layer_epilogue_bf16_backward(const uint16_t* d_x, const float* d_gamma, const float* d_mean,
                                  const float* d_rstd, size_t num_rows, size_t dim, float p,
                                  uint64_t seed, const float* d_grad_out, float* d_partials,
                                  size_t partial_rows, uint16_t* d_grad_x, float* d_grad_gamma,
                                  float* d_grad_beta, int device, hipStream_t stream) {
  backward(d_x, d_gamma, d_mean, d_rstd, num_rows, dim, p, seed, d_grad_out, d_partials,
           partial_rows, d_grad_x, d_grad_gamma, d_grad_beta, device, stream);
}

}  // namespace gf
