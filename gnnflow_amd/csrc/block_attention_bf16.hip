// The kernels of block_attention.hip for bfloat16 q, k, v, out and gradients (carried as
// uint16_t): the same work split, the same two-pass softmax over scores parked in att[], the same
// head_dot() and the same Philox mask.  Every element is widened to float32 when it is loaded
// (exact), the arithmetic is the float32 kernels' own, operation for operation and in the same
// order, and a result is rounded once, to nearest even, when it is stored.  att[] and the dropped
// attention stay float32: the softmax Jacobian needs them at full precision and they are only
// [E, H].  The library is built with -ffp-contract=off and without fast-math, so
//
//   bf16 kernel(x)  ==  round_to_bf16(float32 kernel(widen(x)))      bit for bit,
//
// forward and backward, which is what tests/test_gpu_block_attention_bf16.py asserts.
//
// Loads are one 2-byte access per column.  A lane owns the columns lig + G * j, as in the float32
// kernels: that map fixes the order in which head_dot() sums, so pairing two adjacent columns
// into one 4-byte load would either change the sums (and break the equality above) or need a
// shuffle per pair to hand the odd column to its owner.  A group's 2-byte loads are one
// contiguous run of the row.  Measured at the TGN epoch's shapes (2 heads of 50 columns, 12 000
// destinations, 120 000 edges; profiles/amp_bf16_epoch.json) these kernels take the float32
// kernels' time, 24 us forward and 40 us backward per launch: half the bytes bought nothing
// there, so bytes are not what bounds them at that width and the load form is not either.
#include "block_attention_common.hpp"

namespace gf {
namespace {

using bf16 = uint16_t;

template <int G, int NC>
__global__ void block_attention_bf16_fwd(const int64_t* __restrict__ offsets, uint64_t items,
                                         uint32_t H, uint32_t D, const bf16* __restrict__ q,
                                         const bf16* __restrict__ k, const bf16* __restrict__ v,
                                         float slope, bf16* __restrict__ out, float* att) {
  const uint32_t lig = threadIdx.x & (G - 1);
  const uint64_t w = (static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x) / G;
  if (w >= items) return;                     // group-uniform
  const uint64_t d = w / H;
  const uint32_t h = static_cast<uint32_t>(w - d * H);
  const int64_t b = offsets[d], e = offsets[d + 1];
  const uint64_t width = static_cast<uint64_t>(H) * D;
  bf16* out_row = out + d * width + static_cast<uint64_t>(h) * D;
  if (e <= b) {                               // no in-edges: exactly 0
#pragma unroll
    for (int j = 0; j < NC; ++j)
      if (lig + G * j < D) out_row[lig + G * j] = 0;
    return;
  }
  float qr[NC];
  load_head<G, NC>(qr, q + d * width + static_cast<uint64_t>(h) * D, D, lig);

  // pass 1 (reads k once): scores into att[], running max
  float m = -FLT_MAX;
  for (int64_t i = b; i < e; ++i) {
    const float s = leaky(head_dot<G, NC>(qr, k + i * width + static_cast<uint64_t>(h) * D, D, lig),
                          slope);
    m = fmaxf(m, s);
    if (static_cast<uint32_t>(i - b) % G == lig) att[i * H + h] = s;
  }
  // pass 2a: the lane's own scores -> sum of exponentials
  float l = 0.f;
  for (int64_t i = b + lig; i < e; i += G) l += __expf(att[i * H + h] - m);
  const float inv = 1.f / group_sum<G>(l);
  // pass 2b (reads v once)
  float acc[NC];
#pragma unroll
  for (int j = 0; j < NC; ++j) acc[j] = 0.f;
  for (int64_t base = b; base < e; base += G) {
    const int64_t mine = base + lig;
    float a = 0.f;
    if (mine < e) {
      a = __expf(att[mine * H + h] - m) * inv;
      att[mine * H + h] = a;
    }
    const int n = static_cast<int>(e - base < G ? e - base : G);
    for (int t = 0; t < n; ++t) {
      const float at = group_read<G>(a, t);
      const bf16* vr = v + (base + t) * width + static_cast<uint64_t>(h) * D;
#pragma unroll
      for (int j = 0; j < NC; ++j) {
        const uint32_t c = lig + G * j;
        if (c < D) acc[j] += at * widen(vr[c]);
      }
    }
  }
#pragma unroll
  for (int j = 0; j < NC; ++j)
    if (lig + G * j < D) out_row[lig + G * j] = narrow(acc[j]);
}

template <int G, int NC>
__global__ void block_attention_dropout_bf16_fwd(
    const int64_t* __restrict__ offsets, uint64_t items, uint32_t H, uint32_t D,
    const bf16* __restrict__ q, const bf16* __restrict__ k, const bf16* __restrict__ v,
    float slope, Dropout dr, bf16* __restrict__ out, float* att,
    float* __restrict__ att_dropped) {
  const uint32_t lig = threadIdx.x & (G - 1);
  const uint64_t w = (static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x) / G;
  if (w >= items) return;                     // group-uniform
  const uint64_t d = w / H;
  const uint32_t h = static_cast<uint32_t>(w - d * H);
  const int64_t b = offsets[d], e = offsets[d + 1];
  const uint64_t width = static_cast<uint64_t>(H) * D;
  bf16* out_row = out + d * width + static_cast<uint64_t>(h) * D;
  if (e <= b) {                               // no in-edges: exactly 0
#pragma unroll
    for (int j = 0; j < NC; ++j)
      if (lig + G * j < D) out_row[lig + G * j] = 0;
    return;
  }
  float qr[NC];
  load_head<G, NC>(qr, q + d * width + static_cast<uint64_t>(h) * D, D, lig);

  float m = -FLT_MAX;
  for (int64_t i = b; i < e; ++i) {
    const float s = leaky(head_dot<G, NC>(qr, k + i * width + static_cast<uint64_t>(h) * D, D, lig),
                          slope);
    m = fmaxf(m, s);
    if (static_cast<uint32_t>(i - b) % G == lig) att[i * H + h] = s;
  }
  float l = 0.f;
  for (int64_t i = b + lig; i < e; i += G) l += __expf(att[i * H + h] - m);
  const float inv = 1.f / group_sum<G>(l);
  // pass 2b: the lane's copy of a becomes a * w, or -1 for a dropped edge
  float acc[NC];
#pragma unroll
  for (int j = 0; j < NC; ++j) acc[j] = 0.f;
  for (int64_t base = b; base < e; base += G) {
    const int64_t mine = base + lig;
    float a = 0.f;
    if (mine < e) {
      a = __expf(att[mine * H + h] - m) * inv;
      att[mine * H + h] = a;
      a = kept(dr, static_cast<uint64_t>(mine), H, h) ? a * dr.scale : -1.f;
      if (att_dropped) att_dropped[mine * H + h] = a < 0.f ? 0.f : a;
    }
    const int n = static_cast<int>(e - base < G ? e - base : G);
    for (int t = 0; t < n; ++t) {
      const float at = group_read<G>(a, t);
      if (at < 0.f) continue;                 // dropped: exactly 0, v not read (group-uniform)
      const bf16* vr = v + (base + t) * width + static_cast<uint64_t>(h) * D;
#pragma unroll
      for (int j = 0; j < NC; ++j) {
        const uint32_t c = lig + G * j;
        if (c < D) acc[j] += at * widen(vr[c]);
      }
    }
  }
#pragma unroll
  for (int j = 0; j < NC; ++j)
    if (lig + G * j < D) out_row[lig + G * j] = narrow(acc[j]);
}

// block_attention_bwd on bfloat16 q, k, v, gout; gq, gk, gv rounded once on store
template <int G, int NC>
__global__ void block_attention_bf16_bwd(const int64_t* __restrict__ offsets, uint64_t items,
                                         uint32_t H, uint32_t D, const bf16* __restrict__ q,
                                         const bf16* __restrict__ k, const bf16* __restrict__ v,
                                         const float* __restrict__ att, float slope,
                                         const bf16* __restrict__ gout, bf16* __restrict__ gq,
                                         bf16* __restrict__ gk, bf16* __restrict__ gv) {
  const uint32_t lig = threadIdx.x & (G - 1);
  const uint64_t w = (static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x) / G;
  if (w >= items) return;
  const uint64_t d = w / H;
  const uint32_t h = static_cast<uint32_t>(w - d * H);
  const int64_t b = offsets[d], e = offsets[d + 1];
  const uint64_t width = static_cast<uint64_t>(H) * D;
  const uint64_t head = static_cast<uint64_t>(h) * D;
  if (e <= b) {
    if (gq) {
#pragma unroll
      for (int j = 0; j < NC; ++j)
        if (lig + G * j < D) gq[d * width + head + lig + G * j] = 0;
    }
    return;
  }
  float gr[NC];
  load_head<G, NC>(gr, gout + d * width + head, D, lig);

  if (gv) {
    for (int64_t i = b; i < e; ++i) {
      const float a = att[i * H + h];
#pragma unroll
      for (int j = 0; j < NC; ++j) {
        const uint32_t c = lig + G * j;
        if (c < D) gv[i * width + head + c] = narrow(a * gr[j]);
      }
    }
  }
  if (!gq && !gk) return;

  float dot = 0.f;
  for (int64_t i = b; i < e; ++i)
    dot += att[i * H + h] * head_dot<G, NC>(gr, v + i * width + head, D, lig);

  float qr[NC], acc[NC];
  load_head<G, NC>(qr, q + d * width + head, D, lig);
#pragma unroll
  for (int j = 0; j < NC; ++j) acc[j] = 0.f;
  for (int64_t i = b; i < e; ++i) {
    const bf16* kr = k + i * width + head;
    const float ga = head_dot<G, NC>(gr, v + i * width + head, D, lig);
    const float z = head_dot<G, NC>(qr, kr, D, lig);
    const float gs = att[i * H + h] * (ga - dot);
    const float gz = z > 0.f ? gs : gs * slope;
#pragma unroll
    for (int j = 0; j < NC; ++j) {
      const uint32_t c = lig + G * j;
      if (c < D) {
        if (gk) gk[i * width + head + c] = narrow(gz * qr[j]);
        acc[j] += gz * widen(kr[c]);
      }
    }
  }
  if (gq) {
#pragma unroll
    for (int j = 0; j < NC; ++j)
      if (lig + G * j < D) gq[d * width + head + lig + G * j] = narrow(acc[j]);
  }
}

template <int G, int NC>
__global__ void block_attention_dropout_bf16_bwd(
    const int64_t* __restrict__ offsets, uint64_t items, uint32_t H, uint32_t D,
    const bf16* __restrict__ q, const bf16* __restrict__ k, const bf16* __restrict__ v,
    const float* __restrict__ att, float slope, Dropout dr, const bf16* __restrict__ gout,
    bf16* __restrict__ gq, bf16* __restrict__ gk, bf16* __restrict__ gv) {
  const uint32_t lig = threadIdx.x & (G - 1);
  const uint64_t w = (static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x) / G;
  if (w >= items) return;
  const uint64_t d = w / H;
  const uint32_t h = static_cast<uint32_t>(w - d * H);
  const int64_t b = offsets[d], e = offsets[d + 1];
  const uint64_t width = static_cast<uint64_t>(H) * D;
  const uint64_t head = static_cast<uint64_t>(h) * D;
  if (e <= b) {
    if (gq) {
#pragma unroll
      for (int j = 0; j < NC; ++j)
        if (lig + G * j < D) gq[d * width + head + lig + G * j] = 0;
    }
    return;
  }
  float gr[NC];
  load_head<G, NC>(gr, gout + d * width + head, D, lig);
  const bool chain = gq || gk;

  // sweep 1: gv, and dot = sum a ga over the kept edges (in edge order)
  float dot = 0.f;
  for (int64_t base = b; base < e; base += G) {
    const int64_t mine = base + lig;
    float a = 0.f, wm = 0.f;
    if (mine < e) {
      a = att[mine * H + h];
      wm = kept(dr, static_cast<uint64_t>(mine), H, h) ? dr.scale : 0.f;
    }
    const int n = static_cast<int>(e - base < G ? e - base : G);
    for (int t = 0; t < n; ++t) {
      const float at = group_read<G>(a, t);
      const float wt = group_read<G>(wm, t);   // scale >= 1, so 0 means dropped
      const int64_t i = base + t;
      if (wt == 0.f) {
        if (gv) {
#pragma unroll
          for (int j = 0; j < NC; ++j)
            if (lig + G * j < D) gv[i * width + head + lig + G * j] = 0;
        }
        continue;
      }
      if (gv) {
        const float aw = at * wt;
#pragma unroll
        for (int j = 0; j < NC; ++j) {
          const uint32_t c = lig + G * j;
          if (c < D) gv[i * width + head + c] = narrow(aw * gr[j]);
        }
      }
      if (chain) dot += at * (wt * head_dot<G, NC>(gr, v + i * width + head, D, lig));
    }
  }
  if (!chain) return;

  // sweep 2: ga again (the same head_dot, the same bits), z by the forward's own sequence
  float qr[NC], acc[NC];
  load_head<G, NC>(qr, q + d * width + head, D, lig);
#pragma unroll
  for (int j = 0; j < NC; ++j) acc[j] = 0.f;
  for (int64_t base = b; base < e; base += G) {
    const int64_t mine = base + lig;
    float a = 0.f, wm = 0.f;
    if (mine < e) {
      a = att[mine * H + h];
      wm = kept(dr, static_cast<uint64_t>(mine), H, h) ? dr.scale : 0.f;
    }
    const int n = static_cast<int>(e - base < G ? e - base : G);
    for (int t = 0; t < n; ++t) {
      const float at = group_read<G>(a, t);
      const float wt = group_read<G>(wm, t);
      const int64_t i = base + t;
      const bf16* kr = k + i * width + head;
      float ga = 0.f;
      if (wt != 0.f) ga = wt * head_dot<G, NC>(gr, v + i * width + head, D, lig);
      const float z = head_dot<G, NC>(qr, kr, D, lig);
      const float gs = at * (ga - dot);
      const float gz = z > 0.f ? gs : gs * slope;
#pragma unroll
      for (int j = 0; j < NC; ++j) {
        const uint32_t c = lig + G * j;
        if (c < D) {
          if (gk) gk[i * width + head + c] = narrow(gz * qr[j]);
          acc[j] += gz * widen(kr[c]);
        }
      }
    }
  }
  if (gq) {
#pragma unroll
    for (int j = 0; j < NC; ++j)
      if (lig + G * j < D) gq[d * width + head + lig + G * j] = narrow(acc[j]);
  }
}

struct Fwd {
  Shape s; const bf16 *q, *k, *v; float slope; bf16* out; float* att; hipStream_t stream;
  template <int G, int NC> void operator()() {
    block_attention_bf16_fwd<G, NC><<<dim3(grid_of(s, G)), dim3(kThreads), 0, stream>>>(
        s.offsets, s.items, s.H, s.D, q, k, v, slope, out, att);
  }
};
struct Bwd {
  Shape s; const bf16 *q, *k, *v; const float* att; float slope; const bf16* gout;
  bf16 *gq, *gk, *gv; hipStream_t stream;
  template <int G, int NC> void operator()() {
    block_attention_bf16_bwd<G, NC><<<dim3(grid_of(s, G)), dim3(kThreads), 0, stream>>>(
        s.offsets, s.items, s.H, s.D, q, k, v, att, slope, gout, gq, gk, gv);
  }
};
struct DropoutFwd {
  Shape s; const bf16 *q, *k, *v; float slope; Dropout dr; bf16* out; float *att, *att_dropped;
  hipStream_t stream;
  template <int G, int NC> void operator()() {
    block_attention_dropout_bf16_fwd<G, NC><<<dim3(grid_of(s, G)), dim3(kThreads), 0, stream>>>(
        s.offsets, s.items, s.H, s.D, q, k, v, slope, dr, out, att, att_dropped);
  }
};
struct DropoutBwd {
  Shape s; const bf16 *q, *k, *v; const float* att; float slope; Dropout dr; const bf16* gout;
  bf16 *gq, *gk, *gv; hipStream_t stream;
  template <int G, int NC> void operator()() {
    block_attention_dropout_bf16_bwd<G, NC><<<dim3(grid_of(s, G)), dim3(kThreads), 0, stream>>>(
        s.offsets, s.items, s.H, s.D, q, k, v, att, slope, dr, gout, gq, gk, gv);
  }
};

}  // namespace

// the checks of block_attention.hip's entry points, one for one

void block_attention_bf16_forward(const int64_t* d_offsets, size_t num_dst, size_t num_edges,
                                  size_t heads, size_t head_dim, const uint16_t* d_q,
                                  const uint16_t* d_k, const uint16_t* d_v, float negative_slope,
                                  uint16_t* d_out, float* d_att, int device, hipStream_t stream) {
  const Shape s = checked_shape(d_offsets, num_dst, heads, head_dim);
  if (num_dst == 0) return;
  GF_REQUIRE(d_q && d_out, "block_attention: null q or out");
  GF_REQUIRE(num_edges == 0 || (d_k && d_v && d_att), "block_attention: null k, v or att");
  DeviceGuard dg(device);
  dispatch(s.D, Fwd{s, d_q, d_k, d_v, negative_slope, d_out, d_att, stream});
  GF_HIP(hipGetLastError());
}

void block_attention_bf16_backward(const int64_t* d_offsets, size_t num_dst, size_t num_edges,
                                   size_t heads, size_t head_dim, const uint16_t* d_q,
                                   const uint16_t* d_k, const uint16_t* d_v, const float* d_att,
                                   float negative_slope, const uint16_t* d_grad_out,
                                   uint16_t* d_grad_q, uint16_t* d_grad_k, uint16_t* d_grad_v,
                                   int device, hipStream_t stream) {
  const Shape s = checked_shape(d_offsets, num_dst, heads, head_dim);
  if (num_dst == 0 || (!d_grad_q && !d_grad_k && !d_grad_v)) return;
  GF_REQUIRE(d_grad_out != nullptr, "block_attention backward: null gradient");
  GF_REQUIRE(num_edges == 0 || (d_att && d_v), "block_attention backward: null att or v");
  GF_REQUIRE(num_edges == 0 || (!d_grad_q && !d_grad_k) || (d_q && d_k),
             "block_attention backward: grad_q / grad_k need q and k");
  if (num_edges == 0 && !d_grad_q) return;
  DeviceGuard dg(device);
  dispatch(s.D, Bwd{s, d_q, d_k, d_v, d_att, negative_slope, d_grad_out, d_grad_q, d_grad_k,
                    d_grad_v, stream});
  GF_HIP(hipGetLastError());
}

void block_attention_dropout_bf16_forward(const int64_t* d_offsets, size_t num_dst,
                                          size_t num_edges, size_t heads, size_t head_dim,
                                          const uint16_t* d_q, const uint16_t* d_k,
                                          const uint16_t* d_v, float negative_slope, float p,
                                          uint64_t seed, uint16_t* d_out, float* d_att,
                                          float* d_att_dropped, int device, hipStream_t stream) {
  const Dropout dr = checked_dropout(p, seed);
  const Shape s = checked_shape(d_offsets, num_dst, heads, head_dim);
  if (num_dst == 0) return;
  GF_REQUIRE(d_q && d_out, "block_attention: null q or out");
  GF_REQUIRE(num_edges == 0 || (d_k && d_v && d_att), "block_attention: null k, v or att");
  DeviceGuard dg(device);
  dispatch(s.D, DropoutFwd{s, d_q, d_k, d_v, negative_slope, dr, d_out, d_att, d_att_dropped,
                           stream});
  GF_HIP(hipGetLastError());
}

void block_attention_dropout_bf16_backward(const int64_t* d_offsets, size_t num_dst,
                                           size_t num_edges, size_t heads, size_t head_dim,
                                           const uint16_t* d_q, const uint16_t* d_k,
                                           const uint16_t* d_v, const float* d_att,
                                           float negative_slope, float p, uint64_t seed,
                                           const uint16_t* d_grad_out, uint16_t* d_grad_q,
                                           uint16_t* d_grad_k, uint16_t* d_grad_v, int device,
                                           hipStream_t stream) {
  const Dropout dr = checked_dropout(p, seed);
  const Shape s = checked_shape(d_offsets, num_dst, heads, head_dim);
  if (num_dst == 0 || (!d_grad_q && !d_grad_k && !d_grad_v)) return;
  GF_REQUIRE(d_grad_out != nullptr, "block_attention backward: null gradient");
  GF_REQUIRE(num_edges == 0 || (d_att && d_v), "block_attention backward: null att or v");
  GF_REQUIRE(num_edges == 0 || (!d_grad_q && !d_grad_k) || (d_q && d_k),
             "block_attention backward: grad_q / grad_k need q and k");
  if (num_edges == 0 && !d_grad_q) return;
  DeviceGuard dg(device);
  dispatch(s.D, DropoutBwd{s, d_q, d_k, d_v, d_att, negative_slope, dr, d_grad_out, d_grad_q,
                           d_grad_k, d_grad_v, stream});
  GF_HIP(hipGetLastError());
}

}  // namespace gf
