// Fused temporal attention over a sampled block: the attention of the reference's
// TransfomerAttentionLayer (gnnflow/models/modules/layers.py:144-159) as ONE segment operation.
//
//   z[e,h]     = sum_c q[d,h,c] * k[e,h,c]          d = destination of edge e
//   s[e,h]     = z > 0 ? z : slope * z
//   a[e,h]     = softmax of s over the edges of d (max-subtracted)
//   out[d,h,c] = sum_e a[e,h] * v[e,h,c]
//
// The layer computes K and V PER EDGE and a block's edges are grouped by destination, so edge
// e reads k[e], v[e] and q[row[e]]: no source index, no atomics, forward or backward, and
// every output address is written exactly once.  The arithmetic is fp32 throughout.
//
// Work item = one (destination, head) pair, given to a GROUP of G lanes (G = 8, 16, 32 or 64,
// the smallest that covers the D columns of a head; a head wider than 64 columns gives each
// lane NC = ceil(D / 64) columns, rounded up to a power of two, at most 16).  A head's
// columns are contiguous, so a group's loads are one contiguous run and heads need no
// alignment to the 64-lane stride.  Sums over a head's columns are a per-lane serial sum over
// its NC columns followed by an xor butterfly over the group; `head_dot()` is the only place a
// score is computed, forward and backward, so both passes see bit-identical z (the library is
// built with -ffp-contract=off and without fast-math) and never disagree about its sign.
//
// Softmax: TWO PASSES over the scores, which are parked in att[] itself.  Score i of a segment
// is written, read back and finally replaced by a[i] by the same lane (i mod G) of the same
// group, so no fence is needed; k and v are each read exactly once by the forward.
//
// Attention dropout (the *_dropout kernels; the reference drops the attention weights after the
// softmax, layers.py:153-155) needs no mask tensor: edge i of the grouped order and head h are
//   kept  <=>  gf_philox4x32_10_first(seed, i * H + h, 0) >= T,   T = (uint32_t)(p * 2^32)
//   w[i,h] = kept ? 1 / (1 - p) : 0          out[d,h,:] = sum_i (a[i,h] * w[i,h]) * v[i,h,:]
// a decision per (edge, head), hence uniform over the group that owns the head.  The lane that
// computes a[i] draws the decision, so the forward costs one Philox per (edge, head); the
// backward draws it again the same way (G edges at a time, one per lane, handed round the group)
// instead of reading a stored mask.  att[] keeps the PRE-dropout a -- the softmax Jacobian needs
// it -- and a * w goes to a second, optional buffer.  A dropped edge contributes exactly 0 and
// its v row is NOT READ, forward or backward: a non-finite v on a dropped edge does not
// propagate, unlike 0 * inf = NaN in the composed edge_softmax -> dropout -> block_reduce chain.
// The kernels without dropout are kept as they were and compile to the code they had before
// dropout existed.
//
// Element type T: float, or uint16_t carrying bfloat16, for q, k, v, out and the gradients.
// Every element is widened to float32 when it is loaded (exact; widen() of a float is the float)
// and a result is rounded once, to nearest even, when it is stored (narrow_to<T>()).  att[] and
// the dropped attention stay float32 whatever T: the softmax Jacobian needs them at full
// precision and they are only [E, H].  One body serves both types, so
//
//   bf16 kernel(x)  ==  round_to_bf16(float32 kernel(widen(x)))      bit for bit,
//
// forward and backward, which is what tests/test_gpu_block_attention_bf16.py asserts.
//
// bfloat16 loads are one 2-byte access per column.  A lane owns the columns lig + G * j whatever
// the type: that map fixes the order in which head_dot() sums, so pairing two adjacent columns
// into one 4-byte load would either change the sums (and break the equality above) or need a
// shuffle per pair to hand the odd column to its owner.  A group's 2-byte loads are one
// contiguous run of the row.  Measured at the TGN epoch's shapes (2 heads of 50 columns, 12 000
// destinations, 120 000 edges; profiles/amp_bf16_epoch.json) the bfloat16 kernels take the
// float32 kernels' time, 24 us forward and 40 us backward per launch: half the bytes bought
// nothing there, so bytes are not what bounds them at that width and the load form is not either.
#include "block_attention_common.hpp"

namespace gf {
namespace {

template <class T, int G, int NC>
__global__ void block_attention_fwd(const int64_t* __restrict__ offsets, uint64_t items,
                                    uint32_t H, uint32_t D, const T* __restrict__ q,
                                    const T* __restrict__ k, const T* __restrict__ v,
                                    float slope, T* __restrict__ out, float* att) {
  const uint32_t lig = threadIdx.x & (G - 1);
  const uint64_t w = (static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x) / G;
  if (w >= items) return;                     // group-uniform
  const uint64_t d = w / H;
  const uint32_t h = static_cast<uint32_t>(w - d * H);
  const int64_t b = offsets[d], e = offsets[d + 1];
  const uint64_t width = static_cast<uint64_t>(H) * D;
  T* out_row = out + d * width + static_cast<uint64_t>(h) * D;
  if (e <= b) {                               // no in-edges: exactly 0
#pragma unroll
    for (int j = 0; j < NC; ++j)
      if (lig + G * j < D) out_row[lig + G * j] = narrow_to<T>(0.f);
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
  // pass 2b (reads v once): a = exp(s - m) / l replaces the score, G edges at a time, and each
  // a is handed round the group for the weighted sum
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
      const T* vr = v + (base + t) * width + static_cast<uint64_t>(h) * D;
#pragma unroll
      for (int j = 0; j < NC; ++j) {
        const uint32_t c = lig + G * j;
        if (c < D) acc[j] += at * widen(vr[c]);
      }
    }
  }
#pragma unroll
  for (int j = 0; j < NC; ++j)
    if (lig + G * j < D) out_row[lig + G * j] = narrow_to<T>(acc[j]);
}

// The forward with dropout: block_attention_fwd with the mask applied in pass 2b.  The lane
// that owns a[i] replaces its copy by a * w, or by -1 for a dropped edge (a * w is never
// negative), so still one value per edge goes round the group.  A kernel of its own rather than
// a template flag on block_attention_fwd: a shared body changed the register allocation of the
// NC > 1 instantiations without dropout.
template <class T, int G, int NC>
__global__ void block_attention_dropout_fwd(
    const int64_t* __restrict__ offsets, uint64_t items, uint32_t H, uint32_t D,
    const T* __restrict__ q, const T* __restrict__ k, const T* __restrict__ v, float slope,
    Dropout dr, T* __restrict__ out, float* att, float* __restrict__ att_dropped) {
  const uint32_t lig = threadIdx.x & (G - 1);
  const uint64_t w = (static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x) / G;
  if (w >= items) return;                     // group-uniform
  const uint64_t d = w / H;
  const uint32_t h = static_cast<uint32_t>(w - d * H);
  const int64_t b = offsets[d], e = offsets[d + 1];
  const uint64_t width = static_cast<uint64_t>(H) * D;
  T* out_row = out + d * width + static_cast<uint64_t>(h) * D;
  if (e <= b) {                               // no in-edges: exactly 0
#pragma unroll
    for (int j = 0; j < NC; ++j)
      if (lig + G * j < D) out_row[lig + G * j] = narrow_to<T>(0.f);
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
  // pass 2b: as above; the lane's copy of a becomes a * w, or -1 for a dropped edge
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
      const T* vr = v + (base + t) * width + static_cast<uint64_t>(h) * D;
#pragma unroll
      for (int j = 0; j < NC; ++j) {
        const uint32_t c = lig + G * j;
        if (c < D) acc[j] += at * widen(vr[c]);
      }
    }
  }
#pragma unroll
  for (int j = 0; j < NC; ++j)
    if (lig + G * j < D) out_row[lig + G * j] = narrow_to<T>(acc[j]);
}

// ga[e,h] = sum_c gout[d,h,c] v[e,h,c]        gv[e,h,c] = a[e,h] gout[d,h,c]
// gs[e,h] = a (ga - sum_e' a ga)              gz = gs * (z > 0 ? 1 : slope)
// gq[d,h,c] = sum_e gz k[e,h,c]               gk[e,h,c] = gz q[d,h,c]
// Sweep 1 forms sum a ga; sweep 2 recomputes ga (the same head_dot, so the same bits) instead
// of parking it anywhere.  A null gq / gk / gv skips that output's work; z is recomputed by
// the forward's own instruction sequence only when gq or gk is wanted.
template <class T, int G, int NC>
__global__ void block_attention_bwd(const int64_t* __restrict__ offsets, uint64_t items,
                                    uint32_t H, uint32_t D, const T* __restrict__ q,
                                    const T* __restrict__ k, const T* __restrict__ v,
                                    const float* __restrict__ att, float slope,
                                    const T* __restrict__ gout, T* __restrict__ gq,
                                    T* __restrict__ gk, T* __restrict__ gv) {
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
        if (lig + G * j < D) gq[d * width + head + lig + G * j] = narrow_to<T>(0.f);
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
        if (c < D) gv[i * width + head + c] = narrow_to<T>(a * gr[j]);
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
    const T* kr = k + i * width + head;
    const float ga = head_dot<G, NC>(gr, v + i * width + head, D, lig);
    const float z = head_dot<G, NC>(qr, kr, D, lig);
    const float gs = att[i * H + h] * (ga - dot);
    const float gz = z > 0.f ? gs : gs * slope;
#pragma unroll
    for (int j = 0; j < NC; ++j) {
      const uint32_t c = lig + G * j;
      if (c < D) {
        if (gk) gk[i * width + head + c] = narrow_to<T>(gz * qr[j]);
        acc[j] += gz * widen(kr[c]);
      }
    }
  }
  if (gq) {
#pragma unroll
    for (int j = 0; j < NC; ++j)
      if (lig + G * j < D) gq[d * width + head + lig + G * j] = narrow_to<T>(acc[j]);
  }
}

// The backward with dropout.  With ga_d = gout . v and w as in the forward:
//   gv = (a w) gout      ga = w ga_d      dot = sum_e a ga      gs = a (ga - dot)
// and gz, gq, gk as above.  Edges are taken G at a time: lane t of the group loads a and draws
// w for edge base + t, and both are handed round the group, so each sweep costs one Philox per
// (edge, head) like the forward.  A dropped edge has ga = 0: its v row is not read, its gv row
// is written as zeros, and it still takes its share -a dot of the softmax Jacobian.
template <class T, int G, int NC>
__global__ void block_attention_dropout_bwd(
    const int64_t* __restrict__ offsets, uint64_t items, uint32_t H, uint32_t D,
    const T* __restrict__ q, const T* __restrict__ k, const T* __restrict__ v,
    const float* __restrict__ att, float slope, Dropout dr, const T* __restrict__ gout,
    T* __restrict__ gq, T* __restrict__ gk, T* __restrict__ gv) {
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
        if (lig + G * j < D) gq[d * width + head + lig + G * j] = narrow_to<T>(0.f);
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
            if (lig + G * j < D) gv[i * width + head + lig + G * j] = narrow_to<T>(0.f);
        }
        continue;
      }
      if (gv) {
        const float aw = at * wt;
#pragma unroll
        for (int j = 0; j < NC; ++j) {
          const uint32_t c = lig + G * j;
          if (c < D) gv[i * width + head + c] = narrow_to<T>(aw * gr[j]);
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
      const T* kr = k + i * width + head;
      float ga = 0.f;
      if (wt != 0.f) ga = wt * head_dot<G, NC>(gr, v + i * width + head, D, lig);
      const float z = head_dot<G, NC>(qr, kr, D, lig);
      const float gs = at * (ga - dot);
      const float gz = z > 0.f ? gs : gs * slope;
#pragma unroll
      for (int j = 0; j < NC; ++j) {
        const uint32_t c = lig + G * j;
        if (c < D) {
          if (gk) gk[i * width + head + c] = narrow_to<T>(gz * qr[j]);
          acc[j] += gz * widen(kr[c]);
        }
      }
    }
  }
  if (gq) {
#pragma unroll
    for (int j = 0; j < NC; ++j)
      if (lig + G * j < D) gq[d * width + head + lig + G * j] = narrow_to<T>(acc[j]);
  }
}

template <class T>
struct Fwd {
  Shape s; const T *q, *k, *v; float slope; T* out; float* att; hipStream_t stream;
  template <int G, int NC> void operator()() {
    block_attention_fwd<T, G, NC><<<dim3(grid_of(s, G)), dim3(kThreads), 0, stream>>>(
        s.offsets, s.items, s.H, s.D, q, k, v, slope, out, att);
  }
};
template <class T>
struct Bwd {
  Shape s; const T *q, *k, *v; const float* att; float slope; const T* gout; T *gq, *gk, *gv;
  hipStream_t stream;
  template <int G, int NC> void operator()() {
    block_attention_bwd<T, G, NC><<<dim3(grid_of(s, G)), dim3(kThreads), 0, stream>>>(
        s.offsets, s.items, s.H, s.D, q, k, v, att, slope, gout, gq, gk, gv);
  }
};
template <class T>
struct DropoutFwd {
  Shape s; const T *q, *k, *v; float slope; Dropout dr; T* out; float *att, *att_dropped;
  hipStream_t stream;
  template <int G, int NC> void operator()() {
    block_attention_dropout_fwd<T, G, NC><<<dim3(grid_of(s, G)), dim3(kThreads), 0, stream>>>(
        s.offsets, s.items, s.H, s.D, q, k, v, slope, dr, out, att, att_dropped);
  }
};
template <class T>
struct DropoutBwd {
  Shape s; const T *q, *k, *v; const float* att; float slope; Dropout dr; const T* gout;
  T *gq, *gk, *gv; hipStream_t stream;
  template <int G, int NC> void operator()() {
    block_attention_dropout_bwd<T, G, NC><<<dim3(grid_of(s, G)), dim3(kThreads), 0, stream>>>(
        s.offsets, s.items, s.H, s.D, q, k, v, att, slope, dr, gout, gq, gk, gv);
  }
};

// The host side of the entry points below: the checks once, for both element types and with or
// without dropout (`dr` null: without).  The dropout entry points check p before they call in,
// so every message keeps its place in the order.
template <class T>
void forward(const int64_t* d_offsets, size_t num_dst, size_t num_edges, size_t heads,
             size_t head_dim, const T* d_q, const T* d_k, const T* d_v, float negative_slope,
             const Dropout* dr, T* d_out, float* d_att, float* d_att_dropped, int device,
             hipStream_t stream) {
  const Shape s = checked_shape(d_offsets, num_dst, heads, head_dim);
  if (num_dst == 0) return;
  GF_REQUIRE(d_q && d_out, "block_attention: null q or out");
  GF_REQUIRE(num_edges == 0 || (d_k && d_v && d_att), "block_attention: null k, v or att");
  DeviceGuard dg(device);
  if (dr)
    dispatch(s.D, DropoutFwd<T>{s, d_q, d_k, d_v, negative_slope, *dr, d_out, d_att,
                                d_att_dropped, stream});
  else
    dispatch(s.D, Fwd<T>{s, d_q, d_k, d_v, negative_slope, d_out, d_att, stream});
  GF_HIP(hipGetLastError());
}

template <class T>
void backward(const int64_t* d_offsets, size_t num_dst, size_t num_edges, size_t heads,
              size_t head_dim, const T* d_q, const T* d_k, const T* d_v, const float* d_att,
              float negative_slope, const Dropout* dr, const T* d_grad_out, T* d_grad_q,
              T* d_grad_k, T* d_grad_v, int device, hipStream_t stream) {
  const Shape s = checked_shape(d_offsets, num_dst, heads, head_dim);
  if (num_dst == 0 || (!d_grad_q && !d_grad_k && !d_grad_v)) return;
  GF_REQUIRE(d_grad_out != nullptr, "block_attention backward: null gradient");
  GF_REQUIRE(num_edges == 0 || (d_att && d_v), "block_attention backward: null att or v");
  GF_REQUIRE(num_edges == 0 || (!d_grad_q && !d_grad_k) || (d_q && d_k),
             "block_attention backward: grad_q / grad_k need q and k");
  if (num_edges == 0 && !d_grad_q) return;
  DeviceGuard dg(device);
  if (dr)
    dispatch(s.D, DropoutBwd<T>{s, d_q, d_k, d_v, d_att, negative_slope, *dr, d_grad_out,
                                d_grad_q, d_grad_k, d_grad_v, stream});
  else
    dispatch(s.D, Bwd<T>{s, d_q, d_k, d_v, d_att, negative_slope, d_grad_out, d_grad_q, d_grad_k,
                         d_grad_v, stream});
  GF_HIP(hipGetLastError());
}

}  // namespace

void block_attention_forward(const int64_t* d_offsets, size_t num_dst, size_t num_edges,
                             size_t heads, size_t head_dim, const float* d_q, const float* d_k,
                             const float* d_v, float negative_slope, float* d_out, float* d_att,
                             int device, hipStream_t stream) {
  forward(d_offsets, num_dst, num_edges, heads, head_dim, d_q, d_k, d_v, negative_slope, nullptr,
          d_out, d_att, nullptr, device, stream);
}

void block_attention_backward(const int64_t* d_offsets, size_t num_dst, size_t num_edges,
                              size_t heads, size_t head_dim, const float* d_q, const float* d_k,
                              const float* d_v, const float* d_att, float negative_slope,
                              const float* d_grad_out, float* d_grad_q, float* d_grad_k,
                              float* d_grad_v, int device, hipStream_t stream) {
  backward(d_offsets, num_dst, num_edges, heads, head_dim, d_q, d_k, d_v, d_att, negative_slope,
           nullptr, d_grad_out, d_grad_q, d_grad_k, d_grad_v, device, stream);
}

void block_attention_dropout_forward(const int64_t* d_offsets, size_t num_dst, size_t num_edges,
                                     size_t heads, size_t head_dim, const float* d_q,
                                     const float* d_k, const float* d_v, float negative_slope,
                                     float p, uint64_t seed, float* d_out, float* d_att,
                                     float* d_att_dropped, int device, hipStream_t stream) {
  const Dropout dr = checked_dropout(p, seed);
  forward(d_offsets, num_dst, num_edges, heads, head_dim, d_q, d_k, d_v, negative_slope, &dr,
          d_out, d_att, d_att_dropped, device, stream);
}

void block_attention_dropout_backward(const int64_t* d_offsets, size_t num_dst, size_t num_edges,
                                      size_t heads, size_t head_dim, const float* d_q,
                                      const float* d_k, const float* d_v, const float* d_att,
                                      float negative_slope, float p, uint64_t seed,
                                      const float* d_grad_out, float* d_grad_q, float* d_grad_k,
                                      float* d_grad_v, int device, hipStream_t stream) {
  const Dropout dr = checked_dropout(p, seed);
  backward(d_offsets, num_dst, num_edges, heads, head_dim, d_q, d_k, d_v, d_att, negative_slope,
           &dr, d_grad_out, d_grad_q, d_grad_k, d_grad_v, device, stream);
}

void block_attention_bf16_forward(const int64_t* d_offsets, size_t num_dst, size_t num_edges,
                                  size_t heads, size_t head_dim, const uint16_t* d_q,
                                  const uint16_t* d_k, const uint16_t* d_v, float negative_slope,
                                  uint16_t* d_out, float* d_att, int device, hipStream_t stream) {
  forward(d_offsets, num_dst, num_edges, heads, head_dim, d_q, d_k, d_v, negative_slope, nullptr,
          d_out, d_att, nullptr, device, stream);
}

void block_attention_bf16_backward(const int64_t* d_offsets, size_t num_dst, size_t num_edges,
                                   size_t heads, size_t head_dim, const uint16_t* d_q,
                                   const uint16_t* d_k, const uint16_t* d_v, const float* d_att,
                                   float negative_slope, const uint16_t* d_grad_out,
                                   uint16_t* d_grad_q, uint16_t* d_grad_k, uint16_t* d_grad_v,
                                   int device, hipStream_t stream) {
  backward(d_offsets, num_dst, num_edges, heads, head_dim, d_q, d_k, d_v, d_att, negative_slope,
           nullptr, d_grad_out, d_grad_q, d_grad_k, d_grad_v, device, stream);
}

void block_attention_dropout_bf16_forward(const int64_t* d_offsets, size_t num_dst,
                                          size_t num_edges, size_t heads, size_t head_dim,
                                          const uint16_t* d_q, const uint16_t* d_k,
                                          const uint16_t* d_v, float negative_slope, float p,
                                          uint64_t seed, uint16_t* d_out, float* d_att,
                                          float* d_att_dropped, int device, hipStream_t stream) {
  const Dropout dr = checked_dropout(p, seed);
  forward(d_offsets, num_dst, num_edges, heads, head_dim, d_q, d_k, d_v, negative_slope, &dr,
          d_out, d_att, d_att_dropped, device, stream);
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
  backward(d_offsets, num_dst, num_edges, heads, head_dim, d_q, d_k, d_v, d_att, negative_slope,
           &dr, d_grad_out, d_grad_q, d_grad_k, d_grad_v, device, stream);
}

}  // namespace gf
