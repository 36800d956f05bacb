// Fused GAT attention over a block: the message passing of dgl.nn.GATConv (the layer of the
// reference's static GAT model, gnnflow/models/gat.py:28-46) as ONE segment operation each way.
//
//   z[e,h]     = el[src(e),h] + er[d,h]             d = destination of edge e
//   s[e,h]     = z > 0 ? z : slope * z
//   a[e,h]     = softmax of s over the edges of d (max-subtracted)
//   out[d,h,:] = sum_e (a[e,h] * w[e,h]) * feat[src(e),h,:]     w = 1 without dropout
//
// src(e) = col[e], or num_dst + e when col is null (the sampler's layout, as segment_reduce_*).
// The score is a scalar per (edge, head) and the source row is both key and value, so the
// forward reads el / er as scalars and each feat row once.  The arithmetic is fp32 throughout.
//
// Work decomposition: that of block_attention.hip.  One (destination, head) pair per GROUP of G
// lanes (8, 16, 32 or 64, the smallest that covers a head's D columns; wider heads give each
// lane NC columns).  The lane-group helpers, head_dot(), the mask and the dispatch are that
// file's too, from block_attention_common.hpp.
//
// Forward: the scores need no feat, so pass 1 is lane-strided (lane i mod G takes edge i of the
// segment): score into att[], max.  Pass 2a sums the exponentials of the lane's own scores; pass
// 2b replaces them by a, G edges at a time, and hands each a round the group for the weighted
// sum.  Every att[] element is written and read back by the same lane: no fence.
//
// Backward: ONE sweep.  sum_e a ga = gout[d,h,:] . out[d,h,:] (also with dropout), so with the
// forward's out saved the softmax Jacobian's dot is one head_dot per (destination, head) and
// each feat row is read once.  z is recomputed by the forward's own single add (no contraction,
// no fast-math): both passes take the same side of the kink, slope at z == 0.
//   gfeat[src(e)] += (a w) gout[d]    ga = w (gout[d] . feat[src(e)])    gs = a (ga - dot)
//   gz = gs * (z > 0 ? 1 : slope)     gel[src(e)] += gz                  ger[d] = sum_e gz
// Sampler layout: every source row feeds exactly one edge, so gfeat and gel are plain stores, no
// atomics, bit-identical from run to run; the rows [0, num_dst) no edge reads are cleared by the
// entry point.  General col: a source may feed several edges; gfeat and gel accumulate with
// atomicAdd into buffers the entry point clears (as segment_reduce_bwd).  ger is a lane-strided
// sum and a butterfly, the same order every run, in both layouts.
//
// Dropout: the mask contract of block_attention.hip unchanged (edge i of the grouped order, head
// h kept <=> gf_philox4x32_10_first(seed, i * H + h, 0) >= T), drawn again by the backward.  A
// dropped edge's feat row is not read, forward or backward.  No LDS anywhere.
//
// bfloat16 (the *_bf16 kernels; bf16.hpp): feat, out and their gradients may be bfloat16.  el,
// er, att, the dropped attention and the gradients of el and er stay float32: under autocast el
// and er come out of a float32 sum, and they are [rows, H] only.  Every bfloat16 element is
// widened when it is loaded (exact; one 2-byte access per column, a lane owning the columns
// lig + G * j, which fixes the order of head_dot's sum), the arithmetic is the float32 kernels'
// own in the same order, and a bfloat16 result is rounded once, to nearest even, when it is
// stored.  Built with -ffp-contract=off and without fast-math, so
//
//   bf16 kernel(x)  ==  round_to_bf16(float32 kernel(widen(x)))      bit for bit.
//
// Two things differ from the float32 kernels, and keep the bodies apart.
//   * The backward takes the forward's out for dot = gout . out.  The rounded bfloat16 out would
//     give another dot than the float32 op's, so the forward also stores the UNROUNDED float32
//     out [num_dst, H, D] (out32; num_dst rows, not E) for the backward to read.
//   * With an explicit col a source may feed several edges and gfeat is accumulated with
//     atomicAdd.  The adds go to a caller-owned float32 scratch [num_src, H, D], the float32
//     kernel's own adds into its own zeros, which narrow_rows rounds to the bfloat16 gradient in
//     one launch.  The sampler's layout (col null) stores every row once, directly in bfloat16.
#include "block_attention_common.hpp"

#include <algorithm>

namespace gf {
namespace {

using bf16 = uint16_t;

struct GatShape {
  const int64_t* offsets;
  const int64_t* col;     // null: source of edge i = num_dst + i
  uint64_t num_dst, items;
  uint32_t H, D;
};

__device__ inline uint64_t source_of(const GatShape& s, int64_t i) {
  return s.col ? static_cast<uint64_t>(s.col[i]) : s.num_dst + static_cast<uint64_t>(i);
}

// DROP = false is the op without dropout (dr unused); att_dropped, unless null, then receives a.
template <int G, int NC, bool DROP>
__global__ void block_gat_fwd(GatShape sh, const float* __restrict__ feat,
                              const float* __restrict__ el, const float* __restrict__ er,
                              float slope, Dropout dr, float* __restrict__ out, float* att,
                              float* __restrict__ att_dropped) {
  const uint32_t lig = threadIdx.x & (G - 1);
  const uint64_t w = (static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x) / G;
  if (w >= sh.items) return;                  // group-uniform
  const uint32_t H = sh.H, D = sh.D;
  const uint64_t d = w / H;
  const uint32_t h = static_cast<uint32_t>(w - d * H);
  const int64_t b = sh.offsets[d], e = sh.offsets[d + 1];
  const uint64_t width = static_cast<uint64_t>(H) * D;
  const uint64_t head = static_cast<uint64_t>(h) * D;
  float* out_row = out + d * width + head;
  if (e <= b) {                               // no in-edges: exactly 0
#pragma unroll
    for (int j = 0; j < NC; ++j)
      if (lig + G * j < D) out_row[lig + G * j] = 0.f;
    return;
  }
  const float erd = er[d * H + h];

  // pass 1 (lane-strided, no feat): scores into att[], max
  float m = -FLT_MAX;
  for (int64_t i = b + lig; i < e; i += G) {
    const float s = leaky(el[source_of(sh, i) * H + h] + erd, slope);
    att[i * H + h] = s;
    m = fmaxf(m, s);
  }
  m = group_max<G>(m);
  // pass 2a: the lane's own scores -> sum of exponentials
  float l = 0.f;
  for (int64_t i = b + lig; i < e; i += G) l += __expf(att[i * H + h] - m);
  const float inv = 1.f / group_sum<G>(l);
  // pass 2b (reads feat once): a replaces the score, G edges at a time; the lane's copy becomes
  // a * w, or -1 for a dropped edge (a * w is never negative), and goes round the group
  float acc[NC];
#pragma unroll
  for (int j = 0; j < NC; ++j) acc[j] = 0.f;
  for (int64_t base = b; base < e; base += G) {
    const int64_t mine = base + lig;
    float a = 0.f;
    if (mine < e) {
      a = __expf(att[mine * H + h] - m) * inv;
      att[mine * H + h] = a;
      if (DROP) a = kept(dr, static_cast<uint64_t>(mine), H, h) ? a * dr.scale : -1.f;
      if (att_dropped) att_dropped[mine * H + h] = a < 0.f ? 0.f : a;
    }
    const int n = static_cast<int>(e - base < G ? e - base : G);
    for (int t = 0; t < n; ++t) {
      const float at = group_read<G>(a, t);
      if (DROP && at < 0.f) continue;         // dropped: exactly 0, feat not read (group-uniform)
      const float* fr = feat + source_of(sh, base + t) * width + head;
#pragma unroll
      for (int j = 0; j < NC; ++j) {
        const uint32_t c = lig + G * j;
        if (c < D) acc[j] += at * fr[c];
      }
    }
  }
#pragma unroll
  for (int j = 0; j < NC; ++j)
    if (lig + G * j < D) out_row[lig + G * j] = acc[j];
}

// One sweep, G edges at a time: lane t of the group loads a and draws w for edge base + t; both
// go round the group for gfeat and ga; ga comes back to lane t, which finishes gz for its own
// edge (gel) and adds it to its share of ger.  A null gfeat / gel / ger skips that output's
// work; feat is read only when gel or ger is wanted.  With col the gfeat / gel buffers arrive
// zeroed and are accumulated into; without, every row of an edge is stored exactly once (zeros
// for a dropped edge's gfeat row).
template <int G, int NC, bool DROP>
__global__ void block_gat_bwd(GatShape sh, const float* __restrict__ feat,
                              const float* __restrict__ el, const float* __restrict__ er,
                              const float* __restrict__ att, const float* __restrict__ out,
                              float slope, Dropout dr, const float* __restrict__ gout,
                              float* __restrict__ gfeat, float* __restrict__ gel,
                              float* __restrict__ ger) {
  const uint32_t lig = threadIdx.x & (G - 1);
  const uint64_t w = (static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x) / G;
  if (w >= sh.items) return;                  // group-uniform
  const uint32_t H = sh.H, D = sh.D;
  const uint64_t d = w / H;
  const uint32_t h = static_cast<uint32_t>(w - d * H);
  const int64_t b = sh.offsets[d], e = sh.offsets[d + 1];
  const uint64_t width = static_cast<uint64_t>(H) * D;
  const uint64_t head = static_cast<uint64_t>(h) * D;
  if (e <= b) {
    if (ger && lig == 0) ger[d * H + h] = 0.f;
    return;
  }
  float gr[NC];
  load_head<G, NC>(gr, gout + d * width + head, D, lig);
  const bool chain = gel || ger;
  float dot = 0.f, erd = 0.f;
  if (chain) {
    dot = head_dot<G, NC>(gr, out + d * width + head, D, lig);    // = sum_e a ga
    erd = er[d * H + h];
  }
  float gsum = 0.f;
  for (int64_t base = b; base < e; base += G) {
    const int64_t mine = base + lig;
    float a = 0.f, wm = 0.f;
    if (mine < e) {
      a = att[mine * H + h];
      if (DROP) wm = kept(dr, static_cast<uint64_t>(mine), H, h) ? dr.scale : 0.f;
    }
    const int n = static_cast<int>(e - base < G ? e - base : G);
    float my_ga = 0.f;
    for (int t = 0; t < n; ++t) {
      const float at = group_read<G>(a, t);
      const float wt = DROP ? group_read<G>(wm, t) : 1.f;   // scale >= 1, so 0 means dropped
      const uint64_t row = source_of(sh, base + t) * width + head;
      if (DROP && wt == 0.f) {                // ga = 0 exactly, feat not read
        if (gfeat && !sh.col) {
#pragma unroll
          for (int j = 0; j < NC; ++j)
            if (lig + G * j < D) gfeat[row + lig + G * j] = 0.f;
        }
        continue;
      }
      if (gfeat) {
        const float aw = DROP ? at * wt : at;
#pragma unroll
        for (int j = 0; j < NC; ++j) {
          const uint32_t c = lig + G * j;
          if (c < D) {
            if (sh.col) atomicAdd(&gfeat[row + c], aw * gr[j]);
            else gfeat[row + c] = aw * gr[j];
          }
        }
      }
      if (chain) {
        float ga = head_dot<G, NC>(gr, feat + row, D, lig);
        if (DROP) ga = wt * ga;
        if (lig == static_cast<uint32_t>(t)) my_ga = ga;
      }
    }
    if (chain && mine < e) {
      const uint64_t s = source_of(sh, mine) * H + h;
      const float z = el[s] + erd;
      const float gs = a * (my_ga - dot);
      const float gz = z > 0.f ? gs : gs * slope;
      if (gel) {
        if (sh.col) atomicAdd(&gel[s], gz);
        else gel[s] = gz;
      }
      gsum += gz;
    }
  }
  if (ger) {
    gsum = group_sum<G>(gsum);
    if (lig == 0) ger[d * H + h] = gsum;
  }
}

// The bfloat16 kernels are bodies of their own, not block_gat_fwd / _bwd over an element type:
// out32 and the split gfeat32 / gfeat16 are arguments the float32 kernels would have to take too.
//
// DROP = false is the op without dropout (dr unused); att_dropped, unless null, then receives a.
// out32, unless null, receives the sums before they are rounded.
template <int G, int NC, bool DROP>
__global__ void block_gat_fwd_bf16(GatShape sh, const bf16* __restrict__ feat,
                                   const float* __restrict__ el, const float* __restrict__ er,
                                   float slope, Dropout dr, bf16* __restrict__ out, float* att,
                                   float* __restrict__ att_dropped, float* __restrict__ out32) {
  const uint32_t lig = threadIdx.x & (G - 1);
  const uint64_t w = (static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x) / G;
  if (w >= sh.items) return;                  // group-uniform
  const uint32_t H = sh.H, D = sh.D;
  const uint64_t d = w / H;
  const uint32_t h = static_cast<uint32_t>(w - d * H);
  const int64_t b = sh.offsets[d], e = sh.offsets[d + 1];
  const uint64_t width = static_cast<uint64_t>(H) * D;
  const uint64_t head = static_cast<uint64_t>(h) * D;
  bf16* out_row = out + d * width + head;
  float* out32_row = out32 ? out32 + d * width + head : nullptr;
  if (e <= b) {                               // no in-edges: exactly 0
#pragma unroll
    for (int j = 0; j < NC; ++j)
      if (lig + G * j < D) {
        out_row[lig + G * j] = 0;
        if (out32_row) out32_row[lig + G * j] = 0.f;
      }
    return;
  }
  const float erd = er[d * H + h];

  // pass 1 (lane-strided, no feat): scores into att[], max
  float m = -FLT_MAX;
  for (int64_t i = b + lig; i < e; i += G) {
    const float s = leaky(el[source_of(sh, i) * H + h] + erd, slope);
    att[i * H + h] = s;
    m = fmaxf(m, s);
  }
  m = group_max<G>(m);
  // pass 2a: the lane's own scores -> sum of exponentials
  float l = 0.f;
  for (int64_t i = b + lig; i < e; i += G) l += __expf(att[i * H + h] - m);
  const float inv = 1.f / group_sum<G>(l);
  // pass 2b (reads feat once): a replaces the score, G edges at a time; the lane's copy becomes
  // a * w, or -1 for a dropped edge (a * w is never negative), and goes round the group
  float acc[NC];
#pragma unroll
  for (int j = 0; j < NC; ++j) acc[j] = 0.f;
  for (int64_t base = b; base < e; base += G) {
    const int64_t mine = base + lig;
    float a = 0.f;
    if (mine < e) {
      a = __expf(att[mine * H + h] - m) * inv;
      att[mine * H + h] = a;
      if (DROP) a = kept(dr, static_cast<uint64_t>(mine), H, h) ? a * dr.scale : -1.f;
      if (att_dropped) att_dropped[mine * H + h] = a < 0.f ? 0.f : a;
    }
    const int n = static_cast<int>(e - base < G ? e - base : G);
    for (int t = 0; t < n; ++t) {
      const float at = group_read<G>(a, t);
      if (DROP && at < 0.f) continue;         // dropped: exactly 0, feat not read (group-uniform)
      const bf16* fr = feat + source_of(sh, base + t) * width + head;
#pragma unroll
      for (int j = 0; j < NC; ++j) {
        const uint32_t c = lig + G * j;
        if (c < D) acc[j] += at * widen(fr[c]);
      }
    }
  }
#pragma unroll
  for (int j = 0; j < NC; ++j)
    if (lig + G * j < D) {
      out_row[lig + G * j] = narrow(acc[j]);
      if (out32_row) out32_row[lig + G * j] = acc[j];
    }
}

// block_gat_bwd on bfloat16 feat and gout.  gfeat32 (col != null): the zeroed float32 scratch,
// accumulated with atomicAdd; gfeat16 (col == null): the bfloat16 gradient, every edge's row
// stored once.  At most one of the two is non-null; both null skips that output's work.
template <int G, int NC, bool DROP>
__global__ void block_gat_bwd_bf16(GatShape sh, const bf16* __restrict__ feat,
                                   const float* __restrict__ el, const float* __restrict__ er,
                                   const float* __restrict__ att, const float* __restrict__ out32,
                                   float slope, Dropout dr, const bf16* __restrict__ gout,
                                   float* __restrict__ gfeat32, bf16* __restrict__ gfeat16,
                                   float* __restrict__ gel, float* __restrict__ ger) {
  const uint32_t lig = threadIdx.x & (G - 1);
  const uint64_t w = (static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x) / G;
  if (w >= sh.items) return;                  // group-uniform
  const uint32_t H = sh.H, D = sh.D;
  const uint64_t d = w / H;
  const uint32_t h = static_cast<uint32_t>(w - d * H);
  const int64_t b = sh.offsets[d], e = sh.offsets[d + 1];
  const uint64_t width = static_cast<uint64_t>(H) * D;
  const uint64_t head = static_cast<uint64_t>(h) * D;
  if (e <= b) {
    if (ger && lig == 0) ger[d * H + h] = 0.f;
    return;
  }
  float gr[NC];
  load_head<G, NC>(gr, gout + d * width + head, D, lig);
  const bool chain = gel || ger;
  float dot = 0.f, erd = 0.f;
  if (chain) {
    dot = head_dot<G, NC>(gr, out32 + d * width + head, D, lig);    // = sum_e a ga
    erd = er[d * H + h];
  }
  float gsum = 0.f;
  for (int64_t base = b; base < e; base += G) {
    const int64_t mine = base + lig;
    float a = 0.f, wm = 0.f;
    if (mine < e) {
      a = att[mine * H + h];
      if (DROP) wm = kept(dr, static_cast<uint64_t>(mine), H, h) ? dr.scale : 0.f;
    }
    const int n = static_cast<int>(e - base < G ? e - base : G);
    float my_ga = 0.f;
    for (int t = 0; t < n; ++t) {
      const float at = group_read<G>(a, t);
      const float wt = DROP ? group_read<G>(wm, t) : 1.f;   // scale >= 1, so 0 means dropped
      const uint64_t row = source_of(sh, base + t) * width + head;
      if (DROP && wt == 0.f) {                // ga = 0 exactly, feat not read
        if (gfeat16) {
#pragma unroll
          for (int j = 0; j < NC; ++j)
            if (lig + G * j < D) gfeat16[row + lig + G * j] = 0;
        }
        continue;
      }
      if (gfeat32 || gfeat16) {
        const float aw = DROP ? at * wt : at;
#pragma unroll
        for (int j = 0; j < NC; ++j) {
          const uint32_t c = lig + G * j;
          if (c < D) {
            if (gfeat32) atomicAdd(&gfeat32[row + c], aw * gr[j]);
            else gfeat16[row + c] = narrow(aw * gr[j]);
          }
        }
      }
      if (chain) {
        float ga = head_dot<G, NC>(gr, feat + row, D, lig);
        if (DROP) ga = wt * ga;
        if (lig == static_cast<uint32_t>(t)) my_ga = ga;
      }
    }
    if (chain && mine < e) {
      const uint64_t s = source_of(sh, mine) * H + h;
      const float z = el[s] + erd;
      const float gs = a * (my_ga - dot);
      const float gz = z > 0.f ? gs : gs * slope;
      if (gel) {
        if (sh.col) atomicAdd(&gel[s], gz);
        else gel[s] = gz;
      }
      gsum += gz;
    }
  }
  if (ger) {
    gsum = group_sum<G>(gsum);
    if (lig == 0) ger[d * H + h] = gsum;
  }
}

inline dim3 grid_for(const GatShape& s, int G) {
  return dim3(static_cast<unsigned>((s.items * G + kThreads - 1) / kThreads));
}

struct Fwd {
  GatShape s; const float *feat, *el, *er; float slope; Dropout dr; bool drop;
  float *out, *att, *att_dropped; hipStream_t stream;
  template <int G, int NC> void operator()() {
    if (drop)
      block_gat_fwd<G, NC, true><<<grid_for(s, G), dim3(kThreads), 0, stream>>>(
          s, feat, el, er, slope, dr, out, att, att_dropped);
    else
      block_gat_fwd<G, NC, false><<<grid_for(s, G), dim3(kThreads), 0, stream>>>(
          s, feat, el, er, slope, dr, out, att, att_dropped);
  }
};
struct Bwd {
  GatShape s; const float *feat, *el, *er, *att, *out; float slope; Dropout dr; bool drop;
  const float* gout; float *gfeat, *gel, *ger; hipStream_t stream;
  template <int G, int NC> void operator()() {
    if (drop)
      block_gat_bwd<G, NC, true><<<grid_for(s, G), dim3(kThreads), 0, stream>>>(
          s, feat, el, er, att, out, slope, dr, gout, gfeat, gel, ger);
    else
      block_gat_bwd<G, NC, false><<<grid_for(s, G), dim3(kThreads), 0, stream>>>(
          s, feat, el, er, att, out, slope, dr, gout, gfeat, gel, ger);
  }
};

struct FwdBf16 {
  GatShape s; const bf16* feat; const float *el, *er; float slope; Dropout dr; bool drop;
  bf16* out; float *att, *att_dropped, *out32; hipStream_t stream;
  template <int G, int NC> void operator()() {
    if (drop)
      block_gat_fwd_bf16<G, NC, true><<<grid_for(s, G), dim3(kThreads), 0, stream>>>(
          s, feat, el, er, slope, dr, out, att, att_dropped, out32);
    else
      block_gat_fwd_bf16<G, NC, false><<<grid_for(s, G), dim3(kThreads), 0, stream>>>(
          s, feat, el, er, slope, dr, out, att, att_dropped, out32);
  }
};
struct BwdBf16 {
  GatShape s; const bf16* feat; const float *el, *er, *att, *out32; float slope; Dropout dr;
  bool drop; const bf16* gout; float* gfeat32; bf16* gfeat16; float *gel, *ger;
  hipStream_t stream;
  template <int G, int NC> void operator()() {
    if (drop)
      block_gat_bwd_bf16<G, NC, true><<<grid_for(s, G), dim3(kThreads), 0, stream>>>(
          s, feat, el, er, att, out32, slope, dr, gout, gfeat32, gfeat16, gel, ger);
    else
      block_gat_bwd_bf16<G, NC, false><<<grid_for(s, G), dim3(kThreads), 0, stream>>>(
          s, feat, el, er, att, out32, slope, dr, gout, gfeat32, gfeat16, gel, ger);
  }
};

GatShape checked_gat_shape(const int64_t* d_offsets, size_t num_dst, size_t num_edges,
                           const int64_t* d_col, size_t num_src, size_t heads, size_t head_dim) {
  GF_REQUIRE(heads >= 1 && head_dim >= 1, "block_gat: heads and head_dim must be >= 1");
  GF_REQUIRE(heads <= kBlockAttentionMaxWidth && head_dim <= kBlockAttentionMaxWidth &&
                 heads * head_dim <= kBlockAttentionMaxWidth,
             "block_gat: heads * head_dim exceeds GF_BLOCK_ATTENTION_MAX_WIDTH (1024)");
  static_assert(kBlockAttentionMaxWidth <= 64 * kMaxChunks, "a head must fit one group");
  GF_REQUIRE(d_offsets != nullptr, "block_gat: null offsets");
  GF_REQUIRE(d_col != nullptr || num_src == num_dst + num_edges,
             "block_gat: without col, num_src must be num_dst + num_edges");
  // one group of up to 64 lanes per (destination, head): the grid stays below 2^31 blocks
  GF_REQUIRE(num_dst <= (size_t{1} << 32) / heads, "block_gat: too many destinations");
  return GatShape{d_offsets, d_col, static_cast<uint64_t>(num_dst),
                  static_cast<uint64_t>(num_dst) * heads, static_cast<uint32_t>(heads),
                  static_cast<uint32_t>(head_dim)};
}

// T and 1 / (1 - p) of the mask definition (gnnflow_hip.h); p is an fp32 value in [0, 1)
Dropout checked_gat_dropout(float p, uint64_t seed) {
  GF_REQUIRE(p >= 0.f && p < 1.f, "block_gat: dropout p must be in [0, 1)");   // NaN fails
  return Dropout{static_cast<uint32_t>(static_cast<double>(p) * 4294967296.0), 1.0f / (1.0f - p),
                 seed};
}

}  // namespace

void block_gat_forward(const int64_t* d_offsets, size_t num_dst, size_t num_edges,
                       const int64_t* d_col, size_t num_src, size_t heads, size_t head_dim,
                       const float* d_feat, const float* d_el, const float* d_er,
                       float negative_slope, float p, uint64_t seed, float* d_out, float* d_att,
                       float* d_att_dropped, int device, hipStream_t stream) {
  const Dropout dr = checked_gat_dropout(p, seed);
  const GatShape s =
      checked_gat_shape(d_offsets, num_dst, num_edges, d_col, num_src, heads, head_dim);
  if (num_dst == 0) return;
  GF_REQUIRE(d_er && d_out, "block_gat: null er or out");
  GF_REQUIRE(num_edges == 0 || (d_feat && d_el && d_att), "block_gat: null feat, el or att");
  DeviceGuard dg(device);
  dispatch(s.D, Fwd{s, d_feat, d_el, d_er, negative_slope, dr, p > 0.f, d_out, d_att,
                    d_att_dropped, stream});
  GF_HIP(hipGetLastError());
}

void block_gat_backward(const int64_t* d_offsets, size_t num_dst, size_t num_edges,
                        const int64_t* d_col, size_t num_src, size_t heads, size_t head_dim,
                        const float* d_feat, const float* d_el, const float* d_er,
                        const float* d_att, const float* d_out, float negative_slope, float p,
                        uint64_t seed, const float* d_grad_out, float* d_grad_feat,
                        float* d_grad_el, float* d_grad_er, int device, hipStream_t stream) {
  const Dropout dr = checked_gat_dropout(p, seed);
  const GatShape s =
      checked_gat_shape(d_offsets, num_dst, num_edges, d_col, num_src, heads, head_dim);
  if (!d_grad_feat && !d_grad_el && !d_grad_er) return;
  DeviceGuard dg(device);
  // general blocks accumulate into zeros; the sampler layout stores every edge's row exactly
  // once, so only the rows of the destination nodes themselves are cleared
  const size_t rows = d_col ? num_src : std::min(num_dst, num_src);
  if (rows && d_grad_feat)
    GF_HIP(hipMemsetAsync(d_grad_feat, 0, rows * heads * head_dim * sizeof(float), stream));
  if (rows && d_grad_el) GF_HIP(hipMemsetAsync(d_grad_el, 0, rows * heads * sizeof(float), stream));
  if (num_dst == 0) return;
  GF_REQUIRE(d_grad_out != nullptr, "block_gat backward: null gradient");
  GF_REQUIRE(num_edges == 0 || d_att, "block_gat backward: null att");
  GF_REQUIRE(num_edges == 0 || (!d_grad_el && !d_grad_er) || (d_feat && d_el && d_er && d_out),
             "block_gat backward: grad_el / grad_er need feat, el, er and out");
  if (num_edges == 0 && !d_grad_er) return;
  dispatch(s.D, Bwd{s, d_feat, d_el, d_er, d_att, d_out, negative_slope, dr, p > 0.f,
                    d_grad_out, d_grad_feat, d_grad_el, d_grad_er, stream});
  GF_HIP(hipGetLastError());
}

void block_gat_bf16_forward(const int64_t* d_offsets, size_t num_dst, size_t num_edges,
                            const int64_t* d_col, size_t num_src, size_t heads, size_t head_dim,
                            const uint16_t* d_feat, const float* d_el, const float* d_er,
                            float negative_slope, float p, uint64_t seed, uint16_t* d_out,
                            float* d_att, float* d_att_dropped, float* d_out_f32, int device,
                            hipStream_t stream) {
  const Dropout dr = checked_gat_dropout(p, seed);
  const GatShape s =
      checked_gat_shape(d_offsets, num_dst, num_edges, d_col, num_src, heads, head_dim);
  if (num_dst == 0) return;
  GF_REQUIRE(d_er && d_out, "block_gat: null er or out");
  GF_REQUIRE(num_edges == 0 || (d_feat && d_el && d_att), "block_gat: null feat, el or att");
  DeviceGuard dg(device);
  dispatch(s.D, FwdBf16{s, d_feat, d_el, d_er, negative_slope, dr, p > 0.f, d_out, d_att,
                    d_att_dropped, d_out_f32, stream});
  GF_HIP(hipGetLastError());
}

void block_gat_bf16_backward(const int64_t* d_offsets, size_t num_dst, size_t num_edges,
                             const int64_t* d_col, size_t num_src, size_t heads, size_t head_dim,
                             const uint16_t* d_feat, const float* d_el, const float* d_er,
                             const float* d_att, const float* d_out_f32, float negative_slope,
                             float p, uint64_t seed, const uint16_t* d_grad_out,
                             uint16_t* d_grad_feat, float* d_grad_el, float* d_grad_er,
                             float* d_scratch, int device, hipStream_t stream) {
  const Dropout dr = checked_gat_dropout(p, seed);
  const GatShape s =
      checked_gat_shape(d_offsets, num_dst, num_edges, d_col, num_src, heads, head_dim);
  if (!d_grad_feat && !d_grad_el && !d_grad_er) return;
  DeviceGuard dg(device);
  const size_t width = heads * head_dim;
  const bool via_scratch = d_col && d_grad_feat && num_src;
  GF_REQUIRE(!via_scratch || d_scratch, "block_gat backward: col needs the float32 scratch");
  // general blocks accumulate into zeros (the scratch, all of it); the sampler layout stores
  // every edge's row exactly once, so only the rows of the destination nodes are cleared
  const size_t rows = d_col ? num_src : std::min(num_dst, num_src);
  if (via_scratch) GF_HIP(hipMemsetAsync(d_scratch, 0, num_src * width * sizeof(float), stream));
  else if (rows && d_grad_feat)
    GF_HIP(hipMemsetAsync(d_grad_feat, 0, rows * width * sizeof(uint16_t), stream));
  if (rows && d_grad_el) GF_HIP(hipMemsetAsync(d_grad_el, 0, rows * heads * sizeof(float), stream));
  const auto finish = [&] {
    if (via_scratch) narrow_rows(d_scratch, d_grad_feat, num_src * width, stream);
  };
  if (num_dst == 0) return finish();
  GF_REQUIRE(d_grad_out != nullptr, "block_gat backward: null gradient");
  GF_REQUIRE(num_edges == 0 || d_att, "block_gat backward: null att");
  GF_REQUIRE(num_edges == 0 || (!d_grad_el && !d_grad_er) ||
                 (d_feat && d_el && d_er && d_out_f32),
             "block_gat backward: grad_el / grad_er need feat, el, er and out");
  if (num_edges == 0 && !d_grad_er) return finish();
  dispatch(s.D, BwdBf16{s, d_feat, d_el, d_er, d_att, d_out_f32, negative_slope, dr, p > 0.f,
                    d_grad_out, via_scratch ? d_scratch : nullptr,
                    via_scratch ? nullptr : d_grad_feat, d_grad_el, d_grad_er, stream});
  GF_HIP(hipGetLastError());
  finish();
}

}  // namespace gf
