// A node's newest interactions as one padded sequence, and the tokens a sequence model reads from
// it: for row i with node v = nodes[i], time t = ts[i] and, when `since` is given, lower end
// lo = since[i], with L = length,
//
//   seg[0 .. n)        = the window of v at (t, lo, L), as history_window.hpp defines it, oldest
//                        first; n <= L
//   lengths[i]         = n
//   nodes[i, p], eids[i, p], times[i, p] = seg[p].dst, seg[p].eid, seg[p].ts        p < n
//   delta_t[i, p]      = t - seg[p].ts, one float32 subtraction                     p < n
//   nodes, eids, times, delta_t [i, p]   = -1, -1, 0, 0                             p >= n
//   tokens[i, p, :]    = [E[seg[p].eid, :] | N[seg[p].dst, :] | te_cos(w[j], delta_t[i, p], b[j])]
//                        for p < n, +0.0 in every element for p >= n
//
// E[id, :] and N[id, :] are copies of the table's row, bit for bit, and zeros for an id without a
// row (negative, >= the table's rows); te_cos is time_encode.hip's expression
// (time_encode_expr.hpp).  A part that is not given has width 0; without any part there are no
// tokens.  Every element of every output is written.
//
// A wave takes a row at a time, four rows per workgroup, rows past the grid limit grid-strided.
// All lanes resolve the window together (the same addresses: one request).  Then
//
// - planes: the lanes stride over the L positions; a filled position reads its 32-byte record once
//   and writes the four planes, a position past n writes the padding, in the same loop;
// - tokens: a copy and a cosine, no reduction, so the lanes are spread over the flattened
//   (position, column) space of each part of the row: lane l takes chunks l, l + 64, ... of the
//   part's L * q chunks, chunk k being column k % q of position k / q (kept as a pair that is
//   advanced, not divided).  A chunk is a float4 when every part's width is a multiple of four
//   and the tables and the tokens are 16-byte aligned, one float otherwise.  At de = 16 a wave's
//   load instruction covers 16 positions, not one.  The table parts take kUnroll chunks per lane
//   at a time: the ids are read, then the kUnroll row loads are issued back to back, then they
//   are stored.  The time part has all 64 lanes in the cosine together.
//
// The id a chunk needs is RE-READ from its record (seg[p].eid or .dst; the planes loop has just
// brought those lines in, and the q chunks of a position share one), not staged: no LDS (0 bytes),
// no barrier, and waves of a workgroup never wait for one another.  One writer per output element,
// plain loads and stores, no atomics: the same inputs give the same bits.  Index arithmetic on
// [N, L, W] is 64-bit; inside a row L * W <= 512 * 3072 fits 32 bits.
#include "neighbor_sequence.hpp"
#include "common.hpp"
#include "feature_table.hpp"
#include "history_window.hpp"
#include "time_encode_expr.hpp"

namespace gf {
namespace {

static_assert(kSeqMaxLength == GF_SEQ_MAX_LENGTH && kSeqMaxWidth == GF_SEQ_MAX_WIDTH,
              "gnnflow_hip.h and neighbor_sequence.hpp disagree on the limits");

using namespace wave_per_row;                 // kThreads, kWave, kWaves, kMaxGrid
constexpr uint32_t kUnroll = 4;               // table chunks in flight per lane

struct Part {
  const float* feats;        // a table, or the encoder's weight; nullptr: the part is absent
  uint64_t rows;             // of a table
  uint32_t width;            // floats per position, 0 when absent
};

struct SequenceArgs {
  StoreView store;           // without a node: every row gets the empty answer
  const int64_t* nodes;
  const float* ts;
  const float* since;        // nullptr: no lower end
  uint64_t rows;
  uint32_t length;           // L, 1 .. kSeqMaxLength
  Part edge, node, time;     // rows indexed by a record's eid, by its dst; time.feats is w
  const float* bias;         // of the time part
  int32_t* lengths;          // [rows]
  int64_t* out_nodes;        // [rows, L]
  int64_t* eids;             // [rows, L]
  float* times;              // [rows, L]
  float* delta_t;            // [rows, L]
  float* tokens;             // [rows, L, W]; nullptr when no part is given
};

// columns j .. of the time part at delta dt
__device__ __forceinline__ void encode(float& a, const float* __restrict__ w,
                                       const float* __restrict__ b, uint32_t j, float dt) {
  a = te_cos(w[j], dt, b[j]);
}
__device__ __forceinline__ void encode(float4& a, const float* __restrict__ w,
                                       const float* __restrict__ b, uint32_t j, float dt) {
  a.x = te_cos(w[j], dt, b[j]);
  a.y = te_cos(w[j + 1], dt, b[j + 1]);
  a.z = te_cos(w[j + 2], dt, b[j + 2]);
  a.w = te_cos(w[j + 3], dt, b[j + 3]);
}

// A lane's walk over a part's flattened [L, q] chunks: it starts at chunk `lane` and advances by
// 64 chunks, as (position, column) pairs with column < q.
struct Hop {
  uint32_t q;                // chunks per position, 0: the part is absent
  uint32_t p0, c0;           // chunk `lane`
  uint32_t dp, dc;           // 64 chunks further; dc < q
};
struct Chunk {
  uint32_t p, c;
};

__device__ __forceinline__ Hop hop_of(uint32_t q, uint32_t lane) {
  if (q == 0) return {0, 0, 0, 0, 0};
  return {q, lane / q, lane % q, kWave / q, kWave % q};
}
__device__ __forceinline__ void advance(Chunk& k, const Hop& h) {
  k.p += h.dp;
  k.c += h.dc;               // < 2 q
  if (k.c >= h.q) {
    k.c -= h.q;
    ++k.p;
  }
}

// One table part of one row's tokens; V is the chunk type, kEid picks the id of a record.  `out`
// is the part's first chunk of the row's position 0, Q the chunks of a whole token.  Called by
// the whole wave with the same seg, n and L in every lane.
template <typename V, bool kEid>
__device__ __forceinline__ void copy_part(const EdgePair* __restrict__ seg, uint32_t n, uint32_t L,
                                          const Part& t, const Hop& h, V* __restrict__ out,
                                          uint32_t Q) {
  if (h.q == 0) return;
  const V* const tab = reinterpret_cast<const V*>(t.feats);
  const uint32_t total = L * h.q;
  Chunk k = {h.p0, h.c0};
  for (uint32_t done = 0; done < total; done += kWave * kUnroll) {      // uniform over the wave
    Chunk at[kUnroll];
    int64_t id[kUnroll];
    V v[kUnroll];
#pragma unroll
    for (uint32_t u = 0; u < kUnroll; ++u) {
      at[u] = k;
      advance(k, h);
      id[u] = -1;                                                     // padding: no row
      if (at[u].p < n) id[u] = kEid ? seg[at[u].p].eid : seg[at[u].p].dst;      // p < n: in seg
    }
#pragma unroll
    for (uint32_t u = 0; u < kUnroll; ++u) {
      clear(v[u]);
      if (id[u] >= 0 && static_cast<uint64_t>(id[u]) < t.rows)         // id < rows, c < q
        v[u] = tab[static_cast<uint64_t>(id[u]) * h.q + at[u].c];
    }
#pragma unroll
    for (uint32_t u = 0; u < kUnroll; ++u)
      if (at[u].p < L) out[static_cast<uint64_t>(at[u].p) * Q + at[u].c] = v[u];   // c < q <= Q
  }
}

// The time part of one row's tokens, `out` as in copy_part.
template <typename V>
__device__ __forceinline__ void time_part(const EdgePair* __restrict__ seg, uint32_t n, uint32_t L,
                                          float t, const float* __restrict__ w,
                                          const float* __restrict__ b, const Hop& h,
                                          V* __restrict__ out, uint32_t Q) {
  if (h.q == 0) return;
  constexpr uint32_t kV = sizeof(V) / sizeof(float);
  const uint32_t total = L * h.q;
  Chunk k = {h.p0, h.c0};
  for (uint32_t done = 0; done < total; done += kWave) {               // uniform over the wave
    if (k.p < L) {
      V v;
      clear(v);                                                       // padding: +0.0
      if (k.p < n) encode(v, w, b, k.c * kV, t - seg[k.p].ts);        // c * kV + kV <= width
      out[static_cast<uint64_t>(k.p) * Q + k.c] = v;
    }
    advance(k, h);
  }
}

template <typename V>
__global__ void __launch_bounds__(kThreads) neighbor_sequence_kernel(const SequenceArgs a) {
  constexpr uint32_t kV = sizeof(V) / sizeof(float);
  const uint32_t lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
  const uint32_t L = a.length;
  __builtin_assume(L != 0);      // 1 .. kSeqMaxLength: window_of's "no bound" is dead
  const uint32_t qe = a.edge.width / kV, qn = a.node.width / kV, qt = a.time.width / kV;
  const uint32_t Q = qe + qn + qt;
  const Hop he = hop_of(qe, lane), hn = hop_of(qn, lane), ht = hop_of(qt, lane);
  const uint64_t step = static_cast<uint64_t>(gridDim.x) * kWaves;
  for (uint64_t row = static_cast<uint64_t>(blockIdx.x) * kWaves + wave; row < a.rows;
       row += step) {                                          // uniform over the wave
    const float t = a.ts[row];
    const Window win = window_of(a.store, a.nodes[row], t, a.since, row, L);
    const uint32_t n = win.n;                                  // <= L, the same in every lane
    const uint64_t first = row * L;                            // the row's position 0 in the planes
    if (lane == 0) a.lengths[row] = static_cast<int32_t>(n);
    for (uint32_t p = lane; p < L; p += kWave) {
      int64_t z = -1, eid = -1;
      float tm = 0.0f, dt = 0.0f;
      if (p < n) {
        const EdgePair r = win.seg[p];                         // p < n: inside the window
        z = r.dst, eid = r.eid, tm = r.ts;
        dt = t - tm;
      }
      a.out_nodes[first + p] = z;
      a.eids[first + p] = eid;
      a.times[first + p] = tm;
      a.delta_t[first + p] = dt;
    }
    if (Q == 0) continue;
    V* const out = reinterpret_cast<V*>(a.tokens) + first * Q;
    copy_part<V, true>(win.seg, n, L, a.edge, he, out, Q);
    copy_part<V, false>(win.seg, n, L, a.node, hn, out + qe, Q);
    time_part<V>(win.seg, n, L, t, a.time.feats, a.bias, ht, out + qe + qn, Q);
  }
}

Part part_of(const std::string& w, const char* name, const float* feats, size_t rows,
             size_t width) {
  check_feature_table(w, name, feats, width, kSeqMaxWidth);
  if (feats == nullptr) return {nullptr, 0, 0};
  return {feats, rows, static_cast<uint32_t>(width)};
}

}  // namespace

void neighbor_sequence(const GraphView& g, const int64_t* d_nodes, const float* d_ts,
                       const float* d_since, size_t num_rows, size_t length,
                       const float* d_edge_feats, size_t edge_rows, size_t de,
                       const float* d_node_feats, size_t node_rows, size_t dn,
                       const float* d_weight, const float* d_bias, size_t dim_time,
                       int32_t* d_lengths, int64_t* d_out_nodes, int64_t* d_eids, float* d_times,
                       float* d_delta_t, float* d_tokens, int device, hipStream_t stream) {
  const std::string w("neighbor_sequence");
  GF_REQUIRE(num_rows < (size_t{1} << 31), w + ": 2^31 rows or more");
  // length is window_of's bound, and 0 there means "no bound": it must not get there
  GF_REQUIRE(length >= 1 && length <= kSeqMaxLength,
             w + ": length outside [1, " + std::to_string(kSeqMaxLength) + "]");
  const Part edge = part_of(w, "the edge table", d_edge_feats, edge_rows, de);
  const Part node = part_of(w, "the node table", d_node_feats, node_rows, dn);
  GF_REQUIRE((d_weight == nullptr) == (d_bias == nullptr),
             w + ": the time encoder's weight and bias are given together or not at all");
  const Part time = part_of(w, "the time encoder's weight", d_weight, 0, dim_time);
  if (num_rows == 0) return;
  GF_REQUIRE(d_nodes && d_ts, w + ": null nodes or ts");
  GF_REQUIRE(d_lengths && d_out_nodes && d_eids && d_times && d_delta_t,
             w + ": null lengths, nodes, eids, times or delta_t");
  const bool tokens = edge.width + node.width + time.width != 0;
  GF_REQUIRE(d_tokens != nullptr || !tokens, w + ": null tokens");
  SequenceArgs a = {store_view(g), d_nodes, d_ts, d_since, num_rows,
                    static_cast<uint32_t>(length), edge, node, time, d_bias, d_lengths,
                    d_out_nodes, d_eids, d_times, d_delta_t, tokens ? d_tokens : nullptr};
  const bool vec4 = tokens && de % 4 == 0 && dn % 4 == 0 && dim_time % 4 == 0 &&
                    aligned16(d_edge_feats) && aligned16(d_node_feats) && aligned16(d_tokens);
  DeviceGuard dg(device);
  const dim3 grid = strided_grid(num_rows, kWaves, kMaxGrid);
  if (vec4) neighbor_sequence_kernel<float4><<<grid, dim3(kThreads), 0, stream>>>(a);
  else neighbor_sequence_kernel<float><<<grid, dim3(kThreads), 0, stream>>>(a);
  GF_HIP(hipGetLastError());
}

}  // namespace gf
