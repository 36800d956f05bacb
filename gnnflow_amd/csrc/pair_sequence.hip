// The two padded histories of a pair with their co-occurrence counts, time deltas and finished
// feature channels: for row i with source s = src[i], destination d = dst[i], time t = ts[i] and,
// when `since` is given, lo = since[i], with L = length (slots per side, 2 .. 512),
//
//   W(v)     = the considered records of v at (t, lo, L - 1) as history_window.hpp defines them,
//              oldest first, n(v) = |W(v)| <= L - 1
//   seq(v)   = [v itself] + W(v).dst                         len(v) = 1 + n(v) <= L
//   lengths, nodes, eids, times, counts = neighbor_cooccurrence.hip's with the self slot: the
//              self slot is position 0 with eid -1 and time t and is counted; the padding is
//              -1, -1, 0, (0, 0)
//   delta_t[i, side, p]  = t - times[i, side, p], one float32 subtraction, on a filled slot (the
//              self slot: t - t); +0.0 in the padding
//   node[i, side, p, :]  = N[nodes[i, side, p], :]           the self slot: the node's own row
//   edge[i, side, p, :]  = E[eids[i, side, p], :]            the self slot: eid -1, the zero row
//   time[i, side, p, j]  = te_cos(w[j], delta_t[i, side, p], b[j])      the self slot as any other
//              and +0.0 in every element of a padded slot of the three parts
//
// N[id, :] and E[id, :] are copies of the table's row, bit for bit, and zeros for an id without a
// row (negative, >= the table's rows); te_cos is time_encode.hip's expression
// (time_encode_expr.hpp).  Each part is its own contiguous tensor [N, 2, L, width]; a part that is
// not given is not touched.  Every element of the six planes and of the given parts is written.
//
// Geometry, table and phases are neighbor_cooccurrence.hip's (see there for the table's sizing and
// the occupancy): an open-addressing table in LDS keyed by the 64-bit node id
// (lds_id_table.hpp), `cap` = the power of two >= 4L slots in use, three instantiations by L
//   L <=  32:  128 slots,  2 048 B a row, a wave per row, 4 rows =  8 192 B a workgroup
//   L <= 128:  512 slots,  8 192 B a row, a wave per row, 4 rows = 32 768 B a workgroup
//   L <= 512: 2048 slots, 32 768 B a row, 4 waves on one row     = 32 768 B a workgroup
// and per row clear, insert, emit, each closed by phase_end: a workgroup-scope fence where a wave
// owns its row, __syncthreads() in the largest bucket, where the row loop has the same trip count
// in every wave of the workgroup (the row depends on blockIdx alone) and nothing in the loop body
// leaves it early: no barrier sits in a loop whose trip count differs between the waves it joins.
// The emit loop writes the six planes.
//
// The parts come after the emit's phase_end and need no table: a wave that is done with its share
// goes on to the next row's clear, which cannot overtake a reader of the table because every
// reader is behind that phase_end.  The row's TPR threads (64 or 256) are spread over the
// flattened (side, position, column) chunks of each part: thread r takes chunks r, r + TPR, ... of
// the part's 2L * q chunks, chunk k being column k % q of slot k / q, kept as a (slot, column) pair
// that is advanced, not divided.  The part is contiguous, so chunk k of the row is also element k
// of the row's output: consecutive threads store consecutive chunks.  A chunk is a float4 when the
// part's width is a multiple of four and its table and output are 16-byte aligned, one float
// otherwise, decided per part.  The table parts take kUnroll chunks per thread at a time: the ids
// are read, then the kUnroll row loads are issued back to back, then they are stored.  The id a
// chunk needs is RE-READ from its 32-byte record (the emit loop has just brought those lines in),
// not staged.  Slot 0 of a side is the self slot: the id is the node for the node part, no row for
// the edge part, and t - t for the time part.
//
// Hop, copy_part and time_part restate neighbor_sequence.hip's for a stride of TPR, two windows
// and the self slot; they are a second copy, so that kernel's device code is untouched.  One
// writer per output element, plain loads and stores, no atomics on global memory: the same inputs
// give the same bits.  Index arithmetic on [N, 2, L, d] is 64-bit; inside a row 2L * d <=
// 1024 * 1024 fits 32 bits.
#include "pair_sequence.hpp"
#include "common.hpp"
#include "feature_table.hpp"
#include "history_window.hpp"
#include "lds_id_table.hpp"
#include "time_encode_expr.hpp"

namespace gf {
namespace {

static_assert(kPairSeqMaxLength == GF_PAIRSEQ_MAX_LENGTH &&
                  kPairSeqMaxWidth == GF_PAIRSEQ_MAX_WIDTH,
              "gnnflow_hip.h and pair_sequence.hpp disagree on the limits");

constexpr int kThreads = 256;
constexpr int kWave = kIdTableWave;
constexpr uint32_t kMaxGrid = 4096;      // workgroups; the rows past a pass are grid-strided
constexpr uint32_t kUnroll = 4;          // table chunks in flight per thread

struct Part {
  const float* feats;        // a table, or the encoder's weight; nullptr: the part is absent
  uint64_t rows;             // of a table
  uint32_t width;            // floats per slot, 0 when absent
  uint32_t vec4;             // chunks are float4: width % 4 == 0, table and output aligned
  float* out;                // [rows, 2, L, width]
};

struct PairSeqArgs {
  StoreView store;
  const int64_t* src;
  const int64_t* dst;
  const float* ts;
  const float* since;        // nullptr: no lower end
  uint64_t rows;
  uint32_t length;           // L, 2 .. kPairSeqMaxLength
  uint32_t cap;              // slots in use: the power of two >= 4 * length
  uint32_t shift;            // 64 - log2(cap)
  Part node, edge, time;     // rows indexed by a slot's node, by its eid; time.feats is w
  const float* bias;         // of the time part
  int32_t* lengths;          // [rows, 2]
  int64_t* nodes;            // [rows, 2, L]
  int64_t* eids;             // [rows, 2, L]
  float* times;              // [rows, 2, L]
  float* delta_t;            // [rows, 2, L]
  int2* counts;              // [rows, 2, L] pairs (a, b)
};

template <int CAP>
struct Table {
  int64_t key[CAP];
  uint32_t a[CAP];
  uint32_t b[CAP];
};

// what the parts know of a row: both windows, the two ends and the time
struct PairRow {
  Window A, B;
  int64_t s, d;
  float t;
  uint32_t L;
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

// A thread's walk over a part's flattened [2L, q] chunks: it starts at chunk `rl`, its place among
// the row's TPR threads, and advances by TPR chunks, as (slot, column) pairs with column < q.
struct Hop {
  uint32_t q;                // chunks per slot, 0: the part is absent
  uint32_t x0, c0;           // chunk `rl`
  uint32_t dx, dc;           // TPR chunks further; dc < q
};
struct Chunk {
  uint32_t x, c;             // slot side * L + p, column
};

template <int TPR>
__device__ __forceinline__ Hop hop_of(const Part& t, uint32_t rl) {
  const uint32_t q = t.vec4 ? t.width / 4 : t.width;
  if (q == 0) return {0, 0, 0, 0, 0};
  return {q, rl / q, rl % q, TPR / q, TPR % q};
}
__device__ __forceinline__ void advance(Chunk& k, const Hop& h) {
  k.x += h.dx;
  k.c += h.dc;               // < 2 q
  if (k.c >= h.q) {
    k.c -= h.q;
    ++k.x;
  }
}

// The id of slot x of the row for a table part (kEid: the edge id), -1 where the slot has no row:
// the padding, a slot past 2L, the self slot's eid.  x >= L is side 1; a slot past 2L has
// p - 1 >= L - 1 >= n and reads nothing.
template <bool kEid>
__device__ __forceinline__ int64_t id_of(const PairRow& r, uint32_t x) {
  const bool side = x >= r.L;
  const uint32_t p = side ? x - r.L : x;
  const Window& w = side ? r.B : r.A;
  if (p == 0) return kEid ? -1 : (side ? r.d : r.s);
  if (p - 1 < w.n) return kEid ? w.seg[p - 1].eid : w.seg[p - 1].dst;      // inside the window
  return -1;
}

// One table part of one row; V is the chunk type, kEid picks the id of a slot.  `out` is the
// part's first chunk of the row.  Called by all TPR threads of the row with the same r.
template <typename V, bool kEid, int TPR>
__device__ __forceinline__ void copy_part(const PairRow& r, const Part& t, const Hop& h,
                                          uint32_t rl, V* __restrict__ out) {
  const V* const tab = reinterpret_cast<const V*>(t.feats);
  const uint32_t total = 2 * r.L * h.q;
  Chunk k = {h.x0, h.c0};
  for (uint32_t at0 = rl; at0 < total; at0 += TPR * kUnroll) {
    Chunk at[kUnroll];
    int64_t id[kUnroll];
    V v[kUnroll];
#pragma unroll
    for (uint32_t u = 0; u < kUnroll; ++u) {
      at[u] = k;
      advance(k, h);
      id[u] = id_of<kEid>(r, at[u].x);
    }
#pragma unroll
    for (uint32_t u = 0; u < kUnroll; ++u) {
      clear(v[u]);
      if (id[u] >= 0 && static_cast<uint64_t>(id[u]) < t.rows)         // id < rows, c < q
        v[u] = tab[static_cast<uint64_t>(id[u]) * h.q + at[u].c];
    }
#pragma unroll
    for (uint32_t u = 0; u < kUnroll; ++u)
      if (at0 + u * TPR < total) out[at0 + u * TPR] = v[u];           // chunk at[u] of the row
  }
}

// The time part of one row, `out` as in copy_part.
template <typename V, int TPR>
__device__ __forceinline__ void time_part(const PairRow& r, const float* __restrict__ w,
                                          const float* __restrict__ b, const Hop& h, uint32_t rl,
                                          V* __restrict__ out) {
  constexpr uint32_t kV = sizeof(V) / sizeof(float);
  const uint32_t total = 2 * r.L * h.q;
  Chunk k = {h.x0, h.c0};
  for (uint32_t at = rl; at < total; at += TPR) {      // at < total: k.x < 2L
    const bool side = k.x >= r.L;
    const uint32_t p = side ? k.x - r.L : k.x;
    const Window& win = side ? r.B : r.A;
    V v;
    clear(v);                                                         // padding: +0.0
    if (p == 0) encode(v, w, b, k.c * kV, r.t - r.t);                 // c * kV + kV <= width
    else if (p - 1 < win.n) encode(v, w, b, k.c * kV, r.t - win.seg[p - 1].ts);
    out[at] = v;
    advance(k, h);
  }
}

// a table part with the chunk type its Part was given
template <bool kEid, int TPR>
__device__ __forceinline__ void table_part(const PairRow& r, const Part& t, const Hop& h,
                                           uint32_t rl, uint64_t first) {
  if (h.q == 0) return;
  if (t.vec4)
    copy_part<float4, kEid, TPR>(r, t, h, rl, reinterpret_cast<float4*>(t.out) + first * h.q);
  else
    copy_part<float, kEid, TPR>(r, t, h, rl, t.out + first * h.q);
}

template <int CAP, int TPR>
__global__ void __launch_bounds__(kThreads) pair_sequence_kernel(const PairSeqArgs a) {
  constexpr int kRows = kThreads / TPR;      // rows a workgroup works on at a time
  static_assert(TPR % kWave == 0 && kThreads % TPR == 0, "whole waves on a row");
  __shared__ Table<CAP> tables[kRows];
  Table<CAP>& tb = tables[threadIdx.x / TPR];
  const uint32_t rl = threadIdx.x % TPR;      // the thread's place among those of its row
  const uint32_t L = a.length, cap = a.cap, shift = a.shift;
  const uint32_t H = L - 1;
  __builtin_assume(H != 0);      // 1 .. kPairSeqMaxLength - 1: window_of's "no bound" is dead
  const Hop hn = hop_of<TPR>(a.node, rl), he = hop_of<TPR>(a.edge, rl),
            ht = hop_of<TPR>(a.time, rl);
  const uint64_t step = static_cast<uint64_t>(gridDim.x) * kRows;
  for (uint64_t row = static_cast<uint64_t>(blockIdx.x) * kRows + threadIdx.x / TPR; row < a.rows;
       row += step) {      // uniform over the row's waves; over the workgroup when kRows == 1
    const float t = a.ts[row];
    const int64_t s = a.src[row], d = a.dst[row];
    const Window A = window_of(a.store, s, t, a.since, row, H);
    const Window B = window_of(a.store, d, t, a.since, row, H);
    const uint32_t len_a = 1 + A.n, len_b = 1 + B.n;      // <= L
    const uint64_t out = row * 2 * L;      // the row's first slot in the planes and the parts
    if (rl == 0) {
      a.lengths[row * 2] = static_cast<int32_t>(len_a);
      a.lengths[row * 2 + 1] = static_cast<int32_t>(len_b);
    }

    for (uint32_t x = rl; x < cap; x += TPR) {
      tb.key[x] = kIdEmpty;
      tb.a[x] = tb.b[x] = 0;
    }
    phase_end<TPR>();

    for (uint32_t p = rl; p < A.n; p += TPR) {
      const int64_t z = A.seg[p].dst;
      if (z < 0) continue;
      const uint32_t h = claim(tb, z, cap, shift);
      if (h < cap) atomicAdd(&tb.a[h], 1u);
    }
    for (uint32_t p = rl; p < B.n; p += TPR) {
      const int64_t z = B.seg[p].dst;
      if (z < 0) continue;
      const uint32_t h = claim(tb, z, cap, shift);
      if (h < cap) atomicAdd(&tb.b[h], 1u);
    }
    if (rl < 2) {      // the self slots: s on its own side, d on its own
      const int64_t z = rl == 0 ? s : d;
      if (z >= 0) {
        const uint32_t h = claim(tb, z, cap, shift);
        if (h < cap) atomicAdd(rl == 0 ? &tb.a[h] : &tb.b[h], 1u);
      }
    }
    phase_end<TPR>();

    for (uint32_t x = rl; x < 2 * L; x += TPR) {
      const bool side = x >= L;
      const uint32_t p = side ? x - L : x;
      const Window& w = side ? B : A;
      int64_t z = -1, eid = -1;
      float tm = 0.0f, dt = 0.0f;
      if (p < 1 + w.n) {
        if (p == 0) {
          z = side ? d : s;
          tm = t;
        } else {
          const EdgePair r = w.seg[p - 1];      // p - 1 < w.n: inside the window
          z = r.dst, eid = r.eid, tm = r.ts;
        }
        dt = t - tm;
      }
      int2 c = make_int2(0, 0);
      if (z >= 0) {
        const uint32_t h = find(tb, z, cap, shift);
        if (h < cap) c = make_int2(static_cast<int>(tb.a[h]), static_cast<int>(tb.b[h]));
      }
      a.nodes[out + x] = z;
      a.eids[out + x] = eid;
      a.times[out + x] = tm;
      a.delta_t[out + x] = dt;
      a.counts[out + x] = c;
    }
    phase_end<TPR>();      // the table is read to the end before the next row clears it

    // the parts read no table: a wave goes from here to the next row's clear on its own
    const PairRow r = {A, B, s, d, t, L};
    table_part<false, TPR>(r, a.node, hn, rl, out);
    table_part<true, TPR>(r, a.edge, he, rl, out);
    if (ht.q != 0) {
      if (a.time.vec4)
        time_part<float4, TPR>(r, a.time.feats, a.bias, ht, rl,
                               reinterpret_cast<float4*>(a.time.out) + out * ht.q);
      else
        time_part<float, TPR>(r, a.time.feats, a.bias, ht, rl, a.time.out + out * ht.q);
    }
  }
}

template <int CAP, int TPR>
void launch(const PairSeqArgs& a, hipStream_t stream) {
  constexpr int kRows = kThreads / TPR;
  static_assert(sizeof(Table<CAP>) * kRows <= 64 * 1024, "static LDS of a workgroup");
  pair_sequence_kernel<CAP, TPR>
      <<<strided_grid(a.rows, kRows, kMaxGrid), dim3(kThreads), 0, stream>>>(a);
}

// vec4 is decided by the caller once the outputs are known to be there
Part part_of(const std::string& w, const char* name, const float* feats, size_t rows,
             size_t width, float* out, bool has_rows) {
  check_feature_table(w, name, feats, width, kPairSeqMaxWidth, out != nullptr || !has_rows);
  if (feats == nullptr) return {nullptr, 0, 0, 0, nullptr};
  return {feats, rows, static_cast<uint32_t>(width), 0, out};
}

}  // namespace

void pair_sequence(const GraphView& g, const int64_t* d_src, const int64_t* d_dst,
                   const float* d_ts, const float* d_since, size_t num_rows, size_t length,
                   const float* d_node_feats, size_t node_rows, size_t dn,
                   const float* d_edge_feats, size_t edge_rows, size_t de, const float* d_weight,
                   const float* d_bias, size_t dim_time, int32_t* d_lengths, int64_t* d_nodes,
                   int64_t* d_eids, float* d_times, float* d_delta_t, int32_t* d_counts,
                   float* d_node_out, float* d_edge_out, float* d_time_out, int device,
                   hipStream_t stream) {
  const std::string w("pair_sequence");
  GF_REQUIRE(num_rows < (size_t{1} << 31), w + ": 2^31 rows or more");
  // length - 1 is window_of's bound, and 0 there means "no bound": it must not get there
  GF_REQUIRE(length >= 2 && length <= kPairSeqMaxLength,
             w + ": length outside [2, " + std::to_string(kPairSeqMaxLength) + "]");
  const bool has_rows = num_rows != 0;
  Part node = part_of(w, "the node table", d_node_feats, node_rows, dn, d_node_out, has_rows);
  Part edge = part_of(w, "the edge table", d_edge_feats, edge_rows, de, d_edge_out, has_rows);
  GF_REQUIRE((d_weight == nullptr) == (d_bias == nullptr),
             w + ": the time encoder's weight and bias are given together or not at all");
  Part time = part_of(w, "the time encoder's weight", d_weight, 0, dim_time, d_time_out, has_rows);
  if (num_rows == 0) return;
  GF_REQUIRE(d_src && d_dst && d_ts, w + ": null src, dst or ts");
  GF_REQUIRE(d_lengths && d_nodes && d_eids && d_times && d_delta_t && d_counts,
             w + ": null lengths, nodes, eids, times, delta_t or counts");
  GF_REQUIRE(reinterpret_cast<uintptr_t>(d_counts) % 8 == 0, w + ": counts not 8-byte aligned");
  node.vec4 = node.width && dn % 4 == 0 && aligned16(d_node_feats) && aligned16(d_node_out);
  edge.vec4 = edge.width && de % 4 == 0 && aligned16(d_edge_feats) && aligned16(d_edge_out);
  time.vec4 = time.width && dim_time % 4 == 0 && aligned16(d_time_out);      // w, b: scalar reads
  uint32_t cap = 4, log2cap = 2;
  while (cap < 4 * length) cap <<= 1, ++log2cap;      // <= 2048
  PairSeqArgs a = {store_view(g), d_src, d_dst, d_ts, d_since, num_rows,
                   static_cast<uint32_t>(length), cap, 64 - log2cap, node, edge, time, d_bias,
                   d_lengths, d_nodes, d_eids, d_times, d_delta_t,
                   reinterpret_cast<int2*>(d_counts)};
  DeviceGuard dg(device);
  if (length <= 32) launch<128, kWave>(a, stream);
  else if (length <= 128) launch<512, kWave>(a, stream);
  else launch<2048, kThreads>(a, stream);
  GF_HIP(hipGetLastError());
}

}  // namespace gf
