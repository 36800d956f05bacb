// The features of what a node met, reduced over its history window: for row i with node
// v = nodes[i], time t = ts[i] and, when `since` is given, lower end lo = since[i],
//
//   seg[0 .. n)     = the window of v at (t, lo, max_history), as history_window.hpp defines it,
//                     oldest first
//   count[i]        = n
//   node_out[i, c]  = ((+0.0f + N[seg[0].dst, c]) + N[seg[1].dst, c]) + ...        c < dn
//   edge_out[i, c]  = ((+0.0f + E[seg[0].eid, c]) + E[seg[1].eid, c]) + ...        c < de
//
// in float32, one addition per record in window order; with `mean` the finished sum is divided
// once by float(n), a correctly rounded division (zeros when n == 0).  N[id, :] is the zero row
// for an id without a row in the table (negative, >= the table's rows); such a record still
// counts in n.  Every row's outputs are written, the rows with an empty window too.
//
// A wave takes a row at a time, four rows per workgroup, rows past the grid limit grid-strided.
// All lanes resolve the window together (the same addresses: one request).  The lanes own
// columns: lane l holds column tile + l, a float4 of four columns when the width is a multiple of
// four and the table and the output are 16-byte aligned, one float otherwise, and a table wider
// than 64 of those is taken in tiles of 64, each with its own walk over the window -- the
// accumulator of an element is one register of one lane from the first addition to the store.
// The walk takes kUnroll records at a time: lanes 0 .. kUnroll - 1 read one record's id each (one
// load), the ids are broadcast as scalars, the kUnroll row loads are issued back to back, and
// only then are they added, in order, so that kUnroll rows are in flight per wave while every
// element's additions stay in window order.  One writer per element, plain loads and stores, no
// LDS, no atomics, no waiting on another workgroup: the same inputs give the same bits, and they
// are the bits of a sequential float32 loop on the host.  The cost is the rows read: a hub with
// 10^6 earlier edges is 10^6 row reads for its row, by one wave; max_history and since are what
// bound it.
#include "neighbor_aggregate.hpp"
#include "common.hpp"
#include "feature_table.hpp"
#include "history_window.hpp"

namespace gf {
namespace {

using namespace wave_per_row;                 // kThreads, kWave, kWaves, kMaxGrid
constexpr uint32_t kUnroll = 8;               // rows of a table in flight per wave

struct Table {
  const float* feats;        // nullptr: the table is absent, its output is not written
  uint64_t rows;
  uint32_t width;            // floats per row, 1 .. kAggregateMaxWidth
  uint32_t vec4;             // width % 4 == 0 and feats, out 16-byte aligned: float4 columns
  float* out;                // [rows of the call, width]
};

struct AggregateArgs {
  StoreView store;           // without a node: every row gets the empty answer
  const int64_t* nodes;
  const float* ts;
  const float* since;        // nullptr: no lower end
  uint64_t rows;
  uint32_t max_history;      // 0: the whole window
  uint32_t mean;
  Table node, edge;          // rows indexed by a record's dst, by its eid
  int64_t* count;
};

__device__ __forceinline__ void add_to(float& a, const float& b) { a += b; }
__device__ __forceinline__ void add_to(float4& a, const float4& b) {
  a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
}
__device__ __forceinline__ void divide(float& a, float n) { a = __fdiv_rn(a, n); }
__device__ __forceinline__ void divide(float4& a, float n) {
  a.x = __fdiv_rn(a.x, n); a.y = __fdiv_rn(a.y, n);
  a.z = __fdiv_rn(a.z, n); a.w = __fdiv_rn(a.w, n);
}

// lane `src`'s value in every lane, as a scalar
__device__ __forceinline__ int64_t from_lane(int64_t v, int src) {
  const uint32_t lo = __builtin_amdgcn_readlane(static_cast<uint32_t>(v), src);
  const uint32_t hi = __builtin_amdgcn_readlane(static_cast<uint32_t>(v >> 32), src);
  return static_cast<int64_t>((static_cast<uint64_t>(hi) << 32) | lo);
}

// One table over one row's window; V is the column type, kEid picks the id of a record.  Called
// by the whole wave with the same seg and n in every lane.
template <typename V, bool kEid>
__device__ __forceinline__ void reduce_rows(const EdgePair* __restrict__ seg, uint32_t n,
                                            const Table& t, uint64_t row, bool mean,
                                            uint32_t lane) {
  const uint32_t cols = t.width / (sizeof(V) / sizeof(float));      // columns of type V
  const V* const tab = reinterpret_cast<const V*>(t.feats);
  V* const out = reinterpret_cast<V*>(t.out) + row * cols;
  for (uint32_t tile = 0; tile < cols; tile += kWave) {
    const uint32_t c = tile + lane;
    const bool mine = c < cols;
    V acc;
    clear(acc);
    for (uint32_t x = 0; x < n; x += kUnroll) {
      const uint32_t left = n - x;                                    // >= 1
      int64_t id = -1;                                                // no row: adds nothing
      if (lane < kUnroll && lane < left) id = kEid ? seg[x + lane].eid : seg[x + lane].dst;
      V v[kUnroll];
#pragma unroll
      for (uint32_t u = 0; u < kUnroll; ++u) {
        const int64_t r = from_lane(id, u);                           // -1 past the window
        clear(v[u]);
        if (mine && r >= 0 && static_cast<uint64_t>(r) < t.rows)      // r < rows, c < cols
          v[u] = tab[static_cast<uint64_t>(r) * cols + c];
      }
#pragma unroll
      for (uint32_t u = 0; u < kUnroll; ++u)
        if (u < left) add_to(acc, v[u]);                              // window order
    }
    if (mine) {
      if (mean && n != 0) divide(acc, static_cast<float>(n));
      out[c] = acc;
    }
  }
}

template <bool kEid>
__device__ __forceinline__ void reduce_table(const EdgePair* seg, uint32_t n, const Table& t,
                                             uint64_t row, bool mean, uint32_t lane) {
  if (t.feats == nullptr) return;
  if (t.vec4) reduce_rows<float4, kEid>(seg, n, t, row, mean, lane);
  else reduce_rows<float, kEid>(seg, n, t, row, mean, lane);
}

__global__ void __launch_bounds__(kThreads) neighbor_aggregate_kernel(const AggregateArgs a) {
  const uint32_t lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
  const uint64_t step = static_cast<uint64_t>(gridDim.x) * kWaves;
  for (uint64_t row = static_cast<uint64_t>(blockIdx.x) * kWaves + wave; row < a.rows;
       row += step) {                                          // uniform over the wave
    const Window win = window_of(a.store, a.nodes[row], a.ts[row], a.since, row, a.max_history);
    // n and seg are the same in every lane: the wave takes the branches below as one
    reduce_table<false>(win.seg, win.n, a.node, row, a.mean != 0, lane);
    reduce_table<true>(win.seg, win.n, a.edge, row, a.mean != 0, lane);
    if (lane == 0) a.count[row] = static_cast<int64_t>(win.n);
  }
}

// `out` may be null only in a call without rows
Table table_of(const std::string& w, const char* name, const float* feats, size_t rows,
               size_t width, float* out, bool need_out) {
  check_feature_table(w, name, feats, width, kAggregateMaxWidth, out != nullptr || !need_out);
  if (feats == nullptr) return {nullptr, 0, 0, 0, nullptr};
  const bool vec4 = width % 4 == 0 && aligned16(feats) && aligned16(out);
  return {feats, rows, static_cast<uint32_t>(width), vec4 ? 1u : 0u, out};
}

}  // namespace

void neighbor_aggregate(const GraphView& g, const int64_t* d_nodes, const float* d_ts,
                        const float* d_since, size_t num_rows, size_t max_history,
                        const float* d_node_feats, size_t node_rows, size_t dn,
                        const float* d_edge_feats, size_t edge_rows, size_t de, bool mean,
                        int64_t* d_count, float* d_node_out, float* d_edge_out, int device,
                        hipStream_t stream) {
  const std::string w("neighbor_aggregate");
  GF_REQUIRE(num_rows < (size_t{1} << 31), w + ": 2^31 rows or more");
  GF_REQUIRE(d_node_feats || d_edge_feats, w + ": no feature table");
  const Table node = table_of(w, "the node table", d_node_feats, node_rows, dn, d_node_out,
                              num_rows != 0);
  const Table edge = table_of(w, "the edge table", d_edge_feats, edge_rows, de, d_edge_out,
                              num_rows != 0);
  if (num_rows == 0) return;
  GF_REQUIRE(d_nodes && d_ts, w + ": null nodes or ts");
  GF_REQUIRE(d_count, w + ": null count");
  AggregateArgs a = {store_view(g), d_nodes, d_ts, d_since, num_rows,
                     history_bound(max_history), mean ? 1u : 0u, node, edge, d_count};
  DeviceGuard dg(device);
  neighbor_aggregate_kernel<<<strided_grid(num_rows, kWaves, kMaxGrid), dim3(kThreads), 0,
                              stream>>>(a);
  GF_HIP(hipGetLastError());
}

}  // namespace gf
