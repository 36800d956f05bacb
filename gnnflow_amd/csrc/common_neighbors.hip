// Which nodes have both ends of a pair met before the row's time: for row i with source
// s = src[i], destination d = dst[i], time t = ts[i] and, when `since` is given, lo = since[i],
//
//   window(v) = the considered records of v at (t, lo, H) as history_window.hpp defines them,
//               H = max_history, 1 .. 512; positions 0 .. n - 1 oldest first
//   A = window(s), B = window(d)            pair_history's window, both at the same t and lo
//   a(z), b(z) = records of A, of B with .dst == z, for z >= 0 (a negative .dst is no neighbour)
//   pa(z)      = the largest position in A that holds z
//   n_src, n_dst = |A|, |B|;  u_src, u_dst = #{z : a(z) > 0}, #{z : b(z) > 0}
//   common     = #{z : a(z) > 0 and b(z) > 0}
//   nodes[i, :] = those z by descending pa(z), the first min(common, K), then -1;
//   cnt_src, cnt_dst [i, :] = a(z), b(z) of the slot, 0 in the padding
//
// Every element of the eight outputs is written.  All of it is integer work, and nothing depends
// on the order in which lanes arrive: the counts are sums, pa is a maximum, and an output slot is
// a rank among positions.
//
// The table.  A row gets an open-addressing table in LDS keyed by the 64-bit neighbour id, linear
// probing, as four arrays (key int64, pa int32, a and b uint32: 20 bytes a slot).  The empty mark
// is -1, which no neighbour is.  A record is inserted with a 64-bit LDS compare-and-swap on the
// key (empty -> z; the slot is the record's when the swap saw empty or z), then atomicMax on pa
// and atomicAdd on a (A's records) or atomicAdd on b (B's).  Both windows are inserted: u_dst and
// the union need B's own keys.  So a row holds at most 2H distinct keys, and the slots in use,
// `cap`, are the power of two >= 4H (>= 4): the load stays <= 1/2.  Every probe loop runs at most
// cap trips and then gives the record up instead of spinning; that cannot happen, because with at
// most cap / 2 keys in cap slots a probe sequence meets the record's own key or an empty slot
// first, and no slot is ever emptied while records are inserted.  The probing (claim, find) and
// the end of a phase are lds_id_table.hpp's, shared with neighbor_cooccurrence.hip.
//
// Three instantiations by H, the LDS bytes fixed per instantiation, `cap` slots of it cleared
// and used:
//   H <=  32:  128 slots,  2 576 B a row, a wave per row, 4 rows = 10 304 B a workgroup
//   H <= 128:  512 slots, 10 256 B a row, a wave per row, 4 rows = 41 024 B a workgroup
//   H <= 512: 2048 slots, 40 976 B a row, 4 waves on one row     = 40 976 B a workgroup
// Against 160 KiB of LDS per CU: 15 workgroups of the first fit (the wave slots allow 8 of 256
// threads), 3 of the second and 3 of the third (3 x 41 KB = 123 KB; a fourth does not fit beside
// them), 12 waves per CU in the latter two.
//
// Phases of a row: clear, insert (A and B), count, emit.  Where a wave owns its row, the phases
// are separated by a workgroup-scope fence (the wave's own LDS operations complete in order; the
// fence keeps the compiler from moving accesses across it) and nothing waits for another wave, so
// waves of one workgroup may run different numbers of rows.  In the largest bucket the four waves
// share the row, the phases are separated by __syncthreads(), and the row loop has the same trip
// count in every wave of the workgroup (the row depends on blockIdx alone): no barrier sits in a
// loop whose trip count differs between waves.  A's and B's inserts are one phase: the three
// atomics commute, so nothing orders them against each other.
//
// Count: lanes stride over the cap slots and sum three flags; a wave reduces them with shuffles,
// and in the largest bucket the four waves add their sums into three LDS words.  Emit, by the
// first wave of the row: lanes walk A's positions newest first, 64 at a time.  A position p is a
// leader if its record's slot has pa == p and b > 0; a leader's output slot is the number of
// leaders before it, the ballot's bits below the lane plus the leaders of earlier chunks, and it
// is written while that is < K.  One writer per output element, no atomics on global memory.  The
// same wave writes the padding [min(common, K), K).  Rows past the grid limit are grid-strided.
//
// temporal_degree is c - c0 of one window (window_counts), a lane per element, no LDS.
#include "common_neighbors.hpp"
#include "common.hpp"
#include "history_window.hpp"
#include "lds_id_table.hpp"

namespace gf {
namespace {

static_assert(kCnMaxHistory == GF_CN_MAX_HISTORY,
              "gnnflow_hip.h and common_neighbors.hpp disagree on the history limit");

constexpr int kThreads = 256;
constexpr int kWave = kIdTableWave;
constexpr uint32_t kMaxGrid = 4096;      // workgroups; the rows past a pass are grid-strided

struct CnArgs {
  StoreView store;
  const int64_t* src;
  const int64_t* dst;
  const float* ts;
  const float* since;        // nullptr: no lower end
  uint64_t rows;
  uint32_t max_history;      // 1 .. kCnMaxHistory
  uint32_t max_common;       // K, 0 .. kCnMaxHistory
  uint32_t cap;              // slots in use: the power of two >= 4 * max_history
  uint32_t shift;            // 64 - log2(cap)
  int32_t* n_src;
  int32_t* n_dst;
  int32_t* u_src;
  int32_t* u_dst;
  int32_t* common;
  int64_t* nodes;
  int32_t* cnt_src;
  int32_t* cnt_dst;
};

template <int CAP>
struct Table {
  int64_t key[CAP];
  int32_t pa[CAP];
  uint32_t a[CAP];
  uint32_t b[CAP];
  uint32_t sum[4];           // u_src, u_dst, common of the row where several waves share it
};

template <int CAP, int TPR>
__global__ void __launch_bounds__(kThreads) common_neighbors_kernel(const CnArgs a) {
  constexpr int kRows = kThreads / TPR;      // rows a workgroup works on at a time
  static_assert(TPR % kWave == 0 && kThreads % TPR == 0, "whole waves on a row");
  __shared__ Table<CAP> tables[kRows];
  Table<CAP>& tb = tables[threadIdx.x / TPR];
  const uint32_t rl = threadIdx.x % TPR;      // the thread's place among those of its row
  const uint32_t lane = threadIdx.x % kWave;
  const uint32_t K = a.max_common, cap = a.cap, shift = a.shift;
  __builtin_assume(a.max_history != 0);      // 1 .. kCnMaxHistory: window_of's "no bound" is dead
  const uint64_t step = static_cast<uint64_t>(gridDim.x) * kRows;
  for (uint64_t row = static_cast<uint64_t>(blockIdx.x) * kRows + threadIdx.x / TPR; row < a.rows;
       row += step) {      // uniform over the row's waves; over the workgroup when kRows == 1
    const float t = a.ts[row];
    const Window A = window_of(a.store, a.src[row], t, a.since, row, a.max_history);
    const Window B = window_of(a.store, a.dst[row], t, a.since, row, a.max_history);
    int64_t* const out_nodes = a.nodes + row * K;
    int32_t* const out_a = a.cnt_src + row * K;
    int32_t* const out_b = a.cnt_dst + row * K;
    if (rl == 0) {
      a.n_src[row] = static_cast<int32_t>(A.n);
      a.n_dst[row] = static_cast<int32_t>(B.n);
    }
    // A.n and B.n are the same in every thread of the row: its waves take the branch as one
    if (A.n == 0 && B.n == 0) {      // nothing to insert: the table is not touched
      if (rl == 0) a.u_src[row] = a.u_dst[row] = a.common[row] = 0;
      for (uint32_t x = rl; x < K; x += TPR) {
        out_nodes[x] = -1;
        out_a[x] = out_b[x] = 0;
      }
      continue;
    }

    for (uint32_t x = rl; x < cap; x += TPR) {
      tb.key[x] = kIdEmpty;
      tb.pa[x] = -1;
      tb.a[x] = tb.b[x] = 0;
    }
    if (rl < 4) tb.sum[rl] = 0;
    phase_end<TPR>();

    for (uint32_t p = rl; p < A.n; p += TPR) {
      const int64_t z = A.seg[p].dst;
      if (z < 0) continue;
      const uint32_t h = claim(tb, z, cap, shift);
      if (h < cap) {
        atomicMax(&tb.pa[h], static_cast<int32_t>(p));
        atomicAdd(&tb.a[h], 1u);
      }
    }
    for (uint32_t p = rl; p < B.n; p += TPR) {
      const int64_t z = B.seg[p].dst;
      if (z < 0) continue;
      const uint32_t h = claim(tb, z, cap, shift);
      if (h < cap) atomicAdd(&tb.b[h], 1u);
    }
    phase_end<TPR>();

    uint32_t ua = 0, ub = 0, both = 0;
    for (uint32_t x = rl; x < cap; x += TPR) {
      const bool in_a = tb.a[x] != 0, in_b = tb.b[x] != 0;
      ua += in_a;
      ub += in_b;
      both += in_a && in_b;
    }
    for (int o = kWave / 2; o > 0; o >>= 1) {
      ua += __shfl_xor(ua, o);
      ub += __shfl_xor(ub, o);
      both += __shfl_xor(both, o);
    }
    if constexpr (TPR != kWave) {
      if (lane == 0) {
        atomicAdd(&tb.sum[0], ua);
        atomicAdd(&tb.sum[1], ub);
        atomicAdd(&tb.sum[2], both);
      }
      __syncthreads();
      ua = tb.sum[0], ub = tb.sum[1], both = tb.sum[2];
    }
    if (rl == 0) {
      a.u_src[row] = static_cast<int32_t>(ua);
      a.u_dst[row] = static_cast<int32_t>(ub);
      a.common[row] = static_cast<int32_t>(both);
    }

    if (rl < kWave) {      // the row's first wave, whole
      uint32_t base = 0;      // leaders of the chunks before this one
      for (uint32_t start = 0; start < A.n && base < K; start += kWave) {
        const bool valid = start + lane < A.n;
        const uint32_t p = valid ? A.n - 1 - (start + lane) : 0;
        int64_t z = -1;
        uint32_t h = cap;
        if (valid) {
          z = A.seg[p].dst;
          if (z >= 0) h = find(tb, z, cap, shift);
        }
        const bool leader = h < cap && tb.pa[h] == static_cast<int32_t>(p) && tb.b[h] != 0;
        const unsigned long long leaders = __ballot(leader);
        const uint32_t slot = base + __popcll(leaders & ((1ull << lane) - 1));
        if (leader && slot < K) {
          out_nodes[slot] = z;
          out_a[slot] = static_cast<int32_t>(tb.a[h]);
          out_b[slot] = static_cast<int32_t>(tb.b[h]);
        }
        base += __popcll(leaders);
      }
      for (uint32_t x = (both < K ? both : K) + lane; x < K; x += kWave) {
        out_nodes[x] = -1;
        out_a[x] = out_b[x] = 0;
      }
    }
    phase_end<TPR>();      // the table is read to the end before the next row clears it
  }
}

struct DegArgs {
  StoreView store;
  const int64_t* nodes;
  const float* ts;
  const float* since;
  uint64_t num;
  int64_t* out;
};

__global__ void __launch_bounds__(kThreads) temporal_degree_kernel(const DegArgs a) {
  const uint64_t step = static_cast<uint64_t>(gridDim.x) * kThreads;
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x; i < a.num;
       i += step) {
    NodeEntry e;
    uint32_t c, c0;
    (void)window_counts(a.store, a.nodes[i], a.ts[i], a.since, i, e, c, c0);
    a.out[i] = static_cast<int64_t>(c - c0);
  }
}

template <int CAP, int TPR>
void launch(const CnArgs& a, hipStream_t stream) {
  constexpr int kRows = kThreads / TPR;
  static_assert(sizeof(Table<CAP>) * kRows <= 64 * 1024, "static LDS of a workgroup");
  common_neighbors_kernel<CAP, TPR>
      <<<strided_grid(a.rows, kRows, kMaxGrid), dim3(kThreads), 0, stream>>>(a);
}

}  // namespace

void common_neighbors(const GraphView& g, const int64_t* d_src, const int64_t* d_dst,
                      const float* d_ts, const float* d_since, size_t num_rows,
                      size_t max_history, size_t max_common, int32_t* d_n_src, int32_t* d_n_dst,
                      int32_t* d_u_src, int32_t* d_u_dst, int32_t* d_common, int64_t* d_nodes,
                      int32_t* d_cnt_src, int32_t* d_cnt_dst, int device, hipStream_t stream) {
  const std::string w("common_neighbors");
  GF_REQUIRE(num_rows < (size_t{1} << 31), w + ": 2^31 rows or more");
  GF_REQUIRE(max_history >= 1 && max_history <= kCnMaxHistory,
             w + ": max_history outside [1, " + std::to_string(kCnMaxHistory) + "]");
  GF_REQUIRE(max_common <= kCnMaxHistory,
             w + ": max_common above " + std::to_string(kCnMaxHistory));
  if (num_rows == 0) return;
  GF_REQUIRE(d_src && d_dst && d_ts, w + ": null src, dst or ts");
  GF_REQUIRE(d_n_src && d_n_dst && d_u_src && d_u_dst && d_common,
             w + ": null n_src, n_dst, u_src, u_dst or common");
  GF_REQUIRE(max_common == 0 || (d_nodes && d_cnt_src && d_cnt_dst),
             w + ": null nodes, cnt_src or cnt_dst");
  uint32_t cap = 4, log2cap = 2;
  while (cap < 4 * max_history) cap <<= 1, ++log2cap;      // <= 2048
  CnArgs a = {store_view(g), d_src, d_dst, d_ts, d_since, num_rows,
              static_cast<uint32_t>(max_history), static_cast<uint32_t>(max_common), cap,
              64 - log2cap, d_n_src, d_n_dst, d_u_src, d_u_dst, d_common, d_nodes, d_cnt_src,
              d_cnt_dst};
  DeviceGuard dg(device);
  if (max_history <= 32) launch<128, kWave>(a, stream);
  else if (max_history <= 128) launch<512, kWave>(a, stream);
  else launch<2048, kThreads>(a, stream);
  GF_HIP(hipGetLastError());
}

void temporal_degree(const GraphView& g, const int64_t* d_nodes, const float* d_ts,
                     const float* d_since, size_t num, int64_t* d_out, int device,
                     hipStream_t stream) {
  const std::string w("temporal_degree");
  GF_REQUIRE(num < (size_t{1} << 31), w + ": 2^31 elements or more");
  if (num == 0) return;
  GF_REQUIRE(d_nodes && d_ts && d_out, w + ": null nodes, ts or out");
  DegArgs a = {store_view(g), d_nodes, d_ts, d_since, num, d_out};
  DeviceGuard dg(device);
  temporal_degree_kernel<<<strided_grid(num, kThreads, kMaxGrid), dim3(kThreads), 0, stream>>>(a);
  GF_HIP(hipGetLastError());
}

}  // namespace gf
