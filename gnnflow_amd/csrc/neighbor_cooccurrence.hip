// The two padded histories of a pair and their neighbour co-occurrence counts: for row i with
// source s = src[i], destination d = dst[i], time t = ts[i] and, when `since` is given,
// lo = since[i], with L = length (slots per side) and self = include_self ? 1 : 0,
//
//   H        = L - self                     the bound of the window, 1 .. 512 - self
//   W(v)     = the considered records of v at (t, lo, H) as history_window.hpp defines them,
//              oldest first, n(v) = |W(v)| <= H
//   seq(v)   = [v itself if self] + W(v).dst                 len(v) = self + n(v) <= L
//   a(z), b(z) = how often z occurs in seq(s), in seq(d), for z >= 0 (a negative id is nobody's
//              neighbour: it is not counted and its own counts are 0, 0)
//   lengths[i, :]        = len(s), len(d)
//   nodes[i, side, :]    = seq(v), then -1               side 0: v = s, side 1: v = d
//   eids[i, side, :]     = the records' eid; -1 for the self slot and the padding
//   times[i, side, :]    = the records' ts; t for the self slot; 0 in the padding
//   counts[i, side, p, :] = a(z), b(z) of z = nodes[i, side, p]; 0, 0 in the padding
//
// Every element of the five outputs is written.  All of it is integer work and copies, and nothing
// depends on the order in which lanes arrive: the counts are sums, and an output position is a
// position of the window.  The self slot is here and not in the caller because it is counted: s
// at position 0 of side 0 is one more occurrence of s for every element of either side that is s.
//
// The table.  A row gets an open-addressing table in LDS keyed by the 64-bit node id
// (lds_id_table.hpp: linear probing, the empty mark is -1), as three arrays (key int64, a and b
// uint32: 16 bytes a slot; common_neighbors.hip's pa is not needed, positions are not ranked).  An
// element is inserted with a 64-bit LDS compare-and-swap on the key and atomicAdd on a (s's side)
// or on b (d's side).  A row holds at most 2L distinct keys, the self slots included, and the
// slots in use, `cap`, are the power of two >= 4L (>= 4), sized by L and not by H: the load stays
// <= 1/2, which is what bounds the probe loops.
//
// Three instantiations by L, the LDS bytes fixed per instantiation, `cap` slots of it cleared and
// used:
//   L <=  32:  128 slots,  2 048 B a row, a wave per row, 4 rows =  8 192 B a workgroup
//   L <= 128:  512 slots,  8 192 B a row, a wave per row, 4 rows = 32 768 B a workgroup
//   L <= 512: 2048 slots, 32 768 B a row, 4 waves on one row     = 32 768 B a workgroup
// Against 160 KiB of LDS per CU: 20 workgroups of the first fit (the wave slots allow 8 of 256
// threads, 32 waves per CU), and 5 of the second and of the third (5 x 32 KiB = 160 KiB), 20
// waves per CU in the latter two.
//
// Phases of a row: clear, insert (both sides and the self slots), emit.  They are separated as in
// common_neighbors.hip: where a wave owns its row by a workgroup-scope fence, and nothing waits
// for another wave, so waves of one workgroup may run different numbers of rows; in the largest
// bucket the four waves share the row, the phases are separated by __syncthreads(), and the row
// loop has the same trip count in every wave of the workgroup (the row depends on blockIdx
// alone): no barrier sits in a loop whose trip count differs between waves.  The inserts of both
// sides are one phase: the atomics commute.
//
// Emit: the row's threads stride over the 2L output positions, side 0's then side 1's, so that
// consecutive lanes write consecutive elements of each output plane.  A position inside seq reads
// its record once (one 32-byte sector holds dst, eid and ts), finds its slot and writes nodes,
// eids, times and both counts, the counts as one 8-byte store; a position past len writes the
// padding.  One writer per output element, no atomics on global memory.  A row with both windows
// empty and no self slot does not touch the table.  Rows past the grid limit are grid-strided.
#include "neighbor_cooccurrence.hpp"
#include "common.hpp"
#include "history_window.hpp"
#include "lds_id_table.hpp"

namespace gf {
namespace {

static_assert(kCoocMaxLength == GF_COOC_MAX_LENGTH,
              "gnnflow_hip.h and neighbor_cooccurrence.hpp disagree on the length limit");

constexpr int kThreads = 256;
constexpr int kWave = kIdTableWave;
constexpr uint32_t kMaxGrid = 4096;      // workgroups; the rows past a pass are grid-strided

struct CoocArgs {
  StoreView store;
  const int64_t* src;
  const int64_t* dst;
  const float* ts;
  const float* since;        // nullptr: no lower end
  uint64_t rows;
  uint32_t length;           // L, 1 + self .. kCoocMaxLength
  uint32_t self;             // 0 or 1
  uint32_t cap;              // slots in use: the power of two >= 4 * length
  uint32_t shift;            // 64 - log2(cap)
  int32_t* lengths;          // [rows, 2]
  int64_t* nodes;            // [rows, 2, L]
  int64_t* eids;             // [rows, 2, L]
  float* times;              // [rows, 2, L]
  int2* counts;              // [rows, 2, L] pairs (a, b)
};

template <int CAP>
struct Table {
  int64_t key[CAP];
  uint32_t a[CAP];
  uint32_t b[CAP];
};

template <int CAP, int TPR>
__global__ void __launch_bounds__(kThreads) neighbor_cooccurrence_kernel(const CoocArgs a) {
  constexpr int kRows = kThreads / TPR;      // rows a workgroup works on at a time
  static_assert(TPR % kWave == 0 && kThreads % TPR == 0, "whole waves on a row");
  __shared__ Table<CAP> tables[kRows];
  Table<CAP>& tb = tables[threadIdx.x / TPR];
  const uint32_t rl = threadIdx.x % TPR;      // the thread's place among those of its row
  const uint32_t L = a.length, self = a.self, cap = a.cap, shift = a.shift;
  const uint32_t H = L - self;
  __builtin_assume(H != 0);      // 1 .. kCoocMaxLength - self: window_of's "no bound" is dead
  const uint64_t step = static_cast<uint64_t>(gridDim.x) * kRows;
  for (uint64_t row = static_cast<uint64_t>(blockIdx.x) * kRows + threadIdx.x / TPR; row < a.rows;
       row += step) {      // uniform over the row's waves; over the workgroup when kRows == 1
    const float t = a.ts[row];
    const int64_t s = a.src[row], d = a.dst[row];
    const Window A = window_of(a.store, s, t, a.since, row, H);
    const Window B = window_of(a.store, d, t, a.since, row, H);
    const uint32_t len_a = self + A.n, len_b = self + B.n;      // <= L
    const uint64_t out = row * 2 * L;      // the row's first element in nodes, eids, times, counts
    if (rl == 0) {
      a.lengths[row * 2] = static_cast<int32_t>(len_a);
      a.lengths[row * 2 + 1] = static_cast<int32_t>(len_b);
    }
    // len_a and len_b are the same in every thread of the row: its waves take the branch as one
    if (len_a == 0 && len_b == 0) {      // nothing to insert: the table is not touched
      for (uint32_t x = rl; x < 2 * L; x += TPR) {
        a.nodes[out + x] = -1;
        a.eids[out + x] = -1;
        a.times[out + x] = 0.0f;
        a.counts[out + x] = make_int2(0, 0);
      }
      continue;
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
    if (self && rl < 2) {      // the self slots: s on its own side, d on its own
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
      float tm = 0.0f;
      if (p < self + w.n) {
        if (p < self) {
          z = side ? d : s;
          tm = t;
        } else {
          const EdgePair r = w.seg[p - self];      // p - self < w.n: inside the window
          z = r.dst, eid = r.eid, tm = r.ts;
        }
      }
      int2 c = make_int2(0, 0);
      if (z >= 0) {
        const uint32_t h = find(tb, z, cap, shift);
        if (h < cap) c = make_int2(static_cast<int>(tb.a[h]), static_cast<int>(tb.b[h]));
      }
      a.nodes[out + x] = z;
      a.eids[out + x] = eid;
      a.times[out + x] = tm;
      a.counts[out + x] = c;
    }
    phase_end<TPR>();      // the table is read to the end before the next row clears it
  }
}

template <int CAP, int TPR>
void launch(const CoocArgs& a, hipStream_t stream) {
  constexpr int kRows = kThreads / TPR;
  static_assert(sizeof(Table<CAP>) * kRows <= 64 * 1024, "static LDS of a workgroup");
  neighbor_cooccurrence_kernel<CAP, TPR>
      <<<strided_grid(a.rows, kRows, kMaxGrid), dim3(kThreads), 0, stream>>>(a);
}

}  // namespace

void neighbor_cooccurrence(const GraphView& g, const int64_t* d_src, const int64_t* d_dst,
                           const float* d_ts, const float* d_since, size_t num_rows,
                           size_t length, bool include_self, int32_t* d_lengths,
                           int64_t* d_nodes, int64_t* d_eids, float* d_times, int32_t* d_counts,
                           int device, hipStream_t stream) {
  const std::string w("neighbor_cooccurrence");
  const size_t self = include_self ? 1 : 0;
  GF_REQUIRE(num_rows < (size_t{1} << 31), w + ": 2^31 rows or more");
  // length - self is window_of's bound, and 0 there means "no bound": it must not get there
  GF_REQUIRE(length >= 1 + self && length <= kCoocMaxLength,
             w + ": length outside [" + std::to_string(1 + self) + ", " +
                 std::to_string(kCoocMaxLength) + "]");
  if (num_rows == 0) return;
  GF_REQUIRE(d_src && d_dst && d_ts, w + ": null src, dst or ts");
  GF_REQUIRE(d_lengths && d_nodes && d_eids && d_times && d_counts,
             w + ": null lengths, nodes, eids, times or counts");
  GF_REQUIRE(reinterpret_cast<uintptr_t>(d_counts) % 8 == 0, w + ": counts not 8-byte aligned");
  uint32_t cap = 4, log2cap = 2;
  while (cap < 4 * length) cap <<= 1, ++log2cap;      // <= 2048
  CoocArgs a = {store_view(g), d_src, d_dst, d_ts, d_since, num_rows,
                static_cast<uint32_t>(length), static_cast<uint32_t>(self), cap, 64 - log2cap,
                d_lengths, d_nodes, d_eids, d_times, reinterpret_cast<int2*>(d_counts)};
  DeviceGuard dg(device);
  if (length <= 32) launch<128, kWave>(a, stream);
  else if (length <= 128) launch<512, kWave>(a, stream);
  else launch<2048, kThreads>(a, stream);
  GF_HIP(hipGetLastError());
}

}  // namespace gf
