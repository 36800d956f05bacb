// The position-count ("anonymous") encoding of temporal walks: for row i, with nodes[i] the W
// walks of L + 1 nodes to encode and ref[i] the Wr walks of Lr + 1 nodes to count in,
//
//   out[i, w, j, p] = #{w' < Wr : ref[i, w', p] == nodes[i, w, j]}   if nodes[i, w, j] >= 0, else 0
//
// A negative entry (an ended slot of temporal_walk.hip) encodes to zeros and, being compared only
// with entries >= 0, is never counted.
//
// One workgroup per row, rows past the grid limit grid-strided.  ref[i], at most
// kWalkMaxRefEntries ids = 32 KB, is copied into static LDS once; then every thread takes output
// elements (w, j, p), consecutive threads consecutive p, and scans column p of ref[i] for its
// node: lanes with the same p read the same LDS word (a broadcast), lanes with different p read
// neighbouring words, and a wave's stores are one contiguous run.  The cost is W (L + 1) * Wr
// (Lr + 1) compares per row — every entry against every entry of ref[i] — which is what bounds
// Wr (Lr + 1); a sort-based form would do better on large sets and is not attempted.  Plain loads
// and stores, no atomics: every output element has one writer.
#include "temporal_walk.hpp"
#include "common.hpp"

namespace gf {
namespace {

constexpr int kThreads = 256;
constexpr uint32_t kMaxGrid = 4096;       // rows past it are grid-strided

static_assert(kWalkMaxRefEntries == GF_WALK_MAX_REF_ENTRIES,
              "gnnflow_hip.h and temporal_walk.hpp disagree on the reference set's size");

struct PosArgs {
  const int64_t* nodes;      // [rows, entries]
  const int64_t* ref;        // [rows, ref_entries]
  uint64_t rows;
  uint32_t entries;          // W * (L + 1), entries * ref_len1 < 2^31
  uint32_t ref_len1;         // Lr + 1
  uint32_t ref_entries;      // Wr * (Lr + 1) <= kWalkMaxRefEntries
  int32_t* out;              // [rows, entries, ref_len1]
};

__global__ void __launch_bounds__(kThreads) walk_position_counts_kernel(const PosArgs a) {
  __shared__ int64_t s_ref[kWalkMaxRefEntries];
  const uint32_t elems = a.entries * a.ref_len1;                             // < 2^31 (host)
  for (uint64_t row = blockIdx.x; row < a.rows; row += gridDim.x) {          // uniform
    const int64_t* const ref = a.ref + row * a.ref_entries;
    for (uint32_t k = threadIdx.x; k < a.ref_entries; k += kThreads)
      s_ref[k] = ref[k];                                       // k < ref_entries <= 4096
    __syncthreads();
    const int64_t* const nodes = a.nodes + row * a.entries;
    int32_t* const out = a.out + row * elems;
    for (uint32_t x = threadIdx.x; x < elems; x += kThreads) {      // x + kThreads < 2^32
      const uint32_t entry = x / a.ref_len1;                   // < entries
      const uint32_t p = x - entry * a.ref_len1;               // < ref_len1
      const int64_t v = nodes[entry];
      int32_t count = 0;
      if (v >= 0)
        for (uint32_t k = p; k < a.ref_entries; k += a.ref_len1)             // k < ref_entries
          count += s_ref[k] == v;
      out[x] = count;                                          // x < elems
    }
    __syncthreads();                                           // the next row rewrites the LDS
  }
}

}  // namespace

void walk_position_counts(const int64_t* d_nodes, const int64_t* d_ref, size_t rows, size_t walks,
                          size_t len1, size_t ref_walks, size_t ref_len1, int32_t* d_out,
                          int device, hipStream_t stream) {
  const std::string w("walk_position_counts");
  GF_REQUIRE(len1 >= 1 && len1 <= kWalkMaxLength + 1, w + ": walks of more than 32 steps");
  GF_REQUIRE(ref_len1 >= 1 && ref_len1 <= kWalkMaxLength + 1,
             w + ": reference walks of more than 32 steps");
  GF_REQUIRE(ref_walks <= kWalkMaxRefEntries && ref_walks * ref_len1 <= kWalkMaxRefEntries,
             w + ": more than 4096 reference entries per row");
  GF_REQUIRE(rows < (size_t{1} << 31), w + ": 2^31 rows or more");
  GF_REQUIRE(walks < (size_t{1} << 31) && walks * len1 * ref_len1 < (size_t{1} << 31),
             w + ": 2^31 counts per row or more");
  if (rows == 0 || walks == 0) return;
  GF_REQUIRE(d_nodes && d_out, w + ": null nodes or out");
  GF_REQUIRE(d_ref != nullptr || ref_walks == 0, w + ": null ref");
  PosArgs a = {d_nodes, d_ref, rows, static_cast<uint32_t>(walks * len1),
               static_cast<uint32_t>(ref_len1), static_cast<uint32_t>(ref_walks * ref_len1),
               d_out};
  DeviceGuard dg(device);
  walk_position_counts_kernel<<<dim3(static_cast<uint32_t>(std::min<uint64_t>(rows, kMaxGrid))),
                                dim3(kThreads), 0, stream>>>(a);
  GF_HIP(hipGetLastError());
}

}  // namespace gf
