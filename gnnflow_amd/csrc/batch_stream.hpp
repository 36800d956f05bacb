// batch_stream.hip: the first stage of a training step on the device — the roots and
// timestamps of a batch of an edge stream that lives in HBM, its negatives drawn by Philox
// from the ascending list of distinct destinations — and that list itself, kept as a bitmap
// plus its compaction.  Contracts: include/gnnflow_hip.h (gf_batch_assemble, gf_dst_set_*).
#pragma once

#include <cstddef>
#include <cstdint>

#include <hip/hip_runtime.h>

namespace gf {

constexpr int kDstSetTileWords = 1024;   // 64-bit bitmap words one workgroup compacts

// One batch [lo, hi) of the stream.  d_src == nullptr: negatives only (d_dst, d_time and d_ts
// are not touched, roots[k * B + i] is the draw of tid = (first_row + lo + i) * K + k).
void batch_assemble(const int64_t* d_src, const int64_t* d_dst, const float* d_time,
                    size_t num_rows, size_t lo, size_t hi, size_t neg_ratio, const int64_t* d_dl,
                    const int64_t* d_dl_count, uint64_t seed, uint64_t epoch, uint64_t first_row,
                    int64_t* d_roots, float* d_ts, int device, hipStream_t stream);
// num_batches consecutive batches, borders read from device memory, in one launch.
void batch_assemble_many(const int64_t* d_src, const int64_t* d_dst, const float* d_time,
                         size_t num_rows, const int64_t* d_borders, size_t num_batches,
                         size_t max_batch_rows, size_t neg_ratio, const int64_t* d_dl,
                         const int64_t* d_dl_count, uint64_t seed, uint64_t epoch,
                         uint64_t first_row, int64_t* d_roots, float* d_ts, size_t capacity,
                         int device, hipStream_t stream);

void dst_set_mark(const int64_t* d_ids, size_t n, uint64_t* d_bitmap, size_t num_nodes,
                  uint64_t* d_out_of_range, int device, hipStream_t stream);
size_t dst_set_scratch_bytes(size_t num_nodes);
void dst_set_compact(const uint64_t* d_bitmap, size_t num_nodes, int64_t* d_ids,
                     size_t ids_capacity, int64_t* d_count, void* d_scratch, size_t scratch_bytes,
                     int device, hipStream_t stream);

}  // namespace gf
