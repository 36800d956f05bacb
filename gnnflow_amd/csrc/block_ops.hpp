// Segment operations on a sampled block (block_ops.hip, block_attention.hip): the entry points
// other translation units call.
#pragma once

#include <cstddef>
#include <cstdint>

#include "common.hpp"

namespace gf {

void segment_offsets(const int64_t* d_row, size_t num_edges, size_t num_dst, int64_t* d_offsets,
                     int device, hipStream_t stream);
void edge_softmax(const int64_t* d_offsets, size_t num_dst, size_t num_edges, size_t heads,
                  const float* d_y_or_x, const float* d_grad_y, float* d_out, int device,
                  hipStream_t stream);
void segment_reduce_forward(const int64_t* d_offsets, size_t num_dst, const int64_t* d_col,
                            const float* d_src, size_t dim, const float* d_w, size_t heads,
                            bool mean, float* d_out, int device, hipStream_t stream);
void segment_reduce_backward(const int64_t* d_offsets, size_t num_dst, const int64_t* d_col,
                             const float* d_src, size_t dim, const float* d_w, size_t heads,
                             bool mean, const float* d_grad_out, float* d_grad_src,
                             size_t num_src, float* d_grad_w, int device, hipStream_t stream);
void segment_max_forward(const int64_t* d_offsets, size_t num_dst, const int64_t* d_col,
                         const float* d_src, size_t dim, float* d_out, int64_t* d_arg, int device,
                         hipStream_t stream);
void segment_max_backward(size_t num_dst, const int64_t* d_col, size_t dim,
                          const float* d_grad_out, const int64_t* d_arg, float* d_grad_src,
                          size_t num_src, int device, hipStream_t stream);

// block_attention.hip: fused attention with per-edge K / V.  heads * head_dim is limited to
// kBlockAttentionMaxWidth (GF_BLOCK_ATTENTION_MAX_WIDTH of the C ABI); beyond it both throw
// GF_ERR_INVALID_ARGUMENT.
constexpr size_t kBlockAttentionMaxWidth = 1024;
void block_attention_forward(const int64_t* d_offsets, size_t num_dst, size_t num_edges,
                             size_t heads, size_t head_dim, const float* d_q, const float* d_k,
                             const float* d_v, float negative_slope, float* d_out, float* d_att,
                             int device, hipStream_t stream);
void block_attention_backward(const int64_t* d_offsets, size_t num_dst, size_t num_edges,
                              size_t heads, size_t head_dim, const float* d_q, const float* d_k,
                              const float* d_v, const float* d_att, float negative_slope,
                              const float* d_grad_out, float* d_grad_q, float* d_grad_k,
                              float* d_grad_v, int device, hipStream_t stream);

}  // namespace gf
