// sequence_attention.hip: unmasked multi-head self-attention over short float32 sequences
// (DyGFormer's EncoderBlock: S = 2 L / P <= 128 tokens, head_dim <= 128) straight from the packed
// in_proj rows, one workgroup per (row, head), both products of each direction on the float32
// matrix cores, attention dropout from the stateless Philox mask.  No [S, S] tensor reaches
// memory in either direction.
// Contract: include/gnnflow_hip.h (gf_sequence_attention).
#pragma once

#include <cstddef>
#include <cstdint>

#include <hip/hip_runtime.h>

namespace gf {

constexpr size_t kSeqAttentionMaxLength = 128;       // GF_SEQ_ATTENTION_MAX_LENGTH
constexpr size_t kSeqAttentionMaxHeadDim = 128;      // GF_SEQ_ATTENTION_MAX_HEAD_DIM
constexpr size_t kSeqAttentionMaxWidth = 1024;       // GF_SEQ_ATTENTION_MAX_WIDTH, heads * head_dim

// out[r, i, h, :] = sum_j (softmax_j(q[r,i,h,:] . k[r,j,h,:] / sqrt(head_dim)) * w[r,h,i,j])
// v[r,j,h,:] with q, k, v the three [heads, head_dim] thirds of d_qkv's rows [num_rows, length,
// 3 * heads * head_dim]; d_out [num_rows, length, heads * head_dim]; d_lse [num_rows, heads,
// length] receives the rows' log-sum-exp of the scaled logits.  One launch; num_rows == 0 none.
void sequence_attention_forward(const float* d_qkv, size_t num_rows, size_t length, size_t heads,
                                size_t head_dim, float p, uint64_t seed, float* d_out,
                                float* d_lse, int device, hipStream_t stream);

// d_grad_qkv [num_rows, length, 3 * heads * head_dim] from d_grad_out, with the softmax recomputed
// from d_qkv and d_lse and the mask drawn again.  One launch, every element written once by one
// thread: no atomics, the same bits from run to run.
void sequence_attention_backward(const float* d_qkv, const float* d_lse, size_t num_rows,
                                 size_t length, size_t heads, size_t head_dim, float p,
                                 uint64_t seed, const float* d_grad_out, float* d_grad_qkv,
                                 int device, hipStream_t stream);

}  // namespace gf
