// feed_forward.hip: the transformer feed-forward w2(drop(gelu(w1 x + b1))) + b2 of DyGFormer's
// EncoderBlock and GraphMixer's channel MLP as a chain of two float32 MFMA GEMMs whose hidden
// activation [M, Hd] lives only in registers and LDS, forward and backward.
// Contract: include/gnnflow_hip.h (gf_feed_forward).
#pragma once

#include <cstddef>
#include <cstdint>

#include <hip/hip_runtime.h>

namespace gf {

constexpr size_t kFeedForwardMaxWidth = 256;               // GF_FEED_FORWARD_MAX_WIDTH, C
constexpr size_t kFeedForwardMaxPartialRows = 256;         // GF_FEED_FORWARD_MAX_PARTIAL_ROWS
constexpr size_t kFeedForwardMaxWorkspaceFloats = size_t{16} << 20;      // 64 MiB of float32

// y[m, c] = b2[c] + sum_j (gelu(b1[j] + sum_c' x[m, c'] w1[j, c']) * w[m, j]) w2[c, j] over m <
// num_rows, j < hidden, c < width; w the Philox dropout weight of element m * hidden + j (1 when
// p == 0).  One launch; num_rows == 0 launches nothing.
void feed_forward_forward(const float* d_x, const float* d_w1, const float* d_b1,
                          const float* d_w2, const float* d_b2, size_t num_rows, size_t width,
                          size_t hidden, float p, uint64_t seed, float* d_y, int device,
                          hipStream_t stream);

// Partial rows of the backward's workspace: each row holds 2 * hidden * width + hidden + width
// floats; at most kFeedForwardMaxPartialRows rows and kFeedForwardMaxWorkspaceFloats floats (one
// row at the least).
size_t feed_forward_backward_partial_rows(size_t num_rows, size_t width, size_t hidden);

// The gradients of the five inputs from d_grad_y, u and the mask recomputed from x; each of the
// five outputs may be null.  d_grad_x: one launch.  The four weight gradients: one launch into
// d_partials and one that sums its rows in ascending order; not launched when all four are null.
void feed_forward_backward(const float* d_x, const float* d_w1, const float* d_b1,
                           const float* d_w2, size_t num_rows, size_t width, size_t hidden,
                           float p, uint64_t seed, const float* d_grad_y, float* d_partials,
                           size_t partial_rows, float* d_grad_x, float* d_grad_w1,
                           float* d_grad_b1, float* d_grad_w2, float* d_grad_b2, int device,
                           hipStream_t stream);

// ---- feed_forward_bf16.hip: the same op with both products of every pass on
// v_mfma_f32_16x16x32_bf16.  The interface stays float32; x, dy, w1, w2, the hidden activation and
// du are rounded to bfloat16 where they become matrix operands, the sums are float32 (the
// definition: include/gnnflow_hip.h, gf_feed_forward_bf16).

// Bytes of the caller-owned workspace a call packs bf(w1) and bf(w2) into, every orientation its
// passes read zero-padded to multiples of 64: two arrays for the forward ([Hd][C] of w1, [C][Hd]
// of w2), three for the backward ([Hd][C] and [C][Hd] of w1, [Hd][C] of w2), 2 * round64(hidden) *
// round64(width) bytes each.
size_t feed_forward_bf16_workspace(size_t width, size_t hidden, bool backward);

// feed_forward_forward's contract; a pack launch into d_workspace (16-byte aligned, at least
// feed_forward_bf16_workspace(width, hidden, false) bytes) and the forward launch.
void feed_forward_bf16_forward(const float* d_x, const float* d_w1, const float* d_b1,
                               const float* d_w2, const float* d_b2, size_t num_rows,
                               size_t width, size_t hidden, float p, uint64_t seed,
                               void* d_workspace, size_t workspace_bytes, float* d_y, int device,
                               hipStream_t stream);

// feed_forward_backward_partial_rows' contract and row size, for the bfloat16 weight pass.
size_t feed_forward_bf16_backward_partial_rows(size_t num_rows, size_t width, size_t hidden);

// feed_forward_backward's contract; a pack launch into d_workspace (at least
// feed_forward_bf16_workspace(width, hidden, true) bytes) goes first.
void feed_forward_bf16_backward(const float* d_x, const float* d_w1, const float* d_b1,
                                const float* d_w2, size_t num_rows, size_t width, size_t hidden,
                                float p, uint64_t seed, const float* d_grad_y, void* d_workspace,
                                size_t workspace_bytes, float* d_partials, size_t partial_rows,
                                float* d_grad_x, float* d_grad_w1, float* d_grad_b1,
                                float* d_grad_w2, float* d_grad_b2, int device,
                                hipStream_t stream);

}  // namespace gf
