// token_mix.hip: the token-mixing half of GraphMixer's MixerBlock, x + token_mlp(LayerNorm(x)^T)^T
// over x [N, K, C], as one launch each way: LayerNorm over C, two float32 MFMA GEMMs over the token
// axis with GELU and dropout between them, dropout and the residual, with no transposed copy and no
// tensor of size N * K * C or N * Kh * C besides x and y.
// Contract: include/gnnflow_hip.h (gf_token_mix).
#pragma once

#include <cstddef>
#include <cstdint>

#include <hip/hip_runtime.h>

namespace gf {

constexpr size_t kTokenMixMaxTokens = 64;                  // GF_TOKEN_MIX_MAX_TOKENS, K and Kh
constexpr size_t kTokenMixMaxWidth = 256;                  // GF_TOKEN_MIX_MAX_WIDTH, C
constexpr size_t kTokenMixMaxPartialRows = 512;            // GF_TOKEN_MIX_MAX_PARTIAL_ROWS
constexpr size_t kTokenMixMaxWorkspaceFloats = size_t{16} << 20;         // 64 MiB of float32

// y[n, k, c] = x + m2 (b2[k] + sum_j w2[k, j] h[n, j, c]), h = gelu(b1[j] + sum_k w1[j, k] z[n, k,
// c]) m1, z = LayerNorm over c of x[n, k, :] with (gamma, beta, eps); m1 and m2 the Philox dropout
// weights of elements (n C + c) Kh + j, call 0, and (n C + c) K + k, call 1 (1 when p == 0).
// d_mean and d_rstd [N, K] are what the backward needs besides the inputs.  One launch; num_rows
// == 0 launches nothing.
void token_mix_forward(const float* d_x, const float* d_gamma, const float* d_beta,
                       const float* d_w1, const float* d_b1, const float* d_w2, const float* d_b2,
                       size_t num_rows, size_t tokens, size_t hidden, size_t width, float eps,
                       float p, uint64_t seed, float* d_y, float* d_mean, float* d_rstd, int device,
                       hipStream_t stream);

// Partial rows of the backward's workspace, one per workgroup: each row holds 2 * tokens * hidden
// + tokens + hidden + 2 * width floats; at most kTokenMixMaxPartialRows rows and
// kTokenMixMaxWorkspaceFloats floats (one row at the least).
size_t token_mix_backward_partial_rows(size_t num_rows, size_t tokens, size_t hidden,
                                       size_t width);

// The gradients of the seven inputs from d_grad_y, with z, u, h and both masks recomputed; each of
// the seven outputs may be null.  One launch, which writes d_grad_x and, when a parameter gradient
// is wanted, one partial row per workgroup; then one launch that sums the rows in ascending order
// (neither the partial rows nor that launch when all six are null).
void token_mix_backward(const float* d_x, const float* d_gamma, const float* d_beta,
                        const float* d_w1, const float* d_b1, const float* d_w2,
                        const float* d_mean, const float* d_rstd, size_t num_rows, size_t tokens,
                        size_t hidden, size_t width, float p, uint64_t seed,
                        const float* d_grad_y, float* d_partials, size_t partial_rows,
                        float* d_grad_x, float* d_grad_gamma, float* d_grad_beta,
                        float* d_grad_w1, float* d_grad_b1, float* d_grad_w2, float* d_grad_b2,
                        int device, hipStream_t stream);

}  // namespace gf
