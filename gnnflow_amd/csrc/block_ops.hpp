// Segment operations on a sampled block (block_ops.hip, block_attention.hip, block_gat.hip, each
// for float32 and for bfloat16 rows), the fused time encoding in front of them (time_encode.hip)
// and the fused edge score behind them (edge_score.hip), and the metrics of the scores it leaves (link_metrics.hip), and the GRU gates
// of the memory updater (gru_cell.hip): the entry points other translation units call.
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

// block_ops.hip again: the reductions above for bfloat16 src, out, grad_out and grad_src
// (uint16_t; edge weights, their gradient and arg stay as they are): widened on load, the float32
// kernels' arithmetic, one rounding to nearest even on store.  The same checks.  d_scratch is a
// caller-owned float32 [num_src, dim] the gradient of the source rows is accumulated in when d_col
// is given (then rounded into d_grad_src by narrow_rows); it may be null when d_col is null, or
// when d_grad_src is.
void segment_reduce_bf16_forward(const int64_t* d_offsets, size_t num_dst, const int64_t* d_col,
                                 const uint16_t* d_src, size_t dim, const float* d_w,
                                 size_t heads, bool mean, uint16_t* d_out, int device,
                                 hipStream_t stream);
void segment_reduce_bf16_backward(const int64_t* d_offsets, size_t num_dst, const int64_t* d_col,
                                  const uint16_t* d_src, size_t dim, const float* d_w,
                                  size_t heads, bool mean, const uint16_t* d_grad_out,
                                  uint16_t* d_grad_src, size_t num_src, float* d_grad_w,
                                  float* d_scratch, int device, hipStream_t stream);
void segment_max_bf16_forward(const int64_t* d_offsets, size_t num_dst, const int64_t* d_col,
                              const uint16_t* d_src, size_t dim, uint16_t* d_out, int64_t* d_arg,
                              int device, hipStream_t stream);
void segment_max_bf16_backward(size_t num_dst, const int64_t* d_col, size_t dim,
                               const uint16_t* d_grad_out, const int64_t* d_arg,
                               uint16_t* d_grad_src, size_t num_src, float* d_scratch, int device,
                               hipStream_t stream);
// d_out[i] = d_in[i] rounded to bfloat16, i < n, on `stream` of the current device
void narrow_rows(const float* d_in, uint16_t* d_out, size_t n, hipStream_t stream);

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
// The same with attention dropout: edge i of the grouped order and head h are kept when
// gf_philox4x32_10_first(seed, i * heads + h, 0) >= (uint32_t)(p * 2^32), and a kept weight is
// scaled by 1 / (1 - p).  p outside [0, 1) throws GF_ERR_INVALID_ARGUMENT.  d_att is the
// pre-dropout softmax; d_att_dropped (may be null) receives the weights that multiplied v.
void block_attention_dropout_forward(const int64_t* d_offsets, size_t num_dst, size_t num_edges,
                                     size_t heads, size_t head_dim, const float* d_q,
                                     const float* d_k, const float* d_v, float negative_slope,
                                     float p, uint64_t seed, float* d_out, float* d_att,
                                     float* d_att_dropped, int device, hipStream_t stream);
void block_attention_dropout_backward(const int64_t* d_offsets, size_t num_dst, size_t num_edges,
                                      size_t heads, size_t head_dim, const float* d_q,
                                      const float* d_k, const float* d_v, const float* d_att,
                                      float negative_slope, float p, uint64_t seed,
                                      const float* d_grad_out, float* d_grad_q, float* d_grad_k,
                                      float* d_grad_v, int device, hipStream_t stream);

// block_attention.hip again: the four entry points above for bfloat16 q, k, v, out and gradients
// (uint16_t; d_att and d_att_dropped stay float32): widened on load, the float32 kernels'
// arithmetic, one rounding to nearest even on store.  The same checks.
void block_attention_bf16_forward(const int64_t* d_offsets, size_t num_dst, size_t num_edges,
                                  size_t heads, size_t head_dim, const uint16_t* d_q,
                                  const uint16_t* d_k, const uint16_t* d_v, float negative_slope,
                                  uint16_t* d_out, float* d_att, int device, hipStream_t stream);
void block_attention_bf16_backward(const int64_t* d_offsets, size_t num_dst, size_t num_edges,
                                   size_t heads, size_t head_dim, const uint16_t* d_q,
                                   const uint16_t* d_k, const uint16_t* d_v, const float* d_att,
                                   float negative_slope, const uint16_t* d_grad_out,
                                   uint16_t* d_grad_q, uint16_t* d_grad_k, uint16_t* d_grad_v,
                                   int device, hipStream_t stream);
void block_attention_dropout_bf16_forward(const int64_t* d_offsets, size_t num_dst,
                                          size_t num_edges, size_t heads, size_t head_dim,
                                          const uint16_t* d_q, const uint16_t* d_k,
                                          const uint16_t* d_v, float negative_slope, float p,
                                          uint64_t seed, uint16_t* d_out, float* d_att,
                                          float* d_att_dropped, int device, hipStream_t stream);
void block_attention_dropout_bf16_backward(const int64_t* d_offsets, size_t num_dst,
                                           size_t num_edges, size_t heads, size_t head_dim,
                                           const uint16_t* d_q, const uint16_t* d_k,
                                           const uint16_t* d_v, const float* d_att,
                                           float negative_slope, float p, uint64_t seed,
                                           const uint16_t* d_grad_out, uint16_t* d_grad_q,
                                           uint16_t* d_grad_k, uint16_t* d_grad_v, int device,
                                           hipStream_t stream);

// block_gat.hip: fused GAT attention, z[e,h] = el[src(e),h] + er[d,h], the source rows both key
// and value (feat [num_src, heads, head_dim]).  d_col null = the sampler's layout src(e) =
// num_dst + e (then num_src must be num_dst + num_edges; the backward is free of atomics), else
// d_grad_feat / d_grad_el accumulate with atomicAdd.  The width limit and the dropout mask
// (p, seed; p == 0: none) are those of block_attention above.  d_att is the pre-dropout softmax
// and d_out the forward's output: with them the backward reads each feat row once.  A null
// d_grad_feat / d_grad_el / d_grad_er is skipped; the others are written in full.
void block_gat_forward(const int64_t* d_offsets, size_t num_dst, size_t num_edges,
                       const int64_t* d_col, size_t num_src, size_t heads, size_t head_dim,
                       const float* d_feat, const float* d_el, const float* d_er,
                       float negative_slope, float p, uint64_t seed, float* d_out, float* d_att,
                       float* d_att_dropped, int device, hipStream_t stream);
void block_gat_backward(const int64_t* d_offsets, size_t num_dst, size_t num_edges,
                        const int64_t* d_col, size_t num_src, size_t heads, size_t head_dim,
                        const float* d_feat, const float* d_el, const float* d_er,
                        const float* d_att, const float* d_out, float negative_slope, float p,
                        uint64_t seed, const float* d_grad_out, float* d_grad_feat,
                        float* d_grad_el, float* d_grad_er, int device, hipStream_t stream);

// block_gat.hip again: the two entry points above for bfloat16 feat, out, grad_out and grad_feat
// (el, er, att, the dropped attention, grad_el and grad_er float32).  d_out_f32 [num_dst, heads,
// head_dim] receives the forward's sums before they are rounded: it is the `out` the backward
// reads (null in the forward: not written).  d_scratch: float32 [num_src, heads, head_dim] that
// grad_feat is accumulated in when d_col is given; may be null when d_col or d_grad_feat is.
void block_gat_bf16_forward(const int64_t* d_offsets, size_t num_dst, size_t num_edges,
                            const int64_t* d_col, size_t num_src, size_t heads, size_t head_dim,
                            const uint16_t* d_feat, const float* d_el, const float* d_er,
                            float negative_slope, float p, uint64_t seed, uint16_t* d_out,
                            float* d_att, float* d_att_dropped, float* d_out_f32, int device,
                            hipStream_t stream);
void block_gat_bf16_backward(const int64_t* d_offsets, size_t num_dst, size_t num_edges,
                             const int64_t* d_col, size_t num_src, size_t heads, size_t head_dim,
                             const uint16_t* d_feat, const float* d_el, const float* d_er,
                             const float* d_att, const float* d_out_f32, float negative_slope,
                             float p, uint64_t seed, const uint16_t* d_grad_out,
                             uint16_t* d_grad_feat, float* d_grad_el, float* d_grad_er,
                             float* d_scratch, int device, hipStream_t stream);

// time_encode.hip: out = [a | b | cosf(w * t + bias)] in one launch (a / b may be null with
// width 0), and the gradients of w and bias from the time columns of grad_out, read in place
// (row pitch grad_pitch floats, first time column grad_col).  The backward needs a caller-owned
// buffer of time_encode_backward_partial_rows(n) * 2 * dim_time floats; a null d_grad_w or
// d_grad_bias is skipped.  n == 0 launches nothing.
constexpr size_t kTimeEncodeMaxPartialRows = 1024;
size_t time_encode_backward_partial_rows(size_t n);
void time_encode_cat_forward(const float* d_a, size_t width_a, const float* d_b, size_t width_b,
                             const float* d_t, const float* d_w, const float* d_bias, size_t n,
                             size_t dim_time, float* d_out, int device, hipStream_t stream);
void time_encode_backward(const float* d_t, const float* d_w, const float* d_bias, size_t n,
                          size_t dim_time, const float* d_grad_out, size_t grad_pitch,
                          size_t grad_col, float* d_partials, size_t partial_rows,
                          float* d_grad_w, float* d_grad_bias, int device, hipStream_t stream);
// The same with a bfloat16 d_out (float32 parts, t, w, bias; each value rounded once on store)
// and with a bfloat16 d_grad_out (widened on load; partials, grad_w and grad_bias float32, in
// the float32 path's summation order).
void time_encode_cat_bf16_forward(const float* d_a, size_t width_a, const float* d_b,
                                  size_t width_b, const float* d_t, const float* d_w,
                                  const float* d_bias, size_t n, size_t dim_time, uint16_t* d_out,
                                  int device, hipStream_t stream);
void time_encode_backward_bf16(const float* d_t, const float* d_w, const float* d_bias, size_t n,
                               size_t dim_time, const uint16_t* d_grad_out, size_t grad_pitch,
                               size_t grad_col, float* d_partials, size_t partial_rows,
                               float* d_grad_w, float* d_grad_bias, int device,
                               hipStream_t stream);

// edge_score.hip: out[j] = bias + sum_d w[d] * max(src[j mod num_src, d] + dst[j, d], 0) in one
// launch (num_dst a multiple of num_src), and its gradients in at most two.  The backward needs
// a caller-owned buffer of edge_score_backward_partial_rows(num_src) * (dim + 1) floats when
// d_grad_w or d_grad_bias is asked for; a null d_grad_src / d_grad_dst / d_grad_w / d_grad_bias
// is skipped.  num_dst == 0 launches nothing.
constexpr size_t kEdgeScoreMaxPartialRows = 1024;
size_t edge_score_backward_partial_rows(size_t num_src);
void edge_score_forward(const float* d_src, const float* d_dst, const float* d_w,
                        const float* d_bias, size_t num_src, size_t num_dst, size_t dim,
                        float* d_out, int device, hipStream_t stream);
void edge_score_backward(const float* d_src, const float* d_dst, const float* d_w, size_t num_src,
                         size_t num_dst, size_t dim, const float* d_grad_out, float* d_partials,
                         size_t partial_rows, float* d_grad_src, float* d_grad_dst,
                         float* d_grad_w, float* d_grad_bias, int device, hipStream_t stream);
// The same with bfloat16 src and dst rows and bfloat16 grad_src / grad_dst (widened on load,
// rounded once on store); w, bias, out, grad_out, the partials, grad_w and grad_bias float32.
void edge_score_bf16_forward(const uint16_t* d_src, const uint16_t* d_dst, const float* d_w,
                             const float* d_bias, size_t num_src, size_t num_dst, size_t dim,
                             float* d_out, int device, hipStream_t stream);
void edge_score_bf16_backward(const uint16_t* d_src, const uint16_t* d_dst, const float* d_w,
                              size_t num_src, size_t num_dst, size_t dim, const float* d_grad_out,
                              float* d_partials, size_t partial_rows, uint16_t* d_grad_src,
                              uint16_t* d_grad_dst, float* d_grad_w, float* d_grad_bias,
                              int device, hipStream_t stream);

// layer_epilogue.hip: out = layer_norm(relu(dropout(x))) over the rows of x [num_rows, dim] in one
// launch, with mean and rstd [num_rows] kept for the backward and the dropout mask drawn from
// (p, seed) in both directions, and its gradients in at most two launches.  The backward needs a
// caller-owned buffer of layer_epilogue_backward_partial_rows(num_rows) * 2 * dim floats when
// d_grad_gamma or d_grad_beta is asked for; a null d_grad_x / d_grad_gamma / d_grad_beta is
// skipped.  num_rows == 0 launches nothing (the backward zeroes the parameter gradients given).
constexpr size_t kLayerEpilogueMaxWidth = 1024;
constexpr size_t kLayerEpilogueMaxPartialRows = 1024;
size_t layer_epilogue_backward_partial_rows(size_t num_rows);
void layer_epilogue_forward(const float* d_x, const float* d_gamma, const float* d_beta,
                            size_t num_rows, size_t dim, float eps, float p, uint64_t seed,
                            float* d_out, float* d_mean, float* d_rstd, int device,
                            hipStream_t stream);
void layer_epilogue_backward(const float* d_x, const float* d_gamma, const float* d_mean,
                             const float* d_rstd, size_t num_rows, size_t dim, float p,
                             uint64_t seed, const float* d_grad_out, float* d_partials,
                             size_t partial_rows, float* d_grad_x, float* d_grad_gamma,
                             float* d_grad_beta, int device, hipStream_t stream);
// The same with bfloat16 x rows and a bfloat16 grad_x (widened on load, rounded once on store);
// everything else float32.
void layer_epilogue_bf16_forward(const uint16_t* d_x, const float* d_gamma, const float* d_beta,
                                 size_t num_rows, size_t dim, float eps, float p, uint64_t seed,
                                 float* d_out, float* d_mean, float* d_rstd, int device,
                                 hipStream_t stream);
void layer_epilogue_bf16_backward(const uint16_t* d_x, const float* d_gamma, const float* d_mean,
                                  const float* d_rstd, size_t num_rows, size_t dim, float p,
                                  uint64_t seed, const float* d_grad_out, float* d_partials,
                                  size_t partial_rows, uint16_t* d_grad_x, float* d_grad_gamma,
                                  float* d_grad_beta, int device, hipStream_t stream);

// link_metrics.hip: out[3] = {AP, AUC, MRR} (float64) of the scores pos[num_pos] of the true
// edges and neg[num_neg] of the negative ones, by counting instead of sorting, in two launches
// and without atomics.  MRR exists when num_neg is a multiple of num_pos (positive i's own
// negatives are neg[k * num_pos + i], the layout of edge_score) and is NaN otherwise.  d_acc,
// unless null, is the running sum of a validation pass: {sum_ap, sum_auc, sum_mrr, batches,
// mrr_batches, nonfinite, reserved, reserved}.  A NaN or an infinity among the scores gives
// three NaNs and adds 1 to nonfinite alone.  d_partials: link_metrics_partial_rows(num_pos)
// rows of kLinkMetricsPartialWords 8-byte words, caller-owned.  num_pos, num_neg >= 1 and
// num_pos + num_neg <= kLinkMetricsMaxScores, else GF_ERR_INVALID_ARGUMENT.
constexpr size_t kLinkMetricsMaxScores = 65536;
constexpr size_t kLinkMetricsTile = 2048;      // scores per LDS tile
constexpr size_t kLinkMetricsMaxPartialRows = 256;
constexpr size_t kLinkMetricsPartialWords = 4;
size_t link_metrics_partial_rows(size_t num_pos);
void link_metrics(const float* d_pos, const float* d_neg, size_t num_pos, size_t num_neg,
                  void* d_partials, size_t partial_rows, double* d_out, double* d_acc, int device,
                  hipStream_t stream);

// edge_rank.hip: the edge score of every (source, candidate) pair, src [num_src, dim] against ONE
// set cand [num_cand, dim], of which only the k best candidates per source (values, indices
// [num_src, k]: score descending, then index ascending; NaN below -inf; (-inf, -1) where fewer
// than k are left) and the counts greater / equal [num_src] of the candidates whose score is > /
// == d_ref_score[i] are kept; candidate d_skip[i] is left out of both, and so is every candidate
// whose bit is set in d_exclude [num_src, ceil(num_cand / 64)] (bit c % 64 of word c / 64; null:
// no mask; bits past num_cand are ignored).  Two launches, no atomics,
// bit-reproducible; a pair's score is edge_score_forward's, bit for bit, unless its row holds a
// NaN (which stays one).  d_ref_score null: no counts; k == 0: no list; d_skip null: nothing
// skipped.  d_scratch: edge_rank_scratch_bytes() bytes, 8-byte aligned, caller-owned.
// num_cand >= 1 and < 2^31, k <= min(num_cand, kEdgeRankMaxK), else GF_ERR_INVALID_ARGUMENT;
// num_src == 0 launches nothing.
constexpr size_t kEdgeRankMaxK = 64;
constexpr size_t kEdgeRankChunk = 256;      // candidates per workgroup pass
size_t edge_rank_scratch_bytes(size_t num_src, size_t num_cand, size_t k);
void edge_rank(const float* d_src, const float* d_cand, const float* d_w, const float* d_bias,
               size_t num_src, size_t num_cand, size_t dim, size_t k, const float* d_ref_score,
               const int64_t* d_skip, const uint64_t* d_exclude, void* d_scratch,
               size_t scratch_bytes, float* d_values, int64_t* d_indices, int64_t* d_greater,
               int64_t* d_equal, int device, hipStream_t stream);

// link_loss.hip: out[1] (float32) = mean softplus(-pos) + mean softplus(neg), the reference's
// BCEWithLogitsLoss of the positive logits against 1 plus that of the negative ones against 0,
// float32 terms summed in float64 in a fixed order, in one launch up to kLinkLossSingleTiles
// tiles of kLinkLossTile logits in all and in two beyond; no atomics.  d_acc, unless null, is
// the running sum of a training epoch: {sum_loss, sum_loss_times_num_pos, batches, nonfinite,
// sum_num_pos}; a loss that is not finite adds 1 to nonfinite alone.  d_partials:
// link_loss_partial_rows(num_pos, num_neg) float64 words, caller-owned (0 rows: may be null).
// The backward writes grad_pos [num_pos] and grad_neg [num_neg] (a null one is skipped) times
// the scalar d_grad_out[0] in one launch.  num_pos, num_neg >= 1 and < 2^31, else
// GF_ERR_INVALID_ARGUMENT.
constexpr size_t kLinkLossTile = 1024;      // logits per workgroup pass
constexpr size_t kLinkLossSingleTiles = 8;
constexpr size_t kLinkLossMaxPartialRows = 256;
constexpr size_t kLinkLossAccFields = 5;
size_t link_loss_partial_rows(size_t num_pos, size_t num_neg);
void link_loss_forward(const float* d_pos, const float* d_neg, size_t num_pos, size_t num_neg,
                       double* d_partials, size_t partial_rows, float* d_out, double* d_acc,
                       int device, hipStream_t stream);
void link_loss_backward(const float* d_pos, const float* d_neg, size_t num_pos, size_t num_neg,
                        const float* d_grad_out, float* d_grad_pos, float* d_grad_neg, int device,
                        hipStream_t stream);
// The same with bfloat16 logits (widened on load) and bfloat16 gradients (rounded once on store);
// the loss, the partials and the accumulator are as above.
void link_loss_bf16_forward(const uint16_t* d_pos, const uint16_t* d_neg, size_t num_pos,
                            size_t num_neg, double* d_partials, size_t partial_rows, float* d_out,
                            double* d_acc, int device, hipStream_t stream);
void link_loss_bf16_backward(const uint16_t* d_pos, const uint16_t* d_neg, size_t num_pos,
                             size_t num_neg, const float* d_grad_out, uint16_t* d_grad_pos,
                             uint16_t* d_grad_neg, int device, hipStream_t stream);

// gru_cell.hip: the gates of a GRU cell behind its two GEMMs, gi = x W_ih^T + b_ih and gh = h W_hh^T
// + b_hh [n, 3 * hidden] in the order r, z, n, hx [n, hidden]:
//   r = sigma(gi_r + gh_r), z = sigma(gi_z + gh_z), n = tanh(gi_n + r * gh_n), u = (1 - z) n + z hx
// in one launch: d_out [n, hidden] = u (+ residual, float32 or bfloat16 by residual_bf16, null:
// none) and d_last [num_last, hidden] = the first rows of u (num_last <= n; 0: d_last may be
// null).  The backward recomputes the gates and writes d_grad_gi, d_grad_gh [n, 3 * hidden] and
// d_grad_hx [n, hidden] from d_grad_out [n, hidden] in one launch; a null one is skipped.  The
// residual's gradient is d_grad_out itself.  n == 0 launches nothing.
void gru_cell_forward(const float* d_gi, const float* d_gh, const float* d_hx,
                      const void* d_residual, int residual_bf16, size_t n, size_t hidden,
                      size_t num_last, float* d_out, float* d_last, int device,
                      hipStream_t stream);
void gru_cell_backward(const float* d_gi, const float* d_gh, const float* d_hx, size_t n,
                       size_t hidden, const float* d_grad_out, float* d_grad_gi, float* d_grad_gh,
                       float* d_grad_hx, int device, hipStream_t stream);
// The same with bfloat16 gi and gh and bfloat16 grad_gi / grad_gh (widened on load, rounded once
// on store); hx, out, last, grad_out and grad_hx float32.
void gru_cell_bf16_forward(const uint16_t* d_gi, const uint16_t* d_gh, const float* d_hx,
                           const void* d_residual, int residual_bf16, size_t n, size_t hidden,
                           size_t num_last, float* d_out, float* d_last, int device,
                           hipStream_t stream);
void gru_cell_bf16_backward(const uint16_t* d_gi, const uint16_t* d_gh, const float* d_hx,
                            size_t n, size_t hidden, const float* d_grad_out,
                            uint16_t* d_grad_gi, uint16_t* d_grad_gh, float* d_grad_hx,
                            int device, hipStream_t stream);

}  // namespace gf
