// extern "C" entry points of include/gnnflow_hip.h: thin, exception-free shims.  Here: the error
// slot they all report through, the pid behind foreign_process(), the shims over free functions
// (block ops, time encoding, edge score, link metrics, batch stream, walk encoding, debug counters).  Those over a handle: capi_{graph,sampler,cache,comm}.
#include "batch_stream.hpp"
#include "block_ops.hpp"
#include "capi_handles.hpp"
#include "partition.hpp"
#include "temporal_walk.hpp"

namespace gf {

namespace {
thread_local std::string g_last_error;
}  // namespace

const pid_t g_load_pid = getpid();

void set_last_error(const std::string& msg) { g_last_error = msg; }

}  // namespace gf

extern "C" {

const char* gf_last_error(void) { return gf::g_last_error.c_str(); }
const char* gf_version(void) { return "gnnflow_amd 0.1 (gfx950)"; }

int gf_block_segment_offsets(const int64_t* d_row, size_t num_edges, size_t num_dst,
                             int64_t* d_offsets, int device, void* stream) {
  return guarded([&] {
    gf::segment_offsets(d_row, num_edges, num_dst, d_offsets, device, as_stream(stream));
  });
}
int gf_block_edge_softmax(const int64_t* d_offsets, size_t num_dst, size_t num_edges, size_t heads,
                          const float* d_logits, float* d_out, int device, void* stream) {
  return guarded([&] {
    gf::edge_softmax(d_offsets, num_dst, num_edges, heads, d_logits, nullptr, d_out, device,
                     as_stream(stream));
  });
}
int gf_block_edge_softmax_backward(const int64_t* d_offsets, size_t num_dst, size_t num_edges,
                                   size_t heads, const float* d_out, const float* d_grad_out,
                                   float* d_grad_logits, int device, void* stream) {
  return guarded([&] {
    GF_REQUIRE(d_grad_out != nullptr || num_edges == 0, "edge_softmax backward: null gradient");
    gf::edge_softmax(d_offsets, num_dst, num_edges, heads, d_out, d_grad_out, d_grad_logits,
                     device, as_stream(stream));
  });
}
int gf_block_reduce(const int64_t* d_offsets, size_t num_dst, const int64_t* d_col,
                    const float* d_src, size_t dim, const float* d_edge_weight, size_t heads,
                    int mean, float* d_out, int device, void* stream) {
  return guarded([&] {
    gf::segment_reduce_forward(d_offsets, num_dst, d_col, d_src, dim, d_edge_weight, heads,
                               mean != 0, d_out, device, as_stream(stream));
  });
}
int gf_block_reduce_backward(const int64_t* d_offsets, size_t num_dst, const int64_t* d_col,
                             const float* d_src, size_t dim, const float* d_edge_weight,
                             size_t heads, int mean, const float* d_grad_out, float* d_grad_src,
                             size_t num_src, float* d_grad_edge_weight, int device,
                             void* stream) {
  return guarded([&] {
    gf::segment_reduce_backward(d_offsets, num_dst, d_col, d_src, dim, d_edge_weight, heads,
                                mean != 0, d_grad_out, d_grad_src, num_src, d_grad_edge_weight,
                                device, as_stream(stream));
  });
}
int gf_block_reduce_max(const int64_t* d_offsets, size_t num_dst, const int64_t* d_col,
                        const float* d_src, size_t dim, float* d_out, int64_t* d_arg, int device,
                        void* stream) {
  return guarded([&] {
    gf::segment_max_forward(d_offsets, num_dst, d_col, d_src, dim, d_out, d_arg, device,
                            as_stream(stream));
  });
}
int gf_block_reduce_max_backward(size_t num_dst, const int64_t* d_col, size_t dim,
                                 const float* d_grad_out, const int64_t* d_arg, float* d_grad_src,
                                 size_t num_src, int device, void* stream) {
  return guarded([&] {
    gf::segment_max_backward(num_dst, d_col, dim, d_grad_out, d_arg, d_grad_src, num_src, device,
                             as_stream(stream));
  });
}
static_assert(GF_BLOCK_ATTENTION_MAX_WIDTH == gf::kBlockAttentionMaxWidth,
              "gnnflow_hip.h and block_ops.hpp disagree on the attention width limit");
int gf_block_attention(const int64_t* d_offsets, size_t num_dst, size_t num_edges, size_t heads,
                       size_t head_dim, const float* d_q, const float* d_k, const float* d_v,
                       float negative_slope, float* d_out, float* d_att, int device,
                       void* stream) {
  return guarded([&] {
    gf::block_attention_forward(d_offsets, num_dst, num_edges, heads, head_dim, d_q, d_k, d_v,
                                negative_slope, d_out, d_att, device, as_stream(stream));
  });
}
int gf_block_attention_backward(const int64_t* d_offsets, size_t num_dst, size_t num_edges,
                                size_t heads, size_t head_dim, const float* d_q,
                                const float* d_k, const float* d_v, const float* d_att,
                                float negative_slope, const float* d_grad_out, float* d_grad_q,
                                float* d_grad_k, float* d_grad_v, int device, void* stream) {
  return guarded([&] {
    gf::block_attention_backward(d_offsets, num_dst, num_edges, heads, head_dim, d_q, d_k, d_v,
                                 d_att, negative_slope, d_grad_out, d_grad_q, d_grad_k, d_grad_v,
                                 device, as_stream(stream));
  });
}
int gf_block_attention_dropout(const int64_t* d_offsets, size_t num_dst, size_t num_edges,
                               size_t heads, size_t head_dim, const float* d_q, const float* d_k,
                               const float* d_v, float negative_slope, float p, uint64_t seed,
                               float* d_out, float* d_att, float* d_att_dropped, int device,
                               void* stream) {
  return guarded([&] {
    gf::block_attention_dropout_forward(d_offsets, num_dst, num_edges, heads, head_dim, d_q, d_k,
                                        d_v, negative_slope, p, seed, d_out, d_att,
                                        d_att_dropped, device, as_stream(stream));
  });
}
int gf_block_attention_dropout_backward(const int64_t* d_offsets, size_t num_dst,
                                        size_t num_edges, size_t heads, size_t head_dim,
                                        const float* d_q, const float* d_k, const float* d_v,
                                        const float* d_att, float negative_slope, float p,
                                        uint64_t seed, const float* d_grad_out, float* d_grad_q,
                                        float* d_grad_k, float* d_grad_v, int device,
                                        void* stream) {
  return guarded([&] {
    gf::block_attention_dropout_backward(d_offsets, num_dst, num_edges, heads, head_dim, d_q, d_k,
                                         d_v, d_att, negative_slope, p, seed, d_grad_out,
                                         d_grad_q, d_grad_k, d_grad_v, device, as_stream(stream));
  });
}

int gf_block_attention_bf16(const int64_t* d_offsets, size_t num_dst, size_t num_edges,
                            size_t heads, size_t head_dim, const uint16_t* d_q,
                            const uint16_t* d_k, const uint16_t* d_v, float negative_slope,
                            uint16_t* d_out, float* d_att, int device, void* stream) {
  return guarded([&] {
    gf::block_attention_bf16_forward(d_offsets, num_dst, num_edges, heads, head_dim, d_q, d_k,
                                     d_v, negative_slope, d_out, d_att, device,
                                     as_stream(stream));
  });
}
int gf_block_attention_bf16_backward(const int64_t* d_offsets, size_t num_dst, size_t num_edges,
                                     size_t heads, size_t head_dim, const uint16_t* d_q,
                                     const uint16_t* d_k, const uint16_t* d_v, const float* d_att,
                                     float negative_slope, const uint16_t* d_grad_out,
                                     uint16_t* d_grad_q, uint16_t* d_grad_k, uint16_t* d_grad_v,
                                     int device, void* stream) {
  return guarded([&] {
    gf::block_attention_bf16_backward(d_offsets, num_dst, num_edges, heads, head_dim, d_q, d_k,
                                      d_v, d_att, negative_slope, d_grad_out, d_grad_q, d_grad_k,
                                      d_grad_v, device, as_stream(stream));
  });
}
int gf_block_attention_dropout_bf16(const int64_t* d_offsets, size_t num_dst, size_t num_edges,
                                    size_t heads, size_t head_dim, const uint16_t* d_q,
                                    const uint16_t* d_k, const uint16_t* d_v,
                                    float negative_slope, float p, uint64_t seed, uint16_t* d_out,
                                    float* d_att, float* d_att_dropped, int device,
                                    void* stream) {
  return guarded([&] {
    gf::block_attention_dropout_bf16_forward(d_offsets, num_dst, num_edges, heads, head_dim, d_q,
                                             d_k, d_v, negative_slope, p, seed, d_out, d_att,
                                             d_att_dropped, device, as_stream(stream));
  });
}
int gf_block_attention_dropout_bf16_backward(const int64_t* d_offsets, size_t num_dst,
                                             size_t num_edges, size_t heads, size_t head_dim,
                                             const uint16_t* d_q, const uint16_t* d_k,
                                             const uint16_t* d_v, const float* d_att,
                                             float negative_slope, float p, uint64_t seed,
                                             const uint16_t* d_grad_out, uint16_t* d_grad_q,
                                             uint16_t* d_grad_k, uint16_t* d_grad_v, int device,
                                             void* stream) {
  return guarded([&] {
    gf::block_attention_dropout_bf16_backward(d_offsets, num_dst, num_edges, heads, head_dim, d_q,
                                              d_k, d_v, d_att, negative_slope, p, seed,
                                              d_grad_out, d_grad_q, d_grad_k, d_grad_v, device,
                                              as_stream(stream));
  });
}

int gf_block_gat(const int64_t* d_offsets, size_t num_dst, size_t num_edges, const int64_t* d_col,
                 size_t num_src, size_t heads, size_t head_dim, const float* d_feat,
                 const float* d_el, const float* d_er, float negative_slope, float p,
                 uint64_t seed, float* d_out, float* d_att, float* d_att_dropped, int device,
                 void* stream) {
  return guarded([&] {
    gf::block_gat_forward(d_offsets, num_dst, num_edges, d_col, num_src, heads, head_dim, d_feat,
                          d_el, d_er, negative_slope, p, seed, d_out, d_att, d_att_dropped,
                          device, as_stream(stream));
  });
}
int gf_block_gat_backward(const int64_t* d_offsets, size_t num_dst, size_t num_edges,
                          const int64_t* d_col, size_t num_src, size_t heads, size_t head_dim,
                          const float* d_feat, const float* d_el, const float* d_er,
                          const float* d_att, const float* d_out, float negative_slope, float p,
                          uint64_t seed, const float* d_grad_out, float* d_grad_feat,
                          float* d_grad_el, float* d_grad_er, int device, void* stream) {
  return guarded([&] {
    gf::block_gat_backward(d_offsets, num_dst, num_edges, d_col, num_src, heads, head_dim, d_feat,
                           d_el, d_er, d_att, d_out, negative_slope, p, seed, d_grad_out,
                           d_grad_feat, d_grad_el, d_grad_er, device, as_stream(stream));
  });
}

int gf_block_reduce_bf16(const int64_t* d_offsets, size_t num_dst, const int64_t* d_col,
                         const uint16_t* d_src, size_t dim, const float* d_edge_weight,
                         size_t heads, int mean, uint16_t* d_out, int device, void* stream) {
  return guarded([&] {
    gf::segment_reduce_bf16_forward(d_offsets, num_dst, d_col, d_src, dim, d_edge_weight, heads,
                                    mean != 0, d_out, device, as_stream(stream));
  });
}
int gf_block_reduce_backward_bf16(const int64_t* d_offsets, size_t num_dst, const int64_t* d_col,
                                  const uint16_t* d_src, size_t dim, const float* d_edge_weight,
                                  size_t heads, int mean, const uint16_t* d_grad_out,
                                  uint16_t* d_grad_src, size_t num_src,
                                  float* d_grad_edge_weight, int device, void* stream,
                                  float* d_scratch) {
  return guarded([&] {
    gf::segment_reduce_bf16_backward(d_offsets, num_dst, d_col, d_src, dim, d_edge_weight, heads,
                                     mean != 0, d_grad_out, d_grad_src, num_src,
                                     d_grad_edge_weight, d_scratch, device, as_stream(stream));
  });
}
int gf_block_reduce_max_bf16(const int64_t* d_offsets, size_t num_dst, const int64_t* d_col,
                             const uint16_t* d_src, size_t dim, uint16_t* d_out, int64_t* d_arg,
                             int device, void* stream) {
  return guarded([&] {
    gf::segment_max_bf16_forward(d_offsets, num_dst, d_col, d_src, dim, d_out, d_arg, device,
                                 as_stream(stream));
  });
}
int gf_block_reduce_max_backward_bf16(size_t num_dst, const int64_t* d_col, size_t dim,
                                      const uint16_t* d_grad_out, const int64_t* d_arg,
                                      uint16_t* d_grad_src, size_t num_src, int device,
                                      void* stream, float* d_scratch) {
  return guarded([&] {
    gf::segment_max_bf16_backward(num_dst, d_col, dim, d_grad_out, d_arg, d_grad_src, num_src,
                                  d_scratch, device, as_stream(stream));
  });
}
int gf_block_gat_bf16(const int64_t* d_offsets, size_t num_dst, size_t num_edges,
                      const int64_t* d_col, size_t num_src, size_t heads, size_t head_dim,
                      const uint16_t* d_feat, const float* d_el, const float* d_er,
                      float negative_slope, float p, uint64_t seed, uint16_t* d_out, float* d_att,
                      float* d_att_dropped, int device, void* stream, float* d_out_f32) {
  return guarded([&] {
    gf::block_gat_bf16_forward(d_offsets, num_dst, num_edges, d_col, num_src, heads, head_dim,
                               d_feat, d_el, d_er, negative_slope, p, seed, d_out, d_att,
                               d_att_dropped, d_out_f32, device, as_stream(stream));
  });
}
int gf_block_gat_backward_bf16(const int64_t* d_offsets, size_t num_dst, size_t num_edges,
                               const int64_t* d_col, size_t num_src, size_t heads,
                               size_t head_dim, const uint16_t* d_feat, const float* d_el,
                               const float* d_er, const float* d_att, const float* d_out_f32,
                               float negative_slope, float p, uint64_t seed,
                               const uint16_t* d_grad_out, uint16_t* d_grad_feat,
                               float* d_grad_el, float* d_grad_er, int device, void* stream,
                               float* d_scratch) {
  return guarded([&] {
    gf::block_gat_bf16_backward(d_offsets, num_dst, num_edges, d_col, num_src, heads, head_dim,
                                d_feat, d_el, d_er, d_att, d_out_f32, negative_slope, p, seed,
                                d_grad_out, d_grad_feat, d_grad_el, d_grad_er, d_scratch, device,
                                as_stream(stream));
  });
}

int gf_time_encode_cat(const float* d_a, size_t width_a, const float* d_b, size_t width_b,
                       const float* d_t, const float* d_w, const float* d_bias, size_t n,
                       size_t dim_time, float* d_out, int device, void* stream) {
  return guarded([&] {
    gf::time_encode_cat_forward(d_a, width_a, d_b, width_b, d_t, d_w, d_bias, n, dim_time, d_out,
                                device, as_stream(stream));
  });
}
int gf_time_encode_backward_partial_rows(size_t n, size_t* rows) {
  return guarded([&] {
    GF_REQUIRE(rows != nullptr, "gf_time_encode_backward_partial_rows: null output");
    *rows = gf::time_encode_backward_partial_rows(n);
  });
}
int gf_time_encode_backward(const float* d_t, const float* d_w, const float* d_bias, size_t n,
                            size_t dim_time, const float* d_grad_out, size_t grad_pitch,
                            size_t grad_col, float* d_partials, size_t partial_rows,
                            float* d_grad_w, float* d_grad_bias, int device, void* stream) {
  return guarded([&] {
    gf::time_encode_backward(d_t, d_w, d_bias, n, dim_time, d_grad_out, grad_pitch, grad_col,
                             d_partials, partial_rows, d_grad_w, d_grad_bias, device, as_stream(stream));
  });
}

int gf_time_encode_cat_bf16(const float* d_a, size_t width_a, const float* d_b, size_t width_b,
                            const float* d_t, const float* d_w, const float* d_bias, size_t n,
                            size_t dim_time, uint16_t* d_out, int device, void* stream) {
  return guarded([&] {
    gf::time_encode_cat_bf16_forward(d_a, width_a, d_b, width_b, d_t, d_w, d_bias, n, dim_time,
                                     d_out, device, as_stream(stream));
  });
}
int gf_time_encode_backward_bf16(const float* d_t, const float* d_w, const float* d_bias,
                                 size_t n, size_t dim_time, const uint16_t* d_grad_out,
                                 size_t grad_pitch, size_t grad_col, float* d_partials,
                                 size_t partial_rows, float* d_grad_w, float* d_grad_bias,
                                 int device, void* stream) {
  return guarded([&] {
    gf::time_encode_backward_bf16(d_t, d_w, d_bias, n, dim_time, d_grad_out, grad_pitch, grad_col,
                                  d_partials, partial_rows, d_grad_w, d_grad_bias, device,
                                  as_stream(stream));
  });
}

int gf_edge_score(const float* d_src, const float* d_dst, const float* d_w, const float* d_bias,
                  size_t num_src, size_t num_dst, size_t dim, float* d_out, int device,
                  void* stream) {
  return guarded([&] {
    gf::edge_score_forward(d_src, d_dst, d_w, d_bias, num_src, num_dst, dim, d_out, device,
                           as_stream(stream));
  });
}
int gf_edge_score_backward_partial_rows(size_t num_src, size_t* rows) {
  return guarded([&] {
    GF_REQUIRE(rows != nullptr, "gf_edge_score_backward_partial_rows: null output");
    *rows = gf::edge_score_backward_partial_rows(num_src);
  });
}
int gf_edge_score_backward(const float* d_src, const float* d_dst, const float* d_w,
                           size_t num_src, size_t num_dst, size_t dim, const float* d_grad_out,
                           float* d_partials, size_t partial_rows, float* d_grad_src,
                           float* d_grad_dst, float* d_grad_w, float* d_grad_bias, int device,
                           void* stream) {
  return guarded([&] {
    gf::edge_score_backward(d_src, d_dst, d_w, num_src, num_dst, dim, d_grad_out, d_partials,
                            partial_rows, d_grad_src, d_grad_dst, d_grad_w, d_grad_bias, device,
                            as_stream(stream));
  });
}

int gf_edge_score_bf16(const uint16_t* d_src, const uint16_t* d_dst, const float* d_w,
                       const float* d_bias, size_t num_src, size_t num_dst, size_t dim,
                       float* d_out, int device, void* stream) {
  return guarded([&] {
    gf::edge_score_bf16_forward(d_src, d_dst, d_w, d_bias, num_src, num_dst, dim, d_out, device,
                                as_stream(stream));
  });
}
int gf_edge_score_backward_bf16(const uint16_t* d_src, const uint16_t* d_dst, const float* d_w,
                                size_t num_src, size_t num_dst, size_t dim,
                                const float* d_grad_out, float* d_partials, size_t partial_rows,
                                uint16_t* d_grad_src, uint16_t* d_grad_dst, float* d_grad_w,
                                float* d_grad_bias, int device, void* stream) {
  return guarded([&] {
    gf::edge_score_bf16_backward(d_src, d_dst, d_w, num_src, num_dst, dim, d_grad_out, d_partials,
                                 partial_rows, d_grad_src, d_grad_dst, d_grad_w, d_grad_bias,
                                 device, as_stream(stream));
  });
}

static_assert(GF_LAYER_EPILOGUE_MAX_WIDTH == gf::kLayerEpilogueMaxWidth,
              "gnnflow_hip.h and block_ops.hpp disagree on the layer-epilogue width");
int gf_layer_epilogue(const float* d_x, const float* d_gamma, const float* d_beta,
                      size_t num_rows, size_t dim, float eps, float p, uint64_t seed,
                      float* d_out, float* d_mean, float* d_rstd, int device, void* stream) {
  return guarded([&] {
    gf::layer_epilogue_forward(d_x, d_gamma, d_beta, num_rows, dim, eps, p, seed, d_out, d_mean,
                               d_rstd, device, as_stream(stream));
  });
}
int gf_layer_epilogue_backward_partial_rows(size_t num_rows, size_t* rows) {
  return guarded([&] {
    GF_REQUIRE(rows != nullptr, "gf_layer_epilogue_backward_partial_rows: null output");
    *rows = gf::layer_epilogue_backward_partial_rows(num_rows);
  });
}
int gf_layer_epilogue_backward(const float* d_x, const float* d_gamma, const float* d_mean,
                               const float* d_rstd, size_t num_rows, size_t dim, float p,
                               uint64_t seed, const float* d_grad_out, float* d_partials,
                               size_t partial_rows, float* d_grad_x, float* d_grad_gamma,
                               float* d_grad_beta, int device, void* stream) {
  return guarded([&] {
    gf::layer_epilogue_backward(d_x, d_gamma, d_mean, d_rstd, num_rows, dim, p, seed, d_grad_out,
                                d_partials, partial_rows, d_grad_x, d_grad_gamma, d_grad_beta,
                                device, as_stream(stream));
  });
}
int gf_layer_epilogue_bf16(const uint16_t* d_x, const float* d_gamma, const float* d_beta,
                           size_t num_rows, size_t dim, float eps, float p, uint64_t seed,
                           float* d_out, float* d_mean, float* d_rstd, int device,
                           void* stream) {
  return guarded([&] {
    gf::layer_epilogue_bf16_forward(d_x, d_gamma, d_beta, num_rows, dim, eps, p, seed, d_out,
                                    d_mean, d_rstd, device, as_stream(stream));
  });
}
int gf_layer_epilogue_backward_bf16(const uint16_t* d_x, const float* d_gamma,
                                    const float* d_mean, const float* d_rstd, size_t num_rows,
                                    size_t dim, float p, uint64_t seed, const float* d_grad_out,
                                    float* d_partials, size_t partial_rows, uint16_t* d_grad_x,
                                    float* d_grad_gamma, float* d_grad_beta, int device,
                                    void* stream) {
  return guarded([&] {
    gf::layer_epilogue_bf16_backward(d_x, d_gamma, d_mean, d_rstd, num_rows, dim, p, seed,
                                     d_grad_out, d_partials, partial_rows, d_grad_x, d_grad_gamma,
                                     d_grad_beta, device, as_stream(stream));
  });
}

int gf_gru_cell(const float* d_gi, const float* d_gh, const float* d_hx, const void* d_residual,
                int residual_bf16, size_t n, size_t hidden, size_t num_last, float* d_out,
                float* d_last, int device, void* stream) {
  return guarded([&] {
    gf::gru_cell_forward(d_gi, d_gh, d_hx, d_residual, residual_bf16, n, hidden, num_last, d_out,
                         d_last, device, as_stream(stream));
  });
}
int gf_gru_cell_backward(const float* d_gi, const float* d_gh, const float* d_hx, size_t n,
                         size_t hidden, const float* d_grad_out, float* d_grad_gi,
                         float* d_grad_gh, float* d_grad_hx, int device, void* stream) {
  return guarded([&] {
    gf::gru_cell_backward(d_gi, d_gh, d_hx, n, hidden, d_grad_out, d_grad_gi, d_grad_gh,
                          d_grad_hx, device, as_stream(stream));
  });
}
int gf_gru_cell_bf16(const uint16_t* d_gi, const uint16_t* d_gh, const float* d_hx,
                     const void* d_residual, int residual_bf16, size_t n, size_t hidden,
                     size_t num_last, float* d_out, float* d_last, int device, void* stream) {
  return guarded([&] {
    gf::gru_cell_bf16_forward(d_gi, d_gh, d_hx, d_residual, residual_bf16, n, hidden, num_last,
                              d_out, d_last, device, as_stream(stream));
  });
}
int gf_gru_cell_backward_bf16(const uint16_t* d_gi, const uint16_t* d_gh, const float* d_hx,
                              size_t n, size_t hidden, const float* d_grad_out,
                              uint16_t* d_grad_gi, uint16_t* d_grad_gh, float* d_grad_hx,
                              int device, void* stream) {
  return guarded([&] {
    gf::gru_cell_bf16_backward(d_gi, d_gh, d_hx, n, hidden, d_grad_out, d_grad_gi, d_grad_gh,
                               d_grad_hx, device, as_stream(stream));
  });
}

static_assert(GF_LINK_METRICS_MAX_SCORES == gf::kLinkMetricsMaxScores &&
                  GF_LINK_METRICS_TILE == gf::kLinkMetricsTile &&
                  GF_LINK_METRICS_PARTIAL_WORDS == gf::kLinkMetricsPartialWords,
              "gnnflow_hip.h and block_ops.hpp disagree on the link-metrics constants");
int gf_link_metrics_partial_rows(size_t num_pos, size_t* rows) {
  return guarded([&] {
    GF_REQUIRE(rows != nullptr, "gf_link_metrics_partial_rows: null output");
    *rows = gf::link_metrics_partial_rows(num_pos);
  });
}
int gf_link_metrics(const float* d_pos, const float* d_neg, size_t num_pos, size_t num_neg,
                    void* d_partials, size_t partial_rows, double* d_out, double* d_acc,
                    int device, void* stream) {
  return guarded([&] {
    gf::link_metrics(d_pos, d_neg, num_pos, num_neg, d_partials, partial_rows, d_out, d_acc,
                     device, as_stream(stream));
  });
}

static_assert(GF_EDGE_RANK_MAX_K == gf::kEdgeRankMaxK && GF_EDGE_RANK_CHUNK == gf::kEdgeRankChunk,
              "gnnflow_hip.h and block_ops.hpp disagree on the edge-rank constants");
int gf_edge_rank_scratch(size_t num_src, size_t num_cand, size_t k, size_t* bytes) {
  return guarded([&] {
    GF_REQUIRE(bytes != nullptr, "gf_edge_rank_scratch: null output");
    *bytes = gf::edge_rank_scratch_bytes(num_src, num_cand, k);
  });
}
int gf_edge_rank(const float* d_src, const float* d_cand, const float* d_w, const float* d_bias,
                 size_t num_src, size_t num_cand, size_t dim, size_t k, const float* d_ref_score,
                 const int64_t* d_skip, void* d_scratch, size_t scratch_bytes, float* d_values,
                 int64_t* d_indices, int64_t* d_greater, int64_t* d_equal, int device,
                 void* stream) {
  return guarded([&] {
    gf::edge_rank(d_src, d_cand, d_w, d_bias, num_src, num_cand, dim, k, d_ref_score, d_skip,
                  nullptr, d_scratch, scratch_bytes, d_values, d_indices, d_greater, d_equal,
                  device, as_stream(stream));
  });
}
int gf_edge_rank_masked(const float* d_src, const float* d_cand, const float* d_w,
                        const float* d_bias, size_t num_src, size_t num_cand, size_t dim, size_t k,
                        const float* d_ref_score, const int64_t* d_skip, const uint64_t* d_exclude,
                        void* d_scratch, size_t scratch_bytes, float* d_values, int64_t* d_indices,
                        int64_t* d_greater, int64_t* d_equal, int device, void* stream) {
  return guarded([&] {
    gf::edge_rank(d_src, d_cand, d_w, d_bias, num_src, num_cand, dim, k, d_ref_score, d_skip,
                  d_exclude, d_scratch, scratch_bytes, d_values, d_indices, d_greater, d_equal,
                  device, as_stream(stream));
  });
}

static_assert(GF_LINK_LOSS_TILE == gf::kLinkLossTile &&
                  GF_LINK_LOSS_SINGLE_TILES == gf::kLinkLossSingleTiles &&
                  GF_LINK_LOSS_MAX_PARTIAL_ROWS == gf::kLinkLossMaxPartialRows &&
                  GF_LINK_LOSS_ACC_FIELDS == gf::kLinkLossAccFields,
              "gnnflow_hip.h and block_ops.hpp disagree on the link-loss constants");
int gf_link_loss_partial_rows(size_t num_pos, size_t num_neg, size_t* rows) {
  return guarded([&] {
    GF_REQUIRE(rows != nullptr, "gf_link_loss_partial_rows: null output");
    *rows = gf::link_loss_partial_rows(num_pos, num_neg);
  });
}
int gf_link_loss(const float* d_pos, const float* d_neg, size_t num_pos, size_t num_neg,
                 double* d_partials, size_t partial_rows, float* d_out, double* d_acc, int device,
                 void* stream) {
  return guarded([&] {
    gf::link_loss_forward(d_pos, d_neg, num_pos, num_neg, d_partials, partial_rows, d_out, d_acc,
                          device, as_stream(stream));
  });
}
int gf_link_loss_backward(const float* d_pos, const float* d_neg, size_t num_pos, size_t num_neg,
                          const float* d_grad_out, float* d_grad_pos, float* d_grad_neg,
                          int device, void* stream) {
  return guarded([&] {
    gf::link_loss_backward(d_pos, d_neg, num_pos, num_neg, d_grad_out, d_grad_pos, d_grad_neg,
                           device, as_stream(stream));
  });
}
int gf_link_loss_bf16(const uint16_t* d_pos, const uint16_t* d_neg, size_t num_pos,
                      size_t num_neg, double* d_partials, size_t partial_rows, float* d_out,
                      double* d_acc, int device, void* stream) {
  return guarded([&] {
    gf::link_loss_bf16_forward(d_pos, d_neg, num_pos, num_neg, d_partials, partial_rows, d_out,
                               d_acc, device, as_stream(stream));
  });
}
int gf_link_loss_backward_bf16(const uint16_t* d_pos, const uint16_t* d_neg, size_t num_pos,
                               size_t num_neg, const float* d_grad_out, uint16_t* d_grad_pos,
                               uint16_t* d_grad_neg, int device, void* stream) {
  return guarded([&] {
    gf::link_loss_bf16_backward(d_pos, d_neg, num_pos, num_neg, d_grad_out, d_grad_pos,
                                d_grad_neg, device, as_stream(stream));
  });
}

static_assert(GF_DST_SET_TILE_WORDS == gf::kDstSetTileWords,
              "gnnflow_hip.h and batch_stream.hpp disagree on the destination-set tile");
int gf_batch_assemble(const int64_t* d_src, const int64_t* d_dst, const float* d_time,
                      size_t num_rows, size_t lo, size_t hi, size_t neg_ratio,
                      const int64_t* d_dl, const int64_t* d_dl_count, uint64_t seed,
                      uint64_t epoch, uint64_t first_row, int64_t* d_roots, float* d_ts,
                      int device, void* stream) {
  return guarded([&] {
    gf::batch_assemble(d_src, d_dst, d_time, num_rows, lo, hi, neg_ratio, d_dl, d_dl_count, seed,
                       epoch, first_row, d_roots, d_ts, device, as_stream(stream));
  });
}
int gf_batch_assemble_many(const int64_t* d_src, const int64_t* d_dst, const float* d_time,
                           size_t num_rows, const int64_t* d_borders, size_t num_batches,
                           size_t max_batch_rows, size_t neg_ratio, const int64_t* d_dl,
                           const int64_t* d_dl_count, uint64_t seed, uint64_t epoch,
                           uint64_t first_row, int64_t* d_roots, float* d_ts, size_t capacity,
                           int device, void* stream) {
  return guarded([&] {
    gf::batch_assemble_many(d_src, d_dst, d_time, num_rows, d_borders, num_batches,
                            max_batch_rows, neg_ratio, d_dl, d_dl_count, seed, epoch, first_row,
                            d_roots, d_ts, capacity, device, as_stream(stream));
  });
}
int gf_dst_set_mark(const int64_t* d_ids, size_t n, uint64_t* d_bitmap, size_t num_nodes,
                    uint64_t* d_out_of_range, int device, void* stream) {
  return guarded([&] {
    gf::dst_set_mark(d_ids, n, d_bitmap, num_nodes, d_out_of_range, device, as_stream(stream));
  });
}
int gf_dst_set_scratch_bytes(size_t num_nodes, size_t* bytes) {
  return guarded([&] {
    GF_REQUIRE(bytes != nullptr, "gf_dst_set_scratch_bytes: null output");
    *bytes = gf::dst_set_scratch_bytes(num_nodes);
  });
}
int gf_dst_set_compact(const uint64_t* d_bitmap, size_t num_nodes, int64_t* d_ids,
                       size_t ids_capacity, int64_t* d_count, void* d_scratch,
                       size_t scratch_bytes, int device, void* stream) {
  return guarded([&] {
    gf::dst_set_compact(d_bitmap, num_nodes, d_ids, ids_capacity, d_count, d_scratch,
                        scratch_bytes, device, as_stream(stream));
  });
}

int gf_walk_position_counts(const int64_t* d_nodes, const int64_t* d_ref, size_t rows,
                            size_t walks, size_t len1, size_t ref_walks, size_t ref_len1,
                            int32_t* d_out, int device, void* stream) {
  return guarded([&] {
    gf::walk_position_counts(d_nodes, d_ref, rows, walks, len1, ref_walks, ref_len1, d_out,
                             device, as_stream(stream));
  });
}

int gf_debug_philox(const uint64_t* d_in, size_t n, uint32_t* d_out, void* stream) {
  return guarded([&] {
    GF_REQUIRE(n == 0 || (d_in != nullptr && d_out != nullptr), "gf_debug_philox: null buffer");
    gf::philox_on_device(d_in, n, d_out, as_stream(stream));
  });
}
int gf_debug_part_reused_roots(uint64_t* out) {
  return guarded([&] {
    GF_REQUIRE(out != nullptr, "gf_debug_part_reused_roots: null output");
    *out = gf::part_reused_roots();
  });
}
int gf_debug_merge_recounts(uint64_t* out) {
  return guarded([&] {
    GF_REQUIRE(out != nullptr, "gf_debug_merge_recounts: null output");
    *out = gf::merge_recounts();
  });
}
int gf_debug_lru_recounts(uint64_t* out) {
  return guarded([&] {
    GF_REQUIRE(out != nullptr, "gf_debug_lru_recounts: null output");
    *out = gf::lru_recounts();
  });
}
int gf_debug_part_host_us(double* out, int reset) {
  return guarded([&] {
    GF_REQUIRE(out != nullptr, "gf_debug_part_host_us: null output");
    gf::part_host_us(out, reset != 0);
  });
}

}  // extern "C"
