// patch_project.hip: DyGFormer's patching and channel projection without the channel -- the rows
// of a [*, L] plane of ids are gathered from a feature table (or the time encoding of a plane of
// time deltas is evaluated) straight into LDS and multiplied there by the projection weight on
// the float32 matrix cores, so that only [*, L / P, C] is ever written.
// Contract: include/gnnflow_hip.h (gf_patch_project).
#pragma once

#include <cstddef>
#include <cstdint>

#include <hip/hip_runtime.h>

namespace gf {

constexpr size_t kPatchMaxLength = 512;             // GF_PATCH_MAX_LENGTH
constexpr size_t kPatchMaxWidth = 1024;             // GF_PATCH_MAX_WIDTH
constexpr size_t kPatchMaxPatchWidth = 4096;        // GF_PATCH_MAX_PATCH_WIDTH, P * d
constexpr size_t kPatchMaxChannels = 128;           // GF_PATCH_MAX_CHANNELS
constexpr size_t kPatchMaxPartialRows = 256;        // GF_PATCH_MAX_PARTIAL_ROWS
constexpr size_t kPatchMaxWorkspaceFloats = size_t{16} << 20;      // 64 MiB of float32

// Where the rows x[r, l, :] come from.  Table form: d_ids [num_rows, L] and d_table [table_rows,
// dim]; time form: d_delta_t [num_rows, L] and the encoder's d_time_weight, d_time_bias [dim].
// Exactly one form is given (the other's pointers are null).  d_lengths [num_rows] or null for
// "every slot filled".
struct PatchSource {
  const int64_t* d_ids;
  const float* d_table;
  size_t table_rows;
  const float* d_delta_t;
  const float* d_time_weight;
  const float* d_time_bias;
  const int32_t* d_lengths;
};

// out[m, c] = bias[c] + sum_k x_patch[m, k] * weight[c, k] over the num_rows * (length / patch)
// patches m, k < patch * dim, c < channels.  One launch; num_rows == 0 launches nothing.
void patch_project_forward(const PatchSource& src, size_t num_rows, size_t length, size_t patch,
                           size_t dim, const float* d_weight, const float* d_bias,
                           size_t channels, float* d_out, int device, hipStream_t stream);

// Partial rows of the backward's workspace for num_patches patches: each row holds channels *
// (patch_width + 1) floats; at most kPatchMaxPartialRows rows and kPatchMaxWorkspaceFloats floats.
size_t patch_project_backward_partial_rows(size_t num_patches, size_t channels,
                                           size_t patch_width);

// grad_weight[c, k] = sum_m grad_out[m, c] * x_patch[m, k], grad_bias[c] = sum_m grad_out[m, c],
// x re-gathered (re-encoded) from `src`; either may be null.  Two launches, fixed order.
void patch_project_backward(const PatchSource& src, size_t num_rows, size_t length, size_t patch,
                            size_t dim, size_t channels, const float* d_grad_out,
                            float* d_partials, size_t partial_rows, float* d_grad_weight,
                            float* d_grad_bias, int device, hipStream_t stream);

}  // namespace gf
