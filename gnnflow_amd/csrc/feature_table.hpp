// What the readers of optional feature tables share (neighbor_aggregate.hip,
// neighbor_sequence.hip, pair_sequence.hip): the host check of a float table [rows, width] as it
// arrives over the C ABI, and the zero of a column of one float or four.  How a kernel sees a table stays with its
// reader: each packs what it checked here into its own argument struct.
#pragma once

#include "common.hpp"

namespace gf {

// A table is absent (feats null, width 0) or has 1 .. max_width columns; `has_out` is false when
// a table that is given lacks the output it needs.  `name` reads "the node table".
inline void check_feature_table(const std::string& reader, const char* name, const float* feats,
                                size_t width, size_t max_width, bool has_out = true) {
  if (feats == nullptr) {
    GF_REQUIRE(width == 0, reader + ": " + name + " is null but its width is not 0");
    return;
  }
  GF_REQUIRE(width >= 1 && width <= max_width,
             reader + ": width of " + name + " outside 1 .. " + std::to_string(max_width));
  GF_REQUIRE(has_out, reader + ": null output of " + name);
}

__device__ __forceinline__ void clear(float& a) { a = 0.0f; }
__device__ __forceinline__ void clear(float4& a) { a = make_float4(0.0f, 0.0f, 0.0f, 0.0f); }

}  // namespace gf
