// cos(w * t + b), the time encoding's one expression: time_encode.hip (forward and, through
// te_arg, backward), neighbor_sequence.hip (the time part of a token) and pair_sequence.hip (the
// time part of a pair's slots) evaluate it through this header and nowhere else, so that they
// agree bit for bit.  The library is built with -ffp-contract=off and without fast-math: the
// argument is one multiply and one add, each rounded.
// cosf is the precise form: a real timestamp times the first frequency is an argument of 1e6 rad
// and more, where __cosf is wrong in the first digit.
#pragma once

#include <hip/hip_runtime.h>

namespace gf {

__device__ __forceinline__ float te_arg(float w, float t, float b) { return w * t + b; }
__device__ __forceinline__ float te_cos(float w, float t, float b) { return cosf(te_arg(w, t, b)); }

}  // namespace gf
