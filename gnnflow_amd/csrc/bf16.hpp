// bfloat16 as the kernels carry it: a uint16_t holding the upper half of a float32.  widen() is
// exact (a 16-bit shift); narrow() rounds to nearest even and is what
// tensor.to(torch.bfloat16) gives: infinities stay, a finite value beyond the largest bfloat16
// becomes an infinity, and every NaN becomes the quiet NaN 0x7FC0.  The bfloat16 kernels widen
// on load, compute as their float32 siblings do and narrow once on store.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace gf {

__device__ inline float widen(float x) { return x; }
__device__ inline float widen(uint16_t x) {
  return __uint_as_float(static_cast<uint32_t>(x) << 16);
}
__device__ inline uint16_t narrow(float x) {
  const uint32_t u = __float_as_uint(x);
  if ((u & 0x7fffffffu) > 0x7f800000u) return 0x7fc0;
  return static_cast<uint16_t>((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}

// the value as a kernel templated on its element type T stores it: as it is, or narrowed
template <class T> __device__ inline T narrow_to(float x);
template <> __device__ inline float narrow_to<float>(float x) { return x; }
template <> __device__ inline uint16_t narrow_to<uint16_t>(float x) { return narrow(x); }

}  // namespace gf
