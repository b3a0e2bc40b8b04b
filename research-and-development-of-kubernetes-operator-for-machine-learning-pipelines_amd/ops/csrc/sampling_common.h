// Device helpers shared by the sampling kernels (sampling.hip, sampling_ext.hip).
#pragma once

#include "common.h"

namespace mlop {

constexpr int kSampleThreads = 256;

// monotone uint image of a float: a > b  <=>  fkey(a) > fkey(b) (-0 < +0)
__device__ __forceinline__ uint32_t fkey(float f) {
  uint32_t b = __float_as_uint(f);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// (value, index) argmax with ties to the smallest index; NaN never wins
__device__ __forceinline__ void amax_merge(float& v, int& i, float ov, int oi) {
  if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
}

}  // namespace mlop
