// The order key of a float32 score, shared by the evaluators that define an order among scores.
#pragma once
#include <hip/hip_runtime.h>

// A larger key ranks earlier.  NaN is the smallest key (numpy sorts NaN last), -0 = +0.
__device__ __forceinline__ unsigned score_key(float x) {
  if (x != x) return 0u;
  if (x == 0.f) x = 0.f;
  const unsigned u = __float_as_uint(x);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
