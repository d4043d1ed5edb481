// What the Pillow-exact image kernels share (preprocess.hip: evaluation-time resize / normalise / pad; augment.hip: the
// training augmentation): the tile geometry, Pillow's 8-bit fixed-point rounding, and the 4-wide NCHW / mask stores.
#pragma once
#include "common.h"

#include <stdint.h>

namespace egtr_image {
constexpr int kTW = EGTR_PREPROCESS_TILE_W;   // output tile width (columns)
constexpr int kTH = 8;                  // output tile height (rows)
constexpr int kThreads = 256;           // 8 rows x 32 lanes x 4 columns
constexpr int kStage = 16384;           // LDS bytes for staged input rows
constexpr int kMaxRows = 32;            // input rows per chunk
constexpr int kHRow = kTW * 3;          // bytes of one horizontally resampled row in LDS
constexpr int kPrec = 22;               // Pillow's PRECISION_BITS
static_assert(EGTR_PREPROCESS_STAGE_BYTES == kStage - 30, "header constant out of date");

__device__ __forceinline__ int clip8(int acc) {
  const int v = acc >> kPrec;
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// round to nearest even, as torch's float -> bfloat16 (the table holds no NaN)
__device__ __forceinline__ unsigned short to_bf16(float v) {
  unsigned u = __float_as_uint(v);
  u += 0x7fffu + ((u >> 16) & 1u);
  return (unsigned short)(u >> 16);
}

__device__ __forceinline__ void store4(float* p, const float* v, int n, bool vec) {
  if (vec && n >= 4) {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
    for (int i = 0; i < 4 && i < n; ++i) p[i] = v[i];
  }
}

__device__ __forceinline__ void store4(unsigned short* p, const float* v, int n, bool vec) {
  if (vec && n >= 4) {
    const unsigned lo = to_bf16(v[0]) | ((unsigned)to_bf16(v[1]) << 16);
    const unsigned hi = to_bf16(v[2]) | ((unsigned)to_bf16(v[3]) << 16);
    *reinterpret_cast<uint2*>(p) = make_uint2(lo, hi);
  } else {
    for (int i = 0; i < 4 && i < n; ++i) p[i] = to_bf16(v[i]);
  }
}

__device__ __forceinline__ void store4(long long* p, const int* m, int n, bool vec) {
  if (vec && n >= 4) {
    reinterpret_cast<longlong2*>(p)[0] = make_longlong2(m[0], m[1]);
    reinterpret_cast<longlong2*>(p)[1] = make_longlong2(m[2], m[3]);
  } else {
    for (int i = 0; i < 4 && i < n; ++i) p[i] = m[i];
  }
}
}  // namespace egtr_image
