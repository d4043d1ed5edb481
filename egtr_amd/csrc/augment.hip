// The reference's training augmentation on the device, bit-identical to its PIL chain (model/deformable_detr.py:322-385,
// model/transform.py): RandomHorizontalFlip, then one random-scale Image.resize, or a resize to 400/500/600, an optional
// Image.crop and a second random-scale resize; then the rescale / normalise / pad of preprocess.hip.  The random draws
// are made on the host (feature_extraction.sample_augmentation); these kernels only execute them.
//
// Every resize is Pillow's 8-bit ImagingResample as in preprocess.hip (horizontal pass to uint8, vertical pass to uint8,
// 22-bit fixed-point weights from the host).  Two things are added to that kernel's structure:
//   mirror  a flipped image is never materialised: the pass over the flipped image F[x] = U[in_w - 1 - x] is
//           sum_k w[xx][k] * U[in_w - 1 - (xmin[xx] + k)] with the table of the unflipped size.  The tile stages the
//           mirrored window of each input row and indexes it backwards.  (Resize-then-flip is NOT the same: the
//           fixed-point table of an axis is not symmetric in general.)
//   window  a pass may produce only the rows [off_y, off_y + out_h) and columns [off_x, off_x + out_w) of its resize:
//           each output byte of a Pillow resize depends only on its own table row, so Image.crop after a resize is that
//           window.
// augment_tile<unsigned char>: the first resize of the two-resize branch, written as uint8 HWC into the workspace (crop
//   window only).  The second resize reads those rounded bytes, so the two cannot be merged into one resampling.
// augment_tile<float | bf16>: the final resize from the raw image (one-resize branch, mirrored or not) or from the
//   workspace (two-resize branch), LUT, NCHW and mask stores, zero padding -- preprocess_tile's body.
// augment_hpass: the horizontal pass alone (of the input rows the window needs) into the workspace, for a pass whose tile
//   window does not fit the LDS stage.
#include "image_common.h"

#include <type_traits>

namespace {
using namespace egtr_image;
constexpr int kDescWords = EGTR_AUGMENT_DESC_WORDS;

// descriptor fields (int64 each), see include/egtr_hip.h
enum { D_SRC, D_STRIDE, D_IN_H, D_IN_W, D_OUT_H, D_OUT_W, D_TAB_X, D_KX, D_TAB_Y, D_KY, D_OFF_X, D_OFF_Y, D_FULL_W,
       D_FULL_H, D_FLAGS, D_PRE, D_DST };
static_assert(D_DST + 1 == kDescWords, "descriptor layout out of date");
constexpr long long kMirror = EGTR_AUGMENT_MIRROR, kSrcWs = EGTR_AUGMENT_SRC_WORKSPACE, kPrepass = EGTR_AUGMENT_PREPASS;

__device__ __forceinline__ const unsigned char* source(const long long* d, const unsigned char* ws) {
  return (d[D_FLAGS] & kSrcWs) ? ws + d[D_SRC] : reinterpret_cast<const unsigned char*>(d[D_SRC]);
}

// T = unsigned char: uint8 HWC [out_h][out_w][3] at ws + D_DST, grid over the largest window of the batch.
// T = float / unsigned short (bf16): NCHW planes + mask of the padded [H, W] canvas, grid over the canvas.
template <typename T>
__global__ __launch_bounds__(kThreads) void augment_tile(const long long* __restrict__ desc,
                                                         const int* __restrict__ coeffs,
                                                         const float* __restrict__ lut, int H, int W,
                                                         unsigned char* __restrict__ ws, T* __restrict__ out,
                                                         long long* __restrict__ mask) {
  constexpr bool kBytes = std::is_same<T, unsigned char>::value;
  __shared__ __attribute__((aligned(16))) unsigned char stage[kStage];
  __shared__ __attribute__((aligned(16))) unsigned char hbuf[kMaxRows * kHRow];
  __shared__ float slut[kBytes ? 1 : 3 * 256];
  const int b = blockIdx.z, t = threadIdx.x;
  const int x0 = blockIdx.x * kTW, y0 = blockIdx.y * kTH;
  const int y = y0 + (t >> 5), x = x0 + (t & 31) * 4;
  const long long* d = desc + (size_t)b * kDescWords;
  const int out_h = (int)d[D_OUT_H], out_w = (int)d[D_OUT_W];
  float v[3][4] = {};
  int m[4] = {};
  int res[3][4] = {};
  bool live = false, fits = true;
  int xe = 0;
  if (x0 < out_w && y0 < out_h) {   // uniform over the workgroup
    if (!kBytes)
      for (int i = t; i < 3 * 256; i += kThreads) slut[i] = lut[i];
    const long long flags = d[D_FLAGS];
    const bool pre = (flags & kPrepass) != 0;
    const bool mirror = !pre && (flags & kMirror) != 0;
    const long long stride = pre ? 3ll * out_w : d[D_STRIDE];
    const int in_w = (int)d[D_IN_W];
    const int ox = (int)d[D_OFF_X], oy = (int)d[D_OFF_Y];
    xe = min(x0 + kTW, out_w);
    const int ye = min(y0 + kTH, out_h);
    const int* bx = coeffs + d[D_TAB_X];
    const int* wx = bx + 2 * (size_t)d[D_FULL_W];
    const int kx = (int)d[D_KX];
    const int* by = coeffs + d[D_TAB_Y];
    const int* wy = by + 2 * (size_t)d[D_FULL_H];
    const int ky = (int)d[D_KY];
    // the prepass region starts at the first input row the window reads, by[2 * oy]
    const unsigned char* src = pre ? ws + d[D_PRE] - (long long)by[2 * oy] * stride : source(d, ws);
    // input window of the tile in the coordinates of the (possibly flipped) image: columns [c0, c1), rows [r0, r1)
    // (bounds are non-decreasing in the output index)
    const int c0 = pre ? x0 : bx[2 * (ox + x0)];
    const int c1 = pre ? xe : bx[2 * (ox + xe - 1)] + bx[2 * (ox + xe - 1) + 1];
    const int r0 = by[2 * (oy + y0)], r1 = by[2 * (oy + ye - 1)] + by[2 * (oy + ye - 1) + 1];
    const int cs = mirror ? in_w - c1 : c0;               // first staged column of the stored image
    const int L = (c1 - c0) * 3;                          // bytes of one staged input row
    fits = L <= EGTR_PREPROCESS_STAGE_BYTES;              // else the host should have routed it through the prepass
    const int pu = (min(L, EGTR_PREPROCESS_STAGE_BYTES) + 30) >> 4;   // 16-byte units per row, misalignment included
    const int chunk = min(kMaxRows, kStage / (pu * 16));
    const int ncols = xe - x0;
    int ymin = 0, yn = 0;
    const int* wyy = wy;
    live = y < ye;
    if (live) {
      ymin = by[2 * (oy + y)];
      yn = by[2 * (oy + y) + 1];
      wyy = wy + (size_t)(oy + y) * ky;
    }
    int acc[3][4] = {};
    for (int rc = r0; fits && rc < r1; rc += chunk) {
      const int nr = min(chunk, r1 - rc);
      // (A) stage rows rc .. rc+nr-1: aligned 16-byte loads covering [p, p + L); every loaded granule holds a byte of
      // the row, so no load leaves the row's pages
      for (int i = t; i < nr * pu; i += kThreads) {
        const int r = i / pu, u = i - r * pu;
        const uintptr_t p = reinterpret_cast<uintptr_t>(src + (size_t)(rc + r) * stride + (size_t)cs * 3);
        const uintptr_t a = (p & ~(uintptr_t)15) + (uintptr_t)u * 16;
        if (a < p + (uintptr_t)L)
          *reinterpret_cast<uint4*>(stage + (r * pu + u) * 16) = *reinterpret_cast<const uint4*>(a);
      }
      __syncthreads();
      // (B) horizontal pass of the staged rows into hbuf (uint8, like Pillow's intermediate image)
      for (int i = t; i < nr * kTW; i += kThreads) {
        const int r = i / kTW, j = i - r * kTW;
        if (j >= ncols) continue;
        const uintptr_t p = reinterpret_cast<uintptr_t>(src + (size_t)(rc + r) * stride + (size_t)cs * 3);
        const unsigned char* row = stage + r * pu * 16 + (int)(p & 15);
        unsigned char* h = hbuf + r * kHRow + j * 3;
        if (pre) {
          h[0] = row[j * 3];
          h[1] = row[j * 3 + 1];
          h[2] = row[j * 3 + 2];
        } else {
          const int xx = ox + x0 + j;
          const int xm = bx[2 * xx] - c0, n = bx[2 * xx + 1];
          const int* w = wx + (size_t)xx * kx;
          // pixel c of the flipped image sits at staged pixel c1 - 1 - c
          const unsigned char* q = mirror ? row + (c1 - c0 - 1 - xm) * 3 : row + xm * 3;
          const int step = mirror ? -3 : 3;
          int s0 = 1 << (kPrec - 1), s1 = s0, s2 = s0;
          for (int k = 0; k < n; ++k, q += step) {
            const int wk = w[k];
            s0 += wk * q[0];
            s1 += wk * q[1];
            s2 += wk * q[2];
          }
          h[0] = (unsigned char)clip8(s0);
          h[1] = (unsigned char)clip8(s1);
          h[2] = (unsigned char)clip8(s2);
        }
      }
      __syncthreads();
      // (C) vertical taps of this chunk: 12 bytes = 4 pixels x RGB per lane
      if (live) {
        const int k0 = max(0, rc - ymin), k1 = min(yn, rc + nr - ymin);
        for (int k = k0; k < k1; ++k) {
          const int wk = wyy[k];
          const unsigned* hp = reinterpret_cast<const unsigned*>(hbuf + (ymin + k - rc) * kHRow + (x - x0) * 3);
          const unsigned q[3] = {hp[0], hp[1], hp[2]};
#pragma unroll
          for (int e = 0; e < 12; ++e) acc[e % 3][e / 3] += wk * (int)((q[e >> 2] >> ((e & 3) * 8)) & 255u);
        }
      }
      // the next chunk's stage writes come after (B) of this one, its hbuf writes after the next (A) barrier
    }
    for (int i = 0; i < 4; ++i)
      for (int c = 0; c < 3; ++c) res[c][i] = clip8(acc[c][i] + (1 << (kPrec - 1)));
  }
  if constexpr (kBytes) {
    // a window that does not fit is a host routing error: the final kernel then sees zeros instead of NaN, so the
    // host check (prepare) is what guards it; nothing is written out of the window
    if (live) {
      unsigned char* o = ws + d[D_DST] + ((size_t)y * out_w + x) * 3;
      for (int i = 0; i < 4 && x + i < xe; ++i)
        for (int c = 0; c < 3; ++c) o[i * 3 + c] = fits ? (unsigned char)res[c][i] : 0;
    }
  } else {
    if (live) {
      for (int i = 0; i < 4; ++i) {
        if (x + i >= xe) continue;
        m[i] = 1;
        for (int c = 0; c < 3; ++c) v[c][i] = fits ? slut[c * 256 + res[c][i]] : __builtin_nanf("");
      }
    }
    if (y < H) {
      const bool vec = (W & 3) == 0;
      for (int c = 0; c < 3; ++c) store4(out + (((size_t)b * 3 + c) * H + y) * W + x, v[c], W - x, vec);
      store4(mask + ((size_t)b * H + y) * W + x, m, W - x, vec);
    }
  }
}

// The horizontal pass of the input rows the window reads, [by[oy], by[oy + out_h - 1] + n), into ws + D_PRE
// ([rows][out_w][3] bytes), mirror and column window applied.
__global__ __launch_bounds__(256) void augment_hpass(const long long* __restrict__ desc,
                                                     const int* __restrict__ coeffs, unsigned char* __restrict__ ws) {
  const long long* d = desc + (size_t)blockIdx.z * kDescWords;
  const int xw = blockIdx.x * 256 + threadIdx.x;
  const int in_w = (int)d[D_IN_W], out_h = (int)d[D_OUT_H], out_w = (int)d[D_OUT_W];
  if ((d[D_FLAGS] & kPrepass) == 0 || out_h <= 0 || xw >= out_w) return;
  const int* by = coeffs + d[D_TAB_Y];
  const int oy = (int)d[D_OFF_Y];
  const int r0 = by[2 * oy], r1 = by[2 * (oy + out_h - 1)] + by[2 * (oy + out_h - 1) + 1];
  const int row = r0 + blockIdx.y;
  if (row >= r1) return;
  const bool mirror = (d[D_FLAGS] & kMirror) != 0;
  const unsigned char* s = source(d, ws) + (size_t)row * d[D_STRIDE];
  const int* bx = coeffs + d[D_TAB_X];
  const int xx = (int)d[D_OFF_X] + xw;
  const int xm = bx[2 * xx], n = bx[2 * xx + 1];
  const int* w = bx + 2 * (size_t)d[D_FULL_W] + (size_t)xx * d[D_KX];
  int s0 = 1 << (kPrec - 1), s1 = s0, s2 = s0;
  for (int k = 0; k < n; ++k) {
    const int c = mirror ? in_w - 1 - (xm + k) : xm + k;
    const unsigned char* q = s + (size_t)c * 3;
    s0 += w[k] * q[0];
    s1 += w[k] * q[1];
    s2 += w[k] * q[2];
  }
  unsigned char* o = ws + d[D_PRE] + ((size_t)(row - r0) * out_w + xw) * 3;
  o[0] = (unsigned char)clip8(s0);
  o[1] = (unsigned char)clip8(s1);
  o[2] = (unsigned char)clip8(s2);
}

int launch_hpass(hipStream_t st, const long long* dsc, int batch, const int32_t* coeffs, int rows, int cols,
                 uint8_t* workspace) {
  hipLaunchKernelGGL(augment_hpass, dim3((cols + 255) / 256, rows, batch), dim3(256), 0, st, dsc, coeffs, workspace);
  return egtr_check_launch();
}

template <typename T>
int launch_augment(egtr_stream_t stream, const int64_t* first, const int64_t* final_, int batch, const int32_t* coeffs,
                   const float* lut, int H, int W, int first_rows, int first_cols, int pre1_rows, int pre1_cols,
                   int pre2_rows, int pre2_cols, uint8_t* workspace, T* pixel_values, int64_t* pixel_mask) {
  if (!final_ || !coeffs || !lut || !pixel_values || !pixel_mask || batch <= 0 || H <= 0 || W <= 0) return EGTR_E_ARG;
  if (first_rows < 0 || first_cols < 0 || pre1_rows < 0 || pre1_cols < 0 || pre2_rows < 0 || pre2_cols < 0)
    return EGTR_E_ARG;
  if ((first_rows > 0) != (first_cols > 0) || (pre1_rows > 0) != (pre1_cols > 0) || (pre2_rows > 0) != (pre2_cols > 0) ||
      (pre1_rows > 0 && first_rows == 0))
    return EGTR_E_ARG;
  if ((first_rows > 0 && !first) || ((first_rows > 0 || pre2_rows > 0) && !workspace)) return EGTR_E_ARG;
  if (batch > 65535 || (H + kTH - 1) / kTH > 65535 || (first_rows + kTH - 1) / kTH > 65535 || pre1_rows > 65535 ||
      pre2_rows > 65535)
    return EGTR_E_UNSUPPORTED;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const long long* d1 = reinterpret_cast<const long long*>(first);
  const long long* d2 = reinterpret_cast<const long long*>(final_);
  int rc;
  if (pre1_rows > 0 && (rc = launch_hpass(st, d1, batch, coeffs, pre1_rows, pre1_cols, workspace)) != EGTR_OK) return rc;
  if (first_rows > 0) {
    hipLaunchKernelGGL(augment_tile<unsigned char>, dim3((first_cols + kTW - 1) / kTW, (first_rows + kTH - 1) / kTH, batch),
                       dim3(kThreads), 0, st, d1, coeffs, lut, first_rows, first_cols, workspace,
                       static_cast<unsigned char*>(nullptr), static_cast<long long*>(nullptr));
    if ((rc = egtr_check_launch()) != EGTR_OK) return rc;
  }
  if (pre2_rows > 0 && (rc = launch_hpass(st, d2, batch, coeffs, pre2_rows, pre2_cols, workspace)) != EGTR_OK) return rc;
  hipLaunchKernelGGL(augment_tile<T>, dim3((W + kTW - 1) / kTW, (H + kTH - 1) / kTH, batch), dim3(kThreads), 0, st, d2,
                     coeffs, lut, H, W, workspace, pixel_values, reinterpret_cast<long long*>(pixel_mask));
  return egtr_check_launch();
}
}  // namespace

extern "C" int egtr_preprocess_augment_f32(egtr_stream_t stream, const int64_t* first_desc, const int64_t* final_desc,
                                           int batch, const int32_t* coeffs, const float* lut, int H, int W,
                                           int first_rows, int first_cols, int pre1_rows, int pre1_cols,
                                           int pre2_rows, int pre2_cols, uint8_t* workspace, float* pixel_values,
                                           int64_t* pixel_mask) {
  return launch_augment(stream, first_desc, final_desc, batch, coeffs, lut, H, W, first_rows, first_cols, pre1_rows,
                        pre1_cols, pre2_rows, pre2_cols, workspace, pixel_values, pixel_mask);
}

extern "C" int egtr_preprocess_augment_bf16(egtr_stream_t stream, const int64_t* first_desc, const int64_t* final_desc,
                                            int batch, const int32_t* coeffs, const float* lut, int H, int W,
                                            int first_rows, int first_cols, int pre1_rows, int pre1_cols,
                                            int pre2_rows, int pre2_cols, uint8_t* workspace, uint16_t* pixel_values,
                                            int64_t* pixel_mask) {
  return launch_augment(stream, first_desc, final_desc, batch, coeffs, lut, H, W, first_rows, first_cols, pre1_rows,
                        pre1_cols, pre2_rows, pre2_cols, workspace, reinterpret_cast<unsigned short*>(pixel_values),
                        pixel_mask);
}
