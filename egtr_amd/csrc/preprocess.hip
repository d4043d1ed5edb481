// Reference-exact image preprocessing on the device: the transformers-4.18 DetrFeatureExtractor path the reference's
// datasets run per image (PIL BILINEAR resize of the uint8 RGB image, to_numpy_array's 1/255 rescale, ImageNet
// normalisation) followed by the collate's pad_and_create_pixel_mask -- for a whole batch of raw uint8 HWC images.
//
// Resampling is Pillow's ImagingResample for 8-bit images (bilinear, support 1): a horizontal pass, then a vertical one,
// each computing acc = 2^21 + sum_k w_k * u8 in int32 with 22-bit fixed-point weights and clipping acc >> 22 to uint8.
// The weights and per-output [xmin, n) bounds come from the host (feature_extraction.pil_bilinear_coeffs); an axis that
// keeps its size gets the one-tap identity table, which reproduces Pillow's skipped pass exactly.  The normalisation is a
// host-built [3][256] float32 table indexed by the resampled byte, so the kernel does no float arithmetic.
//
// preprocess_tile: one workgroup per (128 x 8 output tile, image) of the padded canvas.  It streams the input rows its
// tile needs through LDS in chunks (16-byte global loads of the row window, whatever its alignment), runs the horizontal
// pass of each chunk into a uint8 LDS buffer, and adds the chunk's vertical taps into int32 registers -- integer sums, so
// splitting them over chunks is exact.  Each lane finally owns 4 consecutive pixels of one row: LUT lookup, then 16-byte
// stores of the three NCHW planes and the int64 mask.  Tiles outside an image write zeros and mask 0.
// preprocess_hpass: the fallback for an image whose horizontal input window does not fit the LDS stage (downscales
// beyond ~40x): the horizontal pass into a uint8 workspace [in_h][out_w][3], after which preprocess_tile reads that
// image from the workspace with an identity horizontal pass.
#include "image_common.h"

namespace {
using namespace egtr_image;
constexpr int kDescWords = 12;

// descriptor fields (int64 each), see include/egtr_hip.h
enum { D_SRC, D_STRIDE, D_IN_H, D_IN_W, D_OUT_H, D_OUT_W, D_TAB_X, D_KX, D_TAB_Y, D_KY, D_ROUTE, D_WS };

template <typename T>
__global__ __launch_bounds__(kThreads) void preprocess_tile(const long long* __restrict__ desc,
                                                            const int* __restrict__ coeffs,
                                                            const float* __restrict__ lut, int H, int W,
                                                            const unsigned char* __restrict__ ws,
                                                            T* __restrict__ out, long long* __restrict__ mask) {
  __shared__ __attribute__((aligned(16))) unsigned char stage[kStage];
  __shared__ __attribute__((aligned(16))) unsigned char hbuf[kMaxRows * kHRow];
  __shared__ float slut[3 * 256];
  const int b = blockIdx.z, t = threadIdx.x;
  const int x0 = blockIdx.x * kTW, y0 = blockIdx.y * kTH;
  const int y = y0 + (t >> 5), x = x0 + (t & 31) * 4;
  const long long* d = desc + (size_t)b * kDescWords;
  const int out_h = (int)d[D_OUT_H], out_w = (int)d[D_OUT_W];
  float v[3][4] = {};
  int m[4] = {};
  if (x0 < out_w && y0 < out_h) {   // uniform over the workgroup
    for (int i = t; i < 3 * 256; i += kThreads) slut[i] = lut[i];
    const bool pre = d[D_ROUTE] != 0;
    const unsigned char* src = pre ? ws + d[D_WS] : reinterpret_cast<const unsigned char*>(d[D_SRC]);
    const long long stride = pre ? 3ll * out_w : d[D_STRIDE];
    const int xe = min(x0 + kTW, out_w), ye = min(y0 + kTH, out_h);
    const int* bx = coeffs + d[D_TAB_X];
    const int* wx = bx + 2 * (size_t)out_w;
    const int kx = (int)d[D_KX];
    const int* by = coeffs + d[D_TAB_Y];
    const int* wy = by + 2 * (size_t)out_h;
    const int ky = (int)d[D_KY];
    // input window of the tile: columns [c0, c1), rows [r0, r1) (bounds are non-decreasing in the output index)
    const int c0 = pre ? x0 : bx[2 * x0];
    const int c1 = pre ? xe : bx[2 * (xe - 1)] + bx[2 * (xe - 1) + 1];
    const int r0 = by[2 * y0], r1 = by[2 * (ye - 1)] + by[2 * (ye - 1) + 1];
    const int L = (c1 - c0) * 3;                          // bytes of one staged input row
    const bool fits = L <= EGTR_PREPROCESS_STAGE_BYTES;   // else the host should have routed it through the prepass
    const int pu = (min(L, EGTR_PREPROCESS_STAGE_BYTES) + 30) >> 4;   // 16-byte units per row, misalignment included
    const int chunk = min(kMaxRows, kStage / (pu * 16));
    const int ncols = xe - x0;
    int ymin = 0, yn = 0;
    const int* wyy = wy;
    if (y < ye) {
      ymin = by[2 * y];
      yn = by[2 * y + 1];
      wyy = wy + (size_t)y * ky;
    }
    int acc[3][4] = {};
    for (int rc = r0; fits && rc < r1; rc += chunk) {
      const int nr = min(chunk, r1 - rc);
      // (A) stage rows rc .. rc+nr-1: aligned 16-byte loads covering [p, p + L); every loaded granule holds a byte of
      // the row, so no load leaves the row's pages
      for (int i = t; i < nr * pu; i += kThreads) {
        const int r = i / pu, u = i - r * pu;
        const uintptr_t p = reinterpret_cast<uintptr_t>(src + (size_t)(rc + r) * stride + (size_t)c0 * 3);
        const uintptr_t a = (p & ~(uintptr_t)15) + (uintptr_t)u * 16;
        if (a < p + (uintptr_t)L)
          *reinterpret_cast<uint4*>(stage + (r * pu + u) * 16) = *reinterpret_cast<const uint4*>(a);
      }
      __syncthreads();
      // (B) horizontal pass of the staged rows into hbuf (uint8, like Pillow's intermediate image)
      for (int i = t; i < nr * kTW; i += kThreads) {
        const int r = i / kTW, j = i - r * kTW;
        if (j >= ncols) continue;
        const uintptr_t p = reinterpret_cast<uintptr_t>(src + (size_t)(rc + r) * stride + (size_t)c0 * 3);
        const unsigned char* row = stage + r * pu * 16 + (int)(p & 15);
        unsigned char* h = hbuf + r * kHRow + j * 3;
        if (pre) {
          h[0] = row[j * 3];
          h[1] = row[j * 3 + 1];
          h[2] = row[j * 3 + 2];
        } else {
          const int xx = x0 + j;
          const int xm = bx[2 * xx] - c0, n = bx[2 * xx + 1];
          const int* w = wx + (size_t)xx * kx;
          int s0 = 1 << (kPrec - 1), s1 = s0, s2 = s0;
          for (int k = 0; k < n; ++k) {
            const int wk = w[k];
            const unsigned char* q = row + (xm + k) * 3;
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
      if (y < ye) {
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
    if (y < ye) {
      for (int i = 0; i < 4; ++i) {
        if (x + i >= xe) continue;
        m[i] = 1;
        for (int c = 0; c < 3; ++c)
          v[c][i] = fits ? slut[c * 256 + clip8(acc[c][i] + (1 << (kPrec - 1)))] : __builtin_nanf("");
      }
    }
  }
  if (y < H) {
    const bool vec = (W & 3) == 0;
    for (int c = 0; c < 3; ++c) store4(out + (((size_t)b * 3 + c) * H + y) * W + x, v[c], W - x, vec);
    store4(mask + ((size_t)b * H + y) * W + x, m, W - x, vec);
  }
}

__global__ __launch_bounds__(256) void preprocess_hpass(const long long* __restrict__ desc,
                                                        const int* __restrict__ coeffs,
                                                        unsigned char* __restrict__ ws) {
  const long long* d = desc + (size_t)blockIdx.z * kDescWords;
  const int row = blockIdx.y, xx = blockIdx.x * 256 + threadIdx.x;
  const int in_h = (int)d[D_IN_H], out_w = (int)d[D_OUT_W];
  if (d[D_ROUTE] == 0 || row >= in_h || xx >= out_w) return;
  const unsigned char* s = reinterpret_cast<const unsigned char*>(d[D_SRC]) + (size_t)row * d[D_STRIDE];
  const int* bx = coeffs + d[D_TAB_X];
  const int xm = bx[2 * xx], n = bx[2 * xx + 1];
  const int* w = bx + 2 * (size_t)out_w + (size_t)xx * d[D_KX];
  int s0 = 1 << (kPrec - 1), s1 = s0, s2 = s0;
  for (int k = 0; k < n; ++k) {
    const unsigned char* q = s + (size_t)(xm + k) * 3;
    s0 += w[k] * q[0];
    s1 += w[k] * q[1];
    s2 += w[k] * q[2];
  }
  unsigned char* o = ws + d[D_WS] + ((size_t)row * out_w + xx) * 3;
  o[0] = (unsigned char)clip8(s0);
  o[1] = (unsigned char)clip8(s1);
  o[2] = (unsigned char)clip8(s2);
}

template <typename T>
int launch_preprocess(egtr_stream_t stream, const int64_t* desc, int batch, const int32_t* coeffs, const float* lut,
                      int H, int W, int prepass_rows, int prepass_cols, uint8_t* workspace, T* pixel_values,
                      int64_t* pixel_mask) {
  if (!desc || !coeffs || !lut || !pixel_values || !pixel_mask || batch <= 0 || H <= 0 || W <= 0 || prepass_rows < 0 ||
      prepass_cols < 0 || (prepass_rows > 0 && (prepass_cols <= 0 || !workspace)))
    return EGTR_E_ARG;
  if (batch > 65535 || (H + kTH - 1) / kTH > 65535 || prepass_rows > 65535) return EGTR_E_UNSUPPORTED;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const long long* dsc = reinterpret_cast<const long long*>(desc);
  if (prepass_rows > 0) {
    hipLaunchKernelGGL(preprocess_hpass, dim3((prepass_cols + 255) / 256, prepass_rows, batch), dim3(256), 0, st, dsc,
                       coeffs, workspace);
    const int rc = egtr_check_launch();
    if (rc != EGTR_OK) return rc;
  }
  hipLaunchKernelGGL(preprocess_tile<T>, dim3((W + kTW - 1) / kTW, (H + kTH - 1) / kTH, batch), dim3(kThreads), 0, st,
                     dsc, coeffs, lut, H, W, workspace, pixel_values, reinterpret_cast<long long*>(pixel_mask));
  return egtr_check_launch();
}
}  // namespace

extern "C" int egtr_preprocess_f32(egtr_stream_t stream, const int64_t* desc, int batch, const int32_t* coeffs,
                                   const float* lut, int H, int W, int prepass_rows, int prepass_cols,
                                   uint8_t* workspace, float* pixel_values, int64_t* pixel_mask) {
  return launch_preprocess(stream, desc, batch, coeffs, lut, H, W, prepass_rows, prepass_cols, workspace, pixel_values,
                           pixel_mask);
}

extern "C" int egtr_preprocess_bf16(egtr_stream_t stream, const int64_t* desc, int batch, const int32_t* coeffs,
                                    const float* lut, int H, int W, int prepass_rows, int prepass_cols,
                                    uint8_t* workspace, uint16_t* pixel_values, int64_t* pixel_mask) {
  return launch_preprocess(stream, desc, batch, coeffs, lut, H, W, prepass_rows, prepass_cols, workspace,
                           reinterpret_cast<unsigned short*>(pixel_values), pixel_mask);
}
