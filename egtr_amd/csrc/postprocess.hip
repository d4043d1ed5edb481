// Post-processing routines on the device: the evaluator inputs of the reference.
//
// egtr_bbox_overlaps_f64: the reference's native CPU routine lib/fpn/box_intersections_cpu/bbox.pyx (bbox_overlaps,
// :21-61, and bbox_intersections, :64-108) -- float64, "+1 pixel" box convention, zero where the boxes do not overlap.
// One thread per (box n, query k) pair; the arithmetic is egtr_bbox_overlap_pyx (bbox_f64.h, shared with sgg_eval.hip): the
// same operation order as the Cython loops, so results are bit-identical (no FMA contraction).
#include <hip/hip_runtime.h>

#include "bbox_f64.h"
#include "common.h"

namespace {

#pragma clang fp contract(off)
__global__ __launch_bounds__(256) void bbox_overlaps_f64(const double* __restrict__ boxes,
                                                         const double* __restrict__ query, int N, int K, int mode,
                                                         double* __restrict__ out) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long long)N * K) return;
  const int n = (int)(idx / K), k = (int)(idx - (long long)n * K);
  const double bx0 = boxes[n * 4 + 0], by0 = boxes[n * 4 + 1], bx1 = boxes[n * 4 + 2], by1 = boxes[n * 4 + 3];
  const double qx0 = query[k * 4 + 0], qy0 = query[k * 4 + 1], qx1 = query[k * 4 + 2], qy1 = query[k * 4 + 3];
  out[idx] = egtr_bbox_overlap_pyx(bx0, by0, bx1, by1, qx0, qy0, qx1, qy1, mode);
}

}  // namespace

extern "C" int egtr_bbox_overlaps_f64(egtr_stream_t stream, const double* boxes, const double* query_boxes,
                                      int num_boxes, int num_query, int mode, double* out) {
  if (num_boxes < 0 || num_query < 0 || (mode != 0 && mode != 1)) return EGTR_E_ARG;
  if (num_boxes == 0 || num_query == 0) return EGTR_OK;  // empty result, nothing to launch
  if (!boxes || !query_boxes || !out) return EGTR_E_ARG;
  const long long n = (long long)num_boxes * num_query;
  if (n >= (1ll << 31)) return EGTR_E_UNSUPPORTED;
  hipLaunchKernelGGL(bbox_overlaps_f64, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), boxes, query_boxes, num_boxes, num_query, mode, out);
  return egtr_check_launch();
}
