// The reference's bbox.pyx overlap arithmetic (lib/fpn/box_intersections_cpu/bbox.pyx: bbox_overlaps :21-61, bbox_intersections
// :64-108) for ONE (box, query) pair, shared by postprocess.hip (egtr_bbox_overlaps_f64) and sgg_eval.hip (the evaluator's
// sub / obj IoU test).  float64, "+1 pixel" convention, zero where the boxes do not overlap; the same operation order as the
// Cython loops and no FMA contraction (the products are rounded before they are added), so results are bit-identical.
#pragma once

#include <hip/hip_runtime.h>

// b = boxes[n] (x0, y0, x1, y1), q = query_boxes[k]; mode 0 = bbox_overlaps (IoU), 1 = bbox_intersections (inter / query area)
__device__ __forceinline__ double egtr_bbox_overlap_pyx(double bx0, double by0, double bx1, double by1, double qx0,
                                                        double qy0, double qx1, double qy1, int mode) {
#pragma clang fp contract(off)
  const double box_area = (qx1 - qx0 + 1) * (qy1 - qy0 + 1);                 // bbox.pyx:44-47
  double r = 0.0;
  const double iw = fmin(bx1, qx1) - fmax(bx0, qx0) + 1;                     // :49-52
  if (iw > 0) {
    const double ih = fmin(by1, qy1) - fmax(by0, qy0) + 1;                   // :54-57
    if (ih > 0) {
      if (mode == 0) {
        const double ua = (bx1 - bx0 + 1) * (by1 - by0 + 1) + box_area - iw * ih;   // :59-63
        r = iw * ih / ua;                                                    // :64
      } else {
        r = iw * ih / box_area;                                              // :107 (bbox_intersections)
      }
    }
  }
  return r;
}
