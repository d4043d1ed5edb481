// Device code shared by the scene-graph evaluators (sgg_eval.hip: Visual Genome Recall@K, oi_eval.hip: Open Images
// relation metrics): the first-rank matching of _compute_pred_matches (lib/evaluation/sg_eval.py:281-328) for one GT
// triplet by one wave, and the image-ordered fold of per-image slab rows into fp64 accumulators.
#pragma once

#include <hip/hip_runtime.h>

#include "bbox_f64.h"

// Lowest candidate index c < K whose labels (s_lab[c] = class_s, class_o, predicate, valid) equal (gcs, gco, gp) and whose
// subject / object boxes both have bbox.pyx IoU >= thr with the GT's (the boxes are float32, widened to double at the
// test, which is exact); K if none.  Called by all 64 lanes of a wave with the same GT; lanes test candidates
// base .. base+63 in rank order and the ballot's lowest set bit is the wave's min, so the first chunk with a match ends
// the search.  Labels are compared first (intersect_2d), the fp64 IoU runs only on a label match.
__device__ __forceinline__ int egtr_first_rank_wave(const int4* s_lab, const float4* s_sbox, const float4* s_obox, int K,
                                                    long long gcs, long long gco, long long gp, double sx0, double sy0,
                                                    double sx1, double sy1, double ox0, double oy0, double ox1,
                                                    double oy1, double thr, int lane) {
  for (int base = 0; base < K; base += 64) {
    const int c = base + lane;
    bool m = false;
    if (c < K) {
      const int4 lab = s_lab[c];
      if (lab.w && lab.x == gcs && lab.y == gco && lab.z == gp) {
        const float4 q = s_sbox[c], u = s_obox[c];
        m = egtr_bbox_overlap_pyx(sx0, sy0, sx1, sy1, q.x, q.y, q.z, q.w, 0) >= thr &&
            egtr_bbox_overlap_pyx(ox0, oy0, ox1, oy1, u.x, u.y, u.z, u.w, 0) >= thr;
      }
    }
    const unsigned long long bal = __ballot(m);
    if (bal) return base + __ffsll(bal) - 1;
  }
  return K;
}

// acc[j] += slab[0][j]; acc[j] += slab[1][j]; ...  -- image order, so the sums are the same left fold whatever the batch
// size (store-and-sum, no float atomics).  The body of the fold kernels, one thread per column j < W.
__device__ __forceinline__ void egtr_fold_column(const double* __restrict__ slab, int B, int W, double* __restrict__ acc,
                                                 int j) {
  double s = acc[j];
  for (int b = 0; b < B; ++b) s += slab[(long long)b * W + j];
  acc[j] = s;
}
