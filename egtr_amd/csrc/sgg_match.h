// What the relation evaluators share (sgg_eval.hip: Visual Genome sgdet recall and the zero-shot pass, vrd_eval.hip: phrase /
// predicate detection, oi_eval.hip: Open Images, rel_stats.hip): the limits, an image's ranges in the ragged relation
// layout, the candidate label check, the first-rank matching of _compute_pred_matches (lib/evaluation/sg_eval.py:281-328)
// for one GT triplet by one wave, the integer LDS tallies with their slab row, the recall-matching kernel that sgdet and
// phrdet instantiate with their box test, the arguments every launcher fills the same way, and the image-ordered fold.
//
// Slab / accumulator layout of the Visual Genome protocols (W = egtr_sgg_eval_width(R, nk) doubles per row):
//   [0, nk)                  recall at ks[j]            (0 for a skipped image)
//   nk                       1 = image counted
//   nk + 1                   1 = image skipped (no GT relation; the reference asserts there, sg_eval.py:199)
//   nk + 2 + p*nk + j        recall of predicate p at ks[j]  (0 where the image has no GT triplet of p)
//   nk + 2 + R*nk + p        1 = image has >= 1 GT triplet of p (counts for predicate p; train_egtr.py:113)
#pragma once

#include <hip/hip_runtime.h>

#include <stdint.h>

#include "bbox_f64.h"
#include "common.h"

namespace egtr_eval {   // every evaluator translation unit sees these definitions; keep them out of the global namespace

constexpr int kEvalMaxCand = 1024;   // candidates per image whose labels and boxes fit in LDS
constexpr int kEvalMaxRel = 256;
constexpr int kEvalMaxK = 8;
constexpr int kEvalThreads = 256;    // workgroup of the matching kernels: 4 waves, a wave per GT triplet

// ---- host: the arguments every launcher fills the same way ----------------------------------------------------------------
struct EvalCommon {
  const int64_t* gt_rels;       // [T, 3]
  const int64_t* rel_off;       // [B + 1]
  const float* gt_boxes;        // [G, 4] xyxy
  const int64_t* gt_classes;    // [G]
  const int64_t* box_off;       // [B + 1]
  long long T, G;
  int K, N, R, nk, W;           // candidates, predicted objects, predicates, len(ks), slab row width
  int ks[kEvalMaxK];
};

// ks must be 1..kEvalMaxK strictly increasing positive values
inline bool egtr_bad_ks(const int* ks, int num_k) {
  if (!ks || num_k < 1 || num_k > kEvalMaxK) return true;
  for (int j = 0; j < num_k; ++j)
    if (ks[j] < 1 || (j > 0 && ks[j] <= ks[j - 1])) return true;
  return false;
}

// `ks` has passed egtr_bad_ks.  A launcher without boxes, classes or predicted objects passes NULL / 0 there.
inline void egtr_fill_common(EvalCommon* c, const int64_t* gt_rels, const int64_t* rel_off, long long T,
                             const float* gt_boxes, const int64_t* gt_classes, const int64_t* box_off, long long G, int K,
                             int N, int R, int W, const int* ks, int num_k) {
  c->gt_rels = gt_rels;
  c->rel_off = rel_off;
  c->gt_boxes = gt_boxes;
  c->gt_classes = gt_classes;
  c->box_off = box_off;
  c->T = T;
  c->G = G;
  c->K = K;
  c->N = N;
  c->R = R;
  c->nk = num_k;
  c->W = W;
  for (int j = 0; j < kEvalMaxK; ++j) c->ks[j] = j < num_k ? ks[j] : 0;
}

// acc[j] += slab[0][j]; acc[j] += slab[1][j]; ...  -- IN IMAGE ORDER, one thread per column j < W, so the sums are the same
// left fold whatever the batch size (store-and-sum, no float atomics).  A second launch rather than a last-workgroup-done
// counter: the fold must wait for every image of the batch, and a few microseconds of launch buy no cross-workgroup
// fences.  Defined in sgg_eval.hip (kernel eval_fold); returns the launch status.
int egtr_fold_rows(hipStream_t stream, const double* slab, int B, int W, double* acc);

// ---- device: an image's ranges -------------------------------------------------------------------------------------------
__device__ __forceinline__ long long egtr_clamp_off(long long v, long long hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// GT relations [r0, r1) and GT objects [g0, g1) of image b.  Offsets outside [0, T] / [0, G] are clamped and a decreasing
// pair gives an empty range, so no kernel reads outside the arrays whatever the offsets hold.
struct ImageRange {
  long long r0, r1, g0, g1;

  __device__ __forceinline__ ImageRange(const int64_t* rel_off, const int64_t* box_off, long long T, long long G, int b) {
    r0 = egtr_clamp_off(rel_off[b], T);
    r1 = egtr_clamp_off(rel_off[b + 1], T);
    if (r1 < r0) r1 = r0;
    g0 = egtr_clamp_off(box_off[b], G);
    g1 = egtr_clamp_off(box_off[b + 1], G);
    if (g1 < g0) g1 = g0;
  }
  __device__ __forceinline__ long long n_rel() const { return r1 - r0; }
  __device__ __forceinline__ long long n_box() const { return g1 - g0; }
};

// ---- device: candidates --------------------------------------------------------------------------------------------------
// The LDS label (class_s, class_o, predicate, valid) of candidate (s, o, p) of image b, and its two boxes.  A candidate
// with s or o outside [0, N), p outside [0, P) or a class that is no int is invalid: label 0, boxes NULL; it matches no
// GT triplet.
__device__ __forceinline__ int4 egtr_candidate_label(const float* pred_boxes, const int64_t* pred_classes, int b, int N,
                                                     int P, long long s, long long o, long long p, const float** sbox,
                                                     const float** obox) {
  *sbox = *obox = nullptr;
  if (s < 0 || s >= N || o < 0 || o >= N || p < 0 || p >= P) return make_int4(0, 0, 0, 0);
  const long long cs = pred_classes[(long long)b * N + s], co = pred_classes[(long long)b * N + o];
  if (cs != (int)cs || co != (int)co) return make_int4(0, 0, 0, 0);
  *sbox = pred_boxes + ((long long)b * N + s) * 4;
  *obox = pred_boxes + ((long long)b * N + o) * 4;
  return make_int4((int)cs, (int)co, (int)p, 1);
}

__device__ __forceinline__ float4 egtr_load_box(const float* p) { return make_float4(p[0], p[1], p[2], p[3]); }

// Lowest candidate index c < K whose labels s_lab[c] equal (gcs, gco, gp) and whose boxes pass `box_test(c)`; K if none.
// Called by all 64 lanes of a wave with the same GT; lanes test candidates base .. base+63 in rank order and the ballot's
// lowest set bit is the wave's min, so the first chunk with a match ends the search (the trip count is wave-uniform: every
// lane reaches every ballot).  Labels are compared first (intersect_2d); the box test, an fp64 IoU, runs only on a label
// match.
template <class BoxTest>
__device__ __forceinline__ int egtr_first_rank_wave(const int4* s_lab, int K, long long gcs, long long gco, long long gp,
                                                    int lane, BoxTest box_test) {
  for (int base = 0; base < K; base += 64) {
    const int c = base + lane;
    bool m = false;
    if (c < K) {
      const int4 lab = s_lab[c];
      m = lab.w && lab.x == gcs && lab.y == gco && lab.z == gp && box_test(c);
    }
    const unsigned long long bal = __ballot(m);
    if (bal) return base + __ffsll(bal) - 1;
  }
  return K;
}

// bbox.pyx IoU of a GT box and a candidate box >= thr (float32 boxes widened to double at the test, which is exact)
__device__ __forceinline__ bool egtr_iou_ge(float4 g, float4 q, double thr) {
  return egtr_bbox_overlap_pyx(g.x, g.y, g.z, g.w, q.x, q.y, q.z, q.w, 0) >= thr;
}

// The box layout and box test of the sgdet protocol (Open Images matches the same way): subject and object box apart,
// both IoUs >= thr.
struct SubjectObjectBoxes {
  float4 sbox[kEvalMaxCand], obox[kEvalMaxCand];
  struct Gt {
    float4 s, o;
  };

  // bs and bo are both NULL for an invalid candidate (zero boxes).  One branch, so the two loads issue back to back.
  __device__ __forceinline__ void stage(int c, const float* bs, const float* bo) {
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f), o = s;
    if (bs) {
      s = egtr_load_box(bs);
      o = egtr_load_box(bo);
    }
    sbox[c] = s;
    obox[c] = o;
  }
  static __device__ __forceinline__ Gt gt(const float* bs, const float* bo) { return {egtr_load_box(bs), egtr_load_box(bo)}; }
  __device__ __forceinline__ bool test(int c, const Gt& g, double thr) const {
    const float4 q = sbox[c], u = obox[c];   // both LDS reads before the first IoU, not one behind it
    return egtr_iou_ge(g.s, q, thr) && egtr_iou_ge(g.o, u, thr);
  }
};

// ---- device: the integer LDS tallies of the Visual Genome protocols and their slab row ------------------------------------
// Integer atomics, so the tallies do not depend on the order of the waves.
struct RecallTallies {
  int cnt[kEvalMaxRel];                  // GT triplets of predicate p
  int hits_p[kEvalMaxRel * kEvalMaxK];   // ... of them recalled at ks[j]: [p * nk + j]
  int hits[kEvalMaxK];                   // GT triplets recalled at ks[j]

  // all threads; a barrier must follow before the first update
  __device__ __forceinline__ void zero(int R, int nk, int tid) {
    for (int i = tid; i < R * nk; i += kEvalThreads) hits_p[i] = 0;
    for (int i = tid; i < R; i += kEvalThreads) cnt[i] = 0;
    if (tid < kEvalMaxK) hits[tid] = 0;
  }
  // One lane per GT triplet.  A triplet counts for its predicate whenever the predicate is in range, even when its subject
  // or object index is not: such a triplet is never recalled and lowers the predicate's recall, like in the reference.
  __device__ __forceinline__ void count(long long gp, int R) {
    if (gp >= 0 && gp < R) atomicAdd(&cnt[gp], 1);
  }
  // One lane per GT triplet with first rank fr among K candidates.  `fr < K` on top of `fr < ks[j]`: K means "no match" and
  // ks[j] may exceed K.  The per-predicate tally needs gok (gp in range) because gp indexes it.
  __device__ __forceinline__ void hit(int fr, int K, const int* ks, int nk, bool gok, long long gp) {
    for (int j = 0; j < nk; ++j) {
      if (fr < ks[j] && fr < K) {
        atomicAdd(&hits[j], 1);
        if (gok) atomicAdd(&hits_p[gp * nk + j], 1);
      }
    }
  }
  // All threads, after a barrier: the image's slab row (layout at the top).  double(hits) / double(count) is the
  // reference's float(len) / float(n).  `poison`: NaN instead of every recall that has a denominator -- the flag columns
  // stay right.
  __device__ __forceinline__ void write_row(double* out, int W, int R, int nk, long long n_rel, bool poison,
                                            int tid) const {
    const bool skip = n_rel == 0;
    const int pbase = nk + 2, fbase = nk + 2 + R * nk;
    const double bad = __longlong_as_double(0x7ff8000000000000ll);
    for (int j = tid; j < W; j += kEvalThreads) {
      double v = 0.0;
      if (j < nk) {
        v = skip ? 0.0 : (poison ? bad : (double)hits[j] / (double)n_rel);
      } else if (j == nk) {
        v = skip ? 0.0 : 1.0;
      } else if (j == nk + 1) {
        v = skip ? 1.0 : 0.0;
      } else if (j < fbase) {
        const int q = j - pbase, c = cnt[q / nk];
        v = c ? (poison ? bad : (double)hits_p[q] / (double)c) : 0.0;
      } else {
        v = cnt[j - fbase] ? 1.0 : 0.0;
      }
      out[j] = v;
    }
  }
};

// ---- the recall-matching kernel of sgdet and phrdet -----------------------------------------------------------------------
struct RecallArgs : EvalCommon {
  const int64_t* cand;          // [B, K, cols] (s, o[, p])
  const float* rel_scores;      // [B, K, R] (cols == 2)
  const float* pred_boxes;      // [B, N, 4] xyxy
  const int64_t* pred_classes;  // [B, N]
  int* first_rank;              // [T] or NULL
  double* slab;                 // [B, W]
  double thr;
  int cols;
};

// One workgroup per image (4 waves).  The image's candidates go to LDS as labels + the boxes of `Boxes` (a layout, how a
// candidate's and a GT triplet's boxes are taken from the subject and object box, and the test between the two:
// SubjectObjectBoxes above for sgdet, the union box of vrd_eval.hip for phrdet).  A WAVE owns a GT triplet
// (egtr_first_rank_wave), its lane 0 bumps the tallies, and the workgroup writes the image's slab row.
//
// What differs from the other matching kernels ON PURPOSE (each is the reference's behaviour, pinned by a test):
//   * here gok requires the GT predicate in range; oi_match's does not look at it (its label compare fails anyway and it
//     has no per-predicate hit table to index);
//   * a GT triplet whose subject / object index is out of range still counts for its predicate (RecallTallies::count);
//   * hits need fr < ks[j] AND fr < K; preddet_match compares against kNoRank instead, its list is not K long;
//   * thr is an argument here, the literal 0.5 in oi_match, whose K is det_count[b] clamped, not a launch constant.
template <class Boxes>
__global__ __launch_bounds__(kEvalThreads) void recall_match(const RecallArgs a) {
  __shared__ int4 s_lab[kEvalMaxCand];   // class_s, class_o, predicate, valid
  __shared__ Boxes s_box;
  __shared__ RecallTallies s_t;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int K = a.K, R = a.R;

  s_t.zero(R, a.nk, tid);
  for (int c = tid; c < K; c += kEvalThreads) {
    const int64_t* row = a.cand + ((long long)b * K + c) * a.cols;
    const long long s = row[0], o = row[1];   // issued before the predicate's loads, which they do not depend on
    long long p;
    if (a.cols == 3) {
      p = row[2];
    } else {
      // numpy argmax of the row (sg_eval.py:131-135): the lowest index among the maxima, or the first NaN if any
      const float* sc = a.rel_scores + ((long long)b * K + c) * R;
      float best = sc[0];
      int bi = 0;
      if (!isnan(best)) {
        for (int r = 1; r < R; ++r) {
          const float v = sc[r];
          if (isnan(v)) { bi = r; break; }
          if (v > best) { best = v; bi = r; }
        }
      }
      p = bi;
    }
    const float *bs, *bo;
    s_lab[c] = egtr_candidate_label(a.pred_boxes, a.pred_classes, b, a.N, R, s, o, p, &bs, &bo);
    s_box.stage(c, bs, bo);
  }
  __syncthreads();

  const ImageRange im(a.rel_off, a.box_off, a.T, a.G, b);
  for (long long t = im.r0 + wave; t < im.r1; t += kEvalThreads / 64) {
    const long long gs = a.gt_rels[t * 3 + 0], go = a.gt_rels[t * 3 + 1], gp = a.gt_rels[t * 3 + 2];
    const bool gok = gs >= 0 && gs < im.n_box() && go >= 0 && go < im.n_box() && gp >= 0 && gp < R;
    int fr = K;
    if (gok) {
      const typename Boxes::Gt g = Boxes::gt(a.gt_boxes + (im.g0 + gs) * 4, a.gt_boxes + (im.g0 + go) * 4);
      fr = egtr_first_rank_wave(s_lab, K, a.gt_classes[im.g0 + gs], a.gt_classes[im.g0 + go], gp, lane,
                                [&](int c) { return s_box.test(c, g, a.thr); });
    }
    if (lane == 0) {
      if (a.first_rank) a.first_rank[t] = fr;
      s_t.count(gp, R);
      s_t.hit(fr, K, a.ks, a.nk, gok, gp);
    }
  }
  __syncthreads();
  s_t.write_row(a.slab + (long long)b * a.W, a.W, R, a.nk, im.n_rel(), false, tid);
}

// Launch recall_match<Boxes> over `batch` images and, with acc, fold the slab rows into it.
template <class Boxes>
int egtr_launch_recall_match(hipStream_t s, const RecallArgs& a, int batch, double* acc) {
  hipLaunchKernelGGL(recall_match<Boxes>, dim3((unsigned)batch), dim3(kEvalThreads), 0, s, a);
  const int st = egtr_check_launch();
  if (st != EGTR_OK || !acc) return st;
  return egtr_fold_rows(s, a.slab, batch, a.W, acc);
}

}  // namespace egtr_eval
