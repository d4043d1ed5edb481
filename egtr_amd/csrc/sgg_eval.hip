// Scene-graph Recall@K / mean Recall@K on the device: the matching and tallying of the reference's sgdet evaluator
// (lib/evaluation/sg_eval.py: evaluate_from_dict :74-160, evaluate_recall :163-240, _compute_pred_matches :270-313) fed by
// evaluate_batch (train_egtr.py:43-139), and the per-predicate evaluators of the mR@K (train_egtr.py:108-117, 130-139).
//
// The reference's recall at k is len(reduce(np.union1d, pred_to_gt[:k])) / n_gt: the GT triplets matched by one of the
// first k candidates.  That is #{t : first_rank[t] < k} with first_rank[t] the smallest candidate index that matches GT
// triplet t (K = no match).  Filtering the GT list by predicate (the per-predicate evaluators) changes no triplet's match,
// so one matching pass per image gives R@k for every k and every predicate.
//
// The matching kernel is recall_match<SubjectObjectBoxes> of sgg_match.h (shared with phrase detection, which passes
// another box test); the slab rows and the fold (eval_fold below, egtr_fold_rows for every evaluator) are described there.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "common.h"
#include "sgg_match.h"

using namespace egtr_eval;

namespace {

constexpr int kMaxCand = kEvalMaxCand, kMaxRel = kEvalMaxRel, kMaxK = kEvalMaxK, kThreads = kEvalThreads;

__global__ __launch_bounds__(kThreads) void eval_fold(const double* __restrict__ slab, int B, int W,
                                                      double* __restrict__ acc) {
  const int j = blockIdx.x * kThreads + threadIdx.x;
  if (j >= W) return;
  double s = acc[j];
  for (int b = 0; b < B; ++b) s += slab[(long long)b * W + j];
  acc[j] = s;
}

// Zero-shot recall: the recall over the GT triplets whose (subject class, object class, predicate) never
// occurs in training -- bit ((cs * C1 + co) * R + p) of seen_bits is clear.  Filtering the GT list changes no triplet's
// match (the argument at the top of this file), so the first ranks recall_match left behind are all it needs.  One WAVE per
// image: lanes take the image's triplets 64 at a time and the ballots' population counts are the integer tallies.  Row of
// nk + 2 doubles: recall at ks[j] = double(hits) / double(count) (0 without a zero-shot triplet), 1 = the image has one,
// the number of them.  A triplet with an index, class or predicate out of range is not zero-shot.
struct ZeroShotArgs : EvalCommon {   // no boxes, no predicted objects
  const int* first_rank;            // [T]
  const unsigned long long* seen;   // [ceil(C1 * C1 * R / 64)]
  double* slab;                     // [B, W = nk + 2]
  int C1;
};

__global__ __launch_bounds__(64) void sgg_zero_shot(const ZeroShotArgs a) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const ImageRange im(a.rel_off, a.box_off, a.T, a.G, b);
  const long long r0 = im.r0, r1 = im.r1, g0 = im.g0, n_boxes = im.n_box();
  int hits[kMaxK];
  for (int j = 0; j < kMaxK; ++j) hits[j] = 0;
  int count = 0;
  for (long long base = r0; base < r1; base += 64) {   // wave-uniform trip count: every lane reaches every ballot
    const long long t = base + lane;
    bool zs = false;
    int fr = a.K;
    if (t < r1) {
      const long long s = a.gt_rels[t * 3], o = a.gt_rels[t * 3 + 1], p = a.gt_rels[t * 3 + 2];
      if (s >= 0 && s < n_boxes && o >= 0 && o < n_boxes && p >= 0 && p < a.R) {
        const long long cs = a.gt_classes[g0 + s], co = a.gt_classes[g0 + o];
        if (cs >= 0 && cs < a.C1 && co >= 0 && co < a.C1) {
          const long long bit = (cs * a.C1 + co) * a.R + p;
          zs = !((a.seen[bit >> 6] >> (bit & 63)) & 1ull);
          fr = a.first_rank[t];
        }
      }
    }
    count += __popcll(__ballot(zs));
    for (int j = 0; j < kMaxK; ++j)
      if (j < a.nk) hits[j] += __popcll(__ballot(zs && fr < a.ks[j] && fr < a.K));
  }
  double v = 0.0;   // lane j writes column j
  for (int j = 0; j < kMaxK; ++j)
    if (j == lane && j < a.nk) v = count ? (double)hits[j] / (double)count : 0.0;
  if (lane == a.nk) v = count ? 1.0 : 0.0;
  if (lane == a.nk + 1) v = (double)count;
  if (lane < a.nk + 2) a.slab[(long long)b * (a.nk + 2) + lane] = v;
}

}  // namespace

int egtr_eval::egtr_fold_rows(hipStream_t stream, const double* slab, int B, int W, double* acc) {
  hipLaunchKernelGGL(eval_fold, dim3((unsigned)((W + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream, slab, B, W,
                     acc);
  return egtr_check_launch();
}

extern "C" int egtr_sgg_zero_shot_f64(egtr_stream_t stream, const int* first_rank, const int64_t* gt_rels,
                                      const int64_t* rel_offsets, long long num_gt_rels, const int64_t* gt_classes,
                                      const int64_t* box_offsets, long long num_gt_boxes, int batch, int num_cand,
                                      int num_classes, int num_rel, const int64_t* seen_bits, const int* ks, int num_k,
                                      double* slab, double* acc) {
  if (batch < 0 || num_cand < 0 || num_cand > kMaxCand || num_classes < 1 || num_rel < 1 || num_rel > kMaxRel ||
      num_k < 1 || num_k > kMaxK || num_gt_rels < 0 || num_gt_boxes < 0 || !ks)
    return EGTR_E_ARG;
  if ((long long)num_classes * num_classes * num_rel >= (1ll << 31)) return EGTR_E_UNSUPPORTED;
  if (egtr_bad_ks(ks, num_k)) return EGTR_E_ARG;
  if (batch == 0) return EGTR_OK;
  if (!rel_offsets || !box_offsets || !seen_bits || !slab) return EGTR_E_ARG;
  if (num_gt_rels > 0 && (!gt_rels || !first_rank)) return EGTR_E_ARG;
  if (num_gt_boxes > 0 && !gt_classes) return EGTR_E_ARG;

  ZeroShotArgs a;
  egtr_fill_common(&a, gt_rels, rel_offsets, num_gt_rels, nullptr, gt_classes, box_offsets, num_gt_boxes, num_cand, 0,
                   num_rel, num_k + 2, ks, num_k);
  a.first_rank = first_rank;
  a.seen = reinterpret_cast<const unsigned long long*>(seen_bits);
  a.slab = slab;
  a.C1 = num_classes;

  const hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(sgg_zero_shot, dim3((unsigned)batch), dim3(64), 0, s, a);
  const int st = egtr_check_launch();
  if (st != EGTR_OK || !acc) return st;
  return egtr_fold_rows(s, slab, batch, a.W, acc);   // the rows fold like the recall slab
}

extern "C" long long egtr_sgg_eval_width(int num_rel, int num_k) {
  if (num_rel < 1 || num_rel > kMaxRel || num_k < 1 || num_k > kMaxK) return EGTR_E_ARG;
  return (long long)num_k + 2 + (long long)num_rel * (num_k + 1);
}

extern "C" int egtr_sgg_eval_f32(egtr_stream_t stream, const int64_t* cand, int cand_cols, const float* rel_scores,
                                 const float* pred_boxes, const int64_t* pred_classes, int batch, int num_cand,
                                 int num_obj, int num_rel, const int64_t* gt_rels, const int64_t* rel_offsets,
                                 long long num_gt_rels, const float* gt_boxes, const int64_t* gt_classes,
                                 const int64_t* box_offsets, long long num_gt_boxes, const int* ks, int num_k,
                                 double iou_thresh, int* first_rank, double* slab, double* acc) {
  if (batch < 0 || (cand_cols != 2 && cand_cols != 3) || num_cand < 0 || num_cand > kMaxCand || num_obj < 0 ||
      num_rel < 1 || num_rel > kMaxRel || num_gt_rels < 0 || num_gt_boxes < 0 || iou_thresh != iou_thresh ||
      egtr_bad_ks(ks, num_k))
    return EGTR_E_ARG;
  if (num_cand > 0 && (num_obj < 1 || !cand || !pred_boxes || !pred_classes || (cand_cols == 2 && !rel_scores)))
    return EGTR_E_ARG;
  if ((num_gt_rels > 0 && !gt_rels) || (num_gt_boxes > 0 && (!gt_boxes || !gt_classes))) return EGTR_E_ARG;
  if (batch == 0) return EGTR_OK;
  if (!rel_offsets || !box_offsets || !slab) return EGTR_E_ARG;
  if ((long long)batch * num_cand * (cand_cols > 2 ? cand_cols : num_rel) >= (1ll << 40)) return EGTR_E_UNSUPPORTED;

  RecallArgs a;
  egtr_fill_common(&a, gt_rels, rel_offsets, num_gt_rels, gt_boxes, gt_classes, box_offsets, num_gt_boxes, num_cand,
                   num_obj, num_rel, (int)egtr_sgg_eval_width(num_rel, num_k), ks, num_k);
  a.cand = cand;
  a.rel_scores = rel_scores;
  a.pred_boxes = pred_boxes;
  a.pred_classes = pred_classes;
  a.first_rank = first_rank;
  a.slab = slab;
  a.thr = iou_thresh;
  a.cols = cand_cols;
  return egtr_launch_recall_match<SubjectObjectBoxes>(static_cast<hipStream_t>(stream), a, batch, acc);
}
