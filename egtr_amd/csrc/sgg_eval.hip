// Scene-graph Recall@K / mean Recall@K on the device: the matching and tallying of the reference's sgdet evaluator
// (lib/evaluation/sg_eval.py: evaluate_from_dict :74-160, evaluate_recall :163-240, _compute_pred_matches :270-313) fed by
// evaluate_batch (train_egtr.py:43-139), and the per-predicate evaluators of the mR@K (train_egtr.py:108-117, 130-139).
//
// The reference's recall at k is len(reduce(np.union1d, pred_to_gt[:k])) / n_gt: the GT triplets matched by one of the
// first k candidates.  That is #{t : first_rank[t] < k} with first_rank[t] the smallest candidate index that matches GT
// triplet t (K = no match).  Filtering the GT list by predicate (the per-predicate evaluators) changes no triplet's match,
// so one matching pass per image gives R@k for every k and every predicate.
//
// sgg_match: one workgroup per image (4 waves).  The image's candidates go to LDS as (class_s, class_o, predicate) + both
// float32 boxes (widened to double at the test, which is exact).  A WAVE owns a GT triplet: its lanes test candidates
// base .. base+63 in rank order (labels first, the fp64 IoU of bbox_f64.h only on a label match), and the ballot's lowest
// set bit is the wave's min; the first chunk with a match ends the triplet, so no cross-wave reduction is needed.  The
// wave's lane 0 then bumps integer LDS tallies (hits[k], count[p], hits_p[p][k]: integer atomics, order-free) and the
// workgroup writes the image's recalls -- double(hits) / double(count), the reference's float(len) / float(n) -- as one
// row of a slab.
// sgg_fold: a second launch adds the slab rows into the fp64 accumulators IN IMAGE ORDER, one thread per column, so the
// sums are the same left fold whatever the batch size (store-and-sum, no float atomics).  A second launch rather than a
// last-workgroup-done counter: the fold must wait for every image of the batch, and a few microseconds of launch buy no
// cross-workgroup fences.
//
// Slab / accumulator layout (W = egtr_sgg_eval_width(R, nk) doubles per row):
//   [0, nk)                  recall at ks[j]            (0 for a skipped image)
//   nk                       1 = image counted
//   nk + 1                   1 = image skipped (no GT relation; the reference asserts there, sg_eval.py:199)
//   nk + 2 + p*nk + j        recall of predicate p at ks[j]  (0 where the image has no GT triplet of p)
//   nk + 2 + R*nk + p        1 = image has >= 1 GT triplet of p (counts for predicate p; train_egtr.py:113)
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "common.h"
#include "sgg_match.h"

namespace {

constexpr int kMaxCand = 1024;
constexpr int kMaxRel = 256;
constexpr int kMaxK = 8;
constexpr int kThreads = 256;

struct SggArgs {
  const int64_t* cand;          // [B, K, cols] (s, o[, p])
  const float* rel_scores;      // [B, K, R] (cols == 2)
  const float* pred_boxes;      // [B, N, 4] xyxy
  const int64_t* pred_classes;  // [B, N]
  const int64_t* gt_rels;       // [T, 3]
  const int64_t* rel_off;       // [B + 1]
  const float* gt_boxes;        // [G, 4] xyxy
  const int64_t* gt_classes;    // [G]
  const int64_t* box_off;       // [B + 1]
  int* first_rank;              // [T] or NULL
  double* slab;                 // [B, W]
  long long T, G;
  double thr;
  int cols, K, N, R, nk, W;
  int ks[kMaxK];
};

__device__ __forceinline__ long long clamp_off(long long v, long long hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

__global__ __launch_bounds__(kThreads) void sgg_match(const SggArgs a) {
  __shared__ int4 s_lab[kMaxCand];        // class_s, class_o, predicate, valid
  __shared__ float4 s_sbox[kMaxCand];
  __shared__ float4 s_obox[kMaxCand];
  __shared__ int s_cnt[kMaxRel];
  __shared__ int s_hits_p[kMaxRel * kMaxK];
  __shared__ int s_hits[kMaxK];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int K = a.K, N = a.N, R = a.R, nk = a.nk;

  for (int i = tid; i < R * nk; i += kThreads) s_hits_p[i] = 0;
  for (int i = tid; i < R; i += kThreads) s_cnt[i] = 0;
  if (tid < kMaxK) s_hits[tid] = 0;

  for (int c = tid; c < K; c += kThreads) {
    const int64_t* row = a.cand + ((long long)b * K + c) * a.cols;
    const long long s = row[0], o = row[1];
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
    int4 lab = make_int4(0, 0, 0, 0);
    float4 sb = make_float4(0.f, 0.f, 0.f, 0.f), ob = sb;
    if (s >= 0 && s < N && o >= 0 && o < N && p >= 0 && p < R) {
      const long long cs = a.pred_classes[(long long)b * N + s], co = a.pred_classes[(long long)b * N + o];
      if (cs == (int)cs && co == (int)co) {
        lab = make_int4((int)cs, (int)co, (int)p, 1);
        const float* bs = a.pred_boxes + ((long long)b * N + s) * 4;
        const float* bo = a.pred_boxes + ((long long)b * N + o) * 4;
        sb = make_float4(bs[0], bs[1], bs[2], bs[3]);
        ob = make_float4(bo[0], bo[1], bo[2], bo[3]);
      }
    }
    s_lab[c] = lab;
    s_sbox[c] = sb;
    s_obox[c] = ob;
  }
  __syncthreads();

  const long long r0 = clamp_off(a.rel_off[b], a.T);
  long long r1 = clamp_off(a.rel_off[b + 1], a.T);
  if (r1 < r0) r1 = r0;
  const long long g0 = clamp_off(a.box_off[b], a.G);
  long long g1 = clamp_off(a.box_off[b + 1], a.G);
  if (g1 < g0) g1 = g0;
  const long long n_gt_boxes = g1 - g0;

  for (long long t = r0 + wave; t < r1; t += kThreads / 64) {
    const long long gs = a.gt_rels[t * 3 + 0], go = a.gt_rels[t * 3 + 1], gp = a.gt_rels[t * 3 + 2];
    const bool gok = gs >= 0 && gs < n_gt_boxes && go >= 0 && go < n_gt_boxes && gp >= 0 && gp < R;
    int fr = K;
    if (gok) {
      const long long gcs = a.gt_classes[g0 + gs], gco = a.gt_classes[g0 + go];
      const float* gsb = a.gt_boxes + (g0 + gs) * 4;
      const float* gob = a.gt_boxes + (g0 + go) * 4;
      fr = egtr_first_rank_wave(s_lab, s_sbox, s_obox, K, gcs, gco, gp, gsb[0], gsb[1], gsb[2], gsb[3], gob[0], gob[1],
                                gob[2], gob[3], a.thr, lane);
    }
    if (lane == 0) {
      if (a.first_rank) a.first_rank[t] = fr;
      if (gp >= 0 && gp < R) atomicAdd(&s_cnt[gp], 1);
      for (int j = 0; j < nk; ++j) {
        if (fr < a.ks[j] && fr < K) {
          atomicAdd(&s_hits[j], 1);
          if (gok) atomicAdd(&s_hits_p[gp * nk + j], 1);
        }
      }
    }
  }
  __syncthreads();

  const long long n_rel = r1 - r0;
  const bool skip = n_rel == 0;
  const int W = a.W, pbase = nk + 2, fbase = nk + 2 + R * nk;
  double* out = a.slab + (long long)b * W;
  for (int j = tid; j < W; j += kThreads) {
    double v = 0.0;
    if (j < nk) {
      v = skip ? 0.0 : (double)s_hits[j] / (double)n_rel;
    } else if (j == nk) {
      v = skip ? 0.0 : 1.0;
    } else if (j == nk + 1) {
      v = skip ? 1.0 : 0.0;
    } else if (j < fbase) {
      const int q = j - pbase, cnt = s_cnt[q / nk];
      v = cnt ? (double)s_hits_p[q] / (double)cnt : 0.0;
    } else {
      v = s_cnt[j - fbase] ? 1.0 : 0.0;
    }
    out[j] = v;
  }
}

// acc[j] += slab[0][j]; acc[j] += slab[1][j]; ...  -- image order, one thread per column
__global__ __launch_bounds__(kThreads) void sgg_fold(const double* __restrict__ slab, int B, int W,
                                                     double* __restrict__ acc) {
  const int j = blockIdx.x * kThreads + threadIdx.x;
  if (j < W) egtr_fold_column(slab, B, W, acc, j);
}

// Zero-shot recall: the recall over the GT triplets whose (subject class, object class, predicate) never
// occurs in training -- bit ((cs * C1 + co) * R + p) of seen_bits is clear.  Filtering the GT list changes no triplet's
// match (the argument at the top of this file), so the first ranks sgg_match left behind are all it needs.  One WAVE per
// image: lanes take the image's triplets 64 at a time and the ballots' population counts are the integer tallies.  Row of
// nk + 2 doubles: recall at ks[j] = double(hits) / double(count) (0 without a zero-shot triplet), 1 = the image has one,
// the number of them.  A triplet with an index, class or predicate out of range is not zero-shot.
struct ZeroShotArgs {
  const int* first_rank;            // [T]
  const int64_t* gt_rels;           // [T, 3]
  const int64_t* rel_off;           // [B + 1]
  const int64_t* gt_classes;        // [G]
  const int64_t* box_off;           // [B + 1]
  const unsigned long long* seen;   // [ceil(C1 * C1 * R / 64)]
  double* slab;                     // [B, nk + 2]
  long long T, G;
  int K, C1, R, nk;
  int ks[kMaxK];
};

__global__ __launch_bounds__(64) void sgg_zero_shot(const ZeroShotArgs a) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const long long r0 = clamp_off(a.rel_off[b], a.T);
  long long r1 = clamp_off(a.rel_off[b + 1], a.T);
  if (r1 < r0) r1 = r0;
  const long long g0 = clamp_off(a.box_off[b], a.G);
  long long g1 = clamp_off(a.box_off[b + 1], a.G);
  if (g1 < g0) g1 = g0;
  const long long n_boxes = g1 - g0;
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

extern "C" int egtr_sgg_zero_shot_f64(egtr_stream_t stream, const int* first_rank, const int64_t* gt_rels,
                                      const int64_t* rel_offsets, long long num_gt_rels, const int64_t* gt_classes,
                                      const int64_t* box_offsets, long long num_gt_boxes, int batch, int num_cand,
                                      int num_classes, int num_rel, const int64_t* seen_bits, const int* ks, int num_k,
                                      double* slab, double* acc) {
  if (batch < 0 || num_cand < 0 || num_cand > kMaxCand || num_classes < 1 || num_rel < 1 || num_rel > kMaxRel ||
      num_k < 1 || num_k > kMaxK || num_gt_rels < 0 || num_gt_boxes < 0 || !ks)
    return EGTR_E_ARG;
  if ((long long)num_classes * num_classes * num_rel >= (1ll << 31)) return EGTR_E_UNSUPPORTED;
  for (int j = 0; j < num_k; ++j)
    if (ks[j] < 1 || (j > 0 && ks[j] <= ks[j - 1])) return EGTR_E_ARG;
  if (batch == 0) return EGTR_OK;
  if (!rel_offsets || !box_offsets || !seen_bits || !slab) return EGTR_E_ARG;
  if (num_gt_rels > 0 && (!gt_rels || !first_rank)) return EGTR_E_ARG;
  if (num_gt_boxes > 0 && !gt_classes) return EGTR_E_ARG;

  ZeroShotArgs a;
  a.first_rank = first_rank;
  a.gt_rels = gt_rels;
  a.rel_off = rel_offsets;
  a.gt_classes = gt_classes;
  a.box_off = box_offsets;
  a.seen = reinterpret_cast<const unsigned long long*>(seen_bits);
  a.slab = slab;
  a.T = num_gt_rels;
  a.G = num_gt_boxes;
  a.K = num_cand;
  a.C1 = num_classes;
  a.R = num_rel;
  a.nk = num_k;
  for (int j = 0; j < kMaxK; ++j) a.ks[j] = j < num_k ? ks[j] : 0;

  const hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(sgg_zero_shot, dim3((unsigned)batch), dim3(64), 0, s, a);
  int st = egtr_check_launch();
  if (st != EGTR_OK || !acc) return st;
  const int W = num_k + 2;   // the rows fold like the recall slab: image order, one thread per column
  hipLaunchKernelGGL(sgg_fold, dim3(1), dim3(kThreads), 0, s, slab, batch, W, acc);
  return egtr_check_launch();
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
      num_rel < 1 || num_rel > kMaxRel || num_k < 1 || num_k > kMaxK || num_gt_rels < 0 || num_gt_boxes < 0 ||
      iou_thresh != iou_thresh)
    return EGTR_E_ARG;
  if (!ks) return EGTR_E_ARG;
  for (int j = 0; j < num_k; ++j)
    if (ks[j] < 1 || (j > 0 && ks[j] <= ks[j - 1])) return EGTR_E_ARG;
  if (num_cand > 0 && (num_obj < 1 || !cand || !pred_boxes || !pred_classes || (cand_cols == 2 && !rel_scores)))
    return EGTR_E_ARG;
  if ((num_gt_rels > 0 && !gt_rels) || (num_gt_boxes > 0 && (!gt_boxes || !gt_classes))) return EGTR_E_ARG;
  if (batch == 0) return EGTR_OK;
  if (!rel_offsets || !box_offsets || !slab) return EGTR_E_ARG;
  if ((long long)batch * num_cand * (cand_cols > 2 ? cand_cols : num_rel) >= (1ll << 40)) return EGTR_E_UNSUPPORTED;

  SggArgs a;
  a.cand = cand;
  a.rel_scores = rel_scores;
  a.pred_boxes = pred_boxes;
  a.pred_classes = pred_classes;
  a.gt_rels = gt_rels;
  a.rel_off = rel_offsets;
  a.gt_boxes = gt_boxes;
  a.gt_classes = gt_classes;
  a.box_off = box_offsets;
  a.first_rank = first_rank;
  a.slab = slab;
  a.T = num_gt_rels;
  a.G = num_gt_boxes;
  a.thr = iou_thresh;
  a.cols = cand_cols;
  a.K = num_cand;
  a.N = num_obj;
  a.R = num_rel;
  a.nk = num_k;
  a.W = (int)egtr_sgg_eval_width(num_rel, num_k);
  for (int j = 0; j < kMaxK; ++j) a.ks[j] = j < num_k ? ks[j] : 0;

  const hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(sgg_match, dim3((unsigned)batch), dim3(kThreads), 0, s, a);
  int st = egtr_check_launch();
  if (st != EGTR_OK || !acc) return st;
  hipLaunchKernelGGL(sgg_fold, dim3((unsigned)((a.W + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, slab, batch,
                     a.W, acc);
  return egtr_check_launch();
}
