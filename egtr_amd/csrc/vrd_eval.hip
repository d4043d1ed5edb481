// Phrase- and predicate-detection recall on the device: the two VRD protocols of the reference's evaluator
// (lib/evaluation/sg_eval.py: BasicSceneGraphEvaluator.vrd_modes :31-36, the "phrdet" and "preddet" branches of
// evaluate_from_dict :107-132, _compute_pred_matches(phrdet=True) :306-318), with one evaluator per predicate for the mean
// recall.  Slab rows, tallies, width and fold are those of sgg_match.h (egtr_sgg_eval_width doubles per image, folded in
// image order by a second launch), so everything downstream of a slab is shared with the sgdet evaluator.
//
// Phrase detection is recall_match<UnionBoxes> (sgg_match.h): the sgdet kernel with another box test.  A candidate's LDS
// box is the UNION of its subject and object box, (min x1, min y1, max x2, max y2), taken on the float32 boxes (min / max
// of floats are exact, so it is the union the reference takes after widening), and a candidate with matching labels
// matches when the bbox.pyx IoU (bbox_f64.h: float64, "+1", no contraction) of the GT union and its union is >= thr.  It
// writes the same first_rank buffer as sgdet, so egtr_sgg_zero_shot_f64 runs on it unchanged.
//
// preddet_match: no boxes, no classes.  For GT row j the CHOSEN candidate row is the first candidate whose (s, o) equals
// the GT pair, row 0 if there is none (numpy's argmax of an all-false column, :118).  The reference ranks the n_gt x R
// entries (pair of the chosen row of j, p, rel_scores[chosen row of j][p]) by descending score and recalls GT triplet t at
// k when one of the first k entries equals t's (s, o, p).  The order is defined here as: descending score, NaN last, -0 =
// +0, ties by ascending flat index j * R + p -- so an entry's position is #(entries strictly ahead), and no sort is
// needed.  An entry (j, p) equals t's triplet iff p = p_t and the chosen row of j carries t's pair, which holds iff t's
// pair is among the candidates and j chose the same row as t (a j that fell back to row 0 included).  Phase 1: a wave per
// GT row scans the candidates 64 at a time (ballot, lowest lane) and leaves the chosen row in LDS.  Phase 2: the entries'
// order keys go to LDS where n_gt * R <= kMaxEnt (read from rel_scores otherwise).  Phase 3: a wave per GT triplet; for
// every entry that equals it, lanes stride over all entries and count those ahead -- twice in the same loop, over all
// rows and over the rows whose predicate is the owner's (the per-predicate evaluators rank inside the GT list filtered
// by predicate, which shortens the list) -- a wave reduction gives the two positions, the minimum over the equal entries
// the two first ranks.  Integer LDS tallies, no scratch, no float atomics, plain vector stores.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "common.h"
#include "order_key.h"
#include "sgg_match.h"

using namespace egtr_eval;

namespace {

constexpr int kMaxCand = kEvalMaxCand, kMaxRel = kEvalMaxRel, kThreads = kEvalThreads;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxGt = 1024;     // GT relations per image whose chosen rows fit in LDS (preddet)
constexpr int kMaxEnt = 8192;    // preddet entries (n_gt * R) whose order keys fit in LDS
constexpr int kNoRank = 0x7fffffff;

// ---- phrase detection ----------------------------------------------------------------------------------------------------
// fminf / fmaxf return the other operand where one is NaN.  Not oi_eval.hip's oi_union_box, which keeps a NaN like torch.min /
// torch.max: a NaN coordinate gives the two different boxes, so keep both functions.
__device__ __forceinline__ float4 phrase_union_box(const float* a, const float* b) {
  return make_float4(fminf(a[0], b[0]), fminf(a[1], b[1]), fmaxf(a[2], b[2]), fmaxf(a[3], b[3]));
}

// The box layout and test of recall_match for phrase detection: one union box per candidate, one IoU.
struct UnionBoxes {
  float4 ubox[kMaxCand];
  typedef float4 Gt;

  __device__ __forceinline__ void stage(int c, const float* bs, const float* bo) {
    ubox[c] = bs ? phrase_union_box(bs, bo) : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  static __device__ __forceinline__ Gt gt(const float* bs, const float* bo) { return phrase_union_box(bs, bo); }
  __device__ __forceinline__ bool test(int c, const Gt& g, double thr) const { return egtr_iou_ge(g, ubox[c], thr); }
};

// ---- predicate detection -------------------------------------------------------------------------------------------------
struct PredArgs : EvalCommon {   // no boxes, no classes, no predicted objects
  const int64_t* cand;          // [B, K, 2] (s, o): indices of GT objects
  const float* rel_scores;      // [B, K, R]
  int* chosen_row;              // [T] or NULL
  int* first_rank;              // [T] or NULL: position in the image's whole list
  int* first_rank_pred;         // [T] or NULL: position in the list of the rows with the triplet's predicate
  double* slab;                 // [B, W]
};

// Unlike recall_match: no candidate staging; a hit compares the position against ks[j] alone (kNoRank = no entry equals the
// triplet; the list is n_gt * R long, not K).  An image with more than kMaxGt GT relations (`too_many`; the Python caller
// rejects such a batch) gets NaN recalls, correct counted / skipped / presence columns, and kNoRank / row 0 per triplet.
__global__ __launch_bounds__(kThreads) void preddet_match(const PredArgs a) {
  __shared__ unsigned s_key[kMaxEnt];
  __shared__ int s_row[kMaxGt];           // chosen candidate row, -1 = the pair is not among the candidates (row 0 is used)
  __shared__ int s_gp[kMaxGt];            // GT predicate, -1 = the GT row is out of range
  __shared__ RecallTallies s_t;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int K = a.K, R = a.R, nk = a.nk;

  s_t.zero(R, nk, tid);
  __syncthreads();   // phase 1 counts into the tallies

  const ImageRange im(a.rel_off, a.box_off, a.T, a.G, b);
  const long long r0 = im.r0, r1 = im.r1, n_boxes = im.n_box(), n_rel = im.n_rel();
  const bool too_many = n_rel > kMaxGt;
  const int n = too_many ? 0 : (int)n_rel;
  const int64_t* cand = a.cand + (long long)b * K * 2;
  const float* scores = a.rel_scores + (long long)b * K * R;

  // phase 1: the chosen row of every GT row
  for (int j = wave; j < n; j += kWaves) {
    const long long t = r0 + j;
    const long long gs = a.gt_rels[t * 3 + 0], go = a.gt_rels[t * 3 + 1], gp = a.gt_rels[t * 3 + 2];
    const bool gok = gs >= 0 && gs < n_boxes && go >= 0 && go < n_boxes;
    int row = -1;
    if (gok) {
      for (int base = 0; base < K; base += 64) {   // wave-uniform trip count
        const int c = base + lane;
        const bool m = c < K && cand[c * 2] == gs && cand[c * 2 + 1] == go;
        const unsigned long long bal = __ballot(m);
        if (bal) {
          row = base + __ffsll(bal) - 1;
          break;
        }
      }
    }
    if (lane == 0) {
      s_row[j] = row;
      s_gp[j] = (gok && gp >= 0 && gp < R) ? (int)gp : -1;
      if (a.chosen_row) a.chosen_row[t] = row < 0 ? 0 : row;
      s_t.count(gp, R);
    }
  }
  if (too_many) {
    for (long long t = r0 + tid; t < r1; t += kThreads) {
      s_t.count(a.gt_rels[t * 3 + 2], R);
      if (a.chosen_row) a.chosen_row[t] = 0;
      if (a.first_rank) a.first_rank[t] = kNoRank;
      if (a.first_rank_pred) a.first_rank_pred[t] = kNoRank;
    }
  }
  __syncthreads();

  // phase 2: order keys of the n x R entries
  const bool keys_in_lds = K > 0 && n * R <= kMaxEnt;
  if (keys_in_lds) {
    for (int j = wave; j < n; j += kWaves) {
      const int row = s_row[j] < 0 ? 0 : s_row[j];
      for (int p = lane; p < R; p += 64) s_key[j * R + p] = score_key(scores[(long long)row * R + p]);
    }
  }
  __syncthreads();

  // phase 3: a wave per GT triplet
  for (int ti = wave; ti < n; ti += kWaves) {
    const int rt = s_row[ti], gp = s_gp[ti];
    int fr_all = kNoRank, fr_pred = kNoRank;
    if (K > 0 && rt >= 0 && gp >= 0) {
      for (int j = 0; j < n; ++j) {
        const int rj = s_row[j] < 0 ? 0 : s_row[j];
        if (rj != rt) continue;                    // wave-uniform
        const unsigned key0 = keys_in_lds ? s_key[j * R + gp] : score_key(scores[(long long)rj * R + gp]);
        const int flat0 = j * R + gp;
        unsigned long long ahead = 0;              // low word: all rows; high word: rows of predicate gp
        for (int j2 = 0; j2 < n; ++j2) {
          const unsigned long long one = s_gp[j2] == gp ? 0x100000001ull : 1ull;
          const int r2 = s_row[j2] < 0 ? 0 : s_row[j2];
          const int base = j2 * R;
          for (int p = lane; p < R; p += 64) {
            const unsigned k = keys_in_lds ? s_key[base + p] : score_key(scores[(long long)r2 * R + p]);
            if (k > key0 || (k == key0 && base + p < flat0)) ahead += one;
          }
        }
        for (int off = 32; off > 0; off >>= 1) ahead += __shfl_xor(ahead, off);
        const int pos_all = (int)(ahead & 0xffffffffull), pos_pred = (int)(ahead >> 32);
        if (pos_all < fr_all) fr_all = pos_all;
        if (s_gp[j] == gp && pos_pred < fr_pred) fr_pred = pos_pred;
      }
    }
    if (lane == 0) {
      if (a.first_rank) a.first_rank[r0 + ti] = fr_all;
      if (a.first_rank_pred) a.first_rank_pred[r0 + ti] = fr_pred;
      for (int j = 0; j < nk; ++j) {
        if (fr_all < a.ks[j]) atomicAdd(&s_t.hits[j], 1);
        if (gp >= 0 && fr_pred < a.ks[j]) atomicAdd(&s_t.hits_p[gp * nk + j], 1);
      }
    }
  }
  __syncthreads();
  s_t.write_row(a.slab + (long long)b * a.W, a.W, R, nk, n_rel, too_many, tid);
}

}  // namespace

extern "C" int egtr_sgg_eval_phrdet_f32(egtr_stream_t stream, const int64_t* cand, int cand_cols, const float* rel_scores,
                                        const float* pred_boxes, const int64_t* pred_classes, int batch, int num_cand,
                                        int num_obj, int num_rel, const int64_t* gt_rels, const int64_t* rel_offsets,
                                        long long num_gt_rels, const float* gt_boxes, const int64_t* gt_classes,
                                        const int64_t* box_offsets, long long num_gt_boxes, const int* ks, int num_k,
                                        double iou_thresh, int* first_rank, double* slab, double* acc) {
  (void)rel_scores;   // the candidates carry their predicate (vrd_modes are multiple_preds=True)
  if (batch < 0 || cand_cols != 3 || num_cand < 0 || num_cand > kMaxCand || num_obj < 0 || num_rel < 1 ||
      num_rel > kMaxRel || num_gt_rels < 0 || num_gt_boxes < 0 || iou_thresh != iou_thresh || egtr_bad_ks(ks, num_k))
    return EGTR_E_ARG;
  if (num_cand > 0 && (num_obj < 1 || !cand || !pred_boxes || !pred_classes)) return EGTR_E_ARG;
  if ((num_gt_rels > 0 && !gt_rels) || (num_gt_boxes > 0 && (!gt_boxes || !gt_classes))) return EGTR_E_ARG;
  if (batch == 0) return EGTR_OK;
  if (!rel_offsets || !box_offsets || !slab) return EGTR_E_ARG;
  if ((long long)batch * num_cand * 3 >= (1ll << 40)) return EGTR_E_UNSUPPORTED;

  RecallArgs a;
  egtr_fill_common(&a, gt_rels, rel_offsets, num_gt_rels, gt_boxes, gt_classes, box_offsets, num_gt_boxes, num_cand,
                   num_obj, num_rel, (int)egtr_sgg_eval_width(num_rel, num_k), ks, num_k);
  a.cand = cand;
  a.rel_scores = nullptr;
  a.pred_boxes = pred_boxes;
  a.pred_classes = pred_classes;
  a.first_rank = first_rank;
  a.slab = slab;
  a.thr = iou_thresh;
  a.cols = 3;
  return egtr_launch_recall_match<UnionBoxes>(static_cast<hipStream_t>(stream), a, batch, acc);
}

extern "C" int egtr_sgg_eval_preddet_f32(egtr_stream_t stream, const int64_t* cand, const float* rel_scores, int batch,
                                         int num_cand, int num_rel, const int64_t* gt_rels, const int64_t* rel_offsets,
                                         long long num_gt_rels, const int64_t* box_offsets, long long num_gt_boxes,
                                         const int* ks, int num_k, int* chosen_row, int* first_rank,
                                         int* first_rank_pred, double* slab, double* acc) {
  if (batch < 0 || num_cand < 0 || num_cand > kMaxCand || num_rel < 1 || num_rel > kMaxRel || num_gt_rels < 0 ||
      num_gt_boxes < 0 || egtr_bad_ks(ks, num_k))
    return EGTR_E_ARG;
  if (num_cand > 0 && (!cand || !rel_scores)) return EGTR_E_ARG;
  if (num_gt_rels > 0 && !gt_rels) return EGTR_E_ARG;
  if (batch == 0) return EGTR_OK;
  if (!rel_offsets || !box_offsets || !slab) return EGTR_E_ARG;
  if ((long long)batch * num_cand * num_rel >= (1ll << 40)) return EGTR_E_UNSUPPORTED;

  PredArgs a;
  egtr_fill_common(&a, gt_rels, rel_offsets, num_gt_rels, nullptr, nullptr, box_offsets, num_gt_boxes, num_cand, 0,
                   num_rel, (int)egtr_sgg_eval_width(num_rel, num_k), ks, num_k);
  a.cand = cand;
  a.rel_scores = rel_scores;
  a.chosen_row = chosen_row;
  a.first_rank = first_rank;
  a.first_rank_pred = first_rank_pred;
  a.slab = slab;

  const hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(preddet_match, dim3((unsigned)batch), dim3(kThreads), 0, s, a);
  const int st = egtr_check_launch();
  if (st != EGTR_OK || !acc) return st;
  return egtr_fold_rows(s, slab, batch, a.W, acc);
}
