// Phrase- and predicate-detection recall on the device: the two VRD protocols of the reference's evaluator
// (lib/evaluation/sg_eval.py: BasicSceneGraphEvaluator.vrd_modes :31-36, the "phrdet" and "preddet" branches of
// evaluate_from_dict :107-132, _compute_pred_matches(phrdet=True) :306-318), with one evaluator per predicate for the mean
// recall.  Slab rows, width and fold are those of sgg_eval.hip (egtr_sgg_eval_width doubles per image, folded in image
// order by a second launch), so everything downstream of a slab is shared with the sgdet evaluator.
//
// phrdet_match: sgg_match with another box test.  One workgroup per image (4 waves); the candidates go to LDS as
// (class_s, class_o, predicate, valid) + the UNION box of subject and object, (min x1, min y1, max x2, max y2), taken on
// the float32 boxes (min / max of floats are exact, so it is the union the reference takes after widening).  A WAVE owns
// a GT triplet: 64 candidates per step in rank order, labels first, then the bbox.pyx IoU (bbox_f64.h: float64, "+1",
// no contraction) of the GT union and the candidate union >= thr; the ballot's lowest set bit is the first rank.  It
// writes the same first_rank buffer as sgg_match, so egtr_sgg_zero_shot_f64 runs on it unchanged.
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

namespace {

constexpr int kMaxCand = 1024;
constexpr int kMaxRel = 256;
constexpr int kMaxK = 8;
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxGt = 1024;     // GT relations per image whose chosen rows fit in LDS (preddet)
constexpr int kMaxEnt = 8192;    // preddet entries (n_gt * R) whose order keys fit in LDS
constexpr int kNoRank = 0x7fffffff;

__device__ __forceinline__ long long clamp_off(long long v, long long hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// One slab row (layout at the top of sgg_eval.hip) from the integer tallies of an image; `poison`: NaN recalls.
__device__ __forceinline__ void write_slab_row(double* out, int W, int R, int nk, long long n_rel, const int* s_hits,
                                               const int* s_cnt, const int* s_hits_p, bool poison, int tid) {
  const bool skip = n_rel == 0;
  const int pbase = nk + 2, fbase = nk + 2 + R * nk;
  const double bad = __longlong_as_double(0x7ff8000000000000ll);
  for (int j = tid; j < W; j += kThreads) {
    double v = 0.0;
    if (j < nk) {
      v = skip ? 0.0 : (poison ? bad : (double)s_hits[j] / (double)n_rel);
    } else if (j == nk) {
      v = skip ? 0.0 : 1.0;
    } else if (j == nk + 1) {
      v = skip ? 1.0 : 0.0;
    } else if (j < fbase) {
      const int q = j - pbase, cnt = s_cnt[q / nk];
      v = cnt ? (poison ? bad : (double)s_hits_p[q] / (double)cnt) : 0.0;
    } else {
      v = s_cnt[j - fbase] ? 1.0 : 0.0;
    }
    out[j] = v;
  }
}

// ---- phrase detection ----------------------------------------------------------------------------------------------------
struct PhrArgs {
  const int64_t* cand;          // [B, K, 3] (s, o, p)
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
  int K, N, R, nk, W;
  int ks[kMaxK];
};

__device__ __forceinline__ float4 union_box(const float* a, const float* b) {
  return make_float4(fminf(a[0], b[0]), fminf(a[1], b[1]), fmaxf(a[2], b[2]), fmaxf(a[3], b[3]));
}

__global__ __launch_bounds__(kThreads) void phrdet_match(const PhrArgs a) {
  __shared__ int4 s_lab[kMaxCand];        // class_s, class_o, predicate, valid
  __shared__ float4 s_ubox[kMaxCand];     // union of the subject and object boxes
  __shared__ int s_cnt[kMaxRel];
  __shared__ int s_hits_p[kMaxRel * kMaxK];
  __shared__ int s_hits[kMaxK];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int K = a.K, N = a.N, R = a.R, nk = a.nk;

  for (int i = tid; i < R * nk; i += kThreads) s_hits_p[i] = 0;
  for (int i = tid; i < R; i += kThreads) s_cnt[i] = 0;
  if (tid < kMaxK) s_hits[tid] = 0;

  for (int c = tid; c < K; c += kThreads) {
    const int64_t* row = a.cand + ((long long)b * K + c) * 3;
    const long long s = row[0], o = row[1], p = row[2];
    int4 lab = make_int4(0, 0, 0, 0);
    float4 ub = make_float4(0.f, 0.f, 0.f, 0.f);
    if (s >= 0 && s < N && o >= 0 && o < N && p >= 0 && p < R) {
      const long long cs = a.pred_classes[(long long)b * N + s], co = a.pred_classes[(long long)b * N + o];
      if (cs == (int)cs && co == (int)co) {
        lab = make_int4((int)cs, (int)co, (int)p, 1);
        ub = union_box(a.pred_boxes + ((long long)b * N + s) * 4, a.pred_boxes + ((long long)b * N + o) * 4);
      }
    }
    s_lab[c] = lab;
    s_ubox[c] = ub;
  }
  __syncthreads();

  const long long r0 = clamp_off(a.rel_off[b], a.T);
  long long r1 = clamp_off(a.rel_off[b + 1], a.T);
  if (r1 < r0) r1 = r0;
  const long long g0 = clamp_off(a.box_off[b], a.G);
  long long g1 = clamp_off(a.box_off[b + 1], a.G);
  if (g1 < g0) g1 = g0;
  const long long n_gt_boxes = g1 - g0;

  for (long long t = r0 + wave; t < r1; t += kWaves) {
    const long long gs = a.gt_rels[t * 3 + 0], go = a.gt_rels[t * 3 + 1], gp = a.gt_rels[t * 3 + 2];
    const bool gok = gs >= 0 && gs < n_gt_boxes && go >= 0 && go < n_gt_boxes && gp >= 0 && gp < R;
    int fr = K;
    if (gok) {
      const long long gcs = a.gt_classes[g0 + gs], gco = a.gt_classes[g0 + go];
      const float4 gu = union_box(a.gt_boxes + (g0 + gs) * 4, a.gt_boxes + (g0 + go) * 4);
      for (int base = 0; base < K; base += 64) {   // wave-uniform trip count: every lane reaches every ballot
        const int c = base + lane;
        bool m = false;
        if (c < K) {
          const int4 lab = s_lab[c];
          if (lab.w && lab.x == gcs && lab.y == gco && lab.z == gp) {
            const float4 q = s_ubox[c];
            m = egtr_bbox_overlap_pyx(gu.x, gu.y, gu.z, gu.w, q.x, q.y, q.z, q.w, 0) >= a.thr;
          }
        }
        const unsigned long long bal = __ballot(m);
        if (bal) {
          fr = base + __ffsll(bal) - 1;
          break;
        }
      }
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
  write_slab_row(a.slab + (long long)b * a.W, a.W, R, nk, r1 - r0, s_hits, s_cnt, s_hits_p, false, tid);
}

// ---- predicate detection -------------------------------------------------------------------------------------------------
struct PredArgs {
  const int64_t* cand;          // [B, K, 2] (s, o): indices of GT objects
  const float* rel_scores;      // [B, K, R]
  const int64_t* gt_rels;       // [T, 3]
  const int64_t* rel_off;       // [B + 1]
  const int64_t* box_off;       // [B + 1]
  int* chosen_row;              // [T] or NULL
  int* first_rank;              // [T] or NULL: position in the image's whole list
  int* first_rank_pred;         // [T] or NULL: position in the list of the rows with the triplet's predicate
  double* slab;                 // [B, W]
  long long T, G;
  int K, R, nk, W;
  int ks[kMaxK];
};

__global__ __launch_bounds__(kThreads) void preddet_match(const PredArgs a) {
  __shared__ unsigned s_key[kMaxEnt];
  __shared__ int s_row[kMaxGt];           // chosen candidate row, -1 = the pair is not among the candidates (row 0 is used)
  __shared__ int s_gp[kMaxGt];            // GT predicate, -1 = the GT row is out of range
  __shared__ int s_cnt[kMaxRel];
  __shared__ int s_hits_p[kMaxRel * kMaxK];
  __shared__ int s_hits[kMaxK];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int K = a.K, R = a.R, nk = a.nk;

  for (int i = tid; i < R * nk; i += kThreads) s_hits_p[i] = 0;
  for (int i = tid; i < R; i += kThreads) s_cnt[i] = 0;
  if (tid < kMaxK) s_hits[tid] = 0;

  const long long r0 = clamp_off(a.rel_off[b], a.T);
  long long r1 = clamp_off(a.rel_off[b + 1], a.T);
  if (r1 < r0) r1 = r0;
  const long long g0 = clamp_off(a.box_off[b], a.G);
  long long g1 = clamp_off(a.box_off[b + 1], a.G);
  if (g1 < g0) g1 = g0;
  const long long n_boxes = g1 - g0, n_rel = r1 - r0;
  const bool too_many = n_rel > kMaxGt;   // the launcher's caller rejects such a batch; a direct caller gets NaN recalls
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
      if (gp >= 0 && gp < R) atomicAdd(&s_cnt[gp], 1);
    }
  }
  if (too_many) {
    for (long long t = r0 + tid; t < r1; t += kThreads) {
      const long long gp = a.gt_rels[t * 3 + 2];
      if (gp >= 0 && gp < R) atomicAdd(&s_cnt[gp], 1);
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
        if (fr_all < a.ks[j]) atomicAdd(&s_hits[j], 1);
        if (gp >= 0 && fr_pred < a.ks[j]) atomicAdd(&s_hits_p[gp * nk + j], 1);
      }
    }
  }
  __syncthreads();
  write_slab_row(a.slab + (long long)b * a.W, a.W, R, nk, n_rel, s_hits, s_cnt, s_hits_p, too_many, tid);
}

// acc[j] += slab[0][j]; acc[j] += slab[1][j]; ...  -- image order, one thread per column
__global__ __launch_bounds__(kThreads) void vrd_fold(const double* __restrict__ slab, int B, int W,
                                                     double* __restrict__ acc) {
  const int j = blockIdx.x * kThreads + threadIdx.x;
  if (j < W) egtr_fold_column(slab, B, W, acc, j);
}

bool bad_ks(const int* ks, int num_k) {
  if (!ks || num_k < 1 || num_k > kMaxK) return true;
  for (int j = 0; j < num_k; ++j)
    if (ks[j] < 1 || (j > 0 && ks[j] <= ks[j - 1])) return true;
  return false;
}

int fold(hipStream_t s, const double* slab, int batch, int W, double* acc) {
  hipLaunchKernelGGL(vrd_fold, dim3((unsigned)((W + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, slab, batch, W,
                     acc);
  return egtr_check_launch();
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
      num_rel > kMaxRel || num_gt_rels < 0 || num_gt_boxes < 0 || iou_thresh != iou_thresh || bad_ks(ks, num_k))
    return EGTR_E_ARG;
  if (num_cand > 0 && (num_obj < 1 || !cand || !pred_boxes || !pred_classes)) return EGTR_E_ARG;
  if ((num_gt_rels > 0 && !gt_rels) || (num_gt_boxes > 0 && (!gt_boxes || !gt_classes))) return EGTR_E_ARG;
  if (batch == 0) return EGTR_OK;
  if (!rel_offsets || !box_offsets || !slab) return EGTR_E_ARG;
  if ((long long)batch * num_cand * 3 >= (1ll << 40)) return EGTR_E_UNSUPPORTED;

  PhrArgs a;
  a.cand = cand;
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
  a.K = num_cand;
  a.N = num_obj;
  a.R = num_rel;
  a.nk = num_k;
  a.W = (int)egtr_sgg_eval_width(num_rel, num_k);
  for (int j = 0; j < kMaxK; ++j) a.ks[j] = j < num_k ? ks[j] : 0;

  const hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(phrdet_match, dim3((unsigned)batch), dim3(kThreads), 0, s, a);
  const int st = egtr_check_launch();
  if (st != EGTR_OK || !acc) return st;
  return fold(s, slab, batch, a.W, acc);
}

extern "C" int egtr_sgg_eval_preddet_f32(egtr_stream_t stream, const int64_t* cand, const float* rel_scores, int batch,
                                         int num_cand, int num_rel, const int64_t* gt_rels, const int64_t* rel_offsets,
                                         long long num_gt_rels, const int64_t* box_offsets, long long num_gt_boxes,
                                         const int* ks, int num_k, int* chosen_row, int* first_rank,
                                         int* first_rank_pred, double* slab, double* acc) {
  if (batch < 0 || num_cand < 0 || num_cand > kMaxCand || num_rel < 1 || num_rel > kMaxRel || num_gt_rels < 0 ||
      num_gt_boxes < 0 || bad_ks(ks, num_k))
    return EGTR_E_ARG;
  if (num_cand > 0 && (!cand || !rel_scores)) return EGTR_E_ARG;
  if (num_gt_rels > 0 && !gt_rels) return EGTR_E_ARG;
  if (batch == 0) return EGTR_OK;
  if (!rel_offsets || !box_offsets || !slab) return EGTR_E_ARG;
  if ((long long)batch * num_cand * num_rel >= (1ll << 40)) return EGTR_E_UNSUPPORTED;

  PredArgs a;
  a.cand = cand;
  a.rel_scores = rel_scores;
  a.gt_rels = gt_rels;
  a.rel_off = rel_offsets;
  a.box_off = box_offsets;
  a.chosen_row = chosen_row;
  a.first_rank = first_rank;
  a.first_rank_pred = first_rank_pred;
  a.slab = slab;
  a.T = num_gt_rels;
  a.G = num_gt_boxes;
  a.K = num_cand;
  a.R = num_rel;
  a.nk = num_k;
  a.W = (int)egtr_sgg_eval_width(num_rel, num_k);
  for (int j = 0; j < kMaxK; ++j) a.ks[j] = j < num_k ? ks[j] : 0;

  const hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(preddet_match, dim3((unsigned)batch), dim3(kThreads), 0, s, a);
  const int st = egtr_check_launch();
  if (st != EGTR_OK || !acc) return st;
  return fold(s, slab, batch, a.W, acc);
}
