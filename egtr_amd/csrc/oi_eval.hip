// Open Images relation metrics on the device: the detection selection, recall matching and AP scoring of the reference's
// OI evaluator (lib/evaluation/oi_eval.py: OIEvaluator.__call__ :443-477, eval_rel_results :77-294;
// lib/evaluation/ap_eval_rel.py: prepare_mAP_dets, ap_eval, get_ap, bbox_iou), fed by evaluate_batch
// (train_egtr.py:154-174).
//
// oi_select_partial + oi_select_merge (egtr_oi_select_f32): the per-image top `topk` of the [M, kk] array
//   spo[m][j] = (score_s * score_o) * top_j(pred_scores[m])   (float32, two roundings in that order; kk = min(prd_k, R))
// among the entries > 1e-5.  An entry is one 64-bit KEY = float bits of spo (positive, so the bits order like the
// values) << 32 | (2^20 - 1 - flat) << 8 | predicate, flat = m * kk + j: keys order by score descending, then by flat index
// ascending, and are unique.  Pass 1 has many workgroups per image: each takes 512 pairs, finds every pair's kk best
// predicates by kk argmax passes over the row (NaN last, ties to the lower predicate index: numpy argsort(-row) with a
// defined tie rule),
// writes the keys to LDS and keeps its `topk` largest (radix_threshold below: a radix select of the threshold key over the
// nonzero keys; then the compaction of topk_select.h).  Pass 2 is one workgroup per image: the same select over the
// partial lists, the compaction to LDS and the bitonic sort of topk_select.h; it writes the detections (s, o, p, score)
// in rank order and their count.  radix_threshold (8-bit digits) stays beside the 11-bit select of topk_select.h because
// the shared one made oi_select_partial slower than its spread (profiles/eval_kernels_shared_ab.txt).
//
// oi_match + the fold of sgg_match.h (egtr_oi_match_f32): one workgroup per image (4 waves).
//   * recall: the first-rank matching of sgg_match.h with the sgdet box test on the detections -- labels (s, p, o) and
//     the fp64 bbox.pyx IoU >= 0.5 -- gives hits@k = #{GT triplets with first rank < k};
//   * npos: GT triplets per predicate class (integer LDS tallies);
//   * TP flags for the AP: a wave per predicate class walks that class's detections in rank order (the in-image order of
//     prepare_mAP_dets); its lanes hold the image's GT triplets of the class, compute the float32 bbox_iou of
//     ap_eval_rel.py (intersection (min - max) + 1 clamped at 0, areas WITHOUT +1, inter / ((a1 + a2) - inter)) times the
//     label mask, and a wave reduction gives ovmax (NaN if any is NaN, like torch.max) and the first argmax jmax.  A
//     detection is a TP when ovmax > 0.5 and GT jmax is not yet visited (visited bits live in the lanes' registers, one
//     bit per 64 GT triplets); rel mode uses min(iou_s, iou_o), phr mode the IoU of the union boxes, each with its own
//     visited state.  The visited state is per image, so the flags need no other image.
//   Per-image rows go to a slab; egtr_fold_rows adds them into the fp64 accumulators in image order.
//
// oi_ap (egtr_oi_ap_f64): once per evaluation, one workgroup per (class, rel | phr) over the class's records, already
// sorted by confidence: tp cumsum (exact integers in fp64), rec = cum / (npos + 1e-12), prec = cum / (i + 1), the
// reverse-cummax envelope, and AP = sum of (rec_i - rec_{i-1}) * envelope_i as a left fold in record order.
//
// Slab / accumulator layout (W = egtr_oi_eval_width(C, nk) doubles per row):
//   [0, nk)            per-image recall hits / (n_gt + 1e-12) at ks[j]   (0 for a skipped image)
//   [nk, 2nk)          hits at ks[j]
//   2nk                n_gt (GT triplets of the image)
//   2nk + 1            1 = image counted
//   2nk + 2            1 = image skipped (no GT relation; the reference raises a KeyError there)
//   2nk + 3 + c        npos of predicate class c (GT triplets of class c)
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "common.h"
#include "sgg_match.h"
#include "topk_select.h"

using namespace egtr_eval;

namespace {

typedef unsigned long long u64;

constexpr int kMaxRel = kEvalMaxRel, kMaxTopk = kEvalMaxCand, kMaxK = kEvalMaxK;
constexpr int kMaxPrdK = 8;
constexpr long long kMaxPairs = 300ll * 300;
constexpr int kMaxGtPerImage = 64 * 64;   // AP visited bits: one 64-bit register per lane
constexpr int kFlatBits = 20;             // flat = m * kk + j < 2^20 (90000 * 8 < 2^20)
constexpr int kPairsPerBlock = 512;
constexpr int kSelThreads = 256;
constexpr int kMergeThreads = 1024;
constexpr int kMatchThreads = kEvalThreads;
constexpr int kApThreads = 256;

__device__ __forceinline__ u64 oi_key(float score, unsigned flat, int p) {
  return ((u64)__float_as_uint(score) << 32) | ((u64)((1u << kFlatBits) - 1u - flat) << 8) | (u64)(unsigned)p;
}

// (av, ai) ranks above (bv, bi) in numpy's argsort(-row) with the defined tie rule: numbers by value descending, NaN last,
// equal values (or two NaN) by lower index; an empty slot (index < 0) ranks below everything.
__device__ __forceinline__ bool ranks_above(float av, int ai, float bv, int bi) {
  const bool an = av != av, bn = bv != bv;
  const bool tie = (av == bv) || (an && bn);
  return ai >= 0 && (bi < 0 || (!an && bn) || (!an && av > bv) || (tie && ai < bi));
}

// Threshold key T >= 1 such that exactly min(want, nnz) of the nonzero keys get(0 .. n-1) are >= T (the keys are unique).
// MSB-first radix select, 8 bits per pass, over a 256-bin LDS histogram; wave 0 finds the bin that holds the want-th
// largest key with a suffix scan.  A pass whose bin holds exactly the keys still wanted ends the search early.  Called by
// every thread of the workgroup (NT threads) with uniform arguments.
template <int NT, class Get>
__device__ u64 radix_threshold(Get get, int n, int want, int* s_hist, u64* s_b) {
  const int tid = threadIdx.x;
  __shared__ int s_nnz;
  if (tid == 0) s_nnz = 0;
  __syncthreads();
  int local = 0;
  for (int i = tid; i < n; i += NT) local += get(i) != 0;
  if (local) atomicAdd(&s_nnz, local);
  __syncthreads();
  const int nnz = s_nnz;
  if (nnz <= want) return 1;
  u64 prefix = 0, mask = 0;
  int remaining = want;
  for (int shift = 56; shift >= 0; shift -= 8) {
    for (int i = tid; i < 256; i += NT) s_hist[i] = 0;
    __syncthreads();
    for (int i = tid; i < n; i += NT) {
      const u64 k = get(i);
      if (k && (k & mask) == prefix) atomicAdd(&s_hist[(k >> shift) & 255], 1);
    }
    __syncthreads();
    if (tid < 64) {
      const int c0 = s_hist[4 * tid], c1 = s_hist[4 * tid + 1], c2 = s_hist[4 * tid + 2], c3 = s_hist[4 * tid + 3];
      const int tot = c0 + c1 + c2 + c3;
      int suf = tot;   // keys in the bins of lanes >= tid
      for (int off = 1; off < 64; off <<= 1) {
        const int v = __shfl_down(suf, off, 64);
        if (tid + off < 64) suf += v;
      }
      const int above = suf - tot;
      if (above < remaining && remaining <= suf) {
        int acc = above, d = 4 * tid, cnt = c0;
        if (acc + c3 >= remaining) {
          d = 4 * tid + 3;
          cnt = c3;
        } else if ((acc += c3) + c2 >= remaining) {
          d = 4 * tid + 2;
          cnt = c2;
        } else if ((acc += c2) + c1 >= remaining) {
          d = 4 * tid + 1;
          cnt = c1;
        } else {
          acc += c1;
        }
        s_b[0] = (u64)d;
        s_b[1] = ((u64)(unsigned)acc << 32) | (unsigned)cnt;
      }
    }
    __syncthreads();
    const int d = (int)s_b[0], acc = (int)(s_b[1] >> 32), cnt = (int)(s_b[1] & 0xffffffffu);
    __syncthreads();
    remaining -= acc;
    prefix |= (u64)d << shift;
    mask |= 255ull << shift;
    if (cnt == remaining) break;   // every key of this bin is wanted: keys >= prefix are exactly the selection
  }
  return prefix ? prefix : 1;
}

// The nonzero keys of an array, as a source of topk_select.h's compaction.
template <int NT>
struct NonzeroKeys {
  const u64* keys;
  int n;

  template <class F>
  __device__ __forceinline__ void operator()(F&& f) const {
    for (int i = threadIdx.x; i < n; i += NT) {
      const u64 k = keys[i];
      if (k) f(k);
    }
  }
};

struct SelArgs {
  const float* scores;    // [B, M, R] with img_stride / row_stride (elements)
  const float* obj;       // [B, N]
  const int64_t* pairs;   // [M, 2] (s, o) per image at pair_stride, or NULL = row-major cartesian product
  u64* partial;           // [B, nblk, topk]
  int* det_sop;           // [B, topk, 3]
  float* det_score;       // [B, topk]
  int* det_count;         // [B]
  long long img_stride, row_stride, pair_stride;
  int M, N, R, kk, topk, nblk;
};

__device__ __forceinline__ void pair_of(const SelArgs& a, int b, int m, long long* s, long long* o) {
  if (a.pairs) {
    const int64_t* pr = a.pairs + (long long)b * a.pair_stride + (long long)m * 2;
    *s = pr[0];
    *o = pr[1];
  } else {
    *s = m / a.N;
    *o = m % a.N;
  }
}

__global__ __launch_bounds__(kSelThreads) void oi_select_partial(const SelArgs a) {
  __shared__ u64 s_key[kPairsPerBlock * kMaxPrdK];
  __shared__ int s_hist[256];
  __shared__ u64 s_b[2];
  __shared__ int s_cnt;
  const int tid = threadIdx.x, blk = blockIdx.x, b = blockIdx.y, kk = a.kk, R = a.R, N = a.N;
  const int m0 = blk * kPairsPerBlock;
  for (int lp = tid; lp < kPairsPerBlock; lp += kSelThreads) {
    const int m = m0 + lp;
    float so = 0.f;
    const float* row = nullptr;
    if (m < a.M) {
      long long s, o;
      pair_of(a, b, m, &s, &o);
      if (s >= 0 && s < N && o >= 0 && o < N) {
        so = a.obj[(long long)b * N + s] * a.obj[(long long)b * N + o];
        row = a.scores + (long long)b * a.img_stride + (long long)m * a.row_stride;
      }
    }
    // pass q picks the best predicate ranking below pass q-1's pick (the row is re-read from L1; no register arrays)
    float pv = 0.f;
    int pi = -1;
    for (int q = 0; q < kk; ++q) {
      float bv = 0.f;
      int bi = -1;
      if (row) {
        for (int r = 0; r < R; ++r) {
          const float v = row[r];
          const bool take = (pi < 0 || ranks_above(pv, pi, v, r)) && ranks_above(v, r, bv, bi);
          bv = take ? v : bv;
          bi = take ? r : bi;
        }
      }
      u64 key = 0;
      if (bi >= 0) {
        const float v = so * bv;
        if (v > 1e-5f) key = oi_key(v, (unsigned)(m * kk + q), bi);
      }
      s_key[lp * kk + q] = key;
      pv = bv;
      pi = bi;
    }
  }
  __syncthreads();
  const int n = kPairsPerBlock * kk;
  const u64 thr = radix_threshold<kSelThreads>([&](int i) { return s_key[i]; }, n, a.topk, s_hist, s_b);
  u64* out = a.partial + ((long long)b * a.nblk + blk) * a.topk;
  const int cnt = egtr_compact_ge(NonzeroKeys<kSelThreads>{s_key, n}, thr, a.topk, out, &s_cnt);
  for (int i = cnt + tid; i < a.topk; i += kSelThreads) out[i] = 0;
}

__global__ __launch_bounds__(kMergeThreads) void oi_select_merge(const SelArgs a) {
  __shared__ u64 s_sort[kMaxTopk];
  __shared__ int s_hist[256];
  __shared__ u64 s_b[2];
  __shared__ int s_cnt;
  const int tid = threadIdx.x, b = blockIdx.x;
  const int n = a.nblk * a.topk;
  const u64* keys = a.partial + (long long)b * n;
  const u64 thr = radix_threshold<kMergeThreads>([&](int i) { return keys[i]; }, n, a.topk, s_hist, s_b);
  const int cnt = egtr_compact_ge(NonzeroKeys<kMergeThreads>{keys, n}, thr, a.topk, s_sort, &s_cnt);
  egtr_bitonic_sort_desc<kMergeThreads>(s_sort, cnt);
  if (tid < a.topk) {
    int* sop = a.det_sop + ((long long)b * a.topk + tid) * 3;
    if (tid < cnt) {
      const u64 k = s_sort[tid];
      const unsigned flat = (1u << kFlatBits) - 1u - (unsigned)((k >> 8) & ((1u << kFlatBits) - 1u));
      long long s, o;
      pair_of(a, b, (int)(flat / (unsigned)a.kk), &s, &o);
      sop[0] = (int)s;
      sop[1] = (int)o;
      sop[2] = (int)(k & 255);
      a.det_score[(long long)b * a.topk + tid] = __uint_as_float((unsigned)(k >> 32));
    } else {
      sop[0] = -1;
      sop[1] = -1;
      sop[2] = -1;
      a.det_score[(long long)b * a.topk + tid] = 0.f;
    }
  }
  if (tid == 0) a.det_count[b] = cnt;
}

struct MatchArgs : EvalCommon {   // K = topk, R = C predicate classes
  const int* det_sop;           // [B, topk, 3]
  const int* det_count;         // [B]
  const float* pred_boxes;      // [B, N, 4] xyxy
  const int64_t* pred_classes;  // [B, N]
  unsigned char* tp;            // [2, B, topk]: rel flags, then phr flags
  double* slab;                 // [B, W]
};

// NaN-propagating min / max (torch.min / torch.max / np.minimum / np.maximum on two values)
__device__ __forceinline__ float nan_min(float a, float b) { return (a != a || a < b) ? a : b; }
__device__ __forceinline__ float nan_max(float a, float b) { return (a != a || a > b) ? a : b; }

// ap_eval_rel.bbox_iou of one pair, float32, the reference's operation order
__device__ __forceinline__ float bbox_iou_f32(float4 p, float4 q) {
#pragma clang fp contract(off)
  float w = (nan_min(p.z, q.z) - nan_max(p.x, q.x)) + 1.0f;
  float h = (nan_min(p.w, q.w) - nan_max(p.y, q.y)) + 1.0f;
  w = w < 0.0f ? 0.0f : w;   // clamp(min=0), NaN stays NaN
  h = h < 0.0f ? 0.0f : h;
  const float inter = w * h;
  const float a1 = (p.z - p.x) * (p.w - p.y);
  const float a2 = (q.z - q.x) * (q.w - q.y);
  return inter / ((a1 + a2) - inter);
}

// boxes_union of ap_eval_rel.py: a NaN coordinate stays NaN.  Not vrd_eval.hip's phrase_union_box (fminf / fmaxf).
__device__ __forceinline__ float4 oi_union_box(float4 s, float4 o) {
  return make_float4(nan_min(s.x, o.x), nan_min(s.y, o.y), nan_max(s.z, o.z), nan_max(s.w, o.w));
}

// (v, i) is a better torch.max / argmax candidate than (w, j): NaN first, then the larger value, ties to the lower index;
// an empty candidate (index < 0) loses to everything
__device__ __forceinline__ bool argmax_better(float v, int i, float w, int j) {
  const bool vn = v != v, wn = w != w;
  const bool tie = (v == w) || (vn && wn);
  return i >= 0 && (j < 0 || (vn && !wn) || (!wn && v > w) || (tie && i < j));
}

__device__ __forceinline__ void wave_argmax(float* v, int* i) {
  for (int off = 32; off > 0; off >>= 1) {
    const float w = __shfl_xor(*v, off, 64);
    const int j = __shfl_xor(*i, off, 64);
    if (argmax_better(w, j, *v, *i)) {
      *v = w;
      *i = j;
    }
  }
}

// The recall part is recall_match's (sgg_match.h) with these differences, each the reference's OI behaviour: gok does not
// look at the GT predicate, the IoU threshold is the literal 0.5, K is det_count[b] clamped to [0, topk], and the row
// layout (npos, no per-predicate recall) is its own.
__global__ __launch_bounds__(kMatchThreads) void oi_match(const MatchArgs a) {
  __shared__ int4 s_lab[kMaxTopk];   // class_s, class_o, predicate, valid
  __shared__ SubjectObjectBoxes s_box;
  __shared__ int s_npos[kMaxRel];
  __shared__ int s_ndet[kMaxRel];
  __shared__ int s_hits[kMaxK];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int C = a.R, nk = a.nk, topk = a.K;
  int K = a.det_count[b];
  K = K < 0 ? 0 : (K > topk ? topk : K);

  for (int i = tid; i < C; i += kMatchThreads) {
    s_npos[i] = 0;
    s_ndet[i] = 0;
  }
  if (tid < kMaxK) s_hits[tid] = 0;
  __syncthreads();

  for (int d = tid; d < K; d += kMatchThreads) {
    const int* sop = a.det_sop + ((long long)b * topk + d) * 3;
    const float *bs, *bo;
    const int4 lab = egtr_candidate_label(a.pred_boxes, a.pred_classes, b, a.N, C, sop[0], sop[1], sop[2], &bs, &bo);
    if (lab.w) atomicAdd(&s_ndet[lab.z], 1);
    s_lab[d] = lab;
    s_box.stage(d, bs, bo);
  }
  __syncthreads();

  const ImageRange im(a.rel_off, a.box_off, a.T, a.G, b);
  const long long r0 = im.r0, r1 = im.r1, g0 = im.g0, n_gt_boxes = im.n_box(), n_rel = im.n_rel();
  const bool skip = n_rel == 0;
  unsigned char* tp_rel = a.tp + (long long)b * topk;
  unsigned char* tp_phr = a.tp + ((long long)gridDim.x + b) * topk;

  // ---- recall: first matching rank of each GT triplet, one wave per triplet
  for (long long t = r0 + wave; t < r1; t += kMatchThreads / 64) {
    const long long gs = a.gt_rels[t * 3 + 0], go = a.gt_rels[t * 3 + 1], gp = a.gt_rels[t * 3 + 2];
    const bool gok = gs >= 0 && gs < n_gt_boxes && go >= 0 && go < n_gt_boxes;
    int fr = K;
    if (gok) {
      const SubjectObjectBoxes::Gt g = SubjectObjectBoxes::gt(a.gt_boxes + (g0 + gs) * 4, a.gt_boxes + (g0 + go) * 4);
      fr = egtr_first_rank_wave(s_lab, K, a.gt_classes[g0 + gs], a.gt_classes[g0 + go], gp, lane,
                                [&](int c) { return s_box.test(c, g, 0.5); });
    }
    if (lane == 0) {
      if (gp >= 0 && gp < C) atomicAdd(&s_npos[gp], 1);
      for (int j = 0; j < nk; ++j)
        if (fr < a.ks[j] && fr < K) atomicAdd(&s_hits[j], 1);
    }
  }

  // ---- AP flags: one wave per predicate class with detections, detections in rank order
  for (int c = wave; c < C; c += kMatchThreads / 64) {
    if (s_ndet[c] == 0) continue;
    unsigned long long vis_rel = 0, vis_phr = 0;   // bit q of lane l: GT triplet r0 + 64 q + l visited
    const long long nch = (n_rel + 63) / 64;
    const int nchunk = nch < kMaxGtPerImage / 64 ? (int)nch : kMaxGtPerImage / 64;
    for (int base = 0; base < K; base += 64) {
      const int dd = base + lane;
      unsigned long long mine = __ballot(dd < K && s_lab[dd].w && s_lab[dd].z == c);
      while (mine) {
        const int d = base + __ffsll(mine) - 1;
        mine &= mine - 1;
        const int4 lab = s_lab[d];
        const float4 ds = s_box.sbox[d], dob = s_box.obox[d], dr = oi_union_box(ds, dob);
        float best_r = 0.f, best_p = 0.f;
        int ir = -1, ip = -1;
        bool have = false, valid_any = false;
        for (int q = 0; q < nchunk; ++q) {
          const long long t = r0 + 64ll * q + lane;
          if (t < r1 && a.gt_rels[t * 3 + 2] == c) {
            const long long gs = a.gt_rels[t * 3 + 0], go = a.gt_rels[t * 3 + 1];
            if (gs >= 0 && gs < n_gt_boxes && go >= 0 && go < n_gt_boxes) {
              have = true;
              const bool valid = a.gt_classes[g0 + gs] == lab.x && a.gt_classes[g0 + go] == lab.y;
              valid_any |= valid;
              const float* gsb = a.gt_boxes + (g0 + gs) * 4;
              const float* gob = a.gt_boxes + (g0 + go) * 4;
              const float4 gsv = make_float4(gsb[0], gsb[1], gsb[2], gsb[3]);
              const float4 gov = make_float4(gob[0], gob[1], gob[2], gob[3]);
              const float m = valid ? 1.0f : 0.0f;
              const float ovr = nan_min(bbox_iou_f32(ds, gsv), bbox_iou_f32(dob, gov)) * m;
              const float ovp = bbox_iou_f32(dr, oi_union_box(gsv, gov)) * m;
              const int j = 64 * q + lane;
              if (argmax_better(ovr, j, best_r, ir)) {
                best_r = ovr;
                ir = j;
              }
              if (argmax_better(ovp, j, best_p, ip)) {
                best_p = ovp;
                ip = j;
              }
            }
          }
        }
        const bool any_gt = __ballot(have) != 0, any_valid = __ballot(valid_any) != 0;
        wave_argmax(&best_r, &ir);
        wave_argmax(&best_p, &ip);
        bool tr = false, tph = false;
        if (any_gt && any_valid) {
          // ovmax > 0.5 (NaN compares false) and GT jmax not yet visited
          if (best_r > 0.5f) {
            const unsigned long long v = __shfl(vis_rel, ir & 63, 64);
            tr = !((v >> (ir >> 6)) & 1ull);
            if (tr && lane == (ir & 63)) vis_rel |= 1ull << (ir >> 6);
          }
          if (best_p > 0.5f) {
            const unsigned long long v = __shfl(vis_phr, ip & 63, 64);
            tph = !((v >> (ip >> 6)) & 1ull);
            if (tph && lane == (ip & 63)) vis_phr |= 1ull << (ip >> 6);
          }
        }
        if (lane == 0) {
          tp_rel[d] = tr ? 1 : 0;
          tp_phr[d] = tph ? 1 : 0;
        }
      }
    }
  }
  for (int d = tid; d < topk; d += kMatchThreads) {
    const bool lab_ok = d < K && s_lab[d].w;
    if (!lab_ok) {
      tp_rel[d] = 0;
      tp_phr[d] = 0;
    }
  }
  __syncthreads();

  const int W = a.W;
  double* out = a.slab + (long long)b * W;
  for (int j = tid; j < W; j += kMatchThreads) {
    double v = 0.0;
    if (!skip) {
      if (j < nk) {
        v = (double)s_hits[j] / ((double)n_rel + 1e-12);
      } else if (j < 2 * nk) {
        v = (double)s_hits[j - nk];
      } else if (j == 2 * nk) {
        v = (double)n_rel;
      } else if (j == 2 * nk + 1) {
        v = 1.0;
      } else if (j >= 2 * nk + 3) {
        v = (double)s_npos[j - 2 * nk - 3];
      }
    } else if (j == 2 * nk + 2) {
      v = 1.0;
    }
    out[j] = v;
  }
}

// inclusive scan of v over the workgroup (kApThreads threads); s_w: one int per wave
__device__ __forceinline__ int block_inclusive_sum(int v, int* s_w) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int off = 1; off < 64; off <<= 1) {
    const int u = __shfl_up(v, off, 64);
    if (lane >= off) v += u;
  }
  if (lane == 63) s_w[wave] = v;
  __syncthreads();
  for (int w = 0; w < wave; ++w) v += s_w[w];
  __syncthreads();
  return v;
}

// inclusive suffix max of v (>= 0) over the workgroup
__device__ __forceinline__ double block_suffix_max(double v, double* s_w) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int off = 1; off < 64; off <<= 1) {
    const double u = __shfl_down(v, off, 64);
    if (lane + off < 64) v = fmax(v, u);
  }
  if (lane == 0) s_w[wave] = v;
  __syncthreads();
  for (int w = wave + 1; w < kApThreads / 64; ++w) v = fmax(v, s_w[w]);
  __syncthreads();
  return v;
}

__global__ __launch_bounds__(kApThreads) void oi_ap(const unsigned char* __restrict__ tp, const int64_t* seg_off,
                                                     const double* __restrict__ npos, long long n_total, int C,
                                                     double* __restrict__ scratch, double* __restrict__ ap) {
#pragma clang fp contract(off)
  __shared__ int s_wi[kApThreads / 64];
  __shared__ double s_wd[kApThreads / 64];
  const int c = blockIdx.x, mode = blockIdx.y, tid = threadIdx.x;
  const long long a0 = egtr_clamp_off(seg_off[c], n_total);
  long long a1 = egtr_clamp_off(seg_off[c + 1], n_total);
  if (a1 < a0) a1 = a0;
  const long long n = a1 - a0;
  const unsigned char* f = tp + mode * n_total + a0;
  double* cum = scratch + (2ll * mode) * n_total + a0;
  double* env = scratch + (2ll * mode + 1) * n_total + a0;
  const double denom = npos[c] + 1e-12;

  // tp cumsum (exact integers) and prec = cum / (i + 1)
  int carry = 0;
  for (long long t0 = 0; t0 < n; t0 += kApThreads) {
    const long long i = t0 + tid;
    const int v = i < n ? (f[i] != 0) : 0;
    const int incl = block_inclusive_sum(v, s_wi) + carry;
    if (i < n) cum[i] = (double)incl;
    if (tid == kApThreads - 1) s_wi[0] = incl;
    __syncthreads();
    carry = s_wi[0];
    __syncthreads();
  }
  // envelope_i = max(prec_i .. prec_{n-1}, 0), tiles from the end
  double dcarry = 0.0;
  for (long long t1 = n; t1 > 0; t1 -= kApThreads) {
    const long long i = t1 - kApThreads + tid;
    const double pr = i >= 0 ? cum[i] / (double)(i + 1) : 0.0;
    const double e = fmax(block_suffix_max(pr, s_wd), dcarry);
    if (i >= 0) env[i] = e;
    if (tid == 0) s_wd[0] = e;
    __syncthreads();
    dcarry = s_wd[0];
    __syncthreads();
  }
  // AP = sum over i of (rec_i - rec_{i-1}) * envelope_i, a left fold in record order (wave 0)
  if (tid < 64) {
    double sum = 0.0;
    for (long long t0 = 0; t0 < n; t0 += 64) {
      const long long i = t0 + tid;
      double term = 0.0;
      if (i < n) {
        const double r = cum[i] / denom, rp = i > 0 ? cum[i - 1] / denom : 0.0;
        term = (r - rp) * env[i];
      }
      unsigned long long nz = __ballot(term != 0.0);
      while (nz) {
        const int l = __ffsll(nz) - 1;
        nz &= nz - 1;
        sum += __shfl(term, l, 64);
      }
    }
    if (tid == 0) ap[mode * C + c] = sum;
  }
}

}  // namespace

extern "C" long long egtr_oi_eval_width(int num_rel, int num_k) {
  if (num_rel < 1 || num_rel > kMaxRel || num_k < 1 || num_k > kMaxK) return EGTR_E_ARG;
  return 2ll * num_k + 3 + num_rel;
}

extern "C" long long egtr_oi_select_workspace_bytes(int num_pairs, int topk, int prd_k, int batch) {
  if (num_pairs < 0 || num_pairs > kMaxPairs || topk < 1 || topk > kMaxTopk || prd_k < 1 || prd_k > kMaxPrdK ||
      batch < 0)
    return EGTR_E_ARG;
  const long long nblk = num_pairs > 0 ? (num_pairs + kPairsPerBlock - 1) / kPairsPerBlock : 1;
  return (long long)batch * nblk * topk * (long long)sizeof(u64);
}

extern "C" int egtr_oi_select_f32(egtr_stream_t stream, const float* pred_scores, long long img_stride,
                                  long long row_stride, const float* obj_scores, const int64_t* pairs,
                                  long long pair_stride, int batch, int num_pairs, int num_obj, int num_rel, int topk,
                                  int prd_k, void* workspace, int* det_sop, float* det_score, int* det_count) {
  if (batch < 0 || num_pairs < 0 || num_pairs > kMaxPairs || num_obj < 1 || num_rel < 1 || num_rel > kMaxRel ||
      topk < 1 || topk > kMaxTopk || prd_k < 1 || prd_k > kMaxPrdK || img_stride < 0 || row_stride < num_rel ||
      pair_stride < 0)
    return EGTR_E_ARG;
  if (batch == 0) return EGTR_OK;
  if (!obj_scores || !det_sop || !det_score || !det_count || (num_pairs > 0 && (!pred_scores || !workspace)))
    return EGTR_E_ARG;
  if (!pairs && (long long)num_obj * num_obj != num_pairs) return EGTR_E_ARG;
  if (num_pairs > 0 && batch > 1 && img_stride == 0) return EGTR_E_ARG;

  SelArgs a;
  a.scores = pred_scores;
  a.obj = obj_scores;
  a.pairs = pairs;
  a.partial = static_cast<u64*>(workspace);
  a.det_sop = det_sop;
  a.det_score = det_score;
  a.det_count = det_count;
  a.img_stride = img_stride;
  a.row_stride = row_stride;
  a.pair_stride = pair_stride;
  a.M = num_pairs;
  a.N = num_obj;
  a.R = num_rel;
  a.kk = prd_k < num_rel ? prd_k : num_rel;
  a.topk = topk;
  a.nblk = num_pairs > 0 ? (num_pairs + kPairsPerBlock - 1) / kPairsPerBlock : 0;
  const hipStream_t s = static_cast<hipStream_t>(stream);
  if (a.nblk > 0) {
    hipLaunchKernelGGL(oi_select_partial, dim3((unsigned)a.nblk, (unsigned)batch), dim3(kSelThreads), 0, s, a);
    const int st = egtr_check_launch();
    if (st != EGTR_OK) return st;
  }
  hipLaunchKernelGGL(oi_select_merge, dim3((unsigned)batch), dim3(kMergeThreads), 0, s, a);
  return egtr_check_launch();
}

extern "C" int egtr_oi_match_f32(egtr_stream_t stream, const int* det_sop, const int* det_count, int batch, int topk,
                                 const float* pred_boxes, const int64_t* pred_classes, int num_obj, int num_rel,
                                 const int64_t* gt_rels, const int64_t* rel_offsets, long long num_gt_rels,
                                 const float* gt_boxes, const int64_t* gt_classes, const int64_t* box_offsets,
                                 long long num_gt_boxes, const int* ks, int num_k, unsigned char* tp, double* slab,
                                 double* acc) {
  if (batch < 0 || topk < 1 || topk > kMaxTopk || num_obj < 1 || num_rel < 1 || num_rel > kMaxRel ||
      num_gt_rels < 0 || num_gt_boxes < 0 || egtr_bad_ks(ks, num_k))
    return EGTR_E_ARG;
  if ((num_gt_rels > 0 && !gt_rels) || (num_gt_boxes > 0 && (!gt_boxes || !gt_classes))) return EGTR_E_ARG;
  if (batch == 0) return EGTR_OK;
  if (!det_sop || !det_count || !pred_boxes || !pred_classes || !rel_offsets || !box_offsets || !tp || !slab)
    return EGTR_E_ARG;

  MatchArgs a;
  egtr_fill_common(&a, gt_rels, rel_offsets, num_gt_rels, gt_boxes, gt_classes, box_offsets, num_gt_boxes, topk, num_obj,
                   num_rel, (int)egtr_oi_eval_width(num_rel, num_k), ks, num_k);
  a.det_sop = det_sop;
  a.det_count = det_count;
  a.pred_boxes = pred_boxes;
  a.pred_classes = pred_classes;
  a.tp = tp;
  a.slab = slab;

  const hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(oi_match, dim3((unsigned)batch), dim3(kMatchThreads), 0, s, a);
  const int st = egtr_check_launch();
  if (st != EGTR_OK || !acc) return st;
  return egtr_fold_rows(s, slab, batch, a.W, acc);
}

extern "C" int egtr_oi_ap_f64(egtr_stream_t stream, const unsigned char* tp_sorted, const int64_t* seg_offsets,
                              const double* npos, long long num_records, int num_rel, double* scratch, double* ap) {
  if (num_records < 0 || num_rel < 1 || num_rel > kMaxRel) return EGTR_E_ARG;
  if (!seg_offsets || !npos || !ap || (num_records > 0 && (!tp_sorted || !scratch))) return EGTR_E_ARG;
  const hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(oi_ap, dim3((unsigned)num_rel, 2u), dim3(kApThreads), 0, s, tp_sorted, seg_offsets, npos,
                     num_records, num_rel, scratch, ap);
  return egtr_check_launch();
}
