// COCO box-detection AP / AR on the device: pycocotools COCOeval(iouType="bbox") evaluateImg + accumulate, as the
// reference's CocoEvaluator drives it (lib/evaluation/coco_eval.py; evaluate_egtr.py:84-99, train_egtr.py:377-397,
// pretrain_detr.py:150-167).  T = 10 IoU thresholds, A = 4 area ranges, M = 3 maxDets, R = 101 recall thresholds; the
// threshold tables are built by the host (numpy) and passed in as fp64.
//
// coco_match (egtr_coco_match_f32): one workgroup per image.
//   * every detection with a label in [0, K) gets its rank within (image, category): descending score, ties to the lower
//     detection index (the stable sort of evaluateImg); ranks >= maxDets[-1] and labels out of range leave no record;
//   * the categories present in the image (a kept detection or a GT) are compacted; the kept detections are placed in
//     (category, rank) order and the GTs in (category, input order) with exclusive scans over the K categories;
//   * one lane per (category present, t, a): the lane walks its category's detections in rank order and, per detection,
//     its GTs in two passes -- the non-ignored ones, then (only when none matched) the ignored ones.  That is the greedy
//     loop of evaluateImg over GTs sorted stably by gtIg with its `break`, without sorting.  IoU is maskApi bbIou in
//     fp64 on the fp32 xywh of the detection (w = x1 - x0 in fp32), computed on the fly.  Matched flags live in an LDS
//     bitset per (t, a) indexed by the GT's slot (crowd GTs can be matched again); the match and ignore bits of every
//     detection are OR-ed into LDS with 64-bit atomics (bit t * A + a);
//   * npig[K, A]: the non-ignored GTs, added with integer atomics (exact and order-independent).
//   Per detection the kernel writes a record: label (-1 = no record), score, rank, and the match / ignore bit words.
//
// coco_accumulate (egtr_coco_accumulate_f64): once per evaluation, over the records sorted by (category, score
// descending, image, rank).  One workgroup per (category k, area a, maxDet m) computes all T thresholds:
//   * tp / fp prefix counts over the kept records (rank < maxDet), ignored ones included as positions, with a block scan
//     of packed (tp << 32 | fp) words; rc = tp / npig, pr = tp / ((fp + tp) + eps) in fp64;
//   * q[r] = max of pr[j] over the j with rc[j] >= recThrs[r] (the suffix maximum of pr read at searchsorted(rc,
//     recThrs, 'left')): an LDS uint64 atomic max on the bits of the non-negative pr in the bucket of the largest r with
//     recThrs[r] <= rc, then a suffix maximum over the 101 buckets; buckets start at 0, the value of an index past the end;
//   * recall = rc of the last kept record, 0 when there is none; precision and recall stay -1 when npig == 0.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "common.h"

namespace {

typedef unsigned long long u64;

constexpr int kT = 10, kA = 4, kM = 3, kR = 101, kTA = kT * kA;
constexpr int kMaxDet = 1024;
constexpr int kMaxGt = 1024;
constexpr int kMaxCls = 1024;
constexpr int kThreads = 256;

// descending-score order key: larger key = higher score; -0 and +0 are one value (numpy compares them equal).  Not
// order_key.h's score_key: this one has no NaN rule.
__device__ __forceinline__ unsigned coco_score_key(float s) {
  unsigned u = __float_as_uint(s);
  if (u == 0x80000000u) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// in place: a[0, n) -> exclusive prefix sums, a[n] = total (n <= 4 * kThreads); every thread calls it
__device__ void block_exclusive_scan(int* a, int n, int* s_w) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int v[4], sum = 0;
  for (int j = 0; j < 4; ++j) {
    const int i = 4 * tid + j;
    v[j] = i < n ? a[i] : 0;
    sum += v[j];
  }
  int incl = sum;
  for (int off = 1; off < 64; off <<= 1) {
    const int u = __shfl_up(incl, off, 64);
    if (lane >= off) incl += u;
  }
  if (lane == 63) s_w[wave] = incl;
  __syncthreads();
  int base = 0;
  for (int w = 0; w < wave; ++w) base += s_w[w];
  int ex = base + incl - sum;
  for (int j = 0; j < 4; ++j) {
    const int i = 4 * tid + j;
    if (i < n) a[i] = ex;
    ex += v[j];
  }
  if (tid == kThreads - 1) a[n] = base + incl;
  __syncthreads();
}

// maskApi bbIou of one (detection, GT) pair in fp64: xywh boxes, the union of a crowd GT is the detection's area
__device__ __forceinline__ double coco_iou(double dx, double dy, double dw, double dh, double gx, double gy, double gw,
                                          double gh, bool crowd) {
#pragma clang fp contract(off)
  const double da = dw * dh, ga = gw * gh;
  const double w = fmin(dw + dx, gw + gx) - fmax(dx, gx);
  if (w <= 0.0) return 0.0;
  const double h = fmin(dh + dy, gh + gy) - fmax(dy, gy);
  if (h <= 0.0) return 0.0;
  const double i = w * h;
  const double u = crowd ? da : da + ga - i;
  return i / u;
}

struct MatchArgs {
  const float* det_boxes;       // [B, D, 4] xyxy
  const float* det_scores;      // [B, D]
  const int64_t* det_labels;    // [B, D]
  const double* gt_boxes;       // [G, 4] xywh
  const double* gt_area;        // [G]
  const unsigned char* gt_crowd;  // [G]
  const int64_t* gt_labels;     // [G]
  const int64_t* gt_off;        // [B + 1]
  int* rec_label;               // [B, D]
  float* rec_score;             // [B, D]
  int* rec_rank;                // [B, D]
  int64_t* rec_bits;            // [B, D, 2]: match bits, ignore bits
  int* npig;                    // [K, A]
  long long G;
  int D, K, max_det;
  double iou_thr[kT];
  double area_rng[2 * kA];
};

__global__ __launch_bounds__(kThreads) void coco_match(const MatchArgs a) {
#pragma clang fp contract(off)
  __shared__ unsigned s_dkey[kMaxDet];
  __shared__ short s_dlab[kMaxDet], s_drank[kMaxDet], s_dord[kMaxDet];
  __shared__ short s_glab[kMaxGt], s_gidx[kMaxGt], s_gord[kMaxGt];
  __shared__ int s_dst[kMaxCls + 1], s_gst[kMaxCls + 1], s_slot[kMaxCls + 1];
  __shared__ short s_cats[kMaxCls];
  __shared__ unsigned s_gtm[kTA * (kMaxGt / 32)];
  __shared__ u64 s_mb[kMaxDet], s_ib[kMaxDet];
  __shared__ double s_thr[kT], s_rng[2 * kA];
  __shared__ int s_w[kThreads / 64];
  const int b = blockIdx.x, tid = threadIdx.x, D = a.D, K = a.K;

  long long g0 = a.gt_off[b], g1 = a.gt_off[b + 1];
  g0 = g0 < 0 ? 0 : (g0 > a.G ? a.G : g0);
  g1 = g1 < g0 ? g0 : (g1 > a.G ? a.G : g1);
  if (g1 - g0 > kMaxGt) g1 = g0 + kMaxGt;
  const int ng = (int)(g1 - g0);

  for (int i = tid; i < D; i += kThreads) {
    const long long l = a.det_labels[(long long)b * D + i];
    s_dlab[i] = (l >= 0 && l < K) ? (short)l : (short)-1;
    s_dkey[i] = coco_score_key(a.det_scores[(long long)b * D + i]);
    s_mb[i] = 0;
    s_ib[i] = 0;
  }
  for (int i = tid; i < ng; i += kThreads) {
    const long long l = a.gt_labels[g0 + i];
    s_glab[i] = (l >= 0 && l < K) ? (short)l : (short)-1;
  }
  for (int i = tid; i <= K; i += kThreads) {
    s_dst[i] = 0;
    s_gst[i] = 0;
  }
  for (int i = tid; i < kTA * (kMaxGt / 32); i += kThreads) s_gtm[i] = 0;
  if (tid < kT) s_thr[tid] = a.iou_thr[tid];
  if (tid < 2 * kA) s_rng[tid] = a.area_rng[tid];
  __syncthreads();

  // ranks within (image, category) and GT positions within (image, category); per-category counts
  for (int d = tid; d < D; d += kThreads) {
    const int lab = s_dlab[d];
    int r = -1;
    if (lab >= 0) {
      const unsigned key = s_dkey[d];
      r = 0;
      for (int e = 0; e < D; ++e) {
        const unsigned ke = s_dkey[e];
        r += (s_dlab[e] == lab && (ke > key || (ke == key && e < d))) ? 1 : 0;
      }
      if (r >= a.max_det) r = -1;
      if (r >= 0) atomicAdd(&s_dst[lab], 1);
    }
    s_drank[d] = (short)r;
  }
  for (int g = tid; g < ng; g += kThreads) {
    const int lab = s_glab[g];
    int r = 0;
    if (lab >= 0) {
      for (int e = 0; e < g; ++e) r += s_glab[e] == lab ? 1 : 0;
      atomicAdd(&s_gst[lab], 1);
      const double area = a.gt_area[g0 + g];
      const bool crowd = a.gt_crowd[g0 + g] != 0;
      for (int aa = 0; aa < kA; ++aa)
        if (!(crowd || area < s_rng[2 * aa] || area > s_rng[2 * aa + 1])) atomicAdd(&a.npig[lab * kA + aa], 1);
    }
    s_gidx[g] = (short)r;
  }
  __syncthreads();
  for (int c = tid; c < K; c += kThreads) s_slot[c] = (s_dst[c] + s_gst[c]) > 0 ? 1 : 0;
  __syncthreads();
  block_exclusive_scan(s_dst, K, s_w);
  block_exclusive_scan(s_gst, K, s_w);
  block_exclusive_scan(s_slot, K, s_w);
  for (int c = tid; c < K; c += kThreads)
    if (s_slot[c + 1] > s_slot[c]) s_cats[s_slot[c]] = (short)c;
  for (int d = tid; d < D; d += kThreads)
    if (s_drank[d] >= 0) s_dord[s_dst[s_dlab[d]] + s_drank[d]] = (short)d;
  for (int g = tid; g < ng; g += kThreads)
    if (s_glab[g] >= 0) s_gord[s_gst[s_glab[g]] + s_gidx[g]] = (short)g;
  __syncthreads();

  // greedy matching: one lane per (category present, t, a)
  const int n_lanes = s_slot[K] * kTA;
  for (int i = tid; i < n_lanes; i += kThreads) {
    const int slot = i / kTA, ta = i - slot * kTA, t = ta / kA, aa = ta - t * kA;
    const int c = s_cats[slot];
    const int p0 = s_dst[c], p1 = s_dst[c + 1], q0 = s_gst[c], q1 = s_gst[c + 1];
    const double thr = fmin(s_thr[t], 1.0 - 1e-10), lo = s_rng[2 * aa], hi = s_rng[2 * aa + 1];
    unsigned* gtm = s_gtm + ta * (kMaxGt / 32);
    for (int p = p0; p < p1; ++p) {
      const int d = s_dord[p];
      const float* bx = a.det_boxes + ((long long)b * D + d) * 4;
      const float w32 = bx[2] - bx[0], h32 = bx[3] - bx[1];
      const double dx = bx[0], dy = bx[1], dw = w32, dh = h32, darea = dw * dh;
      double best = thr;
      int m = -1;
      bool mig = false;
      for (int pass = 0; pass < 2 && m < 0; ++pass) {
        for (int q = q0; q < q1; ++q) {
          const long long gg = g0 + s_gord[q];
          const bool crowd = a.gt_crowd[gg] != 0;
          const double area = a.gt_area[gg];
          const bool ig = crowd || area < lo || area > hi;
          if (ig != (pass == 1)) continue;
          if (((gtm[q >> 5] >> (q & 31)) & 1u) && !crowd) continue;
          const double* gb = a.gt_boxes + gg * 4;
          const double iou = coco_iou(dx, dy, dw, dh, gb[0], gb[1], gb[2], gb[3], crowd);
          if (iou < best) continue;
          best = iou;
          m = q;
          mig = ig;
        }
      }
      if (m >= 0) {
        atomicOr(&gtm[m >> 5], 1u << (m & 31));
        atomicOr(&s_mb[d], 1ull << ta);
        if (mig) atomicOr(&s_ib[d], 1ull << ta);
      } else if (darea < lo || darea > hi) {
        atomicOr(&s_ib[d], 1ull << ta);
      }
    }
  }
  __syncthreads();

  for (int d = tid; d < D; d += kThreads) {
    const long long o = (long long)b * D + d;
    const int r = s_drank[d];
    a.rec_label[o] = r >= 0 ? (int)s_dlab[d] : -1;
    a.rec_rank[o] = r;
    a.rec_score[o] = a.det_scores[o];
    a.rec_bits[2 * o] = (int64_t)s_mb[d];
    a.rec_bits[2 * o + 1] = (int64_t)s_ib[d];
  }
}

struct AccArgs {
  const int* rank;          // [n] sorted records
  const int64_t* bits;      // [n, 2]
  const int64_t* seg_off;   // [K + 1]
  const int* npig;          // [K, A]
  double* precision;        // [T, R, K, A, M]
  double* recall;           // [T, K, A, M]
  long long n;
  int K;
  int max_dets[kM];
  double rec_thr[kR];
};

__global__ __launch_bounds__(kThreads) void coco_accumulate(const AccArgs a) {
#pragma clang fp contract(off)
  __shared__ u64 s_q[kT][kR];
  __shared__ u64 s_w[kThreads / 64][kT];
  __shared__ double s_thr[kR];
  __shared__ int s_any;
  const int k = blockIdx.x, aa = blockIdx.y, mi = blockIdx.z, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int K = a.K;
  const int npig = a.npig[k * kA + aa];
  if (npig == 0) {
    for (int i = tid; i < kT * kR; i += kThreads) {
      const int t = i / kR, r = i - t * kR;
      a.precision[(((long long)(t * kR + r) * K + k) * kA + aa) * kM + mi] = -1.0;
    }
    if (tid < kT) a.recall[((long long)(tid * K + k) * kA + aa) * kM + mi] = -1.0;
    return;
  }
  for (int i = tid; i < kT * kR; i += kThreads) s_q[i / kR][i % kR] = 0;
  for (int i = tid; i < kR; i += kThreads) s_thr[i] = a.rec_thr[i];
  if (tid == 0) s_any = 0;
  __syncthreads();

  long long s0 = a.seg_off[k], s1 = a.seg_off[k + 1];
  s0 = s0 < 0 ? 0 : (s0 > a.n ? a.n : s0);
  s1 = s1 < s0 ? s0 : (s1 > a.n ? a.n : s1);
  const int max_det = a.max_dets[mi];
  const double np = (double)npig;
  u64 carry[kT];
  for (int t = 0; t < kT; ++t) carry[t] = 0;
  for (long long base = s0; base < s1; base += kThreads) {
    const long long i = base + tid;
    const int rk = i < s1 ? a.rank[i] : -1;
    const bool kept = rk >= 0 && rk < max_det;
    const u64 mb = kept ? (u64)a.bits[2 * i] : 0ull, ib = kept ? (u64)a.bits[2 * i + 1] : 0ull;
    if (kept) s_any = 1;
    u64 v[kT];
    for (int t = 0; t < kT; ++t) {
      const int bit = t * kA + aa;
      const bool ig = (ib >> bit) & 1ull, m = (mb >> bit) & 1ull;
      v[t] = (kept && !ig) ? (m ? (1ull << 32) : 1ull) : 0ull;
      for (int off = 1; off < 64; off <<= 1) {
        const u64 u = __shfl_up(v[t], off, 64);
        if (lane >= off) v[t] += u;
      }
      if (lane == 63) s_w[wave][t] = v[t];
    }
    __syncthreads();
    for (int t = 0; t < kT; ++t) {
      u64 pre = carry[t], tot = carry[t];
      for (int w = 0; w < kThreads / 64; ++w) {
        if (w < wave) pre += s_w[w][t];
        tot += s_w[w][t];
      }
      v[t] += pre;
      carry[t] = tot;
    }
    if (kept) {
      for (int t = 0; t < kT; ++t) {
        const double tp = (double)(v[t] >> 32), fp = (double)(v[t] & 0xffffffffull);
        const double rc = tp / np;
        const double pr = tp / ((fp + tp) + 2.220446049250313e-16);
        int r = (int)(rc * 100.0);
        r = r < 0 ? 0 : (r > kR - 1 ? kR - 1 : r);
        while (r < kR - 1 && s_thr[r + 1] <= rc) ++r;
        while (r > 0 && s_thr[r] > rc) --r;
        atomicMax(&s_q[t][r], (u64)__double_as_longlong(pr));
      }
    }
    __syncthreads();
  }
  if (tid < kT) {
    u64 run = 0;
    for (int r = kR - 1; r >= 0; --r) {
      run = s_q[tid][r] > run ? s_q[tid][r] : run;
      s_q[tid][r] = run;
    }
  }
  __syncthreads();
  for (int i = tid; i < kT * kR; i += kThreads) {
    const int t = i / kR, r = i - t * kR;
    a.precision[(((long long)(t * kR + r) * K + k) * kA + aa) * kM + mi] = __longlong_as_double((long long)s_q[t][r]);
  }
  if (tid < kT)
    a.recall[((long long)(tid * K + k) * kA + aa) * kM + mi] = s_any ? (double)(carry[tid] >> 32) / np : 0.0;
}

}  // namespace

extern "C" int egtr_coco_match_f32(egtr_stream_t stream, const float* det_boxes, const float* det_scores,
                                   const int64_t* det_labels, int batch, int num_det, int num_classes,
                                   const double* gt_boxes, const double* gt_area, const unsigned char* gt_crowd,
                                   const int64_t* gt_labels, const int64_t* gt_offsets, long long num_gt,
                                   const double* iou_thrs, const double* area_rngs, int max_det, int* rec_label,
                                   float* rec_score, int* rec_rank, int64_t* rec_bits, int* npig) {
  if (batch < 0 || num_det < 0 || num_det > kMaxDet || num_classes < 1 || num_classes > kMaxCls || num_gt < 0 ||
      max_det < 1 || !iou_thrs || !area_rngs)
    return EGTR_E_ARG;
  if (batch == 0 || (num_det == 0 && num_gt == 0)) return EGTR_OK;
  if (!gt_offsets || !npig || (num_gt > 0 && (!gt_boxes || !gt_area || !gt_crowd || !gt_labels)) ||
      (num_det > 0 && (!det_boxes || !det_scores || !det_labels || !rec_label || !rec_score || !rec_rank || !rec_bits)))
    return EGTR_E_ARG;
  MatchArgs a;
  a.det_boxes = det_boxes;
  a.det_scores = det_scores;
  a.det_labels = det_labels;
  a.gt_boxes = gt_boxes;
  a.gt_area = gt_area;
  a.gt_crowd = gt_crowd;
  a.gt_labels = gt_labels;
  a.gt_off = gt_offsets;
  a.rec_label = rec_label;
  a.rec_score = rec_score;
  a.rec_rank = rec_rank;
  a.rec_bits = rec_bits;
  a.npig = npig;
  a.G = num_gt;
  a.D = num_det;
  a.K = num_classes;
  a.max_det = max_det;
  for (int t = 0; t < kT; ++t) a.iou_thr[t] = iou_thrs[t];
  for (int i = 0; i < 2 * kA; ++i) a.area_rng[i] = area_rngs[i];
  hipLaunchKernelGGL(coco_match, dim3((unsigned)batch), dim3(kThreads), 0, static_cast<hipStream_t>(stream), a);
  return egtr_check_launch();
}

extern "C" int egtr_coco_accumulate_f64(egtr_stream_t stream, const int* rank_sorted, const int64_t* bits_sorted,
                                        const int64_t* seg_offsets, const int* npig, long long num_records,
                                        int num_classes, const int* max_dets, const double* rec_thrs,
                                        double* precision, double* recall) {
  if (num_records < 0 || num_classes < 1 || num_classes > kMaxCls || !max_dets || !rec_thrs) return EGTR_E_ARG;
  if (!seg_offsets || !npig || !precision || !recall || (num_records > 0 && (!rank_sorted || !bits_sorted)))
    return EGTR_E_ARG;
  AccArgs a;
  a.rank = rank_sorted;
  a.bits = bits_sorted;
  a.seg_off = seg_offsets;
  a.npig = npig;
  a.precision = precision;
  a.recall = recall;
  a.n = num_records;
  a.K = num_classes;
  for (int m = 0; m < kM; ++m) a.max_dets[m] = max_dets[m];
  for (int r = 0; r < kR; ++r) a.rec_thr[r] = rec_thrs[r];
  hipLaunchKernelGGL(coco_accumulate, dim3((unsigned)num_classes, (unsigned)kA, (unsigned)kM), dim3(kThreads), 0,
                     static_cast<hipStream_t>(stream), a);
  return egtr_check_launch();
}
