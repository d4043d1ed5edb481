// The candidate builder of the PredCls / SGCls protocols: the K best relation entries over the MATCHED queries of an image,
// in a defined order, in one pass over pred_rel -- no [M, M, R] score tensor, no sort of the whole domain.
//
// Domain of image b: every (s, o, p) -- (s, o) in mode 1 -- of GT-object indices with s != o, query_of[b, s] >= 0 and
// query_of[b, o] >= 0.  With qs = query_of[b, s], qo = query_of[b, o]:
//   r     = clamp(pred_rel[b, qs, qo, p], 0, 1) [* clamp(pred_conn[b, qs, qo], 0, 1)]
//   so    = obj_score[b, s] * obj_score[b, o]
//   score = r * so (mode 0),  max_p(r) * so (mode 1; a NaN in the row gives NaN, like torch.max)
// Order: descending score_key(score) (order_key.h: NaN last, -0 = +0), ties by ascending (s, o, p).  Every entry gets the
// 64-bit ORDER WORD  c = score_key << 32 | (2^32 - 1 - flat),  flat = (s * Gp + o) * R + p  (s * Gp + o in mode 1): the
// order is descending c, the words of an image are pairwise distinct, and ascending flat is ascending (s, o, p) whatever
// Gp is.  The launcher requires Gp * Gp * R < 2^31.
//
// Two launches, select-then-sort in both:
//   mtk_slice  grid (W, B).  The Gp x Gp pairs of an image are cut into W <= 256 contiguous slices.  A WAVE owns a pair:
//              lanes walk the pair's R predicates (one coalesced row of pred_rel), so nothing is divided per entry.  The
//              workgroup finds the K-th largest order word of its slice with the radix select of topk_select.h (one pass
//              over the slice per digit, recomputing the scores from global memory, which L2 serves after the first
//              pass) and then writes the <= K words >= the threshold to the workspace, unsorted.
//   mtk_merge  grid (B).  The same select over the <= W * K surviving words of the image, a bitonic sort of the <= K
//              winners in LDS, and the outputs: a wave per rank decodes flat, reads the entry's row again and writes
//              indices, r (mode 1: the pair's whole r row) and score; ranks from count to K get index Gp - 1 and score 0.
// The K best of the union of the slices' K best are the K best of the image, because the order is total.
// LDS atomics on integers only, plain vector stores, no host synchronisation.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "common.h"
#include "order_key.h"
#include "topk_select.h"

namespace {

constexpr int kThreads = 512;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxK = 1024;        // _MAX_CAND
constexpr int kMaxRel = 256;
constexpr int kMaxSlices = 256;
constexpr int kSlicePairs = 128;   // (s, o) pairs per slice until kMaxSlices caps the count

struct Args {
  const float* rel;       // [B, N, N, R]
  const float* conn;      // [B, N, N] or NULL
  const int* query_of;    // [B, Gp]
  const float* obj;       // [B, Gp]
  int64_t* inds;          // [B, K, 3 | 2]
  float* rel_scores;      // [B, K] | [B, K, R]
  float* trip;            // [B, K]
  int* count;             // [B]
  unsigned long long* ws_items;   // [B, W, K] order words
  int* ws_count;                  // [B, W]
  int N, R, Gp, K, mode, W;
  long long slice_pairs;
};

__device__ __forceinline__ float clamp01(float x) { return x < 0.f ? 0.f : (x > 1.f ? 1.f : x); }   // keeps NaN

// max that keeps a NaN (torch.max over a dimension)
__device__ __forceinline__ float nan_max(float a, float b) { return a != a ? a : ((b != b || b > a) ? b : a); }

__device__ __forceinline__ float wave_nan_max(float m) {
  for (int off = 32; off > 0; off >>= 1) m = nan_max(m, __shfl_xor(m, off));
  return m;
}

__device__ __forceinline__ unsigned long long order_word(float score, unsigned flat) {
  return ((unsigned long long)score_key(score) << 32) | (unsigned long long)(0xffffffffu - flat);
}

// The entries of the pairs [p0, p1) of image b: calls f(order word) once per entry, from the lane that computed it.
struct SliceSource {
  const Args& a;
  int b;
  long long p0, p1;

  template <class F>
  __device__ __forceinline__ void operator()(F&& f) const {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int N = a.N, R = a.R, Gp = a.Gp;
    const int* qof = a.query_of + (long long)b * Gp;
    const float* obj = a.obj + (long long)b * Gp;
    for (long long pr = p0 + wave; pr < p1; pr += kWaves) {   // wave-uniform
      const int s = (int)(pr / Gp), o = (int)(pr - (long long)s * Gp);
      if (s == o) continue;
      const int qs = qof[s], qo = qof[o];
      if (qs < 0 || qs >= N || qo < 0 || qo >= N) continue;
      const float so = obj[s] * obj[o];
      const long long cell = ((long long)b * N + qs) * N + qo;
      const float* row = a.rel + cell * R;
      const bool has_conn = a.conn != nullptr;
      const float cn = has_conn ? clamp01(a.conn[cell]) : 1.f;
      if (a.mode == 0) {
        for (int p = lane; p < R; p += 64) {
          float r = clamp01(row[p]);
          if (has_conn) r = r * cn;
          f(order_word(r * so, (unsigned)(pr * R + p)));
        }
      } else {
        float m = -1.f;
        for (int p = lane; p < R; p += 64) {
          float r = clamp01(row[p]);
          if (has_conn) r = r * cn;
          m = nan_max(m, r);
        }
        m = wave_nan_max(m);
        if (lane == 0) f(order_word(m * so, (unsigned)pr));
      }
    }
  }
};

// The order words the slices of image b left in the workspace.
struct WorkspaceSource {
  const unsigned long long* items;   // [W, K]
  const int* s_wcnt;                 // LDS [W]
  int W, K;

  template <class F>
  __device__ __forceinline__ void operator()(F&& f) const {
    const int total = W * K;
    for (int i = threadIdx.x; i < total; i += kThreads) {
      const int w = i / K;
      if (i - w * K < s_wcnt[w]) f(items[i]);
    }
  }
};

__global__ __launch_bounds__(kThreads) void mtk_slice(const Args a) {
  __shared__ TopkScratch<kThreads> s_sel;
  const int w = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const long long pairs = (long long)a.Gp * a.Gp;
  long long p0 = (long long)w * a.slice_pairs, p1 = p0 + a.slice_pairs;
  if (p0 > pairs) p0 = pairs;
  if (p1 > pairs) p1 = pairs;
  const SliceSource src{a, b, p0, p1};
  const int K = a.K;
  const unsigned long long thr = egtr_select_threshold(src, K, s_sel);
  const int n = egtr_compact_ge(src, thr, K, a.ws_items + ((long long)b * a.W + w) * K, &s_sel.cnt);
  if (tid == 0) a.ws_count[(long long)b * a.W + w] = n;
}

__global__ __launch_bounds__(kThreads) void mtk_merge(const Args a) {
  __shared__ TopkScratch<kThreads> s_sel;
  __shared__ unsigned long long s_top[kMaxK];
  __shared__ int s_wcnt[kMaxSlices];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int K = a.K, R = a.R, Gp = a.Gp, N = a.N, W = a.W;
  for (int i = tid; i < W; i += kThreads) {
    const int c = a.ws_count[(long long)b * W + i];
    s_wcnt[i] = c < 0 ? 0 : (c > K ? K : c);
  }
  __syncthreads();
  const WorkspaceSource src{a.ws_items + (long long)b * W * K, s_wcnt, W, K};
  const unsigned long long thr = egtr_select_threshold(src, K, s_sel);
  const int n = egtr_compact_ge(src, thr, K, s_top, &s_sel.cnt);
  egtr_bitonic_sort_desc<kThreads>(s_top, n);         // pads with 0: below every real word (flat < 2^31)

  const int cols = a.mode == 0 ? 3 : 2;
  const int* qof = a.query_of + (long long)b * Gp;
  const float* obj = a.obj + (long long)b * Gp;
  for (int rank = wave; rank < K; rank += kWaves) {    // wave-uniform
    const long long orow = (long long)b * K + rank;
    bool real = rank < n;
    int s = 0, o = 0, p = 0, qs = 0, qo = 0;
    if (real) {
      const unsigned flat = 0xffffffffu - (unsigned)(s_top[rank] & 0xffffffffull);
      unsigned pr = flat;
      if (a.mode == 0) {
        pr = flat / (unsigned)R;
        p = (int)(flat - pr * (unsigned)R);
      }
      s = (int)(pr / (unsigned)Gp);
      o = (int)(pr - (unsigned)s * (unsigned)Gp);
      real = s < Gp;                                   // holds for every word a slice wrote
      if (real) {
        qs = qof[s];
        qo = qof[o];
        real = qs >= 0 && qs < N && qo >= 0 && qo < N;
      }
    }
    if (!real) {
      if (lane < cols) a.inds[orow * cols + lane] = Gp - 1;
      if (lane == 0) a.trip[orow] = 0.f;
      if (a.mode == 0) {
        if (lane == 0) a.rel_scores[orow] = 0.f;
      } else {
        for (int q = lane; q < R; q += 64) a.rel_scores[orow * R + q] = 0.f;
      }
      continue;
    }
    const float so = obj[s] * obj[o];
    const long long cell = ((long long)b * N + qs) * N + qo;
    const float* row = a.rel + cell * R;
    const bool has_conn = a.conn != nullptr;
    const float cn = has_conn ? clamp01(a.conn[cell]) : 1.f;
    if (a.mode == 0) {
      if (lane == 0) {
        float r = clamp01(row[p]);
        if (has_conn) r = r * cn;
        a.inds[orow * 3 + 0] = s;
        a.inds[orow * 3 + 1] = o;
        a.inds[orow * 3 + 2] = p;
        a.rel_scores[orow] = r;
        a.trip[orow] = r * so;
      }
    } else {
      float m = -1.f;
      for (int q = lane; q < R; q += 64) {
        float r = clamp01(row[q]);
        if (has_conn) r = r * cn;
        a.rel_scores[orow * R + q] = r;
        m = nan_max(m, r);
      }
      m = wave_nan_max(m);
      if (lane == 0) {
        a.inds[orow * 2 + 0] = s;
        a.inds[orow * 2 + 1] = o;
        a.trip[orow] = m * so;
      }
    }
  }
  if (tid == 0) a.count[b] = n;
}

int slices_of(int Gp) {
  const long long pairs = (long long)Gp * Gp;
  const long long w = (pairs + kSlicePairs - 1) / kSlicePairs;
  return (int)(w < 1 ? 1 : (w > kMaxSlices ? kMaxSlices : w));
}

}  // namespace

extern "C" long long egtr_matched_topk_workspace_bytes(int batch, int num_gt_padded, int num_cand) {
  if (batch < 0 || num_gt_padded < 1 || num_cand < 1 || num_cand > kMaxK) return -1;
  const long long slots = (long long)batch * slices_of(num_gt_padded);
  return slots * num_cand * 8 + ((slots * 4 + 7) / 8) * 8;
}

extern "C" int egtr_matched_topk_f32(egtr_stream_t stream, const float* pred_rel, const float* pred_conn,
                                     const int* query_of, const float* obj_score, int batch, int num_query, int num_rel,
                                     int num_gt_padded, int num_cand, int mode, void* workspace, int64_t* inds,
                                     float* rel_scores, float* triplet_scores, int* count) {
  if (batch < 0 || num_query < 1 || num_rel < 1 || num_rel > kMaxRel || num_gt_padded < 1 || num_cand < 1 ||
      num_cand > kMaxK || (mode != 0 && mode != 1))
    return EGTR_E_ARG;
  if (!pred_rel || !query_of || !obj_score || !workspace || !inds || !rel_scores || !triplet_scores || !count)
    return EGTR_E_ARG;
  if (batch == 0) return EGTR_OK;
  if ((long long)num_gt_padded * num_gt_padded * num_rel >= (1ll << 31) || batch > 65535) return EGTR_E_UNSUPPORTED;

  Args a;
  a.rel = pred_rel;
  a.conn = pred_conn;
  a.query_of = query_of;
  a.obj = obj_score;
  a.inds = inds;
  a.rel_scores = rel_scores;
  a.trip = triplet_scores;
  a.count = count;
  a.N = num_query;
  a.R = num_rel;
  a.Gp = num_gt_padded;
  a.K = num_cand;
  a.mode = mode;
  a.W = slices_of(num_gt_padded);
  const long long pairs = (long long)num_gt_padded * num_gt_padded;
  a.slice_pairs = (pairs + a.W - 1) / a.W;
  a.ws_items = static_cast<unsigned long long*>(workspace);
  a.ws_count = reinterpret_cast<int*>(a.ws_items + (long long)batch * a.W * num_cand);

  const hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(mtk_slice, dim3((unsigned)a.W, (unsigned)batch), dim3(kThreads), 0, s, a);
  const int st = egtr_check_launch();
  if (st != EGTR_OK) return st;
  hipLaunchKernelGGL(mtk_merge, dim3((unsigned)batch), dim3(kThreads), 0, s, a);
  return egtr_check_launch();
}
