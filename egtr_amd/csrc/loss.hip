// Relation / connectivity losses of the SGG criterion on the device: loss AND gradient in a handful of
// passes over pred_rel, no host synchronisation, no index lists.
//
// Reference (model/egtr.py:754-923, training mode with rel_sample_negatives / rel_sample_nonmatching and *_largest=True --
// the configuration train_egtr.py uses): per image it permutes pred_rel / target_rel into "matched queries first" order,
// materialises three nonzero() index lists (true relations of the matched block; false candidates of the block; every
// element with an unmatched subject or object: ~2 M x 3 int64), copies counts to the host, runs two topk's over gathered
// scores and a BCE over the concatenated gather.  The result is a MEAN over a SET of elements, so it can be evaluated in
// place:   loss_rel = sum_{selected e} BCE(x_e, t_e * w_a w_b) / #selected,
//   selected = true relations of the block  U  the k1 largest-logit false candidates of the block  U  the k2 largest-logit
//   elements outside the block, k1 = min(80 n_true, n_false), k2 = min(80 n_true, n_outside) (0 when n_true = 0).
// "k largest" is a threshold: a 3-pass radix select (11 + 11 + 10 bits of the order-preserving integer image of the fp32
// logit) finds the k-th largest key exactly; elements above it are selected, elements equal to it take tickets until k
// is reached (ties have equal logits; which of them the reference's topk returns is unspecified too).
// Launches: prep | 3 x (histogram, find) | final (loss terms, dense d loss / d pred_rel, pair flags) | connectivity.
// All counts stay on the device; the only inputs from the host are tensor shapes.
// The passes that read the target are templates on a target accessor, the entry's target_format: dense fp32 [N, N, R] per image
// (the reference's format), one 64-bit word per (subject, object) pair or, for 65 to 256 predicates,
// ceil(R / 64) words per pair.
// Evaluation mode (and training with both sample counts None) selects nothing: BCE over all elements, egtr_relation_loss_all_f32:
// maps | all-elements pass | connectivity | finalize.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "common.h"
#include "rel_sample_key.h"

namespace {

constexpr int kLT = 256;
constexpr int kRowsPerWg = 1;    // query rows (N*R elements each) per workgroup of the histogram / final passes (8 until round 4: 100
                                 // workgroups at B = 4, N = 200 left 60 % of the CUs idle: final pass 391 us, histogram passes 200 us each)
constexpr int kBins = 2048;

// workspace layout per image (ints), see egtr_relation_loss_workspace_bytes()
struct ImgState {
  int T;            // matched pairs
  int n_true, n_false;
  int k[2];         // elements to select: [0] false candidates of the block, [1] outside the block
  int krem[2];      // still to find below the current prefix
  unsigned prefix[2];   // key bits fixed so far (left-aligned)
  unsigned thr[2];  // final threshold key
  int need[2];      // elements equal to thr to take
  int ticket[2];    // tickets handed out to elements equal to thr
  int n_sel;        // n_true + k[0] + k[1]
  int pad[4];       // POL kernels: the random key words (ka, kb) of problem 0, then of problem 1; zero otherwise
};
// sampling policy of a class (policy_neg / policy_nm of egtr_relation_loss_f32): the k largest logits | a uniform k-subset | the whole class
constexpr int kPolLargest = 0, kPolRandom = 1, kPolAll = 2;
static_assert(sizeof(ImgState) == 80, "layout");

__device__ __forceinline__ unsigned key_of(float x) {   // order-preserving: larger float <-> larger unsigned
  const unsigned u = __float_as_uint(x);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ float bce_logits(float x, float y) {   // BCEWithLogitsLoss(reduction="none")
  return fmaxf(x, 0.f) - x * y + log1pf(expf(-fabsf(x)));
}

// ---- target accessors: what the prep / histogram / final passes read the 0 / 1 relation target through -------------------
// image(b) -> pair(row * N + col) -> at(r) = the target of predicate r between target rows `row` and `col`; count_block():
// (number of non-zero targets, number of targets != 1) over the T x T block of matched target rows, this thread's share.
struct DenseTarget {   // DEVICE array of per-image pointers to dense fp32 [N, N, R] tensors (the reference's format)
  const float* const* rel;
  struct Pair {
    const float* p;
    __device__ __forceinline__ float at(int r) const { return p[r]; }
  };
  struct Image {
    const float* p;
    int R;
    __device__ __forceinline__ Pair pair(size_t rc) const { return Pair{p + rc * R}; }
    __device__ __forceinline__ void count_block(const int64_t* tg, int T, int N, int tid, int nthreads, int& nt,
                                                int& nf) const {
      const int tot = T * T * R;
      for (int e = tid; e < tot; e += nthreads) {
        const int a = e / (T * R), rem = e - a * T * R, c = rem / R, r = rem - c * R;
        const float t = p[((size_t)tg[a] * N + (size_t)tg[c]) * R + r];
        nt += (t != 0.f);
        nf += (t != 1.0f);
      }
    }
  };
  __device__ __forceinline__ Image image(int b, int N, int R) const { return Image{rel[b], R}; }
};

struct PackedTarget {   // [B, N, N] 64-bit words, bit r of word (row, col) = the target of predicate r (R <= 64): ONE load per pair
  const unsigned long long* bits;
  struct Pair {
    unsigned long long w;
    __device__ __forceinline__ float at(int r) const { return ((w >> r) & 1ull) ? 1.0f : 0.0f; }
  };
  struct Image {
    const unsigned long long* w;
    int R;
    __device__ __forceinline__ Pair pair(size_t rc) const { return Pair{w[rc]}; }
    __device__ __forceinline__ void count_block(const int64_t* tg, int T, int N, int tid, int nthreads, int& nt,
                                                int& nf) const {
      // popcount over the T x T words, masked to the low R bits; a false candidate is every element that is not true
      const unsigned long long mask = R >= 64 ? ~0ull : ((1ull << R) - 1ull);
      int n = 0;
      for (int e = tid; e < T * T; e += nthreads) {
        const int a = e / T, c = e - a * T;
        n += __popcll(w[(size_t)tg[a] * N + (size_t)tg[c]] & mask);
      }
      nt += n;
      nf += (tid == 0 ? T * T * R : 0) - n;   // summed over the workgroup: T T R - n_true
    }
  };
  __device__ __forceinline__ Image image(int b, int N, int R) const { return Image{bits + (size_t)b * N * N, R}; }
};

struct PackedTargetWide {   // [B, N, N, W] 64-bit words, W = ceil(R / 64): bit r & 63 of word r >> 6 of pair (row, col) = the
  const unsigned long long* bits;   // target of predicate r (R <= 256); bits at positions >= R are zero
  struct Pair {
    const unsigned long long* w;
    __device__ __forceinline__ float at(int r) const { return ((w[r >> 6] >> (r & 63)) & 1ull) ? 1.0f : 0.0f; }   // ONE word
  };
  struct Image {
    const unsigned long long* w;
    int R, W;
    __device__ __forceinline__ Pair pair(size_t rc) const { return Pair{w + rc * W}; }
    __device__ __forceinline__ void count_block(const int64_t* tg, int T, int N, int tid, int nthreads, int& nt,
                                                int& nf) const {
      // popcount over the T x T x W words, the LAST word of a pair masked to its R - 64 (W - 1) valid bits (1 .. 64: no shift by 64)
      const int tail = R - 64 * (W - 1);
      const unsigned long long last = tail >= 64 ? ~0ull : ((1ull << tail) - 1ull);
      int n = 0;
      for (int e = tid; e < T * T * W; e += nthreads) {
        const int pr = e / W, k = e - pr * W, a = pr / T, c = pr - a * T;
        const unsigned long long v = w[((size_t)tg[a] * N + (size_t)tg[c]) * W + k];
        n += __popcll(k == W - 1 ? (v & last) : v);
      }
      nt += n;
      nf += (tid == 0 ? T * T * R : 0) - n;   // summed over the workgroup: T T R - n_true
    }
  };
  __device__ __forceinline__ Image image(int b, int N, int R) const {
    const int W = (R + 63) >> 6;
    return Image{bits + (size_t)b * N * N * W, R, W};
  }
};

constexpr int kPrepT = 1024;   // one workgroup per image, sixteen waves: the T x T x R count below is ~500 dependent gathers per thread with four
// ---- prep: per image  tq (query -> target row), wq (1 - sigmoid(matching cost)), mq (matched), block counts ------------
// The maps of one image, shared by the sampled and the un-sampled route; every thread of the workgroup (kPrepT) calls it and
// gets T back (0 for an image the matcher refused).  Ends on a barrier: tq / wq / mq of the image are complete for the caller.
__device__ __forceinline__ int rel_prep_maps(const int64_t* __restrict__ pred_idx, const int64_t* __restrict__ tgt_idx,
                                             const float* __restrict__ match_cost, const int* __restrict__ out_off, int N,
                                             float nonmatching_cost, int* tq, float* wq, unsigned char* mq) {
  __shared__ int s_scan[kPrepT];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int o0 = out_off[b];
  int T = out_off[b + 1] - o0;
  // The device matcher writes -1 indices for an image whose cost matrix holds NaN / -inf (scipy raises there): such an
  // image is treated as having NO matches here (never an out-of-bounds access); the Python side turns the matcher's
  // status into NaN loss terms for that output set (SceneGraphGenerationLoss.forward) and a ValueError
  // (DeformableDetrHungarianMatcher.raise_if_invalid).
  int bad_local = 0;
  for (int t = tid; t < T; t += kPrepT) {
    const long long q = pred_idx[o0 + t], g = tgt_idx[o0 + t];
    bad_local |= (q < 0 || q >= N || g < 0 || g >= N) ? 1 : 0;
  }
  if (__syncthreads_or(bad_local)) T = 0;
  int* tq_b = tq + (size_t)b * N;
  float* wq_b = wq + (size_t)b * N;
  unsigned char* mq_b = mq + (size_t)b * N;
  for (int q = tid; q < N; q += kPrepT) { mq_b[q] = 0; wq_b[q] = 1.0f - 1.0f / (1.0f + expf(-nonmatching_cost)); }
  __syncthreads();
  for (int t = tid; t < T; t += kPrepT) {
    const int q = (int)pred_idx[o0 + t];
    mq_b[q] = 1;
    tq_b[q] = (int)tgt_idx[o0 + t];
    wq_b[q] = 1.0f - 1.0f / (1.0f + expf(-match_cost[o0 + t]));     // 1 - cost.sigmoid()  (egtr:844, 920)
  }
  __syncthreads();
  // unmatched queries in ascending order take target rows T, T + 1, ... (egtr:761-768)
  int base = 0;
  for (int q0 = 0; q0 < N; q0 += kPrepT) {
    const int q = q0 + tid;
    const int un = (q < N && !mq_b[q]) ? 1 : 0;
    s_scan[tid] = un;
    __syncthreads();
    for (int o = 1; o < kPrepT; o <<= 1) {
      const int v = tid >= o ? s_scan[tid - o] : 0;
      __syncthreads();
      s_scan[tid] += v;
      __syncthreads();
    }
    if (un) tq_b[q] = T + base + s_scan[tid] - 1;
    base += s_scan[kPrepT - 1];
    __syncthreads();
  }
  return T;
}

// POL (a policy other than `largest`): pol0 / pol1 = the policy of the block's false candidates / of the elements outside the block.  A
// class taken whole has k = its size whatever n_true is (the reference skips its sampling block, egtr:848, 878) and nothing to
// select (krem = 0: the histogram / find passes skip it); a random class gets its key words from (seed, stream, image, class).
template <class Tgt, bool POL = false>
__global__ __launch_bounds__(kPrepT) void rel_loss_prep(const int64_t* __restrict__ pred_idx,
                                                     const int64_t* __restrict__ tgt_idx,
                                                     const float* __restrict__ match_cost,
                                                     const int* __restrict__ out_off,
                                                     const Tgt target_rel, int N, int R,
                                                     float nonmatching_cost, int k_neg, int k_nm, ImgState* st,
                                                     int* tq, float* wq, unsigned char* mq, int* total_sel,
                                                     int pol0, int pol1, unsigned seed_lo, unsigned seed_hi,
                                                     unsigned stream_lo, unsigned stream_hi) {
  __shared__ int s_cnt[2];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int o0 = out_off[b];
  if (tid < 2) s_cnt[tid] = 0;
  const int T = rel_prep_maps(pred_idx, tgt_idx, match_cost, out_off, N, nonmatching_cost, tq, wq, mq);
  // counts over the matched block: true = target != 0, false candidates = target != 1 (egtr:838-840)
  int nt = 0, nf = 0;
  target_rel.image(b, N, R).count_block(tgt_idx + o0, T, N, tid, kPrepT, nt, nf);
  for (int o = 32; o > 0; o >>= 1) { nt += __shfl_xor(nt, o); nf += __shfl_xor(nf, o); }
  if ((tid & 63) == 0) { atomicAdd(&s_cnt[0], nt); atomicAdd(&s_cnt[1], nf); }
  __syncthreads();
  if (tid == 0) {
    ImgState s;
    s.T = T;
    s.n_true = s_cnt[0];
    s.n_false = s_cnt[1];
    const long long n_nm = ((long long)N * N - (long long)T * T) * R;
    const long long want0 = (long long)s.n_true * k_neg, want1 = (long long)s.n_true * k_nm;
    s.k[0] = s.n_true > 0 ? (int)(want0 < s.n_false ? want0 : s.n_false) : 0;       // egtr:852-858 min(n_true * k, #cands)
    s.k[1] = s.n_true > 0 ? (int)(want1 < n_nm ? want1 : n_nm) : 0;
    if constexpr (POL) {
      if (pol0 == kPolAll) s.k[0] = s.n_false;
      if (pol1 == kPolAll) s.k[1] = (int)n_nm;   // < 2^31: checked by the entry
    }
    s.krem[0] = s.k[0];
    s.krem[1] = s.k[1];
    if constexpr (POL) {
      if (pol0 == kPolAll) s.krem[0] = 0;
      if (pol1 == kPolAll) s.krem[1] = 0;
    }
    s.prefix[0] = s.prefix[1] = 0u;
    s.thr[0] = s.thr[1] = 0u;
    s.need[0] = s.need[1] = 0;
    s.ticket[0] = s.ticket[1] = 0;
    s.n_sel = s.n_true + s.k[0] + s.k[1];
    s.pad[0] = s.pad[1] = s.pad[2] = s.pad[3] = 0;
    if constexpr (POL) {
      uint32_t w[4];
      if (pol0 == kPolRandom) {
        egtr_philox4x32_10((uint32_t)b, 0u, stream_lo, stream_hi, seed_lo, seed_hi, w);
        s.pad[0] = (int)w[0];
        s.pad[1] = (int)w[1];
      }
      if (pol1 == kPolRandom) {
        egtr_philox4x32_10((uint32_t)b, 1u, stream_lo, stream_hi, seed_lo, seed_hi, w);
        s.pad[2] = (int)w[0];
        s.pad[3] = (int)w[1];
      }
    }
    st[b] = s;
    atomicAdd(total_sel, s.n_sel);
  }
}

// the maps alone: the un-sampled loss (rel_loss_all below) selects nothing, so it needs no block counts and no ImgState
__global__ __launch_bounds__(kPrepT) void rel_all_prep(const int64_t* __restrict__ pred_idx,
                                                       const int64_t* __restrict__ tgt_idx,
                                                       const float* __restrict__ match_cost,
                                                       const int* __restrict__ out_off, int N, float nonmatching_cost,
                                                       int* tq, float* wq, unsigned char* mq) {
  rel_prep_maps(pred_idx, tgt_idx, match_cost, out_off, N, nonmatching_cost, tq, wq, mq);
}

// ---- histogram pass: digit PASS (0: bits 31..21, 1: bits 20..10, 2: bits 9..0) of the candidates under the prefix --------
// POL: a random class ranks its candidates by egtr_rel_sample_key(flat index) instead of key_of(logit); the select is the same.
template <int PASS, class Tgt, bool POL = false>
__global__ __launch_bounds__(kLT) void rel_loss_hist(const float* __restrict__ pred_rel,
                                                     const Tgt target_rel, int N, int R,
                                                     const ImgState* __restrict__ st, const int* __restrict__ tq,
                                                     const unsigned char* __restrict__ mq, unsigned* __restrict__ hist,
                                                     int pol0, int pol1) {
  __shared__ unsigned s_h[2][kBins];
  const int b = blockIdx.y, tid = threadIdx.x;
  const ImgState s = st[b];
  if (s.krem[0] <= 0 && s.krem[1] <= 0) return;      // nothing (left) to select in this image
  for (int i = tid; i < 2 * kBins; i += kLT) (&s_h[0][0])[i] = 0u;
  __syncthreads();
  const int* tq_b = tq + (size_t)b * N;
  const unsigned char* mq_b = mq + (size_t)b * N;
  const typename Tgt::Image rel = target_rel.image(b, N, R);
  const float* pr = pred_rel + (size_t)b * N * N * R;
  const int NR = N * R;
  const float invR = 1.0f / (float)R;
  constexpr int kShift = PASS == 0 ? 21 : (PASS == 1 ? 10 : 0);
  constexpr unsigned kMask = PASS == 2 ? 1023u : 2047u;
  for (int row = 0; row < kRowsPerWg; ++row) {
    const int qa = blockIdx.x * kRowsPerWg + row;
    if (qa >= N) break;
    const bool ma = mq_b[qa] != 0;
    if (!ma && s.krem[1] <= 0) continue;
    const size_t trow = (size_t)tq_b[qa] * N;
    for (int e = tid; e < NR; e += kLT) {
      const int qb = (int)(((float)e + 0.5f) * invR);   // exact: e < 2^22
      const bool blk = ma && mq_b[qb];
      int prob;
      if (blk) {
        if (s.krem[0] <= 0) continue;
        const float t = rel.pair(trow + tq_b[qb]).at(e - qb * R);
        if (!(t != 1.0f)) continue;
        prob = 0;
      } else {
        if (s.krem[1] <= 0) continue;
        prob = 1;
      }
      unsigned key;
      if constexpr (POL) {
        if ((prob ? pol1 : pol0) == kPolRandom)
          key = egtr_rel_sample_key((unsigned)qa * (unsigned)NR + (unsigned)e, (unsigned)(prob ? s.pad[2] : s.pad[0]),
                                    (unsigned)(prob ? s.pad[3] : s.pad[1]));
        else
          key = key_of(pr[(size_t)qa * NR + e]);
      } else {
        key = key_of(pr[(size_t)qa * NR + e]);
      }
      const unsigned pref = prob ? s.prefix[1] : s.prefix[0];   // a select: indexing the local copy by `prob` put it in scratch
      if (PASS == 1 && (key >> 21) != (pref >> 21)) continue;
      if (PASS == 2 && (key >> 10) != (pref >> 10)) continue;
      atomicAdd(&s_h[prob][(key >> kShift) & kMask], 1u);
    }
  }
  __syncthreads();
  unsigned* gh = hist + ((size_t)b * 3 + PASS) * 2 * kBins;
  for (int i = tid; i < 2 * kBins; i += kLT) {
    const unsigned v = (&s_h[0][0])[i];
    if (v) atomicAdd(&gh[i], v);
  }
}

// ---- find: the digit in which the k-th largest candidate lies (one workgroup per (problem, image)) ----------------------
template <int PASS>
__global__ __launch_bounds__(kLT) void rel_loss_find(ImgState* st, const unsigned* __restrict__ hist) {
  __shared__ unsigned s_sum[kLT];
  const int prob = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const int krem = st[b].krem[prob];
  if (krem <= 0) return;
  const unsigned* h = hist + (((size_t)b * 3 + PASS) * 2 + prob) * kBins;
  constexpr int kPer = kBins / kLT;   // 8 bins per thread, thread 0 owns the TOP bins
  unsigned loc[kPer];
  unsigned tot = 0;
#pragma unroll
  for (int i = 0; i < kPer; ++i) {
    loc[i] = h[kBins - 1 - (tid * kPer + i)];
    tot += loc[i];
  }
  s_sum[tid] = tot;
  __syncthreads();
  for (int o = 1; o < kLT; o <<= 1) {
    const unsigned v = tid >= o ? s_sum[tid - o] : 0u;
    __syncthreads();
    s_sum[tid] += v;
    __syncthreads();
  }
  const unsigned before = s_sum[tid] - tot;   // candidates in bins above this thread's range
  if (before < (unsigned)krem && before + tot >= (unsigned)krem) {
    unsigned c = before;
#pragma unroll
    for (int i = 0; i < kPer; ++i) {
      if (c + loc[i] >= (unsigned)krem) {
        const unsigned digit = (unsigned)(kBins - 1 - (tid * kPer + i));
        constexpr int kShift = PASS == 0 ? 21 : (PASS == 1 ? 10 : 0);
        const unsigned pref = st[b].prefix[prob] | (digit << kShift);
        st[b].prefix[prob] = pref;
        st[b].krem[prob] = krem - (int)c;         // still to take among the elements of this digit
        if (PASS == 2) {
          st[b].thr[prob] = pref;
          st[b].need[prob] = krem - (int)c;      // elements equal to the threshold key to take
        }
        break;
      }
      c += loc[i];
    }
  }
}

// ---- deterministic route, tie count: candidates EQUAL to the threshold key per (image, query row, problem) --------------------
// The final pass of that route takes the need[prob] tied candidates with the LOWEST flat index (qa N + qb) R + r: the counts of
// the rows in front of a row are the rank its first tied candidate starts at.  Integer counts: order-free.
// POL: only a `largest` class has ties; a random or whole class counts nothing.
template <class Tgt, bool POL = false>
__global__ __launch_bounds__(kLT) void rel_loss_tie_count(const float* __restrict__ pred_rel, const Tgt target_rel, int N, int R,
                                                          const ImgState* __restrict__ st, const int* __restrict__ tq,
                                                          const unsigned char* __restrict__ mq, int* __restrict__ tiecnt,
                                                          int pol0, int pol1) {
  __shared__ int s_c[2];
  const int b = blockIdx.y, tid = threadIdx.x;
  const ImgState s = st[b];
  const int* tq_b = tq + (size_t)b * N;
  const unsigned char* mq_b = mq + (size_t)b * N;
  const typename Tgt::Image rel = target_rel.image(b, N, R);
  const float* pr = pred_rel + (size_t)b * N * N * R;
  const int NR = N * R;
  const float invR = 1.0f / (float)R;
  for (int row = 0; row < kRowsPerWg; ++row) {
    const int qa = blockIdx.x * kRowsPerWg + row;
    if (qa >= N) break;
    if (tid < 2) s_c[tid] = 0;
    __syncthreads();
    const bool ma = mq_b[qa] != 0;
    const size_t trow = (size_t)tq_b[qa] * N;
    int c0 = 0, c1 = 0;
    for (int e = tid; e < NR; e += kLT) {
      const int qb = (int)(((float)e + 0.5f) * invR);
      const bool blk = ma && mq_b[qb];
      const int prob = blk ? 0 : 1;
      if (s.k[prob] <= 0) continue;
      if constexpr (POL) {
        if ((blk ? pol0 : pol1) != kPolLargest) continue;
      }
      if (blk && !(rel.pair(trow + tq_b[qb]).at(e - qb * R) != 1.0f)) continue;
      const bool tie = key_of(pr[(size_t)qa * NR + e]) == s.thr[prob];
      c0 += (tie && blk) ? 1 : 0;
      c1 += (tie && !blk) ? 1 : 0;
    }
    for (int o = 32; o > 0; o >>= 1) { c0 += __shfl_xor(c0, o); c1 += __shfl_xor(c1, o); }
    if ((tid & 63) == 0) { atomicAdd(&s_c[0], c0); atomicAdd(&s_c[1], c1); }
    __syncthreads();
    if (tid < 2) tiecnt[((size_t)b * N + qa) * 2 + tid] = s_c[tid];
    __syncthreads();
  }
}

// ---- final pass: loss terms, dense gradient, pair flags (target connectivity in query order) ---------------------------
// DET (deterministic route): candidates equal to the threshold key are taken by their rank in flat-index order -- the tied
// candidates of the rows in front (tiecnt), of the earlier kLT-wide steps of this row (a running base: a step covers kLT
// consecutive indices) and of the lower threads of this step (ballot + popcount) -- instead of by ticket; no ticket is drawn.
// POL: per class -- whole: every candidate is taken; random: the candidates whose egtr_rel_sample_key is at least the
// threshold (tie-free: exactly k, no ticket, no tie rank); largest: as without POL.
template <class Tgt, bool DET = false, bool POL = false>
__global__ __launch_bounds__(kLT) void rel_loss_final(const float* __restrict__ pred_rel,
                                                      const Tgt target_rel, int N, int R,
                                                      ImgState* st, const int* __restrict__ tq,
                                                      const float* __restrict__ wq, const unsigned char* __restrict__ mq,
                                                      const int* __restrict__ total_sel, float* __restrict__ grad_rel,
                                                      unsigned char* __restrict__ pairflag, double* __restrict__ partial,
                                                      const int* __restrict__ tiecnt, int pol0, int pol1) {
  __shared__ double s_red[kLT / 64];
  __shared__ int s_wc[DET ? 2 : 1][kLT / 64][2];   // DET: tied candidates per wave of a step, double-buffered
  __shared__ int s_base[2];                        // DET: tied candidates of the rows in front of this one
  const int b = blockIdx.y, tid = threadIdx.x;
  const ImgState s = st[b];
  const int* tq_b = tq + (size_t)b * N;
  const float* wq_b = wq + (size_t)b * N;
  const unsigned char* mq_b = mq + (size_t)b * N;
  const typename Tgt::Image rel = target_rel.image(b, N, R);
  const float* pr = pred_rel + (size_t)b * N * N * R;
  float* gr = grad_rel + (size_t)b * N * N * R;
  unsigned char* pf = pairflag + (size_t)b * N * N;
  const int NR = N * R;
  const float invR = 1.0f / (float)R;
  const float inv_cnt = 1.0f / (float)(*total_sel);    // mean over every selected element of the batch (egtr:814)
  double acc = 0.0;
  for (int row = 0; row < kRowsPerWg; ++row) {
    const int qa = blockIdx.x * kRowsPerWg + row;
    if (qa >= N) break;
    const bool ma = mq_b[qa] != 0;
    const size_t trow = (size_t)tq_b[qa] * N;
    const float wa = wq_b[qa];
    if constexpr (DET) {
      const int lane = tid & 63, wave = tid >> 6;
      if (tid < 2) s_base[tid] = 0;
      __syncthreads();
      int b0 = 0, b1 = 0;
      for (int r = tid; r < qa; r += kLT) {
        b0 += tiecnt[((size_t)b * N + r) * 2 + 0];
        b1 += tiecnt[((size_t)b * N + r) * 2 + 1];
      }
      for (int o = 32; o > 0; o >>= 1) { b0 += __shfl_xor(b0, o); b1 += __shfl_xor(b1, o); }
      if (lane == 0) { atomicAdd(&s_base[0], b0); atomicAdd(&s_base[1], b1); }
      __syncthreads();
      int run0 = s_base[0], run1 = s_base[1];   // rank of the next tied candidate of problem 0 / 1
      int par = 0;
      for (int e0 = 0; e0 < NR; e0 += kLT) {    // every thread takes every step: the barrier below is uniform
        const int e = e0 + tid;
        const bool in = e < NR;
        float t = 0.f, x = 0.f;
        int qb = 0, mult = 0;
        bool blk = false, tie = false;
        if (in) {
          qb = (int)(((float)e + 0.5f) * invR);
          t = rel.pair(trow + tq_b[qb]).at(e - qb * R);
          if (t != 0.f) pf[(size_t)qa * N + qb] = 1;
          blk = ma && mq_b[qb];
          x = pr[(size_t)qa * NR + e];
          const int prob = blk ? 0 : 1;
          if (blk && t != 0.f) mult = 1;
          if ((!blk || t != 1.0f) && s.k[prob] > 0) {
            if constexpr (POL) {
              const int pol = blk ? pol0 : pol1;
              const unsigned thr = blk ? s.thr[0] : s.thr[1];
              if (pol == kPolAll) {
                mult += 1;
              } else if (pol == kPolRandom) {
                const unsigned key = egtr_rel_sample_key((unsigned)qa * (unsigned)NR + (unsigned)e,
                                                         (unsigned)(blk ? s.pad[0] : s.pad[2]),
                                                         (unsigned)(blk ? s.pad[1] : s.pad[3]));
                if (key >= thr) mult += 1;
              } else {
                const unsigned key = key_of(x);
                if (key > thr) mult += 1;
                else tie = key == thr;
              }
            } else {
              const unsigned key = key_of(x);
              if (key > s.thr[prob]) mult += 1;
              else tie = key == s.thr[prob];
            }
          }
        }
        const unsigned long long m0 = __ballot(tie && blk), m1 = __ballot(tie && !blk);
        if (lane == 0) {
          s_wc[par][wave][0] = __popcll(m0);
          s_wc[par][wave][1] = __popcll(m1);
        }
        __syncthreads();
        const unsigned long long below = (1ull << lane) - 1ull;
        int r0 = run0 + __popcll(m0 & below), r1 = run1 + __popcll(m1 & below);
#pragma unroll
        for (int w = 0; w < kLT / 64; ++w) {
          const int c0 = s_wc[par][w][0], c1 = s_wc[par][w][1];
          if (w < wave) { r0 += c0; r1 += c1; }
          run0 += c0;
          run1 += c1;
        }
        par ^= 1;
        if (tie && (blk ? r0 < s.need[0] : r1 < s.need[1])) mult += 1;
        if (in) {
          float g = 0.f;
          if (mult) {
            const float y = t * (wa * wq_b[qb]);
            acc += (double)((float)mult * bce_logits(x, y));
            g = (float)mult * (1.0f / (1.0f + expf(-x)) - y) * inv_cnt;
          }
          gr[(size_t)qa * NR + e] = g;
        }
      }
    } else
    for (int e = tid; e < NR; e += kLT) {
      const int qb = (int)(((float)e + 0.5f) * invR);
      const float t = rel.pair(trow + tq_b[qb]).at(e - qb * R);
      if (t != 0.f) pf[(size_t)qa * N + qb] = 1;      // benign race: every writer stores 1
      const bool blk = ma && mq_b[qb];
      const float x = pr[(size_t)qa * NR + e];
      int mult = 0;
      const int prob = blk ? 0 : 1;
      if (blk && t != 0.f) mult = 1;                   // true relation of the matched block (egtr:838)
      if ((!blk || t != 1.0f) && s.k[prob] > 0) {      // sampled by score (egtr:852-895)
        if constexpr (POL) {
          const int pol = blk ? pol0 : pol1;
          const unsigned thr = blk ? s.thr[0] : s.thr[1];
          if (pol == kPolAll) {
            mult += 1;
          } else if (pol == kPolRandom) {
            const unsigned key = egtr_rel_sample_key((unsigned)qa * (unsigned)NR + (unsigned)e,
                                                     (unsigned)(blk ? s.pad[0] : s.pad[2]),
                                                     (unsigned)(blk ? s.pad[1] : s.pad[3]));
            if (key >= thr) mult += 1;
          } else {
            const unsigned key = key_of(x);
            if (key > thr) mult += 1;
            else if (key == thr && atomicAdd(&st[b].ticket[prob], 1) < (blk ? s.need[0] : s.need[1])) mult += 1;
          }
        } else {
          const unsigned key = key_of(x);
          if (key > s.thr[prob]) mult += 1;
          else if (key == s.thr[prob] && atomicAdd(&st[b].ticket[prob], 1) < s.need[prob]) mult += 1;
        }
      }
      float g = 0.f;
      if (mult) {
        const float y = t * (wa * wq_b[qb]);           // target * weight[a] * weight[b]  (egtr:918-922)
        acc += (double)((float)mult * bce_logits(x, y));
        g = (float)mult * (1.0f / (1.0f + expf(-x)) - y) * inv_cnt;
      }
      gr[(size_t)qa * NR + e] = g;
    }
  }
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
  if ((tid & 63) == 0) s_red[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0) {
    double t = 0.0;
    for (int w = 0; w < kLT / 64; ++w) t += s_red[w];
    partial[(size_t)b * gridDim.x + blockIdx.x] = t;
  }
}

// ---- un-sampled relation loss (egtr:806-829 with both sample counts None: evaluation mode, validation_loss) ----------------
// BCE over ALL N N R elements of an image against y = t(tq[qa], tq[qb], r) * (wq[qa] wq[qb]); the loss is a mean over every
// element, so it is evaluated in query order through the maps of rel_prep_maps: no selection, no counts, no tickets.  One
// workgroup per (image, subject query row): coalesced reads of the row's N R logits, one double partial per row (lanes by
// shuffle tree, waves in index order), pair flags for conn_loss.  GRAD = false (validation runs under no_grad): nothing but the
// partial and the flags is written.  inv_cnt = 1 / (B N N R).
template <class Tgt, bool GRAD>
__global__ __launch_bounds__(kLT) void rel_loss_all(const float* __restrict__ pred_rel, const Tgt target_rel, int N, int R,
                                                    const int* __restrict__ tq, const float* __restrict__ wq, float inv_cnt,
                                                    float* __restrict__ grad_rel, unsigned char* __restrict__ pairflag,
                                                    double* __restrict__ partial) {
  __shared__ double s_red[kLT / 64];
  const int b = blockIdx.y, qa = blockIdx.x, tid = threadIdx.x;
  const int* tq_b = tq + (size_t)b * N;
  const float* wq_b = wq + (size_t)b * N;
  const typename Tgt::Image rel = target_rel.image(b, N, R);
  const int NR = N * R;
  const float* pr = pred_rel + ((size_t)b * N + qa) * NR;
  unsigned char* pf = pairflag + ((size_t)b * N + qa) * N;
  const float invR = 1.0f / (float)R;
  // (a target row is < N for the matcher's one-to-one indices; the min keeps a malformed index list inside the target)
  const size_t trow = (size_t)min(tq_b[qa], N - 1) * N;
  const float wa = wq_b[qa];
  double acc = 0.0;
  for (int e = tid; e < NR; e += kLT) {
    const int qb = (int)(((float)e + 0.5f) * invR);
    const float t = rel.pair(trow + min(tq_b[qb], N - 1)).at(e - qb * R);
    if (t != 0.f) pf[qb] = 1;                          // benign race: every writer stores 1
    const float x = pr[e];
    const float y = t * (wa * wq_b[qb]);               // target * weight[a] * weight[b]  (egtr:826-828)
    acc += (double)bce_logits(x, y);
    if constexpr (GRAD) grad_rel[((size_t)b * N + qa) * NR + e] = (1.0f / (1.0f + expf(-x)) - y) * inv_cnt;
  }
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
  if ((tid & 63) == 0) s_red[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0) {
    double t = 0.0;
    for (int w = 0; w < kLT / 64; ++w) t += s_red[w];
    partial[(size_t)b * N + qa] = t;
  }
}

// one workgroup: both sums in a fixed order -- every thread a contiguous run of partials in index order, lanes by shuffle tree,
// waves in index order -- then the two fp32 means
__global__ __launch_bounds__(kLT) void rel_loss_all_finalize(const double* __restrict__ partial_rel, int n_rel,
                                                             const double* __restrict__ partial_conn, int n_conn,
                                                             double n_elem, double n_pairs, float* __restrict__ loss_out) {
  __shared__ double s_fin[2][kLT / 64];
  const int tid = threadIdx.x;
  const int cr = (n_rel + kLT - 1) / kLT, cc = (n_conn + kLT - 1) / kLT;
  double sr = 0.0, sc = 0.0;
  for (int i = tid * cr; i < min((tid + 1) * cr, n_rel); ++i) sr += partial_rel[i];
  for (int i = tid * cc; i < min((tid + 1) * cc, n_conn); ++i) sc += partial_conn[i];
  for (int o = 32; o > 0; o >>= 1) {
    sr += __shfl_xor(sr, o);
    sc += __shfl_xor(sc, o);
  }
  if ((tid & 63) == 0) {
    s_fin[0][tid >> 6] = sr;
    s_fin[1][tid >> 6] = sc;
  }
  __syncthreads();
  if (tid == 0) {
    double tr = 0.0, tc = 0.0;
    for (int w = 0; w < kLT / 64; ++w) {
      tr += s_fin[0][w];
      tc += s_fin[1][w];
    }
    loss_out[0] = (float)(tr / n_elem);
    loss_out[1] = (float)(tc / n_pairs);
  }
}

// ---- connectivity BCE (egtr:786-793, 815) + final reduction of both losses (last workgroup, fixed order) ----------------
// FINAL = false (the un-sampled route): the partials only, summed by rel_loss_all_finalize -- no ticket, no total_sel;
// GRAD = false: no gradient is written (grad_conn may be NULL).
template <bool FINAL = true, bool GRAD = true>
__global__ __launch_bounds__(kLT) void conn_loss(const float* __restrict__ pred_conn,
                                                 const unsigned char* __restrict__ pairflag, long long n_pairs,
                                                 float* __restrict__ grad_conn, double* __restrict__ partial_conn,
                                                 const double* __restrict__ partial_rel, int n_partial_rel,
                                                 const int* __restrict__ total_sel, unsigned* __restrict__ done,
                                                 float* __restrict__ loss_out) {
  __shared__ double s_red[kLT / 64];
  __shared__ bool s_last;
  const int tid = threadIdx.x;
  const float inv = 1.0f / (float)n_pairs;
  double acc = 0.0;
  for (long long i = (long long)blockIdx.x * kLT + tid; i < n_pairs; i += (long long)gridDim.x * kLT) {
    const float x = pred_conn[i], y = pairflag[i] ? 1.0f : 0.0f;
    acc += (double)bce_logits(x, y);
    if constexpr (GRAD) grad_conn[i] = (1.0f / (1.0f + expf(-x)) - y) * inv;
  }
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
  if ((tid & 63) == 0) s_red[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0) {
    double t = 0.0;
    for (int w = 0; w < kLT / 64; ++w) t += s_red[w];
    partial_conn[blockIdx.x] = t;
    if constexpr (!FINAL) return;
    __threadfence();
    s_last = atomicAdd(done, 1u) == gridDim.x - 1;
  }
  if constexpr (!FINAL) return;
  __syncthreads();
  if (s_last) {
    // The last workgroup sums the partials of both losses -- every thread a fixed strided share, then lanes and waves in a fixed
    // order: bit-reproducible.  (Round 4: thread 0 alone walked the ~1 400 partials with dependent volatile loads: 125 of the
    // launch's 132 us.)
    __shared__ double s_fin[2][kLT / 64];
    __threadfence();
    double sc = 0.0, sr = 0.0;
    const volatile double* pc = partial_conn;   // written by other workgroups of this launch (released above)
    for (unsigned i = tid; i < gridDim.x; i += kLT) sc += pc[i];
    for (int i = tid; i < n_partial_rel; i += kLT) sr += partial_rel[i];
    for (int o = 32; o > 0; o >>= 1) {
      sc += __shfl_xor(sc, o);
      sr += __shfl_xor(sr, o);
    }
    if ((tid & 63) == 0) {
      s_fin[0][tid >> 6] = sc;
      s_fin[1][tid >> 6] = sr;
    }
    __syncthreads();
    if (tid == 0) {
      double tc = 0.0, tr = 0.0;
      for (int w = 0; w < kLT / 64; ++w) {
        tc += s_fin[0][w];
        tr += s_fin[1][w];
      }
      loss_out[0] = (float)(tr / (double)(*total_sel));   // 0 / 0 = NaN: the reference's mean of an empty tensor
      loss_out[1] = (float)(tc / (double)n_pairs);
    }
  }
}

}  // namespace

static long long rel_loss_layout_bytes(int batch, int num_query) {
  if (batch <= 0 || num_query <= 0) return 0;
  const long long B = batch, N = num_query;
  const long long rows = (N + kRowsPerWg - 1) / kRowsPerWg;
  long long bytes = 256;                       // total_sel, done
  bytes += B * (long long)sizeof(ImgState);
  bytes += B * 3 * 2 * kBins * 4;              // histograms
  bytes += B * N * 4 * 2;                      // tq, wq
  bytes += ((B * N + 15) / 16) * 16;           // mq
  bytes += ((B * N * N + 15) / 16) * 16;       // pairflag
  bytes += (B * rows + 1024) * 8;              // partial sums (relations + connectivity)
  return bytes + 256;
}

// the layout, followed by the tie counts int32 [batch, N, 2] of the deterministic tie rule
extern "C" long long egtr_relation_loss_workspace_bytes(int batch, int num_query) {
  const long long base = rel_loss_layout_bytes(batch, num_query);
  if (base <= 0) return 0;
  return ((base + 15) / 16) * 16 + (long long)batch * num_query * 2 * 4;
}

// The launches of the sampled entry.  pred_idx / tgt_idx / match_cost / out_offsets: the matcher's packed outputs
// (egtr_hungarian_match_f32).  workspace: device, egtr_relation_loss_workspace_bytes() bytes, contents irrelevant (zeroed
// here).  loss_out[0] = loss_rel, loss_out[1] = loss_connectivity; grad_rel [B,N,N,R] / grad_conn [B,N,N] = d loss / d logits.
// POL: a policy other than `largest` in either class (pol_neg / pol_nm per class, seed / stream of the random keys); without
// it the kernels carry no policy code.
template <class Tgt, bool POL = false>
static int relation_loss_launch(egtr_stream_t stream, const float* pred_rel, const float* pred_conn, const Tgt target_rel,
                                const int64_t* pred_idx, const int64_t* tgt_idx, const float* match_cost,
                                const int* out_offsets, int batch, int num_query, int num_rel, float nonmatching_cost,
                                int sample_negatives, int sample_nonmatching, float* loss_out, float* grad_rel,
                                float* grad_conn, void* workspace, bool det = false, int pol_neg = kPolLargest,
                                int pol_nm = kPolLargest, long long seed = 0, long long rng_stream = 0) {
  if (!pred_rel || !pred_conn || !pred_idx || !tgt_idx || !match_cost || !out_offsets || !loss_out || !grad_rel ||
      !grad_conn || !workspace)
    return EGTR_E_ARG;
  if (batch <= 0 || num_query <= 0 || num_rel <= 0 || sample_negatives < 0 || sample_nonmatching < 0) return EGTR_E_ARG;
  if ((long long)num_query * num_rel >= (1 << 22) || num_query > 4096) return EGTR_E_UNSUPPORTED;
  bool select = true, ties = det;
  if constexpr (POL) {
    const long long per_image = (long long)num_query * num_query * num_rel;
    const bool any_random = pol_neg == kPolRandom || pol_nm == kPolRandom;
    const bool any_all = pol_neg == kPolAll || pol_nm == kPolAll;
    if (any_random && per_image >= (1ll << 32)) return EGTR_E_UNSUPPORTED;   // the flat index is the 32-bit input of the key
    // a whole class counts every element: the per-image k and the batch's total_sel are 32-bit ints
    if (any_all && per_image * batch >= (1ll << 31)) return EGTR_E_UNSUPPORTED;
    select = pol_neg != kPolAll || pol_nm != kPolAll;                       // a class taken whole needs no select passes
    ties = det && (pol_neg == kPolLargest || pol_nm == kPolLargest);        // ... and only a `largest` class has ties
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  const long long B = batch, N = num_query;
  const int rows = (int)((N + kRowsPerWg - 1) / kRowsPerWg);
  const long long wsb = rel_loss_layout_bytes(batch, num_query);
  const long long wsb_all = det ? egtr_relation_loss_workspace_bytes(batch, num_query) : wsb;   // the tie counts: det only
  if (hipMemsetAsync(workspace, 0, (size_t)wsb_all, st) != hipSuccess) return EGTR_E_LAUNCH;
  int* tiecnt = reinterpret_cast<int*>(static_cast<char*>(workspace) + ((wsb + 15) / 16) * 16);   // det only
  char* p = static_cast<char*>(workspace);
  int* total_sel = reinterpret_cast<int*>(p);
  unsigned* done = reinterpret_cast<unsigned*>(p + 64);
  p += 256;
  ImgState* state = reinterpret_cast<ImgState*>(p);
  p += B * sizeof(ImgState);
  unsigned* hist = reinterpret_cast<unsigned*>(p);
  p += B * 3 * 2 * kBins * 4;
  int* tq = reinterpret_cast<int*>(p);
  p += B * N * 4;
  float* wq = reinterpret_cast<float*>(p);
  p += B * N * 4;
  unsigned char* mq = reinterpret_cast<unsigned char*>(p);
  p += ((B * N + 15) / 16) * 16;
  unsigned char* pairflag = reinterpret_cast<unsigned char*>(p);
  p += ((B * N * N + 15) / 16) * 16;
  p = reinterpret_cast<char*>((reinterpret_cast<uintptr_t>(p) + 7) & ~(uintptr_t)7);
  double* partial_rel = reinterpret_cast<double*>(p);
  double* partial_conn = partial_rel + B * rows;
  const unsigned long long useed = (unsigned long long)seed, ustream = (unsigned long long)rng_stream;
  hipLaunchKernelGGL((rel_loss_prep<Tgt, POL>), dim3(batch), dim3(kPrepT), 0, st, pred_idx, tgt_idx, match_cost, out_offsets,
                     target_rel, num_query, num_rel, nonmatching_cost, sample_negatives, sample_nonmatching, state, tq, wq,
                     mq, total_sel, pol_neg, pol_nm, (unsigned)useed, (unsigned)(useed >> 32), (unsigned)ustream,
                     (unsigned)(ustream >> 32));
  const dim3 gh(rows, batch), gf(2, batch);
  if (select) {
    hipLaunchKernelGGL((rel_loss_hist<0, Tgt, POL>), gh, dim3(kLT), 0, st, pred_rel, target_rel, num_query, num_rel, state, tq,
                       mq, hist, pol_neg, pol_nm);
    hipLaunchKernelGGL(rel_loss_find<0>, gf, dim3(kLT), 0, st, state, hist);
    hipLaunchKernelGGL((rel_loss_hist<1, Tgt, POL>), gh, dim3(kLT), 0, st, pred_rel, target_rel, num_query, num_rel, state, tq,
                       mq, hist, pol_neg, pol_nm);
    hipLaunchKernelGGL(rel_loss_find<1>, gf, dim3(kLT), 0, st, state, hist);
    hipLaunchKernelGGL((rel_loss_hist<2, Tgt, POL>), gh, dim3(kLT), 0, st, pred_rel, target_rel, num_query, num_rel, state, tq,
                       mq, hist, pol_neg, pol_nm);
    hipLaunchKernelGGL(rel_loss_find<2>, gf, dim3(kLT), 0, st, state, hist);
  }
  if (ties) {
    hipLaunchKernelGGL((rel_loss_tie_count<Tgt, POL>), gh, dim3(kLT), 0, st, pred_rel, target_rel, num_query, num_rel, state,
                       tq, mq, tiecnt, pol_neg, pol_nm);
    hipLaunchKernelGGL((rel_loss_final<Tgt, true, POL>), gh, dim3(kLT), 0, st, pred_rel, target_rel, num_query, num_rel, state,
                       tq, wq, mq, total_sel, grad_rel, pairflag, partial_rel, (const int*)tiecnt, pol_neg, pol_nm);
  } else {
    hipLaunchKernelGGL((rel_loss_final<Tgt, false, POL>), gh, dim3(kLT), 0, st, pred_rel, target_rel, num_query, num_rel, state,
                       tq, wq, mq, total_sel, grad_rel, pairflag, partial_rel, (const int*)nullptr, pol_neg, pol_nm);
  }
  const long long n_pairs = B * N * N;
  const int cblocks = (int)std::min<long long>((n_pairs + kLT - 1) / kLT, 1024);
  hipLaunchKernelGGL((conn_loss<true, true>), dim3(cblocks), dim3(kLT), 0, st, pred_conn, pairflag, n_pairs, grad_conn,
                     partial_conn, partial_rel, (int)(B * rows), total_sel, done, loss_out);
  return egtr_check_launch();
}

// ---- the target form of both C entries ----------------------------------------------------------------------------------------
// (target, target_format, num_rel) -> f(the accessor of that form).  The three accessors run the same kernel templates -- the same
// passes, order and arithmetic -- so on the dense form of the same target every format returns the same bits; the packed forms
// load one 8-byte word per (subject, object) pair where the dense accessor gathers one float per logit.
namespace {
constexpr int kWideMaxRel = 256;
inline bool bad_policy(int p) { return p != kPolLargest && p != kPolRandom && p != kPolAll; }

template <class F>
int with_target(const void* target, int target_format, int num_rel, F&& f) {
  if (!target) return EGTR_E_ARG;
  const auto* words = static_cast<const unsigned long long*>(target);
  switch (target_format) {
    case EGTR_REL_TARGET_DENSE: return f(DenseTarget{static_cast<const float* const*>(target)});
    case EGTR_REL_TARGET_WORDS: return num_rel > 64 ? EGTR_E_UNSUPPORTED : f(PackedTarget{words});
    case EGTR_REL_TARGET_WIDE: return num_rel > kWideMaxRel ? EGTR_E_UNSUPPORTED : f(PackedTargetWide{words});
    default: return EGTR_E_ARG;
  }
}
}  // namespace

// One sampling policy per class: policy_neg / policy_nm 0: the `count n_true` largest logits, 1: a uniform
// random subset of that size, 2: the whole class -- its count is ignored; seed / rng_stream: the words of the random keys
// (rel_sample_key.h).  (largest, largest) -- what the criterion trains with -- runs the kernels without the policy code.
// deterministic: among the candidates equal to the threshold key of an (image, problem) of a `largest` class the `need` ones with
// the lowest flat index (qa N + qb) R + r are taken (query order), one extra pass over pred_rel.
extern "C" int egtr_relation_loss_f32(egtr_stream_t stream, const float* pred_rel, const float* pred_conn, const void* target,
                                      int target_format, const int64_t* pred_idx, const int64_t* tgt_idx,
                                      const float* match_cost, const int* out_offsets, int batch, int num_query, int num_rel,
                                      float nonmatching_cost, int sample_negatives, int sample_nonmatching, float* loss_out,
                                      float* grad_rel, float* grad_conn, void* workspace, int policy_neg, int policy_nm,
                                      long long seed, long long rng_stream, int deterministic) {
  if (bad_policy(policy_neg) || bad_policy(policy_nm)) return EGTR_E_ARG;
  const bool det = deterministic != 0;
  return with_target(target, target_format, num_rel, [&](auto tgt) {
    using Tgt = decltype(tgt);
    if (policy_neg != kPolLargest || policy_nm != kPolLargest)
      return relation_loss_launch<Tgt, true>(stream, pred_rel, pred_conn, tgt, pred_idx, tgt_idx, match_cost, out_offsets,
                                             batch, num_query, num_rel, nonmatching_cost, sample_negatives,
                                             sample_nonmatching, loss_out, grad_rel, grad_conn, workspace, det, policy_neg,
                                             policy_nm, seed, rng_stream);
    return relation_loss_launch<Tgt, false>(stream, pred_rel, pred_conn, tgt, pred_idx, tgt_idx, match_cost, out_offsets,
                                            batch, num_query, num_rel, nonmatching_cost, sample_negatives,
                                            sample_nonmatching, loss_out, grad_rel, grad_conn, workspace, det);
  });
}

// ---- the un-sampled entry (evaluation mode / both sample counts None): BCE over every element, see rel_loss_all ------------
// Launches: maps | all-elements pass | connectivity | finalize.  Deterministic by construction (no atomics on values, no tickets).
// workspace layout: tq, wq [B, N] | mq [B N] | pair flags [B N N] | partial sums: B N of the relations, kAllConnBlocks of the connectivity
namespace {
constexpr int kAllConnBlocks = 1024;
}

extern "C" long long egtr_relation_loss_all_workspace_bytes(int batch, int num_query) {
  if (batch <= 0 || num_query <= 0) return 0;
  const long long B = batch, N = num_query;
  long long bytes = B * N * 4 * 2;             // tq, wq
  bytes += ((B * N + 15) / 16) * 16;           // mq
  bytes += ((B * N * N + 15) / 16) * 16;       // pairflag
  bytes += (B * N + kAllConnBlocks) * 8;       // partial sums (relations + connectivity)
  return bytes + 256;
}

template <class Tgt>
static int relation_loss_all_launch(egtr_stream_t stream, const float* pred_rel, const float* pred_conn, const Tgt target_rel,
                                    const int64_t* pred_idx, const int64_t* tgt_idx, const float* match_cost,
                                    const int* out_offsets, int batch, int num_query, int num_rel, float nonmatching_cost,
                                    float* loss_out, float* grad_rel, float* grad_conn, void* workspace) {
  if (!pred_rel || !pred_conn || !pred_idx || !tgt_idx || !match_cost || !out_offsets || !loss_out || !workspace)
    return EGTR_E_ARG;
  if ((grad_rel == nullptr) != (grad_conn == nullptr)) return EGTR_E_ARG;   // value-only: both NULL
  if (batch <= 0 || num_query <= 0 || num_rel <= 0) return EGTR_E_ARG;
  if ((long long)num_query * num_rel >= (1 << 22) || num_query > 4096 || batch > 65535) return EGTR_E_UNSUPPORTED;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const long long B = batch, N = num_query;
  char* p = static_cast<char*>(workspace);
  int* tq = reinterpret_cast<int*>(p);
  p += B * N * 4;
  float* wq = reinterpret_cast<float*>(p);
  p += B * N * 4;
  unsigned char* mq = reinterpret_cast<unsigned char*>(p);
  p += ((B * N + 15) / 16) * 16;
  unsigned char* pairflag = reinterpret_cast<unsigned char*>(p);
  const size_t flag_bytes = (size_t)(((B * N * N + 15) / 16) * 16);
  p += flag_bytes;
  p = reinterpret_cast<char*>((reinterpret_cast<uintptr_t>(p) + 7) & ~(uintptr_t)7);
  double* partial_rel = reinterpret_cast<double*>(p);
  double* partial_conn = partial_rel + B * N;
  if (hipMemsetAsync(pairflag, 0, flag_bytes, st) != hipSuccess) return EGTR_E_LAUNCH;
  hipLaunchKernelGGL(rel_all_prep, dim3(batch), dim3(kPrepT), 0, st, pred_idx, tgt_idx, match_cost, out_offsets, num_query,
                     nonmatching_cost, tq, wq, mq);
  const double n_pairs = (double)(B * N * N), n_elem = n_pairs * (double)num_rel;
  const float inv_cnt = (float)(1.0 / n_elem);
  const dim3 ga(num_query, batch);
  const long long np = B * N * N;
  const int cblocks = (int)std::min<long long>((np + kLT - 1) / kLT, kAllConnBlocks);
  if (grad_rel) {
    hipLaunchKernelGGL((rel_loss_all<Tgt, true>), ga, dim3(kLT), 0, st, pred_rel, target_rel, num_query, num_rel,
                       (const int*)tq, (const float*)wq, inv_cnt, grad_rel, pairflag, partial_rel);
    hipLaunchKernelGGL((conn_loss<false, true>), dim3(cblocks), dim3(kLT), 0, st, pred_conn, pairflag, np, grad_conn,
                       partial_conn, (const double*)nullptr, 0, (const int*)nullptr, (unsigned*)nullptr, (float*)nullptr);
  } else {
    hipLaunchKernelGGL((rel_loss_all<Tgt, false>), ga, dim3(kLT), 0, st, pred_rel, target_rel, num_query, num_rel,
                       (const int*)tq, (const float*)wq, inv_cnt, (float*)nullptr, pairflag, partial_rel);
    hipLaunchKernelGGL((conn_loss<false, false>), dim3(cblocks), dim3(kLT), 0, st, pred_conn, pairflag, np, (float*)nullptr,
                       partial_conn, (const double*)nullptr, 0, (const int*)nullptr, (unsigned*)nullptr, (float*)nullptr);
  }
  hipLaunchKernelGGL(rel_loss_all_finalize, dim3(1), dim3(kLT), 0, st, (const double*)partial_rel, (int)(B * N),
                     (const double*)partial_conn, cblocks, n_elem, n_pairs, loss_out);
  return egtr_check_launch();
}

// The instantiations, in the order their kernels have always had in the code object (the order in which the forms arrived), so
// that the device assembly of two builds can be compared line by line.  A new form or policy template appends its lines.
template decltype(relation_loss_launch<DenseTarget, false>) relation_loss_launch<DenseTarget, false>;
template decltype(relation_loss_launch<PackedTarget, false>) relation_loss_launch<PackedTarget, false>;
template decltype(relation_loss_all_launch<DenseTarget>) relation_loss_all_launch<DenseTarget>;
template decltype(relation_loss_all_launch<PackedTarget>) relation_loss_all_launch<PackedTarget>;
template decltype(relation_loss_launch<PackedTargetWide, false>) relation_loss_launch<PackedTargetWide, false>;
template decltype(relation_loss_all_launch<PackedTargetWide>) relation_loss_all_launch<PackedTargetWide>;
template decltype(relation_loss_launch<DenseTarget, true>) relation_loss_launch<DenseTarget, true>;
template decltype(relation_loss_launch<PackedTarget, true>) relation_loss_launch<PackedTarget, true>;
template decltype(relation_loss_launch<PackedTargetWide, true>) relation_loss_launch<PackedTargetWide, true>;

// The arguments of egtr_relation_loss_f32 without the sample counts and policies.  grad_rel / grad_conn: both device buffers, or
// both NULL for the value alone (nothing of their size is written).
extern "C" int egtr_relation_loss_all_f32(egtr_stream_t stream, const float* pred_rel, const float* pred_conn,
                                          const void* target, int target_format, const int64_t* pred_idx,
                                          const int64_t* tgt_idx, const float* match_cost, const int* out_offsets, int batch,
                                          int num_query, int num_rel, float nonmatching_cost, float* loss_out, float* grad_rel,
                                          float* grad_conn, void* workspace) {
  return with_target(target, target_format, num_rel, [&](auto tgt) {
    return relation_loss_all_launch(stream, pred_rel, pred_conn, tgt, pred_idx, tgt_idx, match_cost, out_offsets, batch,
                                    num_query, num_rel, nonmatching_cost, loss_out, grad_rel, grad_conn, workspace);
  });
}

// ---- detection losses of one output set (labels / boxes / cardinality, egtr:611-659, 661-670, 692-712) ------------------
// The reference evaluates them as ~40 small tensor ops per output set (7 sets with auxiliary losses), plus their autograd
// graph.  One workgroup per image: target-class map in LDS from the matcher's packed indices, sigmoid focal loss + its
// gradient over the [N, C] logits, argmax-based cardinality count, L1 + generalised-IoU loss + gradients of the matched
// boxes.  Sums are formed in a fixed order (per-thread partial -> LDS -> thread 0): bit-reproducible.  The caller divides
// nothing: every sum and every gradient already carries 1 / num_boxes.
namespace {

constexpr int kDT = 1024;   // one workgroup per image: sixteen waves (round 4; four left ~120 dependent iterations per thread)
constexpr int kDetMaxN = 2048;

__device__ __forceinline__ float softplusf(float z) { return fmaxf(z, 0.f) + log1pf(expf(-fabsf(z))); }

// One element of the sigmoid focal loss, gamma = 2 (egtr:647-656, dd:2687-2722): the term of logit x whose target is t, and
// in `grad` its derivative d f / d x (not yet times 1 / num_boxes).  alpha < 0: no alpha weighting.
__device__ __forceinline__ float focal_term(float x, bool t, float alpha, float& grad) {
  const float p = 1.f / (1.f + expf(-x));
  const float ce = softplusf(t ? -x : x);                       // = -log p_t
  const float pt = t ? p : 1.f - p;
  const float om = 1.f - pt;
  const float a = alpha >= 0.f ? (t ? alpha : 1.f - alpha) : 1.f;
  const float g = a * om * om * (2.f * pt * (-ce) - om);         // d f / d x up to the sign of dp_t/dx
  grad = t ? g : -g;
  return a * om * om * ce;
}

// One matched pair, boxes as (cx, cy, w, h) (egtr:692-712, dd util generalized_box_iou): adds |s - t|_1 to l1sum and
// 1 - GIoU(s, t) to gsum; g_l1 / g_giou: their derivatives w.r.t. s, times inv_num_boxes.
__device__ __forceinline__ void box_term(const float4 s, const float4 t, float inv_num_boxes, float& l1sum, float& gsum,
                                         float4& g_l1, float4& g_giou) {
  l1sum += fabsf(s.x - t.x) + fabsf(s.y - t.y) + fabsf(s.z - t.z) + fabsf(s.w - t.w);
  auto sgn = [](float d) { return d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f); };
  g_l1 = make_float4(sgn(s.x - t.x) * inv_num_boxes, sgn(s.y - t.y) * inv_num_boxes, sgn(s.z - t.z) * inv_num_boxes,
                     sgn(s.w - t.w) * inv_num_boxes);
  // corners
  const float x0 = s.x - 0.5f * s.z, y0 = s.y - 0.5f * s.w, x1 = s.x + 0.5f * s.z, y1 = s.y + 0.5f * s.w;
  const float u0 = t.x - 0.5f * t.z, v0 = t.y - 0.5f * t.w, u1 = t.x + 0.5f * t.z, v1 = t.y + 0.5f * t.w;
  const float as = (x1 - x0) * (y1 - y0), at = (u1 - u0) * (v1 - v0);
  const float iwr = fminf(x1, u1) - fmaxf(x0, u0), ihr = fminf(y1, v1) - fmaxf(y0, v0);
  const float iw = fmaxf(iwr, 0.f), ih = fmaxf(ihr, 0.f);
  const float inter = iw * ih, uni = as + at - inter;
  const float ew = fmaxf(fmaxf(x1, u1) - fminf(x0, u0), 0.f), eh = fmaxf(fmaxf(y1, v1) - fminf(y0, v0), 0.f);
  const float ea = ew * eh;
  const float giou = inter / uni - (ea - uni) / ea;
  gsum += 1.f - giou;
  // d(iw) / d(x0, x1), d(ew) / d(x0, x1) and the same for y
  const float iw_x1 = (iwr > 0.f && x1 < u1) ? 1.f : 0.f, iw_x0 = (iwr > 0.f && x0 > u0) ? -1.f : 0.f;
  const float ih_y1 = (ihr > 0.f && y1 < v1) ? 1.f : 0.f, ih_y0 = (ihr > 0.f && y0 > v0) ? -1.f : 0.f;
  const float ew_x1 = x1 > u1 ? 1.f : 0.f, ew_x0 = x0 < u0 ? -1.f : 0.f;
  const float eh_y1 = y1 > v1 ? 1.f : 0.f, eh_y0 = y0 < v0 ? -1.f : 0.f;
  auto dgiou = [&](float d_as, float d_inter, float d_ea) {
    const float d_uni = d_as - d_inter;
    return (d_inter * uni - inter * d_uni) / (uni * uni) + (d_uni * ea - uni * d_ea) / (ea * ea);
  };
  const float g_x0 = dgiou(-(y1 - y0), iw_x0 * ih, ew_x0 * eh), g_x1 = dgiou((y1 - y0), iw_x1 * ih, ew_x1 * eh);
  const float g_y0 = dgiou(-(x1 - x0), iw * ih_y0, ew * eh_y0), g_y1 = dgiou((x1 - x0), iw * ih_y1, ew * eh_y1);
  // loss = 1 - giou; corners -> (cx, cy, w, h)
  g_giou = make_float4(-(g_x0 + g_x1) * inv_num_boxes, -(g_y0 + g_y1) * inv_num_boxes,
                       -0.5f * (g_x1 - g_x0) * inv_num_boxes, -0.5f * (g_y1 - g_y0) * inv_num_boxes);
}

__global__ __launch_bounds__(kDT) void det_loss_f32(
    const float* __restrict__ logits, const float* __restrict__ boxes, const long long* __restrict__ pred_idx,
    const long long* __restrict__ tgt_idx, const int* __restrict__ moff, const long long* __restrict__ tlabels,
    const float* __restrict__ tboxes, const int* __restrict__ toff, int N, int C, float alpha, float inv_num_boxes,
    float* __restrict__ d_logits, float* __restrict__ d_l1, float* __restrict__ d_giou, float* __restrict__ out) {
  __shared__ int s_cls[kDetMaxN];
  __shared__ double s_red[3][kDT / 64];
  __shared__ int s_cnt[kDT / 64];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int m0 = moff[b], m1 = moff[b + 1], t0 = toff[b];
  for (int n = tid; n < N; n += kDT) s_cls[n] = C;                 // "no object" (egtr:640-642)
  for (int e = tid; e < N * 4; e += kDT) {
    d_l1[(size_t)b * N * 4 + e] = 0.f;
    d_giou[(size_t)b * N * 4 + e] = 0.f;
  }
  __syncthreads();
  // invalid entries (-1 from a matcher that refused the image's cost matrix) are skipped, never dereferenced
  const int nt_img = toff[b + 1] - t0;
  for (int k = m0 + tid; k < m1; k += kDT) {
    const long long n = pred_idx[k], g = tgt_idx[k];
    if (n < 0 || n >= N || g < 0 || g >= nt_img) continue;
    const int cls = (int)tlabels[t0 + (int)g];
    s_cls[(int)n] = (cls >= 0 && cls < C) ? cls : C;
  }
  __syncthreads();

  // ---- sigmoid focal loss, gamma = 2 (egtr:647-656, dd:2687-2722) --------------------------------------------------
  float fsum = 0.f;
  const float* lg = logits + (size_t)b * N * C;
  float* dl = d_logits + (size_t)b * N * C;
  for (int e = tid; e < N * C; e += kDT) {
    const int n = e / C, c = e - n * C;
    float g;
    fsum += focal_term(lg[e], s_cls[n] == c, alpha, g);
    dl[e] = g * inv_num_boxes;
  }

  // ---- cardinality (egtr:661-670): rows whose argmax is not the LAST class; first maximum on ties, like torch.argmax ---
  int cnt = 0;
  for (int n = wave; n < N; n += kDT / 64) {
    float best = -INFINITY;
    int bi = C;
    for (int c = lane; c < C; c += 64) {
      const float v = lg[(size_t)n * C + c];
      if (v > best) { best = v; bi = c; }
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const float ov = __shfl_xor(best, o);
      const int oi = __shfl_xor(bi, o);
      if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
    }
    cnt += (bi != C - 1) ? 1 : 0;
  }
  if (lane == 0) s_cnt[wave] = cnt;

  // ---- matched boxes: L1 + generalised IoU (egtr:692-712, dd util generalized_box_iou) -----------------------------------
  float l1sum = 0.f, gsum = 0.f;
  for (int k = m0 + tid; k < m1; k += kDT) {
    if (pred_idx[k] < 0 || pred_idx[k] >= N || tgt_idx[k] < 0 || tgt_idx[k] >= nt_img) continue;
    const int n = (int)pred_idx[k];
    const float4 s = *reinterpret_cast<const float4*>(boxes + ((size_t)b * N + n) * 4);
    const float4 t = *reinterpret_cast<const float4*>(tboxes + (size_t)(t0 + (int)tgt_idx[k]) * 4);
    float4 g_l1, g_giou;
    box_term(s, t, inv_num_boxes, l1sum, gsum, g_l1, g_giou);
    *reinterpret_cast<float4*>(d_l1 + ((size_t)b * N + n) * 4) = g_l1;
    *reinterpret_cast<float4*>(d_giou + ((size_t)b * N + n) * 4) = g_giou;
  }
  // fixed order: the lanes of a wave (butterfly), then the waves in index order
  double fd = (double)fsum, ld = (double)l1sum, gd = (double)gsum;
  for (int o = 32; o > 0; o >>= 1) {
    fd += __shfl_xor(fd, o);
    ld += __shfl_xor(ld, o);
    gd += __shfl_xor(gd, o);
  }
  if (lane == 0) {
    s_red[0][wave] = fd;
    s_red[1][wave] = ld;
    s_red[2][wave] = gd;
  }
  __syncthreads();
  if (tid == 0) {
    double f = 0.0, l = 0.0, g = 0.0;
    for (int i = 0; i < kDT / 64; ++i) { f += s_red[0][i]; l += s_red[1][i]; g += s_red[2][i]; }
    int c = 0;
    for (int w = 0; w < kDT / 64; ++w) c += s_cnt[w];
    out[b * 4 + 0] = (float)(f * inv_num_boxes);
    out[b * 4 + 1] = (float)(l * inv_num_boxes);
    out[b * 4 + 2] = (float)(g * inv_num_boxes);
    out[b * 4 + 3] = (float)c;
  }
}

// ---- the same losses for proposal-sized output sets (two-stage: one proposal per encoder token, N up to 65 536) --------
// Grid (row chunks, B): a workgroup owns kDetLargeRows consecutive query rows of one image and does everything for them --
// their class map in LDS (the image's match list scanned for entries in its range), the box terms of those matches, the
// zero-fill of its rows of the two box gradients, and one wave per row for the focal term, its gradient and the argmax from
// ONE read of the logits.  Every store goes to a row the workgroup owns: no atomics, no workgroup waits for another.  The
// partial sums of a workgroup (three doubles, one int) go to the workspace; det_loss_large_sum adds them per image in a
// fixed order.  kGrad = false: values only, no gradient pointer is touched.
// Every workgroup of an image scans the image's WHOLE match list (196 workgroups over at most 93 entries at the training
// shape): the reads grow as chunks x matches, which is nothing for proposal sets against tens of targets and would want a
// list sorted by query for a set with thousands of matches per image.
// A row without a finite maximum (all -inf, or NaN) keeps the index C and counts as "not the last class", as in det_loss_f32;
// torch.argmax answers 0 there, which differs only at C = 1.
constexpr int kDLT = 256;             // four waves
constexpr int kDetLargeRows = 32;     // rows per workgroup (DETECTION_LOSS_LARGE_ROWS of the binding)
constexpr int kDetLargeMaxN = 65536;  // the large matcher's bound
constexpr int kDetLargeMaxB = 65535;  // grid.y
template <bool kGrad>
__global__ __launch_bounds__(kDLT) void det_loss_large_f32(
    const float* __restrict__ logits, const float* __restrict__ boxes, const long long* __restrict__ pred_idx,
    const long long* __restrict__ tgt_idx, const int* __restrict__ moff, const long long* __restrict__ tlabels,
    const float* __restrict__ tboxes, const int* __restrict__ toff, int N, int C, float alpha, float inv_num_boxes,
    float* __restrict__ d_logits, float* __restrict__ d_l1, float* __restrict__ d_giou, double* __restrict__ ws_sum,
    int* __restrict__ ws_cnt) {
  __shared__ int s_cls[kDetLargeRows];
  __shared__ double s_red[3][kDLT / 64];
  __shared__ int s_cnt[kDLT / 64];
  const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r0 = blockIdx.x * kDetLargeRows, rows = min(kDetLargeRows, N - r0);
  const int m0 = moff[b], m1 = moff[b + 1], t0 = toff[b], nt_img = toff[b + 1] - t0;
  if (tid < rows) {
    s_cls[tid] = C;                                                // "no object" (egtr:640-642)
    if (kGrad) {
      *reinterpret_cast<float4*>(d_l1 + ((size_t)b * N + r0 + tid) * 4) = make_float4(0.f, 0.f, 0.f, 0.f);
      *reinterpret_cast<float4*>(d_giou + ((size_t)b * N + r0 + tid) * 4) = make_float4(0.f, 0.f, 0.f, 0.f);
    }
  }
  __syncthreads();
  // the image's matches that land in this workgroup's rows; invalid entries are skipped, never dereferenced
  float l1sum = 0.f, gsum = 0.f;
  for (int k = m0 + tid; k < m1; k += kDLT) {
    const long long n = pred_idx[k], g = tgt_idx[k];
    if (n < r0 || n >= r0 + rows || g < 0 || g >= nt_img) continue;
    const int cls = tlabels ? (int)tlabels[t0 + (int)g] : 0;      // no labels: class-agnostic targets
    s_cls[(int)n - r0] = (cls >= 0 && cls < C) ? cls : C;
    const float4 s = *reinterpret_cast<const float4*>(boxes + ((size_t)b * N + (int)n) * 4);
    const float4 t = *reinterpret_cast<const float4*>(tboxes + (size_t)(t0 + (int)g) * 4);
    float4 g_l1, g_giou;
    box_term(s, t, inv_num_boxes, l1sum, gsum, g_l1, g_giou);
    if (kGrad) {
      *reinterpret_cast<float4*>(d_l1 + ((size_t)b * N + (int)n) * 4) = g_l1;
      *reinterpret_cast<float4*>(d_giou + ((size_t)b * N + (int)n) * 4) = g_giou;
    }
  }
  __syncthreads();

  // a wave per row: focal term + gradient and the running first maximum of the same element
  float fsum = 0.f;
  int cnt = 0;
  for (int r = wave; r < rows; r += kDLT / 64) {
    const size_t base = ((size_t)b * N + r0 + r) * C;
    const int cls = s_cls[r];
    float best = -INFINITY;
    int bi = C;
    for (int c = lane; c < C; c += 64) {
      const float x = logits[base + c];
      float g;
      fsum += focal_term(x, cls == c, alpha, g);
      if (kGrad) d_logits[base + c] = g * inv_num_boxes;
      if (x > best) { best = x; bi = c; }
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const float ov = __shfl_xor(best, o);
      const int oi = __shfl_xor(bi, o);
      if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
    }
    cnt += (bi != C - 1) ? 1 : 0;
  }
  if (lane == 0) s_cnt[wave] = cnt;
  // fixed order: the lanes of a wave (butterfly), then the waves in index order
  double fd = (double)fsum, ld = (double)l1sum, gd = (double)gsum;
  for (int o = 32; o > 0; o >>= 1) {
    fd += __shfl_xor(fd, o);
    ld += __shfl_xor(ld, o);
    gd += __shfl_xor(gd, o);
  }
  if (lane == 0) {
    s_red[0][wave] = fd;
    s_red[1][wave] = ld;
    s_red[2][wave] = gd;
  }
  __syncthreads();
  if (tid == 0) {
    double f = 0.0, l = 0.0, g = 0.0;
    int c = 0;
    for (int i = 0; i < kDLT / 64; ++i) { f += s_red[0][i]; l += s_red[1][i]; g += s_red[2][i]; c += s_cnt[i]; }
    const size_t w = (size_t)b * gridDim.x + blockIdx.x;
    ws_sum[w * 3 + 0] = f;
    ws_sum[w * 3 + 1] = l;
    ws_sum[w * 3 + 2] = g;
    ws_cnt[w] = c;
  }
}

// one wave per image: lane i adds chunks i, i + 64, ... in that order, then the lanes (butterfly)
__global__ __launch_bounds__(64) void det_loss_large_sum(const double* __restrict__ ws_sum, const int* __restrict__ ws_cnt,
                                                          int chunks, float inv_num_boxes, float* __restrict__ out) {
  const int b = blockIdx.x, lane = threadIdx.x;
  double f = 0.0, l = 0.0, g = 0.0;
  int c = 0;
  for (int i = lane; i < chunks; i += 64) {
    const size_t w = (size_t)b * chunks + i;
    f += ws_sum[w * 3 + 0];
    l += ws_sum[w * 3 + 1];
    g += ws_sum[w * 3 + 2];
    c += ws_cnt[w];
  }
  for (int o = 32; o > 0; o >>= 1) {
    f += __shfl_xor(f, o);
    l += __shfl_xor(l, o);
    g += __shfl_xor(g, o);
    c += __shfl_xor(c, o);
  }
  if (lane == 0) {
    out[b * 4 + 0] = (float)(f * inv_num_boxes);
    out[b * 4 + 1] = (float)(l * inv_num_boxes);
    out[b * 4 + 2] = (float)(g * inv_num_boxes);
    out[b * 4 + 3] = (float)c;
  }
}

inline bool det_large_served(int batch, int num_query, int num_classes) {
  return batch >= 1 && batch <= kDetLargeMaxB && num_query >= 1 && num_query <= kDetLargeMaxN && num_classes >= 1 &&
         (long long)num_query * num_classes < (1LL << 31);
}

}  // namespace

extern "C" long long egtr_detection_loss_large_workspace_bytes(int batch, int num_query, int num_classes) {
  if (!det_large_served(batch, num_query, num_classes)) return 0;
  const long long chunks = (num_query + kDetLargeRows - 1) / kDetLargeRows;
  return (long long)batch * chunks * (3 * (long long)sizeof(double) + (long long)sizeof(int));
}

extern "C" int egtr_detection_loss_large_f32(egtr_stream_t stream, const float* logits, const float* pred_boxes,
                                             const int64_t* pred_idx, const int64_t* tgt_idx, const int* match_offsets,
                                             const int64_t* target_labels, const float* target_boxes,
                                             const int* target_offsets, int batch, int num_query, int num_classes,
                                             float focal_alpha, float num_boxes, float* grad_logits,
                                             float* grad_boxes_l1, float* grad_boxes_giou, float* out, void* workspace) {
  if (!logits || !pred_boxes || !pred_idx || !tgt_idx || !match_offsets || !target_boxes || !target_offsets || !out ||
      !workspace)
    return EGTR_E_ARG;
  const int n_grad = (grad_logits ? 1 : 0) + (grad_boxes_l1 ? 1 : 0) + (grad_boxes_giou ? 1 : 0);
  if (n_grad != 0 && n_grad != 3) return EGTR_E_ARG;
  if (batch <= 0 || num_query <= 0 || num_classes <= 0 || !(num_boxes > 0.f)) return EGTR_E_ARG;
  if (!det_large_served(batch, num_query, num_classes)) return EGTR_E_UNSUPPORTED;
  const int chunks = (num_query + kDetLargeRows - 1) / kDetLargeRows;
  double* ws_sum = static_cast<double*>(workspace);
  int* ws_cnt = reinterpret_cast<int*>(ws_sum + (size_t)batch * chunks * 3);
  const dim3 grid(chunks, batch);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const long long* pi = reinterpret_cast<const long long*>(pred_idx);
  const long long* ti = reinterpret_cast<const long long*>(tgt_idx);
  const long long* tl = reinterpret_cast<const long long*>(target_labels);
  if (n_grad)
    hipLaunchKernelGGL(det_loss_large_f32<true>, grid, dim3(kDLT), 0, s, logits, pred_boxes, pi, ti, match_offsets, tl,
                       target_boxes, target_offsets, num_query, num_classes, focal_alpha, 1.0f / num_boxes, grad_logits,
                       grad_boxes_l1, grad_boxes_giou, ws_sum, ws_cnt);
  else
    hipLaunchKernelGGL(det_loss_large_f32<false>, grid, dim3(kDLT), 0, s, logits, pred_boxes, pi, ti, match_offsets, tl,
                       target_boxes, target_offsets, num_query, num_classes, focal_alpha, 1.0f / num_boxes, grad_logits,
                       grad_boxes_l1, grad_boxes_giou, ws_sum, ws_cnt);
  int st = egtr_check_launch();
  if (st != 0) return st;
  hipLaunchKernelGGL(det_loss_large_sum, dim3(batch), dim3(64), 0, s, ws_sum, ws_cnt, chunks, 1.0f / num_boxes, out);
  return egtr_check_launch();
}

extern "C" int egtr_detection_loss_f32(egtr_stream_t stream, const float* logits, const float* pred_boxes,
                                       const int64_t* pred_idx, const int64_t* tgt_idx, const int* match_offsets,
                                       const int64_t* target_labels, const float* target_boxes,
                                       const int* target_offsets, int batch, int num_query, int num_classes,
                                       float focal_alpha, float num_boxes, float* grad_logits, float* grad_boxes_l1,
                                       float* grad_boxes_giou, float* out) {
  if (!logits || !pred_boxes || !pred_idx || !tgt_idx || !match_offsets || !target_labels || !target_boxes ||
      !target_offsets || !grad_logits || !grad_boxes_l1 || !grad_boxes_giou || !out)
    return EGTR_E_ARG;
  if (batch <= 0 || num_query <= 0 || num_classes <= 0 || !(num_boxes > 0.f)) return EGTR_E_ARG;
  if (num_query > kDetMaxN) return EGTR_E_UNSUPPORTED;
  hipLaunchKernelGGL(det_loss_f32, dim3(batch), dim3(kDT), 0, static_cast<hipStream_t>(stream), logits, pred_boxes,
                     reinterpret_cast<const long long*>(pred_idx), reinterpret_cast<const long long*>(tgt_idx),
                     match_offsets, reinterpret_cast<const long long*>(target_labels), target_boxes, target_offsets,
                     num_query, num_classes, focal_alpha, 1.0f / num_boxes, grad_logits, grad_boxes_l1,
                     grad_boxes_giou, out);
  return egtr_check_launch();
}
