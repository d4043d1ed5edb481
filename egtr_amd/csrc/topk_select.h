// The workgroup top-K of the evaluators that rank by a 64-bit key (matched_topk.hip, oi_eval.hip): the threshold such that
// exactly min(K, n) of n DISTINCT keys are >= it (radix select), the compaction of the keys >= the threshold into a list,
// and a descending bitonic sort of a list in LDS.  A larger key ranks earlier.
//
// The keys come from a SOURCE: a functor `src(f)` that, called by every thread of the workgroup, calls f(key) once per
// present key, from whichever thread holds it.  The select and the compaction walk the same source, so what a source
// skips is in neither.
//
// The select is templated on the workgroup's thread count NT (whole waves, 2048 % NT == 0).  matched_topk.hip is its one
// user, at NT = 512, so the 256- and 1024-thread paths (8 and 2 bins per thread) are not compiled into the library today;
// Open Images keeps its own 8-bit select (oi_eval.hip).  No harness of its own: the matched top-K tests put
// the K-th rank on a digit boundary, on a bucket boundary and past the last entry; the Open Images selection tests (ties
// across rank topk, adjacent floats, fewer and exactly topk survivors, two partial lists) run the compaction at 256 and
// 1024 threads and the sort at 1024.
#pragma once

#include <hip/hip_runtime.h>

constexpr int kTopkBins = 2048;   // 11-bit digits

template <int NT>
struct TopkScratch {   // LDS of one workgroup
  static_assert(NT % 64 == 0 && kTopkBins % NT == 0, "whole waves, whole bins per thread");
  unsigned hist[kTopkBins];
  unsigned wave_sum[NT / 64];
  unsigned long long prefix;
  int krem;
  int done;   // 1: the bucket of the last digit is taken whole; 2: fewer than K keys, all are taken
  int cnt;    // the compaction's counter
};

// Radix select, all threads of the workgroup: the threshold t such that exactly min(K, #keys) keys of `src` are >= t (0 when
// there are fewer than K).  Digit `pass` of a key: passes 0..2 are bits 63..53, 52..42, 41..32, passes 3..5 the same split
// of the low half; one walk over the source per digit, into an LDS histogram.  Thread t owns NT-th of the bins; a wave
// suffix scan plus the totals of the higher waves tell it how many keys lie in the bins above its own.  The search stops
// at the first digit whose bucket is taken whole -- with a score in the high half and an index in the low half, after the
// three score digits unless scores tie across the K-th rank.
template <int NT, class Src>
__device__ unsigned long long egtr_select_threshold(const Src& src, int K, TopkScratch<NT>& st) {
  constexpr int kPer = kTopkBins / NT;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid == 0) {
    st.prefix = 0ull;
    st.krem = K;
    st.done = 0;
  }
  __syncthreads();
  for (int pass = 0; pass < 6; ++pass) {
    const int sub = pass % 3;
    const int shift = (pass < 3 ? 32 : 0) + (sub == 0 ? 21 : (sub == 1 ? 10 : 0));
    const int width = sub == 2 ? 10 : 11;
    const unsigned mask = (1u << width) - 1u;
    const int hi = shift + width;                      // the bits above the digit; 64 on pass 0
    for (int i = tid; i < kTopkBins; i += NT) st.hist[i] = 0u;
    __syncthreads();
    const unsigned long long prefix = st.prefix;
    const unsigned krem = (unsigned)st.krem;
    src([&](unsigned long long c) {
      if (hi == 64 || (c >> hi) == (prefix >> hi)) atomicAdd(&st.hist[(unsigned)(c >> shift) & mask], 1u);
    });
    __syncthreads();
    unsigned part = 0;                                 // thread t owns bins [t * kPer, (t + 1) * kPer)
    for (int j = 0; j < kPer; ++j) part += st.hist[tid * kPer + j];
    unsigned suf = part;                               // keys in the bins of this and the higher lanes of the wave
    for (int off = 1; off < 64; off <<= 1) {
      const unsigned v = __shfl_down(suf, off, 64);
      if (lane + off < 64) suf += v;
    }
    if (lane == 0) st.wave_sum[wave] = suf;
    __syncthreads();
    unsigned above = suf - part;                       // keys in the bins of higher threads
    for (int w = wave + 1; w < NT / 64; ++w) above += st.wave_sum[w];
    if (tid == 0 && above + part < krem) st.done = 2;
    if (above < krem && krem <= above + part) {        // one thread: the bin of the krem-th largest is among its bins
      unsigned acc = above;
      for (int j = kPer - 1; j >= 0; --j) {
        const unsigned h = st.hist[tid * kPer + j];
        if (krem <= acc + h) {
          st.prefix = prefix | ((unsigned long long)(tid * kPer + j) << shift);
          st.krem = (int)(krem - acc);
          if (acc + h == krem) st.done = 1;
          break;
        }
        acc += h;
      }
    }
    __syncthreads();
    if (st.done) break;                                // uniform: read after the barrier
  }
  const unsigned long long thr = st.done == 2 ? 0ull : st.prefix;
  __syncthreads();                                     // st may be reused
  return thr;
}

// All threads: append every key of `src` that is >= thr to dst (global or LDS, room for cap keys) in no particular order;
// returns how many, at most cap.  With the threshold of a select of cap keys over the same source the count never exceeds
// cap.  s_cnt: one int of LDS.
template <class Src>
__device__ int egtr_compact_ge(const Src& src, unsigned long long thr, int cap, unsigned long long* dst, int* s_cnt) {
  if (threadIdx.x == 0) *s_cnt = 0;
  __syncthreads();
  src([&](unsigned long long c) {
    if (c >= thr) {
      const int pos = atomicAdd(s_cnt, 1);
      if (pos < cap) dst[pos] = c;
    }
  });
  __syncthreads();
  return *s_cnt < cap ? *s_cnt : cap;
}

// All threads: sort the first n keys of the LDS array s (n <= cap, cap a power of two) descending.  The slots from n to
// the next power of two are overwritten with 0, which must rank below every real key.
template <int NT>
__device__ void egtr_bitonic_sort_desc(unsigned long long* s, int n) {
  const int tid = threadIdx.x;
  int P = 1;
  while (P < n) P <<= 1;
  for (int i = n + tid; i < P; i += NT) s[i] = 0ull;
  __syncthreads();
  for (int k = 2; k <= P; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < P; i += NT) {
        const int x = i ^ j;
        if (x > i) {
          const unsigned long long u = s[i], v = s[x];
          if ((i & k) == 0 ? u < v : u > v) {
            s[i] = v;
            s[x] = u;
          }
        }
      }
      __syncthreads();
    }
  }
}
