// Training-set relation statistics: the reference's fg_matrix -- counts[class(s), class(o), p] over every
// relation row of every training image (data/visual_genome.py:84-118 vg_get_statistics, data/open_image.py:161-185
// oi_get_statistics: Python loops over the dataset) -- accumulated on the device from the ragged relation layout the
// evaluators already upload (sgg_eval.hip), and the bitset "this (class, class, predicate) occurs in training" that the
// zero-shot recall reads.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common.h"
#include "sgg_match.h"

using namespace egtr_eval;

namespace {

constexpr int kThreads = 256;

// One thread per relation row: its image from the row offsets (binary search over B + 1 entries), the two classes through
// the image's object range, one 64-bit integer atomic add.  Integer addition is order-free, so the counts are the same on
// every run.  Duplicate rows count each time (both reference loops do).  A row with a subject / object index outside its
// image's objects, a class outside [0, C1) or a predicate outside [0, R) is NOT counted and raises bit 0 of *status (sticky).
__global__ __launch_bounds__(kThreads) void rel_stats_count(const int64_t* __restrict__ rels,
                                                            const int64_t* __restrict__ rel_off, long long T,
                                                            const int64_t* __restrict__ classes,
                                                            const int64_t* __restrict__ box_off, long long G, int B,
                                                            int C1, int R, unsigned long long* __restrict__ counts,
                                                            unsigned* __restrict__ status) {
  const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= T) return;
  int lo = 0, hi = B;   // the image b with rel_off[b] <= i < rel_off[b + 1]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (rel_off[mid] <= i) lo = mid; else hi = mid;
  }
  const ImageRange im(rel_off, box_off, T, G, lo);
  bool ok = im.r0 <= i && i < im.r1;   // offsets that do not cover the row: not counted (0 <= i < T, so clamping keeps this)
  const long long g0 = im.g0, n = im.n_box();
  const long long s = rels[3 * i], o = rels[3 * i + 1], p = rels[3 * i + 2];
  ok = ok && s >= 0 && s < n && o >= 0 && o < n && p >= 0 && p < R;
  if (ok) {
    const long long cs = classes[g0 + s], co = classes[g0 + o];
    ok = cs >= 0 && cs < C1 && co >= 0 && co < C1;
    if (ok) atomicAdd(&counts[(cs * C1 + co) * R + p], 1ull);
  }
  if (!ok) atomicOr(status, 1u);
}

// bit (i & 63) of word i >> 6 = counts[i] > 0: a wave's ballot IS the word (kThreads is a multiple of 64, so a wave covers
// one aligned group of 64 counts); lanes past n vote 0.
__global__ __launch_bounds__(kThreads) void rel_seen_bits(const long long* __restrict__ counts, long long n,
                                                          unsigned long long* __restrict__ bits) {
  const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
  const bool seen = i < n && counts[i] > 0;
  const unsigned long long word = __ballot(seen);
  if ((threadIdx.x & 63) == 0 && (i >> 6) < ((n + 63) >> 6)) bits[i >> 6] = word;
}

}  // namespace

extern "C" int egtr_rel_stats_i64(egtr_stream_t stream, const int64_t* rels, const int64_t* rel_offsets,
                                  long long num_rels, const int64_t* classes, const int64_t* box_offsets,
                                  long long num_boxes, int batch, int num_classes, int num_rel, int64_t* counts,
                                  int* status) {
  if (batch < 0 || num_rels < 0 || num_boxes < 0 || num_classes < 1 || num_rel < 1) return EGTR_E_ARG;
  if ((long long)num_classes * num_classes * num_rel >= (1ll << 31)) return EGTR_E_UNSUPPORTED;
  if (batch == 0 || num_rels == 0) return EGTR_OK;
  if (!rels || !rel_offsets || !box_offsets || !counts || !status || (num_boxes > 0 && !classes)) return EGTR_E_ARG;
  if ((num_rels + kThreads - 1) / kThreads >= (1ll << 31)) return EGTR_E_UNSUPPORTED;
  hipLaunchKernelGGL(rel_stats_count, dim3((unsigned)((num_rels + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                     static_cast<hipStream_t>(stream), rels, rel_offsets, num_rels, classes, box_offsets, num_boxes,
                     batch, num_classes, num_rel, reinterpret_cast<unsigned long long*>(counts),
                     reinterpret_cast<unsigned*>(status));
  return egtr_check_launch();
}

extern "C" int egtr_rel_seen_bits_i64(egtr_stream_t stream, const int64_t* counts, long long num_counts,
                                      int64_t* bits) {
  if (num_counts < 1 || num_counts >= (1ll << 31) || !counts || !bits) return EGTR_E_ARG;
  hipLaunchKernelGGL(rel_seen_bits, dim3((unsigned)((num_counts + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                     static_cast<hipStream_t>(stream), reinterpret_cast<const long long*>(counts), num_counts,
                     reinterpret_cast<unsigned long long*>(bits));
  return egtr_check_launch();
}
