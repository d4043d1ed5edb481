// Relation targets as bit-packed words: an image's relation triplets (subject, object, predicate) -> one
// 64-bit word per (subject, object) pair, bit p set iff (s, o, p) is a triplet.  The reference builds a dense fp32
// [N, N, 50] tensor per image on the host instead (data/visual_genome.py:74-80: 8 MB at N = 200 for a few dozen ones).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common.h"

namespace {

constexpr int kPT = 256;

// One thread per triplet: its image from the offsets (binary search over batch + 1 entries), one 64-bit atomic OR.  A triplet
// with an index outside [0, N) x [0, N) x [0, R) is dropped -- nothing is written for it (triplets that were built on the
// device never passed the host's checks).  Duplicates set the same bit twice.
__global__ __launch_bounds__(kPT) void pack_relations(const long long* __restrict__ triplets,
                                                      const int* __restrict__ offsets, int B, int total, int N, int R,
                                                      unsigned long long* __restrict__ bits) {
  const int i = blockIdx.x * kPT + threadIdx.x;
  if (i >= total || i >= offsets[B]) return;
  int lo = 0, hi = B;   // the image b with offsets[b] <= i < offsets[b + 1]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (offsets[mid] <= i) lo = mid; else hi = mid;
  }
  const long long s = triplets[3 * (size_t)i], o = triplets[3 * (size_t)i + 1], p = triplets[3 * (size_t)i + 2];
  if (s < 0 || s >= N || o < 0 || o >= N || p < 0 || p >= R) return;
  atomicOr(&bits[((size_t)lo * N + (size_t)s) * N + (size_t)o], 1ull << p);
}

// The same thread per triplet for W = ceil(R / 64) words per pair: bit p & 63 of word p >> 6 (R <= 256).
__global__ __launch_bounds__(kPT) void pack_relations_wide(const long long* __restrict__ triplets,
                                                           const int* __restrict__ offsets, int B, int total, int N, int R,
                                                           int W, unsigned long long* __restrict__ bits) {
  const int i = blockIdx.x * kPT + threadIdx.x;
  if (i >= total || i >= offsets[B]) return;
  int lo = 0, hi = B;   // the image b with offsets[b] <= i < offsets[b + 1]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (offsets[mid] <= i) lo = mid; else hi = mid;
  }
  const long long s = triplets[3 * (size_t)i], o = triplets[3 * (size_t)i + 1], p = triplets[3 * (size_t)i + 2];
  if (s < 0 || s >= N || o < 0 || o >= N || p < 0 || p >= R) return;
  atomicOr(&bits[(((size_t)lo * N + (size_t)s) * N + (size_t)o) * W + (size_t)(p >> 6)], 1ull << (p & 63));
}

}  // namespace

// triplets int64 [total, 3] (s, o, p), the images' rows concatenated; offsets int32 [batch + 1] (image b's rows are
// offsets[b] .. offsets[b + 1]), both on the device; rel_bits [batch, N, N] words, fully overwritten: one memset, one launch.
extern "C" int egtr_pack_relations_u64(egtr_stream_t stream, const int64_t* triplets, const int* offsets, int batch,
                                       int total, int num_query, int num_rel, uint64_t* rel_bits) {
  if (!triplets || !offsets || !rel_bits) return EGTR_E_ARG;
  if (batch <= 0 || total < 0 || num_query <= 0 || num_rel <= 0) return EGTR_E_ARG;
  if (num_rel > 64) return EGTR_E_UNSUPPORTED;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (hipMemsetAsync(rel_bits, 0, (size_t)batch * num_query * num_query * 8, st) != hipSuccess) return EGTR_E_LAUNCH;
  if (total > 0)
    hipLaunchKernelGGL(pack_relations, dim3((total + kPT - 1) / kPT), dim3(kPT), 0, st,
                       reinterpret_cast<const long long*>(triplets), offsets, batch, total, num_query, num_rel,
                       reinterpret_cast<unsigned long long*>(rel_bits));
  return egtr_check_launch();
}

// The words of a vocabulary of up to 256 predicates: rel_bits [batch, N, N, W], W = ceil(num_rel / 64); bit p & 63 of word
// (s, o, p >> 6) set iff (s, o, p) is a triplet, bits at positions >= num_rel stay zero.  The contract of the entry above: one
// memset, one launch, rel_bits fully overwritten; with W = 1 the same memory.
extern "C" int egtr_pack_relations_wide_u64(egtr_stream_t stream, const int64_t* triplets, const int* offsets, int batch,
                                            int total, int num_query, int num_rel, uint64_t* rel_bits) {
  if (!triplets || !offsets || !rel_bits) return EGTR_E_ARG;
  if (batch <= 0 || total < 0 || num_query <= 0 || num_rel <= 0) return EGTR_E_ARG;
  if (num_rel > 256) return EGTR_E_UNSUPPORTED;
  const int W = (num_rel + 63) / 64;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (hipMemsetAsync(rel_bits, 0, (size_t)batch * num_query * num_query * W * 8, st) != hipSuccess) return EGTR_E_LAUNCH;
  if (total > 0)
    hipLaunchKernelGGL(pack_relations_wide, dim3((total + kPT - 1) / kPT), dim3(kPT), 0, st,
                       reinterpret_cast<const long long*>(triplets), offsets, batch, total, num_query, num_rel, W,
                       reinterpret_cast<unsigned long long*>(rel_bits));
  return egtr_check_launch();
}
