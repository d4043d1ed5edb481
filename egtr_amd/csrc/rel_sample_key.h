// The random selection key of the relation loss (csrc/loss.hip): a keyed bijection of the 32-bit flat index
// (qa N + qb) R + r of an element, so distinct elements of an image have distinct keys and "the k candidates with the largest
// key" is a k-subset without ties.  The two key words of an (image, class) come from one Philox4x32-10 block
//   (w0, w1, ., .) = Philox(counter = (image, class, lo32(stream), hi32(stream)), key = (lo32(seed), hi32(seed))),
// computed once per image by rel_loss_prep; per element the key costs two multiplies and a few shifts.
// Host and device: the same text serves the stand-alone host check of the known answers.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define EGTR_HD __host__ __device__ __forceinline__
#else
#define EGTR_HD inline
#endif

EGTR_HD void egtr_philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                uint32_t out[4]) {
  for (int round = 0; round < 10; ++round) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u;   // Weyl sequence of the key
    k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

EGTR_HD uint32_t egtr_lb32(uint32_t x) {   // a bijection of 32 bits: xor-shifts and odd multipliers
  x ^= x >> 16;
  x *= 0x7feb352du;
  x ^= x >> 15;
  x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}

EGTR_HD uint32_t egtr_rel_sample_key(uint32_t flat, uint32_t ka, uint32_t kb) {
  return egtr_lb32(egtr_lb32(flat ^ ka) + kb);
}
