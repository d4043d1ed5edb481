// Order-free accumulation of fp32 contributions: 64-bit fixed point, added with INTEGER atomics.  Integer addition is
// associative, so the sum does not depend on the order in which the contributions arrive; one rounding to fp32 follows
// at the end.  Used by the deterministic route of the MSDA backward (grad_value, msda.hip / msda_tile.hip); the header
// has no HIP dependency beyond the __host__ __device__ markers, so a host program can include it (tests/test_deterministic_cpu.py).
//
// The scale is a power of two, 2^k, chosen from three integers that are themselves order-free:
//   ea, eg : binary exponents with  max|attn_weight| < 2^ea,  max|grad_out| < 2^eg  (taken from the BIT PATTERNS of the two
//            maxima, which the device forms with integer atomicMax: |x| as an unsigned is monotone in |x|),
//   en     : ceil(log2(terms)), terms = Lq * L * P = the most contributions ONE element of grad_value can receive (a sample
//            touches four DISTINCT pixels, so it gives a pixel at most one contribution per channel; the weights are not
//            assumed to be a softmax, the C ABI takes arbitrary ones).
//   k = 61 - (ea + eg + en).
// Overflow proof.  A contribution is  w * a * g  with a bilinear weight 0 <= w <= 1, so |c| <= 2^(ea+eg) (the fp32 roundings of
// the product are monotone and cannot step past the power of two).  The exact sum of any subset of the contributions
// to one element is at most terms * 2^(ea+eg) <= 2^(ea+eg+en), i.e. at most 2^61 after scaling.  What is added is
// rint(partial * 2^k) where a partial is one contribution (wave-per-query and generic kernels) or the fp32 sum of up to
// 64 x 16 of them (value-tile kernel: relative error < 2^-13, far inside the spare bit): each rint moves a term by at
// most 1/2 and there are at most `terms` <= 2^en <= 2^40 terms, so |sum| <= 2^61 (1 + 2^-13) + 2^39 < 2^62.  Intermediate
// sums may wrap -- two's complement addition is modular, the final value is what has to fit, and it does.
// Where ea + eg + en > 127 a partial sum could overflow fp32 itself before it is converted; such calls are treated like
// non-finite input (see `poisoned` below) and never reach the conversion.
// Resolution.  One unit is 2^-k = 2^(ea+eg+en-61): against the largest possible single contribution 2^(ea+eg) that is
// 2^(en-61) -- 2^-43 for the 600 x 1000 encoder call (terms = 12 537 * 16 < 2^18), i.e. every contribution larger than
// 2^-20 of the largest possible one is added EXACTLY (its 24-bit mantissa lies above the unit) and smaller ones are
// rounded to 2^-43 of it; fp32 atomics round every partial sum to 2^-24 of the running value.
// Scaling.  ldexpf / the int64 -> fp32 conversion are exact or round once: multiplying every grad_out by 2^j moves eg
// by j and k by -j, the integers added are the same and the result is exactly 2^j times the old one (unless it leaves
// the normal range of fp32).  Exponents are handled as integers throughout: neither the product of the two maxima nor
// the scale is ever formed as a float.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define EGTR_FX_HD __host__ __device__ inline
#else
#define EGTR_FX_HD inline
#endif

namespace egtr_fixed {

// the deterministic workspace starts with this header; the int64 accumulators follow it
constexpr int kHeaderBytes = 64;   // [0] bits of max|attn_weight|, [1] bits of max|grad_out|, rest unused

EGTR_FX_HD unsigned abs_bits(float x) {   // |x| as an unsigned: monotone in |x|, NaN above inf above every finite value
  unsigned u;
  memcpy(&u, &x, 4);
  return u & 0x7fffffffu;
}

EGTR_FX_HD bool bits_finite(unsigned abs_bits_) { return abs_bits_ < 0x7f800000u; }

// e with |x| < 2^e  (denormals: the biased exponent 0 gives -126, and they are below 2^-126)
EGTR_FX_HD int bound_exp(unsigned abs_bits_) { return (int)(abs_bits_ >> 23) - 126; }

EGTR_FX_HD int ceil_log2(unsigned long long n) {
  int e = 0;
  while (e < 63 && (1ull << e) < n) ++e;
  return e;
}

struct Scale {
  int k;           // fixed = rint(x * 2^k)
  bool poisoned;   // a non-finite maximum, or products that could overflow fp32: the result is NaN everywhere
};

EGTR_FX_HD Scale make_scale(unsigned attn_max_bits, unsigned grad_max_bits, unsigned long long terms) {
  Scale s;
  s.k = 0;
  s.poisoned = !bits_finite(attn_max_bits) || !bits_finite(grad_max_bits);
  if (s.poisoned || attn_max_bits == 0u || grad_max_bits == 0u) return s;   // all-zero operand: every contribution is 0
  const int e = bound_exp(attn_max_bits) + bound_exp(grad_max_bits) + ceil_log2(terms);
  if (e > 127) s.poisoned = true;
  s.k = 61 - e;
  return s;
}

EGTR_FX_HD long long to_fixed(float x, int k) { return llrintf(ldexpf(x, k)); }

EGTR_FX_HD float from_fixed(long long sum, int k) { return ldexpf((float)sum, -k); }   // one rounding: int64 -> fp32

}  // namespace egtr_fixed
