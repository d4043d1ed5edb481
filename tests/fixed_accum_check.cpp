// Host check of egtr_amd/csrc/fixed_accum.h (built and run by tests/test_deterministic_cpu.py with
// -fsanitize=undefined,address): the overflow bound at its worst case, order independence, exact power-of-two scaling.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "fixed_accum.h"

namespace fx = egtr_fixed;

static int fails = 0;
#define CHECK(c)                                                    \
  do {                                                              \
    if (!(c)) {                                                     \
      std::printf("FAILED line %d: %s\n", __LINE__, #c);            \
      ++fails;                                                      \
    }                                                               \
  } while (0)

static unsigned fbits(float x) {
  unsigned u;
  std::memcpy(&u, &x, 4);
  return u;
}

// (1) every contribution = max|attn| * max|grad_out| with bilinear weight 1, `terms` of them, one sign: |sum| < 2^62
static void worst_case(float amax, float gmax, unsigned long long terms) {
  const fx::Scale s = fx::make_scale(fx::abs_bits(amax), fx::abs_bits(gmax), terms);
  CHECK(!s.poisoned);
  for (int sign = -1; sign <= 1; sign += 2) {
    const float c = (float)sign * (amax * gmax);
    const long long one = fx::to_fixed(c, s.k);
    const __int128 total = (__int128)one * (__int128)terms;   // what `terms` equal additions give
    const __int128 lim = (__int128)1 << 62;
    CHECK(total < lim && total > -lim);
    // and really added, with signed 64-bit additions (UBSan reports an overflow), for counts that can be looped over
    if (terms <= (1ull << 22)) {
      long long acc = 0;
      for (unsigned long long i = 0; i < terms; ++i) acc += one;
      CHECK((__int128)acc == total);
      const float back = fx::from_fixed(acc, s.k);
      CHECK(std::isfinite(back) || !std::isfinite((float)terms * c));
      if (std::isfinite((float)((double)terms * (double)c)))
        CHECK(std::fabs((double)back - (double)terms * (double)c) <= std::ldexp(std::fabs((double)terms * (double)c), -23));
    }
  }
}

int main() {
  // ---- (1) the bound at its worst case: mantissas all ones (just below the power of two), small / large exponents
  const float just_below_one = std::nextafter(1.0f, 0.0f);
  const unsigned long long counts[] = {1ull, 16ull, 12537ull * 16, 1ull << 22, (1ull << 22) + 1, 22223ull * 16 * 16,
                                       (1ull << 40) - 1, 1ull << 40};
  for (unsigned long long n : counts) {
    worst_case(just_below_one, just_below_one, n);
    worst_case(std::ldexp(just_below_one, -30), std::ldexp(just_below_one, 50), n);
    worst_case(std::ldexp(just_below_one, -100), std::ldexp(just_below_one, -20), n);   // product far below FLT_MIN
    worst_case(std::ldexp(just_below_one, 40), std::ldexp(just_below_one, 40), n);
    worst_case(1.0f, 1.0f, n);   // exact powers of two: the exponent bound is strict (|x| < 2^e)
    worst_case(std::nextafter(0.0f, 1.0f), 3.0f, n);   // denormal maximum
  }
  // all-zero operand: finite scale, zero sum; non-finite operand: poisoned
  {
    const fx::Scale z = fx::make_scale(fx::abs_bits(0.5f), fx::abs_bits(0.0f), 1000);
    CHECK(!z.poisoned && fx::to_fixed(0.0f, z.k) == 0 && fx::from_fixed(0, z.k) == 0.0f);
    CHECK(fx::make_scale(fx::abs_bits(0.5f), fx::abs_bits(INFINITY), 1000).poisoned);
    CHECK(fx::make_scale(fx::abs_bits(-NAN), fx::abs_bits(1.0f), 1000).poisoned);
    CHECK(fx::make_scale(fx::abs_bits(3e38f), fx::abs_bits(3e38f), 1000).poisoned);   // products overflow fp32
  }

  // ---- (2) one fixed list of contributions, 50 random orders: one bit pattern
  std::mt19937 rng(12345);
  std::normal_distribution<float> nd(0.f, 1.f);
  std::uniform_real_distribution<float> ud(0.f, 1.f);
  const int n = 4096;
  std::vector<float> attn(n), go(n), w(n);
  float amax = 0.f, gmax = 0.f;
  for (int i = 0; i < n; ++i) {
    attn[i] = ud(rng) * std::ldexp(1.0f, -(int)(rng() % 12));   // a wide spread of magnitudes
    go[i] = nd(rng) * std::ldexp(1.0f, (int)(rng() % 20) - 10);
    w[i] = ud(rng);
    amax = std::max(amax, std::fabs(attn[i]));
    gmax = std::max(gmax, std::fabs(go[i]));
  }
  auto total = [&](const std::vector<int>& order, float gscale, int* kout) {
    const fx::Scale s = fx::make_scale(fx::abs_bits(amax), fx::abs_bits(gmax * gscale), (unsigned long long)n);
    long long acc = 0;
    for (int i : order) acc += fx::to_fixed(w[i] * ((go[i] * gscale) * attn[i]), s.k);
    if (kout) *kout = s.k;
    return fx::from_fixed(acc, s.k);
  };
  std::vector<int> order(n);
  for (int i = 0; i < n; ++i) order[i] = i;
  const float first = total(order, 1.0f, nullptr);
  double exact = 0.0;
  for (int i = 0; i < n; ++i) exact += (double)(w[i] * (go[i] * attn[i]));
  CHECK(std::fabs((double)first - exact) <= std::ldexp(std::fabs(exact), -23) + 1e-30);   // one rounding to fp32
  for (int r = 0; r < 50; ++r) {
    std::shuffle(order.begin(), order.end(), rng);
    CHECK(fbits(total(order, 1.0f, nullptr)) == fbits(first));
  }

  // ---- (3) grad_out * 2^j scales the result by exactly 2^j
  for (int j : {40, -40}) {
    int k0 = 0, k1 = 0;
    const float base = total(order, 1.0f, &k0);
    const float scaled = total(order, std::ldexp(1.0f, j), &k1);
    CHECK(k1 == k0 - j);
    CHECK(fbits(scaled) == fbits(std::ldexp(base, j)));
  }
  if (fails == 0) std::printf("fixed_accum ok\n");
  return fails == 0 ? 0 : 1;
}
