// Stand-alone development harness of the encoder-tail kernel (csrc/ffn_x6.hip, ffn_x6_kernel<true>): launch time on random
// inputs (correctness: tests/test_gpu_pinning.py, tests/test_gpu_ffn_handover.py).  With -DEGTR_FFN_X6_TIMING on the same command
// line: the kernel's cycle stamps around the stages of the FFN walk and its hand-over (profiles/ffn_x6_handover_ab.txt).
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 tools/enc_tail_bench.hip egtr_amd/csrc/ffn_x6.hip \
//         egtr_amd/csrc/xs_split.hip egtr_amd/csrc/capi.hip -o build/enc_tail_bench && build/enc_tail_bench [M F iters with_pos]
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../include/egtr_hip.h"

#ifdef EGTR_FFN_X6_TIMING
extern "C" int egtr_ffn_x6_stamps(unsigned* host_out);   // csrc/ffn_x6.hip, stamp build: [256 workgroups][24]
#endif

#define CK(x)                                                                   \
  do {                                                                          \
    hipError_t e_ = (x);                                                        \
    if (e_ != hipSuccess) {                                                     \
      fprintf(stderr, "%s:%d %s\n", __FILE__, __LINE__, hipGetErrorString(e_)); \
      exit(2);                                                                  \
    }                                                                           \
  } while (0)


int main(int argc, char** argv) {
  const int M = argc > 1 ? atoi(argv[1]) : 12537, F = argc > 2 ? atoi(argv[2]) : 1024, iters = argc > 3 ? atoi(argv[3]) : 100;
  const int with_pos = argc > 4 ? atoi(argv[4]) : 0;   // the model runs it without the position output since the lazy-pos GEMM
  const int D = 256;
  std::mt19937 rng(4);
  std::normal_distribution<float> nd(0.f, 1.f);
  auto mk = [&](size_t n, float sc, float off = 0.f) {
    std::vector<float> h(n);
    for (auto& v : h) v = off + nd(rng) * sc;
    float* d;
    CK(hipMalloc(&d, n * 4));
    CK(hipMemcpy(d, h.data(), n * 4, hipMemcpyHostToDevice));
    return d;
  };
  float *ctx = mk((size_t)M * D, 1), *hid = mk((size_t)M * D, 1), *pos = mk((size_t)M * D, 1);
  float *wp = mk(D * D, 1 / 16.f), *bp = mk(D, .3f), *g1 = mk(D, .2f, 1.f), *be1 = mk(D, .2f);
  float *w1 = mk((size_t)F * D, 1 / 16.f), *b1 = mk(F, .3f), *w2 = mk((size_t)D * F, 1 / 32.f), *b2 = mk(D, .3f);
  float *g2 = mk(D, .2f, 1.f), *be2 = mk(D, .2f);
  void *xp, *x1, *x2;
  CK(hipMalloc(&xp, egtr_xs_bytes(D, D)));
  CK(hipMalloc(&x1, egtr_xs_bytes(F, D)));
  CK(hipMalloc(&x2, egtr_xs_bytes(D, F)));
  if (egtr_xs_split_f32(nullptr, wp, D, nullptr, 0, D, D, xp, nullptr, 1) ||
      egtr_xs_split_f32(nullptr, w1, D, nullptr, 0, F, D, x1, nullptr, 1) ||
      egtr_xs_split_f32(nullptr, w2, F, nullptr, 0, D, F, x2, nullptr, 1))
    return 2;
  float *out, *outp;
  CK(hipMalloc(&out, (size_t)M * D * 4));
  CK(hipMalloc(&outp, (size_t)M * D * 4));
  auto run = [&]() {
    return egtr_encoder_tail_x6_f32(nullptr, ctx, D, hid, D, xp, bp, g1, be1, 1e-5f, x1, b1, x2, b2, g2, be2, 1e-5f, with_pos ? pos : nullptr, M, out,
                                    with_pos ? outp : nullptr, M, D, F);
  };
  int rc = run();
  CK(hipDeviceSynchronize());
  if (rc) {
    fprintf(stderr, "rc %d (%s)\n", rc, egtr_last_hip_error());
    return 2;
  }
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  CK(hipEventRecord(e0));
  for (int i = 0; i < iters; ++i) run();
  CK(hipEventRecord(e1));
  CK(hipEventSynchronize(e1));
  float ms;
  CK(hipEventElapsedTime(&ms, e0, e1));
  printf("M=%d F=%d: %.2f us per launch\n", M, F, ms * 1e3 / iters);
#ifdef EGTR_FFN_X6_TIMING
  {
    // mean / min / max over the workgroups of the last launch; the steady-state sums per stage
    static const char* const names[9] = {"steady state: L1 stages 0-3, per stage", nullptr,
                                         "steady state: L2 stages 0-2 (hand-over VALU behind the MFMAs), per stage",
                                         "steady state: L2 stage 3 (hand-over LDS stores behind the MFMAs)",
                                         "first hand-over, exposed (last L1 MFMA to the next top), per panel",
                                         "last L2 group, stage 0 (operand read after the top), per panel", "FFN walk, per panel",
                                         "workgroup, per panel", "in front of the FFN walk, per panel"};
    static const int per[9] = {4, 0, 3, 1, 0, 0, 0, 0, 0};   // stages summed per steady-state iteration; 0: once per panel
    std::vector<unsigned> rec(256 * 24);
    if (egtr_ffn_x6_stamps(rec.data())) return 2;
    const int nwg = std::min(256, (M + 63) / 64), nchunk = F / 64;
    for (int k = 0; k < 9; ++k) {
      if (names[k] == nullptr) continue;
      double sum = 0, lo = 1e30, hi = 0;
      const double div = per[k] ? per[k] * std::max(1, nchunk - 1) : 1;
      for (int b = 0; b < nwg; ++b) {
        const double v = rec[b * 24 + k] / div;
        sum += v;
        lo = std::min(lo, v);
        hi = std::max(hi, v);
      }
      printf("  %-74s mean %9.0f  min %9.0f  max %9.0f cycles%s\n", names[k], sum / nwg, lo, hi, "");
    }
  }
#endif
  return 0;
}
