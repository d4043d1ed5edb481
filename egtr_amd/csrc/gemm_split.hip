// Token-sized fp32 linear layers on the bf16 matrix cores:  C[M, N] = act(A[M, K] . W[N, K]^T + bias)  with fp32 operands
// in, fp32 out and fp32-level accuracy, from exact three-way bf16 splits of both operands (see rel_head.hip,
// rel_head_fwd_x6, for the argument: x = hi + mid + lo exactly, the six leading cross terms kept, every bf16 x bf16
// product exact in fp32, fp32 accumulation; the three dropped terms are <= 2^-24 of the product).
//
// Why: the encoder applies five nn.Linear layers per layer to S = 12 537 token rows (value / output projections,
// sampling offsets + attention weights, the two FFN layers): 1.05 of the 4.1 ms forward, running at 100-125 TFLOP/s in
// hipBLASLt -- 65-80 % of the fp32 matrix peak of this part, which is its fp32 VECTOR rate (157 TFLOP/s).  The bf16
// matrix rate is 16x that; six bf16 MFMAs per K = 16 replace eight fp32 MFMAs of twice the length: 2.67x less matrix
// time for the same result to fp32 rounding.
//
// Tiling: a workgroup of 8 waves owns a 128 x 128 (or 64 x 128) tile of C, each wave 32 x 64 (32 x 32) of it on
// v_mfma_f32_32x32x16_bf16.  K runs in stages of 32: the fp32 A tile is split into its three pieces on the way into
// LDS; W arrives pre-split and pre-tiled from the host (one contiguous 24 KiB block per stage:
// wt[N/128][K/32][3 pieces][128 rows][32] bf16, egtr_amd/kernels/linear.py::gemm_split_weights).  The global loads of stage s + 1
// are in flight (inline asm, counted) while stage s is multiplied out of LDS; rows are 80 bytes apart in LDS, which
// makes the 16-byte operand reads of 32 consecutive rows conflict-free.  60 (45) KiB of LDS and <= 128 registers per
// lane: two workgroups = sixteen waves per CU.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "common.h"
#include "x6_staged.h"

namespace {
using namespace x6;   // the staged main loop and its geometry (kBN, kBK, kPitch): x6_staged.h

// The activations are split with xs::split3_fast (round 4; the inf-safe xs::split3 until then): 4 VALU operations per element
// instead of 10 -- these kernels split every activation element N / 128 times over, and the weight-gradient kernel both
// operands: 3-4.5 % off the forward / data-gradient products and 8-9 % off the weight gradients at the training size
// (abl/gemm_fast.sh, two alternations on one box).  What that does to a non-finite element: x6_staged.h, tests/test_gpu_pinning.py.

// A workgroup is 8 waves on a BM x 128 tile, BM = 128 (wave tile 32 x 64) or 64 (wave tile 32 x 32; chosen when 128-row
// tiles would not give every CU two workgroups).  <= 128 registers per lane: four waves per SIMD, so that the load /
// split / store phases of one wave run under the matrix work of the others -- with one or two waves per SIMD every
// per-stage latency (operand reads, barrier, vmcnt, LDS stores) was exposed and the kernel ran at the vendor fp32 rate.
// MFMA roles: A operand = weight piece (i = n), B operand = activation piece (j = m), so that a lane ends up with 4
// CONSECUTIVE output columns per accumulator quad: the epilogue stores float4.
// Up to kMaxProblems independent products with the same M and K in ONE launch (the value projection and the offsets /
// attention-weights projection of an encoder layer; the six value projections of the decoder): their tiles share the
// grid, so that products which do not fill the chip on their own (196-588 tiles on 512 workgroup slots) fill it together.
// The tile order goes through xcd_tile (x6_common.h): the tiles running side by side on one XCD are neighbours in the order
// below (instead of every n block of a row tile fetching the activation rows again through another L2).

constexpr int kMaxProblems = 16;   // (the relation head's 14 slot products share one grid)
struct GemmProblem {
  const float* A;
  const unsigned short* Wt;
  const float* bias;
  float* C;
  int lda, ldc, N, relu;
  const float* pos;   // optional [pos_rows, K] added to the rows of A on their way into LDS (row % pos_rows): the encoder's
  int pos_rows;       // `hidden_states + position_embeddings` (dd:1041) without a materialised sum
  // epilogue extensions of the training step (egtr_linear_split_bf16_ex_f32), applied in this order; all optional:
  const unsigned char* row_keep;   // [M] bytes: rows with 0 produce zeros (value rows of padded tokens, dd:1052, and their
                                   // gradients in the backward)
  const float* relu_ref;           // [M, ldref]: v = relu_ref > 0 ? v : 0 -- the ReLU backward of the layer whose OUTPUT
  int ldref;                       // relu_ref is, applied to this data-gradient product
  const float* add1;               // [M, ldadd] addends (gradient accumulation of the branches that meet at a tensor);
  const float* add2;               // add1 / add2 may alias C (an element is read and written by the same lane)
  int ldadd;
  float* colpart;                  // [ceil(M / 32), N]: column sums of the stored values over each 32-row block (the bias
                                   // gradient of the consuming layer: summed in a fixed order by a second tiny launch)
};
struct GemmProblems {
  GemmProblem p[kMaxProblems];
};

// The epilogue of a tile as a function, for the one-term kernel (gemm_bf16r_f32 below): bias, ReLU, row_keep, relu_ref, add1 / add2,
// the store and colpart, in this order.  wm / wn: the wave's place in the workgroup's BM x 128 tile.  The six-term kernel keeps
// the same statements in its own body: routed through this function its register allocation changed throughout, and its
// instruction stream is to stay the parent's (the weight gradient keeps its own loop for the same reason).
template <int NT>
__device__ __forceinline__ void gemm_epilogue(const GemmProblem& G, const f32x16 (&acc)[NT], int M, int nb, int m0, int wm, int wn,
                                              int li, int hf) {
  const float* __restrict__ bias = G.bias;
  float* __restrict__ C = G.C;
  const int ldc = G.ldc;
  const bool RELU = G.relu != 0;
  // D[i = n][j = m]; accumulator r <-> column n = (r & 3) + 8 (r >> 2) + 4 hf of the 32-wide n tile, row m = lane & 31: one
  // float4 (4 consecutive columns) per accumulator quad
  const int row = m0 + wm * 32 + li;
  const bool in_range = row < M;
  const bool keep = in_range && (G.row_keep == nullptr || G.row_keep[row] != 0);
  const float* __restrict__ relu_ref = G.relu_ref;
  const float* add1 = G.add1;
  const float* add2 = G.add2;
  float* __restrict__ colpart = G.colpart;
#pragma unroll
  for (int nt = 0; nt < NT; ++nt)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int col = nb * kBN + wn * (32 * NT) + nt * 32 + 8 * q + 4 * hf;
      float4 bv = make_float4(0.f, 0.f, 0.f, 0.f);
      if (bias != nullptr) bv = *reinterpret_cast<const float4*>(bias + col);
      float4 v = make_float4(acc[nt][4 * q + 0] + bv.x, acc[nt][4 * q + 1] + bv.y, acc[nt][4 * q + 2] + bv.z,
                             acc[nt][4 * q + 3] + bv.w);
      if (RELU) v = make_float4(egtr_relu(v.x), egtr_relu(v.y), egtr_relu(v.z), egtr_relu(v.w));
      if (!keep) v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (relu_ref != nullptr && in_range) {
        const float4 t = *reinterpret_cast<const float4*>(relu_ref + (size_t)row * G.ldref + col);
        v = make_float4(t.x > 0.f ? v.x : 0.f, t.y > 0.f ? v.y : 0.f, t.z > 0.f ? v.z : 0.f, t.w > 0.f ? v.w : 0.f);
      }
      if (add1 != nullptr && in_range) {
        const float4 t = *reinterpret_cast<const float4*>(add1 + (size_t)row * G.ldadd + col);
        v = make_float4(v.x + t.x, v.y + t.y, v.z + t.z, v.w + t.w);
      }
      if (add2 != nullptr && in_range) {
        const float4 t = *reinterpret_cast<const float4*>(add2 + (size_t)row * G.ldadd + col);
        v = make_float4(v.x + t.x, v.y + t.y, v.z + t.z, v.w + t.w);
      }
      if (in_range) *reinterpret_cast<float4*>(C + (size_t)row * ldc + col) = v;
      if (colpart != nullptr) {   // uniform per workgroup: sum over the wave's 32 rows (the 32 lanes that share hf)
        float4 s = in_range ? v : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int o = 1; o < 32; o <<= 1) {
          s.x += __shfl_xor(s.x, o);
          s.y += __shfl_xor(s.y, o);
          s.z += __shfl_xor(s.z, o);
          s.w += __shfl_xor(s.w, o);
        }
        // (a 32-row block that starts at or beyond M does not exist in the [ceil(M / 32), N] buffer)
        if (li == 0 && m0 + wm * 32 < M) *reinterpret_cast<float4*>(colpart + (size_t)((m0 >> 5) + wm) * G.N + col) = s;
      }
    }
}

// (A double-buffered form of this loop -- two LDS stage buffers, one barrier per stage, 120 KiB of LDS = one workgroup per CU --
// and a ping-pong schedule on it were measured 7-15 % slower in round 5 and removed in round 6: DESIGN.md 4.12,
// profiles/r05_gemm_double_buffer_ab.txt; the code is in the history, commit 46d9c2f and before.)
template <int BM>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(4, 4))) void gemm_split_bf16_f32(
    GemmProblems P, int nprob, int M, int K) {
  // tile -> (problem, n block, m block): n blocks of one m block are neighbours (they read the same activation rows)
  const int mblocks = (M + BM - 1) / BM;
  int tile = xcd_tile(blockIdx.x, gridDim.x), pi = 0;
  for (; pi + 1 < nprob; ++pi) {
    const int t = (P.p[pi].N / kBN) * mblocks;
    if (tile < t) break;
    tile -= t;
  }
  const GemmProblem& G = P.p[pi];
  const int nblocks = G.N / kBN;
  const int nb = tile % nblocks, m0 = (tile / nblocks) * BM;
  const float* __restrict__ A = G.A;
  const unsigned short* __restrict__ Wt = G.Wt;
  const float* __restrict__ bias = G.bias;
  float* __restrict__ C = G.C;
  const int lda = G.lda, ldc = G.ldc;
  const bool RELU = G.relu != 0;
  constexpr int WAVES_M = BM / 32;            // 4 or 2
  constexpr int WAVES_N = 8 / WAVES_M;        // 2 or 4
  constexpr int NT = 4 / WAVES_N;             // 32-column MFMA tiles per wave: 2 or 1
  constexpr int AQ = BM / 64;                 // float4 of A per thread and stage (BM rows x 8 float4 / 512 threads)
  constexpr int kStageElems = 3 * BM * kPitch + 3 * kBN * kPitch;
  __shared__ __attribute__((aligned(16))) __bf16 sbase[kStageElems];
  __bf16* sA = sbase;
  __bf16* sW = sbase + 3 * BM * kPitch;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WAVES_N, wn = wave % WAVES_N;
  const int li = lane & 31, hf = lane >> 5;
  const int nk = K / kBK;

  // global -> register mapping of one stage
  //   A: BM x 8 float4, thread t takes idx = t + 512 q: row = idx >> 3, c4 = idx & 7
  //   W: 1536 16-byte chunks of the contiguous stage block, thread t takes idx = t + 512 q
  const float* arow[AQ];
#pragma unroll
  for (int q = 0; q < AQ; ++q) {
    const int idx = tid + 512 * q;
    const int row = min(m0 + (idx >> 3), M - 1);
    arow[q] = A + (size_t)row * lda + 4 * (idx & 7);
  }
  const char* wblk = w_stage0(Wt, nb, nk, tid);
  const bool has_pos = G.pos != nullptr;   // uniform per workgroup
  const float* prow[AQ];
#pragma unroll
  for (int q = 0; q < AQ; ++q) {
    const int idx = tid + 512 * q;
    const int row = min(m0 + (idx >> 3), M - 1);
    prow[q] = has_pos ? G.pos + (size_t)(row % G.pos_rows) * K + 4 * (idx & 7) : arow[q];
  }

  f32x4v ra[AQ], rp[AQ], rw[3];
  auto issue = [&](int s) {
#pragma unroll
    for (int q = 0; q < AQ; ++q) ra[q] = gload(arow[q] + s * kBK);
    if (has_pos) {
#pragma unroll
      for (int q = 0; q < AQ; ++q) rp[q] = gload(prow[q] + s * kBK);
    }
    issue_w(rw, wblk, s);
  };
  auto stash = [&]() {
    vm_wait0(ra);
    vm_wait0(rw);
    if (has_pos) {
#pragma unroll
      for (int q = 0; q < AQ; ++q) {
        vm_wait0(rp[q]);
        ra[q] += rp[q];
      }
    }
#pragma unroll
    for (int q = 0; q < AQ; ++q) {
      const int idx = tid + 512 * q;
      stash_a4(sA + (idx >> 3) * kPitch + 4 * (idx & 7), ra[q], BM * kPitch);
    }
    stash_w(sW, rw, tid);
  };

  f32x16 acc[NT];
#pragma unroll
  for (int a = 0; a < NT; ++a)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[a][r] = 0.f;

  const __bf16* pa = sA + (wm * 32 + li) * kPitch + 8 * hf;
  const __bf16* pw = sW + (wn * (32 * NT) + li) * kPitch + 8 * hf;
  staged_loop(nk, issue, [&]() { stage_product<NT, BM>(pa, pw, acc); }, stash);

  // epilogue: D[i = n][j = m]; accumulator r <-> column n = (r & 3) + 8 (r >> 2) + 4 hf of the 32-wide n tile, row m =
  // lane & 31: one float4 (4 consecutive columns) per accumulator quad
  const int row = m0 + wm * 32 + li;
  const bool in_range = row < M;
  const bool keep = in_range && (G.row_keep == nullptr || G.row_keep[row] != 0);
  const float* __restrict__ relu_ref = G.relu_ref;
  const float* add1 = G.add1;
  const float* add2 = G.add2;
  float* __restrict__ colpart = G.colpart;
#pragma unroll
  for (int nt = 0; nt < NT; ++nt)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int col = nb * kBN + wn * (32 * NT) + nt * 32 + 8 * q + 4 * hf;
      float4 bv = make_float4(0.f, 0.f, 0.f, 0.f);
      if (bias != nullptr) bv = *reinterpret_cast<const float4*>(bias + col);
      float4 v = make_float4(acc[nt][4 * q + 0] + bv.x, acc[nt][4 * q + 1] + bv.y, acc[nt][4 * q + 2] + bv.z,
                             acc[nt][4 * q + 3] + bv.w);
      if (RELU) v = make_float4(egtr_relu(v.x), egtr_relu(v.y), egtr_relu(v.z), egtr_relu(v.w));
      if (!keep) v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (relu_ref != nullptr && in_range) {
        const float4 t = *reinterpret_cast<const float4*>(relu_ref + (size_t)row * G.ldref + col);
        v = make_float4(t.x > 0.f ? v.x : 0.f, t.y > 0.f ? v.y : 0.f, t.z > 0.f ? v.z : 0.f, t.w > 0.f ? v.w : 0.f);
      }
      if (add1 != nullptr && in_range) {
        const float4 t = *reinterpret_cast<const float4*>(add1 + (size_t)row * G.ldadd + col);
        v = make_float4(v.x + t.x, v.y + t.y, v.z + t.z, v.w + t.w);
      }
      if (add2 != nullptr && in_range) {
        const float4 t = *reinterpret_cast<const float4*>(add2 + (size_t)row * G.ldadd + col);
        v = make_float4(v.x + t.x, v.y + t.y, v.z + t.z, v.w + t.w);
      }
      if (in_range) *reinterpret_cast<float4*>(C + (size_t)row * ldc + col) = v;
      if (colpart != nullptr) {   // uniform per workgroup: sum over the wave's 32 rows (the 32 lanes that share hf)
        float4 s = in_range ? v : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int o = 1; o < 32; o <<= 1) {
          s.x += __shfl_xor(s.x, o);
          s.y += __shfl_xor(s.y, o);
          s.z += __shfl_xor(s.z, o);
          s.w += __shfl_xor(s.w, o);
        }
        // (a 32-row block that starts at or beyond M does not exist in the [ceil(M / 32), N] buffer)
        if (li == 0 && m0 + wm * 32 < M) *reinterpret_cast<float4*>(colpart + (size_t)((m0 >> 5) + wm) * G.N + col) = s;
      }
    }
}

// ---- the one-term counterpart: matmul precision "bf16" of the training routes (ops.set_matmul_precision) ----
// Each operand is rounded ONCE to bf16, round to nearest even: the fp32 activations (after the on-load `+ pos`) by
// v_cvt_pk_bf16_f32 on their way into LDS, the weights by the one-piece tiling launches below.  One MFMA per k-step instead of
// six, fp32 accumulation, the same tiles, grouping and epilogue.  Inf and NaN survive the rounding (a non-finite activation makes
// its output row non-finite and nothing else); a finite value beyond the largest bf16 (3.39e38) rounds to Inf.
// The weight stream is [N/128][K/32][128 rows][32] bf16: 8 KiB blocks, consecutive in k for one n block, so that the stage depth
// is the kernel's own choice.  A stage is BK = kR1StageK columns of k where K allows, else 32 (K % 32 == 0 is all the entry
// asks, like the six-term one): with one piece an LDS stage of depth 32 is 20 KiB and its two barriers no longer hide behind six
// MFMAs per k-step (DESIGN.md 4.12b has the measurements).  LDS rows are BK + 8 elements apart (80 / 144 / 272 bytes): the 16-byte
// operand reads of 16 consecutive rows fall on 16 different bank quads.
#ifndef EGTR_BF16R_STAGE_K
#define EGTR_BF16R_STAGE_K 64
#endif
#ifndef EGTR_BF16R_STAGE_M
#define EGTR_BF16R_STAGE_M 32
#endif
constexpr int kR1StageK = EGTR_BF16R_STAGE_K;   // forward / data gradient: 32, 64 or 128
constexpr int kR1StageM = EGTR_BF16R_STAGE_M;   // weight gradient (rows of the reduction per stage): 32 or 64
// Measured (tools/matmul_precision_bench.py on builds with other -DEGTR_BF16R_STAGE_K / _M, profiles/matmul_precision_stage_ablation.txt;
// sum of the twelve training-size launches, six-term 1407-1445 us): K 32 / M 32: 649 us; K 64 / M 32: 613 us (taken); K 128 spills
// 87 registers in the 128-row form and is slower than the six-term kernel; M 64 makes every weight gradient 1.8-2.6 x SLOWER than
// M 32 (55 vs 30 us at 256 x 256) and its EXT form spills.  The macros stay for such builds; the masked weight gradient is 32 always.
constexpr int kR1StageMExt = 32;
static_assert(kR1StageK == 32 || kR1StageK == 64 || kR1StageK == 128, "stage depth");
static_assert(kR1StageM == 32 || kR1StageM == 64, "stage depth");
constexpr int kR1WBlockBytes = 2 * kBN * 32;

using xs::cvt_pk_bf16_rne;   // two fp32 -> one dword of two bf16, round to nearest even (xs_format.h; rel_head.hip shares it)
// one stage out of LDS: BK / 16 k-steps x (1 + NT) 16-byte reads and one product per 32-column tile of the wave
template <int NT, int BK>
__device__ __forceinline__ void stage_product1(const __bf16* pa, const __bf16* pw, f32x16 (&acc)[NT]) {
  constexpr int pitch = BK + 8;
#pragma unroll
  for (int ks = 0; ks < BK / 16; ++ks) {
    const bf16x8 a = *reinterpret_cast<const bf16x8*>(pa + 16 * ks);
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = mfma(*reinterpret_cast<const bf16x8*>(pw + t * 32 * pitch + 16 * ks), a, acc[t]);
  }
}

template <int BM, int BK>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(4, 4))) void gemm_bf16r_f32(GemmProblems P, int nprob, int M,
                                                                                                  int K) {
  const int mblocks = (M + BM - 1) / BM;
  int tile = xcd_tile(blockIdx.x, gridDim.x), pi = 0;
  for (; pi + 1 < nprob; ++pi) {
    const int t = (P.p[pi].N / kBN) * mblocks;
    if (tile < t) break;
    tile -= t;
  }
  const GemmProblem& G = P.p[pi];
  const int nblocks = G.N / kBN;
  const int nb = tile % nblocks, m0 = (tile / nblocks) * BM;
  const float* __restrict__ A = G.A;
  const int lda = G.lda;
  constexpr int WAVES_M = BM / 32, WAVES_N = 8 / WAVES_M, NT = 4 / WAVES_N;
  constexpr int C4 = BK / 4;            // float4 per row of A and stage
  constexpr int AQ = BM * C4 / 512;     // float4 of A per thread and stage
  constexpr int WQ = BK / 32;           // weight blocks per stage = 16-byte chunks of W per thread and stage
  constexpr int pitch = BK + 8;
  __shared__ __attribute__((aligned(16))) __bf16 sbase[(BM + kBN) * pitch];
  __bf16* sA = sbase;
  __bf16* sW = sbase + BM * pitch;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WAVES_N, wn = wave % WAVES_N;
  const int li = lane & 31, hf = lane >> 5;
  const int nk = K / BK;

  // A: BM x C4 float4 per stage, thread t takes idx = t + 512 q: row = idx / C4, c4 = idx % C4
  // W: WQ blocks of 512 16-byte chunks [row 128][4 chunks of 8 bf16]; thread t takes chunk t of each block
  const float* arow[AQ];
  const float* prow[AQ];
  const bool has_pos = G.pos != nullptr;   // uniform per workgroup
#pragma unroll
  for (int q = 0; q < AQ; ++q) {
    const int idx = tid + 512 * q;
    const int row = min(m0 + idx / C4, M - 1);
    arow[q] = A + (size_t)row * lda + 4 * (idx % C4);
    prow[q] = has_pos ? G.pos + (size_t)(row % G.pos_rows) * K + 4 * (idx % C4) : arow[q];
  }
  const char* wblk = reinterpret_cast<const char*>(G.Wt) + (size_t)nb * (K / 32) * kR1WBlockBytes + (size_t)tid * 16;

  f32x4v ra[AQ], rp[AQ], rw[WQ];
  auto issue = [&](int s) {
#pragma unroll
    for (int q = 0; q < AQ; ++q) ra[q] = gload(arow[q] + s * BK);
    if (has_pos) {
#pragma unroll
      for (int q = 0; q < AQ; ++q) rp[q] = gload(prow[q] + s * BK);
    }
#pragma unroll
    for (int q = 0; q < WQ; ++q) rw[q] = gload(wblk + (size_t)(s * WQ + q) * kR1WBlockBytes);
  };
  auto stash = [&]() {
    vm_wait0(ra);
    vm_wait0(rw);
    if (has_pos) {
#pragma unroll
      for (int q = 0; q < AQ; ++q) {
        vm_wait0(rp[q]);
        ra[q] += rp[q];
      }
    }
#pragma unroll
    for (int q = 0; q < AQ; ++q) {
      const int idx = tid + 512 * q;
      *reinterpret_cast<uint2*>(sA + (idx / C4) * pitch + 4 * (idx % C4)) =
          make_uint2(cvt_pk_bf16_rne(ra[q].x, ra[q].y), cvt_pk_bf16_rne(ra[q].z, ra[q].w));
    }
#pragma unroll
    for (int q = 0; q < WQ; ++q) *reinterpret_cast<f32x4v*>(sW + (tid >> 2) * pitch + 32 * q + 8 * (tid & 3)) = rw[q];
  };

  f32x16 acc[NT];
#pragma unroll
  for (int a = 0; a < NT; ++a)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[a][r] = 0.f;

  const __bf16* pa = sA + (wm * 32 + li) * pitch + 8 * hf;
  const __bf16* pw = sW + (wn * (32 * NT) + li) * pitch + 8 * hf;
  staged_loop(nk, issue, [&]() { stage_product1<NT, BK>(pa, pw, acc); }, stash);

  gemm_epilogue<NT>(G, acc, M, nb, m0, wm, wn, li, hf);
}

}  // namespace

namespace {
// pieces: 3 = the six-term kernel on the three-piece weight stream, 1 = the one-term kernel on the one-piece stream
int launch_grouped(hipStream_t st, const GemmProblems& P, int nprob, int M, int K, int pieces = 3) {
  long long tiles128 = 0, tiles64 = 0;
  for (int i = 0; i < nprob; ++i) {
    tiles128 += (long long)(P.p[i].N / kBN) * ((M + 127) / 128);
    tiles64 += (long long)(P.p[i].N / kBN) * ((M + 63) / 64);
  }
  if (tiles64 >= (1ll << 31)) return EGTR_E_UNSUPPORTED;
  // 128-row tiles when they fill the chip twice over (two co-resident workgroups per CU overlap each other's load /
  // store phases), 64-row tiles otherwise.  (128-row tiles for the K = 1024 product too measured 46.0 vs 53.0 us stand-alone
  // but 262.6 vs 264.5 images/s in the forward, same box, alternating builds: not taken; again with the XCD-aware tile
  // order: 259.0 vs 262.8 / 261.5 images/s.)
  // Round 4: "fill the chip twice over" relaxed to 480 of the 512 workgroup slots.  The encoder layer's grouped launch at 600x1000
  // (value 256 -> 256 + offsets / weights 256 -> 384, M = 12 537) has 490 128-row tiles = 980 64-row tiles: one nearly full round
  // of the larger tiles beats 1.91 rounds of the smaller ones -- 42.9 -> 37.2 us per launch, 281.9 -> 284.7 images/s end to end
  // (three alternations on one box, abl/infer_ab.sh).
  if (pieces == 1) {   // the same tile-height rule; the deep stage where K is a multiple of it
    const bool deep = K % kR1StageK == 0;
    const dim3 grid((unsigned)(tiles128 >= 480 ? tiles128 : tiles64));
    if (tiles128 >= 480 && deep)
      hipLaunchKernelGGL((gemm_bf16r_f32<128, kR1StageK>), grid, dim3(512), 0, st, P, nprob, M, K);
    else if (tiles128 >= 480)
      hipLaunchKernelGGL((gemm_bf16r_f32<128, 32>), grid, dim3(512), 0, st, P, nprob, M, K);
    else if (deep)
      hipLaunchKernelGGL((gemm_bf16r_f32<64, kR1StageK>), grid, dim3(512), 0, st, P, nprob, M, K);
    else
      hipLaunchKernelGGL((gemm_bf16r_f32<64, 32>), grid, dim3(512), 0, st, P, nprob, M, K);
    return egtr_check_launch();
  }
  if (tiles128 >= 480)
    hipLaunchKernelGGL(gemm_split_bf16_f32<128>, dim3((unsigned)tiles128), dim3(512), 0, st, P, nprob, M, K);
  else
    hipLaunchKernelGGL(gemm_split_bf16_f32<64>, dim3((unsigned)tiles64), dim3(512), 0, st, P, nprob, M, K);
  return egtr_check_launch();
}
bool problem_ok(const float* x, int ldx, const uint16_t* w, const float* bias, float* y, int ldy, int K, int N) {
  return x && w && y && ldx >= K && ldy >= N && N > 0 && N % kBN == 0 && !(ldx & 3) && !(ldy & 3) &&
         !(reinterpret_cast<uintptr_t>(x) & 15) && !(reinterpret_cast<uintptr_t>(y) & 15) &&
         !(bias && (reinterpret_cast<uintptr_t>(bias) & 15));
}
// ---- weight gradient of a token-sized linear layer: gw[n][k] = sum_m g[m][n] x[m][k] (M ~ 50 000 rows, N, K a few
// hundred) with the same six-term split arithmetic.  Both operands arrive "reduction-major" (m is the slow index), so the
// transpose happens on the way in: a thread loads 8 consecutive rows m of ONE column (dword loads, a wave covers 64
// consecutive columns = 256 contiguous bytes per row), splits them and stores the 8 bf16 of a piece as one 16-byte LDS
// row segment -- LDS then holds [column][m] tiles exactly like the forward kernel's [row][k] tiles and the MFMA part is
// the same.  The M rows are cut into chunks (split-K) so that (N/128)(K/128) x chunks workgroups fill the chip; every
// workgroup writes its 128 x 128 partial to the workspace and wgrad_reduce_f32 sums the chunks in a fixed order.
// MFMA roles: A operand = x piece (i = k), B operand = g piece (j = n): float4 stores along k of the row-major [N, K]
// result.
// EXT: `xpos` (optional, [pos_rows, K]): x[m] + xpos[m % pos_rows] is the operand (the layer's input was `hidden + pos`, added
// on load in the forward too); `row_keep` (optional, [M] bytes): rows of g with 0 count as zero rows (padded tokens).  A
// template parameter, not a runtime test: with the tests in the load loop the plain kernel lost its batched loads (80 launches
// per train step: 4.1 -> 5.0 ms).
template <bool EXT>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(4, 4))) void wgrad_split_bf16_f32(
    const float* __restrict__ G, int ldg, const float* __restrict__ X, int ldx, float* __restrict__ partial, int M, int N,
    int K, int rows_per_chunk, const float* __restrict__ xpos, int pos_rows, const unsigned char* __restrict__ row_keep) {
  constexpr int BM = 128;
  const int ktiles = K / kBN, tiles = (N / BM) * ktiles;
  const int lb = xcd_tile(blockIdx.x, gridDim.x);
  const int chunk = lb / tiles, t = lb - chunk * tiles;
  const int n0 = (t / ktiles) * BM, k0 = (t % ktiles) * kBN;
  const int mbeg = chunk * rows_per_chunk, mend = min(M, mbeg + rows_per_chunk);
  const int nstage = (mend - mbeg + kBK - 1) / kBK;
  __shared__ __attribute__((aligned(16))) __bf16 sG[3 * BM * kPitch];
  __shared__ __attribute__((aligned(16))) __bf16 sX[3 * kBN * kPitch];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;     // 4 x 2 waves: 32 rows (n) x 64 columns (k) each
  const int li = lane & 31, hf = lane >> 5;
  const int col = tid & 127, mq = tid >> 7;    // loader: column of the tile, rows 8 mq .. 8 mq + 7 of the stage
  const float* gp = G + n0 + col;
  const float* xp = X + k0 + col;
  const float* pp = (EXT && xpos != nullptr) ? xpos + k0 + col : nullptr;

  float rg[8], rx[8];
  auto issue = [&](int s) {
    const int m = mbeg + s * kBK + mq * 8;
    if constexpr (EXT) {
      float rp[8];
      unsigned char rk[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {   // all loads of the stage first (no test between them), then the arithmetic
        const bool ok = m + e < mend;
        const unsigned r = (unsigned)(ok ? m + e : mbeg);
        rg[e] = gp[(size_t)r * ldg];
        rx[e] = xp[(size_t)r * ldx];
        rp[e] = pp != nullptr ? pp[(size_t)(r % (unsigned)pos_rows) * K] : 0.f;
        rk[e] = row_keep != nullptr ? row_keep[r] : (unsigned char)1;
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const bool ok = m + e < mend;
        rg[e] = (ok && rk[e] != 0) ? rg[e] : 0.f;
        rx[e] = ok ? rx[e] + rp[e] : 0.f;
      }
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const bool ok = m + e < mend;
        const size_t r = (size_t)(ok ? m + e : mbeg);
        const float a = gp[r * ldg], b = xp[r * ldx];
        rg[e] = ok ? a : 0.f;
        rx[e] = ok ? b : 0.f;
      }
    }
  };
  // eight reduction rows of one column -> three 16-byte LDS row segments, one per piece
  auto stash_one = [&](const float (&v)[8], __bf16* base) {
    xs::Split3 sp[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) sp[e] = xs::split3_fast(v[e]);
    __bf16* p = base + col * kPitch + mq * 8;
    *reinterpret_cast<uint4*>(p) = make_uint4(xs::pack_hi16(sp[0].hi, sp[1].hi), xs::pack_hi16(sp[2].hi, sp[3].hi),
                                              xs::pack_hi16(sp[4].hi, sp[5].hi), xs::pack_hi16(sp[6].hi, sp[7].hi));
    *reinterpret_cast<uint4*>(p + BM * kPitch) =
        make_uint4(xs::pack_hi16(sp[0].mid, sp[1].mid), xs::pack_hi16(sp[2].mid, sp[3].mid), xs::pack_hi16(sp[4].mid, sp[5].mid),
                   xs::pack_hi16(sp[6].mid, sp[7].mid));
    *reinterpret_cast<uint4*>(p + 2 * BM * kPitch) =
        make_uint4(xs::pack_hi16(sp[0].lo, sp[1].lo), xs::pack_hi16(sp[2].lo, sp[3].lo), xs::pack_hi16(sp[4].lo, sp[5].lo),
                   xs::pack_hi16(sp[6].lo, sp[7].lo));
  };
  auto stash = [&]() {
    stash_one(rg, sG);
    stash_one(rx, sX);
  };

  f32x16 acc[2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[a][r] = 0.f;

  const __bf16* pa = sG + (wm * 32 + li) * kPitch + 8 * hf;
  const __bf16* pw = sX + (wn * 64 + li) * kPitch + 8 * hf;
  // This kernel keeps its own copy of x6::staged_loop and of the stash: routed through the shared ones its instruction stream
  // changed (the other two kernels' did too, within their parents' run-to-run spread) and every weight gradient measured 0.3-0.4 us
  // (1 %) slower, outside that spread (profiles/x6_staged_refactor.txt).  As written here the stream is the earlier one, bit for bit.
  auto compute = [&]() { stage_product<2, BM>(pa, pw, acc); };
  if (nstage > 0) {
    issue(0);
    stash();
    __syncthreads();
#pragma unroll 1
    for (int s = 0; s + 1 < nstage; ++s) {
      issue(s + 1);
      compute();
      __syncthreads();   // every wave has read stage s out of LDS
      stash();
      __syncthreads();
    }
    compute();
  }
  // D[i = k][j = n]: accumulator r <-> k = (r & 3) + 8 (r >> 2) + 4 hf of the 32-wide k tile, n = lane & 31
  float* out = partial + ((size_t)chunk * N + n0 + wm * 32 + li) * K + k0 + wn * 64 + 4 * hf;
#pragma unroll
  for (int nt = 0; nt < 2; ++nt)
#pragma unroll
    for (int q = 0; q < 4; ++q)
      *reinterpret_cast<float4*>(out + nt * 32 + 8 * q) =
          make_float4(acc[nt][4 * q + 0], acc[nt][4 * q + 1], acc[nt][4 * q + 2], acc[nt][4 * q + 3]);
}

// The one-term counterpart (matmul precision "bf16"): both operands rounded once to bf16 (RNE, v_cvt_pk_bf16_f32; x after the
// on-load `+ xpos`) on their way into LDS, one MFMA per k-step.  Same tiles, split-K chunks, workspace layout and fixed-order
// reduction; a stage is BK = kR1StageM rows of the reduction: each thread transposes BK / 32 groups of 8 rows of its column.
template <bool EXT, int BK>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(4, 4))) void wgrad_bf16r_f32(
    const float* __restrict__ G, int ldg, const float* __restrict__ X, int ldx, float* __restrict__ partial, int M, int N,
    int K, int rows_per_chunk, const float* __restrict__ xpos, int pos_rows, const unsigned char* __restrict__ row_keep) {
  constexpr int BM = 128, R = BK / 32, pitch = BK + 8;
  const int ktiles = K / kBN, tiles = (N / BM) * ktiles;
  const int lb = xcd_tile(blockIdx.x, gridDim.x);
  const int chunk = lb / tiles, t = lb - chunk * tiles;
  const int n0 = (t / ktiles) * BM, k0 = (t % ktiles) * kBN;
  const int mbeg = chunk * rows_per_chunk, mend = min(M, mbeg + rows_per_chunk);
  const int nstage = (mend - mbeg + BK - 1) / BK;
  __shared__ __attribute__((aligned(16))) __bf16 sG[BM * pitch];
  __shared__ __attribute__((aligned(16))) __bf16 sX[kBN * pitch];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;     // 4 x 2 waves: 32 rows (n) x 64 columns (k) each
  const int li = lane & 31, hf = lane >> 5;
  const int col = tid & 127, mq = tid >> 7;    // loader: column of the tile, rows 8 (mq + 4 h) .. + 7 of the stage, h < R
  const float* gp = G + n0 + col;
  const float* xp = X + k0 + col;
  const float* pp = (EXT && xpos != nullptr) ? xpos + k0 + col : nullptr;

  float rg[8 * R], rx[8 * R];
  auto issue = [&](int s) {
#pragma unroll
    for (int h = 0; h < R; ++h) {
      const int m = mbeg + s * BK + (mq + 4 * h) * 8;
      if constexpr (EXT) {
        float rp[8];
        unsigned char rk[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {   // all loads of the group first (no test between them), then the arithmetic
          const bool ok = m + e < mend;
          const unsigned r = (unsigned)(ok ? m + e : mbeg);
          rg[8 * h + e] = gp[(size_t)r * ldg];
          rx[8 * h + e] = xp[(size_t)r * ldx];
          rp[e] = pp != nullptr ? pp[(size_t)(r % (unsigned)pos_rows) * K] : 0.f;
          rk[e] = row_keep != nullptr ? row_keep[r] : (unsigned char)1;
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const bool ok = m + e < mend;
          rg[8 * h + e] = (ok && rk[e] != 0) ? rg[8 * h + e] : 0.f;
          rx[8 * h + e] = ok ? rx[8 * h + e] + rp[e] : 0.f;
        }
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const bool ok = m + e < mend;
          const size_t r = (size_t)(ok ? m + e : mbeg);
          const float a = gp[r * ldg], b = xp[r * ldx];
          rg[8 * h + e] = ok ? a : 0.f;
          rx[8 * h + e] = ok ? b : 0.f;
        }
      }
    }
  };
  // eight reduction rows of one column -> one 16-byte LDS row segment
  auto stash_one = [&](const float (&v)[8 * R], __bf16* base) {
#pragma unroll
    for (int h = 0; h < R; ++h)
      *reinterpret_cast<uint4*>(base + col * pitch + (mq + 4 * h) * 8) =
          make_uint4(cvt_pk_bf16_rne(v[8 * h + 0], v[8 * h + 1]), cvt_pk_bf16_rne(v[8 * h + 2], v[8 * h + 3]),
                     cvt_pk_bf16_rne(v[8 * h + 4], v[8 * h + 5]), cvt_pk_bf16_rne(v[8 * h + 6], v[8 * h + 7]));
  };
  auto stash = [&]() {
    stash_one(rg, sG);
    stash_one(rx, sX);
  };

  f32x16 acc[2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[a][r] = 0.f;

  const __bf16* pa = sG + (wm * 32 + li) * pitch + 8 * hf;
  const __bf16* pw = sX + (wn * 64 + li) * pitch + 8 * hf;
  if (nstage > 0) staged_loop(nstage, issue, [&]() { stage_product1<2, BK>(pa, pw, acc); }, stash);
  // D[i = k][j = n]: accumulator r <-> k = (r & 3) + 8 (r >> 2) + 4 hf of the 32-wide k tile, n = lane & 31
  float* out = partial + ((size_t)chunk * N + n0 + wm * 32 + li) * K + k0 + wn * 64 + 4 * hf;
#pragma unroll
  for (int nt = 0; nt < 2; ++nt)
#pragma unroll
    for (int q = 0; q < 4; ++q)
      *reinterpret_cast<float4*>(out + nt * 32 + 8 * q) =
          make_float4(acc[nt][4 * q + 0], acc[nt][4 * q + 1], acc[nt][4 * q + 2], acc[nt][4 * q + 3]);
}

// out[i] = sum over chunks of partial[c][i] (float4 columns; 16 columns x 16 chunk lanes per workgroup, fixed order)
__global__ __launch_bounds__(256) void wgrad_reduce_f32(const float4* __restrict__ partial, int chunks, int n4,
                                                        float4* __restrict__ out) {
  __shared__ float4 sm[256];
  const int cl = threadIdx.x & 15, kl = threadIdx.x >> 4;
  const int c = blockIdx.x * 16 + cl;
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
  if (c < n4) {
#pragma unroll 4
    for (int k = kl; k < chunks; k += 16) {
      const float4 v = partial[(size_t)k * n4 + c];
      s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
  }
  sm[threadIdx.x] = s;
  __syncthreads();
  if (kl == 0 && c < n4) {
#pragma unroll
    for (int k = 1; k < 16; ++k) {
      const float4 v = sm[k * 16 + cl];
      s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
    out[c] = s;
  }
}

struct WgradPlan {
  int chunks, rows_per_chunk;
};
WgradPlan wgrad_plan(int M, int N, int K, int bk = kBK) {   // bk: rows of the reduction per stage
  const int tiles = (N / 128) * (K / 128);
  // two workgroups per CU; measured for 256 x 256 / 256 x 1024 over 50 148 rows with 256 / 384 / 512 / 768 / 1024 / 1536
  // workgroups: 53.6 / 56.4 / 53.2 / 59.8 / 64.4 / 69.8 us and 181.8 / 190.4 / 175.5 / 181.6 / 183.7 / 192.7 us
  int chunks = std::max(1, (512 + tiles - 1) / tiles);
  chunks = std::min(chunks, (M + bk - 1) / bk);
  const int rpc = ((M + chunks - 1) / chunks + bk - 1) / bk * bk;
  return WgradPlan{(M + rpc - 1) / rpc, rpc};
}

// W [N, K] fp32 (or its transpose: `transposed`, element (n, k) at w[k * ldw + n]) -> the operand stream of the kernel
// above, [N/128][K/32][3 pieces][128][32] bf16.  Pieces are rounded to nearest even like ops._split3_bf16 (the residuals
// stay exact in fp32); one thread per element, consecutive threads along k of one row -> 64-byte output segments.
// Thread idx of a [N, K] weight takes element (k = idx & 31, n = (idx >> 5) & 127) of stage block idx >> 12: returns the slot
// of its hi piece in the stream, (n, k) the element's place in the weight.
template <int PIECES>
__device__ __forceinline__ unsigned short* tiled_slot(unsigned short* out, int idx, int K, int& n, int& k) {
  const int kk = idx & 31, nn = (idx >> 5) & 127, blk = idx >> 12;
  const int ktiles = K / kBK;
  n = (blk / ktiles) * kBN + nn;
  k = (blk % ktiles) * kBK + kk;
  return out + (size_t)blk * (PIECES * kWPieceElems) + nn * kBK + kk;
}
// (xs::bf16_rne_bits, not xs::split3_rne: a non-finite weight keeps the NaN residuals inf - inf it always had here)
template <int PIECES>
__device__ __forceinline__ void store_split_rne(unsigned short* o, float x) {
  const unsigned hi = xs::bf16_rne_bits(x);
  if constexpr (PIECES == 1) {   // the one-piece stream of the one-term kernels: the element rounded once
    o[0] = (unsigned short)(hi >> 16);
    return;
  }
  const float r1 = x - __uint_as_float(hi);
  const unsigned mid = xs::bf16_rne_bits(r1);
  const unsigned lo = xs::bf16_rne_bits(r1 - __uint_as_float(mid));
  o[0] = (unsigned short)(hi >> 16);
  o[kWPieceElems] = (unsigned short)(mid >> 16);
  o[2 * kWPieceElems] = (unsigned short)(lo >> 16);
}
// `pair`: the second half of the grid writes the tiling of W^T behind the first one (out + 3 N K), so that the forward
// of a training step prepares the operand of its data-gradient product in the same launch.
template <int PIECES>
__global__ __launch_bounds__(256) void tile_weights_f32(const float* __restrict__ w, int ldw, int transposed, int N, int K,
                                                        unsigned short* __restrict__ out, int pair) {
  int idx = blockIdx.x * 256 + threadIdx.x;
  if (pair && idx >= N * K) {   // W^T [K, N] read in place
    idx -= N * K;
    out += (size_t)PIECES * N * K;
    transposed = 1;
    const int t = N;
    N = K;
    K = t;
  }
  if (idx >= N * K) return;
  int n, k;
  unsigned short* o = tiled_slot<PIECES>(out, idx, K, n, k);
  store_split_rne<PIECES>(o, transposed ? w[(size_t)k * ldw + n] : w[(size_t)n * ldw + k]);
}

// Several weights in ONE launch (a training step re-tiles every encoder weight after each optimizer step: 5 launches + 2
// concatenations per layer before): problem i = the pair tiling (W and W^T) of a [N_i, K_i] weight whose first `split` rows come
// from w and the rest from w2 (the offsets | attention-weights projection as one [384, 256] weight without a materialised cat).
constexpr int kMaxTileProblems = 8;
struct TileProblem {
  const float* w;
  const float* w2;
  unsigned short* out;
  int ldw, ldw2, split, N, K, first_block;
};
struct TileProblems {
  TileProblem p[kMaxTileProblems];
};
template <int PIECES>
__global__ __launch_bounds__(256) void tile_weights_multi_f32(TileProblems P, int nprob) {
  int pi = 0;
  while (pi + 1 < nprob && (int)blockIdx.x >= P.p[pi + 1].first_block) ++pi;
  const TileProblem& T = P.p[pi];
  int idx = ((int)blockIdx.x - T.first_block) * 256 + threadIdx.x;
  int N = T.N, K = T.K;
  unsigned short* out = T.out;
  const bool transposed = idx >= N * K;   // second half: the tiling of W^T [K, N] behind the first one
  if (transposed) {
    idx -= N * K;
    out += (size_t)PIECES * N * K;
    const int t = N;
    N = K;
    K = t;
  }
  if (idx >= N * K) return;
  int n, k;
  unsigned short* o = tiled_slot<PIECES>(out, idx, K, n, k);
  const int r = transposed ? k : n, c = transposed ? n : k;   // element (r, c) of the untransposed weight
  store_split_rne<PIECES>(o, r < T.split ? T.w[(size_t)r * T.ldw + c] : T.w2[(size_t)(r - T.split) * T.ldw2 + c]);
}

}  // namespace

// `terms`, the trailing argument of every entry below but the scalar forward: which arithmetic runs.  6: the six exact cross
// terms on the three-piece weight stream; 1: one product per element, operands rounded once to bf16, on the one-piece stream.
// Anything else is an argument error (0 pieces), answered before any HIP call.
static int pieces_of(int terms) { return terms == 6 ? 3 : terms == 1 ? 1 : 0; }

extern "C" int egtr_gemm_split_tile_weights_multi_f32(egtr_stream_t stream, int num_weights, const float* const* w,
                                                      const int* ldw, const float* const* w2, const int* ldw2,
                                                      const int* split_rows, const int* N, const int* K,
                                                      uint16_t* const* w_tiled_pair, int terms) {
  const int pieces = pieces_of(terms);
  if (!pieces) return EGTR_E_ARG;
  if (!w || !ldw || !N || !K || !w_tiled_pair || num_weights <= 0 || num_weights > kMaxTileProblems) return EGTR_E_ARG;
  TileProblems P = {};
  long long blocks = 0;
  for (int i = 0; i < num_weights; ++i) {
    const float* second = w2 != nullptr ? w2[i] : nullptr;
    const int split = second != nullptr ? split_rows[i] : N[i];
    if (!w[i] || !w_tiled_pair[i] || N[i] <= 0 || K[i] <= 0 || ldw[i] < K[i] || split <= 0 || split > N[i] ||
        (second != nullptr && (!ldw2 || ldw2[i] < K[i])))
      return EGTR_E_ARG;
    if (N[i] % kBN != 0 || K[i] % kBN != 0 || (long long)N[i] * K[i] > (1LL << 29)) return EGTR_E_UNSUPPORTED;
    P.p[i] = TileProblem{w[i], second, reinterpret_cast<unsigned short*>(w_tiled_pair[i]), ldw[i], second ? ldw2[i] : 0, split,
                         N[i], K[i], (int)blocks};
    blocks += 2 * ((long long)N[i] * K[i] / 256);
  }
  if (blocks >= (1ll << 31)) return EGTR_E_UNSUPPORTED;
  if (pieces == 1)
    hipLaunchKernelGGL(tile_weights_multi_f32<1>, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream), P,
                       num_weights);
  else
    hipLaunchKernelGGL(tile_weights_multi_f32<3>, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream), P,
                       num_weights);
  return egtr_check_launch();
}

// The single-problem, scalar-argument form of inference (six terms): no host arrays to build on a host-bound forward.
extern "C" int egtr_linear_split_bf16_f32(egtr_stream_t stream, const float* x, int ldx, const uint16_t* w_tiled,
                                          const float* bias, float* y, int ldy, int M, int K, int N, int relu) {
  if (!x || !w_tiled || !y) return EGTR_E_ARG;
  if (M <= 0 || K <= 0 || N <= 0 || ldx < K || ldy < N) return EGTR_E_ARG;
  if (K % kBK != 0 || !problem_ok(x, ldx, w_tiled, bias, y, ldy, K, N)) return EGTR_E_UNSUPPORTED;
  GemmProblems P = {};
  P.p[0] = GemmProblem{x, w_tiled, bias, y, ldx, ldy, N, relu, nullptr, 1, nullptr, nullptr, 0, nullptr, nullptr, 0, nullptr};
  return launch_grouped(static_cast<hipStream_t>(stream), P, 1, M, K);
}

extern "C" int egtr_linear_split_bf16_ex_f32(egtr_stream_t stream, int num_problems, const float* const* x, const int* ldx,
                                             const uint16_t* const* w_tiled, const float* const* bias, float* const* y,
                                             const int* ldy, const int* N, const int* relu, int M, int K,
                                             const float* const* pos, const int* pos_rows,
                                             const unsigned char* const* row_keep, const float* const* relu_ref,
                                             const int* ldref, const float* const* add1, const float* const* add2,
                                             const int* ldadd, float* const* colpart, int terms) {
  const int pieces = pieces_of(terms);
  if (!pieces) return EGTR_E_ARG;
  if (!x || !ldx || !w_tiled || !bias || !y || !ldy || !N || !relu) return EGTR_E_ARG;
  if (num_problems <= 0 || num_problems > kMaxProblems || M <= 0 || K <= 0) return EGTR_E_ARG;
  if ((pos != nullptr && pos_rows == nullptr) || (relu_ref != nullptr && ldref == nullptr) ||
      ((add1 != nullptr || add2 != nullptr) && ldadd == nullptr))
    return EGTR_E_ARG;
  if (K % kBK != 0) return EGTR_E_UNSUPPORTED;
  GemmProblems P = {};
  for (int i = 0; i < num_problems; ++i) {
    if (!x[i] || !w_tiled[i] || !y[i]) return EGTR_E_ARG;
    if (!problem_ok(x[i], ldx[i], w_tiled[i], bias[i], y[i], ldy[i], K, N[i])) return EGTR_E_UNSUPPORTED;
    const float* p = pos != nullptr ? pos[i] : nullptr;
    if (p != nullptr && pos_rows[i] <= 0) return EGTR_E_ARG;
    if (p != nullptr && (reinterpret_cast<uintptr_t>(p) & 15)) return EGTR_E_UNSUPPORTED;
    const float* rr = relu_ref != nullptr ? relu_ref[i] : nullptr;
    const float* a1 = add1 != nullptr ? add1[i] : nullptr;
    const float* a2 = add2 != nullptr ? add2[i] : nullptr;
    float* cp = colpart != nullptr ? colpart[i] : nullptr;
    if ((rr && (ldref[i] < N[i] || (ldref[i] & 3) || (reinterpret_cast<uintptr_t>(rr) & 15))) ||
        ((a1 || a2) && (ldadd[i] < N[i] || (ldadd[i] & 3))) || (reinterpret_cast<uintptr_t>(a1) & 15) ||
        (reinterpret_cast<uintptr_t>(a2) & 15) || (reinterpret_cast<uintptr_t>(cp) & 15))
      return EGTR_E_UNSUPPORTED;
    P.p[i] = GemmProblem{x[i], w_tiled[i], bias[i], y[i], ldx[i], ldy[i], N[i], relu[i], p, p != nullptr ? pos_rows[i] : 1,
                         row_keep != nullptr ? row_keep[i] : nullptr, rr, rr ? ldref[i] : 0, a1, a2,
                         (a1 || a2) ? ldadd[i] : 0, cp};
  }
  return launch_grouped(static_cast<hipStream_t>(stream), P, num_problems, M, K, pieces);
}

extern "C" int egtr_gemm_split_tile_weights_f32(egtr_stream_t stream, const float* w, int ldw, int transposed, int N, int K,
                                                uint16_t* w_tiled, int terms) {
  const int pieces = pieces_of(terms);
  if (!pieces) return EGTR_E_ARG;
  if (!w || !w_tiled || N <= 0 || K <= 0 || ldw < (transposed ? N : K)) return EGTR_E_ARG;
  if (N % kBN != 0 || K % kBK != 0 || (long long)N * K > (1LL << 30)) return EGTR_E_UNSUPPORTED;
  if (pieces == 1)
    hipLaunchKernelGGL(tile_weights_f32<1>, dim3(N * K / 256), dim3(256), 0, static_cast<hipStream_t>(stream), w, ldw,
                       transposed, N, K, reinterpret_cast<unsigned short*>(w_tiled), 0);
  else
    hipLaunchKernelGGL(tile_weights_f32<3>, dim3(N * K / 256), dim3(256), 0, static_cast<hipStream_t>(stream), w, ldw,
                       transposed, N, K, reinterpret_cast<unsigned short*>(w_tiled), 0);
  return egtr_check_launch();
}

extern "C" int egtr_gemm_split_tile_weights_pair_f32(egtr_stream_t stream, const float* w, int ldw, int N, int K,
                                                     uint16_t* w_tiled_pair, int terms) {
  const int pieces = pieces_of(terms);
  if (!pieces) return EGTR_E_ARG;
  if (!w || !w_tiled_pair || N <= 0 || K <= 0 || ldw < K) return EGTR_E_ARG;
  if (N % kBN != 0 || K % kBN != 0 || (long long)N * K > (1LL << 29)) return EGTR_E_UNSUPPORTED;
  if (pieces == 1)
    hipLaunchKernelGGL(tile_weights_f32<1>, dim3(2 * (N * K / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), w, ldw, 0,
                       N, K, reinterpret_cast<unsigned short*>(w_tiled_pair), 1);
  else
    hipLaunchKernelGGL(tile_weights_f32<3>, dim3(2 * (N * K / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), w, ldw, 0,
                       N, K, reinterpret_cast<unsigned short*>(w_tiled_pair), 1);
  return egtr_check_launch();
}

extern "C" long long egtr_linear_split_bf16_wgrad_workspace_floats(int M, int N, int K, int terms) {
  const int pieces = pieces_of(terms);
  if (!pieces || M <= 0 || N <= 0 || K <= 0 || N % 128 || K % 128) return 0;
  return (long long)wgrad_plan(M, N, K, pieces == 1 ? kR1StageMExt : kBK).chunks * N * K;   // (one term: the larger of its two plans)
}

extern "C" int egtr_linear_split_bf16_wgrad_ex_f32(egtr_stream_t stream, const float* g, int ldg, const float* x, int ldx,
                                                   float* grad_weight, float* workspace, int M, int N, int K,
                                                   const float* x_pos, int pos_rows, const unsigned char* row_keep,
                                                   int terms) {
  const int pieces = pieces_of(terms);
  if (!pieces) return EGTR_E_ARG;
  if (!g || !x || !grad_weight || !workspace || M <= 0 || N <= 0 || K <= 0 || ldg < N || ldx < K) return EGTR_E_ARG;
  if (x_pos != nullptr && pos_rows <= 0) return EGTR_E_ARG;
  if (N % 128 || K % 128 || (reinterpret_cast<uintptr_t>(grad_weight) & 15) || (reinterpret_cast<uintptr_t>(workspace) & 15))
    return EGTR_E_UNSUPPORTED;
  const bool ext = x_pos != nullptr || row_keep != nullptr;
  const WgradPlan pl = wgrad_plan(M, N, K, pieces != 1 ? kBK : ext ? kR1StageMExt : kR1StageM);
  const long long wgs = (long long)pl.chunks * (N / 128) * (K / 128);
  if (wgs >= (1ll << 31)) return EGTR_E_UNSUPPORTED;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (pieces == 1 && ext)
    hipLaunchKernelGGL((wgrad_bf16r_f32<true, kR1StageMExt>), dim3((unsigned)wgs), dim3(512), 0, st, g, ldg, x, ldx, workspace, M, N,
                       K, pl.rows_per_chunk, x_pos, pos_rows, row_keep);
  else if (pieces == 1)
    hipLaunchKernelGGL((wgrad_bf16r_f32<false, kR1StageM>), dim3((unsigned)wgs), dim3(512), 0, st, g, ldg, x, ldx, workspace, M, N,
                       K, pl.rows_per_chunk, x_pos, pos_rows, row_keep);
  else if (ext)
    hipLaunchKernelGGL(wgrad_split_bf16_f32<true>, dim3((unsigned)wgs), dim3(512), 0, st, g, ldg, x, ldx, workspace, M, N, K,
                       pl.rows_per_chunk, x_pos, pos_rows, row_keep);
  else
    hipLaunchKernelGGL(wgrad_split_bf16_f32<false>, dim3((unsigned)wgs), dim3(512), 0, st, g, ldg, x, ldx, workspace, M, N, K,
                       pl.rows_per_chunk, x_pos, pos_rows, row_keep);
  int rc = egtr_check_launch();
  if (rc != EGTR_OK) return rc;
  const int n4 = N * K / 4;
  hipLaunchKernelGGL(wgrad_reduce_f32, dim3((n4 + 15) / 16), dim3(256), 0, st, reinterpret_cast<const float4*>(workspace),
                     pl.chunks, n4, reinterpret_cast<float4*>(grad_weight));
  return egtr_check_launch();
}
