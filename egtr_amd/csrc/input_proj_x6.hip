// The input projections of all feature levels as ONE grouped, K-split launch (inference, fp32): the bias-free 1x1 projections
// of the backbone's feature maps and the extra level's 3x3 / stride 2 / padding 1 convolution of the last one
// (model/deformable_detr.py, DeformableDetrModel.input_proj), all to N = 256 channels, token-major.
//
// Why one launch: the products are independent, all inputs exist when the last bottleneck has finished, and as single launches
// each is a latency chain -- 38 and 10 row tiles walking K = 1024 / 2048, and 160 output pixels walking K = 18 432.  Here a
// work UNIT is (level, 64-row tile, 128-column block, K range of at most 512): the chains are cut short and run side by side.
// A unit writes its fp32 partial tile into slab s of the level's workspace [S_l][M_l][256] with plain vector stores -- no
// atomics, no zero-fill; the slabs are summed in a fixed order by the GroupNorm statistics pass, which reads every element
// anyway (elementwise.hip, gn_partial_tokens<float, true>).
//
// Arithmetic and main loop: those of gemm_split_bf16_f32<64> (gemm_split.hip) -- activations split by truncation on their way
// into LDS, weights pre-split round-to-nearest and pre-tiled [N/128][K/32][3 pieces][128][32] bf16 (one contiguous 24 KiB
// block per K stage, so a K range is a range of blocks), six bf16 MFMAs per K = 16, fp32 accumulation.  The loop and its
// pieces are the shared ones of x6_staged.h; this file keeps the unit mapping, the A-row addressing, the split accumulator
// and the plan.
//
// A-row addressing: *plain* -- row r of the level's [M, K] token matrix; *3x3 / stride 2 / padding 1* -- an implicit GEMM over
// the channels-last map [B, H, W, C] with K = 9 C laid out [dy][dx][c]: output pixel (b, y, x) reads input pixel
// (2y + dy - 1, 2x + dx - 1) of image b, a tap outside the image contributes zeros.  A K stage is 32 channels of ONE tap
// (C % 32 == 0): one contiguous 128-byte run per row, so the loader is the plain one with a per-(row, tap) base and a predicate.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common.h"
#include "x6_staged.h"

namespace {
using namespace x6;   // the staged main loop and its geometry (kBN, kBK, kPitch): x6_staged.h

constexpr int kBM = 64, kN = 256;
constexpr int kMaxLevels = 4;
constexpr int kMaxPiece = 512;    // no unit walks more than this much of K
constexpr int kSlots = 512;       // resident workgroups of the chip: 256 CUs x 2 (45 KiB of LDS, 16 waves per CU)

struct IpLevel {
  const float* A;             // plain: [M, K]; 3x3: [B, H, W, C]
  const unsigned short* Wt;   // [2][K / 32][3][128][32] bf16
  float* ws;                  // [S][M][256]
  int M, K, S, stages;        // stages = K / 32 / S per unit
  int C, H, W, Ho, Wo;        // C == 0: plain
  int unit0;                  // first unit of this level in the launch
};
struct IpLevels {
  IpLevel p[kMaxLevels];
};

// Workgroups are dealt round-robin to the 8 XCDs (blockIdx % 8), each with its own L2.  The two column blocks of a row tile
// and K range read the same activation rows: they are kept on ONE XCD, back to back; the pairs go round-robin over the XCDs,
// which keeps the XCDs evenly loaded although the units of different levels differ in length.  (The grid is padded to a
// multiple of 16; units beyond the last one return.)
__device__ __forceinline__ int paired_unit(int bid) {
  const int x = bid & 7, i = bid >> 3;
  return 2 * ((i >> 1) * 8 + x) + (i & 1);
}

__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(4, 4))) void input_proj_x6_kernel(IpLevels P, int nlev,
                                                                                                       int units) {
  int u = paired_unit(blockIdx.x);
  if (u >= units) return;
  int l = 0;
  while (l + 1 < nlev && u >= P.p[l + 1].unit0) ++l;
  const IpLevel& G = P.p[l];
  u -= G.unit0;
  // unit -> (K range, row tile, column block): the column blocks of a row tile are neighbours, then the row tiles of a K range
  // (they read the same weight blocks)
  const int mblocks = (G.M + kBM - 1) / kBM;
  const int nb = u & 1, mt = (u >> 1) % mblocks, ks = (u >> 1) / mblocks;
  const int m0 = mt * kBM, M = G.M, nstage = G.stages, stage0 = ks * nstage;
  const float* __restrict__ A = G.A;
  const bool conv = G.C != 0;   // uniform per workgroup

  constexpr int kStageElems = 3 * kBM * kPitch + 3 * kBN * kPitch;
  __shared__ __attribute__((aligned(16))) __bf16 sbase[kStageElems];
  __bf16* sA = sbase;
  __bf16* sW = sbase + 3 * kBM * kPitch;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 2, wn = wave & 3;   // 2 x 4 waves: 32 rows x 32 columns each
  const int li = lane & 31, hf = lane >> 5;

  // global -> register mapping of one stage: A is 64 rows x 8 float4 (thread t: row t >> 3, float4 t & 7), W 1536 16-byte
  // chunks of the contiguous stage block (thread t: chunks t, t + 512, t + 1024)
  const int lrow = tid >> 3, c4 = tid & 7;
  const int row = min(m0 + lrow, M - 1);
  const float* aplain = A + (size_t)row * G.K + 4 * c4;
  int iy0 = 0, ix0 = 0;
  const float* aimg = A;
  if (conv) {
    const int hw = G.Ho * G.Wo, b = row / hw, r = row - b * hw, y = r / G.Wo, x = r - y * G.Wo;
    iy0 = 2 * y - 1;
    ix0 = 2 * x - 1;
    aimg = A + (size_t)b * G.H * G.W * G.C + 4 * c4;
  }
  const char* wblk = w_stage0(G.Wt, nb, G.K / kBK, tid);

  f32x4v ra, rw[3];
  bool live = true;   // false: this row's tap of the stage in flight lies outside the image
  auto issue = [&](int s) {
    const int st = stage0 + s;
    const float* ap;
    if (conv) {
      const int k = st * kBK, tap = k / G.C, c0 = k - tap * G.C, dy = tap / 3, dx = tap - 3 * dy;
      const int iy = iy0 + dy, ix = ix0 + dx;
      live = iy >= 0 && iy < G.H && ix >= 0 && ix < G.W;
      ap = live ? aimg + ((size_t)iy * G.W + ix) * G.C + c0 : aimg;   // (a dead tap loads the image's first pixel: in bounds)
    } else {
      ap = aplain + (size_t)st * kBK;
    }
    ra = gload(ap);
    issue_w(rw, wblk, st);
  };
  auto stash = [&]() {
    vm_wait0(ra);
    vm_wait0(rw);
    if (!live) ra = f32x4v{0.f, 0.f, 0.f, 0.f};
    stash_a4(sA + lrow * kPitch + 4 * c4, ra, kBM * kPitch);
    stash_w(sW, rw, tid);
  };

  // Two accumulators (x6::mfma6_split says why): the five small cross terms in one, the leading products w_hi a_hi in the
  // other, added once at the end.  MFMA roles as in gemm_split: A operand = weight piece (i = n), B operand = activation piece
  f32x16 acc, acc_hi;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = acc_hi[r] = 0.f;

  const __bf16* pa = sA + (wm * 32 + li) * kPitch + 8 * hf;
  const __bf16* pw = sW + (wn * 32 + li) * kPitch + 8 * hf;
  staged_loop(nstage, issue, [&]() { stage_product_split<kBM>(pa, pw, acc, acc_hi); }, stash);
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] += acc_hi[r];

  // D[i = n][j = m]: accumulator r <-> column (r & 3) + 8 (r >> 2) + 4 hf of the wave's 32-wide n tile, row = lane & 31.  Every
  // unit writes its whole in-range tile -- zeros too, where all its taps fell outside the image: the reduction reads every slab
  const int orow = m0 + wm * 32 + li;
  if (orow < M) {
    float* out = G.ws + ((size_t)ks * M + orow) * kN + nb * kBN + wn * 32 + 4 * hf;
#pragma unroll
    for (int q = 0; q < 4; ++q)
      *reinterpret_cast<float4*>(out + 8 * q) = make_float4(acc[4 * q + 0], acc[4 * q + 1], acc[4 * q + 2], acc[4 * q + 3]);
  }
}

// ---- the plan: how many K ranges S_l per level, from the shapes alone (no device query: the call is captured in graphs) ----
//  1. No unit walks more than K = 512: the piece is the largest multiple of 32 that is <= 512 and divides the level's K (3x3
//     level: divides C, so that no piece straddles a tap).  Pieces are equal and partition K exactly.
//  2. Levels whose own units do not fill the chip (fewer than the 512 resident workgroups) have their pieces halved, level by
//     level in order and again from the first, as long as a piece stays a multiple of 32 and the launch stays within two
//     resident rounds (1024 units).  A level that fills the chip on its own keeps the split rule 1 alone demands.
// Units at 600 x 1000 (maps 75 x 125, 38 x 63, 19 x 32, extra level 10 x 16; K = 512, 1024, 2048, 9 * 2048):
//   B = 1: row tiles 147 / 38 / 10 / 3, x 2 column blocks.  Rule 1: S = 1 / 2 / 4 / 36 -> 294 + 152 + 80 + 216 = 742 units;
//          rule 2 halves levels 1 and 2 (894, 974 units; halving level 3 would give 1190): S = 1 / 4 / 8 / 36, pieces
//          512 / 256 / 256 / 512, 294 + 304 + 160 + 216 = 974 units.
//   B = 8: row tiles 1172 / 300 / 76 / 20.  Rule 1: S = 1 / 2 / 4 / 36 -> 2344 + 1200 + 608 + 1440 = 5592 units; rule 2 finds
//          every level above 512 units (and the launch beyond two rounds): nothing more is split.
struct IpPlan {
  int S[kMaxLevels];
  long long floats;   // workspace: sum of S_l * M_l * 256
  long long units;
};
bool plan_levels(int n, const int* rows, const int* K, const int* tapc, IpPlan* out) {
  if (n < 1 || n > kMaxLevels || !rows || !K) return false;
  int piece[kMaxLevels];
  long long tiles[kMaxLevels], units = 0;
  for (int l = 0; l < n; ++l) {
    const int unit_k = (tapc && tapc[l]) ? tapc[l] : K[l];
    if (rows[l] <= 0 || K[l] <= 0 || unit_k % kBK || K[l] % unit_k) return false;
    int d = std::min(unit_k, kMaxPiece) / kBK * kBK;
    while (unit_k % d) d -= kBK;
    piece[l] = d;
    tiles[l] = 2LL * ((rows[l] + kBM - 1) / kBM);
    units += tiles[l] * (K[l] / d);
  }
  for (bool again = true; again;) {
    again = false;
    for (int l = 0; l < n; ++l) {
      const long long own = tiles[l] * (K[l] / piece[l]);
      if (own >= kSlots || piece[l] % (2 * kBK) || units + own > 2 * kSlots) continue;
      piece[l] /= 2;
      units += own;
      again = true;
    }
  }
  out->floats = 0;
  out->units = units;
  for (int l = 0; l < n; ++l) {
    out->S[l] = K[l] / piece[l];
    out->floats += (long long)out->S[l] * rows[l] * kN;
  }
  return true;
}

}  // namespace

extern "C" long long egtr_input_proj_x6_workspace_floats(int num_levels, const int* rows, const int* K, const int* tap_channels,
                                                         int* splits) {
  IpPlan pl;
  if (!splits || !plan_levels(num_levels, rows, K, tap_channels, &pl)) return 0;
  for (int l = 0; l < num_levels; ++l) splits[l] = pl.S[l];
  return pl.floats;
}

extern "C" int egtr_input_proj_x6_f32(egtr_stream_t stream, int num_levels, const float* const* x,
                                      const uint16_t* const* w_tiled, float* const* workspace, const int* rows, const int* K,
                                      const int* conv_geometry, const int* splits, int N) {
  if (!x || !w_tiled || !workspace || !rows || !K || !splits || num_levels < 1) return EGTR_E_ARG;
  if (num_levels > kMaxLevels || N != kN) return EGTR_E_UNSUPPORTED;
  IpLevels P = {};
  long long units = 0;
  for (int l = 0; l < num_levels; ++l) {
    if (!x[l] || !w_tiled[l] || !workspace[l] || rows[l] <= 0 || K[l] <= 0 || splits[l] <= 0) return EGTR_E_ARG;
    const int* g = conv_geometry ? conv_geometry + 4 * l : nullptr;   // {B, H, W, C}; C == 0: plain
    IpLevel& L = P.p[l];
    if (g && g[3] != 0) {
      if (g[0] <= 0 || g[1] <= 0 || g[2] <= 0 || g[3] < 0) return EGTR_E_ARG;
      L.H = g[1];
      L.W = g[2];
      L.C = g[3];
      L.Ho = (g[1] - 1) / 2 + 1;
      L.Wo = (g[2] - 1) / 2 + 1;
      if ((long long)g[0] * L.Ho * L.Wo != rows[l] || 9LL * L.C != K[l]) return EGTR_E_ARG;
      if (L.C % kBK) return EGTR_E_UNSUPPORTED;
    }
    if (K[l] % kBK || (reinterpret_cast<uintptr_t>(x[l]) & 15) || (reinterpret_cast<uintptr_t>(w_tiled[l]) & 15) ||
        (reinterpret_cast<uintptr_t>(workspace[l]) & 15) || (long long)rows[l] * K[l] >= (1LL << 40))
      return EGTR_E_UNSUPPORTED;
    if ((K[l] / kBK) % splits[l]) return EGTR_E_ARG;   // equal pieces, each a multiple of 32
    L.A = x[l];
    L.Wt = reinterpret_cast<const unsigned short*>(w_tiled[l]);
    L.ws = workspace[l];
    L.M = rows[l];
    L.K = K[l];
    L.S = splits[l];
    L.stages = K[l] / kBK / splits[l];
    L.unit0 = (int)units;
    units += 2LL * ((rows[l] + kBM - 1) / kBM) * splits[l];
    if (units >= (1LL << 30)) return EGTR_E_UNSUPPORTED;
  }
  const unsigned grid = (unsigned)((units + 15) / 16 * 16);
  hipLaunchKernelGGL(input_proj_x6_kernel, dim3(grid), dim3(512), 0, static_cast<hipStream_t>(stream), P, num_levels,
                     (int)units);
  return egtr_check_launch();
}
