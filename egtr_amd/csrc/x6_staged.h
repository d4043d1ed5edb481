// The register-staged main loop of the split-bf16 GEMMs whose activations arrive as fp32: gemm_split_bf16_f32 and
// wgrad_split_bf16_f32 (gemm_split.hip) and input_proj_x6_kernel (input_proj_x6.hip).  A workgroup is 8 waves = 512 threads;
// K runs in stages of 32.  The global loads of stage s + 1 are issued into registers (inline asm, waited for by hand) while
// stage s is multiplied out of LDS; the fp32 operand is split into its three bf16 pieces on the way into LDS, the pre-split
// weights are copied.  LDS rows are 80 bytes apart, which makes the 16-byte operand reads of 32 consecutive rows conflict-free.
// What a kernel keeps for itself: its tile-to-problem mapping, its A-row addressing, its epilogue and its host-side plan; the
// weight gradient also its loop and its transposing stash (gemm_split.hip says why) -- it takes the geometry and stage_product.
// (The LDS-DMA ring of ffn_x6 / conv3x3_x6 / conv_tail_x6 / stem_x6 is a different pipeline: x6_common.h alone.)
#pragma once
#include "x6_common.h"
#include "xs_format.h"

namespace x6 {

constexpr int kBK = 32;     // K per stage
constexpr int kBN = 128;    // weight rows per stage block
constexpr int kPitch = 40;  // bf16 elements per LDS row: 32 + 8 (80 bytes)
// The tiled weight stream [N/128][K/32][3 pieces][128 rows][32] bf16 (gemm_split.hip tile_weights_*,
// egtr_amd/kernels/linear.py::gemm_split_weights): one contiguous 24 KiB block per (n block, stage).
constexpr int kWPieceElems = kBN * kBK;
constexpr int kWStageElems = 3 * kWPieceElems;
constexpr int kWStageBytes = 2 * kWStageElems;

// global -> register loads the compiler does not count (it would wait for them before the stage's MFMAs): the destination is
// usable only after vm_wait0 has named it
__device__ __forceinline__ f32x4v gload(const void* p) {
  f32x4v v;
  asm volatile("global_load_dwordx4 %0, %1, off" : "=&v"(v) : "v"(p));
  return v;
}
__device__ __forceinline__ void vm_wait0(f32x4v& v) { asm volatile("s_waitcnt vmcnt(0)" : "+v"(v)); }
template <int N>
__device__ __forceinline__ void vm_wait0(f32x4v (&v)[N]) {
#pragma unroll
  for (int q = 0; q < N; ++q) vm_wait0(v[q]);
}

// ---- W: a stage block is 1536 16-byte chunks [piece][row 128][4 chunks of 8 bf16]; thread t moves chunks t, t + 512, t + 1024
// this thread's first chunk of stage 0 of n block `nb` (nk = K / 32 stages per n block)
__device__ __forceinline__ const char* w_stage0(const void* wt, int nb, int nk, int tid) {
  return reinterpret_cast<const char*>(wt) + (size_t)nb * nk * kWStageBytes + (size_t)tid * 16;
}
__device__ __forceinline__ void issue_w(f32x4v (&rw)[3], const char* wblk, int stage) {
  const char* wp = wblk + (size_t)stage * kWStageBytes;
#pragma unroll
  for (int q = 0; q < 3; ++q) rw[q] = gload(wp + q * (512 * 16));
}
__device__ __forceinline__ void stash_w(__bf16* sW, const f32x4v (&rw)[3], int tid) {   // sW: [3][128][kPitch]
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    const int idx = tid + 512 * q;
    const int piece = idx >> 9, row = (idx >> 2) & 127, c = idx & 3;
    *reinterpret_cast<f32x4v*>(sW + (piece * kBN + row) * kPitch + 8 * c) = rw[q];
  }
}

// ---- A: exact truncation split (xs::split3_fast: for a non-finite element the lower pieces come out NaN, so its output row --
// weight gradient: its column -- is NaN, non-finite either way and nothing else is touched) into three LDS tiles `piece`
// elements apart
// four consecutive k of one row: 3 x 8 bytes
__device__ __forceinline__ void stash_a4(__bf16* p, f32x4v v, int piece) {
  const xs::Split3 s0 = xs::split3_fast(v.x), s1 = xs::split3_fast(v.y), s2 = xs::split3_fast(v.z), s3 = xs::split3_fast(v.w);
  *reinterpret_cast<uint2*>(p) = make_uint2(xs::pack_hi16(s0.hi, s1.hi), xs::pack_hi16(s2.hi, s3.hi));
  *reinterpret_cast<uint2*>(p + piece) = make_uint2(xs::pack_hi16(s0.mid, s1.mid), xs::pack_hi16(s2.mid, s3.mid));
  *reinterpret_cast<uint2*>(p + 2 * piece) = make_uint2(xs::pack_hi16(s0.lo, s1.lo), xs::pack_hi16(s2.lo, s3.lo));
}
// (The weight gradient's transposing stash -- eight rows of one column, 3 x 16 bytes -- stays in gemm_split.hip with its loop.)

// ---- one stage out of LDS: 2 k-steps x (3 + 3 NT) 16-byte reads and the six-term product of each of the wave's NT 32-column
// tiles.  pa / pw: this lane's 8 k of its row in the hi piece of the A tile [3][BM][kPitch] / of the wave's first W tile.
template <int NT, int BM>
__device__ __forceinline__ void read_kstep(const __bf16* pa, const __bf16* pw, int ks, bf16x8 (&a)[3], bf16x8 (&w)[NT][3]) {
#pragma unroll
  for (int p = 0; p < 3; ++p) {
    a[p] = *reinterpret_cast<const bf16x8*>(pa + p * BM * kPitch + 16 * ks);
#pragma unroll
    for (int t = 0; t < NT; ++t) w[t][p] = *reinterpret_cast<const bf16x8*>(pw + (p * kBN + t * 32) * kPitch + 16 * ks);
  }
}
template <int NT, int BM>
__device__ __forceinline__ void stage_product(const __bf16* pa, const __bf16* pw, f32x16 (&acc)[NT]) {
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
    bf16x8 a[3], w[NT][3];
    read_kstep<NT, BM>(pa, pw, ks, a, w);
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = mfma6(w[t], a, acc[t]);
  }
}
template <int BM>
__device__ __forceinline__ void stage_product_split(const __bf16* pa, const __bf16* pw, f32x16& acc, f32x16& acc_hi) {
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
    bf16x8 a[3], w[1][3];
    read_kstep<1, BM>(pa, pw, ks, a, w);
    mfma6_split(w[0], a, acc, acc_hi);
  }
}

// ---- the loop (nstage >= 1).  Every iteration issues the loads of the NEXT stage, multiplies the current one out of LDS and
// stores the next one (issue and stash unconditionally paired: no path leaves a load in flight); the last stage is peeled.
template <class Issue, class Compute, class Stash>
__device__ __forceinline__ void staged_loop(int nstage, Issue&& issue, Compute&& compute, Stash&& stash) {
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

}  // namespace x6
