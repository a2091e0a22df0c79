// pdegym_mlp_tile.h -- the MFMA reduction of one 16 x 16 output tile of a dense layer (v_mfma_f32_16x16x4_f32, float32 in, float32
// accumulate), shared by pdegym_mlp_forward (pdegym_mlp.hip) and by the policies of more than 64 units evaluated inside the 1D
// rollout kernels (pdegym_policy.h): the same operand order and the same accumulator chain, hence the same bits.
//
// Operands: lane l holds (row or neuron li = l % 16, k-slot lg = l / 16).  Per 16 reduction indices a lane supplies ONE float4 of the
// layer input (row li, inputs 16 kb + 4 lg .. + 3, from LDS) and ONE float4 of weights per tile (blocked layout
// wq[k / 4][neuron][k % 4]: a wave's load is four contiguous 256-byte pieces) for four MFMAs; weight loads run a software pipeline
// of kStage k-blocks.  Accumulation order is that of the MFMA (k in groups of four, ascending).
#ifndef PDEGYM_MLP_TILE_H
#define PDEGYM_MLP_TILE_H

#include <hip/hip_runtime.h>

#include "pdegym.h"
#include "pdegym_common.h"

namespace pdegym_mlp_tile {

typedef float v4f __attribute__((ext_vector_type(4)));

// LDS row strides are (a multiple of 64) + 4 floats: 16-byte aligned rows, and 16 rows x one float4 hit 64 distinct banks.
// The staging area is sized by the launch for the layer widths at hand (dynamic LDS): a 257-64-64-1 policy takes 25 KB per
// workgroup instead of the 50 KB of the largest shapes, so four workgroups share a CU when the batch is large.
__host__ __device__ constexpr int lds_stride(int width) { return ((width + 63) / 64) * 64 + 4; }
constexpr int kStage = 4;                   // k-blocks (of 16 inputs) per software-pipeline stage

__device__ __forceinline__ float activate(float v, int act) {
  if (act == PDEGYM_MLP_TANH) return tanhf(v);
  if (act == PDEGYM_MLP_RELU) return (v > 0.f || v != v) ? v : 0.f;      // torch.relu keeps a NaN
  return v;
}

// The squashed-Gaussian head (include/pdegym.h: PDEGYM_MLP_HEAD_SQUASHED_GAUSSIAN), the ONE copy of its arithmetic: pdegym_mlp_forward's
// epilogue and both evaluators inside the rollout kernels call it, so equal pre-activations give equal bits everywhere.  Every
// operation is rounded on its own (hipcc contracts a * b + c by default: the _rn intrinsics do not contract), in the order of SB3's
// torch ops.  noisy false: the deterministic actor, log_std is not looked at.
__device__ __forceinline__ float squashed_gaussian(float mu, float log_std, bool noisy, float eps, const pdegym_mlp& N) {
  float z = mu;
  if (noisy) z = __fadd_rn(mu, __fmul_rn(expf(pdegym::clip_keep_nan(log_std, N.log_std_min, N.log_std_max)), eps));
  const float u = tanhf(z);
  const float c = __fadd_rn(N.lo, __fmul_rn(__fmul_rn(0.5f, __fadd_rn(u, 1.0f)), __fsub_rn(N.hi, N.lo)));
  return pdegym::clip_keep_nan(c, N.lo, N.hi);
}

// Rows by index (include/pdegym.h: pdegym_mlp_gather), the ONE copy of how an index entry becomes a row: row r of a call of B rows is
// row index[r] of a storage of M rows.  An entry outside [0, M) is never an address: row 0 stands in for it and `outside` tells the
// caller to select the row's values to NaN.  The x2 row is the indexed row, or row r itself.  Values, not the kernel's argument
// structure: see pdegym_mlp_backward_common.h.
__device__ __forceinline__ void indexed_row(const long long* index, long long M, int x2_indexed, int r, int B, long long& xrow,
                                            long long& x2row, bool& outside) {
  const long long j = r < B ? index[r] : 0;
  const bool inside = (unsigned long long)j < (unsigned long long)M;      // one comparison: j >= 0 and j < M
  xrow = inside ? j : 0;
  x2row = x2_indexed ? xrow : (r < B ? r : 0);
  outside = !inside;
}

// lane i <- lane i + A of its row of 16 lanes, A = 1 .. 8 wave-uniform (DPP row_shl:A, one v_mov_b32_dpp: no LDS round trip as a
// ds_bpermute would be); lanes i + A >= 16 of a row get 0.  Every lane of the wave must be active (pdegym_common.h, at pinned_from_left).
__device__ __forceinline__ float row_lane_plus(float v, int A) {
  using pdegym::wave::dpp_move;
  float r = 0.f;
  switch (A) {
    case 1: r = dpp_move<0x101, 0xf, true>(v); break;
    case 2: r = dpp_move<0x102, 0xf, true>(v); break;
    case 3: r = dpp_move<0x103, 0xf, true>(v); break;
    case 4: r = dpp_move<0x104, 0xf, true>(v); break;
    case 5: r = dpp_move<0x105, 0xf, true>(v); break;
    case 6: r = dpp_move<0x106, 0xf, true>(v); break;
    case 7: r = dpp_move<0x107, 0xf, true>(v); break;
    default: r = dpp_move<0x108, 0xf, true>(v); break;
  }
  asm volatile("" : "+v"(r));
  return r;
}

// weights of k-blocks kb0 .. kb0 + kStage - 1 for this lane: group g = 4 kb + l / 16 of the blocked matrix, neuron n (already
// clamped to the layer width); groups past the end of the (zero-padded) matrix read as zero
template <int NT, int ST = kStage>
__device__ __forceinline__ void load_w(v4f (&w)[ST][NT], const v4f* __restrict__ wq, int H, int ngroups, int kb0, int lg,
                                       const int (&col)[NT]) {
#pragma unroll
  for (int s = 0; s < ST; ++s) {
    const int g = 4 * (kb0 + s) + lg;
    const bool ok = g < ngroups;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const v4f v = wq[(ok ? g : ngroups - 1) * H + col[t]];
      w[s][t] = ok ? v : (v4f){0.f, 0.f, 0.f, 0.f};
    }
  }
}

template <int NT, int ST = kStage>
__device__ __forceinline__ void mma_stage(v4f (&acc)[NT], const v4f (&w)[ST][NT], const float* in_row, int kb0, int nblk, int lg) {
#pragma unroll
  for (int s = 0; s < ST; ++s) {
    if (kb0 + s < nblk) {     // wave-uniform
      const v4f a = *reinterpret_cast<const v4f*>(in_row + 16 * (kb0 + s) + 4 * lg);
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, w[s][t].x, acc[t], 0, 0, 0);
        acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, w[s][t].y, acc[t], 0, 0, 0);
        acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, w[s][t].z, acc[t], 0, 0, 0);
        acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, w[s][t].w, acc[t], 0, 0, 0);
      }
    }
  }
}

// acc[t] += in[16 rows, nblk k-blocks] x W^T for this wave's NT tiles; in_row = this lane's input row in LDS (index 0 = first
// input of the chunk), gofs = k-block offset of the chunk within the weight matrix.  wa: the first stage's weights, loaded
// by the caller BEFORE it waited for the inputs (the barrier after staging / after the previous layer's epilogue).
template <int NT, int ST = kStage>
__device__ __forceinline__ void reduce_blocks(v4f (&acc)[NT], v4f (&wa)[ST][NT], const v4f* __restrict__ wq, int H, int ngroups,
                                              int gofs, int nblk, const float* in_row, int lg, const int (&col)[NT]) {
  v4f wb[ST][NT];
  int kb = 0;
  while (true) {
    const bool more_b = kb + ST < nblk;
    if (more_b) load_w<NT, ST>(wb, wq, H, ngroups, gofs + kb + ST, lg, col);
    mma_stage<NT, ST>(acc, wa, in_row, kb, nblk, lg);
    kb += ST;
    if (!more_b) break;
    const bool more_a = kb + ST < nblk;
    if (more_a) load_w<NT, ST>(wa, wq, H, ngroups, gofs + kb + ST, lg, col);
    mma_stage<NT, ST>(acc, wb, in_row, kb, nblk, lg);
    kb += ST;
    if (!more_a) break;
  }
}

}  // namespace pdegym_mlp_tile
#endif
