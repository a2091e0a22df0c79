// pdegym_mlp.hip -- fused forward pass of a small multi-layer perceptron policy (see include/pdegym.h: pdegym_mlp_forward).
//
// The caller on the other side of env.step(): the reference trains SB3 "MlpPolicy" networks (two hidden layers of 64 tanh
// units by default, examples/transportPDE/transport1Dppo.py:88-90) and evaluates them once per env-step.  Inside an
// on-device rollout (pde_control_gym.DeviceRollout) that evaluation was 3 GEMM + 3 tanh + clamp + copy launches -- 29 us
// per step next to a 20 us environment step at C2 -- so the whole forward pass is ONE launch here.  The arithmetic is
// tiny (85 MFLOP at B = 4096); what decides the time is operand delivery and the number of dependent memory round trips.
//
// Mapping (the one GEMM-shaped piece of the project -> MFMA): a workgroup of four waves (8 / 16 for layers wider than 64 /
// 128 units) owns 16 observation rows for all layers; wave w computes the 16 x 16 output tiles w, w + WV, ... of a layer with v_mfma_f32_16x16x4_f32 (float32 in,
// float32 accumulate).  Per 16 reduction indices a lane supplies ONE float4 of the layer input (row l % 16, inputs
// 4 (l / 16) .. + 3, read from LDS: the observation rows are staged there once, hidden activations are written there by
// the previous layer) and ONE float4 of weights per tile (blocked layout wq[k / 4][neuron][k % 4]: a wave's load is four
// contiguous 256-byte pieces) for four MFMAs -- 1/8 float per FMA, against 1.25 for a VALU formulation whose wave-uniform
// inputs have to be broadcast (the first versions: LDS broadcast reads and the texture addresser bound them at 12-17 us).
// Weight loads run a software pipeline of 64 reduction indices (a wave is alone on its SIMD).  Accumulation order is that
// of the MFMA (k in groups of four, ascending), bias added last: deterministic, but not the summation order of a BLAS GEMM
// -- results match torch within float32 rounding (tests: rtol 2e-5, atol 4e-6 on O(1) values).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "pdegym.h"
#include "pdegym_common.h"
#include "pdegym_mlp_tile.h"

namespace {

using namespace pdegym_mlp_tile;     // v4f, lds_stride, kStage, activate, load_w, mma_stage, reduce_blocks

constexpr int kRows = 16;                   // observation rows per workgroup (the M of the MFMA tile)
constexpr int kMaxWidth = PDEGYM_MLP_MAX_WIDTH;
constexpr int kXChunk = 512;                // observation entries per row staged in LDS at a time

// rows by index (pdegym_mlp_forward_gather): the INDEXED instantiations, which are never MASKED, take it in the place of rows_not, so
// that every other instantiation keeps the argument list it had
struct RowIndex {
  const long long* index;      // [B]
  long long M;                 // rows of x (and of x2 when x2_indexed)
  int x2_indexed;
};
using MaskPointer = const uint8_t* __restrict__;

// NT = 16-neuron tiles per wave, WV = waves per workgroup: one tile per wave throughout -- 4 waves for layers of up to 64
// units, 8 up to 128, 16 up to 256.  The reduction is bound by the latency of the weight stream, and more waves keep more
// loads in flight per CU than fewer waves with more tiles each (257-256-256-1 at B = 4096: 27.7 us with 4 waves x 4 tiles,
// 21.4 with 8 x 2, 19.2 with 16 x 1).
// GAUSS: the squashed-Gaussian head's epilogue, compiled apart -- as a run-time branch it cost the plain head 1 %
// CAT: rows in two parts (pdegym_mlp_forward_cat), columns 0 .. D-1 from x and D .. in_dim-1 from the float32 x2; compiled apart as
// well, so that pdegym_mlp_forward's staging loop stays the code it was
// MASKED (pdegym_mlp_forward_masked): row r is live when rows[r] != 0 and (rows_not == nullptr or rows_not[r] == 0); only live rows are
// stored, and a workgroup without one returns before it requests a weight (and before its first barrier: the condition is the same
// in every wave).  Dead rows are staged and reduced like any other -- the rows of a tile are independent in the MFMA, so a live row's
// bits do not depend on them -- which keeps the reduction the unmasked kernel's, instruction for instruction.  Compiled apart as well.
// INDEXED (pdegym_mlp_forward_gather): row b of the call is row index[b] of x (and of x2 with x2_indexed); only the CAT instantiations
// have the form (n2 == 0: D = in_dim, the tail is never read), compiled apart as the others.  A wave loads the index entries of the rows
// it stages once, before the first chunk; an entry outside [0, M) is replaced by row 0 for the address and the row is selected to NaN.
template <int NT, int WV, typename TX, typename TY, bool GAUSS, bool CAT, bool MASKED = false, bool INDEXED = false>
__global__ __launch_bounds__(64 * WV) void mlp_forward_kernel(pdegym_mlp N, const TX* __restrict__ x, long long x_stride,
                                                          TY* __restrict__ y, long long y_stride, int B, int ldx,
                                                          const float* __restrict__ x2, long long x2_stride, int D,
                                                          const uint8_t* __restrict__ rows,
                                                          std::conditional_t<INDEXED, RowIndex, MaskPointer> rows_not) {
  static_assert(!MASKED || (!GAUSS && !CAT), "the masked launch takes plain rows and the plain head");
  static_assert(!INDEXED || (CAT && !MASKED), "rows by index: the two-part instantiations, never the masked launch");
  // LDS: activations ping-pong between hb0 and hb1; the staged observation chunk shares its space with hb1 (first written
  // by the second layer, when the observations are no longer needed)
  extern __shared__ __attribute__((aligned(16))) float mlp_smem[];
  constexpr int kLdh = lds_stride(16 * WV * NT);
  constexpr int kRowsPerWave = kRows / WV;        // observation rows a wave stages
  const int kLdx = ldx;                              // >= kLdh (the launch takes the larger of the two)
  float* const hb0 = mlp_smem;
  float* const xs = mlp_smem + kRows * kLdh;
  auto hbuf = [&](int i) -> float* { return i ? xs : hb0; };
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, lg = lane >> 4;      // MFMA operand lane = (row or neuron li, k-slot lg)
  const int row0 = blockIdx.x * kRows;
  // bit r: row row0 + r is live.  Lane l looks at row l % 16, so every wave of the workgroup forms the same 16 bits.
  unsigned live_rows = 0xffffu;
  if constexpr (MASKED) {
    const int r = row0 + li;
    const bool live = r < B && rows[r] != 0 && !(rows_not && rows_not[r] != 0);
    live_rows = (unsigned)__ballot(live) & 0xffffu;
    if (live_rows == 0) return;      // workgroup-uniform
  }

  // INDEXED: the storage rows of the kRowsPerWave rows this wave stages, and whether their entries lie outside [0, M)
  long long xrow[kRowsPerWave], x2row[kRowsPerWave];
  bool outside[kRowsPerWave];
  if constexpr (INDEXED) {
    const RowIndex& gth = rows_not;
#pragma unroll
    for (int rr = 0; rr < kRowsPerWave; ++rr) {
      indexed_row(gth.index, gth.M, gth.x2_indexed, row0 + kRowsPerWave * wave + rr, B, xrow[rr], x2row[rr], outside[rr]);
    }
  }

  // weights of the first pipeline stage of the coming layer: requested before the barrier that publishes its inputs
  v4f wfirst[kStage][NT];
  auto tile_cols = [&](int H, int (&col)[NT]) {
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int n = 16 * (wave + WV * t) + li;
      col[t] = n < H ? n : H - 1;
    }
  };
  {
    int col0[NT];
    tile_cols(N.layer[0].out_dim, col0);
    if (16 * wave < N.layer[0].out_dim)
      load_w<NT>(wfirst, reinterpret_cast<const v4f*>(N.layer[0].w), N.layer[0].out_dim, (N.layer[0].in_dim + 3) >> 2, 0, lg, col0);
  }

  // biases of every layer up front (their pointers and the loads are off the critical path of the layers); the layer loop
  // is unrolled over the at most four layers so that the descriptors are read with constant offsets at kernel start
  float bias_all[PDEGYM_MLP_MAX_LAYERS][NT];
#pragma unroll
  for (int l = 0; l < PDEGYM_MLP_MAX_LAYERS; ++l) {
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int n = 16 * (wave + WV * t) + li;
      bias_all[l][t] = (l < N.n_layers && N.layer[l].b && n < N.layer[l].out_dim) ? N.layer[l].b[n] : 0.f;
    }
  }
#pragma unroll
  for (int l = 0; l < PDEGYM_MLP_MAX_LAYERS; ++l) {
    if (l >= N.n_layers) break;
    const pdegym_mlp_layer L = N.layer[l];
    const int K = L.in_dim, H = L.out_dim;
    const int ngroups = (K + 3) >> 2;
    const v4f* __restrict__ wq = reinterpret_cast<const v4f*>(L.w);
    int col[NT];
    tile_cols(H, col);
    v4f acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = (v4f){0.f, 0.f, 0.f, 0.f};
    const bool any_tile = 16 * wave < H;      // this wave has at least one tile of the layer
    const bool last = l == N.n_layers - 1;
    // the NEXT layer's first weights are requested now: they travel while this layer is reduced
    v4f wnext[kStage][NT];
    if (!last) {
      const pdegym_mlp_layer Ln = N.layer[l + 1];
      int coln[NT];
      tile_cols(Ln.out_dim, coln);
      if (16 * wave < Ln.out_dim)
        load_w<NT>(wnext, reinterpret_cast<const v4f*>(Ln.w), Ln.out_dim, (Ln.in_dim + 3) >> 2, 0, lg, coln);
    }
    if (l == 0) {
      for (int c0 = 0; c0 < K; c0 += kXChunk) {
        const int clen = (K - c0) < kXChunk ? (K - c0) : kXChunk;
        const int cpad = (clen + 15) & ~15;
        // stage the chunk: wave w copies rows kRowsPerWave w .. + kRowsPerWave - 1, a wave-wide load = 64 consecutive entries of one row; all
        // the loads of a thread are issued before the first LDS store.  Rows past the batch and entries past K read as zero.
        {
          float v[kRowsPerWave][kXChunk / 64];
#pragma unroll
          for (int rr = 0; rr < kRowsPerWave; ++rr) {
            const int r = kRowsPerWave * wave + rr;
            const bool row_ok = row0 + r < B;
            const TX* src = x + (long long)(row_ok ? row0 + r : 0) * x_stride + c0;
            const float* tail = CAT ? x2 + (long long)(row_ok ? row0 + r : 0) * x2_stride : nullptr;
            if constexpr (INDEXED) {
              src = x + xrow[rr] * x_stride + c0;
              tail = x2 + x2row[rr] * x2_stride;
            }
#pragma unroll
            for (int i = 0; i < kXChunk / 64; ++i) {
              const int c = lane + 64 * i;
              if (CAT) {      // column c0 + c of the row: the first part, or entry c0 + c - D of the tail
                v[rr][i] = 0.f;
                if (row_ok && c < clen) v[rr][i] = c0 + c < D ? (float)src[c] : tail[c0 + c - D];
                if constexpr (INDEXED) {
                  if (row_ok && c < clen && outside[rr]) v[rr][i] = __builtin_nanf("");
                }
              } else {
                v[rr][i] = (row_ok && c < clen) ? (float)src[c] : 0.f;
              }
            }
          }
          if (c0 > 0 && any_tile) load_w<NT>(wfirst, wq, H, ngroups, c0 / 16, lg, col);
#pragma unroll
          for (int rr = 0; rr < kRowsPerWave; ++rr)
#pragma unroll
            for (int i = 0; i < kXChunk / 64; ++i) {
              const int c = lane + 64 * i;
              if (c < cpad) xs[(kRowsPerWave * wave + rr) * kLdx + c] = v[rr][i];
            }
        }
        __syncthreads();
        if (any_tile) reduce_blocks<NT>(acc, wfirst, wq, H, ngroups, c0 / 16, cpad / 16, xs + li * kLdx, lg, col);
        __syncthreads();
      }
    } else {
      const float* hin = hbuf((l + 1) & 1);       // written by layer l - 1, zero beyond its width up to a multiple of 16
      if (any_tile) reduce_blocks<NT>(acc, wfirst, wq, H, ngroups, 0, (K + 15) >> 4, hin + li * kLdh, lg, col);
    }
    if (!last) {
#pragma unroll
      for (int s2 = 0; s2 < kStage; ++s2)
#pragma unroll
        for (int t = 0; t < NT; ++t) wfirst[s2][t] = wnext[s2][t];
    }
    // bias, activation; D[i = 4 lg + v][j = li] of tile t.  Hidden layers go to LDS, zero-padded to a multiple of 16 columns.
    float* hout = hbuf(l & 1);
    const int Hpad = (H + 15) & ~15;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int n = 16 * (wave + WV * t) + li;
      if (n < Hpad) {
        const float av[4] = {acc[t].x, acc[t].y, acc[t].z, acc[t].w};
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          const int r = 4 * lg + v;
          float o = n < H ? activate(av[v] + bias_all[l][t], L.act) : 0.f;
          if (GAUSS && last) {
            // H = 2A <= 16: tile 0 of wave 0, all of whose lanes are here; lane li = a holds mu[a] of row r and lane A + a of the
            // same row of 16 lanes its log_std[a].  Only the mu lanes store, into the A columns of y.
            const int A = H >> 1;
            const float log_std = row_lane_plus(o, A);
            const bool mine = n < A && row0 + r < B;
            const float eps = (N.noise && mine) ? N.noise[(long long)(row0 + r) * N.noise_stride + n] : 0.f;
            if (mine) y[(long long)(row0 + r) * y_stride + n] = (TY)squashed_gaussian(o, log_std, N.noise != nullptr, eps, N);
          } else if (last) {
            if (N.noise && n < H && row0 + r < B) o += N.noise[(long long)(row0 + r) * N.noise_stride + n];
            if (N.clamp) o = pdegym::clip_keep_nan(o, N.lo, N.hi);
            if (n < H && row0 + r < B && (!MASKED || ((live_rows >> r) & 1u))) y[(long long)(row0 + r) * y_stride + n] = (TY)o;
          } else {
            hout[r * kLdh + n] = o;
          }
        }
      }
    }
    __syncthreads();
  }
}

}  // namespace

// the second part of a two-part row (pdegym_mlp_forward_cat); x2 == nullptr: the plain row of pdegym_mlp_forward
// rows / rows_not: the row mask of pdegym_mlp_forward_masked (plain head, float32 y, no second part); rows == nullptr: every row
struct Tail {
  const float* x2;
  long long x2_stride;
  int D;
  const uint8_t* rows;
  const uint8_t* rows_not;
  const pdegym_mlp_gather* g;      // rows by index (pdegym_mlp_forward_gather); nullptr: row b is row b
};

template <int NT, int WV, typename TX, typename TY, bool GAUSS>
static void launch_mlp_nt(const pdegym_mlp* net, const TX* xp, long long xs, TY* yp, long long ys, int B, const Tail& tl, hipStream_t st) {
  const int kin = net->layer[0].in_dim < kXChunk ? net->layer[0].in_dim : kXChunk;
  const int ldh = lds_stride(16 * WV * NT);
  const int ldx = lds_stride(kin) > ldh ? lds_stride(kin) : ldh;
  const size_t lds_bytes = (size_t)kRows * (ldh + ldx) * sizeof(float);         // <= 50 KB: below the 64 KB that need no opt-in
  const dim3 grid((B + kRows - 1) / kRows), block(64 * WV);
  if (tl.g) {
    const RowIndex gth = {reinterpret_cast<const long long*>(tl.g->index), tl.g->M, tl.g->x2_indexed};
    hipLaunchKernelGGL((mlp_forward_kernel<NT, WV, TX, TY, GAUSS, true, false, true>), grid, block, lds_bytes, st, *net, xp, xs, yp, ys, B,
                       ldx, tl.x2, tl.x2_stride, tl.D, nullptr, gth);
  } else if (tl.x2)
    hipLaunchKernelGGL((mlp_forward_kernel<NT, WV, TX, TY, GAUSS, true>), grid, block, lds_bytes, st, *net, xp, xs, yp, ys, B, ldx, tl.x2,
                       tl.x2_stride, tl.D, nullptr, nullptr);
  else if constexpr (!GAUSS && std::is_same<TY, float>::value) {
    if (tl.rows)
      hipLaunchKernelGGL((mlp_forward_kernel<NT, WV, TX, TY, false, false, true>), grid, block, lds_bytes, st, *net, xp, xs, yp, ys, B, ldx,
                         nullptr, 0LL, 0, tl.rows, tl.rows_not);
    else
      hipLaunchKernelGGL((mlp_forward_kernel<NT, WV, TX, TY, GAUSS, false>), grid, block, lds_bytes, st, *net, xp, xs, yp, ys, B, ldx, nullptr, 0LL, 0, nullptr, nullptr);
  } else
    hipLaunchKernelGGL((mlp_forward_kernel<NT, WV, TX, TY, GAUSS, false>), grid, block, lds_bytes, st, *net, xp, xs, yp, ys, B, ldx, nullptr, 0LL, 0, nullptr, nullptr);
}

template <typename TX, typename TY, bool GAUSS>
static void launch_mlp_head(const pdegym_mlp* net, const TX* xp, long long xs, TY* yp, long long ys, int B, int width, const Tail& tl,
                            hipStream_t st) {
  if (width <= 64) launch_mlp_nt<1, 4, TX, TY, GAUSS>(net, xp, xs, yp, ys, B, tl, st);
  else if (width <= 128) launch_mlp_nt<1, 8, TX, TY, GAUSS>(net, xp, xs, yp, ys, B, tl, st);
  else launch_mlp_nt<1, 16, TX, TY, GAUSS>(net, xp, xs, yp, ys, B, tl, st);
}

template <typename TX, typename TY>
static void launch_mlp(const pdegym_mlp* net, const void* x, long long xs, void* y, long long ys, int B, int width, const Tail& tl,
                       hipStream_t st) {
  const TX* xp = static_cast<const TX*>(x);
  TY* yp = static_cast<TY*>(y);
  if (net->head == PDEGYM_MLP_HEAD_SQUASHED_GAUSSIAN) launch_mlp_head<TX, TY, true>(net, xp, xs, yp, ys, B, width, tl, st);
  else launch_mlp_head<TX, TY, false>(net, xp, xs, yp, ys, B, width, tl, st);
}

// pdegym_mlp_forward (n2 == 0, x2 == nullptr), pdegym_mlp_forward_cat (n2 >= 1) and pdegym_mlp_forward_masked (rows): one set of checks,
// one dispatch
static int mlp_forward_rows(const pdegym_mlp* net, const void* x, int64_t x_stride, const float* x2, int64_t x2_stride, int32_t n2,
                            void* y, int64_t y_stride, int32_t B, void* stream, const uint8_t* rows = nullptr,
                            const uint8_t* rows_not = nullptr, const pdegym_mlp_gather* g = nullptr) {
  if (!net || !x || !y) return pdegym::fail(-3, "null pointer");
  if (rows && (net->head != PDEGYM_MLP_HEAD_PLAIN || net->noise || net->y_f64))
    return pdegym::fail(-2, "mlp_forward_masked: the plain head, no noise and float32 y");
  if (B < 0) return pdegym::fail(-2, "B must be >= 0");
  if (net->n_layers < 1 || net->n_layers > PDEGYM_MLP_MAX_LAYERS) return pdegym::fail(-2, "n_layers must be 1..4");
  for (int l = 0; l < net->n_layers; ++l) {
    const pdegym_mlp_layer& L = net->layer[l];
    if (!L.w) return pdegym::fail(-3, "null weight pointer");
    if (!pdegym::is_aligned(L.w, 16)) return pdegym::fail(-2, "layer weights (w) must be 16-byte aligned");
    if (L.in_dim < 1 || L.out_dim < 1) return pdegym::fail(-2, "layer dimensions must be >= 1");
    if (L.out_dim > PDEGYM_MLP_MAX_WIDTH) return pdegym::fail(-2, "layer wider than PDEGYM_MLP_MAX_WIDTH");
    if (l == 0 && L.in_dim > PDEGYM_MLP_MAX_INPUT) return pdegym::fail(-2, "observation wider than PDEGYM_MLP_MAX_INPUT");
    if (l > 0 && L.in_dim != net->layer[l - 1].out_dim) return pdegym::fail(-2, "layer input size does not match the previous layer");
    if (L.act < PDEGYM_MLP_IDENTITY || L.act > PDEGYM_MLP_RELU) return pdegym::fail(-2, "unknown activation");
  }
  int n_out = net->layer[net->n_layers - 1].out_dim;      // columns of y and of noise
  if (net->head == PDEGYM_MLP_HEAD_SQUASHED_GAUSSIAN) {
    if (n_out % 2) return pdegym::fail(-2, "squashed-Gaussian head: the last layer holds [mu; log_std], an even number of outputs");
    if (net->layer[net->n_layers - 1].act != PDEGYM_MLP_IDENTITY) return pdegym::fail(-2, "squashed-Gaussian head: the last layer's activation must be IDENTITY");
    if (n_out > 16) return pdegym::fail(-2, "squashed-Gaussian head: pdegym_mlp_forward takes at most 8 actions");
    if (!net->clamp || !(net->lo < net->hi)) return pdegym::fail(-2, "squashed-Gaussian head: clamp must be set with lo < hi (the action box)");
    if (!(net->log_std_min <= net->log_std_max)) return pdegym::fail(-2, "squashed-Gaussian head: log_std_min <= log_std_max");
    n_out /= 2;
  } else if (net->head != PDEGYM_MLP_HEAD_PLAIN) {
    return pdegym::fail(-2, "unknown head");
  }
  if (x_stride < net->layer[0].in_dim - n2 || y_stride < n_out) return pdegym::fail(-2, "row stride shorter than the row");
  if (n2 >= net->layer[0].in_dim) return pdegym::fail(-2, "mlp_forward_cat: n2 must be below the first layer's in_dim (D >= 1)");
  if (n2 && x2_stride < n2) return pdegym::fail(-2, "mlp_forward_cat: x2 row stride shorter than the row");
  if (net->clamp && !(net->lo <= net->hi)) return pdegym::fail(-2, "clamp bounds must satisfy lo <= hi");
  if (net->noise && net->noise_stride < n_out) return pdegym::fail(-2, "noise row stride shorter than the row");
  if (B == 0) return 0;
  int width = 0;
  for (int l = 0; l < net->n_layers; ++l) width = net->layer[l].out_dim > width ? net->layer[l].out_dim : width;
  hipStream_t st = (hipStream_t)stream;
  const long long xs = x_stride, ys = y_stride;
  const Tail tl = {x2, x2_stride, net->layer[0].in_dim - n2, rows, rows_not, g};
  if (net->x_f64 && net->y_f64) launch_mlp<double, double>(net, x, xs, y, ys, B, width, tl, st);
  else if (net->x_f64) launch_mlp<double, float>(net, x, xs, y, ys, B, width, tl, st);
  else if (net->y_f64) launch_mlp<float, double>(net, x, xs, y, ys, B, width, tl, st);
  else launch_mlp<float, float>(net, x, xs, y, ys, B, width, tl, st);
  return pdegym::check_launch(g ? "mlp_forward_gather" : n2 ? "mlp_forward_cat" : (rows ? "mlp_forward_masked" : "mlp_forward"));
}

extern "C" int pdegym_mlp_forward(const pdegym_mlp* net, const void* x, int64_t x_stride, void* y, int64_t y_stride, int32_t B,
                                  void* stream) {
  return mlp_forward_rows(net, x, x_stride, nullptr, 0, 0, y, y_stride, B, stream);
}

extern "C" int pdegym_mlp_forward_masked(const pdegym_mlp* net, const void* x, int64_t x_stride, void* y, int64_t y_stride,
                                         const uint8_t* rows, const uint8_t* rows_not, int32_t B, void* stream) {
  if (!rows) return pdegym::fail(-1, "mlp_forward_masked: null rows (pdegym_mlp_forward evaluates every row)");
  return mlp_forward_rows(net, x, x_stride, nullptr, 0, 0, y, y_stride, B, stream, rows, rows_not);
}

extern "C" int pdegym_mlp_forward_cat(const pdegym_mlp* net, const void* x, int64_t x_stride, const float* x2, int64_t x2_stride,
                                      int32_t n2, void* y, int64_t y_stride, int32_t B, void* stream) {
  if (n2 < 1 || n2 > 8) return pdegym::fail(-2, "mlp_forward_cat: n2 must be 1..8");
  if (!x2) return pdegym::fail(-3, "null pointer");
  if (!pdegym::is_aligned(x2, 4)) return pdegym::fail(-2, "mlp_forward_cat: x2 must be 4-byte aligned");
  return mlp_forward_rows(net, x, x_stride, x2, x2_stride, n2, y, y_stride, B, stream);
}

// Rows by index: row b of the call is row g->index[b] of x (include/pdegym.h).  The CAT instantiations with the index; n2 == 0 is the
// plain row (D = in_dim).
extern "C" int pdegym_mlp_forward_gather(const pdegym_mlp* net, const void* x, int64_t x_stride, const float* x2, int64_t x2_stride,
                                         int32_t n2, const pdegym_mlp_gather* g, void* y, int64_t y_stride, int32_t B, void* stream) {
  if (!g || !g->index) return pdegym::fail(-1, "mlp_forward_gather: null gather descriptor or index");
  if (!pdegym::is_aligned(g->index, 8)) return pdegym::fail(-2, "mlp_forward_gather: index must be 8-byte aligned");
  if (g->M < 1) return pdegym::fail(-2, "mlp_forward_gather: M must be >= 1");
  if (n2 < 0 || n2 > 8) return pdegym::fail(-2, "mlp_forward_gather: n2 must be 0..8");
  if (g->x2_indexed && !n2) return pdegym::fail(-2, "mlp_forward_gather: x2_indexed with n2 == 0");
  if (n2 && !x2) return pdegym::fail(-3, "null pointer");
  if (n2 && !pdegym::is_aligned(x2, 4)) return pdegym::fail(-2, "mlp_forward_gather: x2 must be 4-byte aligned");
  return mlp_forward_rows(net, x, x_stride, n2 ? x2 : nullptr, n2 ? x2_stride : 0, n2, y, y_stride, B, stream, nullptr, nullptr, g);
}
