// pdegym_mlp_backward_wide.hip -- backward pass of the MLP that pdegym_mlp_forward evaluates, for layers of up to 256 units (see
// include/pdegym.h: pdegym_mlp_backward_wide): dW, db of every layer and optionally dx, float32, deterministic, no atomics.
//
// The caller is the update half of the reference's SAC scripts ("MlpPolicy" of Stable-Baselines3: an actor and two critics of
// 256-256 ReLU units).  pdegym_mlp_backward.hip keeps the dW_l accumulators of its hidden layers in registers across a slab, which
// ends at 64 units: a [256, 256] dW is 256 KB, more than the register file of a SIMD.  Here EVERY layer's dZ_l and H_{l-1} go through
// the workspace and one accumulation launch forms every dZ_l^T H_{l-1}:
//
//   1. mlp_backward_wide_tiles: a workgroup of 16 waves (the forward kernel's, one 16-unit tile of a 256-unit layer per wave) owns ONE
//      16-row tile.  It recomputes the activations of every layer into LDS with the forward kernel's own reduction
//      (pdegym_mlp_tile.h: the same bits), then walks the layers backwards: dZ_l = dH_l * act'(H_l) elementwise, in place; dZ_l and
//      H_{l-1} (l >= 1; the first layer's input is x itself) to the workspace; dH_{l-1} = dZ_l W_l on the matrix cores into LDS, or
//      into dx for the first layer.  It keeps nothing from one tile to the next, so its grid has no bearing on any sum.
//   2. mlp_backward_wide_accumulate: a workgroup of four waves owns (layer, 64-unit block, 64-input block, slab): the partial
//      dZ_l^T H_{l-1} of the slab's rows, ascending; the workgroups of input block 0 form db_l from the same dZ_l.  No LDS, no barrier.
//   3. mlp_backward_wide_reduce: dw, db = the slabs' partials added in ascending slab order, one thread per element.
//
// All products run on v_mfma_f32_16x16x4_f32 (float32 in, float32 accumulate: an exact fmaf chain), in the order the header states
// for pdegym_mlp_backward: rows ascending within a slab (four MFMAs per 16-row tile), slabs ascending, a layer's units in blocks of
// 16 in ONE accumulator chain (four MFMAs per block, unit 16 kb + 4 lg + c in the c-th).  On a network both entry points take, with
// the same explicit slab count, the two return identical bits.  Rows >= B of the last tile are selected to zero (never multiplied by
// zero) and never read.
//
// The launches are made with hipLaunchKernel, the runtime's C entry point; tests/test_mlp_backward_wide.py
// reads the kernels launched here from the launch(...) calls below.  What this unit has in common with pdegym_mlp_backward.hip lives in
// pdegym_mlp_backward_common.h: the argument checks of all entry points, the overlap scan, the slab and workspace arithmetic, the fill
// of the plan's common members, and mma / act_backward / slab_begin / the slab sum of the kernels; how an index entry becomes a row
// (rows by index) in pdegym_mlp_tile.h.  Here: the limits, the slab choice, the workspace layout, the kernels and their launches.
// Kernel code that both units have and that no helper could hold without changing an instantiation says where its twin is.
//
// pdegym_mlp_backward_wide_cat (rows in two parts, the critic(obs, action) call) launches the same kernels,
// instantiated with CAT (two-part addressing of the first layer's input and of dx) and, for params == 0, without PARAMS (the tile
// kernel alone, no workspace traffic).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "pdegym.h"
#include "pdegym_common.h"
#include "pdegym_mlp_backward_common.h"
#include "pdegym_mlp_tile.h"

namespace {

using namespace pdegym_mlp_tile;     // v4f, lds_stride, kStage, activate, load_w, reduce_blocks, indexed_row
using namespace pdegym_mlp_backward_common;      // kRows, kLayers, mma, slab_begin, act_backward, slab_sum; the host checks

constexpr int kWaves = 16;                  // waves of the tile kernel: one 16-unit tile of the widest layer each
constexpr int kWidth = PDEGYM_MLP_MAX_WIDTH;      // 256: widest layer output this file takes
constexpr int kLdh = lds_stride(kWidth);    // 260: LDS row stride of a [16, 256] block
constexpr int kXChunk = 512;                // observation entries per row staged at a time, as in the forward kernel
constexpr int kBlock = 64;                  // units / inputs per workgroup of the accumulation kernel; the workspace rows are padded to it
constexpr int kSlabTiles = 8;               // the library's choice: slabs of at least 8 tiles (128 rows) ...
constexpr int kMaxSlabs = 64;               // ... and at most 64 of them
constexpr int kMaxLdsBytes = ((kLayers + 2) * kRows * kLdh + kRows * lds_stride(kXChunk)) * (int)sizeof(float);      // 132 864
static_assert(kWidth == 16 * kWaves, "one 16-unit tile per wave");
static_assert(kMaxLdsBytes <= 160 * 1024, "the LDS of a CDNA4 compute unit");

struct Plan {
  const void* x;
  long long x_stride;
  const float* dy;
  long long dy_stride;
  const float* w[kLayers];      // row-major [out, in]
  float* dw[kLayers];
  float* db[kLayers];
  float* dx;
  long long dx_stride;
  float* dz[kLayers];           // workspace: [16 * tiles, hp[l]] dZ_l, zero in rows >= B and columns >= out_dim
  float* hin[kLayers];          // workspace: [16 * tiles, kp[l]] H_{l-1} for l >= 1, zero likewise (hin[0] is not used: x)
  float* part;                  // workspace: [slabs, per_slab] partial dW_l, db_l of every layer, in the order of off_w / off_b
  int off_w[kLayers], off_b[kLayers];
  int in[kLayers], out[kLayers];
  int hp[kLayers], kp[kLayers];      // out / in rounded up to a multiple of 64
  int item0[kLayers + 1];            // first (unit block, input block) work item of layer l in the accumulation grid
  int per_slab, n_layers, B, tiles, slabs;
  // rows in two parts (pdegym_mlp_backward_wide_cat; read by the CAT instantiations alone): columns 0 .. D-1 of the first layer's
  // input come from x, columns D .. in[0]-1 from x2; dx holds the first D columns of dZ_0 W_0, dx2 the others
  const float* x2;
  long long x2_stride;
  float* dx2;
  long long dx2_stride;
  int D;
};

// rows by index (pdegym_mlp_backward_wide_gather): the plan of the INDEXED instantiations, the others take Plan as they did
struct GatherPlan : Plan {
  const long long* index;      // [B]: row b of the call is row index[b] of x (and of x2 with x2_indexed)
  long long M;                 // rows of x; an entry outside [0, M) is never an address, its row reads as NaN
  int x2_indexed;
};

// CAT: rows in two parts.  PARAMS false: the input gradient alone -- neither dZ_l nor H_{l-1} goes to the workspace
// (pdegym_mlp_backward_wide_cat with params == 0; the only launch of that call).  pdegym_mlp_backward_wide runs <TX, false, true>, the
// code it was.
// INDEXED (pdegym_mlp_backward_wide_gather; CAT instantiations only): a wave loads the index entry of the one row it stages once,
// before the first chunk.
template <typename TX, bool CAT, bool PARAMS, bool INDEXED = false>
__global__ __launch_bounds__(64 * kWaves) void mlp_backward_wide_tiles(pdegym_mlp N, std::conditional_t<INDEXED, GatherPlan, Plan> P,
                                                                       int ldx) {
  static_assert(!INDEXED || CAT, "rows by index: the two-part instantiations");
  extern __shared__ __attribute__((aligned(16))) float bww_smem[];
  float* const hs = bww_smem;                                  // [kLayers][16][kLdh]: the activations of every layer
  float* const gs = hs + kLayers * kRows * kLdh;               // [2][16][kLdh]: dH / dZ of the layer at hand, and of the one below
  float* const xs = gs + 2 * kRows * kLdh;                     // [16][ldx]: a chunk of the observation rows
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, lg = lane >> 4;
  const int er = tid >> 6, ec = tid & 63;      // elementwise passes: thread = (row er, columns ec, ec + 64, ec + 128, ec + 192)
  const TX* __restrict__ x = static_cast<const TX*>(P.x);
  const int B = P.B, nl = P.n_layers;
  const int n = 16 * wave + li;                 // this lane's unit: neuron of the forward tiles
  const int row0 = blockIdx.x * kRows;

  // ---- forward, as pdegym_mlp_forward computes it: the same operands in the same order ------------------------------------------------
#pragma unroll
  for (int l = 0; l < kLayers; ++l) {
    if (l >= nl) break;
    const pdegym_mlp_layer L = N.layer[l];
    const int K = L.in_dim, H = L.out_dim, ngroups = (K + 3) >> 2;
    const v4f* __restrict__ wq = reinterpret_cast<const v4f*>(L.w);
    const int col[1] = {n < H ? n : H - 1};
    const bool any_tile = 16 * wave < H;
    v4f acc[1] = {(v4f){0.f, 0.f, 0.f, 0.f}};
    v4f wfirst[kStage][1];
    if (l == 0) {
      // INDEXED: the storage row of the row this wave stages, and whether its entry lies outside [0, M)
      long long xrow = 0, x2row = 0;
      bool outside = false;
      if constexpr (INDEXED) {
        indexed_row(P.index, P.M, P.x2_indexed, row0 + wave, B, xrow, x2row, outside);
      }
      for (int c0 = 0; c0 < K; c0 += kXChunk) {      // (the staging has a twin in mlp_backward_tiles: four rows per wave there)
        const int clen = (K - c0) < kXChunk ? (K - c0) : kXChunk;
        const int cpad = (clen + 15) & ~15;
        {
          const int r = wave;      // one row per wave
          const bool row_ok = row0 + r < B;
          const TX* src = x + (long long)(row_ok ? row0 + r : 0) * P.x_stride + c0;
          if (CAT) {      // column c0 + c: the first part, or entry c0 + c - D of the tail
            const float* tail = P.x2 + (long long)(row_ok ? row0 + r : 0) * P.x2_stride;
            if constexpr (INDEXED) {
              src = x + xrow * P.x_stride + c0;
              tail = P.x2 + x2row * P.x2_stride;
            }
            for (int c = lane; c < cpad; c += 64) {
              float v = 0.f;
              if (row_ok && c < clen) v = c0 + c < P.D ? (float)src[c] : tail[c0 + c - P.D];
              if constexpr (INDEXED) {
                if (row_ok && c < clen && outside) v = __builtin_nanf("");
              }
              xs[r * ldx + c] = v;
            }
          } else {
            for (int c = lane; c < cpad; c += 64) xs[r * ldx + c] = (row_ok && c < clen) ? (float)src[c] : 0.f;
          }
        }
        if (any_tile) load_w<1>(wfirst, wq, H, ngroups, c0 / 16, lg, col);
        __syncthreads();
        if (any_tile) reduce_blocks<1>(acc, wfirst, wq, H, ngroups, c0 / 16, cpad / 16, xs + li * ldx, lg, col);
        __syncthreads();
      }
    } else if (any_tile) {
      load_w<1>(wfirst, wq, H, ngroups, 0, lg, col);
      reduce_blocks<1>(acc, wfirst, wq, H, ngroups, 0, (K + 15) >> 4, hs + ((l - 1) * kRows + li) * kLdh, lg, col);
    }
    const float bias = (L.b && n < H) ? L.b[n] : 0.f;
    const float av[4] = {acc[0].x, acc[0].y, acc[0].z, acc[0].w};
#pragma unroll
    for (int v = 0; v < 4; ++v) {      // D[row 4 lg + v][unit n]; zero past the layer's width and past the batch: all 256 columns are written
      const int r = 4 * lg + v;
      hs[(l * kRows + r) * kLdh + n] = (n < H && row0 + r < B) ? activate(av[v] + bias, L.act) : 0.f;
    }
    __syncthreads();
  }

  // ---- backward -----------------------------------------------------------------------------------------------------------------------
  float* g = gs;                       // dH of the layer at hand, then its dZ in place
  float* gn = gs + kRows * kLdh;       // dH of the layer below
  {
    int H = P.out[0];
#pragma unroll
    for (int k = 1; k < kLayers; ++k)
      if (k < nl) H = P.out[k];
    const bool row_ok = row0 + er < B;
    const float* src = P.dy + (long long)(row_ok ? row0 + er : 0) * P.dy_stride;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c = ec + 64 * j;
      g[er * kLdh + c] = (row_ok && c < H) ? src[c] : 0.f;
    }
  }
  __syncthreads();
#pragma unroll
  for (int l = kLayers - 1; l >= 0; --l) {
    if (l >= nl) continue;
    const int K = P.in[l], H = P.out[l], act = N.layer[l].act;
    // dZ_l = dH_l * act'(H_l), in place; selected to zero outside the batch and the layer.  dZ_l and H_{l-1} go to the workspace, every
    // row of the tile and every column up to the next multiple of 64: the accumulation kernel reads them without a bound.
    {
      float* const dzrow = P.dz[l] + (long long)(row0 + er) * P.hp[l];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int c = ec + 64 * j;
        const bool ok = row0 + er < B && c < H;
        const float dz = ok ? act_backward(g[er * kLdh + c], hs[(l * kRows + er) * kLdh + c], act) : 0.f;
        g[er * kLdh + c] = dz;
        if (PARAMS && c < P.hp[l]) dzrow[c] = dz;
      }
      if (PARAMS && l >= 1) {
        float* const hrow = P.hin[l] + (long long)(row0 + er) * P.kp[l];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int c = ec + 64 * j;
          if (c < P.kp[l]) hrow[c] = hs[((l - 1) * kRows + er) * kLdh + c];
        }
      }
    }
    __syncthreads();
    // dH_{l-1} = dZ_l W_l (into dx for the first layer): A[row][unit] = dZ, B[unit][input] = W row-major, units in blocks of 16 in
    // one accumulator chain (a twin of this product is in mlp_backward_tiles, pdegym_mlp_backward.hip: four waves and its own kLdh)
    if (l >= 1 || P.dx || (CAT && P.dx2)) {
      const float* __restrict__ W = P.w[l];
      const int in_tiles = (K + 15) >> 4, unit_blocks = (H + 15) >> 4;
      // two-part rows, first layer: only the 16-column tiles that meet a part someone asked for
      const int t_first = (CAT && l == 0 && !P.dx) ? P.D >> 4 : 0;
      const int t_last = (CAT && l == 0 && !P.dx2) ? (P.D + 15) >> 4 : in_tiles;
      for (int t = t_first + wave; t < t_last; t += kWaves) {
        const int i = 16 * t + li, ic = i < K ? i : K - 1;
        v4f d = {0.f, 0.f, 0.f, 0.f};
        for (int kb = 0; kb < unit_blocks; ++kb) {
          const v4f a4 = *reinterpret_cast<const v4f*>(g + li * kLdh + 16 * kb + 4 * lg);
          const int o = 16 * kb + 4 * lg;
          float wv[4];
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            const float v = W[(long long)(o + c < H ? o + c : H - 1) * K + ic];
            wv[c] = o + c < H ? v : 0.f;
          }
          d = mma(a4.x, wv[0], d);
          d = mma(a4.y, wv[1], d);
          d = mma(a4.z, wv[2], d);
          d = mma(a4.w, wv[3], d);
        }
        const float dv[4] = {d.x, d.y, d.z, d.w};
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          const int r = 4 * lg + v;
          if (l >= 1) gn[r * kLdh + i] = dv[v];                  // (i < 256: in_tiles <= 16)
          else if (!CAT) {
            if (i < K && row0 + r < B) P.dx[(long long)(row0 + r) * P.dx_stride + i] = dv[v];
          } else if (i < K && row0 + r < B) {
            if (i < P.D) {
              if (P.dx) P.dx[(long long)(row0 + r) * P.dx_stride + i] = dv[v];
            } else if (P.dx2) {
              P.dx2[(long long)(row0 + r) * P.dx2_stride + (i - P.D)] = dv[v];
            }
          }
        }
      }
    }
    __syncthreads();
    float* const swap = g;
    g = gn, gn = swap;
  }
}

// The partial dW_l of (work item blockIdx.x = layer, 64 units, 64 inputs; slab blockIdx.y) = dZ_l^T H_{l-1} over the slab's rows,
// ascending, and with input block 0 the partial db_l = dZ_l^T 1.  No LDS, no barrier.
// INDEXED: a lane loads the index entries of its four rows once per tile (first layer's work items), outside the loops over the columns.
template <typename TX, bool CAT, bool INDEXED = false>
__global__ __launch_bounds__(256) void mlp_backward_wide_accumulate(std::conditional_t<INDEXED, GatherPlan, Plan> P) {
  static_assert(!INDEXED || CAT, "rows by index: the two-part instantiations");
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int li = lane & 15, lg = lane >> 4;
  // the layer of this work item and its figures, selected with constant indices (the plan lives in the kernel's arguments)
  int l = 0, K = P.in[0], H = P.out[0], hp = P.hp[0], kp = P.kp[0], first = 0, off_w = P.off_w[0], off_b = P.off_b[0];
  const float* __restrict__ dzl = P.dz[0];
  const float* __restrict__ hl = nullptr;
#pragma unroll
  for (int k = 1; k < kLayers; ++k)
    if (k < P.n_layers && (int)blockIdx.x >= P.item0[k]) {
      l = k, K = P.in[k], H = P.out[k], hp = P.hp[k], kp = P.kp[k], first = P.item0[k], off_w = P.off_w[k], off_b = P.off_b[k];
      dzl = P.dz[k], hl = P.hin[k];
    }
  const int B = P.B;
  const int in_blocks = kp / kBlock, item = (int)blockIdx.x - first;
  const int u0 = kBlock * (item / in_blocks) + 16 * wave, i0 = kBlock * (item % in_blocks);
  if (u0 >= H) return;      // wave-uniform
  const bool bias_too = i0 == 0;
  const TX* __restrict__ x = static_cast<const TX*>(P.x);
  v4f acc[4], accb = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = (v4f){0.f, 0.f, 0.f, 0.f};
  const int t_end = slab_begin(blockIdx.y + 1, P.tiles, P.slabs);
  for (int tile = slab_begin(blockIdx.y, P.tiles, P.slabs); tile < t_end; ++tile) {
    const int row0 = tile * kRows;
    float a[4], b[4][4];
#pragma unroll
    for (int s = 0; s < 4; ++s) a[s] = dzl[(long long)(row0 + 4 * s + lg) * hp + u0 + li];
    long long xrow[4], x2row[4];      // INDEXED: the storage rows of rows row0 + 4 s + lg
    bool outside[4];
    if constexpr (INDEXED) {
      if (l == 0) {
#pragma unroll
        for (int s = 0; s < 4; ++s) indexed_row(P.index, P.M, P.x2_indexed, row0 + 4 * s + lg, B, xrow[s], x2row[s], outside[s]);
      }
    }
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const int r = row0 + 4 * s + lg, i = i0 + 16 * t + li;
        if (l == 0) {
          const bool ok = r < B && i < K;
          if constexpr (INDEXED) {      // (this load has a twin in mlp_backward_dw0, pdegym_mlp_backward.hip)
            b[t][s] = 0.f;
            if (ok) b[t][s] = i < P.D ? (float)x[xrow[s] * P.x_stride + i] : P.x2[x2row[s] * P.x2_stride + (i - P.D)];
            if (ok && outside[s]) b[t][s] = __builtin_nanf("");
          } else if (CAT) {
            b[t][s] = 0.f;
            if (ok) b[t][s] = i < P.D ? (float)x[(long long)r * P.x_stride + i] : P.x2[(long long)r * P.x2_stride + (i - P.D)];
          } else {
            const TX v = x[ok ? (long long)r * P.x_stride + i : 0];
            b[t][s] = ok ? (float)v : 0.f;
          }
        } else {
          b[t][s] = hl[(long long)r * kp + i];      // (padded to 64 columns and 16 rows, zero there)
        }
      }
    if (bias_too) {
#pragma unroll
      for (int s = 0; s < 4; ++s) accb = mma(a[s], 1.0f, accb);
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      if (i0 + 16 * t < K) {      // wave-uniform
#pragma unroll
        for (int s = 0; s < 4; ++s) acc[t] = mma(a[s], b[t][s], acc[t]);
      }
    }
  }
  // (the stores of a dW tile and of a db column have twins in mlp_backward_tiles and mlp_backward_dw0, pdegym_mlp_backward.hip)
  float* const part = P.part + (long long)blockIdx.y * P.per_slab;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const float wv[4] = {acc[t].x, acc[t].y, acc[t].z, acc[t].w};
    const int i = i0 + 16 * t + li;
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int o = u0 + 4 * lg + v;
      if (o < H && i < K) part[off_w + o * K + i] = wv[v];
    }
  }
  if (bias_too) {
    const float bv[4] = {accb.x, accb.y, accb.z, accb.w};
#pragma unroll
    for (int v = 0; v < 4; ++v) {      // D[unit u0 + 4 lg + v][column li]: every column of the db tile holds the sum
      const int o = u0 + 4 * lg + v;
      if (li == 0 && o < H) part[off_b + o] = bv[v];
    }
  }
}

// dw, db = the slabs' partials, added in ascending slab order; one thread per element, eight loads in flight
__global__ __launch_bounds__(256) void mlp_backward_wide_reduce(Plan P) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= P.per_slab) return;
  float* dst = nullptr;
#pragma unroll
  for (int l = 0; l < kLayers; ++l) {
    if (l >= P.n_layers) break;
    if (e >= P.off_w[l] && e < P.off_b[l]) dst = P.dw[l] + (e - P.off_w[l]);
    if (e >= P.off_b[l] && e < P.off_b[l] + P.out[l]) dst = P.db[l] ? P.db[l] + (e - P.off_b[l]) : nullptr;
  }
  if (!dst) return;
  *dst = slab_sum(P.part + e, P.slabs, P.per_slab);
}

// hipLaunchKernel takes the arguments as an array of pointers to them (their types are the kernel's: nothing is deduced from p)
template <typename T>
struct as_declared {
  using type = T;
};
template <typename... A>
void launch(void (*kernel)(A...), dim3 grid, dim3 block, size_t lds_bytes, hipStream_t stream, typename as_declared<A>::type... p) {
  void* args[] = {(void*)&p...};
  (void)hipLaunchKernel((const void*)kernel, grid, block, args, lds_bytes, stream);      // (check_launch reads the error)
}

int pad64(int n) { return (n + kBlock - 1) / kBlock * kBlock; }

// the workspace in front of the partials: 16 rows of the dZ_l (every layer) and H_{l-1} (l >= 1) blocks per tile
int64_t tile_floats(const pdegym_mlp* net) {
  int n = 0;
  for (int l = 0; l < net->n_layers; ++l) n += pad64(net->layer[l].out_dim) + (l >= 1 ? pad64(net->layer[l].in_dim) : 0);
  return (int64_t)kRows * n;
}

int own_slabs(int tiles) {
  const int own = (tiles + kSlabTiles - 1) / kSlabTiles;
  return own < kMaxSlabs ? own : kMaxSlabs;
}

constexpr Entry kEntry = {"mlp_backward_wide", kWidth, own_slabs, tile_floats};

// G: rows by index (pdegym_mlp_backward_wide_gather), the INDEXED instantiations of the first two kernels; nullptr: row b is row b
template <typename TX, bool CAT, bool PARAMS>
int launch_all(const pdegym_mlp* net, const Plan& P, hipStream_t st, const GatherPlan* G = nullptr) {
  static signed char attr[pdegym::kMaxDevices] = {}, attr_indexed[pdegym::kMaxDevices] = {};
  if constexpr (CAT) {
    if (G && !pdegym::raise_dynamic_lds_limit(reinterpret_cast<const void*>(&mlp_backward_wide_tiles<TX, CAT, PARAMS, true>), kMaxLdsBytes,
                                              attr_indexed))
      return pdegym::fail(-4, "cannot raise the dynamic LDS limit of mlp_backward_wide_tiles");
  }
  if (!G && !pdegym::raise_dynamic_lds_limit(reinterpret_cast<const void*>(&mlp_backward_wide_tiles<TX, CAT, PARAMS>), kMaxLdsBytes, attr))
    return pdegym::fail(-4, "cannot raise the dynamic LDS limit of mlp_backward_wide_tiles");
  const int K0 = P.in[0];
  const int kin = ((K0 < kXChunk ? K0 : kXChunk) + 15) & ~15;
  const int ldx = lds_stride(kin);
  const size_t lds_bytes = (size_t)((kLayers + 2) * kRows * kLdh + kRows * ldx) * sizeof(float);      // 101 .. 130 KB: above the 64 KB a kernel gets without asking
  if constexpr (CAT) {
    if (G) {
      launch(mlp_backward_wide_tiles<TX, CAT, PARAMS, true>, dim3((unsigned)P.tiles), dim3(64 * kWaves), lds_bytes, st, *net, *G, ldx);
      if (PARAMS) {
        launch(mlp_backward_wide_accumulate<TX, CAT, true>, dim3((unsigned)P.item0[P.n_layers], (unsigned)P.slabs), dim3(256), 0, st, *G);
        launch(mlp_backward_wide_reduce, dim3((unsigned)((P.per_slab + 255) / 256)), dim3(256), 0, st, P);
      }
      return pdegym::check_launch("mlp_backward_wide_gather");
    }
  }
  launch(mlp_backward_wide_tiles<TX, CAT, PARAMS>, dim3((unsigned)P.tiles), dim3(64 * kWaves), lds_bytes, st, *net, P, ldx);
  if (PARAMS) {
    launch(mlp_backward_wide_accumulate<TX, CAT>, dim3((unsigned)P.item0[P.n_layers], (unsigned)P.slabs), dim3(256), 0, st, P);
    launch(mlp_backward_wide_reduce, dim3((unsigned)((P.per_slab + 255) / 256)), dim3(256), 0, st, P);
  }
  return pdegym::check_launch(CAT ? "mlp_backward_wide_cat" : "mlp_backward_wide");
}

// All three entry points.  params != 0: the three launches; params == 0 (two-part rows alone): the tile kernel alone, without its
// workspace stores.  two_part false: pdegym_mlp_backward_wide, the <TX, false, true> instantiations; else the CAT ones.
// g: rows by index (pdegym_mlp_backward_wide_gather), the same launches on the INDEXED instantiations; nullptr: row b is row b.
int backward_wide_rows(const pdegym_mlp* net, const pdegym_mlp_backward_cat_args* a, const pdegym_mlp_gather* g, bool two_part,
                       int32_t B, void* stream) {
  Call c;
  if (int rc = check_call(kEntry, net, a, g, two_part, B, c)) return rc;
  Plan P = {};
  fill_plan(P, net, a, B, c);
  const int64_t rows = tiles_of(B) * kRows;
  float* ws = c.params ? static_cast<float*>(a->workspace) : nullptr;
  int items = 0;
  for (int l = 0; l < P.n_layers; ++l) {
    P.hp[l] = pad64(P.out[l]), P.kp[l] = pad64(P.in[l]);
    if (c.params) {
      P.dz[l] = ws, ws += rows * P.hp[l];
      if (l >= 1) P.hin[l] = ws, ws += rows * P.kp[l];
    }
    P.item0[l] = items, items += (P.hp[l] / kBlock) * (P.kp[l] / kBlock);
  }
  for (int l = P.n_layers; l <= kLayers; ++l) P.item0[l] = items;
  P.part = ws;
  hipStream_t st = (hipStream_t)stream;
  if (!two_part) return net->x_f64 ? launch_all<double, false, true>(net, P, st) : launch_all<float, false, true>(net, P, st);
  GatherPlan G = {};
  if (g) G = gather_plan<GatherPlan>(P, g);
  const GatherPlan* Gp = g ? &G : nullptr;
  if (!c.params) return net->x_f64 ? launch_all<double, true, false>(net, P, st, Gp) : launch_all<float, true, false>(net, P, st, Gp);
  return net->x_f64 ? launch_all<double, true, true>(net, P, st, Gp) : launch_all<float, true, true>(net, P, st, Gp);
}

}  // namespace

extern "C" {

int64_t pdegym_mlp_backward_wide_workspace(const pdegym_mlp* net, int32_t B, int32_t slabs) {
  return workspace_query(kEntry, net, B, slabs);
}

int pdegym_mlp_backward_wide(const pdegym_mlp* net, const pdegym_mlp_backward_args* a, int32_t B, void* stream) {
  return backward_wide_rows(net, TwoPart(a).p, nullptr, false, B, stream);
}

// Rows in two parts, the parameter gradients on request (include/pdegym.h).
int pdegym_mlp_backward_wide_cat(const pdegym_mlp* net, const pdegym_mlp_backward_cat_args* a, int32_t B, void* stream) {
  return backward_wide_rows(net, a, nullptr, true, B, stream);
}

// Rows by index (include/pdegym.h): row b of the call is row g->index[b] of x; dw, db (and dx2 with x2_indexed == 0) as
// pdegym_mlp_backward_wide_cat forms them on the materialised rows.
int pdegym_mlp_backward_wide_gather(const pdegym_mlp* net, const pdegym_mlp_backward_cat_args* a, const pdegym_mlp_gather* g, int32_t B,
                                    void* stream) {
  if (!g || !g->index) return pdegym::fail(-1, "mlp_backward_wide_gather: null gather descriptor or index");
  return backward_wide_rows(net, a, g, true, B, stream);
}

}  // extern "C"
