// pdegym_mlp_backward.hip -- backward pass of the small MLP that pdegym_mlp_forward evaluates (see include/pdegym.h:
// pdegym_mlp_backward): dW, db of every layer and optionally dx, float32, deterministic, no atomics.
//
// The caller is the update half of the reference's training scripts (PPO / SAC "MlpPolicy": two hidden layers of 64 units): per
// network and minibatch torch autograd issues about ten small GEMMs and as many elementwise kernels; here a backward pass is three
// launches, whatever the number of layers.
//
//   1. mlp_backward_tiles: a workgroup of four waves owns a SLAB of consecutive 16-row tiles.  Per tile it recomputes the
//      activations of every layer into LDS with the forward kernel's own reduction (pdegym_mlp_tile.h: the same bits, nothing is
//      saved by the forward launch), then walks the layers backwards: dZ_l = dH_l * act'(H_l) elementwise, dW_l += dZ_l^T H_{l-1} and
//      db_l += sum_rows dZ_l into accumulators that live in registers across the tiles of the slab, dH_{l-1} = dZ_l W_l into LDS
//      (or into dx for the first layer).  The first layer's dZ_0 goes to the workspace instead of into a dW_0 accumulator: at
//      in_dim = 1024 that accumulator would be 256 registers per lane, so dW_0 is the second launch, which needs no LDS and spreads
//      over in_dim as well as over the slabs.
//   2. mlp_backward_dw0: a workgroup owns (64 input columns, one slab): dW_0 partial = dZ_0^T X, rows ascending.
//   3. mlp_backward_reduce: dw, db = the slabs' partials added in ascending slab order, one thread per element.
//
// All three products run on v_mfma_f32_16x16x4_f32 (float32 in, float32 accumulate: an exact fmaf chain), so the order of every sum
// is fixed by the code: rows ascending within a slab, slabs ascending, a layer's units in blocks of 16 (four MFMAs per block, unit 16 kb + 4 lg + c in the c-th).  Rows >= B of
// the last tile are selected to zero (never multiplied by zero: a non-finite weight would turn that into NaN) and never read.
//
// pdegym_mlp_backward_cat (rows in two parts, the critic(obs, action) call) launches the same kernels,
// instantiated with CAT (two-part addressing of the first layer's input and of dx) and, for params == 0, without PARAMS (the tile
// kernel alone: no dW / db products, no workspace).
//
// What this unit has in common with pdegym_mlp_backward_wide.hip lives in pdegym_mlp_backward_common.h: the argument checks of all
// entry points, the overlap scan, the slab and workspace arithmetic, the fill of the plan's common members, and mma / act_backward /
// slab_begin / the slab sum of the kernels; how an index entry becomes a row (rows by index) in pdegym_mlp_tile.h.  Here: the
// limits, the slab choice, the workspace layout, the kernels and their launches.  Kernel code that both units have and that no helper
// could hold without changing an instantiation says where its twin is.
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

constexpr int kWidth = 64;                  // widest layer output this file takes
constexpr int kLdh = lds_stride(kWidth);    // LDS row stride of a [16, 64] block: 16 rows x one float, or x one float4, hit distinct banks
constexpr int kXChunk = 512;                // observation entries per row staged at a time, as in the forward kernel
constexpr int kMaxSlabs = 256;              // the library's choice: min(tiles, 256) -- B = 32768: 256 slabs of 128 rows

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
  float* dz0;                   // workspace: [16 * tiles, 64] the first layer's dZ, zero in rows >= B and columns >= out_dim
  float* part;                  // workspace: [slabs, per_slab] partial dW_l, db_l of every layer, in the order of off_w / off_b
  int off_w[kLayers], off_b[kLayers];
  int in[kLayers], out[kLayers];
  int per_slab, n_layers, B, tiles, slabs;
  // rows in two parts (pdegym_mlp_backward_cat; read by the CAT instantiations alone): columns 0 .. D-1 of the first layer's input
  // come from x, columns D .. in[0]-1 from x2; dx holds the first D columns of dZ_0 W_0, dx2 the others
  const float* x2;
  long long x2_stride;
  float* dx2;
  long long dx2_stride;
  int D;
};

// rows by index (pdegym_mlp_backward_gather): the plan of the INDEXED instantiations, the others take Plan as they did
struct GatherPlan : Plan {
  const long long* index;      // [B]: row b of the call is row index[b] of x (and of x2 with x2_indexed)
  long long M;                 // rows of x; an entry outside [0, M) is never an address, its row reads as NaN
  int x2_indexed;
};

// v of lane l, l wave-uniform
__device__ __forceinline__ long long lane_value(long long v, int l) {
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, l), hi = (unsigned)__builtin_amdgcn_readlane((int)(v >> 32), l);
  return (long long)(((unsigned long long)hi << 32) | lo);
}

// CAT: rows in two parts.  PARAMS false: the input gradient alone -- no dW / db products, no dZ_0 in the workspace, no partial stores
// (pdegym_mlp_backward_cat with params == 0; the only launch of that call).  pdegym_mlp_backward runs <TX, false, true>, the code it was.
// INDEXED (pdegym_mlp_backward_gather; CAT instantiations only): a wave loads the index entries of the four rows it stages once per
// tile, before the first chunk.
template <typename TX, bool CAT, bool PARAMS, bool INDEXED = false>
__global__ __launch_bounds__(256) void mlp_backward_tiles(pdegym_mlp N, std::conditional_t<INDEXED, GatherPlan, Plan> P, int ldx) {
  static_assert(!INDEXED || CAT, "rows by index: the two-part instantiations");
  extern __shared__ __attribute__((aligned(16))) float bw_smem[];
  float* const hs = bw_smem;                                   // [kLayers][16][kLdh]: the activations of every layer
  float* const gs = hs + kLayers * kRows * kLdh;               // [2][16][kLdh]: dH / dZ of the layer at hand, and of the one below
  float* const xs = gs + 2 * kRows * kLdh;                     // [16][ldx]: a chunk of the observation rows
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, lg = lane >> 4;
  const int er = tid >> 4, ec = tid & 15;      // elementwise passes: thread = (row er, columns ec, ec + 16, ec + 32, ec + 48)
  const TX* __restrict__ x = static_cast<const TX*>(P.x);
  const int B = P.B, nl = P.n_layers;
  const int n = 16 * wave + li;                 // this lane's unit: neuron of the forward tiles, column of D in the backward ones

  v4f accw[kLayers][4], accb[kLayers];           // dW_l (l >= 1) tiles [unit tile = wave][input tile], db_l; live across the slab
#pragma unroll
  for (int l = 0; l < kLayers; ++l) {
    accb[l] = (v4f){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < 4; ++t) accw[l][t] = (v4f){0.f, 0.f, 0.f, 0.f};
  }

  const int t_end = slab_begin(blockIdx.x + 1, P.tiles, P.slabs);
  for (int tile = slab_begin(blockIdx.x, P.tiles, P.slabs); tile < t_end; ++tile) {
    const int row0 = tile * kRows;
    // ---- forward, as pdegym_mlp_forward computes it: the same operands in the same order --------------------------------------------
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
        // INDEXED: lane l holds the storage row of row 4 wave + l % 4, one of the four this wave stages, and whether its entry lies
        // outside [0, M); the staging loop reads them with the wave-uniform rr (lane_value: scalar row bases)
        long long xrow = 0, x2row = 0;
        int outside = 0;
        if constexpr (INDEXED) {
          bool out;      // (outside is an int: readlane takes one)
          indexed_row(P.index, P.M, P.x2_indexed, row0 + 4 * wave + (lane & 3), B, xrow, x2row, out);
          outside = out;
        }
        for (int c0 = 0; c0 < K; c0 += kXChunk) {      // (the staging has a twin in mlp_backward_wide_tiles: one row per wave there)
          const int clen = (K - c0) < kXChunk ? (K - c0) : kXChunk;
          const int cpad = (clen + 15) & ~15;
          for (int rr = 0; rr < 4; ++rr) {
            const int r = 4 * wave + rr;
            const bool row_ok = row0 + r < B;
            const TX* src = x + (long long)(row_ok ? row0 + r : 0) * P.x_stride + c0;
            if (CAT) {      // column c0 + c: the first part, or entry c0 + c - D of the tail
              const float* tail = P.x2 + (long long)(row_ok ? row0 + r : 0) * P.x2_stride;
              bool nan_row = false;
              if constexpr (INDEXED) {
                src = x + lane_value(xrow, rr) * P.x_stride + c0;
                tail = P.x2 + lane_value(x2row, rr) * P.x2_stride;
                nan_row = __builtin_amdgcn_readlane(outside, rr) != 0;
              }
              for (int c = lane; c < cpad; c += 64) {
                float v = 0.f;
                if (row_ok && c < clen) v = c0 + c < P.D ? (float)src[c] : tail[c0 + c - P.D];
                if constexpr (INDEXED) {
                  if (row_ok && c < clen && nan_row) v = __builtin_nanf("");
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
      for (int v = 0; v < 4; ++v) {      // D[row 4 lg + v][unit n]; zero past the layer's width and past the batch
        const int r = 4 * lg + v;
        hs[(l * kRows + r) * kLdh + n] = (n < H && row0 + r < B) ? activate(av[v] + bias, L.act) : 0.f;
      }
      __syncthreads();
    }

    // ---- backward -------------------------------------------------------------------------------------------------------------------
    float* g = gs;                       // dH of the layer at hand, then its dZ in place
    float* gn = gs + kRows * kLdh;       // dH of the layer below
    {
      const int H = P.out[nl - 1];
      const bool row_ok = row0 + er < B;
      const float* src = P.dy + (long long)(row_ok ? row0 + er : 0) * P.dy_stride;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int c = ec + 16 * j;
        g[er * kLdh + c] = (row_ok && c < H) ? src[c] : 0.f;
      }
    }
    __syncthreads();
#pragma unroll
    for (int l = kLayers - 1; l >= 0; --l) {
      if (l >= nl) continue;
      const int K = P.in[l], H = P.out[l], act = N.layer[l].act;
      // dZ_l = dH_l * act'(H_l), in place; selected to zero outside the batch and the layer
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int c = ec + 16 * j;
        const bool ok = row0 + er < B && c < H;
        const float dz = ok ? act_backward(g[er * kLdh + c], hs[(l * kRows + er) * kLdh + c], act) : 0.f;
        g[er * kLdh + c] = dz;
        if (PARAMS && l == 0) P.dz0[(long long)(row0 + er) * kWidth + c] = dz;
      }
      __syncthreads();
      // db_l += sum_rows dZ_l, dW_l += dZ_l^T H_{l-1}: A[unit][row] = dZ, B[row][input] = H (or ones); rows in four groups of four
      if (PARAMS && 16 * wave < H) {
        float a[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) a[s] = g[(4 * s + lg) * kLdh + n];
#pragma unroll
        for (int s = 0; s < 4; ++s) accb[l] = mma(a[s], 1.0f, accb[l]);
        if (l >= 1) {
          const float* hin = hs + (l - 1) * kRows * kLdh;
#pragma unroll
          for (int t = 0; t < 4; ++t) {
            if (16 * t < K) {      // wave-uniform
#pragma unroll
              for (int s = 0; s < 4; ++s) accw[l][t] = mma(a[s], hin[(4 * s + lg) * kLdh + 16 * t + li], accw[l][t]);
            }
          }
        }
      }
      // dH_{l-1} = dZ_l W_l (into dx for the first layer): A[row][unit] = dZ, B[unit][input] = W row-major, units in blocks of 16
      // (a twin of this product is in mlp_backward_wide_tiles, pdegym_mlp_backward_wide.hip: 16 waves and its own kLdh)
      if (l >= 1 || P.dx || (CAT && P.dx2)) {
        const float* __restrict__ W = P.w[l];
        const int in_tiles = (K + 15) >> 4, unit_blocks = (H + 15) >> 4;
        // two-part rows, first layer: only the 16-column tiles that meet a part someone asked for
        const int t_first = (CAT && l == 0 && !P.dx) ? P.D >> 4 : 0;
        const int t_last = (CAT && l == 0 && !P.dx2) ? (P.D + 15) >> 4 : in_tiles;
        for (int t = t_first + wave; t < t_last; t += 4) {
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
            if (l >= 1) gn[r * kLdh + i] = dv[v];                  // (i < 64: in_tiles <= 4)
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

  // ---- the slab's partial sums --------------------------------------------------------------------------------------------------------
  if (!PARAMS) return;
  // (the stores of a db column and of a dW tile have twins below and in mlp_backward_wide_accumulate, pdegym_mlp_backward_wide.hip)
  float* const part = P.part + (long long)blockIdx.x * P.per_slab;
#pragma unroll
  for (int l = 0; l < kLayers; ++l) {
    if (l >= nl) break;
    const int K = P.in[l], H = P.out[l];
    if (16 * wave >= H) continue;
    const float bv[4] = {accb[l].x, accb[l].y, accb[l].z, accb[l].w};
#pragma unroll
    for (int v = 0; v < 4; ++v) {      // D[unit 16 wave + 4 lg + v][column li]: every column of the db tile holds the sum
      const int o = 16 * wave + 4 * lg + v;
      if (li == 0 && o < H) part[P.off_b[l] + o] = bv[v];
    }
    if (l >= 1) {
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const float wv[4] = {accw[l][t].x, accw[l][t].y, accw[l][t].z, accw[l][t].w};
        const int i = 16 * t + li;
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          const int o = 16 * wave + 4 * lg + v;
          if (o < H && i < K) part[P.off_w[l] + o * K + i] = wv[v];
        }
      }
    }
  }
}

// dW_0 partial of (64 input columns blockIdx.x, slab blockIdx.y) = dZ_0^T X over the slab's rows, ascending.  No LDS, no barrier.
// INDEXED: a lane loads the index entries of its four rows once per tile, outside the loops over the columns.
template <typename TX, bool CAT, bool INDEXED = false>
__global__ __launch_bounds__(256) void mlp_backward_dw0(std::conditional_t<INDEXED, GatherPlan, Plan> P) {
  static_assert(!INDEXED || CAT, "rows by index: the two-part instantiations");
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int li = lane & 15, lg = lane >> 4;
  const int K = P.in[0], H = P.out[0], B = P.B;
  if (16 * wave >= H) return;
  const TX* __restrict__ x = static_cast<const TX*>(P.x);
  const int i0 = 64 * blockIdx.x;
  v4f acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = (v4f){0.f, 0.f, 0.f, 0.f};
  const int t_end = slab_begin(blockIdx.y + 1, P.tiles, P.slabs);
  for (int tile = slab_begin(blockIdx.y, P.tiles, P.slabs); tile < t_end; ++tile) {
    const int row0 = tile * kRows;
    float a[4], b[4][4];
#pragma unroll
    for (int s = 0; s < 4; ++s) a[s] = P.dz0[(long long)(row0 + 4 * s + lg) * kWidth + 16 * wave + li];
    long long xrow[4], x2row[4];      // INDEXED: the storage rows of rows row0 + 4 s + lg
    bool outside[4];
    if constexpr (INDEXED) {
#pragma unroll
      for (int s = 0; s < 4; ++s) indexed_row(P.index, P.M, P.x2_indexed, row0 + 4 * s + lg, B, xrow[s], x2row[s], outside[s]);
    }
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const int r = row0 + 4 * s + lg, i = i0 + 16 * t + li;
        const bool ok = r < B && i < K;
        if constexpr (INDEXED) {      // (this load has a twin in mlp_backward_wide_accumulate, pdegym_mlp_backward_wide.hip)
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
      }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      if (i0 + 16 * t < K) {      // wave-uniform
#pragma unroll
        for (int s = 0; s < 4; ++s) acc[t] = mma(a[s], b[t][s], acc[t]);
      }
    }
  }
  float* const part = P.part + (long long)blockIdx.y * P.per_slab + P.off_w[0];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const float wv[4] = {acc[t].x, acc[t].y, acc[t].z, acc[t].w};
    const int i = i0 + 16 * t + li;
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int o = 16 * wave + 4 * lg + v;
      if (o < H && i < K) part[o * K + i] = wv[v];
    }
  }
}

// dw, db = the slabs' partials, added in ascending slab order; one thread per element, eight loads in flight
__global__ __launch_bounds__(256) void mlp_backward_reduce(Plan P) {
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

// the workspace in front of the partials: dz0, [16, 64] per tile
int64_t tile_floats(const pdegym_mlp*) { return kRows * kWidth; }

int own_slabs(int tiles) { return tiles < kMaxSlabs ? tiles : kMaxSlabs; }

constexpr Entry kEntry = {"mlp_backward", kWidth, own_slabs, tile_floats};

// All three entry points.  params != 0: the three launches; params == 0 (two-part rows alone): the tile kernel alone, without its
// dW / db half, over the library's own slabs (a partition of the tiles among workgroups that no result depends on).
// two_part false: pdegym_mlp_backward, the <TX, false, true> instantiations; else the CAT ones.
// g: rows by index (pdegym_mlp_backward_gather), the same launches on the INDEXED instantiations; nullptr: row b is row b.
int backward_rows(const pdegym_mlp* net, const pdegym_mlp_backward_cat_args* a, const pdegym_mlp_gather* g, bool two_part, int32_t B,
                  void* stream) {
  Call c;
  if (int rc = check_call(kEntry, net, a, g, two_part, B, c)) return rc;
  const bool params = c.params;
  const int slabs = c.slabs, K0 = net->layer[0].in_dim;
  Plan P = {};
  fill_plan(P, net, a, B, c);
  P.dz0 = params ? static_cast<float*>(a->workspace) : nullptr;
  P.part = params ? P.dz0 + P.tiles * tile_floats(net) : nullptr;
  hipStream_t st = (hipStream_t)stream;
  const int kin = ((K0 < kXChunk ? K0 : kXChunk) + 15) & ~15;
  const int ldx = lds_stride(kin);
  const size_t lds_bytes = (size_t)((kLayers + 2) * kRows * kLdh + kRows * ldx) * sizeof(float);      // <= 58 KB: no opt-in needed
  const dim3 grid0((unsigned)((K0 + 63) / 64), (unsigned)slabs);
  const dim3 block(256), grid_reduce((unsigned)((P.per_slab + 255) / 256));
  if (!two_part) {
    if (net->x_f64) {
      mlp_backward_tiles<double, false, true><<<dim3(slabs), block, lds_bytes, st>>>(*net, P, ldx);
      mlp_backward_dw0<double, false><<<grid0, block, 0, st>>>(P);
    } else {
      mlp_backward_tiles<float, false, true><<<dim3(slabs), block, lds_bytes, st>>>(*net, P, ldx);
      mlp_backward_dw0<float, false><<<grid0, block, 0, st>>>(P);
    }
    mlp_backward_reduce<<<grid_reduce, block, 0, st>>>(P);
    return pdegym::check_launch("mlp_backward");
  }
  if (g) {
    const GatherPlan G = gather_plan<GatherPlan>(P, g);
    if (!params) {
      if (net->x_f64) mlp_backward_tiles<double, true, false, true><<<dim3(slabs), block, lds_bytes, st>>>(*net, G, ldx);
      else mlp_backward_tiles<float, true, false, true><<<dim3(slabs), block, lds_bytes, st>>>(*net, G, ldx);
      return pdegym::check_launch("mlp_backward_gather");
    }
    if (net->x_f64) {
      mlp_backward_tiles<double, true, true, true><<<dim3(slabs), block, lds_bytes, st>>>(*net, G, ldx);
      mlp_backward_dw0<double, true, true><<<grid0, block, 0, st>>>(G);
    } else {
      mlp_backward_tiles<float, true, true, true><<<dim3(slabs), block, lds_bytes, st>>>(*net, G, ldx);
      mlp_backward_dw0<float, true, true><<<grid0, block, 0, st>>>(G);
    }
    mlp_backward_reduce<<<grid_reduce, block, 0, st>>>(P);
    return pdegym::check_launch("mlp_backward_gather");
  }
  if (!params) {
    if (net->x_f64) mlp_backward_tiles<double, true, false><<<dim3(slabs), block, lds_bytes, st>>>(*net, P, ldx);
    else mlp_backward_tiles<float, true, false><<<dim3(slabs), block, lds_bytes, st>>>(*net, P, ldx);
    return pdegym::check_launch("mlp_backward_cat");
  }
  if (net->x_f64) {
    mlp_backward_tiles<double, true, true><<<dim3(slabs), block, lds_bytes, st>>>(*net, P, ldx);
    mlp_backward_dw0<double, true><<<grid0, block, 0, st>>>(P);
  } else {
    mlp_backward_tiles<float, true, true><<<dim3(slabs), block, lds_bytes, st>>>(*net, P, ldx);
    mlp_backward_dw0<float, true><<<grid0, block, 0, st>>>(P);
  }
  mlp_backward_reduce<<<grid_reduce, block, 0, st>>>(P);
  return pdegym::check_launch("mlp_backward_cat");
}

}  // namespace

extern "C" {

int64_t pdegym_mlp_backward_workspace(const pdegym_mlp* net, int32_t B, int32_t slabs) { return workspace_query(kEntry, net, B, slabs); }

int pdegym_mlp_backward(const pdegym_mlp* net, const pdegym_mlp_backward_args* a, int32_t B, void* stream) {
  return backward_rows(net, TwoPart(a).p, nullptr, false, B, stream);
}

// Rows in two parts, the parameter gradients on request (include/pdegym.h).
int pdegym_mlp_backward_cat(const pdegym_mlp* net, const pdegym_mlp_backward_cat_args* a, int32_t B, void* stream) {
  return backward_rows(net, a, nullptr, true, B, stream);
}

// Rows by index (include/pdegym.h): row b of the call is row g->index[b] of x; dw, db (and dx2 with x2_indexed == 0) as
// pdegym_mlp_backward_cat forms them on the materialised rows.
int pdegym_mlp_backward_gather(const pdegym_mlp* net, const pdegym_mlp_backward_cat_args* a, const pdegym_mlp_gather* g, int32_t B,
                               void* stream) {
  if (!g || !g->index) return pdegym::fail(-1, "mlp_backward_gather: null gather descriptor or index");
  return backward_rows(net, a, g, true, B, stream);
}

}  // extern "C"
