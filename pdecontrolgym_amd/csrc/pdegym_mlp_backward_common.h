// pdegym_mlp_backward_common.h -- what pdegym_mlp_backward.hip (layers of up to 64 units) and pdegym_mlp_backward_wide.hip (up to 256)
// share, each piece once.
//
// Host: the descriptor and argument checks of all six entry points (plain, _cat and _gather of either unit), the overlap scan, the
// slab and workspace arithmetic and the fill of the plan members both units have.  A unit describes itself in an Entry and keeps
// its Plan (a kernel argument: the members and their order are the kernels' business), the layout of its workspace and its launches.
//
// Device: the __forceinline__ pieces that leave every kernel's instructions as they were (tools/compare_kernel_isa.py).  They take
// VALUES, never the plan: a helper that took the plan, by reference or by value, changed the kernels it was inlined into.  The dW_0
// operand load, the stores of a dW tile and a db column, the dH_{l-1} = dZ_l W_l product and the first-layer row staging are not here
// for the same reason -- every form tried changed some instantiation (docs/HISTORY.md); each copy names its twin.
#ifndef PDEGYM_MLP_BACKWARD_COMMON_H
#define PDEGYM_MLP_BACKWARD_COMMON_H

#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "pdegym.h"
#include "pdegym_common.h"
#include "pdegym_mlp_tile.h"

namespace pdegym_mlp_backward_common {

using pdegym_mlp_tile::v4f;

constexpr int kRows = 16;                   // rows per tile (the M of the MFMA tile)
constexpr int kMaxIn = 1024;                // widest first-layer input
constexpr int kLayers = PDEGYM_MLP_MAX_LAYERS;

// ---- device -------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ v4f mma(float a, float b, v4f acc) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc, 0, 0, 0); }

// first tile of a slab: the tiles are dealt to the slabs in consecutive runs whose lengths differ by at most one
__device__ __forceinline__ int slab_begin(int slab, int tiles, int slabs) { return (int)((long long)slab * tiles / slabs); }

// torch's backward ops (tanh_backward, threshold_backward), each operation rounded on its own
__device__ __forceinline__ float act_backward(float dh, float h, int act) {
  if (act == PDEGYM_MLP_TANH) return __fmul_rn(dh, __fsub_rn(1.0f, __fmul_rn(h, h)));
  if (act == PDEGYM_MLP_RELU) return h <= 0.f ? 0.f : dh;      // a NaN activation passes the gradient
  return dh;
}

// one element of the slabs' partials, added in ascending slab order; eight loads in flight
__device__ __forceinline__ float slab_sum(const float* src, int slabs, int per_slab) {
  float sum = src[0];
  int k = 1;
  for (; k + 8 <= slabs; k += 8) {
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = src[(long long)(k + j) * per_slab];
#pragma unroll
    for (int j = 0; j < 8; ++j) sum = __fadd_rn(sum, v[j]);
  }
  for (; k < slabs; ++k) sum = __fadd_rn(sum, src[(long long)k * per_slab]);
  return sum;
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------
// what a unit says about itself
struct Entry {
  const char* name;                              // as the messages spell it: "mlp_backward", "mlp_backward_wide"
  int width;                                     // widest layer output the unit takes
  int (*own_slabs)(int tiles);                   // the unit's choice for slabs == 0
  int64_t (*tile_floats)(const pdegym_mlp*);     // floats of workspace in front of the partials, per tile of 16 rows
};

// what the argument check resolved
struct Call {
  int slabs, D;       // slabs in use; columns of the first part of a row (in_dim - n2)
  bool params;        // dw / db are wanted: three launches and a workspace
};

inline int failf(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  std::vsnprintf(pdegym::error_slot(), 512, fmt, ap);
  va_end(ap);
  return code;
}

struct Range {
  const char* lo;
  const char* hi;      // one past the last byte
  bool overlaps(const Range& o) const { return lo && o.lo && lo < o.hi && o.lo < hi; }
};

// bytes [p, p + ((rows - 1) * stride + width) * size): the part of a [rows, stride] array the call touches
inline Range extent(const void* p, int64_t rows, int64_t stride, int64_t width, int64_t size) {
  const char* c = (const char*)p;
  return {c, c ? c + ((rows - 1) * stride + width) * size : c};
}

// no output overlaps an input or another output; 0, or the code of pdegym::fail
inline int check_overlap(const Range* in, int n_in, const Range* out, int n_out) {
  for (int i = 0; i < n_out; ++i) {
    for (int j = 0; j < n_in; ++j)
      if (out[i].overlaps(in[j])) return pdegym::fail(-3, "an output or the workspace overlaps an input");
    for (int j = i + 1; j < n_out; ++j)
      if (out[i].overlaps(out[j])) return pdegym::fail(-3, "two outputs overlap (the workspace counts as one)");
  }
  return 0;
}

// the descriptor limits of a backward pass; 0, or the code of pdegym::fail
inline int check_net(const Entry& e, const pdegym_mlp* net) {
  if (!net) return pdegym::fail(-1, "null descriptor");
  if (net->n_layers < 1 || net->n_layers > kLayers) return pdegym::fail(-2, "n_layers must be 1..4");
  if (net->head != PDEGYM_MLP_HEAD_PLAIN) return failf(-2, "%s: the head must be PLAIN (a squashed-Gaussian head is applied by the caller)", e.name);
  if (net->clamp) return failf(-2, "%s: clamp must be 0", e.name);
  if (net->noise) return failf(-2, "%s: noise must be NULL", e.name);
  for (int l = 0; l < net->n_layers; ++l) {
    const pdegym_mlp_layer& L = net->layer[l];
    if (!L.w) return pdegym::fail(-3, "null weight pointer");
    if (!pdegym::is_aligned(L.w, 16)) return pdegym::fail(-2, "layer weights (w) must be 16-byte aligned");
    if (L.in_dim < 1 || L.out_dim < 1) return pdegym::fail(-2, "layer dimensions must be >= 1");
    if (L.out_dim > e.width) return failf(-2, "%s: a layer wider than %d units", e.name, e.width);
    if (l == 0 && L.in_dim > kMaxIn) return failf(-2, "%s: in_dim above 1024", e.name);
    if (l > 0 && L.in_dim != net->layer[l - 1].out_dim) return pdegym::fail(-2, "layer input size does not match the previous layer");
    if (L.act < PDEGYM_MLP_IDENTITY || L.act > PDEGYM_MLP_RELU) return pdegym::fail(-2, "unknown activation");
  }
  return 0;
}

inline int64_t tiles_of(int32_t B) { return ((int64_t)B + kRows - 1) / kRows; }

// the number of slabs in use (the unit's choice for 0), or the code of pdegym::fail
inline int resolve_slabs(const Entry& e, int32_t B, int32_t slabs) {
  if (B < 1) return pdegym::fail(-2, "B must be >= 1");
  const int tiles = (int)tiles_of(B);
  if (slabs < 0) return pdegym::fail(-2, "slabs must be >= 0");
  if (slabs > tiles) return pdegym::fail(-2, "more slabs than tiles of 16 rows");
  return slabs ? slabs : e.own_slabs(tiles);
}

// floats of one slab's partials: dW_l, db_l of every layer
inline int per_slab_floats(const pdegym_mlp* net) {
  int n = 0;
  for (int l = 0; l < net->n_layers; ++l) n += net->layer[l].out_dim * (net->layer[l].in_dim + 1);
  return n;
}

inline int64_t workspace_bytes(const Entry& e, const pdegym_mlp* net, int32_t B, int slabs) {
  return (tiles_of(B) * e.tile_floats(net) + (int64_t)slabs * per_slab_floats(net)) * (int64_t)sizeof(float);
}

// pdegym_mlp_backward_workspace / pdegym_mlp_backward_wide_workspace
inline int64_t workspace_query(const Entry& e, const pdegym_mlp* net, int32_t B, int32_t slabs) {
  if (int rc = check_net(e, net)) return rc;
  const int s = resolve_slabs(e, B, slabs);
  if (s < 0) return s;
  return workspace_bytes(e, net, B, s);
}

// The arguments of a plain entry point as the two-part ones: n2 = 0, params = 1, no x2 / dx2.  pdegym_mlp_backward_args is, field for
// field, the head of pdegym_mlp_backward_cat_args (reserved_ where params is).  A null pointer stays null: the check answers it.
struct TwoPart {
  pdegym_mlp_backward_cat_args args;
  const pdegym_mlp_backward_cat_args* p;
  explicit TwoPart(const pdegym_mlp_backward_args* a) : args{}, p(a ? &args : nullptr) {
    static_assert(offsetof(pdegym_mlp_backward_cat_args, x2) == sizeof(pdegym_mlp_backward_args) &&
                      offsetof(pdegym_mlp_backward_cat_args, params) == offsetof(pdegym_mlp_backward_args, reserved_) &&
                      offsetof(pdegym_mlp_backward_cat_args, workspace_bytes) == offsetof(pdegym_mlp_backward_args, workspace_bytes),
                  "the plain arguments are the head of the two-part ones");
    if (a) std::memcpy(&args, a, sizeof(*a)), args.params = 1;
  }
};

// The argument check of every backward entry point; 0 and what it resolved in c, or the code of pdegym::fail.  g: rows by index, or
// nullptr.  two_part false: a plain entry point (its arguments through TwoPart), which words one message its own way and asks for w[l]
// before db[l] where the others ask after.
inline int check_call(const Entry& e, const pdegym_mlp* net, const pdegym_mlp_backward_cat_args* a, const pdegym_mlp_gather* g,
                      bool two_part, int32_t B, Call& c) {
  if (int rc = check_net(e, net)) return rc;
  if (!a) return pdegym::fail(-1, "null arguments");
  if (g) {
    if (!pdegym::is_aligned(g->index, 8)) return failf(-2, "%s_gather: index must be 8-byte aligned", e.name);
    if (g->M < 1) return failf(-2, "%s_gather: M must be >= 1", e.name);
    if (a->dx) return failf(-2, "%s_gather: dx must be NULL (a gradient of gathered rows is a scatter-add)", e.name);
    if (a->dx2 && g->x2_indexed) return failf(-2, "%s_gather: dx2 needs x2_indexed == 0", e.name);
    if (g->x2_indexed && !a->n2) return failf(-2, "%s_gather: x2_indexed with n2 == 0", e.name);
  }
  const int64_t x_rows = g ? g->M : B, x2_rows = g && g->x2_indexed ? g->M : B;
  const bool params = a->params != 0;
  const int slabs = resolve_slabs(e, B, params ? a->slabs : 0);
  if (slabs < 0) return slabs;
  const int nl = net->n_layers, K0 = net->layer[0].in_dim, n_out = net->layer[nl - 1].out_dim, n2 = a->n2;
  if (n2 < 0 || n2 > 8) return failf(-2, "%s_cat: n2 must be 0..8", e.name);
  if (n2 >= K0) return failf(-2, "%s_cat: n2 must be below the first layer's in_dim (D >= 1)", e.name);
  const int D = K0 - n2;
  if (!a->x || !a->dy) return pdegym::fail(-3, "null x/dy");
  if (n2 && !a->x2) return pdegym::fail(-3, "null x2");
  if (!n2 && a->dx2) return failf(-2, "%s_cat: dx2 given with n2 == 0", e.name);
  if (n2 && !pdegym::is_aligned(a->x2, 4)) return pdegym::fail(-2, "x2 must be 4-byte aligned");
  if (a->dx2 && !pdegym::is_aligned(a->dx2, 4)) return pdegym::fail(-2, "dx2 must be 4-byte aligned");
  if (params) {
    if (!a->workspace) return pdegym::fail(-3, "null workspace");
    if (!pdegym::is_aligned(a->workspace, 4)) return pdegym::fail(-2, "workspace must be 4-byte aligned");
  } else if (!a->dx && !a->dx2) {
    return pdegym::fail(-3, "params == 0: one of dx and dx2 is required");
  }
  const bool want_dx = a->dx || a->dx2;
  for (int l = 0; l < nl; ++l) {
    const bool no_w = !a->w[l] && (l > 0 || want_dx);
    if (params && !a->dw[l]) return pdegym::fail(-3, "null dw");
    if (no_w && !two_part) return pdegym::fail(-3, "null row-major weights (w[0] is needed with dx, the others always)");
    if (params) {
      if (a->db[l] && !net->layer[l].b) return pdegym::fail(-3, "db given for a layer without bias");
      if (!a->db[l] && net->layer[l].b) return pdegym::fail(-3, "null db for a layer with bias");
    } else if (a->dw[l] || a->db[l]) {
      return pdegym::fail(-2, "params == 0: dw and db must all be NULL");
    }
    if (no_w) return pdegym::fail(-3, "null row-major weights (w[0] is needed with dx / dx2, the others always)");
  }
  if (a->dx && net->x_f64) return pdegym::fail(-2, "dx needs float32 x");
  if (a->x_stride < D || a->dy_stride < n_out || (a->dx && a->dx_stride < D) || (n2 && a->x2_stride < n2) || (a->dx2 && a->dx2_stride < n2))
    return pdegym::fail(-2, "row stride shorter than the row");
  const int64_t need = params ? workspace_bytes(e, net, B, slabs) : 0;
  if (params && a->workspace_bytes < need) return failf(-2, "workspace smaller than pdegym_%s_workspace answers", e.name);

  Range in[4 + 3 * kLayers], out[3 + 2 * kLayers];
  int n_in = 0, n_outr = 0;
  in[n_in++] = extent(a->x, x_rows, a->x_stride, D, net->x_f64 ? 8 : 4);
  in[n_in++] = extent(n2 ? a->x2 : nullptr, x2_rows, a->x2_stride, n2, 4);
  in[n_in++] = extent(a->dy, B, a->dy_stride, n_out, 4);
  in[n_in++] = extent(g ? g->index : nullptr, 1, B, B, 8);
  for (int l = 0; l < nl; ++l) {
    const pdegym_mlp_layer& L = net->layer[l];
    const int64_t cells = (int64_t)L.out_dim * L.in_dim;
    in[n_in++] = extent(a->w[l], 1, cells, cells, 4);
    in[n_in++] = extent(L.w, 1, 0, (int64_t)((L.in_dim + 3) / 4) * L.out_dim * 4, 4);
    in[n_in++] = extent(L.b, 1, L.out_dim, L.out_dim, 4);
    out[n_outr++] = extent(a->dw[l], 1, cells, cells, 4);
    out[n_outr++] = extent(a->db[l], 1, L.out_dim, L.out_dim, 4);
  }
  out[n_outr++] = extent(a->dx, B, a->dx_stride, D, 4);
  out[n_outr++] = extent(a->dx2, B, a->dx2_stride, n2, 4);
  out[n_outr++] = extent(params ? a->workspace : nullptr, 1, need, need, 1);
  if (int rc = check_overlap(in, n_in, out, n_outr)) return rc;
  c.slabs = slabs, c.D = D, c.params = params;
  return 0;
}

// the members both units' plans have; the unit lays out its workspace
template <typename Plan>
void fill_plan(Plan& P, const pdegym_mlp* net, const pdegym_mlp_backward_cat_args* a, int32_t B, const Call& c) {
  P.x = a->x, P.x_stride = a->x_stride, P.dy = a->dy, P.dy_stride = a->dy_stride, P.dx = a->dx, P.dx_stride = a->dx_stride;
  P.x2 = a->x2, P.x2_stride = a->x2_stride, P.dx2 = a->dx2, P.dx2_stride = a->dx2_stride, P.D = c.D;
  int at = 0;
  for (int l = 0; l < net->n_layers; ++l) {
    const pdegym_mlp_layer& L = net->layer[l];
    P.w[l] = a->w[l], P.dw[l] = a->dw[l], P.db[l] = a->db[l], P.in[l] = L.in_dim, P.out[l] = L.out_dim;
    P.off_w[l] = at, at += L.out_dim * L.in_dim;
    P.off_b[l] = at, at += L.out_dim;
  }
  P.per_slab = at, P.n_layers = net->n_layers, P.B = B, P.tiles = (int)tiles_of(B), P.slabs = c.slabs;
}

// the plan of the INDEXED instantiations: P and the index
template <typename GatherPlan, typename Plan>
GatherPlan gather_plan(const Plan& P, const pdegym_mlp_gather* g) {
  GatherPlan G = {};
  static_cast<Plan&>(G) = P;
  G.index = reinterpret_cast<const long long*>(g->index), G.M = g->M, G.x2_indexed = g->x2_indexed;
  return G;
}

}  // namespace pdegym_mlp_backward_common
#endif
