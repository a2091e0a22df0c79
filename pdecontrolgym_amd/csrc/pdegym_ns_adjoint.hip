// pdegym_ns_adjoint.hip -- the adjoint-optimisation baseline of the NavierStokes2D result tables on the device (include/pdegym.h):
//   pdegym_ns2d_adjoint_f64   the backward march and the control read-off of examples/NavierStokes/NS2Doptimization.py:83-107
// All T-1 backward steps of a batch in ONE launch, float64 (the script's arithmetic).  The shape is the column kernel's (ns_col_body,
// pdegym_ns2d.hip): one lane per grid column, floor(64 / nx) instances side by side in a wave, East / West neighbours by DPP lane
// shifts, no barriers.  lambda1, lambda2 and the pressure (the warm start of the next backward step) stay on chip from the first
// backward step to the last; a step reads one forward frame and one target frame and writes one gradient, one command and --
// when asked -- one frame of (lambda1, lambda2).
// While the K Jacobi sweeps run (p, its ping-pong copy and dx*dy*rhs: 3 NY float64 registers per lane) lambda1 and lambda2 wait in
// wave-private LDS (2 * NY * 64 doubles: 32 KB at 32 rows): no caller scratch, no traffic beyond the CU.
// The sweeps, the right-hand side and the wall write-out restate the forward kernel's (col_rhs_term / col_jacobi_solve below).
// Expression trees are the script's, operand order as written at :89-100; -ffp-contract=off and IEEE division
// keep every value bit-identical to NumPy.
// Output contracts (poisoned buffers, guard bands): tests/test_gpu_adjoint.py, KERNEL_CASES there.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "pdegym.h"
#include "pdegym_common.h"

#include "pdegym_ns_common.h"

namespace {

using namespace pdegym::ns;

// ---- the pressure solve of a column-per-lane field: the right-hand side of a row, the K sweeps, the wall write-out ----------------
// A second copy of what ns_col_body (pdegym_ns2d.hip) does inline, same expression trees: calling one shared copy from there moved
// the register counts and scratch sizes of several ns_col_step instantiations, so the forward kernels keep their code untouched.

// dx*dy*rhs of row i (navier_stokes2D.py:101-103, :108) from the row's u and the v above / below; 0 on the edge lanes.
template <typename T>
__device__ __forceinline__ T col_rhs_term(const NSScal<T>& S, T u_c, T v_n, T v_s, bool icol) {
  const T ue = pinned_from_right(u_c), uw = pinned_from_left(u_c);
  const T dudx = div_c(ue - uw, S.two_dx, S.inv_two_dx);
  const T dvdy = div_c(v_n - v_s, S.two_dy, S.inv_two_dy);
  const T r = S.rho_over_dt * (dudx + dvdy);
  if constexpr (sizeof(T) == 4) return icol ? jacobi_rhs_term(S.dxdy, r) : 0.f;
  else return icol ? S.dxdy * r : (T)0;
}

// K Jacobi sweeps (:104-114) on p, walls included on the way out.
// FIRST sweep: the walls as given (edge lanes and rows 0, NY-1 hold them); afterwards a stencil next to a wall reads the cell's
// own old value (= what the Neumann copies of the previous sweep left in the wall).  Edge lanes run the same arithmetic on
// whatever their neighbours hold: nothing reads them until the walls are written out after the last sweep.
template <typename T, int NY>
__device__ __forceinline__ void col_jacobi_solve(T (&p)[NY], const T (&rq)[NY], int iters, bool lef, bool rig, bool icol,
                                                 bool next_to_left, bool next_to_right) {
  auto sweep = [&](auto first_tag) {
    constexpr bool FIRST = decltype(first_tag)::value;
    T below = p[0];                      // old value of the row below
#pragma unroll
    for (int i = 1; i < NY - 1; ++i) {
      const T cur = p[i];
      const T wl = pinned_from_left(cur), er = pinned_from_right(cur);
      const T w = (!FIRST && next_to_left) ? cur : wl;
      const T e = (!FIRST && next_to_right) ? cur : er;
      const T sv = (!FIRST && i == 1) ? cur : below;
      const T nv = (!FIRST && i == NY - 2) ? cur : p[i + 1];
      const T s4 = ((w + sv) + e) + nv;
      T val;
      if constexpr (sizeof(T) == 4) val = jacobi_update(s4, rq[i]);
      else val = (T)0.25 * (s4 - rq[i]);
      p[i] = FIRST ? (icol ? val : cur) : val;
      below = cur;
    }
  };
  // every later sweep reads one array and writes the other (p -> q, q -> p): the old row below is still in place when row i
  // needs it, so nothing is carried along (one 64-bit move per row and sweep less; p, q and rq are 126 float64 registers)
  auto sweep_into = [&](const T (&src)[NY], T (&dst)[NY]) {
#pragma unroll
    for (int i = 1; i < NY - 1; ++i) {
      const T cur = src[i];
      const T wl = pinned_from_left(cur), er = pinned_from_right(cur);
      const T w = next_to_left ? cur : wl;
      const T e = next_to_right ? cur : er;
      const T sv = (i == 1) ? cur : src[i - 1];
      const T nv = (i == NY - 2) ? cur : src[i + 1];
      const T s4 = ((w + sv) + e) + nv;
      if constexpr (sizeof(T) == 4) dst[i] = jacobi_update(s4, rq[i]);
      else dst[i] = (T)0.25 * (s4 - rq[i]);
    }
  };
  if (iters > 0) {
    sweep(std::true_type{});
    T q[NY];
#pragma unroll
    for (int i = 0; i < NY; ++i) q[i] = p[i];
    int it = 1;
    for (; it + 2 <= iters; it += 2) {
      sweep_into(p, q);
      sweep_into(q, p);
    }
    if (it < iters) {
      sweep_into(p, q);
#pragma unroll
      for (int i = 1; i < NY - 1; ++i) p[i] = q[i];
    }
    // the four Neumann copies of the last sweep (:110-113): every wall cell = its nearest interior cell
    p[0] = p[1];
    p[NY - 1] = p[NY - 2];
#pragma unroll
    for (int i = 0; i < NY; ++i) {
      const T from_r = pinned_from_right(p[i]), from_l = pinned_from_left(p[i]);
      p[i] = lef ? from_r : (rig ? from_l : p[i]);
    }
  }
}

struct AdjointArgs {
  int T, t0, nt_ref;
  const double* obs;       // [T + 1, B, ny, nx, 2]
  const double* U_ref;     // [nt_ref, ny, nx, 2]
  const double* a_nom;     // [T]
  double ratio, width, dx;
  double* grad;            // [T, B]
  double* actions;         // [T, B]
  double* lam;             // [T, B, ny, nx, 2] or NULL
};

// One wave per SIMD (the float64 column kernels' build without spills, ns_col_step_w1): p, q and rq alone are 192 registers at 32 rows.
template <int NY>
__global__ __launch_bounds__(64, 1) void ns_adjoint_march(NSConst C, NSScal<double> S, AdjointArgs A, int B) {
  __shared__ double park[2][NY][64];      // lambda1, lambda2 of this wave's lanes during the sweeps
  __shared__ double red[64];
  const int nx = C.nx, ncell = nx * NY;
  const int lane = threadIdx.x;
  const int G = 64 / nx;
  const int g = lane / nx;
  const int live_g = g < G ? g : G - 1;
  const int j = g < G ? lane - g * nx : nx - 1;                 // idle lanes shadow a valid cell and never store
  const int b_raw = blockIdx.x * G + live_g;
  const bool live = g < G && b_raw < B;
  const int b = b_raw < B ? b_raw : B - 1;
  const bool lef = j == 0, rig = j == nx - 1, icol = !lef && !rig;
  const int T = A.T;

  // what one time index of the outputs receives: the frame of (lambda1, lambda2), the gradient and the command (:103-107)
  auto write_out = [&](int t, const double (&l1)[NY], const double (&l2)[NY]) {
    if (A.lam && live) {
      double2* dst = reinterpret_cast<double2*>(A.lam) + ((size_t)t * B + b) * ncell;
#pragma unroll
      for (int i = 0; i < NY; ++i) dst[i * nx + j] = make_double2(l1[i], l2[i]);
    }
    // central_difference(Lam1[t], "y", dy)[-2, :] (:106): zero in the wall columns, summed from the first column on (:107)
    red[lane] = icol ? div_c(l1[NY - 1] - l1[NY - 3], S.two_dy, S.inv_two_dy) : 0.0;
    wave_lds_sync();
    if (live && j == 0) {
      double ss = 0.0;
      for (int k = 0; k < nx; ++k) ss += red[lane + k];
      A.grad[(size_t)t * B + b] = ss;
      A.actions[(size_t)t * B + b] = A.a_nom[t] - ((A.ratio * ss) * A.width) * A.dx;
    }
    wave_lds_sync();
  };

  double l1[NY], l2[NY], p[NY];
#pragma unroll
  for (int i = 0; i < NY; ++i) l1[i] = l2[i] = p[i] = 0.0;      // Lam1[0], Lam2[0], pressure (:84-86)
  write_out(T - 1, l1, l2);

  for (int k = 0; k + 1 < T; ++k) {
    const int s = T - k;                                          // U[-1-t], V[-1-t] of the script: the state at time index t0 + s
    const int tr = A.t0 + s < A.nt_ref ? A.t0 + s : A.nt_ref - 1;
    const double2* st = reinterpret_cast<const double2*>(A.obs) + ((size_t)s * B + b) * ncell;
    const double2* tg = reinterpret_cast<const double2*>(A.U_ref) + (size_t)tr * ncell;
    // ---- dlam/dt and the explicit step (:89-96), in place with the old row below carried along ----
    {
      double b1 = l1[0], b2 = l2[0];
#pragma unroll
      for (int i = 1; i < NY - 1; ++i) {
        const double c1 = l1[i], c2 = l2[i];
        const double w1 = pinned_from_left(c1), e1 = pinned_from_right(c1), w2 = pinned_from_left(c2), e2 = pinned_from_right(c2);
        const double s1 = b1, s2 = b2, n1 = l1[i + 1], n2 = l2[i + 1];
        const double2 uv = st[i * nx + j], tv = tg[i * nx + j];
        const double U = uv.x, V = uv.y;
        const double dl1dx = div_c(e1 - w1, S.two_dx, S.inv_two_dx), dl1dy = div_c(n1 - s1, S.two_dy, S.inv_two_dy);
        const double dl2dx = div_c(e2 - w2, S.two_dx, S.inv_two_dx), dl2dy = div_c(n2 - s2, S.two_dy, S.inv_two_dy);
        const double lap1 = div_c((((w1 + s1) - 4.0 * c1) + e1) + n1, S.dxdy, S.inv_dxdy);
        const double lap2 = div_c((((w2 + s2) - 4.0 * c2) + e2) + n2, S.dxdy, S.inv_dxdy);
        const double d1 = (((((-2.0) * dl1dx) * U - dl1dy * V) - dl2dx * V) - S.nu * lap1) + (U - tv.x);      // :92
        const double d2 = (((((-2.0) * dl2dy) * V - dl1dy * U) - dl2dx * U) - S.nu * lap2) + (V - tv.y);      // :93
        l1[i] = icol ? c1 - S.dt * d1 : 0.0;                      // apply_boundary of the script (:56-61): the four walls are zero
        l2[i] = icol ? c2 - S.dt * d2 : 0.0;
        b1 = c1;
        b2 = c2;
        __builtin_amdgcn_sched_barrier(0);      // one row at a time: interleaved rows multiply the live temporaries
      }
      l1[0] = l1[NY - 1] = l2[0] = l2[NY - 1] = 0.0;
    }
    // ---- pressure = solve_pressure(lam1, lam2, pressure) (:97), warm-started from the previous backward step ----
    {
      double rq[NY];
#pragma unroll
      for (int i = 0; i < NY; ++i) {
        rq[i] = 0.0;
        park[0][i][lane] = l1[i];
        park[1][i][lane] = l2[i];
        if (i >= 1 && i < NY - 1) rq[i] = col_rhs_term<double>(S, l1[i], l2[i + 1], l2[i - 1], icol);
        __builtin_amdgcn_sched_barrier(0);
      }
      wave_lds_sync();
      col_jacobi_solve<double, NY>(p, rq, C.iters, lef, rig, icol, j == 1, j == nx - 2);
    }
    wave_lds_sync();
#pragma unroll
    for (int i = 0; i < NY; ++i) {
      l1[i] = park[0][i][lane];      // written by this same lane above
      l2[i] = park[1][i][lane];
    }
    // ---- lam -= dt * grad p, no division by the density (:98-100); the walls stay zero ----
#pragma unroll
    for (int i = 1; i < NY - 1; ++i) {
      const double pe = pinned_from_right(p[i]), pw = pinned_from_left(p[i]);
      const double dpdx = div_c(pe - pw, S.two_dx, S.inv_two_dx);
      const double dpdy = div_c(p[i + 1] - p[i - 1], S.two_dy, S.inv_two_dy);
      l1[i] = icol ? l1[i] - S.dt * dpdx : 0.0;
      l2[i] = icol ? l2[i] - S.dt * dpdy : 0.0;
      __builtin_amdgcn_sched_barrier(0);
    }
    write_out(T - 2 - k, l1, l2);      // Lam1[::-1] (:103): backward step k lands at time index T - 2 - k
  }
}

bool launch_adjoint(const NSConst& C, const NSScal<double>& S, const AdjointArgs& A, int B, hipStream_t st) {
  const int G = 64 / C.nx;
  const dim3 grid((B + G - 1) / G), block(64);
#define PDEGYM_LAUNCH(NY) case NY: ns_adjoint_march<NY><<<grid, block, 0, st>>>(C, S, A, B); return true;
  switch (C.ny) {
    PDEGYM_LAUNCH(8) PDEGYM_LAUNCH(11) PDEGYM_LAUNCH(16) PDEGYM_LAUNCH(21) PDEGYM_LAUNCH(26) PDEGYM_LAUNCH(31) PDEGYM_LAUNCH(32)
    default: return false;
  }
#undef PDEGYM_LAUNCH
}

}  // namespace

extern "C" {

int pdegym_ns2d_adjoint_f64(const pdegym_params_ns2d* prm, const void* U_ref, int32_t nt_ref, const pdegym_adjoint_ns2d* adj, int32_t B,
                            void* stream) {
  NSConst C;
  NSScal<double> S;
  if (int rc = fill<double>(prm, C, S)) return rc;
  if (!adj) return pdegym::fail(-1, "null adjoint descriptor");
  if (!U_ref) return pdegym::fail(-3, "null U_ref");
  if (!adj->obs || !adj->a_nom || !adj->grad || !adj->actions) return pdegym::fail(-3, "null obs/a_nom/grad/actions");
  if (adj->T < 1) return pdegym::fail(-2, "T must be >= 1");
  if (adj->t0 < 0) return pdegym::fail(-2, "t0 must be >= 0");
  if (nt_ref < 1) return pdegym::fail(-2, "nt_ref must be >= 1");
  // the march moves (u, v) / (lambda1, lambda2) pairs as one naturally aligned 16-byte access
  if (!pdegym::is_aligned(U_ref, 16)) return pdegym::fail(-2, "U_ref must be 16-byte aligned");
  if (!pdegym::is_aligned(adj->obs, 16)) return pdegym::fail(-2, "obs must be 16-byte aligned");
  if (!pdegym::is_aligned(adj->lam, 16)) return pdegym::fail(-2, "lam must be 16-byte aligned");
  const int ny = C.ny;
  if (C.nx > 64 || !(ny == 8 || ny == 11 || ny == 16 || ny == 21 || ny == 26 || ny == 31 || ny == 32))
    return pdegym::fail(-2, "the adjoint march needs a column-kernel grid: 8, 11, 16, 21, 26, 31 or 32 rows, 3 .. 64 columns");
  if (C.action_dim != 1) return pdegym::fail(-2, "the adjoint march needs action_dim == 1 (one command per instance and step)");
  // the zeroed adjoint walls and the gradient row (d lambda1 / dy under the upper wall) belong to this table and no other
  for (int e = 0; e < 4; ++e)
    for (int k = 0; k < 2; ++k) {
      const int want = (e == PDEGYM_EDGE_UPPER && k == 0) ? PDEGYM_BC_CONTROLLABLE : PDEGYM_BC_DIRICHLET;
      if (C.bc[e][k] != want)
        return pdegym::fail(-2, "the adjoint march needs the script's boundary table: upper u Controllable, every other entry Dirichlet");
    }
  if (B <= 0) return 0;
  const AdjointArgs A{adj->T, adj->t0, nt_ref, adj->obs, static_cast<const double*>(U_ref), adj->a_nom, adj->ratio, adj->width, prm->dx,
                      adj->grad, adj->actions, adj->lam};
  if (!launch_adjoint(C, S, A, B, (hipStream_t)stream)) return pdegym::fail(-2, "no adjoint kernel for this grid");
  return pdegym::check_launch("ns2d_adjoint");
}

}  // extern "C"
