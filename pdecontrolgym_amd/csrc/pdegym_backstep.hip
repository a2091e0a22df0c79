// pdegym_backstep.hip -- the backstepping baseline of the reference's result tables on the device (see include/pdegym.h):
//   pdegym_backstep_gain_parabolic   solveKernelFunction   examples/reactionDiffusionPDE/reactionDiffusion1DBackstepping.py:22-35
//   pdegym_backstep_gain_transport   solveKernelFunction   examples/transportPDE/transport1Dbackstepping.py:22-29
//   pdegym_backstep_control          solveControl          transport1Dbackstepping.py:32-36, reactionDiffusion1DBackstepping.py:38-39
// One wave per row of theta (gains) or per instance (control law).  The gains are bit-identical to the reference's: every element
// is the reference's own expression tree (NumPy >= 2 promotion: float32 scalars stay float32 until they meet the float64 kernel),
// and -ffp-contract=off keeps the compiler from fusing any of it.
// Output contracts (poisoned buffers, guard bands) of the three kernels: tests/test_gpu_backstepping.py, KERNEL_CASES there;
// tests/test_backstepping.py fails when a kernel launched here is missing from that table.
#include <hip/hip_runtime.h>

#include <cmath>
#include <type_traits>

#include "pdegym.h"
#include "pdegym_backstep_law.h"
#include "pdegym_common.h"

namespace {

using namespace pdegym::wave;      // kWave, kWavesPerBlock, lane shifts, wave_sum, lane_value, wave_lds_sync, pool_row
using pdegym_backstep_law::chain_add;      // the ordered chain: shared with the control law's dot product (pdegym_backstep_law.h)

// ---- parabolic gain: the last row k[m-1][:] of the reference's m x m kernel matrix ------------------------------------------------
// The reference marches in i: row i+1 from rows i and i-1 at columns j-1, j, j+1 (the shape of the 1D steppers).  Lane l holds the
// E consecutive columns l*E .. l*E+E-1 of the two live rows in registers; the neighbours across a lane boundary come by DPP.  Every
// column evaluates all three forms of the update (interior stencil, sub-diagonal, diagonal) and selects: no lane is ever masked off.
//   k[1][1]     = -(a[1] + a[0]) * dx / 4                          float32 throughout
//   k[i+1][i+1] = k[i][i] - dx/4.0 * (a[i-1] + a[i])               float32 product joins the float64 k
//   k[i+1][i]   = k[i][i] - dx/2 * a[i]
//   k[i+1][j]   = -k[i-1][j] + k[i][j+1] + k[i][j-1] + a[j]*(dx**2)*(k[i][j+1] + k[i][j-1])/2      0 < j < i
template <int E>
__global__ __launch_bounds__(kWave* kWavesPerBlock) void gain_parabolic_kernel(const float* __restrict__ theta,
                                                                               double* __restrict__ gain, int R, int m, float dx,
                                                                               float dx_4, float dx_2, float dx_sq) {
  const int lane = threadIdx.x % kWave;
  const int row = blockIdx.x * kWavesPerBlock + threadIdx.x / kWave;
  if (row >= R) return;      // wave-uniform
  const float* a = theta + (size_t)row * m;
  const int j0 = lane * E;
  double prev[E], cur[E];      // rows i-1 and i
  float c[E], d_sub[E], d_diag[E];
  const float k11 = ((-(a[1] + a[0])) * dx) / 4.0f;
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const int j = j0 + e;
    const float aj = j < m ? a[j] : 0.f;
    const float am1 = (j >= 1 && j - 1 < m) ? a[j - 1] : 0.f;
    const float am2 = (j >= 2 && j - 2 < m) ? a[j - 2] : 0.f;
    c[e] = aj * dx_sq;                 // a[j]*(dx**2)
    d_sub[e] = dx_2 * aj;              // dx/2 * a[i]               where j == i
    d_diag[e] = dx_4 * (am2 + am1);    // dx/4.0 * (a[i-1] + a[i])  where j == i + 1
    prev[e] = 0.0;
    cur[e] = j == 1 ? (double)k11 : 0.0;
  }
  for (int i = 1; i <= m - 2; ++i) {
    const double left_in = pinned_from_left(cur[E - 1]), right_in = pinned_from_right(cur[0]);
    double nxt[E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const int j = j0 + e;
      const double l = e > 0 ? cur[e > 0 ? e - 1 : 0] : left_in, r = e < E - 1 ? cur[e < E - 1 ? e + 1 : 0] : right_in;
      const double inner = ((-prev[e] + r) + l) + (((double)c[e] * (r + l)) / 2.0);
      const double sub = cur[e] - (double)d_sub[e];
      const double diag = l - (double)d_diag[e];
      nxt[e] = (j >= 1 && j < i) ? inner : (j == i ? sub : (j == i + 1 ? diag : 0.0));
    }
#pragma unroll
    for (int e = 0; e < E; ++e) {
      prev[e] = cur[e];
      cur[e] = nxt[e];
    }
  }
  double* out = gain + (size_t)row * m;
#pragma unroll
  for (int e = 0; e < E; ++e)
    if (j0 + e < m) out[j0 + e] = cur[e];
}

// ---- transport gain: kappa[i] = (sum_{j<i} (kappa[i-j]*theta[j])*dx) - theta[i], flipped --------------------------------------------
// kappa lives in LDS (it is read back to front); lane l forms the products of columns j = e*64 + l in parallel, the sum is the
// reference's ordered chain (chain_add).  The j = 0 term reads the not yet written kappa[i] = 0, as the reference does.
template <int E>
__global__ __launch_bounds__(kWave) void gain_transport_kernel(const float* __restrict__ theta, double* __restrict__ gain, int m,
                                                               double dx) {
  __shared__ double kap[PDEGYM_MAX_N1D];
  const int lane = threadIdx.x;
  const float* th = theta + (size_t)blockIdx.x * m;
  float t[E];
#pragma unroll
  for (int e = 0; e < E; ++e) t[e] = e * kWave + lane < m ? th[e * kWave + lane] : 0.f;
  for (int j = lane; j < m; j += kWave) kap[j] = 0.0;
  wave_lds_sync();
  for (int i = 0; i < m; ++i) {
    const float ti = th[i];
    double s = 0.0;
#pragma unroll
    for (int e = 0; e < E; ++e) {
      if (e * kWave < i) {      // wave-uniform
        const int j = e * kWave + lane;
        const double p = j < i ? (kap[i - j] * (double)t[e]) * dx : 0.0;
        s = chain_add(s, p, min(kWave, i - e * kWave));
      }
    }
    if (lane == 0) kap[i] = s - (double)ti;
    wave_lds_sync();
  }
  double* out = gain + (size_t)blockIdx.x * m;
  for (int j = lane; j < m; j += kWave) out[j] = kap[m - 1 - j];
}

// ---- control law: a[b] = (sum_{i<len} gain_row(b)[i] * (double)obs[b, i]) * scale ----------------------------------------------------
template <bool ORDERED>
__global__ __launch_bounds__(kWave* kWavesPerBlock) void backstep_control_kernel(pdegym_backstep A, int B) {
  const int lane = threadIdx.x % kWave;
  const int inst = blockIdx.x * kWavesPerBlock + threadIdx.x / kWave;
  if (inst >= B) return;      // wave-uniform
  const double* g = A.gain0 + (size_t)inst * A.gain_stride;
  // an instance that has restarted c >= 1 times runs the episode the step kernel started from pool row (inst + (c-1)*B) mod rows:
  // the row pool_row() named when the counter still read c - 1
  if (A.gain_pool && A.reset_count[inst] > 0) g = A.gain_pool + (size_t)pool_row(A.pool_rows, A.reset_count, inst, B, -1) * A.m;
  const float* o = A.obs + (size_t)inst * A.obs_stride;
  // both orders of addition: pdegym_backstep_law.h (the one-launch rollout kernel evaluates the same function)
  const double s = pdegym_backstep_law::dot<ORDERED>(A.len, lane, [&](int, int i) { return g[i] * (double)o[i]; });
  const double act = s * A.scale;
  if (lane != 0) return;
  if (A.out64) {
    A.out64[inst] = act;
  } else {
    float f = (float)act;
    if (A.noise) f += A.noise[inst];
    if (A.clamp) f = pdegym::clip_keep_nan(f, A.lo, A.hi);
    A.out32[inst] = f;
  }
}

int check_gain_args(const float* theta, const double* gain, int R, int m, double dx) {
  if (!theta || !gain) return pdegym::fail(-1, "null theta/gain");
  if (R < 0) return pdegym::fail(-2, "R must be >= 0");
  if (m < 2 || m > PDEGYM_MAX_N1D) return pdegym::fail(-2, "m must be in [2, 2048] (PDEGYM_MAX_N1D)");
  if (!std::isfinite(dx) || !(dx > 0.0)) return pdegym::fail(-2, "dx must be a positive finite number");
  return 0;
}

// elements per lane, rounded up to the instantiated widths
template <typename F>
void with_epl(int m, F&& go) {
  const int epl = (m + kWave - 1) / kWave;
  if (epl <= 1) go(std::integral_constant<int, 1>{});
  else if (epl <= 2) go(std::integral_constant<int, 2>{});
  else if (epl <= 4) go(std::integral_constant<int, 4>{});
  else if (epl <= 8) go(std::integral_constant<int, 8>{});
  else if (epl <= 16) go(std::integral_constant<int, 16>{});
  else go(std::integral_constant<int, 32>{});
}

}  // namespace

extern "C" {

int pdegym_backstep_gain_parabolic(const float* theta, double* gain, int32_t R, int32_t m, double dx, void* stream) {
  if (const int rc = check_gain_args(theta, gain, R, m, dx)) return rc;
  if (R == 0) return 0;
  const dim3 grid((R + kWavesPerBlock - 1) / kWavesPerBlock), block(kWave * kWavesPerBlock);
  // the Python doubles dx/4.0, dx/2 and dx**2 are cast to float32 where they meet the float32 scalar a[j]
  const float dxf = (float)dx, dx_4 = (float)(dx / 4.0), dx_2 = (float)(dx / 2.0), dx_sq = (float)(dx * dx);
  with_epl(m, [&](auto tag) {
    constexpr int E = decltype(tag)::value;
    gain_parabolic_kernel<E><<<grid, block, 0, (hipStream_t)stream>>>(theta, gain, R, m, dxf, dx_4, dx_2, dx_sq);
  });
  return pdegym::check_launch("backstep_gain_parabolic");
}

int pdegym_backstep_gain_transport(const float* theta, double* gain, int32_t R, int32_t m, double dx, void* stream) {
  if (const int rc = check_gain_args(theta, gain, R, m, dx)) return rc;
  if (R == 0) return 0;
  with_epl(m, [&](auto tag) {
    constexpr int E = decltype(tag)::value;
    gain_transport_kernel<E><<<dim3(R), dim3(kWave), 0, (hipStream_t)stream>>>(theta, gain, m, dx);
  });
  return pdegym::check_launch("backstep_gain_transport");
}

int pdegym_backstep_control(const pdegym_backstep* c, int32_t B, void* stream) {
  if (!c) return pdegym::fail(-1, "null descriptor");
  if (B <= 0) return 0;
  if (!c->gain0 || !c->obs) return pdegym::fail(-3, "null gain0/obs");
  if ((c->out64 != nullptr) == (c->out32 != nullptr)) return pdegym::fail(-3, "exactly one of out64 / out32 must be given");
  if (c->m < 1 || c->len < 1 || c->len > c->m) return pdegym::fail(-2, "need 1 <= len <= m");
  if (c->gain_stride != 0 && c->gain_stride < c->m) return pdegym::fail(-2, "gain_stride must be 0 (one shared row) or >= m");
  if (c->obs_stride < c->len) return pdegym::fail(-2, "obs_stride shorter than len");
  if (c->order != PDEGYM_BACKSTEP_TREE && c->order != PDEGYM_BACKSTEP_ORDERED) return pdegym::fail(-2, "bad order");
  if (c->gain_pool && !c->reset_count) return pdegym::fail(-3, "gain_pool needs reset_count (which episode an instance is in)");
  if (c->pool_rows < 0) return pdegym::fail(-2, "pool_rows must be >= 0 (0 = B)");
  if (c->out64 && (c->noise || c->clamp)) return pdegym::fail(-2, "noise / clamp belong to the float32 output");
  if (c->clamp && !(c->lo <= c->hi)) return pdegym::fail(-2, "clamp bounds must satisfy lo <= hi");
  const dim3 grid((B + kWavesPerBlock - 1) / kWavesPerBlock), block(kWave * kWavesPerBlock);
  if (c->order == PDEGYM_BACKSTEP_ORDERED)
    backstep_control_kernel<true><<<grid, block, 0, (hipStream_t)stream>>>(*c, B);
  else
    backstep_control_kernel<false><<<grid, block, 0, (hipStream_t)stream>>>(*c, B);
  return pdegym::check_launch("backstep_control");
}

}  // extern "C"
