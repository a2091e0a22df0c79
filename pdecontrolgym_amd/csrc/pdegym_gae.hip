// pdegym_gae.hip -- GAE(lambda) advantages, returns and episode statistics of a [T, B] rollout in one launch (see include/pdegym.h):
//   pdegym_gae   RolloutBuffer.compute_returns_and_advantage   stable_baselines3/common/buffers.py
//                + the truncation bootstrap of OnPolicyAlgorithm.collect_rollouts   common/on_policy_algorithm.py
// One lane per environment, workgroups of ONE wave: the recurrence is serial in t and independent across environments, rows
// [t, b .. b+63] are read and written coalesced, and B = 4096 spreads over 64 compute units instead of 16.  No LDS, no barriers, no
// atomics, no cross-lane operation.  The dependent chain of a step is one multiply and one add (last -> (gl*nn)*last -> + delta);
// everything else hangs on loads that do not depend on it, so the reverse loop is unrolled kSteps = 16 times with the loads of all
// those steps issued first: a wave pays one memory round trip per 16 steps, and the chain of step j waits (counted vmcnt) only for
// the loads of steps <= j.  values[t+1] is carried in a register.  The episode statistics run FORWARD in t, so they are a second
// workgroup row of the same launch (blockIdx.y == 1) with the same loop shape: both directions run side by side.
// With at most one wave per compute unit nothing hides an instruction's issue: the loops count instructions (moving per-lane
// pointers instead of a 64-bit scalar multiply per row address, no per-step branch in the main loops).
// (Loads carried across the back edge -- block k+1 requested while block k computes -- were tried: the register allocator answers
// the loop-carried values with a copy of the youngest load at the loop header, i.e. a vmcnt(0) per iteration, which is this loop
// with more registers.)
// Every float32 operation is __fmul_rn / __fadd_rn / __fsub_rn: one rounding each, no contraction whatever the flags.
// Output contract, batch invariance, non-finite data: tests/test_gpu_gae.py.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <type_traits>

#include "pdegym.h"
#include "pdegym_common.h"

namespace {

using pdegym::wave::kWave;

// Steps per iteration of the main loops.  With the optional arrays a step is five loads, so an iteration has up to 80 loads in
// flight (vmcnt tells 63 apart: the first waits of such an iteration are a little early, nothing more), and the registers of 16
// steps (<= 16 * 6) are a fraction of the file a lone wave owns.
constexpr int kSteps = 16;

template <bool F64>
using reward_t = std::conditional_t<F64, double, float>;

template <bool F64>
struct Step {
  float v, boot;
  reward_t<F64> r;
  uint8_t te, tr;
};

// Per-lane pointers to element (t, b) of every input, moved a row at a time: one vector add per array and step, and no scalar
// 64-bit multiply per row address (a lone wave pays for every instruction it issues, scalar ones included).
template <bool F64, bool TRUNC, bool BOOT, bool VALUES>
struct Cursor {
  const reward_t<F64>* r;
  const float *v, *boot;
  const uint8_t *te, *tr;
  __device__ __forceinline__ Cursor(const pdegym_gae_args& A, int64_t at)
      : r((const reward_t<F64>*)A.rewards + at), v(A.values + at), boot(A.boot + at), te(A.terminated + at), tr(A.truncated + at) {}
  __device__ __forceinline__ Step<F64> load() const {
    Step<F64> s;
    s.r = *r;
    s.te = *te;
    s.tr = TRUNC ? *tr : (uint8_t)0;
    s.v = VALUES ? *v : 0.f;
    s.boot = (BOOT && VALUES) ? *boot : 0.f;
    return s;
  }
  __device__ __forceinline__ Cursor moved(int64_t elements) const {
    Cursor c = *this;
    c.r += elements, c.v += elements, c.boot += elements, c.te += elements, c.tr += elements;      // (unused ones are never read)
    return c;
  }
};

// ---- advantages and returns: t = T-1 .. 0 -------------------------------------------------------------------------------------------
// Main loop: kSteps whole steps per iteration, all their loads first.  Tail (T % kSteps steps, at t = top .. 0): the same shape once
// more; the slots below t = 0 load row 0 again (in bounds), compute on it and store nothing -- they come after every real step.
template <bool F64, bool TRUNC, bool BOOT>
__device__ __forceinline__ void gae_pass(const pdegym_gae_args& A, int64_t b0, unsigned lane) {
  const int T = A.T;
  const int64_t ld = A.ld, at = (int64_t)(T - 1) * ld + b0 + lane;
  const float g = (float)A.gamma, gl = (float)(A.gamma * A.gae_lambda);
  float v_next = A.values[at + ld], last = 0.f;
  Cursor<F64, TRUNC, BOOT, true> in(A, at);
  float *adv = A.advantages + at, *ret = A.returns + at;
  Step<F64> S[kSteps];
  auto step = [&](const Step<F64>& s) {
    const float nn = __fsub_rn(1.0f, (s.te | s.tr) ? 1.0f : 0.0f);
    float r = (float)s.r;
    if (BOOT) r = (s.tr && !s.te) ? __fadd_rn(r, __fmul_rn(g, s.boot)) : r;
    const float delta = __fsub_rn(__fadd_rn(r, __fmul_rn(__fmul_rn(g, v_next), nn)), s.v);
    last = __fadd_rn(delta, __fmul_rn(__fmul_rn(gl, nn), last));
    v_next = s.v;
  };
  int top = T - 1;
  for (; top >= kSteps - 1; top -= kSteps) {
#pragma unroll
    for (int j = 0; j < kSteps; ++j) {
      S[j] = in.load();
      in = in.moved(-ld);
    }
#pragma unroll
    for (int j = 0; j < kSteps; ++j) {
      step(S[j]);
      *adv = last;
      *ret = __fadd_rn(last, S[j].v);
      adv -= ld, ret -= ld;
    }
  }
  if (top < 0) return;      // wave-uniform
#pragma unroll
  for (int j = 0; j < kSteps; ++j) S[j] = in.moved(-(int64_t)min(j, top) * ld).load();
#pragma unroll
  for (int j = 0; j < kSteps; ++j) {
    step(S[j]);
    if (j <= top) {      // wave-uniform
      adv[-(int64_t)j * ld] = last;
      ret[-(int64_t)j * ld] = __fadd_rn(last, S[j].v);
    }
  }
}

// ---- episode statistics: t = 0 .. T-1, in double ---------------------------------------------------------------------------------------
// The same two loops forward; the tail's slots past T-1 load row T-1 again and are skipped whole (the accumulators outlive them).
template <bool F64, bool TRUNC>
__device__ __forceinline__ void stats_pass(const pdegym_gae_args& A, int64_t b0, unsigned lane) {
  const int T = A.T;
  const int64_t ld = A.ld, at = b0 + lane;
  double acc = A.ep_return_acc ? A.ep_return_acc[at] : 0.0;
  int32_t len = A.ep_length_acc ? A.ep_length_acc[at] : 0;
  Cursor<F64, TRUNC, false, false> in(A, at);
  double* ep_ret = A.episode_return + at;
  int32_t* ep_len = A.episode_length + at;
  Step<F64> S[kSteps];
  auto step = [&](const Step<F64>& s, double* out_ret, int32_t* out_len) {
    const bool done = (s.te | s.tr) != 0;
    acc += (double)s.r;
    len += 1;
    *out_ret = done ? acc : 0.0;
    *out_len = done ? len : 0;
    acc = done ? 0.0 : acc;
    len = done ? 0 : len;
  };
  int t0 = 0;
  for (; t0 + kSteps <= T; t0 += kSteps) {
#pragma unroll
    for (int j = 0; j < kSteps; ++j) {
      S[j] = in.load();
      in = in.moved(ld);
    }
#pragma unroll
    for (int j = 0; j < kSteps; ++j) {
      step(S[j], ep_ret, ep_len);
      ep_ret += ld, ep_len += ld;
    }
  }
  const int left = T - t0;      // 0 .. kSteps-1
  if (left > 0) {               // wave-uniform
#pragma unroll
    for (int j = 0; j < kSteps; ++j) S[j] = in.moved((int64_t)min(j, left - 1) * ld).load();
#pragma unroll
    for (int j = 0; j < kSteps; ++j)
      if (j < left) step(S[j], ep_ret + (int64_t)j * ld, ep_len + (int64_t)j * ld);      // wave-uniform
  }
  if (A.ep_return_acc) {
    A.ep_return_acc[at] = acc;
    A.ep_length_acc[at] = len;
  }
}

template <bool F64, bool TRUNC, bool BOOT>
__global__ __launch_bounds__(kWave) void gae_kernel(pdegym_gae_args A, int B) {
  const int64_t b0 = (int64_t)blockIdx.x * kWave;      // the wave's first column
  const unsigned lane = threadIdx.x;
  if (b0 + lane >= B) return;
  if (blockIdx.y == 0)      // workgroup-uniform
    gae_pass<F64, TRUNC, BOOT>(A, b0, lane);
  else
    stats_pass<F64, TRUNC>(A, b0, lane);
}

struct Range {
  const char* lo;
  const char* hi;      // one past the last byte
  bool overlaps(const Range& o) const { return lo && o.lo && lo < o.hi && o.lo < hi; }
};

// bytes [p, p + ((rows - 1) * ld + B) * size): the part of a [rows, ld] array the call touches
Range extent(const void* p, int64_t rows, int64_t ld, int64_t B, int64_t size) {
  const char* c = (const char*)p;
  return {c, c ? c + ((rows - 1) * ld + B) * size : c};
}

template <bool... Done, typename F>
void with_flags(F&& go) {
  go(std::integral_constant<bool, Done>{}...);
}
template <bool... Done, typename F, typename... Rest>
void with_flags(F&& go, bool first, Rest... rest) {
  if (first)
    with_flags<Done..., true>(go, rest...);
  else
    with_flags<Done..., false>(go, rest...);
}

}  // namespace

extern "C" {

int pdegym_gae(const pdegym_gae_args* g, int32_t B, void* stream) {
  if (!g) return pdegym::fail(-1, "null descriptor");
  if (g->T < 1) return pdegym::fail(-2, "T must be >= 1");
  if (B < 1) return pdegym::fail(-2, "B must be >= 1");
  if (g->ld < B) return pdegym::fail(-2, "ld must be >= B");
  if (!std::isfinite(g->gamma) || !std::isfinite(g->gae_lambda)) return pdegym::fail(-2, "gamma and gae_lambda must be finite");
  if (!g->rewards || !g->values || !g->terminated) return pdegym::fail(-3, "null rewards/values/terminated");
  if (!g->advantages || !g->returns) return pdegym::fail(-3, "null advantages/returns");
  if ((g->episode_return != nullptr) != (g->episode_length != nullptr))
    return pdegym::fail(-3, "episode_return and episode_length must be given together");
  if ((g->ep_return_acc != nullptr) != (g->ep_length_acc != nullptr))
    return pdegym::fail(-3, "ep_return_acc and ep_length_acc must be given together");
  if (g->ep_return_acc && !g->episode_return) return pdegym::fail(-3, "the accumulators need episode_return / episode_length");
  const int64_t T = g->T, ld = g->ld;
  const Range in[] = {extent(g->rewards, T, ld, B, g->rewards_f64 ? 8 : 4), extent(g->values, T + 1, ld, B, 4),
                      extent(g->terminated, T, ld, B, 1), extent(g->truncated, T, ld, B, 1), extent(g->boot, T, ld, B, 4)};
  const Range out[] = {extent(g->advantages, T, ld, B, 4),     extent(g->returns, T, ld, B, 4),
                       extent(g->episode_return, T, ld, B, 8), extent(g->episode_length, T, ld, B, 4),
                       extent(g->ep_return_acc, 1, B, B, 8),   extent(g->ep_length_acc, 1, B, B, 4)};
  constexpr int n_out = sizeof out / sizeof out[0];
  for (int i = 0; i < n_out; ++i) {
    for (const Range& r : in)
      if (out[i].overlaps(r)) return pdegym::fail(-3, "an output overlaps an input");
    for (int j = i + 1; j < n_out; ++j)
      if (out[i].overlaps(out[j])) return pdegym::fail(-3, "two outputs overlap");
  }
  const dim3 grid((unsigned)(((int64_t)B + kWave - 1) / kWave), g->episode_return ? 2 : 1), block(kWave);
  with_flags(
      [&](auto f64, auto trunc, auto boot) {
        gae_kernel<decltype(f64)::value, decltype(trunc)::value, decltype(boot)::value><<<grid, block, 0, (hipStream_t)stream>>>(*g, B);
      },
      g->rewards_f64 != 0, g->truncated != nullptr, g->boot != nullptr);
  return pdegym::check_launch("gae");
}

}  // extern "C"
