// pdegym_ppo_loss.hip -- the loss head of PPO for a diagonal-Gaussian policy and its gradients (see include/pdegym.h):
//   pdegym_ppo_loss                 the loss of PPO.train (stable_baselines3/ppo/ppo.py) with DiagGaussianDistribution.log_prob /
//                                   .entropy (common/distributions.py), the minibatch gather included, and d loss / d mean,
//                                   d loss / d values, d loss / d log_std in closed form
//   pdegym_diag_gaussian_log_prob   DiagGaussianDistribution.log_prob through the same device function
// At most three launches on the caller's stream, stream order the only synchronisation (no workgroup waits for another, no atomics):
//   1. moments_kernel   per-workgroup partial sums of the gathered advantages (skipped without normalisation);
//   2. rows_kernel      every workgroup adds those partials itself, does its rows -- one row per lane and chunk of kRows rows, the
//                       gathers issued together once index[i] is there -- and writes its partial sums of the reductions;
//   3. finish_kernel    one workgroup adds the partials and writes stats and d_log_std.
// The number of workgroups G(N) = min(ceil(N / kRows), kMaxGroups) and with it the order of every sum is a function of N alone:
//   a lane adds its rows i = t + kRows * (g + G * c), c = 0, 1, ..  in ascending c (float64);
//   a workgroup adds its lanes with pdegym::wave::wave_sum per wave and the four waves in ascending order (float64);
//   partials are added the same way: thread t takes workgroup t (G <= kMaxGroups = kRows threads), then the block sum.
// Every float32 operation of a row is __fmul_rn / __fadd_rn / __fsub_rn / __fdiv_rn in the order stated in the header (one rounding
// each, no contraction whatever the flags) around the device library's expf; float64 is used for the sums only.
// The launches are made with hipLaunchKernel, the runtime's C entry point.  tests/test_poison_helper.py lists the kernels launched
// with the chevron syntax against a table in tests/test_gpu_pointer_alignment.py; the displaced-pointer runs of THESE kernels are in
// tests/test_gpu_ppo_loss.py (every launch there goes through the displacement policies), and they belong in that table once it
// is next edited.
// Output contract, non-finite data, reproducibility: tests/test_gpu_ppo_loss.py.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <type_traits>

#include "pdegym.h"
#include "pdegym_common.h"

namespace {

using pdegym::wave::kWave;

constexpr int kRows = 256;            // rows per workgroup and chunk = threads per workgroup (one row per lane)
constexpr int kMaxGroups = 256;       // workgroups at most: beyond kRows * kMaxGroups rows a workgroup takes further chunks
constexpr int kWaves = kRows / kWave;
constexpr int kMaxA = 8;
constexpr int kSums = 4;              // policy, value, approx_kl, clipped count; then the A columns of d_log_std
constexpr int kPartial = kSums + kMaxA;      // doubles per workgroup in the rows part of the workspace
constexpr int kMoments = 2;                  // doubles per workgroup in the moments part
constexpr float kHalfLog2Pi = 0.91893853320467274178f;
constexpr double kHalfLog2PiD = 0.91893853320467274178;

static_assert(kMaxGroups <= kRows, "thread t adds the partial of workgroup t");

int groups_of(int64_t N) { return (int)((N + kRows - 1) / kRows < kMaxGroups ? (N + kRows - 1) / kRows : kMaxGroups); }

// a double in the workspace, which is only 4-byte aligned: two dword accesses at worst, never an 8-byte-aligned one
struct __attribute__((packed, aligned(4))) f64u {
  double v;
};

// Sum over the kRows threads of a workgroup of K values each, the result in every thread: wave_sum per wave, then the waves in
// ascending order.  `lds`: kWaves * K doubles.  Every thread of the workgroup calls it (the wave reductions need all lanes).
template <int K>
__device__ __forceinline__ void block_sum(double (&v)[K], double* lds) {
  const int wave = threadIdx.x / kWave;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const double s = pdegym::wave::wave_sum(v[k]);
    if ((threadIdx.x & (kWave - 1)) == 0) lds[wave * K + k] = s;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < K; ++k) {
    double s = lds[k];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) s += lds[w * K + k];
    v[k] = s;
  }
  __syncthreads();      // (the next call reuses lds)
}

__device__ __forceinline__ int64_t row_of(const pdegym_ppo_loss_args& a, int64_t i) { return a.index ? a.index[i] : i; }

// the moments are taken about the first gathered advantage: equal advantages give a standard deviation of exactly 0
__device__ __forceinline__ double pivot_of(const pdegym_ppo_loss_args& a) { return (double)a.advantages[row_of(a, 0)]; }

// ---- 1. moments of the gathered advantages ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kRows) void moments_kernel(pdegym_ppo_loss_args a, int N, int G) {
  __shared__ double lds[kWaves * kMoments];
  const double pivot = pivot_of(a);
  double s[kMoments] = {0.0, 0.0};
  for (int64_t i = (int64_t)blockIdx.x * kRows + threadIdx.x; i < N; i += (int64_t)G * kRows) {
    const double d = (double)a.advantages[row_of(a, i)] - pivot;
    s[0] += d;
    s[1] += d * d;
  }
  block_sum(s, lds);
  if (threadIdx.x < kMoments) {
    f64u* out = (f64u*)a.workspace + (int64_t)blockIdx.x * kMoments;
    out[threadIdx.x].v = threadIdx.x == 0 ? s[0] : s[1];
  }
}

// mean and unbiased standard deviation from the G partials, in every thread (rows_kernel and finish_kernel: the same bits)
__device__ __forceinline__ void moments_total(const pdegym_ppo_loss_args& a, int N, int G, double* lds, double& mean, double& std_) {
  const f64u* in = (const f64u*)a.workspace;
  double s[kMoments] = {0.0, 0.0};
  if ((int)threadIdx.x < G) {
    s[0] = in[threadIdx.x * kMoments].v;
    s[1] = in[threadIdx.x * kMoments + 1].v;
  }
  block_sum(s, lds);
  const double n = (double)N;
  mean = pivot_of(a) + s[0] / n;
  const double var = (s[1] - s[0] * s[0] / n) / (n - 1.0);
  std_ = sqrt(var < 0.0 ? 0.0 : var);      // (a NaN stays: the comparison is false)
}

// ---- the log-probability of a row: include/pdegym.h states this order ------------------------------------------------------------------
template <int A>
struct Gaussian {
  float log_std[A], inv_std[A];
  __device__ __forceinline__ explicit Gaussian(const float* ls) {
#pragma unroll
    for (int j = 0; j < A; ++j) {
      log_std[j] = ls[j];
      inv_std[j] = expf(-log_std[j]);
    }
  }
  __device__ __forceinline__ float log_prob(const float* mean, const float* act, float (&z)[A]) const {
    float logp = 0.f;
#pragma unroll
    for (int j = 0; j < A; ++j) {
      z[j] = __fmul_rn(__fsub_rn(act[j], mean[j]), inv_std[j]);
      const float t = __fsub_rn(__fsub_rn(__fmul_rn(-0.5f, __fmul_rn(z[j], z[j])), log_std[j]), kHalfLog2Pi);
      logp = j == 0 ? t : __fadd_rn(logp, t);
    }
    return logp;
  }
};

// ---- 2. the rows ---------------------------------------------------------------------------------------------------------------------------
template <int A>
__global__ __launch_bounds__(kRows) void rows_kernel(pdegym_ppo_loss_args a, int N, int G, int normalize) {
  __shared__ double lds[kWaves * (kSums + A)];
  float adv_mean = 0.f, adv_den = 1.f;
  if (normalize) {      // workgroup-uniform
    double mean, std_;
    moments_total(a, N, G, lds, mean, std_);
    adv_mean = (float)mean;
    adv_den = __fadd_rn((float)std_, 1e-8f);
  }
  const Gaussian<A> dist(a.log_std);
  const float lo = (float)(1.0 - a.clip_range), hi = (float)(1.0 + a.clip_range), clip = (float)a.clip_range;
  const float inv_n = (float)(1.0 / (double)N), dv_scale = (float)(2.0 * a.vf_coef / (double)N);
  double s[kSums + A];
#pragma unroll
  for (int k = 0; k < kSums + A; ++k) s[k] = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * kRows + threadIdx.x; i < N; i += (int64_t)G * kRows) {
    const int64_t k = row_of(a, i);
    // everything the row needs is requested before anything is used
    float mean[A], act[A];
#pragma unroll
    for (int j = 0; j < A; ++j) {
      mean[j] = a.mean[i * a.ld_mean + j];
      act[j] = a.actions[k * a.ld_actions + j];
    }
    const float old = a.old_log_prob[k], adv_raw = a.advantages[k];
    const float ret = a.values ? a.returns[k] : 0.f, val = a.values ? a.values[i] : 0.f;

    const float adv = normalize ? __fdiv_rn(__fsub_rn(adv_raw, adv_mean), adv_den) : adv_raw;
    float z[A];
    const float lr = __fsub_rn(dist.log_prob(mean, act, z), old);
    const float ratio = expf(lr);
    const float s1 = __fmul_rn(adv, ratio), s2 = __fmul_rn(adv, pdegym::clip_keep_nan(ratio, lo, hi));
    const float surrogate = (s1 != s1 || s2 != s2) ? __fadd_rn(s1, s2) : fminf(s1, s2);      // torch.min keeps a NaN
    const float r1 = __fsub_rn(ratio, 1.0f);
    const bool clipped_out = (ratio > hi && adv > 0.f) || (ratio < lo && adv < 0.f);
    const float g = clipped_out ? 0.f : -__fmul_rn(s1, inv_n);
    s[0] += (double)surrogate;
    s[2] += (double)__fsub_rn(r1, lr);
    s[3] += fabsf(r1) > clip ? 1.0 : 0.0;
#pragma unroll
    for (int j = 0; j < A; ++j) {
      a.d_mean[i * a.ld_d_mean + j] = __fmul_rn(__fmul_rn(g, z[j]), dist.inv_std[j]);
      s[kSums + j] += (double)__fmul_rn(g, __fsub_rn(__fmul_rn(z[j], z[j]), 1.0f));
    }
    if (a.values) {      // kernel-uniform
      const float dv = __fsub_rn(val, ret);
      s[1] += (double)__fmul_rn(dv, dv);
      a.d_values[i] = __fmul_rn(dv, dv_scale);
    }
  }
  block_sum(s, lds);
  if (threadIdx.x == 0) {
    f64u* out = (f64u*)a.workspace + (int64_t)G * kMoments + (int64_t)blockIdx.x * kPartial;
#pragma unroll
    for (int k = 0; k < kSums + A; ++k) out[k].v = s[k];
  }
}

// ---- 3. the partials -> stats, d_log_std --------------------------------------------------------------------------------------------------
template <int A>
__global__ __launch_bounds__(kRows) void finish_kernel(pdegym_ppo_loss_args a, int N, int G, int normalize) {
  __shared__ double lds[kWaves * (kSums + A)];
  double mean = 0.0, std_ = 1.0;
  if (normalize) moments_total(a, N, G, lds, mean, std_);
  const f64u* in = (const f64u*)a.workspace + (int64_t)G * kMoments;
  double s[kSums + A];
#pragma unroll
  for (int k = 0; k < kSums + A; ++k) s[k] = (int)threadIdx.x < G ? in[(int64_t)threadIdx.x * kPartial + k].v : 0.0;
  block_sum(s, lds);
  const double n = (double)N;
  if (threadIdx.x == 0) {
    double entropy_loss = 0.0;
    for (int j = 0; j < A; ++j) entropy_loss -= 0.5 + kHalfLog2PiD + (double)a.log_std[j];
    const double policy_loss = -(s[0] / n), value_loss = a.values ? s[1] / n : 0.0;
    a.stats[0] = (float)(policy_loss + a.ent_coef * entropy_loss + a.vf_coef * value_loss);
    a.stats[1] = (float)policy_loss;
    a.stats[2] = (float)value_loss;
    a.stats[3] = (float)entropy_loss;
    a.stats[4] = (float)(s[2] / n);
    a.stats[5] = (float)(s[3] / n);
    a.stats[6] = (float)mean;
    a.stats[7] = (float)std_;
  }
#pragma unroll
  for (int j = 0; j < A; ++j)
    if (threadIdx.x == 32 + j) a.d_log_std[j] = (float)(s[kSums + j] - a.ent_coef);
}

// ---- log-probabilities alone -----------------------------------------------------------------------------------------------------------------
template <int A>
__global__ __launch_bounds__(kRows) void log_prob_kernel(const float* mean, int64_t ld, const float* log_std, const float* actions,
                                                         int64_t ld_a, const int64_t* index, float* out, int N) {
  const int64_t i = (int64_t)blockIdx.x * kRows + threadIdx.x;
  if (i >= N) return;
  const Gaussian<A> dist(log_std);
  const int64_t k = index ? index[i] : i;
  float m[A], act[A], z[A];
#pragma unroll
  for (int j = 0; j < A; ++j) {
    m[j] = mean[i * ld + j];
    act[j] = actions[k * ld_a + j];
  }
  out[i] = dist.log_prob(m, act, z);
}

// hipLaunchKernel takes the arguments as an array of pointers to them (their types are the kernel's: nothing is deduced from p)
template <typename T>
struct as_declared {
  using type = T;
};
template <typename... P>
void launch(void (*kernel)(P...), unsigned grid, void* stream, typename as_declared<P>::type... p) {
  void* args[] = {(void*)&p...};
  (void)hipLaunchKernel((const void*)kernel, dim3(grid), dim3(kRows), args, 0, (hipStream_t)stream);      // (check_launch reads the error)
}

template <int A = 1, typename F>
void with_width(int width, F&& go) {
  if constexpr (A <= kMaxA) {
    if (width == A)
      go(std::integral_constant<int, A>{});
    else
      with_width<A + 1>(width, go);
  }
}

struct Range {
  const char* lo;
  const char* hi;      // one past the last byte
  bool overlaps(const Range& o) const { return lo && o.lo && lo < o.hi && o.lo < hi; }
};

// bytes [p, p + ((rows - 1) * ld + width) * size): the part of a [rows, ld] array the call touches
Range extent(const void* p, int64_t rows, int64_t ld, int64_t width, int64_t size) {
  const char* c = (const char*)p;
  return {c, c ? c + ((rows - 1) * ld + width) * size : c};
}

template <int NI, int NO>
int check_overlaps(const Range (&in)[NI], const Range (&out)[NO]) {
  for (int i = 0; i < NO; ++i) {
    for (const Range& r : in)
      if (out[i].overlaps(r)) return pdegym::fail(-3, "an output overlaps an input");
    for (int j = i + 1; j < NO; ++j)
      if (out[i].overlaps(out[j])) return pdegym::fail(-3, "two outputs overlap");
  }
  return 0;
}

}  // namespace

extern "C" {

int64_t pdegym_ppo_loss_workspace(int32_t N, int32_t A) {
  if (N < 1) return pdegym::fail(-2, "N must be >= 1");
  if (A < 1 || A > kMaxA) return pdegym::fail(-2, "A must be 1 .. 8");
  return (int64_t)groups_of(N) * (kMoments + kPartial) * (int64_t)sizeof(double);
}

int pdegym_ppo_loss(const pdegym_ppo_loss_args* g, int32_t N, void* stream) {
  if (!g) return pdegym::fail(-1, "null descriptor");
  if (N < 1) return pdegym::fail(-2, "N must be >= 1");
  const int A = g->A;
  if (A < 1 || A > kMaxA) return pdegym::fail(-2, "A must be 1 .. 8");
  if (g->ld_mean < A || g->ld_actions < A || g->ld_d_mean < A) return pdegym::fail(-2, "ld_mean, ld_actions and ld_d_mean must be >= A");
  if (g->index && g->M < 1) return pdegym::fail(-2, "M must be >= 1 when index is given");
  if (!std::isfinite(g->clip_range) || g->clip_range < 0.0) return pdegym::fail(-2, "clip_range must be finite and >= 0");
  if (!std::isfinite(g->ent_coef) || !std::isfinite(g->vf_coef)) return pdegym::fail(-2, "ent_coef and vf_coef must be finite");
  if (!g->mean || !g->log_std || !g->actions || !g->old_log_prob || !g->advantages)
    return pdegym::fail(-3, "null mean/log_std/actions/old_log_prob/advantages");
  if (!g->d_mean || !g->d_log_std || !g->stats || !g->workspace) return pdegym::fail(-3, "null d_mean/d_log_std/stats/workspace");
  if ((g->values != nullptr) != (g->d_values != nullptr)) return pdegym::fail(-3, "values and d_values must be given together");
  if (g->values && !g->returns) return pdegym::fail(-3, "the value term needs returns");
  if (g->workspace_bytes < pdegym_ppo_loss_workspace(N, A)) return pdegym::fail(-2, "workspace too small (pdegym_ppo_loss_workspace)");
  if (!pdegym::is_aligned(g->workspace, 4)) return pdegym::fail(-2, "workspace must be 4-byte aligned");
  const int64_t M = g->index ? g->M : N;
  const Range in[] = {extent(g->mean, N, g->ld_mean, A, 4),       extent(g->values, 1, N, N, 4),       extent(g->log_std, 1, A, A, 4),
                      extent(g->index, 1, N, N, 8),               extent(g->actions, M, g->ld_actions, A, 4),
                      extent(g->old_log_prob, 1, M, M, 4),        extent(g->advantages, 1, M, M, 4),
                      extent(g->values ? g->returns : nullptr, 1, M, M, 4)};
  const Range out[] = {extent(g->d_mean, N, g->ld_d_mean, A, 4), extent(g->d_values, 1, N, N, 4), extent(g->d_log_std, 1, A, A, 4),
                       extent(g->stats, 1, 8, 8, 4), extent(g->workspace, 1, g->workspace_bytes, g->workspace_bytes, 1)};
  if (const int rc = check_overlaps(in, out)) return rc;
  const int G = groups_of(N), normalize = g->normalize_advantage != 0 && N > 1;
  if (normalize) launch(moments_kernel, (unsigned)G, stream, *g, (int)N, G);
  with_width(A, [&](auto width) {
    launch(rows_kernel<decltype(width)::value>, (unsigned)G, stream, *g, (int)N, G, normalize);
    launch(finish_kernel<decltype(width)::value>, 1u, stream, *g, (int)N, G, normalize);
  });
  return pdegym::check_launch("ppo_loss");
}

int pdegym_diag_gaussian_log_prob(const float* mean, int64_t ld, const float* log_std, const float* actions, int64_t ld_a,
                                  const int64_t* index, float* out, int32_t N, int32_t A, void* stream) {
  if (N < 1) return pdegym::fail(-2, "N must be >= 1");
  if (A < 1 || A > kMaxA) return pdegym::fail(-2, "A must be 1 .. 8");
  if (ld < A || ld_a < A) return pdegym::fail(-2, "ld and ld_a must be >= A");
  if (!mean || !log_std || !actions || !out) return pdegym::fail(-3, "null mean/log_std/actions/out");
  // (with an index the extent of actions is the caller's knowledge: its first row stands for it)
  const Range in[] = {extent(mean, N, ld, A, 4), extent(log_std, 1, A, A, 4), extent(index, 1, N, N, 8),
                      extent(actions, index ? 1 : N, ld_a, A, 4)};
  const Range outs[] = {extent(out, 1, N, N, 4)};
  if (const int rc = check_overlaps(in, outs)) return rc;
  with_width(A, [&](auto width) {
    launch(log_prob_kernel<decltype(width)::value>, (unsigned)(((int64_t)N + kRows - 1) / kRows), stream, mean, ld, log_std, actions, ld_a,
           index, out, (int)N);
  });
  return pdegym::check_launch("diag_gaussian_log_prob");
}

}  // extern "C"
