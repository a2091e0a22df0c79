// pdegym_sac_loss.hip -- the loss heads of SAC for a squashed-Gaussian actor and twin critics (see include/pdegym.h):
//   pdegym_squashed_gaussian_sample            a = tanh(mu + exp(clip(log_std)) * eps) and SB3's SquashedDiagGaussianDistribution
//                                              .log_prob of it (common/distributions.py, epsilon 1e-6), optionally written behind the
//                                              observation columns of a [N, D + A] block (the critics' input)          -- one launch
//   pdegym_squashed_gaussian_sample_backward   d_raw from d_actions and / or d_log_prob; a, w, u, sigma are recomputed from raw and
//                                              eps, the forward launch saves nothing                                    -- one launch
//   pdegym_sac_critic_loss                     the soft Bellman target, 0.5 * sum_c mse(q_c, y) and d loss / d q_c     -- two launches
//   pdegym_sac_actor_loss                      mean(alpha * logp - min_c q_c), the entropy-coefficient loss and their gradients
//                                                                                                                      -- two launches
// The sample kernels do one row per lane.  The loss kernels are rows + finish, as in pdegym_ppo_loss.hip, stream order the only
// synchronisation (no workgroup waits for another, no atomics).  The number of workgroups G(N) = min(ceil(N / kRows), kMaxGroups)
// and with it the order of every sum is a function of N alone:
//   a lane adds its rows i = t + kRows * (g + G * c), c = 0, 1, ..  in ascending c (float64);
//   a workgroup adds its lanes with pdegym::wave::wave_sum per wave and the four waves in ascending order (float64);
//   partials are added the same way: thread t takes workgroup t (G <= kMaxGroups = kRows threads), then the block sum.
// Every float32 operation of a row is __fmul_rn / __fadd_rn / __fsub_rn / __fdiv_rn in the order stated in the header (one rounding
// each, no contraction whatever the flags) around the device library's expf, tanhf and logf; float64 is used for the sums only.
// The launches are made with hipLaunchKernel, the runtime's C entry point; the displaced-pointer runs of
// these kernels are in tests/test_gpu_sac_loss.py (every launch there goes through the displacement policies).
// Output contract, non-finite data, reproducibility: tests/test_gpu_sac_loss.py.
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
constexpr int kCriticSums = 5;        // e_1^2, e_2^2, q1, q2, y
constexpr int kActorSums = 3;         // alpha * logp - m, logp + target_entropy, logp
constexpr int kPartial = kCriticSums; // doubles per workgroup in the workspace (both heads)
constexpr float kHalfLog2Pi = 0.91893853320467274178f;
constexpr float kEpsilon = 1e-6f;     // SB3's SquashedDiagGaussianDistribution(epsilon=1e-6)

static_assert(kMaxGroups <= kRows, "thread t adds the partial of workgroup t");
static_assert(kActorSums <= kPartial, "one workspace size for both heads");

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
  __syncthreads();
}

template <int K>
__device__ __forceinline__ void store_partials(void* workspace, const double (&s)[K]) {
  if (threadIdx.x == 0) {
    f64u* out = (f64u*)workspace + (int64_t)blockIdx.x * kPartial;
#pragma unroll
    for (int k = 0; k < K; ++k) out[k].v = s[k];
  }
}

template <int K>
__device__ __forceinline__ void total_of_partials(const void* workspace, int G, double (&s)[K], double* lds) {
  const f64u* in = (const f64u*)workspace;
#pragma unroll
  for (int k = 0; k < K; ++k) s[k] = (int)threadIdx.x < G ? in[(int64_t)threadIdx.x * kPartial + k].v : 0.0;
  block_sum(s, lds);
}

// torch.min of two floats: a NaN in either is the result
__device__ __forceinline__ float min_keep_nan(float a, float b) { return (a != a || b != b) ? __fadd_rn(a, b) : fminf(a, b); }

// ---- the squashed Gaussian of one column: include/pdegym.h states this order -------------------------------------------------------
struct Squashed {
  float ls, sigma, a, w, u;
  __device__ __forceinline__ Squashed(float mu, float log_std, float eps, float lo, float hi) {
    ls = pdegym::clip_keep_nan(log_std, lo, hi);
    sigma = expf(ls);
    a = tanhf(__fadd_rn(mu, __fmul_rn(sigma, eps)));
    w = __fsub_rn(1.0f, __fmul_rn(a, a));
    u = __fadd_rn(w, kEpsilon);
  }
  __device__ __forceinline__ float log_prob_term(float eps) const {
    return __fsub_rn(__fsub_rn(__fsub_rn(__fmul_rn(-0.5f, __fmul_rn(eps, eps)), ls), kHalfLog2Pi), logf(u));
  }
};

template <int A>
__global__ __launch_bounds__(kRows) void sample_kernel(pdegym_squashed_gaussian_sample_args s, int N) {
  const int64_t i = (int64_t)blockIdx.x * kRows + threadIdx.x;
  if (i >= N) return;
  float mu[A], ls[A], eps[A];
#pragma unroll
  for (int j = 0; j < A; ++j) {
    mu[j] = s.raw[i * s.ld_raw + j];
    ls[j] = s.raw[i * s.ld_raw + A + j];
    eps[j] = s.eps[i * s.ld_eps + j];
  }
  float* row = s.actions + i * s.ld_actions;
  for (int c = 0; c < s.D; ++c) row[c] = s.obs[i * s.ld_obs + c];      // (D == 0 without obs)
  float logp = 0.f;
#pragma unroll
  for (int j = 0; j < A; ++j) {
    const Squashed q(mu[j], ls[j], eps[j], s.log_std_min, s.log_std_max);
    row[s.D + j] = q.a;
    const float t = q.log_prob_term(eps[j]);
    logp = j == 0 ? t : __fadd_rn(logp, t);
  }
  s.log_prob[i] = logp;
}

template <int A>
__global__ __launch_bounds__(kRows) void sample_backward_kernel(pdegym_squashed_gaussian_sample_backward_args s, int N) {
  const int64_t i = (int64_t)blockIdx.x * kRows + threadIdx.x;
  if (i >= N) return;
  float mu[A], ls[A], eps[A], da[A];
#pragma unroll
  for (int j = 0; j < A; ++j) {
    mu[j] = s.raw[i * s.ld_raw + j];
    ls[j] = s.raw[i * s.ld_raw + A + j];
    eps[j] = s.eps[i * s.ld_eps + j];
    da[j] = s.d_actions ? s.d_actions[i * s.ld_d_actions + j] : 0.f;
  }
  const float dlp = s.d_log_prob ? s.d_log_prob[i * s.d_log_prob_stride] : 0.f;
#pragma unroll
  for (int j = 0; j < A; ++j) {
    const Squashed q(mu[j], ls[j], eps[j], s.log_std_min, s.log_std_max);
    const float k = __fdiv_rn(__fmul_rn(__fmul_rn(2.0f, q.a), q.w), q.u);
    const float se = __fmul_rn(q.sigma, eps[j]);
    const float daw = __fmul_rn(da[j], q.w);
    s.d_raw[i * s.ld_d_raw + j] = __fadd_rn(daw, __fmul_rn(dlp, k));
    const bool pass = ls[j] >= s.log_std_min && ls[j] <= s.log_std_max;      // torch's clamp backward: the closed interval
    const float g = __fadd_rn(__fmul_rn(daw, se), __fmul_rn(dlp, __fsub_rn(__fmul_rn(k, se), 1.0f)));
    s.d_raw[i * s.ld_d_raw + A + j] = pass ? g : 0.f;                        // selected, never multiplied by 0
  }
}

// ---- critic loss ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kRows) void critic_rows_kernel(pdegym_sac_critic_loss_args a, int N, int G) {
  __shared__ double lds[kWaves * kCriticSums];
  const float alpha = expf(*a.log_alpha);
  const float gamma = (float)a.gamma, inv_n = (float)(1.0 / (double)N);
  const bool two = a.q2 != nullptr;      // kernel-uniform
  double s[kCriticSums] = {0.0, 0.0, 0.0, 0.0, 0.0};
  for (int64_t i = (int64_t)blockIdx.x * kRows + threadIdx.x; i < N; i += (int64_t)G * kRows) {
    const int64_t k = a.index ? a.index[i] : i;
    const float q1 = a.q1[i], q1t = a.q1_target[i], lp = a.next_log_prob[i];
    const float q2 = two ? a.q2[i] : 0.f, q2t = two ? a.q2_target[i] : 0.f;
    const float r = a.rewards[k], d = a.dones[k];
    const float m = two ? min_keep_nan(q1t, q2t) : q1t;
    const float v = __fsub_rn(m, __fmul_rn(alpha, lp));
    const float y = __fadd_rn(r, __fmul_rn(__fmul_rn(__fsub_rn(1.0f, d), gamma), v));
    const float e1 = __fsub_rn(q1, y);
    a.d_q1[i] = __fmul_rn(e1, inv_n);
    s[0] += (double)__fmul_rn(e1, e1);
    s[2] += (double)q1;
    s[4] += (double)y;
    if (two) {
      const float e2 = __fsub_rn(q2, y);
      a.d_q2[i] = __fmul_rn(e2, inv_n);
      s[1] += (double)__fmul_rn(e2, e2);
      s[3] += (double)q2;
    }
    if (a.target) a.target[i] = y;
  }
  block_sum(s, lds);
  store_partials(a.workspace, s);
}

__global__ __launch_bounds__(kRows) void critic_finish_kernel(pdegym_sac_critic_loss_args a, int N, int G) {
  __shared__ double lds[kWaves * kCriticSums];
  double s[kCriticSums];
  total_of_partials(a.workspace, G, s, lds);
  const double n = (double)N;
  if (threadIdx.x == 0 && a.stats) {
    a.stats[0] = (float)(0.5 * (s[0] + s[1]) / n);
    a.stats[1] = (float)(s[2] / n);
    a.stats[2] = (float)(s[3] / n);
    a.stats[3] = (float)(s[4] / n);
  }
}

// ---- actor loss ----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kRows) void actor_rows_kernel(pdegym_sac_actor_loss_args a, int N, int G) {
  __shared__ double lds[kWaves * kActorSums];
  const float alpha = expf(*a.log_alpha);
  const float te = (float)a.target_entropy, neg_inv_n = -(float)(1.0 / (double)N);
  const bool two = a.q2_pi != nullptr;      // kernel-uniform
  double s[kActorSums] = {0.0, 0.0, 0.0};
  for (int64_t i = (int64_t)blockIdx.x * kRows + threadIdx.x; i < N; i += (int64_t)G * kRows) {
    const float q1 = a.q1_pi[i], lp = a.log_prob[i];
    const float q2 = two ? a.q2_pi[i] : 0.f;
    // torch.min(cat, dim=1): the FIRST minimal column, a NaN counting as minimal
    const bool second = two && q1 == q1 && (q2 != q2 || q2 < q1);
    const float m = second ? q2 : q1;
    a.d_q1_pi[i] = second ? 0.f : neg_inv_n;
    if (two) a.d_q2_pi[i] = second ? neg_inv_n : 0.f;
    s[0] += (double)__fsub_rn(__fmul_rn(alpha, lp), m);
    s[1] += (double)__fadd_rn(lp, te);
    s[2] += (double)lp;
  }
  block_sum(s, lds);
  store_partials(a.workspace, s);
}

__global__ __launch_bounds__(kRows) void actor_finish_kernel(pdegym_sac_actor_loss_args a, int N, int G) {
  __shared__ double lds[kWaves * kActorSums];
  double s[kActorSums];
  total_of_partials(a.workspace, G, s, lds);
  const double n = (double)N;
  if (threadIdx.x == 0) {
    const float log_alpha = *a.log_alpha;
    const float alpha = expf(log_alpha);
    const double ent = s[1] / n;
    a.d_log_prob[0] = __fmul_rn(alpha, (float)(1.0 / n));
    a.d_log_alpha[0] = (float)(-ent);
    if (a.stats) {
      a.stats[0] = (float)(s[0] / n);
      a.stats[1] = (float)(-(double)log_alpha * ent);
      a.stats[2] = alpha;
      a.stats[3] = (float)(s[2] / n);
    }
  }
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
Range dense(const void* p, int64_t n, int64_t size) { return extent(p, 1, n, n, size); }

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

int check_workspace(const void* workspace, int64_t bytes, int32_t N) {
  if (!workspace) return pdegym::fail(-3, "null workspace");
  if (bytes < pdegym_sac_loss_workspace(N)) return pdegym::fail(-2, "workspace too small (pdegym_sac_loss_workspace)");
  if (!pdegym::is_aligned(workspace, 4)) return pdegym::fail(-2, "workspace must be 4-byte aligned");
  return 0;
}

int check_sample_common(int32_t N, int A, int64_t ld_raw, int64_t ld_eps, float lo, float hi) {
  if (N < 1) return pdegym::fail(-2, "N must be >= 1");
  if (A < 1 || A > kMaxA) return pdegym::fail(-2, "A must be 1 .. 8");
  if (ld_raw < 2 * A) return pdegym::fail(-2, "ld_raw must be >= 2 A");
  if (ld_eps < A) return pdegym::fail(-2, "ld_eps must be >= A");
  if (!(lo < hi)) return pdegym::fail(-2, "log_std_min must be < log_std_max");
  return 0;
}

unsigned row_blocks(int32_t N) { return (unsigned)(((int64_t)N + kRows - 1) / kRows); }

}  // namespace

extern "C" {

int64_t pdegym_sac_loss_workspace(int32_t N) {
  if (N < 1) return pdegym::fail(-2, "N must be >= 1");
  return (int64_t)groups_of(N) * kPartial * (int64_t)sizeof(double);
}

int pdegym_squashed_gaussian_sample(const pdegym_squashed_gaussian_sample_args* s, int32_t N, void* stream) {
  if (!s) return pdegym::fail(-1, "null descriptor");
  const int A = s->A;
  if (const int rc = check_sample_common(N, A, s->ld_raw, s->ld_eps, s->log_std_min, s->log_std_max)) return rc;
  if (s->D < 0 || (s->obs == nullptr) != (s->D == 0)) return pdegym::fail(-2, "D must be >= 1 with obs and 0 without");
  if (s->obs && s->ld_obs < s->D) return pdegym::fail(-2, "ld_obs must be >= D");
  if (s->ld_actions < (int64_t)s->D + A) return pdegym::fail(-2, "ld_actions must be >= D + A");
  if (!s->raw || !s->eps || !s->actions || !s->log_prob) return pdegym::fail(-3, "null raw/eps/actions/log_prob");
  const Range in[] = {extent(s->raw, N, s->ld_raw, 2 * A, 4), extent(s->eps, N, s->ld_eps, A, 4), extent(s->obs, N, s->ld_obs, s->D, 4)};
  const Range out[] = {extent(s->actions, N, s->ld_actions, s->D + A, 4), dense(s->log_prob, N, 4)};
  if (const int rc = check_overlaps(in, out)) return rc;
  with_width(A, [&](auto width) { launch(sample_kernel<decltype(width)::value>, row_blocks(N), stream, *s, (int)N); });
  return pdegym::check_launch("squashed_gaussian_sample");
}

int pdegym_squashed_gaussian_sample_backward(const pdegym_squashed_gaussian_sample_backward_args* s, int32_t N, void* stream) {
  if (!s) return pdegym::fail(-1, "null descriptor");
  const int A = s->A;
  if (const int rc = check_sample_common(N, A, s->ld_raw, s->ld_eps, s->log_std_min, s->log_std_max)) return rc;
  if (s->d_actions && s->ld_d_actions < A) return pdegym::fail(-2, "ld_d_actions must be >= A");
  if (s->d_log_prob && s->d_log_prob_stride != 0 && s->d_log_prob_stride != 1)
    return pdegym::fail(-2, "d_log_prob_stride must be 1 (an array) or 0 (one device scalar)");
  if (s->ld_d_raw < 2 * A) return pdegym::fail(-2, "ld_d_raw must be >= 2 A");
  if (!s->raw || !s->eps || !s->d_raw) return pdegym::fail(-3, "null raw/eps/d_raw");
  if (!s->d_actions && !s->d_log_prob) return pdegym::fail(-3, "d_actions and d_log_prob are both NULL");
  const Range in[] = {extent(s->raw, N, s->ld_raw, 2 * A, 4), extent(s->eps, N, s->ld_eps, A, 4),
                      extent(s->d_actions, N, s->ld_d_actions, A, 4), dense(s->d_log_prob, s->d_log_prob_stride ? N : 1, 4)};
  const Range out[] = {extent(s->d_raw, N, s->ld_d_raw, 2 * A, 4)};
  if (const int rc = check_overlaps(in, out)) return rc;
  with_width(A, [&](auto width) { launch(sample_backward_kernel<decltype(width)::value>, row_blocks(N), stream, *s, (int)N); });
  return pdegym::check_launch("squashed_gaussian_sample_backward");
}

int pdegym_sac_critic_loss(const pdegym_sac_critic_loss_args* g, int32_t N, void* stream) {
  if (!g) return pdegym::fail(-1, "null descriptor");
  if (N < 1) return pdegym::fail(-2, "N must be >= 1");
  if (g->index && g->M < 1) return pdegym::fail(-2, "M must be >= 1 when index is given");
  if (!std::isfinite(g->gamma)) return pdegym::fail(-2, "gamma must be finite");
  if (!g->q1 || !g->q1_target || !g->next_log_prob || !g->rewards || !g->dones || !g->log_alpha)
    return pdegym::fail(-3, "null q1/q1_target/next_log_prob/rewards/dones/log_alpha");
  if (!g->d_q1) return pdegym::fail(-3, "null d_q1");
  if ((g->q2 != nullptr) != (g->q2_target != nullptr) || (g->q2 != nullptr) != (g->d_q2 != nullptr))
    return pdegym::fail(-3, "q2, q2_target and d_q2 must be given together");
  if (const int rc = check_workspace(g->workspace, g->workspace_bytes, N)) return rc;
  const int64_t M = g->index ? g->M : N;
  const Range in[] = {dense(g->q1, N, 4),      dense(g->q2, N, 4),    dense(g->q1_target, N, 4), dense(g->q2_target, N, 4),
                      dense(g->next_log_prob, N, 4), dense(g->index, N, 8), dense(g->rewards, M, 4),   dense(g->dones, M, 4),
                      dense(g->log_alpha, 1, 4)};
  const Range out[] = {dense(g->d_q1, N, 4), dense(g->d_q2, N, 4), dense(g->target, N, 4), dense(g->stats, 4, 4),
                       dense(g->workspace, g->workspace_bytes, 1)};
  if (const int rc = check_overlaps(in, out)) return rc;
  const int G = groups_of(N);
  launch(critic_rows_kernel, (unsigned)G, stream, *g, (int)N, G);
  if (g->stats) launch(critic_finish_kernel, 1u, stream, *g, (int)N, G);
  return pdegym::check_launch("sac_critic_loss");
}

int pdegym_sac_actor_loss(const pdegym_sac_actor_loss_args* g, int32_t N, void* stream) {
  if (!g) return pdegym::fail(-1, "null descriptor");
  if (N < 1) return pdegym::fail(-2, "N must be >= 1");
  if (!std::isfinite(g->target_entropy)) return pdegym::fail(-2, "target_entropy must be finite");
  if (!g->q1_pi || !g->log_prob || !g->log_alpha) return pdegym::fail(-3, "null q1_pi/log_prob/log_alpha");
  if (!g->d_q1_pi || !g->d_log_prob || !g->d_log_alpha) return pdegym::fail(-3, "null d_q1_pi/d_log_prob/d_log_alpha");
  if ((g->q2_pi != nullptr) != (g->d_q2_pi != nullptr)) return pdegym::fail(-3, "q2_pi and d_q2_pi must be given together");
  if (const int rc = check_workspace(g->workspace, g->workspace_bytes, N)) return rc;
  const Range in[] = {dense(g->q1_pi, N, 4), dense(g->q2_pi, N, 4), dense(g->log_prob, N, 4), dense(g->log_alpha, 1, 4)};
  const Range out[] = {dense(g->d_q1_pi, N, 4),    dense(g->d_q2_pi, N, 4), dense(g->d_log_prob, 1, 4),
                       dense(g->d_log_alpha, 1, 4), dense(g->stats, 4, 4),   dense(g->workspace, g->workspace_bytes, 1)};
  if (const int rc = check_overlaps(in, out)) return rc;
  const int G = groups_of(N);
  launch(actor_rows_kernel, (unsigned)G, stream, *g, (int)N, G);
  launch(actor_finish_kernel, 1u, stream, *g, (int)N, G);
  return pdegym::check_launch("sac_actor_loss");
}

}  // extern "C"
