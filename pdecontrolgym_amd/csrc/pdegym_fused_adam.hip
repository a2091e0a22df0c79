// pdegym_fused_adam.hip -- the optimiser step of the training examples (see include/pdegym.h):
//   pdegym_fused_adam      global-norm clip, Adam, the blocked weight mirrors FusedMLP's kernels read and the Polyak average of the
//                          target networks for up to 32 float32 tensors                                             -- two launches
// head + update, stream order the only synchronisation (no workgroup waits for another, no atomics).  The table of tensors travels by
// value in the kernel arguments.  Tensor k takes c_k = min(ceil(n_k / kChunk), kMaxGroups) workgroups in table order, so the grid and
// the order of every sum are a function of the list of sizes alone:
//   a thread adds the squares of its elements e = kChunk * (j + c_k * r) + kThreads * q + t in the order r, then q (float64);
//   a workgroup adds its threads with pdegym::wave::wave_sum per wave and the four waves in ascending order (float64);
//   every workgroup of the update launch adds the G partials the same way: thread t takes the partials t, t + kThreads, .. in
//   ascending order, then the workgroup sum.
// Every float32 operation is __fmul_rn / __fadd_rn / __fsub_rn / __fdiv_rn in the order stated in the header (one rounding each, no
// contraction whatever the flags) and sqrtf for the root of v -- the correctly rounded one: this toolchain's __fsqrt_rn is the
// native v_sqrt_f32 (1 ulp), which misses torch's and NumPy's bits about once in a few thousand elements; the float64 scalars (sqrt of the sum, lr / (1 - beta1^t), sqrt(1 - beta2^t))
// are IEEE operations formed once per thread at the top of the launch.  The launches are made with hipLaunchKernel (DESIGN.md
// section 4.15).  Output contract, displaced pointers, non-finite data, captured graphs: tests/test_gpu_fused_adam.py.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "pdegym.h"
#include "pdegym_common.h"

namespace {

using pdegym::wave::kWave;

constexpr int kThreads = 256;                 // threads per workgroup
constexpr int kPerThread = 4;                 // elements of a chunk per thread
constexpr int kChunk = kThreads * kPerThread; // elements per workgroup and pass
constexpr int kMaxGroups = 256;               // workgroups per tensor at most: beyond kChunk * kMaxGroups elements they take further passes
constexpr int kWaves = kThreads / kWave;
constexpr int kMaxK = PDEGYM_FUSED_ADAM_MAX_TENSORS;

int groups_of(int64_t n) {
  const int64_t c = (n + kChunk - 1) / kChunk;
  return (int)(c < kMaxGroups ? c : kMaxGroups);
}

// what the kernels are given: the caller's descriptor and the first workgroup of every tensor (first[K] = G)
struct KernelArgs {
  pdegym_fused_adam_args a;
  int32_t first[kMaxK + 1];
  int32_t norm;      // != 0: the head writes partial sums and the update reads them
  int32_t clip;      // != 0: g is scaled
};

// a double in the workspace, which is only 4-byte aligned: two dword accesses at worst, never an 8-byte-aligned one
struct __attribute__((packed, aligned(4))) f64u {
  double v;
};

// Sum over the threads of a workgroup, the result in every thread: wave_sum per wave, then the waves in ascending order.
__device__ __forceinline__ double block_sum(double v, double* lds) {
  const double s = pdegym::wave::wave_sum(v);
  if ((threadIdx.x & (kWave - 1)) == 0) lds[threadIdx.x / kWave] = s;
  __syncthreads();
  double r = lds[0];
#pragma unroll
  for (int w = 1; w < kWaves; ++w) r += lds[w];
  __syncthreads();
  return r;
}

// the tensor of this workgroup (uniform: a scalar search over at most 32 entries) and the workgroup's index in it
__device__ __forceinline__ int tensor_of(const KernelArgs& k, int* j, int* c) {
  const int b = (int)blockIdx.x;
  int i = 0;
  while (i + 1 < k.a.K && k.first[i + 1] <= b) ++i;
  *j = b - k.first[i];
  *c = k.first[i + 1] - k.first[i];
  return i;
}

__global__ __launch_bounds__(kThreads) void head_kernel(KernelArgs k) {
  __shared__ double lds[kWaves];
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    double* st = k.a.state;
    st[0] = st[0] + 1.0;
    st[1] = st[1] * k.a.beta1;
    st[2] = st[2] * k.a.beta2;
  }
  if (!k.norm) return;      // kernel-uniform
  int j, c;
  const pdegym_fused_adam_tensor& T = k.a.tensor[tensor_of(k, &j, &c)];
  const float* __restrict__ g = T.g;
  const int64_t n = T.n;
  double s = 0.0;
  for (int64_t base = (int64_t)j * kChunk; base < n; base += (int64_t)c * kChunk) {
#pragma unroll
    for (int q = 0; q < kPerThread; ++q) {
      const int64_t e = base + q * kThreads + threadIdx.x;
      if (e < n) {
        const float x = g[e];
        s += (double)__fmul_rn(x, x);
      }
    }
  }
  s = block_sum(s, lds);
  if (threadIdx.x == 0) ((f64u*)k.a.workspace)[blockIdx.x].v = s;
}

// element (o, i) of an (out, in) tensor in rows row0 .. of a blocked array [ceil(in / 4), out_total, 4]
__device__ __forceinline__ int64_t blocked_index(int64_t e, int in, int out_total, int row0) {
  const int64_t o = e / in;
  const int i = (int)(e - o * in);
  return ((int64_t)(i >> 2) * out_total + row0 + o) * 4 + (i & 3);
}

__global__ __launch_bounds__(kThreads) void update_kernel(KernelArgs k) {
  __shared__ double lds[kWaves];
  const int G = k.first[k.a.K];
  float coef = 1.0f;
  if (k.norm) {      // kernel-uniform
    double s = 0.0;
    const f64u* part = (const f64u*)k.a.workspace;
    for (int i = (int)threadIdx.x; i < G; i += kThreads) s += part[i].v;
    s = block_sum(s, lds);
    const float total = (float)sqrt(s);
    if (k.a.total_norm && blockIdx.x == 0 && threadIdx.x == 0) *k.a.total_norm = total;
    const float c = __fdiv_rn((float)k.a.max_grad_norm, __fadd_rn(total, 1e-6f));
    coef = c != c ? c : fminf(c, 1.0f);
  }
  const bool clip = k.clip != 0;
  const double* st = k.a.state;
  const double lr = k.a.lr_device ? (double)*k.a.lr_device : k.a.lr;
  const float step_size = (float)(lr / (1.0 - st[1]));
  const float bc2_sqrt = (float)sqrt(1.0 - st[2]);
  const float c1 = (float)(1.0 - k.a.beta1), b2 = (float)k.a.beta2, c2 = (float)(1.0 - k.a.beta2), eps = (float)k.a.eps;
  const float tau = (float)k.a.tau, one_minus_tau = (float)(1.0 - k.a.tau);

  int j, c;
  const pdegym_fused_adam_tensor& T = k.a.tensor[tensor_of(k, &j, &c)];
  const float* __restrict__ g = T.g;
  float* p = T.p;
  float* m = T.m;
  float* v = T.v;
  float* copy = T.copy;
  float* wt = T.wt;
  float* pt = k.a.polyak ? T.pt : nullptr;
  float* pt_copy = T.pt_copy;
  float* pt_wt = T.pt_wt;
  const int in = T.in;
  const int64_t n = T.n;
  for (int64_t base = (int64_t)j * kChunk; base < n; base += (int64_t)c * kChunk) {
#pragma unroll
    for (int q = 0; q < kPerThread; ++q) {
      const int64_t e = base + q * kThreads + threadIdx.x;
      if (e >= n) continue;
      const float gr = g[e];
      const float gs = clip ? __fmul_rn(gr, coef) : gr;
      const float m0 = m[e], v0 = v[e], p0 = p[e];
      const float m1 = __fadd_rn(m0, __fmul_rn(c1, __fsub_rn(gs, m0)));
      const float v1 = __fadd_rn(__fmul_rn(b2, v0), __fmul_rn(c2, __fmul_rn(gs, gs)));
      const float denom = __fadd_rn(__fdiv_rn(sqrtf(v1), bc2_sqrt), eps);
      const float p1 = __fsub_rn(p0, __fmul_rn(step_size, __fdiv_rn(m1, denom)));
      m[e] = m1;
      v[e] = v1;
      p[e] = p1;
      if (copy) copy[e] = p1;
      if (wt) wt[blocked_index(e, in, T.wt_out_total, T.wt_row0)] = p1;
      if (pt) {
        const float t1 = __fadd_rn(__fmul_rn(one_minus_tau, pt[e]), __fmul_rn(tau, p1));
        pt[e] = t1;
        if (pt_copy) pt_copy[e] = t1;
        if (pt_wt) pt_wt[blocked_index(e, in, T.pt_wt_out_total, T.pt_wt_row0)] = t1;
      }
    }
  }
}

void launch(void (*kernel)(KernelArgs), unsigned grid, void* stream, KernelArgs& k) {
  void* args[] = {(void*)&k};
  (void)hipLaunchKernel((const void*)kernel, dim3(grid), dim3(kThreads), args, 0, (hipStream_t)stream);      // (check_launch reads the error)
}

// ---- host checks ---------------------------------------------------------------------------------------------------------------------
struct Range {
  const char* lo;
  const char* hi;          // one past the last byte
  bool output;
  const void* blocked;     // base of a blocked array (NULL: a dense range): two blocked ranges of one array with one out_total may
  int out_total, row0, out; // interleave on disjoint rows
};

bool clash(const Range& a, const Range& b) {
  if (!(a.output || b.output) || !(a.lo < b.hi && b.lo < a.hi)) return false;
  if (a.blocked && a.blocked == b.blocked && a.out_total == b.out_total)
    return a.row0 < b.row0 + b.out && b.row0 < a.row0 + a.out;
  return true;
}

struct Ranges {
  Range r[kMaxK * 9 + 4];
  int count = 0;
  void dense(const void* p, int64_t bytes, bool output) {
    if (p) r[count++] = {(const char*)p, (const char*)p + bytes, output, nullptr, 0, 0, 0};
  }
  void blocked(const float* wt, int out, int in, int out_total, int row0) {
    if (!wt) return;
    const int64_t k4 = (in + 3) / 4;
    const char* base = (const char*)wt;
    r[count++] = {base + (int64_t)row0 * 16, base + (((k4 - 1) * out_total + row0 + out) * 4) * 4, true, wt, out_total, row0, out};
  }
};

int check_mirror(const float* wt, const pdegym_fused_adam_tensor& t, int out_total, int row0) {
  if (!wt) return 0;
  if (t.out < 1 || t.in < 1 || (int64_t)t.out * t.in != t.n) return pdegym::fail(-2, "a blocked mirror needs out * in == n");
  if (row0 < 0 || out_total < 1 || (int64_t)row0 + t.out > out_total) return pdegym::fail(-2, "a blocked mirror needs row0 + out <= out_total");
  if (!pdegym::is_aligned(wt, 4)) return pdegym::fail(-2, "a blocked mirror must be 4-byte aligned");
  return 0;
}

int64_t workspace_of(const int64_t* n, int K, int32_t* first) {
  if (K < 1 || K > kMaxK) return pdegym::fail(-2, "K must be 1 .. 32");
  int64_t G = 0;
  for (int i = 0; i < K; ++i) {
    if (n[i] < 1) return pdegym::fail(-2, "n must be >= 1");
    if (first) first[i] = (int32_t)G;
    G += groups_of(n[i]);
  }
  if (first) first[K] = (int32_t)G;
  return G * (int64_t)sizeof(double);
}

}  // namespace

extern "C" {

int64_t pdegym_fused_adam_workspace(const int64_t* n, int32_t K) {
  if (!n) return pdegym::fail(-3, "null n");
  return workspace_of(n, K, nullptr);
}

int pdegym_fused_adam(const pdegym_fused_adam_args* a, void* stream) {
  if (!a) return pdegym::fail(-1, "null descriptor");
  const int K = a->K;
  if (K < 1 || K > kMaxK) return pdegym::fail(-2, "K must be 1 .. 32");
  if (!a->lr_device && !std::isfinite(a->lr)) return pdegym::fail(-2, "lr must be finite");
  if (!std::isfinite(a->beta1) || !std::isfinite(a->beta2) || !(a->beta1 >= 0.0 && a->beta1 < 1.0) || !(a->beta2 >= 0.0 && a->beta2 < 1.0))
    return pdegym::fail(-2, "beta1 and beta2 must be in [0, 1)");
  if (!std::isfinite(a->eps) || !(a->eps > 0.0)) return pdegym::fail(-2, "eps must be finite and > 0");
  if (std::isinf(a->max_grad_norm)) return pdegym::fail(-2, "max_grad_norm must not be infinite (<= 0 or NaN: no clipping)");
  if (!a->state) return pdegym::fail(-3, "null state");
  if (!pdegym::is_aligned(a->state, 8)) return pdegym::fail(-2, "state must be 8-byte aligned");
  if (a->lr_device && !pdegym::is_aligned(a->lr_device, 4)) return pdegym::fail(-2, "lr_device must be 4-byte aligned");
  if (a->total_norm && !pdegym::is_aligned(a->total_norm, 4)) return pdegym::fail(-2, "total_norm must be 4-byte aligned");

  KernelArgs k;
  int64_t sizes[kMaxK];
  bool targets = false;
  for (int i = 0; i < K; ++i) {
    const pdegym_fused_adam_tensor& t = a->tensor[i];
    if (!t.p || !t.g || !t.m || !t.v) return pdegym::fail(-3, "null p/g/m/v");
    if (t.n < 1) return pdegym::fail(-2, "n must be >= 1");
    for (const void* q : {(const void*)t.p, (const void*)t.g, (const void*)t.m, (const void*)t.v, (const void*)t.copy, (const void*)t.pt,
                          (const void*)t.pt_copy})
      if (!pdegym::is_aligned(q, 4)) return pdegym::fail(-2, "p/g/m/v/copy/pt/pt_copy must be 4-byte aligned");
    if (!t.pt && (t.pt_copy || t.pt_wt)) return pdegym::fail(-3, "a target mirror without a target");
    if (const int rc = check_mirror(t.wt, t, t.wt_out_total, t.wt_row0)) return rc;
    if (const int rc = check_mirror(t.pt_wt, t, t.pt_wt_out_total, t.pt_wt_row0)) return rc;
    targets = targets || t.pt;
    sizes[i] = t.n;
  }
  if (targets && !(std::isfinite(a->tau) && a->tau >= 0.0 && a->tau <= 1.0)) return pdegym::fail(-2, "tau must be in [0, 1] when a target is given");
  const int64_t need = workspace_of(sizes, K, k.first);
  if (!a->workspace) return pdegym::fail(-3, "null workspace");
  if (a->workspace_bytes < need) return pdegym::fail(-2, "workspace too small (pdegym_fused_adam_workspace)");
  if (!pdegym::is_aligned(a->workspace, 4)) return pdegym::fail(-2, "workspace must be 4-byte aligned");

  Ranges R;
  R.dense(a->state, 3 * sizeof(double), true);
  R.dense(a->total_norm, 4, true);
  R.dense(a->workspace, need, true);
  R.dense(a->lr_device, 4, false);
  for (int i = 0; i < K; ++i) {
    const pdegym_fused_adam_tensor& t = a->tensor[i];
    const int64_t bytes = t.n * 4;
    R.dense(t.p, bytes, true);
    R.dense(t.g, bytes, false);
    R.dense(t.m, bytes, true);
    R.dense(t.v, bytes, true);
    R.dense(t.copy, bytes, true);
    R.dense(t.pt, bytes, true);
    R.dense(t.pt_copy, bytes, true);
    R.blocked(t.wt, t.out, t.in, t.wt_out_total, t.wt_row0);
    R.blocked(t.pt_wt, t.out, t.in, t.pt_wt_out_total, t.pt_wt_row0);
  }
  for (int i = 0; i < R.count; ++i)
    for (int j = i + 1; j < R.count; ++j)
      if (clash(R.r[i], R.r[j])) return pdegym::fail(-3, "an output overlaps another tensor of the call");

  k.a = *a;
  k.clip = a->max_grad_norm > 0.0 ? 1 : 0;      // (false for a NaN)
  k.norm = (k.clip || a->total_norm) ? 1 : 0;
  const unsigned G = (unsigned)k.first[K];
  launch(head_kernel, k.norm ? G : 1u, stream, k);
  launch(update_kernel, G, stream, k);
  return pdegym::check_launch("fused_adam");
}

}  // extern "C"
