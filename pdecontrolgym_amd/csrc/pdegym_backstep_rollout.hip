// pdegym_backstep_rollout.hip -- T env-steps of the 1D transport / reaction-diffusion environments in ONE launch with the backstepping
// control law (include/pdegym.h: pdegym_backstep) evaluated inside it: pdegym_{transport,parabolic}_backstep_rollout.  What the
// two-launch path does per env-step -- backstep_control_kernel (pdegym_backstep.hip), then the step kernel -- happens between two
// iterations of one loop, with the row, beta, the norm ring, the running sums AND the instance's gain row held in registers for the whole
// rollout.  Every value is bit-identical to the two-launch path: the env-step is step1d_body of pdegym_1d_body.h as the carried policy
// kernel instantiates it (pdegym_1d_rollout.hip: rollout1d_policy_kernel), the dot product is pdegym_backstep_law.h, the function the
// control kernel calls, on the same operands.  What the kernel shares with the other 1D rollout kernels is pdegym_1d_rollout.h.
// Output contract (poisoned buffers, guard bands): tests/test_gpu_backstep_rollout.py, KERNEL_CASES there; tests/test_backstep_rollout.py
// fails when a kernel launched here is missing from that table.
#include "pdegym_1d_rollout.h"
#include "pdegym_backstep_law.h"

namespace {

constexpr int kMaxRow = 513;                     // the longest row: 8 slots per lane + node 0 of a parabolic row (transport: 512)
constexpr int kStrip = (kMaxRow + 3) / 4 * 4;    // floats of one wave's LDS strip

// One wave per instance, kWavesPerBlock waves per workgroup (rollout1d_kernel's shape).  Dirichlet actuation, full-state sensing,
// float32 operands, no history, temporal reward horizon, at most 8 slots per lane (n <= 512 transport / 513 parabolic): the corner
// rollout1d_policy_kernel carries in registers.
// FULL: the row fills the wave exactly (n - J0 == 64 EPL), as there.
// Gains: lane l holds terms l, 64 + l, ... of the instance's gain row (NK = EPL + J0 chunks cover len <= n), loaded once; a restart made
// inside the launch by the fused auto-reset switches the row before the next command (count: restarts so far, the snapshot of
// reset_count[inst] taken at the head of the launch plus the restarts seen since -- the value the control kernel would read there).
template <int EPL, bool PARABOLIC, bool ORDERED, bool FULL>
__global__ __launch_bounds__(kWave* kWavesPerBlock) void backstep_rollout1d_kernel(pdegym_params1d P, pdegym_bufs1d Bf, pdegym_rollout1d Ro,
                                                                                  pdegym_backstep L, int B) {
  __shared__ float strips[kWavesPerBlock][kStrip];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
  const int inst = blockIdx.x * kWavesPerBlock + wave;
  if (inst >= B) return;  // wave-uniform; the kernel has no workgroup barrier
  constexpr int J0 = PARABOLIC ? 1 : 0;
  constexpr int NK = EPL + J0;
  const int n = P.n;      // (the kernel argument even under FULL: stage_carried_row)
  const size_t slot = (size_t)B * n;
  float* const xw = strips[wave];

  double gain[NK];
  auto load_gains = [&](int count) {      // count: restarts of this instance so far (wave-uniform)
    const double* g = L.gain0 + (size_t)inst * L.gain_stride;
    // after c >= 1 restarts: pool row (inst + (c-1)*B) mod rows, the row the fused auto-reset took the running episode's beta from
    if (L.gain_pool && count > 0) g = L.gain_pool + (size_t)pool_row(L.pool_rows, nullptr, inst, B, count - 1) * L.m;
#pragma unroll
    for (int k = 0; k < NK; ++k) gain[k] = (k * kWave + lane < L.len) ? g[k * kWave + lane] : 0.0;
  };
  // the plant's counter is the controller's (checked by the entry point); without a pool the row never changes
  int count = (L.gain_pool && L.reset_count) ? __builtin_amdgcn_readfirstlane(L.reset_count[inst]) : 0;
  const bool follows = L.gain_pool && L.reset_count && Bf.reset_count && Bf.reset_init;      // kernel-uniform
  load_gains(count);

  Carry<EPL> C;       // the state stays in registers over the T env-steps (see rollout1d_kernel)
  carry_load<EPL, PARABOLIC, FULL>(C, P, Bf, Ro.obs, inst, lane);      // ends with drain_vmem(): the gains have landed too
  for (int t = 0; t < Ro.T; ++t) {
    stage_carried_row<EPL, PARABOLIC>(C, xw, n, lane);
    sense_noise(Ro.obs_noise, Ro.obs_seen, xw, n, B, inst, lane, t);
    const double s = pdegym_backstep_law::dot<ORDERED, NK>(L.len, lane, [&](int k, int i) { return gain[k] * (double)xw[i]; });
    float a = (float)(s * L.scale);      // rounded once, as the control kernel's out32
    if (L.noise) a += L.noise[(size_t)t * B + inst];
    if (L.clamp) a = pdegym::clip_keep_nan(a, L.lo, L.hi);
    if (lane == 0) Ro.actions[(size_t)t * B + inst] = a;

    const pdegym_bufs1d S = rollout_step_view(Bf, Ro, B, slot, t);
    step1d_body<EPL, PARABOLIC, false, false, false, false, true, true, FULL>(P, S, B, inst, lane, &a, &C, t == Ro.T - 1);
    // The auto-reset branch of step1d_body is the only place that leaves the carried time index at 0 (a step from index 0 advances it:
    // substeps >= 1, nt >= 2, checked by the entry point): the instance restarted, and its next command takes the next gain row.
    if (follows && __builtin_amdgcn_readfirstlane(C.t) == 0) {      // wave-uniform, rare
      ++count;
      load_gains(count);
      drain_vmem();
    }
  }
  carry_store_ring<EPL>(C, Bf, inst, lane);
}

template <bool PARABOLIC>
int launch_backstep_rollout(const pdegym_params1d* prm, const pdegym_bufs1d* buf, const pdegym_rollout1d* ro, const pdegym_backstep* law,
                            int B, void* stream) {
  if (!prm || !buf || !ro || !law) return pdegym::fail(-1, "null params/bufs/rollout/law");
  if (B <= 0 || ro->T <= 0) return 0;
  const pdegym_params1d& P = *prm;
  const pdegym_backstep& L = *law;
  // the plant: the checks of every 1D rollout, then what narrows them to the corner this kernel covers
  if (const int rc = check_rollout_plant(P, *buf, *ro, "backstep rollout")) return rc;
  // at most 8 slots per lane (the widest instantiation): 512 nodes of a transport row, 513 of a parabolic one (node 0 is not a slot)
  if (P.n - (PARABOLIC ? 1 : 0) > 8 * kWave)
    return pdegym::fail(-2, PARABOLIC ? "backstep rollout: rows of up to 513 nodes (longer rows: pdegym_backstep_control + pdegym_parabolic_step)"
                                      : "backstep rollout: rows of up to 512 nodes (longer rows: pdegym_backstep_control + pdegym_transport_step)");
  if (P.substeps < 1) return pdegym::fail(-2, "backstep rollout: substeps must be >= 1");
  if (P.sensing != PDEGYM_SENSE_FULL) return pdegym::fail(-2, "backstep rollout: the law reads the whole row (full-state sensing only)");
  if (P.control_type != PDEGYM_CONTROL_DIRICHLET) return pdegym::fail(-2, "backstep rollout: Dirichlet actuation only (Neumann: pdegym_backstep_control + pdegym_*_step)");
  if (P.flux != PDEGYM_FLUX_LINEAR) return pdegym::fail(-2, "backstep rollout: the law exists for the linear transport term only");
  if (ro->policy) return pdegym::fail(-2, "backstep rollout: the law replaces the policy (rollout.policy must be NULL)");
  // the law: the checks of pdegym_backstep_control
  if (!L.gain0) return pdegym::fail(-3, "null gain0");
  if (L.obs || L.out64 || L.out32) return pdegym::fail(-2, "backstep rollout: law.obs / out64 / out32 must be NULL (the rollout's obs and actions are used)");
  if (L.m < 1 || L.len < 1 || L.len > L.m || L.len > P.n) return pdegym::fail(-2, "need 1 <= len <= min(m, n)");
  if (L.gain_stride != 0 && L.gain_stride < L.m) return pdegym::fail(-2, "gain_stride must be 0 (one shared row) or >= m");
  if (L.order != PDEGYM_BACKSTEP_TREE && L.order != PDEGYM_BACKSTEP_ORDERED) return pdegym::fail(-2, "bad order");
  if (L.gain_pool && !L.reset_count) return pdegym::fail(-3, "gain_pool needs reset_count (which episode an instance is in)");
  if (L.reset_count && buf->reset_count && L.reset_count != buf->reset_count)
    return pdegym::fail(-2, "law.reset_count and bufs.reset_count must be the same counter (controller and plant count the same restarts)");
  if (L.pool_rows < 0) return pdegym::fail(-2, "pool_rows must be >= 0 (0 = B)");
  if (L.clamp && !(L.lo <= L.hi)) return pdegym::fail(-2, "clamp bounds must satisfy lo <= hi");

  hipStream_t st = (hipStream_t)stream;
  const int nslots = P.n - (PARABOLIC ? 1 : 0);
  const int epl = (nslots + kWave - 1) / kWave;      // the slots-per-lane choice of launch_step / launch_rollout: rewards depend on it
  const bool ordered = L.order == PDEGYM_BACKSTEP_ORDERED;
  const dim3 grid((B + kWavesPerBlock - 1) / kWavesPerBlock), block(kWave * kWavesPerBlock);
  with_epl<8>(epl, [&](auto tag) {      // (more than 8 was refused above)
    constexpr int E = decltype(tag)::value;
    constexpr bool kHasFull = epl_has_full(E);
    if (kHasFull && nslots == kWave * E) {
      if (ordered) backstep_rollout1d_kernel<E, PARABOLIC, true, kHasFull><<<grid, block, 0, st>>>(P, *buf, *ro, L, B);
      else backstep_rollout1d_kernel<E, PARABOLIC, false, kHasFull><<<grid, block, 0, st>>>(P, *buf, *ro, L, B);
    } else {
      if (ordered) backstep_rollout1d_kernel<E, PARABOLIC, true, false><<<grid, block, 0, st>>>(P, *buf, *ro, L, B);
      else backstep_rollout1d_kernel<E, PARABOLIC, false, false><<<grid, block, 0, st>>>(P, *buf, *ro, L, B);
    }
  });
  return pdegym::check_launch("backstep_rollout1d");
}

}  // namespace

extern "C" {

int pdegym_transport_backstep_rollout(const pdegym_params1d* prm, const pdegym_bufs1d* buf, const pdegym_rollout1d* ro,
                                      const pdegym_backstep* law, int32_t B, void* stream) {
  return launch_backstep_rollout<false>(prm, buf, ro, law, B, stream);
}

int pdegym_parabolic_backstep_rollout(const pdegym_params1d* prm, const pdegym_bufs1d* buf, const pdegym_rollout1d* ro,
                                      const pdegym_backstep* law, int32_t B, void* stream) {
  return launch_backstep_rollout<true>(prm, buf, ro, law, B, stream);
}

}  // extern "C"
