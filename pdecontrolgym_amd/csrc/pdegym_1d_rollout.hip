// pdegym_1d_rollout.hip -- T env-steps of the 1D transport / reaction-diffusion environments in ONE launch (pdegym_*_rollout),
// optionally with the MLP policy that commands them evaluated inside the launch (pdegym_policy.h).  The env-step itself is
// step1d_body of pdegym_1d_body.h: every value equals what T step calls produce, bit for bit.  Shared with pdegym_backstep_rollout.hip: pdegym_1d_rollout.h.
#include "pdegym_1d_rollout.h"
#include "pdegym_policy.h"

namespace {

// T env-steps of one instance by one wave in ONE launch (pdegym_*_rollout): iteration t is the step kernel's body with the
// row written to observation slot t + 1, action / reward / flags taken from / written to row t of the [T, B] rollout arrays
// -- every value equals what T separate step calls produce, bit for bit.  What it removes is the kernel boundary between
// env-steps: no dispatch gap, no load phase (the state stays in registers, Carry), and the waves of a SIMD drift apart
// instead of finishing in two generations (docs/HISTORY.md section 3.2).
// FULL: the row fills the wave exactly (n - J0 == 64 EPL): the slot masks fold away (pdegym_1d_body.h: run_substeps).
// PER_STEP (PDEGYM_ROLLOUT_FINAL_OBS_PER_STEP): final_obs is [T, B, n] and advances with the view.  Compiled apart: the form without
// it is the kernel it was, and a stride, a flag or a second advancing pointer in this loop costs the transport FULL form (99 SGPRs) a
// wave of occupancy.
template <int EPL, bool PARABOLIC, bool BURGERS, bool FULL, bool PER_STEP = false>
__global__ __launch_bounds__(kWave* kWavesPerBlock) void rollout1d_kernel(pdegym_params1d P, pdegym_bufs1d Bf, pdegym_rollout1d Ro,
                                                                         int B) {
  const int lane = threadIdx.x & (kWave - 1);
  const int inst = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
  if (inst >= B) return;  // wave-uniform
  const int n = FULL ? kWave * EPL + (PARABOLIC ? 1 : 0) : P.n;
  const size_t slot = (size_t)B * n;
  // The state -- row, beta, time index, sums AND the norm ring -- stays in registers over the T env-steps (Carry).  Round 5: the
  // steady state of the loop has NO load at all: the commands of 64 env-steps arrive in one load per lane (lane l holds step
  // t0 + l; handed out by v_readlane), the ring is two registers per lane, and the per-instance
  // state words that every step would overwrite are stored by the last step only.  gfx9 counts loads and stores in one counter
  // (vmcnt), so the single ring / command load per env-step of the round-4 loop made every step wait for the stores of the step
  // before (SQ_WAIT_ANY 57 % of the wave cycles at S = 1); now only the batch hand-over, once per 64 env-steps, waits.
  Carry<EPL> C;
  carry_load<EPL, PARABOLIC, FULL>(C, P, Bf, Ro.obs, inst, lane);
  // the per-step views of the rollout arrays advance by one slot / row per env-step (no 64-bit multiplications in the loop)
  pdegym_bufs1d S = rollout_step_view(Bf, Ro, B, slot, 0);
  S.final_obs = Bf.final_obs;      // (slot 0 of it, or the [B, n] array: the mode is PER_STEP here, not the descriptor's bit)
  auto command_batch = [&](int t0) { return (t0 + lane < Ro.T) ? Ro.actions[(size_t)(t0 + lane) * B + inst] : 0.f; };
  float a_cur = command_batch(0);
  drain_vmem();
  for (int t = 0; t < Ro.T; ++t) {
    const int j = t & (kWave - 1);
    if (j == 0 && t) {      // wave-uniform; once per 64 env-steps, the loop's only wait for memory
      a_cur = command_batch(t);
      drain_vmem();
    }
    const float a = lane_value(a_cur, j);
    step1d_body<EPL, PARABOLIC, false, false, BURGERS, false, true, true, FULL>(P, S, B, inst, lane, &a, &C, t == Ro.T - 1);
    S.state_in = S.obs;
    S.obs += slot;
    S.action = static_cast<const float*>(S.action) + B;
    S.reward += B;
    S.terminated += B;
    S.truncated += B;
    if constexpr (PER_STEP) S.final_obs += slot;
  }
  carry_store_ring<EPL>(C, Bf, inst, lane);
}


// The general form (round 4): Neumann actuation and / or scalar sensing -- what the reference's control / sensing table offers
// beyond the Dirichlet / full-state corner (hyperbolic.py:66-124, parabolic.py:66-122).  Iteration t is the step kernel's body
// exactly as step1d_kernel instantiates it (select form for Neumann, the fast form otherwise), with the state going through
// memory between iterations: full-state sensing keeps it in the observation slots (slot t in, slot t + 1 out), scalar sensing in
// bufs.u (in place) while the observation slots receive the sensed value.  A wave re-reads what its own lanes stored (rows, time
// index, sums, ring), so iterations are separated by a workgroup-scope release / acquire pair, nothing more.
template <int EPL, bool PARABOLIC, bool NEUMANN, bool BURGERS>
__device__ __forceinline__ void rollout1d_general_step(const pdegym_params1d& P, const pdegym_bufs1d& Bf, const pdegym_rollout1d& Ro, int B,
                                                        int inst, int lane, int t, const float* command) {
  const bool full = P.sensing == PDEGYM_SENSE_FULL;
  const pdegym_bufs1d S = rollout_step_view(Bf, Ro, B, (size_t)B * (full ? P.n : 1), t, full);
  step1d_body<EPL, PARABOLIC, NEUMANN, false, BURGERS>(P, S, B, inst, lane, command);
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

template <int EPL, bool PARABOLIC, bool NEUMANN, bool BURGERS>
__global__ __launch_bounds__(kWave* kWavesPerBlock) void rollout1d_general_kernel(pdegym_params1d P, pdegym_bufs1d Bf, pdegym_rollout1d Ro,
                                                                                 int B) {
  const int lane = threadIdx.x & (kWave - 1);
  const int inst = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
  if (inst >= B) return;  // wave-uniform
  for (int t = 0; t < Ro.T; ++t) rollout1d_general_step<EPL, PARABOLIC, NEUMANN, BURGERS>(P, Bf, Ro, B, inst, lane, t, nullptr);
}


// ================================================================================================
// ---- the policy inside the rollout kernel (pdegym_policy.h: prologue, evaluate, command, shaped) ----------------------------------
// A wave without an instance of a WIDE workgroup stays in the loop of T iterations and `continue`s behind the evaluation (not
// pdegym_policy::attend, the traffic and tumor kernels' way: here the loop's form is the quicker one, profiles/policy_host_resources.txt).
// The network's output on its way to the command of step t (either head), stored to actions[t, b].
template <bool WIDE, bool GAUSS>
__device__ __forceinline__ float policy_command(float o, const pdegym_mlp& N, const pdegym_policy::Wide& Wd, const pdegym_rollout1d& Ro, int B,
                                                int inst, int wave, int lane, int t) {
  namespace pol = pdegym_policy;
  float a;
  if constexpr (GAUSS)      // the squashed-Gaussian head: neuron 0 is mu, neuron 1 log_std
    a = pol::shaped_gaussian(pol::command<WIDE>(o, Wd, wave, 0), pol::command<WIDE>(o, Wd, wave, 1), N, t, B, inst, 0);
  else
    a = pol::shaped(pol::command<WIDE>(o, Wd, wave, 0), N, t, B, inst, 0);
  if (lane == 0) Ro.actions[(size_t)t * B + inst] = a;
  return a;
}

template <int EPL, bool PARABOLIC, bool BURGERS, bool WIDE, bool FULL, bool GAUSS>
__global__ __launch_bounds__(kWave* pdegym_policy::kWaves) void rollout1d_policy_kernel(pdegym_params1d P, pdegym_bufs1d Bf,
                                                                                        pdegym_rollout1d Ro, pdegym_mlp N, int B) {
  namespace pol = pdegym_policy;
  extern __shared__ __attribute__((aligned(16))) float pol_smem[];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
  const int inst = blockIdx.x * pol::kWaves + wave;
  const bool active = inst < B;           // wave-uniform
  const int n = P.n;                      // (the kernel argument even under FULL: stage_carried_row)
  pol::PolicyWave W;
  pol::Wide Wd;
  if (!pol::prologue<WIDE>(W, Wd, N, pol_smem, n, active, wave, lane)) return;
  const size_t slot = (size_t)B * n;
  Carry<EPL> C;       // the state stays in registers over the T env-steps (see rollout1d_kernel)
  if (active) carry_load<EPL, PARABOLIC, FULL>(C, P, Bf, Ro.obs, inst, lane);
  for (int t = 0; t < Ro.T; ++t) {
    if (active) {
      stage_carried_row<EPL, PARABOLIC>(C, W.xw, n, lane);
      sense_noise(Ro.obs_noise, Ro.obs_seen, W.xw, n, B, inst, lane, t);
    }
    const float o = pol::evaluate<WIDE, GAUSS>(W, Wd, N, pol_smem, n, wave, lane);
    if (!active) continue;
    float a = policy_command<WIDE, GAUSS>(o, N, Wd, Ro, B, inst, wave, lane, t);
    const pdegym_bufs1d S = rollout_step_view(Bf, Ro, B, slot, t);
    step1d_body<EPL, PARABOLIC, false, false, BURGERS, false, true, true, FULL>(P, S, B, inst, lane, &a, &C, t == Ro.T - 1);
  }
  if (active) carry_store_ring<EPL>(C, Bf, inst, lane);
}

// The policy in front of the general step (Neumann actuation / scalar sensing): its input is observation slot t as stored -- od = n
// values, or the one sensed value -- read back from memory after the previous iteration's fence.
template <int EPL, bool PARABOLIC, bool NEUMANN, bool BURGERS, bool WIDE, bool GAUSS>
__global__ __launch_bounds__(kWave* pdegym_policy::kWaves) void rollout1d_policy_general_kernel(pdegym_params1d P, pdegym_bufs1d Bf,
                                                                                                pdegym_rollout1d Ro, pdegym_mlp N, int B) {
  namespace pol = pdegym_policy;
  extern __shared__ __attribute__((aligned(16))) float pol_smem[];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
  const int inst = blockIdx.x * pol::kWaves + wave;
  const bool active = inst < B;           // wave-uniform
  const int od = P.sensing == PDEGYM_SENSE_FULL ? P.n : 1;
  pol::PolicyWave W;
  pol::Wide Wd;
  if (!pol::prologue<WIDE>(W, Wd, N, pol_smem, od, active, wave, lane)) return;
  for (int t = 0; t < Ro.T; ++t) {
    if (active) {
      const float* orow = Ro.obs + ((size_t)t * B + inst) * od;
      for (int j = lane; j < od; j += kWave) W.xw[j] = orow[j];
      wave_lds_sync();
      sense_noise(Ro.obs_noise, Ro.obs_seen, W.xw, od, B, inst, lane, t);
    }
    const float o = pol::evaluate<WIDE, GAUSS>(W, Wd, N, pol_smem, od, wave, lane);
    if (!active) continue;
    float a = policy_command<WIDE, GAUSS>(o, N, Wd, Ro, B, inst, wave, lane, t);
    rollout1d_general_step<EPL, PARABOLIC, NEUMANN, BURGERS>(P, Bf, Ro, B, inst, lane, t, &a);
  }
}

template <bool PARABOLIC, bool BURGERS = false>
int launch_rollout(const pdegym_params1d* prm, const pdegym_bufs1d* buf, const pdegym_rollout1d* ro, int B, void* stream) {
  if (!prm || !buf || !ro) return pdegym::fail(-1, "null params/bufs/rollout");
  if (B <= 0 || ro->T <= 0) return 0;
  const pdegym_params1d& P = *prm;
  if (const int rc = check_rollout_plant(P, *buf, *ro, "rollout")) return rc;
  hipStream_t st = (hipStream_t)stream;
  const int nslots = P.n - (PARABOLIC ? 1 : 0);
  const int epl = (nslots + kWave - 1) / kWave;
  // the carried, register-resident form is the Dirichlet / full-state corner; everything else takes the general kernels
  const bool neumann = P.control_type == PDEGYM_CONTROL_NEUMANN;
  const bool general = neumann || P.sensing != PDEGYM_SENSE_FULL;
  if ((ro->obs_noise || ro->obs_seen) && !ro->policy) return pdegym::fail(-2, "rollout: obs_noise / obs_seen belong to the policy's input (policy is NULL)");
  if (ro->policy) {
    const pdegym_mlp& N = *ro->policy;
    const int od = P.sensing == PDEGYM_SENSE_FULL ? P.n : 1;
    const pdegym_policy::Plan pl = pdegym_policy::plan(&N, od, 1, B);
    if (pl.why) return pdegym::fail(-2, pl.why);
    if (N.x_f64 || N.y_f64) return pdegym::fail(-2, "policy inside the 1D rollout kernel: float32 observations and commands");
    if (epl > 8) return pdegym::fail(-2, "policy inside the rollout kernel: rows of up to 513 nodes");
    // (round 5, measured again after the loop lost its waits: the cooperative MFMA evaluation forced onto a 64-64 network is slower
    // than one fma chain per neuron -- 0.99 against 0.73 ms per 100 env-steps at S = 1, 0.55 against 0.45 ms per 25 at S = 100: four
    // workgroup barriers per env-step and twelve of sixteen waves without an output tile)
    const bool wide = pl.wide;
    int rc = 0;
    const char* const failure = "cannot raise the dynamic LDS limit of rollout1d_policy_kernel";
    constexpr std::true_type yes{};
    constexpr std::false_type no{};
    // each kernel is named where it is launched (tests/test_poison_helper.py reads the names there)
    // the head is compiled in (a run-time branch on it cost the plain head 1 % at C2: DESIGN.md section 4.11)
    auto with_head = [&](auto tag, auto gauss_tag) {
      constexpr int E = decltype(tag)::value;
      constexpr bool G = decltype(gauss_tag)::value;
      auto carried = [&](auto wide_tag, auto full_tag) {
        constexpr bool W = decltype(wide_tag)::value, F = decltype(full_tag)::value;
        if (pdegym_policy::lds_limit_raised<&rollout1d_policy_kernel<E, PARABOLIC, BURGERS, W, F, G>>(failure, rc))
          hipLaunchKernelGGL((rollout1d_policy_kernel<E, PARABOLIC, BURGERS, W, F, G>), pl.grid, pl.block, pl.lds_bytes, st, P, *buf, *ro, N, B);
      };
      auto in_general = [&](auto neumann_tag, auto wide_tag) {
        constexpr bool NEU = decltype(neumann_tag)::value, W = decltype(wide_tag)::value;
        if (pdegym_policy::lds_limit_raised<&rollout1d_policy_general_kernel<E, PARABOLIC, NEU, BURGERS, W, G>>(failure, rc))
          hipLaunchKernelGGL((rollout1d_policy_general_kernel<E, PARABOLIC, NEU, BURGERS, W, G>), pl.grid, pl.block, pl.lds_bytes, st, P, *buf, *ro, N, B);
      };
      if (general) {
        if (neumann) return wide ? in_general(yes, yes) : in_general(yes, no);
        return wide ? in_general(no, yes) : in_general(no, no);
      }
      if constexpr (epl_has_full(E)) {
        if (nslots == kWave * E) return wide ? carried(yes, yes) : carried(no, yes);
      }
      return wide ? carried(yes, no) : carried(no, no);
    };
    with_epl<8>(epl, [&](auto tag) { return pdegym_policy::is_gaussian(N) ? with_head(tag, yes) : with_head(tag, no); });
    return rc ? rc : pdegym::check_launch("rollout1d_policy");
  }
  const dim3 grid((B + kWavesPerBlock - 1) / kWavesPerBlock), block(kWave * kWavesPerBlock);
  // the same slots-per-lane choice as launch_step: the norm reductions (hence rewards) depend on the layout
  const bool per_step = (ro->reserved_ & PDEGYM_ROLLOUT_FINAL_OBS_PER_STEP) != 0;
  with_epl<32>(epl, [&](auto tag) {
    constexpr int E = decltype(tag)::value;
    auto carried = [&](auto full_tag) {
      constexpr bool F = decltype(full_tag)::value;
      if (per_step) hipLaunchKernelGGL((rollout1d_kernel<E, PARABOLIC, BURGERS, F, true>), grid, block, 0, st, P, *buf, *ro, B);
      else hipLaunchKernelGGL((rollout1d_kernel<E, PARABOLIC, BURGERS, F>), grid, block, 0, st, P, *buf, *ro, B);
    };
    if constexpr (epl_has_full(E)) {
      if (!general && nslots == kWave * E) return carried(std::true_type{});
    }
    if (!general) carried(std::false_type{});
    else if (neumann) hipLaunchKernelGGL((rollout1d_general_kernel<E, PARABOLIC, true, BURGERS>), grid, block, 0, st, P, *buf, *ro, B);
    else hipLaunchKernelGGL((rollout1d_general_kernel<E, PARABOLIC, false, BURGERS>), grid, block, 0, st, P, *buf, *ro, B);
  });
  return pdegym::check_launch("rollout1d");
}

}  // namespace

extern "C" {

int pdegym_transport_rollout(const pdegym_params1d* prm, const pdegym_bufs1d* buf, const pdegym_rollout1d* ro, int32_t B,
                             void* stream) {
  if (prm && prm->flux == PDEGYM_FLUX_BURGERS) return launch_rollout<false, true>(prm, buf, ro, B, stream);
  return launch_rollout<false, false>(prm, buf, ro, B, stream);
}

int pdegym_parabolic_rollout(const pdegym_params1d* prm, const pdegym_bufs1d* buf, const pdegym_rollout1d* ro, int32_t B,
                             void* stream) {
  return launch_rollout<true>(prm, buf, ro, B, stream);
}

}  // extern "C"
