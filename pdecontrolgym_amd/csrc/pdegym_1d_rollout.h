// pdegym_1d_rollout.h -- what the one-launch 1D rollout units share (pdegym_1d_rollout.hip: open loop and with the MLP policy inside;
// pdegym_backstep_rollout.hip: with the backstepping law inside), one copy of each: the sensing noise, the carried row's way to LDS, the
// per-step view of the rollout arrays, the checks of the plant.  (The slots-per-lane ladder, with_epl / epl_has_full, is the step launcher's
// too: pdegym_1d_body.h.)  Kernels and launches stay in the .hip files.
#pragma once
#include <cstdio>

#include "pdegym_1d_body.h"

namespace {

// The sensing-noise hook of the reference (hyperbolic.py:160-164: the agent sees sensing_noise_func(observation)) as pre-drawn
// additive noise: the wave's LDS copy of observation t (od values) becomes obs + obs_noise[t], which is what the controller reads
// and what obs_seen[t] receives; the observation slots themselves -- the plant state with full-state sensing -- stay clean.
__device__ __forceinline__ void sense_noise(const float* obs_noise, float* obs_seen, float* xw, int od, int B, int inst, int lane, int t) {
  if (!obs_noise && !obs_seen) return;     // wave-uniform
  const size_t base = ((size_t)t * B + inst) * od;
  for (int j = lane; j < od; j += kWave) {
    float v = xw[j];
    if (obs_noise) v += obs_noise[base + j];
    xw[j] = v;
    if (obs_seen) obs_seen[base + j] = v;
  }
  wave_lds_sync();
}

// Observation of a carried instance -> the wave's LDS row xw, straight from the registers (slot t of the rollout's obs holds the same values).
// n is the kernel argument even under FULL: with a compile-time trip count the compiler unrolls the policy's whole reduction and spills 74 registers.
template <int EPL, bool PARABOLIC>
__device__ __forceinline__ void stage_carried_row(const Carry<EPL>& C, float* xw, int n, int lane) {
  constexpr int J0 = PARABOLIC ? 1 : 0;
  const int ns = n - J0, s0 = lane * EPL;
  if (PARABOLIC && lane == 0) xw[0] = C.bl;
#pragma unroll
  for (int e = 0; e < EPL; ++e)
    if (s0 + e < ns) xw[J0 + s0 + e] = C.x[e];
  wave_lds_sync();
}

// The buffers as env-step t of a rollout sees them: observation slot t + 1 out (slot = B * observation length, in floats), row t of
// the [T, B] arrays.  full (full-state sensing): the state comes from slot t; otherwise it lives in bufs.u, advanced in place.
// PDEGYM_ROLLOUT_FINAL_OBS_PER_STEP: bufs.final_obs is [T, B, observation length] and step t sees slot t of it.  (rollout1d_kernel,
// whose view advances incrementally, has the mode as a template parameter instead: pdegym_1d_rollout.hip.)
__device__ __forceinline__ size_t terminal_obs_stride(const pdegym_rollout1d& Ro, size_t slot) {
  return (Ro.reserved_ & PDEGYM_ROLLOUT_FINAL_OBS_PER_STEP) ? slot : 0;      // uniform over the launch
}

__device__ __forceinline__ pdegym_bufs1d rollout_step_view(const pdegym_bufs1d& Bf, const pdegym_rollout1d& Ro, int B, size_t slot, int t,
                                                           bool full = true) {
  pdegym_bufs1d S = Bf;
  S.history = nullptr;
  S.final_obs = Bf.final_obs + (size_t)t * terminal_obs_stride(Ro, slot);      // (NULL stays NULL: the launchers refuse the flag without it)
  if (full) S.u = nullptr;
  S.state_in = full ? Ro.obs + (size_t)t * slot : nullptr;
  S.obs = Ro.obs + (size_t)(t + 1) * slot;
  S.action = Ro.actions + (size_t)t * B;
  S.reward = Ro.rewards + (size_t)t * B;
  S.terminated = Ro.terminated + (size_t)t * B;
  S.truncated = Ro.truncated + (size_t)t * B;
  return S;
}

// What every 1D rollout entry point asks of the plant and its buffers, in one order: 0, or the code to return (message, who in front, in the error slot).
inline int check_rollout_plant(const pdegym_params1d& P, const pdegym_bufs1d& buf, const pdegym_rollout1d& ro, const char* who) {
  auto fail = [who](int code, const char* msg) { return std::snprintf(pdegym::error_slot(), 512, "%s: %s", who, msg), code; };
  if (P.n < 3 || P.n > PDEGYM_MAX_N1D) return fail(-2, "n must be in [3, 2048] (register-resident rows)");
  if (P.nt < 2) return fail(-2, "nt must be >= 2");
  if (P.sensing < PDEGYM_SENSE_FULL || P.sensing > PDEGYM_SENSE_FIRST) return fail(-2, "bad sensing code");
  if (P.sensing != PDEGYM_SENSE_FULL && !buf.u) return fail(-3, "with scalar sensing the state lives in bufs.u (obs slots hold the sensed values)");
  if (P.control_type != PDEGYM_CONTROL_DIRICHLET && P.control_type != PDEGYM_CONTROL_NEUMANN) return fail(-2, "bad control_type");
  if (P.beta_f64 || P.action_kind != PDEGYM_ACTION_F32) return fail(-2, "float32 beta and actions only");
  if (buf.history) return fail(-2, "a rollout cannot record a history buffer");
  if (P.reward_horizon != PDEGYM_HORIZON_TEMPORAL) return fail(-2, "only the temporal reward horizon is evaluated in the rollout kernels");
  if (!buf.beta || !buf.time_index || !buf.bsum || !buf.ring || !buf.norm_now || !buf.norm_back) return fail(-3, "null device buffer");
  if (!ro.obs || !ro.actions || !ro.terminated || !ro.truncated) return fail(-3, "null rollout buffer");
  if (P.reward_kind != PDEGYM_REWARD_NONE && !ro.rewards) return fail(-3, "null reward buffer");
  if (ro.reserved_ & PDEGYM_ROLLOUT_FINAL_OBS_PER_STEP) {
    if (!buf.final_obs) return fail(-3, "PDEGYM_ROLLOUT_FINAL_OBS_PER_STEP needs bufs->final_obs [T, B, obs_dim]");
    if (!buf.reset_init) return fail(-2, "PDEGYM_ROLLOUT_FINAL_OBS_PER_STEP needs the auto-reset pool (reset_init): only a restart keeps a final observation");
  }
  return 0;
}

}  // namespace
