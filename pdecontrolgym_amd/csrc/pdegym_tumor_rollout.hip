// pdegym_tumor_rollout.hip -- gfx950 kernel for TherapyWrapper(BrainTumor1D) steps (float64): one wrapper step of every patient, or a
// whole rollout of T wrapper steps with the policy inside, in ONE launch (brain_tumor_env.py:385-505).
//
// One 64-lane wavefront owns one patient for the whole launch, as in pdegym_tumor.hip: the density row ping-pongs between the
// wave's two LDS copies, the stage machine, the day counters and the wrapper's counters (consecutive treatment days, treatment
// calls, soft-constraint violations) stay in scalars, and global memory sees the state once at the end.  A wrapper step is what
// TumorVecEnv.step_tensor composes from launches -- a post-therapy run, or one treatment day (+ the two weekend days), the kept
// last row, the restart and the growth run of a finished patient -- as calls of the ONE simulated day of pdegym_tumor_body.h:
// the same expressions in the same order under the same flags, hence the same bits.
// With a policy (pdegym_policy.h, 16 waves per workgroup) the command of step t is evaluated from the row the wrapper returned at
// step t - 1, which the wave writes into its float32 policy row at the moment it stores the observation slot (no read-back from
// global memory, so no fence).  Layers of more than 64 units are evaluated by the 16 waves together, one workgroup barrier per
// layer per step: EVERY wave of the workgroup attends every barrier of every step -- a wave without a patient only attends, a wave
// in a 300-day run makes the others wait -- and none returns before the last step.
#include <hip/hip_runtime.h>

#include "pdegym.h"
#include "pdegym_common.h"
#include "pdegym_policy.h"
#include "pdegym_tumor_body.h"

namespace {

using namespace pdegym_tumor;      // tumor_stage_row, tumor_day, tumor_reset_scalars, tumor_store_scalars (pdegym_tumor_body.h)
namespace pol = pdegym_policy;

// obs0: observation slot 0 (read by a policy only); obs1: slot 1 (slot t + 1 = obs1 + t * B * nx) or nullptr (the observation is
// the live row, written once at the end); actions / rewards / terminated / truncated: rows of B, row t per wrapper step.
// final_stride: 0, or B * nx when wrap.final_obs is [T, B, nx] and step t keeps its last row in slot t (PDEGYM_ROLLOUT_FINAL_OBS_PER_STEP).
struct Slots {
  int T;
  int64_t final_stride;
  const double* obs0;
  double* obs1;
  double* actions;
  double* rewards;
  uint8_t* terminated;
  uint8_t* truncated;
};

template <bool WIDE, bool POLICY, bool GAUSS = false>
__global__ __launch_bounds__(kWave* pol::kWaves) void tumor_rollout_kernel(pdegym_params_tumor P, pdegym_bufs_tumor Bf, pdegym_wrap_tumor Wr,
                                                                           Slots Ro, pdegym_mlp N, int rows_off, int B) {
  static_assert(POLICY || !WIDE, "the cooperative evaluation belongs to a policy");
  extern __shared__ __attribute__((aligned(16))) float pol_smem[];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
  const int wpb = blockDim.x >> 6;      // 16 with a policy; 4, 2 or 1 without (the host's choice by nx)
  const int inst = __builtin_amdgcn_readfirstlane(blockIdx.x * wpb + wave);
  const int nx = P.nx;
  const bool active = inst < B;      // wave-uniform
  pol::PolicyWave W;
  pol::Wide Wd;
  if constexpr (POLICY) {
    if (!pol::prologue<WIDE>(W, Wd, N, pol_smem, nx, active, wave, lane)) return;
  }
  if (!active) {      // (WIDE: a wave without a patient attends the barriers of every step)
    if constexpr (WIDE) pol::attend(N, Wd, nx, Ro.T, wave, lane, std::bool_constant<GAUSS>{});
    return;
  }
  double* cur = reinterpret_cast<double*>(reinterpret_cast<char*>(pol_smem) + rows_off) + (size_t)(2 * wave) * nx;
  double* nxt = cur + nx;
  double* g = Bf.u + (size_t)inst * nx;
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  // ---- the patient: row into LDS, scalars into registers (read once)
  TumorState S;
  S.t = Bf.time_index[inst];
  S.stage = Bf.stage[inst];
  tumor_stage_row(P, g, cur, lane, S.t2_idx);
  S.remaining = Bf.remaining[inst];
  {
    const int32_t* days = Bf.days + (size_t)inst * PDEGYM_TUMOR_DAYS;
    S.growth = days[PDEGYM_TUMOR_DAY_GROWTH], S.therapyDays = days[PDEGYM_TUMOR_DAY_THERAPY];
    S.post = days[PDEGYM_TUMOR_DAY_POST], S.sim = days[PDEGYM_TUMOR_DAY_SIM], S.death = days[PDEGYM_TUMOR_DAY_DEATH];
  }
  const double tb = Bf.t_benchmark ? Bf.t_benchmark[inst] : nan;
  const bool has_tb = tb == tb;
  // E: the engine's own outputs of this patient -- every simulated day overwrites them, a step that simulates nothing keeps them
  TumorDay E;
  {
    const double* o = Bf.out + (size_t)inst * PDEGYM_TUMOR_OUTS;
    E.reward = Bf.reward[inst];
    E.term = Bf.terminated[inst] != 0;
    E.lethal = Bf.truncated[inst] != 0;
    E.T1 = o[PDEGYM_TUMOR_OUT_T1], E.T2 = o[PDEGYM_TUMOR_OUT_T2], E.treat_r = o[PDEGYM_TUMOR_OUT_TREAT], E.applied = o[PDEGYM_TUMOR_OUT_DOSE];
  }
  int cons = Wr.consecutive[inst];
  long long calls = Wr.treatment_calls[inst], viol = Wr.soft_constraint_violations[inst];
  const double* init_row = Wr.init + (size_t)inst * (size_t)Wr.init_stride;
  const size_t slot = (size_t)B * nx;
  if constexpr (POLICY) {      // the policy row of step 0: the caller's observation slot 0, rounded to float32
    const double* x0 = Ro.obs0 + (size_t)inst * nx;
    for (int j = lane; j < nx; j += kWave) W.xw[j] = (float)x0[j];
  }
  // The days of a wrapper step are ONE loop over phases with ONE copy of the simulated day in it (the day is ~1500 instructions):
  // a post-therapy run, or the treatment day and the two weekend days; then, for a finished patient, the growth run.
  enum { PH_NONE, PH_POST, PH_TREAT, PH_REST1, PH_REST2, PH_GROWTH };
  for (int t = 0; t < Ro.T; ++t) {
    // ---- today's command
    double a;
    if constexpr (POLICY) {
      wave_lds_sync();      // the policy row written by the step before (emit_row) or above
      const float o = pol::evaluate<WIDE, GAUSS>(W, Wd, N, pol_smem, nx, wave, lane);
      if constexpr (GAUSS)      // the squashed-Gaussian head: neuron 0 is mu, neuron 1 log_std
        a = (double)pol::shaped_gaussian(pol::command<WIDE>(o, Wd, wave, 0), pol::command<WIDE>(o, Wd, wave, 1), N, t, B, inst, 0);
      else
        a = (double)pol::shaped(pol::command<WIDE>(o, Wd, wave, 0), N, t, B, inst, 0);
      if (lane == 0) Ro.actions[(size_t)t * B + inst] = a;
    } else {
      a = Ro.actions[(size_t)t * B + inst];
    }
    double* oslot = Ro.obs1 ? Ro.obs1 + (size_t)t * slot + (size_t)inst * nx : nullptr;
    // the live row as the returned observation: the slot, and the float32 row the policy reads at the next step
    auto emit_row = [&]() {
      wave_lds_sync();
      for (int i = lane; i < nx; i += kWave) {
        const double v = cur[i];
        if (oslot) oslot[i] = v;
        if constexpr (POLICY) W.xw[i] = (float)v;
      }
    };
    // ---- TherapyWrapper.step :430-486
    const int stage0 = S.stage;
    bool rest = false;
    // Growth (its growth run hit the time limit) is outside the wrapper's contract: nothing is simulated, reward 0, no flag
    double rep_reward = 0.0, keep_reward = 0.0;
    bool rep_term = false, rep_lethal = false, keep_term = false, keep_lethal = false;
    int phase = stage0 == PDEGYM_TUMOR_POST ? PH_POST : (stage0 == PDEGYM_TUMOR_THERAPY ? PH_TREAT : PH_NONE);
    while (phase != PH_NONE) {
      const bool live = S.t < P.nt - 1;                                 // :136
      const bool run = phase == PH_POST || phase == PH_GROWTH;          // env.step(0) until ... (pdegym_tumor_advance)
      if (live) {
        tumor_day<false>(P, Bf.xscale, S, E, phase == PH_TREAT ? a : 0.0, false, nullptr, inst, cur, nxt, nullptr, nullptr, nullptr, tb,
                         has_tb, lane);
      } else if (!run) {      // one env.step past the last day (pdegym_tumor_step): state and out stay, reward 0, no flag
        E.reward = 0.0;
        E.term = E.lethal = false;
      }
      const bool ended = E.term || E.lethal;
      bool report = false;
      if (phase == PH_POST) {                                           // :437-446 (a run that cannot start reports what it found)
        report = !live || ended;
      } else if (phase == PH_TREAT) {                                   // :452-456
        calls += 1;
        viol += E.reward < 0.0 ? 1 : 0;
        report = true;
        if (Wr.weekends) {                                              // :458-472
          cons = a > 0.0 ? cons + 1 : 0;
          rest = cons >= 5 && !ended;
          if (rest) {
            cons = 0;
            keep_reward = E.reward;
            keep_term = E.term;
            keep_lethal = E.lethal;
            emit_row();                                                 // the wrapper returns the TREATMENT day's row (:456, :481)
            report = false;
            phase = PH_REST1;
          }
        }
      } else if (phase == PH_REST1) {
        phase = PH_REST2;
      } else if (phase == PH_REST2) {                                   // the weekend's reward and flags are discarded
        E.reward = keep_reward;
        E.term = keep_term;
        E.lethal = keep_lethal;
        report = true;
      } else {                                                          // PH_GROWTH :409-428
        if (!live || ended || S.stage != PDEGYM_TUMOR_GROWTH) phase = PH_NONE;
      }
      if (report) {
        rep_reward = E.reward;
        rep_term = E.term;
        rep_lethal = E.lethal;
        phase = PH_NONE;
        if (rep_term || rep_lethal) {                                   // SB3 auto-reset: keep the last row, restart, growth run
          wave_lds_sync();
          if (Wr.final_obs) {
            double* fo = Wr.final_obs + (size_t)t * (size_t)Ro.final_stride + (size_t)inst * nx;
            for (int i = lane; i < nx; i += kWave) fo[i] = cur[i];
          }
          tumor_stage_row(P, init_row, cur, lane, S.t2_idx);
          tumor_reset_scalars(P, S);
          cons = 0;
          phase = PH_GROWTH;
        }
      }
    }
    if (!rest) emit_row();
    if (lane == 0) {
      Ro.rewards[(size_t)t * B + inst] = rep_reward;
      Ro.terminated[(size_t)t * B + inst] = rep_term;
      Ro.truncated[(size_t)t * B + inst] = rep_lethal;
    }
    E.reward = rep_reward;      // the engine's reward and flags are the step's reported ones (out: the last simulated day's)
    E.term = rep_term;
    E.lethal = rep_lethal;
  }
  // ---- state, counters and the engine's [B] outputs, written once
  wave_lds_sync();
  for (int i = lane; i < nx; i += kWave) g[i] = cur[i];
  if (lane != 0) return;
  tumor_store_scalars(Bf, inst, S);
  Bf.reward[inst] = E.reward;
  Bf.terminated[inst] = E.term;
  Bf.truncated[inst] = E.lethal;
  double* o = Bf.out + (size_t)inst * PDEGYM_TUMOR_OUTS;
  o[PDEGYM_TUMOR_OUT_T1] = E.T1;
  o[PDEGYM_TUMOR_OUT_T2] = E.T2;
  o[PDEGYM_TUMOR_OUT_TREAT] = E.treat_r;
  o[PDEGYM_TUMOR_OUT_DOSE] = E.applied;
  Wr.consecutive[inst] = cons;
  Wr.treatment_calls[inst] = calls;
  Wr.soft_constraint_violations[inst] = viol;
}

int check_wrap(const pdegym_params_tumor* prm, const pdegym_bufs_tumor* buf, const pdegym_wrap_tumor* wrap) {
  if (int rc = check(prm, buf)) return rc;
  if (!wrap) return pdegym::fail(-1, "null wrapper state");
  if (!buf->xscale || !buf->reward || !buf->terminated || !buf->truncated || !buf->out) return pdegym::fail(-3, "null device buffer");
  if (buf->history || buf->t1_log) return pdegym::fail(-2, "tumor wrapper step: history / t1_log recording is not supported inside the launch");
  if (!wrap->init) return pdegym::fail(-1, "null init");
  if (wrap->init_stride != 0 && wrap->init_stride < prm->nx) return pdegym::fail(-2, "tumor wrapper step: init_stride must be 0 (one shared row) or >= nx");
  if (!wrap->consecutive || !wrap->treatment_calls || !wrap->soft_constraint_violations) return pdegym::fail(-3, "null wrapper counter");
  return 0;
}

// one launch of T wrapper steps; net: the policy or nullptr
int launch(const pdegym_params_tumor* prm, const pdegym_bufs_tumor* buf, const pdegym_wrap_tumor* wrap, const Slots& ro, const pdegym_mlp* policy,
           int32_t B, void* stream, const char* what) {
  const int nx = prm->nx;
  const size_t row_bytes = (size_t)2 * nx * sizeof(double);      // two LDS rows per wave, after the policy's floats
  const int wpb = nx <= 1024 ? 4 : (nx <= 2048 ? 2 : 1);      // no policy: at most 64 KB of rows per workgroup
  pol::Plan pl = {nullptr, false, 0, wpb * row_bytes, dim3((B + wpb - 1) / wpb), dim3(kWave * wpb)};
  if (policy) {
    pl = pol::plan(policy, nx, 1, B, pol::kWaves * row_bytes);
    if (pl.why) return pdegym::fail(-2, pl.why);
    if (pl.lds_bytes > (size_t)pol::kMaxLdsBytes)
      return pdegym::fail(-2, "tumor rollout: the policy's LDS and two float64 rows for each of 16 patients do not fit into 160 KB of LDS");
  }
  const pdegym_mlp net = policy ? *policy : pdegym_mlp{};
  int rc = 0;
  pol::dispatch(policy, pl.wide, [&](auto wide_tag, auto policy_tag, auto gauss_tag) {
    constexpr bool W = decltype(wide_tag)::value, Pol = decltype(policy_tag)::value, G = decltype(gauss_tag)::value;
    if (!Pol || pol::lds_limit_raised<&tumor_rollout_kernel<W, Pol, G>>("cannot raise the dynamic LDS limit of tumor_rollout_kernel", rc))
      tumor_rollout_kernel<W, Pol, G><<<pl.grid, pl.block, pl.lds_bytes, (hipStream_t)stream>>>(*prm, *buf, *wrap, ro, net, (int)pl.extra_off, B);
  });
  return rc ? rc : pdegym::check_launch(what);
}

}  // namespace

extern "C" {

int pdegym_tumor_therapy_step(const pdegym_params_tumor* prm, const pdegym_bufs_tumor* buf, const pdegym_wrap_tumor* wrap, int32_t B,
                              void* stream) {
  if (int rc = check_wrap(prm, buf, wrap)) return rc;
  if (!buf->control) return pdegym::fail(-3, "null device buffer");
  if (wrap->weekends && !wrap->obs)
    return pdegym::fail(-2, "tumor wrapper step: weekends needs an obs row per patient (a resting patient returns the treatment day's row, not the live one)");
  if (B <= 0) return 0;
  const Slots ro = {1, 0, nullptr, wrap->obs, const_cast<double*>(buf->control), buf->reward, buf->terminated, buf->truncated};
  return launch(prm, buf, wrap, ro, nullptr, B, stream, "tumor_therapy_step");
}

int pdegym_tumor_rollout(const pdegym_params_tumor* prm, const pdegym_bufs_tumor* buf, const pdegym_wrap_tumor* wrap,
                         const pdegym_rollout_tumor* ro, int32_t B, void* stream) {
  if (int rc = check_wrap(prm, buf, wrap)) return rc;
  if (!ro) return pdegym::fail(-1, "null rollout descriptor");
  if (B <= 0 || ro->T <= 0) return 0;
  if (!ro->obs || !ro->actions || !ro->rewards || !ro->terminated || !ro->truncated) return pdegym::fail(-3, "null rollout buffer");
  const bool per_step = (ro->reserved_ & PDEGYM_ROLLOUT_FINAL_OBS_PER_STEP) != 0;
  if (per_step && !wrap->final_obs) return pdegym::fail(-3, "tumor rollout: PDEGYM_ROLLOUT_FINAL_OBS_PER_STEP needs wrap->final_obs [T, B, nx]");
  const Slots s = {ro->T, per_step ? (int64_t)B * prm->nx : 0, ro->obs, ro->obs + (size_t)B * prm->nx, ro->actions, ro->rewards, ro->terminated, ro->truncated};
  return launch(prm, buf, wrap, s, ro->policy, B, stream, "tumor_rollout");
}

}  // extern "C"
