// pdegym_traffic.hip -- gfx950 kernel for the Aw-Rascle-Zhang traffic environment (float64).
//
// One 64-lane wavefront owns one freeway instance, lane j holds node j (the reference's M = 51 nodes), both fields
// (r, y) stay in registers for the control_freq sub-steps of a step() call.  Neighbour values cross lanes with
// wave shuffles; the "minus" midpoint of node j IS the "plus" midpoint of node j-1 (same floating-point expression,
// addition is commutative), so each lane evaluates one midpoint flux and the other arrives from lane j-1.
// Operation order follows environments1d/traffic_arz_env.py:172-227 exactly (-ffp-contract=off, IEEE division):
// fields are bit-identical to NumPy; the reward norms are wave reductions (rtol 1e-14 vs BLAS ddot).
#include <hip/hip_runtime.h>

#include "pdegym.h"
#include "pdegym_common.h"
#include "pdegym_policy.h"
#include "pdegym_traffic_body.h"      // Veq / F_r / F_y, TrafficConsts, traffic_commands, traffic_step_wave, traffic_emit_obs, traffic_auto_reset

namespace {

// the commands of a step (traffic_commands) read from bufs.action (action_stride 1: one command per freeway, no second column to read)
__device__ __forceinline__ void traffic_load_action(const pdegym_bufs_traffic& Bf, int inst, double& a0, double& a1) {
  const int astr = Bf.action_stride > 0 ? Bf.action_stride : 2;
  a0 = Bf.action[(size_t)inst * astr];
  a1 = astr > 1 ? Bf.action[(size_t)inst * astr + 1] : 0.0;
}

__global__ __launch_bounds__(kWave* kWavesPerBlock) void traffic_step_kernel(pdegym_params_traffic P, pdegym_bufs_traffic Bf, TrafficConsts K, int B) {
  const int lane = threadIdx.x & (kWave - 1);
  const int inst = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
  if (inst >= B) return;
  const int M = P.M;
  const bool in = lane < M;
  double r = in ? Bf.r[(size_t)inst * M + lane] : 1.0;
  double y = in ? Bf.y[(size_t)inst * M + lane] : 0.0;
  double rs = Bf.rs[inst];
  double a0, a1;
  traffic_load_action(Bf, inst, a0, a1);
  double time = Bf.time[inst];
  const TrafficStepOut o = traffic_step_wave(P, K, r, y, time, rs, Bf.qs_clip[inst], a0, a1, lane);
  double* ob = Bf.obs + (size_t)inst * 2 * M;
  if (Bf.reset_rs && (o.done || o.trunc)) {       // wave-uniform
    traffic_auto_reset(P, Bf, Bf.final_obs, inst, B, 0, in ? Bf.reset_profile[lane] : 1.0, r, y, rs, o.v, o.vs, ob, lane);
    time = 0.0;
    if (lane == 0) {
      Bf.rs[inst] = rs;
      if (Bf.reset_count) Bf.reset_count[inst] += 1;
    }
  } else {
    traffic_emit_obs(P, ob, r, o.v, rs, o.vs, lane);
  }
  if (in) {
    Bf.r[(size_t)inst * M + lane] = r;
    Bf.y[(size_t)inst * M + lane] = y;
  }
  if (lane == 0) {
    Bf.time[inst] = time;
    Bf.reward[inst] = o.reward;
    Bf.done[inst] = o.done ? 1 : 0;
    Bf.truncated[inst] = o.trunc ? 1 : 0;
  }
}

// T env-steps of one freeway by one wave in ONE launch (pdegym_traffic_rollout): (r, y) stay in registers across env-steps,
// iteration t is traffic_step_wave with the command of row t, and writes observation slot t + 1, reward / done / truncated row
// t -- bit-identical to T pdegym_traffic_step calls (a finished episode keeps running, as it does there: restarting is the
// caller's business in this engine).  With a policy (pdegym_policy.h) the command of step t is computed inside the launch
// from observation slot t rounded to float32 -- the cast SB3 makes in front of its float32 network -- widened back to
// float64, plus noise, clamped, and stored to actions row t.
// WIDE: a policy with a layer of more than 64 units -- the 16 waves of the workgroup evaluate it together; a wave without a freeway
// only attends their barriers (pdegym_policy.h: attend) and loads nothing.
// POLICY: compiled apart, so that the commands-given-ahead form carries none of the policy's loads (a load under a run-time branch
// leaves the compiler's wait-count pass with "may be pending" registers at every join of the loop).
template <bool WIDE, bool POLICY, bool GAUSS = false>
__global__ __launch_bounds__(kWave* pdegym_policy::kWaves) void traffic_rollout_kernel(pdegym_params_traffic P, pdegym_bufs_traffic Bf,
                                                                                       pdegym_rollout_traffic Ro, pdegym_mlp N, TrafficConsts K,
                                                                                       int B) {
  static_assert(POLICY || !WIDE, "the cooperative evaluation belongs to a policy");
  constexpr bool has_policy = POLICY;
  namespace pol = pdegym_policy;
  extern __shared__ __attribute__((aligned(16))) float pol_smem[];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
  const int inst = blockIdx.x * pol::kWaves + wave;
  const int M = P.M, D = 2 * M;
  const bool active = inst < B;      // wave-uniform
  pol::PolicyWave W;
  pol::Wide Wd;
  if constexpr (has_policy) {
    if (!pol::prologue<WIDE>(W, Wd, N, pol_smem, D, active, wave, lane)) return;
  }
  if (!active) {
    if constexpr (WIDE) pol::attend(N, Wd, D, Ro.T, wave, lane, std::bool_constant<GAUSS>{});
    return;
  }
  const bool in = lane < M;
  double r = in ? Bf.r[(size_t)inst * M + lane] : 1.0;
  double y = in ? Bf.y[(size_t)inst * M + lane] : 0.0;
  double rs = Bf.rs[inst];
  const double qc = Bf.qs_clip[inst];
  double time = Bf.time[inst];
  int restarts = 0;
  const double prof = (Bf.reset_rs && in) ? Bf.reset_profile[lane] : 1.0;
  const int A = Bf.action_stride > 0 ? Bf.action_stride : 2;
  const size_t slot = (size_t)B * D;
  // commands given ahead (no policy): 64 env-steps per load -- lane l holds the command(s) of step t0 + l, handed out by v_readlane --
  // and no fence between iterations (nothing stored by an iteration is read by the next): as in rollout1d_kernel, a load or a
  // fence per env-step makes every step wait for the stores of the step before (gfx9 counts both in vmcnt)
  auto command_batch = [&](int t0, int col) {
    return (!has_policy && t0 + lane < Ro.T && col < A) ? Ro.actions[((size_t)(t0 + lane) * B + inst) * A + col] : 0.0;
  };
  double b0 = command_batch(0, 0), b1 = command_batch(0, 1);
  // drain_vmem() wherever the open-loop form loads (here, at a batch hand-over, after a restart): the wait-count pass then knows
  // that nothing is pending at the joins of the loop and puts no static wait into its steady state
  if constexpr (!has_policy) drain_vmem();
  for (int t = 0; t < Ro.T; ++t) {
    double* arow = Ro.actions + ((size_t)t * B + inst) * A;
    double a0, a1 = 0.0;
    const int tj = t & (kWave - 1);
    if (!has_policy && tj == 0 && t) {      // wave-uniform, once per 64 env-steps; the loop's only wait for memory
      b0 = command_batch(t, 0);
      b1 = command_batch(t, 1);
      drain_vmem();
    }
    if constexpr (has_policy) {
      const double* xrow = Ro.obs + (size_t)t * slot + (size_t)inst * D;
      for (int j = lane; j < D; j += kWave) W.xw[j] = (float)xrow[j];
      wave_lds_sync();
      const float o = pol::evaluate<WIDE, GAUSS>(W, Wd, N, pol_smem, D, wave, lane);      // one evaluation, both commands
      if constexpr (GAUSS) {      // the squashed-Gaussian head: neurons 0 .. A-1 are mu, A .. 2A-1 log_std
        a0 = (double)pol::shaped_gaussian(pol::command<WIDE>(o, Wd, wave, 0), pol::command<WIDE>(o, Wd, wave, A), N, t, B, inst, 0);
        if (A > 1) a1 = (double)pol::shaped_gaussian(pol::command<WIDE>(o, Wd, wave, 1), pol::command<WIDE>(o, Wd, wave, A + 1), N, t, B, inst, 1);
      } else {
        a0 = (double)pol::shaped(pol::command<WIDE>(o, Wd, wave, 0), N, t, B, inst, 0);
        if (A > 1) a1 = (double)pol::shaped(pol::command<WIDE>(o, Wd, wave, 1), N, t, B, inst, 1);
      }
      if (lane == 0) {
        arow[0] = a0;
        if (A > 1) arow[1] = a1;
      }
    } else {
      a0 = lane_value(b0, tj);
      a1 = lane_value(b1, tj);
    }
    const TrafficStepOut o = traffic_step_wave(P, K, r, y, time, rs, qc, a0, a1, lane);
    double* onext = Ro.obs + (size_t)(t + 1) * slot + (size_t)inst * D;
    if (Bf.reset_rs && (o.done || o.trunc)) {     // wave-uniform
      traffic_auto_reset(P, Bf, traffic_terminal_slot(Bf, Ro, slot, t), inst, B, restarts, prof, r, y, rs, o.v, o.vs, onext, lane);
      ++restarts;
      time = 0.0;
      if constexpr (!has_policy) drain_vmem();
    } else {
      traffic_emit_obs(P, onext, r, o.v, rs, o.vs, lane);
    }
    if (lane == 0) {
      Ro.rewards[(size_t)t * B + inst] = o.reward;
      Ro.done[(size_t)t * B + inst] = o.done ? 1 : 0;
      Ro.truncated[(size_t)t * B + inst] = o.trunc ? 1 : 0;
    }
    if constexpr (has_policy) {      // the observation row just stored is read back (by other lanes) at the start of the next iteration
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    }
  }
  // (never taken; without it the compiler inverts the exit test of the open-loop form's loop, which otherwise is the parent form's
  // instruction for instruction: profiles/policy_host_resources.txt)
  if (!active) return;
  if (in) {
    Bf.r[(size_t)inst * M + lane] = r;
    Bf.y[(size_t)inst * M + lane] = y;
  }
  if (lane == 0) {
    Bf.time[inst] = time;
    if (restarts) {
      Bf.rs[inst] = rs;
      if (Bf.reset_count) Bf.reset_count[inst] += restarts;
    }
  }
}

// ---- rows of more than 64 nodes (finer grids than the reference notebook's M = 51): one wave still owns one freeway,
// node j lives in lane j % 64; the fields and the per-sub-step intermediates go through a wave-private LDS region so that
// every node reaches its neighbours (wave-level ordering only: no workgroup barrier).  Same expressions, same order; the commands
// and the end of the step are the register kernel's (traffic_commands, traffic_step_end), the sub-step loop and the auto-reset are
// strided loops over the LDS rows and stay this kernel's own.
__global__ __launch_bounds__(kWave* kWavesPerBlock) void traffic_step_wide_kernel(pdegym_params_traffic P, pdegym_bufs_traffic Bf, TrafficConsts K, int B) {
  extern __shared__ double tl[];
  const int lane = threadIdx.x & (kWave - 1);
  const int w = threadIdx.x >> 6, wpb = blockDim.x >> 6;
  const int inst = __builtin_amdgcn_readfirstlane(blockIdx.x * wpb + w);
  if (inst >= B) return;
  const int M = P.M;
  double* R = tl + (size_t)w * 7 * M;      // r, y, fr, fy | y_pm, Frp, Fyp
  double* Y = R + M;
  double* FR = Y + M;
  double* FY = FR + M;
  double* YPM = FY + M;
  double* FRP = YPM + M;
  double* FYP = FRP + M;
  const double vm = P.vm, rm = P.rm;
  for (int j = lane; j < M; j += kWave) {
    R[j] = Bf.r[(size_t)inst * M + j];
    Y[j] = Bf.y[(size_t)inst * M + j];
  }
  const double rs = Bf.rs[inst];
  const double vs = Veq(vm, rm, rs);
  double a0, a1, q_in, q_out;
  traffic_load_action(Bf, inst, a0, a1);
  traffic_commands(P, Bf.qs_clip[inst], rs * vs, a0, a1, q_in, q_out);
  double time = Bf.time[inst] + P.dt;
  const double c1 = K.c1, c2 = K.c2, c3 = K.c3, c4 = K.c4;
  wave_lds_sync();
  if (time < P.T) {
    for (int s = 0; s < P.control_freq; ++s) {
      // boundary conditions :174-190 (read the neighbours first, then overwrite the two end nodes)
      const double r1 = R[1], rm2 = R[M - 2];
      wave_lds_sync();
      if (lane == 0) {
        R[0] = r1;
        Y[0] = q_in - r1 * Veq(vm, rm, r1);
        R[M - 1] = rm2;
        Y[M - 1] = q_out - rm2 * Veq(vm, rm, rm2);
      }
      wave_lds_sync();
      for (int j = lane; j < M; j += kWave) {      // nodal fluxes :201-204
        const double r = R[j], y = Y[j];
        FR[j] = F_r(vm, rm, r, y);
        FY[j] = F_y(vm, rm, r, y);
      }
      wave_lds_sync();
      for (int j = lane; j < M - 1; j += kWave) {  // "plus" midpoint of node j and its fluxes :205-216
        const double r = R[j], y = Y[j], r_p = R[j + 1], y_p = Y[j + 1];
        const double r_pm = 0.5 * (r_p + r) - c1 * (FR[j + 1] - FR[j]);
        const double y_pm = (0.5 * (y_p + y) - c1 * (FY[j + 1] - FY[j])) - c2 * (y_p + y);
        YPM[j] = y_pm;
        FRP[j] = F_r(vm, rm, r_pm, y_pm);
        FYP[j] = F_y(vm, rm, r_pm, y_pm);
      }
      wave_lds_sync();
      for (int j = lane; j < M; j += kWave) {      // inner update :219-223 ("minus" midpoint of j = "plus" of j-1)
        if (j >= 1 && j <= M - 2) {
          const double r = R[j], y = Y[j];
          R[j] = r - c3 * (FRP[j] - FRP[j - 1]);
          Y[j] = y - (c3 * (FYP[j] - FYP[j - 1]) + c4 * (YPM[j] + YPM[j - 1]));
        }
      }
      wave_lds_sync();
    }
  }
  double sv = 0.0, sr = 0.0;
  bool over = false, moved = false;
  double* o = Bf.obs + (size_t)inst * 2 * M;
  for (int j = lane; j < M; j += kWave) {
    const double r = R[j], y = Y[j];
    const double v = y / r + Veq(vm, rm, r);       // :227
    const double dv = v - vs, dr = r - rs;
    sv += dv * dv;
    sr += dr * dr;
    over = over || v > vm || r > rm;
    moved = moved || dr != 0.0 || dv != 0.0;
    Bf.r[(size_t)inst * M + j] = r;
    Bf.y[(size_t)inst * M + j] = y;
    traffic_emit_obs(P, o, r, v, rs, vs, j);
  }
  const TrafficEnd e = traffic_step_end(P, K, wave_sum(sv), wave_sum(sr), over, moved, time, vs, rs, lane);
  if (Bf.reset_rs && (e.done || e.trunc)) {       // fused auto-reset, as traffic_auto_reset (each lane re-reads its own stores)
    const double rs_new = Bf.reset_rs[pool_row(Bf.reset_pool_rows, Bf.reset_count, inst, B)];
    double* fo = Bf.final_obs ? Bf.final_obs + (size_t)inst * 2 * M : nullptr;
    for (int j = lane; j < M; j += kWave) {
      if (fo) {
        fo[j] = o[j];
        fo[M + j] = o[M + j];
      }
      double r, y, v;
      traffic_restart_node(P, rs_new, Bf.reset_profile[j], r, y, v);
      Bf.r[(size_t)inst * M + j] = r;
      Bf.y[(size_t)inst * M + j] = y;
      o[j] = r;
      o[M + j] = v;
    }
    time = 0.0;
    if (lane == 0) {
      Bf.rs[inst] = rs_new;
      if (Bf.reset_count) Bf.reset_count[inst] += 1;
    }
  }
  if (lane == 0) {
    Bf.time[inst] = time;
    Bf.reward[inst] = e.reward;
    Bf.done[inst] = e.done ? 1 : 0;
    Bf.truncated[inst] = e.trunc ? 1 : 0;
  }
}

__global__ __launch_bounds__(kWave* kWavesPerBlock) void traffic_reset_kernel(pdegym_params_traffic P, pdegym_bufs_traffic Bf,
                                                                               const double* profile, const uint8_t* mask, int B) {
  const int lane = threadIdx.x & (kWave - 1);
  const int inst = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
  if (inst >= B || (mask && !mask[inst])) return;
  const int M = P.M;
  const double rs = Bf.rs[inst];
  for (int j = lane; j < M; j += kWave) {
    double r, y, v;
    traffic_restart_node(P, rs, profile[j], r, y, v);
    Bf.r[(size_t)inst * M + j] = r;
    Bf.y[(size_t)inst * M + j] = y;
    Bf.obs[(size_t)inst * 2 * M + j] = r;
    Bf.obs[(size_t)inst * 2 * M + M + j] = v;
  }
  if (lane == 0) {
    Bf.time[inst] = 0.0;
    Bf.done[inst] = 0;
    Bf.truncated[inst] = 0;
  }
}

int check(const pdegym_params_traffic* prm, const pdegym_bufs_traffic* buf) {
  if (!prm || !buf) return pdegym::fail(-1, "null params/bufs");
  if (prm->M < 4 || prm->M > PDEGYM_TRAFFIC_MAX_M) return pdegym::fail(-2, "traffic: M must be in [4, 1024]");
  if (prm->control_freq < 1) return pdegym::fail(-2, "control_freq must be >= 1");
  if (prm->sim < 0 || prm->sim > 3) return pdegym::fail(-2, "bad simulation type");
  if (!buf->r || !buf->y || !buf->time || !buf->rs || !buf->qs_clip || !buf->obs || !buf->done || !buf->truncated)
    return pdegym::fail(-3, "null device buffer");
  if (buf->reset_rs && !buf->reset_profile) return pdegym::fail(-3, "reset_rs needs reset_profile");
  if (buf->reset_pool_rows < 0) return pdegym::fail(-2, "reset_pool_rows must be >= 0");
  return 0;
}

}  // namespace

extern "C" {

int pdegym_traffic_step(const pdegym_params_traffic* prm, const pdegym_bufs_traffic* buf, int32_t B, void* stream) {
  if (int rc = check(prm, buf)) return rc;
  if (!buf->action || !buf->reward) return pdegym::fail(-3, "null device buffer");
  if (B <= 0) return 0;
  if (prm->M <= kWave) {       // the reference's grid (M = 51): one node per lane, fields in registers
    const dim3 grid((B + kWavesPerBlock - 1) / kWavesPerBlock), block(kWave * kWavesPerBlock);
    hipLaunchKernelGGL(traffic_step_kernel, grid, block, 0, (hipStream_t)stream, *prm, *buf, traffic_consts(*prm), B);
  } else {                     // finer grids: wave-private LDS rows, at most 56 KB per workgroup
    const int wpb = prm->M <= 256 ? 4 : (prm->M <= 512 ? 2 : 1);
    const dim3 grid((B + wpb - 1) / wpb), block(kWave * wpb);
    hipLaunchKernelGGL(traffic_step_wide_kernel, grid, block, (size_t)wpb * 7 * prm->M * sizeof(double), (hipStream_t)stream,
                       *prm, *buf, traffic_consts(*prm), B);
  }
  return pdegym::check_launch("traffic_step");
}

int pdegym_traffic_rollout(const pdegym_params_traffic* prm, const pdegym_bufs_traffic* buf, const pdegym_rollout_traffic* ro, int32_t B,
                           void* stream) {
  if (int rc = check(prm, buf)) return rc;
  if (!ro) return pdegym::fail(-1, "null rollout descriptor");
  if (B <= 0 || ro->T <= 0) return 0;
  if (prm->M > kWave) return pdegym::fail(-2, "traffic rollout: freeways of up to 64 nodes (the register-resident kernel)");
  if (!ro->obs || !ro->actions || !ro->rewards || !ro->done || !ro->truncated) return pdegym::fail(-3, "null rollout buffer");
  if (int rc = check_terminal_slots(*buf, *ro, "traffic rollout")) return rc;
  const int A = buf->action_stride > 0 ? buf->action_stride : 2;
  if (A > 2) return pdegym::fail(-2, "action_stride must be 1 or 2");
  if (ro->policy && A > pdegym_policy::kWideOut) return pdegym::fail(-2, "policy: at most two commands");
  const pdegym_policy::Plan pl = pdegym_policy::plan(ro->policy, 2 * prm->M, A, B);
  if (pl.why) return pdegym::fail(-2, pl.why);
  const pdegym_mlp net = ro->policy ? *ro->policy : pdegym_mlp{};
  int rc = 0;
  pdegym_policy::dispatch(ro->policy, pl.wide, [&](auto wide_tag, auto policy_tag, auto gauss_tag) {
    constexpr bool W = decltype(wide_tag)::value, Pol = decltype(policy_tag)::value, G = decltype(gauss_tag)::value;
    if (!Pol || pdegym_policy::lds_limit_raised<&traffic_rollout_kernel<W, Pol, G>>("cannot raise the dynamic LDS limit of traffic_rollout_kernel", rc))
      hipLaunchKernelGGL((traffic_rollout_kernel<W, Pol, G>), pl.grid, pl.block, pl.lds_bytes, (hipStream_t)stream, *prm, *buf, *ro, net, traffic_consts(*prm), B);
  });
  return rc ? rc : pdegym::check_launch("traffic_rollout");
}

int pdegym_traffic_reset_masked(const pdegym_params_traffic* prm, const pdegym_bufs_traffic* buf, const double* profile,
                                const uint8_t* mask, int32_t B, void* stream) {
  if (int rc = check(prm, buf)) return rc;
  if (!profile) return pdegym::fail(-1, "null profile");
  if (B <= 0) return 0;
  const dim3 grid((B + kWavesPerBlock - 1) / kWavesPerBlock), block(kWave * kWavesPerBlock);
  hipLaunchKernelGGL(traffic_reset_kernel, grid, block, 0, (hipStream_t)stream, *prm, *buf, profile, mask, B);
  return pdegym::check_launch("traffic_reset");
}

}  // extern "C"
