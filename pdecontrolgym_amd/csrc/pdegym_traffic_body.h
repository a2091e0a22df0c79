// pdegym_traffic_body.h -- the device-side body shared by the traffic kernels (pdegym_traffic.hip) and the traffic backstepping
// kernels (pdegym_traffic_backstep.hip): the equilibrium law and the fluxes, the host-formed constants, the commands of a step, one
// env-step of one freeway by one wave (traffic_step_wave), the observation, the restart of a node and the fused auto-reset.  ONE copy:
// the one-launch law kernel is bit-identical to control launch + step launch because it runs these very functions.
// Design notes: at the top of pdegym_traffic.hip.
#ifndef PDEGYM_TRAFFIC_BODY_H
#define PDEGYM_TRAFFIC_BODY_H

#include <hip/hip_runtime.h>

#include <cstdio>

#include "pdegym.h"
#include "pdegym_common.h"

namespace {

using namespace pdegym::wave;      // kWave, kWavesPerBlock, wave_sum, pinned_from_left / _right, lane_value, wave_lds_sync, drain_vmem, pool_row

__device__ __forceinline__ double Veq(double vm, double rm, double rho) { return vm * (1 - rho / rm); }  // :270-272
__device__ __forceinline__ double F_r(double vm, double rm, double rho, double y) { return y + rho * Veq(vm, rm, rho); }
__device__ __forceinline__ double F_y(double vm, double rm, double rho, double y) { return y * (y / rho + Veq(vm, rm, rho)); }

// Scalar sub-expressions that Python evaluates before they meet an array (traffic_arz_env.py:201-222, :106): formed ONCE on the
// host in the same double arithmetic (IEEE division is correctly rounded on both sides, so the values are bit-identical to
// forming them per wave on the device -- which cost five float64 divisions, a third of the step kernel's instructions).
struct TrafficConsts {
  double c1, c2, c3, c4;   // dt/(2 dx), 0.25 dt/tau, dt/dx, 0.5 dt/tau
  double t_end;            // T/dt  (:106: seconds compared with a step count -- kept)
};
inline TrafficConsts traffic_consts(const pdegym_params_traffic& P) {
  TrafficConsts K;
  K.c1 = P.dt / (2 * P.dx);
  K.c2 = 0.25 * P.dt / P.tau;
  K.c3 = P.dt / P.dx;
  K.c4 = 0.5 * P.dt / P.tau;
  K.t_end = P.T / P.dt;
  return K;
}

// The commands of a step: action clip (:151-156) -- np.clip(a, low, high): min(max(a, low), high) for every a but NaN, which np.clip
// keeps (pdegym_common.h: clip_keep_nan) -- and which end each one drives
__device__ __forceinline__ void traffic_commands(const pdegym_params_traffic& P, double qc, double qs, double a0, double a1, double& q_in,
                                                 double& q_out) {
  const double lo = qc * 0.8, hi = 1.2 * qc;
  a0 = pdegym::clip_keep_nan(a0, lo, hi);
  a1 = pdegym::clip_keep_nan(a1, lo, hi);
  if (P.sim == PDEGYM_TRAFFIC_BOTH) { q_in = a0; q_out = a1; }
  else if (P.sim == PDEGYM_TRAFFIC_INLET) { q_in = a0; q_out = qs; }
  else { q_in = qs; q_out = a0; }
}

// The end of an env-step (whole wave): reward (traffic_arz_reward.py:22) from the wave sums sv = sum (v - vs)^2 and sr = sum (r - rs)^2,
// flags from "some node of this lane is over the limits" / "... has moved"; `time` returns to zero on termination.
struct TrafficEnd {
  double reward;
  bool done, trunc;
};
__device__ __forceinline__ TrafficEnd traffic_step_end(const pdegym_params_traffic& P, const TrafficConsts& K, double sv, double sr, bool over,
                                                       bool moved, double& time, double vs, double rs, int lane) {
  // ||v - vs|| / vs + ||r - rs|| / rs: the two square roots and the two divisions act on wave-uniform values, so they share ONE
  // float64 sqrt and ONE division sequence -- lane 0 takes the speed term, every other lane the density term (same operands, same
  // operations: the same bits as two scalar evaluations)
  const double term_ = sqrt(lane == 0 ? sv : sr) / (lane == 0 ? vs : rs);
  TrafficEnd e;
  e.reward = -(lane_value(term_, 0) + lane_value(term_, 1));
  const bool term = time >= K.t_end;               // :106 (seconds compared with a step count -- kept)
  if (term) time = 0.0;
  bool trunc = false;
  if (P.limit) trunc = __any(over);
  e.trunc = trunc || !__any(moved);                // exact steady state (:127-128)
  e.done = (P.sim == PDEGYM_TRAFFIC_OUTLET_TRAIN) ? term : (term || e.reward > -0.00023);
  return e;
}

// One env-step of one freeway held by one wave (M <= 64: node j in lane j): action clip, control_freq Lax-Wendroff sub-steps,
// speed, reward, flags.  Shared by traffic_step_kernel and every iteration of traffic_rollout_kernel.
struct TrafficStepOut : TrafficEnd {
  double v, vs;
};

__device__ __forceinline__ TrafficStepOut traffic_step_wave(const pdegym_params_traffic& P, const TrafficConsts& K, double& r, double& y,
                                                            double& time, const double rs, const double qc, double a0, double a1,
                                                            const int lane) {
  const int M = P.M;
  const bool in = lane < M;
  const double vm = P.vm, rm = P.rm;
  const double vs = Veq(vm, rm, rs);              // :66-72
  double q_in, q_out;
  traffic_commands(P, qc, rs * vs, a0, a1, q_in, q_out);

  time = time + P.dt;                             // :146
  const double c1 = K.c1, c2 = K.c2, c3 = K.c3, c4 = K.c4;
  if (time < P.T) {                               // :172  (time does not change inside the loop)
    for (int s = 0; s < P.control_freq; ++s) {
      // boundary conditions :174-190: the end nodes take their neighbour's density, then y = q - r Veq(r).  Round 5: that Veq(r)
      // IS the Veq(r) the nodal fluxes below evaluate for the same lane (same expression, same operand), so the density is set
      // first, Veq is formed ONCE for the whole wave and the two end lanes pick their y by select -- the round-4 form ran two more
      // float64 division sequences per sub-step under single-lane branches (a third of the loop's divisions).
      const double r1 = lane_value(r, 1), rm2 = lane_value(r, M - 2);
      const bool first = lane == 0, last = lane == M - 1;
      r = first ? r1 : (last ? rm2 : r);
      const double ve = Veq(vm, rm, r);
      const double yb = (first ? q_in : q_out) - r * ve;
      y = (first || last) ? yb : y;
      // nodal fluxes and the "plus" midpoint (:201-216); the neighbours' values arrive by pinned lane shifts (pdegym_common.h: the
      // inner update below runs on lanes 1 .. M-2 only, and the lane without a source reads 0, which no valid node ever uses)
      const double fr = y + r * ve, fy = y * (y / r + ve);      // F_r, F_y with the shared Veq(r)
      const double r_p = pinned_from_right(r), y_p = pinned_from_right(y), fr_p = pinned_from_right(fr), fy_p = pinned_from_right(fy);
      const double r_pm = 0.5 * (r_p + r) - c1 * (fr_p - fr);
      const double y_pm = (0.5 * (y_p + y) - c1 * (fy_p - fy)) - c2 * (y_p + y);
      const double Frp = F_r(vm, rm, r_pm, y_pm), Fyp = F_y(vm, rm, r_pm, y_pm);
      // the "minus" midpoint of node j is the "plus" midpoint of node j-1
      const double Frm = pinned_from_left(Frp), Fym = pinned_from_left(Fyp), y_mm = pinned_from_left(y_pm);
      if (lane >= 1 && lane <= M - 2) {           // inner update :219-223
        r = r - c3 * (Frp - Frm);
        y = y - (c3 * (Fyp - Fym) + c4 * (y_pm + y_mm));
      }
    }
  }
  TrafficStepOut o;
  o.vs = vs;
  o.v = y / r + Veq(vm, rm, r);                    // :227
  const double dv = in ? o.v - vs : 0.0, dr = in ? r - rs : 0.0;
  static_cast<TrafficEnd&>(o) = traffic_step_end(P, K, wave_sum(dv * dv), wave_sum(dr * dr), in && (o.v > vm || r > rm),
                                                 in && (dr != 0.0 || dv != 0.0), time, vs, rs, lane);
  return o;
}

// observation of node j of one freeway: (r, v), or ((r - rs)/rs, (v - vs)/vs) for outlet-train (:227-230)
__device__ __forceinline__ void traffic_emit_obs(const pdegym_params_traffic& P, double* o, double r, double v, double rs, double vs,
                                                 int j) {
  const int M = P.M;
  if (j < M) {
    if (P.sim == PDEGYM_TRAFFIC_OUTLET_TRAIN) {
      o[j] = (r - rs) / rs;
      o[M + j] = (v - vs) / vs;
    } else {
      o[j] = r;
      o[M + j] = v;
    }
  }
}

// TrafficPDE1D.reset of one node (traffic_arz_env.py:256-258):
//   r = rs*(sin(3x/L pi)*0.1 + 1) ; y = qs - vm r + vm/rm r^2 ; v = y/r + Veq(r)
__device__ __forceinline__ void traffic_restart_node(const pdegym_params_traffic& P, double rs, double prof, double& r, double& y,
                                                     double& v) {
  const double vs = Veq(P.vm, P.rm, rs), qs = rs * vs;
  r = rs * prof;
  y = (qs * 1.0 - P.vm * r) + (P.vm / P.rm) * (r * r);
  v = y / r + Veq(P.vm, P.rm, r);
}

// Where env-step t of a rollout keeps the final observation: bufs.final_obs itself, or slot t of it when it is [T, B, 2M]
// (PDEGYM_ROLLOUT_FINAL_OBS_PER_STEP).  Evaluated on the restart path only.
__device__ __forceinline__ double* traffic_terminal_slot(const pdegym_bufs_traffic& Bf, const pdegym_rollout_traffic& Ro, size_t slot, int t) {
  return (Ro.reserved_ & PDEGYM_ROLLOUT_FINAL_OBS_PER_STEP) ? Bf.final_obs + (size_t)t * slot : Bf.final_obs;
}

// The flag asks for something to keep and a restart to keep it at: 0, or the code to return (message in the error slot).
inline int check_terminal_slots(const pdegym_bufs_traffic& buf, const pdegym_rollout_traffic& ro, const char* who) {
  if (!(ro.reserved_ & PDEGYM_ROLLOUT_FINAL_OBS_PER_STEP)) return 0;
  auto fail = [who](int code, const char* msg) { return std::snprintf(pdegym::error_slot(), 512, "%s: %s", who, msg), code; };
  if (!buf.final_obs) return fail(-3, "PDEGYM_ROLLOUT_FINAL_OBS_PER_STEP needs bufs->final_obs [T, B, 2M]");
  if (!buf.reset_rs) return fail(-2, "PDEGYM_ROLLOUT_FINAL_OBS_PER_STEP needs the auto-reset pool (reset_rs): only a restart keeps a final observation");
  return 0;
}

// Fused auto-reset of a freeway held in registers (wave-uniform): the final observation, rs of the pool row of this restart
// (`extra`: restarts made inside the launch and not yet in reset_count), the nodes restarted with profile value `prof`, the
// observation of the restarted state into `obs`.  What goes back to memory besides is each kernel's own business.
// final_obs: the [B, 2M] array that keeps the final observation, or NULL -- bufs.final_obs, or the slot of this env-step of it
// (traffic_terminal_slot).
__device__ __forceinline__ void traffic_auto_reset(const pdegym_params_traffic& P, const pdegym_bufs_traffic& Bf, double* final_obs, int inst,
                                                   int B, int extra, double prof, double& r, double& y, double& rs, double v, double vs,
                                                   double* obs, int lane) {
  const int M = P.M;
  if (final_obs) traffic_emit_obs(P, final_obs + (size_t)inst * 2 * M, r, v, rs, vs, lane);
  rs = Bf.reset_rs[pool_row(Bf.reset_pool_rows, Bf.reset_count, inst, B, extra)];
  if (lane < M) {
    double v0;
    traffic_restart_node(P, rs, prof, r, y, v0);
    obs[lane] = r;
    obs[M + lane] = v0;
  }
}

}  // namespace
#endif
