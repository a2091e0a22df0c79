// pdegym_traffic_backstep.hip -- the backstepping baseline of the reference's traffic result table on the device (see include/pdegym.h):
//   pdegym_traffic_backstep_control   bcksController   examples/TrafficPDE1D/Backstepping control.ipynb, cell 5
//   pdegym_traffic_backstep_rollout   the loop of runSingleEpisode around it (same cell), T env-steps in ONE launch
// One wave per freeway.  The command is  q_out = (qs + rs Iv) + Iq  with  Iv = trapz(cv (v - vs), dx),  Iq = trapz(cq (r v - qs), dx):
// two weighted trapezoid sums over the observation row.  The weight rows cv, cq hold NumPy's exp and are formed on the host (as the
// reset profile holds NumPy's sin); the device forms the products, the trapezoid terms t_i = (dx (p[i+1] + p[i])) / 2.0 and their sum,
// in one of two orders (include/pdegym.h: PDEGYM_TRAFFIC_BACKSTEP_TREE / _NUMPY).  -ffp-contract=off keeps every operation apart.
// The rollout kernel is traffic_rollout_kernel (pdegym_traffic.hip) with the law in the policy's slot: step, fused auto-reset and
// observation are the shared functions of pdegym_traffic_body.h, the law is the function the control kernel runs (traffic_law_wave), so
// one launch is bit-identical to T x (control launch + step launch) because it performs the same operations.
// Output contracts (poisoned buffers, guard bands) of the kernels: tests/test_gpu_traffic_backstep.py, KERNEL_CASES there;
// tests/test_traffic_backstep.py fails when a kernel launched here is missing from that table.
#include <hip/hip_runtime.h>

#include <cmath>

#include "pdegym.h"
#include "pdegym_common.h"
#include "pdegym_traffic_body.h"

namespace {

// ---- the sum of the trapezoid terms ---------------------------------------------------------------------------------------------------
// np.trapz adds its terms with np.add.reduce, whose order for a contiguous float64 row of n <= 128 terms is: fewer than 8 terms, one
// chain from 0.0; otherwise eight accumulators a_k = t_k that take t_{k+8}, t_{k+16}, ... in ascending order over the first n - n % 8
// terms, combined as ((a0 + a1) + (a2 + a3)) + ((a4 + a5) + (a6 + a7)), then the last n % 8 terms one after the other.  (Longer rows
// halve recursively; the entry points refuse them in this order.)  get(i): term i, wave-uniform, i < n.  Result in every lane.
template <typename Get>
__device__ __forceinline__ double numpy_order_sum(int n, Get&& get) {
  if (n < 8) {
    double s = 0.0;
    for (int i = 0; i < n; ++i) s += get(i);
    return s;
  }
  double a[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) a[k] = get(k);
  const int n8 = n - (n & 7);
  for (int i = 8; i < n8; i += 8) {
#pragma unroll
    for (int k = 0; k < 8; ++k) a[k] += get(i + k);
  }
  double s = ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
  for (int i = n8; i < n; ++i) s += get(i);
  return s;
}

__device__ __forceinline__ double trapz_term(double dx, double p_next, double p) { return (dx * (p_next + p)) / 2.0; }

// The law on a freeway held in registers (M <= 64: node j in lane j, its weights cv, cq in the same lane; lanes >= M hold any finite
// filler, no term reads them): the products at the nodes, the neighbour's by a lane shift, term i in lane i, i < n = M - 1.
//   NUMPY   np.trapz's order (above), the terms handed round by v_readlane;
//   tree    the wave reduction of pdegym_common.h over the lanes' terms.
// Every lane must be active (the lane shift reads its right neighbour).  Result in every lane.
template <bool NUMPY>
__device__ __forceinline__ double traffic_law_wave(const pdegym_params_traffic& P, double r, double v, double cv, double cq, double rs,
                                                   double vs, double qs, int lane) {
  const int n = P.M - 1;
  const double pv = cv * (v - vs);
  const double q = r * v;
  const double pq = cq * (q - qs);
  const double tv = trapz_term(P.dx, pinned_from_right(pv), pv), tq = trapz_term(P.dx, pinned_from_right(pq), pq);
  double Iv, Iq;
  if constexpr (NUMPY) {
    Iv = numpy_order_sum(n, [&](int i) { return lane_value(tv, i); });
    Iq = numpy_order_sum(n, [&](int i) { return lane_value(tq, i); });
  } else {
    Iv = wave_sum(lane < n ? tv : 0.0);
    Iq = wave_sum(lane < n ? tq : 0.0);
  }
  return (qs + rs * Iv) + Iq;
}

// The law on a row of more than 64 nodes, read from memory (node j by lane j % 64; both nodes of a term by the lane that forms it).
//   NUMPY   n <= 128: lane l forms terms l and 64 + l, handed round as above;
//   tree    lane l adds terms l, l + 64, ... in ascending order from 0.0, then the wave reduction.
template <bool NUMPY>
__device__ __forceinline__ double traffic_law_strided(const pdegym_params_traffic& P, const double* o, const double* wv, const double* wq,
                                                      double rs, double vs, double qs, int lane) {
  const int M = P.M, n = M - 1;
  auto terms = [&](int i, double& tv, double& tq) {
    const double v0 = o[M + i], v1 = o[M + i + 1];
    const double pv0 = wv[i] * (v0 - vs), pv1 = wv[i + 1] * (v1 - vs);
    const double q0 = o[i] * v0, q1 = o[i + 1] * v1;
    const double pq0 = wq[i] * (q0 - qs), pq1 = wq[i + 1] * (q1 - qs);
    tv = trapz_term(P.dx, pv1, pv0);
    tq = trapz_term(P.dx, pq1, pq0);
  };
  double Iv, Iq;
  if constexpr (NUMPY) {
    double tv0 = 0.0, tq0 = 0.0, tv1 = 0.0, tq1 = 0.0;
    if (lane < n) terms(lane, tv0, tq0);
    if (kWave + lane < n) terms(kWave + lane, tv1, tq1);
    Iv = numpy_order_sum(n, [&](int i) { return i < kWave ? lane_value(tv0, i) : lane_value(tv1, i - kWave); });
    Iq = numpy_order_sum(n, [&](int i) { return i < kWave ? lane_value(tq0, i) : lane_value(tq1, i - kWave); });
  } else {
    double sv = 0.0, sq = 0.0;
    for (int i = lane; i < n; i += kWave) {
      double tv, tq;
      terms(i, tv, tq);
      sv += tv;
      sq += tq;
    }
    Iv = wave_sum(sv);
    Iq = wave_sum(sq);
  }
  return (qs + rs * Iv) + Iq;
}

// a command on its way out: + noise (float32, widened), clamp (np.clip: a NaN stays NaN)
__device__ __forceinline__ double law_finish(const pdegym_traffic_backstep& L, double c, bool has_noise, float nz) {
  if (has_noise) c = c + (double)nz;
  if (L.clamp) c = pdegym::clip_keep_nan(c, L.lo, L.hi);
  return c;
}

// ---- control law: out[b, :] = the command(s) for observation row obs[b, :] ------------------------------------------------------------
template <bool NUMPY>
__global__ __launch_bounds__(kWave* kWavesPerBlock) void traffic_backstep_control_kernel(pdegym_params_traffic P, pdegym_traffic_backstep L,
                                                                                         const double* __restrict__ obs, long long obs_stride,
                                                                                         const double* __restrict__ rs_in,
                                                                                         double* __restrict__ out, int out_stride, int B) {
  const int lane = threadIdx.x & (kWave - 1);
  const int inst = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
  if (inst >= B) return;      // wave-uniform
  const int M = P.M;
  const double rs = rs_in[inst];
  const double vs = Veq(P.vm, P.rm, rs);      // as traffic_step_wave forms them
  const double qs = rs * vs;
  double q_out = 0.0;
  if (P.sim != PDEGYM_TRAFFIC_INLET) {        // (the inlet law is the constant qs: no integral)
    const double* o = obs + (size_t)inst * obs_stride;
    const double* wv = L.weights_v + (size_t)inst * L.weight_stride;
    const double* wq = L.weights_q + (size_t)inst * L.weight_stride;
    if (M <= kWave) {
      const bool in = lane < M;
      const double r = in ? o[lane] : 1.0, v = in ? o[M + lane] : 0.0;
      const double cv = in ? wv[lane] : 0.0, cq = in ? wq[lane] : 0.0;
      q_out = traffic_law_wave<NUMPY>(P, r, v, cv, cq, rs, vs, qs, lane);
    } else {
      q_out = traffic_law_strided<NUMPY>(P, o, wv, wq, rs, vs, qs, lane);
    }
  }
  if (lane != 0) return;
  const float* nz = L.noise ? L.noise + (size_t)inst * L.noise_stride : nullptr;
  double* a = out + (size_t)inst * out_stride;
  a[0] = law_finish(L, P.sim == PDEGYM_TRAFFIC_OUTLET ? q_out : qs, nz != nullptr, nz ? nz[0] : 0.f);
  if (P.sim == PDEGYM_TRAFFIC_BOTH) a[1] = law_finish(L, q_out, nz != nullptr, nz ? nz[1] : 0.f);
}

// ---- T env-steps with the law inside, one launch (M <= 64) ----------------------------------------------------------------------------
// (r, y) and the law's input stay in registers across env-steps: the command of step 0 comes from observation slot 0 (what the control
// kernel would read), the command of step t >= 1 from r and the speed traffic_step_wave returned -- or, after a restart, the speed of
// the restarted nodes (traffic_restart_node's expression on the same operands): the very values observation slot t holds.  No memory
// round trip, no fence, no LDS.  Noise: 64 env-steps per load, lane l holding the draw(s) of step t0 + l (as the open-loop rollout
// holds its commands), so the loop's steady state waits for no load.
template <bool NUMPY>
__global__ __launch_bounds__(kWave* kWavesPerBlock) void traffic_backstep_rollout_kernel(pdegym_params_traffic P, pdegym_bufs_traffic Bf,
                                                                                         pdegym_rollout_traffic Ro, pdegym_traffic_backstep L,
                                                                                         TrafficConsts K, int B) {
  const int lane = threadIdx.x & (kWave - 1);
  const int inst = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
  if (inst >= B) return;      // wave-uniform
  const int M = P.M, D = 2 * M;
  const bool in = lane < M;
  const bool outlet = P.sim != PDEGYM_TRAFFIC_INLET;
  const int A = P.sim == PDEGYM_TRAFFIC_BOTH ? 2 : 1;
  double r = in ? Bf.r[(size_t)inst * M + lane] : 1.0;
  double y = in ? Bf.y[(size_t)inst * M + lane] : 0.0;
  double rs = Bf.rs[inst];
  const double qc = Bf.qs_clip[inst];
  double time = Bf.time[inst];
  int restarts = 0;
  const double prof = (Bf.reset_rs && in) ? Bf.reset_profile[lane] : 1.0;
  const double cv = (outlet && in) ? L.weights_v[(size_t)inst * L.weight_stride + lane] : 0.0;
  const double cq = (outlet && in) ? L.weights_q[(size_t)inst * L.weight_stride + lane] : 0.0;
  // the law's input: observation slot 0 now, the wave's own registers from step 1 on
  double lr = (outlet && in) ? Ro.obs[(size_t)inst * D + lane] : 1.0;
  double lv = (outlet && in) ? Ro.obs[(size_t)inst * D + M + lane] : 0.0;
  const size_t slot = (size_t)B * D;
  const bool has_noise = L.noise != nullptr;
  auto noise_batch = [&](int t0, int col) {
    return (has_noise && t0 + lane < Ro.T && col < A) ? L.noise[((size_t)(t0 + lane) * B + inst) * L.noise_stride + col] : 0.f;
  };
  float n0 = noise_batch(0, 0), n1 = noise_batch(0, 1);
  drain_vmem();      // wherever this kernel loads (here, at a batch hand-over, after a restart): nothing is pending at the loop's joins
  for (int t = 0; t < Ro.T; ++t) {
    const int tj = t & (kWave - 1);
    if (has_noise && tj == 0 && t) {      // wave-uniform, once per 64 env-steps
      n0 = noise_batch(t, 0);
      n1 = noise_batch(t, 1);
      drain_vmem();
    }
    const double vs_now = Veq(P.vm, P.rm, rs), qs_now = rs * vs_now;
    const double q_out = outlet ? traffic_law_wave<NUMPY>(P, lr, lv, cv, cq, rs, vs_now, qs_now, lane) : 0.0;
    const double a0 = law_finish(L, P.sim == PDEGYM_TRAFFIC_OUTLET ? q_out : qs_now, has_noise, lane_value(n0, tj));
    const double a1 = A > 1 ? law_finish(L, q_out, has_noise, lane_value(n1, tj)) : 0.0;
    if (lane == 0) {
      double* arow = Ro.actions + ((size_t)t * B + inst) * A;
      arow[0] = a0;
      if (A > 1) arow[1] = a1;
    }
    const TrafficStepOut o = traffic_step_wave(P, K, r, y, time, rs, qc, a0, a1, lane);
    double* onext = Ro.obs + (size_t)(t + 1) * slot + (size_t)inst * D;
    if (Bf.reset_rs && (o.done || o.trunc)) {     // wave-uniform
      traffic_auto_reset(P, Bf, traffic_terminal_slot(Bf, Ro, slot, t), inst, B, restarts, prof, r, y, rs, o.v, o.vs, onext, lane);
      ++restarts;
      time = 0.0;
      lv = y / r + Veq(P.vm, P.rm, r);            // traffic_restart_node's speed: what the slot just received
      drain_vmem();
    } else {
      traffic_emit_obs(P, onext, r, o.v, rs, o.vs, lane);
      lv = o.v;
    }
    lr = r;
    if (lane == 0) {
      Ro.rewards[(size_t)t * B + inst] = o.reward;
      Ro.done[(size_t)t * B + inst] = o.done ? 1 : 0;
      Ro.truncated[(size_t)t * B + inst] = o.trunc ? 1 : 0;
    }
  }
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

// what both entry points ask of the plant's parameters and of the law
int check_law(const pdegym_params_traffic* prm, const pdegym_traffic_backstep* law, int max_m, const char* too_long) {
  if (!prm || !law) return pdegym::fail(-1, "null params / law descriptor");
  if (prm->sim != PDEGYM_TRAFFIC_INLET && prm->sim != PDEGYM_TRAFFIC_OUTLET && prm->sim != PDEGYM_TRAFFIC_BOTH)
    return pdegym::fail(-2, "traffic backstepping: the law exists for 'inlet', 'outlet' and 'both' (the train types have no ps and a normalised observation)");
  if (prm->M < 4 || prm->M > max_m) return pdegym::fail(-2, too_long);
  if (law->order != PDEGYM_TRAFFIC_BACKSTEP_TREE && law->order != PDEGYM_TRAFFIC_BACKSTEP_NUMPY) return pdegym::fail(-2, "bad order");
  if (law->order == PDEGYM_TRAFFIC_BACKSTEP_NUMPY && prm->M > PDEGYM_TRAFFIC_BACKSTEP_NUMPY_MAX_M)
    return pdegym::fail(-2, "traffic backstepping: the numpy order covers rows of up to 129 nodes (longer rows: the tree order)");
  if (!std::isfinite(prm->dx) || !(prm->dx > 0.0)) return pdegym::fail(-2, "dx must be a positive finite number");
  if (prm->sim != PDEGYM_TRAFFIC_INLET) {
    if (!law->weights_v || !law->weights_q) return pdegym::fail(-3, "null weights_v / weights_q");
    if (law->weight_stride != 0 && law->weight_stride < prm->M) return pdegym::fail(-2, "weight_stride must be 0 (one shared row) or >= M");
  }
  const int ncmd = prm->sim == PDEGYM_TRAFFIC_BOTH ? 2 : 1;
  if (law->noise && law->noise_stride < ncmd) return pdegym::fail(-2, "noise_stride shorter than the commands of an instance");
  if (law->clamp && !(law->lo <= law->hi)) return pdegym::fail(-2, "clamp bounds must satisfy lo <= hi");
  return 0;
}

}  // namespace

extern "C" {

int pdegym_traffic_backstep_control(const pdegym_params_traffic* prm, const pdegym_traffic_backstep* law, const double* obs,
                                    int64_t obs_stride, const double* rs, double* out, int32_t out_stride, int32_t B, void* stream) {
  if (const int rc = check_law(prm, law, PDEGYM_TRAFFIC_MAX_M, "traffic backstepping: M must be in [4, 1024]")) return rc;
  if (B < 0) return pdegym::fail(-2, "B must be >= 0");
  if (!rs || !out) return pdegym::fail(-3, "null rs / out");
  const int ncmd = prm->sim == PDEGYM_TRAFFIC_BOTH ? 2 : 1;
  if (out_stride < ncmd) return pdegym::fail(-2, "out_stride shorter than the commands of an instance");
  if (prm->sim != PDEGYM_TRAFFIC_INLET) {
    if (!obs) return pdegym::fail(-3, "null obs");
    if (obs_stride < 2 * (int64_t)prm->M) return pdegym::fail(-2, "obs_stride shorter than a row of 2M");
  }
  if (B == 0) return 0;
  const dim3 grid((B + kWavesPerBlock - 1) / kWavesPerBlock), block(kWave * kWavesPerBlock);
  if (law->order == PDEGYM_TRAFFIC_BACKSTEP_NUMPY)
    traffic_backstep_control_kernel<true><<<grid, block, 0, (hipStream_t)stream>>>(*prm, *law, obs, obs_stride, rs, out, out_stride, B);
  else
    traffic_backstep_control_kernel<false><<<grid, block, 0, (hipStream_t)stream>>>(*prm, *law, obs, obs_stride, rs, out, out_stride, B);
  return pdegym::check_launch("traffic_backstep_control");
}

int pdegym_traffic_backstep_rollout(const pdegym_params_traffic* prm, const pdegym_bufs_traffic* buf, const pdegym_rollout_traffic* ro,
                                    const pdegym_traffic_backstep* law, int32_t B, void* stream) {
  if (!buf || !ro) return pdegym::fail(-1, "null bufs / rollout descriptor");
  if (const int rc = check_law(prm, law, kWave, "traffic backstepping rollout: freeways of 4 to 64 nodes (the register-resident kernel)"))
    return rc;
  if (B < 0) return pdegym::fail(-2, "B must be >= 0");
  if (ro->T < 1) return pdegym::fail(-2, "T must be >= 1");
  if (prm->control_freq < 1) return pdegym::fail(-2, "control_freq must be >= 1");
  if (ro->policy) return pdegym::fail(-2, "the law takes the policy's slot: ro->policy must be NULL");
  if (!buf->r || !buf->y || !buf->time || !buf->rs || !buf->qs_clip) return pdegym::fail(-3, "null device buffer");
  if (buf->reset_rs && !buf->reset_profile) return pdegym::fail(-3, "reset_rs needs reset_profile");
  if (buf->reset_pool_rows < 0) return pdegym::fail(-2, "reset_pool_rows must be >= 0");
  if (!ro->obs || !ro->actions || !ro->rewards || !ro->done || !ro->truncated) return pdegym::fail(-3, "null rollout buffer");
  if (int rc = check_terminal_slots(*buf, *ro, "traffic backstep rollout")) return rc;
  const int ncmd = prm->sim == PDEGYM_TRAFFIC_BOTH ? 2 : 1;
  if ((buf->action_stride > 0 ? buf->action_stride : 2) != ncmd)
    return pdegym::fail(-2, "action_stride must be the number of commands (1; 2 for 'both'): every column of actions is written");
  if (B == 0) return 0;
  const dim3 grid((B + kWavesPerBlock - 1) / kWavesPerBlock), block(kWave * kWavesPerBlock);
  if (law->order == PDEGYM_TRAFFIC_BACKSTEP_NUMPY)
    traffic_backstep_rollout_kernel<true><<<grid, block, 0, (hipStream_t)stream>>>(*prm, *buf, *ro, *law, traffic_consts(*prm), B);
  else
    traffic_backstep_rollout_kernel<false><<<grid, block, 0, (hipStream_t)stream>>>(*prm, *buf, *ro, *law, traffic_consts(*prm), B);
  return pdegym::check_launch("traffic_backstep_rollout");
}

}  // extern "C"
