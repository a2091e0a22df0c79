// pdegym_tumor_body.h -- the device code the brain-tumour units share (pdegym_tumor.hip: one day / a run of days per launch;
// pdegym_tumor_rollout.hip: TherapyWrapper steps and whole rollouts per launch): one interior node of the finite-difference update,
// the clip, the MRI radius as a ballot and the argument check for both units; and, for pdegym_tumor_rollout.hip, the staging of a row
// into the wave's LDS copy, ONE simulated day (update, stage machine, terminate / truncate, reward: brain_tumor_env.py:123-352) and
// the restart of one patient (:354-384) as functions.  tumor_stage_row and tumor_day restate, line by line, the text the day kernels
// of pdegym_tumor.hip keep inline (rewritten onto these functions their code object changes and the one-day launch runs 1.8 % slower:
// DESIGN.md section 4.10); the GPU tests of the rollout unit compare the two bit for bit.
#ifndef PDEGYM_TUMOR_BODY_H
#define PDEGYM_TUMOR_BODY_H

#include <hip/hip_runtime.h>

#include "pdegym.h"
#include "pdegym_common.h"

namespace pdegym_tumor {

using namespace pdegym::wave;      // kWave, kWavesPerBlock, wave_lds_sync
constexpr int kMaxNx = 4096;

// index of the highest lane set in a chunk's ballot (chunks are visited left to right, so a later hit wins)
__device__ __forceinline__ int rightmost(unsigned long long ballot, int chunk_base, int so_far) {
  return ballot ? chunk_base + 63 - __builtin_clzll(ballot) : so_far;
}

// brain_tumor_env.py:221-245, one interior node.
__device__ __forceinline__ double fd_node(const pdegym_params_tumor& P, double ul, double uc, double ur, double R, bool rad) {
  double lap = (ur - 2.0 * uc) + ul;
  if (P.dx2 != 1.0) lap = lap / P.dx2;                                 // x / 1.0 == x: skip the f64 division when dx = 1
  const double diffusion = P.D * lap;
  const double logistic = 1.0 - (uc / P.k);
  const double proliferation = (P.rho * uc) * logistic;
  double s = diffusion + proliferation;
  if (rad) s = s - (R * uc) * logistic;
  return uc + P.dt * s;
}

__device__ __forceinline__ double clip0k(double x, double k) { return pdegym::clip_keep_nan(x, 0.0, k); }      // np.clip(nextU, 0, k) :244

// The scalars of one patient (every lane of the wave carries the same values) and the outputs of one simulated day.
struct TumorState {
  int t, stage;
  int t2_idx;       // rightmost node of the live row at or above the T2 threshold (-1: none): the treated region of the NEXT day
  double remaining;
  int growth, therapyDays, post, sim, death;
};
struct TumorDay {
  double reward, T1, T2, treat_r, applied;
  bool term, lethal;
};

// ---- stage a row (global memory: the live row, or the initial row of a restart) in the wave's LDS copy; returns the T2 index of
// that row (:255 reads time_index-1)
// "rightmost node at or above a threshold" (:106-121) = highest set bit of a wave ballot, chunk of 64 nodes by chunk:
// scalar results without a shuffle reduction
__device__ __forceinline__ void tumor_stage_row(const pdegym_params_tumor& P, const double* g, double* cur, int lane, int& t2_idx) {
  const int nx = P.nx;
  t2_idx = -1;
  if (nx <= 4 * kWave) {       // rows of up to 256 nodes (the shipped 201): the four loads of a lane are issued together
    double v4[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int i = c * kWave + lane;
      v4[c] = i < nx ? g[i] : -1.0;
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int i = c * kWave + lane;
      if (i < nx) cur[i] = v4[c];
      if (c * kWave < nx) t2_idx = rightmost(__ballot(i < nx && v4[c] >= P.thr_t2), c * kWave, t2_idx);
    }
  } else {
    for (int i0 = 0; i0 < nx; i0 += kWave) {
      const int i = i0 + lane;
      double v = -1.0;
      if (i < nx) {
        v = g[i];
        cur[i] = v;
      }
      t2_idx = rightmost(__ballot(i < nx && v >= P.thr_t2), i0, t2_idx);
    }
  }
}

// ---- one simulated day of one patient: the row in `cur` (LDS, visible to the wave after the wave_lds_sync this begins with) is
// advanced into `nxt` -- TO_GLOBAL: straight into the patient's global row g instead -- and the two pointers change places.
// host_kill with a kill_arr: the kill fraction of a Therapy day is kill_arr[inst] (the caller's libm value), otherwise exp is evaluated here.
// hist / t1log: the patient's trajectory rows or nullptr.
template <bool TO_GLOBAL>
__device__ __forceinline__ void tumor_day(const pdegym_params_tumor& P, const double* xscale, TumorState& S, TumorDay& O, double control,
                                          bool host_kill, const double* kill_arr, int inst, double*& cur, double*& nxt, double* g,
                                          double* hist, double* t1log, double tb, bool has_tb, int lane) {
  const int nx = P.nx;
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  wave_lds_sync();                                                   // the row written by the previous day is visible
  S.t += 1;
  const int t = S.t;
  const int stage0 = S.stage;
  const bool therapy = stage0 == PDEGYM_TUMOR_THERAPY;
  O.applied = 0.0;
  O.treat_r = 0.0;
  double kill = 0.0;
  if (therapy) {                                                     // :158-168, :247-263
    const double want = control * P.total_dosage;
    O.applied = S.remaining < want ? S.remaining : want;             // Python min(want, remaining)
    S.remaining = S.remaining - O.applied;
    O.treat_r = S.t2_idx < 0 ? 0.0 : (double)S.t2_idx * P.dx + P.margin;
    if (host_kill && kill_arr) {
      kill = kill_arr[inst];
    } else {
      const double bed = O.applied + ((O.applied * O.applied) / P.alpha_beta_ratio);
      kill = 1.0 - exp(-P.alpha * bed);
    }
  }
  // ---- finite-difference update, Neumann ends, clip to [0, k]; T1/T2 radii of the new row
  int t1_idx = -1, t2n_idx = -1;
  double* hrow = hist ? hist + (size_t)t * nx : nullptr;
  // four chunks of 64 nodes per trip, fully unrolled: their LDS reads and f64 division chains are independent, so one
  // wave overlaps them (a lone wave issues an instruction only every ~6.5 cycles; the day loop is latency-bound)
  for (int ib = 0; ib < nx; ib += 4 * kWave) {
    double vv[4];
    bool inn[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int i = ib + q * kWave + lane;
      inn[q] = i < nx;
      vv[q] = -1.0;
      if (inn[q]) {
        const int c = i == 0 ? 1 : (i == nx - 1 ? nx - 2 : i);       // :241-242 copy the neighbour's new value
        const bool rad = therapy && xscale[c] <= O.treat_r;          // outside: BED = 0 -> R = 1 - exp(-0) = 0
        vv[q] = clip0k(fd_node(P, cur[c - 1], cur[c], cur[c + 1], kill, rad), P.k);
      }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int i0 = ib + q * kWave, i = i0 + lane;
      if (inn[q]) {
        if constexpr (TO_GLOBAL) g[i] = vv[q];      // the only day of this launch: straight to global memory
        else nxt[i] = vv[q];
        if (hrow) hrow[i] = vv[q];
      }
      t1_idx = rightmost(__ballot(inn[q] && vv[q] >= P.thr_t1), i0, t1_idx);
      t2n_idx = rightmost(__ballot(inn[q] && vv[q] >= P.thr_t2), i0, t2n_idx);
    }
  }
  S.t2_idx = t2n_idx;
  {
    double* sw = cur;
    cur = nxt;
    nxt = sw;
  }
  // ---- stage machine :146-177, terminate/truncate :280-352, reward (every lane carries the same scalars)
  O.T1 = t1_idx < 0 ? nan : (double)t1_idx * P.dx;
  O.T2 = t2n_idx < 0 ? nan : (double)t2n_idx * P.dx;
  if (t1log && lane == 0) t1log[t] = t1_idx < 0 ? nan : O.T1 / P.dx;   // _log_radii :271-273
  if (stage0 == PDEGYM_TUMOR_GROWTH) {
    S.growth = t;
    if (t1_idx >= 0 && O.T1 >= P.detect_radius) S.stage = PDEGYM_TUMOR_THERAPY;
  } else if (therapy && S.remaining < P.dose_end) {
    S.therapyDays = t - S.growth;
    S.stage = PDEGYM_TUMOR_POST;
  }
  O.term = t >= P.nt - 1;
  O.lethal = t1_idx >= 0 && O.T1 >= P.death_radius;
  if (O.term || (O.lethal && S.death < 0)) {
    if (S.stage == PDEGYM_TUMOR_THERAPY) {
      S.therapyDays = t - S.growth;
      S.sim = S.growth + S.therapyDays;
    } else if (S.stage == PDEGYM_TUMOR_POST) {
      S.post = t - S.therapyDays - S.growth;
      S.sim = S.growth + S.therapyDays + S.post;
    }
  }
  if (O.lethal && S.death < 0) S.death = t;
  O.reward = 0.0;
  if (therapy) {
    if (!has_tb) O.reward = 0.0;
    else if (O.term || O.lethal) O.reward = (double)t - tb;
    else {                                                           // brain_tumor_reward.py:59-73
      const double maxsafe = 116.0 * pow(O.treat_r, -0.685);
      const double ratio = (O.applied - maxsafe) / (P.total_dosage - maxsafe);
      const double r = pdegym::clip_keep_nan(ratio, 0.0, 1.0);      // Python min(max(ratio, 0.0), 1.0): NaN for a NaN ratio
      O.reward = -50.0 * pow(r, 1.0 / 3.0);
    }
  } else if (S.stage == PDEGYM_TUMOR_POST && (O.term || O.lethal)) {
    O.reward = has_tb ? (double)t - tb : 0.0;
  }
}

// ---- the scalars of a restarted patient (the state part of BrainTumor1D.reset :354-384); the row is the caller's copy
__device__ __forceinline__ void tumor_reset_scalars(const pdegym_params_tumor& P, TumorState& S) {
  S.t = 0;
  S.stage = PDEGYM_TUMOR_GROWTH;
  S.remaining = P.total_dosage;
  S.growth = S.therapyDays = S.post = S.sim = 0;
  S.death = -1;
}

// the scalars of one patient, from / to the engine's arrays (lane-independent: scalar loads; the stores are the caller's lane 0)
__device__ __forceinline__ void tumor_store_scalars(const pdegym_bufs_tumor& Bf, int inst, const TumorState& S) {
  Bf.time_index[inst] = S.t;
  Bf.stage[inst] = S.stage;
  Bf.remaining[inst] = S.remaining;
  int32_t* days = Bf.days + (size_t)inst * PDEGYM_TUMOR_DAYS;
  days[PDEGYM_TUMOR_DAY_GROWTH] = S.growth;
  days[PDEGYM_TUMOR_DAY_THERAPY] = S.therapyDays;
  days[PDEGYM_TUMOR_DAY_POST] = S.post;
  days[PDEGYM_TUMOR_DAY_SIM] = S.sim;
  days[PDEGYM_TUMOR_DAY_DEATH] = S.death;
}

// null / range checks of the parameter block and the state arrays every entry point of the family needs
inline int check(const pdegym_params_tumor* prm, const pdegym_bufs_tumor* buf) {
  if (!prm || !buf) return pdegym::fail(-1, "null params/bufs");
  if (prm->nx < 3 || prm->nx > kMaxNx) return pdegym::fail(-2, "tumor: nx must be in [3, 4096]");
  if (prm->nt < 2) return pdegym::fail(-2, "tumor: nt must be >= 2");
  if (!buf->u || !buf->time_index || !buf->stage || !buf->remaining || !buf->days)
    return pdegym::fail(-3, "null device buffer");
  return 0;
}

}  // namespace pdegym_tumor
#endif
