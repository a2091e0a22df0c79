// pdegym_1d_body.h -- the device-side body shared by the 1D step kernels (pdegym_1d.hip) and the 1D rollout kernels
// (pdegym_1d_rollout.hip): the magnitude maxima on the wave reduction of pdegym_common.h, the sub-step loops, one env-step of one instance by one wave
// (step1d_body) and the state a rollout carries in registers.  Two translation units so that they compile in parallel and so
// that a change of the rollout kernels leaves the fingerprint of the step kernels (and the counters committed for them) alone.
// Design notes: at the top of pdegym_1d.hip.
#ifndef PDEGYM_1D_BODY_H
#define PDEGYM_1D_BODY_H

#include <hip/hip_runtime.h>

#include <type_traits>

#include "pdegym.h"
#include "pdegym_common.h"

// Hook of the launch-head diagnostic (tools/head_stamps.py builds pdegym_1d.hip with PDEGYM_HEAD_STAMPS into a library of its own,
// never the shipped one): empty in every other build, so no stamp executes in a product kernel.
#ifndef PDEGYM_HEAD_STAMP
#define PDEGYM_HEAD_STAMP(k)
#endif

namespace {

using namespace pdegym::wave;      // kWave, kWavesPerBlock, lane shifts, wave_reduce / wave_sum, lane_value, drain_vmem, pool_row

// max of two magnitudes (sign bit clear) that propagates NaN like np.max: non-negative floats order as their bit patterns,
// and every NaN pattern lies above +inf.  The Linf reward norms use it (np.linalg.norm(row, ord=inf) of a row holding NaN is NaN).
__device__ __forceinline__ float mag_max(float a, float b) {
  const unsigned int ua = __float_as_uint(a), ub = __float_as_uint(b);
  return __uint_as_float(ua > ub ? ua : ub);
}
// (The overflow pre-check of step1d_body / carry_refresh_beta uses it too -- one v_max_u32 with a DPP operand per stage: a NaN that comes
// through makes the pre-check's comparison fail, and the wave takes the exact loop.)
__device__ __forceinline__ float wave_mag_max(float v) {
  return wave_reduce(v, [](float a, float b) { return mag_max(a, b); });
}

// value of slot s when lane l holds slots [l*EPL, l*EPL+EPL)
template <int EPL>
__device__ __forceinline__ float slot_get(const float (&x)[EPL], int s) {
  const int src = s / EPL, e = s - src * EPL;
  float sel = x[0];
#pragma unroll
  for (int k = 1; k < EPL; ++k) sel = (e == k) ? x[k] : sel;
  return __shfl(sel, src);
}

template <int EPL>
__device__ __forceinline__ float slots_sumsq(const float (&x)[EPL], int s0, int ns) {
  float s = 0.f;
#pragma unroll
  for (int e = 0; e < EPL; ++e) s += (s0 + e < ns) ? x[e] * x[e] : 0.f;
  return wave_sum(s);
}

// (a+1)*m-m, base_env_1d.py:36-39
__device__ __forceinline__ float normalize_ctrl(float a, float m, int on) { return on ? (a + 1.0f) * m - m : a; }

// The norm ring of one instance (PDEGYM_RING slots, slot = fine time index mod PDEGYM_RING) as the step body sees it.
// RingMem: the ring in memory, written and read by lane 0 alone (program order of one lane).
// RingReg (the carried rollout kernels, round 5): the 128 slots live in TWO registers per lane for the whole launch (lane l holds
// slots l and 64 + l) -- a rollout step neither loads from nor stores to the ring, so nothing in its steady state waits on vmcnt
// (gfx9 counts loads AND stores in vmcnt: the one ring load per env-step made every step wait for the 13 stores of the step before;
// SQ_WAIT_ANY was 57 % of the wave cycles of parabolic_c2_s1_open_loop_rollout, profiles/r04p_summary.json).  The memory ring is
// read once at the head of the launch and written back once at its end (rollout1d_kernel).  Values are wave-uniform.
struct RingMem {
  float* mem;
  __device__ __forceinline__ void put(int idx, float v, int lane) {
    if (lane == 0) mem[idx] = v;
  }
  __device__ __forceinline__ float get(int idx, int lane) const { return lane == 0 ? mem[idx] : 0.f; }   // lane 0's value
};
struct RingReg {
  float lo, hi;
  __device__ __forceinline__ void put(int idx, float v, int lane) {
    lo = (lane == idx) ? v : lo;
    hi = (lane + kWave == idx) ? v : hi;
  }
  __device__ __forceinline__ float get(int idx, int) const {
    const float src = (idx & kWave) ? hi : lo;
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, src), idx & (kWave - 1)));
  }
};
static_assert(PDEGYM_RING == 2 * kWave, "RingReg keeps the ring in two registers per lane");

// EPL consecutive floats of one lane from / to a row (`base` = the row's first slot: 4-byte aligned, rows of 257 floats are not
// 16-byte aligned): a lane whose slots are all inside the row moves them as dwordx4 / x2 pieces (gfx950 global accesses need no
// alignment beyond the dword; the type says so to the compiler), the row's last lanes fall back to guarded dwords.
typedef float pdegym_f4u __attribute__((ext_vector_type(4), aligned(4)));
typedef float pdegym_f2u __attribute__((ext_vector_type(2), aligned(4)));
template <int EPL>
__device__ __forceinline__ void store_slots(float* base, const float (&x)[EPL], int s0, int ns) {
  if (s0 + EPL <= ns) {
    float* p = base + s0;
    constexpr int Q = EPL / 4 * 4, D = (EPL - Q) / 2 * 2;
#pragma unroll
    for (int e = 0; e < Q; e += 4) *reinterpret_cast<pdegym_f4u*>(p + e) = pdegym_f4u{x[e], x[e + 1], x[e + 2], x[e + 3]};
    if constexpr (D == 2) *reinterpret_cast<pdegym_f2u*>(p + Q) = pdegym_f2u{x[Q], x[Q + 1]};
    if constexpr (Q + D < EPL) p[EPL - 1] = x[EPL - 1];
  } else {
#pragma unroll
    for (int e = 0; e < EPL; ++e)
      if (s0 + e < ns) base[s0 + e] = x[e];
  }
}
// The row store of a lane with FOUR slots as write-through (sc1): one dwordx4 per lane, so one instruction of the wave covers 1 KB
// without gaps and every line it touches leaves the XCD's L2 once, as the store is issued, where a plain store leaves the line dirty
// until the release at the end of the kernel writes all of them back at once (4.4 MB at B = 4096, nx = 256).  Only this layout: with
// more slots per lane each dwordx4 of the wave covers 16 of every 32 (or more) bytes and every line goes out several times as a
// masked write (EPL = 8 measured: WRITE_SIZE of transport_c3 35.2 -> 68.9 MB per step for no gain, profiles/r07_ab_notes.txt), and
// narrower write-through stores are a fabric write each.  `row` = the row's node 0, the slots start J0 floats in: the byte offset is
// the instruction's immediate, as in the compiler's own stores.  The compiler does not look inside the statement: the dwordx4 store
// ends with the two wait states that must separate it from a write of its data registers, and its vmcnt is not in the compiler's
// books -- which only makes the waits the compiler inserts stricter (the counter is in order); drain_vmem() waits for these stores
// like for any other.  The guarded dwords of a lane that straddles the row's end stay plain stores.
typedef float pdegym_f4 __attribute__((ext_vector_type(4)));
template <int BYTES>
__device__ __forceinline__ void store_wt(float* p, pdegym_f4 v) {
  asm volatile("global_store_dwordx4 %0, %1, off offset:%2 sc1\n\ts_nop 1" : : "v"(p), "v"(v), "n"(BYTES) : "memory");
}
template <int BYTES>
__device__ __forceinline__ void store_wt(float* p, float v) {      // (node 0 of a parabolic row: one lane)
  asm volatile("global_store_dword %0, %1, off offset:%2 sc1" : : "v"(p), "v"(v), "n"(BYTES) : "memory");
}
template <int J0>
__device__ __forceinline__ void store_slots_wt(float* row, const float (&x)[4], int s0, int ns) {
  if (s0 + 4 <= ns) {
    store_wt<4 * J0>(row + s0, pdegym_f4{x[0], x[1], x[2], x[3]});
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (s0 + e < ns) row[J0 + s0 + e] = x[e];
  }
}
template <int EPL>
__device__ __forceinline__ void load_slots(const float* base, float (&x)[EPL], int s0, int ns) {
  if (s0 + EPL <= ns) {
    const float* p = base + s0;
    constexpr int Q = EPL / 4 * 4, D = (EPL - Q) / 2 * 2;
#pragma unroll
    for (int e = 0; e < Q; e += 4) {
      const pdegym_f4u v = *reinterpret_cast<const pdegym_f4u*>(p + e);
      x[e] = v.x; x[e + 1] = v.y; x[e + 2] = v.z; x[e + 3] = v.w;
    }
    if constexpr (D == 2) {
      const pdegym_f2u v = *reinterpret_cast<const pdegym_f2u*>(p + Q);
      x[Q] = v.x; x[Q + 1] = v.y;
    }
    if constexpr (Q + D < EPL) x[EPL - 1] = p[EPL - 1];
  } else {
#pragma unroll
    for (int e = 0; e < EPL; ++e) x[e] = (s0 + e < ns) ? base[s0 + e] : 0.f;
  }
}

// normalize(control_update(control, neighbour, dx), max_control_value) as NumPy evaluates it for the given kind of `control`
// (hyperbolic.py:143-145, parabolic.py:148-150, base_env_1d.py:36-39); the result is what lands in the float32 row.
template <bool M64>
__device__ __forceinline__ float boundary_value(const pdegym_params1d& P, float a32, double a64, float neighbour, bool neumann) {
  if (!M64 || P.action_kind == PDEGYM_ACTION_F32) {
    const float v = neumann ? a32 * P.dx + neighbour : a32;
    return normalize_ctrl(v, P.max_control, P.normalize);
  }
  if (P.action_kind == PDEGYM_ACTION_F64 || !neumann) {
    double v = neumann ? a64 * P.dx64 + (double)neighbour : a64;
    if (P.normalize) v = (v + 1.0) * P.max_control64 - P.max_control64;
    return (float)v;
  }
  // NEP 50 weak Python scalar: control*dx is a Python float product, then adopts the float32 of the neighbour
  const float v = (float)(a64 * P.dx64) + neighbour;
  return normalize_ctrl(v, P.max_control, P.normalize);
}

// Per-wave state of one instance while it is stepped.
template <int EPL>
struct Row {
  float x[EPL];   // slots (row nodes J0 .. n-1)
  float bl;       // parabolic: node 0 (u(0,t)); unused for transport
  int t;          // time_index
  int k;          // (t + LOOKBACK) mod S
  double bsum;    // running sum of |u[tau,-1]|
  int back_row;   // row index the reward of THIS call looks back at (t_end - 100), if it is produced in this call
  float back_norm;  // its norm, captured in the loop (lane-uniform)
};

// State of one instance kept in registers ACROSS the env-steps of a rollout launch (rollout1d_kernel): the row, its plant
// parameter, the time index, the running |u[-1]| sum and the wave maximum of |dt*beta| (constant between resets).
template <int EPL>
struct Carry {
  float x[EPL];
  float beta[EPL];
  float bl;
  float cm;       // wave_max |dt * beta[j]| (the fast-loop overflow pre-check)
  float norm;     // ||row||_2 as the previous step (or the prologue) computed it: an upper bound of max |row[j]|
  int t;
  int k;          // (t + LOOKBACK) mod S, advanced with t (no division per env-step)
  double bsum;
  RingReg ring;   // the instance's norm ring, register-resident for the launch
  float glog;     // log2 of the growth bound g(cm): constant between resets (follows beta)
};

// growth bound of one parabolic sub-step (see the overflow pre-check in step1d_body)
__device__ __forceinline__ float growth_bound(const pdegym_params1d& P, float cm) {
  return ((P.F >= 0.0f && P.F <= 0.5f) ? 1.0f : 1.0f + 4.0f * fabsf(P.F)) + cm + 9.5367431640625e-7f;
}
// what follows a (re)draw of the carried beta: wave maximum of |dt*beta| and log2 of the growth bound.  (Carrying the fast loop's
// coefficients as well saved ~12 instructions per env-step of the open-loop kernel and cost 8 registers: the policy kernels -- 16 waves
// per workgroup, 128 registers per lane -- spilled 78 of them; with FULL rows the coefficients are four multiplications and one select.)
template <int EPL, bool PARABOLIC>
__device__ __forceinline__ void carry_refresh_beta(Carry<EPL>& C, const pdegym_params1d& P, int s0, int ns) {
  float cm = 0.f;
#pragma unroll
  for (int e = 0; e < EPL; ++e) cm = fmaxf(cm, fabsf(P.dt * C.beta[e]));
  C.cm = wave_mag_max(cm);
  C.glog = __log2f(growth_bound(P, C.cm));
  (void)s0;
  (void)ns;
}

// ---- step bookkeeping: the pieces around the sub-step loop that step1d_body (rows in registers) and step1d_wide_kernel (pdegym_1d.hip:
// rows in LDS) both call.  Only pieces whose call leaves every register-resident kernel's instructions as they were; the look-back
// plan, the reward selection, the NormReward norms and the beta redraw stay written out in both (docs/HISTORY.md, section 3).
// rows whose norm a later reward call looks back at (tuned_reward_1d.py:40): r+100 is a step end
__device__ __forceinline__ bool ring_records(const pdegym_params1d& P, int k, int t) {
  return P.nt <= PDEGYM_RING || k == 0 || t + PDEGYM_LOOKBACK == P.nt - 1;
}
// NormReward "t-horizon" (norm_reward.py:60-73): the length that applies (0: another reward)
__device__ __forceinline__ int thor_length(const pdegym_params1d& P) {
  return (P.reward_horizon == PDEGYM_HORIZON_T && P.reward_kind >= PDEGYM_REWARD_NORM_L1) ? P.reward_t_horizon : 0;
}
__device__ __forceinline__ bool step_terminates(const pdegym_params1d& P, int t) { return t >= P.nt - 1; }   // hyperbolic.py:171-180
__device__ __forceinline__ bool step_truncates(const pdegym_params1d& P, float norm_now) {                   // hyperbolic.py:182-194
  return P.limit_state && (norm_now >= P.max_state);
}
// The scalar observation of sensing_update (hyperbolic.py:72-116) from a node accessor: node(j) = u[j] of the row's n nodes
// (the memory-resident forms: step1d_wide_kernel, reset1d_kernel; step1d_body's, whose accessor shuffles, is written out there).
template <typename NodeF>
__device__ __forceinline__ float sensed_value(const pdegym_params1d& P, int n, NodeF&& node) {
  if (P.sensing == PDEGYM_SENSE_LAST) return node(n - 1);
  if (P.sensing == PDEGYM_SENSE_LAST_DERIV) return (node(n - 1) - node(n - 2)) / P.dx;
  if (P.sensing == PDEGYM_SENSE_FIRST_DERIV) return (node(1) - node(0)) / P.dx;
  return node(0);
}
// What lane 0 stores of every step: reward, flags, and (store_state: not overwritten by a later step of the same launch) the norms.
__device__ __forceinline__ void store_step_words(const pdegym_params1d& P, const pdegym_bufs1d& Bf, int inst, int lane, float reward,
                                                 float norm_now, float norm_back, bool terminate, bool truncate, bool store_state) {
  if (lane == 0) {
    if (P.reward_kind != PDEGYM_REWARD_NONE) Bf.reward[inst] = reward;
    if (store_state) {
      Bf.norm_now[inst] = norm_now;
      Bf.norm_back[inst] = norm_back;
    }
    Bf.terminated[inst] = terminate ? 1 : 0;
    Bf.truncated[inst] = truncate ? 1 : 0;
  }
}
// Fused auto-reset: the trajectory restarts -- history = zeros((nt, n)); history[0] = the pool row (hyperbolic.py:214-217)
__device__ __forceinline__ void wipe_history(float* hist, const float* irow, int nt, int n, int lane) {
  for (size_t q = lane; q < (size_t)nt * n; q += kWave) hist[q] = (q < (size_t)n) ? irow[q] : 0.f;
}

// The reward's own norm of a register-resident row (NormReward kinds; same expressions as the epilogue of step1d_body), for the
// "t-horizon" reward: -(mean of the norms of the last k fine-time rows), norm_reward.py:60-73.
template <int EPL>
__device__ __forceinline__ float kind_norm(const float (&x)[EPL], float bl, int s0, int ns, int kind) {
  if (kind == PDEGYM_REWARD_NORM_L1) {
    float s1 = 0.f;
#pragma unroll
    for (int e = 0; e < EPL; ++e) s1 += (s0 + e < ns) ? fabsf(x[e]) : 0.f;
    return wave_sum(s1) + fabsf(bl);
  }
  if (kind == PDEGYM_REWARD_NORM_LINF) {
    float m = fabsf(bl);
#pragma unroll
    for (int e = 0; e < EPL; ++e) m = mag_max(m, (s0 + e < ns) ? fabsf(x[e]) : 0.f);
    return wave_mag_max(m);
  }
  return sqrtf(slots_sumsq<EPL>(x, s0, ns) + bl * bl);
}

// S sub-steps of one instance.  FAST: boundary/padding slots are frozen by zero coefficients (no selects);
// otherwise explicit selects (exact for non-finite states, and required when the boundary value changes every
// sub-step, i.e. parabolic Neumann control).
// M64: float64 beta and/or float64 / Python-float control (pdegym_params1d.beta_f64 / action_kind): the select form with the
// reference's mixed-precision expressions (see step1d_wide_kernel for the same arithmetic on LDS-resident rows).
// FOLD (step1d_kernel<HeadArgsFold, 4, true, false, true> only, the headline shape): when the caller says fold_ok -- F = 2^-k, 1 <= k <= 24,
// more than one sub-step -- the sub-steps behind the peeled first one form t5 = fma(F, t3, x) instead of x + RN(F * t3): F * t3 is exact
// unless it underflows, and then the two agree bit for bit.  The guard (tests/test_fold_lemma.py): a slot can differ only
// where |x| < 2^-100 AND a neighbour is below 2^-78; of two adjacent slots one is even, so a row whose EVEN slots (e = 0 and 2 of every
// lane; the frozen boundary slot 255 and node 0 are odd / outside) all hold |x| >= 2^-78 is folded exactly.  One v_min3_f32 per sub-step
// keeps the running minimum of the even slots' magnitudes of every row a fold sub-step reads, against the floor 2^-64.  A row below the
// floor after the peeled sub-step (zeros, compact support, denormals) never enters the fold loop; one that sinks below it later makes
// the caller run the whole call again in the plain form (*fold_redo).  NaN compares as not-below in v_min3_f32 and is left to the
// caller's non-finite test, like today.
constexpr float kFoldFloor = 5.421010862427522e-20f;      // 2^-64
template <int EPL, bool PARABOLIC, bool NEUMANN, bool FAST, bool HIST, bool BURGERS = false, bool M64 = false, bool ROLL = false,
          typename RingT = RingMem, bool FULL = false, bool FOLD = false>
__device__ __forceinline__ void run_substeps(Row<EPL>& R, const float (&beta)[EPL], const pdegym_params1d& P, int nsub,
                                             float a, RingT& ring, float* hist, int lane, const double* b64 = nullptr, double a64 = 0.0,
                                             float* xprev = nullptr, float* blprev = nullptr, int thor_k = 0, bool fold_ok = false,
                                             bool* fold_redo = nullptr) {
  static_assert(!FOLD || (FAST && PARABOLIC && FULL && !HIST && !ROLL && EPL == 4), "the fold is the headline instantiation's");
  // xprev/blprev (select form only): the row BEFORE the last sub-step, for NormReward's "differential" horizon
  // thor_k (select form only): NormReward "t-horizon" of length thor_k -- the reward's norm of each of the last thor_k - 1 rows
  // before the final one goes into the ring (the final row's is the epilogue's)
  // FAST && HIST (round 6): the fast arithmetic with one row store per sub-step into the trajectory -- the single environments'
  // default configuration (record_history: env.u is the whole trajectory, as in the reference)
  static_assert(!(FAST && NEUMANN), "fast mode is the Dirichlet path");
  static_assert(!(FAST && M64), "the mixed-precision mode uses the select form");
  constexpr int J0 = PARABOLIC ? 1 : 0;
  // FULL (round 5): the row fills the wave exactly (n - J0 == 64 EPL, checked by the launcher) -- with the slot count a compile-time
  // constant every "is this slot inside the row" select folds away and "is this the boundary slot" becomes lane 63's last slot
  const int n = FULL ? kWave * EPL + J0 : P.n, ns = n - J0, s0 = lane * EPL;
  const float dx = P.dx, dt = P.dt, F = P.F;
  const int S = P.substeps > 0 ? P.substeps : 1;
  const bool rec_all = P.nt <= PDEGYM_RING;
  // control_update (hyperbolic.py:68,95). Transport/Neumann reads u[t][-2] of the NEW row, which is still zero
  // (hyperbolic.py:144), so its boundary value is constant over the sub-steps.
  const float cdx = a * dx;
  const float rdxf = 1.0f / dx;   // exact when dx is a power of two (the only case it is used in)
  const bool pow2_dx = !PARABOLIC && dx > 0.0f && (__float_as_uint(dx) & 0x7fffffu) == 0u && rdxf * dx == 1.0f &&
                       rdxf < 3.0e38f;
  float bval = M64 ? boundary_value<true>(P, a, a64, 0.0f, NEUMANN)
                   : (NEUMANN ? normalize_ctrl(cdx + 0.0f, P.max_control, P.normalize) : normalize_ctrl(a, P.max_control, P.normalize));
  const bool beta64 = M64 && P.beta_f64;
  double c64[M64 ? EPL : 1];        // parabolic: dt*beta in double (parabolic.py:144 forms dt*beta first); transport: beta
  if constexpr (M64) {
#pragma unroll
    for (int e = 0; e < EPL; ++e) c64[e] = beta64 ? (PARABOLIC ? P.dt64 * b64[e] : b64[e]) : 0.0;
  }

  // per-slot coefficients: parabolic c = dt*beta (parabolic.py:144 forms dt*beta first), transport c = beta
  float c[EPL], fe[EPL];
#pragma unroll
  for (int e = 0; e < EPL; ++e) {
    const bool interior = (s0 + e < ns - 1);
    const float cc = PARABOLIC ? dt * beta[e] : beta[e];
    if constexpr (FAST) {
      c[e] = interior ? cc : 0.0f;
      fe[e] = interior ? (PARABOLIC ? F : dt) : 0.0f;
    } else {
      c[e] = cc;
      fe[e] = PARABOLIC ? F : dt;
    }
  }

  // FOLD: running minimum of the even slots' magnitudes (one instruction; the compiler's fminf would canonicalise the carried value)
  float fold_min = __builtin_inff();
  auto fold_track = [&]() {
    if constexpr (FOLD) asm("v_min3_f32 %0, %1, |%2|, |%3|" : "=v"(fold_min) : "v"(fold_min), "v"(R.x[0]), "v"(R.x[2 % EPL]));
  };
  auto fold_below = [&]() { return __builtin_amdgcn_ballot_w64(!(fold_min >= kFoldFloor)) != 0ull; };     // wave-uniform

  // one PDE sub-step on the register-resident row (no bookkeeping).  GENERAL_EDGE: node 0 may be non-zero (first
  // sub-step after a reset) and, on the fast path, the frozen boundary slot takes the new control value.
  // pow2_tag: transport -- dx is a power of two; parabolic with FOLD -- the folded form (F is a power of two, see above).
  auto pde_substep = [&](auto general_edge, auto pow2_tag) {
    constexpr bool GENERAL_EDGE = decltype(general_edge)::value;
    constexpr bool POW2_DX = !PARABOLIC && decltype(pow2_tag)::value;
    constexpr bool FOLDED = FOLD && PARABOLIC && decltype(pow2_tag)::value && !GENERAL_EDGE;
    // p[first slot - 1]; after the first sub-step node 0 is identically 0, so the shift needs no fill operand
    const float xl = PARABOLIC ? from_left_lane(R.x[EPL - 1], GENERAL_EDGE ? R.bl : 0.0f) : 0.0f;
    const float xr = from_right_lane(R.x[0], 0.0f);                          // p[last slot + 1]
    float p0 = 0.f;
    if constexpr (!PARABOLIC) p0 = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, R.x[0])));
    if constexpr (PARABOLIC && NEUMANN) {
      // parabolic.py:148-150: previous row's neighbour u[t-1][-2]
      if constexpr (M64) bval = boundary_value<true>(P, a, a64, slot_get<EPL>(R.x, ns - 2), true);
      else bval = normalize_ctrl(cdx + slot_get<EPL>(R.x, ns - 2), P.max_control, P.normalize);
    }
    float y[EPL];
    if constexpr (FAST && PARABOLIC) {
      // Stage-major form of the same expression tree: the EPL independent chains advance together, so consecutive
      // instructions of a wave do not depend on each other (in-order issue stalls on back-to-back dependent VALU ops).
      // parabolic.py:143-144   u + F*(um - 2*u + up) + (dt*beta)*u
      float t2[EPL], t3[EPL], t4[EPL], t5[EPL], t7[EPL];
#pragma unroll
      for (int e = 0; e < EPL; ++e) {
        // pm - 2p: 2p is exact, so fma(-2, p, pm) == pm + (-2p).  The first slot takes the product form so that the
        // lane shift folds into the add (v_add_f32_dpp); VOP3 fma cannot carry a DPP operand.
        // ROLL (the T-steps-per-launch kernels, whose waves drift apart) with EPL > 1: the two DPP operands are written out with
        // an s_nop 0 ahead of each (the wave yields its issue slot before the DPP operation: open-loop rollout 368 -> 350 us per
        // 25 env-steps; in the lock-step per-env-step launch the same form is 2 % slower, so it stays on the compiler's).  Each
        // statement opens with a plain VALU instruction of its own, so that together with the s_nop two wait states separate
        // the DPP read from whatever the compiler scheduled in front (VALU write -> DPP read hazard).
        if (ROLL && EPL > 1 && e == 0 && !GENERAL_EDGE) {
          asm volatile("v_add_f32 %0, %2, %2\n\ts_nop 0\n\tv_sub_f32_dpp %0, %1, %0 wave_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1"
                       : "=&v"(t2[0]) : "v"(R.x[EPL - 1]), "v"(R.x[0]));
        } else if (ROLL && EPL > 1 && e == EPL - 1 && !GENERAL_EDGE) {
          t2[e] = 0.f;     // formed inside the statement below
        } else if (e == 0 && !GENERAL_EDGE) t2[e] = xl + (-2.0f * R.x[e]);
        else t2[e] = __builtin_fmaf(-2.0f, R.x[e], (e == 0) ? xl : R.x[e - 1]);
      }
#pragma unroll
      for (int e = 0; e < EPL; ++e) {
        if (ROLL && EPL > 1 && e == EPL - 1 && !GENERAL_EDGE)
          asm volatile("v_fma_f32 %0, -2.0, %2, %3\n\ts_nop 0\n\tv_add_f32_dpp %0, %1, %0 wave_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1"
                       : "=&v"(t3[e]) : "v"(R.x[0]), "v"(R.x[e]), "v"(R.x[e > 0 ? e - 1 : 0]));
        else
          t3[e] = t2[e] + ((e == EPL - 1) ? xr : R.x[e + 1]);
      }
#pragma unroll
      for (int e = 0; e < EPL; ++e) t7[e] = c[e] * R.x[e];
      if constexpr (FOLDED) {
#pragma unroll
        for (int e = 0; e < EPL; ++e) t5[e] = __builtin_fmaf(fe[e], t3[e], R.x[e]);
        (void)t4;
      } else {
#pragma unroll
        for (int e = 0; e < EPL; ++e) t4[e] = fe[e] * t3[e];
#pragma unroll
        for (int e = 0; e < EPL; ++e) t5[e] = R.x[e] + t4[e];
      }
#pragma unroll
      for (int e = 0; e < EPL; ++e) y[e] = t5[e] + t7[e];
    } else if constexpr (FAST && !PARABOLIC) {
      // hyperbolic.py:146-155   u + dt*((up - u)/dx + u[0]*beta), stage-major like the parabolic form above.
      // Quotient: RN32(RN64(d1 * RN64(1/dx))) == RN32(d1/dx): the double product is within 2^-52 (relative) of the
      // true quotient, while a quotient of two 24-bit floats is never closer than 2^-50 to a float rounding boundary
      // (checked on the device by pdegym_selftest_quotient).
      float d1[EPL], d2[EPL], r[EPL], d3[EPL], d4[EPL];
      double q[EPL];
#pragma unroll
      for (int e = 0; e < EPL; ++e) d1[e] = ((e == EPL - 1) ? xr : R.x[e + 1]) - R.x[e];
#pragma unroll
      for (int e = 0; e < EPL; ++e) r[e] = p0 * c[e];
      if constexpr (POW2_DX) {
        // dx = 2^k: d/dx == d * 2^-k exactly (same rounding into the denormal range, same overflow), one multiply
#pragma unroll
        for (int e = 0; e < EPL; ++e) d2[e] = d1[e] * rdxf;
        (void)q;
      } else {
#pragma unroll
        for (int e = 0; e < EPL; ++e) q[e] = (double)d1[e];
#pragma unroll
        for (int e = 0; e < EPL; ++e) q[e] = q[e] * P.rdx;
#pragma unroll
        for (int e = 0; e < EPL; ++e) d2[e] = (float)q[e];
      }
      if constexpr (BURGERS) {   // extension: u_t = u u_x + beta(x) u(0,t)  ->  p*((pp - p)/dx) replaces (pp - p)/dx
#pragma unroll
        for (int e = 0; e < EPL; ++e) d2[e] = R.x[e] * d2[e];
      }
#pragma unroll
      for (int e = 0; e < EPL; ++e) d3[e] = d2[e] + r[e];
#pragma unroll
      for (int e = 0; e < EPL; ++e) d4[e] = fe[e] * d3[e];
#pragma unroll
      for (int e = 0; e < EPL; ++e) y[e] = R.x[e] + d4[e];
      (void)xl;
    } else {
#pragma unroll
    for (int e = 0; e < EPL; ++e) {
      const float p = R.x[e];
      const float pm = (e == 0) ? xl : R.x[e - 1];
      const float pp = (e == EPL - 1) ? xr : R.x[e + 1];
      float v;
      if constexpr (PARABOLIC) {
        // parabolic.py:143-144   u + F*(um - 2*u + up) + (dt*beta)*u
        float t2;
        if constexpr (FAST) {
          t2 = __builtin_fmaf(-2.0f, p, pm);  // == pm - RN(2p): 2p is exact unless it overflows (-> EXACT redo)
        } else {
          const float t1 = 2.0f * p;
          t2 = pm - t1;
        }
        const float t3 = t2 + pp;
        const float t4 = fe[e] * t3;
        const float t5 = p + t4;
        if (M64 && beta64) {          // float64 beta: (dt*beta)*u and the final sum are double, rounded once
          v = (float)((double)t5 + c64[M64 ? e : 0] * (double)p);
        } else {
          const float t7 = c[e] * p;
          v = t5 + t7;
        }
      } else {
        // hyperbolic.py:146-155   u + dt*((up - u)/dx + u[0]*beta)
        const float d1 = pp - p;
        float d2;
        if constexpr (FAST) {
          // RN32(RN64(d1 * RN64(1/dx))) == RN32(d1/dx): the double product is within 2^-52 (relative) of the true
          // quotient, while a quotient of two 24-bit floats is never closer than 2^-50 to a float rounding boundary.
          d2 = (float)((double)d1 * P.rdx);
        } else {
          d2 = d1 / dx;
        }
        if (M64 && beta64) {          // float64 beta: u[0]*beta, the sum, dt*(...) and u + ... are double, rounded once
          const double r = (double)p0 * c64[M64 ? e : 0];
          const double d3 = (double)(BURGERS ? p * d2 : d2) + r;
          v = (float)((double)p + P.dt64 * d3);
        } else {
          const float r = p0 * c[e];
          const float d3 = (BURGERS ? p * d2 : d2) + r;
          const float d4 = fe[e] * d3;
          v = p + d4;
        }
        (void)pm;
      }
      if constexpr (!FAST) {
        const int sl = s0 + e;
        v = (sl >= ns - 1) ? ((sl == ns - 1) ? bval : 0.0f) : v;  // controlled boundary node; padding stays 0
      }
      y[e] = v;
    }
    }
#pragma unroll
    for (int e = 0; e < EPL; ++e) R.x[e] = y[e];
    if constexpr (FAST && GENERAL_EDGE) {  // the frozen boundary slot takes the new control value once (parabolic.py:148-150)
#pragma unroll
      for (int e = 0; e < EPL; ++e) R.x[e] = (s0 + e == ns - 1) ? bval : R.x[e];
    }
    R.bl = 0.0f;  // parabolic.py:146  u(0,t) = 0
    if constexpr (FOLDED) fold_track();      // the row the next fold sub-step reads
  };
  // rows whose norm a later reward call looks back at (tuned_reward_1d.py:40): r+100 is a step end
  auto record_norm = [&](int done) {
    if (done < nsub && (rec_all || R.k == 0 || R.t + PDEGYM_LOOKBACK == P.nt - 1)) {
      const float nr = sqrtf(slots_sumsq<EPL>(R.x, s0, ns));  // node 0 is 0 after any sub-step
      ring.put(R.t & (PDEGYM_RING - 1), nr, lane);
      if (R.t == R.back_row) R.back_norm = nr;                // this call's own look-back row: no memory round trip
    }
  };
  if constexpr (FAST) {
    // Every instruction of the loop -- scalar bookkeeping included -- takes an issue slot of the SIMD (about one per
    // 2.8 cycles with four resident waves), so the sub-steps between two norm records run in a bare inner loop and the
    // time index / phase counters advance once per run.
    int s = 0;
    // HIST: row R.t of the trajectory after every sub-step (frozen boundary slot = the commanded value, node 0 = 0: the row
    // as the reference stores it); the stores are fire-and-forget, nothing in the loop waits for them
    // `hist` is wave-uniform (step1d_body forms it from a scalar instance index): the row address is a scalar base, advanced by one
    // scalar add per sub-step, + the lane's slot offset.  A lane whose EPL slots all lie inside the row stores them as one vector; the
    // at most one lane that straddles the row's end stores slot by slot -- and only when there is such a lane (hoisted, wave-uniform).
    float* hrow = nullptr;
    const bool hfull = s0 + EPL <= ns, hpart = !hfull && s0 < ns;
    bool any_part = false;
    if constexpr (HIST) {
      if (hist) {
        hrow = hist + (size_t)R.t * n + J0;
        any_part = __builtin_amdgcn_ballot_w64(hpart) != 0ull;
        if constexpr (PARABOLIC) {
          for (int i = lane; i < nsub; i += kWave) hist[(size_t)(R.t + 1 + i) * n] = 0.0f;   // rows t_in+1 .. t_in+nsub <= nt-1
        }
      }
    }
    // PART: some lane straddles the row's end (decided once per call: the loops below exist in both forms, so the common form has no
    // test and no skipped block inside).  Node 0 of a parabolic row (0 after any sub-step, parabolic.py:146) is not part of the
    // slots: the nsub words of column 0 are stored once above, one per lane, so the rows are complete whatever the buffer held
    // before (history is a plain output, include/pdegym.h) and the sub-step loop carries no extra store.
    auto store_row = [&](auto part_tag) {
      if constexpr (HIST) {
        hrow += n;
        if (hfull) {
          float* q = hrow + s0;
          constexpr int Q = EPL / 4 * 4, D = (EPL - Q) / 2 * 2;
#pragma unroll
          for (int e = 0; e < Q; e += 4) *reinterpret_cast<pdegym_f4u*>(q + e) = pdegym_f4u{R.x[e], R.x[e + 1], R.x[e + 2], R.x[e + 3]};
          if constexpr (D == 2) *reinterpret_cast<pdegym_f2u*>(q + Q) = pdegym_f2u{R.x[Q], R.x[Q + 1]};
          if constexpr (Q + D < EPL) q[EPL - 1] = R.x[EPL - 1];
        }
        if constexpr (decltype(part_tag)::value) {
          if (hpart) {
#pragma unroll
            for (int e = 0; e < EPL; ++e)
              if (s0 + e < ns) hrow[s0 + e] = R.x[e];
          }
        }
      }
    };
    auto run_of = [&](int run, auto pow2_tag, auto part_tag) {
      for (int i = 0; i < run; ++i) {
        pde_substep(std::false_type{}, pow2_tag);
        store_row(part_tag);
      }
    };
    if (nsub > 0) {
      pde_substep(std::true_type{}, std::false_type{});
      ++R.t;
      R.k = (R.k + 1 == S) ? 0 : R.k + 1;
      s = 1;
      if (HIST && hrow) store_row(std::true_type{});
      record_norm(s);
    }
    bool folding = false;      // wave-uniform
    if constexpr (FOLD) {
      if (fold_ok) {           // (implies nsub > 1: the peeled sub-step has run)
        fold_track();
        folding = !fold_below();
      }
    }
    while (s < nsub) {
      int run = nsub - s;
      if (rec_all) {
        run = 1;
      } else {
        const int to_phase0 = S - R.k;                                   // sub-steps until R.k wraps to 0
        const int to_lookback = (P.nt - 1 - PDEGYM_LOOKBACK) - R.t;      // ... until R.t + LOOKBACK == nt - 1
        run = run < to_phase0 ? run : to_phase0;
        if (to_lookback > 0) run = run < to_lookback ? run : to_lookback;
      }
      if constexpr (HIST) {
        if (hrow == nullptr) {        // (never with HFAST: the launcher takes it only with a trajectory buffer)
          if (pow2_dx) for (int i = 0; i < run; ++i) pde_substep(std::false_type{}, std::true_type{});
          else for (int i = 0; i < run; ++i) pde_substep(std::false_type{}, std::false_type{});
        } else if (pow2_dx) {
          if (any_part) run_of(run, std::true_type{}, std::true_type{});
          else run_of(run, std::true_type{}, std::false_type{});
        } else {
          if (any_part) run_of(run, std::false_type{}, std::true_type{});
          else run_of(run, std::false_type{}, std::false_type{});
        }
      } else if constexpr (FOLD) {
        if (folding) for (int i = 0; i < run; ++i) pde_substep(std::false_type{}, std::true_type{});
        else for (int i = 0; i < run; ++i) pde_substep(std::false_type{}, std::false_type{});
      } else {
        if (pow2_dx) for (int i = 0; i < run; ++i) pde_substep(std::false_type{}, std::true_type{});
        else for (int i = 0; i < run; ++i) pde_substep(std::false_type{}, std::false_type{});
      }
      R.t += run;
      R.k += run;
      if (R.k >= S) R.k -= S;
      s += run;
      record_norm(s);
    }
    if constexpr (FOLD) {
      if (folding) *fold_redo = fold_below();      // some row a fold sub-step read was below the floor: the caller starts over
    }
  } else {
    for (int s = 0; s < nsub; ++s) {
      if (xprev && s == nsub - 1) {
#pragma unroll
        for (int e = 0; e < EPL; ++e) xprev[e] = R.x[e];
        *blprev = R.bl;
      }
      pde_substep(std::true_type{}, std::false_type{});
      ++R.t;
      R.k = (R.k + 1 == S) ? 0 : R.k + 1;
      if constexpr (NEUMANN) R.bsum += (double)fabsf(bval);
      if constexpr (HIST) {
        if (hist) {     // HIST without a buffer: the select-form kernel taken for the "differential" reward
          float* hrow = hist + (size_t)R.t * n;
          if (PARABOLIC && lane == 0) hrow[0] = 0.0f;
#pragma unroll
          for (int e = 0; e < EPL; ++e)
            if (s0 + e < ns) hrow[J0 + s0 + e] = R.x[e];
        }
      }
      record_norm(s + 1);
      if (thor_k > 0 && s + 1 < nsub && nsub - (s + 1) < thor_k) {    // wave-uniform; after record_norm: this slot holds the reward's norm
        const float nk = kind_norm<EPL>(R.x, R.bl, s0, ns, P.reward_kind);
        ring.put(R.t & (PDEGYM_RING - 1), nk, lane);
      }
    }
  }
  if constexpr (!NEUMANN) R.bsum += (double)nsub * (double)fabsf(bval);
}

template <int EPL, bool PARABOLIC>
__device__ __forceinline__ void load_row(Row<EPL>& R, float (&beta)[EPL], const float* urow, const float* brow, const int n,
                                         int lane) {
  constexpr int J0 = PARABOLIC ? 1 : 0;
  const int ns = n - J0, s0 = lane * EPL;
  load_slots<EPL>(urow + J0, R.x, s0, ns);
  load_slots<EPL>(brow + J0, beta, s0, ns);
  R.bl = PARABOLIC ? urow[0] : 0.f;
}

// One env-step of one instance by one wave: the body of step1d_kernel, and of every iteration of rollout1d_kernel.
// CARRY (rollout1d_kernel): the state enters and leaves through *carry instead of memory -- no row / beta / time-index / sum /
// ring loads at the head of the step.  What a step stores is what a caller can see of it afterwards: observation slot t + 1 and
// row t of the reward / flag arrays always; the per-instance state words that every step would overwrite (norm_now, norm_back,
// time_index, bsum -- and the ring, kept in registers) only when store_state says this is the launch's last step.
// STEP_KERNEL (round 7): the caller is step1d_kernel -- one env-step per launch, nothing in the launch reads what the step stored (kObsEarly).
// HFAST (round 6, with HIST): the fast sub-step loop storing every row into the trajectory buffer (bufs.history must be given; the
// launcher keeps the NormReward "differential" / "t-horizon" requests on the select form).
template <int EPL, bool PARABOLIC, bool NEUMANN, bool HIST, bool BURGERS = false, bool M64 = false, bool ROLL = false,
          bool CARRY = false, bool FULL = false, bool HFAST = false, bool STEP_KERNEL = false, bool FOLD = false>
__device__ __forceinline__ void step1d_body(const pdegym_params1d& P, const pdegym_bufs1d& Bf, const int B, const int inst,
                                            const int lane, const float* command = nullptr, Carry<EPL>* carry = nullptr,
                                            const bool store_state = true) {
  constexpr int J0 = PARABOLIC ? 1 : 0;
  static_assert(!HFAST || HIST, "HFAST is a history mode");
  constexpr bool kFast = !NEUMANN && !M64 && (!HIST || HFAST);
  static_assert(!CARRY || kFast, "the carried state is the float32 Dirichlet rollout path");
  static_assert(!FULL || kFast, "FULL rows: the float32 Dirichlet fast path only");
  // The fast-path step kernels with four slots per lane (nx = 256: the headline shape; not the carried rollouts, whose launches are
  // bound by HBM, and not the trajectory mode) with state_in -- the row's only home is obs, which is never the buffer being read --
  // store the row right after the sub-step loop, beside the norm chain instead of behind it, and write-through (store_slots_wt: why
  // four slots).  The rare paths that change what obs must hold (exact redo, auto-reset) drain the wave's stores and store again, with
  // plain stores like every store at the end of the step: write-through pays only together with the early position
  // (profiles/r07_ab_notes.txt: at the end of the wave it costs 0.37 us at S = 1).  STEP_KERNEL: step1d_kernel alone asks for it -- the
  // general rollout kernels instantiate this body without CARRY too, and a rollout step may re-read, behind a workgroup-scope fence,
  // a row that an earlier step stored: not one stored by a statement the compiler does not track.
  constexpr bool kObsEarly = STEP_KERNEL && kFast && !CARRY && !HFAST && EPL == 4;
  const int n = FULL ? kWave * EPL + J0 : P.n, ns = n - J0, s0 = lane * EPL;
  // state_in given: the row comes from the previous call's observation and goes to obs only (include/pdegym.h)
  const float* urow_in = (Bf.state_in ? Bf.state_in : Bf.u) + (size_t)inst * n;
  float* urow = Bf.state_in ? nullptr : Bf.u + (size_t)inst * n;
  const bool beta64 = M64 && P.beta_f64;
  // float32 beta row; in the mixed-precision mode with a float64 beta it is read as double below (beta then stays zero)
  const float* brow = beta64 ? urow_in : static_cast<const float*>(Bf.beta) + (size_t)inst * Bf.beta_stride;
  float* const ring_mem = Bf.ring + (size_t)inst * PDEGYM_RING;
  using RingT = std::conditional_t<CARRY, RingReg, RingMem>;
  RingT ring;
  if constexpr (CARRY) ring = carry->ring;
  else ring.mem = ring_mem;
  // (HFAST: a scalar instance index, so that the trajectory pointer is wave-uniform -- scalar base + lane offset addressing in the loop)
  float* hist = (HIST && Bf.history) ? Bf.history + (size_t)(HFAST ? __builtin_amdgcn_readfirstlane(inst) : inst) * P.nt * n : nullptr;

  Row<EPL> R;
  float beta[EPL];
  if constexpr (CARRY) {
#pragma unroll
    for (int e = 0; e < EPL; ++e) {
      R.x[e] = carry->x[e];
      beta[e] = carry->beta[e];
    }
    R.bl = carry->bl;
  } else {
    load_row<EPL, PARABOLIC>(R, beta, urow_in, brow, n, lane);
  }
  double b64[M64 ? EPL : 1];
  if constexpr (M64) {
    const double* brow64 = static_cast<const double*>(Bf.beta) + (size_t)inst * Bf.beta_stride;
#pragma unroll
    for (int e = 0; e < EPL; ++e) b64[e] = (beta64 && s0 + e < ns) ? brow64[J0 + s0 + e] : 0.0;
  }
  int t_in;
  double bsum_in;
  if constexpr (CARRY) {
    t_in = __builtin_amdgcn_readfirstlane(carry->t);     // wave-uniform by construction; keeps the loop counters scalar
    bsum_in = carry->bsum;
  } else {
    t_in = __builtin_amdgcn_readfirstlane(Bf.time_index[inst]);
    bsum_in = Bf.bsum[inst];
  }
  const int S = P.substeps > 0 ? P.substeps : 1;
  int nsub = P.nt - 1 - t_in;  // hyperbolic.py:140: while i < sample_rate and time_index < nt-1
  nsub = nsub < P.substeps ? nsub : P.substeps;
  nsub = nsub > 0 ? nsub : 0;
  const bool act64 = M64 && P.action_kind != PDEGYM_ACTION_F32;
  // command: the control input computed inside the launch (rollout kernel with its policy) instead of bufs.action
  const float a = command ? *command : (act64 ? 0.f : static_cast<const float*>(Bf.action)[inst]);
  const double a64 = act64 ? static_cast<const double*>(Bf.action)[inst] : 0.0;
  R.t = t_in;
  if constexpr (CARRY) R.k = __builtin_amdgcn_readfirstlane(carry->k);
  else R.k = (t_in + PDEGYM_LOOKBACK) % S;
  R.bsum = bsum_in;
  // look-back row of this call's reward (tuned_reward_1d.py:40): t_end - 100, Python negative index wraps into the
  // zero-filled tail of the history.  Rows that predate this call are fetched NOW (latency hidden by the loop).
  const int t_end = t_in + nsub;
  const int tb = t_end - PDEGYM_LOOKBACK;
  const int src_row = tb < 0 ? P.nt + tb : tb;
  const bool zero_row = (tb < 0 && src_row > t_end) || src_row < 0;
  const bool from_ring = !zero_row && src_row <= t_in;
  float norm_back_pre = 0.f;
  if (from_ring) norm_back_pre = ring.get(src_row & (PDEGYM_RING - 1), lane);
  R.back_row = (!zero_row && !from_ring) ? src_row : -1;
  R.back_norm = 0.f;

  // NormReward "differential" (norm_reward.py:55-59): ||u[t] - u[t-1]|| over FINE rows, so the row before the last sub-step is
  // kept.  Only the select-form instantiations evaluate it (launch_epl routes the request there; rollouts refuse it).
  const bool differential = !kFast && P.reward_horizon == PDEGYM_HORIZON_DIFFERENTIAL && P.reward_kind >= PDEGYM_REWARD_NORM_L1;
  float xprev[kFast ? 1 : EPL], blprev = 0.f;
#pragma unroll
  for (int e = 0; e < (kFast ? 1 : EPL); ++e) xprev[e] = 0.f;
  // NormReward "t-horizon" (norm_reward.py:60-73): the ring holds the reward's own norm of the rows the mean looks back at --
  // the row this call starts from (recorded here: independent of how the previous call or the reset left the slot), the last
  // rows of the sub-step loop, the final row (epilogue).  Select-form instantiations only, like "differential".
  const int thor_k = kFast ? 0 : thor_length(P);
  if constexpr (!kFast) {
    if (thor_k > 0) {
      const float nk0 = kind_norm<EPL>(R.x, R.bl, s0, ns, P.reward_kind);
      ring.put(t_in & (PDEGYM_RING - 1), nk0, lane);
    }
  }
  PDEGYM_HEAD_STAMP(2);      // (diagnostic build only: the row, beta and the per-instance words have arrived)
  float norm_now;
  bool obs_early = false;      // wave-uniform: the fast loop's row is already on its way to obs
  bool obs_final = false;      // ... and it is the row obs must hold unless an auto-reset follows
  if constexpr (kFast) {
    // The fast loop freezes the controlled boundary slot with zero coefficients: x + 0*t keeps every x except -0.0
    // (-0.0 + +0.0 = +0.0), so a commanded boundary value of exactly -0.0 takes the exact loop (wave-uniform test).
    bool exact = __float_as_uint(normalize_ctrl(a, P.max_control, P.normalize)) == 0x80000000u;
    if constexpr (PARABOLIC) {
      // The fast stencil forms um - 2u as ONE fma, which stays finite where the reference's 2*u overflows (|u| >= 2^127)
      // and could then decay back to a finite row that the non-finite test below never sees.  Rule it out up front: for
      // 0 <= F <= 1/2 the diffusion part is a convex combination (max-norm contraction), so one sub-step grows max|u| by at
      // most g = 1 + max|dt*beta| (+ rounding); otherwise by 1 + 4|F| + max|dt*beta|.  If max|u| * g^nsub can reach 2^126 the
      // exact loop runs instead (wave-uniform; costs two wave reductions per launch).
      float mx = fmaxf(fabsf(R.bl), fabsf(normalize_ctrl(a, P.max_control, P.normalize))), cm = 0.f;
      if constexpr (CARRY) {
        // no reductions here: max|dt*beta| is carried, and max|u| <= ||u||_2, the norm the previous step ended with.  That norm
        // is a float sum of squares: any |u[j]| >= 2^-60 has a normal square, so norm*(1 + 2^-10) bounds it; smaller rows are
        // covered by the 2^-60 floor.  A non-finite norm (NaN would be dropped by fmaxf) takes the exact loop.
        mx = fmaxf(fabsf(normalize_ctrl(a, P.max_control, P.normalize)), fmaxf(carry->norm * 1.0009765625f, 8.673617379884035e-19f));
        cm = carry->cm;
        exact = exact || !(carry->norm <= 3.4028234663852886e38f);
      } else {
#pragma unroll
        for (int e = 0; e < EPL; ++e) {
          mx = fmaxf(mx, fabsf(R.x[e]));
          cm = fmaxf(cm, fabsf(P.dt * beta[e]));
        }
        mx = wave_mag_max(mx);
        cm = wave_mag_max(cm);
      }
      if constexpr (CARRY) {
        // log2 g is carried, and log2 mx is only formed when the bound could matter: mx <= 2^40 and nsub log2 g <= 80 give
        // log2 mx + nsub log2 g <= 120 < 126 in the formula below as well -- the same decision, two v_log_f32 fewer per env-step
        const float budget = (float)nsub * carry->glog;
        if (!(mx <= 1.099511627776e12f && budget <= 80.0f)) exact = exact || !(__log2f(mx) + budget < 126.0f);
        (void)cm;
      } else {
        exact = exact || !(__log2f(mx) + (float)nsub * __log2f(growth_bound(P, cm)) < 126.0f);   // NaN / inf anywhere -> exact
      }
    }
    norm_now = 0.f;
    if (!exact) {
      if constexpr (FOLD) {
        // F = 2^-1 ... 2^-24 exactly (positive, zero mantissa, biased exponent 103 ... 126) and more than one sub-step: scalar tests
        // (run_substeps: FOLD).  The second pass, if the guard tripped inside the call, is the plain fast loop from the untouched input
        // row, set up like the exact redo below: it rewrites the ring slots of the first pass, same lane, program order.
        const unsigned int fbits = __float_as_uint(P.F);
        const bool fold_ok = nsub > 1 && (fbits & 0x7fffffu) == 0u && (fbits >> 23) >= 103u && (fbits >> 23) <= 126u;
        bool fold_redo = false;
        run_substeps<EPL, PARABOLIC, false, true, HFAST, BURGERS, false, ROLL, RingT, FULL, true>(
            R, beta, P, nsub, a, ring, hist, lane, nullptr, 0.0, nullptr, nullptr, 0, fold_ok, &fold_redo);
        if (fold_redo) {      // wave-uniform
          load_row<EPL, PARABOLIC>(R, beta, urow_in, brow, n, lane);
          R.t = t_in;
          R.k = (t_in + PDEGYM_LOOKBACK) % S;
          R.bsum = bsum_in;
          R.back_norm = 0.f;
          run_substeps<EPL, PARABOLIC, false, true, HFAST, BURGERS, false, ROLL, RingT, FULL>(R, beta, P, nsub, a, ring, hist, lane);
        }
      } else {
        run_substeps<EPL, PARABOLIC, false, true, HFAST, BURGERS, false, ROLL, RingT, FULL>(R, beta, P, nsub, a, ring, hist, lane);
      }
      if constexpr (kObsEarly) {
        if (Bf.state_in && P.sensing == PDEGYM_SENSE_FULL) {
          float* orow = Bf.obs + (size_t)inst * n;
          if (PARABOLIC && lane == 0) store_wt<0>(orow, R.bl);
          store_slots_wt<J0>(orow, R.x, s0, ns);
          obs_early = true;
        }
      }
      norm_now = sqrtf(slots_sumsq<EPL>(R.x, s0, ns) + R.bl * R.bl);
      // inf/NaN somewhere (or a squared overflow): 0*inf may have leaked into a frozen slot -> redo exactly
      exact = !(fabsf(norm_now) <= 3.4028234663852886e38f);
      obs_final = obs_early && !exact;
      if (exact) {
        if constexpr (CARRY) {
          // the carried input was overwritten: observation slot t holds the row (each lane re-reads the slots it stored),
          // beta may have been redrawn by another lane's stores of an earlier auto-reset -> order them first
          __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
          __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        }
        load_row<EPL, PARABOLIC>(R, beta, urow_in, brow, n, lane);
        if constexpr (CARRY) {
          R.bl = carry->bl;
          drain_vmem();
        }
        R.t = t_in;
        R.k = (t_in + PDEGYM_LOOKBACK) % S;
        R.bsum = bsum_in;
        R.back_norm = 0.f;
      }
    }
    if (exact) {
      // (HFAST: the exact loop rewrites the same trajectory rows)
      run_substeps<EPL, PARABOLIC, false, false, HFAST, BURGERS, false, false, RingT, FULL>(R, beta, P, nsub, a, ring, hist, lane);
      norm_now = sqrtf(slots_sumsq<EPL>(R.x, s0, ns) + R.bl * R.bl);
    }
  } else {
    run_substeps<EPL, PARABOLIC, NEUMANN, false, HIST, BURGERS, M64>(R, beta, P, nsub, a, ring, hist, lane, b64, a64,
                                                                     differential ? xprev : nullptr, &blprev, thor_k);
    norm_now = sqrtf(slots_sumsq<EPL>(R.x, s0, ns) + R.bl * R.bl);
  }
  const int t = R.t;

  // ---- epilogue: norms, flags, reward, observation ------------------------------------------------
  if (nsub > 0 && ring_records(P, R.k, t)) ring.put(t & (PDEGYM_RING - 1), norm_now, lane);
  const bool terminate = step_terminates(P, t);
  const bool truncate = step_truncates(P, norm_now);
  // NormReward variants need wave-wide reductions: do them before the single-lane tail
  float nr_alt = norm_now;
  bool nr_diff = false;
  if constexpr (!kFast) {
    if (differential && t > 0 && nsub > 0) {    // the row minus the one before it; the sign flips (norm_reward.py:56-58)
      nr_diff = true;
      const float d0 = fabsf(R.bl - blprev);      // node 0 is wave-uniform: joined after the reduction
      float acc = 0.f;
#pragma unroll
      for (int e = 0; e < EPL; ++e) {
        const float d = (s0 + e < ns) ? fabsf(R.x[e] - xprev[e]) : 0.f;
        if (P.reward_kind == PDEGYM_REWARD_NORM_L1) acc += d;
        else if (P.reward_kind == PDEGYM_REWARD_NORM_L2) acc += d * d;
        else acc = mag_max(acc, d);
      }
      if (P.reward_kind == PDEGYM_REWARD_NORM_L1) nr_alt = wave_sum(acc) + d0;
      else if (P.reward_kind == PDEGYM_REWARD_NORM_L2) nr_alt = sqrtf(wave_sum(acc) + d0 * d0);
      else nr_alt = mag_max(wave_mag_max(acc), d0);
    }
  }
  if (!nr_diff && P.reward_kind == PDEGYM_REWARD_NORM_L1) {
    float s1 = 0.f;
#pragma unroll
    for (int e = 0; e < EPL; ++e) s1 += (s0 + e < ns) ? fabsf(R.x[e]) : 0.f;
    nr_alt = wave_sum(s1) + fabsf(R.bl);
  } else if (!nr_diff && P.reward_kind == PDEGYM_REWARD_NORM_LINF) {
    float m = fabsf(R.bl);
#pragma unroll
    for (int e = 0; e < EPL; ++e) m = mag_max(m, (s0 + e < ns) ? fabsf(R.x[e]) : 0.f);
    nr_alt = wave_mag_max(m);
  }
  float thor_mean = 0.f;
  if constexpr (!kFast) {
    if (thor_k > 0 && lane == 0) {      // -sum(norm(u[t - i]) for i in range(k)) / k, k = min(t_horizon_length, t + 1): one float32 chain
      if (nsub > 0) ring.mem[t & (PDEGYM_RING - 1)] = nr_alt;
      const int kk = thor_k < t + 1 ? thor_k : t + 1;
      float acc = nr_alt;
      for (int i = 1; i < kk; ++i) acc += ring.mem[(t - i) & (PDEGYM_RING - 1)];
      thor_mean = acc / (float)kk;
    }
  }
  // look-back norm: fetched before the loop, captured inside it, the final row itself (nsub == 100 ends on it only
  // when LOOKBACK == 0, never), or 0 for an unwritten row
  float norm_back = 0.f;
  float reward = 0.f;
  if (lane == 0) {
    norm_back = from_ring ? norm_back_pre : ((R.back_row >= 0) ? ((R.back_row == t) ? norm_now : R.back_norm) : 0.f);
    if (P.reward_kind == PDEGYM_REWARD_TUNED1D) {
      if (terminate && norm_now < 20.0f) {
        reward = (P.terminate_reward - ((float)R.bsum) / 1000.0f) - norm_now;  // tuned_reward_1d.py:36-37
      } else if (truncate) {
        reward = (float)((double)P.truncate_penalty * (double)(P.reward_nt - t));  // tuned_reward_1d.py:38-39
      } else {
        reward = norm_back - norm_now;  // tuned_reward_1d.py:40
      }
    } else if (P.reward_kind >= PDEGYM_REWARD_NORM_L1) {
      // documented intent of norm_reward.py:48-54 ("temporal" horizon)
      reward = terminate ? P.terminate_reward
                         : (truncate ? (float)((double)P.truncate_penalty * (double)(P.reward_nt - t))
                                     : (nr_diff ? nr_alt : (thor_k > 0 ? -thor_mean : -nr_alt)));
    }
  }

  // sensing_update (hyperbolic.py:72-116)
  const bool auto_reset = (Bf.reset_init != nullptr) && (terminate || truncate);  // wave-uniform
  auto node = [&](int j) -> float { return (PARABOLIC && j == 0) ? R.bl : slot_get<EPL>(R.x, j - J0); };
  auto emit_obs = [&](float* obs_base) {
    if (P.sensing == PDEGYM_SENSE_FULL) {
      float* orow = obs_base + (size_t)inst * n;
      if (PARABOLIC && lane == 0) orow[0] = R.bl;
      store_slots<EPL>(orow + J0, R.x, s0, ns);
    } else {
      float o;
      if (P.sensing == PDEGYM_SENSE_LAST) o = node(n - 1);
      else if (P.sensing == PDEGYM_SENSE_LAST_DERIV) o = (node(n - 1) - node(n - 2)) / P.dx;
      else if (P.sensing == PDEGYM_SENSE_FIRST_DERIV) o = (node(1) - node(0)) / P.dx;
      else o = node(0);
      if (lane == 0) obs_base[inst] = o;
    }
  };
  store_step_words(P, Bf, inst, lane, reward, norm_now, norm_back, terminate, truncate, store_state);
  if (!auto_reset) {
    if (nsub > 0 && urow) {
      if (PARABOLIC && lane == 0) urow[0] = R.bl;
      store_slots<EPL>(urow + J0, R.x, s0, ns);
    }
    if (!obs_final) {
      if (obs_early) drain_vmem();      // the exact redo's row goes over the fast loop's
      emit_obs(Bf.obs);
    }
    if (lane == 0 && store_state) {
      Bf.time_index[inst] = t;
      Bf.bsum[inst] = R.bsum;
    }
    if constexpr (CARRY) {
      carry->t = t;
      carry->k = R.k;
      carry->bsum = R.bsum;
      carry->norm = norm_now;
    }
  } else {
    // fused VecEnv auto-reset: keep the terminal observation, restart from the pool row (hyperbolic.py:214-227)
    if (Bf.final_obs) emit_obs(Bf.final_obs);
    const int prow = pool_row(Bf.reset_pool_rows, Bf.reset_count, inst, B);
    const float* irow = Bf.reset_init + (size_t)prow * n;
    if (Bf.reset_beta && Bf.beta_stride != 0) {      // the reference redraws beta at every reset (hyperbolic.py:208)
      if (beta64) {
        double* bdst = const_cast<double*>(static_cast<const double*>(Bf.beta)) + (size_t)inst * Bf.beta_stride;
        const double* bsrc = static_cast<const double*>(Bf.reset_beta) + (size_t)prow * n;
        for (int j = lane; j < n; j += kWave) bdst[j] = bsrc[j];
      } else {
        float* bdst = const_cast<float*>(brow);
        const float* bsrc = static_cast<const float*>(Bf.reset_beta) + (size_t)prow * n;
        for (int j = lane; j < n; j += kWave) bdst[j] = bsrc[j];
        if constexpr (CARRY) {      // the carried copy follows the redraw
#pragma unroll
          for (int e = 0; e < EPL; ++e) carry->beta[e] = (s0 + e < ns) ? bsrc[J0 + s0 + e] : 0.f;
          carry_refresh_beta<EPL, PARABOLIC>(*carry, P, s0, ns);
        }
      }
    }
    if (Bf.reset_count && lane == 0) Bf.reset_count[inst] += 1;
    R.bl = PARABOLIC ? irow[0] : 0.f;
    if (PARABOLIC && lane == 0 && urow) urow[0] = R.bl;
#pragma unroll
    for (int e = 0; e < EPL; ++e) {
      R.x[e] = (s0 + e < ns) ? irow[J0 + s0 + e] : 0.f;
      if (s0 + e < ns && urow) urow[J0 + s0 + e] = R.x[e];
    }
    if constexpr (HIST) {
      if (hist) wipe_history(hist, irow, P.nt, n, lane);
    }
    const float n0 = sqrtf(slots_sumsq<EPL>(R.x, s0, ns) + R.bl * R.bl);
    const float last = node(n - 1);
    if (obs_early) drain_vmem();        // the pool row goes over the terminal row stored after the fast loop
    emit_obs(Bf.obs);
    if (lane == 0 && store_state) {
      Bf.time_index[inst] = 0;
      Bf.bsum[inst] = (double)fabsf(last);
    }
    ring.put(0, n0, lane);
    if constexpr (CARRY) {
      carry->t = 0;
      carry->k = PDEGYM_LOOKBACK % S;
      carry->bsum = (double)fabsf(last);
      carry->norm = n0;
      drain_vmem();
    }
  }
  if constexpr (CARRY) {
#pragma unroll
    for (int e = 0; e < EPL; ++e) carry->x[e] = R.x[e];
    carry->bl = R.bl;
    carry->ring = ring;
  }
}

// The state a rollout launch starts from, read ONCE: row (observation slot 0), beta, time index and |u[-1]| sum.
template <int EPL, bool PARABOLIC, bool FULL = false>
__device__ __forceinline__ void carry_load(Carry<EPL>& C, const pdegym_params1d& P, const pdegym_bufs1d& Bf, const float* row0, int inst,
                                           int lane) {
  constexpr int J0 = PARABOLIC ? 1 : 0;
  const int n = FULL ? kWave * EPL + J0 : P.n, ns = n - J0, s0 = lane * EPL;
  Row<EPL> R0;
  load_row<EPL, PARABOLIC>(R0, C.beta, row0 + (size_t)inst * n, static_cast<const float*>(Bf.beta) + (size_t)inst * Bf.beta_stride, n, lane);
#pragma unroll
  for (int e = 0; e < EPL; ++e) C.x[e] = R0.x[e];
  C.bl = R0.bl;
  carry_refresh_beta<EPL, PARABOLIC>(C, P, s0, ns);
  C.norm = sqrtf(slots_sumsq<EPL>(C.x, s0, ns) + C.bl * C.bl);
  C.t = __builtin_amdgcn_readfirstlane(Bf.time_index[inst]);
  C.k = (C.t + PDEGYM_LOOKBACK) % (P.substeps > 0 ? P.substeps : 1);
  C.bsum = Bf.bsum[inst];
  const float* ring = Bf.ring + (size_t)inst * PDEGYM_RING;
  C.ring.lo = ring[lane];
  C.ring.hi = ring[kWave + lane];
  drain_vmem();
}

// ... and the ring written back at the end of the launch (the other state words were stored by the last step, store_state).
template <int EPL>
__device__ __forceinline__ void carry_store_ring(const Carry<EPL>& C, const pdegym_bufs1d& Bf, int inst, int lane) {
  float* ring = Bf.ring + (size_t)inst * PDEGYM_RING;
  ring[lane] = C.ring.lo;
  ring[kWave + lane] = C.ring.hi;
}

// ---- host side: the slots-per-lane ladder, once: f(std::integral_constant<int, E>) for the E that serves a float32 row of epl =
// ceil(slots / 64) slots per lane.  The step launcher and every rollout launcher pick through it: the norm reductions, hence the
// rewards, depend on the layout.  MAX_E = 32: every row; MAX_E = 8: the kernels that carry a controller (longer rows were refused).
template <int MAX_E, typename F>
inline void with_epl(int epl, F&& f) {
  if (epl <= 1) f(std::integral_constant<int, 1>{});
  else if (epl <= 2) f(std::integral_constant<int, 2>{});
  else if (epl <= 3) f(std::integral_constant<int, 3>{});
  else if (epl <= 4) f(std::integral_constant<int, 4>{});
  else if (epl <= 5) f(std::integral_constant<int, 5>{});
  else if (epl <= 6) f(std::integral_constant<int, 6>{});
  else if (MAX_E == 8 || epl <= 8) f(std::integral_constant<int, 8>{});
  else if constexpr (MAX_E == 32) {
    if (epl <= 12) f(std::integral_constant<int, 12>{});
    else if (epl <= 16) f(std::integral_constant<int, 16>{});
    else if (epl <= 24) f(std::integral_constant<int, 24>{});
    else f(std::integral_constant<int, 32>{});
  }
}
// E with a FULL instantiation: rows of exactly 64 / 128 / 256 / 512 slots, whose slot masks fold away
constexpr bool epl_has_full(int E) { return E == 1 || E == 2 || E == 4 || E == 8; }

}  // namespace
#endif
