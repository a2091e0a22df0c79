/*
 * pdegym.h -- C ABI of the MI355X (gfx950) batched PDE-environment stepper.
 *
 * Drop-in boundary for the hot path of lukebhan/PDEControlGym (reference checkout paths below are
 * relative to that repository):
 *
 *   pdegym_transport_step   replaces TransportPDE1D.step          environments1d/hyperbolic.py:126-169
 *                           + terminate()/truncate()              environments1d/hyperbolic.py:171-194
 *                           + TunedReward1D.reward                rewards/tuned_reward_1d.py:25-40
 *   pdegym_parabolic_step   replaces ReactionDiffusionPDE1D.step  environments1d/parabolic.py:126-164
 *                           + terminate()/truncate()              environments1d/parabolic.py:166-189
 *   pdegym_reset1d_masked   replaces the state part of reset()    hyperbolic.py:214-219, parabolic.py:208-213
 *   pdegym_ns2d_step_f32/_f64  replaces NavierStokes2D.step       environments2d/navier_stokes2D.py:118-157
 *                           (apply_boundary :68-91, solve_pressure :94-116, NSReward ns_reward.py:28)
 *   pdegym_ns2d_solve_pressure_f32/_f64  replaces NavierStokes2D.solve_pressure  navier_stokes2D.py:94-116
 *                           (public API: examples/NavierStokes/NS2Doptimization.py:97)
 *   pdegym_ns2d_reset_masked_f32/_f64    replaces the state part of NavierStokes2D.reset  navier_stokes2D.py:186-192
 *   pdegym_rownorm2_f32     replaces np.linalg.norm(row, 2)       hyperbolic.py:190, parabolic.py:185
 *   pdegym_backstep_gain_transport / _parabolic  replace solveKernelFunction   examples/transportPDE/transport1Dbackstepping.py:22-29,
 *                                                examples/reactionDiffusionPDE/reactionDiffusion1DBackstepping.py:22-35
 *   pdegym_backstep_control replaces solveControl                 transport1Dbackstepping.py:32-36, reactionDiffusion1DBackstepping.py:38-39
 *   pdegym_traffic_backstep_control replaces bcksController       examples/TrafficPDE1D/Backstepping control.ipynb, cell 5
 *   pdegym_traffic_backstep_rollout replaces runSingleEpisode's loop around it (same cell)
 *   pdegym_ns2d_adjoint_f64 replaces the backward march and the control read-off of the adjoint-optimisation baseline
 *                                                examples/NavierStokes/NS2Doptimization.py:83-107
 *   pdegym_gae              replaces what SB3's PPO runs after every rollout of the reference's training scripts
 *                           (examples/transportPDE/transport1Dppo.py:88-90): RolloutBuffer.compute_returns_and_advantage
 *   pdegym_mlp_backward     replaces the autograd backward pass of the MlpPolicy networks in the gradient step of the same scripts
 *                           (model.learn: PPO.train / SAC.train), for layers of at most 64 units
 *   pdegym_ppo_loss         replaces the loss of PPO.train in the same scripts (stable_baselines3/ppo/ppo.py: clipped surrogate,
 *                           F.mse_loss value term, entropy term, approx_kl, clip_fraction, per-minibatch advantage normalisation)
 *                           for MlpPolicy's DiagGaussianDistribution, the minibatch gathers and the autograd pass back to the
 *                           networks' outputs
 *   pdegym_diag_gaussian_log_prob  replaces DiagGaussianDistribution.log_prob (common/distributions.py)
 *   pdegym_squashed_gaussian_sample (+ _backward), pdegym_sac_critic_loss, pdegym_sac_actor_loss
 *                           replace the losses of SAC.train (stable_baselines3/sac/sac.py) in the reference's SAC scripts
 *                           (examples/transportPDE/transport1Dsac.py): SquashedDiagGaussianDistribution sample and log_prob, the
 *                           soft Bellman target, critic, actor and entropy-coefficient losses and the autograd pass back to the
 *                           networks' outputs
 *   pdegym_fused_adam       replaces the tail of every gradient step of those scripts (torch.nn.utils.clip_grad_norm_, torch.optim.Adam
 *                           and, for SAC, stable_baselines3/common/utils.py: polyak_update) and writes the blocked weight copies of
 *                           pdegym_mlp_forward while it is there
 *   PDEGYM_ROLLOUT_FINAL_OBS_PER_STEP (a bit of the rollout descriptors' reserved_) keeps what SB3's VecEnv hands on as
 *                           infos[i]["terminal_observation"] for EVERY step of a one-launch rollout (final_obs becomes [T, B, obs_dim]),
 *                           and pdegym_mlp_forward_masked evaluates V(terminal_observation) on the rows with
 *                           infos[i]["TimeLimit.truncated"] only: the two halves of the truncation bootstrap of
 *                           stable_baselines3/common/on_policy_algorithm.py: collect_rollouts
 *   pdegym_mlp_forward_gather, pdegym_mlp_backward_gather, pdegym_mlp_backward_wide_gather
 *                           replace the replay_data.observations[...] / rollout_data minibatch gathers in front of the networks in
 *                           SAC.train and PPO.train (stable_baselines3/common/buffers.py: ReplayBuffer._get_samples): the first layer
 *                           reads row index[b] of the storage in place
 *
 * One call advances EVERY instance of a batch by one env-step (S PDE sub-steps for the 1D envs, one
 * Chorin projection step with K Jacobi sweeps for NS2D).  Instances are independent.
 *
 * Conventions
 *   - every pointer is a DEVICE-ACCESSIBLE pointer owned by the caller (PyTorch-ROCm tensors in this repo): HBM, or pinned
 *     host memory mapped into the device's address space (hipHostMalloc).  The plant state belongs in HBM; per-call INPUTS
 *     (action, control, kill, t_benchmark) and pure OUTPUTS (obs, reward, norm_now, norm_back, terminated, truncated, done) may
 *     live in pinned host memory -- the kernels read / write them in place, which is how the batch-of-one faces of the Python
 *     layer take a command and hand back a result with one launch + one stream synchronisation and no copies
 *     (PDEBatch1D.enable_host_io; the reference's own callers step ONE environment: examples/transportPDE/transport1Dppo.py:59-90);
 *     the library allocates nothing and keeps no state besides a thread-local error string;
 *   - calls only ENQUEUE work on `stream` (a hipStream_t passed as void*); they never synchronise;
 *   - return value 0 = success, negative = error (message via pdegym_last_error()); nothing throws;
 *   - arrays are C-contiguous; the grid axis is the fastest axis;
 *   - a pointer needs only the NATURAL ALIGNMENT OF ITS ELEMENT TYPE (1 byte for the uint8 flags, 4 for float / int32, 8 for double /
 *     int64), unless its parameter says otherwise: a slot of a [T + 1, B, obs_dim] rollout buffer, a view into a larger tensor and an
 *     array carved out of a pool are all valid, and the results do not depend on where a buffer starts.  The exceptions -- the
 *     blocked MLP weights and obs / U_ref / lam of the adjoint march: 16 bytes; the workspace of pdegym_mlp_backward: 4 -- are
 *     stated at the parameter (every pointer of pdegym_ppo_loss and pdegym_diag_gaussian_log_prob takes element accesses only;
 *     the workspace of pdegym_ppo_loss holds doubles and needs 4 bytes), and a pointer that violates one is refused with -2 and a message naming the argument BEFORE anything
 *     is launched (never rerouted to another kernel: the bits of a result must not depend on an address).  The refusals are new
 *     with this wording (the struct layouts and PDEGYM_ABI_VERSION are unchanged): earlier libraries launched such a call and its
 *     16-byte accesses were the undefined behaviour the requirement now names;
 *   - non-finite data is ordinary data, as it is to the reference: a NaN command, observation or state cell propagates exactly as
 *     NumPy / PyTorch propagate it there (a stencil spreads it to the cells that read it, norms and rewards become NaN, comparisons
 *     with it are false), and every clamp (the action clips of the environments, the fused clamp of pdegym_mlp_forward, of the
 *     in-kernel policies and of pdegym_backstep_control's out32, the tumour's clip to [0, k]) KEEPS a NaN like np.clip and
 *     torch.clamp do -- a diverged policy shows up as NaN observations and rewards within a step, not as the lower action bound.
 *     +-Inf is clamped to the bound.  relu keeps a NaN too (torch.relu).  Instances are independent in this as well: a non-finite
 *     value in one instance changes no bit of another.  Clamp BOUNDS, sizes, strides and counts must be finite.
 */
#ifndef PDEGYM_H
#define PDEGYM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PDEGYM_ABI_VERSION 21
/* Bit 0 of pdegym_rollout1d.reserved_, pdegym_rollout_traffic.reserved_ and pdegym_rollout_tumor.reserved_ (the other bits are ignored):
 * the final_obs of the call (pdegym_bufs1d.final_obs, pdegym_bufs_traffic.final_obs, pdegym_wrap_tumor.final_obs) is an array
 * [T, B, obs_dim] instead of [B, obs_dim].  Row (t, b) receives what final_obs[b] would hold after the t-th of T consecutive step
 * calls -- the last observation of the finished episode -- and is written ONLY where step t ended the episode of instance b
 * (terminated | truncated) and the fused auto-reset restarted it; no other row is touched, and the engine's own [B, obs_dim] final_obs
 * is NOT written by such a call.  Every other output and the state left behind keep their bits.  With the bit set, final_obs == NULL
 * is refused with -3 and a call without an auto-reset pool (reset_init / reset_rs) with -2, before anything is launched. */
#define PDEGYM_ROLLOUT_FINAL_OBS_PER_STEP 1
#define PDEGYM_RING 128          /* slots of the per-instance row-norm ring (look-back is 100 rows) */
#define PDEGYM_LOOKBACK 100      /* tuned_reward_1d.py:25,40: int(1/0.01) rows */
#define PDEGYM_MAX_N1D 2048      /* nodes per 1D row kept in registers by the wave-per-instance kernels */
#define PDEGYM_MAX_N1D_WIDE 8192 /* longer rows (up to this) ping-pong through wave-private LDS */

/* control_type (hyperbolic.py:66-124): the reference's (mis)spelling "Dirchilet" is kept in the Python layer */
enum { PDEGYM_CONTROL_DIRICHLET = 0, PDEGYM_CONTROL_NEUMANN = 1 };
enum { PDEGYM_FLUX_LINEAR = 0, PDEGYM_FLUX_BURGERS = 1 };   /* transport kernels only */
/* What the caller of the reference's step() passed as `control` -- it decides, under NumPy's promotion rules, in which
 * precision control_update()/normalize() are evaluated before the value is stored into the float32 row
 * (hyperbolic.py:143-145, parabolic.py:148-150, base_env_1d.py:36-39): */
enum {
  PDEGYM_ACTION_F32 = 0,   /* float32 array / np.float32 (what SB3 passes): everything in float32; action = float[B]     */
  PDEGYM_ACTION_F64 = 1,   /* np.float64 scalar or array (and a Python float under NumPy 1.x value-based casting):
                              control*dx + neighbour and (a+1)*max-max in double, rounded once on store; action = double[B] */
  PDEGYM_ACTION_WEAK = 2   /* Python float / int under NumPy >= 2 (NEP 50 weak scalar): Dirichlet as F64; Neumann forms
                              control*dx in double, then joins the float32 neighbour in float32; action = double[B]        */
};
/* sensing_update variants (hyperbolic.py:72-116, parabolic.py:72-116) */
enum {
  PDEGYM_SENSE_FULL = 0,        /* obs = row                              obs_dim = n */
  PDEGYM_SENSE_LAST = 1,        /* obs = row[-1]                          (Neumann control, collocated) */
  PDEGYM_SENSE_LAST_DERIV = 2,  /* obs = (row[-1]-row[-2])/dx             (Dirichlet control, collocated) */
  PDEGYM_SENSE_FIRST_DERIV = 3, /* obs = (row[1]-row[0])/dx               (opposite, Neumann sensing) */
  PDEGYM_SENSE_FIRST = 4        /* obs = row[0]                           (opposite, Dirichlet sensing) */
};
/* reward evaluated inside the step kernel */
enum {
  PDEGYM_REWARD_NONE = 0,       /* reward[] untouched; norms/flags still produced (host-side custom rewards) */
  PDEGYM_REWARD_TUNED1D = 1,    /* rewards/tuned_reward_1d.py:25-40 */
  PDEGYM_REWARD_NORM_L1 = 2,    /* rewards/norm_reward.py "temporal" intent (parity unpinned: reference class raises) */
  PDEGYM_REWARD_NORM_L2 = 3,
  PDEGYM_REWARD_NORM_LINF = 4
};
/* NormReward horizon (rewards/norm_reward.py:52-73) */
enum {
  PDEGYM_HORIZON_TEMPORAL = 0,     /* -||u[t]||                                                                */
  PDEGYM_HORIZON_DIFFERENTIAL = 1, /* +||u[t] - u[t-1]|| over fine-time rows (t > 0), evaluated by pdegym_step1d_* */
  PDEGYM_HORIZON_T = 2             /* "t-horizon": -(||u[t]|| + ... + ||u[t-k+1]||) / k over fine-time rows, k =
                                      min(reward_t_horizon, t + 1), one float32 chain starting at row t; pdegym_*_step only.
                                      The ring then holds the reward's own norms (norm_back is meaningless)        */
};

/* Scalars of one 1D environment family (same for every instance of the batch). */
typedef struct pdegym_params1d {
  int32_t n;                /* nodes per row: nx (transport) or nx+1 (parabolic ghost point, parabolic.py:124) */
  int32_t nt;               /* rows per episode, int(round(T/dt)+1)                       base_env_1d.py:23 */
  int32_t substeps;         /* S = int(round(control_sample_rate/dt))                     hyperbolic.py:137 */
  int32_t control_type;     /* PDEGYM_CONTROL_*                                                              */
  int32_t normalize;        /* (a+1)*max-max if non-zero                                  base_env_1d.py:36-39 */
  int32_t sensing;          /* PDEGYM_SENSE_*                                                                */
  int32_t limit_state;      /* limit_pde_state_size                                       hyperbolic.py:188-191 */
  int32_t reward_kind;      /* PDEGYM_REWARD_*                                                               */
  int32_t reward_nt;        /* TunedReward1D(nt, ...) ctor argument                       tuned_reward_1d.py:17-23 */
  float dt;                 /* float32 cast of the Python doubles: NumPy casts them where they meet a float32 array */
  float dx;
  float F;                  /* (float)(dt/dx**2)                                          parabolic.py:138 */
  float max_control;        /* max_control_value */
  float max_state;          /* max_state_value */
  float truncate_penalty;   /* TunedReward1D / NormReward arguments */
  float terminate_reward;
  double rdx;               /* 1.0/(double)(float)dx: the transport quotient (u[j+1]-u[j])/dx is formed as
                               (float)((double)d * rdx), which equals the IEEE float32 division bit for bit */
  int32_t flux;             /* PDEGYM_FLUX_LINEAR = the reference's transport term; PDEGYM_FLUX_BURGERS = extension,
                               NOT in the reference (parity unpinned): n[j] = p[j] + dt*(p[j]*((p[j+1]-p[j])/dx) + (p[0]*beta)[j]) */
  int32_t beta_f64;         /* non-zero: bufs.beta is double[] -- the reference's arithmetic when reset_recirculation_func returns
                               float64 (e.g. np.ones(nx), docs/source/guide/quickstart.rst:27-28): u[0]*beta, dt*beta*u and the
                               sums they enter are evaluated in double and rounded once when the row is stored
                               (hyperbolic.py:146-155, parabolic.py:143-144)                                              */
  int32_t action_kind;      /* PDEGYM_ACTION_*                                                                            */
  int32_t reward_horizon;   /* PDEGYM_HORIZON_* (NormReward kinds only; pdegym_step1d, not the rollout entry points)      */
  double dt64, dx64;        /* the Python doubles themselves (used where they meet a float64 operand)                     */
  double max_control64;
  int32_t reward_t_horizon; /* PDEGYM_HORIZON_T: t_horizon_length of NormReward (norm_reward.py:19), 1 .. PDEGYM_RING             */
  int32_t reserved1_;
} pdegym_params1d;

/* Per-instance device buffers of a 1D batch (B instances). */
typedef struct pdegym_bufs1d {
  float* u;                 /* [B, n]   live row (in/out)                                                     */
  const void* beta;         /* [B, n] or [n]   plant parameter beta(x) / lambda(x): float, or double when beta_f64    */
  int64_t beta_stride;      /* elements between instances; 0 = one shared row                                 */
  const void* action;       /* [B]      control input of this env-step: float, or double when action_kind != F32      */
  int32_t* time_index;      /* [B]      in/out                                                                */
  double* bsum;             /* [B]      running sum |u[tau,-1]| over written rows (in/out)  tuned_reward_1d.py:37 */
  float* ring;              /* [B, PDEGYM_RING]  row norms that a later look-back will read (in/out)          */
  float* obs;               /* [B, obs_dim] out                                                               */
  float* reward;            /* [B] out                                                                        */
  float* norm_now;          /* [B] out  ||u_t||_2                                                             */
  float* norm_back;         /* [B] out  ||u_{t-100}||_2 (0 for an unwritten row)                              */
  uint8_t* terminated;      /* [B] out                                                                        */
  uint8_t* truncated;       /* [B] out                                                                        */
  float* history;           /* optional [B, nt, n] full trajectory (NULL = keep only the live row): a step writes the
                               whole rows t_in+1 .. t_in+nsub of each instance (every node, the parabolic node 0 included)
                               and no other row; pdegym_reset1d_masked writes row 0 = init and zero-fills the rest        */
  const float* reset_init;  /* optional [B, n] pool of next initial conditions: when non-NULL an instance whose
                               step ends terminated|truncated is restarted INSIDE the same launch (state := pool row,
                               time_index := 0) and obs[b] is the first observation of the new episode            */
  float* final_obs;         /* optional [B, obs_dim]: last observation of the finished episode (written only for
                               instances that were auto-reset in this call; SB3's "terminal_observation"); [T, B, obs_dim]
                               in a rollout call with PDEGYM_ROLLOUT_FINAL_OBS_PER_STEP                             */
  /* The reference redraws BOTH the initial condition and beta at every reset (hyperbolic.py:207-209).  With a pool of
   * reset_pool_rows >= B rows, the k-th restart of instance b takes pool row (b + k*B) mod reset_pool_rows, so consecutive
   * episodes of one instance start from different rows without any host work; reset_pool_rows == 0 means B (row b always). */
  const void* reset_beta;   /* optional [reset_pool_rows, n] (same element type as beta): on an auto-reset beta[b] := the pool row
                               (needs beta_stride != 0, i.e. per-instance beta, and a writable beta buffer)        */
  int32_t* reset_count;     /* optional [B] in/out: restarts of each instance so far (k above); NULL = always row b  */
  int32_t reset_pool_rows;  /* rows of reset_init / reset_beta (0 = B)                                            */
  int32_t reserved_;
  /* With full-state sensing the observation IS the row (hyperbolic.py:72-75, parabolic.py:74-77).  state_in, when non-NULL
   * (needs sensing == PDEGYM_SENSE_FULL and history == NULL): the rows are READ from state_in [B, n] -- the obs buffer of the
   * previous call -- and the new rows are written to obs only; u is not touched and may be NULL.  One row store per instance
   * and env-step instead of two; obs must not alias state_in (double-buffer the observations).  pdegym_reset1d_masked with
   * u == NULL likewise writes the reset rows to obs only. */
  const float* state_in;
} pdegym_bufs1d;

int pdegym_abi_version(void);
const char* pdegym_last_error(void);

int pdegym_transport_step(const pdegym_params1d* prm, const pdegym_bufs1d* buf, int32_t B, void* stream);
int pdegym_parabolic_step(const pdegym_params1d* prm, const pdegym_bufs1d* buf, int32_t B, void* stream);

/* T env-steps in ONE launch (the on-device rollout of SURVEY.md section 8f rank 1 without a kernel boundary per step):
 * replaces the loop of env.step calls that SB3's model.learn() drives (examples/transportPDE/transport1Dppo.py:88-90,
 * examples/reactionDiffusionPDE/reactionDiffusion1Dppo.py), i.e. T x (hyperbolic.py:126-194 / parabolic.py:126-189).
 * Step t reads the rows from obs slot t, the commands from actions row t, and writes obs slot t + 1, rewards / terminated /
 * truncated row t; everything else (beta, time_index, bsum, ring, norm_now, norm_back, the auto-reset pools, final_obs,
 * reset_count) comes from the pdegym_bufs1d of the call and behaves as in T consecutive pdegym_*_step calls with state_in --
 * the results are bit-identical to those calls.  bufs->state_in / obs / action / reward / terminated / truncated / history are
 * ignored.  Every control / sensing combination of the reference's table (hyperbolic.py:66-124, parabolic.py:66-122):
 *   - full-state sensing: the observation slots [T + 1, B, n] hold the state (slot t in, slot t + 1 out); bufs->u is ignored.
 *     Dirichlet actuation keeps the row in registers across the T env-steps; Neumann actuation passes it through the slots;
 *   - scalar sensing (PDEGYM_SENSE_LAST / _LAST_DERIV / _FIRST_DERIV / _FIRST): the state lives in bufs->u [B, n] (required,
 *     advanced in place) and the observation slots are [T + 1, B, 1]: slot t + 1 receives the value sensed after step t
 *     (slot 0 is only read by a policy).
 * Needs float32 beta and actions, the temporal reward horizon, n <= 2048. */
typedef struct pdegym_rollout1d {
  int32_t T;                /* env-steps per call                                                              */
  int32_t reserved_;        /* bit 0: PDEGYM_ROLLOUT_FINAL_OBS_PER_STEP (bufs->final_obs is [T, B, obs_dim]; with scalar sensing
                               obs_dim == 1); other bits ignored                                               */
  float* obs;               /* [T + 1, B, n]  slot 0 = the input rows; slots 1 .. T are written                 */
  float* actions;           /* [T, B]  read; with a policy: WRITTEN (the command the policy issued, after noise and clamp) */
  float* rewards;           /* [T, B]  (may be NULL with PDEGYM_REWARD_NONE)                                   */
  uint8_t* terminated;      /* [T, B]                                                                          */
  uint8_t* truncated;       /* [T, B]                                                                          */
  /* Optional policy (HOST pointer, read during the call; see pdegym_mlp below): evaluated INSIDE the launch on observation
   * slot t -- the caller of env.step of an SB3 rollout (transport1Dppo.py:88-90) without a launch of its own.  First in_dim ==
   * the observation row (n, or 1 with scalar sensing; n <= 513), one output.  Layers of up to 64 units: the whole network must
   * fit into 160 KB of LDS next to 16 observation rows; same arithmetic as pdegym_mlp_forward except for the order of the
   * additions inside a group of 16 inputs.  With a layer of 65 .. 256 units (SB3's 256-256 actors, reactionDiffusion1Dsac.py:95)
   * the 16 waves of a workgroup evaluate the network together with pdegym_mlp_forward's own MFMA reduction, weights streamed from
   * L2: the commands equal pdegym_mlp_forward's BIT FOR BIT.  noise, when given, is [T, B] (row t, instance b at
   * noise[(t * B + b) * noise_stride]), added before the clamp. */
  const struct pdegym_mlp_s* policy;
  /* The sensing-noise hook (hyperbolic.py:160-164: the agent sees sensing_noise_func(observation)) for the policy inside the
   * launch, as noise the caller drew ahead: the policy of step t reads obs[t] + obs_noise[t]; obs itself stays clean (with
   * full-state sensing it is the plant state).  Both optional, both only with a policy:                                    */
  const float* obs_noise;   /* [T, B, obs_dim] added to observation slot t on its way into the policy                  */
  float* obs_seen;          /* [T, B, obs_dim] receives what the policy read (obs[t] + obs_noise[t]): the rollout's
                               training input                                                                          */
} pdegym_rollout1d;

int pdegym_transport_rollout(const pdegym_params1d* prm, const pdegym_bufs1d* buf, const pdegym_rollout1d* ro, int32_t B,
                             void* stream);
int pdegym_parabolic_rollout(const pdegym_params1d* prm, const pdegym_bufs1d* buf, const pdegym_rollout1d* ro, int32_t B,
                             void* stream);

/* Where mask[b] != 0 (or mask == NULL): u[b] = init[b], beta untouched, time_index = 0, bsum = |init[b,-1]|,
 * ring[b, 0] = ||init[b]|| , obs[b] = sensing(init[b]).  (hyperbolic.py:214-227) */
int pdegym_reset1d_masked(const pdegym_params1d* prm, const pdegym_bufs1d* buf, const float* init,
                          const uint8_t* mask, int32_t B, void* stream);

/* Self-test of the transport quotient: counts i where (float)((double)a[i] * rdx) != a[i] / dx (IEEE division),
 * bitwise, NaNs compared as equal.  *mismatches (device uint32) must be zeroed by the caller. */
int pdegym_selftest_quotient(const float* a, float dx, double rdx, uint32_t* mismatches, int32_t n, void* stream);

/* out[b] = ||rows[b, 0:n]||_2 */
int pdegym_rownorm2_f32(const float* rows, float* out, int32_t n, int32_t B, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Navier-Stokes 2D (collocated grid, Chorin projection, Jacobi pressure Poisson)
 * ------------------------------------------------------------------------------------------------ */
enum { PDEGYM_BC_NEUMANN = 0, PDEGYM_BC_DIRICHLET = 1, PDEGYM_BC_CONTROLLABLE = 2 };
/* edge order of apply_boundary (navier_stokes2D.py:76): lower (row 0), upper (row ny-1), left (col 0), right (col nx-1) */
enum { PDEGYM_EDGE_LOWER = 0, PDEGYM_EDGE_UPPER = 1, PDEGYM_EDGE_LEFT = 2, PDEGYM_EDGE_RIGHT = 3 };

typedef struct pdegym_params_ns2d {
  int32_t nx, ny;           /* int(round(X/dx+1)), int(round(Y/dy+1))                      base_env_2d.py:28-29 */
  int32_t nt;               /* int(round(T/dt))                                           base_env_2d.py:27 */
  int32_t iters;            /* maximum_pressure_iteration (Jacobi sweeps per step)        navier_stokes2D.py:104 */
  int32_t action_dim;       /* 1 = one scalar per instance; nx (== ny) = one value per edge node */
  int32_t bc[4][2];         /* [edge][component u,v] -> PDEGYM_BC_*                        navier_stokes2D.py:61-91 */
  double dt, dx, dy;        /* the float32 entry points cast them */
  double viscosity, density;
  double gamma;             /* NSReward(gamma)                                             ns_reward.py:15-28 */
} pdegym_params_ns2d;

/* T = float (f32 entry points) or double (f64 entry points). Fields are [B, ny, nx], row = y, col = x.  Every member needs only its
 * element's alignment, on every grid: the register-tiled kernels (64 x 64, 128 x 128, 256 x 256) move 8- and 16-byte pieces of a row
 * through accesses that are typed with the element's alignment. */
typedef struct pdegym_bufs_ns2d {
  void* u;                  /* [B, ny, nx] in/out; may be NULL (together with v) when state_in is given        */
  void* v;                  /* [B, ny, nx] in/out                                                             */
  void* p;                  /* [B, ny, nx] in/out (warm start of the next step, navier_stokes2D.py:115)        */
  void* scratch;            /* [B, 4, ny, nx] work space (u*, v*, rhs, p')                                    */
  const void* action;       /* [B, action_dim]                                                                */
  int32_t* time_index;      /* [B] in/out                                                                     */
  const void* U_ref;        /* [nt_ref, ny, nx, 2] shared reference trajectory (indexed AFTER the increment)  */
  const void* action_ref;   /* [>= nt] shared reference actions                                               */
  int32_t nt_ref;           /* rows of U_ref / action_ref (index is clamped to nt_ref-1)                       */
  void* obs;                /* [B, ny, nx, 2] out (u,v interleaved; base_env_2d.py:50)                         */
  void* reward;             /* [B] out                                                                        */
  uint8_t* terminated;      /* [B] out; truncated is always False in the reference (navier_stokes2D.py:155)    */
  void* p_out;              /* optional [B, ny, nx]: where the solved pressure of this step goes (must not alias p).  NULL = in place
                               (p is overwritten).  With it the caller ping-pongs two pressure tensors: the 256x256 pipeline
                               then needs no copy of its last pass back into p                                             */
  const void* state_in;     /* optional [B, ny, nx, 2]: the observation written by the PREVIOUS call.  When non-NULL the
                               velocity state is read from it and written only to obs (the reference's obs is the state,
                               navier_stokes2D.py:147-154), which saves one write of u and v per step; must not alias obs */
  /* Fused VecEnv auto-reset: when reset_u0 is non-NULL, an instance whose step ends terminated
   * (time_index >= nt-1, navier_stokes2D.py:159-168) restarts inside the same call, without a host round trip: its observation
   * is first copied to final_obs (if given), then (u, v, p) := pool row, time_index := 0, obs := (u0, v0).  The k-th restart of
   * instance b takes pool row (b + k*B) mod reset_pool_rows (k from reset_count, see pdegym_bufs1d). */
  const void* reset_u0;     /* optional [reset_pool_rows, ny, nx]                                                            */
  const void* reset_v0;     /* [reset_pool_rows, ny, nx]  (required with reset_u0)                                            */
  const void* reset_p0;     /* [reset_pool_rows, ny, nx]  (required with reset_u0)                                            */
  void* final_obs;          /* optional [B, ny, nx, 2]: last observation of the finished episode ("terminal_observation")    */
  int32_t* reset_count;     /* optional [B] in/out                                                                           */
  int32_t reset_pool_rows;  /* rows of the pools (0 = B)                                                                     */
  int32_t reserved_;
} pdegym_bufs_ns2d;

int pdegym_ns2d_step_f32(const pdegym_params_ns2d* prm, const pdegym_bufs_ns2d* buf, int32_t B, void* stream);
int pdegym_ns2d_step_f64(const pdegym_params_ns2d* prm, const pdegym_bufs_ns2d* buf, int32_t B, void* stream);

/* T env-steps in ONE launch for small grids (the reference's shipped 21 x 21 example; grids of 8, 11, 16, 21, 26, 31 or 32 rows and at
 * most 64 columns): the loop of env.step calls of examples/NavierStokes/NS2Dppo.py:52-66 / the forward sweeps of the adjoint example
 * (NS2Doptimization.py:74-76) with the commands given ahead.  Step t reads the state from obs slot t and the command from actions row
 * t, writes obs slot t + 1 and rewards / terminated row t; p, time_index, U_ref / action_ref, the auto-reset pools, final_obs and
 * reset_count come from the pdegym_bufs_ns2d of the call and behave as in T consecutive pdegym_ns2d_step calls with state_in (fused
 * auto-reset included; the pressure stays in bufs->p).  Observation slots, pressure, flags, time index, restart counters and rewards
 * are bit-identical to those calls, whichever kernel the step calls take.  NS rewards are bit-identical at any batch size, batch
 * position and device partition for every grid not handled by a register-tiled kernel (64 x 64 / 128 x 128 / 256 x 256): the column and
 * workgroup kernels add the squared distances in one order (per column over rows, du^2 then dv^2; then the columns in sequence).
 * bufs->u / v / state_in / obs / action / reward / terminated / p_out are ignored. */
typedef struct pdegym_rollout_ns2d {
  int32_t T;                /* env-steps per call                                                              */
  int32_t reserved_;
  void* obs;                /* [T + 1, B, ny, nx, 2]  slot 0 = the input state; slots 1 .. T are written       */
  const void* actions;      /* [T, B, action_dim]                                                             */
  void* rewards;            /* [T, B]                                                                         */
  uint8_t* terminated;      /* [T, B]                                                                         */
} pdegym_rollout_ns2d;
int pdegym_ns2d_rollout_f32(const pdegym_params_ns2d* prm, const pdegym_bufs_ns2d* buf, const pdegym_rollout_ns2d* ro, int32_t B,
                            void* stream);
int pdegym_ns2d_rollout_f64(const pdegym_params_ns2d* prm, const pdegym_bufs_ns2d* buf, const pdegym_rollout_ns2d* ro, int32_t B,
                            void* stream);

/* p_out = K Jacobi sweeps from p_in with rhs = rho/dt*(d/dx u + d/dy v)  (navier_stokes2D.py:94-116).
 * u, v, p_in, p_out: [B, ny, nx]; scratch: [B, 2, ny, nx]. p_out may alias p_in. */
int pdegym_ns2d_solve_pressure_f32(const pdegym_params_ns2d* prm, const void* u, const void* v, const void* p_in,
                                   void* p_out, void* scratch, int32_t B, void* stream);
int pdegym_ns2d_solve_pressure_f64(const pdegym_params_ns2d* prm, const void* u, const void* v, const void* p_in,
                                   void* p_out, void* scratch, int32_t B, void* stream);

/* Where mask[b] != 0 (or mask == NULL): u,v,p[b] = u0,v0,p0[b]; time_index = 0; obs[b] = (u0,v0). */
int pdegym_ns2d_reset_masked_f32(const pdegym_params_ns2d* prm, const pdegym_bufs_ns2d* buf, const void* u0,
                                 const void* v0, const void* p0, const uint8_t* mask, int32_t B, void* stream);
int pdegym_ns2d_reset_masked_f64(const pdegym_params_ns2d* prm, const pdegym_bufs_ns2d* buf, const void* u0,
                                 const void* v0, const void* p0, const uint8_t* mask, int32_t B, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Traffic ARZ 1D: Aw-Rascle-Zhang freeway model in (r, y), float64,
 * two-step Lax-Wendroff with relaxation, flux boundary control.
 *   pdegym_traffic_step          replaces TrafficPDE1D.step + terminate/truncate   environments1d/traffic_arz_env.py:103-233
 *                                + TrafficARZReward.reward                          rewards/traffic_arz_reward.py:12-22
 *   pdegym_traffic_reset_masked  replaces the state part of TrafficPDE1D.reset     traffic_arz_env.py:245-260
 * ------------------------------------------------------------------------------------------------ */
enum { PDEGYM_TRAFFIC_INLET = 0, PDEGYM_TRAFFIC_OUTLET = 1, PDEGYM_TRAFFIC_BOTH = 2, PDEGYM_TRAFFIC_OUTLET_TRAIN = 3 };
#define PDEGYM_TRAFFIC_MAX_M 1024  /* nodes per freeway (the reference notebook uses 51; up to 64 stay in registers) */

typedef struct pdegym_params_traffic {
  int32_t M;               /* len(np.arange(0, X+dx, dx))                                   traffic_arz_env.py:77-79 */
  int32_t control_freq;    /* PDE sub-steps per step() call                                  :41-42 */
  int32_t sim;             /* PDEGYM_TRAFFIC_*  (simulation_type)                            :44-57 */
  int32_t limit;           /* limit_pde_state_size                                           :124 */
  double dt, dx, T;        /* T in seconds; time advances by dt per step() (not per sub-step) :146 */
  double vm, rm, tau;      /* v_max, ro_max, relaxation time */
} pdegym_params_traffic;

typedef struct pdegym_bufs_traffic {
  double* r;               /* [B, M] density (in/out)                                                       */
  double* y;               /* [B, M] relative flow y = r (v - Veq(r)) (in/out)                              */
  const double* action;    /* [B, action_stride] inlet / outlet flux command; column 1 is used by 'both' only */
  double* time;            /* [B] simulated seconds ("time_index" of the reference) in/out                  */
  double* rs;              /* [B] steady-state density of each instance (vs, qs follow the equilibrium law); rewritten
                              for an instance that the fused auto-reset restarts (reset_rs below)                     */
  const double* qs_clip;   /* [B] qs the action bounds [0.8 qs, 1.2 qs] were built from (:97-100)           */
  double* obs;             /* [B, 2M] out: (r, v), or ((r-rs)/rs, (v-vs)/vs) for outlet-train (:227-230)    */
  double* reward;          /* [B] out                                                                       */
  uint8_t* done;           /* [B] out: terminate() or reward > -0.00023 (:230)                              */
  uint8_t* truncated;      /* [B] out                                                                       */
  int32_t action_stride;   /* elements between the commands of consecutive instances: 2 (or 0 = 2), or 1 for the
                              single-command simulation types (the caller's [B] / [B,1] tensor is used as it is)      */
  int32_t reserved_;
  /* Fused VecEnv auto-reset (as for the 1D and NS engines): when reset_rs is non-NULL, an
   * instance whose step ends done | truncated restarts INSIDE the same launch the way TrafficPDE1D.reset does
   * (traffic_arz_env.py:245-260): its observation goes to final_obs (if given), then rs[b] := reset_rs[(b + k*B) mod
   * reset_pool_rows] (k from reset_count: the reference redraws the steady state in 'outlet-train'), r = rs * profile,
   * y = qs - vm r + vm/rm r^2, time = 0, and obs[b] is the first observation (r, v) of the new episode.  done / truncated /
   * reward still report the finished step.  qs_clip (the construction-time action bounds) is left alone. */
  const double* reset_rs;      /* optional [reset_pool_rows] steady-state densities of the coming episodes              */
  const double* reset_profile; /* [M] sin(3 x/L pi)*0.1 + 1 as for pdegym_traffic_reset_masked (required with reset_rs)  */
  double* final_obs;           /* optional [B, 2M]: last observation of the finished episode ("terminal_observation");
                                  [T, B, 2M] in a rollout call with PDEGYM_ROLLOUT_FINAL_OBS_PER_STEP                    */
  int32_t* reset_count;        /* optional [B] in/out: restarts so far; NULL = always pool row b mod reset_pool_rows     */
  int32_t reset_pool_rows;     /* rows of reset_rs (0 = B)                                                              */
  int32_t reserved2_;
} pdegym_bufs_traffic;

int pdegym_traffic_step(const pdegym_params_traffic* prm, const pdegym_bufs_traffic* buf, int32_t B, void* stream);

/* T env-steps in ONE launch (M <= 64; T x traffic_arz_env.py:131-233, the loop of the reference's "RL control" notebook):
 * step t takes the command(s) from actions row t and writes observation slot t + 1,
 * rewards / done / truncated row t; r, y, time of the pdegym_bufs_traffic are read once and written back at the end
 * (bufs->action / obs / reward / done / truncated are ignored).  Bit-identical to T pdegym_traffic_step calls; like them it
 * keeps stepping a finished episode.  With a policy (HOST pointer; layers of <= 256 units -- more than 64: evaluated cooperatively with
 * pdegym_mlp_forward's MFMA reduction, see pdegym_rollout1d.policy --, 2M inputs, action_stride outputs)
 * the command of step t is computed inside the launch from observation slot t (slot 0 = the caller's current observation)
 * rounded to float32, plus noise [T, B, action_stride] (row stride noise_stride), clamped, widened and stored to actions. */
typedef struct pdegym_rollout_traffic {
  int32_t T;
  int32_t reserved_;        /* bit 0: PDEGYM_ROLLOUT_FINAL_OBS_PER_STEP (bufs->final_obs is double [T, B, 2M]); other bits ignored;
                               pdegym_traffic_backstep_rollout takes it too                                     */
  double* obs;              /* [T + 1, B, 2M]  slot 0 is read only by a policy; slots 1 .. T are written         */
  double* actions;          /* [T, B, action_stride]  read, or written when a policy is given                   */
  double* rewards;          /* [T, B]                                                                          */
  uint8_t* done;            /* [T, B]                                                                          */
  uint8_t* truncated;       /* [T, B]                                                                          */
  const struct pdegym_mlp_s* policy;
} pdegym_rollout_traffic;

int pdegym_traffic_rollout(const pdegym_params_traffic* prm, const pdegym_bufs_traffic* buf, const pdegym_rollout_traffic* ro,
                           int32_t B, void* stream);
/* Where mask[b] != 0 (or mask == NULL): rs[b] is taken as given, r = rs*profile, y = qs - vm r + vm/rm r^2, time = 0,
 * obs = (r, v).  profile[M] = sin(3 x/L pi)*0.1 + 1 is computed by the caller in NumPy (libm sin, bit parity). */
int pdegym_traffic_reset_masked(const pdegym_params_traffic* prm, const pdegym_bufs_traffic* buf, const double* profile,
                                const uint8_t* mask, int32_t B, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Brain tumour 1D (float64) -- SURVEY.md section 8f rank 3
 *
 *   pdegym_tumor_step          replaces BrainTumor1D.step + _update_fd + _compute_radiation_field + getTumorRadius
 *                              + terminate/truncate                               environments1d/brain_tumor_env.py:106-352
 *                              + BrainTumorReward.reward                          rewards/brain_tumor_reward.py:30-73
 *   pdegym_tumor_reset_masked  replaces the state part of BrainTumor1D.reset      brain_tumor_env.py:354-384
 * ------------------------------------------------------------------------------------------------------------------ */
enum { PDEGYM_TUMOR_GROWTH = 0, PDEGYM_TUMOR_THERAPY = 1, PDEGYM_TUMOR_POST = 2 };   /* "Growth" / "Therapy" / "Post-Therapy" */
enum { PDEGYM_TUMOR_DAY_GROWTH = 0, PDEGYM_TUMOR_DAY_THERAPY = 1, PDEGYM_TUMOR_DAY_POST = 2, PDEGYM_TUMOR_DAY_SIM = 3,
       PDEGYM_TUMOR_DAY_DEATH = 4, PDEGYM_TUMOR_DAYS = 5 };
enum { PDEGYM_TUMOR_OUT_T1 = 0, PDEGYM_TUMOR_OUT_T2 = 1, PDEGYM_TUMOR_OUT_TREAT = 2, PDEGYM_TUMOR_OUT_DOSE = 3,
       PDEGYM_TUMOR_OUTS = 4 };

typedef struct pdegym_params_tumor {
  int32_t nx;              /* int(round(X/dx)+1)                                             brain_tumor_env.py:51 */
  int32_t nt;              /* int(round(T/dt)+1)                                             base_env_1d.py:23 */
  double dt, dx, dx2;      /* dx2 = dx**2 as the caller's Python evaluates it                :226 */
  double D, rho, alpha, alpha_beta_ratio, k;
  double thr_t1, thr_t2;   /* detection_threshold * k  (caller's double product)             :114 */
  double detect_radius;    /* t1_detection_radius: Growth -> Therapy                          :151 */
  double death_radius;     /* t1_death_radius: truncation                                    :327 */
  double total_dosage, dose_end;   /* total_dosage, dosage_termination_threshold             :159, :171 */
  double margin;           /* 25 (mm) added to the T2 radius for the treated region          :257 */
} pdegym_params_tumor;

typedef struct pdegym_bufs_tumor {
  double* u;               /* [B, nx] live density row, updated in place (it IS the observation)               */
  const double* xscale;    /* [nx] np.linspace(0, X, nx) from the caller                                  :56 */
  const double* control;   /* [B] proportion of total_dosage requested this day (used in Therapy only)         */
  const double* kill;      /* [B] or NULL: 1 - exp(-alpha*BED) precomputed by the caller (bit parity with
                              NumPy's exp); NULL = the kernel evaluates exp itself (<= 1 ulp apart)   :260-262 */
  int32_t* time_index;     /* [B] in/out                                                                       */
  int32_t* stage;          /* [B] in/out PDEGYM_TUMOR_*                                                        */
  double* remaining;       /* [B] in/out remaining_dosage                                                      */
  int32_t* days;           /* [B, 5] in/out growthDays, therapyDays, postTherapyDays, simulationDays, cDeathDay (-1 = None) */
  const double* t_benchmark; /* [B] NaN = not set (reward 0)                                                   */
  double* reward;          /* [B] out                                                                          */
  uint8_t* terminated;     /* [B] out                                                                          */
  uint8_t* truncated;      /* [B] out                                                                          */
  double* out;             /* [B, 4] out: T1 radius and T2 radius of the new row (NaN = invisible), treatment radius and
                              applied dose of this step (0 outside Therapy)                                    */
  const uint8_t* active;   /* [B] or NULL: instances with active[b] == 0 are left untouched (no output is written)    */
  double* history;         /* [B, nt, nx] or NULL: the row of every simulated day t is stored at [b, t] (env.u)   :143 */
  double* t1_log;          /* [B, nt] or NULL: T1 radius / dx of every simulated day (t1_radius_idx_vs_time) :271-273  */
} pdegym_bufs_tumor;

/* Runs of days inside one launch (the loops of TherapyWrapper, brain_tumor_env.py:385-505) */
enum {
  PDEGYM_TUMOR_RUN_ONE_DAY = 0, /* == pdegym_tumor_step                                                                 */
  PDEGYM_TUMOR_RUN_GROWTH = 1,  /* instances in Growth: step(0) until the stage changes or the episode ends  :409-428   */
  PDEGYM_TUMOR_RUN_POST = 2,    /* instances in Post-Therapy: step(0) until terminated or truncated          :437-446   */
  PDEGYM_TUMOR_RUN_TO_END = 3   /* every live instance: step(0) until terminated or truncated (benchmark())  :488-503   */
};

/* One day per call.  nx <= 4096.  An active instance with time_index >= nt-1 (its episode is over) keeps its state and out[b];
 * the call writes reward[b] = 0, terminated[b] = truncated[b] = 0 for it.
 * Where the reference raises: a Therapy day on which the tumour is invisible on T2 has treatment radius 0, and the reference's toxicity
 * reward evaluates 0.0 ** -0.685 (brain_tumor_reward.py:63, ZeroDivisionError) -- reached e.g. the day after a NaN or -Inf dosage, which
 * turns the whole treated region into NaN.  The kernel cannot raise: it advances the state, the counters and the flags as on any day
 * (nothing is irradiated), reports out[b] treatment radius 0 and T2 NaN, and returns reward[b] = NaN (116 * 0^-0.685 = +Inf makes the
 * dose ratio Inf / Inf).  Other instances of the batch are not affected.  (The CPU double of the tests raises, like the reference.) */
int pdegym_tumor_step(const pdegym_params_tumor* prm, const pdegym_bufs_tumor* buf, int32_t B, void* stream);
/* Up to max_days days per participating instance inside ONE launch (row and stage machine stay on chip between days);
 * control is 0 on every day of modes 1-3; reward / flags / out are those of the LAST simulated day; instances that do not
 * take part (wrong stage, inactive, or past nt-1) are left untouched.  kill is only honoured by RUN_ONE_DAY. */
int pdegym_tumor_advance(const pdegym_params_tumor* prm, const pdegym_bufs_tumor* buf, int32_t mode, int32_t max_days,
                         int32_t B, void* stream);
/* Where mask[b] != 0 (or mask == NULL): u = init (init_stride = 0 broadcasts one row), time_index = 0, stage = Growth,
 * remaining = total_dosage, days = (0,0,0,0,-1). */
int pdegym_tumor_reset_masked(const pdegym_params_tumor* prm, const pdegym_bufs_tumor* buf, const double* init,
                              int64_t init_stride, const uint8_t* mask, int32_t B, void* stream);

/* ---- TherapyWrapper(BrainTumor1D) for every patient: one wrapper step, or T of them with the policy inside, in ONE launch
 * (brain_tumor_env.py:385-505; the notebook's PPO("MlpPolicy", TherapyWrapper(gym.make("PDEControlGym-BrainTumor1D")))).
 * The wrapper's own state, per patient; in/out arrays are read once and written once per launch.                           */
typedef struct pdegym_wrap_tumor {
  int32_t weekends;                     /* nonzero: two untreated days after five consecutive treatment days      :458-472 */
  int32_t reserved_;
  const double* init;                   /* initial row(s) a finished patient restarts from                        :409-428 */
  int64_t init_stride;                  /* doubles between the rows of consecutive patients: 0 = one shared [nx] row, nx = [B, nx] */
  int32_t* consecutive;                 /* [B] in/out consecutive treatment days (used with weekends; 0 after a restart)   */
  int64_t* treatment_calls;             /* [B] in/out Therapy-stage wrapper steps                                          */
  int64_t* soft_constraint_violations;  /* [B] in/out Therapy-stage wrapper steps whose reward was negative                */
  double* final_obs;                    /* [B, nx] or NULL: the last row of an episode that ended in this launch (rows of
                                           other patients are left untouched); [T, B, nx] in a pdegym_tumor_rollout call with
                                           PDEGYM_ROLLOUT_FINAL_OBS_PER_STEP                                               */
  double* obs;                          /* pdegym_tumor_therapy_step only: [B, nx] receives the returned observation, or NULL:
                                           the observation is buf->u (not with weekends)                                   */
} pdegym_wrap_tumor;

/* One wrapper step (TherapyWrapper.step, brain_tumor_env.py:385-505) of every patient in one launch, per patient in this order:
 *  1. stage Post-Therapy: days with control 0 until terminated or truncated; reward / flags / out of the last simulated day.
 *  2. stage Therapy: one day with buf->control[b] (the kill fraction is evaluated in the kernel: buf->kill is ignored, as are
 *     buf->active and the launch's days are not recorded: history / t1_log must be NULL); treatment_calls += 1,
 *     soft_constraint_violations += (reward < 0).  With weekends: consecutive = control > 0 ? consecutive + 1 : 0; if it reaches 5 and
 *     the day did not end the episode, consecutive = 0 and two more days with control 0 follow (each as pdegym_tumor_step: none once
 *     time_index has reached nt-1); the state, the day counters and out keep them, reward and flags stay the treatment day's.
 *  3. terminated | truncated: the live row goes to final_obs, the patient restarts from init (pdegym_tumor_reset_masked),
 *     consecutive = 0, and the growth stage runs until the stage changes or the episode ends (PDEGYM_TUMOR_RUN_GROWTH).
 *  4. the observation is the live row -- for a patient that took weekend days and is not finished: the treatment day's row.
 * A patient found in Growth (its growth run hit the time limit) is outside the wrapper's contract: reward 0, no flag, state
 * untouched.  A patient past its last day (time_index >= nt-1) simulates nothing: Therapy reports reward 0 and no flag, Post-Therapy
 * reports buf->reward / terminated / truncated as it found them.
 * buf->reward / terminated / truncated receive the step's reported values (before the restart), buf->out the last simulated day's.
 * Bit-identical to the launches TumorVecEnv.step_tensor composes the step from.                                                  */
int pdegym_tumor_therapy_step(const pdegym_params_tumor* prm, const pdegym_bufs_tumor* buf, const pdegym_wrap_tumor* wrap, int32_t B,
                              void* stream);

/* T wrapper steps (brain_tumor_env.py:385-505, the loop SB3 runs around TherapyWrapper.step) in ONE launch: step t takes the command
 * from actions row t and writes observation slot t + 1, rewards / terminated / truncated row t; the state, the wrapper's counters
 * and the engine's [B] outputs are read once and written back at the end (reward / terminated / truncated: the last step's;
 * buf->control and wrap->obs are ignored).  Bit-identical to T pdegym_tumor_therapy_step calls.  With a policy (HOST pointer;
 * nx inputs, one output; layers of <= 256 units -- more than 64: evaluated cooperatively with pdegym_mlp_forward's MFMA reduction,
 * bit-identical to it, see pdegym_rollout1d.policy) the command of step t is computed inside the launch from observation slot t
 * (slot 0 = the caller's current observation) rounded to float32, plus noise [T, B] (row stride noise_stride), clamped, widened
 * and stored to actions -- the contract of pdegym_rollout_traffic.policy.  The policy's LDS plus two float64 rows for each of the
 * workgroup's 16 patients must fit into 160 KB (nx = 201: a 64-64 actor and a 256-256 actor both fit); history / t1_log recording
 * is refused.                                                                                                                     */
typedef struct pdegym_rollout_tumor {
  int32_t T;
  int32_t reserved_;        /* bit 0: PDEGYM_ROLLOUT_FINAL_OBS_PER_STEP (wrap->final_obs is [T, B, nx]); other bits ignored */
  double* obs;              /* [T + 1, B, nx]  slot 0 is read only by a policy; slots 1 .. T are written        */
  double* actions;          /* [T, B]  read, or written when a policy is given                                  */
  double* rewards;          /* [T, B]                                                                           */
  uint8_t* terminated;      /* [T, B]                                                                           */
  uint8_t* truncated;       /* [T, B]                                                                           */
  const struct pdegym_mlp_s* policy;
} pdegym_rollout_tumor;

int pdegym_tumor_rollout(const pdegym_params_tumor* prm, const pdegym_bufs_tumor* buf, const pdegym_wrap_tumor* wrap,
                         const pdegym_rollout_tumor* ro, int32_t B, void* stream);

/* ---- policy network on the device (the caller of env.step inside an on-device rollout) ------------------------------
 * The reference evaluates an SB3 "MlpPolicy" (two hidden layers of 64 tanh units by default) between two env.step calls:
 * model = PPO("MlpPolicy", env) / model.predict(obs), examples/transportPDE/transport1Dppo.py:88-90 and
 * transport1DtestAlgorithm.py (the RL controllers).  pdegym_mlp_forward evaluates such a network for B observation rows
 * in ONE launch (float32; weights in a blocked transpose of torch.nn.Linear.weight W[out_dim, in_dim]:
 * w[(k / 4) * out_dim * 4 + n * 4 + k % 4] = W[n][k], zero-padded to a multiple of four k, 16-byte aligned -- one 16-byte
 * load per lane brings four consecutive inputs of its neuron and a wave's load is contiguous; a layer whose w is not 16-byte aligned
 * is refused with -2, by pdegym_mlp_forward, pdegym_mlp_backward and every rollout that takes the network as its policy; x, y, b
 * and noise need only their element's alignment), optionally clamping the
 * output to the action box, so that policy + step + auto-reset of a rollout are two launches per env-step.
 * Summation order is k ascending with the bias added last (not a BLAS order): float32-rounding agreement with torch. */
#define PDEGYM_MLP_MAX_LAYERS 4
#define PDEGYM_MLP_MAX_WIDTH 256   /* widest layer output                          */
#define PDEGYM_MLP_MAX_INPUT 8192  /* widest observation row (first layer in_dim)  */
enum { PDEGYM_MLP_IDENTITY = 0, PDEGYM_MLP_TANH = 1, PDEGYM_MLP_RELU = 2 };

typedef struct {
  const float* w;      /* [ceil(in_dim / 4), out_dim, 4] blocked transpose, see above; 16-BYTE ALIGNED (else -2) */
  const float* b;      /* [out_dim] or NULL                                         */
  int32_t in_dim, out_dim;
  int32_t act;         /* PDEGYM_MLP_* applied to this layer's output               */
  int32_t reserved_;
} pdegym_mlp_layer;

typedef struct pdegym_mlp_s {
  int32_t n_layers;    /* 1 .. PDEGYM_MLP_MAX_LAYERS                                 */
  int32_t clamp;       /* nonzero: the last layer's output is clamped to [lo, hi]   */
  float lo, hi;
  int32_t x_f64;       /* nonzero: x holds float64 rows (TrafficPDE1D, BrainTumor1D, float64 NavierStokes2D observations),
                          rounded to float32 as they are read -- what SB3 does before it evaluates its policy           */
  int32_t y_f64;       /* nonzero: y receives float64 (the float32 result widened: those environments' action dtype)   */
  const float* noise;  /* [B, out_dim] float32 or NULL: added to the last layer's output before the clamp -- the exploration
                          noise of a stochastic policy (SB3's Gaussian MlpPolicy samples mean + std * eps), drawn by the caller */
  int64_t noise_stride; /* floats between consecutive rows of noise                                                     */
  /* The head's fields (ABI 21) occupy the reserved words of layer[0], layer[1] and layer[2]: the descriptor keeps the size and every
   * offset of ABI 20 (168 bytes, layer[] at 40), and a zero-initialised descriptor means the plain head.                          */
  union {
    pdegym_mlp_layer layer[PDEGYM_MLP_MAX_LAYERS];
    struct {
      char in_layer0_[28];
      int32_t head;        /* PDEGYM_MLP_HEAD_*: what becomes of the last layer's output (0: PLAIN)                              */
      char in_layer1_[28];
      float log_std_min;   /* SQUASHED_GAUSSIAN: the clip of log_std (SB3's SAC: -20, 2), min <= max                             */
      char in_layer2_[28];
      float log_std_max;
    };
  };
} pdegym_mlp;

/* The head.  PLAIN: y = clamp(last layer + noise), as described at the fields above.
 * SQUASHED_GAUSSIAN: the actor SB3's SAC samples while it learns, a = tanh(mu(s) + exp(clip(log_std(s), min, max)) * eps), rescaled
 * from [-1, 1] to the action box.  The last layer has 2A outputs and the IDENTITY activation: neurons 0 .. A-1 are mu, neurons
 * A .. 2A-1 are log_std (the rows [mu; log_std] of the two torch.nn.Linear heads, one above the other).  y, the actions of a rollout
 * and noise have A columns; noise holds STANDARD-NORMAL draws eps (not pre-scaled noise: the standard deviation depends on the state),
 * noise_stride >= A.  clamp must be set with lo < hi -- the action box -- and log_std_min <= log_std_max; anything else is -2.
 * pdegym_mlp_forward takes A <= 8 (mu and log_std of a row then sit in one row of 16 lanes of the matrix-core result, one DPP row shift
 * apart); the rollout kernels take their own A (1, or 2 for two-command traffic).  Arithmetic, per output, float32, every operation
 * rounded on its own (no fused multiply-add), in the order of SB3's torch ops -- expf and tanhf are the only places where the result
 * can differ from torch float32:
 *     s = clip_keep_nan(log_std, log_std_min, log_std_max)
 *     z = noise ? mu + (expf(s) * eps) : mu            noise == NULL: the deterministic actor; log_std is not looked at at all
 *     u = tanhf(z)
 *     c = lo + ((0.5f * (u + 1.0f)) * (hi - lo))       SB3's unscale_action, in its order
 *     c = clip_keep_nan(c, lo, hi)                     the box contract survives the last rounding
 * One device function (pdegym_mlp_tile.h: squashed_gaussian) serves pdegym_mlp_forward and both evaluators inside the rollout
 * kernels: equal pre-activations give equal bits everywhere.  Non-finite data (conventions above): a NaN in mu, or with noise a NaN
 * in log_std or in eps, gives a NaN command; mu = -Inf gives lo, mu = +Inf gives lo + (hi - lo) clipped to the box (hi itself
 * whenever that sum is exact, e.g. for dyadic bounds; otherwise within one rounding of it); log_std = +-Inf is clipped like any
 * other value; eps = +-Inf gives hi / lo (NaN when sigma underflowed to 0: 0 * Inf).  A replay buffer that stores SB3's scaled
 * action recovers it as 2 (c - lo) / (hi - lo) - 1.  Log-probabilities are not computed (SAC recomputes them under autograd). */
enum { PDEGYM_MLP_HEAD_PLAIN = 0, PDEGYM_MLP_HEAD_SQUASHED_GAUSSIAN = 1 };

/* y[b, :] = net(x[b, :]) for b < B; x_stride / y_stride = ELEMENTS between consecutive rows (>= the row lengths). */
int pdegym_mlp_forward(const pdegym_mlp* net, const void* x, int64_t x_stride, void* y, int64_t y_stride, int32_t B,
                       void* stream);

/* The same launch on the LIVE rows only: row r is live when rows[r] != 0 and (rows_not == NULL or rows_not[r] == 0) -- e.g.
 * rows = truncated, rows_not = terminated of a rollout, x = its terminal observations: SB3's V(terminal_observation) where
 * infos[i]["TimeLimit.truncated"], with no compaction, no allocation and no synchronisation (the call can be captured in a graph).
 * rows (required, else -1) and rows_not are uint8 [B] device arrays.  y is stored for live rows only: dead rows of y are NOT
 * touched.  A live row carries the BITS of pdegym_mlp_forward on the same row (the rows of a 16-row tile are independent in the
 * matrix-core reduction), whatever the dead rows of x hold -- NaN included.  A workgroup whose 16 rows are all dead returns
 * before it loads a weight.  Plain head only (head == PLAIN, else -2), noise == NULL (else -2); float32 or float64 x (x_f64),
 * float32 y (y_f64 is refused); clamp as in pdegym_mlp_forward; both tile plans (layers of <= 64 and of <= 256 units). */
int pdegym_mlp_forward_masked(const pdegym_mlp* net, const void* x, int64_t x_stride, void* y, int64_t y_stride, const uint8_t* rows,
                              const uint8_t* rows_not, int32_t B, void* stream);

/* ---- backward pass of the same network (the gradient step of the reference's PPO / SAC training scripts) ------------------------
 * Given dy = dLoss/dy [B, out_dim], pdegym_mlp_backward writes dLoss/dW and dLoss/db of every layer, and optionally dLoss/dx, in three
 * launches whatever the number of layers (csrc/pdegym_mlp_backward.hip).  Nothing is saved by the forward launch: the activations are
 * recomputed from `net` (its blocked weights and biases) with the forward kernel's own reduction, hence with its bits.
 *
 * net      the forward descriptor, with head == PLAIN, clamp == 0 and noise == NULL (a clamp or a squashed-Gaussian head is the
 *          caller's to differentiate); x_f64 is allowed -- rows are rounded to float32 as they are read -- and y_f64 is ignored.
 * Limits   n_layers <= PDEGYM_MLP_MAX_LAYERS, every layer's out_dim <= 64, the first layer's in_dim <= 1024; anything else is -2.
 *          (SB3's PPO default [64, 64] and every observation row of the five families fit; 256-unit layers do not.)
 * Inputs   x [B, in_dim] (x_stride), dy [B, out_dim] float32 (dy_stride), w[l] = the ROW-MAJOR [out_dim, in_dim] float32 weights of
 *          layer l -- torch.nn.Linear.weight's own storage: dH = dZ W reduces over it with `in` contiguous, and no second blocked
 *          copy can go stale.  w[0] is needed only with dx.  Strides are ELEMENTS between rows (>= the row lengths).
 * Outputs  dw[l] [out_dim, in_dim] float32 contiguous (torch layout), WRITTEN, not accumulated; db[l] [out_dim], NULL exactly where the
 *          layer has no bias; dx [B, in_dim] float32 (dx_stride) or NULL -- only with float32 x.  Rows >= B are not touched.
 * slabs    the B rows are cut into ceil(B / 16) tiles of 16 rows and the tiles into `slabs` runs of consecutive tiles (slab s: tiles
 *          floor(s tiles / slabs) .. floor((s + 1) tiles / slabs) - 1); a slab's partial sums are formed rows ascending and the slabs'
 *          partials are added in ascending order.  0: the library's choice, min(tiles, 256) -- a function of B alone.
 *          1 <= slabs <= tiles otherwise.
 * workspace  device memory of at least pdegym_mlp_backward_workspace (net, B, slabs) bytes, 4-byte aligned (else -2); every byte that
 *          is read was written by the same call.  net->layer[l].w: 16-byte aligned, as for pdegym_mlp_forward (else -2, from
 *          pdegym_mlp_backward_workspace as well: the size query checks the same descriptor).
 * Arithmetic  float32 throughout.  Activation derivatives as torch's backward ops, each operation rounded on its own:
 *          tanh dz = dh * (1 - h * h); ReLU dz = (h <= 0) ? 0 : dh (a NaN activation passes the gradient, as threshold_backward).
 *          The three products dW_l = dZ_l^T H_{l-1} (over rows), db_l = sum_rows dZ_l and dH_{l-1} = dZ_l W_l (over the layer's units) run
 *          on v_mfma_f32_16x16x4_f32, an exact fmaf chain: the order of every sum is fixed by the code.
 * Determinism  no floating-point atomics; every output bit is a function of the inputs, B and slabs alone -- not of the stream, of
 *          earlier calls or of what the workspace held.  Rows >= B of the last tile are never read and contribute nothing (they are
 *          selected to zero, not multiplied by it).
 * Non-finite data propagates as IEEE makes it: a NaN in row i of x or dy reaches dx[i] and the weight gradients, and no other row of dx.
 * Errors: -1 null descriptor / arguments; -2 a limit above, B < 1, a stride shorter than its row, slabs out of range, a workspace that
 * is too small or not 4-byte aligned, blocked weights that are not 16-byte aligned, dx with x_f64; -3 a required pointer is NULL, db that does not match the layer's bias, or an output (the workspace
 * included) that overlaps an input or another output as byte ranges. */
typedef struct pdegym_mlp_backward_args {
  const void* x;
  int64_t x_stride;
  const float* dy;
  int64_t dy_stride;
  const float* w[PDEGYM_MLP_MAX_LAYERS];
  float* dw[PDEGYM_MLP_MAX_LAYERS];
  float* db[PDEGYM_MLP_MAX_LAYERS];
  float* dx;
  int64_t dx_stride;
  int32_t slabs;
  int32_t reserved_;
  void* workspace;
  int64_t workspace_bytes;
} pdegym_mlp_backward_args;
/* bytes of workspace for B rows and `slabs` (0: the library's choice), or a negative code */
int64_t pdegym_mlp_backward_workspace(const pdegym_mlp* net, int32_t B, int32_t slabs);
int pdegym_mlp_backward(const pdegym_mlp* net, const pdegym_mlp_backward_args* a, int32_t B, void* stream);

/* ---- the same backward pass for layers of up to 256 units (Stable-Baselines3's SAC networks: actor and critics of 256-256 ReLU) ---
 * pdegym_mlp_backward_wide takes the descriptor and the argument structure of pdegym_mlp_backward and gives the same gradients under
 * the same contract (csrc/pdegym_mlp_backward_wide.hip, three launches whatever the number of layers); only what differs is said here.
 *
 * Limits   n_layers <= PDEGYM_MLP_MAX_LAYERS, every layer's out_dim <= PDEGYM_MLP_MAX_WIDTH (256), the first layer's in_dim <= 1024;
 *          anything else is -2.  A superset of pdegym_mlp_backward's domain: narrow networks are taken too.
 * Launches 1. tiles: a workgroup of 16 waves per tile of 16 rows recomputes every layer's activations (the forward kernel's reduction
 *          and bits), forms dZ_l in place, stores dZ_l and H_{l-1} (l >= 1; H_{-1} is x itself) in the workspace and forms
 *          dH_{l-1} = dZ_l W_l, dx for the first layer.  2. accumulation: per (layer, 64 units, 64 inputs, slab) the partial
 *          dZ_l^T H_{l-1} of the slab's rows, and db_l from the same dZ_l.  3. the slabs' partials added in ascending order.
 * Order of every sum: the one stated above.  dW_l, db_l: rows ascending within a slab (four MFMAs per tile of 16 rows), slabs
 *          ascending.  dH_{l-1}: the layer's units in blocks of 16, ascending, in ONE accumulator chain (a 256-unit layer: 16 blocks).
 *          Hence on a network both entry points take, with the same explicit `slabs`, both return IDENTICAL BITS in dw, db and dx.
 * slabs    as above; 0: this entry's own choice, min(ceil(tiles / 8), 64) with tiles = ceil(B / 16) -- a function of B alone.  A
 *          slab costs one write and one read of every partial (83 000 floats for a 66-256-256-1 critic, against 4 500 for the
 *          66-64-64-1 one), so slabs hold at least 8 tiles (128 rows: the accumulation then reads 128 x (in + out) floats per
 *          64 x 64 partial it writes) and there are at most 64 of them (B = 32768: 21 MB of partials for that critic).
 * workspace  at least pdegym_mlp_backward_wide_workspace (net, B, slabs) bytes, 4-byte aligned (else -2):
 *          16 tiles x sum_l (pad64(out_l) + [l >= 1] pad64(in_l)) floats of dZ_l / H_{l-1}, then slabs x sum_l out_l (in_l + 1)
 *          floats of partials (pad64: rounded up to a multiple of 64).  Every byte that is read was written by the same call.
 * Determinism, non-finite data, rows >= B, alignment (blocked weights 16 bytes, everything else its element's) and every error
 * code: as for pdegym_mlp_backward; -4 when the tile kernel's 130 KB of LDS cannot be granted (a compute unit of CDNA4 holds 160 KB).  No
 * floating-point atomics, tickets or fences: stream order is the only synchronisation between the three launches. */
int64_t pdegym_mlp_backward_wide_workspace(const pdegym_mlp* net, int32_t B, int32_t slabs);
int pdegym_mlp_backward_wide(const pdegym_mlp* net, const pdegym_mlp_backward_args* a, int32_t B, void* stream);

/* ---- the critic(obs, action) call: rows in two parts, gradient to the action part alone, parameter gradients on request ----------
 * SB3's critics are called as critic(obs, actions) (stable_baselines3/common/policies.py: ContinuousCritic.forward concatenates the
 * two and evaluates its q-networks).  The three entry points below take the two arrays as they are: no [obs | action] block is
 * written, and the actor step of a SAC update -- which wants dQ/d(action) and nothing else -- pays for neither the first D columns
 * of dx nor the parameter gradients.  They launch the kernels of the entry points they shadow (new instantiations: no new kernel).
 *
 * Row      row b of the first layer's input is [ x[b, 0 .. D) | x2[b, 0 .. n2) ] with D = net->layer[0].in_dim - n2 >= 1 and
 *          1 <= n2 <= 8 (the action limit of the heads; the two backward entry points also take n2 == 0, the plain row, with x2 and
 *          dx2 NULL).  x: float32, or float64 with net->x_f64, rounded as it is read; x2: always float32.  Strides in ELEMENTS:
 *          x_stride >= D, x2_stride >= n2.  x, x2, dx, dx2 need their element's alignment, the blocked weights 16 bytes.
 * Limits   those of the shadowed entry point: in_dim = D + n2 <= PDEGYM_MLP_MAX_INPUT for the forward, <= 1024 for the backward
 *          passes; 64 units per layer for pdegym_mlp_backward_cat, 256 for pdegym_mlp_backward_wide_cat; up to 4 layers.
 * Bits     y, dw, db, dx and dx2 equal, BIT FOR BIT, y, dw, db, dx[:, :D] and dx[:, D:] of pdegym_mlp_forward / pdegym_mlp_backward /
 *          pdegym_mlp_backward_wide on the materialised rows with the same `slabs`: the same operands meet the same accumulator chains.
 * Forward  every head, clamp and noise option of pdegym_mlp_forward; one launch.
 * Backward pdegym_mlp_backward_cat_args holds the fields of pdegym_mlp_backward_args and the second part.  dx is the gradient of the
 *          FIRST D columns, [B, D] (dx_stride >= D) or NULL, only with float32 x; dx2 that of the tail, [B, n2] (dx2_stride >= n2) or
 *          NULL.  params != 0: the three launches, the workspace and the slabs of the shadowed pass; dw and db are written.
 *          params == 0: the input gradient alone in ONE launch -- the tile kernel instantiated without the dW / db products, without
 *          their partial stores and without the dZ / H workspace traffic of the wide pass.  dw[] and db[] must all be NULL (else -2),
 *          workspace may be NULL, slabs is ignored, and at least one of dx and dx2 is required (else -3).  dx and dx2 carry the bits
 *          of params != 0: dH = dZ W runs over the units in blocks of 16 in one chain, whatever the slabs.  With dx == NULL only the
 *          16-column blocks of dZ_0 W_0 that meet the tail are formed (with dx2 == NULL only those that meet the first part).
 * Rows >= B of the last tile are never read from x or x2 and never written to dx or dx2 (selected to zero, not multiplied by it).
 * Non-finite data: a NaN in x2[i] reaches row i of y, dx, dx2 and the weight gradients, and no other row of y, dx or dx2.
 * Errors   as the shadowed entry points: -1 null descriptor / arguments; -2 a limit, n2 out of range or not below in_dim, a stride
 *          shorter than its row, dx with x_f64, dw / db given with params == 0, dx2 given with n2 == 0, and everything the shadowed
 *          pass answers -2 to; -3 a required pointer is NULL (x, x2 with n2 >= 1, y / dy, with params != 0 dw, db of a layer with
 *          bias and the workspace, with params == 0 both of dx and dx2), or an output (dx2 and the workspace included) that
 *          overlaps an input (x2 included) or another output as byte ranges. */
int pdegym_mlp_forward_cat(const pdegym_mlp* net, const void* x, int64_t x_stride, const float* x2, int64_t x2_stride, int32_t n2,
                           void* y, int64_t y_stride, int32_t B, void* stream);

typedef struct pdegym_mlp_backward_cat_args {
  const void* x;       /* [B, D], D = in_dim - n2 */
  int64_t x_stride;
  const float* dy;
  int64_t dy_stride;
  const float* w[PDEGYM_MLP_MAX_LAYERS];
  float* dw[PDEGYM_MLP_MAX_LAYERS];
  float* db[PDEGYM_MLP_MAX_LAYERS];
  float* dx;           /* [B, D] or NULL */
  int64_t dx_stride;
  int32_t slabs;
  int32_t params;      /* 0: dx / dx2 alone, one launch */
  void* workspace;
  int64_t workspace_bytes;
  const float* x2;     /* [B, n2] float32 */
  int64_t x2_stride;
  float* dx2;          /* [B, n2] or NULL */
  int64_t dx2_stride;
  int32_t n2;          /* 0 .. 8 */
  int32_t reserved_;
} pdegym_mlp_backward_cat_args;
/* (the workspace of params != 0 is that of pdegym_mlp_backward_workspace / pdegym_mlp_backward_wide_workspace) */
int pdegym_mlp_backward_cat(const pdegym_mlp* net, const pdegym_mlp_backward_cat_args* a, int32_t B, void* stream);
int pdegym_mlp_backward_wide_cat(const pdegym_mlp* net, const pdegym_mlp_backward_cat_args* a, int32_t B, void* stream);

/* ---- rows by index: the networks read a minibatch out of a storage in place, no [N, D] copy of the rows ------------------------------
 * A replay buffer (pde_control_gym.DeviceReplayBuffer) or a rollout holds [M, D] observations; an update step draws a minibatch as an
 * int64 index and, until now, gathered x[index] (and the stored actions) into fresh arrays before a network saw a row.  The three
 * entry points below read row index[b] of the storage where the shadowed ones read row b of the copy.  They launch the kernels of
 * pdegym_mlp_forward_cat, pdegym_mlp_backward_cat and pdegym_mlp_backward_wide_cat (new instantiations: no new kernel).
 *
 * Row      row b of the first layer's input is [ x[index[b], 0 .. D) | x2[(x2_indexed ? index[b] : b), 0 .. n2) ], 0 <= n2 <= 8,
 *          D = in_dim - n2 >= 1; n2 == 0 is the plain row (x2 == NULL).  y, dy and dx2 stay dense: row b.  x: float32, or float64 with
 *          net->x_f64, rounded as it is read.  Duplicated index entries are ordinary (sampling with replacement).
 * Bits     y, dw, db and dx2 equal, BIT FOR BIT, those of pdegym_mlp_forward / _cat, pdegym_mlp_backward_cat and
 *          pdegym_mlp_backward_wide_cat on the materialised rows with the same `slabs`: only the address of a row changes.  Every head,
 *          clamp and noise option of the forward, params 0 / 1 of the backward (one launch, or three) are kept.
 * Gradients  dx must be NULL (-2): a gradient of gathered rows is a scatter-add over duplicates, and the library has no float atomics.
 *          dx2 only with x2_indexed == 0 (the actor step: stored observation, fresh action).
 * Range    UNLIKE the `index` of pdegym_ppo_loss and pdegym_sac_critic_loss, whose range is the caller's to keep, an entry outside
 *          [0, M) is NEVER DEREFERENCED here (the index addresses a large storage on machines others share): where the row base is
 *          formed, one comparison per row replaces such an entry by row 0 for the address and selects the whole row to quiet NaN.  Its
 *          y is NaN and it reaches the weight gradients as a NaN row would; no other row of y or dx2 changes a bit.
 * Errors   as the shadowed entry points, and: -1 g or g->index NULL; -2 M < 1, index not 8-byte aligned, dx given, dx2 with
 *          x2_indexed, x2_indexed with n2 == 0.  The overlap checks of the backward passes take M rows for x (and for x2 with
 *          x2_indexed) and the B entries of index as an input. */
typedef struct pdegym_mlp_gather {
  const int64_t* index;   /* [B] device array: row b of the call is row index[b] of x             */
  int64_t M;              /* rows of x (and of x2 when x2_indexed); >= 1                          */
  int32_t x2_indexed;     /* 0: the tail of row b is x2[b]; 1: it is x2[index[b]]                */
  int32_t reserved_;
} pdegym_mlp_gather;
int pdegym_mlp_forward_gather(const pdegym_mlp* net, const void* x, int64_t x_stride, const float* x2, int64_t x2_stride,
                              int32_t n2, const pdegym_mlp_gather* g, void* y, int64_t y_stride, int32_t B, void* stream);
int pdegym_mlp_backward_gather(const pdegym_mlp* net, const pdegym_mlp_backward_cat_args* a, const pdegym_mlp_gather* g,
                               int32_t B, void* stream);
int pdegym_mlp_backward_wide_gather(const pdegym_mlp* net, const pdegym_mlp_backward_cat_args* a, const pdegym_mlp_gather* g,
                                    int32_t B, void* stream);

/* ---- backstepping baseline (the controller every result table of the reference compares the learned policies against) ------
 * Gains: theta [R, m] float32 rows, sampled by the caller (the examples use linspace(dx, X, m), NOT the plant's grid) -> gain [R, m]
 * float64, one wave per row, 2 <= m <= PDEGYM_MAX_N1D; dx is the Python double.  Both are BIT-IDENTICAL to the reference under
 * NumPy >= 2 (NEP 50: a float32 scalar times a Python double stays float32):
 *   parabolic: the last row k[m-1][:] of solveKernelFunction (the only row solveControl reads);
 *   transport: np.flip(kappa), kappa[i] = (sum_{j<i} (kappa[i-j]*theta[j])*dx) - theta[i] added left to right from 0 -- an ordered
 *              chain of m(m-1)/2 additions per row: computed once per theta row, never per step. */
int pdegym_backstep_gain_parabolic(const float* theta, double* gain, int32_t R, int32_t m, double dx, void* stream);
int pdegym_backstep_gain_transport(const float* theta, double* gain, int32_t R, int32_t m, double dx, void* stream);

/* Order of the additions of the control law's dot product */
enum {
  PDEGYM_BACKSTEP_TREE = 0,     /* products per lane (i = lane, lane + 64, ...), then the wave reduction: the batch default     */
  PDEGYM_BACKSTEP_ORDERED = 1   /* i ascending from 0.0, the reference's Python loop / builtin sum: commands bit-identical to it */
};
/* a[b] = (sum_{i<len} gain_row(b)[i] * (double)obs[b, i]) * scale, one wave per instance, the observation row read once.
 * transport1Dbackstepping.py: len = n, scale = 1e-2; reactionDiffusion1DBackstepping.py: len = min(m, n - 1), scale = dx.
 * gain_row(b) = gain0 + b * gain_stride until instance b has restarted; with gain_pool and reset_count[b] = c >= 1 it is pool row
 * (b + (c - 1)*B) mod pool_rows -- the row the step kernel's fused auto-reset took reset_beta from when it started the running
 * episode (pdegym_bufs1d.reset_count: the SAME counter, read through the same function).  The two orders differ by at most
 * 2 * len * 2^-53 * sum|gain_i * obs_i| * |scale|. */
typedef struct pdegym_backstep {
  const double* gain0;        /* [B, m], or one shared row with gain_stride = 0                                             */
  int64_t gain_stride;        /* doubles between the rows of consecutive instances                                          */
  const double* gain_pool;    /* optional [pool_rows, m]: gains of the reset pool's theta rows (needs reset_count)           */
  const int32_t* reset_count; /* [B] restarts so far, as the step kernels keep it; NULL = gain0 always                       */
  int32_t pool_rows;          /* rows of gain_pool (0 = B)                                                                   */
  int32_t m;                  /* length of a gain row                                                                        */
  const float* obs;           /* [B, obs_stride] observation rows (full-state sensing)                                       */
  int64_t obs_stride;         /* floats between consecutive rows (>= len)                                                    */
  int32_t len;                /* 1 .. m terms                                                                                */
  int32_t order;              /* PDEGYM_BACKSTEP_*                                                                           */
  double scale;
  double* out64;              /* [B] the command in double (PDEGYM_ACTION_F64: the reference's own call), or NULL            */
  float* out32;               /* [B] the command rounded once to float32, + noise, clamped -- exactly one of the two outputs */
  const float* noise;         /* optional [B], added before the clamp (out32 only)                                           */
  int32_t clamp;              /* nonzero: clamp to [lo, hi] (out32 only)                                                     */
  float lo, hi;
  int32_t reserved_;
} pdegym_backstep;
int pdegym_backstep_control(const pdegym_backstep* c, int32_t B, void* stream);

/* The law INSIDE the one-launch rollout: T x (pdegym_backstep_control into actions[t], then one env-step) as ONE kernel launch, the
 * row, beta, the norm ring, the sums and the instance's gain row held in registers throughout.  Every output -- obs slots 1 .. T,
 * actions (WRITTEN: the command after noise and clamp), rewards, terminated, truncated -- and the engine state left behind (time_index,
 * bsum, ring, norm_now, norm_back, beta, reset_count, final_obs) is BIT-IDENTICAL to that loop of two calls per env-step, in both
 * orders of addition (the kernels share one copy of the dot product).  prm / buf / ro as for pdegym_*_rollout, in its register-resident
 * corner only: Dirichlet actuation, full-state sensing, the linear flux, float32 beta and actions (beta_f64 == 0, action_kind ==
 * PDEGYM_ACTION_F32), no history, the temporal reward horizon, substeps >= 1 and rows of at most 8 slots per lane: 3 <= n <= 512
 * (transport) / 3 <= n <= 513 (parabolic: node 0 is held apart from the slots); ro->policy must be NULL.  ro->obs_noise /
 * ro->obs_seen ([T, B, n], optional) shape the LAW's input as they do a policy's: the law of step t reads obs[t] + obs_noise[t], which
 * obs_seen[t] receives, and the observation slots stay clean.  Everything else takes the two calls.
 * From `law` the call reads gain0, gain_stride, gain_pool, reset_count, pool_rows, m; len (1 <= len <= min(m, n)), order, scale; noise
 * -- here [T, B]: row t, instance b at noise[t * B + b] -- clamp, lo, hi.  law->obs, law->out64 and law->out32 must be NULL (the
 * observation is the rollout's slot t, the command goes to actions[t] as out32 would receive it).  gain_row(b) follows the rule of
 * pdegym_backstep_control; a restart made INSIDE the launch by the fused auto-reset switches the row before the next command, as the
 * counter would between two launches.  law->reset_count, when both are given, must be buf->reset_count: controller and plant read the
 * same counter (with buf->reset_count NULL the counter never moves, in either path). */
int pdegym_transport_backstep_rollout(const pdegym_params1d* prm, const pdegym_bufs1d* buf, const pdegym_rollout1d* ro,
                                      const pdegym_backstep* law, int32_t B, void* stream);
int pdegym_parabolic_backstep_rollout(const pdegym_params1d* prm, const pdegym_bufs1d* buf, const pdegym_rollout1d* ro,
                                      const pdegym_backstep* law, int32_t B, void* stream);

/* ---- backstepping baseline of TrafficPDE1D (the model-based row of the reference's traffic result table) -------------------------
 * pdegym_traffic_backstep_control replaces bcksController, examples/TrafficPDE1D/Backstepping control.ipynb cell 5, for a whole batch:
 *   'inlet'   the constant qs;      'outlet'  q_out;      'both'  (qs, q_out);      the train types are refused (no ps, normalised obs)
 *   q_out = (qs + rs*Iv) + Iq,  Iv = np.trapz(cv*(v - vs), dx=dx),  Iq = np.trapz(cq*(r*v - qs), dx=dx)
 * with (r, v) the two halves of the float64 observation row, vs = vm*(1 - rs/rm) and qs = rs*vs formed as the step kernels form them.
 * The weight rows cv, cq [M] hold NumPy's exp and are formed by the caller on the host, in the notebook's order of operations:
 *   K = -(1/(gamma*ps))*(-1/tau)*exp(-x/(tau*vs)), Mk = -K, E = exp(x/(vs*tau)), cv = Mk + (l2/l1)*K*E, cq = ((l1 - l2)/l1)*K*E,
 *   ps = vm/rm*qs/vs, l1 = vs, l2 = vs + rs*(-vm/rm), gamma = 1, x = np.arange(0, X + dx, dx).
 * The device forms the products at the nodes, the terms t_i = (dx*(p[i+1] + p[i]))/2.0, i < n = M - 1, and adds them in one of two orders: */
enum {
  PDEGYM_TRAFFIC_BACKSTEP_TREE = 0,   /* lane l adds t_l, t_{l+64}, ... in ascending order, then the wave reduction: any M, the batch default */
  PDEGYM_TRAFFIC_BACKSTEP_NUMPY = 1   /* np.add.reduce's order for n <= 128 (n < 8: one chain from 0.0; else eight accumulators a_k = t_k
                                         taking t_{k+8}, ... over the first n - n%8 terms, ((a0+a1)+(a2+a3))+((a4+a5)+(a6+a7)), then the
                                         last n%8 terms in turn): commands BIT-IDENTICAL to the notebook's.  M <= 129               */
};
#define PDEGYM_TRAFFIC_BACKSTEP_NUMPY_MAX_M 129
/* The two orders differ by at most 2^-52 * [(n + 2)*(|rs|*sum|tv_i| + sum|tq_i|) + |rs*Iv| + |qs + rs*Iv| + |q_out|]. */
typedef struct pdegym_traffic_backstep {
  const double* weights_v;  /* cv: [B, M] rows weight_stride apart, or one shared row with weight_stride = 0 (unused by 'inlet')   */
  const double* weights_q;  /* cq: the same layout                                                                                */
  int64_t weight_stride;    /* doubles between the rows of consecutive instances, 0 = shared                                      */
  int32_t order;            /* PDEGYM_TRAFFIC_BACKSTEP_*                                                                          */
  int32_t clamp;            /* nonzero: every command is clamped to [lo, hi] (np.clip: a NaN stays NaN)                           */
  const float* noise;       /* optional float32 [B, commands] (control) / [T, B, commands] (rollout), widened and added first      */
  int64_t noise_stride;     /* floats between the rows of consecutive instances (>= the number of commands: 1, 'both' 2)          */
  double lo, hi;
} pdegym_traffic_backstep;
/* obs [B, obs_stride >= 2M] float64, rs [B], out [B, out_stride >= commands] float64: out[b, 0] (and out[b, 1] for 'both').
 * 4 <= M <= PDEGYM_TRAFFIC_MAX_M.  'inlet' reads neither obs nor the weights. */
int pdegym_traffic_backstep_control(const pdegym_params_traffic* prm, const pdegym_traffic_backstep* law, const double* obs,
                                    int64_t obs_stride, const double* rs, double* out, int32_t out_stride, int32_t B, void* stream);
/* The law INSIDE the one-launch rollout (the loop of runSingleEpisode around bcksController, same cell): T x
 * (pdegym_traffic_backstep_control on observation slot t into actions[t], then pdegym_traffic_step) as ONE launch, 4 <= M <= 64.
 * prm / buf / ro as for pdegym_traffic_rollout; ro->policy must be NULL, ro->T >= 1, buf->action_stride the number of commands
 * (1; 2 or 0 for 'both').  Slot 0 of ro->obs is the caller's current observation; actions is WRITTEN (the command after noise and
 * clamp).  The law reads rs as the plant holds it, also after a restart by the fused auto-reset -- the weight rows do not follow a
 * restart, so a pool of other densities needs new weights (the Python layer refuses it).  Every output and the state left behind
 * are BIT-IDENTICAL to that loop of two calls per env-step, in both orders. */
int pdegym_traffic_backstep_rollout(const pdegym_params_traffic* prm, const pdegym_bufs_traffic* buf, const pdegym_rollout_traffic* ro,
                                    const pdegym_traffic_backstep* law, int32_t B, void* stream);

/* ---- adjoint-optimisation baseline of NavierStokes2D (the model-based row of the reference's NS result table) ----------------
 * examples/NavierStokes/NS2Doptimization.py:83-107 for a whole batch in ONE launch, float64 (the script's arithmetic), on the grids of
 * pdegym_ns2d_rollout_* (8, 11, 16, 21, 26, 31 or 32 rows, 3 .. 64 columns).  From Lam1 = Lam2 = pressure = 0 (:84-86), backward step
 * k = 0 .. T-2 reads the forward state of obs slot s = T - k (U[-1-t], V[-1-t] of :92-93: the state at time index t0 + s) and the target
 * frame U_ref[min(t0 + s, nt_ref - 1)] (u_target[-1-t] for the script's T = nt - 1, t0 = 0), and computes, operands in the order written:
 *   dlam1 = ((((-2*dx(lam1))*U - dy(lam1)*V) - dx(lam2)*V) - nu*lap(lam1)) + (U - U_tgt)       :92   (nu = prm->viscosity; the script
 *   dlam2 = ((((-2*dy(lam2))*V - dy(lam1)*U) - dx(lam2)*U) - nu*lap(lam2)) + (V - V_tgt)       :93    writes its environment's 0.1)
 *   lam  <- lam - dt*dlam, the four walls of both fields zero                                  :94-96 (apply_boundary of :56-61)
 *   p    <- solve_pressure(lam1, lam2, p): prm->density / dt, prm->iters sweeps, warm start    :97    (navier_stokes2D.py:94-116)
 *   lam1 <- lam1 - dt*dx(p), lam2 <- lam2 - dt*dy(p) (no division by the density), walls zero  :98-100
 * After backward step k, time index t = T-2-k receives (Lam1[::-1] of :103)
 *   grad[t, b]    = sum(central_difference(lam1, "y", dy)[ny-2, :]), columns 0 .. nx-1 added in sequence from the first   :106-107
 *   actions[t, b] = a_nom[t] - ((ratio*grad[t, b])*width)*dx      (the script: ratio = 0.1/0.1, width = 5)               :107
 *   lam[t, b]     = (lam1, lam2) interleaved, when lam is given
 * and t = T-1 the zero field: grad = 0, actions = a_nom[T-1].  Every value is bit-identical to the script's NumPy arithmetic.
 * Needs action_dim == 1 and the script's boundary table (:21-26): upper u Controllable, every other entry Dirichlet -- the zeroed
 * adjoint walls and the gradient row under the upper wall assume exactly that table. */
typedef struct pdegym_adjoint_ns2d {
  int32_t T;                /* forward steps of the trajectory (the script's T = 199, :65); T - 1 backward steps                 */
  int32_t t0;               /* time index of obs slot 0 (0 after a reset)                                                        */
  const double* obs;        /* [T + 1, B, ny, nx, 2] the forward rollout, pdegym_rollout_ns2d.obs (slot 0 is not read)   :74-76;
                               16-BYTE ALIGNED (else -2): the march reads (u, v) pairs                                              */
  const double* a_nom;      /* [T] nominal commands, the script's u_ref                                                  :81     */
  double ratio, width;
  double* grad;             /* [T, B] out                                                                                        */
  double* actions;          /* [T, B] out                                                                                :104-107 */
  double* lam;              /* optional [T, B, ny, nx, 2] out: Lam1[::-1] (:103) and Lam2 in the same order; NULL = not stored;
                               16-BYTE ALIGNED (else -2)                                                                            */
} pdegym_adjoint_ns2d;
/* U_ref: [nt_ref, ny, nx, 2], the targets of :79-80 as the step kernels read them (pdegym_bufs_ns2d.U_ref); 16-BYTE ALIGNED (else -2).
 * a_nom, grad and actions need 8 bytes. */
int pdegym_ns2d_adjoint_f64(const pdegym_params_ns2d* prm, const void* U_ref, int32_t nt_ref, const pdegym_adjoint_ns2d* adj, int32_t B,
                            void* stream);

/* ---- GAE(lambda) advantages, returns and episode statistics of a [T, B] rollout, one launch -----------------------------------
 * What every PPO user of the reference runs after a rollout (transport1Dppo.py, reactionDiffusion1Dppo.py, NS2Dppo.py and the
 * traffic and tumour notebooks: PPO("MlpPolicy", env)): Stable-Baselines3's RolloutBuffer.compute_returns_and_advantage
 * (stable_baselines3/common/buffers.py) and the truncation bootstrap of OnPolicyAlgorithm.collect_rollouts
 * (common/on_policy_algorithm.py: rewards[idx] += gamma * V(terminal_observation) where an episode was cut off by a time limit),
 * restated for the buffers of pdegym_*_rollout.  One lane per environment, t from T-1 down to 0, float32 with ONE rounding per
 * operation (nothing is fused, whatever the compiler flags), in SB3's order -- bit-identical to its NumPy loop:
 *     g  = (float)gamma;   gl = (float)(gamma * gae_lambda)         the product in double, rounded once: NumPy's weak-scalar rule
 *     done = terminated[t,b] | truncated[t,b];   nn = 1.0f - (float)done
 *     r  = (float)rewards[t,b];   if (boot && truncated[t,b] && !terminated[t,b]) r = r + g * boot[t,b]
 *     delta = (r + (g * values[t+1,b]) * nn) - values[t,b]
 *     last  = delta + ((gl * nn) * last)                            last = 0 before t = T-1
 *     advantages[t,b] = last;   returns[t,b] = last + values[t,b]
 * done[t] is SB3's episode_starts[t + 1] (its `dones` for t = T-1); values[t+1] after a restart is the value of the new episode's
 * first observation, multiplied by nn = 0, exactly as in SB3.  No clamps and no special cases: non-finite inputs propagate as IEEE
 * arithmetic makes them (conventions above), 0 * NaN crosses an episode boundary as it does in NumPy, and boot is a SELECT -- a NaN
 * in an entry the rule does not pick has no effect.  Columns are independent: a value in one changes no bit of another.
 * Episode statistics (optional), forward in t, in double: acc += (double)r_as_loaded (the reward BEFORE the bootstrap term; the
 * float64 reward itself with rewards_f64), len += 1; where done, episode_return[t,b] = acc and episode_length[t,b] = len and both
 * go back to zero; elsewhere the outputs receive 0.0 and 0.  ep_return_acc / ep_length_acc carry the running episode from one
 * call to the next (given together; NULL: every environment starts from zero); episode_return / episode_length are given together
 * or not at all (NULL: the statistics are skipped, and accumulators are then refused).
 * Every [., ld] array has `ld` ELEMENTS between consecutive rows t, ld >= B: a column shard of a wider batch is a pointer offset.
 * Errors: -1 null descriptor; -2 T < 1, B < 1, ld < B, gamma or gae_lambda not finite; -3 a required pointer is NULL, the optional
 * outputs are not given together, or an output (the accumulators included) overlaps an input or another output. */
typedef struct pdegym_gae_args {
  int32_t T;                 /* >= 1 steps                                                                                     */
  int32_t rewards_f64;       /* 0: rewards float32; nonzero: float64, rounded ONCE to float32 as it is read (SB3 stores float32) */
  const void* rewards;       /* [T, ld]                                                                                        */
  const float* values;       /* [T + 1, ld]: V(observation slot t); slot T is SB3's last_values                                */
  const uint8_t* terminated; /* [T, ld]                                                                                        */
  const uint8_t* truncated;  /* [T, ld] or NULL                                                                                */
  const float* boot;         /* optional [T, ld]: V(terminal observation); USED only where truncated && !terminated            */
  int64_t ld;                /* elements between consecutive rows t of EVERY [., ld] array, >= B                               */
  double gamma, gae_lambda;  /* the Python doubles                                                                             */
  float* advantages;         /* [T, ld], written for b < B                                                                     */
  float* returns;            /* [T, ld], written for b < B                                                                     */
  double* ep_return_acc;     /* optional [B], in/out: sum of the rewards of the running episode                                */
  int32_t* ep_length_acc;    /* optional [B], in/out: its length so far                                                        */
  double* episode_return;    /* optional [T, ld]: where an episode ended at (t, b) its return, else 0.0                        */
  int32_t* episode_length;   /* optional [T, ld]: its length, else 0                                                           */
} pdegym_gae_args;
int pdegym_gae(const pdegym_gae_args* g, int32_t B, void* stream);

/* ---- PPO loss head: surrogate, value and entropy terms of a minibatch with their gradients, at most three launches --------------
 * SB3's PPO.train (stable_baselines3/ppo/ppo.py) for the DiagGaussianDistribution of MlpPolicy on a Box action space
 * (common/distributions.py), from the outputs of the two networks to the gradients with respect to those outputs.  Row i < N of the
 * minibatch reads mean[i, 0..A) and values[i] (dense, minibatch order) and row k = index ? index[i] : i of the rollout buffer:
 * actions[k, 0..A), old_log_prob[k], advantages[k], returns[k] -- the gather of a_f[mb] and friends happens in the kernel.
 * Per row, float32 with ONE rounding per operation, in this order (c = clip_range; * + - / are single roundings, exp is expf):
 *     inv_j = exp(-log_std[j])                                                                        (once per lane)
 *     a     = advantages[k];  with normalize_advantage and N > 1:  a = (a - (float)mean_N) / ((float)std_N + 1e-8f)
 *     z_j   = (actions[k,j] - mean[i,j]) * inv_j
 *     t_j   = ((-0.5f * (z_j * z_j)) - log_std[j]) - 0.5 log(2 pi);   logp = t_0, then logp = logp + t_j for j = 1 .. A-1
 *     lr    = logp - old_log_prob[k];   ratio = exp(lr)
 *     s1    = a * ratio;   s2 = a * clamp(ratio, (float)(1 - c), (float)(1 + c))        the clamp keeps a NaN, like torch.clamp
 *     surr  = min(s1, s2), NaN if either is (torch.min)
 *     g     = 0 where (ratio > (float)(1 + c) && a > 0) || (ratio < (float)(1 - c) && a < 0), else -(s1 * (float)(1.0 / N))
 *     d_mean[i,j] = (g * z_j) * inv_j;      the term of d_log_std[j]: g * ((z_j * z_j) - 1)
 *     dv    = values[i] - returns[k];   the term of value_loss: dv * dv;   d_values[i] = dv * (float)(2 vf_coef / N)
 *     the term of approx_kl: (ratio - 1) - lr;   of clip_fraction: |ratio - 1| > (float)c
 * g is what torch's min / clamp backward gives (the clamp passes the gradient on its closed interval, ties add up to the full
 * gradient); the advantage normalisation is a constant with respect to the gradients, as in SB3.  mean_N and std_N (unbiased) of
 * the N gathered advantages are formed in float64 about the first gathered advantage (equal advantages: std_N == 0 exactly).
 * Every sum over rows is a float64 sum of the float32 terms in an order that is a function of N alone (csrc/pdegym_ppo_loss.hip),
 * rounded once at the end: bit-reproducible from run to run.
 *     policy_loss  = -sum surr / N;   value_loss = sum dv^2 / N (0 without values);   entropy_loss = -sum_j (0.5 + 0.5 log 2 pi + log_std[j])
 *     loss         = policy_loss + ent_coef * entropy_loss + vf_coef * value_loss            (in double, rounded once)
 *     d_log_std[j] = sum_i g_i (z_ij^2 - 1) - ent_coef
 *     stats[8]     = loss, policy_loss, value_loss, entropy_loss, approx_kl, clip_fraction, adv_mean, adv_std  (the last two 0 and 1
 *                    without normalisation)
 * Non-finite data is ordinary data: a NaN advantage without normalisation reaches the sums and its own row of d_mean only, with
 * normalisation every row; a NaN return reaches d_values[i], value_loss and loss only.  index entries must lie in [0, M).
 * Every pointer takes element accesses only (natural alignment of float / int64); the workspace holds doubles and needs 4 bytes.
 * Errors: -1 null descriptor; -2 N < 1, A outside 1 .. 8, a stride < A, M < 1 with an index, clip_range negative or not finite,
 * ent_coef / vf_coef not finite, workspace too small or not 4-byte aligned; -3 a required pointer is NULL, values / d_values not
 * given together (values needs returns), or an output (the workspace included) overlaps an input or another output. */
typedef struct pdegym_ppo_loss_args {
  int32_t A;                   /* action dimensions, 1 .. 8                                                                    */
  int32_t normalize_advantage; /* nonzero: normalise the N gathered advantages (skipped for N == 1, as SB3 does)               */
  const float* mean;           /* [N, ld_mean]: the actor's output                                                             */
  int64_t ld_mean;             /* elements between rows, >= A                                                                  */
  const float* values;         /* optional [N]: the critic's output; NULL = no value term                                      */
  const float* log_std;        /* [A], shared by all rows                                                                      */
  const int64_t* index;        /* optional [N], entries in [0, M): the minibatch's rows of the buffer; NULL = row i            */
  int64_t M;                   /* rows of the buffer arrays (used with index; without it they have N rows)                     */
  const float* actions;        /* [M, ld_actions]                                                                              */
  int64_t ld_actions;          /* >= A                                                                                         */
  const float* old_log_prob;   /* [M]                                                                                          */
  const float* advantages;     /* [M]                                                                                          */
  const float* returns;        /* [M]; required with values                                                                    */
  double clip_range, ent_coef, vf_coef; /* the Python doubles; clip_range >= 0                                                 */
  float* d_mean;               /* [N, ld_d_mean] out, columns < A written                                                      */
  int64_t ld_d_mean;           /* >= A                                                                                         */
  float* d_values;             /* [N] out; given if and only if values is                                                      */
  float* d_log_std;            /* [A] out                                                                                      */
  float* stats;                /* [8] out                                                                                      */
  void* workspace;             /* pdegym_ppo_loss_workspace(N, A) bytes, 4-BYTE ALIGNED (else -2); every word read was written
                                  by the same call                                                                             */
  int64_t workspace_bytes;
} pdegym_ppo_loss_args;
int64_t pdegym_ppo_loss_workspace(int32_t N, int32_t A);      /* bytes; negative: error code (N < 1, A outside 1 .. 8)          */
int pdegym_ppo_loss(const pdegym_ppo_loss_args* g, int32_t N, void* stream);
/* out[i] = logp of row i as above (mean [N, ld], actions [N or more, ld_a] gathered by the optional index [N], log_std [A]): what
 * fills old_log_prob after a rollout -- with unchanged weights pdegym_ppo_loss then sees lr == 0 and ratio == 1 exactly.
 * Errors: -2 N < 1, A outside 1 .. 8, ld or ld_a < A; -3 a NULL pointer (index excepted), out overlapping an input. */
int pdegym_diag_gaussian_log_prob(const float* mean, int64_t ld, const float* log_std, const float* actions, int64_t ld_a,
                                  const int64_t* index, float* out, int32_t N, int32_t A, void* stream);

/* ---- SAC loss heads: squashed-Gaussian sample with its backward, critic loss, actor + entropy-coefficient loss ---------------------
 * SB3's SAC.train (stable_baselines3/sac/sac.py) for the SquashedDiagGaussianDistribution of MlpPolicy (common/distributions.py,
 * epsilon = 1e-6) and one or two Q critics, from the networks' outputs to the gradients with respect to those outputs.  Everything
 * float32 with ONE rounding per operation in the order written below (* + - / are single roundings; exp, tanh and log are the
 * device library's expf, tanhf, logf -- the only places where a result may differ from torch float32); every sum over rows is a
 * float64 sum of the float32 terms in an order that is a function of N alone (csrc/pdegym_sac_loss.hip), rounded once.  No atomics:
 * stream order is the only synchronisation, and every word of a workspace that is read was written by the same call.  Every pointer
 * takes element accesses only (natural alignment of float / int64); a workspace holds doubles and needs 4 bytes.
 *
 * 1. pdegym_squashed_gaussian_sample (one launch, one row per lane).  raw[i] holds the 2A columns [mu_0 .. mu_{A-1}; log_std_0 ..]
 *    of the actor's last layer (FusedMLP.squashed_gaussian(...).with_grad), eps[i] the A standard-normal draws.  Per column j:
 *        ls    = clamp(log_std_j, log_std_min, log_std_max)                    the clamp keeps a NaN, like torch.clamp
 *        sigma = exp(ls);   z = mu_j + (sigma * eps_j);   a_j = tanh(z);   w = 1 - (a_j * a_j);   u = w + 1e-6f
 *        t_j   = (((-0.5f * (eps_j * eps_j)) - ls) - 0.5 log(2 pi)) - log(u)
 *        logp  = t_0, then logp = logp + t_j for j = 1 .. A-1
 *    which is SquashedDiagGaussianDistribution.log_prob on its own gaussian_actions: (z - mu) / sigma IS eps by construction, so
 *    eps is used directly.  actions[i, D + j] = a_j in [-1, 1], log_prob[i] = logp.  With obs (and D >= 1) the launch also copies
 *    obs[i, 0..D) into actions[i, 0..D): `actions` is then the critics' input block [obs | a], torch.cat([obs, a], 1) disappears.
 *    Columns >= D + A of a row are never written.
 *
 * 2. pdegym_squashed_gaussian_sample_backward (one launch).  Recomputes a_j, w, u, sigma from raw and eps -- the forward launch saves
 *    nothing -- and, with da_j = d_actions[i, j] (a NULL d_actions reads as +0) and dl = d_log_prob[i * d_log_prob_stride] (NULL: +0):
 *        k        = ((2 * a_j) * w) / u;      se = sigma * eps_j;      daw = da_j * w
 *        d_raw[i, j]     = daw + (dl * k)                                                                         (d / d mu_j)
 *        d_raw[i, A + j] = (daw * se) + (dl * ((k * se) - 1))  where log_std_min <= log_std_j <= log_std_max, else +0   (d / d log_std_j)
 *    The gate is the closed interval torch's clamp backward passes; it SELECTS 0 and never multiplies by it (a NaN log_std is outside).
 *    The Gaussian part of logp contributes exactly -1 to d / d log_std and 0 to d / d mu: autograd over ((z - mu) / sigma)^2 with
 *    z = mu + sigma eps leaves further terms that are 0 in exact arithmetic and rounding residue in floating point; they are dropped.
 *    d_log_prob is an ARRAY with an element stride: d_log_prob_stride = 1 is a dense [N] array, 0 is ONE device scalar for all rows
 *    (what pdegym_sac_actor_loss writes).  d_actions may point into a wider block: the action columns of a critic's dx [N, D + A]
 *    are passed in place as d_actions = dx + D, ld_d_actions = D + A.
 *    Saturated rows (|z| large: a_j = +-1) have w = 0, u = 1e-6f, a finite log_prob and k == 0 exactly.
 *
 * 3. pdegym_sac_critic_loss (two launches: rows, finish; the second is skipped without stats).  Row i < N reads q1[i], q2[i],
 *    q1_target[i], q2_target[i], next_log_prob[i] (dense) and rewards[k], dones[k] (0.0 / 1.0) at k = index ? index[i] : i.
 *    log_alpha is a DEVICE pointer to one float (no host synchronisation): alpha = exp(*log_alpha).
 *        m   = min(q1_target[i], q2_target[i]), NaN if either is (torch.min); one critic: q1_target[i]
 *        y   = r + (((1 - d) * (float)gamma) * (m - (alpha * next_log_prob[i])))
 *        e_c = q_c[i] - y;     d_q_c[i] = e_c * (float)(1.0 / N);     target[i] = y
 *        critic_loss = 0.5 * (sum e_1 * e_1 + sum e_2 * e_2) / N               (SB3: 0.5 * sum_c F.mse_loss(q_c, y))
 *        stats[4]    = critic_loss, mean q1, mean q2 (0 with one critic), mean y
 *    q2 / q2_target / d_q2 all NULL: one critic.  A NaN in a row reaches that row's outputs and the sums only.
 *
 * 4. pdegym_sac_actor_loss (two launches).  alpha = exp(*log_alpha);
 *        m_i         = min over the critics as torch.min(torch.cat((q1_pi, q2_pi), 1), dim=1) computes it: the FIRST minimal
 *                      column, a NaN counting as minimal; its gradient -(float)(1.0 / N) goes to that column (a tie: q1_pi), the
 *                      other column gets 0
 *        actor_loss    = sum((alpha * log_prob[i]) - m_i) / N
 *        ent_mean      = sum(log_prob[i] + (float)target_entropy) / N
 *        ent_coef_loss = -(*log_alpha) * ent_mean;      d_log_alpha[0] = -ent_mean
 *        d_log_prob[0] = alpha * (float)(1.0 / N)       ONE scalar: d actor_loss / d log_prob[i] for every i (the sample backward
 *                                                       takes it with d_log_prob_stride = 0)
 *        stats[4]      = actor_loss, ent_coef_loss, alpha, mean log_prob
 *
 * Errors: -1 null descriptor; -2 N < 1, A outside 1 .. 8, a stride shorter than its row (ld_raw, ld_d_raw < 2A; ld_eps,
 * ld_d_actions < A; ld_obs < D; ld_actions < D + A), D and obs not given together, d_log_prob_stride not 0 or 1,
 * log_std_min >= log_std_max, M < 1 with an index, gamma or target_entropy not finite, a workspace too small or not 4-byte aligned;
 * -3 a required pointer is NULL (d_actions and d_log_prob both NULL; q2 and its companions given in part), or an output (the workspace
 * included) overlaps an input or another output. */
typedef struct pdegym_squashed_gaussian_sample_args {
  int32_t A;                   /* action dimensions, 1 .. 8                                                                    */
  int32_t D;                   /* observation columns copied in front of the actions; 0 without obs                            */
  const float* raw;            /* [N, ld_raw]: columns [mu; log_std], 2A of them                                               */
  int64_t ld_raw;              /* >= 2A                                                                                        */
  const float* eps;            /* [N, ld_eps]                                                                                  */
  int64_t ld_eps;              /* >= A                                                                                         */
  float log_std_min, log_std_max;
  const float* obs;            /* optional [N, ld_obs]                                                                         */
  int64_t ld_obs;              /* >= D                                                                                         */
  float* actions;              /* [N, ld_actions] out: columns [0, D) the observation, [D, D + A) the actions                  */
  int64_t ld_actions;          /* >= D + A                                                                                     */
  float* log_prob;             /* [N] out                                                                                      */
} pdegym_squashed_gaussian_sample_args;
int pdegym_squashed_gaussian_sample(const pdegym_squashed_gaussian_sample_args* s, int32_t N, void* stream);

typedef struct pdegym_squashed_gaussian_sample_backward_args {
  int32_t A;
  int32_t reserved_;
  const float* raw;            /* [N, ld_raw], as in the forward call                                                          */
  int64_t ld_raw;
  const float* eps;            /* [N, ld_eps]                                                                                  */
  int64_t ld_eps;
  float log_std_min, log_std_max;
  const float* d_actions;      /* optional [N, ld_d_actions]                                                                   */
  int64_t ld_d_actions;        /* >= A                                                                                         */
  const float* d_log_prob;     /* optional; not both NULL                                                                      */
  int64_t d_log_prob_stride;   /* 1: a dense [N] array; 0: one device scalar                                                   */
  float* d_raw;                /* [N, ld_d_raw] out, columns < 2A written                                                      */
  int64_t ld_d_raw;            /* >= 2A                                                                                        */
} pdegym_squashed_gaussian_sample_backward_args;
int pdegym_squashed_gaussian_sample_backward(const pdegym_squashed_gaussian_sample_backward_args* s, int32_t N, void* stream);

typedef struct pdegym_sac_critic_loss_args {
  const float* q1;             /* [N]                                                                                          */
  const float* q2;             /* optional [N]; with q2_target and d_q2                                                        */
  const float* q1_target;      /* [N]                                                                                          */
  const float* q2_target;      /* optional [N]                                                                                 */
  const float* next_log_prob;  /* [N]                                                                                          */
  const int64_t* index;        /* optional [N], entries in [0, M); NULL = row i                                                */
  int64_t M;                   /* rows of rewards / dones (used with index; without it they have N rows)                       */
  const float* rewards;        /* [M]                                                                                          */
  const float* dones;          /* [M], 0.0 or 1.0                                                                              */
  const float* log_alpha;      /* DEVICE pointer to one float                                                                  */
  double gamma;                /* the Python double                                                                            */
  float* d_q1;                 /* [N] out                                                                                      */
  float* d_q2;                 /* [N] out; given if and only if q2 is                                                          */
  float* target;               /* optional [N] out                                                                             */
  float* stats;                /* optional [4] out                                                                             */
  void* workspace;             /* pdegym_sac_loss_workspace(N) bytes, 4-BYTE ALIGNED (else -2)                                 */
  int64_t workspace_bytes;
} pdegym_sac_critic_loss_args;
int pdegym_sac_critic_loss(const pdegym_sac_critic_loss_args* g, int32_t N, void* stream);

typedef struct pdegym_sac_actor_loss_args {
  const float* q1_pi;          /* [N]                                                                                          */
  const float* q2_pi;          /* optional [N]; with d_q2_pi                                                                   */
  const float* log_prob;       /* [N]                                                                                          */
  const float* log_alpha;      /* DEVICE pointer to one float                                                                  */
  double target_entropy;       /* the Python double                                                                            */
  float* d_q1_pi;              /* [N] out                                                                                      */
  float* d_q2_pi;              /* [N] out; given if and only if q2_pi is                                                       */
  float* d_log_prob;           /* [1] out                                                                                      */
  float* d_log_alpha;          /* [1] out                                                                                      */
  float* stats;                /* optional [4] out                                                                             */
  void* workspace;             /* pdegym_sac_loss_workspace(N) bytes, 4-BYTE ALIGNED (else -2)                                 */
  int64_t workspace_bytes;
} pdegym_sac_actor_loss_args;
int pdegym_sac_actor_loss(const pdegym_sac_actor_loss_args* g, int32_t N, void* stream);
int64_t pdegym_sac_loss_workspace(int32_t N);      /* bytes, for either loss; negative: error code (N < 1)                      */

/* ---- fused optimiser step: global-norm clip, Adam, weight mirrors and Polyak targets in two launches ------------------------------
 * One call updates K <= PDEGYM_FUSED_ADAM_MAX_TENSORS float32 tensors as torch.nn.utils.clip_grad_norm_ followed by torch.optim.Adam
 * (no weight decay, no amsgrad, one step count for all tensors) update them, writes each new parameter to its MIRRORS -- the
 * blocked transpose pdegym_mlp_forward reads, so FusedMLP.refresh() has nothing left to do -- and, with `polyak`, moves a target
 * copy towards it (SB3's polyak_update).  The table is passed by value in the kernel arguments (gradient addresses change from one
 * eager step to the next; a stream capture bakes them in).
 *
 * Two launches on `stream`, stream order the only synchronisation (no atomics, no workgroup waits for another):
 *   head    per-workgroup sums of g * g in float64 into the workspace (only when a norm is wanted: max_grad_norm > 0, or total_norm
 *           given; otherwise the launch is one workgroup); thread 0 of workgroup 0 advances the state block:
 *               state[0] += 1;   state[1] *= beta1;   state[2] *= beta2          (step count, beta1^t, beta2^t: doubles, no pow)
 *   update  every workgroup adds the partial sums itself and updates its elements.
 * Decomposition (a function of the list n_0 .. n_{K-1} alone): tensor k takes c_k = min(ceil(n_k / 1024), 256) workgroups of 256
 * threads, in table order; workgroup j of tensor k, thread t takes the elements e = 1024 (j + c_k r) + 256 q + t, q = 0 .. 3,
 * r = 0, 1, .. while e < n_k.  Order of the sum of squares: a thread adds its (double) g * g (one float32 product, widened) in the
 * order r ascending, q ascending within r; a workgroup adds its threads with the wave reduction of csrc/pdegym_common.h per wave and
 * the four waves in ascending order; the G = sum c_k partials are added the same way, thread t taking the partials t, t + 256, ..
 * in ascending order, then the workgroup sum.
 *
 * Arithmetic: float32, every operation rounded on its own, in this order (the double-precision scalars are formed once per launch):
 *     total  = (float) sqrt(sum_double(g^2))                                       one rounding
 *     coef   = min(max_grad_norm / (total + 1e-6f), 1.0f)                          a NaN stays NaN, as torch.clamp keeps it
 *     g'     = g * coef                                                            multiplied even when coef == 1 (clip_grad_norm_);
 *                                                                                  without clipping g' = g
 *     m      = m + (float)(1 - beta1) * (g' - m)
 *     v      = (float)beta2 * v + (float)(1 - beta2) * (g' * g')
 *     p      = p - (float)(lr / (1 - beta1^t)) * (m / (sqrt(v) / (float)sqrt(1 - beta2^t) + (float)eps))
 *     pt     = (float)(1 - tau) * pt + (float)tau * p                              only with polyak, p the NEW value
 * lr is the host double `lr`, or (double)*lr_device when lr_device is given.  UNLIKE clip_grad_norm_, g itself is NOT modified.
 * Clipping is off for max_grad_norm <= 0 or NaN.  total_norm (optional, one float) receives `total` whenever a norm is computed.
 *
 * Mirrors of tensor k (each optional): `copy` receives p[e] at copy[e]; `wt`, for a tensor of shape (out, in), n = out * in,
 * receives element (o, i) at wt[(i / 4) * wt_out_total * 4 + (wt_row0 + o) * 4 + i % 4] -- rows wt_row0 .. wt_row0 + out of a
 * blocked array [ceil(in / 4), wt_out_total, 4]; its padding entries (i >= in) are never written.  The target pt has the same two
 * mirrors (pt_copy, pt_wt with pt_wt_out_total, pt_wt_row0), written only with polyak; without polyak pt and its mirrors are untouched.
 *
 * Errors: -1 null descriptor; -2 K outside 1 .. 32, n < 1, a non-finite hyper-parameter, beta outside [0, 1), eps <= 0, tau outside
 * [0, 1] with a target, out * in != n or row0 + out > out_total of a mirror, a workspace that is too small, a misaligned pointer
 * (4 bytes; state: 8); -3 a NULL required pointer (p, g, m, v, state, workspace), a target mirror without a target, an output that
 * overlaps another tensor of the call as a byte range (two blocked mirrors may share one array on disjoint rows). */
#define PDEGYM_FUSED_ADAM_MAX_TENSORS 32
typedef struct pdegym_fused_adam_tensor {
  float* p;                    /* [n] parameter, updated in place                                                              */
  const float* g;              /* [n] gradient, read only                                                                      */
  float* m;                    /* [n] first moment                                                                             */
  float* v;                    /* [n] second moment                                                                            */
  int64_t n;
  float* copy;                 /* NULL or [n]: plain mirror                                                                    */
  float* wt;                   /* NULL or blocked mirror                                                                       */
  int32_t out, in;             /* the tensor's shape, used with wt / pt_wt                                                     */
  int32_t wt_out_total, wt_row0;
  float* pt;                   /* NULL or [n]: Polyak target                                                                   */
  float* pt_copy;              /* NULL or [n]: plain mirror of the target                                                      */
  float* pt_wt;                /* NULL or blocked mirror of the target                                                         */
  int32_t pt_wt_out_total, pt_wt_row0;
} pdegym_fused_adam_tensor;

typedef struct pdegym_fused_adam_args {
  int32_t K;                   /* tensors in use, 1 .. 32                                                                      */
  int32_t polyak;              /* != 0: update the targets in this call                                                        */
  double lr;                   /* used when lr_device is NULL                                                                  */
  const float* lr_device;      /* NULL or one float on the device                                                              */
  double beta1, beta2, eps;
  double max_grad_norm;        /* <= 0 or NaN: no clipping                                                                     */
  double tau;                  /* in [0, 1] when any tensor has a target                                                       */
  double* state;               /* [3] step count, beta1^t, beta2^t; start at {0, 1, 1}; 8-BYTE ALIGNED                         */
  float* total_norm;           /* NULL or one float                                                                            */
  void* workspace;             /* pdegym_fused_adam_workspace(...) bytes, 4-BYTE ALIGNED (else -2)                             */
  int64_t workspace_bytes;
  pdegym_fused_adam_tensor tensor[PDEGYM_FUSED_ADAM_MAX_TENSORS];
} pdegym_fused_adam_args;
int pdegym_fused_adam(const pdegym_fused_adam_args* a, void* stream);
/* bytes for the tensor sizes n[0 .. K); negative: error code (K outside 1 .. 32, an n < 1) */
int64_t pdegym_fused_adam_workspace(const int64_t* n, int32_t K);

/* ---- test-only: kernel dispatch overrides -------------------------------------------------------------------------
 * Nothing on the product path calls this (the reference has no counterpart); the parity tests use it to run the SAME step
 * through two kernel families and compare the results bit for bit, developer tools for A/B timings.  Process-wide; returns
 * the previous value, or a negative error code for an unknown key. */
enum {
  PDEGYM_DEBUG_NS_GENERIC = 0,        /* != 0: every NavierStokes2D step takes ns_generic_step (workgroup per instance)     */
  PDEGYM_DEBUG_NS_NO_COL = 1,         /* != 0: small grids skip the column-per-lane kernel                                   */
  PDEGYM_DEBUG_NS_COL_MIN_BATCH = 2,  /* >= 0: smallest batch the column-per-lane kernel takes (-1: the built-in rule)       */
  PDEGYM_DEBUG_NS_NO_LDS_JACOBI = 3,  /* != 0: ns_generic_step keeps the pressure in global memory during the sweeps         */
  PDEGYM_DEBUG_COUNT = 4
};
int32_t pdegym_debug_set(int32_t key, int32_t value);

#ifdef __cplusplus
}
#endif
#endif /* PDEGYM_H */
