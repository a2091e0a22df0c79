/* terminal_obs_validation.c -- argument validation of what the per-step terminal observations add to the C ABI (include/pdegym.h:
 * PDEGYM_ROLLOUT_FINAL_OBS_PER_STEP in pdegym_rollout1d / pdegym_rollout_traffic / pdegym_rollout_tumor .reserved_, and
 * pdegym_mlp_forward_masked) WITHOUT a GPU: the flag with final_obs == NULL (-3) or without an auto-reset pool (-2) in every rollout
 * entry point that takes it, the other bits of reserved_ ignored, NULL rows, misaligned weights and the heads / outputs the masked
 * launch does not take.  Every bad call must come back with the code the header states and a message in pdegym_last_error();
 * tests/test_terminal_obs.py links it against the host halves of the units built with AddressSanitizer and
 * UndefinedBehaviorSanitizer.  Well-formed calls carry fake device addresses: the host code runs up to the launch, which fails cleanly
 * on a machine without a device (-4 / -100); no pointer is dereferenced on the host and no kernel is launched. */
#include <stdio.h>
#include <string.h>

#include "pdegym.h"

static int n_calls = 0, n_bad = 0;

static void expect_code(const char* what, int rc, int code) {
  const char* msg = pdegym_last_error();
  ++n_calls;
  if (rc != code || msg == NULL || msg[0] == '\0') {
    ++n_bad;
    printf("UNEXPECTED %s -> %d \"%s\" (expected %d)\n", what, rc, msg ? msg : "(null)", code);
  } else {
    printf("%-64s %5d  %s\n", what, rc, msg);
  }
}

/* the refusal names the flag */
static void expect_flag(const char* what, int rc, int code) {
  const char* msg = pdegym_last_error();
  expect_code(what, rc, code);
  if (rc == code && msg && !strstr(msg, "PDEGYM_ROLLOUT_FINAL_OBS_PER_STEP")) {
    ++n_bad;
    printf("UNEXPECTED %s: the message does not name the flag: \"%s\"\n", what, msg);
  }
}

static void expect_launch(const char* what, int rc) {
  const char* msg = pdegym_last_error();
  ++n_calls;
  if ((rc != -100 && rc != -4) || msg == NULL || msg[0] == '\0') {
    ++n_bad;
    printf("UNEXPECTED %s -> %d \"%s\" (a well-formed call fails only at the launch)\n", what, rc, msg ? msg : "(null)");
  } else {
    printf("%-64s %5d  %s\n", what, rc, msg);
  }
}

#define FAKE(k) ((void*)(uintptr_t)(0x7f0000000000ull + 0x4000000ull * (k)))
#define B_ 6

/* ---- 1D ---- */
typedef struct call1d {
  pdegym_params1d p;
  pdegym_bufs1d b;
  pdegym_rollout1d r;
  pdegym_backstep l;
} call1d;

static call1d good1d(int n, int parabolic) {
  call1d c;
  memset(&c, 0, sizeof c);
  c.p.n = n; c.p.nt = 1001; c.p.substeps = 100; c.p.control_type = PDEGYM_CONTROL_DIRICHLET; c.p.sensing = PDEGYM_SENSE_FULL;
  c.p.limit_state = 1; c.p.reward_kind = PDEGYM_REWARD_TUNED1D; c.p.reward_nt = 1000; c.p.dt = 1e-4f; c.p.dx = 1e-2f; c.p.F = 0.25f;
  c.p.max_control = 20; c.p.max_state = 1e10f; c.p.truncate_penalty = -1e3f; c.p.terminate_reward = 3e2f; c.p.rdx = 100.0;
  c.p.dt64 = 1e-4; c.p.dx64 = 1e-2; c.p.max_control64 = 20;
  (void)parabolic;
  c.b.u = FAKE(20); c.b.beta = FAKE(1); c.b.beta_stride = n; c.b.time_index = FAKE(2); c.b.bsum = FAKE(3); c.b.ring = FAKE(4);
  c.b.norm_now = FAKE(5); c.b.norm_back = FAKE(6); c.b.reset_init = FAKE(7); c.b.reset_beta = FAKE(8); c.b.reset_count = FAKE(9);
  c.b.reset_pool_rows = 7; c.b.final_obs = FAKE(18);
  c.r.T = 8; c.r.obs = FAKE(10); c.r.actions = FAKE(11); c.r.rewards = FAKE(12); c.r.terminated = FAKE(13); c.r.truncated = FAKE(14);
  c.r.reserved_ = PDEGYM_ROLLOUT_FINAL_OBS_PER_STEP;
  c.l.gain0 = FAKE(15); c.l.gain_stride = n; c.l.m = n; c.l.len = n - 1; c.l.gain_pool = FAKE(16); c.l.reset_count = FAKE(9);
  c.l.pool_rows = 7; c.l.order = PDEGYM_BACKSTEP_ORDERED; c.l.scale = 1e-2; c.l.noise = FAKE(17); c.l.clamp = 1; c.l.lo = -20; c.l.hi = 20;
  return c;
}

typedef int (*roll1d_fn)(const pdegym_params1d*, const pdegym_bufs1d*, const pdegym_rollout1d*, int32_t, void*);
typedef int (*law1d_fn)(const pdegym_params1d*, const pdegym_bufs1d*, const pdegym_rollout1d*, const pdegym_backstep*, int32_t, void*);

static char label[160];
static const char* tag(const char* who, const char* what) {
  snprintf(label, sizeof label, "%s: %s", who, what);
  return label;
}

static void cases1d(const char* who, roll1d_fn f, law1d_fn g, int parabolic) {
  const int n = parabolic ? 65 : 64;
  call1d c;
#define RUN1D(c) (f ? f(&(c).p, &(c).b, &(c).r, B_, NULL) : g(&(c).p, &(c).b, &(c).r, &(c).l, B_, NULL))
  c = good1d(n, parabolic); c.b.final_obs = NULL; expect_flag(tag(who, "flag with final_obs=NULL"), RUN1D(c), -3);
  c = good1d(n, parabolic); c.b.reset_init = NULL; c.b.reset_beta = NULL; expect_flag(tag(who, "flag without reset_init"), RUN1D(c), -2);
  c = good1d(n, parabolic); c.b.final_obs = NULL; c.r.reserved_ = 0x7ffffffe;      /* the other bits stay ignored */
  expect_launch(tag(who, "launch (every bit but bit 0, no final_obs)"), RUN1D(c));
  c = good1d(n, parabolic); c.r.reserved_ = 0; expect_launch(tag(who, "launch (flag clear)"), RUN1D(c));
  c = good1d(n, parabolic); expect_launch(tag(who, "launch (flag set)"), RUN1D(c));
  c = good1d(n, parabolic); c.r.reserved_ = -1; expect_launch(tag(who, "launch (all bits set)"), RUN1D(c));
  if (f) {      /* the general kernels: Neumann actuation, scalar sensing (one float per slot) */
    c = good1d(n, parabolic); c.p.control_type = PDEGYM_CONTROL_NEUMANN; expect_launch(tag(who, "launch (flag set, Neumann)"), RUN1D(c));
    c = good1d(n, parabolic); c.p.sensing = PDEGYM_SENSE_LAST; expect_launch(tag(who, "launch (flag set, scalar sensing)"), RUN1D(c));
    c = good1d(n, parabolic); c.p.sensing = PDEGYM_SENSE_LAST; c.b.final_obs = NULL;
    expect_flag(tag(who, "flag with final_obs=NULL, scalar sensing"), RUN1D(c), -3);
  }
  /* an empty call stays a no-op, flag or not */
  c = good1d(n, parabolic); c.b.final_obs = NULL; c.r.T = 0;
  ++n_calls;
  if (RUN1D(c) != 0) { ++n_bad; printf("UNEXPECTED %s: T=0 is not a no-op\n", who); }
#undef RUN1D
}

/* ---- traffic ---- */
typedef struct call_traffic {
  pdegym_params_traffic p;
  pdegym_bufs_traffic b;
  pdegym_rollout_traffic r;
  pdegym_traffic_backstep l;
} call_traffic;

static call_traffic good_traffic(int M, int sim) {
  call_traffic c;
  memset(&c, 0, sizeof c);
  c.p.M = M; c.p.control_freq = 2; c.p.sim = sim; c.p.limit = 1; c.p.dt = 0.25; c.p.dx = 10; c.p.T = 240; c.p.vm = 40; c.p.rm = 0.16; c.p.tau = 60;
  c.b.r = FAKE(1); c.b.y = FAKE(2); c.b.time = FAKE(3); c.b.rs = FAKE(4); c.b.qs_clip = FAKE(5); c.b.obs = FAKE(19); c.b.done = FAKE(20);
  c.b.truncated = FAKE(21);
  c.b.action_stride = sim == PDEGYM_TRAFFIC_BOTH ? 2 : 1;
  c.b.reset_rs = FAKE(6); c.b.reset_profile = FAKE(7); c.b.final_obs = FAKE(8); c.b.reset_count = FAKE(9); c.b.reset_pool_rows = 7;
  c.r.T = 8; c.r.obs = FAKE(10); c.r.actions = FAKE(11); c.r.rewards = FAKE(12); c.r.done = FAKE(13); c.r.truncated = FAKE(14);
  c.r.reserved_ = PDEGYM_ROLLOUT_FINAL_OBS_PER_STEP;
  c.l.weights_v = FAKE(15); c.l.weights_q = FAKE(16); c.l.weight_stride = M; c.l.order = PDEGYM_TRAFFIC_BACKSTEP_TREE; c.l.noise = FAKE(17);
  c.l.noise_stride = c.b.action_stride; c.l.clamp = 1; c.l.lo = 0.96; c.l.hi = 1.44;
  return c;
}

static void cases_traffic(int law) {
  const char* who = law ? "traffic backstep rollout" : "traffic rollout";
  call_traffic c;
#define RUNT(c) (law ? pdegym_traffic_backstep_rollout(&(c).p, &(c).b, &(c).r, &(c).l, B_, NULL) : pdegym_traffic_rollout(&(c).p, &(c).b, &(c).r, B_, NULL))
  c = good_traffic(12, PDEGYM_TRAFFIC_OUTLET); c.b.final_obs = NULL; expect_flag(tag(who, "flag with final_obs=NULL"), RUNT(c), -3);
  c = good_traffic(12, PDEGYM_TRAFFIC_OUTLET); c.b.reset_rs = NULL; c.b.reset_profile = NULL; expect_flag(tag(who, "flag without reset_rs"), RUNT(c), -2);
  c = good_traffic(12, PDEGYM_TRAFFIC_OUTLET); c.b.final_obs = NULL; c.r.reserved_ = 0x7ffffffe;
  expect_launch(tag(who, "launch (every bit but bit 0, no final_obs)"), RUNT(c));
  c = good_traffic(12, PDEGYM_TRAFFIC_OUTLET); c.r.reserved_ = 0; expect_launch(tag(who, "launch (flag clear)"), RUNT(c));
  c = good_traffic(12, PDEGYM_TRAFFIC_OUTLET); expect_launch(tag(who, "launch (flag set)"), RUNT(c));
  c = good_traffic(12, PDEGYM_TRAFFIC_BOTH); expect_launch(tag(who, "launch (flag set, two commands)"), RUNT(c));
#undef RUNT
}

/* ---- tumour ---- */
typedef struct call_tumor {
  pdegym_params_tumor p;
  pdegym_bufs_tumor b;
  pdegym_wrap_tumor w;
  pdegym_rollout_tumor r;
} call_tumor;

static call_tumor good_tumor(int nx) {
  call_tumor c;
  memset(&c, 0, sizeof c);
  c.p.nx = nx; c.p.nt = 601; c.p.dt = 1; c.p.dx = 1; c.p.dx2 = 1; c.p.D = 0.2; c.p.rho = 0.03; c.p.alpha = 0.04; c.p.alpha_beta_ratio = 10;
  c.p.k = 1e5; c.p.thr_t1 = 8e4; c.p.thr_t2 = 1.6e4; c.p.detect_radius = 15; c.p.death_radius = 35; c.p.total_dosage = 61.2;
  c.p.dose_end = 0.1; c.p.margin = 25;
  c.b.u = FAKE(1); c.b.xscale = FAKE(2); c.b.control = FAKE(3); c.b.time_index = FAKE(4); c.b.stage = FAKE(5); c.b.remaining = FAKE(6);
  c.b.days = FAKE(7); c.b.t_benchmark = FAKE(8); c.b.reward = FAKE(9); c.b.terminated = FAKE(10); c.b.truncated = FAKE(11); c.b.out = FAKE(12);
  c.w.weekends = 1; c.w.init = FAKE(13); c.w.init_stride = nx; c.w.consecutive = FAKE(14); c.w.treatment_calls = FAKE(15);
  c.w.soft_constraint_violations = FAKE(16); c.w.final_obs = FAKE(17); c.w.obs = FAKE(18);
  c.r.T = 8; c.r.obs = FAKE(19); c.r.actions = FAKE(20); c.r.rewards = FAKE(21); c.r.terminated = FAKE(22); c.r.truncated = FAKE(23);
  c.r.reserved_ = PDEGYM_ROLLOUT_FINAL_OBS_PER_STEP;
  return c;
}

#define ROLLTU(c) pdegym_tumor_rollout(&(c).p, &(c).b, &(c).w, &(c).r, B_, NULL)

/* ---- masked forward ---- */
static pdegym_mlp net_good(int width) {
  pdegym_mlp n;
  memset(&n, 0, sizeof n);
  n.n_layers = 3;
  n.layer[0].w = FAKE(1); n.layer[0].b = FAKE(2); n.layer[0].in_dim = 9; n.layer[0].out_dim = width; n.layer[0].act = PDEGYM_MLP_TANH;
  n.layer[1].w = FAKE(3); n.layer[1].b = FAKE(4); n.layer[1].in_dim = width; n.layer[1].out_dim = 33; n.layer[1].act = PDEGYM_MLP_RELU;
  n.layer[2].w = FAKE(5); n.layer[2].b = FAKE(6); n.layer[2].in_dim = 33; n.layer[2].out_dim = 1; n.layer[2].act = PDEGYM_MLP_IDENTITY;
  return n;
}

int main(void) {
  if (pdegym_abi_version() != PDEGYM_ABI_VERSION || PDEGYM_ABI_VERSION != 21) { printf("ABI mismatch\n"); return 1; }
  if (PDEGYM_ROLLOUT_FINAL_OBS_PER_STEP != 1) { printf("the flag is bit 0\n"); return 1; }

  cases1d("transport rollout", pdegym_transport_rollout, NULL, 0);
  cases1d("parabolic rollout", pdegym_parabolic_rollout, NULL, 1);
  cases1d("transport backstep rollout", NULL, pdegym_transport_backstep_rollout, 0);
  cases1d("parabolic backstep rollout", NULL, pdegym_parabolic_backstep_rollout, 1);
  cases_traffic(0);
  cases_traffic(1);

  call_tumor c;
  c = good_tumor(21); c.w.final_obs = NULL; expect_flag("tumor rollout: flag with final_obs=NULL", ROLLTU(c), -3);
  c = good_tumor(21); c.w.final_obs = NULL; c.r.reserved_ = 0x7ffffffe; expect_launch("tumor rollout: launch (every bit but bit 0, no final_obs)", ROLLTU(c));
  c = good_tumor(21); c.r.reserved_ = 0; expect_launch("tumor rollout: launch (flag clear)", ROLLTU(c));
  c = good_tumor(21); expect_launch("tumor rollout: launch (flag set)", ROLLTU(c));

  pdegym_mlp n = net_good(64);
  void* x = FAKE(7); void* y = FAKE(9); const uint8_t* rows = FAKE(24); const uint8_t* rows_not = (const uint8_t*)FAKE(25) + 3;
  expect_code("masked forward: rows=NULL", pdegym_mlp_forward_masked(&n, x, 9, y, 1, NULL, rows_not, 37, NULL), -1);
  expect_code("masked forward: rows=NULL, rows_not=NULL", pdegym_mlp_forward_masked(&n, x, 9, y, 1, NULL, NULL, 37, NULL), -1);
  expect_code("masked forward: NULL net", pdegym_mlp_forward_masked(NULL, x, 9, y, 1, rows, NULL, 37, NULL), -3);
  expect_code("masked forward: x=NULL", pdegym_mlp_forward_masked(&n, NULL, 9, y, 1, rows, NULL, 37, NULL), -3);
  expect_code("masked forward: y=NULL", pdegym_mlp_forward_masked(&n, x, 9, NULL, 1, rows, NULL, 37, NULL), -3);
  expect_code("masked forward: B=-1", pdegym_mlp_forward_masked(&n, x, 9, y, 1, rows, NULL, -1, NULL), -2);
  expect_code("masked forward: x_stride < in_dim", pdegym_mlp_forward_masked(&n, x, 8, y, 1, rows, NULL, 37, NULL), -2);
  expect_code("masked forward: y_stride < out_dim", pdegym_mlp_forward_masked(&n, x, 9, y, 0, rows, NULL, 37, NULL), -2);
  n = net_good(64); n.layer[1].w = (const float*)((const char*)n.layer[1].w + 4);
  expect_code("masked forward: blocked weights off 16 bytes", pdegym_mlp_forward_masked(&n, x, 9, y, 1, rows, NULL, 37, NULL), -2);
  n = net_good(257); expect_code("masked forward: 257 units", pdegym_mlp_forward_masked(&n, x, 9, y, 1, rows, NULL, 37, NULL), -2);
  n = net_good(64); n.y_f64 = 1; expect_code("masked forward: float64 y", pdegym_mlp_forward_masked(&n, x, 9, y, 1, rows, NULL, 37, NULL), -2);
  n = net_good(64); n.noise = FAKE(30); n.noise_stride = 1; expect_code("masked forward: noise", pdegym_mlp_forward_masked(&n, x, 9, y, 1, rows, NULL, 37, NULL), -2);
  n = net_good(64); n.layer[2].out_dim = 2; n.head = PDEGYM_MLP_HEAD_SQUASHED_GAUSSIAN; n.clamp = 1; n.lo = -1; n.hi = 1; n.log_std_min = -20; n.log_std_max = 2;
  expect_code("masked forward: squashed-Gaussian head", pdegym_mlp_forward_masked(&n, x, 9, y, 1, rows, NULL, 37, NULL), -2);
  n = net_good(64); n.clamp = 1; n.lo = 1; n.hi = -1; expect_code("masked forward: clamp lo > hi", pdegym_mlp_forward_masked(&n, x, 9, y, 1, rows, NULL, 37, NULL), -2);
  n = net_good(64);
  ++n_calls;
  if (pdegym_mlp_forward_masked(&n, x, 9, y, 1, rows, NULL, 0, NULL) != 0) { ++n_bad; printf("UNEXPECTED masked forward B=0 is not a no-op\n"); }
  expect_launch("masked forward: launch (64 units)", pdegym_mlp_forward_masked(&n, x, 9, y, 1, rows, NULL, 37, NULL));
  expect_launch("masked forward: launch (rows_not, odd address)", pdegym_mlp_forward_masked(&n, x, 9, y, 1, rows + 1, rows_not, 37, NULL));
  n = net_good(65); expect_launch("masked forward: launch (65 units)", pdegym_mlp_forward_masked(&n, x, 9, y, 1, rows, rows_not, 37, NULL));
  n = net_good(256); n.x_f64 = 1; n.clamp = 1; n.lo = -1; n.hi = 1;
  expect_launch("masked forward: launch (256 units, float64 rows, clamp)", pdegym_mlp_forward_masked(&n, x, 9, y, 1, rows, NULL, 37, NULL));

  printf("calls %d bad %d\n", n_calls, n_bad);
  if (n_bad) return 1;
  printf("TERMINAL-OBS-VALIDATION-OK\n");
  return 0;
}
