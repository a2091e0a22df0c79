/* tumor_rollout_validation.c -- argument validation of pdegym_tumor_therapy_step / pdegym_tumor_rollout (include/pdegym.h) WITHOUT a
 * GPU: null pointers, rows out of range, history recording, weekends without an observation buffer, an inconsistent init stride,
 * policies that do not match the row or do not fit the LDS next to the rows.  Every bad call must come back with a negative code
 * and a message in pdegym_last_error(); tests/test_tumor_rollout.py links it against the host half of the library built with
 * AddressSanitizer and UndefinedBehaviorSanitizer.  The last group hands over well-formed arguments with fake device addresses: the
 * host code then runs up to the launch, which fails cleanly on a machine without a device (the pointers are never dereferenced on
 * the host). */
#include <stdio.h>
#include <string.h>

#include "pdegym.h"

static int n_calls = 0, n_bad = 0;

/* refused by the validation (not by a launch that found no device: -100, nor by the LDS limit that needs one: -4) */
static void expect_refused(const char* what, int rc) {
  const char* msg = pdegym_last_error();
  ++n_calls;
  if (rc >= 0 || rc == -100 || rc == -4 || msg == NULL || msg[0] == '\0') {
    ++n_bad;
    printf("UNEXPECTED %s -> %d \"%s\"\n", what, rc, msg ? msg : "(null)");
  } else {
    printf("%-60s %5d  %s\n", what, rc, msg);
  }
}

/* validation passed: only the launch (or, with a policy, raising the kernel's LDS limit) failed, for want of a device */
static void expect_launch(const char* what, int rc) {
  ++n_calls;
  if (rc != -100 && rc != -4) {
    ++n_bad;
    printf("UNEXPECTED %s -> %d \"%s\"\n", what, rc, pdegym_last_error());
  }
}

static void expect_ok(const char* what, int rc) {
  ++n_calls;
  if (rc != 0) {
    ++n_bad;
    printf("UNEXPECTED %s -> %d \"%s\"\n", what, rc, pdegym_last_error());
  }
}

#define FAKE(k) ((void*)(uintptr_t)(0x7f0000000000ull + 65536ull * (k)))

typedef struct call {
  pdegym_params_tumor p;
  pdegym_bufs_tumor b;
  pdegym_wrap_tumor w;
  pdegym_rollout_tumor r;
  pdegym_mlp net;
} call;

/* a well-formed call on rows of nx nodes: weekends, per-patient initial rows, both optional outputs; no policy */
static call good(int nx) {
  call c;
  memset(&c, 0, sizeof c);
  c.p.nx = nx; c.p.nt = 601; c.p.dt = 1; c.p.dx = 1; c.p.dx2 = 1; c.p.D = 0.2; c.p.rho = 0.03; c.p.alpha = 0.04; c.p.alpha_beta_ratio = 10;
  c.p.k = 1e5; c.p.thr_t1 = 8e4; c.p.thr_t2 = 1.6e4; c.p.detect_radius = 15; c.p.death_radius = 35; c.p.total_dosage = 61.2;
  c.p.dose_end = 0.1; c.p.margin = 25;
  c.b.u = FAKE(1); c.b.xscale = FAKE(2); c.b.control = FAKE(3); c.b.time_index = FAKE(4); c.b.stage = FAKE(5); c.b.remaining = FAKE(6);
  c.b.days = FAKE(7); c.b.t_benchmark = FAKE(8); c.b.reward = FAKE(9); c.b.terminated = FAKE(10); c.b.truncated = FAKE(11); c.b.out = FAKE(12);
  c.w.weekends = 1; c.w.init = FAKE(13); c.w.init_stride = nx; c.w.consecutive = FAKE(14); c.w.treatment_calls = FAKE(15);
  c.w.soft_constraint_violations = FAKE(16); c.w.final_obs = FAKE(17); c.w.obs = FAKE(18);
  c.r.T = 8; c.r.obs = FAKE(19); c.r.actions = FAKE(20); c.r.rewards = FAKE(21); c.r.terminated = FAKE(22); c.r.truncated = FAKE(23);
  return c;
}

/* nx -> hidden -> hidden -> 1, tanh, clamp [0, 1], noise [T, B] */
static void with_policy(call* c, int hidden) {
  memset(&c->net, 0, sizeof c->net);
  c->net.n_layers = 3; c->net.clamp = 1; c->net.lo = 0.f; c->net.hi = 1.f; c->net.noise = (const float*)FAKE(30); c->net.noise_stride = 1;
  const int dims[4] = {c->p.nx, hidden, hidden, 1};
  for (int l = 0; l < 3; ++l) {
    c->net.layer[l].w = (const float*)FAKE(31 + 2 * l);
    c->net.layer[l].b = (const float*)FAKE(32 + 2 * l);
    c->net.layer[l].in_dim = dims[l]; c->net.layer[l].out_dim = dims[l + 1];
    c->net.layer[l].act = l < 2 ? PDEGYM_MLP_TANH : PDEGYM_MLP_IDENTITY;
  }
  c->r.policy = &c->net;
}

#define STEP(c) pdegym_tumor_therapy_step(&(c).p, &(c).b, &(c).w, 6, NULL)
#define ROLL(c) pdegym_tumor_rollout(&(c).p, &(c).b, &(c).w, &(c).r, 6, NULL)

int main(void) {
  if (pdegym_abi_version() != PDEGYM_ABI_VERSION) { printf("ABI mismatch\n"); return 1; }
  call c = good(201);
  /* ---- null pointers */
  expect_refused("step: NULL params", pdegym_tumor_therapy_step(NULL, &c.b, &c.w, 6, NULL));
  expect_refused("step: NULL bufs", pdegym_tumor_therapy_step(&c.p, NULL, &c.w, 6, NULL));
  expect_refused("step: NULL wrap", pdegym_tumor_therapy_step(&c.p, &c.b, NULL, 6, NULL));
  expect_refused("rollout: NULL params", pdegym_tumor_rollout(NULL, &c.b, &c.w, &c.r, 6, NULL));
  expect_refused("rollout: NULL bufs", pdegym_tumor_rollout(&c.p, NULL, &c.w, &c.r, 6, NULL));
  expect_refused("rollout: NULL wrap", pdegym_tumor_rollout(&c.p, &c.b, NULL, &c.r, 6, NULL));
  expect_refused("rollout: NULL rollout", pdegym_tumor_rollout(&c.p, &c.b, &c.w, NULL, 6, NULL));
  expect_ok("step: B=0", pdegym_tumor_therapy_step(&c.p, &c.b, &c.w, 0, NULL));
  expect_ok("step: B=-1", pdegym_tumor_therapy_step(&c.p, &c.b, &c.w, -1, NULL));
  expect_ok("rollout: B=0", pdegym_tumor_rollout(&c.p, &c.b, &c.w, &c.r, 0, NULL));
  c = good(201); c.r.T = 0; expect_ok("rollout: T=0 (nothing to do)", ROLL(c));
  /* ---- both entries: the engine and the wrapper's state */
  for (int k = 0; k < 2; ++k) {
#define RUN(c) (k == 0 ? STEP(c) : ROLL(c))
    c = good(2); expect_refused("nx=2", RUN(c));
    c = good(4097); expect_refused("nx=4097", RUN(c));
    c = good(201); c.p.nt = 1; expect_refused("nt=1", RUN(c));
    c = good(201); c.b.u = NULL; expect_refused("u=NULL", RUN(c));
    c = good(201); c.b.time_index = NULL; expect_refused("time_index=NULL", RUN(c));
    c = good(201); c.b.stage = NULL; expect_refused("stage=NULL", RUN(c));
    c = good(201); c.b.remaining = NULL; expect_refused("remaining=NULL", RUN(c));
    c = good(201); c.b.days = NULL; expect_refused("days=NULL", RUN(c));
    c = good(201); c.b.xscale = NULL; expect_refused("xscale=NULL", RUN(c));
    c = good(201); c.b.reward = NULL; expect_refused("reward=NULL", RUN(c));
    c = good(201); c.b.terminated = NULL; expect_refused("terminated=NULL", RUN(c));
    c = good(201); c.b.truncated = NULL; expect_refused("truncated=NULL", RUN(c));
    c = good(201); c.b.out = NULL; expect_refused("out=NULL", RUN(c));
    c = good(201); c.b.history = FAKE(40); expect_refused("history recording", RUN(c));
    c = good(201); c.b.t1_log = FAKE(41); expect_refused("t1_log recording", RUN(c));
    c = good(201); c.w.init = NULL; expect_refused("init=NULL", RUN(c));
    c = good(201); c.w.init_stride = 200; expect_refused("init_stride<nx", RUN(c));
    c = good(201); c.w.init_stride = -201; expect_refused("init_stride<0", RUN(c));
    c = good(201); c.w.consecutive = NULL; expect_refused("consecutive=NULL", RUN(c));
    c = good(201); c.w.treatment_calls = NULL; expect_refused("treatment_calls=NULL", RUN(c));
    c = good(201); c.w.soft_constraint_violations = NULL; expect_refused("soft_constraint_violations=NULL", RUN(c));
#undef RUN
  }
  /* ---- the step alone */
  c = good(201); c.b.control = NULL; expect_refused("step: control=NULL", STEP(c));
  c = good(201); c.w.obs = NULL; expect_refused("step: weekends without obs", STEP(c));
  /* ---- the rollout alone */
  c = good(201); c.r.obs = NULL; expect_refused("rollout: obs=NULL", ROLL(c));
  c = good(201); c.r.actions = NULL; expect_refused("rollout: actions=NULL", ROLL(c));
  c = good(201); c.r.rewards = NULL; expect_refused("rollout: rewards=NULL", ROLL(c));
  c = good(201); c.r.terminated = NULL; expect_refused("rollout: terminated=NULL", ROLL(c));
  c = good(201); c.r.truncated = NULL; expect_refused("rollout: truncated=NULL", ROLL(c));
  c = good(201); with_policy(&c, 64); c.net.layer[0].in_dim = 200; expect_refused("policy: 200 inputs on rows of 201", ROLL(c));
  c = good(201); with_policy(&c, 64); c.net.layer[2].out_dim = 2; expect_refused("policy: two outputs", ROLL(c));
  c = good(201); with_policy(&c, 64); c.net.layer[1].w = NULL; expect_refused("policy: NULL weights", ROLL(c));
  /* the blocked weights are 16-byte aligned by the header, in the narrow (64) and the cooperative (256) evaluation alike: -2 and the
   * argument's name before the launch; the float64 arrays of the call need 8 bytes only */
  for (int hidden = 64; hidden <= 256; hidden += 192)
    for (int off = 4; off < 16; off += 4) {
      c = good(201); with_policy(&c, hidden); c.net.layer[2].w = (const float*)((const char*)c.net.layer[2].w + off);
      const int rc = ROLL(c);
      expect_refused("policy: blocked weights off a 16-byte boundary", rc);
      if (rc != -2 || strstr(pdegym_last_error(), "layer weights (w) must be 16-byte aligned") == NULL) { ++n_bad; printf("UNEXPECTED code or message for displaced policy weights\n"); }
    }
  c = good(201); with_policy(&c, 64); c.b.u += 1; c.r.obs += 1; c.r.actions += 1; c.r.rewards += 1; c.w.final_obs += 1;
  c.r.terminated += 1; c.r.truncated += 3; c.net.noise += 1; c.net.layer[0].b += 1;
  expect_launch("rollout with a 64-64 policy, every element-aligned pointer displaced", ROLL(c));
  c = good(201); with_policy(&c, 257); expect_refused("policy: 257 units", ROLL(c));
  c = good(201); with_policy(&c, 64); c.net.n_layers = 5; expect_refused("policy: 5 layers", ROLL(c));
  c = good(201); with_policy(&c, 64); c.net.lo = 2.f; expect_refused("policy: lo>hi", ROLL(c));
  c = good(201); with_policy(&c, 64); c.net.noise_stride = 0; expect_refused("policy: noise_stride=0", ROLL(c));
  c = good(201); with_policy(&c, 64); c.net.layer[0].act = 7; expect_refused("policy: unknown activation", ROLL(c));
  /* the LDS budget: the policy's floats and 16 x 2 rows of nx doubles within 160 KB */
  c = good(701); with_policy(&c, 64); expect_refused("policy 64-64 on rows of 701: rows do not fit", ROLL(c));
  c = good(500); with_policy(&c, 256); expect_refused("policy 256-256 on rows of 500: rows do not fit", ROLL(c));
  c = good(501); with_policy(&c, 8); expect_refused("policy 8-8 on rows of 501: rows do not fit", ROLL(c));
  c = good(4096); with_policy(&c, 8); expect_refused("policy on rows of 4096", ROLL(c));

  /* ---- well-formed calls: the host side picks an instantiation and runs up to the launch; without a device that fails with a
   * message.  Rows on both staging paths, the workgroup shapes of the form without a policy, both policy forms. */
  const int rows[] = {3, 70, 201, 256, 257, 300, 1024, 1025, 2048, 2049, 4096};
  for (unsigned i = 0; i < sizeof rows / sizeof rows[0]; ++i) {
    c = good(rows[i]); expect_launch("step launch without a device", STEP(c));
    c = good(rows[i]); c.w.weekends = 0; c.w.obs = NULL; c.w.final_obs = NULL; c.w.init_stride = 0; c.b.t_benchmark = NULL;
    expect_launch("step launch without a device (bare)", STEP(c));
    c = good(rows[i]); expect_launch("rollout launch without a device", ROLL(c));
    c = good(rows[i]); c.w.obs = NULL; c.r.T = 1; expect_launch("rollout launch without a device (weekends need no wrap obs)", ROLL(c));
  }
  const int prows[] = {3, 70, 201, 300};
  for (unsigned i = 0; i < sizeof prows / sizeof prows[0]; ++i) {
    c = good(prows[i]); with_policy(&c, 64);
    if (prows[i] <= 201) expect_launch("rollout with a 64-64 policy", ROLL(c));
    else expect_refused("policy 64-64 on rows of 300: 120 KB of weights and rows + 75 KB of patient rows", ROLL(c));
    c = good(prows[i]); with_policy(&c, 256); expect_launch("rollout with a 256-256 policy", ROLL(c));
    c = good(prows[i]); with_policy(&c, 65); c.net.noise = NULL; c.net.clamp = 0; expect_launch("rollout with a 65-65 policy, bare", ROLL(c));
  }
  printf("calls %d bad %d\n", n_calls, n_bad);
  if (n_bad) return 1;
  printf("TUMOR-ROLLOUT-VALIDATION-OK\n");
  return 0;
}
