/* backstep_rollout_validation.c -- argument validation of pdegym_{transport,parabolic}_backstep_rollout (include/pdegym.h) WITHOUT a
 * GPU: null pointers, a plant outside the kernel's corner, an inconsistent law descriptor.  Every bad call must come back with a
 * negative code and a message in pdegym_last_error(); tests/test_backstep_rollout.py links it against the host half of the library
 * built with AddressSanitizer and UndefinedBehaviorSanitizer.  The last group hands over well-formed arguments with fake device
 * addresses: the host code then runs up to the launch, which fails cleanly on a machine without a device (the pointers are never
 * dereferenced on the host). */
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "pdegym.h"

static int n_calls = 0, n_bad = 0;

static void expect_error(const char* what, int rc) {
  const char* msg = pdegym_last_error();
  ++n_calls;
  if (rc >= 0 || msg == NULL || msg[0] == '\0') {
    ++n_bad;
    printf("UNEXPECTED %s -> %d \"%s\"\n", what, rc, msg ? msg : "(null)");
  } else {
    printf("%-44s %5d  %s\n", what, rc, msg);
  }
}

/* refused by the validation (code -2, a message about the row), not by a launch that found no device (-100) */
static void expect_refused_row(const char* what, int rc) {
  const char* msg = pdegym_last_error();
  ++n_calls;
  if (rc != -2 || msg == NULL || strstr(msg, "rows of up to") == NULL) {
    ++n_bad;
    printf("UNEXPECTED %s -> %d \"%s\"\n", what, rc, msg ? msg : "(null)");
  } else {
    printf("%-44s %5d  %s\n", what, rc, msg);
  }
}

static void expect_launch(const char* what, int rc) {      /* validation passed: only the launch failed, for want of a device */
  ++n_calls;
  if (rc != -100) {
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

#define FAKE(k) ((void*)(uintptr_t)(0x7f0000000000ull + 4096ull * (k)))

typedef int (*entry_fn)(const pdegym_params1d*, const pdegym_bufs1d*, const pdegym_rollout1d*, const pdegym_backstep*, int32_t, void*);

typedef struct call {
  pdegym_params1d p;
  pdegym_bufs1d b;
  pdegym_rollout1d r;
  pdegym_backstep l;
} call;

/* a well-formed call on rows of n nodes: per-instance gains, the pool rule, noise and clamp */
static call good(int n) {
  call c;
  memset(&c, 0, sizeof c);
  c.p.n = n; c.p.nt = 1001; c.p.substeps = 100; c.p.control_type = PDEGYM_CONTROL_DIRICHLET; c.p.sensing = PDEGYM_SENSE_FULL;
  c.p.limit_state = 1; c.p.reward_kind = PDEGYM_REWARD_TUNED1D; c.p.reward_nt = 1000; c.p.dt = 1e-4f; c.p.dx = 1e-2f; c.p.F = 0.25f;
  c.p.max_control = 20; c.p.max_state = 1e10f; c.p.truncate_penalty = -1e3f; c.p.terminate_reward = 3e2f; c.p.rdx = 100.0;
  c.p.dt64 = 1e-4; c.p.dx64 = 1e-2; c.p.max_control64 = 20;
  c.b.beta = FAKE(1); c.b.beta_stride = n; c.b.time_index = FAKE(2); c.b.bsum = FAKE(3); c.b.ring = FAKE(4); c.b.norm_now = FAKE(5);
  c.b.norm_back = FAKE(6); c.b.reset_init = FAKE(7); c.b.reset_beta = FAKE(8); c.b.reset_count = FAKE(9); c.b.reset_pool_rows = 7;
  c.r.T = 8; c.r.obs = FAKE(10); c.r.actions = FAKE(11); c.r.rewards = FAKE(12); c.r.terminated = FAKE(13); c.r.truncated = FAKE(14);
  c.l.gain0 = FAKE(15); c.l.gain_stride = n; c.l.m = n; c.l.len = n - 1; c.l.gain_pool = FAKE(16); c.l.reset_count = FAKE(9);
  c.l.pool_rows = 7; c.l.order = PDEGYM_BACKSTEP_ORDERED; c.l.scale = 1e-2; c.l.noise = FAKE(17); c.l.clamp = 1; c.l.lo = -20; c.l.hi = 20;
  return c;
}

#define RUN(c) f(&(c).p, &(c).b, &(c).r, &(c).l, 6, NULL)

int main(void) {
  if (pdegym_abi_version() != PDEGYM_ABI_VERSION) { printf("ABI mismatch\n"); return 1; }
  const entry_fn entries[2] = {pdegym_transport_backstep_rollout, pdegym_parabolic_backstep_rollout};
  for (int k = 0; k < 2; ++k) {
    entry_fn f = entries[k];
    call c = good(101);
    /* null pointers */
    expect_error("NULL params", f(NULL, &c.b, &c.r, &c.l, 6, NULL));
    expect_error("NULL bufs", f(&c.p, NULL, &c.r, &c.l, 6, NULL));
    expect_error("NULL rollout", f(&c.p, &c.b, NULL, &c.l, 6, NULL));
    expect_error("NULL law", f(&c.p, &c.b, &c.r, NULL, 6, NULL));
    expect_ok("B=0", f(&c.p, &c.b, &c.r, &c.l, 0, NULL));
    c = good(101); c.r.T = 0; expect_ok("T=0", RUN(c));
    c = good(101); c.b.beta = NULL; expect_error("beta=NULL", RUN(c));
    c = good(101); c.b.time_index = NULL; expect_error("time_index=NULL", RUN(c));
    c = good(101); c.b.bsum = NULL; expect_error("bsum=NULL", RUN(c));
    c = good(101); c.b.ring = NULL; expect_error("ring=NULL", RUN(c));
    c = good(101); c.b.norm_now = NULL; expect_error("norm_now=NULL", RUN(c));
    c = good(101); c.b.norm_back = NULL; expect_error("norm_back=NULL", RUN(c));
    c = good(101); c.r.obs = NULL; expect_error("obs=NULL", RUN(c));
    c = good(101); c.r.actions = NULL; expect_error("actions=NULL", RUN(c));
    c = good(101); c.r.rewards = NULL; expect_error("rewards=NULL with a reward", RUN(c));
    c = good(101); c.r.terminated = NULL; expect_error("terminated=NULL", RUN(c));
    c = good(101); c.r.truncated = NULL; expect_error("truncated=NULL", RUN(c));
    c = good(101); c.l.gain0 = NULL; expect_error("gain0=NULL", RUN(c));
    /* the plant outside the kernel's corner */
    c = good(101); c.p.control_type = PDEGYM_CONTROL_NEUMANN; expect_error("Neumann actuation", RUN(c));
    c = good(101); c.p.control_type = 7; expect_error("control_type=7", RUN(c));
    c = good(101); c.p.sensing = PDEGYM_SENSE_LAST; c.b.u = FAKE(20); expect_error("scalar sensing (last)", RUN(c));
    c = good(101); c.p.sensing = PDEGYM_SENSE_FIRST_DERIV; c.b.u = FAKE(20); expect_error("scalar sensing (first deriv)", RUN(c));
    c = good(101); c.p.sensing = -1; expect_error("sensing=-1", RUN(c));
    c = good(101); c.p.beta_f64 = 1; expect_error("beta_f64", RUN(c));
    c = good(101); c.p.action_kind = PDEGYM_ACTION_F64; expect_error("action_kind=F64", RUN(c));
    c = good(101); c.p.action_kind = PDEGYM_ACTION_WEAK; expect_error("action_kind=WEAK", RUN(c));
    c = good(101); c.b.history = FAKE(21); expect_error("history", RUN(c));
    c = good(101); c.p.reward_kind = PDEGYM_REWARD_NORM_L2; c.p.reward_horizon = PDEGYM_HORIZON_DIFFERENTIAL; expect_error("differential horizon", RUN(c));
    c = good(101); c.p.reward_kind = PDEGYM_REWARD_NORM_L2; c.p.reward_horizon = PDEGYM_HORIZON_T; c.p.reward_t_horizon = 5; expect_error("t-horizon", RUN(c));
    c = good(101); c.p.flux = PDEGYM_FLUX_BURGERS; expect_error("Burgers flux", RUN(c));
    c = good(514); expect_refused_row("n=514", RUN(c));
    /* a transport row has no node outside the slots: 513 nodes are 9 slots per lane, one more than the widest instantiation */
    if (k == 0) { c = good(513); expect_refused_row("transport n=513", RUN(c)); }
    if (k == 0) { c = good(513); c.l.order = PDEGYM_BACKSTEP_TREE; expect_refused_row("transport n=513 (tree)", RUN(c)); }
    if (k == 0) { c = good(512); expect_launch("transport n=512", RUN(c)); }
    if (k == 1) { c = good(513); expect_launch("parabolic n=513", RUN(c)); }
    c = good(2048); expect_error("n=2048", RUN(c));
    c = good(101); c.p.n = 2; c.l.len = 1; expect_error("n=2", RUN(c));
    c = good(101); c.p.nt = 1; expect_error("nt=1", RUN(c));
    c = good(101); c.p.substeps = 0; expect_error("substeps=0", RUN(c));
    c = good(101); c.r.policy = (const struct pdegym_mlp_s*)FAKE(22); expect_error("policy given", RUN(c));
    /* the law */
    c = good(101); c.l.obs = FAKE(23); expect_error("law.obs given", RUN(c));
    c = good(101); c.l.out64 = FAKE(24); expect_error("law.out64 given", RUN(c));
    c = good(101); c.l.out32 = FAKE(25); expect_error("law.out32 given", RUN(c));
    c = good(101); c.l.m = 0; expect_error("m=0", RUN(c));
    c = good(101); c.l.len = 0; expect_error("len=0", RUN(c));
    c = good(101); c.l.len = -3; expect_error("len=-3", RUN(c));
    c = good(101); c.l.m = 50; c.l.gain_stride = 50; c.l.len = 51; expect_error("len>m", RUN(c));
    c = good(101); c.l.m = 200; c.l.gain_stride = 200; c.l.len = 102; expect_error("len>n", RUN(c));
    c = good(101); c.l.gain_stride = 100; expect_error("gain_stride<m", RUN(c));
    c = good(101); c.l.gain_stride = -101; expect_error("gain_stride<0", RUN(c));
    c = good(101); c.l.order = 2; expect_error("order=2", RUN(c));
    c = good(101); c.l.order = -1; expect_error("order=-1", RUN(c));
    c = good(101); c.l.reset_count = NULL; expect_error("pool without reset_count", RUN(c));
    c = good(101); c.l.reset_count = FAKE(26); expect_error("law and plant count differently", RUN(c));
    c = good(101); c.l.pool_rows = -1; expect_error("pool_rows=-1", RUN(c));
    c = good(101); c.l.lo = 1; c.l.hi = -1; expect_error("lo>hi", RUN(c));
    c = good(101); c.l.lo = NAN; expect_error("lo=nan", RUN(c));
    c = good(101); c.l.hi = NAN; expect_error("hi=nan", RUN(c));

    /* well-formed calls: the host side picks an instantiation and runs up to the launch; without a device that launch fails with a
     * message.  Rows of every slots-per-lane count, the FULL sizes among them, both orders, with and without the optional parts. */
    const int ns[] = {3, 40, 64, 65, 100, 101, 128, 129, 150, 200, 256, 257, 300, 321, 400, 449, 512, 513};
    for (unsigned i = 0; i < sizeof ns / sizeof ns[0]; ++i) {
      if (k == 0 && ns[i] > 512) continue;      /* the longest transport row is 512 nodes (refused above) */
      c = good(ns[i]); expect_error("launch without a device (ordered, pool)", RUN(c));
      c = good(ns[i]); c.l.order = PDEGYM_BACKSTEP_TREE; c.l.gain_pool = NULL; c.l.reset_count = NULL; c.l.gain_stride = 0; c.l.noise = NULL;
      c.l.clamp = 0; c.l.len = ns[i]; c.b.reset_init = NULL; c.b.reset_beta = NULL; c.b.reset_count = NULL;
      expect_error("launch without a device (tree, shared row)", RUN(c));
    }
    c = good(101); c.r.obs_noise = FAKE(27); c.r.obs_seen = FAKE(28); expect_error("launch with obs_noise / obs_seen", RUN(c));
    c = good(101); c.b.reset_count = NULL; expect_error("launch, plant without a counter", RUN(c));
    c = good(101); c.p.reward_kind = PDEGYM_REWARD_NONE; c.r.rewards = NULL; expect_error("launch without rewards", RUN(c));
  }
  printf("calls %d bad %d\n", n_calls, n_bad);
  if (n_bad) return 1;
  printf("BACKSTEP-ROLLOUT-VALIDATION-OK\n");
  return 0;
}
