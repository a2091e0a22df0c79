/* traffic_backstep_validation.c -- argument validation of pdegym_traffic_backstep_control / _rollout (include/pdegym.h) WITHOUT a GPU:
 * null pointers, the train simulation types, rows out of range, the numpy order on a row np.trapz would halve, T < 1, an inconsistent
 * law descriptor.  Every bad call must come back with a negative code and a message in pdegym_last_error();
 * tests/test_traffic_backstep.py links it against the host half of the library built with AddressSanitizer and
 * UndefinedBehaviorSanitizer.  The last group hands over well-formed arguments with fake device addresses: the host code then runs up
 * to the launch, which fails cleanly on a machine without a device (the pointers are never dereferenced on the host). */
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
    printf("%-52s %5d  %s\n", what, rc, msg);
  }
}

/* refused by the validation (not by a launch that found no device: -100) */
static void expect_refused(const char* what, int rc) {
  const char* msg = pdegym_last_error();
  ++n_calls;
  if (rc >= 0 || rc == -100 || msg == NULL || msg[0] == '\0') {
    ++n_bad;
    printf("UNEXPECTED %s -> %d \"%s\"\n", what, rc, msg ? msg : "(null)");
  } else {
    printf("%-52s %5d  %s\n", what, rc, msg);
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

typedef struct call {
  pdegym_params_traffic p;
  pdegym_bufs_traffic b;
  pdegym_rollout_traffic r;
  pdegym_traffic_backstep l;
} call;

/* a well-formed call on freeways of M nodes: per-instance weights, noise and clamp, the fused auto-reset */
static call good(int M, int sim, int order) {
  call c;
  memset(&c, 0, sizeof c);
  c.p.M = M; c.p.control_freq = 2; c.p.sim = sim; c.p.limit = 1; c.p.dt = 0.25; c.p.dx = 10; c.p.T = 240; c.p.vm = 40; c.p.rm = 0.16; c.p.tau = 60;
  c.b.r = FAKE(1); c.b.y = FAKE(2); c.b.time = FAKE(3); c.b.rs = FAKE(4); c.b.qs_clip = FAKE(5);
  c.b.action_stride = sim == PDEGYM_TRAFFIC_BOTH ? 2 : 1;
  c.b.reset_rs = FAKE(6); c.b.reset_profile = FAKE(7); c.b.final_obs = FAKE(8); c.b.reset_count = FAKE(9); c.b.reset_pool_rows = 7;
  c.r.T = 8; c.r.obs = FAKE(10); c.r.actions = FAKE(11); c.r.rewards = FAKE(12); c.r.done = FAKE(13); c.r.truncated = FAKE(14);
  c.l.weights_v = FAKE(15); c.l.weights_q = FAKE(16); c.l.weight_stride = M; c.l.order = order; c.l.noise = FAKE(17);
  c.l.noise_stride = c.b.action_stride; c.l.clamp = 1; c.l.lo = 0.96; c.l.hi = 1.44;
  return c;
}

#define CTRL(c) pdegym_traffic_backstep_control(&(c).p, &(c).l, FAKE(20), 2 * (c).p.M, FAKE(4), FAKE(21), (c).b.action_stride, 6, NULL)
#define ROLL(c) pdegym_traffic_backstep_rollout(&(c).p, &(c).b, &(c).r, &(c).l, 6, NULL)
#define OUT PDEGYM_TRAFFIC_OUTLET
#define NPY PDEGYM_TRAFFIC_BACKSTEP_NUMPY
#define TREE PDEGYM_TRAFFIC_BACKSTEP_TREE

int main(void) {
  if (pdegym_abi_version() != PDEGYM_ABI_VERSION) { printf("ABI mismatch\n"); return 1; }
  call c = good(51, OUT, NPY);
  /* ---- control: null pointers */
  expect_error("control: NULL params", pdegym_traffic_backstep_control(NULL, &c.l, FAKE(20), 102, FAKE(4), FAKE(21), 1, 6, NULL));
  expect_error("control: NULL law", pdegym_traffic_backstep_control(&c.p, NULL, FAKE(20), 102, FAKE(4), FAKE(21), 1, 6, NULL));
  expect_error("control: NULL obs", pdegym_traffic_backstep_control(&c.p, &c.l, NULL, 102, FAKE(4), FAKE(21), 1, 6, NULL));
  expect_error("control: NULL rs", pdegym_traffic_backstep_control(&c.p, &c.l, FAKE(20), 102, NULL, FAKE(21), 1, 6, NULL));
  expect_error("control: NULL out", pdegym_traffic_backstep_control(&c.p, &c.l, FAKE(20), 102, FAKE(4), NULL, 1, 6, NULL));
  expect_error("control: B=-1", pdegym_traffic_backstep_control(&c.p, &c.l, FAKE(20), 102, FAKE(4), FAKE(21), 1, -1, NULL));
  expect_ok("control: B=0", pdegym_traffic_backstep_control(&c.p, &c.l, FAKE(20), 102, FAKE(4), FAKE(21), 1, 0, NULL));
  expect_error("control: obs_stride<2M", pdegym_traffic_backstep_control(&c.p, &c.l, FAKE(20), 101, FAKE(4), FAKE(21), 1, 6, NULL));
  expect_error("control: out_stride=0", pdegym_traffic_backstep_control(&c.p, &c.l, FAKE(20), 102, FAKE(4), FAKE(21), 0, 6, NULL));
  c = good(51, PDEGYM_TRAFFIC_BOTH, NPY);
  expect_error("control: 'both' with out_stride=1", pdegym_traffic_backstep_control(&c.p, &c.l, FAKE(20), 102, FAKE(4), FAKE(21), 1, 6, NULL));
  /* ---- both entries: the plant and the law */
  for (int k = 0; k < 2; ++k) {
#define RUN(c) (k == 0 ? CTRL(c) : ROLL(c))
    c = good(51, PDEGYM_TRAFFIC_OUTLET_TRAIN, NPY); expect_refused("outlet-train", RUN(c));
    c = good(51, 4, NPY); expect_refused("sim=4 (inlet-train)", RUN(c));
    c = good(51, -1, NPY); expect_refused("sim=-1", RUN(c));
    c = good(3, OUT, NPY); expect_refused("M=3", RUN(c));
    c = good(0, OUT, TREE); expect_refused("M=0", RUN(c));
    c = good(1025, OUT, TREE); expect_refused("M=1025", RUN(c));
    c = good(130, OUT, NPY); expect_refused("numpy order, M=130", RUN(c));
    c = good(1024, OUT, NPY); expect_refused("numpy order, M=1024", RUN(c));
    c = good(51, OUT, 2); expect_refused("order=2", RUN(c));
    c = good(51, OUT, -1); expect_refused("order=-1", RUN(c));
    c = good(51, OUT, NPY); c.p.dx = 0; expect_refused("dx=0", RUN(c));
    c = good(51, OUT, NPY); c.p.dx = NAN; expect_refused("dx=nan", RUN(c));
    c = good(51, OUT, NPY); c.l.weights_v = NULL; expect_refused("weights_v=NULL", RUN(c));
    c = good(51, OUT, NPY); c.l.weights_q = NULL; expect_refused("weights_q=NULL", RUN(c));
    c = good(51, OUT, NPY); c.l.weight_stride = 50; expect_refused("weight_stride<M", RUN(c));
    c = good(51, OUT, NPY); c.l.weight_stride = -51; expect_refused("weight_stride<0", RUN(c));
    c = good(51, OUT, NPY); c.l.noise_stride = 0; expect_refused("noise_stride=0", RUN(c));
    c = good(51, PDEGYM_TRAFFIC_BOTH, NPY); c.l.noise_stride = 1; expect_refused("'both' with noise_stride=1", RUN(c));
    c = good(51, OUT, NPY); c.l.lo = 2; c.l.hi = 1; expect_refused("lo>hi", RUN(c));
    c = good(51, OUT, NPY); c.l.lo = NAN; expect_refused("lo=nan", RUN(c));
    c = good(51, OUT, NPY); c.l.hi = NAN; expect_refused("hi=nan", RUN(c));
#undef RUN
  }
  /* ---- rollout */
  c = good(51, OUT, NPY);
  expect_error("rollout: NULL params", pdegym_traffic_backstep_rollout(NULL, &c.b, &c.r, &c.l, 6, NULL));
  expect_error("rollout: NULL bufs", pdegym_traffic_backstep_rollout(&c.p, NULL, &c.r, &c.l, 6, NULL));
  expect_error("rollout: NULL rollout", pdegym_traffic_backstep_rollout(&c.p, &c.b, NULL, &c.l, 6, NULL));
  expect_error("rollout: NULL law", pdegym_traffic_backstep_rollout(&c.p, &c.b, &c.r, NULL, 6, NULL));
  expect_error("rollout: B=-1", pdegym_traffic_backstep_rollout(&c.p, &c.b, &c.r, &c.l, -1, NULL));
  expect_ok("rollout: B=0", pdegym_traffic_backstep_rollout(&c.p, &c.b, &c.r, &c.l, 0, NULL));
  c = good(51, OUT, NPY); c.r.T = 0; expect_refused("rollout: T=0", ROLL(c));
  c = good(51, OUT, NPY); c.r.T = -4; expect_refused("rollout: T=-4", ROLL(c));
  c = good(65, OUT, NPY); expect_refused("rollout: M=65", ROLL(c));
  c = good(129, OUT, TREE); expect_refused("rollout: M=129", ROLL(c));
  c = good(51, OUT, NPY); c.p.control_freq = 0; expect_refused("rollout: control_freq=0", ROLL(c));
  c = good(51, OUT, NPY); c.r.policy = (const struct pdegym_mlp_s*)FAKE(22); expect_refused("rollout: policy given", ROLL(c));
  c = good(51, OUT, NPY); c.b.r = NULL; expect_refused("rollout: r=NULL", ROLL(c));
  c = good(51, OUT, NPY); c.b.y = NULL; expect_refused("rollout: y=NULL", ROLL(c));
  c = good(51, OUT, NPY); c.b.time = NULL; expect_refused("rollout: time=NULL", ROLL(c));
  c = good(51, OUT, NPY); c.b.rs = NULL; expect_refused("rollout: rs=NULL", ROLL(c));
  c = good(51, OUT, NPY); c.b.qs_clip = NULL; expect_refused("rollout: qs_clip=NULL", ROLL(c));
  c = good(51, OUT, NPY); c.b.reset_profile = NULL; expect_refused("rollout: reset_rs without reset_profile", ROLL(c));
  c = good(51, OUT, NPY); c.b.reset_pool_rows = -1; expect_refused("rollout: reset_pool_rows=-1", ROLL(c));
  c = good(51, OUT, NPY); c.r.obs = NULL; expect_refused("rollout: obs=NULL", ROLL(c));
  c = good(51, OUT, NPY); c.r.actions = NULL; expect_refused("rollout: actions=NULL", ROLL(c));
  c = good(51, OUT, NPY); c.r.rewards = NULL; expect_refused("rollout: rewards=NULL", ROLL(c));
  c = good(51, OUT, NPY); c.r.done = NULL; expect_refused("rollout: done=NULL", ROLL(c));
  c = good(51, OUT, NPY); c.r.truncated = NULL; expect_refused("rollout: truncated=NULL", ROLL(c));
  c = good(51, OUT, NPY); c.b.action_stride = 2; expect_refused("rollout: outlet with action_stride=2", ROLL(c));
  c = good(51, PDEGYM_TRAFFIC_BOTH, NPY); c.b.action_stride = 1; expect_refused("rollout: 'both' with action_stride=1", ROLL(c));

  /* ---- well-formed calls: the host side picks an instantiation and runs up to the launch; without a device that launch fails with
   * a message.  Every simulation type, both orders, the sizes where the kernels change path. */
  const int sims[3] = {PDEGYM_TRAFFIC_INLET, PDEGYM_TRAFFIC_OUTLET, PDEGYM_TRAFFIC_BOTH};
  const int Ms[] = {4, 9, 12, 51, 64, 65, 129, 200, 1024};
  for (int s = 0; s < 3; ++s)
    for (int o = 0; o < 2; ++o)
      for (unsigned i = 0; i < sizeof Ms / sizeof Ms[0]; ++i) {
        if (o == NPY && Ms[i] > 129) continue;
        c = good(Ms[i], sims[s], o); expect_launch("control launch without a device", CTRL(c));
        c = good(Ms[i], sims[s], o); c.l.noise = NULL; c.l.clamp = 0; c.l.weight_stride = 0;
        expect_launch("control launch without a device (shared row)", CTRL(c));
        if (Ms[i] > 64) continue;
        c = good(Ms[i], sims[s], o); expect_launch("rollout launch without a device", ROLL(c));
        c = good(Ms[i], sims[s], o); c.l.noise = NULL; c.l.clamp = 0; c.l.weight_stride = 0; c.b.reset_rs = NULL; c.b.reset_profile = NULL;
        c.b.final_obs = NULL; c.b.reset_count = NULL; c.r.T = 1;
        expect_launch("rollout launch without a device (bare)", ROLL(c));
      }
  c = good(51, PDEGYM_TRAFFIC_INLET, TREE); c.l.weights_v = NULL; c.l.weights_q = NULL;
  expect_launch("inlet needs no weights (control)", pdegym_traffic_backstep_control(&c.p, &c.l, NULL, 0, FAKE(4), FAKE(21), 1, 6, NULL));
  expect_launch("inlet needs no weights (rollout)", ROLL(c));
  c = good(51, PDEGYM_TRAFFIC_BOTH, TREE); c.b.action_stride = 0; expect_launch("'both' with action_stride=0 (= 2)", ROLL(c));
  printf("calls %d bad %d\n", n_calls, n_bad);
  if (n_bad) return 1;
  printf("TRAFFIC-BACKSTEP-VALIDATION-OK\n");
  return 0;
}
