/* backstep_validation.c -- argument validation of the three backstepping entry points (include/pdegym.h) WITHOUT a GPU: null
 * pointers, sizes out of range, inconsistent descriptors.  Every bad call must come back with a negative code and a message in
 * pdegym_last_error(); tests/test_backstepping.py links it against the host half of the library built with AddressSanitizer and
 * UndefinedBehaviorSanitizer.  The last group hands over well-formed arguments with fake device addresses: the host code then runs
 * up to the launch, which fails cleanly on a machine without a device (the pointers are never dereferenced on the host). */
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

static void expect_ok(const char* what, int rc) {
  ++n_calls;
  if (rc != 0) {
    ++n_bad;
    printf("UNEXPECTED %s -> %d \"%s\"\n", what, rc, pdegym_last_error());
  }
}

#define FAKE(k) ((void*)(uintptr_t)(0x7f0000000000ull + 4096ull * (k)))

typedef int (*gain_fn)(const float*, double*, int32_t, int32_t, double, void*);

static pdegym_backstep good(void) {
  pdegym_backstep c;
  memset(&c, 0, sizeof c);
  c.gain0 = FAKE(1); c.gain_stride = 200; c.m = 200; c.obs = FAKE(2); c.obs_stride = 201; c.len = 200;
  c.order = PDEGYM_BACKSTEP_TREE; c.scale = 5e-3; c.out64 = FAKE(3);
  return c;
}

int main(void) {
  if (pdegym_abi_version() != PDEGYM_ABI_VERSION) { printf("ABI mismatch\n"); return 1; }
  const gain_fn gains[2] = {pdegym_backstep_gain_parabolic, pdegym_backstep_gain_transport};
  for (int k = 0; k < 2; ++k) {
    gain_fn f = gains[k];
    expect_error("gain(NULL theta)", f(NULL, FAKE(2), 4, 100, 1e-2, NULL));
    expect_error("gain(NULL gain)", f(FAKE(1), NULL, 4, 100, 1e-2, NULL));
    expect_error("gain R=-1", f(FAKE(1), FAKE(2), -1, 100, 1e-2, NULL));
    expect_error("gain m=1", f(FAKE(1), FAKE(2), 4, 1, 1e-2, NULL));
    expect_error("gain m=0", f(FAKE(1), FAKE(2), 4, 0, 1e-2, NULL));
    expect_error("gain m=-5", f(FAKE(1), FAKE(2), 4, -5, 1e-2, NULL));
    expect_error("gain m=2049", f(FAKE(1), FAKE(2), 4, PDEGYM_MAX_N1D + 1, 1e-2, NULL));
    expect_error("gain dx=0", f(FAKE(1), FAKE(2), 4, 100, 0.0, NULL));
    expect_error("gain dx<0", f(FAKE(1), FAKE(2), 4, 100, -1e-2, NULL));
    expect_error("gain dx=nan", f(FAKE(1), FAKE(2), 4, 100, NAN, NULL));
    expect_error("gain dx=inf", f(FAKE(1), FAKE(2), 4, 100, INFINITY, NULL));
    expect_ok("gain R=0", f(FAKE(1), FAKE(2), 0, 100, 1e-2, NULL));
  }

  pdegym_backstep c;
  expect_error("control(NULL)", pdegym_backstep_control(NULL, 4, NULL));
  c = good(); expect_ok("control B=0", pdegym_backstep_control(&c, 0, NULL));
  c = good(); c.gain0 = NULL; expect_error("control gain0=NULL", pdegym_backstep_control(&c, 4, NULL));
  c = good(); c.obs = NULL; expect_error("control obs=NULL", pdegym_backstep_control(&c, 4, NULL));
  c = good(); c.out64 = NULL; expect_error("control no output", pdegym_backstep_control(&c, 4, NULL));
  c = good(); c.out32 = FAKE(4); expect_error("control two outputs", pdegym_backstep_control(&c, 4, NULL));
  c = good(); c.m = 0; expect_error("control m=0", pdegym_backstep_control(&c, 4, NULL));
  c = good(); c.len = 0; expect_error("control len=0", pdegym_backstep_control(&c, 4, NULL));
  c = good(); c.len = 201; expect_error("control len>m", pdegym_backstep_control(&c, 4, NULL));
  c = good(); c.gain_stride = 199; expect_error("control gain_stride<m", pdegym_backstep_control(&c, 4, NULL));
  c = good(); c.gain_stride = -200; expect_error("control gain_stride<0", pdegym_backstep_control(&c, 4, NULL));
  c = good(); c.obs_stride = 199; expect_error("control obs_stride<len", pdegym_backstep_control(&c, 4, NULL));
  c = good(); c.order = 2; expect_error("control order=2", pdegym_backstep_control(&c, 4, NULL));
  c = good(); c.order = -1; expect_error("control order=-1", pdegym_backstep_control(&c, 4, NULL));
  c = good(); c.gain_pool = FAKE(5); expect_error("control pool without reset_count", pdegym_backstep_control(&c, 4, NULL));
  c = good(); c.gain_pool = FAKE(5); c.reset_count = FAKE(6); c.pool_rows = -1;
  expect_error("control pool_rows=-1", pdegym_backstep_control(&c, 4, NULL));
  c = good(); c.noise = FAKE(7); expect_error("control noise with out64", pdegym_backstep_control(&c, 4, NULL));
  c = good(); c.clamp = 1; c.lo = -1; c.hi = 1; expect_error("control clamp with out64", pdegym_backstep_control(&c, 4, NULL));
  c = good(); c.out64 = NULL; c.out32 = FAKE(4); c.clamp = 1; c.lo = 1; c.hi = -1;
  expect_error("control lo>hi", pdegym_backstep_control(&c, 4, NULL));
  c = good(); c.out64 = NULL; c.out32 = FAKE(4); c.clamp = 1; c.lo = NAN; c.hi = 1;
  expect_error("control lo=nan", pdegym_backstep_control(&c, 4, NULL));

  /* well-formed calls: the host side runs up to the launch; without a device that launch fails with a message */
  for (int k = 0; k < 2; ++k) {
    const int ms[] = {2, 64, 65, 200, 513, 2048};
    for (unsigned i = 0; i < sizeof ms / sizeof ms[0]; ++i) expect_error("gain launch without a device", gains[k](FAKE(1), FAKE(2), 70, ms[i], 5e-3, NULL));
  }
  c = good(); expect_error("control launch (tree)", pdegym_backstep_control(&c, 70, NULL));
  c = good(); c.order = PDEGYM_BACKSTEP_ORDERED; c.gain_stride = 0; c.gain_pool = FAKE(5); c.reset_count = FAKE(6); c.pool_rows = 7;
  c.out64 = NULL; c.out32 = FAKE(4); c.noise = FAKE(7); c.clamp = 1; c.lo = -20; c.hi = 20;
  expect_error("control launch (ordered, pool, f32)", pdegym_backstep_control(&c, 6, NULL));

  printf("calls %d bad %d\n", n_calls, n_bad);
  if (n_bad) return 1;
  printf("BACKSTEP-VALIDATION-OK\n");
  return 0;
}
