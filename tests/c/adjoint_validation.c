/* adjoint_validation.c -- argument validation of pdegym_ns2d_adjoint_f64 (include/pdegym.h) WITHOUT a GPU: null pointers, sizes
 * out of range, grids without a kernel, a boundary table other than the script's.  Every bad call must come back with a negative
 * code and a message in pdegym_last_error(); tests/test_adjoint.py links it against the host half of the library built with
 * AddressSanitizer and UndefinedBehaviorSanitizer.  The last group hands over well-formed arguments with fake device addresses: the
 * host code then runs up to the launch, which fails cleanly on a machine without a device (the pointers are never dereferenced on
 * the host). */
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

/* an alignment the header states at the parameter: code -2 (never the failed launch, -100) and the argument's name in the message */
static void expect_misaligned(const char* what, int rc, const char* argument) {
  const char* msg = pdegym_last_error();
  if (rc != -2 || msg == NULL || strstr(msg, argument) == NULL || strstr(msg, "aligned") == NULL) {
    ++n_calls;
    ++n_bad;
    printf("UNEXPECTED %s -> %d \"%s\" (expected -2 naming %s)\n", what, rc, msg ? msg : "(null)", argument);
    return;
  }
  expect_error(what, rc);
}

/* a well-formed call fails only at the launch, for want of a device */
static void expect_launch(const char* what, int rc) {
  if (rc != -100) {
    ++n_calls;
    ++n_bad;
    printf("UNEXPECTED %s -> %d \"%s\" (a well-formed call fails only at the launch)\n", what, rc, pdegym_last_error());
    return;
  }
  expect_error(what, rc);
}

#define FAKE(k) ((void*)(uintptr_t)(0x7f0000000000ull + 4096ull * (k)))

static pdegym_params_ns2d good_prm(int ny, int nx) {
  pdegym_params_ns2d p;
  memset(&p, 0, sizeof p);
  p.nx = nx; p.ny = ny; p.nt = 200; p.iters = 3; p.action_dim = 1;
  for (int e = 0; e < 4; ++e)
    for (int k = 0; k < 2; ++k) p.bc[e][k] = PDEGYM_BC_DIRICHLET;
  p.bc[PDEGYM_EDGE_UPPER][0] = PDEGYM_BC_CONTROLLABLE;
  p.dt = 1e-3; p.dx = 1.0 / (nx - 1); p.dy = 1.0 / (ny - 1); p.viscosity = 0.1; p.density = 1.0; p.gamma = 0.1;
  return p;
}

static pdegym_adjoint_ns2d good_adj(void) {
  pdegym_adjoint_ns2d a;
  memset(&a, 0, sizeof a);
  a.T = 6; a.t0 = 0; a.obs = FAKE(1); a.a_nom = FAKE(2); a.ratio = 1.0; a.width = 5.0; a.grad = FAKE(3); a.actions = FAKE(4);
  return a;
}

int main(void) {
  if (pdegym_abi_version() != PDEGYM_ABI_VERSION) { printf("ABI mismatch\n"); return 1; }
  pdegym_params_ns2d p = good_prm(21, 21);
  pdegym_adjoint_ns2d a = good_adj();
  const void* uref = FAKE(9);

  expect_error("adjoint(NULL params)", pdegym_ns2d_adjoint_f64(NULL, uref, 7, &a, 4, NULL));
  expect_error("adjoint(NULL descriptor)", pdegym_ns2d_adjoint_f64(&p, uref, 7, NULL, 4, NULL));
  expect_error("adjoint(NULL U_ref)", pdegym_ns2d_adjoint_f64(&p, NULL, 7, &a, 4, NULL));
  a = good_adj(); a.obs = NULL; expect_error("adjoint obs=NULL", pdegym_ns2d_adjoint_f64(&p, uref, 7, &a, 4, NULL));
  a = good_adj(); a.a_nom = NULL; expect_error("adjoint a_nom=NULL", pdegym_ns2d_adjoint_f64(&p, uref, 7, &a, 4, NULL));
  a = good_adj(); a.grad = NULL; expect_error("adjoint grad=NULL", pdegym_ns2d_adjoint_f64(&p, uref, 7, &a, 4, NULL));
  a = good_adj(); a.actions = NULL; expect_error("adjoint actions=NULL", pdegym_ns2d_adjoint_f64(&p, uref, 7, &a, 4, NULL));
  a = good_adj(); a.T = 0; expect_error("adjoint T=0", pdegym_ns2d_adjoint_f64(&p, uref, 7, &a, 4, NULL));
  a = good_adj(); a.T = -3; expect_error("adjoint T=-3", pdegym_ns2d_adjoint_f64(&p, uref, 7, &a, 4, NULL));
  a = good_adj(); a.t0 = -1; expect_error("adjoint t0=-1", pdegym_ns2d_adjoint_f64(&p, uref, 7, &a, 4, NULL));
  a = good_adj(); expect_error("adjoint nt_ref=0", pdegym_ns2d_adjoint_f64(&p, uref, 0, &a, 4, NULL));
  /* grids without a column kernel */
  const int bad_grid[][2] = {{20, 21}, {33, 21}, {7, 8}, {21, 65}, {21, 2}, {64, 64}, {256, 256}};
  for (unsigned i = 0; i < sizeof bad_grid / sizeof bad_grid[0]; ++i) {
    p = good_prm(bad_grid[i][0], bad_grid[i][1]);
    expect_error("adjoint unsupported grid", pdegym_ns2d_adjoint_f64(&p, uref, 7, &a, 4, NULL));
  }
  p = good_prm(21, 21); p.iters = -1; expect_error("adjoint iters=-1", pdegym_ns2d_adjoint_f64(&p, uref, 7, &a, 4, NULL));
  p = good_prm(21, 21); p.action_dim = 21; expect_error("adjoint action_dim=21", pdegym_ns2d_adjoint_f64(&p, uref, 7, &a, 4, NULL));
  p = good_prm(21, 21); p.action_dim = 0; expect_error("adjoint action_dim=0", pdegym_ns2d_adjoint_f64(&p, uref, 7, &a, 4, NULL));
  /* any boundary table other than the script's: every entry flipped to each other code in turn */
  for (int e = 0; e < 4; ++e)
    for (int k = 0; k < 2; ++k)
      for (int code = 0; code < 3; ++code) {
        p = good_prm(21, 21);
        if (p.bc[e][k] == code) continue;
        p.bc[e][k] = code;
        expect_error("adjoint other boundary table", pdegym_ns2d_adjoint_f64(&p, uref, 7, &a, 4, NULL));
      }
  p = good_prm(21, 21); p.bc[0][0] = 3; expect_error("adjoint bad bc code", pdegym_ns2d_adjoint_f64(&p, uref, 7, &a, 4, NULL));

  /* U_ref, obs and lam are moved as (u, v) pairs of 16 bytes: a pointer that is only double-aligned is refused with -2 and its
   * name, before any launch (a call that reaches the launch answers -100 here); the [T] / [T, B] arrays need 8 bytes only */
  p = good_prm(21, 21);
  a = good_adj(); expect_misaligned("adjoint U_ref + 8", pdegym_ns2d_adjoint_f64(&p, (const char*)uref + 8, 7, &a, 4, NULL), "U_ref");
  a = good_adj(); a.obs += 1; expect_misaligned("adjoint obs + 8", pdegym_ns2d_adjoint_f64(&p, uref, 7, &a, 4, NULL), "obs");
  a = good_adj(); a.lam = (double*)FAKE(5) + 1; expect_misaligned("adjoint lam + 8", pdegym_ns2d_adjoint_f64(&p, uref, 7, &a, 4, NULL), "lam");
  a = good_adj(); a.a_nom += 1; a.grad += 1; a.actions += 1;
  expect_launch("adjoint a_nom, grad, actions + 8", pdegym_ns2d_adjoint_f64(&p, uref, 7, &a, 4, NULL));

  p = good_prm(21, 21); a = good_adj();
  expect_ok("adjoint B=0", pdegym_ns2d_adjoint_f64(&p, uref, 7, &a, 0, NULL));

  /* well-formed calls: the host side runs up to the launch; without a device that launch fails with a message */
  const int grids[][2] = {{8, 8}, {11, 11}, {16, 16}, {21, 21}, {26, 26}, {31, 31}, {32, 32}, {8, 64}, {32, 3}};
  for (unsigned i = 0; i < sizeof grids / sizeof grids[0]; ++i) {
    p = good_prm(grids[i][0], grids[i][1]);
    a = good_adj(); a.lam = (i & 1) ? FAKE(5) : NULL; a.T = 1 + (int)i;
    expect_error("adjoint launch without a device", pdegym_ns2d_adjoint_f64(&p, uref, 7, &a, 70, NULL));
  }

  printf("calls %d bad %d\n", n_calls, n_bad);
  if (n_bad) return 1;
  printf("ADJOINT-VALIDATION-OK\n");
  return 0;
}
