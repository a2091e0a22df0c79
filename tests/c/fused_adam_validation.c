/* fused_adam_validation.c -- argument validation of pdegym_fused_adam and pdegym_fused_adam_workspace (include/pdegym.h) WITHOUT a
 * GPU: the number of tensors, sizes, non-finite or out-of-range hyper-parameters, mirror geometry, targets without tau, target
 * mirrors without a target, a workspace that is too small or displaced, null and misaligned pointers, outputs that overlap another
 * tensor of the call.  Every bad call must come back with its code and a message in pdegym_last_error();
 * tests/test_fused_adam.py links it against the host half of pdegym_fused_adam.hip + pdegym_abi.hip built with AddressSanitizer and
 * UndefinedBehaviorSanitizer.  The last group hands over well-formed descriptors with fake device addresses: the host code then runs
 * up to the launch, which fails cleanly on a machine without a device (the pointers are never dereferenced on the host). */
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "pdegym.h"

static int n_calls = 0, n_bad = 0;

static void expect_code(const char* what, int want, int rc) {
  const char* msg = pdegym_last_error();
  ++n_calls;
  if (rc != want || msg == NULL || msg[0] == '\0') {
    ++n_bad;
    printf("UNEXPECTED %s -> %d (wanted %d) \"%s\"\n", what, rc, want, msg ? msg : "(null)");
  } else {
    printf("%-58s %5d  %s\n", what, rc, msg);
  }
}

/* 16 MiB apart: no two arrays of the cases below overlap unless a case makes them */
#define FAKE(k) ((void*)(uintptr_t)(0x7f0000000000ull + 0x1000000ull * (k)))
#define OUT_ 7
#define IN_ 5
#define A_ 2

/* tensor 0: a weight (OUT_, IN_) with a blocked mirror, a target and the target's blocked mirror; tensor 1: a bias with a plain
 * mirror, a target and its plain mirror; tensors 2, 3: the (A_, IN_) heads mu and log_std sharing ONE blocked array on rows 0.. and
 * A_.., each with a plain mirror */
static pdegym_fused_adam_args good(void) {
  static int64_t sizes[4] = {OUT_ * IN_, OUT_, A_ * IN_, A_ * IN_};
  pdegym_fused_adam_args a;
  memset(&a, 0, sizeof a);
  a.K = 4; a.lr = 3e-4; a.beta1 = 0.9; a.beta2 = 0.999; a.eps = 1e-8; a.max_grad_norm = 0.5; a.tau = 0.005; a.polyak = 1;
  a.state = FAKE(1); a.total_norm = FAKE(2); a.workspace = FAKE(3); a.workspace_bytes = pdegym_fused_adam_workspace(sizes, 4);
  for (int i = 0; i < 4; ++i) {
    pdegym_fused_adam_tensor* t = &a.tensor[i];
    t->p = FAKE(10 + 10 * i); t->g = FAKE(11 + 10 * i); t->m = FAKE(12 + 10 * i); t->v = FAKE(13 + 10 * i); t->n = sizes[i];
  }
  a.tensor[0].out = OUT_; a.tensor[0].in = IN_; a.tensor[0].wt = FAKE(14); a.tensor[0].wt_out_total = OUT_;
  a.tensor[0].pt = FAKE(15); a.tensor[0].pt_wt = FAKE(16); a.tensor[0].pt_wt_out_total = OUT_;
  a.tensor[1].out = 1; a.tensor[1].in = OUT_; a.tensor[1].copy = FAKE(24); a.tensor[1].pt = FAKE(25); a.tensor[1].pt_copy = FAKE(26);
  for (int i = 2; i < 4; ++i) {
    a.tensor[i].out = A_; a.tensor[i].in = IN_; a.tensor[i].wt = FAKE(60); a.tensor[i].wt_out_total = 2 * A_;
    a.tensor[i].wt_row0 = (i - 2) * A_; a.tensor[i].copy = (float*)FAKE(61) + (i - 2) * A_ * IN_;
  }
  return a;
}

#define CALL(what, want) expect_code(what, want, pdegym_fused_adam(&a, NULL))

int main(void) {
  if (pdegym_abi_version() != PDEGYM_ABI_VERSION) { printf("ABI mismatch\n"); return 1; }
  pdegym_fused_adam_args a;
  int64_t n[PDEGYM_FUSED_ADAM_MAX_TENSORS + 1];
  for (int i = 0; i <= PDEGYM_FUSED_ADAM_MAX_TENSORS; ++i) n[i] = 1;
  /* 1024 elements per workgroup, 256 workgroups per tensor at most, one double each */
  if (pdegym_fused_adam_workspace(n, 1) != 8 || pdegym_fused_adam_workspace(n, 32) != 256) { printf("UNEXPECTED workspace of ones\n"); ++n_bad; }
  n[0] = 1024; n[1] = 1025; n[2] = 256 * 256; n[3] = 1000000000;
  if (pdegym_fused_adam_workspace(n, 4) != 8 * (1 + 2 + 64 + 256)) { printf("UNEXPECTED workspace of four\n"); ++n_bad; }
  expect_code("workspace(NULL)", -3, (int)pdegym_fused_adam_workspace(NULL, 1));
  expect_code("workspace(K=0)", -2, (int)pdegym_fused_adam_workspace(n, 0));
  expect_code("workspace(K=33)", -2, (int)pdegym_fused_adam_workspace(n, 33));
  n[1] = 0;
  expect_code("workspace(n=0)", -2, (int)pdegym_fused_adam_workspace(n, 4));

  expect_code("null descriptor", -1, pdegym_fused_adam(NULL, NULL));
  a = good(); a.K = 0; CALL("K = 0", -2);
  a = good(); a.K = 33; CALL("K = 33", -2);
  a = good(); a.K = -1; CALL("K = -1", -2);
  a = good(); a.tensor[1].n = 0; CALL("n = 0", -2);
  a = good(); a.lr = NAN; CALL("lr NaN", -2);
  a = good(); a.lr = INFINITY; CALL("lr Inf", -2);
  a = good(); a.beta1 = 1.0; CALL("beta1 = 1", -2);
  a = good(); a.beta1 = -0.1; CALL("beta1 < 0", -2);
  a = good(); a.beta2 = NAN; CALL("beta2 NaN", -2);
  a = good(); a.beta2 = 1.5; CALL("beta2 > 1", -2);
  a = good(); a.eps = 0.0; CALL("eps = 0", -2);
  a = good(); a.eps = -1e-8; CALL("eps < 0", -2);
  a = good(); a.eps = NAN; CALL("eps NaN", -2);
  a = good(); a.max_grad_norm = INFINITY; CALL("max_grad_norm Inf", -2);
  a = good(); a.tau = 1.5; CALL("tau > 1 with targets", -2);
  a = good(); a.tau = -0.1; CALL("tau < 0 with targets", -2);
  a = good(); a.tau = NAN; CALL("tau NaN with targets", -2);
  a = good(); a.tensor[0].in = IN_ + 1; CALL("mirror: out * in != n", -2);
  a = good(); a.tensor[0].out = 0; CALL("mirror: out = 0", -2);
  a = good(); a.tensor[3].wt_row0 = A_ + 1; CALL("mirror: row0 + out > out_total", -2);
  a = good(); a.tensor[3].wt_row0 = -1; CALL("mirror: row0 < 0", -2);
  a = good(); a.tensor[0].pt_wt_out_total = OUT_ - 1; CALL("target mirror: out > out_total", -2);
  a = good(); a.workspace_bytes -= 1; CALL("workspace one byte short", -2);
  a = good(); a.workspace = (char*)a.workspace + 2; CALL("workspace 2 bytes on", -2);
  a = good(); a.state = (double*)((char*)a.state + 4); CALL("state 4 bytes on", -2);
  a = good(); a.total_norm = (float*)((char*)a.total_norm + 2); CALL("total_norm 2 bytes on", -2);
  a = good(); a.lr_device = (const float*)((char*)FAKE(4) + 1); CALL("lr_device 1 byte on", -2);
  a = good(); a.tensor[2].g = (const float*)((char*)a.tensor[2].g + 2); CALL("g 2 bytes on", -2);
  a = good(); a.tensor[0].wt = (float*)((char*)a.tensor[0].wt + 1); CALL("wt 1 byte on", -2);
  a = good(); a.tensor[1].pt_copy = (float*)((char*)a.tensor[1].pt_copy + 3); CALL("pt_copy 3 bytes on", -2);

  a = good(); a.state = NULL; CALL("null state", -3);
  a = good(); a.workspace = NULL; CALL("null workspace", -3);
  a = good(); a.tensor[0].p = NULL; CALL("null p", -3);
  a = good(); a.tensor[1].g = NULL; CALL("null g", -3);
  a = good(); a.tensor[2].m = NULL; CALL("null m", -3);
  a = good(); a.tensor[3].v = NULL; CALL("null v", -3);
  a = good(); a.tensor[1].pt = NULL; CALL("pt_copy without pt", -3);
  a = good(); a.tensor[0].pt = NULL; CALL("pt_wt without pt", -3);

  a = good(); a.tensor[1].p = a.tensor[0].p + (OUT_ * IN_ - 1); CALL("p[1] on the last element of p[0]", -3);
  a = good(); a.tensor[0].g = a.tensor[0].p; CALL("g = p", -3);
  a = good(); a.tensor[0].m = a.tensor[0].v; CALL("m = v", -3);
  a = good(); a.tensor[2].g = a.tensor[3].m; CALL("g[2] = m[3]", -3);
  a = good(); a.tensor[1].copy = a.tensor[1].p; CALL("copy = p", -3);
  a = good(); a.tensor[1].pt = a.tensor[1].p; CALL("pt = p", -3);
  a = good(); a.tensor[0].pt_wt = a.tensor[0].wt; CALL("pt_wt = wt (same rows)", -3);
  a = good(); a.tensor[3].wt_row0 = A_ - 1; a.tensor[3].wt_out_total = 2 * A_; CALL("two heads on overlapping rows", -3);
  a = good(); a.tensor[3].wt_out_total = 2 * A_ + 1; CALL("two heads, one array, two out_totals", -3);
  a = good(); a.tensor[3].copy = a.tensor[2].copy + 1; CALL("copy[3] inside copy[2]", -3);
  a = good(); a.total_norm = a.tensor[0].p + 3; CALL("total_norm inside p", -3);
  a = good(); a.state = (double*)a.tensor[0].m; CALL("state = m", -3);
  a = good(); a.workspace = a.tensor[1].v; CALL("workspace = v", -3);
  a = good(); a.lr_device = a.tensor[0].p; CALL("lr_device inside p", -3);
  a = good(); a.tensor[1].g = a.tensor[0].wt + 8; CALL("g inside a blocked mirror", -3);

  /* well-formed descriptors: the host side runs up to the launch; without a device that launch fails with a message */
  a = good(); CALL("launch (everything given)", -100);
  a = good(); a.polyak = 0; CALL("launch (no polyak)", -100);
  a = good(); a.max_grad_norm = 0.0; a.total_norm = NULL; CALL("launch (no clipping, no norm)", -100);
  a = good(); a.max_grad_norm = NAN; CALL("launch (max_grad_norm NaN: no clipping)", -100);
  a = good(); a.lr = NAN; a.lr_device = FAKE(4); CALL("launch (device lr, host lr unused)", -100);
  a = good(); a.tensor[2].g = a.tensor[3].g; CALL("launch (one gradient read twice)", -100);
  a = good(); a.K = 1; CALL("launch (K = 1)", -100);
  a = good(); a.K = 2; a.tensor[0].pt = NULL; a.tensor[0].pt_wt = NULL; a.tensor[1].pt = NULL; a.tensor[1].pt_copy = NULL; a.tau = NAN;
  CALL("launch (no targets: tau unused)", -100);
  a = good(); a.workspace_bytes += 4; a.workspace = (char*)a.workspace + 4; CALL("launch (workspace 4 bytes on, larger)", -100);
  a = good(); a.K = 32;
  for (int i = 4; i < 32; ++i) { a.tensor[i] = a.tensor[1]; a.tensor[i].p = FAKE(100 + 4 * i); a.tensor[i].m = FAKE(101 + 4 * i);
    a.tensor[i].v = FAKE(102 + 4 * i); a.tensor[i].g = FAKE(103 + 4 * i); a.tensor[i].copy = NULL; a.tensor[i].pt = NULL; a.tensor[i].pt_copy = NULL; }
  a.workspace_bytes = 8 * 32; CALL("launch (K = 32)", -100);

  printf("calls %d bad %d\n", n_calls, n_bad);
  if (n_bad) return 1;
  printf("FUSED-ADAM-VALIDATION-OK\n");
  return 0;
}
