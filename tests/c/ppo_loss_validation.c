/* ppo_loss_validation.c -- argument validation of pdegym_ppo_loss, pdegym_ppo_loss_workspace and pdegym_diag_gaussian_log_prob
 * (include/pdegym.h) WITHOUT a GPU: sizes and strides out of range, non-finite or negative scalars, a workspace that is too small or
 * displaced, null pointers, values / d_values given in halves, outputs that overlap an input or each other.  Every bad call must come
 * back with its code and a message in pdegym_last_error(); tests/test_ppo_loss.py links it against the host half of
 * pdegym_ppo_loss.hip + pdegym_abi.hip built with AddressSanitizer and UndefinedBehaviorSanitizer.  The last group hands over
 * well-formed descriptors with fake device addresses: the host code then runs up to the launch, which fails cleanly on a machine
 * without a device (the pointers are never dereferenced on the host). */
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
    printf("%-52s %5d  %s\n", what, rc, msg);
  }
}

/* 16 MiB apart: no two arrays of the cases below overlap unless a case makes them */
#define FAKE(k) ((void*)(uintptr_t)(0x7f0000000000ull + 0x1000000ull * (k)))
#define N_ 1000
#define M_ 3000
#define A_ 3
#define LD_ 5

static pdegym_ppo_loss_args good(void) {
  pdegym_ppo_loss_args g;
  memset(&g, 0, sizeof g);
  g.A = A_; g.normalize_advantage = 1;
  g.mean = FAKE(1); g.ld_mean = LD_; g.values = FAKE(2); g.log_std = FAKE(3); g.index = FAKE(4); g.M = M_;
  g.actions = FAKE(5); g.ld_actions = LD_; g.old_log_prob = FAKE(6); g.advantages = FAKE(7); g.returns = FAKE(8);
  g.clip_range = 0.2; g.ent_coef = 1e-3; g.vf_coef = 0.5;
  g.d_mean = FAKE(9); g.ld_d_mean = LD_; g.d_values = FAKE(10); g.d_log_std = FAKE(11); g.stats = FAKE(12);
  g.workspace = FAKE(13); g.workspace_bytes = pdegym_ppo_loss_workspace(N_, A_);
  return g;
}

#define LOSS(what, want) expect_code(what, want, pdegym_ppo_loss(&g, N_, NULL))

int main(void) {
  if (pdegym_abi_version() != PDEGYM_ABI_VERSION) { printf("ABI mismatch\n"); return 1; }
  pdegym_ppo_loss_args g;
  const int64_t need = pdegym_ppo_loss_workspace(N_, A_);
  if (need < 8 || need % 8 != 0 || need != pdegym_ppo_loss_workspace(N_, 1) || pdegym_ppo_loss_workspace(1, 8) < 8
      || pdegym_ppo_loss_workspace(100000, 8) < need) {
    printf("UNEXPECTED workspace sizes: %lld\n", (long long)need);
    ++n_bad;
  }
  expect_code("workspace(0, 1)", -2, (int)pdegym_ppo_loss_workspace(0, 1));
  expect_code("workspace(-5, 1)", -2, (int)pdegym_ppo_loss_workspace(-5, 1));
  expect_code("workspace(10, 0)", -2, (int)pdegym_ppo_loss_workspace(10, 0));
  expect_code("workspace(10, 9)", -2, (int)pdegym_ppo_loss_workspace(10, 9));

  expect_code("ppo_loss(NULL)", -1, pdegym_ppo_loss(NULL, N_, NULL));
  g = good(); expect_code("N=0", -2, pdegym_ppo_loss(&g, 0, NULL));
  g = good(); expect_code("N=-1", -2, pdegym_ppo_loss(&g, -1, NULL));
  g = good(); g.A = 0; LOSS("A=0", -2);
  g = good(); g.A = 9; LOSS("A=9", -2);
  g = good(); g.A = -1; LOSS("A=-1", -2);
  g = good(); g.ld_mean = A_ - 1; LOSS("ld_mean<A", -2);
  g = good(); g.ld_actions = A_ - 1; LOSS("ld_actions<A", -2);
  g = good(); g.ld_d_mean = 0; LOSS("ld_d_mean=0", -2);
  g = good(); g.ld_mean = -LD_; LOSS("ld_mean<0", -2);
  g = good(); g.M = 0; LOSS("M=0 with an index", -2);
  g = good(); g.clip_range = NAN; LOSS("clip_range=nan", -2);
  g = good(); g.clip_range = INFINITY; LOSS("clip_range=inf", -2);
  g = good(); g.clip_range = -0.1; LOSS("clip_range<0", -2);
  g = good(); g.ent_coef = NAN; LOSS("ent_coef=nan", -2);
  g = good(); g.ent_coef = -INFINITY; LOSS("ent_coef=-inf", -2);
  g = good(); g.vf_coef = NAN; LOSS("vf_coef=nan", -2);
  g = good(); g.vf_coef = INFINITY; LOSS("vf_coef=inf", -2);
  g = good(); g.workspace_bytes -= 1; LOSS("workspace one byte short", -2);
  g = good(); g.workspace_bytes = 0; LOSS("workspace_bytes=0", -2);
  g = good(); g.workspace = (char*)g.workspace + 2; LOSS("workspace off a 4-byte boundary", -2);
  g = good(); g.workspace = (char*)g.workspace + 1; LOSS("workspace at an odd address", -2);
  /* required pointers */
  g = good(); g.mean = NULL; LOSS("mean=NULL", -3);
  g = good(); g.log_std = NULL; LOSS("log_std=NULL", -3);
  g = good(); g.actions = NULL; LOSS("actions=NULL", -3);
  g = good(); g.old_log_prob = NULL; LOSS("old_log_prob=NULL", -3);
  g = good(); g.advantages = NULL; LOSS("advantages=NULL", -3);
  g = good(); g.d_mean = NULL; LOSS("d_mean=NULL", -3);
  g = good(); g.d_log_std = NULL; LOSS("d_log_std=NULL", -3);
  g = good(); g.stats = NULL; LOSS("stats=NULL", -3);
  g = good(); g.workspace = NULL; LOSS("workspace=NULL", -3);
  g = good(); g.returns = NULL; LOSS("values without returns", -3);
  /* the value term comes whole */
  g = good(); g.values = NULL; LOSS("d_values without values", -3);
  g = good(); g.d_values = NULL; LOSS("values without d_values", -3);
  /* no output aliases an input, in whole or in part */
  g = good(); g.d_mean = (float*)g.mean; LOSS("d_mean = mean", -3);
  g = good(); g.d_values = (float*)g.values; LOSS("d_values = values", -3);
  g = good(); g.d_log_std = (float*)g.log_std; LOSS("d_log_std = log_std", -3);
  g = good(); g.d_log_std = (float*)g.log_std + (A_ - 1); LOSS("d_log_std on log_std's last element", -3);
  g = good(); g.stats = (float*)g.advantages + (M_ - 1); LOSS("stats on the last advantage (row M-1)", -3);
  g = good(); g.d_values = (float*)g.returns + (M_ - 1); LOSS("d_values on the last return (row M-1)", -3);
  g = good(); g.d_mean = (float*)g.actions + ((size_t)(M_ - 1) * LD_ + A_ - 1); LOSS("d_mean on the last action", -3);
  g = good(); g.stats = (float*)((int64_t*)g.index + (N_ - 1)); LOSS("stats on the last index entry", -3);
  g = good(); g.d_values = (float*)g.old_log_prob; LOSS("d_values = old_log_prob", -3);
  g = good(); g.workspace = (void*)g.mean; LOSS("workspace = mean", -3);
  g = good(); g.d_values = g.d_mean; LOSS("d_values = d_mean", -3);
  g = good(); g.stats = g.d_log_std + (A_ - 1); LOSS("stats on d_log_std's last element", -3);
  g = good(); g.d_log_std = g.stats + 7; LOSS("d_log_std on stats[7]", -3);
  g = good(); g.workspace = (char*)g.d_values + 4 * (N_ - 1); LOSS("workspace on the last d_values", -3);
  g = good(); g.d_mean = (float*)((char*)g.workspace + g.workspace_bytes - 4); LOSS("d_mean on the workspace's last word", -3);

  /* the log-probability entry point */
  expect_code("log_prob N=0", -2, pdegym_diag_gaussian_log_prob(FAKE(1), LD_, FAKE(2), FAKE(3), LD_, NULL, FAKE(4), 0, A_, NULL));
  expect_code("log_prob A=9", -2, pdegym_diag_gaussian_log_prob(FAKE(1), LD_, FAKE(2), FAKE(3), LD_, NULL, FAKE(4), N_, 9, NULL));
  expect_code("log_prob A=0", -2, pdegym_diag_gaussian_log_prob(FAKE(1), LD_, FAKE(2), FAKE(3), LD_, NULL, FAKE(4), N_, 0, NULL));
  expect_code("log_prob ld<A", -2, pdegym_diag_gaussian_log_prob(FAKE(1), A_ - 1, FAKE(2), FAKE(3), LD_, NULL, FAKE(4), N_, A_, NULL));
  expect_code("log_prob ld_a<A", -2, pdegym_diag_gaussian_log_prob(FAKE(1), LD_, FAKE(2), FAKE(3), 0, NULL, FAKE(4), N_, A_, NULL));
  expect_code("log_prob mean=NULL", -3, pdegym_diag_gaussian_log_prob(NULL, LD_, FAKE(2), FAKE(3), LD_, NULL, FAKE(4), N_, A_, NULL));
  expect_code("log_prob log_std=NULL", -3, pdegym_diag_gaussian_log_prob(FAKE(1), LD_, NULL, FAKE(3), LD_, NULL, FAKE(4), N_, A_, NULL));
  expect_code("log_prob actions=NULL", -3, pdegym_diag_gaussian_log_prob(FAKE(1), LD_, FAKE(2), NULL, LD_, NULL, FAKE(4), N_, A_, NULL));
  expect_code("log_prob out=NULL", -3, pdegym_diag_gaussian_log_prob(FAKE(1), LD_, FAKE(2), FAKE(3), LD_, NULL, NULL, N_, A_, NULL));
  expect_code("log_prob out = mean", -3, pdegym_diag_gaussian_log_prob(FAKE(1), LD_, FAKE(2), FAKE(3), LD_, NULL, FAKE(1), N_, A_, NULL));
  expect_code("log_prob out on the last action", -3,
              pdegym_diag_gaussian_log_prob(FAKE(1), LD_, FAKE(2), FAKE(3), LD_, NULL, (float*)FAKE(3) + ((size_t)(N_ - 1) * LD_ + A_ - 1), N_,
                                            A_, NULL));
  expect_code("log_prob out = index", -3, pdegym_diag_gaussian_log_prob(FAKE(1), LD_, FAKE(2), FAKE(3), LD_, FAKE(4), FAKE(4), N_, A_, NULL));

  /* well-formed descriptors: the host side runs up to the launch; without a device that launch fails with a message */
  g = good(); LOSS("launch (everything given)", -100);
  g = good(); g.normalize_advantage = 0; LOSS("launch (no normalisation)", -100);
  g = good(); g.values = NULL; g.d_values = NULL; g.returns = NULL; LOSS("launch (no value term)", -100);
  g = good(); g.index = NULL; g.M = 0; LOSS("launch (dense: M unused)", -100);
  g = good(); g.clip_range = 0.0; g.ent_coef = 0.0; g.vf_coef = -1.0; LOSS("launch (clip_range 0, negative vf_coef)", -100);
  g = good(); g.ld_mean = A_; g.ld_actions = A_; g.ld_d_mean = A_; LOSS("launch (dense rows)", -100);
  g = good(); g.d_values = (float*)g.values + N_; LOSS("launch (d_values right after values)", -100);      /* touching is not overlapping */
  g = good(); g.workspace_bytes += 4; g.workspace = (char*)g.workspace + 4; LOSS("launch (workspace 4 bytes on, larger)", -100);
  g = good(); g.A = 1; g.ld_mean = 1; g.ld_actions = 1; g.ld_d_mean = 1; g.index = NULL; g.workspace_bytes = pdegym_ppo_loss_workspace(1, 1);
  expect_code("launch (N=1, A=1)", -100, pdegym_ppo_loss(&g, 1, NULL));
  g = good(); g.A = 8; g.ld_mean = 8; g.ld_actions = 9; g.ld_d_mean = 10; LOSS("launch (A=8)", -100);
  expect_code("launch log_prob (dense)", -100, pdegym_diag_gaussian_log_prob(FAKE(1), LD_, FAKE(2), FAKE(3), LD_, NULL, FAKE(4), N_, A_, NULL));
  expect_code("launch log_prob (index)", -100, pdegym_diag_gaussian_log_prob(FAKE(1), A_, FAKE(2), FAKE(3), A_, FAKE(5), FAKE(4), N_, A_, NULL));

  printf("calls %d bad %d\n", n_calls, n_bad);
  if (n_bad) return 1;
  printf("PPO-LOSS-VALIDATION-OK\n");
  return 0;
}
