/* gae_validation.c -- argument validation of pdegym_gae (include/pdegym.h) WITHOUT a GPU: sizes out of range, non-finite discount
 * factors, null pointers, optional outputs given in halves, outputs that overlap an input or each other.  Every bad call must come back
 * with a negative code and a message in pdegym_last_error(); tests/test_gae.py links it against the host half of pdegym_gae.hip +
 * pdegym_abi.hip built with AddressSanitizer and UndefinedBehaviorSanitizer.  The last group hands over well-formed descriptors with
 * fake device addresses: the host code then runs up to the launch, which fails cleanly on a machine without a device (the pointers
 * are never dereferenced on the host). */
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

/* a validation error (-1 .. -3), not the failed launch (-100) of a descriptor that passed */
static void expect_refused(const char* what, int rc) {
  if (rc < -3) {
    ++n_calls;
    ++n_bad;
    printf("UNEXPECTED %s reached the launch (%d)\n", what, rc);
    return;
  }
  expect_error(what, rc);
}

static void expect_launch(const char* what, int rc) {
  if (rc != -100) {
    ++n_calls;
    ++n_bad;
    printf("UNEXPECTED %s -> %d \"%s\" (a well-formed descriptor fails only at the launch)\n", what, rc, pdegym_last_error());
    return;
  }
  expect_error(what, rc);
}

/* 16 MiB apart: no two arrays of the cases below overlap unless a case makes them */
#define FAKE(k) ((void*)(uintptr_t)(0x7f0000000000ull + 0x1000000ull * (k)))
#define T_ 33
#define B_ 130
#define LD_ 133

static pdegym_gae_args good(void) {
  pdegym_gae_args g;
  memset(&g, 0, sizeof g);
  g.T = T_; g.ld = LD_; g.gamma = 0.99; g.gae_lambda = 0.95;
  g.rewards = FAKE(1); g.values = FAKE(2); g.terminated = FAKE(3); g.truncated = FAKE(4); g.boot = FAKE(5);
  g.advantages = FAKE(6); g.returns = FAKE(7);
  g.ep_return_acc = FAKE(8); g.ep_length_acc = FAKE(9); g.episode_return = FAKE(10); g.episode_length = FAKE(11);
  return g;
}

int main(void) {
  if (pdegym_abi_version() != PDEGYM_ABI_VERSION) { printf("ABI mismatch\n"); return 1; }
  pdegym_gae_args g;
  expect_refused("gae(NULL)", pdegym_gae(NULL, B_, NULL));
  g = good(); g.T = 0; expect_refused("T=0", pdegym_gae(&g, B_, NULL));
  g = good(); g.T = -3; expect_refused("T=-3", pdegym_gae(&g, B_, NULL));
  g = good(); expect_refused("B=0", pdegym_gae(&g, 0, NULL));
  g = good(); expect_refused("B=-1", pdegym_gae(&g, -1, NULL));
  g = good(); g.ld = B_ - 1; expect_refused("ld<B", pdegym_gae(&g, B_, NULL));
  g = good(); g.ld = 0; expect_refused("ld=0", pdegym_gae(&g, B_, NULL));
  g = good(); g.ld = -LD_; expect_refused("ld<0", pdegym_gae(&g, B_, NULL));
  g = good(); g.gamma = NAN; expect_refused("gamma=nan", pdegym_gae(&g, B_, NULL));
  g = good(); g.gamma = INFINITY; expect_refused("gamma=inf", pdegym_gae(&g, B_, NULL));
  g = good(); g.gae_lambda = NAN; expect_refused("gae_lambda=nan", pdegym_gae(&g, B_, NULL));
  g = good(); g.gae_lambda = -INFINITY; expect_refused("gae_lambda=-inf", pdegym_gae(&g, B_, NULL));
  g = good(); g.rewards = NULL; expect_refused("rewards=NULL", pdegym_gae(&g, B_, NULL));
  g = good(); g.values = NULL; expect_refused("values=NULL", pdegym_gae(&g, B_, NULL));
  g = good(); g.terminated = NULL; expect_refused("terminated=NULL", pdegym_gae(&g, B_, NULL));
  g = good(); g.advantages = NULL; expect_refused("advantages=NULL", pdegym_gae(&g, B_, NULL));
  g = good(); g.returns = NULL; expect_refused("returns=NULL", pdegym_gae(&g, B_, NULL));
  /* the optional outputs come together */
  g = good(); g.episode_return = NULL; expect_refused("episode_length without episode_return", pdegym_gae(&g, B_, NULL));
  g = good(); g.episode_length = NULL; expect_refused("episode_return without episode_length", pdegym_gae(&g, B_, NULL));
  g = good(); g.ep_return_acc = NULL; expect_refused("ep_length_acc without ep_return_acc", pdegym_gae(&g, B_, NULL));
  g = good(); g.ep_length_acc = NULL; expect_refused("ep_return_acc without ep_length_acc", pdegym_gae(&g, B_, NULL));
  g = good(); g.episode_return = NULL; g.episode_length = NULL;
  expect_refused("accumulators without the outputs", pdegym_gae(&g, B_, NULL));
  /* no output aliases an input, in whole or in part */
  g = good(); g.advantages = (float*)g.rewards; expect_refused("advantages = rewards", pdegym_gae(&g, B_, NULL));
  g = good(); g.returns = (float*)g.values; expect_refused("returns = values", pdegym_gae(&g, B_, NULL));
  g = good(); g.advantages = (float*)g.boot; expect_refused("advantages = boot", pdegym_gae(&g, B_, NULL));
  g = good(); g.advantages = (float*)g.values + (size_t)T_ * LD_;      /* row T of values is the last one read */
  expect_refused("advantages inside values' last row", pdegym_gae(&g, B_, NULL));
  g = good(); g.returns = (float*)((char*)g.terminated + (size_t)(T_ - 1) * LD_ + B_ - 2);      /* (a multiple of 4) */
  expect_refused("returns on terminated's last two bytes", pdegym_gae(&g, B_, NULL));
  g = good(); g.episode_length = (int32_t*)g.truncated; expect_refused("episode_length = truncated", pdegym_gae(&g, B_, NULL));
  g = good(); g.rewards_f64 = 1; g.episode_return = (double*)g.rewards;
  expect_refused("episode_return = rewards (f64)", pdegym_gae(&g, B_, NULL));
  g = good(); g.ep_return_acc = (double*)g.rewards + 5; expect_refused("ep_return_acc inside rewards", pdegym_gae(&g, B_, NULL));
  g = good(); g.returns = g.advantages; expect_refused("returns = advantages", pdegym_gae(&g, B_, NULL));
  g = good(); g.returns = g.advantages + B_ - 1; expect_refused("returns one element into advantages' first row", pdegym_gae(&g, B_, NULL));
  g = good(); g.ep_length_acc = g.episode_length; expect_refused("ep_length_acc = episode_length", pdegym_gae(&g, B_, NULL));
  /* float64 rewards reach twice as far: an output just past the float32 extent is inside the float64 one */
  g = good(); g.rewards_f64 = 1; g.advantages = (float*)g.rewards + ((size_t)(T_ - 1) * LD_ + B_);
  expect_refused("advantages inside f64 rewards", pdegym_gae(&g, B_, NULL));

  /* well-formed descriptors: the host side runs up to the launch; without a device that launch fails with a message */
  g = good(); expect_launch("launch (everything given)", pdegym_gae(&g, B_, NULL));
  g = good(); g.advantages = (float*)g.rewards + ((size_t)(T_ - 1) * LD_ + B_);      /* touching is not overlapping */
  expect_launch("launch (advantages right after rewards)", pdegym_gae(&g, B_, NULL));
  g = good(); g.rewards_f64 = 1; g.truncated = NULL; g.boot = NULL; expect_launch("launch (f64, no truncated, no boot)", pdegym_gae(&g, B_, NULL));
  g = good(); g.ep_return_acc = NULL; g.ep_length_acc = NULL; expect_launch("launch (statistics without accumulators)", pdegym_gae(&g, B_, NULL));
  g = good(); g.ep_return_acc = NULL; g.ep_length_acc = NULL; g.episode_return = NULL; g.episode_length = NULL;
  expect_launch("launch (no statistics)", pdegym_gae(&g, B_, NULL));
  g = good(); g.T = 1; g.ld = 1; g.gamma = 0.0; g.gae_lambda = 1.0; expect_launch("launch (T=1, B=1, ld=1)", pdegym_gae(&g, 1, NULL));
  g = good(); g.boot = NULL; g.ld = B_; g.gamma = 1.0; g.gae_lambda = 1.0; expect_launch("launch (ld=B, no boot)", pdegym_gae(&g, B_, NULL));
  g = good(); g.truncated = NULL; expect_launch("launch (boot without truncated)", pdegym_gae(&g, B_, NULL));

  printf("calls %d bad %d\n", n_calls, n_bad);
  if (n_bad) return 1;
  printf("GAE-VALIDATION-OK\n");
  return 0;
}
