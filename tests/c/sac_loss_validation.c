/* sac_loss_validation.c -- argument validation of pdegym_squashed_gaussian_sample, pdegym_squashed_gaussian_sample_backward,
 * pdegym_sac_critic_loss, pdegym_sac_actor_loss and pdegym_sac_loss_workspace (include/pdegym.h) WITHOUT a GPU: sizes and strides
 * out of range, bounds in the wrong order, non-finite scalars, a workspace that is too small or displaced, null pointers, the second
 * critic given in part, outputs that overlap an input or each other.  Every bad call must come back with its code and a message in
 * pdegym_last_error(); tests/test_sac_loss.py links it against the host half of pdegym_sac_loss.hip + pdegym_abi.hip built with
 * AddressSanitizer and UndefinedBehaviorSanitizer.  The last group hands over well-formed descriptors with fake device addresses:
 * the host code then runs up to the launch, which fails cleanly on a machine without a device (the pointers are never dereferenced
 * on the host). */
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
#define N_ 1000
#define M_ 3000
#define A_ 3
#define D_ 5
#define LD_ 9      /* >= 2 A and >= D + A */

static pdegym_squashed_gaussian_sample_args good_sample(void) {
  pdegym_squashed_gaussian_sample_args s;
  memset(&s, 0, sizeof s);
  s.A = A_; s.D = D_; s.raw = FAKE(1); s.ld_raw = LD_; s.eps = FAKE(2); s.ld_eps = LD_; s.log_std_min = -20.f; s.log_std_max = 2.f;
  s.obs = FAKE(3); s.ld_obs = LD_; s.actions = FAKE(4); s.ld_actions = LD_; s.log_prob = FAKE(5);
  return s;
}

static pdegym_squashed_gaussian_sample_backward_args good_backward(void) {
  pdegym_squashed_gaussian_sample_backward_args s;
  memset(&s, 0, sizeof s);
  s.A = A_; s.raw = FAKE(1); s.ld_raw = LD_; s.eps = FAKE(2); s.ld_eps = LD_; s.log_std_min = -20.f; s.log_std_max = 2.f;
  s.d_actions = FAKE(3); s.ld_d_actions = LD_; s.d_log_prob = FAKE(4); s.d_log_prob_stride = 1; s.d_raw = FAKE(5); s.ld_d_raw = LD_;
  return s;
}

static pdegym_sac_critic_loss_args good_critic(void) {
  pdegym_sac_critic_loss_args g;
  memset(&g, 0, sizeof g);
  g.q1 = FAKE(1); g.q2 = FAKE(2); g.q1_target = FAKE(3); g.q2_target = FAKE(4); g.next_log_prob = FAKE(5); g.index = FAKE(6); g.M = M_;
  g.rewards = FAKE(7); g.dones = FAKE(8); g.log_alpha = FAKE(9); g.gamma = 0.99;
  g.d_q1 = FAKE(10); g.d_q2 = FAKE(11); g.target = FAKE(12); g.stats = FAKE(13);
  g.workspace = FAKE(14); g.workspace_bytes = pdegym_sac_loss_workspace(N_);
  return g;
}

static pdegym_sac_actor_loss_args good_actor(void) {
  pdegym_sac_actor_loss_args g;
  memset(&g, 0, sizeof g);
  g.q1_pi = FAKE(1); g.q2_pi = FAKE(2); g.log_prob = FAKE(3); g.log_alpha = FAKE(4); g.target_entropy = -1.0;
  g.d_q1_pi = FAKE(5); g.d_q2_pi = FAKE(6); g.d_log_prob = FAKE(7); g.d_log_alpha = FAKE(8); g.stats = FAKE(9);
  g.workspace = FAKE(10); g.workspace_bytes = pdegym_sac_loss_workspace(N_);
  return g;
}

#define SAMPLE(what, want) expect_code("sample: " what, want, pdegym_squashed_gaussian_sample(&s, N_, NULL))
#define BACK(what, want) expect_code("backward: " what, want, pdegym_squashed_gaussian_sample_backward(&b, N_, NULL))
#define CRITIC(what, want) expect_code("critic: " what, want, pdegym_sac_critic_loss(&c, N_, NULL))
#define ACTOR(what, want) expect_code("actor: " what, want, pdegym_sac_actor_loss(&a, N_, NULL))

int main(void) {
  if (pdegym_abi_version() != PDEGYM_ABI_VERSION) { printf("ABI mismatch\n"); return 1; }
  pdegym_squashed_gaussian_sample_args s;
  pdegym_squashed_gaussian_sample_backward_args b;
  pdegym_sac_critic_loss_args c;
  pdegym_sac_actor_loss_args a;
  const int64_t need = pdegym_sac_loss_workspace(N_);
  if (need < 8 || need % 8 != 0 || pdegym_sac_loss_workspace(1) < 8 || pdegym_sac_loss_workspace(100000) < need
      || pdegym_sac_loss_workspace(2000000000) != pdegym_sac_loss_workspace(100000)) {
    printf("UNEXPECTED workspace sizes: %lld\n", (long long)need);
    ++n_bad;
  }
  expect_code("workspace(0)", -2, (int)pdegym_sac_loss_workspace(0));
  expect_code("workspace(-5)", -2, (int)pdegym_sac_loss_workspace(-5));

  /* ---- sample ---- */
  expect_code("sample(NULL)", -1, pdegym_squashed_gaussian_sample(NULL, N_, NULL));
  s = good_sample(); expect_code("sample: N=0", -2, pdegym_squashed_gaussian_sample(&s, 0, NULL));
  s = good_sample(); expect_code("sample: N=-1", -2, pdegym_squashed_gaussian_sample(&s, -1, NULL));
  s = good_sample(); s.A = 0; SAMPLE("A=0", -2);
  s = good_sample(); s.A = 9; s.ld_raw = 18; s.ld_actions = 18; SAMPLE("A=9", -2);
  s = good_sample(); s.A = -1; SAMPLE("A=-1", -2);
  s = good_sample(); s.ld_raw = 2 * A_ - 1; SAMPLE("ld_raw<2A", -2);
  s = good_sample(); s.ld_raw = -LD_; SAMPLE("ld_raw<0", -2);
  s = good_sample(); s.ld_eps = A_ - 1; SAMPLE("ld_eps<A", -2);
  s = good_sample(); s.ld_obs = D_ - 1; SAMPLE("ld_obs<D", -2);
  s = good_sample(); s.ld_actions = D_ + A_ - 1; SAMPLE("ld_actions<D+A", -2);
  s = good_sample(); s.D = -1; SAMPLE("D<0", -2);
  s = good_sample(); s.D = 0; SAMPLE("obs with D=0", -2);
  s = good_sample(); s.obs = NULL; SAMPLE("D without obs", -2);
  s = good_sample(); s.log_std_min = 2.f; SAMPLE("log_std_min == log_std_max", -2);
  s = good_sample(); s.log_std_min = 3.f; SAMPLE("log_std_min > log_std_max", -2);
  s = good_sample(); s.log_std_max = NAN; SAMPLE("log_std_max=nan", -2);
  s = good_sample(); s.raw = NULL; SAMPLE("raw=NULL", -3);
  s = good_sample(); s.eps = NULL; SAMPLE("eps=NULL", -3);
  s = good_sample(); s.actions = NULL; SAMPLE("actions=NULL", -3);
  s = good_sample(); s.log_prob = NULL; SAMPLE("log_prob=NULL", -3);
  s = good_sample(); s.actions = (float*)s.raw; SAMPLE("actions = raw", -3);
  s = good_sample(); s.actions = (float*)s.obs; SAMPLE("actions = obs", -3);
  s = good_sample(); s.log_prob = (float*)s.eps + ((size_t)(N_ - 1) * LD_ + A_ - 1); SAMPLE("log_prob on the last eps", -3);
  s = good_sample(); s.log_prob = s.actions + ((size_t)(N_ - 1) * LD_ + D_ + A_ - 1); SAMPLE("log_prob on the last action", -3);
  s = good_sample(); s.actions = (float*)s.raw + ((size_t)(N_ - 1) * LD_ + 2 * A_ - 1); SAMPLE("actions on the last raw", -3);

  /* ---- sample backward ---- */
  expect_code("backward(NULL)", -1, pdegym_squashed_gaussian_sample_backward(NULL, N_, NULL));
  b = good_backward(); expect_code("backward: N=0", -2, pdegym_squashed_gaussian_sample_backward(&b, 0, NULL));
  b = good_backward(); b.A = 0; BACK("A=0", -2);
  b = good_backward(); b.A = 9; b.ld_raw = 18; b.ld_d_raw = 18; BACK("A=9", -2);
  b = good_backward(); b.ld_raw = 2 * A_ - 1; BACK("ld_raw<2A", -2);
  b = good_backward(); b.ld_eps = 0; BACK("ld_eps=0", -2);
  b = good_backward(); b.ld_d_actions = A_ - 1; BACK("ld_d_actions<A", -2);
  b = good_backward(); b.ld_d_raw = 2 * A_ - 1; BACK("ld_d_raw<2A", -2);
  b = good_backward(); b.d_log_prob_stride = 2; BACK("d_log_prob_stride=2", -2);
  b = good_backward(); b.d_log_prob_stride = -1; BACK("d_log_prob_stride=-1", -2);
  b = good_backward(); b.log_std_min = 2.f; b.log_std_max = -20.f; BACK("bounds swapped", -2);
  b = good_backward(); b.raw = NULL; BACK("raw=NULL", -3);
  b = good_backward(); b.eps = NULL; BACK("eps=NULL", -3);
  b = good_backward(); b.d_raw = NULL; BACK("d_raw=NULL", -3);
  b = good_backward(); b.d_actions = NULL; b.d_log_prob = NULL; BACK("d_actions and d_log_prob both NULL", -3);
  b = good_backward(); b.d_raw = (float*)b.raw; BACK("d_raw = raw", -3);
  b = good_backward(); b.d_raw = (float*)b.d_actions + ((size_t)(N_ - 1) * LD_ + A_ - 1); BACK("d_raw on the last d_action", -3);
  b = good_backward(); b.d_raw = (float*)b.d_log_prob + (N_ - 1); BACK("d_raw on the last d_log_prob", -3);
  b = good_backward(); b.d_raw = (float*)b.eps; BACK("d_raw = eps", -3);

  /* ---- critic ---- */
  expect_code("critic(NULL)", -1, pdegym_sac_critic_loss(NULL, N_, NULL));
  c = good_critic(); expect_code("critic: N=0", -2, pdegym_sac_critic_loss(&c, 0, NULL));
  c = good_critic(); expect_code("critic: N=-1", -2, pdegym_sac_critic_loss(&c, -1, NULL));
  c = good_critic(); c.M = 0; CRITIC("M=0 with an index", -2);
  c = good_critic(); c.gamma = NAN; CRITIC("gamma=nan", -2);
  c = good_critic(); c.gamma = INFINITY; CRITIC("gamma=inf", -2);
  c = good_critic(); c.workspace_bytes -= 1; CRITIC("workspace one byte short", -2);
  c = good_critic(); c.workspace_bytes = 0; CRITIC("workspace_bytes=0", -2);
  c = good_critic(); c.workspace = (char*)c.workspace + 2; CRITIC("workspace off a 4-byte boundary", -2);
  c = good_critic(); c.workspace = (char*)c.workspace + 1; CRITIC("workspace at an odd address", -2);
  c = good_critic(); c.q1 = NULL; CRITIC("q1=NULL", -3);
  c = good_critic(); c.q1_target = NULL; CRITIC("q1_target=NULL", -3);
  c = good_critic(); c.next_log_prob = NULL; CRITIC("next_log_prob=NULL", -3);
  c = good_critic(); c.rewards = NULL; CRITIC("rewards=NULL", -3);
  c = good_critic(); c.dones = NULL; CRITIC("dones=NULL", -3);
  c = good_critic(); c.log_alpha = NULL; CRITIC("log_alpha=NULL", -3);
  c = good_critic(); c.d_q1 = NULL; CRITIC("d_q1=NULL", -3);
  c = good_critic(); c.workspace = NULL; CRITIC("workspace=NULL", -3);
  c = good_critic(); c.q2 = NULL; CRITIC("q2_target and d_q2 without q2", -3);
  c = good_critic(); c.q2_target = NULL; CRITIC("q2 without q2_target", -3);
  c = good_critic(); c.d_q2 = NULL; CRITIC("q2 without d_q2", -3);
  c = good_critic(); c.d_q1 = (float*)c.q1; CRITIC("d_q1 = q1", -3);
  c = good_critic(); c.d_q2 = (float*)c.q2_target + (N_ - 1); CRITIC("d_q2 on the last q2_target", -3);
  c = good_critic(); c.target = (float*)c.rewards + (M_ - 1); CRITIC("target on the last reward (row M-1)", -3);
  c = good_critic(); c.stats = (float*)c.dones + (M_ - 1); CRITIC("stats on the last done (row M-1)", -3);
  c = good_critic(); c.stats = (float*)((int64_t*)c.index + (N_ - 1)); CRITIC("stats on the last index entry", -3);
  c = good_critic(); c.stats = (float*)c.log_alpha; CRITIC("stats = log_alpha", -3);
  c = good_critic(); c.d_q2 = c.d_q1; CRITIC("d_q2 = d_q1", -3);
  c = good_critic(); c.target = c.d_q1 + (N_ - 1); CRITIC("target on the last d_q1", -3);
  c = good_critic(); c.workspace = (void*)c.next_log_prob; CRITIC("workspace = next_log_prob", -3);
  c = good_critic(); c.stats = (float*)((char*)c.workspace + c.workspace_bytes - 4); CRITIC("stats on the workspace's last word", -3);

  /* ---- actor ---- */
  expect_code("actor(NULL)", -1, pdegym_sac_actor_loss(NULL, N_, NULL));
  a = good_actor(); expect_code("actor: N=0", -2, pdegym_sac_actor_loss(&a, 0, NULL));
  a = good_actor(); a.target_entropy = NAN; ACTOR("target_entropy=nan", -2);
  a = good_actor(); a.target_entropy = -INFINITY; ACTOR("target_entropy=-inf", -2);
  a = good_actor(); a.workspace_bytes -= 1; ACTOR("workspace one byte short", -2);
  a = good_actor(); a.workspace = (char*)a.workspace + 2; ACTOR("workspace off a 4-byte boundary", -2);
  a = good_actor(); a.q1_pi = NULL; ACTOR("q1_pi=NULL", -3);
  a = good_actor(); a.log_prob = NULL; ACTOR("log_prob=NULL", -3);
  a = good_actor(); a.log_alpha = NULL; ACTOR("log_alpha=NULL", -3);
  a = good_actor(); a.d_q1_pi = NULL; ACTOR("d_q1_pi=NULL", -3);
  a = good_actor(); a.d_log_prob = NULL; ACTOR("d_log_prob=NULL", -3);
  a = good_actor(); a.d_log_alpha = NULL; ACTOR("d_log_alpha=NULL", -3);
  a = good_actor(); a.workspace = NULL; ACTOR("workspace=NULL", -3);
  a = good_actor(); a.q2_pi = NULL; ACTOR("d_q2_pi without q2_pi", -3);
  a = good_actor(); a.d_q2_pi = NULL; ACTOR("q2_pi without d_q2_pi", -3);
  a = good_actor(); a.d_q1_pi = (float*)a.q1_pi; ACTOR("d_q1_pi = q1_pi", -3);
  a = good_actor(); a.d_log_prob = (float*)a.log_prob + (N_ - 1); ACTOR("d_log_prob on the last log_prob", -3);
  a = good_actor(); a.d_log_alpha = (float*)a.log_alpha; ACTOR("d_log_alpha = log_alpha", -3);
  a = good_actor(); a.d_log_alpha = a.d_log_prob; ACTOR("d_log_alpha = d_log_prob", -3);
  a = good_actor(); a.stats = a.d_q2_pi + (N_ - 1); ACTOR("stats on the last d_q2_pi", -3);
  a = good_actor(); a.d_log_prob = a.stats + 3; ACTOR("d_log_prob on stats[3]", -3);
  a = good_actor(); a.workspace = (void*)a.d_q1_pi; ACTOR("workspace = d_q1_pi", -3);

  /* well-formed descriptors: the host side runs up to the launch; without a device that launch fails with a message */
  s = good_sample(); SAMPLE("launch (fused block)", -100);
  s = good_sample(); s.obs = NULL; s.D = 0; s.ld_obs = 0; s.ld_actions = A_; SAMPLE("launch (actions alone, dense)", -100);
  s = good_sample(); s.A = 8; s.D = 1; s.ld_raw = 16; s.ld_eps = 8; s.ld_obs = 1; s.ld_actions = 9; SAMPLE("launch (A=8, D=1)", -100);
  s = good_sample(); s.A = 1; s.ld_raw = 2; s.ld_eps = 1; s.obs = NULL; s.D = 0; s.ld_actions = 1;
  expect_code("sample: launch (N=1, A=1)", -100, pdegym_squashed_gaussian_sample(&s, 1, NULL));
  s = good_sample(); s.log_prob = s.actions + (size_t)N_ * LD_; SAMPLE("launch (log_prob right after the block)", -100);
  b = good_backward(); BACK("launch (both gradients)", -100);
  b = good_backward(); b.d_actions = NULL; BACK("launch (d_log_prob alone)", -100);
  b = good_backward(); b.d_log_prob = NULL; BACK("launch (d_actions alone)", -100);
  b = good_backward(); b.d_log_prob_stride = 0; BACK("launch (d_log_prob a device scalar)", -100);
  b = good_backward(); b.d_log_prob_stride = 0; b.d_raw = (float*)b.d_log_prob + 1; BACK("launch (d_raw right after the scalar)", -100);
  b = good_backward(); b.d_actions = (const float*)FAKE(3) + D_; b.ld_d_actions = D_ + A_; BACK("launch (d_actions inside a dx block)", -100);
  c = good_critic(); CRITIC("launch (everything given)", -100);
  c = good_critic(); c.q2 = NULL; c.q2_target = NULL; c.d_q2 = NULL; CRITIC("launch (one critic)", -100);
  c = good_critic(); c.index = NULL; c.M = 0; CRITIC("launch (dense: M unused)", -100);
  c = good_critic(); c.target = NULL; c.stats = NULL; CRITIC("launch (no optional outputs)", -100);
  c = good_critic(); c.gamma = 0.0; CRITIC("launch (gamma 0)", -100);
  c = good_critic(); c.workspace_bytes += 4; c.workspace = (char*)c.workspace + 4; CRITIC("launch (workspace 4 bytes on, larger)", -100);
  c = good_critic(); c.index = NULL; c.workspace_bytes = pdegym_sac_loss_workspace(1);
  expect_code("critic: launch (N=1)", -100, pdegym_sac_critic_loss(&c, 1, NULL));
  a = good_actor(); ACTOR("launch (everything given)", -100);
  a = good_actor(); a.q2_pi = NULL; a.d_q2_pi = NULL; ACTOR("launch (one critic)", -100);
  a = good_actor(); a.stats = NULL; ACTOR("launch (no stats)", -100);
  a = good_actor(); a.d_log_alpha = a.d_log_prob + 1; ACTOR("launch (d_log_alpha right after d_log_prob)", -100);

  printf("calls %d bad %d\n", n_calls, n_bad);
  if (n_bad) return 1;
  printf("SAC-LOSS-VALIDATION-OK\n");
  return 0;
}
