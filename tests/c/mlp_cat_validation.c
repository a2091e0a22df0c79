/* mlp_cat_validation.c -- argument validation of pdegym_mlp_forward_cat, pdegym_mlp_backward_cat and pdegym_mlp_backward_wide_cat
 * (include/pdegym.h: the critic(obs, action) call) WITHOUT a GPU: n2 out of range or not below in_dim, the limits of the shadowed entry
 * points (8193 / 1025 inputs, 65 / 257 units), null pointers, strides of both parts, dx with float64 rows, dw / db with params == 0,
 * neither dx nor dx2 with params == 0, dx2 with n2 == 0, overlapping byte ranges with x2 and dx2 among them, the stated alignments.
 * Every bad call must come back with the code the header states and a message in pdegym_last_error(); tests/test_mlp_cat.py links it
 * against the host halves of the three files + pdegym_abi.hip built with AddressSanitizer and UndefinedBehaviorSanitizer.  The last
 * group hands over well-formed calls with fake device addresses: the host code then runs up to the launch, which fails cleanly on a
 * machine without a device (-4: no LDS to grant; -100: the launch failed); the pointers are never dereferenced on the host. */
#include <stdio.h>
#include <string.h>

#include "pdegym.h"

static int n_calls = 0, n_bad = 0;

/* exactly the code the header states, and a message */
static void expect_code(const char* what, int64_t rc, int64_t code) {
  const char* msg = pdegym_last_error();
  ++n_calls;
  if (rc != code || msg == NULL || msg[0] == '\0') {
    ++n_bad;
    printf("UNEXPECTED %s -> %lld \"%s\" (expected %lld)\n", what, (long long)rc, msg ? msg : "(null)", (long long)code);
  } else {
    printf("%-56s %5lld  %s\n", what, (long long)rc, msg);
  }
}

/* a well-formed call: every check passed, the device is missing */
static void expect_launch(const char* what, int rc) {
  const char* msg = pdegym_last_error();
  ++n_calls;
  if ((rc != -100 && rc != -4) || msg == NULL || msg[0] == '\0') {
    ++n_bad;
    printf("UNEXPECTED %s -> %d \"%s\" (a well-formed call fails only at the launch)\n", what, rc, msg ? msg : "(null)");
  } else {
    printf("%-56s %5d  %s\n", what, rc, msg);
  }
}

/* 64 MiB apart: no two arrays of the cases below overlap unless a case makes them */
#define FAKE(k) ((void*)(uintptr_t)(0x7f0000000000ull + 0x4000000ull * (k)))
#define B_ 49
#define K_ 70      /* in_dim = D + n2 */
#define N2_ 4
#define D_ (K_ - N2_)
#define XS_ 72

typedef int (*backward_fn)(const pdegym_mlp*, const pdegym_mlp_backward_cat_args*, int32_t, void*);

static pdegym_mlp net_good(int width) {
  pdegym_mlp n;
  memset(&n, 0, sizeof n);
  n.n_layers = 3;
  n.layer[0].w = FAKE(1); n.layer[0].b = FAKE(2); n.layer[0].in_dim = K_; n.layer[0].out_dim = width; n.layer[0].act = PDEGYM_MLP_TANH;
  n.layer[1].w = FAKE(3); n.layer[1].b = FAKE(4); n.layer[1].in_dim = width; n.layer[1].out_dim = 33; n.layer[1].act = PDEGYM_MLP_RELU;
  n.layer[2].w = FAKE(5); n.layer[2].b = FAKE(6); n.layer[2].in_dim = 33; n.layer[2].out_dim = 2; n.layer[2].act = PDEGYM_MLP_IDENTITY;
  return n;
}

static pdegym_mlp_backward_cat_args args_good(const pdegym_mlp* n, int wide, int params) {
  pdegym_mlp_backward_cat_args a;
  memset(&a, 0, sizeof a);
  a.x = FAKE(7); a.x_stride = XS_; a.dy = FAKE(8); a.dy_stride = 3;
  a.x2 = FAKE(24); a.x2_stride = N2_ + 1; a.n2 = N2_; a.dx2 = FAKE(25); a.dx2_stride = N2_;
  a.dx = FAKE(22); a.dx_stride = D_;
  a.params = params;
  for (int l = 0; l < n->n_layers; ++l) {
    a.w[l] = FAKE(10 + l);
    if (params) { a.dw[l] = FAKE(14 + l); a.db[l] = n->layer[l].b ? FAKE(18 + l) : NULL; }
  }
  if (params) {
    a.slabs = 2;
    a.workspace = FAKE(23);
    a.workspace_bytes = wide ? pdegym_mlp_backward_wide_workspace(n, B_, a.slabs) : pdegym_mlp_backward_workspace(n, B_, a.slabs);
  }
  return a;
}

static char label[128];
static const char* tag(int wide, const char* what) {
  snprintf(label, sizeof label, "%s %s", wide ? "wide" : "narrow", what);
  return label;
}

static void backward_cases(int wide) {
  const backward_fn f = wide ? pdegym_mlp_backward_wide_cat : pdegym_mlp_backward_cat;
  const int width = wide ? 256 : 64;
  pdegym_mlp n = net_good(width);
  pdegym_mlp_backward_cat_args a = args_good(&n, wide, 1);

  /* descriptor and limits: those of the shadowed entry point */
  expect_code(tag(wide, "NULL net"), f(NULL, &a, B_, NULL), -1);
  expect_code(tag(wide, "NULL args"), f(&n, NULL, B_, NULL), -1);
  n = net_good(width + 1); expect_code(tag(wide, "a layer one unit too wide"), f(&n, &a, B_, NULL), -2);
  n = net_good(width); n.layer[0].in_dim = 1025; expect_code(tag(wide, "in_dim=1025"), f(&n, &a, B_, NULL), -2);
  n = net_good(width); n.n_layers = 5; expect_code(tag(wide, "n_layers=5"), f(&n, &a, B_, NULL), -2);
  n = net_good(width); n.clamp = 1; n.lo = -1; n.hi = 1; expect_code(tag(wide, "clamp set"), f(&n, &a, B_, NULL), -2);
  n = net_good(width); n.layer[1].w = (const float*)((const char*)n.layer[1].w + 4); expect_code(tag(wide, "blocked weights off 16 bytes"), f(&n, &a, B_, NULL), -2);
  n = net_good(width);
  a = args_good(&n, wide, 1); expect_code(tag(wide, "B=0"), f(&n, &a, 0, NULL), -2);

  /* the second part */
  a = args_good(&n, wide, 1); a.n2 = -1; expect_code(tag(wide, "n2=-1"), f(&n, &a, B_, NULL), -2);
  a = args_good(&n, wide, 1); a.n2 = 9; expect_code(tag(wide, "n2=9"), f(&n, &a, B_, NULL), -2);
  n = net_good(width); n.layer[0].in_dim = 4; a = args_good(&n, wide, 1); expect_code(tag(wide, "n2 = in_dim (D = 0)"), f(&n, &a, B_, NULL), -2);
  n = net_good(width);
  a = args_good(&n, wide, 1); a.x2 = NULL; expect_code(tag(wide, "x2=NULL"), f(&n, &a, B_, NULL), -3);
  a = args_good(&n, wide, 1); a.x = NULL; expect_code(tag(wide, "x=NULL"), f(&n, &a, B_, NULL), -3);
  a = args_good(&n, wide, 1); a.dy = NULL; expect_code(tag(wide, "dy=NULL"), f(&n, &a, B_, NULL), -3);
  a = args_good(&n, wide, 1); a.n2 = 0; a.x2 = NULL; expect_code(tag(wide, "dx2 with n2=0"), f(&n, &a, B_, NULL), -2);
  a = args_good(&n, wide, 1); a.x2_stride = N2_ - 1; expect_code(tag(wide, "x2_stride < n2"), f(&n, &a, B_, NULL), -2);
  a = args_good(&n, wide, 1); a.dx2_stride = N2_ - 1; expect_code(tag(wide, "dx2_stride < n2"), f(&n, &a, B_, NULL), -2);
  a = args_good(&n, wide, 1); a.x_stride = D_ - 1; expect_code(tag(wide, "x_stride < D"), f(&n, &a, B_, NULL), -2);
  a = args_good(&n, wide, 1); a.dx_stride = D_ - 1; expect_code(tag(wide, "dx_stride < D"), f(&n, &a, B_, NULL), -2);
  a = args_good(&n, wide, 1); a.dy_stride = 1; expect_code(tag(wide, "dy_stride < out_dim"), f(&n, &a, B_, NULL), -2);
  a = args_good(&n, wide, 1); a.x2 = (const float*)((const char*)a.x2 + 2); expect_code(tag(wide, "x2 off a 4-byte boundary"), f(&n, &a, B_, NULL), -2);
  a = args_good(&n, wide, 1); a.dx2 = (float*)((char*)a.dx2 + 1); expect_code(tag(wide, "dx2 off a 4-byte boundary"), f(&n, &a, B_, NULL), -2);
  n = net_good(width); n.x_f64 = 1; a = args_good(&n, wide, 1); expect_code(tag(wide, "dx with x_f64"), f(&n, &a, B_, NULL), -2);
  n = net_good(width);

  /* params != 0: the shadowed pass's requirements */
  a = args_good(&n, wide, 1); a.workspace = NULL; expect_code(tag(wide, "workspace=NULL"), f(&n, &a, B_, NULL), -3);
  a = args_good(&n, wide, 1); a.workspace = (char*)a.workspace + 2; expect_code(tag(wide, "workspace off a 4-byte boundary"), f(&n, &a, B_, NULL), -2);
  a = args_good(&n, wide, 1); a.workspace_bytes -= 1; expect_code(tag(wide, "workspace one byte short"), f(&n, &a, B_, NULL), -2);
  a = args_good(&n, wide, 1); a.slabs = 5; expect_code(tag(wide, "slabs=5 > 4 tiles"), f(&n, &a, B_, NULL), -2);
  a = args_good(&n, wide, 1); a.dw[1] = NULL; expect_code(tag(wide, "dw[1]=NULL"), f(&n, &a, B_, NULL), -3);
  a = args_good(&n, wide, 1); a.db[0] = NULL; expect_code(tag(wide, "db[0]=NULL for a layer with bias"), f(&n, &a, B_, NULL), -3);
  a = args_good(&n, wide, 1); a.w[2] = NULL; expect_code(tag(wide, "w[2]=NULL"), f(&n, &a, B_, NULL), -3);
  a = args_good(&n, wide, 1); a.dx = NULL; a.w[0] = NULL; expect_code(tag(wide, "w[0]=NULL with dx2"), f(&n, &a, B_, NULL), -3);

  /* params == 0 */
  a = args_good(&n, wide, 0); a.dw[1] = FAKE(15); expect_code(tag(wide, "params=0 with dw[1]"), f(&n, &a, B_, NULL), -2);
  a = args_good(&n, wide, 0); a.db[2] = FAKE(20); expect_code(tag(wide, "params=0 with db[2]"), f(&n, &a, B_, NULL), -2);
  a = args_good(&n, wide, 0); a.dx = NULL; a.dx2 = NULL; expect_code(tag(wide, "params=0 with neither dx nor dx2"), f(&n, &a, B_, NULL), -3);
  a = args_good(&n, wide, 0); a.w[0] = NULL; expect_code(tag(wide, "params=0 with w[0]=NULL"), f(&n, &a, B_, NULL), -3);

  /* byte ranges: x2 is an input, dx2 an output */
  a = args_good(&n, wide, 1); a.dx2 = (float*)a.x2; expect_code(tag(wide, "dx2 = x2"), f(&n, &a, B_, NULL), -3);
  a = args_good(&n, wide, 1); a.dx2 = (float*)a.x2 + (size_t)(B_ - 1) * (N2_ + 1) + N2_ - 1; expect_code(tag(wide, "dx2 on x2's last float"), f(&n, &a, B_, NULL), -3);
  a = args_good(&n, wide, 1); a.dx = (float*)a.x2; expect_code(tag(wide, "dx = x2"), f(&n, &a, B_, NULL), -3);
  a = args_good(&n, wide, 1); a.dx2 = a.dx + 5; expect_code(tag(wide, "dx2 inside dx"), f(&n, &a, B_, NULL), -3);
  a = args_good(&n, wide, 1); a.dx2 = a.dw[0] + 7; expect_code(tag(wide, "dx2 inside dw[0]"), f(&n, &a, B_, NULL), -3);
  a = args_good(&n, wide, 1); a.dw[2] = (float*)a.x2 + 3; expect_code(tag(wide, "dw[2] inside x2"), f(&n, &a, B_, NULL), -3);
  a = args_good(&n, wide, 1); a.workspace = (void*)a.x2; expect_code(tag(wide, "workspace = x2"), f(&n, &a, B_, NULL), -3);
  a = args_good(&n, wide, 1); a.workspace = (char*)a.dx2 + 4 * ((size_t)(B_ - 1) * N2_ + N2_ - 1); expect_code(tag(wide, "workspace on dx2's last float"), f(&n, &a, B_, NULL), -3);
  a = args_good(&n, wide, 0); a.dx2 = (float*)a.dy; expect_code(tag(wide, "params=0, dx2 = dy"), f(&n, &a, B_, NULL), -3);
  a = args_good(&n, wide, 0); a.dx = (float*)a.x; expect_code(tag(wide, "params=0, dx = x"), f(&n, &a, B_, NULL), -3);

  /* well-formed calls */
  a = args_good(&n, wide, 1); expect_launch(tag(wide, "launch (params, everything given)"), f(&n, &a, B_, NULL));
  a = args_good(&n, wide, 1); a.dx = NULL; expect_launch(tag(wide, "launch (params, dx2 alone)"), f(&n, &a, B_, NULL));
  a = args_good(&n, wide, 1); a.dx = NULL; a.dx2 = NULL; a.w[0] = NULL; expect_launch(tag(wide, "launch (params, no input gradient, no w[0])"), f(&n, &a, B_, NULL));
  a = args_good(&n, wide, 1); a.dx2 = (float*)a.x2 + (size_t)(B_ - 1) * (N2_ + 1) + N2_;      /* touching is not overlapping */
  expect_launch(tag(wide, "launch (dx2 right after x2)"), f(&n, &a, B_, NULL));
  a = args_good(&n, wide, 1); a.x2 += 1; a.dx2 += 3; a.x = (const char*)a.x + 4; a.dx += 1;
  expect_launch(tag(wide, "launch (element-aligned pointers displaced)"), f(&n, &a, B_, NULL));
  a = args_good(&n, wide, 0); a.dx = NULL; expect_launch(tag(wide, "launch (params=0, dx2 alone, no workspace)"), f(&n, &a, B_, NULL));
  a = args_good(&n, wide, 0); a.dx2 = NULL; a.slabs = 77; expect_launch(tag(wide, "launch (params=0, dx alone, slabs ignored)"), f(&n, &a, B_, NULL));
  a = args_good(&n, wide, 0); a.n2 = 0; a.x2 = NULL; a.dx2 = NULL; a.dx_stride = K_; expect_launch(tag(wide, "launch (params=0, n2=0: the plain row)"), f(&n, &a, B_, NULL));
  n = net_good(width); n.x_f64 = 1; a = args_good(&n, wide, 0); a.dx = NULL; expect_launch(tag(wide, "launch (params=0, float64 rows)"), f(&n, &a, B_, NULL));
  n = net_good(width); n.layer[0].in_dim = 1024; a = args_good(&n, wide, 1); a.n2 = 8; a.x_stride = 1016; a.dx_stride = 1016; a.x2_stride = 8; a.dx2_stride = 8;
  a.workspace_bytes = wide ? pdegym_mlp_backward_wide_workspace(&n, B_, 2) : pdegym_mlp_backward_workspace(&n, B_, 2);
  expect_launch(tag(wide, "launch (D=1016, n2=8)"), f(&n, &a, B_, NULL));
}

int main(void) {
  if (pdegym_abi_version() != PDEGYM_ABI_VERSION) { printf("ABI mismatch\n"); return 1; }
  pdegym_mlp n = net_good(256);
  void* x = FAKE(7); const float* x2 = FAKE(24); void* y = FAKE(9);

  /* ---- pdegym_mlp_forward_cat ---- */
  expect_code("forward NULL net", pdegym_mlp_forward_cat(NULL, x, XS_, x2, N2_, N2_, y, 2, B_, NULL), -3);
  expect_code("forward x=NULL", pdegym_mlp_forward_cat(&n, NULL, XS_, x2, N2_, N2_, y, 2, B_, NULL), -3);
  expect_code("forward x2=NULL", pdegym_mlp_forward_cat(&n, x, XS_, NULL, N2_, N2_, y, 2, B_, NULL), -3);
  expect_code("forward y=NULL", pdegym_mlp_forward_cat(&n, x, XS_, x2, N2_, N2_, NULL, 2, B_, NULL), -3);
  expect_code("forward n2=0", pdegym_mlp_forward_cat(&n, x, XS_, x2, N2_, 0, y, 2, B_, NULL), -2);
  expect_code("forward n2=9", pdegym_mlp_forward_cat(&n, x, XS_, x2, 9, 9, y, 2, B_, NULL), -2);
  expect_code("forward n2=-3", pdegym_mlp_forward_cat(&n, x, XS_, x2, N2_, -3, y, 2, B_, NULL), -2);
  expect_code("forward x_stride < D", pdegym_mlp_forward_cat(&n, x, D_ - 1, x2, N2_, N2_, y, 2, B_, NULL), -2);
  expect_code("forward x2_stride < n2", pdegym_mlp_forward_cat(&n, x, XS_, x2, N2_ - 1, N2_, y, 2, B_, NULL), -2);
  expect_code("forward y_stride < out_dim", pdegym_mlp_forward_cat(&n, x, XS_, x2, N2_, N2_, y, 1, B_, NULL), -2);
  expect_code("forward B=-1", pdegym_mlp_forward_cat(&n, x, XS_, x2, N2_, N2_, y, 2, -1, NULL), -2);
  expect_code("forward x2 off a 4-byte boundary", pdegym_mlp_forward_cat(&n, x, XS_, (const float*)((const char*)x2 + 2), N2_, N2_, y, 2, B_, NULL), -2);
  n = net_good(256); n.layer[0].in_dim = 3; expect_code("forward n2 = in_dim + 1", pdegym_mlp_forward_cat(&n, x, XS_, x2, N2_, N2_, y, 2, B_, NULL), -2);
  n = net_good(256); n.layer[0].in_dim = 4; expect_code("forward n2 = in_dim (D = 0)", pdegym_mlp_forward_cat(&n, x, XS_, x2, N2_, N2_, y, 2, B_, NULL), -2);
  n = net_good(256); n.layer[0].in_dim = 8193; expect_code("forward in_dim=8193", pdegym_mlp_forward_cat(&n, x, 8200, x2, N2_, N2_, y, 2, B_, NULL), -2);
  n = net_good(257); expect_code("forward 257 units", pdegym_mlp_forward_cat(&n, x, XS_, x2, N2_, N2_, y, 2, B_, NULL), -2);
  n = net_good(256); n.layer[2].w = (const float*)((const char*)n.layer[2].w + 8); expect_code("forward blocked weights off 16 bytes", pdegym_mlp_forward_cat(&n, x, XS_, x2, N2_, N2_, y, 2, B_, NULL), -2);
  n = net_good(256); n.clamp = 1; n.lo = 1; n.hi = -1; expect_code("forward clamp lo > hi", pdegym_mlp_forward_cat(&n, x, XS_, x2, N2_, N2_, y, 2, B_, NULL), -2);
  n = net_good(256); n.noise = FAKE(30); n.noise_stride = 1; expect_code("forward noise_stride < out_dim", pdegym_mlp_forward_cat(&n, x, XS_, x2, N2_, N2_, y, 2, B_, NULL), -2);
  n = net_good(256);
  ++n_calls;
  if (pdegym_mlp_forward_cat(&n, x, XS_, x2, N2_, N2_, y, 2, 0, NULL) != 0) { ++n_bad; printf("UNEXPECTED forward B=0 is not a no-op\n"); }
  expect_launch("forward launch (256 units, plain head)", pdegym_mlp_forward_cat(&n, x, XS_, x2, N2_ + 1, N2_, y, 2, B_, NULL));
  n = net_good(64); expect_launch("forward launch (64 units)", pdegym_mlp_forward_cat(&n, x, D_, x2, N2_, N2_, y, 2, B_, NULL));
  n = net_good(128); n.x_f64 = 1; n.y_f64 = 1; expect_launch("forward launch (128 units, float64 rows)", pdegym_mlp_forward_cat(&n, x, XS_, x2, N2_, N2_, y, 2, B_, NULL));
  n = net_good(256); n.clamp = 1; n.lo = -1; n.hi = 1; n.noise = FAKE(30); n.noise_stride = 2;
  expect_launch("forward launch (clamp and noise)", pdegym_mlp_forward_cat(&n, x, XS_, x2, N2_, N2_, y, 2, B_, NULL));
  n = net_good(256); n.head = PDEGYM_MLP_HEAD_SQUASHED_GAUSSIAN; n.clamp = 1; n.lo = -1; n.hi = 1; n.log_std_min = -20; n.log_std_max = 2; n.noise = FAKE(30); n.noise_stride = 1;
  expect_launch("forward launch (squashed-Gaussian head)", pdegym_mlp_forward_cat(&n, x, XS_, x2, N2_, N2_, y, 1, B_, NULL));
  n = net_good(256); n.layer[0].in_dim = 8192; expect_launch("forward launch (D=8184, n2=8)", pdegym_mlp_forward_cat(&n, x, 8184, x2, 8, 8, y, 2, B_, NULL));
  n = net_good(256); expect_launch("forward launch (x2 displaced by one float)", pdegym_mlp_forward_cat(&n, x, XS_, x2 + 1, N2_, N2_, y, 2, B_, NULL));

  /* ---- the two backward entry points ---- */
  backward_cases(0);
  backward_cases(1);

  printf("calls %d bad %d\n", n_calls, n_bad);
  if (n_bad) return 1;
  printf("MLP-CAT-VALIDATION-OK\n");
  return 0;
}
