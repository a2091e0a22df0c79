/* mlp_gather_validation.c -- argument validation of pdegym_mlp_forward_gather, pdegym_mlp_backward_gather and
 * pdegym_mlp_backward_wide_gather (include/pdegym.h: rows by index) WITHOUT a GPU: a NULL descriptor or index, M < 1, an index off its
 * 8-byte boundary, dx given, dx2 with x2_indexed, x2_indexed with n2 == 0, n2 out of range, the errors of the shadowed entry points, and
 * the byte ranges -- x takes M rows (and x2 with x2_indexed), the index is an input.  Every bad call must come back with the code the
 * header states and a message in pdegym_last_error(); tests/test_mlp_gather.py links it against the host halves of the three files +
 * pdegym_abi.hip built with AddressSanitizer and UndefinedBehaviorSanitizer.  The last group of each part hands over well-formed calls
 * with fake device addresses: the host code then runs up to the launch, which fails cleanly on a machine without a device (-4: no LDS
 * to grant; -100: the launch failed); the pointers are never dereferenced on the host. */
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
    printf("%-60s %5lld  %s\n", what, (long long)rc, msg);
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
    printf("%-60s %5d  %s\n", what, rc, msg);
  }
}

/* 64 MiB apart: no two arrays of the cases below overlap unless a case makes them */
#define FAKE(k) ((void*)(uintptr_t)(0x7f0000000000ull + 0x4000000ull * (k)))
#define B_ 49
#define M_ 1000    /* rows of the storage */
#define K_ 70      /* in_dim = D + n2 */
#define N2_ 4
#define D_ (K_ - N2_)
#define XS_ 72

typedef int (*backward_fn)(const pdegym_mlp*, const pdegym_mlp_backward_cat_args*, const pdegym_mlp_gather*, int32_t, void*);

static pdegym_mlp net_good(int width) {
  pdegym_mlp n;
  memset(&n, 0, sizeof n);
  n.n_layers = 3;
  n.layer[0].w = FAKE(1); n.layer[0].b = FAKE(2); n.layer[0].in_dim = K_; n.layer[0].out_dim = width; n.layer[0].act = PDEGYM_MLP_TANH;
  n.layer[1].w = FAKE(3); n.layer[1].b = FAKE(4); n.layer[1].in_dim = width; n.layer[1].out_dim = 33; n.layer[1].act = PDEGYM_MLP_RELU;
  n.layer[2].w = FAKE(5); n.layer[2].b = FAKE(6); n.layer[2].in_dim = 33; n.layer[2].out_dim = 2; n.layer[2].act = PDEGYM_MLP_IDENTITY;
  return n;
}

static pdegym_mlp_gather gather_good(int x2_indexed) {
  pdegym_mlp_gather g;
  memset(&g, 0, sizeof g);
  g.index = FAKE(26); g.M = M_; g.x2_indexed = x2_indexed;
  return g;
}

/* the arguments of a gather call: no dx, dx2 unless the tail is read by index */
static pdegym_mlp_backward_cat_args args_good(const pdegym_mlp* n, int wide, int params, int x2_indexed) {
  pdegym_mlp_backward_cat_args a;
  memset(&a, 0, sizeof a);
  a.x = FAKE(7); a.x_stride = XS_; a.dy = FAKE(8); a.dy_stride = 3;
  a.x2 = FAKE(24); a.x2_stride = N2_ + 1; a.n2 = N2_;
  if (!x2_indexed) { a.dx2 = FAKE(25); a.dx2_stride = N2_; }
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
  const backward_fn f = wide ? pdegym_mlp_backward_wide_gather : pdegym_mlp_backward_gather;
  const int width = wide ? 256 : 64;
  pdegym_mlp n = net_good(width);
  pdegym_mlp_gather g = gather_good(0);
  pdegym_mlp_backward_cat_args a = args_good(&n, wide, 1, 0);

  /* the gather descriptor */
  expect_code(tag(wide, "NULL gather"), f(&n, &a, NULL, B_, NULL), -1);
  g = gather_good(0); g.index = NULL; expect_code(tag(wide, "NULL index"), f(&n, &a, &g, B_, NULL), -1);
  g = gather_good(0); g.M = 0; expect_code(tag(wide, "M=0"), f(&n, &a, &g, B_, NULL), -2);
  g = gather_good(0); g.M = -5; expect_code(tag(wide, "M=-5"), f(&n, &a, &g, B_, NULL), -2);
  g = gather_good(0); g.index = (const int64_t*)((const char*)g.index + 4); expect_code(tag(wide, "index off an 8-byte boundary"), f(&n, &a, &g, B_, NULL), -2);
  g = gather_good(0);
  a = args_good(&n, wide, 1, 0); a.dx = FAKE(22); a.dx_stride = D_; expect_code(tag(wide, "dx given"), f(&n, &a, &g, B_, NULL), -2);
  a = args_good(&n, wide, 0, 0); a.dx = FAKE(22); a.dx_stride = D_; a.dx2 = NULL; expect_code(tag(wide, "params=0, dx given"), f(&n, &a, &g, B_, NULL), -2);
  g = gather_good(1); a = args_good(&n, wide, 1, 0); expect_code(tag(wide, "dx2 with x2_indexed"), f(&n, &a, &g, B_, NULL), -2);
  g = gather_good(1); a = args_good(&n, wide, 1, 1); a.n2 = 0; a.x2 = NULL; expect_code(tag(wide, "x2_indexed with n2=0"), f(&n, &a, &g, B_, NULL), -2);
  g = gather_good(1); a = args_good(&n, wide, 0, 1); expect_code(tag(wide, "params=0 with x2_indexed (no gradient left to ask for)"), f(&n, &a, &g, B_, NULL), -3);
  g = gather_good(0);

  /* descriptor, limits and arguments: those of the shadowed entry point */
  a = args_good(&n, wide, 1, 0);
  expect_code(tag(wide, "NULL net"), f(NULL, &a, &g, B_, NULL), -1);
  expect_code(tag(wide, "NULL args"), f(&n, NULL, &g, B_, NULL), -1);
  n = net_good(width + 1); expect_code(tag(wide, "a layer one unit too wide"), f(&n, &a, &g, B_, NULL), -2);
  n = net_good(width); n.layer[0].in_dim = 1025; expect_code(tag(wide, "in_dim=1025"), f(&n, &a, &g, B_, NULL), -2);
  n = net_good(width); n.clamp = 1; n.lo = -1; n.hi = 1; expect_code(tag(wide, "clamp set"), f(&n, &a, &g, B_, NULL), -2);
  n = net_good(width);
  expect_code(tag(wide, "B=0"), f(&n, &a, &g, 0, NULL), -2);
  a = args_good(&n, wide, 1, 0); a.n2 = -1; expect_code(tag(wide, "n2=-1"), f(&n, &a, &g, B_, NULL), -2);
  a = args_good(&n, wide, 1, 0); a.n2 = 9; expect_code(tag(wide, "n2=9"), f(&n, &a, &g, B_, NULL), -2);
  a = args_good(&n, wide, 1, 0); a.x2 = NULL; expect_code(tag(wide, "x2=NULL"), f(&n, &a, &g, B_, NULL), -3);
  a = args_good(&n, wide, 1, 0); a.x = NULL; expect_code(tag(wide, "x=NULL"), f(&n, &a, &g, B_, NULL), -3);
  a = args_good(&n, wide, 1, 0); a.dy = NULL; expect_code(tag(wide, "dy=NULL"), f(&n, &a, &g, B_, NULL), -3);
  a = args_good(&n, wide, 1, 0); a.x_stride = D_ - 1; expect_code(tag(wide, "x_stride < D"), f(&n, &a, &g, B_, NULL), -2);
  a = args_good(&n, wide, 1, 0); a.x2_stride = N2_ - 1; expect_code(tag(wide, "x2_stride < n2"), f(&n, &a, &g, B_, NULL), -2);
  a = args_good(&n, wide, 1, 0); a.workspace = NULL; expect_code(tag(wide, "workspace=NULL"), f(&n, &a, &g, B_, NULL), -3);
  a = args_good(&n, wide, 1, 0); a.workspace_bytes -= 1; expect_code(tag(wide, "workspace one byte short"), f(&n, &a, &g, B_, NULL), -2);
  a = args_good(&n, wide, 1, 0); a.slabs = 5; expect_code(tag(wide, "slabs=5 > 4 tiles"), f(&n, &a, &g, B_, NULL), -2);
  a = args_good(&n, wide, 1, 0); a.dw[1] = NULL; expect_code(tag(wide, "dw[1]=NULL"), f(&n, &a, &g, B_, NULL), -3);
  a = args_good(&n, wide, 0, 0); a.dw[1] = FAKE(15); expect_code(tag(wide, "params=0 with dw[1]"), f(&n, &a, &g, B_, NULL), -2);
  a = args_good(&n, wide, 0, 0); a.dx2 = NULL; expect_code(tag(wide, "params=0 without dx2"), f(&n, &a, &g, B_, NULL), -3);

  /* byte ranges: x has M rows, not B; so has x2 with x2_indexed; the index is an input */
  a = args_good(&n, wide, 1, 0); a.dw[0] = (float*)a.x + (size_t)(M_ - 1) * XS_ + D_ - 1; expect_code(tag(wide, "dw[0] on the last float of x's row M-1"), f(&n, &a, &g, B_, NULL), -3);
  a = args_good(&n, wide, 1, 0); a.dx2 = (float*)a.x + (size_t)B_ * XS_; expect_code(tag(wide, "dx2 on row B of x"), f(&n, &a, &g, B_, NULL), -3);
  g = gather_good(1); a = args_good(&n, wide, 1, 1); a.dw[2] = (float*)a.x2 + (size_t)(M_ - 1) * (N2_ + 1); expect_code(tag(wide, "dw[2] on row M-1 of an indexed x2"), f(&n, &a, &g, B_, NULL), -3);
  g = gather_good(0);
  a = args_good(&n, wide, 1, 0); a.dx2 = (float*)g.index; expect_code(tag(wide, "dx2 = index"), f(&n, &a, &g, B_, NULL), -3);
  a = args_good(&n, wide, 1, 0); a.workspace = (char*)g.index + 8 * (B_ - 1); expect_code(tag(wide, "workspace on the last index entry"), f(&n, &a, &g, B_, NULL), -3);

  /* well-formed calls */
  a = args_good(&n, wide, 1, 0); expect_launch(tag(wide, "launch (params, dx2)"), f(&n, &a, &g, B_, NULL));
  a = args_good(&n, wide, 1, 0); a.dx2 = NULL; a.w[0] = NULL; expect_launch(tag(wide, "launch (params, no input gradient, no w[0])"), f(&n, &a, &g, B_, NULL));
  a = args_good(&n, wide, 1, 0); a.dw[2] = (float*)a.x2 + (size_t)(B_ - 1) * (N2_ + 1) + N2_;      /* a dense x2 has B rows */
  expect_launch(tag(wide, "launch (dw[2] right after a dense x2)"), f(&n, &a, &g, B_, NULL));
  a = args_good(&n, wide, 1, 0); a.dx2 = (float*)g.index + 2 * B_; expect_launch(tag(wide, "launch (dx2 right after the index)"), f(&n, &a, &g, B_, NULL));
  a = args_good(&n, wide, 0, 0); expect_launch(tag(wide, "launch (params=0, dx2 alone, no workspace)"), f(&n, &a, &g, B_, NULL));
  g = gather_good(1); a = args_good(&n, wide, 1, 1); expect_launch(tag(wide, "launch (params, x2 by index)"), f(&n, &a, &g, B_, NULL));
  g = gather_good(0); a = args_good(&n, wide, 1, 0); a.n2 = 0; a.x2 = NULL; a.dx2 = NULL; a.x_stride = K_; expect_launch(tag(wide, "launch (params, n2=0: the plain row)"), f(&n, &a, &g, B_, NULL));
  g = gather_good(0); g.M = 1; a = args_good(&n, wide, 1, 0); expect_launch(tag(wide, "launch (M=1)"), f(&n, &a, &g, B_, NULL));
  g = gather_good(0); g.index += 1; a = args_good(&n, wide, 1, 0); a.x = (const char*)a.x + 4; a.x2 += 1;
  expect_launch(tag(wide, "launch (element-aligned pointers displaced)"), f(&n, &a, &g, B_, NULL));
  n = net_good(width); n.x_f64 = 1; g = gather_good(0); a = args_good(&n, wide, 1, 0); expect_launch(tag(wide, "launch (float64 storage)"), f(&n, &a, &g, B_, NULL));
}

int main(void) {
  if (pdegym_abi_version() != PDEGYM_ABI_VERSION) { printf("ABI mismatch\n"); return 1; }
  pdegym_mlp n = net_good(256);
  pdegym_mlp_gather g = gather_good(0);
  void* x = FAKE(7); const float* x2 = FAKE(24); void* y = FAKE(9);

  /* ---- pdegym_mlp_forward_gather ---- */
  expect_code("forward NULL gather", pdegym_mlp_forward_gather(&n, x, XS_, x2, N2_, N2_, NULL, y, 2, B_, NULL), -1);
  g.index = NULL; expect_code("forward NULL index", pdegym_mlp_forward_gather(&n, x, XS_, x2, N2_, N2_, &g, y, 2, B_, NULL), -1);
  g = gather_good(0); g.M = 0; expect_code("forward M=0", pdegym_mlp_forward_gather(&n, x, XS_, x2, N2_, N2_, &g, y, 2, B_, NULL), -2);
  g = gather_good(0); g.index = (const int64_t*)((const char*)g.index + 2); expect_code("forward index off an 8-byte boundary", pdegym_mlp_forward_gather(&n, x, XS_, x2, N2_, N2_, &g, y, 2, B_, NULL), -2);
  g = gather_good(1); expect_code("forward x2_indexed with n2=0", pdegym_mlp_forward_gather(&n, x, XS_, NULL, 0, 0, &g, y, 2, B_, NULL), -2);
  g = gather_good(0);
  expect_code("forward NULL net", pdegym_mlp_forward_gather(NULL, x, XS_, x2, N2_, N2_, &g, y, 2, B_, NULL), -3);
  expect_code("forward x=NULL", pdegym_mlp_forward_gather(&n, NULL, XS_, x2, N2_, N2_, &g, y, 2, B_, NULL), -3);
  expect_code("forward x2=NULL with n2=4", pdegym_mlp_forward_gather(&n, x, XS_, NULL, N2_, N2_, &g, y, 2, B_, NULL), -3);
  expect_code("forward y=NULL", pdegym_mlp_forward_gather(&n, x, XS_, x2, N2_, N2_, &g, NULL, 2, B_, NULL), -3);
  expect_code("forward n2=9", pdegym_mlp_forward_gather(&n, x, XS_, x2, 9, 9, &g, y, 2, B_, NULL), -2);
  expect_code("forward n2=-3", pdegym_mlp_forward_gather(&n, x, XS_, x2, N2_, -3, &g, y, 2, B_, NULL), -2);
  expect_code("forward x_stride < D", pdegym_mlp_forward_gather(&n, x, D_ - 1, x2, N2_, N2_, &g, y, 2, B_, NULL), -2);
  expect_code("forward x2_stride < n2", pdegym_mlp_forward_gather(&n, x, XS_, x2, N2_ - 1, N2_, &g, y, 2, B_, NULL), -2);
  expect_code("forward y_stride < out_dim", pdegym_mlp_forward_gather(&n, x, XS_, x2, N2_, N2_, &g, y, 1, B_, NULL), -2);
  expect_code("forward B=-1", pdegym_mlp_forward_gather(&n, x, XS_, x2, N2_, N2_, &g, y, 2, -1, NULL), -2);
  expect_code("forward x2 off a 4-byte boundary", pdegym_mlp_forward_gather(&n, x, XS_, (const float*)((const char*)x2 + 2), N2_, N2_, &g, y, 2, B_, NULL), -2);
  n = net_good(256); n.layer[0].in_dim = 4; expect_code("forward n2 = in_dim (D = 0)", pdegym_mlp_forward_gather(&n, x, XS_, x2, N2_, N2_, &g, y, 2, B_, NULL), -2);
  n = net_good(257); expect_code("forward 257 units", pdegym_mlp_forward_gather(&n, x, XS_, x2, N2_, N2_, &g, y, 2, B_, NULL), -2);
  n = net_good(256);
  ++n_calls;
  if (pdegym_mlp_forward_gather(&n, x, XS_, x2, N2_, N2_, &g, y, 2, 0, NULL) != 0) { ++n_bad; printf("UNEXPECTED forward B=0 is not a no-op\n"); }
  expect_launch("forward launch (256 units, plain head)", pdegym_mlp_forward_gather(&n, x, XS_, x2, N2_ + 1, N2_, &g, y, 2, B_, NULL));
  expect_launch("forward launch (n2=0: the plain row)", pdegym_mlp_forward_gather(&n, x, K_, NULL, 0, 0, &g, y, 2, B_, NULL));
  g = gather_good(1); expect_launch("forward launch (x2 by index)", pdegym_mlp_forward_gather(&n, x, XS_, x2, N2_, N2_, &g, y, 2, B_, NULL));
  g = gather_good(0);
  n = net_good(64); expect_launch("forward launch (64 units)", pdegym_mlp_forward_gather(&n, x, D_, x2, N2_, N2_, &g, y, 2, B_, NULL));
  n = net_good(128); n.x_f64 = 1; n.y_f64 = 1; expect_launch("forward launch (128 units, float64 storage)", pdegym_mlp_forward_gather(&n, x, XS_, x2, N2_, N2_, &g, y, 2, B_, NULL));
  n = net_good(256); n.clamp = 1; n.lo = -1; n.hi = 1; n.noise = FAKE(30); n.noise_stride = 2;
  expect_launch("forward launch (clamp and noise)", pdegym_mlp_forward_gather(&n, x, XS_, x2, N2_, N2_, &g, y, 2, B_, NULL));
  n = net_good(256); n.head = PDEGYM_MLP_HEAD_SQUASHED_GAUSSIAN; n.clamp = 1; n.lo = -1; n.hi = 1; n.log_std_min = -20; n.log_std_max = 2; n.noise = FAKE(30); n.noise_stride = 1;
  expect_launch("forward launch (squashed-Gaussian head)", pdegym_mlp_forward_gather(&n, x, XS_, x2, N2_, N2_, &g, y, 1, B_, NULL));
  n = net_good(256); g.index += 1; expect_launch("forward launch (index displaced by one entry)", pdegym_mlp_forward_gather(&n, x, XS_, x2, N2_, N2_, &g, y, 2, B_, NULL));

  /* ---- the two backward entry points ---- */
  backward_cases(0);
  backward_cases(1);

  printf("calls %d bad %d\n", n_calls, n_bad);
  if (n_bad) return 1;
  printf("MLP-GATHER-VALIDATION-OK\n");
  return 0;
}
