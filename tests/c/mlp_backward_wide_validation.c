/* mlp_backward_wide_validation.c -- argument validation of pdegym_mlp_backward_wide / pdegym_mlp_backward_wide_workspace
 * (include/pdegym.h) WITHOUT a GPU: descriptor limits (257 units and 1025 inputs refused; 65, 256 and a narrow 64-64 network taken),
 * sizes, null pointers, strides, slab counts, the workspace size, dx with float64 rows, overlapping byte ranges, the two stated
 * alignments.  Every bad call must come back with -1 .. -3 and a message in pdegym_last_error(); tests/test_mlp_backward_wide.py links
 * it against the host half of pdegym_mlp_backward_wide.hip + pdegym_abi.hip built with AddressSanitizer and UndefinedBehaviorSanitizer.
 * The last group hands over well-formed calls with fake device addresses: the host code then runs up to the launch, which fails
 * cleanly on a machine without a device -- at the request for the tile kernel's LDS (-4) or at the launch itself (-100); the pointers
 * are never dereferenced on the host. */
#include <stdio.h>
#include <string.h>

#include "pdegym.h"

static int n_calls = 0, n_bad = 0;

static void expect_error(const char* what, int64_t rc) {
  const char* msg = pdegym_last_error();
  ++n_calls;
  if (rc >= 0 || msg == NULL || msg[0] == '\0') {
    ++n_bad;
    printf("UNEXPECTED %s -> %lld \"%s\"\n", what, (long long)rc, msg ? msg : "(null)");
  } else {
    printf("%-52s %5lld  %s\n", what, (long long)rc, msg);
  }
}

/* a validation error (-1 .. -3), not the failed launch of a call that passed */
static void expect_refused(const char* what, int64_t rc) {
  if (rc < -3) {
    ++n_calls;
    ++n_bad;
    printf("UNEXPECTED %s reached the launch (%lld)\n", what, (long long)rc);
    return;
  }
  expect_error(what, rc);
}

/* a well-formed call: every check passed, the device is missing (-4: no LDS to grant; -100: the launch failed) */
static void expect_launch(const char* what, int rc) {
  if (rc != -100 && rc != -4) {
    ++n_calls;
    ++n_bad;
    printf("UNEXPECTED %s -> %d \"%s\" (a well-formed call fails only at the launch)\n", what, rc, pdegym_last_error());
    return;
  }
  expect_error(what, rc);
}

/* an alignment the header states at the parameter: code -2 (never the failed launch) and the argument's name in the message */
static void expect_misaligned(const char* what, int64_t rc, const char* argument) {
  const char* msg = pdegym_last_error();
  if (rc != -2 || msg == NULL || strstr(msg, argument) == NULL || strstr(msg, "aligned") == NULL) {
    ++n_calls;
    ++n_bad;
    printf("UNEXPECTED %s -> %lld \"%s\" (expected -2 naming %s)\n", what, (long long)rc, msg ? msg : "(null)", argument);
    return;
  }
  expect_error(what, rc);
}

/* 64 MiB apart: no two arrays of the cases below overlap unless a case makes them */
#define FAKE(k) ((void*)(uintptr_t)(0x7f0000000000ull + 0x4000000ull * (k)))
#define B_ 49
#define K_ 70
#define H0_ 256
#define H1_ 65
#define XS_ 72

static pdegym_mlp net_good(void) {
  pdegym_mlp n;
  memset(&n, 0, sizeof n);
  n.n_layers = 3;
  n.layer[0].w = FAKE(1); n.layer[0].b = FAKE(2); n.layer[0].in_dim = K_; n.layer[0].out_dim = H0_; n.layer[0].act = PDEGYM_MLP_TANH;
  n.layer[1].w = FAKE(3); n.layer[1].b = FAKE(4); n.layer[1].in_dim = H0_; n.layer[1].out_dim = H1_; n.layer[1].act = PDEGYM_MLP_RELU;
  n.layer[2].w = FAKE(5); n.layer[2].b = FAKE(6); n.layer[2].in_dim = H1_; n.layer[2].out_dim = 2; n.layer[2].act = PDEGYM_MLP_IDENTITY;
  return n;
}

/* the narrow network of tests/c/mlp_backward_validation.c: the wide entry takes it too */
static pdegym_mlp net_narrow(void) {
  pdegym_mlp n = net_good();
  n.layer[0].out_dim = 64; n.layer[1].in_dim = 64; n.layer[1].out_dim = 64; n.layer[2].in_dim = 64;
  return n;
}

static pdegym_mlp_backward_args args_good(const pdegym_mlp* n) {
  pdegym_mlp_backward_args a;
  memset(&a, 0, sizeof a);
  a.x = FAKE(7); a.x_stride = XS_; a.dy = FAKE(8); a.dy_stride = 3;
  for (int l = 0; l < n->n_layers; ++l) { a.w[l] = FAKE(10 + l); a.dw[l] = FAKE(14 + l); a.db[l] = n->layer[l].b ? FAKE(18 + l) : NULL; }
  a.dx = FAKE(22); a.dx_stride = K_;
  a.slabs = 2;
  a.workspace = FAKE(23);
  a.workspace_bytes = pdegym_mlp_backward_wide_workspace(n, B_, a.slabs);
  return a;
}

int main(void) {
  if (pdegym_abi_version() != PDEGYM_ABI_VERSION) { printf("ABI mismatch\n"); return 1; }
  pdegym_mlp n = net_good();
  pdegym_mlp_backward_args a;
  const int64_t need = pdegym_mlp_backward_wide_workspace(&n, B_, 2);
  /* 4 tiles x 16 rows x (256 + (128 + 256) + (64 + 128)) floats of dZ_l / H_{l-1}, 2 slabs x (70*256+256 + 256*65+65 + 65*2+2) floats */
  ++n_calls;
  if (need != 4 * (4 * 16 * (256 + 128 + 256 + 64 + 128) + 2 * (70 * 256 + 256 + 256 * 65 + 65 + 65 * 2 + 2))) { ++n_bad; printf("UNEXPECTED workspace size %lld\n", (long long)need); }
  /* slabs = 0: min(ceil(tiles / 8), 64) -- 1 slab at 4 tiles, 17 at 129 tiles (B = 2049), 64 from 505 tiles on */
  ++n_calls;
  if (pdegym_mlp_backward_wide_workspace(&n, B_, 0) != pdegym_mlp_backward_wide_workspace(&n, B_, 1)) { ++n_bad; printf("UNEXPECTED: slabs = 0 at 4 tiles is not 1 slab\n"); }
  ++n_calls;
  if (pdegym_mlp_backward_wide_workspace(&n, 2049, 0) != pdegym_mlp_backward_wide_workspace(&n, 2049, 17)) { ++n_bad; printf("UNEXPECTED: slabs = 0 at 129 tiles is not 17 slabs\n"); }
  ++n_calls;
  if (pdegym_mlp_backward_wide_workspace(&n, 32768, 0) != pdegym_mlp_backward_wide_workspace(&n, 32768, 64)) { ++n_bad; printf("UNEXPECTED: slabs = 0 at 2048 tiles is not 64 slabs\n"); }
  ++n_calls;
  if (pdegym_mlp_backward_wide_workspace(&n, 1, 0) != 4 * (16 * (256 + 128 + 256 + 64 + 128) + (70 * 256 + 256 + 256 * 65 + 65 + 65 * 2 + 2))) { ++n_bad; printf("UNEXPECTED workspace size at B = 1\n"); }

  /* the workspace query validates what it can */
  expect_refused("workspace(NULL)", pdegym_mlp_backward_wide_workspace(NULL, B_, 0));
  expect_refused("workspace B=0", pdegym_mlp_backward_wide_workspace(&n, 0, 0));
  expect_refused("workspace slabs=-1", pdegym_mlp_backward_wide_workspace(&n, B_, -1));
  expect_refused("workspace slabs=5 > 4 tiles", pdegym_mlp_backward_wide_workspace(&n, B_, 5));
  n = net_good(); n.layer[1].out_dim = 257; n.layer[2].in_dim = 257; expect_refused("workspace 257 units", pdegym_mlp_backward_wide_workspace(&n, B_, 0));
  n = net_good(); n.layer[0].in_dim = 1025; expect_refused("workspace in_dim=1025", pdegym_mlp_backward_wide_workspace(&n, B_, 0));

  /* descriptor limits */
  n = net_good(); a = args_good(&n);
  expect_refused("backward(NULL net)", pdegym_mlp_backward_wide(NULL, &a, B_, NULL));
  expect_refused("backward(NULL args)", pdegym_mlp_backward_wide(&n, NULL, B_, NULL));
  n = net_good(); n.n_layers = 0; expect_refused("n_layers=0", pdegym_mlp_backward_wide(&n, &a, B_, NULL));
  n = net_good(); n.n_layers = 5; expect_refused("n_layers=5", pdegym_mlp_backward_wide(&n, &a, B_, NULL));
  n = net_good(); n.layer[1].out_dim = 257; n.layer[2].in_dim = 257; expect_refused("a layer of 257 units", pdegym_mlp_backward_wide(&n, &a, B_, NULL));
  n = net_good(); n.layer[0].out_dim = 257; n.layer[1].in_dim = 257; expect_refused("a first layer of 257 units", pdegym_mlp_backward_wide(&n, &a, B_, NULL));
  n = net_good(); n.layer[2].out_dim = 1000; expect_refused("a last layer of 1000 units", pdegym_mlp_backward_wide(&n, &a, B_, NULL));
  n = net_good(); n.layer[0].in_dim = 1025; expect_refused("in_dim=1025", pdegym_mlp_backward_wide(&n, &a, B_, NULL));
  n = net_good(); n.layer[0].in_dim = 0; expect_refused("in_dim=0", pdegym_mlp_backward_wide(&n, &a, B_, NULL));
  n = net_good(); n.layer[2].out_dim = 0; expect_refused("out_dim=0", pdegym_mlp_backward_wide(&n, &a, B_, NULL));
  n = net_good(); n.layer[1].in_dim = 255; expect_refused("layer sizes do not chain", pdegym_mlp_backward_wide(&n, &a, B_, NULL));
  n = net_good(); n.layer[1].act = 3; expect_refused("unknown activation", pdegym_mlp_backward_wide(&n, &a, B_, NULL));
  n = net_good(); n.layer[1].act = -1; expect_refused("negative activation", pdegym_mlp_backward_wide(&n, &a, B_, NULL));
  n = net_good(); n.layer[0].w = NULL; expect_refused("blocked weights NULL", pdegym_mlp_backward_wide(&n, &a, B_, NULL));
  n = net_good(); n.head = PDEGYM_MLP_HEAD_SQUASHED_GAUSSIAN; n.clamp = 1; n.lo = -1; n.hi = 1;
  expect_refused("squashed-Gaussian head", pdegym_mlp_backward_wide(&n, &a, B_, NULL));
  n = net_good(); n.clamp = 1; n.lo = -1; n.hi = 1; expect_refused("clamp set", pdegym_mlp_backward_wide(&n, &a, B_, NULL));
  n = net_good(); n.noise = FAKE(30); n.noise_stride = 2; expect_refused("noise set", pdegym_mlp_backward_wide(&n, &a, B_, NULL));

  /* sizes, pointers, strides, slabs, workspace */
  n = net_good();
  a = args_good(&n); expect_refused("B=0", pdegym_mlp_backward_wide(&n, &a, 0, NULL));
  a = args_good(&n); expect_refused("B=-1", pdegym_mlp_backward_wide(&n, &a, -1, NULL));
  a = args_good(&n); a.x = NULL; expect_refused("x=NULL", pdegym_mlp_backward_wide(&n, &a, B_, NULL));
  a = args_good(&n); a.dy = NULL; expect_refused("dy=NULL", pdegym_mlp_backward_wide(&n, &a, B_, NULL));
  a = args_good(&n); a.workspace = NULL; expect_refused("workspace=NULL", pdegym_mlp_backward_wide(&n, &a, B_, NULL));
  a = args_good(&n); a.dw[1] = NULL; expect_refused("dw[1]=NULL", pdegym_mlp_backward_wide(&n, &a, B_, NULL));
  a = args_good(&n); a.w[2] = NULL; expect_refused("w[2]=NULL", pdegym_mlp_backward_wide(&n, &a, B_, NULL));
  a = args_good(&n); a.w[0] = NULL; expect_refused("w[0]=NULL with dx", pdegym_mlp_backward_wide(&n, &a, B_, NULL));
  a = args_good(&n); a.db[0] = NULL; expect_refused("db[0]=NULL for a layer with bias", pdegym_mlp_backward_wide(&n, &a, B_, NULL));
  n = net_good(); n.layer[1].b = NULL; a = args_good(&n); a.db[1] = FAKE(19);
  expect_refused("db[1] given for a layer without bias", pdegym_mlp_backward_wide(&n, &a, B_, NULL));
  n = net_good();
  a = args_good(&n); a.x_stride = K_ - 1; expect_refused("x_stride < in_dim", pdegym_mlp_backward_wide(&n, &a, B_, NULL));
  a = args_good(&n); a.x_stride = -XS_; expect_refused("x_stride < 0", pdegym_mlp_backward_wide(&n, &a, B_, NULL));
  a = args_good(&n); a.dy_stride = 1; expect_refused("dy_stride < out_dim", pdegym_mlp_backward_wide(&n, &a, B_, NULL));
  a = args_good(&n); a.dx_stride = K_ - 1; expect_refused("dx_stride < in_dim", pdegym_mlp_backward_wide(&n, &a, B_, NULL));
  a = args_good(&n); a.slabs = -1; expect_refused("slabs=-1", pdegym_mlp_backward_wide(&n, &a, B_, NULL));
  a = args_good(&n); a.slabs = 5; expect_refused("slabs=5 > 4 tiles", pdegym_mlp_backward_wide(&n, &a, B_, NULL));
  a = args_good(&n); a.slabs = 2; expect_refused("slabs=2 > 1 tile (B=16)", pdegym_mlp_backward_wide(&n, &a, 16, NULL));
  a = args_good(&n); a.workspace_bytes -= 1; expect_refused("workspace one byte short", pdegym_mlp_backward_wide(&n, &a, B_, NULL));
  a = args_good(&n); a.slabs = 3; expect_refused("workspace sized for 2 slabs, 3 asked", pdegym_mlp_backward_wide(&n, &a, B_, NULL));
  a = args_good(&n); a.workspace_bytes = 0; expect_refused("workspace_bytes=0", pdegym_mlp_backward_wide(&n, &a, B_, NULL));
  a = args_good(&n); a.workspace_bytes = -2;      /* (a refused size query handed on unchecked) */
  expect_refused("workspace_bytes < 0", pdegym_mlp_backward_wide(&n, &a, B_, NULL));
  n = net_good(); n.x_f64 = 1; a = args_good(&n); expect_refused("dx with x_f64", pdegym_mlp_backward_wide(&n, &a, B_, NULL));

  /* no output or workspace overlaps an input or another output, as byte ranges */
  n = net_good();
  a = args_good(&n); a.dx = (float*)a.x; expect_refused("dx = x", pdegym_mlp_backward_wide(&n, &a, B_, NULL));
  a = args_good(&n); a.dw[0] = (float*)a.w[0]; expect_refused("dw[0] = w[0]", pdegym_mlp_backward_wide(&n, &a, B_, NULL));
  a = args_good(&n); a.dw[1] = (float*)a.w[1] + H0_ * H1_ - 1; expect_refused("dw[1] on w[1]'s last float", pdegym_mlp_backward_wide(&n, &a, B_, NULL));
  a = args_good(&n); a.dw[2] = (float*)n.layer[2].w; expect_refused("dw[2] = the blocked copy", pdegym_mlp_backward_wide(&n, &a, B_, NULL));
  a = args_good(&n); a.db[1] = (float*)n.layer[1].b + H1_ - 1; expect_refused("db[1] on the bias' last float", pdegym_mlp_backward_wide(&n, &a, B_, NULL));
  a = args_good(&n); a.db[0] = (float*)a.dy + (size_t)(B_ - 1) * 3 + 1; expect_refused("db[0] on dy's last float", pdegym_mlp_backward_wide(&n, &a, B_, NULL));
  a = args_good(&n); a.dw[0] = a.dw[1]; expect_refused("dw[0] = dw[1]", pdegym_mlp_backward_wide(&n, &a, B_, NULL));
  a = args_good(&n); a.db[2] = a.dw[2] + 2 * H1_ - 1; expect_refused("db[2] on dw[2]'s last float", pdegym_mlp_backward_wide(&n, &a, B_, NULL));
  a = args_good(&n); a.dx = a.dw[0] + 5; expect_refused("dx inside dw[0]", pdegym_mlp_backward_wide(&n, &a, B_, NULL));
  a = args_good(&n); a.workspace = (void*)a.x; expect_refused("workspace = x", pdegym_mlp_backward_wide(&n, &a, B_, NULL));
  a = args_good(&n); a.workspace = (char*)a.dw[1] - a.workspace_bytes + 4; expect_refused("workspace's last float on dw[1]", pdegym_mlp_backward_wide(&n, &a, B_, NULL));
  a = args_good(&n); a.workspace = (char*)a.dx + 4 * ((size_t)(B_ - 1) * K_ + K_ - 1); expect_refused("workspace on dx's last float", pdegym_mlp_backward_wide(&n, &a, B_, NULL));
  n = net_good(); n.x_f64 = 1; a = args_good(&n); a.dx = NULL; a.dw[0] = (float*)a.x + ((size_t)(B_ - 1) * XS_ + K_);      /* past the float32 extent */
  expect_refused("dw[0] inside float64 x", pdegym_mlp_backward_wide(&n, &a, B_, NULL));

  /* the two alignment requirements the header states: refused with -2 and the argument's name, before any launch.  Every other pointer
   * needs only its element's alignment: the launches below include such ones. */
  for (int l = 0; l < 3; ++l)
    for (int off = 4; off < 16; off += 4) {
      n = net_good(); n.layer[l].w = (const float*)((const char*)n.layer[l].w + off); a = args_good(&n);
      expect_misaligned("blocked weights off a 16-byte boundary", pdegym_mlp_backward_wide(&n, &a, B_, NULL), "(w)");
      expect_misaligned("workspace query, blocked weights displaced", pdegym_mlp_backward_wide_workspace(&n, B_, 2), "(w)");
    }
  n = net_good();
  for (int off = 1; off < 4; ++off) {
    a = args_good(&n); a.workspace = (char*)a.workspace + off;
    expect_misaligned("workspace off a 4-byte boundary", pdegym_mlp_backward_wide(&n, &a, B_, NULL), "workspace");
  }
  a = args_good(&n); a.workspace = (char*)a.workspace + 4; a.x = (const char*)a.x + 4; a.dy += 1; a.dx += 3; a.w[1] += 1; a.dw[0] += 1; a.dw[2] += 3; a.db[1] += 1;
  expect_launch("launch (every element-aligned pointer displaced)", pdegym_mlp_backward_wide(&n, &a, B_, NULL));

  /* well-formed calls: the host side runs up to the launch; without a device that fails with a message */
  n = net_good();
  a = args_good(&n); expect_launch("launch (256-65-2, everything given)", pdegym_mlp_backward_wide(&n, &a, B_, NULL));
  a = args_good(&n); a.dx = NULL; a.w[0] = NULL; expect_launch("launch (no dx, no w[0])", pdegym_mlp_backward_wide(&n, &a, B_, NULL));
  a = args_good(&n); a.dw[0] = (float*)a.x + ((size_t)(B_ - 1) * XS_ + K_);      /* touching is not overlapping */
  expect_launch("launch (dw[0] right after x)", pdegym_mlp_backward_wide(&n, &a, B_, NULL));
  a = args_good(&n); a.slabs = 0; a.workspace_bytes = pdegym_mlp_backward_wide_workspace(&n, B_, 0); expect_launch("launch (slabs=0)", pdegym_mlp_backward_wide(&n, &a, B_, NULL));
  a = args_good(&n); a.slabs = 4; a.workspace_bytes = pdegym_mlp_backward_wide_workspace(&n, B_, 4); expect_launch("launch (slabs=tiles)", pdegym_mlp_backward_wide(&n, &a, B_, NULL));
  n = net_good(); n.x_f64 = 1; n.y_f64 = 1; a = args_good(&n); a.dx = NULL; expect_launch("launch (float64 rows)", pdegym_mlp_backward_wide(&n, &a, B_, NULL));
  n = net_good(); n.layer[1].b = NULL; a = args_good(&n); expect_launch("launch (a layer without bias)", pdegym_mlp_backward_wide(&n, &a, B_, NULL));
  n = net_good(); n.layer[0].out_dim = 65; n.layer[1].in_dim = 65; a = args_good(&n); expect_launch("launch (a layer of 65 units)", pdegym_mlp_backward_wide(&n, &a, B_, NULL));
  n = net_good(); n.layer[1].out_dim = 256; n.layer[2].in_dim = 256; n.layer[2].out_dim = 256; a = args_good(&n); a.dy_stride = 256;
  expect_launch("launch (256-256-256)", pdegym_mlp_backward_wide(&n, &a, B_, NULL));
  n = net_narrow(); a = args_good(&n); expect_launch("launch (the narrow 64-64-2 network)", pdegym_mlp_backward_wide(&n, &a, B_, NULL));
  n = net_good(); n.n_layers = 1; n.layer[0].in_dim = 1024; n.layer[0].out_dim = 256; a = args_good(&n); a.x_stride = 1024; a.dx_stride = 1024; a.dy_stride = 256; a.slabs = 1;
  a.workspace_bytes = pdegym_mlp_backward_wide_workspace(&n, 1, 1);
  expect_launch("launch (one layer 1024 -> 256, B=1)", pdegym_mlp_backward_wide(&n, &a, 1, NULL));

  printf("calls %d bad %d\n", n_calls, n_bad);
  if (n_bad) return 1;
  printf("MLP-BACKWARD-WIDE-VALIDATION-OK\n");
  return 0;
}
