"""Exactly summable networks and one-hot probes for the MLP policy kernels (tests/test_gpu_mlp_exact.py).

The policy path (pdegym_mlp_forward, and ``eval`` / ``eval_wide`` inside the rollout kernels) is a float32 reduction whose summation
order differs from kernel to kernel and from any BLAS, so against random weights nothing can be asserted exactly.  Two constructions
remove the rounding, so that the comparison is ``assert_array_equal`` against a float64 NumPy reference:

- **Exactly summable networks** (``exact_net`` / ``exact_inputs``): inputs, biases and noise are integers times one power of two (the
  case's ``unit``), weights are -1, 0 or 1, activations Identity or ReLU.  Every partial sum of every neuron, in ANY order and with or
  without fused multiply-adds, is then an integer multiple of the unit; when sum |w| * (bound of the input) + |b| stays below 2**24
  units, every float32 operation is exact.  ``reference`` computes that bound layer by layer in float64 and ``assert_exact`` raises
  when it is not met -- a case is never trimmed or skipped to fit.  A layer whose dense bound would leave the range keeps only as many
  non-zero weights per neuron as fit (``exact_net`` works that number out from the bound of the layer's input).
  A last layer may use tanh: its pre-activation is still exact, the expectation is ``np.tanh`` of it in float64 and the comparison
  uses the policy tolerance of tests/test_policy.py (``TANH_RTOL`` / ``TANH_ATOL``) -- tanhf is then the only inexact operation.
- **One-hot probes** (``one_hot_rows`` / ``one_hot_expected``): ONE Linear layer with ordinary random float32 weights; row r of the
  input is the unit vector e_k(r).  All products are w * 1 or w * 0 and the running sum holds one non-zero term, so the output is
  ``float32(W[:, k]) + float32(b)`` with the bias add as its only rounding -- for every (k, neuron) pair this pins the blocked
  transpose, the weight addressing and the full float32 width of the operands (small integers cannot show a truncated mantissa).

The case lists of the GPU file live here, so that tests/test_mlp_exact_helper.py can check on the CPU that every one of them keeps
the bound, is sensitive to the errors it is meant to catch, and is reproduced by the host wrapper.  Plain helper module (not a
conftest): imported by the tests that need it.
"""
from __future__ import annotations

import dataclasses

import numpy as np

LIMIT = 2.0 ** 24              # float32 holds every integer below it
NET_LIMIT = 2.0 ** 23          # what exact_net plans for: head-room for noise and for inputs wider than its `xmax`
TANH_RTOL, TANH_ATOL = 2e-5, 4e-6      # tests/test_policy.py: kernel against torch float32, here against float64 tanh of an exact value
X_CHUNK = 512                  # csrc/pdegym_mlp.hip: kXChunk
EPS = 2.0 ** -40               # added to non-zero float64 inputs: must round away on the way in


# ---- construction ------------------------------------------------------------------------------------------------------------------------
def exact_net(sizes, acts, seed, bias=True, unit=1.0, xmax=2, head_shift=0):
    """``torch.nn.Sequential`` of Linear (+ ReLU / Tanh) layers ``sizes[0] -> ... -> sizes[-1]`` with weights in {-1, 0, 1} and biases
    in {-3 .. 3} * unit.  ``acts[i]``: None (Identity), "relu", or "tanh" (last layer only).  ``xmax``: bound of |input| in units.
    Layers are dense while sum |w| * bound + 3 stays below ``NET_LIMIT`` units; beyond, a neuron keeps the largest number of non-zero
    weights (at random positions) that does.  The weights of a layer's first and last input are never zero.  ``head_shift`` = s: the LAST layer's weights are {-1, 0, 1} * 2**-s, so that its
    values are multiples of unit * 2**-s and a tanh behind it is not saturated (its biases stay multiples of ``unit``)."""
    import torch
    assert len(acts) == len(sizes) - 1
    rng = np.random.default_rng(seed)
    mods, bound = [], float(xmax)
    for i in range(len(sizes) - 1):
        K, H = int(sizes[i]), int(sizes[i + 1])
        assert acts[i] in (None, "relu") or (acts[i] == "tanh" and i == len(sizes) - 2), "tanh only as the last activation"
        last = i == len(sizes) - 2
        scale = 2.0 ** -head_shift if last else 1.0          # (in units of unit * scale the bias is at most 3 / scale)
        nnz = int(min(K, (NET_LIMIT - 3 / scale - 1) // bound))
        assert nnz >= 1, f"layer {i}: inputs bounded by {bound} units leave no room for a single weight"
        w = rng.integers(-1, 2, (H, K))
        edge = sorted({0, K - 1})          # the first and the last input (the one next to the zero padding) always count
        w[:, edge] = rng.choice((-1, 1), (H, len(edge)))
        if nnz < K:
            keep = np.zeros((H, K), bool)
            keep[:, edge[:nnz]] = True
            for j in range(H):
                keep[j, rng.choice(np.arange(1, K - 1), max(nnz - 2, 0), replace=False)] = True
            w = np.where(keep, w, 0)
        w = (w * scale).astype(np.float32)
        lin = torch.nn.Linear(K, H, bias=bias)
        with torch.no_grad():
            lin.weight.copy_(torch.from_numpy(w))
            if bias:
                lin.bias.copy_(torch.from_numpy((rng.integers(-3, 4, H) * unit).astype(np.float32)))
        mods.append(lin)
        if acts[i] == "relu":
            mods.append(torch.nn.ReLU())
        elif acts[i] == "tanh":
            mods.append(torch.nn.Tanh())
        bound = min(K, nnz) * bound + 3
    return torch.nn.Sequential(*mods)


def exact_inputs(B, K, seed, dtype=np.float32, unit=1.0, lo=-2, hi=2):
    """[B, K] integers of [lo, hi] times ``unit``; the first and the last column hold no zero (a zero there would hide the weights
    of the edge columns)."""
    rng = np.random.default_rng([int(seed), 77])
    v = rng.integers(lo, hi + 1, (B, K))
    for k in {0, K - 1}:
        v[:, k] = np.where(v[:, k] == 0, hi, v[:, k])
    return (v * float(unit)).astype(dtype)


def exact_noise(shape, seed, unit=1.0, lo=-4, hi=4):
    rng = np.random.default_rng([int(seed), 99])
    return (rng.integers(lo, hi + 1, shape) * float(unit)).astype(np.float32)


def layers_of(net):
    """[(W float64 [out, in], b float64 [out] or None, act)] of a Linear / ReLU / Tanh stack."""
    import torch
    out = []
    for m in ([net] if isinstance(net, torch.nn.Linear) else list(net)):
        if isinstance(m, torch.nn.Linear):
            out.append([m.weight.detach().cpu().numpy().astype(np.float64),
                        None if m.bias is None else m.bias.detach().cpu().numpy().astype(np.float64), None])
        elif isinstance(m, torch.nn.ReLU):
            out[-1][2] = "relu"
        elif isinstance(m, torch.nn.Tanh):
            out[-1][2] = "tanh"
        else:
            raise TypeError(type(m).__name__)
    return [tuple(x) for x in out]


# ---- the float64 reference and its bound -----------------------------------------------------------------------------------------------
def reference(net, x, noise=None, clamp=None):
    """``(y, bounds)``: the network on rows ``x`` in NumPy float64, layer by layer, plus ``noise``, clipped to ``clamp``; ``net`` is a
    module or the list ``layers_of`` returns.  ``bounds[l]`` = max over the neurons of layer l of sum_k |w_k| * max_rows |in_k| + |b|:
    no partial sum of the layer, in any order, exceeds it (a last entry covers the noise add).  float64 itself is exact here for the
    same reason with 2**53 in place of 2**24."""
    L = net if isinstance(net, list) else layers_of(net)
    h = np.asarray(x, np.float64)
    bound, bounds = np.abs(h).max(axis=0) if h.shape[0] else np.zeros(h.shape[1]), []
    for W, b, act in L:
        z = h @ W.T + (0.0 if b is None else b)
        bound = np.abs(W) @ bound + (0.0 if b is None else np.abs(b))
        bounds.append(float(bound.max()))
        if act == "tanh":
            h, bound = np.tanh(z), np.minimum(bound, 1.0)
        else:
            h = np.maximum(z, 0.0) if act == "relu" else z
    if noise is not None:
        nz = np.asarray(noise, np.float64).reshape(h.shape)
        h = h + nz
        bounds.append(float(bound.max() + (np.abs(nz).max() if nz.size else 0.0)))
    if clamp is not None:
        h = np.clip(h, clamp[0], clamp[1])
    return h, bounds


def assert_dyadic(unit, **arrays):
    """Every value of every array is an integer multiple of ``unit`` (a power of two)."""
    m, e = np.frexp(unit)
    assert m == 0.5 and unit > 0, f"unit {unit} is not a power of two"
    for name, a in arrays.items():
        if a is None:
            continue
        q = np.asarray(a, np.float64) / unit
        assert np.array_equal(q, np.rint(q)), f"{name} holds values that are no integer multiple of {unit}"


def assert_exact(bounds, unit=1.0, what="case"):
    """Raise unless every layer's bound is below 2**24 units: the premise of the bitwise comparison.  ``unit``: one power of two, or
    one per entry of ``bounds`` (a last layer with scaled weights has a finer unit)."""
    units = np.broadcast_to(np.asarray(unit, np.float64), (len(bounds),))
    worst = float((np.asarray(bounds, np.float64) / units).max())
    if not worst < LIMIT:
        raise AssertionError(f"{what}: a partial sum may reach {worst:.0f} units >= 2**24; float32 arithmetic is not exact for this case")
    return worst


# ---- one-hot probes ------------------------------------------------------------------------------------------------------------------------
def one_hot_rows(K, ks, dtype=np.float32):
    """[len(ks), K]: row r is the unit vector e_{ks[r]}."""
    ks = np.asarray(ks, np.int64)
    assert ks.size and 0 <= ks.min() and ks.max() < K
    x = np.zeros((ks.size, K), dtype)
    x[np.arange(ks.size), ks] = 1
    return x


def one_hot_expected(W, b, ks):
    """[len(ks), H] float32: ``float32(W[:, k]) + float32(b)``, one float32 addition (none without a bias)."""
    W = np.asarray(W)
    assert W.dtype == np.float32
    col = W[:, np.asarray(ks, np.int64)].T.copy()
    out = col if b is None else (col + np.asarray(b, np.float32)[None, :]).astype(np.float32)
    tiny = np.finfo(np.float32).tiny
    assert (np.abs(W) >= tiny).all() and (b is None or (np.abs(b) >= tiny).all()) and (np.abs(out[out != 0]) >= tiny).all(), "denormal operand"
    return out


def real_linear(K, H, seed, bias=True):
    """One ``torch.nn.Linear`` with ordinary random float32 parameters (normal, never denormal, full mantissas)."""
    import torch
    g = torch.Generator().manual_seed(int(seed))
    lin = torch.nn.Linear(K, H, bias=bias)
    with torch.no_grad():
        lin.weight.copy_(torch.randn(H, K, generator=g) * 0.7 + 0.01)
        if bias:
            lin.bias.copy_(torch.randn(H, generator=g) * 0.3 + 0.02)
    return lin


def seam_ks(K):
    """Input indices around every chunk (512) and pipeline (64, 128, 576) seam of pdegym_mlp_forward, and the last one."""
    ks = {0, 63, 64, 127, 128, 511, 512, 513, 575, 576, 1023, 1024, K - 1}
    for m in range(X_CHUNK, K + X_CHUNK, X_CHUNK):
        ks.update((m - 1, m, m + 1))
    return sorted(k for k in ks if 0 <= k < K)


# ---- cases -----------------------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    sizes: tuple
    acts: tuple
    B: int
    seed: int = 0
    bias: bool = True
    unit: float = 1.0
    xlo: int = -2
    xhi: int = 2
    noise: bool = False
    clamp: bool = False
    x_f64: bool = False
    y_f64: bool = False
    head_shift: int = 0       # the last layer's weights are {-1, 0, 1} * 2**-head_shift (tanh heads: pre-activations of O(1))
    eps: bool = False         # float64 inputs v + 2**-40 (v != 0): rounded to v as they are read
    gaps: bool = False        # x_stride > K, y_stride > out_dim, noise_stride > out_dim (forward cases)
    env: tuple = ()           # rollout cases: the engine (see tests/test_gpu_mlp_exact.py)

    @property
    def tanh(self):
        return self.acts[-1] == "tanh"


@dataclasses.dataclass
class Built:
    net: object
    x: np.ndarray             # float64, the exact input values [B, K]
    x_dev: np.ndarray         # what the kernel is given: float32, or float64 (+ EPS on non-zero entries)
    noise: object             # float32 [B, out] or None
    clamp: object             # (lo, hi) or None
    want: np.ndarray          # float64 [B, out]
    bounds: list
    pre: np.ndarray           # float64 [B, out]: the last layer before its activation


def clamp_for(case, y):
    """Dyadic clamp bounds that bind on some outputs: around the 30th and 70th percentile of the unclamped reference, in whole units
    (tanh heads: fixed, their outputs lie in (-1.5, 1.5))."""
    if case.tanh:
        return (-0.5, 0.75)
    lo = float(np.floor(np.percentile(y, 30) / case.unit) * case.unit)
    hi = float(np.ceil(np.percentile(y, 70) / case.unit) * case.unit)
    return (lo, max(lo, hi))


def build(case: Case, x=None) -> Built:
    """Network, inputs, noise, clamp and the float64 expectation of ``case``; the bound is asserted."""
    K, out = case.sizes[0], case.sizes[-1]
    net = exact_net(case.sizes, case.acts, case.seed, case.bias, case.unit, max(abs(case.xlo), abs(case.xhi)), case.head_shift)
    if x is None:
        x = exact_inputs(case.B, K, case.seed, np.float64, case.unit, case.xlo, case.xhi)
    noise = None
    if case.noise:
        noise = exact_noise((case.B, out), case.seed, 0.125, -4, 4) if case.tanh else exact_noise((case.B, out), case.seed, case.unit)
    L = layers_of(net)
    clamp = clamp_for(case, reference(L, x, noise)[0]) if case.clamp else None
    want, bounds = reference(L, x, noise, clamp)
    fine = case.unit * 2.0 ** -case.head_shift
    assert_dyadic(case.unit, x=x, **{f"b{i}": b for i, (_, b, _) in enumerate(L)})
    assert_dyadic(fine, noise=None if case.tanh else noise, clamp=None if (clamp is None or case.tanh) else np.array(clamp))
    assert_dyadic(1.0, **{f"w{i}": w for i, (w, _, _) in enumerate(L[:-1])})
    assert_dyadic(2.0 ** -case.head_shift, w_last=L[-1][0])
    assert_exact(bounds, [case.unit] * (len(L) - 1) + [fine] * (len(bounds) - len(L) + 1), case.name)
    pre = reference(L[:-1] + [(L[-1][0], L[-1][1], None)], x)[0]
    if case.x_f64 or case.env:
        x_dev = np.where(x != 0, x + EPS, 0.0) if case.eps else x.copy()
        assert not case.eps or (x_dev.astype(np.float32) == x).all()
    else:
        x_dev = x.astype(np.float32)
    return Built(net, x, x_dev, noise, clamp, want, bounds, pre)


def _variant(v):
    """Row v of the orthogonal array L8 over five two-level factors: every pair of factor values occurs in two of the eight rows."""
    a, b, c = v & 1, (v >> 1) & 1, (v >> 2) & 1
    return dict(x_f64=bool(a), y_f64=bool(b), gaps=bool(c), bias=not (a ^ b), noise=bool(a ^ c), clamp=bool(a ^ c), eps=bool(a and (b or c)))


FORWARD_K = (1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 127, 128, 129, 511, 512, 513, 575, 576, 577, 1023, 1024, 1025, 1090, 2049, 8191, 8192)
WIDTHS = (1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256)
BATCHES = (1, 15, 16, 17, 33)


def _forward_cases():
    cases = []
    # first-layer K: one hidden layer of 64, one output, 17 rows -- each K plain, and once more in a rotating variant
    for i, K in enumerate(FORWARD_K):
        cases.append(Case(f"K{K}", (K, 64, 1), ("relu", None), 17, seed=K))
        v = 1 + i % 7
        cases.append(Case(f"K{K}-v{v}", (K, 64, 1), ("relu", None), 17, seed=K + 1, **_variant(v)))
    # layer widths at K = 70 (70 % 4 == 2), as hidden and as last layer; the batch walks over the row-tile edges
    for i, W in enumerate(WIDTHS):
        B = BATCHES[i % 5]
        cases.append(Case(f"hidden{W}-B{B}", (70, W, 3), ("relu", None), B, seed=100 + W, **_variant(i % 8)))
        B = BATCHES[(i + 2) % 5]
        cases.append(Case(f"last{W}-B{B}", (70, 16, W), ("relu", None), B, seed=200 + W, **_variant((i + 3) % 8)))
        cases.append(Case(f"single{W}", (70, W), (None,), BATCHES[(i + 4) % 5], seed=300 + W))
    # four-layer stacks with ragged widths that cross the 64 / 128 launch thresholds in different layers
    stacks = [((70, 17, 129, 63, 5), ("relu", "relu", "relu", None), 15), ((6, 256, 255, 16, 33), ("relu", None, "relu", None), 33),
              ((70, 65, 64, 128, 1), ("relu", None, "relu", None), 17), ((130, 128, 129, 127, 256), ("relu", "relu", None, "relu"), 16),
              ((3, 1, 1, 1, 1), (None, "relu", None, None), 1), ((513, 255, 15, 2), ("relu", "relu", None), 17)]
    for i, (sizes, acts, B) in enumerate(stacks):
        cases.append(Case("stack" + "-".join(map(str, sizes)), sizes, acts, B, seed=400 + i))
        cases.append(Case("stack" + "-".join(map(str, sizes)) + f"-v{i + 1}", sizes, acts, B, seed=500 + i, **_variant(i + 1)))
    # tanh heads: exact pre-activation, compared at the policy tolerance
    cases.append(Case("tanh-64-64-1", (64, 64, 1), ("relu", "tanh"), 17, seed=600, head_shift=6))
    cases.append(Case("tanh-70-129-2", (70, 129, 2), ("relu", "tanh"), 33, seed=601, noise=True, clamp=True, gaps=True, head_shift=7))
    cases.append(Case("tanh-577-16-17", (577, 16, 17), (None, "tanh"), 15, seed=602, x_f64=True, y_f64=True, eps=True, head_shift=6))
    return cases


# seeds chosen by hand where the generated one gave a case that tests/test_mlp_exact_helper.py::test_no_case_is_blind refuses (a closed
# ReLU in a network of width one, two edge weights that cancel in the output)
_SEEDS = {"hidden1-B1": 2, "stack3-1-1-1-1": 5, "stack3-1-1-1-1-v5": 5, "rd513-5": 2}


def _reseed(cases):
    return [dataclasses.replace(c, seed=_SEEDS.get(c.name, c.seed)) for c in cases]


FORWARD_CASES = _reseed(_forward_cases())

# one-hot probes of pdegym_mlp_forward: (K, H, rows) -- the full identity sweep (rows None: B = K), or the seams only
ONE_HOT_CASES = [(K, H, None) for K in (5, 64, 130, 513, 1090) for H in (1, 17, 64, 65, 256)] + \
                [(K, H, "seams") for K in (2049, 8192) for H in (64, 256)]


def _rollout_cases():
    """The evaluators inside the rollout kernels.  env: ("1d", kind, control, sensing_loc, nodes) / ("traffic", simulation type) /
    ("tumor", nx).  The observation of a 1D row takes integers -2 .. 2, of the freeway multiples of 1/4 in 0.5 .. 1.5 (densities and
    speeds relative to the steady state), of the tumour row 0 .. 4 cells."""
    P, T = "PDEControlGym-ReactionDiffusionPDE1D", "PDEControlGym-TransportPDE1D"
    D, Nm = "Dirchilet", "Neumann"
    r, n_ = "relu", None
    c = []

    def one_d(name, kind, n, hidden, acts, B, control=D, loc="full", **kw):
        k = 1 if loc != "full" else n
        c.append(Case(name, (k,) + tuple(hidden) + (1,), acts, B, seed=1000 + len(c), env=("1d", kind, control, loc, n), **kw))

    # ---- eval: one neuron per lane (layers of at most 64 units), widths {1, 3, 4, 5, 16, 33, 63, 64}
    one_d("rd30-5-63", P, 30, (5, 63), (r, r, n_), 17, noise=True, clamp=True)        # 30 % 4 == 2, 8 groups: stage() pads to 9
    one_d("tr30-64", T, 30, (64,), (r, n_), 5)
    one_d("rd65-33-4-16", P, 65, (33, 4, 16), (r, n_, r, n_), 17)
    one_d("tr65-1", T, 65, (1,), (n_, n_), 16, bias=False)
    one_d("rd100-3", P, 100, (3,), (r, n_), 33, noise=True)
    one_d("tr100-16-64-tanh", T, 100, (16, 64), (r, r, "tanh"), 17, noise=True, clamp=True, head_shift=7)
    one_d("rd257-64-64", P, 257, (64, 64), (r, r, n_), 17, clamp=True)
    one_d("tr257-linear", T, 257, (), (n_,), 15, bias=False)
    one_d("rd512-4", P, 512, (4,), (r, n_), 5)
    one_d("tr512-32-64", T, 512, (32, 64), (r, r, n_), 17, noise=True)
    one_d("rd513-5", P, 513, (5,), (n_, n_), 17)
    one_d("rd513-lds-limit", P, 513, ("LDS",), (r, n_), 17)                           # the widest first layer that fits into 160 KB
    one_d("tr100-scalar-32-32", T, 100, (32, 32), (r, r, n_), 17, loc="collocated", noise=True, clamp=True)
    one_d("rd65-neumann-scalar-16", P, 65, (16,), (r, n_), 5, control=Nm, loc="collocated")
    one_d("rd129-neumann-64-63", P, 129, (64, 63), (r, r, n_), 17, control=Nm)
    # ---- eval_wide: the cooperative MFMA form, widths {65, 127, 128, 129, 255, 256}; batches that leave idle waves
    one_d("rd257-wide-256-255", P, 257, (256, 255), (r, r, n_), 17, noise=True, clamp=True)
    one_d("tr100-wide-65", T, 100, (65,), (r, n_), 5)
    one_d("tr512-wide-128-129", T, 512, (128, 129), (r, r, n_), 33)
    one_d("rd65-wide-127", P, 65, (127,), (r, n_), 17, bias=False)
    one_d("rd513-wide-16-129", P, 513, (16, 129), (n_, r, n_), 17)
    one_d("tr100-wide-scalar-256-72", T, 100, (256, 72), (r, r, n_), 17, loc="collocated", noise=True)
    one_d("rd129-wide-neumann-127-tanh", P, 129, (127,), (r, "tanh"), 20, control=Nm, noise=True, clamp=True, head_shift=7)

    def traffic(name, sim, hidden, acts, B, **kw):
        A = 2 if sim == "both" else 1
        c.append(Case(name, (102,) + tuple(hidden) + (A,), acts, B, seed=1000 + len(c), unit=0.25, xlo=2, xhi=6, eps=True,
                      env=("traffic", sim), **kw))

    traffic("traffic-both-64-64", "both", (64, 64), (r, r, n_), 17, noise=True, clamp=True)     # 102 % 4 == 2, 26 groups: padded to 27
    traffic("traffic-both-63", "both", (63,), (r, n_), 5)
    traffic("traffic-both-linear", "both", (), (n_,), 16, bias=False)
    traffic("traffic-outlet-33", "outlet", (33,), (r, n_), 17, noise=True)
    traffic("traffic-both-wide-256-255", "both", (256, 255), (r, r, n_), 17, noise=True, clamp=True)
    traffic("traffic-both-wide-65", "both", (65,), (r, n_), 5)
    traffic("traffic-inlet-wide-128-tanh", "inlet", (128,), (r, "tanh"), 33, noise=True, head_shift=7)

    def tumor(name, nx, hidden, acts, B, **kw):
        c.append(Case(name, (nx,) + tuple(hidden) + (1,), acts, B, seed=1000 + len(c), xlo=0, xhi=4, eps=True, env=("tumor", nx), **kw))

    tumor("tumor201-64", 201, (64,), (r, n_), 17, noise=True, clamp=True)
    tumor("tumor201-5-16", 201, (5, 16), (r, r, n_), 5)
    tumor("tumor70-33", 70, (33,), (r, n_), 17)                                      # 70 % 4 == 2, 18 groups: padded to 19
    tumor("tumor201-wide-128", 201, (128,), (r, n_), 17, noise=True)
    tumor("tumor201-wide-129-65", 201, (129, 65), (r, r, n_), 5, clamp=True)
    return c


ROLLOUT_CASES = _rollout_cases()
ROLLOUT_LDS_BYTES = 160 * 1024


def lds_limit_width(n_in):
    """The widest hidden layer H of an n_in -> H -> 1 network that the neuron-per-lane evaluation keeps in 160 KB of LDS
    (FusedMLP.rollout_lds_bytes' own formula is asserted against it in the tests)."""
    def floats(H):
        return sum((((i + 3) // 4) | 1) * 4 * o + 64 for i, o in ((n_in, H), (H, 1))) + 16 * (((n_in + 3) // 4) * 4 + 128)
    H = max(h for h in range(1, 65) if 4 * floats(h) <= ROLLOUT_LDS_BYTES)
    return H


def resolve(case: Case) -> Case:
    """A rollout case with its "LDS" placeholder replaced by the widest layer that fits."""
    if "LDS" in case.sizes:
        return dataclasses.replace(case, sizes=tuple(lds_limit_width(case.sizes[0]) if s == "LDS" else s for s in case.sizes))
    return case


ROLLOUT_CASES = _reseed([resolve(c) for c in ROLLOUT_CASES])
ONE_HOT_ROLLOUT_NODES = (257, 513)      # one Linear layer with real weights through the narrow path: stage()'s re-layout, exactly
