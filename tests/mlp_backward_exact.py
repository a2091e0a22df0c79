"""Float64 reference, exactly summable cases and one-hot probes for the MLP backward pass (pdegym_mlp_backward, FusedMLP.with_grad).

``reference_backward(layers, x, dy)`` restates the backward pass in NumPy float64 and returns, next to the gradients, a bound on every
partial sum of both passes.  As in tests/mlp_exact.py, weights in {-1, 0, 1}, inputs and ``dy`` that are small integers times one power
of two, and Identity / ReLU activations make every product and every partial sum -- in ANY order, fused or not -- an integer multiple
of one unit; while the bounds stay below 2**24 units float32 arithmetic is exact and the GPU comparison is ``assert_array_equal``.

``mlp_exact.exact_net`` plans the forward bound only.  The backward sums grow with B x |dZ| x |H| (dW) and with the width x |dZ|
(dH), so ``sparse_net`` keeps a fixed small number of non-zero weights per neuron (``Case.nnz``: first layer, other layers): hidden
values stay in the hundreds and every case of the list keeps the bound without being trimmed -- ``build`` asserts it.

The GPU case list lives here, so that tests/test_mlp_backward_helper.py can check every case on the CPU.  Plain helper module (not a
conftest): imported by the tests that need it.
"""
from __future__ import annotations

import dataclasses

import numpy as np

from tests import mlp_exact as X

LIMIT = X.LIMIT
ROWS = 16          # rows per tile (csrc/pdegym_mlp_backward.hip: kRows)
MAX_SLABS = 256    # the library's choice for slabs = 0: min(tiles, 256)


# ---- slabs (include/pdegym.h) --------------------------------------------------------------------------------------------------------
def tiles_of(B):
    return (B + ROWS - 1) // ROWS


def slab_rows(B, slabs):
    """[(first row, one past the last row)] of every slab: slab s holds tiles floor(s tiles / slabs) .. floor((s+1) tiles / slabs) - 1."""
    tiles = tiles_of(B)
    slabs = slabs or min(tiles, MAX_SLABS)
    assert 1 <= slabs <= tiles
    return [(min(B, ROWS * (s * tiles // slabs)), min(B, ROWS * ((s + 1) * tiles // slabs))) for s in range(slabs)]


# ---- the reference -------------------------------------------------------------------------------------------------------------------
def _mm(a, b):
    """a @ b; with non-finite entries by plain loops (einsum), so that 0 * Inf = NaN holds term by term whatever a BLAS does."""
    if np.isfinite(a).all() and np.isfinite(b).all():
        return a @ b
    return np.einsum("ij,jk->ik", a, b)


def forward_all(layers, x):
    """[H_0 = x, H_1, ..., H_L] in float64 (ReLU keeps a NaN, as torch.relu and the kernel do)."""
    hs = [np.asarray(x, np.float64)]
    with np.errstate(all="ignore"):
        for W, b, act in layers:
            z = _mm(hs[-1], W.T) + (0.0 if b is None else b)
            hs.append(np.tanh(z) if act == "tanh" else np.where(z <= 0, 0.0, z) if act == "relu" else z)
    return hs


def reference_backward(layers, x, dy, keep_derivative=True, transposed=False):
    """``(grads, bounds)`` of the stack ``layers`` = [(W [out, in], b or None, act)] (``mlp_exact.layers_of``) on rows ``x`` for ``dy`` =
    dLoss/dy, all float64.  ``grads``: {"dw": [..], "db": [..] (None without bias), "dx"}.  ``bounds``: per layer, what no partial sum
    can exceed in magnitude -- "forward" (sum_k |w| max_rows|in| + |b|, from ``mlp_exact.reference``), "dw" = max (|dZ|^T |H|), "db" = max
    sum_rows |dZ|, "dh" = max (|dZ| |W|).  The derivative follows torch: tanh dh (1 - h h); ReLU (h <= 0) ? 0 : dh.
    ``keep_derivative=False`` / ``transposed=True`` are the two mutations the helper test must see: no activation derivative, and W's
    row-major storage read with swapped strides in dH = dZ W."""
    x = np.asarray(x, np.float64)
    hs = forward_all(layers, x)
    finite = np.isfinite(x).all()
    fwd = X.reference(layers, x)[1] if finite else [np.nan] * len(layers)
    g = np.asarray(dy, np.float64)
    n = len(layers)
    dw, db, bounds = [None] * n, [None] * n, [None] * n
    with np.errstate(all="ignore"):
        for l in range(n - 1, -1, -1):
            W, b, act = layers[l]
            h = hs[l + 1]
            if not keep_derivative or act is None:
                dz = g
            elif act == "tanh":
                dz = g * (1.0 - h * h)
            else:
                dz = np.where(h <= 0, 0.0, g)
            dw[l] = _mm(dz.T, hs[l])
            db[l] = None if b is None else dz.sum(axis=0)
            Wd = W.T.reshape(W.shape) if transposed else W
            g = _mm(dz, Wd)
            bounds[l] = {"forward": float(fwd[l]), "dw": float((np.abs(dz).T @ np.abs(hs[l])).max(initial=0.0)),
                         "db": float(np.abs(dz).sum(axis=0).max(initial=0.0)), "dh": float((np.abs(dz) @ np.abs(W)).max(initial=0.0))}
    return {"dw": dw, "db": db, "dx": g}, bounds


def assert_exact(bounds, unit, dunit, what="case"):
    """Every bound below 2**24 of its own unit: forward sums in ``unit``, dZ sums in ``dunit``, dW sums in ``unit * dunit``."""
    worst = 0.0
    for l, b in enumerate(bounds):
        for key, u in (("forward", unit), ("dw", unit * dunit), ("db", dunit), ("dh", dunit)):
            v = b[key] / u
            worst = max(worst, v)
            if not v < LIMIT:
                raise AssertionError(f"{what}: layer {l} {key} may reach {v:.0f} units >= 2**24; float32 arithmetic is not exact for this case")
    return worst


# ---- construction --------------------------------------------------------------------------------------------------------------------
def sparse_net(sizes, acts, seed, bias=True, unit=1.0, nnz=(16, 4)):
    """Linear (+ ReLU) stack with weights in {-1, 0, 1}, at most ``nnz[0]`` / ``nnz[1]`` non-zero per neuron of the first / the other
    layers (the first and the last input always among them), biases in {-3 .. 3} * unit."""
    import torch
    rng = np.random.default_rng([int(seed), 5])
    mods = []
    for i in range(len(sizes) - 1):
        K, H = int(sizes[i]), int(sizes[i + 1])
        assert acts[i] in (None, "relu")
        q = nnz[0] if i == 0 else nnz[1]
        w = rng.choice((-1, 1), (H, K))
        if q < K:
            keep = np.zeros((H, K), bool)
            keep[:, [0, K - 1]] = True
            for j in range(H):
                keep[j, rng.choice(np.arange(1, K - 1), max(q - 2, 0), replace=False)] = True
            w = np.where(keep, w, 0)
        lin = torch.nn.Linear(K, H, bias=bias)
        with torch.no_grad():
            lin.weight.copy_(torch.from_numpy(w.astype(np.float32)))
            if bias:
                lin.bias.copy_(torch.from_numpy((rng.integers(-3, 4, H) * unit).astype(np.float32)))
        mods.append(lin)
        if acts[i] == "relu":
            mods.append(torch.nn.ReLU())
    return torch.nn.Sequential(*mods)


def exact_dy(B, n, seed, dunit=1.0):
    """[B, n] integers of [-2, 2] times ``dunit``, no zero in the first and the last column."""
    rng = np.random.default_rng([int(seed), 31])
    v = rng.integers(-2, 3, (B, n))
    for k in {0, n - 1}:
        v[:, k] = np.where(v[:, k] == 0, 1, v[:, k])
    return (v * float(dunit)).astype(np.float64)


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    sizes: tuple
    acts: tuple
    B: int
    slabs: int = 0
    seed: int = 0
    bias: bool = True
    unit: float = 1.0
    dunit: float = 1.0
    x_f64: bool = False
    eps: bool = False         # float64 inputs v + 2**-40 (v != 0): rounded to v as they are read
    gaps: bool = False        # row strides longer than the rows
    dx: bool = True
    nnz: tuple = (16, 4)


@dataclasses.dataclass
class Built:
    net: object
    layers: list
    x: np.ndarray             # float64, the exact input values
    x_dev: np.ndarray         # what the kernel is given
    dy: np.ndarray            # float64
    want: dict
    bounds: list


def build(case: Case) -> Built:
    net = sparse_net(case.sizes, case.acts, case.seed, case.bias, case.unit, case.nnz)
    x = X.exact_inputs(case.B, case.sizes[0], case.seed, np.float64, case.unit)
    dy = exact_dy(case.B, case.sizes[-1], case.seed, case.dunit)
    L = X.layers_of(net)
    want, bounds = reference_backward(L, x, dy)
    X.assert_dyadic(case.unit, x=x, **{f"b{i}": b for i, (_, b, _) in enumerate(L)})
    X.assert_dyadic(case.dunit, dy=dy)
    X.assert_dyadic(1.0, **{f"w{i}": w for i, (w, _, _) in enumerate(L)})
    assert_exact(bounds, case.unit, case.dunit, case.name)
    if case.x_f64:
        x_dev = np.where(x != 0, x + X.EPS, 0.0) if case.eps else x.copy()
        assert (x_dev.astype(np.float32) == x).all()
    else:
        x_dev = x.astype(np.float32)
    return Built(net, L, x, x_dev, dy, want, bounds)


def valid_slabs(B):
    """The ``slabs`` arguments of {0, 1, 2, 3} that B rows allow."""
    return [s for s in (0, 1, 2, 3) if s <= tiles_of(B)]


def _variant(v):
    """Row v of the orthogonal array L8 (``mlp_exact._variant``) over the factors of the backward pass."""
    a, b, c = v & 1, (v >> 1) & 1, (v >> 2) & 1
    return dict(x_f64=bool(a), gaps=bool(c), bias=not (a ^ b), eps=bool(a and (b or c)), dx=bool(not a and (b or not c)))


IN_DIMS = (1, 3, 4, 5, 63, 64, 65, 70, 513, 1024)
WIDTHS = (1, 15, 16, 17, 63, 64)
BATCHES = (1, 15, 16, 17, 33, 49)


def _slabs_for(B, i):
    ok = valid_slabs(B)
    return ok[i % len(ok)]


def _cases():
    r, n_ = "relu", None
    c = []
    # first-layer in_dim: plain, and once more in a rotating variant; batches and slab counts walk along
    for i, K in enumerate(IN_DIMS):
        B = BATCHES[i % 6]
        c.append(Case(f"K{K}-B{B}", (K, 64, 1), (r, n_), B, _slabs_for(B, i), seed=K))
        B = BATCHES[(i + 3) % 6]
        c.append(Case(f"K{K}-B{B}-v{1 + i % 7}", (K, 17, 3), (r, n_), B, _slabs_for(B, i + 1), seed=K + 1, **_variant(1 + i % 7)))
    # widths at K = 70, as hidden layer, as last layer and alone
    for i, W in enumerate(WIDTHS):
        B = BATCHES[(i + 1) % 6]
        c.append(Case(f"hidden{W}-B{B}", (70, W, 3), (r, n_), B, _slabs_for(B, i + 2), seed=100 + W, **_variant(i % 8)))
        B = BATCHES[(i + 4) % 6]
        c.append(Case(f"last{W}-B{B}", (70, 16, W), (r, n_), B, _slabs_for(B, i + 3), seed=200 + W, **_variant((i + 3) % 8)))
        B = BATCHES[(i + 5) % 6]
        c.append(Case(f"single{W}-B{B}", (70, W), (n_,), B, _slabs_for(B, i), seed=300 + W, **_variant((i + 5) % 8)))
    # the tile loop, the slab store and the slab reduction at the smallest sizes that have them
    c.append(Case("two-tiles-per-slab", (65, 64, 64, 1), (r, r, n_), 49, 2, seed=400))
    c.append(Case("one-tile-per-slab", (65, 64, 64, 1), (r, r, n_), 33, 3, seed=401))
    # 1 .. 4 layers with ragged widths
    stacks = [((70, 64, 64, 64, 1), (r, r, r, n_), 49, 3), ((5, 17, 63, 15, 16), (r, n_, r, n_), 33, 2), ((3, 1, 1, 1, 1), (n_, r, n_, n_), 1, 1),
              ((513, 64, 64, 1), (r, r, n_), 33, 0), ((1024, 64, 17), (r, n_), 49, 3), ((64, 16, 64, 2), (r, r, r), 17, 2)]
    for i, (sizes, acts, B, slabs) in enumerate(stacks):
        name = "stack" + "-".join(map(str, sizes))
        c.append(Case(name, sizes, acts, B, slabs, seed=500 + i))
        c.append(Case(f"{name}-v{i + 1}", sizes, acts, B, slabs, seed=600 + i, **_variant(i + 1)))
    # other units: quarter inputs, dy in eighths
    c.append(Case("units-70-64-64-1", (70, 64, 64, 1), (r, r, n_), 33, 2, seed=700, unit=0.25, dunit=0.125))
    return c


# seeds chosen by hand where the generated one gave a case that tests/test_mlp_backward_helper.py::test_no_case_is_blind refuses
_SEEDS = {"stack3-1-1-1-1": 1, "stack3-1-1-1-1-v3": 1, "stack64-16-64-2": 2, "stack64-16-64-2-v6": 1}
CASES = [dataclasses.replace(c, seed=_SEEDS.get(c.name, c.seed)) for c in _cases()]

# one-hot probes: one Linear layer with ordinary random float32 weights (mlp_exact.real_linear), (in_dim, out_dim)
ONE_HOT_CASES = [(K, H) for K in (5, 64, 130, 513, 1024) for H in (1, 17, 64)]


def seam_ks(K):
    """Input columns around every tile (16), column-chunk (64) and staging-chunk (512) seam of the backward kernels, and the last."""
    ks = {0, 1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 511, 512, 513, 1007, 1008, 1023, K - 1}
    return sorted(k for k in ks if 0 <= k < K)


# real-valued tanh networks of the tolerance test: (sizes, B)
REAL_CASES = [((65, 64, 64, 1), 17), ((65, 64, 64, 1), 4113), ((257, 64, 64, 1), 17), ((257, 64, 64, 1), 4113), ((65, 64, 64, 1), 32768)]
