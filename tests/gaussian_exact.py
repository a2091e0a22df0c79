"""Exactly summable networks for the squashed-Gaussian head (include/pdegym.h: PDEGYM_MLP_HEAD_SQUASHED_GAUSSIAN), in the style of
tests/mlp_exact.py, whose constructions this module uses: the last layer holds the rows [mu; log_std], its weights are
{-1, 0, 1} * 2**-head_shift (the log_std rows times a further power of two, worked out per case so that log_std leaves its bounds
on both sides while mu stays of O(1)), so the 2A pre-activations of a row are exact in float32 in any summation order.  Behind them the head is

    s = clip(log_std, min, max);  z = mu + exp(s) * eps  (no noise: z = mu);  u = tanh(z);  c = clip(lo + 0.5 (u + 1) (hi - lo), lo, hi)

with eps dyadic (multiples of 1/8, |eps| <= 2) and a dyadic box of half-width <= 4.  The expectation is NumPy float64 of that; a kernel
differs from it by its expf (documented within 2 ulp: 2**-20 on |sigma eps| <= 4), the roundings of the product and of the sum
(2**-21 each on |z| <= 8), tanhf and the rescale -- ``tolerance`` below, the bound the GPU tests assert.

tests/test_gaussian_exact_helper.py checks on the CPU, for EVERY case: the exactness bound, ``max |sigma eps| <= 4``, at least half of
the outputs with |z| < 2, and that the expectation moves by more than the tolerance under each mutation of ``MUTATIONS`` (so a wrong
sigma, a wrong order or a wrong half shows); and per case set, log_std below, inside and above its bounds.  No case is trimmed or
skipped to fit; seeds are picked by hand where a generated one is blind (``_SEEDS``).  Plain helper module, not a conftest."""
from __future__ import annotations

import dataclasses

import numpy as np

from tests import mlp_exact as mx

EXP_ATOL = 2.0 ** -19          # expf within 2 ulp on |sigma eps| <= 4: 2**-20; product and sum rounded on |z| <= 8: 2**-21 each
SB3_BOUNDS = (-20.0, 2.0)


def tolerance(box):
    """(rtol, atol) of a command against the float64 expectation: tanh's slope is at most 1, the rescale multiplies by the half width."""
    half = 0.5 * (box[1] - box[0])
    return mx.TANH_RTOL, (mx.TANH_ATOL + EXP_ATOL) * half


@dataclasses.dataclass(frozen=True)
class GCase:
    name: str
    sizes: tuple              # (inputs, hidden ..., A): the last layer has 2 A neurons
    acts: tuple               # activations of the hidden layers (None / "relu")
    B: int
    seed: int = 0
    box: tuple = (-1.0, 3.0)
    bounds: tuple = (-2.0, 0.5)       # log_std_min, log_std_max
    eps_max: float = 2.0              # eps: multiples of 1/8 in [-eps_max, eps_max]; sigma_max * eps_max <= 4
    noise: bool = True
    bias: bool = True
    unit: float = 1.0
    xlo: int = -2
    xhi: int = 2
    x_f64: bool = False
    y_f64: bool = False
    gaps: bool = False
    eps_in: bool = False              # float64 inputs v + 2**-40: rounded to v as they are read
    env: tuple = ()

    @property
    def A(self):
        return self.sizes[-1]

    @property
    def wide(self):
        return max(self.sizes[1:-1] + (2 * self.A,)) > 64


@dataclasses.dataclass
class GBuilt:
    latent: list              # torch modules in front of the heads
    mu: object                # torch.nn.Linear [A, width]
    log_std: object
    x: np.ndarray             # float64 exact inputs [B, K]
    x_dev: np.ndarray         # what the kernel is given
    eps: object               # float32 [B, A] or None
    pre: np.ndarray           # float64 [B, 2A]: [mu | log_std], exact
    want: np.ndarray          # float64 [B, A]
    head_shift: int


def head(pre, eps, bounds, box, mutation=None):
    """The head in float64 on exact pre-activations [B, 2A]; ``mutation``: one of MUTATIONS (what a wrong kernel would compute)."""
    pre = np.asarray(pre, np.float64)
    A = pre.shape[1] // 2
    mu, ls = pre[:, :A], pre[:, A:]
    if mutation == "halves_swapped":
        mu, ls = ls, mu
    lo, hi = box
    s = ls if mutation == "log_std_clamp_dropped" else np.clip(ls, bounds[0], bounds[1])
    with np.errstate(over="ignore"):
        sigma = np.exp(s)
    z = mu
    if eps is not None:
        e = np.asarray(eps, np.float64)
        if mutation == "noise_after_tanh":
            u = np.tanh(mu) + sigma * e
        else:
            z = mu + (e if mutation == "eps_pre_multiplied" else sigma * e)
    if eps is None or mutation != "noise_after_tanh":
        u = np.tanh(z)
    c = u if mutation == "rescale_dropped" else lo + 0.5 * (u + 1.0) * (hi - lo)
    return np.clip(c, lo, hi), z, (sigma * np.asarray(eps, np.float64) if eps is not None else np.zeros_like(mu)), ls


MUTATIONS = ("halves_swapped", "log_std_clamp_dropped", "noise_after_tanh", "rescale_dropped", "eps_pre_multiplied")
DETERMINISTIC_MUTATIONS = ("halves_swapped", "rescale_dropped")      # without noise sigma is not evaluated


def _net(case, head_shift):
    sizes = tuple(case.sizes[:-1]) + (2 * case.A,)
    return mx.exact_net(sizes, tuple(case.acts) + (None,), case.seed, case.bias, case.unit, max(abs(case.xlo), abs(case.xhi)), head_shift)


def build(case: GCase, x=None) -> GBuilt:
    import torch
    K, A = case.sizes[0], case.A
    if x is None:
        x = mx.exact_inputs(case.B, K, case.seed, np.float64, case.unit, case.xlo, case.xhi)
    # the head shift that brings the median |mu| to about 1/2: the generator consumes the same random numbers for every shift
    # (measured without the last bias; the mu biases are scaled to multiples of unit / 4 below, hence a shift of at least 2)
    L0 = mx.layers_of(_net(case, 0))
    L0[-1] = (L0[-1][0][:A], None, None)
    raw = mx.reference(L0, mx.exact_inputs(33, K, case.seed, np.float64, case.unit, case.xlo, case.xhi))[0]
    med = float(np.median(np.abs(raw)))
    shift = max(2, int(np.ceil(np.log2(max(med, 2.0 ** -20) / 0.5))))
    net = _net(case, shift)
    mods = list(net)
    fused = mods[-1]
    # ls_scale, a power of two: the log_std rows' values over the case's rows then span about twice the width of the bounds
    # (over the case's rows and 33 probe rows of the same kind: a batch of one row has no span of its own)
    xs = np.concatenate([x, mx.exact_inputs(33, K, case.seed + 1, np.float64, case.unit, case.xlo, case.xhi)])
    hid = mx.reference(mx.layers_of(torch.nn.Sequential(*mods[:-1])), xs)[0] if mods[:-1] else xs
    ls0 = hid @ fused.weight[A:].detach().numpy().astype(np.float64).T
    span = float((ls0.max(axis=0) - ls0.min(axis=0)).min())
    assert span > 0, f"{case.name}: a log_std neuron takes one value on all rows"
    ls_scale = 2.0 ** int(np.ceil(np.log2(2 * (case.bounds[1] - case.bounds[0]) / span)))
    mu, ls = torch.nn.Linear(fused.in_features, A, bias=case.bias), torch.nn.Linear(fused.in_features, A, bias=case.bias)
    with torch.no_grad():
        mu.weight.copy_(fused.weight[:A])
        ls.weight.copy_(fused.weight[A:] * ls_scale)
        if case.bias:
            mu.bias.copy_(fused.bias[:A] * 0.25)
            # the log_std biases put the middle of each neuron's values (over the case's rows) on the middle of the bounds, in whole
            # units of the row
            u_ls = case.unit * 2.0 ** -shift * ls_scale
            centre = 0.5 * (case.bounds[0] + case.bounds[1]) - 0.5 * ls_scale * (ls0.max(axis=0) + ls0.min(axis=0))
            ls.bias.copy_(torch.from_numpy((np.rint(centre / u_ls) * u_ls).astype(np.float32)))
    L = mx.layers_of(torch.nn.Sequential(*mods[:-1])) if mods[:-1] else []
    Wl = np.concatenate([mu.weight.detach().numpy(), ls.weight.detach().numpy()]).astype(np.float64)
    bl = None if not case.bias else np.concatenate([mu.bias.detach().numpy(), ls.bias.detach().numpy()]).astype(np.float64)
    L = L + [(Wl, bl, None)]
    pre, bounds = mx.reference(L, x)
    fine = case.unit * 2.0 ** -shift
    mx.assert_dyadic(case.unit, x=x, **{f"b{i}": b for i, (_, b, _) in enumerate(L[:-1])})
    mx.assert_dyadic(1.0, **{f"w{i}": w for i, (w, _, _) in enumerate(L[:-1])})
    # exactness is a neuron's own affair: the partial sums of a mu row are multiples of `fine`, those of a log_std row of fine * ls_scale
    for rows, u, what in ((slice(0, A), fine, "mu"), (slice(A, 2 * A), fine * ls_scale, "log_std")):
        mx.assert_dyadic(u / case.unit, **{"w_" + what: Wl[rows]})
        mx.assert_dyadic(u, **{"b_" + what: None if bl is None else bl[rows]})
        half = L[:-1] + [(Wl[rows], None if bl is None else bl[rows], None)]
        mx.assert_exact(mx.reference(half, x)[1], [case.unit] * (len(L) - 1) + [u], f"{case.name} ({what})")
    eps = None
    if case.noise:
        steps = int(round(case.eps_max * 8))
        eps = mx.exact_noise((case.B, A), case.seed, 0.125, -steps, steps)
    mx.assert_dyadic(0.125, eps=eps, box=np.array(case.box))
    assert case.box[0] < case.box[1] and 0.5 * (case.box[1] - case.box[0]) <= 4 and case.eps_max <= 2
    want = head(pre, eps, case.bounds, case.box)[0]
    if case.x_f64 or case.env:
        x_dev = np.where(x != 0, x + mx.EPS, 0.0) if case.eps_in else x.copy()
        assert not case.eps_in or (x_dev.astype(np.float32) == x).all()
    else:
        x_dev = x.astype(np.float32)
    return GBuilt(mods[:-1], mu, ls, x, x_dev, eps, pre, want, shift)


def policy(b: GBuilt, case: GCase, device="cpu", backend=None):
    """``FusedMLP.squashed_gaussian`` of a built case."""
    import torch
    from pdecontrolgym_amd.policy import FusedMLP
    mods = [m.to(device) for m in b.latent]
    return FusedMLP.squashed_gaussian(torch.nn.Sequential(*mods), b.mu.to(device), b.log_std.to(device), case.bounds, backend=backend)


# ---- cases -----------------------------------------------------------------------------------------------------------------------------------
SB3 = dict(bounds=SB3_BOUNDS, eps_max=0.5)       # sigma <= e**2 = 7.39, |sigma eps| <= 3.7
r = "relu"


def _forward_cases():
    """pdegym_mlp_forward: A in {1, 2, 8}; last-layer inputs of 16, 64, 65 and 256 units (the 4-, 8- and 16-wave launches); batches
    1, 15, 17, 33; float64 rows in and out, strides with gaps, noise given and NULL -- rotating over the orthogonal array of
    tests/mlp_exact.py."""
    c = []
    batches = {1: (15, 17, 33, 17), 2: (1, 15, 17, 33), 8: (33, 1, 15, 17)}      # (a batch of one row has its say where A > 1)
    boxes = ((-1.0, 3.0), (0.0, 0.5), (-4.0, 4.0), (0.25, 1.75))
    i = 0
    for A in (1, 2, 8):
        for W in (16, 64, 65, 256):
            v = mx._variant(i % 8)
            kw = dict(x_f64=v["x_f64"], y_f64=v["y_f64"], gaps=v["gaps"], bias=v["bias"], eps_in=v["eps"], noise=(i % 4 != 3))
            if i % 3 == 1:
                kw.update(SB3)
            B = batches[A][i % 4]
            c.append(GCase(f"A{A}-W{W}-B{B}", (70, W, A), (r,), B, seed=2000 + i, box=boxes[i % 4], **kw))
            i += 1
    # the heads directly on the observation, two hidden layers, and the 256-256 actor shape
    c.append(GCase("A2-linear", (65, 2), (), 17, seed=2100, gaps=True))
    c.append(GCase("A1-257-64-64", (257, 64, 64, 1), (r, r), 33, seed=2101, **SB3))
    c.append(GCase("A1-257-256-256", (257, 256, 256, 1), (r, r), 17, seed=2102, box=(-2.0, 2.0)))
    c.append(GCase("A8-513-65-no-noise", (513, 65, 8), (r,), 15, seed=2103, noise=False, x_f64=True, y_f64=True, eps_in=True))
    return c


def _rollout_cases():
    """The evaluators inside the rollout kernels: each environment with a narrow network (<= 64 units: ``eval``) and a wide one
    (65 .. 256: ``eval_wide``) at batches 5, 17 and 33 (the wide batches leave a workgroup with waves that only attend the barriers)."""
    P, T = "PDEControlGym-ReactionDiffusionPDE1D", "PDEControlGym-TransportPDE1D"
    D = "Dirchilet"
    c = []
    envs = [("tr30", ("1d", T, D, "full", 30), 30, 1, dict(box=(-2.0, 2.0))),
            ("rd65", ("1d", P, D, "full", 65), 65, 1, dict(box=(-1.0, 3.0))),
            ("rd257", ("1d", P, D, "full", 257), 257, 1, dict(box=(-4.0, 4.0))),
            ("tr100-scalar", ("1d", T, D, "collocated", 100), 1, 1, dict(box=(-0.5, 1.5))),
            ("traffic-both", ("traffic", "both"), 102, 2, dict(box=(3.0, 6.0), unit=0.25, xlo=2, xhi=6, eps_in=True)),
            ("traffic-outlet", ("traffic", "outlet"), 102, 1, dict(box=(3.5, 5.5), unit=0.25, xlo=2, xhi=6, eps_in=True)),
            ("tumor70", ("tumor", 70), 70, 1, dict(box=(0.0, 0.5), xlo=0, xhi=4, eps_in=True))]
    hidden = {"narrow": [((64,), (r,)), ((33, 16), (r, r)), ((5,), (r,))], "wide": [((256, 255), (r, r)), ((65,), (r,)), ((16, 129), (r, r))]}
    for e, (name, env, K, A, kw) in enumerate(envs):
        for width in ("narrow", "wide"):
            for j, B in enumerate((5, 17, 33)):
                h, acts = hidden[width][(j + e) % 3]
                extra = dict(SB3) if (e + j) % 3 == 1 else {}
                if (e + j) % 4 == 3:
                    extra["noise"] = False
                c.append(GCase(f"{name}-{width}-B{B}", (K,) + h + (A,), acts, B, seed=3000 + len(c), env=env, **kw, **extra))
    return c


# seeds chosen by hand where the generated one gave a case that tests/test_gaussian_exact_helper.py refuses
_SEEDS = {"traffic-both-wide-B5": 3527}      # (five rows, SB3 bounds: no log_std above its bound met a non-zero eps)


def _reseed(cases):
    return [dataclasses.replace(c, seed=_SEEDS.get(c.name, c.seed)) for c in cases]


FORWARD_CASES = _reseed(_forward_cases())
ROLLOUT_CASES = _reseed(_rollout_cases())
CASE_SETS = {"forward": FORWARD_CASES, "rollout": ROLLOUT_CASES}
