"""GPU tests of pdegym_fused_adam (csrc/pdegym_fused_adam.hip) and pde_control_gym.FusedAdam: parameters, moments, mirrors, targets
and the state block BIT FOR BIT against the float32 NumPy restatement (tests/fused_adam_restatement.py) over consecutive steps, the
blocked mirrors against a freshly built ``FusedMLP``, Polyak targets, edge values and non-finite gradients against torch's eager
``clip_grad_norm_`` + ``Adam``, real-valued norms, captured graphs (the optimiser alone, and forward + loss + backward + step of an
attached network), and both examples with the switch on.

Every kernel-level launch goes through ``_run``, which ALWAYS checks the poisoned-buffer contract of tests/poison.py: all tensors
live in guarded buffers, mirrors, total_norm and the workspace start poisoned, after a step every element that must be written is
written, padding entries of blocked mirrors, targets of a call without ``polyak`` and all guards are untouched, the gradients are
bit-unchanged.  ``policy`` displaces every buffer off its 256-byte boundary (tests/poison.py; the workspace, a buffer of 32-bit
words, then starts 4, 8 or 12 bytes past one), and every sequence runs on two differently poisoned workspaces, both held to the
restatement's bits.

Bit comparisons use gradients that are multiples of 2^-10 with |g| <= 4: their squares are multiples of 2^-20 below 2^4 (exact in
float32) and any float64 sum of up to 2^17 of them is exact, so the restatement need not mirror the order of the partial sums.

Tolerance factor of the real-valued comparison with torch: e_kernel <= M_FACTOR * e_torch + 2^-20 (the rule and the floor of
DESIGN.md section 4.13), both errors against the float64 restatement after 10 steps.  M_FACTOR = 2 was measured on the first run of
that case (profiles/r16_fused_adam.json, "tolerance"): (e_kernel, e_torch) = (7.911e-7, 7.911e-7) for the
(256, 256) tensor and (5.534e-7, 5.534e-7) for the (256,) one, both e_torch above 2^-24, worst ratio 1.0 -- doubled and rounded up to
a power of two."""
import importlib.util
import os
import sys

import numpy as np
import pytest

from tests import fused_adam_restatement as R
from tests import poison

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POLICIES = poison.POLICIES
WS_FILLS = (0x7FF8DEAD, -0x0123457)      # (as doubles: a NaN pattern, then a huge negative number)
M_FACTOR = 2
FLOOR = 2.0 ** -20
LR, BETA1, BETA2, EPS, TAU = 3e-4, 0.9, 0.999, 1e-5, 0.005
# an element; around a wave; a workgroup's pass of 1024 with an odd row length; a second pass of a workgroup (65536 > 1024) and one
# workgroup per tensor after it; the table's last slot
TENSOR_LISTS = {"one": [(1,)], "wave": [(3,), (64,), (65,)], "odd": [(255, 5)], "passes": [(256, 256), (256,), (1, 256), (1,)],
                "table": [(1,)] * 32}
MIRROR_GRID = [(o, i) for i in (1, 3, 4, 5, 66) for o in (1, 2, 64, 65, 256)]


def _backend():
    from pdecontrolgym_amd.backend import default_backend
    return default_backend()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize])


def _same(a, b, what):
    """Bit equality; two NaNs count as equal whatever their payloads (host and device produce different ones)."""
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, f"{what}: {a.shape} {a.dtype} against {b.shape} {b.dtype}"
    bad = (_bits(a) != _bits(b)) & ~(np.isnan(a) & np.isnan(b))
    assert not bad.any(), f"{what}: {int(bad.sum())} of {a.size} element(s) differ"


def exact_grads(shapes, rng, big=True):
    """Multiples of 2^-10 with |g| <= 4; ``big``: the first element is 3.0, so the norm is above any bound below 3."""
    gs = [(rng.integers(-4096, 4097, s) / 1024.0).astype(np.float32) for s in shapes]
    if big:
        gs[0].reshape(-1)[0] = 3.0
    return gs


def make_case(shapes, rng, mirrors=True, targets=True):
    """Real-valued parameters and moments; 2-D tensors get a blocked mirror, 1-D ones a plain copy; every tensor a target."""
    case = []
    for s in shapes:
        t = {"p": rng.standard_normal(s).astype(np.float32), "m": (0.1 * rng.standard_normal(s)).astype(np.float32),
             "v": (0.01 * rng.random(s) + 1e-4).astype(np.float32), "blocked": mirrors and len(s) == 2, "copy": mirrors and len(s) == 1}
        if targets:
            t["pt"] = rng.standard_normal(s).astype(np.float32)
        case.append(t)
    return case


def _run(case, grads, max_norm, polyak, policy=None, ws_fill=WS_FILLS[0], lr=LR, eps=EPS):
    """``len(grads)`` consecutive pdegym_fused_adam calls on guarded copies of ``case`` and the same steps of the float32 restatement;
    asserts the contract and bit equality after EVERY step.  ``polyak``: one flag per step.  Returns the device results of the last
    step as NumPy arrays."""
    be = _backend()
    arena = poison.Arena("cuda", policy=policy)
    f32 = torch.float32
    entries, ref = [], []
    for k, t in enumerate(case):
        s = t["p"].shape
        e = {n: arena.like(f"{n}{k}", torch.from_numpy(t[n])) for n in ("p", "m", "v")}
        e["g"] = arena.new(f"g{k}", s, f32)
        r = {n: t[n].copy() for n in ("p", "m", "v")}
        geometry = (s[0], s[1]) if len(s) == 2 else (1, s[0])
        prefixes = [""] + (["pt_"] if "pt" in t else [])
        if "pt" in t:
            e["pt"] = arena.like(f"pt{k}", torch.from_numpy(t["pt"]))
            r["pt"] = t["pt"].copy()
        for pre in prefixes:
            if t["copy"]:
                e[pre + "copy"] = poison.poison_(arena.new(f"{pre}copy{k}", s, f32))
                r[pre + "copy"] = np.zeros(s, np.float32)
            if t["blocked"]:
                out, in_ = geometry
                wt = poison.poison_(arena.new(f"{pre}wt{k}", ((in_ + 3) // 4, out + 3, 4), f32))      # rows 2 .. 2 + out of out + 3
                e[pre + "wt"] = (wt, out + 3, 2)
                r[pre + "wt"] = (np.zeros(((in_ + 3) // 4, out + 3, 4), np.float32), out + 3, 2)
        entries.append(e)
        ref.append(r)
    state = arena.new("state", (3,), torch.float64)
    state.copy_(torch.tensor([0.0, 1.0, 1.0], dtype=torch.float64))
    ref_state = R.new_state()
    total = poison.poison_(arena.new("total_norm", (1,), f32)) if max_norm is not None else None
    need = be.fused_adam_workspace([t["p"].size for t in case])
    ws = arena.new("workspace", (need // 4,), torch.int32)
    written = {}
    for it, (gs, pk) in enumerate(zip(grads, polyak)):
        ws.fill_(ws_fill)
        for e, r, g in zip(entries, ref, gs):
            e["g"].copy_(torch.from_numpy(g))
            r["g"] = g
        be.fused_adam(entries, state, ws.view(torch.uint8), lr, BETA1, BETA2, eps, max_grad_norm=max_norm, tau=TAU, polyak=pk,
                      total_norm=total)
        want_total = R.step(ref, ref_state, lr, BETA1, BETA2, eps, max_norm, TAU, pk, dtype=np.float32)
        arena.check()
        _same(state.cpu().numpy(), ref_state, f"state after step {it}")
        if total is not None:
            poison.assert_written(total, None, "total_norm")
            _same(total.cpu().numpy(), np.array([want_total], np.float32), f"total_norm after step {it}")
        for k, (e, r, g) in enumerate(zip(entries, ref, gs)):
            _same(e["g"].cpu().numpy(), g, f"g{k} (an input)")
            for n in ("p", "m", "v"):
                _same(e[n].cpu().numpy(), r[n], f"{n}{k} after step {it}")
            for pre in ("", "pt_"):
                done = pre == "" or written.get(k) or pk
                if pre == "pt_" and "pt" in e:
                    if done:
                        _same(e["pt"].cpu().numpy(), r["pt"], f"pt{k} after step {it}")
                        written[k] = True
                    else:
                        _same(e["pt"].cpu().numpy(), case[k]["pt"], f"pt{k} without polyak")
                if pre + "copy" in e:
                    if done:
                        poison.assert_written(e[pre + "copy"], None, f"{pre}copy{k}")
                        _same(e[pre + "copy"].cpu().numpy(), r[pre + "copy"], f"{pre}copy{k} after step {it}")
                    else:
                        poison.assert_untouched(e[pre + "copy"], None, f"{pre}copy{k} without polyak")
                if pre + "wt" in e:
                    wt, out_total, row0 = e[pre + "wt"]
                    s = case[k]["p"].shape
                    out, in_ = (s[0], s[1]) if len(s) == 2 else (1, s[0])
                    live = torch.zeros(wt.shape, dtype=torch.bool, device="cuda")
                    if done:
                        live[:, row0:row0 + out, :] = True
                        if in_ % 4:
                            live[-1, :, in_ % 4:] = False      # padding entries of the last block
                        poison.assert_written(wt, live, f"{pre}wt{k}")
                        _same(wt[live].cpu().numpy(), r[pre + "wt"][0][live.cpu().numpy()], f"{pre}wt{k} after step {it}")
                    poison.assert_untouched(wt, ~live, f"{pre}wt{k}: padding, other rows" + ("" if done else ", everything without polyak"))
    return {"p": [e["p"].cpu().numpy() for e in entries], "total": None if total is None else float(total[0])}


# ---- bit for bit against the float32 restatement -------------------------------------------------------------------------------------
@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("clip", ["off", "active", "coef-one"])
@pytest.mark.parametrize("name", list(TENSOR_LISTS))
def test_three_steps_equal_the_restatement_bit_for_bit(name, clip, policy):
    shapes = TENSOR_LISTS[name]
    rng = np.random.default_rng(len(shapes) + 7)
    case = make_case(shapes, rng)
    grads = [exact_grads(shapes, rng) for _ in range(3)]
    max_norm = {"off": None, "active": 0.5, "coef-one": 1.0e6}[clip]
    for g in grads:      # the case is what it claims to be
        total = np.float32(np.sqrt(sum((x.astype(np.float32) ** 2).astype(np.float64).sum() for x in g)))
        if clip == "active":
            assert total > 0.5 and np.float32(0.5) / (total + np.float32(1e-6)) < 1.0
        if clip == "coef-one":
            assert min(np.float32(max_norm) / (total + np.float32(1e-6)), np.float32(1.0)) == np.float32(1.0)
    results = [_run(case, grads, max_norm, (False, True, True), policy, fill) for fill in WS_FILLS]
    for a, b in zip(results[0]["p"], results[1]["p"]):
        _same(a, b, "two workspaces")


@pytest.mark.parametrize("policy", POLICIES)
def test_blocked_mirrors_of_every_row_length_and_width(policy):
    """in_dim in {1, 3, 4, 5, 66} x out in {1, 2, 64, 65, 256}: 25 weights with blocked mirrors (and blocked target mirrors) in one call."""
    rng = np.random.default_rng(11)
    case = make_case(MIRROR_GRID, rng)
    grads = [exact_grads(MIRROR_GRID, rng) for _ in range(3)]
    for fill in WS_FILLS:
        _run(case, grads, 0.5, (True, False, True), policy, fill)


@pytest.mark.parametrize("in_dim,out_dim", MIRROR_GRID)
def test_attached_wrapper_equals_a_fresh_one_after_every_step(in_dim, out_dim):
    from pde_control_gym import FusedAdam, FusedMLP
    torch.manual_seed(in_dim * 1000 + out_dim)
    net = torch.nn.Sequential(torch.nn.Linear(in_dim, out_dim), torch.nn.Tanh(), torch.nn.Linear(out_dim, 3)).cuda()
    f = FusedMLP(net)
    params = list(net.parameters())
    opt = FusedAdam(params, lr=1e-2, max_grad_norm=0.5).attach(f)
    obs = torch.randn(37, in_dim, device="cuda")
    for _ in range(3):
        for p in params:
            p.grad = torch.randn_like(p)
        opt.step()
        seen = list(f._seen)
        out = f(obs)
        assert f._seen == seen and seen == [w._version for w, _, _ in f.layers]      # refresh() found nothing to do
        fresh = FusedMLP(net)
        for a, b in zip(f._wt, fresh._wt):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))
        assert torch.equal(out.view(torch.int32), fresh(obs).view(torch.int32))


def test_attached_squashed_gaussian_wrapper_equals_a_fresh_one():
    from pde_control_gym import FusedAdam, FusedMLP
    torch.manual_seed(3)
    latent = torch.nn.Sequential(torch.nn.Linear(5, 64), torch.nn.ReLU(), torch.nn.Linear(64, 65), torch.nn.ReLU()).cuda()
    mu, ls = torch.nn.Linear(65, 2).cuda(), torch.nn.Linear(65, 2).cuda()
    make = lambda: FusedMLP.squashed_gaussian(latent, mu, ls)      # noqa: E731
    f = make()
    params = list(latent.parameters()) + list(mu.parameters()) + list(ls.parameters())
    opt = FusedAdam(params, lr=1e-2, max_grad_norm=0.5).attach(f)
    obs, eps = torch.randn(33, 5, device="cuda"), torch.randn(33, 2, device="cuda")
    for _ in range(3):
        for p in params:
            p.grad = torch.randn_like(p)
        opt.step()
        fresh = make()
        for a, b in zip(f._wt + [f._fused.weight.detach(), f._fused.bias.detach()],
                        fresh._wt + [fresh._fused.weight.detach(), fresh._fused.bias.detach()]):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))
        outs = [w.forward_into(obs, torch.empty(33, 2, device="cuda"), clamp=(-10.0, 10.0), noise=eps) for w in (f, fresh)]
        raws = [w.with_grad(obs) for w in (f, fresh)]
        assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))
        assert torch.equal(raws[0].detach().view(torch.int32), raws[1].detach().view(torch.int32))


# ---- Polyak targets ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("policy", POLICIES)
def test_targets_and_their_mirrors_follow_only_with_polyak(policy):
    """(``_run`` holds target, plain and blocked target mirrors to the restatement after a polyak step and to their poison before.)"""
    shapes = [(65, 66), (65,), (2, 65), (2,)]
    rng = np.random.default_rng(5)
    case = make_case(shapes, rng)
    grads = [exact_grads(shapes, rng) for _ in range(4)]
    for fill in WS_FILLS:
        _run(case, grads, None, (False, False, True, False), policy, fill)


# ---- edge values ------------------------------------------------------------------------------------------------------------------------
def test_zero_gradients_and_zero_moments_leave_the_parameters_unchanged():
    shapes = [(65, 5), (7,)]
    rng = np.random.default_rng(6)
    case = make_case(shapes, rng)
    for t in case:
        t["m"][...] = 0.0
        t["v"][...] = 0.0
    zeros = [[np.zeros(s, np.float32) for s in shapes]] * 2
    for max_norm in (None, 0.5):
        out = _run(case, zeros, max_norm, (False, False))
        for a, t in zip(out["p"], case):
            _same(a, t["p"], "p after zero gradients")
        assert max_norm is None or out["total"] == 0.0


def _torch_reference(case, grads, max_norm, eps=EPS, lr=LR):
    """torch's eager float32 clip_grad_norm_ + Adam on the device, from the case's moments (its own step count starts at 0 too)."""
    params = [torch.nn.Parameter(torch.from_numpy(t["p"]).cuda()) for t in case]
    opt = torch.optim.Adam(params, lr=lr, betas=(BETA1, BETA2), eps=eps)
    for p, t in zip(params, case):
        opt.state[p] = {"step": torch.tensor(0.0), "exp_avg": torch.from_numpy(t["m"]).cuda(), "exp_avg_sq": torch.from_numpy(t["v"]).cuda()}
    totals = []
    for gs in grads:
        for p, g in zip(params, gs):
            p.grad = torch.from_numpy(g).cuda()
        if max_norm is not None:
            totals.append(float(torch.nn.utils.clip_grad_norm_(params, max_norm)))
        opt.step()
    return [p.detach().cpu().numpy() for p in params], totals


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")])
def test_a_non_finite_gradient_gives_torchs_nan_pattern(bad):
    shapes = [(65, 5), (64,), (1,)]
    rng = np.random.default_rng(8)
    case = make_case(shapes, rng, mirrors=False, targets=False)
    grads = [exact_grads(shapes, rng) for _ in range(2)]
    grads[0][1][17] = bad
    mine = _run(case, grads, 0.5, (False, False))["p"]
    want, _ = _torch_reference(case, grads, 0.5)
    for k, (a, b) in enumerate(zip(mine, want)):
        assert np.array_equal(np.isnan(a), np.isnan(b)), f"tensor {k}: NaN pattern differs from torch's"
        assert np.array_equal(np.isinf(a), np.isinf(b)), f"tensor {k}: Inf pattern differs from torch's"
    assert any(np.isnan(a).any() for a in mine)


# ---- real-valued gradients: the norm, and the parameters against torch ----------------------------------------------------------------------
_pairs = None


def tolerance_pairs():
    """(tensor, e_kernel, e_torch) after 10 steps of N(0, 1) gradients at [(256, 256), (256,)], clip 0.5, both against the float64
    restatement; and the norms of the first step.  Computed once."""
    global _pairs
    if _pairs is not None:
        return _pairs
    shapes = [(256, 256), (256,)]
    rng = np.random.default_rng(9)
    case = make_case(shapes, rng, mirrors=False, targets=False)
    grads = [[rng.standard_normal(s).astype(np.float32) for s in shapes] for _ in range(10)]
    be = _backend()
    dev = [{n: torch.from_numpy(t[n]).cuda() for n in ("p", "m", "v")} for t in case]
    for e, t in zip(dev, case):
        e["g"] = torch.empty(t["p"].shape, device="cuda")
    state = torch.tensor([0.0, 1.0, 1.0], dtype=torch.float64, device="cuda")
    total = torch.zeros(1, device="cuda")
    ws = torch.empty(be.fused_adam_workspace([t["p"].size for t in case]), dtype=torch.uint8, device="cuda")
    ref = [{n: t[n].astype(np.float64) for n in ("p", "m", "v")} for t in case]
    ref_state, norms = R.new_state(), []
    for gs in grads:
        for e, r, g in zip(dev, ref, gs):
            e["g"].copy_(torch.from_numpy(g))
            r["g"] = g.astype(np.float64)
        be.fused_adam(dev, state, ws, LR, BETA1, BETA2, EPS, max_grad_norm=0.5, total_norm=total)
        norms.append((float(total[0]), float(R.step(ref, ref_state, LR, BETA1, BETA2, EPS, 0.5, dtype=np.float64))))
    want, _ = _torch_reference(case, grads, 0.5)
    pairs = [(k, float(np.abs(e["p"].cpu().numpy() - r["p"]).max()), float(np.abs(w - r["p"]).max())) for k, (e, r, w) in enumerate(zip(dev, ref, want))]
    _pairs = {"pairs": pairs, "norms": norms}
    return _pairs


def test_total_norm_is_within_one_ulp_of_the_float64_value():
    for mine, exact in tolerance_pairs()["norms"]:
        print(f"total_norm {mine!r} float64 {exact!r}")
        assert abs(mine - exact) <= float(np.spacing(np.float32(exact)))


def test_parameters_are_as_close_to_float64_as_torch_float32():
    for k, e_kernel, e_torch in tolerance_pairs()["pairs"]:
        print(f"tensor {k}: e_kernel {e_kernel:.3e} e_torch {e_torch:.3e}")
        assert e_kernel <= M_FACTOR * e_torch + FLOOR, (k, e_kernel, e_torch)


# ---- captured graphs -------------------------------------------------------------------------------------------------------------------
def _snapshot(opt, params, extra=()):
    return [p.detach().clone() for p in params] + [x.clone() for x in opt.exp_avg + opt.exp_avg_sq + [opt.state] + list(extra)]


def _equal_bits(a, b):
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and torch.equal(x.view(torch.uint8), y.view(torch.uint8))


def test_a_captured_step_replays_like_eager_steps_and_follows_a_device_lr():
    from pde_control_gym import FusedAdam
    shapes = [(65, 64), (64,), (1, 64), (1,)]
    torch.manual_seed(1)
    start = [torch.randn(s, device="cuda") for s in shapes]
    grads = [[torch.randn(s, device="cuda") for s in shapes] for _ in range(3)]
    lrs = (1e-3, 5e-4, 2e-3)
    results = []
    for captured in (False, True):
        params = [torch.nn.Parameter(x.clone()) for x in start]
        lr = torch.tensor(lrs[0], device="cuda")
        opt = FusedAdam(params, lr=lr, eps=EPS, max_grad_norm=0.5)
        for p in params:
            p.grad = torch.zeros_like(p)
        if captured:
            sd = opt.state_dict()
            for p, g in zip(params, grads[0]):
                p.grad.copy_(g)
            opt.step()                                  # warm-up: the workspace and the descriptor exist from here on
            opt.load_state_dict(sd)
            with torch.no_grad():
                for p, x in zip(params, start):
                    p.copy_(x)
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                opt.step()
        for gs, value in zip(grads, lrs):
            lr.fill_(value)
            for p, g in zip(params, gs):
                p.grad.copy_(g)
            graph.replay() if captured else opt.step()
        torch.cuda.synchronize()
        results.append(_snapshot(opt, params, [opt.total_norm.reshape(1)]))
        assert float(opt.state[0]) == 3.0
    _equal_bits(*results)
    # the device lr was followed: the same run with the first lr throughout ends elsewhere
    params = [torch.nn.Parameter(x.clone()) for x in start]
    opt = FusedAdam(params, lr=lrs[0], eps=EPS, max_grad_norm=0.5)
    for gs in grads:
        for p, g in zip(params, gs):
            p.grad = g.clone()
        opt.step()
    assert not torch.equal(params[0].detach(), results[0][0])


@pytest.mark.parametrize("sizes,act", [((65, 64, 64, 1), "Tanh"), ((66, 256, 256, 1), "ReLU")])
def test_a_captured_update_replays_like_eager_iterations(sizes, act):
    """with_grad forward of an attached network, a sum-of-squares loss, backward() and step() in ONE torch.cuda.graph: three replays
    equal three eager iterations bit for bit in parameters, moments and weight copies; an unattached wrapper still refuses."""
    import copy
    from pde_control_gym import FusedAdam, FusedMLP
    torch.manual_seed(sizes[1])
    mods = []
    for i in range(len(sizes) - 1):
        mods += [torch.nn.Linear(sizes[i], sizes[i + 1]), getattr(torch.nn, act)()]
    proto = torch.nn.Sequential(*mods[:-1]).cuda()
    xs = [torch.randn(64, sizes[0], device="cuda") for _ in range(3)]
    x = torch.empty(64, sizes[0], device="cuda")
    results = []

    def iteration(f, opt):
        y = f.with_grad(x)
        (y * y).sum().backward()
        opt.step()

    for captured in (False, True):
        net = copy.deepcopy(proto)
        params = list(net.parameters())
        f = FusedMLP(net)
        opt = FusedAdam(params, lr=1e-3, max_grad_norm=0.5).attach(f)
        if captured:
            sd = opt.state_dict()
            x.copy_(xs[0])
            iteration(f, opt)                           # warm-up
            opt.load_state_dict(sd)
            net.load_state_dict(proto.state_dict())
            f.refresh()                                 # (load_state_dict went behind the optimiser's back)
            opt.zero_grad(set_to_none=True)
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                iteration(f, opt)
        for xk in xs:
            x.copy_(xk)
            if captured:
                graph.replay()
            else:
                opt.zero_grad(set_to_none=True)
                iteration(f, opt)
        torch.cuda.synchronize()
        results.append(_snapshot(opt, params, f._wt))
        fresh = FusedMLP(net)
        for a, b in zip(f._wt, fresh._wt):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    _equal_bits(*results)
    assert not torch.equal(results[0][0], proto[0].weight.detach())
    other = FusedMLP(copy.deepcopy(proto))                # not attached to any optimiser
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    keep = torch.zeros(4, device="cuda")
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            keep.add_(1.0)
            with pytest.raises(RuntimeError, match="stream capture: refresh\\(\\) has to see the optimiser's last step"):
                other.with_grad(x)


# ---- both examples ------------------------------------------------------------------------------------------------------------------------
def _example(name):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    try:
        spec = importlib.util.spec_from_file_location(name + "_fused_opt", os.path.join(ROOT, "examples", name + ".py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        sys.path.pop(0)
    return mod


@pytest.mark.parametrize("hidden", [64, 256])
def test_sac_example_runs_with_fused_opt(hidden):
    hist = _example("train_sac_device").main(iterations=2, num_envs=64, n_steps=8, hidden=hidden, quiet=True, updates=2, batch=256,
                                             fused_grad=True, fused_loss=True, fused_opt=True)
    for k in ("q_loss", "actor_loss", "alpha", "mean_reward"):
        assert len(hist[k]) == 2 and np.isfinite(hist[k]).all(), k
    assert hist["moved"] == {"actor": True, "q1": True, "q2": True}


@pytest.mark.parametrize("hidden", [64, 256])
def test_ppo_example_runs_with_fused_opt(hidden):
    hist = _example("train_ppo_device").main(iterations=2, B=64, quiet=True, hidden=hidden, fused_grad=True, fused_loss=True, fused_opt=True)
    assert len(hist) == 2 and hist[-1].pop("moved") == {"actor": True, "critic": True}
    assert all(np.isfinite(list(h.values())).all() for h in hist)


def test_ppo_example_graph_update_replays_the_fused_step():
    """One captured minibatch step replayed for the rest of the run: the same kernels in the same order as ``fused_opt`` alone, so the
    same figures."""
    mod = _example("train_ppo_device")
    kw = dict(iterations=2, B=64, quiet=True, hidden=64, fused_grad=True, fused_loss=True, fused_opt=True)
    eager, graphed = mod.main(**kw), mod.main(graph_update=True, **kw)
    assert graphed[-1]["moved"] == {"actor": True, "critic": True}
    for a, b in zip(eager, graphed):
        assert a == b, (a, b)
    with pytest.raises(ValueError, match="graph_update needs"):
        mod.main(iterations=1, B=64, quiet=True, graph_update=True)
