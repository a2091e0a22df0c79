"""The squashed-Gaussian (SAC) actor head on the device: pdegym_mlp_forward's epilogue and the two evaluators inside the rollout
kernels (csrc/pdegym_mlp_tile.h: ``squashed_gaussian``, the one copy of the arithmetic; csrc/pdegym_policy.h: ``shaped_gaussian``).

(a), (b): exactly summable networks (tests/gaussian_exact.py; tests/test_gaussian_exact_helper.py checks every case on the CPU) against
the float64 expectation, at ``rtol = TANH_RTOL, atol = (TANH_ATOL + 2**-19) * half_width`` -- 2**-19 derived there from an expf within
2 ulp and the roundings of the product and the sum.  The pre-activations are exact and the head is one shared function, so both
evaluators inside the rollout kernels must return pdegym_mlp_forward's BITS on the same rows.  (c) DeviceRollout: one launch against
policy launch + step launch per env-step, in a hipGraph and eagerly.  (d) a random 257-256-256-(1+1) ReLU actor against the torch
float32 restatement.  (e) non-finite inputs.  (f) batch invariance.  (g) the SAC example."""
import os
import sys

import numpy as np
import pytest

from tests import gaussian_exact as gx
from tests import nonfinite as nf
from tests import poison

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

F32, F64, U8 = torch.float32, torch.float64, torch.uint8
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _close(case, got, want, what):
    rtol, atol = gx.tolerance(case.box)
    got = np.asarray(got, np.float64).reshape(want.shape)
    err = np.abs(got - want) - rtol * np.abs(want)
    print(f"{case.name}: {what}: worst |got - want| - rtol |want| = {err.max():.3e} (atol {atol:.3e})")
    np.testing.assert_allclose(got, want, rtol=rtol, atol=atol, err_msg=f"{case.name}: {what}")
    assert (got >= case.box[0]).all() and (got <= case.box[1]).all(), "a command outside the action box"


# ---- (a) pdegym_mlp_forward ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", gx.FORWARD_CASES, ids=[c.name for c in gx.FORWARD_CASES])
def test_forward_kernel_against_the_float64_expectation(case, policy=None):
    """Every buffer in a guarded allocation; with ``gaps`` the rows sit in wider, poisoned rows.  Only the A columns of y are written.
    ``policy`` displaces every guarded buffer off its 256-byte boundary (tests/poison.py; tests/test_gpu_pointer_alignment.py)."""
    b = gx.build(case)
    B, K, A = case.B, case.sizes[0], case.A
    gx_, gy, gn = (5, 3, 2) if case.gaps else (0, 0, 0)
    arena = poison.Arena("cuda", policy=policy)
    xbig = poison.poison_(arena.new("x", (B, K + gx_), F64 if case.x_f64 else F32))
    ybig = poison.poison_(arena.new("y", (B, A + gy), F64 if case.y_f64 else F32))
    xbig[:, :K] = torch.from_numpy(b.x_dev)
    nbig = None
    if b.eps is not None:
        nbig = poison.poison_(arena.new("eps", (B, A + gn), F32))
        nbig[:, :A] = torch.from_numpy(b.eps)
    pol = gx.policy(b, case, "cuda")
    x, y = xbig[:, :K], ybig[:, :A]
    pol.forward_into(x, y, clamp=case.box, noise=None if nbig is None else nbig[:, :A])
    torch.cuda.synchronize()
    arena.check()
    poison.assert_written(ybig, (slice(None), slice(0, A)), "y")
    if case.gaps:
        poison.assert_untouched(ybig, (slice(None), slice(A, None)), "the gap of the output rows")
        poison.assert_untouched(xbig, (slice(None), slice(K, None)), "the gap of the input rows")
        if nbig is not None:
            poison.assert_untouched(nbig, (slice(None), slice(A, None)), "the gap of the eps rows")
    assert np.array_equal(xbig[:, :K].cpu().numpy(), b.x_dev), "the input rows were changed"
    _close(case, y.cpu().numpy(), b.want, "y")


def test_forward_kernel_refuses_what_the_header_says():
    from pdecontrolgym_amd import _native as N
    from pdecontrolgym_amd.policy import FusedMLP

    def pol(A, **kw):
        return FusedMLP.squashed_gaussian(torch.nn.Sequential(torch.nn.Linear(6, 16), torch.nn.ReLU()).cuda(),
                                          torch.nn.Linear(16, A).cuda(), torch.nn.Linear(16, A).cuda(), **kw)
    x = torch.zeros(3, 6, device="cuda")
    y = poison.poison_(torch.empty(3, 9, device="cuda"))
    with pytest.raises(N.NativeError, match="at most 8 actions"):
        pol(9).forward_into(x, y, clamp=(-1.0, 1.0))
    poison.assert_untouched(y, None, "y")
    p = pol(2)
    y2 = torch.empty(3, 2, device="cuda")

    def call(**fields):
        net = p._net((-1.0, 1.0))
        for k, v in fields.items():
            setattr(net, k, v)
        p.backend.mlp_forward(net, x, y2, 3)
    for fields, why in ((dict(clamp=0), "clamp must be set"), (dict(lo=1.0, hi=1.0), "lo < hi"), (dict(log_std_min=1.0, log_std_max=0.0), "log_std_min <= log_std_max"),
                        (dict(log_std_min=float("nan")), "log_std_min <= log_std_max"), (dict(head=2), "unknown head")):
        with pytest.raises(N.NativeError, match=why):
            call(**fields)
    net = p._net((-1.0, 1.0))
    net.layer[1].act = N.MLP_TANH
    with pytest.raises(N.NativeError, match="IDENTITY"):
        p.backend.mlp_forward(net, x, y2, 3)
    call()                                               # ... and the untouched descriptor is accepted
    torch.cuda.synchronize()


# ---- (b) the evaluators inside the rollout kernels --------------------------------------------------------------------------------------
def _eps_buffer(b, T, B, A, three):
    if b.eps is None:
        return None
    nz = torch.zeros((T, B, A) if three else (T, B), dtype=F32, device="cuda")
    nz[0] = torch.from_numpy(b.eps).cuda().reshape(nz[0].shape)
    return nz


def _rollout(case, b):
    """actions[0] of a rollout of T = 2 steps from an observation slot 0 that holds the case's rows; the action buffer poisoned."""
    from tests.test_gpu_mlp_exact import _env_1d, _env_tumor
    B, T, A = case.B, 2, case.A
    pol = gx.policy(b, case, "cuda")
    z = lambda dt: torch.zeros(T, B, dtype=dt, device="cuda")      # noqa: E731
    if case.env[0] == "1d":
        _, kind, control, loc, n = case.env
        core = _env_1d(kind, control, loc, n, B).core
        assert core.obs_dim == case.sizes[0] and core.policy_fits_rollout(pol)
        rows, dt = torch.from_numpy(b.x.astype(np.float32)).cuda(), F32
        obs = torch.zeros(T + 1, B, core.obs_dim, dtype=F32, device="cuda")
        act = poison.poison_(torch.empty(T, B, dtype=F32, device="cuda"))
        nz = _eps_buffer(b, T, B, A, False)
        obs[0] = rows
        core.rollout(obs, act, z(F32), z(U8), z(U8), policy=pol, clamp=case.box, noise=nz)
    elif case.env[0] == "traffic":
        from pdecontrolgym_amd.batch_traffic import TrafficBatch
        env = TrafficBatch(240, 0.25, 500, 10, case.env[1], 40, 0.16, 60, True, 2, num_envs=B, device="cuda")
        rs = np.full(B, 0.12)
        env.set_action_bounds(rs * (40 * (1 - rs / 0.16)))
        env.reset(rs)
        assert env.action_dim == A and 2 * env.M == case.sizes[0] and env.policy_fits_rollout(pol)
        rows, dt = torch.from_numpy(b.x_dev).cuda(), F64
        obs = torch.zeros(T + 1, B, 2 * env.M, dtype=F64, device="cuda")
        act = poison.poison_(torch.empty(T, B, A, dtype=F64, device="cuda"))
        nz = _eps_buffer(b, T, B, A, True)
        obs[0] = rows
        env.rollout(obs, act, z(F64), z(U8), z(U8), policy=pol, clamp=case.box, noise=nz)
    else:
        nx = case.env[1]
        venv = _env_tumor(nx, B)
        assert venv.core.policy_fits_rollout(pol)
        rows, dt = torch.from_numpy(b.x_dev).cuda(), F64
        obs = torch.zeros(T + 1, B, nx, dtype=F64, device="cuda")
        act = poison.poison_(torch.empty(T, B, dtype=F64, device="cuda"))
        nz = _eps_buffer(b, T, B, A, False)
        obs[0] = rows
        venv.core.rollout(obs, act, z(F64), z(U8), z(U8), policy=pol, clamp=case.box, noise=nz, wrap_state=dict(venv._wrapper_state()))
    torch.cuda.synchronize()
    poison.assert_written(act, None, "actions")
    assert torch.equal(obs[0], rows), "observation slot 0 was changed"
    return pol, rows, None if nz is None else nz[0].reshape(B, A), act[0].reshape(B, A), dt


@pytest.mark.parametrize("case", gx.ROLLOUT_CASES, ids=[c.name for c in gx.ROLLOUT_CASES])
def test_evaluators_inside_the_rollout_kernels(case):
    """actions[0] against the float64 expectation, and bit for bit against pdegym_mlp_forward on the same rows -- for the cooperative
    evaluation (same reduction) and for the neuron-per-lane one as well (exact pre-activations, one shared head function)."""
    b = gx.build(case)
    pol, rows, eps0, got, dt = _rollout(case, b)
    assert got.dtype == dt
    _close(case, got.cpu().numpy(), b.want, "actions[0]")
    fwd = torch.empty(case.B, case.A, dtype=dt, device="cuda")
    pol.forward_into(rows.clone(), fwd, clamp=case.box, noise=eps0)
    assert torch.equal(poison.bits(got.contiguous()), poison.bits(fwd)), "the evaluator inside the rollout kernel differs from pdegym_mlp_forward"


# ---- (c) DeviceRollout: one launch == policy launch + step launch per env-step ---------------------------------------------------------
def _actor(n_in, hidden, A, seed, first_scale=0.3, ls_bias=-1.0):
    torch.manual_seed(seed)
    mods, k = [], n_in
    for h in hidden:
        mods += [torch.nn.Linear(k, h), torch.nn.ReLU()]
        k = h
    mu, ls = torch.nn.Linear(k, A), torch.nn.Linear(k, A)
    with torch.no_grad():
        mods[0].weight.mul_(first_scale)
        ls.bias.fill_(ls_bias)
    return torch.nn.Sequential(*mods).cuda(), mu.cuda(), ls.cuda()


def _family(name, B):
    """(venv, inputs, A, box, scale of the first layer, state tensors of the engine)"""
    import pde_control_gym
    if name == "1d":
        from tests.test_policy import _rd_env
        venv = _rd_env(B, 64, 5, horizon=4)
        return venv, 65, 1, (-2.0, 2.0), 0.3, ("obs", "time_index")
    if name == "traffic":
        import random
        from pde_control_gym.src import TrafficARZReward
        from tests.test_traffic import BASE
        random.seed(0)
        venv = pde_control_gym.make_vec("PDEControlGym-TrafficPDE1D", num_envs=B, reward_class=TrafficARZReward(), simulation_type="both",
                                        limit_pde_state_size=True, control_freq=2, **dict(BASE, T=0.25))      # (episodes of four env-steps)
        venv.reset_tensor()
        venv.enable_fused_auto_reset()
        return venv, 102, 2, (3.0, 6.0), 0.3, ("obs", "time", "r", "y")
    from tests.test_gpu_tumor_rollout import ENGINE_KEYS, _venv
    return _venv(201, 600, True, num_envs=B), 201, 1, (0.0, 1.0), 1e-5, ENGINE_KEYS


@pytest.mark.parametrize("hidden", [(48,), (128, 65)], ids=["narrow", "wide"])
@pytest.mark.parametrize("family", ["1d", "traffic", "tumor"])
def test_device_rollout_one_launch_equals_the_launches_per_step(family, hidden):
    """B = 17, T = 6, episodes end and restart inside the rollout.  one_launch=True against one_launch=False in a hipGraph and against
    the eager loop: every buffer and the engine state bit-identical for the wide policy; for the narrow one (another summation order
    in front of the head) the first commands agree at the policy tolerance and the trajectories follow (tests/test_policy.py's bounds)."""
    from pde_control_gym import DeviceRollout
    from pdecontrolgym_amd.policy import FusedMLP
    B, T = 17, 6
    runs = {}
    for mode, (one_launch, graph) in {"one": (True, True), "graph": (False, True), "eager": (False, False)}.items():
        venv, n_in, A, box, scale, keys = _family(family, B)
        lat, mu, ls = _actor(n_in, hidden, A, seed=21, first_scale=scale)
        if family == "tumor":
            with torch.no_grad():
                mu.bias.fill_(1.0)          # doses in the upper half of the box: episodes end within the six steps
        pol = FusedMLP.squashed_gaussian(lat, mu, ls)
        ro = DeviceRollout(venv, pol, T, use_graph=graph, action_low=box[0], action_high=box[1], action_noise=True, one_launch=one_launch)
        assert ro.one_launch is one_launch
        ro.action_noise.copy_(torch.randn(ro.action_noise.shape, generator=torch.Generator().manual_seed(5)).cuda())
        ro.run()
        torch.cuda.synchronize()
        runs[mode] = {k: getattr(ro, k).clone() for k in ("actions", "obs", "rewards", "terminated", "truncated")}
        runs[mode].update({"state_" + k: venv.core.t[k].clone() for k in keys})
    one = runs["one"]
    assert bool((one["terminated"] | one["truncated"]).any()), "no episode ended inside the rollout"
    acts = one["actions"]
    assert float(acts.min()) >= box[0] and float(acts.max()) <= box[1] and float(acts.std()) > 0
    for k in one:      # the hipGraph of the step loop replays what the eager loop computes
        assert torch.equal(poison.bits(runs["graph"][k]), poison.bits(runs["eager"][k])), k
    half = 0.5 * (box[1] - box[0])
    for other in ("graph", "eager"):
        for k, v in one.items():
            w = runs[other][k]
            if len(hidden) == 2:
                assert torch.equal(poison.bits(v), poison.bits(w)), f"{k} against {other}"
            elif k == "actions":
                np.testing.assert_allclose(v[0].cpu().numpy(), w[0].cpu().numpy(), rtol=2e-5, atol=4e-6 * half, err_msg="actions[0]")
            elif family != "tumor":      # (a patient's last day depends on the doses: compared through the wide policy only)
                if v.dtype in (U8, torch.int32, torch.int64, torch.bool):
                    assert torch.equal(v, w), f"{k} against {other}"
                elif k in ("obs", "rewards"):
                    np.testing.assert_allclose(v.cpu().numpy(), w.cpu().numpy(), rtol=1e-4, atol=2e-5, err_msg=f"{k} against {other}")


# ---- (d) a random actor against the torch float32 restatement ----------------------------------------------------------------------------
def test_random_256_256_actor_against_the_torch_restatement():
    """257-256-256-(1 + 1) ReLU, sigma <= 1 (log_std clipped to [-20, 0] by a bias that keeps it negative), |eps| <= 3: the project's policy
    tolerance, rtol 2e-5 and atol 4e-6 times the half width."""
    from pdecontrolgym_amd.policy import FusedMLP
    from tests.test_gaussian_head import restatement
    lat, mu, ls = _actor(257, (256, 256), 1, seed=8, first_scale=1.0)
    B, box = 333, (-3.0, 5.0)
    g = torch.Generator().manual_seed(9)
    x = torch.randn(B, 257, generator=g).cuda()
    eps = torch.randn(B, 1, generator=g).clamp(-3.0, 3.0).cuda()
    with torch.no_grad():
        ls.bias.sub_(ls(lat(x)).max().clamp(min=0.0) + 0.1)                 # log_std < 0 on these rows: sigma <= 1
        assert float(ls(lat(x)).max()) < 0
    pol = FusedMLP.squashed_gaussian(lat, mu, ls)
    for noise in (eps, None):
        got = pol.forward_into(x, torch.empty(B, 1, device="cuda"), clamp=box, noise=noise)
        want = restatement(lat, mu, ls, x, noise, (-20.0, 2.0), box)
        np.testing.assert_allclose(got.cpu().numpy(), want.cpu().numpy(), rtol=2e-5, atol=4e-6 * 4.0)
        assert float(got.std()) > 0.1


# ---- (e) non-finite inputs -----------------------------------------------------------------------------------------------------------
def _nf_policy(A=1, hidden=(16,)):
    from pdecontrolgym_amd.policy import FusedMLP
    lat, mu, ls = _actor(30, hidden, A, seed=2)
    return FusedMLP.squashed_gaussian(lat, mu, ls), lat, mu, ls


@pytest.mark.parametrize("hidden", [(16,), (80,)], ids=["narrow", "wide"])
def test_non_finite_inputs_follow_the_header_in_every_evaluator(hidden):
    """NaN / +-Inf planted in the observation, in eps and in each head's bias: a NaN in mu, log_std or eps gives a NaN command,
    mu = +-Inf gives hi / lo (a dyadic box), log_std = +-Inf is clipped, and no other row changes a bit (no fault either).  The same
    rows through pdegym_mlp_forward and through the transport rollout kernel."""
    from tests.test_gpu_mlp_exact import _env_1d
    B, box = 19, (-1.0, 3.0)      # (an engine of its own: 19 instances)
    pol, lat, mu, ls = _nf_policy(hidden=hidden)
    g = torch.Generator().manual_seed(3)
    x0 = torch.randn(B, 30, generator=g).cuda()
    eps0 = torch.randn(B, 1, generator=g).cuda()
    core = _env_1d("PDEControlGym-TransportPDE1D", "Dirchilet", "full", 30, B).core

    def both(x, eps):
        fwd = pol.forward_into(x, torch.empty(B, 1, device="cuda"), clamp=box, noise=eps)
        obs = torch.zeros(3, B, 30, device="cuda")
        obs[0] = x
        act = poison.poison_(torch.empty(2, B, device="cuda"))
        nz = None
        if eps is not None:
            nz = torch.zeros(2, B, device="cuda")
            nz[0] = eps[:, 0]
        z = lambda dt: torch.zeros(2, B, dtype=dt, device="cuda")      # noqa: E731
        core.rollout(obs, act, z(F32), z(U8), z(U8), policy=pol, clamp=box, noise=nz)
        torch.cuda.synchronize()
        if len(hidden) == 1 and hidden[0] > 64:
            nf.same_bits_and_nans(act[0], fwd[:, 0], "rollout kernel against pdegym_mlp_forward")
        return fwd[:, 0].cpu().numpy(), act[0].cpu().numpy()
    clean = both(x0, eps0)
    assert all(np.isfinite(c).all() for c in clean)
    # the observation: a NaN reaches mu through the network (ReLU keeps it); +-Inf times a weight is +-Inf or NaN -- never a fault
    for plant in nf.PLANTS.values():
        x = x0.clone()
        x[3, 7] = plant
        for got, ref in zip(both(x, eps0), clean):
            rows = np.arange(B) != 3
            assert np.array_equal(got[rows].view(np.uint32), ref[rows].view(np.uint32)), "a non-finite observation changed another row"
            assert np.isnan(got[3]) or box[0] <= got[3] <= box[1]
        if plant != plant:
            assert all(np.isnan(got[3]) for got in both(x, eps0))
    # eps
    for plant, want in ((nf.NAN, np.nan), (nf.PINF, box[1]), (nf.NINF, box[0])):
        e = eps0.clone()
        e[5, 0] = plant
        for got, ref in zip(both(x0, e), clean):
            rows = np.arange(B) != 5
            assert np.array_equal(got[rows].view(np.uint32), ref[rows].view(np.uint32))
            assert (np.isnan(got[5]) if want != want else got[5] == np.float32(want)), (plant, got[5])
    # the heads' biases: every row sees them
    for head, plant, check in ((mu, nf.NAN, lambda c: np.isnan(c).all()), (mu, nf.PINF, lambda c: (c == np.float32(box[1])).all()),
                               (mu, nf.NINF, lambda c: (c == np.float32(box[0])).all()), (ls, nf.NAN, lambda c: np.isnan(c).all()),
                               (ls, nf.PINF, lambda c: np.isfinite(c).all()), (ls, nf.NINF, lambda c: np.isfinite(c).all())):
        keep = head.bias.detach().clone()
        with torch.no_grad():
            head.bias.fill_(plant)
        pol.refresh()
        for got in both(x0, eps0):
            assert check(got), (("mu" if head is mu else "log_std"), plant, got[:4])
        if head is ls:      # without noise log_std is not looked at: the deterministic actor stays what it was
            with torch.no_grad():
                head.bias.copy_(keep)
            pol.refresh()
            det_clean = both(x0, None)
            with torch.no_grad():
                head.bias.fill_(plant)
            pol.refresh()
            for got, ref in zip(both(x0, None), det_clean):
                assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
        with torch.no_grad():
            head.bias.copy_(keep)
        pol.refresh()
    for got, ref in zip(both(x0, eps0), clean):
        assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))


# ---- (f) batch invariance -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A,hidden", [(1, (64,)), (2, (256, 256)), (8, (65,))])
def test_a_rows_command_does_not_depend_on_the_batch(A, hidden):
    from pdecontrolgym_amd.policy import FusedMLP
    lat, mu, ls = _actor(70, hidden, A, seed=4)
    pol = FusedMLP.squashed_gaussian(lat, mu, ls)
    g = torch.Generator().manual_seed(1)
    x, eps = torch.randn(33, 70, generator=g).cuda(), torch.randn(33, A, generator=g).cuda()
    full = pol.forward_into(x, torch.empty(33, A, device="cuda"), clamp=(-1.0, 3.0), noise=eps)
    for B in (1, 17):
        part = pol.forward_into(x[:B].clone(), torch.empty(B, A, device="cuda"), clamp=(-1.0, 3.0), noise=eps[:B].clone())
        assert torch.equal(poison.bits(part), poison.bits(full[:B])), f"B = {B}"
    assert float(full.std()) > 0


# ---- (g) the example ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("one_launch", [True, False])
def test_sac_example_smoke(one_launch):
    """examples/train_sac_device.py, two iterations: finite losses, and the parameters of the actor and of both critics moved.  A smoke
    test, not a learning claim."""
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    try:
        import train_sac_device
    finally:
        sys.path.pop(0)
    hist = train_sac_device.main(iterations=2, num_envs=64, n_steps=8, hidden=64, one_launch=one_launch, quiet=True)
    assert len(hist["q_loss"]) == 2 and len(hist["mean_reward"]) == 2
    for k in ("q_loss", "actor_loss", "alpha", "mean_reward"):
        assert np.isfinite(hist[k]).all(), k
    assert hist["moved"] == {"actor": True, "q1": True, "q2": True}
