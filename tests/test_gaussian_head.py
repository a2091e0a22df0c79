"""The squashed-Gaussian (SAC) actor head on the host side (CPU): the descriptor ``FusedMLP.squashed_gaussian`` builds, ``refresh()``
over the four parameter tensors of the two heads, the refusals, ``from_sb3(stochastic=True)``, and ``DeviceRollout`` -- step loop and
one rollout call -- on the CPU doubles of tests/fake_gaussian_backend.py against a step-by-step torch restatement of

    a = tanh(mu(s) + exp(clip(log_std(s), min, max)) * eps),    command = lo + 0.5 (a + 1) (hi - lo)

for a 1D, a two-command traffic and a brain-tumour environment.  The kernels themselves: tests/test_gpu_gaussian_head.py."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest

from pdecontrolgym_amd import _native as N
from pdecontrolgym_amd.policy import FusedMLP
from tests.fake_gaussian_backend import FakeGaussianBackend, FakeGaussianTumorBackend, gaussian_head

torch = pytest.importorskip("torch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL, ATOL = 2e-5, 4e-6          # the policy tolerance of tests/test_policy.py (atol times the box's half width)


def _actor(n_in, hidden, A, seed=0, act=torch.nn.ReLU, ls_bias=-1.0):
    torch.manual_seed(seed)
    mods, k = [], n_in
    for h in hidden:
        mods += [torch.nn.Linear(k, h), act()]
        k = h
    mu, ls = torch.nn.Linear(k, A), torch.nn.Linear(k, A)
    with torch.no_grad():
        ls.bias.fill_(ls_bias)
    return torch.nn.Sequential(*mods), mu, ls


def restatement(latent, mu, log_std, obs, eps, bounds, box):
    """SB3's sequence of torch ops in float32 on observation rows ``obs`` (any dtype: rounded to float32 first)."""
    lo, hi = box
    with torch.no_grad():
        h = latent(obs.float())
        z = mu(h)
        if eps is not None:
            z = z + log_std(h).clamp(bounds[0], bounds[1]).exp() * eps
        return (lo + (0.5 * (torch.tanh(z) + 1.0)) * (hi - lo)).clamp(lo, hi)


def _blocked(w):
    out_dim, in_dim = w.shape
    k4 = (in_dim + 3) // 4
    return torch.nn.functional.pad(w, (0, 4 * k4 - in_dim)).view(out_dim, k4, 4).permute(1, 0, 2).contiguous()


# ---- the descriptor ---------------------------------------------------------------------------------------------------------------
def test_versions_and_struct_layout():
    hdr = open(os.path.join(ROOT, "include", "pdegym.h")).read()
    assert N.ABI_VERSION == 21 and "#define PDEGYM_ABI_VERSION 21" in hdr
    assert "enum { PDEGYM_MLP_HEAD_PLAIN = 0, PDEGYM_MLP_HEAD_SQUASHED_GAUSSIAN = 1 };" in hdr
    assert (N.MLP_HEAD_PLAIN, N.MLP_HEAD_SQUASHED_GAUSSIAN) == (0, 1)
    # the new fields sit in the reserved words of layer[0 .. 2]: size and every offset of ABI 20 are what they were, and a
    # zero-initialised descriptor is the plain head
    assert C.sizeof(N.Mlp) == 40 + 4 * 32 and N.Mlp.layer.offset == 40 and N.MlpLayer.reserved_.offset == 28
    assert (N.Mlp.head.offset, N.Mlp.log_std_min.offset, N.Mlp.log_std_max.offset) == (40 + 28, 40 + 32 + 28, 40 + 64 + 28)
    net = N.Mlp()
    assert net.head == N.MLP_HEAD_PLAIN
    net.head, net.log_std_min, net.log_std_max = 1, -20.0, 2.0
    for i in range(4):      # ... and the layers' own fields are untouched by them
        L = net.layer[i]
        assert (L.w, L.b, L.in_dim, L.out_dim, L.act) == (None, None, 0, 0, 0)
    assert net.layer[0].reserved_ == 1 and net.layer[3].reserved_ == 0
    body = hdr[hdr.index("typedef struct pdegym_mlp_s {"):hdr.index("} pdegym_mlp;")]
    assert re.search(r"char in_layer0_\[28\];\s+int32_t head;", body) and re.search(r"char in_layer1_\[28\];\s+float log_std_min;", body)
    assert re.search(r"char in_layer2_\[28\];\s+float log_std_max;", body)


def test_descriptor_of_squashed_gaussian():
    lat, mu, ls = _actor(9, (16, 12), 2)
    pol = FusedMLP.squashed_gaussian(lat, mu, ls, log_std_bounds=(-5.0, 1.5), backend=object())
    assert pol.in_dim == 9 and pol.out_dim == 2 and pol.head == N.MLP_HEAD_SQUASHED_GAUSSIAN and pol.log_std_bounds == (-5.0, 1.5)
    net = pol._net((-1.0, 3.0))
    assert net.head == 1 and net.log_std_min == -5.0 and net.log_std_max == 1.5 and net.clamp == 1 and (net.lo, net.hi) == (-1.0, 3.0)
    assert net.n_layers == 3 and [net.layer[i].out_dim for i in range(3)] == [16, 12, 4] and net.layer[2].in_dim == 12
    assert [net.layer[i].act for i in range(3)] == [N.MLP_RELU, N.MLP_RELU, N.MLP_IDENTITY]
    # the last layer: rows [mu; log_std] in the blocked transpose, its bias one concatenated buffer of the wrapper's
    assert torch.equal(pol._wt[2], _blocked(torch.cat([mu.weight, ls.weight]).detach()))
    bias = np.ctypeslib.as_array(C.cast(net.layer[2].b, C.POINTER(C.c_float)), (4,))
    np.testing.assert_array_equal(bias, torch.cat([mu.bias, ls.bias]).detach().numpy())
    assert net.layer[2].b not in (mu.bias.data_ptr(), ls.bias.data_ptr())
    assert net.layer[0].b == lat[0].bias.data_ptr()                      # the latent layers point at the parameters themselves
    # no latent layers, no biases, the default bounds (SB3's LOG_STD_MIN / LOG_STD_MAX)
    m2, l2 = torch.nn.Linear(7, 1, bias=False), torch.nn.Linear(7, 1, bias=False)
    p2 = FusedMLP.squashed_gaussian([], m2, l2, backend=object())
    n2 = p2._net((0.0, 1.0))
    assert n2.n_layers == 1 and n2.layer[0].out_dim == 2 and not n2.layer[0].b and (n2.log_std_min, n2.log_std_max) == (-20.0, 2.0)
    # the plain head's descriptor is what it was
    plain = FusedMLP(torch.nn.Sequential(torch.nn.Linear(4, 3)), backend=object())._net(None)
    assert plain.head == 0 and plain.log_std_min == 0 and plain.log_std_max == 0


@pytest.mark.parametrize("which", ["mu.weight", "mu.bias", "log_std.weight", "log_std.bias"])
def test_refresh_sees_an_in_place_update_of_each_head_tensor(which):
    lat, mu, ls = _actor(6, (8,), 2, seed=1)
    pol = FusedMLP.squashed_gaussian(lat, mu, ls, backend=FakeGaussianBackend())
    net = pol._net((-1.0, 1.0))
    ptrs = (net.layer[1].w, net.layer[1].b)
    x, eps = torch.randn(5, 6), torch.randn(5, 2)
    before = pol.forward_into(x, torch.empty(5, 2), clamp=(-1.0, 1.0), noise=eps).clone()
    mod, name = which.split(".")
    with torch.no_grad():
        getattr({"mu": mu, "log_std": ls}[mod], name).add_(0.25)
    after = pol.forward_into(x, torch.empty(5, 2), clamp=(-1.0, 1.0), noise=eps)
    assert not torch.equal(before, after)
    np.testing.assert_allclose(after.numpy(), restatement(lat, mu, ls, x, eps, (-20.0, 2.0), (-1.0, 1.0)).numpy(), rtol=RTOL, atol=ATOL)
    net = pol._net((-1.0, 1.0))
    assert (net.layer[1].w, net.layer[1].b) == ptrs                     # rewritten in place: a captured graph sees the update
    assert torch.equal(pol._wt[1], _blocked(torch.cat([mu.weight, ls.weight]).detach()))
    seen = pol._heads_seen
    pol.refresh()
    assert pol._heads_seen == seen                                      # nothing changed: nothing rewritten


def test_refusals():
    lat, mu, ls = _actor(6, (8,), 2)
    bk = FakeGaussianBackend()
    with pytest.raises(ValueError, match="equal shapes"):
        FusedMLP.squashed_gaussian(lat, mu, torch.nn.Linear(8, 1), backend=bk)
    with pytest.raises(ValueError, match="torch.nn.Linear"):
        FusedMLP.squashed_gaussian(lat, torch.nn.Sequential(mu), ls, backend=bk)
    with pytest.raises(ValueError, match="both have a bias"):
        FusedMLP.squashed_gaussian(lat, mu, torch.nn.Linear(8, 2, bias=False), backend=bk)
    with pytest.raises(ValueError, match="min <= max"):
        FusedMLP.squashed_gaussian(lat, mu, ls, log_std_bounds=(1.0, -1.0), backend=bk)
    with pytest.raises(ValueError, match="Linear / Tanh / ReLU"):
        FusedMLP.squashed_gaussian([torch.nn.Linear(6, 8), torch.nn.Sigmoid()], mu, ls, backend=bk)
    with pytest.raises(ValueError, match="takes 8 inputs"):
        FusedMLP.squashed_gaussian([torch.nn.Linear(6, 9), torch.nn.ReLU()], mu, ls, backend=bk)
    with pytest.raises(ValueError, match="float32"):
        FusedMLP.squashed_gaussian(lat, mu.double(), ls.double(), backend=bk)
    lat, mu, ls = _actor(6, (8,), 2)
    pol = FusedMLP.squashed_gaussian(lat, mu, ls, backend=bk)
    x, y = torch.zeros(3, 6), torch.zeros(3, 2)
    with pytest.raises(ValueError, match="needs clamp"):
        pol.forward_into(x, y, clamp=None)
    with pytest.raises(ValueError, match="needs clamp"):
        pol(x)                                                          # no default box
    with pytest.raises(ValueError, match="lo < hi"):
        pol.forward_into(x, y, clamp=(1.0, 1.0))
    with pytest.raises(ValueError, match="needs clamp"):
        pol.rollout_net(x, torch.zeros(4, 3, 2), clamp=None)
    with pytest.raises(ValueError, match="noise must be"):
        pol.rollout_net(x, torch.zeros(4, 3, 2), clamp=(0.0, 1.0), noise=torch.zeros(4, 3, 4))       # eps has A columns, not 2A
    assert pol.fits_rollout(6, 2) and not pol.fits_rollout(6, 4) and not pol.fits_rollout(6, 1)       # out_dim is A


def test_from_sb3_stochastic_on_a_stand_in_policy():
    lat, mu, ls = _actor(9, (16, 16), 2, seed=3)
    sac = types.SimpleNamespace(actor=types.SimpleNamespace(latent_pi=lat, mu=mu, log_std=ls, use_sde=False))
    bk = FakeGaussianBackend()
    g = FusedMLP.from_sb3(sac, stochastic=True, backend=bk)
    assert g.head == N.MLP_HEAD_SQUASHED_GAUSSIAN and g.log_std_bounds == (-20.0, 2.0) and g.out_dim == 2
    assert g.layers[0][0] is lat[0].weight                              # shared parameters
    x, eps = torch.randn(7, 9), torch.randn(7, 2)
    got = g.forward_into(x, torch.empty(7, 2), clamp=(-2.0, 6.0), noise=eps)
    np.testing.assert_allclose(got.numpy(), restatement(lat, mu, ls, x, eps, (-20.0, 2.0), (-2.0, 6.0)).numpy(), rtol=RTOL, atol=4 * ATOL)
    det = g.forward_into(x, torch.empty(7, 2), clamp=(-1.0, 1.0))
    np.testing.assert_allclose(det.numpy(), torch.tanh(mu(lat(x))).detach().numpy(), rtol=RTOL, atol=ATOL)
    # stochastic=False (the default) is the deterministic actor of before: latent_pi + mu + tanh, plain head
    d = FusedMLP.from_sb3(sac, backend=bk)
    assert d.head == N.MLP_HEAD_PLAIN and d.out_dim == 2 and len(d.layers) == 3
    np.testing.assert_allclose(d(x).numpy(), det.numpy(), rtol=RTOL, atol=ATOL)
    with pytest.raises(ValueError, match="gSDE"):
        FusedMLP.from_sb3(types.SimpleNamespace(actor=types.SimpleNamespace(latent_pi=lat, mu=mu, log_std=ls, use_sde=True)), stochastic=True)
    with pytest.raises(ValueError, match="SACPolicy"):
        FusedMLP.from_sb3(types.SimpleNamespace(actor=types.SimpleNamespace(mu=mu)), stochastic=True)
    ppo = types.SimpleNamespace(mlp_extractor=types.SimpleNamespace(policy_net=lat), action_net=mu)
    with pytest.raises(ValueError, match="SACPolicy"):
        FusedMLP.from_sb3(ppo, stochastic=True)
    with pytest.raises(ValueError, match="action box"):
        FusedMLP.from_sb3(sac, stochastic=True, clamp=(-1.0, 1.0))


def test_numpy_double_of_the_head_keeps_the_headers_nan_conventions():
    nan, inf = np.nan, np.inf
    raw = np.array([[nan, 0.0], [0.0, nan], [0.0, 0.0], [inf, 0.0], [-inf, 0.0], [0.0, inf], [0.0, -inf]], np.float32)
    eps = np.array([[1.0], [1.0], [nan], [1.0], [1.0], [0.5], [0.5]], np.float32)
    c = gaussian_head(raw, eps, -20.0, 2.0, -1.0, 3.0)[:, 0]
    assert np.isnan(c[:3]).all() and c[3] == 3.0 and c[4] == -1.0
    want = -1.0 + 0.5 * (np.tanh(np.exp(2.0) * 0.5) + 1) * 4
    np.testing.assert_allclose(c[5], want, rtol=1e-6)
    assert c[6] == np.float32(1.0)                                      # sigma = exp(-20): tanh(1e-9) rescaled, the middle of the box
    det = gaussian_head(raw, None, -20.0, 2.0, -1.0, 3.0)[:, 0]
    assert np.isnan(det[0]) and det[1] == 1.0                           # no noise: log_std is not looked at


# ---- LDS of the in-kernel evaluation -------------------------------------------------------------------------------------------------
def test_rollout_lds_formula_matches_the_header_for_both_heads():
    hdr = open(os.path.join(ROOT, "pdecontrolgym_amd", "csrc", "pdegym_policy.h")).read()
    assert "constexpr int kWideOut = 2;" in hdr and "constexpr int kWaves = 16;" in hdr
    assert re.search(r"wide_kept\(const pdegym_mlp& N\) \{ return is_gaussian\(N\) \? 2 \* kWideOut : kWideOut; \}", hdr)
    assert "return kWaves * (wide_ldx(n_in) + 2 * kWideLdh) + wide_kept(N) * kWaves;" in hdr
    stride = lambda w: (w + 63) // 64 * 64 + 4       # noqa: E731
    groups = lambda n: ((n + 3) >> 2) | 1            # noqa: E731
    bk = object()
    for n_in in (30, 201, 257):
        lat, mu, ls = _actor(n_in, (256, 256), 1)
        wide_g = FusedMLP.squashed_gaussian(lat, mu, ls, backend=bk)
        wide_p = FusedMLP(torch.nn.Sequential(*lat, mu), backend=bk)
        base = 16 * (stride((n_in + 15) // 16 * 16) + 2 * stride(256))
        assert wide_p.rollout_lds_bytes(n_in) == 4 * (base + 32)             # unchanged
        assert wide_g.rollout_lds_bytes(n_in) == 4 * (base + 64)
        lat, mu, ls = _actor(n_in, (64,), 1)
        nar_g = FusedMLP.squashed_gaussian(lat, mu, ls, backend=bk)
        nar_p = FusedMLP(torch.nn.Sequential(*lat, mu), backend=bk)
        rows = 16 * ((n_in + 3) // 4 * 4 + 128)
        assert nar_p.rollout_lds_bytes(n_in) == 4 * (groups(n_in) * 4 * 64 + 64 + groups(64) * 4 * 1 + 64 + rows)
        assert nar_g.rollout_lds_bytes(n_in) == 4 * (groups(n_in) * 4 * 64 + 64 + groups(64) * 4 * 2 + 64 + rows)     # a last layer of 2 A neurons
        assert nar_g.fits_rollout(n_in, 1) and wide_g.fits_rollout(n_in, 1)


# ---- DeviceRollout on the CPU doubles -------------------------------------------------------------------------------------------------
def _venv_1d(bk, B):
    import pde_control_gym
    from pde_control_gym.src import TunedReward1D
    nx = 32
    dx = 1.0 / nx
    dt = 0.25 * dx * dx
    S, horizon = 3, 4
    beta = np.full(nx + 1, 3.0, np.float32)
    p = {"T": horizon * S * dt, "dt": dt, "X": 1, "dx": dx, "reward_class": TunedReward1D(horizon * S, -1e3, 3e2), "normalize": True,
         "sensing_loc": "full", "control_type": "Dirchilet", "sensing_type": None, "sensing_noise_func": None,
         "limit_pde_state_size": True, "max_state_value": 1e10, "max_control_value": 5, "control_sample_rate": S * dt,
         "batched_reset_func": lambda idx, nx_: (np.random.default_rng(3).uniform(1, 2, (len(idx), 1)).astype(np.float32)
                                                 * np.ones((1, nx + 1), np.float32), np.tile(beta, (len(idx), 1)))}
    venv = pde_control_gym.make_vec("PDEControlGym-ReactionDiffusionPDE1D", num_envs=B, device="cpu", backend=bk, **p)
    venv.reset_tensor()
    venv.enable_fused_auto_reset()
    return venv, nx + 1, 1, (-2.0, 2.0)


def _venv_traffic(bk, B):
    import random
    import pde_control_gym
    from pde_control_gym.src import TrafficARZReward
    from tests.test_traffic import BASE
    random.seed(0)
    venv = pde_control_gym.make_vec("PDEControlGym-TrafficPDE1D", num_envs=B, device="cpu", backend=bk, reward_class=TrafficARZReward(),
                                    simulation_type="both", limit_pde_state_size=True, control_freq=2, **BASE)
    venv.reset_tensor()
    return venv, 102, 2, (3.0, 6.0)


def _venv_tumor(bk, B):
    from tests.test_tumor_rollout import _venv
    return _venv(bk, 600, True, num_envs=B), 201, 1, (0.0, 1.0)


@pytest.mark.parametrize("family,make,backend", [("1d", _venv_1d, FakeGaussianBackend), ("traffic", _venv_traffic, FakeGaussianBackend),
                                                 ("tumor", _venv_tumor, FakeGaussianTumorBackend)])
@pytest.mark.parametrize("noisy", [True, False])
def test_device_rollout_reproduces_the_torch_restatement_step_by_step(family, make, backend, noisy):
    """``action_low/high`` are the box, ``action_noise`` holds eps (``normal_()`` and no ``mul_``), ``actions[t]`` the command in the box;
    the step loop (one_launch=False) and the single rollout call (one_launch=True) return the same buffers, and every actions[t] is the
    restatement of the formula on obs[t] and eps[t] in torch float32."""
    from pde_control_gym import DeviceRollout
    B, T = 5, 6
    runs = {}
    for one_launch in (False, True):
        bk = backend()
        venv, n_in, A, box = make(bk, B)
        lat, mu, ls = _actor(n_in, (16,), A, seed=4, act=torch.nn.Tanh)
        with torch.no_grad():
            lat[0].weight.mul_(0.05)
        pol = FusedMLP.squashed_gaussian(lat, mu, ls, backend=bk)
        assert venv.one_launch_fits(pol) == (family != "tumor")          # (the tumour engine's one launch is opt-in, as for plain heads)
        ro = DeviceRollout(venv, pol, T, use_graph=False, action_low=box[0], action_high=box[1], action_noise=noisy, one_launch=one_launch)
        assert ro.one_launch is one_launch and (ro.action_noise is not None) == noisy
        assert tuple(ro.actions.shape) == ((T, B) if A == 1 and family != "traffic" else (T, B, A))
        if noisy:
            assert ro.action_noise.shape == ro.actions.shape and ro.action_noise.dtype == torch.float32
            ro.action_noise.copy_(torch.randn(ro.action_noise.shape, generator=torch.Generator().manual_seed(7)))
        ro.run()
        runs[one_launch] = ro
        acts = ro.actions.reshape(T, B, A)
        assert (acts >= box[0]).all() and (acts <= box[1]).all() and acts.std() > 0
        for t in range(T):
            eps = ro.action_noise[t].reshape(B, A) if noisy else None
            want = restatement(lat, mu, ls, ro.obs[t].reshape(B, -1), eps, (-20.0, 2.0), box)
            np.testing.assert_allclose(acts[t].numpy(), want.double().numpy(), rtol=RTOL, atol=ATOL * 0.5 * (box[1] - box[0]), err_msg=f"step {t}")
    # one_launch=None picks the one-launch kernel when the policy fits, as for plain heads
    assert DeviceRollout(venv, pol, T, use_graph=False, action_low=box[0], action_high=box[1]).one_launch is (family != "tumor")
    a, b = runs[False], runs[True]
    for k in ("obs", "actions", "rewards", "terminated", "truncated"):
        np.testing.assert_array_equal(getattr(a, k).numpy(), getattr(b, k).numpy(), err_msg=k)
