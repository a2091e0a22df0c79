"""CPU tests of the SAC loss heads (include/pdegym.h: pdegym_squashed_gaussian_sample, its backward, pdegym_sac_critic_loss,
pdegym_sac_actor_loss; pde_control_gym.SACLoss): the float64 NumPy restatement with its closed-form gradients against torch float64
autograd over SB3's expressions, boundary rows included; a fake backend built on the restatement drives the head's host logic on CPU
tensors; the new names are exported; and tests/c/sac_loss_validation.c runs against the host half of the library under
AddressSanitizer and UBSan.  No kernel is launched; the kernels are pinned to the restatements in tests/test_gpu_sac_loss.py."""
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import sac_loss_restatement as R
from tests.fake_sac_loss_backend import FakeSACLossBackend

torch = pytest.importorskip("torch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LO, HI = -20.0, 2.0
GAMMA, TARGET_ENTROPY = 0.99, -1.5


# ---- SB3's expressions on torch tensors of any float dtype -----------------------------------------------------------------------------
def sb3_sample(raw, eps, lo=LO, hi=HI, through_z=True):
    """SquashedDiagGaussianDistribution: actions = tanh(rsample), log_prob(actions, gaussian_actions) with epsilon 1e-6.  With
    ``through_z`` the Gaussian term is evaluated the way SB3 does, Normal(mu, sigma).log_prob(z) with z = mu + sigma * eps; without,
    with eps as the sample (a constant): the two differ by terms that are 0 in exact arithmetic."""
    A = raw.shape[1] // 2
    mu, log_std = raw[:, :A], torch.clamp(raw[:, A:], lo, hi)
    sigma = log_std.exp()
    z = mu + sigma * eps
    if through_z:
        gauss = torch.distributions.Normal(mu, sigma).log_prob(z).sum(1)
    else:
        gauss = (-0.5 * eps * eps - log_std - 0.5 * math.log(2 * math.pi)).sum(1)
    a = torch.tanh(z)
    return a, gauss - torch.log(1 - a ** 2 + 1e-6).sum(1)


def sb3_critic_loss(q1, q2, q1_target, q2_target, next_log_prob, rewards, dones, log_alpha, gamma):
    """SAC.train: the target under no_grad, 0.5 * sum(F.mse_loss(q, target))."""
    F = torch.nn.functional
    with torch.no_grad():
        alpha = log_alpha.detach().exp()
        nq = q1_target if q2 is None else torch.min(torch.cat((q1_target.unsqueeze(1), q2_target.unsqueeze(1)), 1), dim=1)[0]
        target = rewards + (1 - dones) * gamma * (nq - alpha * next_log_prob)
    qs = (q1,) if q2 is None else (q1, q2)
    return 0.5 * sum(F.mse_loss(q, target) for q in qs), target


def sb3_actor_losses(q1_pi, q2_pi, log_prob, log_alpha, target_entropy):
    """SAC.train: (ent_coef * log_prob - min_qf_pi).mean() and -(log_ent_coef * (log_prob + target_entropy).detach()).mean()."""
    alpha = log_alpha.detach().exp()
    m = q1_pi if q2_pi is None else torch.min(torch.cat((q1_pi.unsqueeze(1), q2_pi.unsqueeze(1)), 1), dim=1)[0]
    return (alpha * log_prob - m).mean(), -(log_alpha * (log_prob + target_entropy).detach()).mean()


def _close(a, b, what, tol=1e-12):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    scale = max(np.abs(b).max(), 1e-300)
    assert np.abs(a - b).max() <= tol * scale, (what, np.abs(a - b).max() / scale)


def _t64(x):
    return torch.tensor(np.asarray(x, np.float64), dtype=torch.float64)


def boundary_sample_case(n, A, seed):
    """A float64 sample case; with n >= 37 rows 0 .. 3 carry a log_std exactly on log_std_min, exactly on log_std_max, 1e-3 below the
    minimum and 1e-3 above the maximum (every column).  The rows at and below the minimum have mu == 0: with sigma = e^-20 SB3's own
    (z - mu) / sigma loses eleven digits to the cancellation in z - mu for any other mean, which says nothing about the restatement."""
    case = {k: v.astype(np.float64) for k, v in R.seeded_sample_case(n, A, seed=seed).items()}
    if n >= 37:
        for row, v in enumerate((LO, HI, LO - 1e-3, HI + 1e-3)):
            case["raw"][row, A:] = v
        case["raw"][:4, :A] *= 0.1
        case["raw"][[0, 2], :A] = 0.0
        case["eps"][1] *= 0.05              # sigma = e^2 there: keep z moderate
        case["eps"][3] *= 0.05
    return case


# ---- the float64 restatement against autograd ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 37])
@pytest.mark.parametrize("A", [1, 3, 8])
def test_sample_restatement_equals_autograd_over_the_sb3_expression(A, n):
    case = boundary_sample_case(n, A, seed=A)
    rng = np.random.default_rng([A, n])
    d_a, d_lp = rng.normal(0, 1, (n, A)), rng.normal(0, 1, n)
    block, logp = R.sample_float64(case["raw"], case["eps"], LO, HI)
    # forward: SB3's own evaluation through z
    raw = _t64(case["raw"]).requires_grad_()
    a_t, lp_t = sb3_sample(raw, _t64(case["eps"]), through_z=True)
    _close(block, a_t.detach().numpy(), "actions")
    _close(logp, lp_t.detach().numpy(), "log_prob")
    # gradients: against autograd with eps as the sample -- (z - mu) / sigma IS eps, the closed form drops nothing else
    a_e, lp_e = sb3_sample(raw, _t64(case["eps"]), through_z=False)
    torch.autograd.backward([a_e, lp_e], [_t64(d_a), _t64(d_lp)])
    want = raw.grad.numpy().copy()
    _close(R.sample_backward_float64(case["raw"], case["eps"], LO, HI, d_a, d_lp), want, "d_raw")
    # either gradient alone
    for da, dl in ((d_a, None), (None, d_lp)):
        raw.grad = None
        a_e, lp_e = sb3_sample(raw, _t64(case["eps"]), through_z=False)
        if da is not None:
            a_e.backward(_t64(da))
        else:
            lp_e.backward(_t64(dl))
        _close(R.sample_backward_float64(case["raw"], case["eps"], LO, HI, da, dl), raw.grad.numpy(), "d_raw (one gradient)")
    # through z autograd leaves rounding residue of terms that cancel exactly, of size ulp(eps) / sigma: the same gradient to
    # 1e-9 where log_std >= -3 (1 / sigma <= 20), not to 1e-12 -- and at sigma = e^-20 (the planted rows, left out here) to 1e-7 only
    raw.grad = None
    torch.autograd.backward(list(sb3_sample(raw, _t64(case["eps"]), through_z=True)), [_t64(d_a), _t64(d_lp)])
    free = slice(4, None) if n >= 37 else slice(None)
    _close(want[free], raw.grad.numpy()[free], "through z", tol=1e-9)
    if n >= 37:
        got = R.sample_backward_float64(case["raw"], case["eps"], LO, HI, d_a, d_lp)
        assert (got[:2, A:] != 0).all(), "on the closed interval the clamp passes the gradient"
        assert (got[2:4, A:] == 0).all() and (want[2:4, A:] == 0).all(), "outside it the gradient is exactly 0"
        assert (got[2:4, :A] != 0).all()
    # a scalar d_log_prob is the array of equal entries
    np.testing.assert_array_equal(R.sample_backward_float64(case["raw"], case["eps"], LO, HI, d_a, 0.25),
                                  R.sample_backward_float64(case["raw"], case["eps"], LO, HI, d_a, np.full(n, 0.25)))


def tie_loss_case(n, seed, dtype=np.float64):
    case = {k: v.astype(dtype) for k, v in R.seeded_loss_case(n, seed=seed, rows=3 * n).items()}
    case["index"] = np.random.default_rng([seed, n]).permutation(3 * n)[:n].astype(np.int64)
    for row in range(0, n, 5):              # ties in known rows
        case["q2"][row] = case["q1"][row]
        case["q2_target"][row] = case["q1_target"][row]
    return case


@pytest.mark.parametrize("two", [True, False], ids=["twin", "single"])
@pytest.mark.parametrize("n", [1, 37])
def test_critic_and_actor_restatements_equal_autograd_over_the_sb3_expressions(n, two):
    case = tie_loss_case(n, seed=n)
    log_alpha = -0.3
    idx = case["index"]
    q1, q2 = _t64(case["q1"]).requires_grad_(), (_t64(case["q2"]).requires_grad_() if two else None)
    la = torch.tensor([log_alpha], dtype=torch.float64, requires_grad=True)
    loss, target = sb3_critic_loss(q1, q2, _t64(case["q1_target"]), _t64(case["q2_target"]) if two else None, _t64(case["next_log_prob"]),
                                   _t64(case["rewards"][idx]), _t64(case["dones"][idx]), la[0], GAMMA)
    loss.backward()
    got = R.critic_float64(case["q1"], case["q2"] if two else None, case["q1_target"], case["q2_target"] if two else None,
                           case["next_log_prob"], case["rewards"], case["dones"], log_alpha, GAMMA, index=idx)
    _close(got["d_q1"], q1.grad.numpy(), "d_q1")
    _close(got["target"], target.numpy(), "target")
    _close(got["stats"][0], float(loss), "critic_loss")
    _close(got["stats"][1], float(q1.mean()), "q1_mean")
    _close(got["stats"][3], float(target.mean()), "target_mean")
    if two:
        _close(got["d_q2"], q2.grad.numpy(), "d_q2")
        _close(got["stats"][2], float(q2.mean()), "q2_mean")
    else:
        assert got["d_q2"] is None and got["stats"][2] == 0.0
    # actor and entropy coefficient
    q1, q2 = _t64(case["q1"]).requires_grad_(), (_t64(case["q2"]).requires_grad_() if two else None)
    lp = _t64(case["log_prob"]).requires_grad_()
    actor_loss, ent_loss = sb3_actor_losses(q1, q2, lp, la[0], TARGET_ENTROPY)
    actor_loss.backward()
    ent_loss.backward()
    got = R.actor_float64(case["q1"], case["q2"] if two else None, case["log_prob"], log_alpha, TARGET_ENTROPY)
    _close(got["d_q1_pi"], q1.grad.numpy(), "d_q1_pi")
    _close(np.full(n, got["d_log_prob"][0]), lp.grad.numpy(), "d_log_prob")
    _close(got["d_log_alpha"], la.grad.numpy(), "d_log_alpha")
    _close(got["stats"], [float(actor_loss), float(ent_loss), math.exp(log_alpha), float(lp.mean())], "actor stats")
    if two:
        _close(got["d_q2_pi"], q2.grad.numpy(), "d_q2_pi")
        ties = np.arange(0, n, 5)
        assert (got["d_q1_pi"][ties] == -1.0 / n).all() and (got["d_q2_pi"][ties] == 0).all(), "a tie goes to the FIRST critic"
        assert n == 1 or ((got["d_q2_pi"] != 0).any() and ((got["d_q1_pi"] == 0) == (got["d_q2_pi"] != 0)).all())


@pytest.mark.parametrize("A", [1, 8])
def test_float32_restatements_are_the_float64_ones_to_float32_accuracy(A):
    n = 300
    case = R.seeded_sample_case(n, A, seed=3, D=4)
    rng = np.random.default_rng(3)
    d_a, d_lp = rng.normal(0, 1, (n, A)).astype(np.float32), rng.normal(0, 1, n).astype(np.float32)
    b32, l32 = R.sample_float32(case["raw"], case["eps"], LO, HI, case["obs"])
    b64, l64 = R.sample_float64(case["raw"], case["eps"], LO, HI, case["obs"])
    assert b32.dtype == np.float32 and l32.dtype == np.float32 and b32.shape == (n, 4 + A)
    np.testing.assert_array_equal(b32[:, :4], case["obs"])
    assert np.abs(b32 - b64).max() <= 1e-6 and np.abs(l32 - l64).max() <= 2e-4 * np.abs(l64).max()
    g32 = R.sample_backward_float32(case["raw"], case["eps"], LO, HI, d_a, d_lp)
    g64 = R.sample_backward_float64(case["raw"], case["eps"], LO, HI, d_a, d_lp)
    assert g32.dtype == np.float32 and np.abs(g32 - g64).max() <= 2e-4 * np.abs(g64).max()
    loss = tie_loss_case(n, seed=4, dtype=np.float32)
    args = (loss["q1"], loss["q2"], loss["q1_target"], loss["q2_target"], loss["next_log_prob"], loss["rewards"], loss["dones"], 0.2, GAMMA)
    c32, c64 = R.critic_float32(*args, index=loss["index"]), R.critic_float64(*args, index=loss["index"])
    for k in ("d_q1", "d_q2", "target", "stats"):
        assert c32[k].dtype == np.float32 and np.abs(c32[k] - c64[k]).max() <= 2e-6 * np.abs(c64[k]).max(), k
    dense = R.critic_float32(*args[:5], loss["rewards"][loss["index"]], loss["dones"][loss["index"]], 0.2, GAMMA)
    for k in ("d_q1", "d_q2", "target", "stats"):
        assert np.array_equal(c32[k].view(np.int32), dense[k].view(np.int32)), k
    a32 = R.actor_float32(loss["q1"], loss["q2"], loss["log_prob"], 0.2, TARGET_ENTROPY)
    a64 = R.actor_float64(loss["q1"], loss["q2"], loss["log_prob"], 0.2, TARGET_ENTROPY)
    for k in ("d_q1_pi", "d_q2_pi", "d_log_prob", "d_log_alpha", "stats"):
        assert a32[k].dtype == np.float32 and np.abs(a32[k] - a64[k]).max() <= 2e-6 * np.abs(a64[k]).max(), k
    # saturation: |z| >= 20 gives a = +-1, a finite log-probability and k == 0 exactly
    sat = {"raw": np.array([[25.0, -1.0], [-30.0, 0.0]], np.float32), "eps": np.array([[0.5], [-0.25]], np.float32)}
    b, lp = R.sample_float32(sat["raw"], sat["eps"], LO, HI)
    assert b[:, 0].tolist() == [1.0, -1.0] and np.isfinite(lp).all()
    assert (R.saturation_k_float32(sat["raw"], sat["eps"], LO, HI) == 0).all()


# ---- SACLoss on the fake backend -------------------------------------------------------------------------------------------------------
def _mlp(sizes, seed):
    torch.manual_seed(seed)
    mods = []
    for i in range(len(sizes) - 1):
        mods.append(torch.nn.Linear(sizes[i], sizes[i + 1]))
        if i < len(sizes) - 2:
            mods.append(torch.nn.Tanh())
    return torch.nn.Sequential(*mods)


@pytest.mark.parametrize("A,indexed,two", [(1, True, True), (3, True, True), (3, False, True), (2, True, False)])
def test_backward_fills_the_grads_autograd_gives_for_the_same_losses(A, indexed, two):
    import pde_control_gym
    n, D, rows = 20, 5, 60
    torch.manual_seed(7)
    o, o2 = torch.randn(n, D), torch.randn(n, D)
    act = torch.rand(n, A) * 2 - 1
    rewards, dones = torch.randn(rows if indexed else n), (torch.rand(rows if indexed else n) < 0.3).float()
    index = torch.randperm(rows)[:n] if indexed else None
    gather = (lambda x: x) if index is None else (lambda x: x[index])
    eps, eps2 = torch.randn(n, A), torch.randn(n, A)
    actor, q1, q2 = _mlp([D, 8, 2 * A], 1), _mlp([D + A, 8, 1], 2), (_mlp([D + A, 8, 1], 3) if two else None)
    q1_t, q2_t = _mlp([D + A, 8, 1], 4).requires_grad_(False), (_mlp([D + A, 8, 1], 5).requires_grad_(False) if two else None)
    with torch.no_grad():
        actor[-1].bias[A:] -= 1.0
    log_alpha = torch.full((1,), -0.4, requires_grad=True)
    critics = [q1] + ([q2] if two else [])
    params = [p for net in [actor] + critics for p in net.parameters()] + [log_alpha]

    def grads():
        out = [None if p.grad is None else p.grad.clone() for p in params]
        for p in params:
            p.grad = None
        return out

    # the torch twin: SB3's three losses under autograd
    with torch.no_grad():
        a2, logp2 = sb3_sample(actor(o2), eps2)
        oa2 = torch.cat([o2, a2], 1)
    oa = torch.cat([o, act], 1)
    critic_loss, target = sb3_critic_loss(q1(oa).squeeze(1), q2(oa).squeeze(1) if two else None, q1_t(oa2).squeeze(1),
                                          q2_t(oa2).squeeze(1) if two else None, logp2, gather(rewards), gather(dones), log_alpha[0], GAMMA)
    critic_loss.backward()
    want_critic = grads()
    a_pi, logp = sb3_sample(actor(o), eps)
    oa_pi = torch.cat([o, a_pi], 1)
    actor_loss, ent_loss = sb3_actor_losses(q1(oa_pi).squeeze(1), q2(oa_pi).squeeze(1) if two else None, logp, log_alpha[0], TARGET_ENTROPY)
    actor_loss.backward()
    ent_loss.backward()
    want_actor = grads()

    bk = FakeSACLossBackend()
    head = pde_control_gym.SACLoss(GAMMA, TARGET_ENTROPY, backend=bk)
    with torch.no_grad():
        block2, lp2 = head.sample(actor(o2), eps2, obs=o2)
    assert block2.grad_fn is None and not block2.requires_grad and not lp2.requires_grad, "no_grad keeps no graph"
    assert torch.equal(block2[:, :D], o2) and torch.allclose(block2[:, D:], a2, atol=1e-6) and torch.allclose(lp2, logp2, rtol=1e-4, atol=1e-5)
    res = head.critic(q1(oa), q2(oa) if two else None, q1_t(block2), q2_t(block2) if two else None, lp2, rewards, dones, log_alpha, index=index)
    assert all(p.grad is None for p in params), "the head itself does not touch the graphs"
    res.backward()
    got = grads()
    for p, g, w in zip(params, got, want_critic):
        assert (g is None) == (w is None), p.shape
        assert g is None or torch.allclose(g, w, rtol=2e-4, atol=2e-7), (p.shape, (g - w).abs().max())
    assert got[-1] is None and got[0] is None, "the critic step reaches neither log_alpha nor the actor"
    assert float(res.critic_loss) == pytest.approx(float(critic_loss), rel=2e-5) and torch.allclose(res.target, target, rtol=1e-5, atol=1e-6)
    for i, name in enumerate(R.CRITIC_STATS):
        x = getattr(res, name)
        assert x.dim() == 0 and x.data_ptr() == res.stats[i].data_ptr()
    assert (res.grad_q2 is None) == (not two) and tuple(res.grad_q1.shape) == (n,)

    block, lp = head.sample(actor(o), eps, obs=o)
    assert block.requires_grad and lp.requires_grad and tuple(block.shape) == (n, D + A) and tuple(lp.shape) == (n,)
    assert block.data_ptr() != block2.data_ptr() and lp.data_ptr() != lp2.data_ptr(), "the no_grad sample survives the policy sample"
    res = head.actor(q1(block), q2(block) if two else None, lp, log_alpha)
    assert all(p.grad is None for p in params)
    res.backward()
    got = grads()
    for p, g, w in zip(params, got, want_actor):
        assert g is not None and torch.allclose(g, w, rtol=5e-4, atol=5e-7), (p.shape, (g - w).abs().max())
    assert bk.calls == {"sample": 2, "sample_backward": 1, "critic": 1, "actor": 1}, "ONE autograd call: one sample backward"
    d_actions_stride, d_log_prob = bk.strides[0]
    assert d_actions_stride == (D + A, 1), "the action columns of the critics' dx are read in place"
    assert d_log_prob == ((n,), (0,)), "d_log_prob arrives as the one scalar"
    for name, want in zip(R.ACTOR_STATS, (actor_loss, ent_loss, log_alpha.exp()[0], logp.mean())):
        assert float(getattr(res, name)) == pytest.approx(float(want), rel=5e-5, abs=1e-6), name
    # a second backward() accumulates, as autograd does
    block, lp = head.sample(actor(o), eps, obs=o)
    head.actor(q1(block), q2(block) if two else None, lp, log_alpha).backward()
    block, lp = head.sample(actor(o), eps, obs=o)
    head.actor(q1(block), q2(block) if two else None, lp, log_alpha).backward()
    assert torch.allclose(log_alpha.grad, 2 * want_actor[-1], rtol=5e-4) and torch.allclose(params[0].grad, 2 * want_actor[0], rtol=5e-4, atol=5e-7)


def test_sample_shapes_strides_and_reuse():
    import pde_control_gym
    bk = FakeSACLossBackend()
    head = pde_control_gym.SACLoss(GAMMA, TARGET_ENTROPY, log_std_bounds=(-5.0, 1.0), backend=bk)
    assert (head.gamma, head.target_entropy, head.log_std_min, head.log_std_max) == (GAMMA, TARGET_ENTROPY, -5.0, 1.0)
    assert pde_control_gym.SACLoss(0.9, -1.0, backend=bk).log_std_min == -20.0
    n, A, D = 12, 2, 3
    case = R.seeded_sample_case(n, A, seed=1, D=D)
    wide = torch.zeros(n, 2 * A + 3)
    wide[:, :2 * A] = torch.from_numpy(case["raw"])
    raw, eps, obs = wide[:, :2 * A], torch.from_numpy(case["eps"]), torch.from_numpy(case["obs"])      # raw: a view with a row stride
    a, lp = head.sample(raw, eps)
    want_b, want_lp = R.sample_float32(case["raw"], case["eps"], -5.0, 1.0)
    assert tuple(a.shape) == (n, A) and np.array_equal(a.numpy(), want_b) and np.array_equal(lp.numpy(), want_lp)
    b, lp2 = head.sample(raw, eps, obs=obs)
    assert tuple(b.shape) == (n, D + A) and torch.equal(b[:, :D], obs) and np.array_equal(b[:, D:].numpy(), want_b)
    a2, _ = head.sample(raw, eps)
    assert a2.data_ptr() == a.data_ptr() and b.data_ptr() != a.data_ptr(), "outputs are reused per shape"
    assert bk.seen[0] == bk.seen[2] and bk.seen[0] != bk.seen[1]
    # a graph through raw alone: d_actions without d_log_prob, and the other way round
    leaf = torch.from_numpy(case["raw"]).requires_grad_()
    a, lp = head.sample(leaf, eps)
    d_a = torch.randn(n, A)
    a.backward(d_a)
    want = R.sample_backward_float32(case["raw"], case["eps"], -5.0, 1.0, d_a.numpy(), None)
    assert np.array_equal(leaf.grad.numpy(), want) and bk.strides[-1] == ((A, 1), None)
    leaf.grad = None
    a, lp = head.sample(leaf, eps)
    lp.sum().backward()
    want = R.sample_backward_float32(case["raw"], case["eps"], -5.0, 1.0, None, np.ones(n, np.float32))
    assert np.array_equal(leaf.grad.numpy(), want) and bk.strides[-1][0] is None
    with torch.no_grad():
        a, lp = head.sample(leaf, eps)
    assert not a.requires_grad and a.grad_fn is None and not lp.requires_grad
    # one critic, A = 1 written as [N, 1] outputs of the critics
    loss = R.seeded_loss_case(n, seed=2)
    t = {k: torch.from_numpy(v) for k, v in loss.items()}
    la = torch.zeros(1)
    r1 = head.critic(t["q1"].unsqueeze(1), None, t["q1_target"].unsqueeze(1), None, t["next_log_prob"], t["rewards"].unsqueeze(1),
                     t["dones"].unsqueeze(1), la)
    r2 = head.critic(t["q1"], None, t["q1_target"], None, t["next_log_prob"], t["rewards"], t["dones"], la)
    assert r1.grad_q2 is None and r1.grad_q1.data_ptr() == r2.grad_q1.data_ptr() and float(r1.q2_mean) == 0.0
    r1.backward()                                                # nothing requires grad: a no-op, not an error
    r3 = head.actor(t["q1"], None, t["log_prob"], la)
    assert r3.grad_q2_pi is None and float(r3.alpha) == 1.0 and tuple(r3.grad_log_prob.shape) == (1,)
    r3.backward()
    assert la.grad is None


def test_value_errors():
    import pde_control_gym
    bk = FakeSACLossBackend()
    head = pde_control_gym.SACLoss(GAMMA, TARGET_ENTROPY, backend=bk)
    with pytest.raises(ValueError):
        pde_control_gym.SACLoss(GAMMA, TARGET_ENTROPY, log_std_bounds=(2.0, 2.0), backend=bk)
    n, A, D = 16, 2, 3
    case = R.seeded_sample_case(n, A, seed=1, D=D)
    raw, eps, obs = (torch.from_numpy(case[k]) for k in ("raw", "eps", "obs"))
    head.sample(raw, eps, obs=obs)
    bad_sample = [dict(raw=raw.double()), dict(raw=raw[:, :3]), dict(raw=torch.zeros(n, 18), eps=torch.zeros(n, 9)), dict(raw=raw.numpy()),
                  dict(raw=raw[:, 0]), dict(eps=eps.double()), dict(eps=eps[:15]), dict(eps=eps[:, :1]), dict(eps=eps.to("meta")),
                  dict(obs=obs.double()), dict(obs=obs[:15]), dict(obs=obs[:, 0]), dict(obs=obs.to("meta")), dict(obs=obs.numpy())]
    for change in bad_sample:
        with pytest.raises(ValueError):
            head.sample(**{**dict(raw=raw, eps=eps, obs=obs), **change})
    assert bk.calls["sample"] == 1
    t = {k: torch.from_numpy(v) for k, v in R.seeded_loss_case(n, seed=2, rows=48).items()}
    index = torch.randperm(48)[:n]
    la = torch.zeros(1)
    ok = dict(q1=t["q1"], q2=t["q2"], q1_target=t["q1_target"], q2_target=t["q2_target"], next_log_prob=t["next_log_prob"],
              rewards=t["rewards"], dones=t["dones"], log_alpha=la, index=index)
    head.critic(**ok)
    bad_critic = [dict(q1=t["q1"].double()), dict(q2=t["q2"][:15]), dict(q2=None), dict(q2_target=None), dict(q1_target=t["q1_target"].half()),
                  dict(next_log_prob=t["next_log_prob"][:15]), dict(rewards=t["rewards"].double()), dict(dones=t["dones"].bool()),
                  dict(dones=t["dones"][:47]), dict(index=index.int()), dict(index=index[:15]), dict(index=None), dict(index=index.to("meta")),
                  dict(log_alpha=torch.zeros(2)), dict(log_alpha=0.0), dict(log_alpha=la.double()), dict(q1=t["q1"].numpy()),
                  dict(q1=torch.zeros(n, 2))]
    for change in bad_critic:
        with pytest.raises(ValueError):
            head.critic(**{**ok, **change})
    assert bk.calls["critic"] == 1
    ok = dict(q1_pi=t["q1"], q2_pi=t["q2"], log_prob=t["log_prob"], log_alpha=la)
    head.actor(**ok)
    for change in (dict(q1_pi=t["q1"].double()), dict(q2_pi=t["q2"][:15]), dict(log_prob=t["log_prob"][:15]), dict(log_prob=t["log_prob"].double()),
                   dict(log_alpha=torch.zeros(3)), dict(log_alpha=None), dict(q1_pi=None), dict(q2_pi=t["q2"].to("meta"))):
        with pytest.raises(ValueError):
            head.actor(**{**ok, **change})
    assert bk.calls["actor"] == 1


# ---- exports and documentation ----------------------------------------------------------------------------------------------------------
NEW_NAMES = ("pdegym_squashed_gaussian_sample", "pdegym_squashed_gaussian_sample_backward", "pdegym_sac_critic_loss",
             "pdegym_sac_actor_loss", "pdegym_sac_loss_workspace")


def _struct_fields(header, name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for d in filter(None, (x.strip() for x in body.split(";"))):
        d = re.sub(r"^(const\s+)?(int32_t|int64_t|uint8_t|float|double|void)\s*\*?", "", d).strip()
        names += [x.strip().lstrip("*") for x in d.split(",")]
    return names


def test_new_names_are_exported_and_documented():
    import ctypes
    import pde_control_gym
    from pdecontrolgym_amd import _native as N
    from pdecontrolgym_amd import backend, build
    for name in NEW_NAMES:
        assert name in N.EXPORTS, name
    assert "pdegym_sac_loss.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "pdegym_sac_loss.hip"))
    assert N.ABI_VERSION == 21
    assert N.SAC_CRITIC_STATS == R.CRITIC_STATS == pde_control_gym.sac_loss.CRITIC_STATS
    assert N.SAC_ACTOR_STATS == R.ACTOR_STATS == pde_control_gym.sac_loss.ACTOR_STATS
    assert "SACLoss" in pde_control_gym.__all__ and pde_control_gym.SACLoss.__module__ == "pde_control_gym.sac_loss"
    for fn in (backend.HipBackend.squashed_gaussian_sample, backend.HipBackend.squashed_gaussian_sample_backward,
               backend.HipBackend.sac_critic_loss, backend.HipBackend.sac_actor_loss):
        assert hasattr(fn, "device_guard_key")
    header = open(os.path.join(ROOT, "include", "pdegym.h")).read()
    assert "#define PDEGYM_ABI_VERSION 21" in header
    for name in NEW_NAMES[:4]:
        assert f"int {name}(const {name}_args* " in header, name
    assert "int64_t pdegym_sac_loss_workspace(int32_t N);" in header
    # the ctypes mirrors follow the header's structures field for field
    for struct, mirror, size in (("pdegym_squashed_gaussian_sample_args", N.SquashedGaussianSample, 8 * 11),
                                 ("pdegym_squashed_gaussian_sample_backward_args", N.SquashedGaussianSampleBackward, 8 * 12),
                                 ("pdegym_sac_critic_loss_args", N.SacCriticLoss, 8 * 17), ("pdegym_sac_actor_loss_args", N.SacActorLoss, 8 * 12)):
        assert _struct_fields(header, struct) == [f[0] for f in mirror._fields_], struct
        assert ctypes.sizeof(mirror) == size, struct
    for where in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        text = open(os.path.join(ROOT, where)).read()
        assert "SACLoss" in text and "pdegym_sac_critic_loss" in text, where
    assert "### 4.16" in open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "r14_sac_loss.json" in open(os.path.join(ROOT, "profiles", "README.md")).read()
    # the source keeps its promises about synchronisation and launches
    src = open(os.path.join(build.CSRC, "pdegym_sac_loss.hip")).read()
    code = re.sub(r"//[^\n]*", "", src)
    assert "atomic" not in code and "__threadfence" not in code and "<<<" not in code and "hipLaunchKernel" in code


def test_the_sac_example_has_the_switch_and_keeps_its_defaults():
    import importlib.util
    import inspect
    import sys
    path = os.path.join(ROOT, "examples", "train_sac_device.py")
    src = open(path).read()
    assert "SACLoss" in src and "head.sample" in src and "head.critic" in src and "head.actor" in src and "result.backward()" in src
    sys.path.insert(0, os.path.dirname(path))
    try:
        spec = importlib.util.spec_from_file_location("train_sac_device_for_test", path)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        sys.path.remove(os.path.dirname(path))
    sig = inspect.signature(mod.main)
    assert sig.parameters["fused_loss"].default is False and sig.parameters["fused_grad"].default is False
    assert list(sig.parameters)[:9] == ["iterations", "num_envs", "n_steps", "hidden", "one_launch", "quiet", "updates", "batch", "fused_grad"]


# ---- argument validation of the entry points, host half under ASan + UBSan -------------------------------------------------------------
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="needs hipcc")
def test_sac_loss_entry_points_validate_their_arguments_under_asan_and_ubsan(tmp_path):
    """tests/c/sac_loss_validation.c (its own main) against the host half of pdegym_sac_loss.hip + pdegym_abi.hip, compiled with
    --cuda-host-only and the sanitizers and given an empty device image: every refusal answers with its code and a message, a
    well-formed descriptor fails only at the launch, and no call reaches a device."""
    from pdecontrolgym_amd import build
    hipcc = shutil.which("hipcc")
    inc = ["-I" + os.path.join(ROOT, "include"), "-I" + build.CSRC]
    objs = []
    for s in ("pdegym_abi.hip", "pdegym_sac_loss.hip"):
        o = str(tmp_path / s.replace(".hip", ".o"))
        r = subprocess.run([hipcc, "--offload-arch=gfx950", "--cuda-host-only", "-O1", "-g", "-std=c++17", "-fPIC"]
                           + SAN + inc + ["-c", os.path.join(build.CSRC, s), "-o", o],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        assert r.returncode == 0, r.stdout.decode()[-3000:]
        objs.append(o)
    nm = subprocess.run(["nm", "-u"] + objs, stdout=subprocess.PIPE, check=True).stdout.decode()
    names = sorted({ln.split()[-1] for ln in nm.splitlines() if "__hip_fatbin_" in ln})
    stub = tmp_path / "empty_fatbins.c"
    stub.write_text("".join(f'__attribute__((aligned(4096))) const char {n}[4096] = "__CLANG_OFFLOAD_BUNDLE__";\n' for n in names))
    stub_o = str(tmp_path / "empty_fatbins.o")
    subprocess.run(["gcc", "-c", "-fPIC", str(stub), "-o", stub_o], check=True)
    lib = str(tmp_path / "libpdegym_sac_loss_asan.so")
    r = subprocess.run([hipcc, "-shared", "-fPIC"] + SAN + ["-o", lib] + objs + [stub_o], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()[-3000:]
    exe = str(tmp_path / "sac_loss_validation")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    r = subprocess.run([hipcc, "-x", "c", "-std=c11", "-Wall", "-Werror", "-g"] + SAN
                       + [os.path.join(ROOT, "tests", "c", "sac_loss_validation.c"), "-I" + os.path.join(ROOT, "include"),
                          "-L" + str(tmp_path), "-lpdegym_sac_loss_asan", "-Wl,-rpath," + str(tmp_path),
                          "-Wl,-rpath," + os.path.join(rocm, "lib"), "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1", HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, env=env, timeout=120)
    out = r.stdout.decode()
    assert r.returncode == 0 and "SAC-LOSS-VALIDATION-OK" in out, out[-4000:]
    assert "runtime error" not in out and "AddressSanitizer" not in out, out[-4000:]
    assert int(out.strip().splitlines()[-2].split()[1]) >= 120, out[-1000:]
