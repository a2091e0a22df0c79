"""A CPU double of ``HipBackend.squashed_gaussian_sample`` / ``..._backward`` / ``sac_critic_loss`` / ``sac_actor_loss`` built on the
NumPy restatement (tests/sac_loss_restatement.py): it drives ``pde_control_gym.SACLoss`` on CPU tensors, so the head's host logic
is tested without a GPU.  Same signatures, the same shape / dtype / stride checks as assertions; results are written into the
output tensors in place."""
from __future__ import annotations

import torch

from tests import sac_loss_restatement as R

F32 = torch.float32


def _num(x):
    return None if x is None else x.detach().numpy()


def _rows2(x, n, width):
    assert x.dtype == F32 and tuple(x.shape) == (n, width) and not x.requires_grad, (x.dtype, tuple(x.shape))
    assert (width == 1 or x.stride(1) == 1) and (n == 1 or x.stride(0) >= width), x.stride()


def _rows1(x, n, dtype=F32):
    assert x.dtype == dtype and tuple(x.shape) == (n,) and not x.requires_grad and (n == 1 or x.stride(0) == 1), (x.dtype, tuple(x.shape))


class FakeSACLossBackend:
    name = "sac-loss-restatement"

    def __init__(self):
        self.calls = {"sample": 0, "sample_backward": 0, "critic": 0, "actor": 0}
        self.seen = []
        self.strides = []

    def squashed_gaussian_sample(self, raw, eps, actions, log_prob, log_std_min, log_std_max, obs=None):
        n, A = raw.shape[0], raw.shape[1] // 2
        D = 0 if obs is None else obs.shape[1]
        _rows2(raw, n, 2 * A)
        _rows2(eps, n, A)
        _rows2(actions, n, D + A)
        _rows1(log_prob, n)
        if obs is not None:
            _rows2(obs, n, D)
        block, logp = R.sample_float32(_num(raw), _num(eps), log_std_min, log_std_max, _num(obs))
        actions.copy_(torch.from_numpy(block))
        log_prob.copy_(torch.from_numpy(logp))
        self.calls["sample"] += 1
        self.seen.append(("sample", actions.data_ptr(), log_prob.data_ptr()))

    def squashed_gaussian_sample_backward(self, raw, eps, d_actions, d_log_prob, d_raw, log_std_min, log_std_max):
        n, A = raw.shape[0], raw.shape[1] // 2
        _rows2(raw, n, 2 * A)
        _rows2(eps, n, A)
        _rows2(d_raw, n, 2 * A)
        assert d_actions is not None or d_log_prob is not None
        if d_actions is not None:
            _rows2(d_actions, n, A)
        if d_log_prob is not None:
            assert d_log_prob.dtype == F32 and d_log_prob.dim() == 1
            assert d_log_prob.shape[0] == 1 or (d_log_prob.shape[0] == n and d_log_prob.stride(0) in (0, 1))
        self.strides.append((None if d_actions is None else tuple(d_actions.stride()),
                             None if d_log_prob is None else (tuple(d_log_prob.shape), tuple(d_log_prob.stride()))))
        out = R.sample_backward_float32(_num(raw), _num(eps), log_std_min, log_std_max, _num(d_actions),
                                        None if d_log_prob is None else d_log_prob.detach().contiguous().numpy())
        d_raw.copy_(torch.from_numpy(out))
        self.calls["sample_backward"] += 1

    def sac_critic_loss(self, q1, q2, q1_target, q2_target, next_log_prob, rewards, dones, log_alpha, gamma, d_q1, d_q2, target=None,
                        stats=None, index=None, workspace=None):
        n = q1.shape[0]
        rows = rewards.shape[0]
        assert (q2 is None) == (q2_target is None) == (d_q2 is None)
        for x in (q1, q1_target, next_log_prob, d_q1) + (() if q2 is None else (q2, q2_target, d_q2)) + (() if target is None else (target,)):
            _rows1(x, n)
        _rows1(rewards, rows)
        _rows1(dones, rows)
        _rows1(log_alpha, 1)
        assert index is not None or rows == n
        if index is not None:
            _rows1(index, n, torch.int64)
        out = R.critic_float32(_num(q1), _num(q2), _num(q1_target), _num(q2_target), _num(next_log_prob), _num(rewards), _num(dones),
                               float(log_alpha[0]), gamma, _num(index))
        d_q1.copy_(torch.from_numpy(out["d_q1"]))
        if q2 is not None:
            d_q2.copy_(torch.from_numpy(out["d_q2"]))
        if target is not None:
            target.copy_(torch.from_numpy(out["target"]))
        if stats is not None:
            _rows1(stats, len(R.CRITIC_STATS))
            stats.copy_(torch.from_numpy(out["stats"]))
        self.calls["critic"] += 1
        self.seen.append(("critic", d_q1.data_ptr(), None if d_q2 is None else d_q2.data_ptr(), None if stats is None else stats.data_ptr()))

    def sac_actor_loss(self, q1_pi, q2_pi, log_prob, log_alpha, target_entropy, d_q1_pi, d_q2_pi, d_log_prob, d_log_alpha, stats=None,
                       workspace=None):
        n = q1_pi.shape[0]
        assert (q2_pi is None) == (d_q2_pi is None)
        for x in (q1_pi, log_prob, d_q1_pi) + (() if q2_pi is None else (q2_pi, d_q2_pi)):
            _rows1(x, n)
        for x in (log_alpha, d_log_prob, d_log_alpha):
            _rows1(x, 1)
        out = R.actor_float32(_num(q1_pi), _num(q2_pi), _num(log_prob), float(log_alpha[0]), target_entropy)
        d_q1_pi.copy_(torch.from_numpy(out["d_q1_pi"]))
        if q2_pi is not None:
            d_q2_pi.copy_(torch.from_numpy(out["d_q2_pi"]))
        d_log_prob.copy_(torch.from_numpy(out["d_log_prob"]))
        d_log_alpha.copy_(torch.from_numpy(out["d_log_alpha"]))
        if stats is not None:
            _rows1(stats, len(R.ACTOR_STATS))
            stats.copy_(torch.from_numpy(out["stats"]))
        self.calls["actor"] += 1
        self.seen.append(("actor", d_q1_pi.data_ptr(), d_log_prob.data_ptr(), None if stats is None else stats.data_ptr()))
