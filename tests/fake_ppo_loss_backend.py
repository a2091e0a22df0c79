"""A CPU double of ``HipBackend.ppo_loss`` / ``diag_gaussian_log_prob`` built on the NumPy restatement
(tests/ppo_loss_restatement.py): it drives ``pde_control_gym.PPOLoss`` on CPU tensors, so the head's host logic is tested without a
GPU.  Same signatures, the same shape / dtype checks as assertions; results are written into the output tensors in place."""
from __future__ import annotations

import torch

from tests import ppo_loss_restatement as R


class FakePPOLossBackend:
    name = "ppo-loss-restatement"

    def __init__(self):
        self.calls = 0
        self.seen = []

    def ppo_loss(self, mean, log_std, values, actions, old_log_prob, advantages, returns, d_mean, d_values, d_log_std, stats,
                 clip_range, ent_coef, vf_coef, normalize_advantage, index=None, workspace=None):
        n, A = mean.shape
        rows = actions.shape[0]
        f32 = torch.float32
        assert not mean.requires_grad and (values is None or not values.requires_grad) and not log_std.requires_grad
        assert mean.dtype == f32 and tuple(log_std.shape) == (A,) and tuple(actions.shape) == (rows, A) and actions.dtype == f32
        assert (values is None) == (d_values is None)
        for x in (old_log_prob, advantages) + (() if values is None else (returns,)):
            assert x.dtype == f32 and tuple(x.shape) == (rows,)
        assert index is None or (index.dtype == torch.int64 and tuple(index.shape) == (n,))
        assert index is not None or rows == n
        assert tuple(d_mean.shape) == (n, A) and tuple(d_log_std.shape) == (A,) and tuple(stats.shape) == (len(R.STATS),)
        num = lambda x: None if x is None else x.numpy()      # noqa: E731
        out = R.head_float32(num(mean), num(log_std), num(values), num(actions), num(old_log_prob), num(advantages), num(returns),
                             clip_range, ent_coef, vf_coef, normalize_advantage, num(index))
        d_mean.copy_(torch.from_numpy(out["d_mean"]))
        d_log_std.copy_(torch.from_numpy(out["d_log_std"]))
        stats.copy_(torch.from_numpy(out["stats"]))
        if values is not None:
            d_values.copy_(torch.from_numpy(out["d_values"]))
        self.calls += 1
        self.seen.append((d_mean.data_ptr(), d_log_std.data_ptr(), stats.data_ptr(), None if d_values is None else d_values.data_ptr()))

    def diag_gaussian_log_prob(self, mean, log_std, actions, out, index=None):
        n, A = mean.shape
        assert tuple(out.shape) == (n,) and out.dtype == torch.float32 and tuple(log_std.shape) == (A,)
        logp, _, _ = R.log_prob_float32(mean.numpy(), log_std.numpy(), actions.numpy(), None if index is None else index.numpy())
        out.copy_(torch.from_numpy(logp))
        self.calls += 1
