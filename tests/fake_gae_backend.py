"""A CPU double of ``HipBackend.gae`` built on the NumPy restatement (tests/gae_restatement.py): it drives
``pde_control_gym.DeviceRolloutBuffer`` on CPU tensors, so the buffer's host logic is tested without a GPU.  Same signature, same
shape / dtype / stride checks; results are written into the output tensors in place, as the kernel writes them."""
from __future__ import annotations

import torch

from tests import gae_restatement as R


class FakeGaeBackend:
    name = "gae-restatement"

    def __init__(self):
        self.calls = 0

    def gae(self, rewards, values, terminated, truncated, advantages, returns, gamma, gae_lambda, boot=None, ep_return_acc=None,
            ep_length_acc=None, episode_return=None, episode_length=None):
        T, B = rewards.shape
        assert rewards.dtype in (torch.float32, torch.float64)
        assert values.dtype == torch.float32 and tuple(values.shape) == (T + 1, B)
        for x, dtype in ((terminated, torch.uint8), (truncated, torch.uint8), (boot, torch.float32), (advantages, torch.float32),
                         (returns, torch.float32), (episode_return, torch.float64), (episode_length, torch.int32)):
            assert x is None or (x.dtype == dtype and tuple(x.shape) == (T, B)), (dtype, None if x is None else (x.dtype, x.shape))
        assert (episode_return is None) == (episode_length is None) and (ep_return_acc is None) == (ep_length_acc is None)
        assert ep_return_acc is None or episode_return is not None
        n = lambda x: None if x is None else x.numpy()      # noqa: E731
        adv, ret = R.gae_reference(n(rewards), n(values), n(terminated), n(truncated), gamma, gae_lambda, n(boot))
        advantages.copy_(torch.from_numpy(adv))
        returns.copy_(torch.from_numpy(ret))
        if episode_return is not None:
            er, el, acc, ln = R.episode_scan(n(rewards), n(terminated), n(truncated), n(ep_return_acc), n(ep_length_acc))
            episode_return.copy_(torch.from_numpy(er))
            episode_length.copy_(torch.from_numpy(el))
            if ep_return_acc is not None:
                ep_return_acc.copy_(torch.from_numpy(acc))
                ep_length_acc.copy_(torch.from_numpy(ln))
        self.calls += 1
