"""The CPU doubles of tests/fake_backend.py and tests/fake_tumor_rollout_backend.py with the squashed-Gaussian head
(include/pdegym.h: PDEGYM_MLP_HEAD_SQUASHED_GAUSSIAN) in ``mlp_forward``: the network's 2A raw outputs come from the parent's double
(head, noise and clamp taken off the descriptor), the head is applied in NumPy float32, one rounding per operation, in the header's
order.  The fake rollouts call ``self.mlp_forward``, so they pick it up.  ``gaussian_head`` is the restatement on its own."""
import ctypes as C

import numpy as np
import torch

from pdecontrolgym_amd import _native as N
from tests.fake_backend import FakeBackend
from tests.fake_tumor_rollout_backend import FakeTumorRolloutBackend


def _clip_keep_nan(x, lo, hi):
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(x), x, np.minimum(np.maximum(x, lo), hi)).astype(np.float32)


def gaussian_head(raw, eps, log_std_min, log_std_max, lo, hi):
    """[B, 2A] float32 raw outputs [mu | log_std], eps [B, A] float32 or None -> [B, A] float32 commands."""
    f = np.float32
    raw = np.asarray(raw, f)
    A = raw.shape[1] // 2
    mu, log_std = raw[:, :A], raw[:, A:]
    lo, hi = f(lo), f(hi)
    with np.errstate(all="ignore"):
        z = mu
        if eps is not None:
            s = _clip_keep_nan(log_std, f(log_std_min), f(log_std_max))
            z = (mu + (np.exp(s).astype(f) * np.asarray(eps, f)).astype(f)).astype(f)
        u = np.tanh(z).astype(f)
        c = (lo + ((f(0.5) * (u + f(1.0)).astype(f)).astype(f) * f(hi - lo)).astype(f)).astype(f)
    return _clip_keep_nan(c, lo, hi)


class GaussianHead:
    """Mixin: ``mlp_forward`` with the head.  A plain-head descriptor goes to the parent unchanged."""

    def mlp_forward(self, net, x, y, B):
        if net.head != N.MLP_HEAD_SQUASHED_GAUSSIAN:
            return super().mlp_forward(net, x, y, B)
        last = net.layer[net.n_layers - 1]
        assert last.out_dim % 2 == 0 and last.act == N.MLP_IDENTITY and net.clamp and net.lo < net.hi
        assert net.log_std_min <= net.log_std_max
        A = last.out_dim // 2
        raw_net = N.Mlp()
        C.memmove(C.byref(raw_net), C.byref(net), C.sizeof(N.Mlp))
        raw_net.head, raw_net.clamp, raw_net.noise = N.MLP_HEAD_PLAIN, 0, None
        raw = torch.empty(B, 2 * A, dtype=torch.float32)
        super().mlp_forward(raw_net, x, raw, B)
        eps = None
        if net.noise:
            eps = np.ctypeslib.as_array(C.cast(net.noise, C.POINTER(C.c_float)), (B, int(net.noise_stride)))[:, :A]
        out = gaussian_head(raw.numpy(), eps, net.log_std_min, net.log_std_max, net.lo, net.hi)
        y[:B].copy_(torch.from_numpy(out).to(y.dtype).reshape(y[:B].shape))


class FakeGaussianBackend(GaussianHead, FakeBackend):
    pass


class FakeGaussianTumorBackend(GaussianHead, FakeTumorRolloutBackend):
    pass
