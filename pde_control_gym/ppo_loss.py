"""The loss of a PPO minibatch step on the device: from the outputs of actor and critic to the gradients with respect to those
outputs in at most three launches (pdegym_ppo_loss), with the statistics SB3's ``PPO.train`` logs and acts on.

The reference's users train with SB3's ``PPO("MlpPolicy", env)`` (examples/transportPDE/transport1Dppo.py:88-90).  Between the
networks' outputs and ``loss.backward()`` that loss is some forty elementwise launches per minibatch on device tensors -- the gathers
``actions[mb]`` and friends, the Gaussian log-probability, ratio, clamp, min, three means and the mirror image of each under autograd.
``PPOLoss`` restates it (include/pdegym.h: pdegym_ppo_loss) for the ``DiagGaussianDistribution`` of ``MlpPolicy`` on a Box action
space: clipped surrogate, ``F.mse_loss`` value term, entropy term, ``approx_kl``, ``clip_fraction`` and SB3's per-minibatch advantage
normalisation, the gather by the minibatch's indices included, and the closed-form gradients ``d loss / d mean``,
``d loss / d values`` and ``d loss / d log_std``.
"""
from __future__ import annotations

STATS = ("loss", "policy_loss", "value_loss", "entropy_loss", "approx_kl", "clip_fraction", "adv_mean", "adv_std")
MAX_ACTION_DIM = 8


class PPOLossResult:
    """What one ``PPOLoss`` call returns: the eight statistics (``loss``, ``policy_loss``, ``value_loss``, ``entropy_loss``,
    ``approx_kl``, ``clip_fraction``, ``adv_mean``, ``adv_std``) as 0-d views of ONE device tensor ``stats`` -- reading them makes no
    host synchronisation, ``.item()`` them when logging or for the ``target_kl`` stop -- and ``grad_mean`` [N, A], ``grad_values``
    [N] (None without a value term), ``grad_log_std`` [A].  The tensors are the head's own and are overwritten by its next call
    with the same shapes."""

    def __init__(self, stats, grad_mean, grad_values, grad_log_std, mean, values, log_std):
        self.stats, self.grad_mean, self.grad_values, self.grad_log_std = stats, grad_mean, grad_values, grad_log_std
        self._mean, self._values, self._log_std = mean, values, log_std
        for i, name in enumerate(STATS):
            setattr(self, name, stats[i])

    def backward(self):
        """Send the gradients into the graphs that produced ``mean`` and ``values`` -- ONE ``torch.autograd.backward`` call, so
        both networks' backward passes (``FusedMLP.with_grad`` or plain modules) run from it -- and accumulate ``grad_log_std``
        into ``log_std.grad``."""
        import torch
        roots, grads = [], []
        for t, g in ((self._mean, self.grad_mean), (self._values, self.grad_values)):
            if t is not None and t.requires_grad:
                roots.append(t)
                grads.append(g.reshape(t.shape))
        if roots:
            torch.autograd.backward(roots, grads)
        ls = self._log_std
        if ls.requires_grad:
            if ls.is_leaf:
                with torch.no_grad():
                    g = self.grad_log_std.reshape(ls.shape)
                    ls.grad = g.clone() if ls.grad is None else ls.grad.add_(g)
            else:
                torch.autograd.backward([ls], [self.grad_log_std.reshape(ls.shape)])


class PPOLoss:
    """``head = PPOLoss(clip_range=0.2, ent_coef=0.0, vf_coef=0.5, normalize_advantage=True)``; per minibatch
    ``result = head(mean, log_std, values, actions, old_log_prob, advantages, returns, index=mb)`` and ``result.backward()``.

    ``mean`` [N, A] (or [N] for A = 1) and ``values`` [N] or [N, 1] (None: no value term) are the networks' outputs in minibatch
    order; they may carry a ``grad_fn`` and are read detached.  ``log_std`` [A].  ``actions`` [M, A] (or [M]), ``old_log_prob``,
    ``advantages``, ``returns`` [M] are the rollout buffer's flat arrays; ``index`` (int64 [N], what ``torch.randperm(M).chunk()``
    yields) picks the minibatch's rows INSIDE the kernel; without it M = N.  Everything float32 on one device.

    Outputs are allocated at the first call with a shape ``(N, A)`` and reused: a later call allocates nothing and can be captured
    in a ``torch.cuda.graph``.  ``normalize_advantage`` is SB3's: mean and unbiased standard deviation of the minibatch's N
    advantages (skipped for N = 1)."""

    def __init__(self, clip_range: float = 0.2, ent_coef: float = 0.0, vf_coef: float = 0.5, normalize_advantage: bool = True,
                 backend=None):
        self.clip_range, self.ent_coef, self.vf_coef = float(clip_range), float(ent_coef), float(vf_coef)
        self.normalize_advantage = bool(normalize_advantage)
        if backend is None:
            from pdecontrolgym_amd.backend import default_backend
            backend = default_backend()
        self.backend = backend
        self._buffers = {}

    @staticmethod
    def _rows(name, x, width, dev, dtype=None):
        """``x`` as [rows, width] (width None: [rows]): a view, never a copy."""
        import torch
        dtype = torch.float32 if dtype is None else dtype
        if not torch.is_tensor(x):
            raise ValueError(f"{name} must be a tensor, got {type(x).__name__}")
        if x.dtype != dtype:
            raise ValueError(f"{name} must be {dtype}, got {x.dtype}")
        if x.device != dev:
            raise ValueError(f"{name} is on {x.device}, mean on {dev}: every tensor of a call lives on one device")
        x = x.detach()
        if width is None:
            if x.dim() == 2 and x.shape[1] == 1:
                x = x[:, 0]
            if x.dim() != 1:
                raise ValueError(f"{name} must be [rows] (or [rows, 1]), got {tuple(x.shape)}")
            return x if x.shape[0] <= 1 or x.stride(0) == 1 else x.contiguous()
        if x.dim() == 1 and width == 1:
            x = x.unsqueeze(1)
        if x.dim() != 2 or x.shape[1] != width:
            raise ValueError(f"{name} must be [rows, {width}], got {tuple(x.shape)}")
        return x if width == 1 or x.stride(1) == 1 else x.contiguous()

    @staticmethod
    def _width(mean, log_std):
        import torch
        if not torch.is_tensor(mean) or not torch.is_tensor(log_std) or mean.dim() not in (1, 2) or log_std.dim() > 1:
            raise ValueError("mean must be a [N, A] (or [N]) tensor and log_std a [A] tensor")
        A = int(log_std.numel())
        if A > MAX_ACTION_DIM or A < 1:
            raise ValueError(f"the loss head takes 1 .. {MAX_ACTION_DIM} action dimensions, log_std has {A}")
        if (mean.shape[1] if mean.dim() == 2 else 1) != A:
            raise ValueError(f"mean {tuple(mean.shape)} does not match log_std [{A}]")
        return A

    def __call__(self, mean, log_std, values, actions, old_log_prob, advantages, returns, index=None):
        import torch
        A = self._width(mean, log_std)
        dev = mean.device
        m = self._rows("mean", mean, A, dev)
        n = int(m.shape[0])
        ls = self._rows("log_std", log_std.reshape(A), None, dev)
        v = None if values is None else self._rows("values", values, None, dev)
        act = self._rows("actions", actions, A, dev)
        old, adv = self._rows("old_log_prob", old_log_prob, None, dev), self._rows("advantages", advantages, None, dev)
        ret = None if v is None else self._rows("returns", returns, None, dev)
        idx = None if index is None else self._rows("index", index, None, dev, torch.int64)
        if v is not None and v.shape[0] != n:
            raise ValueError(f"values has {v.shape[0]} rows, mean {n}")
        if idx is not None and idx.shape[0] != n:
            raise ValueError(f"index has {idx.shape[0]} entries, mean {n} rows")
        rows = int(act.shape[0])
        if idx is None and rows != n:
            raise ValueError(f"without an index actions must have the {n} rows of mean, got {rows}")
        for name, x in (("old_log_prob", old), ("advantages", adv), ("returns", ret)):
            if x is not None and x.shape[0] != rows:
                raise ValueError(f"{name} has {x.shape[0]} rows, actions {rows}")
        key = (n, A, v is not None, dev)
        buf = self._buffers.get(key)
        if buf is None:
            buf = {"stats": torch.zeros(len(STATS), dtype=torch.float32, device=dev),
                   "d_mean": torch.zeros(n, A, dtype=torch.float32, device=dev),
                   "d_values": torch.zeros(n, dtype=torch.float32, device=dev) if v is not None else None,
                   "d_log_std": torch.zeros(A, dtype=torch.float32, device=dev)}
            self._buffers[key] = buf
        self.backend.ppo_loss(m, ls, v, act, old, adv, ret, buf["d_mean"], buf["d_values"], buf["d_log_std"], buf["stats"],
                              self.clip_range, self.ent_coef, self.vf_coef, self.normalize_advantage, index=idx)
        return PPOLossResult(buf["stats"], buf["d_mean"], buf["d_values"], buf["d_log_std"], mean, values, log_std)

    def log_prob(self, mean, log_std, actions, out=None):
        """``out[i]`` = log-probability of ``actions[i]`` under N(mean[i], exp(log_std)), summed over the action dimensions, through
        the device function the head itself uses (pdegym_diag_gaussian_log_prob): filled after a rollout, the head then sees a
        ratio of exactly 1 while the weights are unchanged.  ``out``: a float32 [N] tensor to write into (default: a new one)."""
        import torch
        A = self._width(mean, log_std)
        dev = mean.device
        m = self._rows("mean", mean, A, dev)
        n = int(m.shape[0])
        act = self._rows("actions", actions, A, dev)
        if act.shape[0] != n:
            raise ValueError(f"actions has {act.shape[0]} rows, mean {n}")
        if out is None:
            out = torch.empty(n, dtype=torch.float32, device=dev)
        flat = self._rows("out", out.reshape(-1) if torch.is_tensor(out) and out.is_contiguous() else out, None, dev)
        if flat.shape[0] != n or flat.data_ptr() != out.data_ptr():
            raise ValueError(f"out must be a contiguous float32 tensor of {n} elements")
        self.backend.diag_gaussian_log_prob(m, self._rows("log_std", log_std.reshape(A), None, dev), act, flat)
        return out
