"""Fused forward pass of a small MLP policy on the device (C ABI: pdegym_mlp_forward, csrc/pdegym_mlp.hip).

The reference's RL controllers are SB3 ``MlpPolicy`` networks -- Linear/Tanh stacks, two hidden layers of 64 units by
default (examples/transportPDE/transport1Dppo.py:88-90) -- evaluated once per ``env.step``.  ``FusedMLP`` wraps such a
``torch.nn.Sequential`` (or any iterable of ``Linear`` / ``Tanh`` / ``ReLU`` / ``Identity`` / ``Flatten`` modules) and
evaluates it in ONE kernel launch.  The kernel reads the weights in a blocked transpose ``[ceil(in/4), out, 4]`` (one
16-byte load per lane = four inputs of its neuron, contiguous per wave), so the wrapper keeps that copy next to the module's
parameters: ``refresh()`` re-transposes the layers
whose parameters changed (checked through the tensors' version counters; called automatically by ``__call__`` /
``forward_into`` outside graph capture and by ``DeviceRollout.run`` before it replays its hipGraph).  The copies keep their
addresses, so a captured graph sees refreshed weights.

``FusedMLP.squashed_gaussian`` / ``FusedMLP.from_sb3(policy, stochastic=True)``: the actor SAC samples while it learns -- a
state-dependent standard deviation, the tanh squash AFTER the noise, the result rescaled to the action box -- as a second head of
the same kernels (include/pdegym.h: PDEGYM_MLP_HEAD_SQUASHED_GAUSSIAN).

``FusedMLP.with_grad(obs)``: the same forward launch under autograd -- its backward is ``pdegym_mlp_backward``
(csrc/pdegym_mlp_backward.hip) for layers of at most 64 units and ``pdegym_mlp_backward_wide``
(csrc/pdegym_mlp_backward_wide.hip) for layers of up to 256 -- SB3's SAC networks --, and fills the ``.grad`` of the wrapped module's
Parameters.

``policy(obs, tail)`` / ``forward_into(obs, out, tail=...)`` / ``with_grad(obs, tail, params=...)``: SB3's ``critic(obs, actions)`` call
form -- the first layer reads its row from the two tensors (pdegym_mlp_forward_cat: no ``torch.cat``), the gradient goes back to
``tail`` (and to a float32 ``obs`` that asks for it) as ``[B, n2]`` / ``[B, D]`` tensors of their own, and ``params=False`` -- the critic
pass of SAC's actor step -- runs the backward as ONE launch that forms no parameter gradient (pdegym_mlp_backward_cat / _wide_cat).
"""
from __future__ import annotations

from . import _native as N


def fits_rollout_kernel(policy, in_dim: int, out_dim: int, extra_lds_bytes: int = 0) -> bool:
    """Whether ``policy`` fits a rollout kernel with ``in_dim`` inputs, ``out_dim`` outputs and ``extra_lds_bytes`` of the engine's
    own LDS per workgroup: what the engines' ``policy_fits_rollout`` add their own conditions to.  Duck-typed: an object without
    ``fits_rollout`` (anything but a ``FusedMLP``) does not fit."""
    fits = getattr(policy, "fits_rollout", None)
    return fits is not None and fits(in_dim, out_dim, extra_lds_bytes)


class FusedMLP:
    """``policy = FusedMLP(torch_module)``; ``policy(obs)`` -> ``[B, out_dim]`` float32 actions on the same device.

    ``clamp=(lo, hi)`` fuses the action-box clamp into the launch.  ``forward_into(obs, out)`` writes into a caller tensor
    (``pde_control_gym.DeviceRollout`` points it at slot t of its action buffer).  ``__call__`` and ``forward_into`` are inference
    only (no autograd graph); ``with_grad(obs)`` is the differentiable evaluation -- the same forward launch with a ``grad_fn``
    whose backward is ``pdegym_mlp_backward`` (three launches) and fills the ``.grad`` of the wrapped module's own Parameters, for
    networks that ``fits_backward()`` (layers of at most 64 units); wider ones that ``fits_backward_wide()`` (up to 256 units) go
    through ``pdegym_mlp_backward_wide``, three launches as well.
    """

    def __init__(self, module, clamp=None, backend=None):
        import torch
        layers = []            # [weight, bias, act]
        mods = list(module) if not isinstance(module, torch.nn.Linear) else [module]
        for m in mods:
            if isinstance(m, torch.nn.Linear):
                layers.append([m.weight, m.bias, N.MLP_IDENTITY])
            elif isinstance(m, (torch.nn.Tanh, torch.nn.ReLU)):
                if not layers or layers[-1][2] != N.MLP_IDENTITY:
                    raise ValueError("an activation must follow a Linear layer (one activation per layer)")
                layers[-1][2] = N.MLP_TANH if isinstance(m, torch.nn.Tanh) else N.MLP_RELU
            elif isinstance(m, (torch.nn.Identity, torch.nn.Flatten)):
                continue
            else:
                raise ValueError(f"FusedMLP supports Linear / Tanh / ReLU / Identity / Flatten stacks, got {type(m).__name__}")
        if not 1 <= len(layers) <= N.MLP_MAX_LAYERS:
            raise ValueError(f"FusedMLP takes 1..{N.MLP_MAX_LAYERS} Linear layers, got {len(layers)}")
        for i, (w, b, _) in enumerate(layers):
            if w.dtype != torch.float32 or not w.is_contiguous() or (b is not None and (b.dtype != torch.float32 or not b.is_contiguous())):
                raise ValueError("FusedMLP needs contiguous float32 parameters")
            if w.shape[0] > N.MLP_MAX_WIDTH:
                raise ValueError(f"layer {i} is wider than {N.MLP_MAX_WIDTH} units")
            if i and w.shape[1] != layers[i - 1][0].shape[0]:
                raise ValueError(f"layer {i} takes {w.shape[1]} inputs but layer {i - 1} produces {layers[i - 1][0].shape[0]}")
        if layers[0][0].shape[1] > N.MLP_MAX_INPUT:
            raise ValueError(f"observation rows wider than {N.MLP_MAX_INPUT} are not supported")
        if clamp is not None and not float(clamp[0]) <= float(clamp[1]):
            raise ValueError("clamp must be (lo, hi) with lo <= hi")
        self.module, self.layers = module, layers
        self.head, self.log_std_bounds, self._heads = N.MLP_HEAD_PLAIN, (0.0, 0.0), None
        # blocked transpose [ceil(in/4), out, 4] (include/pdegym.h); the buffers keep their addresses for captured graphs
        self._wt = [torch.zeros((w.shape[1] + 3) // 4, w.shape[0], 4, dtype=torch.float32, device=w.device) for w, _, _ in layers]
        self._seen = [None] * len(layers)
        self._optimizer = None      # the pde_control_gym.FusedAdam that maintains the copies, once attached
        self.refresh(force=True)
        self.in_dim, self.out_dim = int(layers[0][0].shape[1]), int(layers[-1][0].shape[0])
        self.clamp = None if clamp is None else (float(clamp[0]), float(clamp[1]))
        self.device = layers[0][0].device
        if backend is None:
            from .backend import default_backend
            backend = default_backend()
        self.backend = backend

    def _refresh_unless_capturing(self, x):
        """Pick up in-place parameter updates before a launch that reads ``x`` -- except while a hipGraph is being captured
        (``refresh`` launches copies of its own; ``DeviceRollout.run`` refreshes before it replays)."""
        import torch
        if not (x.is_cuda and torch.cuda.is_current_stream_capturing()):
            self.refresh()

    @classmethod
    def squashed_gaussian(cls, latent, mu, log_std, log_std_bounds=(-20.0, 2.0), backend=None):
        """The squashed-Gaussian actor of SAC: ``latent`` (an iterable of Linear / Tanh / ReLU modules, may be empty) followed by the two
        ``torch.nn.Linear`` heads ``mu`` and ``log_std`` of equal shapes [A, width].  Per action, in float32 and in SB3's order
        (include/pdegym.h)::

            a = tanh(mu(s) + exp(clip(log_std(s), *log_std_bounds)) * eps),    command = lo + 0.5 (a + 1) (hi - lo)

        ``eps`` is what ``forward_into`` / ``rollout_net`` are given as ``noise`` -- STANDARD-NORMAL draws, not pre-scaled noise;
        ``noise=None`` is the deterministic actor ``tanh(mu(s))``, rescaled.  ``(lo, hi)`` is the ``clamp`` they are given, here the
        action box: this head has no default clamp, ``clamp=None`` is a ``ValueError``.  ``out_dim == A``; the fused last layer
        holds the rows ``[mu; log_std]`` (its bias a concatenated buffer of the wrapper's, rewritten in place by ``refresh()`` like
        the weights, which watches all four parameter tensors).  ``forward_into`` takes A <= 8; inside the rollout kernels A is the
        engine's (1, or 2 for two-command traffic).  A replay buffer that stores SB3's scaled action recovers it from the command
        as ``2 (c - lo) / (hi - lo) - 1``.  Log-probabilities are not computed: SAC recomputes them under autograd at update time."""
        import torch
        for m, name in ((mu, "mu"), (log_std, "log_std")):
            if not isinstance(m, torch.nn.Linear):
                raise ValueError(f"{name} must be a torch.nn.Linear, got {type(m).__name__}")
        if mu.weight.shape != log_std.weight.shape:
            raise ValueError(f"mu and log_std must have equal shapes, got {tuple(mu.weight.shape)} and {tuple(log_std.weight.shape)}")
        if any(p.dtype != torch.float32 for m in (mu, log_std) for p in m.parameters()):
            raise ValueError("FusedMLP needs float32 parameters")
        if (mu.bias is None) != (log_std.bias is None):
            raise ValueError("mu and log_std must both have a bias or both have none")
        lo_, hi_ = float(log_std_bounds[0]), float(log_std_bounds[1])
        if not lo_ <= hi_:
            raise ValueError("log_std_bounds must be (min, max) with min <= max")
        A = int(mu.weight.shape[0])
        fused = torch.nn.Linear(int(mu.weight.shape[1]), 2 * A, bias=mu.bias is not None, device=mu.weight.device)
        self = cls(torch.nn.Sequential(*list(latent), fused), clamp=None, backend=backend)
        self.module = None                               # (the fused layer is the wrapper's own: its values come from the heads)
        self.head, self.log_std_bounds, self._heads = N.MLP_HEAD_SQUASHED_GAUSSIAN, (lo_, hi_), (mu, log_std)
        self.latent = list(latent)
        self._fused = fused.requires_grad_(False)
        self._heads_seen = None
        self.out_dim = A
        self.refresh(force=True)
        return self

    @classmethod
    def from_sb3(cls, policy, clamp=None, backend=None, stochastic=False):
        """``stochastic=True``: the actor an SB3 ``SACPolicy`` SAMPLES from while it learns, as ``squashed_gaussian(actor.latent_pi,
        actor.mu, actor.log_std)`` with SB3's ``LOG_STD_MIN`` / ``LOG_STD_MAX`` (-20, 2); ``use_sde`` (gSDE) actors are refused, and so
        are policies without ``actor.log_std`` (PPO's Gaussian has a state-independent deviation: ``DeviceRollout(action_noise=True)``
        with pre-scaled draws is exact for it).  ``clamp`` is not taken here: the box is what each call passes.
        ``stochastic=False`` (the default):

        The deterministic actor of a Stable-Baselines3 policy as a ``FusedMLP`` (duck-typed, SB3 itself is not imported):
        ``ActorCriticPolicy`` (PPO / A2C ``MlpPolicy``): ``mlp_extractor.policy_net`` followed by ``action_net`` -- the mean of
        the Gaussian, which SB3 clips to the action box (pass ``clamp``); ``SACPolicy``: ``actor.latent_pi`` + ``actor.mu`` with
        the tanh squashing of ``actor.forward(deterministic=True)``; ``TD3Policy``: ``actor.mu`` alone (a Sequential that already
        ends in Tanh -- its actor has no ``latent_pi``).  The wrapper shares the parameters
        with ``policy`` (no copy), so ``model.learn()`` steps are picked up by ``refresh()``.  Observations must already be
        flat vectors (``FlattenExtractor``), which is what ``MlpPolicy`` uses on these environments."""
        import torch
        if stochastic:
            actor = getattr(policy, "actor", None)
            if actor is None or not (hasattr(actor, "mu") and hasattr(actor, "log_std")):
                raise ValueError("stochastic=True expects an SB3 SACPolicy (actor.latent_pi, actor.mu, actor.log_std)")
            if getattr(actor, "use_sde", False):
                raise ValueError("stochastic=True: gSDE actors (use_sde=True) are not supported")
            if clamp is not None:
                raise ValueError("stochastic=True: the action box is the clamp each call passes, not a property of the wrapper")
            lat = getattr(actor, "latent_pi", None)
            return cls.squashed_gaussian(list(lat) if lat is not None else [], actor.mu, actor.log_std, (-20.0, 2.0), backend=backend)
        if hasattr(policy, "mlp_extractor") and hasattr(policy, "action_net"):
            mods = list(policy.mlp_extractor.policy_net) + [policy.action_net]
        elif hasattr(policy, "actor") and hasattr(policy.actor, "mu"):
            head = policy.actor.mu
            lat = getattr(policy.actor, "latent_pi", None)
            mods = (list(lat) if lat is not None else []) + (list(head) if isinstance(head, torch.nn.Sequential) else [head])
            if not isinstance(mods[-1], torch.nn.Tanh):
                mods.append(torch.nn.Tanh())          # SAC squashes the mean; TD3's mu already ends in Tanh
        else:
            raise ValueError("expected an SB3 ActorCriticPolicy (mlp_extractor + action_net) or SAC/TD3 policy (actor.mu, with actor.latent_pi in front for SAC)")
        return cls(torch.nn.Sequential(*mods), clamp=clamp, backend=backend)

    def refresh(self, force: bool = False):
        """Bring the transposed weight copies up to date with the module's parameters (in-place updates such as optimizer
        steps bump a tensor's version counter).  Not callable while a hipGraph is being captured."""
        import torch
        with torch.no_grad():
            if self._heads is not None:      # the fused last layer [mu; log_std]: rewritten in place when any of the four tensors changed
                mu, ls = self._heads
                seen = tuple(p._version for m in (mu, ls) for p in (m.weight, m.bias) if p is not None)
                if force or seen != self._heads_seen:
                    A = mu.weight.shape[0]
                    self._fused.weight[:A].copy_(mu.weight.detach())
                    self._fused.weight[A:].copy_(ls.weight.detach())
                    if mu.bias is not None:
                        self._fused.bias[:A].copy_(mu.bias.detach())
                        self._fused.bias[A:].copy_(ls.bias.detach())
                    self._heads_seen = seen
            for i, (w, _, _) in enumerate(self.layers):
                if force or w._version != self._seen[i]:
                    out_dim, in_dim = w.shape
                    k4 = (in_dim + 3) // 4
                    padded = torch.nn.functional.pad(w.detach(), (0, 4 * k4 - in_dim))      # [out, 4 k4], zeros past in_dim
                    self._wt[i].permute(1, 0, 2).copy_(padded.view(out_dim, k4, 4))        # write through the [out, k4, 4] view
                    self._seen[i] = w._version
        return self

    def _net(self, clamp, x_f64=False, y_f64=False, plain=False) -> N.Mlp:
        """``plain``: the descriptor of the bare layers, whatever the wrapper's head (what ``with_grad`` evaluates and differentiates)."""
        net = N.Mlp()
        net.x_f64, net.y_f64 = int(x_f64), int(y_f64)
        net.n_layers = len(self.layers)
        if self.head == N.MLP_HEAD_SQUASHED_GAUSSIAN and not plain:
            if clamp is None:
                raise ValueError("a squashed-Gaussian head needs clamp=(lo, hi), the action box its output is rescaled to")
            if not float(clamp[0]) < float(clamp[1]):
                raise ValueError("a squashed-Gaussian head needs an action box (lo, hi) with lo < hi")
            net.head, (net.log_std_min, net.log_std_max) = self.head, self.log_std_bounds
        net.clamp = 0 if clamp is None else 1
        net.lo, net.hi = (0.0, 0.0) if clamp is None else (float(clamp[0]), float(clamp[1]))
        for i, (w, b, act) in enumerate(self.layers):
            L = net.layer[i]
            L.w, L.b = self._wt[i].data_ptr(), (b.data_ptr() if b is not None else None)
            L.in_dim, L.out_dim, L.act = int(w.shape[1]), int(w.shape[0]), act
        return net

    # ---- the policy inside a rollout kernel (pdegym_*_rollout with ``policy`` set: 1D, traffic and brain-tumour engines) ---------
    def fits_rollout(self, in_dim: int, out_dim: int, extra_lds_bytes: int = 0) -> bool:
        """Whether a rollout kernel can evaluate this network on rows of ``in_dim`` values for ``out_dim`` commands (the engines'
        ``policy_fits_rollout`` ask through ``fits_rollout_kernel``; having this method is the test for a ``FusedMLP``): those
        sizes, layers of at most 256 units.  Layers of at most 64 units: one neuron per lane, the weights + 16 observation rows
        within 160 KB of LDS.  A layer of 65 .. 256 units (SB3's 256-256 actors): the 16 waves of a workgroup evaluate the network
        together on the matrix cores, weights streamed from L2 -- bit-identical to ``pdegym_mlp_forward`` (16 observation rows +
        the hidden rows within 160 KB of LDS: any row the kernels take).  ``extra_lds_bytes``: LDS of the engine's own per
        workgroup of 16 instances, which starts on the 16-byte boundary after the policy's (csrc/pdegym_policy.h: plan)."""
        dims = [(int(w.shape[1]), int(w.shape[0])) for w, _, _ in self.layers]
        if dims[0][0] != in_dim or self.out_dim != out_dim or any(o > 256 for _, o in dims):
            return False
        return (self.rollout_lds_bytes(in_dim) + 15) // 16 * 16 + extra_lds_bytes <= self.ROLLOUT_LDS_BYTES

    ROLLOUT_LDS_BYTES = 160 * 1024      # csrc/pdegym_policy.h: kMaxLdsBytes

    def rollout_lds_bytes(self, in_dim: int) -> int:
        """LDS bytes the in-kernel evaluation takes per workgroup of 16 instances (csrc/pdegym_policy.h: wide_lds_floats, over
        pdegym_mlp_tile.h: lds_stride, for a layer of more than 64 units; lds_floats otherwise).  An engine whose rollout kernel keeps
        LDS rows of its own (the brain-tumour engine) adds them to this figure."""
        dims = [(int(w.shape[1]), int(w.shape[0])) for w, _, _ in self.layers]
        if any(o > 64 for _, o in dims):
            stride = lambda w: (w + 63) // 64 * 64 + 4                  # noqa: E731
            kept = 64 if self.head == N.MLP_HEAD_SQUASHED_GAUSSIAN else 32       # wide_kept: [mu; log_std] of two commands per row
            floats = 16 * (stride((in_dim + 15) // 16 * 16) + 2 * stride(256)) + kept
        else:
            floats = sum((((i + 3) // 4) | 1) * 4 * o + 64 for i, o in dims) + 16 * (((in_dim + 3) // 4) * 4 + 128)
        return 4 * floats

    def rollout_net(self, obs, actions, clamp="default", noise=None) -> N.Mlp:
        """The descriptor for a rollout that reads ``obs`` and writes ``actions`` ([T, B] or [T, B, A]): weights refreshed (unless
        capturing), ``clamp`` (default: the policy's own), and ``noise`` -- float32, contiguous, the actions' shape -- added to
        the network output of step t before the clamp.  Squashed-Gaussian head: ``noise`` holds the standard-normal draws ``eps`` and
        the clamp is the action box (required)."""
        import torch
        self._refresh_unless_capturing(obs)
        net = self._net(self.clamp if clamp == "default" else clamp)
        if noise is not None:
            if noise.dtype != torch.float32 or tuple(noise.shape) != tuple(actions.shape) or not noise.is_contiguous():
                raise ValueError("noise must be a contiguous float32 tensor of the actions' shape")
            net.noise, net.noise_stride = noise.data_ptr(), (1 if actions.dim() == 2 else int(actions.shape[2]))
        return net

    def _check_index(self, x, index, tail, tail_indexed, rows, what):
        """``index`` as the rows of the storage ``x`` [M, D] a call reads: a contiguous int64 [N] tensor on x's device, on a backend with
        the gather entry points, without ``rows=``; ``tail_indexed`` only with an index and a tail.  Returns N (x's rows without index)."""
        import torch
        if index is None:
            if tail_indexed:
                raise ValueError(f"FusedMLP.{what}: tail_indexed=True needs index=")
            return x.shape[0]
        if not (hasattr(self.backend, "mlp_forward_gather") and hasattr(self.backend, "mlp_backward_gather")):
            raise ValueError(f"FusedMLP.{what}: index= needs a backend with mlp_forward_gather / mlp_backward_gather, "
                             f"{type(self.backend).__name__} has none")
        if rows is not None:
            raise ValueError(f"FusedMLP.{what}: rows= and index= do not combine (the masked launch reads row b)")
        if not torch.is_tensor(index) or index.dtype != torch.int64 or index.dim() != 1 or not index.is_contiguous():
            raise ValueError(f"FusedMLP.{what}: index must be a contiguous int64 [N] tensor")
        if index.device != x.device:
            raise ValueError(f"FusedMLP.{what}: index is on {index.device}, the observations on {x.device}")
        if tail_indexed and tail is None:
            raise ValueError(f"FusedMLP.{what}: tail_indexed=True needs tail=")
        return index.shape[0]

    def _check_tail(self, x, tail, what, rows=None):
        """``tail`` as the second part of the rows whose first part is ``x`` [B, D]: float32 [B, n2] on x's device, 1 <= n2 <= 8, the
        widths adding up to ``in_dim``; on a backend with the two-part entry points.  ``ValueError`` otherwise.  ``rows``: the rows the
        tail must have when they are not x's (a call with ``index``)."""
        import torch
        if not (hasattr(self.backend, "mlp_forward_cat") and hasattr(self.backend, "mlp_backward_cat")):
            raise ValueError(f"FusedMLP.{what}: tail= needs a backend with mlp_forward_cat / mlp_backward_cat, {type(self.backend).__name__} has none")
        if rows is not None and (not torch.is_tensor(tail) or tail.dim() != 2 or tail.shape[0] != rows):
            raise ValueError(f"FusedMLP.{what}: tail must be a [{rows}, n2] tensor (the index's N rows, or the storage's M with tail_indexed)")
        if rows is None and (not torch.is_tensor(tail) or tail.dim() != 2 or tail.shape[0] != x.shape[0]):
            raise ValueError(f"FusedMLP.{what}: tail must be a [B, n2] tensor with the observations' B = {x.shape[0]}")
        if tail.dtype != torch.float32:
            raise ValueError(f"FusedMLP.{what}: tail must be float32, got {tail.dtype}")
        if tail.device != x.device:
            raise ValueError(f"FusedMLP.{what}: tail is on {tail.device}, the observations on {x.device}")
        if not 1 <= tail.shape[1] <= 8:
            raise ValueError(f"FusedMLP.{what}: tail must have 1..8 columns, got {tail.shape[1]}")
        if x.shape[1] + tail.shape[1] != self.in_dim:
            raise ValueError(f"observation rows have {x.shape[1]} entries and tail rows {tail.shape[1]}, the network takes {self.in_dim}")

    def forward_into(self, obs, out, clamp="default", noise=None, tail=None, rows=None, rows_not=None, index=None, tail_indexed=False):
        """``index`` (contiguous int64 [N] on the observations' device): ``obs`` is a STORAGE of M rows -- a replay buffer's or a
        rollout's observations -- and row b of the call is ``obs[index[b]]``, read in place by the first layer
        (pdegym_mlp_forward_gather: no ``obs[index]`` copy); ``out`` and ``noise`` have N rows, ``tail`` N rows too, or the storage's M with
        ``tail_indexed=True`` (row b's tail is then ``tail[index[b]]``: the stored actions).  Bits: those of the call on the gathered
        rows.  An entry outside [0, M) is never an address: its row of ``out`` is NaN.  Not with ``rows=``.  Inside a stream capture
        the ADDRESS of ``index`` is baked into the graph: keep one static index tensor and copy each minibatch's indices into it.

        ``tail`` (float32 [B, n2], n2 <= 8): the rows are ``[obs | tail]``, read from the two tensors as they are -- SB3's
        ``critic(obs, actions)`` -- with the bits of the call on ``torch.cat([obs, tail], 1)``.  Without it:

        out[b, :] = net(obs[b, :]); ``obs`` [B, in_dim] (any trailing shape that flattens to in_dim), ``out`` [B, out_dim]
        or [B] when out_dim == 1, on the parameters' device.  float64 observations (traffic, tumour, float64 Navier-Stokes)
        are rounded to float32 as they are read and a float64 ``out`` receives the widened float32 result -- the casts SB3
        makes around its float32 policy.  ``noise`` (float32, same shape as the action): added to the network output before
        the clamp -- the caller's pre-scaled exploration noise of a Gaussian policy.  Returns ``out``.
        A NaN observation propagates as in PyTorch (the row's output is NaN) and the clamp keeps a NaN like ``torch.clamp`` /
        ``np.clip``; +-Inf is clamped to the bound (include/pdegym.h, conventions).  Squashed-Gaussian head (``squashed_gaussian``):
        ``noise`` is ``eps`` (standard-normal draws; None: the deterministic actor), ``clamp`` the action box (required), and
        ``out_dim`` <= 8.

        ``rows`` (uint8 [B], with ``rows_not`` uint8 [B] or None): only the rows with ``rows[b] != 0 and rows_not[b] == 0`` are
        evaluated and stored (pdegym_mlp_forward_masked) -- the other rows of ``out`` are left as they are, a stored row has the
        bits of the unmasked call, and what the other rows of ``obs`` hold (NaN included) does not matter.  No compaction, no
        allocation, no synchronisation: V(terminal observation) on the truncated rows of a rollout inside a captured graph.  Plain
        head, float32 ``out``, no ``noise``, no ``tail``."""
        x = obs.reshape(obs.shape[0], -1)
        B = self._check_index(x, index, tail, tail_indexed, rows if rows is not None else rows_not, "forward_into")
        if tail is not None:
            self._check_tail(x, tail, "forward_into", rows=None if index is None else (x.shape[0] if tail_indexed else B))
        elif x.shape[1] != self.in_dim:
            raise ValueError(f"observation rows have {x.shape[1]} entries, the network takes {self.in_dim}")
        y = out.reshape(B, self.out_dim)
        if y.data_ptr() != out.data_ptr():
            raise ValueError("out must be viewable as [B, out_dim] without a copy")
        import torch
        self._refresh_unless_capturing(x)
        for t_, name in ((x, "obs"), (y, "out")):
            if t_.dtype not in (torch.float32, torch.float64):
                raise N.NativeError(f"FusedMLP: {name} must be float32 or float64, got {t_.dtype}")
        net = self._net(self.clamp if clamp == "default" else clamp, x.dtype == torch.float64, y.dtype == torch.float64)
        if noise is not None:       # exploration noise, added before the clamp (float32 [B, out_dim] or [B] when out_dim == 1)
            nz = noise.reshape(B, self.out_dim)
            if nz.dtype != torch.float32 or nz.device != x.device or nz.stride(1) != 1 or nz.data_ptr() != noise.data_ptr():
                raise ValueError("noise must be a float32 tensor on the observations' device, viewable as [B, out_dim]")
            net.noise, net.noise_stride = nz.data_ptr(), nz.stride(0)
        if rows is not None or rows_not is not None:
            if rows is None:
                raise ValueError("rows_not knocks rows out of `rows`: give rows")
            if tail is not None or noise is not None or net.head != N.MLP_HEAD_PLAIN or y.dtype != torch.float32:
                raise ValueError("forward_into(rows=...) takes the plain head and a float32 out, without noise or tail")
            for m, name in ((rows, "rows"), (rows_not, "rows_not")):
                if m is not None and (m.dtype != torch.uint8 or m.numel() != B or m.device != x.device or not m.is_contiguous()):
                    raise ValueError(f"{name} must be a contiguous uint8 tensor of {B} flags on the observations' device")
            self.backend.mlp_forward(net, x, y, B, rows=rows.reshape(B), rows_not=None if rows_not is None else rows_not.reshape(B))
        elif index is not None:
            self.backend.mlp_forward_gather(net, _rows(x), None if tail is None else _rows(tail), index, y, B, x2_indexed=bool(tail_indexed))
        elif tail is not None:
            self.backend.mlp_forward_cat(net, x, _rows(tail), y, B)
        else:
            self.backend.mlp_forward(net, x, y, B)
        return out

    # ---- the differentiable evaluation (pdegym_mlp_forward + pdegym_mlp_backward / _wide) ---------------------------------------------
    def backward_limit(self):
        """None when ``pdegym_mlp_backward`` takes this network, otherwise the limit it breaks, in words."""
        for i, (w, _, _) in enumerate(self.layers):
            if w.shape[0] > N.MLP_BACKWARD_MAX_WIDTH:
                return f"layer {i} has {w.shape[0]} units, the backward pass takes at most {N.MLP_BACKWARD_MAX_WIDTH} per layer"
        if self.in_dim > N.MLP_BACKWARD_MAX_INPUT:
            return f"rows of {self.in_dim} inputs, the backward pass takes at most {N.MLP_BACKWARD_MAX_INPUT}"
        return None

    def fits_backward(self) -> bool:
        """Whether ``with_grad`` can differentiate this network: every layer of at most 64 units, rows of at most 1024 inputs."""
        return self.backward_limit() is None

    def wide_backward_limit(self):
        """None when ``pdegym_mlp_backward_wide`` takes this network, otherwise the limit it breaks, in words."""
        for i, (w, _, _) in enumerate(self.layers):
            if w.shape[0] > N.MLP_BACKWARD_WIDE_MAX_WIDTH:
                return f"layer {i} has {w.shape[0]} units, the wide backward pass takes at most {N.MLP_BACKWARD_WIDE_MAX_WIDTH} per layer"
        if self.in_dim > N.MLP_BACKWARD_WIDE_MAX_INPUT:
            return f"rows of {self.in_dim} inputs, the wide backward pass takes at most {N.MLP_BACKWARD_WIDE_MAX_INPUT}"
        return None

    def fits_backward_wide(self) -> bool:
        """Whether ``pdegym_mlp_backward_wide`` can differentiate this network: every layer of at most 256 units, rows of at most 1024
        inputs (a superset of ``fits_backward()``; ``with_grad`` uses it for the networks that do not fit the narrow pass)."""
        return self.wide_backward_limit() is None

    def _backward_entry(self):
        """The backend method behind ``with_grad``'s backward: ``mlp_backward`` for a network that ``fits_backward()``, otherwise
        ``mlp_backward_wide`` where the backend offers it and the network ``fits_backward_wide()``, otherwise None."""
        if self.fits_backward():
            return self.backend.mlp_backward
        wide = getattr(self.backend, "mlp_backward_wide", None)
        return wide if wide is not None and self.fits_backward_wide() else None

    def grad_parameters(self):
        """The Parameters ``with_grad`` returns gradients for, in its order: weight, bias (if any) of every layer of the wrapped
        module; with a squashed-Gaussian head the latent layers' followed by those of ``mu`` and of ``log_std``."""
        own = self.layers[:-1] if self._heads is not None else self.layers
        ps = [p for w, b, _ in own for p in (w, b) if p is not None]
        if self._heads is not None:
            ps += [p for m in self._heads for p in (m.weight, m.bias) if p is not None]
        return ps

    def with_grad(self, obs, tail=None, params=True, index=None, tail_indexed=False):
        """``index`` (contiguous int64 [N] on the observations' device): ``obs`` is a storage of M rows and row b of the call is
        ``obs[index[b]]``, read in place by the forward AND the backward launches (pdegym_mlp_forward_gather, pdegym_mlp_backward_gather /
        _wide_gather); what is saved for the backward is the storage and the index themselves, never a copy of the rows.  ``tail`` has N
        rows, or M with ``tail_indexed=True``.  The storage receives no gradient (it would be a scatter-add over duplicated entries):
        ``ValueError`` when ``obs`` requires grad, and when ``tail`` does with ``tail_indexed``; a dense ``tail`` that requires grad gets its
        ``[N, n2]`` gradient (SAC's actor step: stored observation, fresh action).  Bits: those of the call on the gathered rows.  Inside
        a stream capture the ADDRESS of ``index`` is baked into the graph: keep one static index tensor and copy each minibatch's
        indices into it.

        ``tail`` (float32 [B, n2], n2 <= 8): the rows are ``[obs | tail]`` -- SB3's ``critic(obs, actions)`` -- and ``tail`` receives its
        own ``[B, n2]`` gradient when it requires grad (``obs``, float32 and requiring grad, the ``[B, D]`` one of the first part: no
        full-width dx exists).  ``params=False``: no gradient goes to ``grad_parameters()`` and the backward is ONE launch that forms
        none (the critic pass of SAC's actor step); the same pass runs when no parameter requires grad.  Bits: those of the call on
        ``torch.cat([obs, tail], 1)``.  ``ValueError`` on a backend without the two-part entry points.  Without the two arguments:

        ``[B, n]`` float32 WITH a ``grad_fn``: the last layer's output (no clamp, no noise, no head: a squashed-Gaussian wrapper
        returns the raw ``[B, 2A]`` rows -- mu columns, then log_std columns -- and SAC's torch code applies clip / exp / tanh under
        autograd).  Forward: one ``pdegym_mlp_forward`` launch after ``refresh()``; backward: ``pdegym_mlp_backward`` for a network
        that ``fits_backward()``, ``pdegym_mlp_backward_wide`` for a wider one that ``fits_backward_wide()``; either returns the
        gradients of ``grad_parameters()`` -- so ``loss.backward()`` fills (accumulates into) the ``.grad`` of the module's own
        Parameters and any torch optimiser works unchanged -- and of ``obs`` when it is float32 and requires grad.  The activations
        are recomputed in the backward launch, nothing is kept but ``obs``.  ``ValueError`` when the network fits neither pass (or
        does not ``fits_backward()`` on a backend without the wide pass), naming the limit of ``backward_limit()``; ``RuntimeError`` inside a stream capture (``refresh()`` cannot run there: a captured update would
        train on stale weight copies) -- unless the wrapper is attached to a ``pde_control_gym.FusedAdam``, whose step writes the
        copies itself: ``refresh()`` is then skipped inside the capture and forward, loss, backward and step make one graph."""
        import torch
        if self._backward_entry() is None:
            raise ValueError(f"FusedMLP.with_grad: {self.backward_limit()}")
        x = obs.reshape(obs.shape[0], -1)
        B = self._check_index(x, index, tail, tail_indexed, None, "with_grad")
        if tail is not None:
            self._check_tail(x, tail, "with_grad", rows=None if index is None else (x.shape[0] if tail_indexed else B))
        elif x.shape[1] != self.in_dim:
            raise ValueError(f"observation rows have {x.shape[1]} entries, the network takes {self.in_dim}")
        if x.dtype not in (torch.float32, torch.float64):
            raise ValueError(f"FusedMLP.with_grad: obs must be float32 or float64, got {x.dtype}")
        if index is not None and obs.requires_grad:
            raise ValueError("FusedMLP.with_grad: obs requires grad and is read by index: a gradient of gathered rows would be a scatter-add")
        if tail_indexed and tail.requires_grad:
            raise ValueError("FusedMLP.with_grad: tail requires grad and is read by index (tail_indexed=True)")
        two_part = hasattr(self.backend, "mlp_forward_cat") and hasattr(self.backend, "mlp_backward_cat")
        if not params and not two_part:
            raise ValueError(f"FusedMLP.with_grad: params=False needs a backend with mlp_backward_cat, {type(self.backend).__name__} has none")
        if x.is_cuda and torch.cuda.is_current_stream_capturing():
            if self._optimizer is None:      # (attached: the optimiser's own launch writes the copies, there is nothing to refresh)
                raise RuntimeError("FusedMLP.with_grad cannot run inside a stream capture: refresh() has to see the optimiser's last step")
        else:
            self.refresh()
        ps = self.grad_parameters()
        if index is not None:
            if not params:
                ps = [p.detach() for p in ps]
            return _with_grad_function(gather=True).apply(self, bool(params), x, tail, index, bool(tail_indexed), *ps)
        if tail is not None or not params or (two_part and not any(p.requires_grad for p in ps)):
            if not params:      # detached: no edge to the parameters (saved all the same: a backward after an in-place step is refused)
                ps = [p.detach() for p in ps]
            return _with_grad_function(cat=True).apply(self, bool(params), x, tail, *ps)
        return _with_grad_function().apply(self, x, *ps)

    def __call__(self, obs, tail=None, index=None, tail_indexed=False):
        """``forward_into`` with a fresh ``out`` of the observations' dtype: [B, out_dim], or [N, out_dim] with ``index`` [N]."""
        import torch
        n = obs.shape[0] if index is None or not torch.is_tensor(index) else index.shape[0]
        out = torch.empty(n, self.out_dim, dtype=obs.dtype, device=obs.device)
        return self.forward_into(obs, out, tail=tail, index=index, tail_indexed=tail_indexed)      # (squashed-Gaussian head: a ValueError -- it has no default box; use forward_into)


def _rows(t):
    """``t`` [B, n] detached, with unit inner stride and rows that do not overlap (what the entry points take), copied only if not."""
    t = t.detach()
    if t.stride(1) != 1 or (t.shape[0] > 1 and t.stride(0) < t.shape[1]):
        t = t.contiguous()
    return t


_function = _cat_function = _gather_function = None


def _with_grad_function(cat=False, gather=False):
    """The ``torch.autograd.Function`` behind ``FusedMLP.with_grad`` (built on first use: this module imports torch lazily).  ``cat``:
    the one behind ``with_grad(obs, tail, params)``, on the two-part entry points; ``gather``: the one behind ``with_grad(..., index=)``."""
    global _function, _cat_function, _gather_function
    if _function is not None:
        return _gather_function if gather else (_cat_function if cat else _function)
    import torch

    class FusedMLPFunction(torch.autograd.Function):
        @staticmethod
        def forward(ctx, policy, x, *params):
            xd = x.detach()
            if xd.stride(1) != 1 or (xd.shape[0] > 1 and xd.stride(0) < xd.shape[1]):
                xd = xd.contiguous()
            n_out = int(policy.layers[-1][0].shape[0])
            y = torch.empty(xd.shape[0], n_out, dtype=torch.float32, device=xd.device)
            policy.backend.mlp_forward(policy._net(None, xd.dtype == torch.float64, plain=True), xd, y, xd.shape[0])
            ctx.policy, ctx.want_dx = policy, bool(ctx.needs_input_grad[1]) and x.dtype == torch.float32
            ctx.save_for_backward(xd, *params)      # (the parameters: autograd refuses a backward after they changed in place)
            return y

        @staticmethod
        def backward(ctx, dy):
            policy = ctx.policy
            xd = ctx.saved_tensors[0]
            dy = dy.to(torch.float32).contiguous()
            weights = [w.detach() for w, _, _ in policy.layers]
            dw = [torch.empty_like(w) for w in weights]
            db = [None if b is None else torch.empty_like(b.detach()) for _, b, _ in policy.layers]
            dx = torch.empty(xd.shape, dtype=torch.float32, device=xd.device) if ctx.want_dx else None
            policy._backward_entry()(policy._net(None, xd.dtype == torch.float64, plain=True), xd, dy, weights, dw, db, dx)
            heads = policy._heads is not None
            grads = [g for w_, b_ in zip(dw[:-1] if heads else dw, db[:-1] if heads else db) for g in (w_, b_) if g is not None]
            if heads:      # rows 0 .. A-1 of the fused last layer are mu's, rows A .. 2A-1 log_std's
                A = dw[-1].shape[0] // 2
                for rows in (slice(0, A), slice(A, 2 * A)):
                    grads += [dw[-1][rows]] + ([db[-1][rows]] if db[-1] is not None else [])
            wanted = ctx.needs_input_grad[2:]
            return (None, dx) + tuple(g if need else None for g, need in zip(grads, wanted))

    class FusedMLPCatFunction(torch.autograd.Function):
        @staticmethod
        def forward(ctx, policy, params, x, tail, *ps):
            xd, td = _rows(x), (None if tail is None else _rows(tail))
            n_out = int(policy.layers[-1][0].shape[0])
            y = torch.empty(xd.shape[0], n_out, dtype=torch.float32, device=xd.device)
            net = policy._net(None, xd.dtype == torch.float64, plain=True)
            if td is None:
                policy.backend.mlp_forward(net, xd, y, xd.shape[0])
            else:
                policy.backend.mlp_forward_cat(net, xd, td, y, xd.shape[0])
            ctx.policy = policy
            ctx.want_dx = bool(ctx.needs_input_grad[2]) and x.dtype == torch.float32
            ctx.want_dx2 = td is not None and bool(ctx.needs_input_grad[3])
            ctx.want_params = params and any(ctx.needs_input_grad[4:])
            ctx.has_tail = td is not None
            ctx.save_for_backward(xd, *(() if td is None else (td,)), *ps)
            return y

        @staticmethod
        def backward(ctx, dy):
            policy = ctx.policy
            xd, td = ctx.saved_tensors[0], (ctx.saved_tensors[1] if ctx.has_tail else None)
            none = (None,) * (4 + len(ctx.needs_input_grad[4:]))
            if not (ctx.want_params or ctx.want_dx or ctx.want_dx2):
                return none
            dy = dy.to(torch.float32).contiguous()
            weights = [w.detach() for w, _, _ in policy.layers]
            dw = db = None
            if ctx.want_params:
                dw = [torch.empty_like(w) for w in weights]
                db = [None if b is None else torch.empty_like(b.detach()) for _, b, _ in policy.layers]
            dx = torch.empty(xd.shape, dtype=torch.float32, device=xd.device) if ctx.want_dx else None
            dx2 = torch.empty(td.shape, dtype=torch.float32, device=td.device) if ctx.want_dx2 else None
            policy.backend.mlp_backward_cat(policy._net(None, xd.dtype == torch.float64, plain=True), xd, td, dy, weights, dw, db, dx, dx2,
                                            params=ctx.want_params, wide=not policy.fits_backward())
            if not ctx.want_params:
                return (None, None, dx, dx2) + none[4:]
            heads = policy._heads is not None
            grads = [g for w_, b_ in zip(dw[:-1] if heads else dw, db[:-1] if heads else db) for g in (w_, b_) if g is not None]
            if heads:      # rows 0 .. A-1 of the fused last layer are mu's, rows A .. 2A-1 log_std's
                A = dw[-1].shape[0] // 2
                for rows in (slice(0, A), slice(A, 2 * A)):
                    grads += [dw[-1][rows]] + ([db[-1][rows]] if db[-1] is not None else [])
            return (None, None, dx, dx2) + tuple(g if need else None for g, need in zip(grads, ctx.needs_input_grad[4:]))

    class FusedMLPGatherFunction(torch.autograd.Function):
        @staticmethod
        def forward(ctx, policy, params, x, tail, index, tail_indexed, *ps):
            xd, td = _rows(x), (None if tail is None else _rows(tail))
            n_out = int(policy.layers[-1][0].shape[0])
            y = torch.empty(index.shape[0], n_out, dtype=torch.float32, device=xd.device)
            policy.backend.mlp_forward_gather(policy._net(None, xd.dtype == torch.float64, plain=True), xd, td, index, y, index.shape[0],
                                              x2_indexed=tail_indexed)
            ctx.policy, ctx.tail_indexed, ctx.has_tail = policy, tail_indexed, td is not None
            ctx.want_dx2 = td is not None and not tail_indexed and bool(ctx.needs_input_grad[3])
            ctx.want_params = params and any(ctx.needs_input_grad[6:])
            ctx.save_for_backward(xd, index, *(() if td is None else (td,)), *ps)      # the storage and the index: no copy of the rows
            return y

        @staticmethod
        def backward(ctx, dy):
            policy = ctx.policy
            xd, index, td = ctx.saved_tensors[0], ctx.saved_tensors[1], (ctx.saved_tensors[2] if ctx.has_tail else None)
            none = (None,) * (6 + len(ctx.needs_input_grad[6:]))
            if not (ctx.want_params or ctx.want_dx2):
                return none
            dy = dy.to(torch.float32).contiguous()
            weights = [w.detach() for w, _, _ in policy.layers]
            dw = db = None
            if ctx.want_params:
                dw = [torch.empty_like(w) for w in weights]
                db = [None if b is None else torch.empty_like(b.detach()) for _, b, _ in policy.layers]
            dx2 = torch.empty(td.shape, dtype=torch.float32, device=td.device) if ctx.want_dx2 else None
            policy.backend.mlp_backward_gather(policy._net(None, xd.dtype == torch.float64, plain=True), xd, td, index, dy, weights, dw, db, dx2,
                                               params=ctx.want_params, wide=not policy.fits_backward(), x2_indexed=ctx.tail_indexed)
            if not ctx.want_params:
                return (None, None, None, dx2) + none[4:]
            heads = policy._heads is not None
            grads = [g for w_, b_ in zip(dw[:-1] if heads else dw, db[:-1] if heads else db) for g in (w_, b_) if g is not None]
            if heads:      # rows 0 .. A-1 of the fused last layer are mu's, rows A .. 2A-1 log_std's
                A = dw[-1].shape[0] // 2
                for rows in (slice(0, A), slice(A, 2 * A)):
                    grads += [dw[-1][rows]] + ([db[-1][rows]] if db[-1] is not None else [])
            return (None, None, None, dx2, None, None) + tuple(g if need else None for g, need in zip(grads, ctx.needs_input_grad[6:]))

    _function, _cat_function, _gather_function = FusedMLPFunction, FusedMLPCatFunction, FusedMLPGatherFunction
    return _gather_function if gather else (_cat_function if cat else _function)
