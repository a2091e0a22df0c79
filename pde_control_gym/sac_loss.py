"""The losses of a SAC update step on the device: from the outputs of actor and critics to the gradients with respect to those
outputs in a handful of launches (pdegym_squashed_gaussian_sample, its backward, pdegym_sac_critic_loss, pdegym_sac_actor_loss),
with the statistics SB3's ``SAC.train`` logs.

The reference's users train with SB3's ``SAC("MlpPolicy", env)`` (examples/transportPDE/transport1Dsac.py).  Between the networks'
outputs and the three ``backward()`` calls that update is some sixty elementwise launches on device tensors -- clamp, exp, tanh, the
Gaussian term, ``log(1 - a * a + 1e-6)``, the sums, three ``cat``, the gathers of rewards and dones, two ``min``, the target, the MSE
terms, the means -- and the mirror image of each under autograd.  ``SACLoss`` restates it (include/pdegym.h) for the
``SquashedDiagGaussianDistribution`` of ``MlpPolicy`` and one or two Q critics:

    head = SACLoss(gamma=0.99, target_entropy=-1.0)
    block2, logp2 = head.sample(raw_fn(o2), eps2, obs=o2)                    # under torch.no_grad(): [o2 | a2], log pi(a2 | o2)
    result = head.critic(q1(oa), q2(oa), q1_t(block2), q2_t(block2), logp2, rewards, dones, log_alpha, index=mb)
    result.backward()                                                        # one autograd call into both critics
    block, logp = head.sample(raw_fn(o), eps, obs=o)                         # an autograd node over two launches
    result = head.actor(q1(block), q2(block), logp, log_alpha)
    result.backward()                                                        # one autograd call; log_alpha.grad accumulated
"""
from __future__ import annotations

CRITIC_STATS = ("critic_loss", "q1_mean", "q2_mean", "target_mean")
ACTOR_STATS = ("actor_loss", "ent_coef_loss", "alpha", "log_prob_mean")
MAX_ACTION_DIM = 8


def _accumulate(leaf_or_node, grad):
    """``grad`` into ``.grad`` of a leaf (accumulating, as autograd does) or into the graph that produced a non-leaf."""
    import torch
    t = leaf_or_node
    if not t.requires_grad:
        return
    if t.is_leaf:
        with torch.no_grad():
            g = grad.reshape(t.shape)
            t.grad = g.clone() if t.grad is None else t.grad.add_(g)
    else:
        torch.autograd.backward([t], [grad.reshape(t.shape)])


class SACCriticResult:
    """What ``SACLoss.critic`` returns: the statistics ``critic_loss``, ``q1_mean``, ``q2_mean``, ``target_mean`` as 0-d views of
    ONE device tensor ``stats`` (reading them makes no host synchronisation), ``grad_q1`` / ``grad_q2`` [N] (``grad_q2`` None with one
    critic) and ``target`` [N].  The tensors are the head's own and are overwritten by its next call with the same shapes."""

    def __init__(self, stats, grad_q1, grad_q2, target, q1, q2):
        self.stats, self.grad_q1, self.grad_q2, self.target = stats, grad_q1, grad_q2, target
        self._q1, self._q2 = q1, q2
        for i, name in enumerate(CRITIC_STATS):
            setattr(self, name, stats[i])

    def backward(self):
        """Send the gradients into the graphs that produced ``q1`` and ``q2``: ONE ``torch.autograd.backward`` call, so both
        critics' backward passes (``FusedMLP.with_grad`` or plain modules) run from it."""
        import torch
        roots, grads = [], []
        for t, g in ((self._q1, self.grad_q1), (self._q2, self.grad_q2)):
            if t is not None and t.requires_grad:
                roots.append(t)
                grads.append(g.reshape(t.shape))
        if roots:
            torch.autograd.backward(roots, grads)


class SACActorResult:
    """What ``SACLoss.actor`` returns: the statistics ``actor_loss``, ``ent_coef_loss``, ``alpha``, ``log_prob_mean`` as 0-d views of
    ONE device tensor ``stats``, ``grad_q1_pi`` / ``grad_q2_pi`` [N], ``grad_log_prob`` [1] (ONE scalar: the same for every row) and
    ``grad_log_alpha`` [1].  Overwritten by the head's next call with the same shapes."""

    def __init__(self, stats, grad_q1_pi, grad_q2_pi, grad_log_prob, grad_log_alpha, q1_pi, q2_pi, log_prob, log_alpha):
        self.stats, self.grad_q1_pi, self.grad_q2_pi = stats, grad_q1_pi, grad_q2_pi
        self.grad_log_prob, self.grad_log_alpha = grad_log_prob, grad_log_alpha
        self._q1_pi, self._q2_pi, self._log_prob, self._log_alpha = q1_pi, q2_pi, log_prob, log_alpha
        for i, name in enumerate(ACTOR_STATS):
            setattr(self, name, stats[i])

    def backward(self):
        """ONE ``torch.autograd.backward`` call with the roots ``[q1_pi, q2_pi, log_prob]`` -- the critics' backward passes hand
        their ``dx`` to the node of ``SACLoss.sample``, which receives ``grad_log_prob`` as a stride-0 view of the one scalar -- and
        then ``grad_log_alpha`` is accumulated into ``log_alpha.grad``.  The critics' own parameters collect gradients on the way, as
        they do in SB3's actor step: zero them before the next critic step."""
        import torch
        roots, grads = [], []
        for t, g in ((self._q1_pi, self.grad_q1_pi), (self._q2_pi, self.grad_q2_pi)):
            if t is not None and t.requires_grad:
                roots.append(t)
                grads.append(g.reshape(t.shape))
        lp = self._log_prob
        if lp.requires_grad:
            roots.append(lp)
            grads.append(self.grad_log_prob.expand(lp.shape))       # stride 0: no [N] tensor is filled
        if roots:
            torch.autograd.backward(roots, grads)
        _accumulate(self._log_alpha, self.grad_log_alpha)


class SACLoss:
    """``head = SACLoss(gamma, target_entropy, log_std_bounds=(-20, 2))`` with ``head.sample``, ``head.critic``, ``head.actor``
    (module docstring).  Everything float32 on one device; up to 8 action dimensions.

    Outputs are allocated at the first call with a shape and reused: a later call allocates nothing in its forward part and can be
    captured in a ``torch.cuda.graph``.  ``sample`` keeps separate outputs for calls with and without a graph, so the next-state
    sample made under ``torch.no_grad()`` survives the policy sample of the same shape."""

    def __init__(self, gamma: float, target_entropy: float, log_std_bounds=(-20.0, 2.0), backend=None):
        self.gamma, self.target_entropy = float(gamma), float(target_entropy)
        self.log_std_min, self.log_std_max = float(log_std_bounds[0]), float(log_std_bounds[1])
        if not self.log_std_min < self.log_std_max:
            raise ValueError(f"log_std_bounds must be (min, max) with min < max, got {log_std_bounds}")
        if backend is None:
            from pdecontrolgym_amd.backend import default_backend
            backend = default_backend()
        self.backend = backend
        self._buffers = {}

    @staticmethod
    def _rows(name, x, width, dev, dtype=None, rows=None):
        """``x`` detached as [rows, width] (width None: [rows]): a view, never a copy unless its inner stride is not 1."""
        import torch
        dtype = torch.float32 if dtype is None else dtype
        if not torch.is_tensor(x):
            raise ValueError(f"{name} must be a tensor, got {type(x).__name__}")
        if x.dtype != dtype:
            raise ValueError(f"{name} must be {dtype}, got {x.dtype}")
        if x.device != dev:
            raise ValueError(f"{name} is on {x.device}, expected {dev}: every tensor of a call lives on one device")
        x = x.detach()
        if width is None:
            if x.dim() == 2 and x.shape[1] == 1:
                x = x[:, 0]
            if x.dim() != 1:
                raise ValueError(f"{name} must be [rows] (or [rows, 1]), got {tuple(x.shape)}")
            x = x if x.shape[0] <= 1 or x.stride(0) == 1 else x.contiguous()
        else:
            if x.dim() == 1 and width == 1:
                x = x.unsqueeze(1)
            if x.dim() != 2 or x.shape[1] != width:
                raise ValueError(f"{name} must be [rows, {width}], got {tuple(x.shape)}")
            x = x if (width == 1 or x.stride(1) == 1) and (x.shape[0] <= 1 or x.stride(0) >= width) else x.contiguous()
        if rows is not None and x.shape[0] != rows:
            raise ValueError(f"{name} has {x.shape[0]} rows, expected {rows}")
        return x

    def _buffer(self, key, make):
        buf = self._buffers.get(key)
        if buf is None:
            buf = self._buffers[key] = make()
        return buf

    # ---- sample -----------------------------------------------------------------------------------------------------------------------
    def sample(self, raw, eps, obs=None):
        """``raw`` [N, 2A] (the columns ``[mu; log_std]`` of ``FusedMLP.squashed_gaussian(...).with_grad``, or ``torch.cat`` of two
        modules' outputs), ``eps`` [N, A] standard-normal draws, optional ``obs`` [N, D].  Returns ``(actions, log_prob)``:
        ``actions`` [N, A] in [-1, 1], or with ``obs`` the block ``[obs | actions]`` [N, D + A] -- the critics' input, no ``cat`` --
        and ``log_prob`` [N].  One launch; with a graph (``raw`` requires grad, grad mode on) it is a ``torch.autograd.Function`` whose
        backward is the second launch: critics evaluated on the block chain through ordinary autograd."""
        import torch
        if not torch.is_tensor(raw) or raw.dim() != 2 or raw.shape[1] % 2 or not 1 <= raw.shape[1] // 2 <= MAX_ACTION_DIM:
            raise ValueError(f"raw must be a [N, 2A] tensor with A = 1 .. {MAX_ACTION_DIM}, got "
                             f"{tuple(raw.shape) if torch.is_tensor(raw) else type(raw).__name__}")
        n, A, dev = int(raw.shape[0]), int(raw.shape[1]) // 2, raw.device
        self._rows("raw", raw, 2 * A, dev)
        self._rows("eps", eps, A, dev, rows=n)
        D = 0
        if obs is not None:
            if not torch.is_tensor(obs) or obs.dim() != 2 or obs.shape[1] < 1:
                raise ValueError("obs must be a [N, D] tensor")
            D = int(obs.shape[1])
            self._rows("obs", obs, D, dev, rows=n)
        if torch.is_grad_enabled() and raw.requires_grad:
            return _Sample.apply(raw, eps, obs, self)
        return self._sample_forward(raw, eps, obs, False)

    def _sample_forward(self, raw, eps, obs, graph):
        import torch
        n, A, dev = int(raw.shape[0]), int(raw.shape[1]) // 2, raw.device
        D = 0 if obs is None else int(obs.shape[1])
        buf = self._buffer(("sample", n, A, D, dev, graph), lambda: {
            "block": torch.zeros(n, D + A, dtype=torch.float32, device=dev), "log_prob": torch.zeros(n, dtype=torch.float32, device=dev)})
        self.backend.squashed_gaussian_sample(self._rows("raw", raw, 2 * A, dev), self._rows("eps", eps, A, dev), buf["block"],
                                              buf["log_prob"], self.log_std_min, self.log_std_max,
                                              obs=None if obs is None else self._rows("obs", obs, D, dev))
        # fresh views: a tensor handed out twice by an autograd Function would carry the first call's node
        return buf["block"].view(n, D + A), buf["log_prob"].view(n)

    def _sample_backward(self, raw, eps, d_block, d_log_prob, D):
        import torch
        n, A, dev = int(raw.shape[0]), int(raw.shape[1]) // 2, raw.device
        d_actions = None
        if d_block is not None:
            d_block = self._rows("d_actions", d_block, D + A, dev, rows=n)
            d_actions = d_block[:, D:]                   # in place: the action columns of the critics' dx
        if d_log_prob is not None and not (d_log_prob.dim() == 1 and d_log_prob.stride(0) == 0):
            d_log_prob = self._rows("d_log_prob", d_log_prob, None, dev, rows=n)
        d_raw = torch.empty(n, 2 * A, dtype=torch.float32, device=dev)      # (autograd may keep it as a leaf's .grad)
        self.backend.squashed_gaussian_sample_backward(self._rows("raw", raw, 2 * A, dev), self._rows("eps", eps, A, dev), d_actions,
                                                       d_log_prob, d_raw, self.log_std_min, self.log_std_max)
        return d_raw

    # ---- critic -----------------------------------------------------------------------------------------------------------------------
    def critic(self, q1, q2, q1_target, q2_target, next_log_prob, rewards, dones, log_alpha, index=None):
        """``q1`` / ``q2`` [N] or [N, 1]: the critics on the stored (observation, action) rows, in minibatch order (they may carry a
        ``grad_fn``; ``q2`` and ``q2_target`` None: one critic); ``q1_target`` / ``q2_target`` / ``next_log_prob`` [N]: the target
        critics on ``sample``'s next-state block and its log-probability; ``rewards`` / ``dones`` [M] or [M, 1] float32: the replay
        buffer's arrays, gathered by ``index`` (int64 [N]) INSIDE the kernel (without it M = N); ``log_alpha``: a 1-element device
        tensor, read on the device.  Returns a ``SACCriticResult``."""
        import torch
        if not torch.is_tensor(q1):
            raise ValueError(f"q1 must be a tensor, got {type(q1).__name__}")
        dev = q1.device
        a1 = self._rows("q1", q1, None, dev)
        n = int(a1.shape[0])
        if (q2 is None) != (q2_target is None):
            raise ValueError("q2 and q2_target are given together")
        a2 = None if q2 is None else self._rows("q2", q2, None, dev, rows=n)
        t1 = self._rows("q1_target", q1_target, None, dev, rows=n)
        t2 = None if q2 is None else self._rows("q2_target", q2_target, None, dev, rows=n)
        lp = self._rows("next_log_prob", next_log_prob, None, dev, rows=n)
        idx = None if index is None else self._rows("index", index, None, dev, torch.int64, rows=n)
        r = self._rows("rewards", rewards, None, dev, rows=n if idx is None else None)
        d = self._rows("dones", dones, None, dev, rows=int(r.shape[0]))
        la = self._log_alpha(log_alpha, dev)
        buf = self._buffer(("critic", n, a2 is not None, dev), lambda: {
            "stats": torch.zeros(len(CRITIC_STATS), dtype=torch.float32, device=dev), "d_q1": torch.zeros(n, dtype=torch.float32, device=dev),
            "d_q2": torch.zeros(n, dtype=torch.float32, device=dev) if a2 is not None else None,
            "target": torch.zeros(n, dtype=torch.float32, device=dev)})
        self.backend.sac_critic_loss(a1, a2, t1, t2, lp, r, d, la, self.gamma, buf["d_q1"], buf["d_q2"], target=buf["target"],
                                     stats=buf["stats"], index=idx)
        return SACCriticResult(buf["stats"], buf["d_q1"], buf["d_q2"], buf["target"], q1, q2)

    def _log_alpha(self, log_alpha, dev):
        import torch
        if not torch.is_tensor(log_alpha) or log_alpha.numel() != 1:
            raise ValueError("log_alpha must be a tensor of one element (it is read on the device)")
        return self._rows("log_alpha", log_alpha.reshape(1), None, dev)

    # ---- actor ------------------------------------------------------------------------------------------------------------------------
    def actor(self, q1_pi, q2_pi, log_prob, log_alpha):
        """``q1_pi`` / ``q2_pi`` [N] or [N, 1]: the critics on ``sample``'s block (``q2_pi`` None: one critic); ``log_prob`` [N]:
        ``sample``'s; ``log_alpha``: a 1-element device tensor (a leaf Parameter, or any tensor with a graph).  Returns a
        ``SACActorResult``."""
        import torch
        if not torch.is_tensor(q1_pi):
            raise ValueError(f"q1_pi must be a tensor, got {type(q1_pi).__name__}")
        dev = q1_pi.device
        a1 = self._rows("q1_pi", q1_pi, None, dev)
        n = int(a1.shape[0])
        a2 = None if q2_pi is None else self._rows("q2_pi", q2_pi, None, dev, rows=n)
        lp = self._rows("log_prob", log_prob, None, dev, rows=n)
        la = self._log_alpha(log_alpha, dev)
        buf = self._buffer(("actor", n, a2 is not None, dev), lambda: {
            "stats": torch.zeros(len(ACTOR_STATS), dtype=torch.float32, device=dev), "d_q1": torch.zeros(n, dtype=torch.float32, device=dev),
            "d_q2": torch.zeros(n, dtype=torch.float32, device=dev) if a2 is not None else None,
            "d_log_prob": torch.zeros(1, dtype=torch.float32, device=dev), "d_log_alpha": torch.zeros(1, dtype=torch.float32, device=dev)})
        self.backend.sac_actor_loss(a1, a2, lp, la, self.target_entropy, buf["d_q1"], buf["d_q2"], buf["d_log_prob"], buf["d_log_alpha"],
                                    stats=buf["stats"])
        return SACActorResult(buf["stats"], buf["d_q1"], buf["d_q2"], buf["d_log_prob"], buf["d_log_alpha"], q1_pi, q2_pi, log_prob,
                              log_alpha)


def _make_sample_function():
    import torch

    class _SampleFunction(torch.autograd.Function):
        """``SACLoss.sample`` under autograd: forward = pdegym_squashed_gaussian_sample, backward = its _backward launch, which
        recomputes what it needs from ``raw`` and ``eps`` (nothing else is saved)."""

        @staticmethod
        def forward(ctx, raw, eps, obs, head):
            block, log_prob = head._sample_forward(raw, eps, obs, True)
            ctx.save_for_backward(raw, eps)
            ctx.head, ctx.D = head, 0 if obs is None else int(obs.shape[1])
            ctx.set_materialize_grads(False)
            return block, log_prob

        @staticmethod
        def backward(ctx, d_block, d_log_prob):
            raw, eps = ctx.saved_tensors
            if d_block is None and d_log_prob is None:
                return None, None, None, None
            d_raw = ctx.head._sample_backward(raw, eps, d_block, d_log_prob, ctx.D)
            d_obs = d_block[:, :ctx.D] if (ctx.D and d_block is not None and ctx.needs_input_grad[2]) else None
            return d_raw, None, d_obs, None

    return _SampleFunction


class _Sample:
    """Builds the autograd Function at first use (torch is imported lazily throughout the package)."""
    _fn = None

    @classmethod
    def apply(cls, *args):
        if cls._fn is None:
            cls._fn = _make_sample_function()
        return cls._fn.apply(*args)
