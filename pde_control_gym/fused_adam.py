"""The optimiser step of a training loop on the device: global-norm clipping, the Adam update, the blocked weight copies that
``FusedMLP``'s kernels read and the Polyak average of target networks in two launches (pdegym_fused_adam).

Both training examples end an update with ``clip_grad_norm_`` + ``torch.optim.Adam`` (+ a loop of ``lerp_`` over SAC's target
critics), after which the next ``FusedMLP.with_grad`` / ``DeviceRollout.run`` calls ``FusedMLP.refresh()`` to rebuild the blocked
transposes ``[ceil(in/4), out, 4]`` of every changed layer.  ``FusedAdam`` owns those copies instead: the launch that updates a
weight writes it to its mirrors as well, ``refresh()`` finds nothing to do, and -- because nothing on the host has to look at version
counters any more -- forward, loss, backward and optimiser step of attached networks capture into one ``torch.cuda.graph``.

The arithmetic (include/pdegym.h) is ``clip_grad_norm_`` followed by ``torch.optim.Adam``'s single-tensor update in float32, each
operation rounded once, with ``beta^t`` kept as running products in float64 on the device; ``tests/fused_adam_restatement.py``
restates it in NumPy.  Unlike ``clip_grad_norm_`` the call does NOT modify the gradients: the scaled gradient exists only inside
the kernel.
"""
from __future__ import annotations

MAX_TENSORS = 32


class FusedAdam:
    """``opt = FusedAdam(params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, max_grad_norm=None)``; ``opt.attach(fused_mlp)``;
    per update ``opt.zero_grad(); loss.backward(); opt.step()``.

    ``params``: at most 32 float32 contiguous ``torch.nn.Parameter`` on one device, updated by ONE ``pdegym_fused_adam`` call (a longer
    list is refused with ``ValueError``: use one optimiser per group of networks; their norms are then separate, as separate
    ``clip_grad_norm_`` calls would be).  ``weight_decay`` and ``amsgrad`` are not offered, and all tensors share one step count.
    ``lr`` is a float (``opt.lr = x`` changes it between steps) or a 0-d / 1-element float32 DEVICE tensor, read by the kernel: a
    captured graph follows a schedule written into it.  ``betas``, ``eps`` and ``max_grad_norm`` are fixed at construction.
    ``max_grad_norm`` (None: off) clips the global norm over ALL of ``params`` as ``clip_grad_norm_(params, max_grad_norm)`` does;
    ``opt.total_norm`` is then a 0-d device view of the norm of the last step (None without clipping).

    ``attach(fused_mlp)`` / ``attach_target(...)`` register the copies the step maintains.  ``step()`` makes no host
    synchronisation and, after the first call, no allocation: a warmed-up ``step()`` captures into a ``torch.cuda.graph``."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, max_grad_norm=None, backend=None):
        import torch
        params = list(params)
        if not 1 <= len(params) <= MAX_TENSORS:
            raise ValueError(f"FusedAdam takes 1..{MAX_TENSORS} parameter tensors per optimiser, got {len(params)}")
        dev = params[0].device
        for p in params:
            if not torch.is_tensor(p) or p.dtype != torch.float32 or not p.is_contiguous() or p.device != dev or p.numel() < 1:
                raise ValueError("FusedAdam needs non-empty contiguous float32 parameters on one device")
        if len({id(p) for p in params}) != len(params):
            raise ValueError("FusedAdam: a parameter appears twice")
        beta1, beta2 = float(betas[0]), float(betas[1])
        if not (0.0 <= beta1 < 1.0 and 0.0 <= beta2 < 1.0):
            raise ValueError("betas must be in [0, 1)")
        if not float(eps) > 0.0:
            raise ValueError("eps must be > 0")
        if torch.is_tensor(lr):
            if lr.dtype != torch.float32 or lr.numel() != 1 or lr.device != dev:
                raise ValueError("a tensor lr must be one float32 element on the parameters' device")
            lr = lr.detach().reshape(1)
        else:
            lr = float(lr)
        if backend is None:
            from pdecontrolgym_amd.backend import default_backend
            backend = default_backend()
        self.backend, self.params, self.device = backend, params, dev
        self.lr, self.betas, self.eps = lr, (beta1, beta2), float(eps)
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.tau = None
        self.exp_avg = [torch.zeros_like(p, memory_format=torch.contiguous_format) for p in params]
        self.exp_avg_sq = [torch.zeros_like(p, memory_format=torch.contiguous_format) for p in params]
        self.state = torch.tensor([0.0, 1.0, 1.0], dtype=torch.float64, device=dev)      # step count, beta1^t, beta2^t
        self._total_norm = torch.zeros(1, dtype=torch.float32, device=dev) if self.max_grad_norm is not None else None
        self._index = {id(p): i for i, p in enumerate(params)}
        self._entries = [{"p": p.detach(), "g": None, "m": m, "v": v} for p, m, v in zip(params, self.exp_avg, self.exp_avg_sq)]
        self._targets = []            # the target tensors of attach_target, in registration order
        self._mlps, self._target_mlps = [], []
        self._workspace, self._cache = None, {}

    # ---- what the step maintains besides the parameters --------------------------------------------------------------------------
    @staticmethod
    def _mirrors_of(fused_mlp):
        """(parameter, key, value) for every copy of a wrapper that follows a parameter: the blocked transposes of its layers and,
        with a squashed-Gaussian head, the rows of the fused last layer [mu; log_std] in both of its forms and its bias."""
        heads = fused_mlp._heads is not None
        own = fused_mlp.layers[:-1] if heads else fused_mlp.layers
        out = [(w, "wt", (fused_mlp._wt[i], int(w.shape[0]), 0)) for i, (w, _, _) in enumerate(own)]
        if heads:
            fused = fused_mlp._fused
            A = int(fused_mlp._heads[0].weight.shape[0])
            for j, m in enumerate(fused_mlp._heads):
                rows = slice(j * A, (j + 1) * A)
                out.append((m.weight, "wt", (fused_mlp._wt[-1], 2 * A, j * A)))
                out.append((m.weight, "copy", fused.weight.detach()[rows]))
                if m.bias is not None:
                    out.append((m.bias, "copy", fused.bias.detach()[rows]))
        return out

    def _register(self, fused_mlp, index, prefix, what):
        import torch
        if fused_mlp.device != self.device:
            raise ValueError(f"{what}: the network is on {fused_mlp.device}, the optimiser on {self.device}")
        missing = [p for p in fused_mlp.grad_parameters() if id(p) not in index]
        if missing:
            raise ValueError(f"{what}: {len(missing)} of the network's {len(fused_mlp.grad_parameters())} parameter tensors do not belong to "
                             "this optimiser; a network is maintained as a whole or not at all")
        mirrors = self._mirrors_of(fused_mlp)
        for p, key, _ in mirrors:
            if self._entries[index[id(p)]].get(prefix + key) is not None:
                raise ValueError(f"{what}: a parameter already has a mirror of this kind (one FusedMLP per module and optimiser)")
        if self.device.type == "cuda" and torch.cuda.is_current_stream_capturing():
            raise RuntimeError(f"{what} cannot run inside a stream capture")
        fused_mlp.refresh()      # the copies are current from here on; the step keeps them so
        for p, key, value in mirrors:
            self._entries[index[id(p)]][prefix + key] = value
        self._cache.clear()

    def attach(self, fused_mlp):
        """Maintain the blocked weight copies of ``fused_mlp`` (and, for a squashed-Gaussian wrapper, the rows and the bias of its
        fused last layer): every ``step()`` writes them, ``fused_mlp.refresh()`` then has nothing to do, and ``fused_mlp.with_grad``
        may run inside a stream capture.  ``ValueError`` unless every tensor of ``fused_mlp.grad_parameters()`` belongs to this
        optimiser.  Returns ``self``."""
        self._register(fused_mlp, self._index, "", "FusedAdam.attach")
        self._mlps.append(fused_mlp)
        fused_mlp._optimizer = self
        return self

    def attach_target(self, params, target_params, tau, target_mlp=None):
        """``step(polyak=True)`` also moves ``target_params[i]`` towards the NEW ``params[i]``: ``pt = (1 - tau) * pt + tau * p``, SB3's
        ``polyak_update`` order (``lerp_`` computes ``pt + tau * (p - pt)``: equal in exact arithmetic).  ``params`` must belong to
        this optimiser; ``tau`` in [0, 1] is one value per optimiser.  ``target_mlp``: the ``FusedMLP`` that evaluates the target
        network, if any -- its copies are then maintained like those of ``attach``.  Returns ``self``."""
        import torch
        params, target_params, tau = list(params), list(target_params), float(tau)
        if len(params) != len(target_params):
            raise ValueError("attach_target: params and target_params differ in length")
        if not 0.0 <= tau <= 1.0:
            raise ValueError("attach_target: tau must be in [0, 1]")
        if self.tau is not None and tau != self.tau:
            raise ValueError(f"attach_target: this optimiser's targets use tau = {self.tau}")
        for p, pt in zip(params, target_params):
            if id(p) not in self._index:
                raise ValueError("attach_target: a parameter does not belong to this optimiser")
            if not torch.is_tensor(pt) or pt.dtype != torch.float32 or pt.shape != p.shape or pt.device != self.device or not pt.is_contiguous():
                raise ValueError("attach_target: a target must be a contiguous float32 tensor of its parameter's shape and device")
            if self._entries[self._index[id(p)]].get("pt") is not None:
                raise ValueError("attach_target: a parameter already has a target")
        for p, pt in zip(params, target_params):
            self._entries[self._index[id(p)]]["pt"] = pt.detach()
            self._targets.append(pt)
        self.tau = tau
        self._cache.clear()
        if target_mlp is not None:
            self._register(target_mlp, {id(pt): self._index[id(p)] for p, pt in zip(params, target_params)}, "pt_", "FusedAdam.attach_target")
            self._target_mlps.append(target_mlp)
        return self

    # ---- the step ------------------------------------------------------------------------------------------------------------------
    @property
    def total_norm(self):
        """The global gradient norm of the last ``step()`` as a 0-d device view (no host synchronisation); None without clipping."""
        return None if self._total_norm is None else self._total_norm[0]

    @staticmethod
    def _mark_seen(fused_mlp):
        for i, (w, _, _) in enumerate(fused_mlp.layers):
            fused_mlp._seen[i] = w._version
        if fused_mlp._heads is not None:
            mu, ls = fused_mlp._heads
            fused_mlp._heads_seen = tuple(p._version for m in (mu, ls) for p in (m.weight, m.bias) if p is not None)

    def step(self, polyak: bool = False):
        """One ``pdegym_fused_adam`` call on the current stream.  ``polyak=True`` also updates the targets of ``attach_target``.
        ``ValueError`` when a parameter has no gradient (the step count is shared, so no tensor can sit a step out)."""
        import torch
        if polyak and not self._targets:
            raise ValueError("FusedAdam.step(polyak=True): no targets were registered with attach_target")
        for p, e in zip(self.params, self._entries):
            g = p.grad
            if g is None:
                raise ValueError("FusedAdam.step: a parameter has no gradient (.grad is None)")
            if g.dtype != torch.float32 or g.shape != p.shape:
                raise ValueError("FusedAdam.step: a gradient must be float32 and of its parameter's shape")
            e["g"] = g if g.is_contiguous() else g.contiguous()
        if self._workspace is None:
            need = self.backend.fused_adam_workspace([p.numel() for p in self.params])
            self._workspace = torch.empty(max(int(need), 8), dtype=torch.uint8, device=self.device)
        self.backend.fused_adam(self._entries, self.state, self._workspace, self.lr, self.betas[0], self.betas[1], self.eps,
                                max_grad_norm=self.max_grad_norm, tau=self.tau, polyak=polyak, total_norm=self._total_norm,
                                cache=self._cache)
        bump = torch.autograd.graph.increment_version
        for p in self.params:
            bump(p)
        for m in self._mlps:
            self._mark_seen(m)
        if polyak:
            for pt in self._targets:
                bump(pt)
            for m in self._target_mlps:
                self._mark_seen(m)

    def zero_grad(self, set_to_none: bool = True):
        for p in self.params:
            if p.grad is not None:
                if set_to_none:
                    p.grad = None
                else:
                    p.grad.detach_()
                    p.grad.requires_grad_(False)
                    p.grad.zero_()

    def state_dict(self):
        """Moments, step count and running products (copies), with the hyper-parameters for reference."""
        return {"state": self.state.clone(), "exp_avg": [m.clone() for m in self.exp_avg], "exp_avg_sq": [v.clone() for v in self.exp_avg_sq],
                "lr": self.lr.clone() if hasattr(self.lr, "clone") else self.lr, "betas": self.betas, "eps": self.eps,
                "max_grad_norm": self.max_grad_norm, "tau": self.tau}

    def load_state_dict(self, sd):
        """Restore ``state_dict()`` IN PLACE (the buffers keep their addresses, a captured graph stays valid).  The hyper-parameters
        of the dictionary are not applied, except a float ``lr``."""
        import torch
        if len(sd["exp_avg"]) != len(self.params) or len(sd["exp_avg_sq"]) != len(self.params):
            raise ValueError("load_state_dict: the state has another number of tensors")
        for mine, theirs in zip(self.exp_avg + self.exp_avg_sq, list(sd["exp_avg"]) + list(sd["exp_avg_sq"])):
            if mine.shape != theirs.shape:
                raise ValueError("load_state_dict: a moment has another shape")
        with torch.no_grad():
            self.state.copy_(sd["state"])
            for mine, theirs in zip(self.exp_avg + self.exp_avg_sq, list(sd["exp_avg"]) + list(sd["exp_avg_sq"])):
                mine.copy_(theirs)
        if not torch.is_tensor(self.lr) and not torch.is_tensor(sd.get("lr", None)) and sd.get("lr") is not None:
            self.lr = float(sd["lr"])
