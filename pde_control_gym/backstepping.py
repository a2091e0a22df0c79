"""The backstepping baseline on the device: the controller every result table of the reference compares its learned policies
against (examples/transportPDE/transport1Dbackstepping.py:22-36, examples/reactionDiffusionPDE/reactionDiffusion1DBackstepping.py:22-39),
for a whole batch at once.

The gain is a function of each instance's theta row (the plant parameter sampled on the controller's grid), so it is computed per
row on the device at construction (``solveKernelFunction``), and the control law (``solveControl``: one dot product per instance)
is one kernel launch per env-step.  ``DeviceRollout(venv, controller, T)`` drives it like a ``FusedMLP`` (control launch, then step
launch); with ``pool_theta`` the gains follow the fused auto-reset, which redraws beta from a pool at every restart.
``DeviceRollout(venv, controller.attach(venv), T, one_launch=True)`` evaluates the law INSIDE the one-launch rollout kernel instead
(``rollout_law``: Dirichlet actuation, rows of up to 512 / 513 nodes): one launch per rollout, the same bits.
"""
from __future__ import annotations

_KINDS = ("transport", "parabolic")


def pool_row(b: int, restarts: int, num_envs: int, pool_rows: int):
    """Row of the reset pools that instance ``b`` runs on after ``restarts`` restarts (None: none yet, its initial row ``b``).  The
    fused auto-reset gives the k-th restart (k = 0, 1, ...) row (b + k*num_envs) mod pool_rows, so after c restarts the running
    episode came from row (b + (c - 1)*num_envs) mod pool_rows."""
    return None if restarts <= 0 else (b + (restarts - 1) * num_envs) % pool_rows


class BacksteppingController:
    """``BacksteppingController(kind, theta, dx)`` with ``kind`` "transport" or "parabolic"; ``theta``: float32 [m] (one row shared
    by every instance) or [B, m] (row b for instance b), sampled by the caller -- the examples use ``linspace(dx, X, m)``, not the
    plant's grid; ``dx``: the Python double of the script.  ``.gain`` (float64, the shape of ``theta``) is bit-identical to the
    reference's ``solveKernelFunction`` (NumPy >= 2).

    ``controller(obs)`` -> float64 commands [B] (feed ``PDEBatch1D.step(..., action_kind=ACTION_F64)``: the reference's own call);
    ``forward_into(obs, out, clamp=None, noise=None)`` writes float32 (rounded once from the double, + noise, clamped) or float64
    commands into ``out`` -- the contract of ``FusedMLP.forward_into``.

    ``order="tree"`` (default): products per lane and a wave reduction; ``"ordered"``: the reference's left-to-right sum, commands
    bit-identical to the reference's.  The two differ by at most 2 * len * 2**-53 * sum|gain_i * obs_i| * |scale|.

    ``pool_theta`` [P, m]: theta rows of the environment's reset pool (row r belongs to ``beta_pool[r]``); ``attach(venv)`` then
    takes the restart counters from the environment, and instance b uses ``.pool_gain[pool_row(b, count[b], B, P)]`` once it has
    restarted."""

    def __init__(self, kind, theta, dx, *, pool_theta=None, order="tree", device=None, backend=None):
        import torch
        if kind not in _KINDS:
            raise ValueError(f"kind must be one of {_KINDS} (the two 1D families the reference ships a backstepping law for), got {kind!r}")
        if order not in ("tree", "ordered"):
            raise ValueError(f"order must be 'tree' or 'ordered', got {order!r}")
        self.kind, self.dx, self.order = kind, float(dx), order
        if device is None:
            device = theta.device if torch.is_tensor(theta) else "cuda"
        self.device = torch.device(device)
        if backend is None:
            from pdecontrolgym_amd.backend import default_backend
            backend = default_backend()
        self.backend = backend
        theta = torch.as_tensor(theta).to(device=self.device, dtype=torch.float32).contiguous()
        if theta.dim() not in (1, 2) or theta.shape[-1] < 2:
            raise ValueError(f"theta must be [m] or [B, m] with m >= 2, got {tuple(theta.shape)}")
        self.m = int(theta.shape[-1])
        self.gain = self._gains(theta.reshape(-1, self.m)).reshape(theta.shape)
        self.pool_gain = None
        if pool_theta is not None:
            pool = torch.as_tensor(pool_theta).to(device=self.device, dtype=torch.float32).contiguous()
            if pool.dim() != 2 or pool.shape[1] != self.m:
                raise ValueError(f"pool_theta must be [P, {self.m}] (rows as long as theta's), got {tuple(pool.shape)}")
            if theta.dim() != 2:
                raise ValueError("pool_theta redraws the gain per instance: theta must be [B, m] as well")
            self.pool_gain = self._gains(pool)
        self._reset_count = None
        self._core = None       # the engine attach() bound this controller to

    def _gains(self, theta):
        import torch
        gain = torch.empty(theta.shape, dtype=torch.float64, device=self.device)
        self.backend.backstep_gain(self.kind, theta, gain, self.dx)
        return gain

    def attach(self, venv):
        """Bind to a ``PDEVecEnv`` of the same 1D family with full-state sensing: checks what the law needs and, with
        ``pool_theta``, takes the environment's restart counters so that the gains follow its fused auto-reset.  Returns self."""
        core = getattr(venv, "core", None)
        kind = getattr(core, "kind", None)
        if kind not in _KINDS or getattr(core, "flux", "linear") != "linear":
            raise ValueError(f"the backstepping law exists for the TransportPDE1D and ReactionDiffusionPDE1D families only, not for "
                             f"{type(venv).__name__} ({getattr(venv, 'kind', kind)})")
        if kind != self.kind:
            raise ValueError(f"a {self.kind} controller cannot drive a {kind} environment (the gain recursions differ)")
        if core.obs_dim != core.n:
            raise ValueError("the backstepping law is a dot product with the whole row: it needs sensing_loc='full', "
                             "this environment senses one scalar")
        if self.gain.dim() == 2 and self.gain.shape[0] != core.num_envs:
            raise ValueError(f"theta has {self.gain.shape[0]} rows, the environment {core.num_envs} instances")
        self._length(core.n)
        pool, count = core.t.get("reset_init"), core.t.get("reset_count")
        rows = 0 if pool is None else int(pool.shape[0])
        if self.pool_gain is not None:
            if rows != self.pool_gain.shape[0] or count is None:
                raise ValueError(f"pool_theta has {self.pool_gain.shape[0]} rows, the environment's reset pool {rows}: row r of "
                                 "pool_theta must be the theta of beta_pool[r] (enable_fused_auto_reset first)")
        elif core.t.get("reset_beta") is not None:
            raise ValueError(f"the environment redraws beta from a pool of {rows} rows at every restart and pool_theta was not "
                             "given (0 rows): the gains would be stale after the first restart")
        self._reset_count = count if self.pool_gain is not None else None
        self._core = core
        return self

    # ---- the law inside the one-launch rollout kernel (pdegym_*_backstep_rollout) --------------------------------------------------------
    def rollout_gap(self, core):
        """What keeps this controller out of ``core``'s one-launch rollout, as a sentence -- or None when nothing does (the engines'
        ``law_rollout_gap`` ask, after their own checks): the law needs the checks of ``attach`` and, with ``pool_theta``, the
        engine's restart counters."""
        if self._core is None:
            return "the controller is not attached to the environment (controller.attach(venv) first)"
        if self._core is not core:
            return (f"the {self.kind} controller is attached to another environment than this {getattr(core, 'kind', '?')} one "
                    "(controller.attach(venv) binds it to the one it drives)")
        return None

    def rollout_law(self, actions, clamp=None, noise=None):
        """The ``pdegym_backstep`` descriptor of a rollout that writes its commands into ``actions`` [T, B]: gains (with the pool
        and the restart counters ``attach`` took), length, order and scale of the attached environment; ``noise`` -- float32,
        contiguous, the actions' shape -- added to the command of step t before the clamp to ``clamp`` = (lo, hi).  The
        observation and output pointers stay unset: the rollout's own buffers are used."""
        import torch
        from pdecontrolgym_amd import _native as N
        if self._core is None:
            raise ValueError("rollout_law needs an attached controller (controller.attach(venv) first)")
        c = N.Backstep()
        c.gain0, c.gain_stride, c.m = self.gain.data_ptr(), (0 if self.gain.dim() == 1 else self.gain.stride(0)), self.m
        if self._reset_count is not None:
            c.gain_pool, c.pool_rows, c.reset_count = self.pool_gain.data_ptr(), int(self.pool_gain.shape[0]), self._reset_count.data_ptr()
        c.len, c.order, c.scale = self._length(self._core.n), (N.BACKSTEP_ORDERED if self.order == "ordered" else N.BACKSTEP_TREE), self.scale
        if noise is not None:
            if noise.dtype != torch.float32 or tuple(noise.shape) != tuple(actions.shape) or not noise.is_contiguous():
                raise ValueError("noise must be a contiguous float32 tensor of the actions' shape")
            c.noise = noise.data_ptr()
        if clamp is not None:
            c.clamp, c.lo, c.hi = 1, float(clamp[0]), float(clamp[1])
        return c

    def _length(self, n):
        """Terms of the dot product for rows of n nodes: transport1Dbackstepping.py:33-35 runs over len(u);
        reactionDiffusion1DBackstepping.py:39 over kernel[-1][0:len(u)-1]."""
        if self.kind == "transport":
            if n > self.m:
                raise ValueError(f"the transport law sums over all {n} nodes of the row, theta has only {self.m}")
            return n
        return min(self.m, n - 1)

    @property
    def scale(self):
        # transport1Dbackstepping.py:36 writes the literal 1e-2; reactionDiffusion1DBackstepping.py:39 multiplies by dx
        return 1e-2 if self.kind == "transport" else self.dx

    def forward_into(self, obs, out, clamp=None, noise=None):
        """out[b] = the command for observation row obs[b]: ``obs`` float32 [B, n]; ``out`` [B] or [B, 1], float64, or float32
        (rounded once from the double, then ``noise`` [B] added, then clamped to ``clamp`` = (lo, hi)).  Returns ``out``.
        A NaN in an observation row makes that row's command NaN, as in the reference's dot product, and the clamp keeps it like
        ``np.clip``; +-Inf is clamped to the bound (include/pdegym.h, conventions)."""
        x = obs.reshape(obs.shape[0], -1)
        self.backend.backstep_control(x, out, self.gain, self._length(int(x.shape[1])), self.scale, ordered=self.order == "ordered",
                                      gain_pool=self.pool_gain if self._reset_count is not None else None,
                                      reset_count=self._reset_count, noise=noise, clamp=clamp)
        return out

    def __call__(self, obs):
        import torch
        return self.forward_into(obs, torch.empty(obs.shape[0], dtype=torch.float64, device=obs.device))


class TrafficBacksteppingController:
    """The model-based baseline of the reference's traffic result table (examples/TrafficPDE1D/Backstepping control.ipynb, cell 5) for a
    whole batch of freeways: ``TrafficBacksteppingController(venv_or_core, order="tree", gamma=1.0)``.

    The command is the constant ``qs`` for 'inlet', the outlet feedback ``q_out = (qs + rs*Iv) + Iq`` for 'outlet', and
    ``(qs, q_out)`` for 'both', with ``Iv = trapz(cv*(v - vs), dx)``, ``Iq = trapz(cq*(r*v - qs), dx)`` over the two halves (r, v) of
    the float64 observation.  The weight rows ``.weights_v`` (cv) and ``.weights_q`` (cq) are built here with NumPy -- its ``exp``
    has no bit-exact twin on the device -- from the engine's grid, ``dx``, ``vm``, ``rm``, ``tau`` and the per-instance ``rs``: one
    shared row [M] when every instance has the same ``rs``, else one row per instance [B, M].  They belong to the ``rs`` values the
    engine holds at ``attach``; the engine counts every change of them (``rs_version``: a reset to other densities, a reset pool
    switched on, off or refilled), and a controller whose count is behind refuses to form commands until it is attached again.

    ``controller(obs)`` -> float64 commands [B] ([B, 2] for 'both'); ``forward_into(obs, out, clamp=None, noise=None)`` writes them
    (+ float32 ``noise`` of ``out``'s shape, widened; clamped to ``clamp`` = (lo, hi), a NaN stays NaN) into ``out`` -- the contract
    of ``FusedMLP.forward_into``, so ``DeviceRollout(venv, controller, T)`` drives it (control launch, then step launch), and
    ``DeviceRollout(venv, controller, T, one_launch=True)`` evaluates the law INSIDE the one-launch traffic rollout kernel
    (``rollout_law``: freeways of up to 64 nodes): one launch per rollout, the same bits.

    ``order="numpy"``: the terms of each trapezoid sum are added in ``np.trapz``'s own order, commands bit-identical to the
    reference's; rows of up to 129 nodes (longer rows make NumPy halve recursively: refused here).  ``order="tree"`` (default): each
    lane adds its terms in ascending order, then a wave reduction; any row the engine takes.  With t_i = (dx*(p[i+1] + p[i]))/2.0
    the n = M - 1 terms of a sum (tv of Iv, tq of Iq), the two orders differ by at most
    ``2 * 2**-53 * ((n + 2)*(|rs|*sum|tv_i| + sum|tq_i|) + |rs*Iv| + |qs + rs*Iv| + |q_out|)``:
    any order of n terms lies within (n - 1)*2**-53*sum|t_i| of the exact sum (n + 2 covers the second-order terms), the integrals
    enter q_out with the weights |rs| and 1, and each of q_out's three roundings may differ by one unit of its result per order."""

    def __init__(self, venv_or_core, order="tree", gamma=1.0):
        if order not in ("tree", "numpy"):
            raise ValueError(f"order must be 'tree' or 'numpy', got {order!r}")
        self.order, self.gamma = order, gamma
        self._core = None
        self._rs_seen = None
        self.weights_v = self.weights_q = None
        self.attach(venv_or_core)

    def attach(self, venv):
        """Bind to a TrafficPDE1D environment (a ``PDEVecEnv`` or its ``TrafficBatch``): checks what the law needs, reads the
        per-instance ``rs`` (one device-to-host read; with a fused auto-reset one more, of the pool) and builds the weight rows.
        Returns self."""
        import numpy as np
        import torch
        from pdecontrolgym_amd import _native as N
        core = getattr(venv, "core", venv)
        sim = getattr(core, "simulation_type", None)
        if sim is None or not hasattr(core, "Veq") or "rs" not in getattr(core, "t", {}):
            raise ValueError(f"the traffic backstepping law exists for the TrafficPDE1D family only, not for {type(venv).__name__} "
                             f"({getattr(venv, 'kind', getattr(core, 'kind', '?'))})")
        if sim not in ("inlet", "outlet", "both"):
            raise ValueError(f"the traffic backstepping law exists for 'inlet', 'outlet' and 'both', not for {sim!r}: the reference "
                             "defines ps for those three only, and the train types observe a normalised state")
        if self.order == "numpy" and core.M > N.TRAFFIC_BACKSTEP_NUMPY_MAX_M:
            raise ValueError(f"order='numpy' covers freeways of up to {N.TRAFFIC_BACKSTEP_NUMPY_MAX_M} nodes (np.trapz halves longer "
                             f"rows recursively), this one has {core.M}: use order='tree'")
        rs = core.t["rs"].detach().cpu().numpy().astype(np.float64).reshape(-1)
        if rs.shape[0] != core.num_envs or not np.all(rs > 0):
            raise ValueError("the engine holds no steady-state density yet (rs <= 0): reset the environment before attaching")
        pool = core.t.get("reset_rs")
        if pool is not None:
            # restart k of instance b takes pool row (b + k*B) mod P: the rows congruent to b modulo gcd(B, P)
            pv = pool.detach().cpu().numpy().reshape(-1)
            g = int(np.gcd(core.num_envs, pv.shape[0]))
            if not (np.array_equal(pv, rs[:g][np.arange(pv.shape[0]) % g]) and np.array_equal(rs, rs[:g][np.arange(rs.shape[0]) % g])):
                raise ValueError("the environment's fused auto-reset redraws rs from a pool whose values differ from the instances' "
                                 "own: the weight rows would be stale after a restart")
        shared = bool(np.all(rs == rs[0]))
        rows = [self._weights(core, float(r)) for r in (rs[:1] if shared else rs)]
        wv, wq = (np.stack([row[k] for row in rows]) for k in (0, 1))
        if shared:
            wv, wq = wv[0], wq[0]
        self.weights_v = torch.as_tensor(wv, dtype=torch.float64).to(core.device).contiguous()
        self.weights_q = torch.as_tensor(wq, dtype=torch.float64).to(core.device).contiguous()
        self._core, self._rs_seen = core, core.rs_version
        self.n_commands = 2 if sim == "both" else 1
        return self

    def _weights(self, core, rs):
        """(cv, cq) of one steady-state density, every operation in the order the law is written in (the constants as the reference
        and the engine form them: vs = Veq(rs), qs = rs*vs, ps = vm/rm*qs/vs)."""
        import numpy as np
        vm, rm, tau, gamma, x = core.vm, core.rm, core.tau, self.gamma, core.x
        vs = vm * (1 - rs / rm)
        qs = rs * vs
        ps = vm / rm * qs / vs
        lam1 = vs
        lam2 = vs + rs * (-vm / rm)
        K = -(1 / (gamma * ps)) * (-1 / tau) * np.exp(-x / (tau * vs))
        Mk = -K
        E = np.exp(x / (vs * tau))
        cv = Mk + (lam2 / lam1) * K * E
        cq = ((lam1 - lam2) / lam1) * K * E
        return np.asarray(cv, dtype=np.float64), np.asarray(cq, dtype=np.float64)

    def rollout_gap(self, core):
        """What keeps this controller out of ``core``'s one-launch rollout, as a sentence -- or None (``TrafficBatch.law_rollout_gap``
        asks after its own checks)."""
        if self._core is not core:
            return "the controller is attached to another environment than this one (controller.attach(venv) binds it to the one it drives)"
        if core.rs_version != self._rs_seen:
            return ("the environment's steady-state densities or its reset pool changed after the controller was attached: the weight "
                    "rows may be stale (controller.attach(venv) again)")
        return None

    def _descriptor(self, shape, clamp, noise):
        import torch
        from pdecontrolgym_amd import _native as N
        gap = self.rollout_gap(self._core)
        if gap is not None:
            raise ValueError(gap)
        c = N.TrafficBackstep()
        c.weights_v, c.weights_q = self.weights_v.data_ptr(), self.weights_q.data_ptr()
        c.weight_stride = 0 if self.weights_v.dim() == 1 else self.weights_v.stride(0)
        c.order = N.TRAFFIC_BACKSTEP_NUMPY if self.order == "numpy" else N.TRAFFIC_BACKSTEP_TREE
        if noise is not None:
            if noise.dtype != torch.float32 or tuple(noise.shape) != tuple(shape) or not noise.is_contiguous():
                raise ValueError("noise must be a contiguous float32 tensor of the commands' shape")
            c.noise, c.noise_stride = noise.data_ptr(), self.n_commands
        if clamp is not None:
            c.clamp, c.lo, c.hi = 1, float(clamp[0]), float(clamp[1])
        return c

    def rollout_law(self, actions, clamp=None, noise=None):
        """The ``pdegym_traffic_backstep`` descriptor of a rollout that writes its commands into ``actions`` [T, B, commands]:
        weights and order; ``noise`` -- float32, contiguous, the actions' shape -- added to the commands of step t before the clamp
        to ``clamp`` = (lo, hi)."""
        if actions.dim() != 3 or actions.shape[2] != self.n_commands:
            raise ValueError(f"actions must be [T, B, {self.n_commands}], got {tuple(actions.shape)}")
        return self._descriptor(actions.shape, clamp, noise)

    def forward_into(self, obs, out, clamp=None, noise=None):
        """out[b] = the command(s) for observation row obs[b]: ``obs`` float64 [B, 2M]; ``out`` float64, contiguous, [B] or [B, 1]
        ([B, 2] for 'both': inlet, outlet).  Returns ``out``.  A NaN or Inf in a row makes that row's outlet command non-finite, as
        in the reference's sums, and the clamp keeps a NaN like ``np.clip``."""
        law = self._descriptor(out.shape, clamp, noise)
        self._core.backend.traffic_backstep_control(self._core.params, obs.reshape(obs.shape[0], -1), self._core.t["rs"], out, law)
        return out

    def __call__(self, obs):
        import torch
        shape = (obs.shape[0],) if self.n_commands == 1 else (obs.shape[0], 2)
        return self.forward_into(obs, torch.empty(shape, dtype=torch.float64, device=obs.device))
