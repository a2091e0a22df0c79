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
