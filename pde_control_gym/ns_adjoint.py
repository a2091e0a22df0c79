"""The adjoint-optimisation baseline of NavierStokes2D on the device: the model-based row of the reference's NS result table
(examples/NavierStokes/NS2Doptimization.py:56-118), for a whole batch at once.

The script rolls the plant forward under some commands, marches two adjoint fields backward through the stored trajectory (one
pressure projection per step), reads a correction of the nominal command off the adjoint under the actuated wall, and replays.
Here the forward rollouts are ``NSBatch2D.rollout`` (one launch each) and the backward march with the read-off is one launch of
``pdegym_ns2d_adjoint_f64`` (include/pdegym.h) -- 198 host iterations of NumPy stencils and ``solve_pressure`` in the script.
Every number is bit-identical to the script's float64 arithmetic.
"""
from __future__ import annotations

_GRID = "8 / 11 / 16 / 21 / 26 / 31 / 32 rows, 3 .. 64 columns"
_TABLE = {"upper": ["Controllable", "Dirchilet"], "lower": ["Dirchilet", "Dirchilet"], "left": ["Dirchilet", "Dirchilet"],
          "right": ["Dirchilet", "Dirchilet"]}


class NSAdjointOptimizer:
    """``NSAdjointOptimizer(env, a_nom=2.0, ratio=1.0, width=5.0)`` for an ``NSVecEnv`` or an ``NSBatch2D`` in float64 on one of
    the rollout grids, with the script's boundary table (upper u "Controllable", every other entry "Dirchilet") and
    ``action_dim=1``.

    ``a_nom``: the nominal command, a scalar or one value per step (the script's ``u_ref``, :81); ``ratio`` and ``width``: the
    script's ``0.1/0.1`` and ``5`` of :107.  The viscosity of the adjoint equation is the environment's (the script writes the
    literal 0.1, its environment's value).

    ``sweep(obs, t0=0, keep_lam=False)`` -> ``(actions [T, B, 1], grad [T, B])`` from a forward rollout ``obs`` [T+1, B, ny, nx, 2]
    whose slot 0 is the state at time index ``t0``; with ``keep_lam`` a third value ``lam`` [T, B, ny, nx, 2] holds ``Lam1[::-1]``
    (:103) and ``Lam2`` in the same order.

    ``optimize(u0, v0, p0, actions0)`` is the script's flow: reset, rollout under ``actions0``, sweep, reset, replay under the new
    commands.  Both rollouts start from the caller's ``u0, v0, p0``: in the script the second ``env.reset(seed=400)`` draws NEW
    random fields (``np.random`` is not reseeded by it), so its replay starts elsewhere than the trajectory it linearised about;
    here the replay starts where the first rollout did."""

    def __init__(self, env, a_nom=2.0, ratio=1.0, width=5.0):
        import torch
        core = getattr(env, "core", env)
        if not hasattr(core, "can_rollout") or not hasattr(core, "iters"):
            raise ValueError(f"the adjoint baseline exists for the NavierStokes2D family only, not for {type(env).__name__}")
        if core.dtype != torch.float64:
            raise ValueError(f"the adjoint march is float64 (the script's arithmetic), this environment is {core.dtype}: build it "
                             "with dtype='float64'")
        if not core.can_rollout():
            raise ValueError(f"the adjoint march runs on the rollout grids ({_GRID}) with the interleaved state layout, this "
                             f"environment is {core.ny} x {core.nx}")
        if core.action_dim != 1:
            raise ValueError(f"the adjoint read-off gives one command per instance and step: action_dim must be 1, not {core.action_dim}")
        table = core.ctor["boundary_condition"]
        bad = [f"{edge} {'uv'[k]}: {table[edge][k]}" for edge in _TABLE for k in range(2) if table[edge][k] != _TABLE[edge][k]]
        if bad:
            raise ValueError("the adjoint march assumes the script's boundary table (upper u 'Controllable', every other entry "
                             "'Dirchilet': zero adjoint walls, gradient read under the upper wall); this environment has " + ", ".join(bad))
        if not hasattr(core.backend, "ns2d_adjoint"):
            raise ValueError(f"backend {getattr(core.backend, 'name', type(core.backend).__name__)} has no ns2d_adjoint")
        self.env, self.core = env, core
        self.a_nom, self.ratio, self.width = a_nom, float(ratio), float(width)

    def _nominal(self, T):
        import torch
        a = torch.as_tensor(self.a_nom, dtype=torch.float64, device=self.core.device).reshape(-1)
        if a.numel() == 1:
            return a.expand(T).contiguous()
        if a.numel() < T:
            raise ValueError(f"a_nom has {a.numel()} values, the trajectory {T} steps")
        return a[:T].contiguous()

    def sweep(self, obs, t0: int = 0, keep_lam: bool = False):
        import torch
        c = self.core
        want = (c.num_envs, c.ny, c.nx, 2)
        if obs.dim() != 5 or tuple(obs.shape[1:]) != want or obs.shape[0] < 2:
            raise ValueError(f"obs must be a forward rollout [T+1, {', '.join(map(str, want))}] with T >= 1, got {tuple(obs.shape)}")
        if obs.dtype != torch.float64:
            raise ValueError(f"obs must be float64, got {obs.dtype}")
        T, B = int(obs.shape[0]) - 1, c.num_envs
        grad = torch.empty(T, B, dtype=torch.float64, device=c.device)
        actions = torch.empty(T, B, dtype=torch.float64, device=c.device)
        lam = torch.empty(T, B, c.ny, c.nx, 2, dtype=torch.float64, device=c.device) if keep_lam else None
        c.backend.ns2d_adjoint(c.params, c.t, obs.contiguous(), self._nominal(T), self.ratio, self.width, grad, actions, lam=lam, t0=int(t0))
        actions = actions.reshape(T, B, 1)
        return (actions, grad, lam) if keep_lam else (actions, grad)

    def _rollout(self, u0, v0, p0, actions):
        import torch
        c = self.core
        T, B = int(actions.shape[0]), c.num_envs
        obs = torch.empty(T + 1, B, c.ny, c.nx, 2, dtype=torch.float64, device=c.device)
        rewards = torch.empty(T, B, dtype=torch.float64, device=c.device)
        terminated = torch.empty(T, B, dtype=torch.uint8, device=c.device)
        obs[0].copy_(c.reset(u0, v0, p0))
        c.rollout(obs, actions, rewards, terminated)
        return obs, rewards

    def optimize(self, u0, v0, p0, actions0):
        """Returns a dict: ``actions`` [T, B, 1] (the optimised commands), ``grad`` [T, B], ``reward_before`` / ``reward_after`` [B]
        (reward sums of the first rollout and of the replay), ``rewards`` [T, B] and ``obs`` [T+1, B, ny, nx, 2] of the replay."""
        import torch
        c = self.core
        if c.t.get("reset_u0") is not None:
            raise ValueError("the fused auto-reset would restart instances inside the trajectory the adjoint marches through: "
                             "disable_auto_reset() first")
        a0 = torch.as_tensor(actions0, dtype=torch.float64, device=c.device)
        if a0.dim() == 1:
            a0 = a0.reshape(-1, 1, 1).expand(-1, c.num_envs, 1)
        if a0.dim() == 2:
            a0 = a0.unsqueeze(-1)
        if a0.dim() != 3 or tuple(a0.shape[1:]) != (c.num_envs, 1) or a0.shape[0] < 1:
            raise ValueError(f"actions0 must be [T], [T, {c.num_envs}] or [T, {c.num_envs}, 1], got {tuple(torch.as_tensor(actions0).shape)}")
        obs, rewards = self._rollout(u0, v0, p0, a0.contiguous())
        before = rewards.sum(dim=0)
        actions, grad = self.sweep(obs)
        obs, rewards = self._rollout(u0, v0, p0, actions)
        return {"actions": actions, "grad": grad, "reward_before": before, "reward_after": rewards.sum(dim=0), "rewards": rewards,
                "obs": obs}
