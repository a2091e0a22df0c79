"""Batched Aw-Rascle-Zhang traffic environments (float64) on device tensors.

Mirrors the constructor arithmetic of the reference's TrafficPDE1D (environments1d/traffic_arz_env.py:24-101):
``M = len(np.arange(0, X+dx, dx))``, equilibrium velocity ``Veq(rho) = vm (1 - rho/rm)``, ``qs = rs * vs``, action
bounds ``[0.8 qs, 1.2 qs]`` fixed at construction, initial profile ``rs (sin(3 x/L pi) 0.1 + 1)``.
"""
from __future__ import annotations

import numpy as np

from . import _native as N
from .checkpoint import EngineCheckpoint
from .hostio import PackLayout, as_kernel_input
from .policy import fits_rollout_kernel


class TrafficBatch(EngineCheckpoint):
    def __init__(self, T: float, dt: float, X: float, dx: float, simulation_type: str = "inlet", v_max: float = 40,
                 ro_max: float = 0.16, tau: float = 60, limit_pde_state_size: bool = False, control_freq: int = 1,
                 num_envs: int = 1, device="cuda", backend=None):
        import torch
        if simulation_type not in N.TRAFFIC_SIM:
            raise ValueError("Invalid simulation type")
        assert isinstance(control_freq, int) and control_freq >= 1, \
            f"control_freq must be a positive integer (got {control_freq} of type {type(control_freq).__name__})"
        self.T, self.dt, self.X, self.dx = T, dt, X, dx
        self.simulation_type = simulation_type
        self.vm, self.rm, self.tau = v_max, ro_max, tau
        self.limit, self.control_freq = bool(limit_pde_state_size), control_freq
        self.x = np.arange(0, X + dx, dx)
        self.M = len(self.x)
        self.num_envs = int(num_envs)
        self.device = torch.device(device)
        self.action_dim = 2 if simulation_type == "both" else 1
        self._bind_backend(backend)
        P = N.ParamsTraffic()
        P.M, P.control_freq, P.sim, P.limit = self.M, control_freq, N.TRAFFIC_SIM[simulation_type], int(self.limit)
        P.dt, P.dx, P.T, P.vm, P.rm, P.tau = dt, dx, T, v_max, ro_max, tau
        self.params = P
        B, M, dev, f64 = self.num_envs, self.M, self.device, torch.float64
        # the initial profile uses NumPy's sin so that resets are bit-identical to the reference's (:256)
        self.profile = torch.as_tensor(np.sin(3 * self.x / X * np.pi) * 0.1 + np.ones(M), dtype=f64, device=dev)
        # everything a host-facing caller reads after a step lives in ONE allocation (hostio.PackLayout): the single environment
        # fetches observation, fields, clock, reward and flags with one device-to-host copy
        u8 = torch.uint8
        self.pack_layout = PackLayout([("obs0", (B, 2 * M), f64), ("obs1", (B, 2 * M), f64), ("r", (B, M), f64), ("y", (B, M), f64),
                                       ("time", (B,), f64), ("reward", (B,), f64), ("done", (B,), u8), ("truncated", (B,), u8)])
        self.host_pack, pv = self.pack_layout.allocate(dev)
        self.t = {
            "r": pv["r"], "y": pv["y"],
            "action": torch.zeros(B, 2, dtype=f64, device=dev), "time": pv["time"],
            "rs": torch.zeros(B, dtype=f64, device=dev), "qs_clip": torch.zeros(B, dtype=f64, device=dev),
            "obs": None, "reward": pv["reward"],
            "done": pv["done"], "truncated": pv["truncated"],
        }
        self._obs = [pv["obs0"], pv["obs1"]]
        self._flip = 0
        self.rs_version, self._rs_host = 0, None      # counts the changes of rs and of the reset pool (reset, *_auto_reset, pool_refreshed)
        self.t["obs"] = self._obs[0]

    def Veq(self, rho):
        return self.vm * (1 - rho / self.rm)

    @property
    def obs_segment(self) -> str:
        """The segment of ``host_pack`` / ``pack_layout`` that holds the current observation."""
        return "obs1" if self.t["obs"] is self._obs[1] else "obs0"

    def set_action_bounds(self, qs_clip):
        import torch
        self.t["qs_clip"] = torch.as_tensor(qs_clip, dtype=torch.float64, device=self.device).reshape(self.num_envs).contiguous()

    def reset(self, rs, mask=None):
        """rs [B]: steady-state density per instance; where ``mask`` is given only those instances restart."""
        import torch
        host = None if torch.is_tensor(rs) else np.asarray(rs, dtype=np.float64).reshape(self.num_envs).copy()
        rs = torch.as_tensor(rs, dtype=torch.float64, device=self.device).reshape(self.num_envs).contiguous()
        if mask is not None:
            mask = self._as_mask(mask)
            self.t["rs"] = torch.where(mask.bool(), rs, self.t["rs"]).contiguous()
            if host is not None and self._rs_host is not None:
                host = np.where(mask.bool().cpu().numpy(), host, self._rs_host)
            else:
                host = None
        else:
            self.t["rs"] = rs
        # rs_version: what a controller built from the densities compares (TrafficBacksteppingController); a reset that hands over
        # the densities the engine already holds (every restart of the non-train types) leaves it alone
        if host is None or self._rs_host is None or not np.array_equal(host, self._rs_host):
            self.rs_version += 1
        self._rs_host = host
        self.backend.traffic_reset(self.params, self.t, self.profile, mask, self.num_envs)
        return self.t["obs"]

    def enable_auto_reset(self, rs_pool, keep_final_obs: bool = True):
        """Fused VecEnv auto-reset: an instance whose step ends done | truncated restarts inside the same launch (step and
        rollout alike) the way ``TrafficPDE1D.reset`` does, with the steady-state density of pool row (b + k*B) mod P for its
        k-th restart (``rs_pool`` [P]: the reference redraws it in 'outlet-train'); ``t['final_obs']`` keeps the last
        observation of the finished episode."""
        import torch
        pool = torch.as_tensor(rs_pool, dtype=torch.float64, device=self.device).reshape(-1).contiguous()
        self._set_auto_reset({"reset_rs": pool, "reset_profile": self.profile}, keep_final_obs)
        self.rs_version += 1

    def pool_refreshed(self):
        """The caller rewrote ``t['reset_rs']`` in place: the densities of coming episodes may have changed."""
        self.rs_version += 1

    def disable_auto_reset(self):
        self._clear_auto_reset(("reset_rs", "reset_profile"))
        self.rs_version += 1

    def can_rollout(self) -> bool:
        """``rollout`` needs the register-resident kernel (freeways of up to 64 nodes: the reference's grid has 51)."""
        return self.M <= 64 and hasattr(self.backend, "traffic_rollout")

    def policy_fits_rollout(self, policy) -> bool:
        """Whether ``policy`` (a ``FusedMLP``) can run inside the rollout kernel (``FusedMLP.fits_rollout``): 2M inputs, one
        output per command."""
        return self.can_rollout() and fits_rollout_kernel(policy, 2 * self.M, self.action_dim)

    def law_rollout_gap(self, controller):
        """What keeps ``controller`` (a ``TrafficBacksteppingController``) out of the one-launch rollout kernel with the control
        law inside (pdegym_traffic_backstep_rollout), as a sentence; None when it fits: freeways of at most 64 nodes and a
        controller attached to this engine (asked of the controller: ``rollout_gap``)."""
        if not hasattr(controller, "rollout_law") or not hasattr(controller, "rollout_gap"):
            return "the policy is not a controller with a rollout descriptor (TrafficBacksteppingController.rollout_law)"
        if not hasattr(self.backend, "traffic_backstep_rollout"):
            return "the backend has no traffic_backstep_rollout"
        if self.M > 64:
            return f"freeways of {self.M} nodes (the kernel keeps freeways of up to 64 nodes in registers)"
        return controller.rollout_gap(self)

    def rollout(self, obs, actions, rewards, done, truncated, policy=None, clamp="default", noise=None, law=None, final_obs_steps=None):
        """T env-steps in ONE launch (include/pdegym.h: pdegym_traffic_rollout): step t takes ``actions[t]`` ([T, B, action_dim]),
        writes ``obs[t + 1]`` ([T+1, B, 2M]), ``rewards[t]``, ``done[t]``, ``truncated[t]`` -- bit-identical to T ``step`` calls.
        With ``policy`` (a ``FusedMLP``) the commands are computed inside the launch from ``obs[t]`` (``obs[0]`` = the current
        observation, supplied by the caller) and written to ``actions``; ``noise`` [T, B, action_dim] float32 is added before
        the clamp.  With ``law`` (an ``N.TrafficBackstep`` descriptor: ``TrafficBacksteppingController.rollout_law``) the
        backstepping law forms the commands inside the launch instead (pdegym_traffic_backstep_rollout), bit-identical to control
        launch + ``step`` per env-step.  The engine's own observation / reward / flag tensors receive the values of the last step.
        ``final_obs_steps`` float64 [T, B, 2M] (needs ``enable_auto_reset``): row (t, b) receives the last observation of the episode
        that step t ended; no other row is written, and ``t['final_obs']`` is not."""
        if not self.can_rollout():
            raise ValueError("rollout needs freeways of at most 64 nodes")
        if law is not None and policy is not None:
            raise ValueError("rollout takes a policy or a law, not both")
        if policy is not None and not self.policy_fits_rollout(policy):
            raise ValueError("this policy cannot run inside the rollout kernel (see policy_fits_rollout)")
        extra = {} if final_obs_steps is None else {"final_obs_steps": final_obs_steps}      # (backends without the keyword stay valid)
        if law is not None:
            self.backend.traffic_backstep_rollout(self.params, self.t, obs, actions, rewards, done, truncated, self.num_envs, law, **extra)
        else:
            net = policy.rollout_net(obs, actions, clamp, noise) if policy is not None else None
            self.backend.traffic_rollout(self.params, self.t, obs, actions, rewards, done, truncated, self.num_envs, policy=net, **extra)
        self.t["obs"].copy_(obs[-1])
        self.t["reward"].copy_(rewards[-1])
        self.t["done"].copy_(done[-1])
        self.t["truncated"].copy_(truncated[-1])
        return obs, rewards, done, truncated

    def step(self, action):
        """action [B] / [B,1] (inlet, outlet) or [B,2] ('both'). Returns (obs [B,2M], reward, done, truncated)."""
        import torch
        a = as_kernel_input(action, torch.float64, self.device, (self.num_envs, -1))     # (a pinned host tensor is read in place)
        if a.shape[1] > 2 or (self.action_dim == 2 and a.shape[1] != 2):
            raise ValueError(f"action must be [B] / [B, 1] / [B, 2] ('both' needs two columns), got {tuple(a.shape)}")
        self.t["action"] = a.contiguous()       # used in place: the kernel takes the column count as the stride
        self._flip_obs()
        self.backend.traffic_step(self.params, self.t, self.num_envs)
        return self.t["obs"], self.t["reward"], self.t["done"], self.t["truncated"]
