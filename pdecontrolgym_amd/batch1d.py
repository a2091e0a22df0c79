"""Batched 1D PDE environments (transport / reaction-diffusion) on device tensors.

``PDEBatch1D`` owns the per-instance state of B independent environments as PyTorch-ROCm tensors and
advances all of them with ONE kernel launch per env-step through the C ABI (include/pdegym.h).  It
mirrors the reference's constructor arithmetic:

    nt = int(round(T/dt)+1), nx = int(round(X/dx))          environments1d/base_env_1d.py:23-24
    S  = int(round(control_sample_rate/dt))                 environments1d/hyperbolic.py:137
    parabolic rows carry a ghost node (nx+1)                environments1d/parabolic.py:124
    sensing / control enums and their error strings         environments1d/hyperbolic.py:48-124

The full trajectory ``u[nt, nx]`` the reference keeps per environment (80 MB each at the shipped
parabolic settings) is NOT kept: only the live row plus the three scalars TunedReward1D needs
(SURVEY.md section 8a, rows R1/R2).  ``record_history=True`` restores the full history on device for
small batches (custom reward callbacks, plotting).
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

from . import _native as N
from .checkpoint import EngineCheckpoint
from .policy import fits_rollout_kernel


@dataclass
class RewardSpec:
    """Which reward the step kernel evaluates in its epilogue."""
    kind: int = N.REWARD_NONE
    nt: int = 0
    truncate_penalty: float = -1e-4
    terminate_reward: float = 1e2
    horizon: int = N.HORIZON_TEMPORAL      # NormReward kinds: HORIZON_DIFFERENTIAL = +||u[t] - u[t-1]||, HORIZON_T = -(mean of the
    t_horizon: int = 5                     # last t_horizon row norms) -- both evaluated by the step kernels only


_BAD_SENSING_LOC = "Invalid sensing_loc parameter. Please use 'full', 'collocated', or 'opposite'. See documentation for details."
_BAD_SENSING_TYPE = "Invalid sensing_type parameter. Please use 'Neumann' or 'Dirchilet'. See documentation for details."
_BAD_CONTROL = "Invalid control_type parameter. Please use 'Neumann' or 'Dirchilet'. See documentation for details."
_PARABOLIC_OPPOSITE_DIR = "In the parabolic PDE system, u(0, t)=0 and so Dirchilet sensing at u(0, t) is not viable. See documentation for details."


def sensing_mode(kind: str, control_type: str, sensing_loc: str, sensing_type) -> int:
    """Maps the reference's (control_type, sensing_loc, sensing_type) table onto one PDEGYM_SENSE_* code,
    raising the same bare ``Exception`` messages (hyperbolic.py:66-124, parabolic.py:66-122)."""
    if sensing_loc not in ("full", "collocated", "opposite"):
        raise Exception(_BAD_SENSING_LOC)
    if control_type not in ("Neumann", "Dirchilet"):
        raise Exception(_BAD_CONTROL)
    if sensing_loc == "full":
        return N.SENSE_FULL
    if sensing_loc == "collocated":
        return N.SENSE_LAST if control_type == "Neumann" else N.SENSE_LAST_DERIV
    if sensing_type == "Neumann":
        return N.SENSE_FIRST_DERIV
    if sensing_type == "Dirchilet":
        if kind == "parabolic":
            raise Exception(_PARABOLIC_OPPOSITE_DIR)
        return N.SENSE_FIRST
    raise Exception(_BAD_SENSING_TYPE)


class PDEBatch1D(EngineCheckpoint):
    def __init__(self, kind: str, T: float, dt: float, X: float, dx: float, control_sample_rate: float,
                 control_type: str = "Dirchilet", sensing_loc: str = "full", sensing_type="Dirchilet",
                 normalize: bool = False, max_control_value: float = 20, limit_pde_state_size: bool = False,
                 max_state_value: float = 1e10, reward: RewardSpec | None = None, num_envs: int = 1,
                 device="cuda", backend=None, record_history: bool = False, state_in_obs: bool = True, flux: str = "linear"):
        import torch
        assert kind in ("transport", "parabolic")
        if flux not in ("linear", "burgers") or (flux == "burgers" and kind != "transport"):
            raise ValueError("flux must be 'linear' (the reference's transport term) or 'burgers' (extension, transport only)")
        self.kind, self.flux = kind, flux
        self.T, self.dt, self.X, self.dx = T, dt, X, dx
        self.nt = int(round(T / dt) + 1)
        self.nx = int(round(X / dx))
        self.n = self.nx + (1 if kind == "parabolic" else 0)
        self.substeps = int(round(control_sample_rate / dt))
        self.sensing = sensing_mode(kind, control_type, sensing_loc, sensing_type)
        self.obs_dim = self.n if self.sensing == N.SENSE_FULL else 1
        self.num_envs = int(num_envs)
        self.device = torch.device(device)
        self.reward_spec = reward or RewardSpec()
        self.control_sample_rate, self.control_type = control_sample_rate, control_type
        self.sensing_loc, self.sensing_type, self.normalize = sensing_loc, sensing_type, bool(normalize)
        self.max_control_value, self.max_state_value = max_control_value, max_state_value
        self.limit_pde_state_size = limit_pde_state_size
        self._bind_backend(backend)

        P = N.Params1D()
        P.n, P.nt, P.substeps = self.n, self.nt, self.substeps
        P.control_type = N.CONTROL[control_type]
        P.normalize = 1 if normalize else 0
        P.sensing = self.sensing
        P.limit_state = 1 if limit_pde_state_size else 0
        P.reward_kind = self.reward_spec.kind
        P.reward_nt = int(self.reward_spec.nt)
        P.reward_horizon = int(self.reward_spec.horizon) if self.reward_spec.kind >= N.REWARD_NORM_L1 else N.HORIZON_TEMPORAL
        P.reward_t_horizon = int(self.reward_spec.t_horizon) if P.reward_horizon == N.HORIZON_T else 0
        P.dt, P.dx = dt, dx                       # ctypes c_float rounds the Python double to float32
        P.F = dt / (dx ** 2)                      # parabolic.py:138, computed in double then cast
        P.rdx = 1.0 / float(C.c_float(dx).value)  # reciprocal of the float32 dx, in double (see pdegym.h)
        P.max_control = max_control_value
        P.dt64, P.dx64, P.max_control64 = dt, dx, max_control_value   # the Python doubles, for float64 operands
        P.beta_f64, P.action_kind = 0, N.ACTION_F32
        P.max_state = min(max_state_value, 3.4028234663852886e38)
        P.flux = N.FLUX_BURGERS if flux == "burgers" else N.FLUX_LINEAR
        P.truncate_penalty = self.reward_spec.truncate_penalty
        P.terminate_reward = self.reward_spec.terminate_reward
        self.params = P

        B, n, dev = self.num_envs, self.n, self.device
        f32 = torch.float32
        # reward, terminated and truncated share one allocation (4B + B + B bytes): a host-facing caller fetches the three with
        # ONE device-to-host copy (pde_control_gym.PDEVecEnv.step_wait) instead of three latency-bound ones
        self.host_pack = torch.zeros(6 * B, dtype=torch.uint8, device=dev)
        self.t = {
            "u": torch.zeros(B, n, dtype=f32, device=dev),
            "beta": torch.zeros(B, n, dtype=f32, device=dev),
            "action": torch.zeros(B, dtype=f32, device=dev),
            "time_index": torch.zeros(B, dtype=torch.int32, device=dev),
            "bsum": torch.zeros(B, dtype=torch.float64, device=dev),
            "ring": torch.zeros(B, N.RING, dtype=f32, device=dev),
            "obs": None,
            "reward": self.host_pack[:4 * B].view(f32),
            "norm_now": torch.zeros(B, dtype=f32, device=dev),
            "norm_back": torch.zeros(B, dtype=f32, device=dev),
            "terminated": self.host_pack[4 * B:5 * B],
            "truncated": self.host_pack[5 * B:],
            "history": torch.zeros(B, self.nt, n, dtype=f32, device=dev) if record_history else None,
            "reset_init": None,
            "final_obs": None,
            "reset_beta": None,
            "reset_count": None,
        }
        self._obs = [torch.zeros(B, self.obs_dim, dtype=f32, device=dev) for _ in range(2)]
        self._flip = 0
        self.t["obs"] = self._obs[0]
        # Full-state sensing: the observation IS the row (hyperbolic.py:72-75), so the state lives only in the observation
        # tensors -- a step reads the previous observation (bufs.state_in) and writes the next one, one row store instead of
        # two.  ``t["u"]`` then names the CURRENT observation tensor (rebound after every step / reset).
        self.state_in_obs = self.sensing == N.SENSE_FULL and not record_history and state_in_obs
        self.t["state_in"] = None
        if self.state_in_obs:
            self.t["u"] = self.t["obs"]

    # ---- state accessors ---------------------------------------------------------------------------
    @property
    def u(self):
        return self.t["u"]

    @property
    def time_index(self):
        return self.t["time_index"]

    # ---- API -----------------------------------------------------------------------------------------
    def set_beta(self, beta, dtype=None):
        """beta: [n] (shared) or [B, n].  Its dtype selects the arithmetic, as in the reference: float32 -> the float32
        kernels; float64 (what ``np.ones(nx)`` or an un-cast ``np.cos(...)`` gives) or an integer type -> the reference's
        mixed-precision update, evaluated in double and rounded once per stored row (hyperbolic.py:146-155,
        parabolic.py:143-144; slower kernel).  ``dtype=torch.float32`` forces the float32 path."""
        import torch
        beta = torch.as_tensor(beta)
        if dtype is None:
            dtype = torch.float32 if beta.dtype in (torch.float32, torch.float16, torch.bfloat16) else torch.float64
        beta = beta.to(device=self.device, dtype=dtype).contiguous()
        if beta.shape[-1] != self.n:
            raise ValueError(f"beta must have {self.n} nodes, got {tuple(beta.shape)}")
        self.t["beta"] = beta
        self.params.beta_f64 = 1 if dtype == torch.float64 else 0
        self._drop_prepared_call()

    def reset(self, init, beta=None, mask=None):
        """(Re)start instances from ``init`` [B, n]; where ``mask`` [B] (uint8/bool) is given only those."""
        import torch
        if beta is not None:
            self.set_beta(beta)
        init = torch.as_tensor(init, dtype=torch.float32, device=self.device).contiguous()
        if init.shape != (self.num_envs, self.n):
            raise ValueError(f"init must be [{self.num_envs}, {self.n}], got {tuple(init.shape)}")
        if mask is not None:
            mask = self._as_mask(mask)     # a masked reset writes into the CURRENT obs buffer: untouched instances keep theirs
        else:
            self._flip_obs()
        if self.state_in_obs:
            self.t["u"] = None                      # the reset rows go to the observation buffer only
        self.backend.reset1d(self.params, self.t, init, mask, self.num_envs)
        if self.state_in_obs:
            self.t["u"] = self.t["obs"]
        return self.t["obs"]

    def enable_auto_reset(self, init_pool, keep_final_obs: bool = True, beta_pool=None):
        """Fused VecEnv auto-reset: an instance that ends a step terminated|truncated restarts inside the same kernel launch
        (no host round trip).  ``init_pool`` is a caller-owned [P, n] tensor with P >= B rows; the k-th restart of instance b
        takes row (b + k*B) mod P, so with P > B consecutive episodes of one instance start from different rows.  With
        ``beta_pool`` [P, n] (same dtype as the current beta) the plant parameter is redrawn from the same row -- the
        reference calls BOTH reset callbacks at every reset (hyperbolic.py:207-209).  Pools may be refreshed between steps
        (e.g. re-sampled on device)."""
        import torch
        pool = torch.as_tensor(init_pool, dtype=torch.float32, device=self.device).contiguous()
        if pool.dim() != 2 or pool.shape[1] != self.n or pool.shape[0] < self.num_envs:
            raise ValueError(f"init_pool must be [P >= {self.num_envs}, {self.n}], got {tuple(pool.shape)}")
        bp = None
        if beta_pool is not None:
            if self.t["beta"].dim() == 1:        # a shared row cannot be redrawn per instance: give every instance its own
                self.t["beta"] = self.t["beta"].unsqueeze(0).repeat(self.num_envs, 1).contiguous()
            bp = torch.as_tensor(beta_pool).to(device=self.device, dtype=self.t["beta"].dtype).contiguous()
            if bp.shape != pool.shape:
                raise ValueError(f"beta_pool must have the shape of init_pool {tuple(pool.shape)}, got {tuple(bp.shape)}")
        self._set_auto_reset({"reset_init": pool, "reset_beta": bp}, keep_final_obs)

    def disable_auto_reset(self):
        self._clear_auto_reset(("reset_init", "reset_beta"))

    def step(self, action, out_obs=None, out_reward=None, out_terminated=None, out_truncated=None, action_kind=None):
        """Advance every instance by one env-step (S sub-steps). action: [B] tensor.
        Returns (obs, reward, terminated, truncated) device tensors (uint8 flags).  The ``out_*`` tensors, when given,
        receive the outputs directly (contiguous, right dtype/shape) -- e.g. slot t of a rollout buffer.
        ``action_kind``: how NumPy would type the reference's ``control`` argument (_native.ACTION_F32 / _F64 / _WEAK, see
        include/pdegym.h); default: float64 tensors -> ACTION_F64, everything else -> float32."""
        import torch
        action = torch.as_tensor(action)
        if action_kind is None:
            action_kind = N.ACTION_F64 if action.dtype == torch.float64 else N.ACTION_F32
        adt = torch.float32 if action_kind == N.ACTION_F32 else torch.float64
        if action.dtype == adt and action.device == self.device and action.dim() == 1 and action.shape[0] == self.num_envs and action.is_contiguous():
            a = action                      # already what the kernel reads (the VecEnv face's staging tensor): no torch dispatch
        else:
            a = action.to(device=self.device, dtype=adt).reshape(self.num_envs).contiguous()
        self.t["action"] = a
        self.params.action_kind = action_kind
        prev = self.t["obs"]
        self._flip_obs(out_obs, avoid=prev if self.state_in_obs else None)
        if self.state_in_obs:
            if self.t["obs"].data_ptr() == prev.data_ptr():
                raise ValueError("out_obs must not be the tensor that holds the current observation (it is the state)")
            self.t["state_in"], self.t["u"] = prev, None
        for key, out in (("reward", out_reward), ("terminated", out_terminated), ("truncated", out_truncated)):
            if out is not None:
                self.t[key] = out
        self.backend.step1d(self.kind, self.params, self.t, self.num_envs)
        if self.state_in_obs:
            self.t["u"] = self.t["obs"]
        return self.t["obs"], self.t["reward"], self.t["terminated"], self.t["truncated"]

    # ---- batch-of-one face: command in / results out through ONE pinned host allocation ------------------------------
    def enable_host_io(self):
        """Host-facing mode of the single environments (``EngineCheckpoint._enable_host_io``): the command, observation, reward,
        ||u||, terminated and truncated live in one pinned host allocation, so an env-step is ONE stream operation (the kernel
        launch) + ONE stream synchronisation.  The plant state (row, beta, ring, running sums, time index, history) stays in HBM.
        Not for ``state_in_obs`` engines (their observation IS the state).  Returns the NumPy views ``{"obs", "reward",
        "norm_now", "terminated", "truncated"}`` (valid after ``step_host`` / ``sync_host``; overwritten by the next step)."""
        import numpy as np
        import torch
        if self.state_in_obs:
            raise ValueError("host I/O needs the state in its own tensor (build the engine with state_in_obs=False)")
        if self.num_envs != 1:
            # (the command slot is 8 bytes wide so that one address serves float32 and float64 commands: an array of float32
            # commands would need 4-byte slots -- batches take the staged path of PDEVecEnv)
            raise ValueError("host I/O is the batch-of-one face (num_envs = 1)")
        if self._hio is not None:
            return self._hio["np"]
        B, f32, u8 = self.num_envs, torch.float32, torch.uint8
        nv = self._enable_host_io([("action", (B,), torch.float64), ("obs", (B, self.obs_dim), f32), ("reward", (B,), f32),
                                   ("norm_now", (B,), f32), ("terminated", (B,), u8), ("truncated", (B,), u8)], align=1)
        # one 8-byte slot per instance: a float32 command occupies its first four bytes, a float64 one all eight (the kernel reads
        # the slot as params.action_kind says)
        a64 = nv.pop("action")
        self._hio.update(action=self.t["action"], a64=a64, a32=a64.view(np.float32)[::2], key=None)
        return nv

    def _host_call(self):
        """The prepared C-ABI call of ``step_host`` (argument structures filled once; rebuilt when a tensor of the dictionary
        has been replaced, e.g. a new beta at reset)."""
        io = self._hio
        self.t["action"] = io["action"]
        key = (self.t["beta"].data_ptr(), self.t["u"].data_ptr(), None if self.t["history"] is None else self.t["history"].data_ptr(),
               int(self.params.beta_f64))
        if io["call"] is None or io["key"] != key:
            prep = getattr(self.backend, "prepare_step1d", None)
            if prep is not None:
                io["call"] = prep(self.kind, self.params, self.t, self.num_envs)
            else:                        # (the CPU tests' oracle double: the plain entry point, the command as a typed tensor)
                def call():
                    import torch
                    f32 = self.params.action_kind == N.ACTION_F32
                    self.t["action"] = torch.from_numpy((io["a32"] if f32 else io["a64"]).copy())
                    self.backend.step1d(self.kind, self.params, self.t, self.num_envs)
                io["call"] = call
            io["key"] = key
        return io["call"]

    def step_host(self, value: float, action_kind: int = N.ACTION_F32):
        """One env-step of a batch of one commanded from the host: ``value`` (a Python float) is written into the pinned command
        slot in the precision ``action_kind`` names, the step kernel is launched, the stream is synchronised.  The results are in
        the views ``enable_host_io`` returned."""
        io = self._hio
        if action_kind == N.ACTION_F32:
            io["a32"][:] = value
        else:
            io["a64"][:] = value
        self.params.action_kind = action_kind
        self._host_call()()
        self.sync_host()

    def can_rollout(self) -> bool:
        """True when ``rollout`` applies: every control / sensing combination (round 4: Neumann actuation and scalar sensing
        too), as long as the state has ONE home -- the observation slots with full-state sensing (``state_in_obs``), ``u``
        with scalar sensing -- no history is recorded, the operands are float32, the rows are register-resident, and the
        reward is one the rollout kernels evaluate (not the "differential" horizon)."""
        return bool((self.state_in_obs or self.sensing != N.SENSE_FULL) and self.t["history"] is None and not self.params.beta_f64
                    and self.params.reward_horizon == N.HORIZON_TEMPORAL
                    and self.n <= N.MAX_N1D_REG and hasattr(self.backend, "rollout1d"))

    def policy_fits_rollout(self, policy) -> bool:
        """Whether ``policy`` (a ``FusedMLP``) can be evaluated inside the rollout kernel (``FusedMLP.fits_rollout``): the
        observation (the row of at most 513 nodes, or the one sensed value) as its input and one output."""
        return self.can_rollout() and self.n <= 513 and fits_rollout_kernel(policy, self.obs_dim, 1)

    def law_rollout_gap(self, law):
        """What keeps ``law`` (a ``BacksteppingController``) out of the one-launch rollout kernel with the control law inside
        (pdegym_*_backstep_rollout), as a sentence; None when it fits: the register-resident corner of ``rollout`` -- Dirichlet
        actuation, full-state sensing, the linear flux, rows of at most 512 (transport) / 513 (parabolic) nodes -- and a controller attached to this engine
        (asked of the controller: ``rollout_gap``)."""
        if not hasattr(law, "rollout_law") or not hasattr(law, "rollout_gap"):
            return "the policy is not a controller with a rollout descriptor (BacksteppingController.rollout_law)"
        if not hasattr(self.backend, "backstep_rollout1d"):
            return "the backend has no backstep_rollout1d"
        if self.control_type != "Dirchilet":
            return f"{self.control_type} actuation (the kernel covers Dirichlet actuation; others take the two-launch path)"
        if self.sensing != N.SENSE_FULL:
            return "scalar sensing (the law reads the whole row: sensing_loc='full')"
        if self.flux != "linear":
            return f"the {self.flux} flux (the law exists for the linear transport term)"
        most = 513 if self.kind == "parabolic" else 512          # 8 slots per lane (node 0 of a parabolic row is not a slot)
        if self.n > most:
            return f"rows of {self.n} nodes (the kernel keeps {self.kind} rows of up to {most} nodes in registers)"
        if not self.can_rollout():
            return "the engine cannot roll out in one launch (state with one home: state_in_obs, no history; float32 beta; temporal reward horizon)"
        return law.rollout_gap(self)

    def law_fits_rollout(self, law) -> bool:
        """Whether ``rollout(..., policy=law)`` can evaluate the controller inside the launch (``law_rollout_gap`` says why not)."""
        return self.law_rollout_gap(law) is None

    def rollout(self, obs, actions, rewards, terminated, truncated, policy=None, clamp="default", noise=None, obs_noise=None,
                obs_seen=None, final_obs_steps=None):
        """T env-steps in ONE launch (include/pdegym.h: pdegym_*_rollout): step t takes the commands from ``actions[t]`` and
        writes ``obs[t + 1]`` ([T+1, B, obs_dim]), ``rewards[t]``, ``terminated[t]``, ``truncated[t]`` -- bit-identical to T
        calls of ``step(actions[t], out_obs=obs[t + 1], ...)``, fused auto-reset included.  With full-state sensing ``obs[0]``
        is the state the rollout starts from and the engine's current observation (its state) is a copy of ``obs[T]``
        afterwards; with scalar sensing the state is the engine's own ``u`` (advanced in place) and ``obs[0]`` only feeds a
        policy.

        ``policy`` (a ``FusedMLP`` with layers of at most 256 units and one output, see ``policy_fits_rollout``): evaluated
        inside the launch on ``obs[t]`` (+ ``obs_noise[t]`` [T, B, obs_dim], the pre-drawn sensing noise; ``obs_seen[t]``
        receives what the policy read); ``actions[t]`` then RECEIVES the command (after ``noise[t]`` [T, B] float32 and the
        clamp).  A policy with a layer of 65 .. 256 units is evaluated by the 16 waves of a workgroup in ``policy.forward_into``'s
        own MFMA reduction order: commands -- hence whole trajectories -- are bit-identical to the two-launch loop
        (``forward_into`` + ``step``).  A policy whose layers all have <= 64 units sums each neuron in one fmaf chain instead:
        its commands agree with ``forward_into`` to float32 rounding (rtol ~2e-5), NOT bit for bit, and trajectories drift apart
        accordingly -- the environment arithmetic is bit-identical to step calls either way (given the same commands).

        ``policy`` may also be an attached ``BacksteppingController`` that fits (``law_fits_rollout``): the law is evaluated inside the
        launch on ``obs[t]`` (+ ``obs_noise[t]``), ``actions[t]`` receives the command after ``noise[t]`` and the clamp (``clamp``:
        (lo, hi) or None; "default" = none), and everything is bit-identical to ``controller.forward_into`` + ``step`` per env-step,
        in both summation orders, with gains that follow the restarts the fused auto-reset makes inside the launch.

        ``final_obs_steps`` float32 [T, B, obs_dim] (needs ``enable_auto_reset``): row (t, b) receives what ``t['final_obs'][b]`` holds
        after step t of the step loop -- the last observation of the finished episode -- where step t ended the episode of instance
        b; no other row is written, and ``t['final_obs']`` itself is not."""
        if not self.can_rollout():
            raise ValueError("rollout needs a state with one home (full-state sensing: state_in_obs; no history) and float32 operands")
        self.params.action_kind = N.ACTION_F32
        net = None
        extra = {} if final_obs_steps is None else {"final_obs_steps": final_obs_steps}      # (backends without the keyword stay valid)
        if hasattr(policy, "rollout_law"):          # a controller: its descriptor travels with the launch (pdegym_*_backstep_rollout)
            gap = self.law_rollout_gap(policy)
            if gap is not None:
                raise ValueError("this controller cannot run inside the rollout kernel: " + gap)
            law = policy.rollout_law(actions, None if clamp == "default" else clamp, noise)
            self.backend.backstep_rollout1d(self.kind, self.params, self.t, obs, actions, rewards, terminated, truncated, self.num_envs,
                                            law, obs_noise=obs_noise, obs_seen=obs_seen, **extra)
            self.t["obs"].copy_(obs[-1])
            if self.state_in_obs:
                self.t["u"] = self.t["obs"]
            return obs, rewards, terminated, truncated
        if policy is not None:
            if not self.policy_fits_rollout(policy):
                raise ValueError("this policy cannot run inside the rollout kernel (see policy_fits_rollout)")
            net = policy.rollout_net(obs, actions, clamp, noise)
        elif obs_noise is not None or obs_seen is not None:
            raise ValueError("obs_noise / obs_seen shape the policy's input: they need a policy")
        self.backend.rollout1d(self.kind, self.params, self.t, obs, actions, rewards, terminated, truncated, self.num_envs,
                               policy=net, obs_noise=obs_noise, obs_seen=obs_seen, **extra)
        self.t["obs"].copy_(obs[-1])
        if self.state_in_obs:
            self.t["u"] = self.t["obs"]
        return obs, rewards, terminated, truncated

    # ---- checkpoint / resume (pdecontrolgym_amd/checkpoint.py) ---------------------------------------------
    def _checkpoint_meta(self):
        # the reward kind / horizon decide what the norm ring HOLDS (TunedReward1D: 2-norms of look-back rows; NormReward "t-horizon":
        # the reward's own norm of every recent row), sensing / control what the observation and the boundary sums mean: a
        # checkpoint of one configuration must not load silently into another
        return {"engine": "PDEBatch1D", "kind": self.kind, "flux": self.flux, "num_envs": self.num_envs, "n": self.n,
                "nt": self.nt, "substeps": self.substeps, "obs_dim": self.obs_dim, "state_in_obs": bool(self.state_in_obs),
                "reward_kind": int(self.params.reward_kind), "reward_horizon": int(self.params.reward_horizon),
                "reward_t_horizon": int(self.params.reward_t_horizon), "sensing": int(self.sensing),
                "control_type": str(self.control_type)}

    def _after_load(self, sd):
        import torch
        self.params.beta_f64 = 1 if self.t["beta"].dtype == torch.float64 else 0
        if self.state_in_obs:            # the row lives in the observation tensor: "u" names it, it is not a second tensor
            self.t["u"] = self.t["obs"]

    # ---- roofline bookkeeping ---------------------------------------------
    def algorithmic_bytes_per_env_step(self) -> int:
        """Streaming model: each sub-step reads the previous row and beta and writes the new row
        (12 B per node), plus the observation row and ~16 B of scalars per env-step."""
        return self.substeps * 12 * self.n + 4 * self.n + 16

    def compulsory_bytes_per_env_step(self) -> int:
        """What the fused kernel must move: row in, beta in, row out, obs out (+ scalars); with the state in the observation
        tensors the row is written once."""
        return 4 * self.n * (2 if self.state_in_obs else 3) + 4 * self.obs_dim + 64
