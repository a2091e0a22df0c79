"""On-device rollout loop: policy inference and environment stepping never leave the GPU.

The reference trains with SB3, which steps ONE environment per Python call (``DummyVecEnv(n=1)``,
examples/transportPDE/transport1Dppo.py:77-90).  With thousands of instances per launch the per-step host work
(Python, launch latency) becomes the bottleneck at small sub-step counts, so ``DeviceRollout`` records the whole
T-step rollout -- policy forward pass (any torch module), action clamp, environment step with fused auto-reset,
writes into the [T, B, ...] rollout buffers -- into ONE hipGraph and replays it: zero host work per step.
"""
from __future__ import annotations


class DeviceRollout:
    """``policy``: callable mapping an observation tensor [B, obs_dim] to actions [B] (or [B, 1]) on the same device -- any
    torch module, or a ``pdecontrolgym_amd.FusedMLP`` (Linear/Tanh/ReLU stack evaluated, clamped and stored in ONE launch).
    Buffers: ``obs[T+1, B, D]``, ``actions[T, B]`` (``[T, B, action_dim]`` for Navier-Stokes and two-command traffic), ``rewards[T, B]``, ``terminated[T, B]``, ``truncated[T, B]``; with
    ``action_noise=True`` also ``action_noise[T, B]`` (float32), added to the policy output of step t before the clamp.
    With a squashed-Gaussian policy (``FusedMLP.squashed_gaussian`` / ``FusedMLP.from_sb3(policy, stochastic=True)``: SAC's sampling
    actor) ``action_low`` / ``action_high`` are the action BOX the squashed sample is rescaled to, ``action_noise=True`` allocates the
    standard-normal draws ``eps`` (fill with ``ro.action_noise.normal_()``, no ``mul_``: the deviation depends on the state),
    ``action_noise=False`` gives the deterministic actor, and ``actions[t]`` holds the command ``c`` in ``[lo, hi]``; SB3's scaled
    action, which a replay buffer stores, is ``2 (c - lo) / (hi - lo) - 1``.  Step loop, hipGraph and ``one_launch`` all take it.
    ``one_launch``: see the constructor (1D engines with full-state sensing + a small ``FusedMLP``: the rollout is ONE kernel).
    ``one_launch=True`` with an attached ``BacksteppingController`` on a transport / reaction-diffusion environment (Dirichlet
    actuation, full-state sensing, rows of up to 512 (transport) / 513 (parabolic) nodes): the law runs inside the rollout kernel as
    well -- one launch per ``run()``, results bit-identical to the default two launches per env-step, and faster at all three
    measured shapes.  ``one_launch=True`` also takes an attached ``TrafficBacksteppingController`` on a
    TrafficPDE1D environment of up to 64 nodes into the traffic rollout kernel: opt-in, results bit-identical to the two launches per
    env-step (timings: DESIGN.md section 4.9); ``sensing_noise=True`` keeps its two launches (the traffic kernels take no observation
    noise).  ``one_launch=True`` on a BrainTumor1D environment (``TumorVecEnv``) runs the T ``TherapyWrapper`` steps -- treatment
    days, weekend days, post-therapy and growth runs, restarts -- and a ``FusedMLP`` that fits, or commands given ahead
    (``policy=None``, fill ``ro.actions``), in one launch: opt-in, bit-identical to the default path.
    ``terminal_obs=True`` (after ``venv.enable_fused_auto_reset()``; not on NavierStokes2D, not with sensing noise): ``terminal_obs``
    ``[T, B, D]``, zero-filled once, keeps SB3's ``infos[b]["terminal_observation"]`` of every step -- row (t, b) receives the last
    observation of the episode that step t ended (``terminated[t, b] | truncated[t, b]``) while ``obs[t + 1, b]`` is the first of the
    next one; rows of steps that ended nothing are never written.  Every run path fills it with the same bits (DESIGN.md section
    4.21); ``DeviceRolloutBuffer`` bootstraps truncated steps from it."""

    def __init__(self, venv, policy, n_steps: int, use_graph: bool = True, action_low: float = -1.0, action_high: float = 1.0,
                 action_noise: bool = False, one_launch=None, sensing_noise: bool = False, terminal_obs: bool = False):
        import torch
        self.venv, self.policy, self.T = venv, policy, int(n_steps)
        self.lo, self.hi = float(action_low), float(action_high)
        # What depends on the environment family is asked of the environment (BatchedVecEnv.rollout_* / one_launch_fits): the
        # transport / reaction-diffusion and Navier-Stokes engines write straight into the rollout buffers; the other engines
        # (traffic, brain tumour: several launches and device-side masks per step) go through step_tensor and one copy per output
        cur = venv.rollout_obs()
        B, dev, dt = venv.num_envs, cur.device, cur.dtype
        oshape = tuple(cur.shape[1:])                                # (D,) for the 1D engines, (ny, nx, 2) for Navier-Stokes
        self.obs = torch.zeros((self.T + 1, B) + oshape, dtype=dt, device=dev)
        # (Navier-Stokes: [B, action_dim]; traffic 'both': the inlet and the outlet command)
        self.actions = torch.zeros((self.T, B) + venv.rollout_action_shape, dtype=dt, device=dev)
        self.rewards = torch.zeros(self.T, B, dtype=dt, device=dev)
        self.terminated = torch.zeros(self.T, B, dtype=torch.uint8, device=dev)
        self.truncated = torch.zeros(self.T, B, dtype=torch.uint8, device=dev)
        # exploration noise of a stochastic policy: slot t is added to the policy output of step t before the clamp.  The
        # caller fills the buffer in place before each run() (e.g. ``ro.action_noise.normal_().mul_(std)``): a replayed graph
        # reads the new draws.
        self.action_noise = torch.zeros_like(self.actions, dtype=torch.float32) if action_noise else None
        # transport / reaction-diffusion (any control / sensing combination), or traffic, and a FusedMLP of <= 256-unit layers: the WHOLE rollout is one
        # kernel launch (pdegym_*_rollout with the policy inside: no kernel boundary between env-steps, none between policy and step).
        # one_launch=None: whenever it applies; True: required; False: T x (policy launch + step launch) as for the others.
        # A controller with a rollout descriptor (BacksteppingController) inside the launch is opt-in, one_launch=True only:
        # pdegym_*_backstep_rollout, bit-identical to T x (control launch + step launch); timings: DESIGN.md section 4.7.
        # one_launch=None keeps the two launches per env-step for it.
        fits = bool(venv.one_launch_fits(policy))
        if one_launch and not fits and hasattr(policy, "rollout_law"):
            gap = venv.one_launch_law_gap(policy)
            if gap is not None:
                raise ValueError("one_launch=True cannot take this controller into the rollout kernel: " + gap)
            fits = True
        # BrainTumor1D (TumorVecEnv): the wrapper steps and the policy inside pdegym_tumor_rollout, opt-in like the control laws --
        # one_launch=True with a FusedMLP that fits or with policy=None (commands given ahead in ``actions``); one_launch=None keeps
        # the launches of step_tensor.  Bit-identical to them; timings: DESIGN.md section 4.10.
        if one_launch and not fits and getattr(venv, "one_launch_opt_in", False):
            gap = venv.one_launch_gap(policy)
            if gap is not None:
                raise ValueError("one_launch=True cannot take this rollout into the rollout kernel: " + gap)
            fits = True
        if one_launch and not fits:
            raise ValueError("one_launch=True needs a transport / reaction-diffusion engine whose state has one home (any control / "
                             "sensing combination, no history, float32 operands) or a traffic engine of <= 64 nodes, and a FusedMLP "
                             "that fits the rollout kernel (layers of <= 256 units, see policy_fits_rollout)")
        self.one_launch = fits if one_launch is None else bool(one_launch)
        # device-side sensing noise (PDEVecEnv(sensing_noise_tensor_func=...)): the policy reads obs_seen[t] = f(obs[t]) while
        # obs[t] -- the plant state with full-state sensing -- stays clean; the call is part of the captured graph (torch's
        # random generators are graph-safe: every replay draws new numbers).  The one-launch kernel has no such hook.
        self._noise_f = venv.sensing_noise_tensor_func
        # sensing_noise=True: the same hook as ADDITIVE noise the caller draws ahead (fill ``ro.sensing_noise`` [T + 1, B, ...] in
        # place before each run(), e.g. ``ro.sensing_noise.normal_().mul_(sigma)``): obs_seen[t] = obs[t] + sensing_noise[t].
        # This form also runs inside the one-launch rollout kernels (pdegym_rollout1d.obs_noise / obs_seen).
        self.sensing_noise = None
        if sensing_noise:
            if self._noise_f is not None:
                raise ValueError("sensing_noise=True and sensing_noise_tensor_func are two forms of the same hook: use one")
            self.sensing_noise = torch.zeros_like(self.obs)
            self._noise_f = None
        self.obs_seen = torch.zeros_like(self.obs) if (self._noise_f is not None or sensing_noise) else None
        if self._noise_f is not None:
            if one_launch:
                raise ValueError("one_launch=True cannot apply sensing_noise_tensor_func (the policy runs inside the step kernel); "
                                 "sensing_noise=True (pre-drawn additive noise) can")
            self.one_launch = False
        if self.sensing_noise is not None and not venv.one_launch_obs_noise:
            self.one_launch = False          # (the traffic rollout kernel has no obs_noise input)
        # terminal_obs=True: what SB3's VecEnv hands on as infos[b]["terminal_observation"], for every step of the rollout
        self.terminal_obs = None
        if terminal_obs:
            if sensing_noise or self._noise_f is not None:
                raise ValueError("terminal_obs=True cannot be combined with sensing_noise=True / sensing_noise_tensor_func: the agent "
                                 "would see the NOISY terminal observation, and the rollout has no noise slot for a terminal row "
                                 "(sensing_noise is [T + 1, B, ...], one slot per observation slot)")
            gap = venv.terminal_obs_gap()
            if gap is not None:
                raise ValueError("terminal_obs=True: " + gap)
            self.terminal_obs = torch.zeros_like(self.obs[:self.T])
        self.use_graph = bool(use_graph) and dev.type == "cuda"
        self._graph = None
        self._state_buf = None     # observation tensor the captured graph leaves the end state in (see adopt_rollout_obs)

    def _body(self):
        import torch
        if self.one_launch:
            extra = {}
            if self.sensing_noise is not None:
                extra = dict(obs_noise=self.sensing_noise[:self.T], obs_seen=self.obs_seen[:self.T])
            if self.terminal_obs is not None:
                extra = dict(final_obs_steps=self.terminal_obs)
            self.venv.rollout_one_launch(self.obs, self.actions, self.rewards, self.terminated, self.truncated, policy=self.policy,
                                         clamp=(self.lo, self.hi), noise=self.action_noise, **extra)
            if self.sensing_noise is not None:
                torch.add(self.obs[self.T], self.sensing_noise[self.T], out=self.obs_seen[self.T])
            return
        # engines that write into the rollout buffers themselves are pointed at slot 0 first, and get the end state and their
        # own output tensors back afterwards
        with self.venv.rollout_body(self.obs):
            fused = hasattr(self.policy, "forward_into") and self.obs.dtype in (torch.float32, torch.float64)
            seen = self.obs if self.obs_seen is None else self.obs_seen
            for t in range(self.T):
                nz = self.action_noise[t] if self.action_noise is not None else None
                if self.obs_seen is not None:
                    with torch.no_grad():
                        self._see(t, torch)
                if fused:       # pdecontrolgym_amd.FusedMLP: forward pass (+ noise) + action clamp in one launch, written into slot t
                    self.policy.forward_into(seen[t], self.actions[t], clamp=(self.lo, self.hi), noise=nz)
                else:
                    with torch.no_grad():
                        a = self.policy(seen[t]).reshape(self.actions[t].shape)
                        if nz is not None:
                            a = a + nz.to(a.dtype)
                        a = a.clamp(self.lo, self.hi)
                    self.actions[t].copy_(a)
                self.venv.rollout_step(t, self.obs, self.actions, self.rewards, self.terminated, self.truncated)
                if self.terminal_obs is not None:       # the rows this step ended: engine's final_obs -> row t (no other row is written)
                    self.venv.rollout_keep_terminal(self.terminal_obs[t], self.terminated[t], self.truncated[t])
            if self.obs_seen is not None:
                with torch.no_grad():
                    self._see(self.T, torch)

    def _see(self, t, torch):
        """obs_seen[t]: what the policy reads of observation t (sensing_noise_tensor_func, or obs + the pre-drawn noise)."""
        if self.sensing_noise is not None:
            torch.add(self.obs[t], self.sensing_noise[t], out=self.obs_seen[t])
        else:
            self.obs_seen[t].copy_(self._noise_f(self.obs[t]))

    def run(self, first_obs=None):
        """Roll T steps from ``first_obs`` (default: the environment's current observation). Returns self."""
        import torch
        venv = self.venv
        if hasattr(self.policy, "refresh"):      # FusedMLP: pick up optimizer updates before the graph is (re)played
            self.policy.refresh()
        self.obs[0].copy_(venv.rollout_obs() if first_obs is None else first_obs)
        if not self.use_graph:
            self._body()
            return self
        if self._graph is None:
            torch.cuda.synchronize()
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            snapshot = {k: v.clone() for k, v in venv.rollout_state().items()}

            def rewind():
                state = venv.rollout_state()
                for k, v in snapshot.items():
                    if state[k].shape == v.shape:          # (an input slot such as the traffic engine's "action" may have been rebound)
                        state[k].copy_(v)
            self._state_buf = venv.rollout_obs()
            with torch.cuda.stream(side):
                self._body()                               # warm-up on the side stream (allocator, lazy init)
                rewind()                                   # ... then rewind the environment state
                self._graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(self._graph, stream=side):
                    self._body()
            torch.cuda.current_stream().wait_stream(side)
            rewind()
        self._graph.replay()
        venv.adopt_rollout_obs(self._state_buf)
        return self
