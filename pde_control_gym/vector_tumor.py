"""TumorVecEnv -- a batch of ``TherapyWrapper(BrainTumor1D)`` patients behind one VecEnv-style object.

What the reference offers one patient at a time (examples/BrainTumor1D: ``TherapyWrapper(gym.make("PDEControlGym-BrainTumor1D",
**params))`` driven by SAC/PPO) happens here for ``num_envs`` patients with a handful of launches per step and no host
synchronisation: the agent only sees treatment days; growth (at reset) and post-therapy (after the last dose) run as
in-kernel day loops (``pdegym_tumor_advance``), finished patients restart inside the same ``step`` (SB3 auto-reset
semantics: ``infos[i]["terminal_observation"]``).  Per-patient semantics follow brain_tumor_env.py:385-505 including
the ``weekends`` option (two untreated days after five consecutive treatment days).

``fused_step=True``: the whole wrapper step is ONE launch (``pdegym_tumor_therapy_step``), bit-identical to the sequence above;
``DeviceRollout(venv, policy, T, one_launch=True)`` goes further and runs T wrapper steps with the policy inside one launch
(``pdegym_tumor_rollout``).  Both are opt-in: the default stays the launch sequence.
"""
from __future__ import annotations

import numpy as np

from pde_control_gym._compat import spaces
from pde_control_gym.vector import BatchedVecEnv


class TumorVecEnv(BatchedVecEnv):
    _checkpoint_attrs = ("_consecutive", "treatment_calls", "soft_constraint_violations")

    one_launch_opt_in = True               # DeviceRollout(one_launch=True) asks one_launch_gap; one_launch=None keeps step_tensor
    one_launch_obs_noise = False           # (the tumour rollout kernel has no obs_noise input)

    def __init__(self, num_envs: int, weekends: bool = False, device="cuda", backend=None, t_benchmark=None, fused_step: bool = False,
                 **kw):
        import torch
        from pdecontrolgym_amd.batch_tumor import TumorBatch
        from pdecontrolgym_amd import _native as N
        self._N = N
        self.num_envs = int(num_envs)
        self.device = torch.device(device)
        self.weekends = bool(weekends)
        self.reward_class = kw.pop("reward_class", None)
        kw.pop("normalize", None)
        kw.pop("verbose", None)
        self.reset_init_condition_func = kw.pop("reset_init_condition_func")
        self.core = TumorBatch(num_envs=self.num_envs, device=device, backend=backend, **kw)
        c = self.core
        self.observation_space = spaces.Box(np.full(c.nx, 0, dtype="float64"), np.full(c.nx, c.k, dtype="float64"), dtype=np.float64)
        self.action_space = spaces.Box(np.full(1, 0, dtype="float32"), np.full(1, 1, dtype="float32"))
        self._init_rows = torch.as_tensor(np.asarray(self.reset_init_condition_func(c.X, c.nx), dtype=np.float64), device=self.device)
        self._consecutive = torch.zeros(self.num_envs, dtype=torch.int32, device=self.device)
        self.treatment_calls = torch.zeros(self.num_envs, dtype=torch.int64, device=self.device)
        self.soft_constraint_violations = torch.zeros(self.num_envs, dtype=torch.int64, device=self.device)
        self.t_benchmark = None
        if t_benchmark is not None:
            self.t_benchmark = t_benchmark
            c.set_benchmark(t_benchmark)
        self._actions = None
        # fused_step: step_tensor is one pdegym_tumor_therapy_step launch.  The wrapper's state travels as one dictionary: the
        # counters above (in place), the initial row(s), and two buffers the kernels write -- the last row of every episode that
        # ended (terminal_obs) and, with weekends, the returned observation (a resting patient returns the treatment day's row)
        self.fused_step = bool(fused_step)
        if self.fused_step:
            gap = c.rollout_gap()
            if gap is not None:
                raise ValueError("fused_step=True is not available: " + gap)
        self._wrap_state = None
        self._finish_vec_env_init()

    def _wrapper_state(self):
        import torch
        if self._wrap_state is None:
            B, nx = self.num_envs, self.core.nx
            self._final_obs = torch.zeros(B, nx, dtype=torch.float64, device=self.device)
            self._fused_obs = torch.zeros(B, nx, dtype=torch.float64, device=self.device) if self.weekends else None
            self._wrap_state = {"weekends": self.weekends, "init": self._init_rows.contiguous(), "consecutive": self._consecutive,
                                "treatment_calls": self.treatment_calls, "soft_constraint_violations": self.soft_constraint_violations,
                                "final_obs": self._final_obs, "obs": self._fused_obs}
        return self._wrap_state

    # ---- TherapyWrapper.benchmark / reset -------------------------------------------------------------------------
    def benchmark(self):
        """Open-loop survival days of every patient (no treatment); stored as ``t_benchmark`` (brain_tumor_env.py:488-503)."""
        import torch
        c = self.core
        c.set_benchmark(float("nan"))
        c.reset(self._init_rows)
        c.advance(self._N.TUMOR_RUN_TO_END)
        tb = c.t["days"][:, 3].to(torch.float64).clone()
        self.t_benchmark = tb
        c.set_benchmark(tb)
        self.reset_tensor()
        return tb

    def reset_tensor(self, mask=None):
        """Restart (``mask``: only those patients) and run the growth stage: the first observation is the first treatment day."""
        c = self.core
        c.reset(self._init_rows, mask=mask)
        c.advance(self._N.TUMOR_RUN_GROWTH, active=mask)
        if mask is None:
            self._consecutive.zero_()
        else:
            self._consecutive.masked_fill_(mask.bool(), 0)
        return c.t["u"]

    def reset(self, seed=None, options=None):
        obs = self.reset_tensor().cpu().numpy().copy()
        self._consume_reset_arguments()
        return obs

    # ---- TherapyWrapper.step for every patient ------------------------------------------------------------------------
    def step_tensor(self, actions):
        """actions [B] (or [B, 1]) = fraction of total_dosage for today's treatment.  Returns device tensors
        (obs [B, nx], reward [B], terminated [B] bool, truncated [B] bool); finished patients have already been restarted
        and their last observation is kept in ``self.terminal_obs``."""
        import torch
        N, c = self._N, self.core
        a = torch.as_tensor(actions, dtype=torch.float64, device=self.device).reshape(self.num_envs)
        if self.fused_step:                                          # the same step as ONE launch (pdegym_tumor_therapy_step)
            W = self._wrapper_state()
            obs, rew, term, trunc = c.therapy_step(a, W)
            self.terminal_obs = W["final_obs"]                       # (rows of patients whose episode ended in this step)
            return obs, rew.clone(), term.bool(), trunc.bool()
        stage = c.t["stage"]
        in_post = stage == N.TUMOR_POST
        in_therapy = stage == N.TUMOR_THERAPY                       # Growth cannot be observed here (reset runs it)
        # Case 1 (:437-446): patients whose therapy is over run to the end of their episode inside one launch
        c.advance(N.TUMOR_RUN_POST, active=in_post)
        # Case 2 (:452-456): one treatment day for the others
        c.step(a, active=in_therapy)
        rew, term, trunc = c.t["reward"], c.t["terminated"].bool(), c.t["truncated"].bool()
        self.treatment_calls += in_therapy
        self.soft_constraint_violations += in_therapy & (rew < 0.0)
        if self.weekends:                                            # :458-472
            # in-place updates: the counter must live in ONE tensor so that a captured hipGraph can be replayed
            self._consecutive.copy_(torch.where(in_therapy, torch.where(a > 0, self._consecutive + 1, torch.zeros_like(self._consecutive)),
                                                self._consecutive))
            rest = in_therapy & (self._consecutive >= 5) & ~(term | trunc)
            self._consecutive.masked_fill_(rest, 0)
            keep = (rew.clone(), c.t["terminated"].clone(), c.t["truncated"].clone())
            seen = c.t["u"].clone()                                  # the wrapper returns the TREATMENT day's row (:456, :481)
            zero = torch.zeros_like(a)
            for _ in range(2):                                       # two untreated days; their outputs are discarded
                c.step(zero, active=rest)
            for dst, src in zip((c.t["reward"], c.t["terminated"], c.t["truncated"]), keep):
                dst.copy_(src)
            rew = c.t["reward"]
        done = term | trunc
        rewards = rew.clone()
        self.terminal_obs = c.t["u"].clone()
        self.reset_tensor(mask=done)
        obs = c.t["u"]
        if self.weekends:
            obs = torch.where((rest & ~done)[:, None], seen, obs)
        return obs, rewards, term, trunc

    def rollout_obs(self):          # (DeviceRollout: the observation IS the engine's one live row)
        return self.core.t["u"]

    def one_launch_gap(self, policy):
        """What keeps ``DeviceRollout(self, policy, T, one_launch=True)`` out of pdegym_tumor_rollout, as a sentence; None when it
        fits: a ``FusedMLP`` of nx inputs and one output that fits the kernel's LDS next to the rows, or ``policy=None`` (commands
        given ahead in ``DeviceRollout.actions``)."""
        gap = self.core.rollout_gap()
        if gap is not None:
            return gap
        if policy is None:
            return None
        if not hasattr(policy, "fits_rollout"):
            return "the policy is not a FusedMLP (or None: commands given ahead in the rollout's actions buffer)"
        if not self.core.policy_fits_rollout(policy):
            return (f"the policy does not fit the rollout kernel: {self.core.nx} inputs, one output, layers of <= 256 units, and its LDS plus "
                    f"two float64 rows of {self.core.nx} nodes for 16 patients within 160 KB (TumorBatch.policy_fits_rollout)")
        return None

    def rollout_one_launch(self, obs, actions, rewards, terminated, truncated, policy=None, clamp="default", noise=None,
                           final_obs_steps=None, **kw):
        """T wrapper steps (and the policy) in ONE launch; ``terminal_obs`` holds the last row of every episode that ended in it
        (the latest one per patient) -- or, with ``final_obs_steps`` [T, B, nx], row (t, b) of that tensor holds the last row of the
        episode that step t ended, and ``terminal_obs`` is left as it was."""
        if kw:
            raise ValueError(f"the tumour rollout kernel takes no {sorted(kw)}")
        W = self._wrapper_state()
        extra = {} if final_obs_steps is None else {"final_obs_steps": final_obs_steps}
        self.core.rollout(obs, actions, rewards, terminated, truncated, policy=policy, clamp=clamp,
                          noise=noise if policy is not None else None, wrap_state=W, **extra)
        if final_obs_steps is None:
            self.terminal_obs = W["final_obs"]

    def terminal_obs_gap(self):          # (the wrapper restarts every finished patient itself: nothing to enable)
        return None

    def rollout_final_obs(self):
        return self.terminal_obs

    # ---- SB3 VecEnv face ------------------------------------------------------------------------------------------------
    def step_wait(self):
        obs, rew, term, trunc = self.step_tensor(np.asarray(self._actions, dtype=np.float64).reshape(self.num_envs))
        done = (term | trunc).cpu().numpy()
        tr = trunc.cpu().numpy()
        infos = [{} for _ in range(self.num_envs)]
        if done.any():
            tob = self.terminal_obs.cpu().numpy()
            for i in np.nonzero(done)[0]:
                infos[i]["terminal_observation"] = tob[i].copy()
                infos[i]["TimeLimit.truncated"] = bool(tr[i] and not term[i])
        return obs.cpu().numpy().copy(), rew.cpu().numpy().copy(), done, infos
