"""BrainTumor1D and TherapyWrapper -- 1D reaction-diffusion glioma growth under radiotherapy (interface of the
reference's environments1d/brain_tumor_env.py:10-505).

The density row lives on the GPU in float64; one ``step`` is one simulated day in one kernel launch
(pdecontrolgym_amd/csrc/pdegym_tumor.hip): finite-difference update with the radiation kill term, T1/T2 MRI radii,
the Growth -> Therapy -> Post-Therapy stage machine, its day counters, terminate/truncate.  The host keeps what the
reference keeps as Python attributes (``stage``, ``remaining_dosage``, the ``*Days`` counters, ``t_benchmark``,
``t1_radius_idx_vs_time``, ``dosage_vs_time``) by reading the handful of scalars the kernel returns.  Bit parity with
the reference: the kill fraction ``1 - exp(-alpha*BED)`` and the toxicity reward's powers are evaluated on the host with
the same NumPy / Python calls the reference makes, everything else is IEEE arithmetic in the reference's order.
"""
from __future__ import annotations

from typing import Optional

import numpy as np

from pde_control_gym._compat import Wrapper, spaces
from pde_control_gym.src.environments1d.base_env_1d import PDEEnv1D

_STAGES = ("Growth", "Therapy", "Post-Therapy")


class BrainTumor1D(PDEEnv1D):
    """:param t1_detection_threshold, t2_detection_threshold: fraction of ``k`` visible on T1Gd / T2 MRI.
    :param dosage_termination_threshold: therapy ends once less than this many Gy remain.
    :param D, rho: diffusion (mm^2/day) and proliferation (1/day).  :param alpha, alpha_beta_ratio: radiosensitivity.
    :param k: carrying capacity (cells/mm).  :param t1_detection_radius, t1_death_radius: mm.
    :param reset_init_condition_func: ``f(X, nx) -> row``.  :param total_dosage: Gy.  :param verbose: print progress.
    Extra: ``device``, ``record_history`` (default True: keeps ``env.u[nt, nx]`` on the host like the reference)."""

    u = None        # plain attribute here (the trajectory array), not the base class's device view

    def __init__(self, t1_detection_threshold: float = 0.8, t2_detection_threshold: float = 0.16,
                 dosage_termination_threshold: float = 0.1, D: float = 0.2, rho: float = 0.03, alpha: float = 0.04,
                 alpha_beta_ratio: int = 10, k: float = 1e5, t1_detection_radius: int = 15, t1_death_radius: int = 35,
                 reset_init_condition_func=None, total_dosage=None, verbose=True, device="cuda", backend=None,
                 record_history=True, **kwargs):
        super().__init__(**kwargs)
        from pdecontrolgym_amd.batch_tumor import TumorBatch
        self.verbose = verbose
        self.nx = int(round(self.X / self.dx) + 1)
        self._core = TumorBatch(self.T, self.dt, self.X, self.dx, total_dosage, t1_detection_threshold,
                                t2_detection_threshold, dosage_termination_threshold, D, rho, alpha, alpha_beta_ratio, k,
                                t1_detection_radius, t1_death_radius, num_envs=1, device=device, backend=backend,
                                record_history=bool(record_history))
        self._record = bool(record_history)
        self.u = np.zeros((self.nt, self.nx)) if self._record else np.zeros((1, self.nx))
        self.t1_radius_idx_vs_time = np.zeros(self.nt)
        self.t1_radius_idx_vs_time[0] = np.nan
        self.dosage_vs_time = np.zeros(self.nt)
        self.xScale = self._core.xScale
        if self.verbose:
            print(f"nx: {self.nx}, nt: {self.nt}")
            print(f"u.shape: {self.u.shape}")
        self.action_space = spaces.Box(np.full(1, 0, dtype="float32"), np.full(1, 1, dtype="float32"))
        self.observation_space = spaces.Box(np.full(self.nx, 0, dtype="float64"), np.full(self.nx, k, dtype="float64"),
                                            dtype=np.float64)
        self.t1_detection_threshold, self.t2_detection_threshold = t1_detection_threshold, t2_detection_threshold
        self.dosage_termination_threshold = dosage_termination_threshold
        self.reset_init_condition_func = reset_init_condition_func
        self.D, self.rho, self.alpha, self.alphaBetaRatio, self.k = D, rho, alpha, alpha_beta_ratio, k
        self.t1_detection_radius, self.t1_death_radius = t1_detection_radius, t1_death_radius
        self.total_dosage = float(total_dosage)
        self.remaining_dosage = float(total_dosage)
        self.stage = "Growth"
        self.simulationDays = self.growthDays = self.therapyDays = self.postTherapyDays = 0
        self.firstTherapyDay = self.firstPostTherapyDay = self.cDeathDay = None
        self.t_benchmark = None
        self._terminated = self._truncated = False

    # ---- reference helpers ------------------------------------------------------------------------------------
    def getTumorRadius(self, time_index, detectionRatio):
        """Radius (mm) of the rightmost node at or above ``detectionRatio * k`` in row ``time_index`` (None if
        invisible).  Needs ``record_history`` for rows other than the live one."""
        densities = self.u[time_index if self._record else 0]
        binaryMask = densities >= detectionRatio * self.k
        if not binaryMask.any():
            return None
        return (binaryMask.size - 1 - np.argmax(binaryMask[::-1])) * self.dx

    def terminate(self):
        return bool(self._terminated)

    def truncate(self):
        return bool(self._truncated)

    def _pull(self, row=False):
        """ONE device->host copy (+ one synchronisation) of everything a step produced: the engine keeps its per-patient scalars and
        the live row in one allocation (TumorBatch.host_pack).  ``row``: also return (a view of) the live row."""
        core = self._core
        if getattr(self, "_fetch", None) is None:
            from pdecontrolgym_amd.hostio import HostFetch
            self._fetch = HostFetch(core.device)
        v = core.host_views(self._fetch)
        self.time_index = int(v["time_index"][0])
        days = v["days"][0].tolist()
        self.growthDays, self.therapyDays, self.postTherapyDays, self.simulationDays = days[:4]
        self.cDeathDay = None if days[4] < 0 else days[4]
        self.remaining_dosage = float(v["remaining"][0])
        self._terminated, self._truncated = bool(v["terminated"][0]), bool(v["truncated"][0])
        res = (int(v["stage"][0]), v["out"][0].tolist())
        return res + (v["u"][0],) if row else res

    def step(self, control: float):
        """One simulated day.  ``control`` = proportion of ``total_dosage`` to apply (used in the Therapy stage)."""
        if self.verbose:
            print(f"\tEnvironment: Call step(). Perform dimensionalized finite differencing for time_index={self.time_index+1}")
        if not (self.time_index < self.nt - 1):
            return None                                  # the reference's step falls through without a return here
        stage_before = self.stage
        kill = None
        if stage_before == "Therapy":
            control = float(np.asarray(control).squeeze())
            applied = min(control * self.total_dosage, self.remaining_dosage)
            dArray = np.array([applied])
            BED = dArray + ((dArray ** 2) / (self.alphaBetaRatio))          # brain_tumor_env.py:260-262
            kill = 1.0 - np.exp(-self.alpha * BED)
            ctl = [control]
        else:
            ctl = [0.0]
        # the day's inputs are read by the kernel from pinned host memory in place (no upload)
        if getattr(self, "_pins", None) is None:
            from pdecontrolgym_amd.hostio import PinnedInputs
            self._pins = PinnedInputs(self._core.device)
        import torch
        f64 = torch.float64
        self._core.set_benchmark(self._pins("t_benchmark", [float("nan") if self.t_benchmark is None else float(self.t_benchmark)], f64))
        self._core.step(self._pins("control", ctl, f64), kill=None if kill is None else self._pins("kill", kill, f64))
        stage_i, (T1, T2, treatmentRadius, applied_dosage), row = self._pull(row=True)
        self.stage = _STAGES[stage_i]
        if self._record:
            self.u[self.time_index] = row
            obs = self.u[self.time_index]
        else:
            self.u[0] = row
            obs = self.u[0]
        T1 = None if np.isnan(T1) else T1
        self.t1_radius_idx_vs_time[self.time_index] = np.nan if T1 is None else T1 / self.dx
        if self.verbose:
            t1r = float("nan") if T1 is None else T1
            print(f"\t{stage_before:<15} {self.time_index:<5} {t1r:<15.2f} {T2:<15.2f}\n")
        if stage_before == "Growth" and self.stage == "Therapy":
            self.firstTherapyDay = self.time_index + 1
        if stage_before == "Therapy":
            self.dosage_vs_time[self.time_index] = applied_dosage
            if self.stage == "Post-Therapy":
                self.firstPostTherapyDay = self.time_index + 1
            if isinstance(self.dx, (int, np.integer)) and treatmentRadius != 0:
                # the reference's radius is ``index * dx + 25``: a NumPy integer when dx is an int (the shipped dx=1), and
                # ``radius ** -0.685`` then takes NumPy's power loop, whose last bit differs from pow() at some radii
                treatmentRadius = np.int64(treatmentRadius)
            reward = self.reward_class.reward(
                uVec=self.u, time_index=self.time_index, terminate=self._terminated, truncate=self._truncated,
                action=control, verbose=self.verbose, t_benchmark=self.t_benchmark, tumor_radius=T1,
                treatment_radius=treatmentRadius, applied_dosage=applied_dosage, total_dosage=self.total_dosage)
        elif self.stage == "Post-Therapy" and (self._terminated or self._truncated):
            reward = self.reward_class.reward(
                uVec=self.u, time_index=self.time_index, terminate=self._terminated, truncate=self._truncated,
                action=control, verbose=self.verbose, t_benchmark=self.t_benchmark)
        else:
            reward = 0.0
        return obs, reward, self._terminated, self._truncated, {"stage": self.stage}

    def run_days(self, mode: str):
        """Whole stretches of untreated days in ONE kernel launch (what TherapyWrapper's loops do with ``step(0)``):
        ``"growth"`` -- until the stage leaves Growth; ``"post"`` -- from Post-Therapy to death / time limit; ``"to_end"`` --
        from any stage to death / time limit (the open-loop benchmark).  Fills ``u``, ``t1_radius_idx_vs_time`` and the day
        counters exactly like the same number of ``step(0)`` calls and returns the last call's 5-tuple."""
        from pdecontrolgym_amd import _native as N
        code = {"growth": N.TUMOR_RUN_GROWTH, "post": N.TUMOR_RUN_POST, "to_end": N.TUMOR_RUN_TO_END}[mode]
        if not (self.time_index < self.nt - 1) or (mode == "growth" and self.stage != "Growth") or \
                (mode == "post" and self.stage != "Post-Therapy"):
            return None
        t0, stage_before = self.time_index, self.stage
        self._core.set_benchmark(float("nan") if self.t_benchmark is None else float(self.t_benchmark))
        u, rew, *_ = self._core.advance(code)
        stage_i, (T1, T2, treatmentRadius, applied_dosage) = self._pull()
        self.stage = _STAGES[stage_i]
        t1 = self.time_index
        if self._record:
            self.u[t0 + 1: t1 + 1] = self._core.t["history"][0, t0 + 1: t1 + 1].cpu().numpy()
            self.t1_radius_idx_vs_time[t0 + 1: t1 + 1] = self._core.t["t1_log"][0, t0 + 1: t1 + 1].cpu().numpy()
            obs = self.u[t1]
        else:
            self.u[0] = u[0].cpu().numpy()
            self.t1_radius_idx_vs_time[t1] = np.nan if np.isnan(T1) else T1 / self.dx
            obs = self.u[0]
        if stage_before == "Growth" and self.stage != "Growth":
            self.firstTherapyDay = self.growthDays + 1
        ended = self._terminated or self._truncated
        if self.t_benchmark is None or not ended or self.stage == "Growth":
            reward = 0 if (ended and self.stage != "Growth") else 0.0
        else:
            reward = self.time_index - self.t_benchmark
        return obs, reward, self._terminated, self._truncated, {"stage": self.stage}

    def reset(self, seed: Optional[int] = None, options: Optional[dict] = None):
        try:
            init_condition = self.reset_init_condition_func(self.X, self.nx)
        except:  # noqa: E722 - the reference converts any failure into this message (brain_tumor_env.py:363-368)
            raise Exception("Please pass an initial condition function")
        self.u = np.zeros((self.nt, self.nx)) if self._record else np.zeros((1, self.nx))
        self.dosage_vs_time = np.zeros(self.nt)
        self.u[0] = init_condition
        self._core.reset(self.u[0].copy())
        self.time_index = 0
        self.stage = "Growth"
        self.remaining_dosage = self.total_dosage
        self.simulationDays = self.growthDays = self.therapyDays = self.postTherapyDays = 0
        self.firstTherapyDay = self.firstPostTherapyDay = self.cDeathDay = None
        self._terminated = self._truncated = False
        return self.u[0], {}


class TherapyWrapper(Wrapper):
    """Shows an agent only the treatment days of a ``BrainTumor1D`` episode (behaviour of the reference's wrapper,
    brain_tumor_env.py:385-505; the implementation is this repository's).

    An episode is three stretches of simulated days.  The two untreated ones -- growth up to detection, and post-therapy
    up to death or the time limit -- never need the agent, so the wrapper *coasts* through them: ``reset`` coasts through
    growth, the first ``step`` after the dose budget is spent coasts to the end of the episode, and ``benchmark`` coasts
    through a whole untreated episode to obtain the survival baseline.  A coast is ONE kernel launch
    (``BrainTumor1D.run_days``: the day loop, the stage machine and the history stay on the GPU); day-by-day ``step(0)``
    calls are used only when per-day printing is wanted or ``fused_loops=False``.

    ``weekends``: after ``WORK_DAYS`` consecutive treated days (``control > 0``) the patient rests ``REST_DAYS`` untreated
    days whose results the agent never sees.
    """

    WORK_DAYS, REST_DAYS = 5, 2

    def __init__(self, env: BrainTumor1D, weekends=False, verbose=True, fused_loops=True):
        super().__init__(env)
        self.verbose, self.weekends, self.fused_loops = verbose, weekends, fused_loops
        self.treatment_calls = 0                  # agent-visible steps so far
        self.soft_constraint_violations = 0       # ... of which drew a toxicity penalty
        self.consecutive_treatment_days = 0       # current run of treated days (weekend rule)

    # ---- coasting ---------------------------------------------------------------------------------------------------
    def _say(self, msg):
        if self.verbose:
            print(f"[therapy wrapper] {msg}")

    def _in_kernel(self):
        base = self.env.unwrapped
        return self.fused_loops and not (self.verbose or getattr(base, "verbose", False)) and hasattr(base, "run_days")

    def _coast(self, stretch):
        """Untreated days until the stretch is over.  ``stretch``: "growth" (while the stage is Growth), "post" / "to_end"
        (until terminated or truncated).  Returns the last simulated day's 5-tuple, or None if no day was simulated."""
        base = self.env.unwrapped
        last = base.run_days(stretch) if self._in_kernel() else None
        over = (lambda: base.stage != "Growth") if stretch == "growth" else (lambda: False)
        while not over() and not (last is not None and (last[2] or last[3])):
            last = self.env.step(0)
            if last is None:        # stepping a finished episode: the reference fails unpacking the None its step() returns
                raise TypeError("cannot unpack non-iterable NoneType object (the episode is over: call reset())")
        return last

    # ---- gym interface ----------------------------------------------------------------------------------------------
    def reset(self, seed: Optional[int] = None, options: Optional[dict] = None):
        """Reset the patient and coast through the growth stage; the returned observation is the day of detection."""
        self.consecutive_treatment_days = 0
        obs, info = self.env.reset()
        self._say("reset; coasting through the growth stage")
        day = self._coast("growth")
        if day is not None:
            obs, info = day[0], day[4]
        self._say(f"tumour detected after {self.env.unwrapped.growthDays} days")
        return obs, info

    def step(self, control: float):
        """One treatment day with dose fraction ``control`` -- or, once therapy is over, the rest of the episode."""
        base = self.env.unwrapped
        if base.stage == "Post-Therapy":
            day = self._coast("post")
            rate = 100.0 * self.soft_constraint_violations / max(self.treatment_calls, 1)
            self._say(f"episode over, reward {day[1]}; {rate:.1f}% of the treatment days were toxic")
            return day
        day = self.env.step(control)
        reward, ended = day[1], bool(day[2] or day[3])
        self.treatment_calls += 1
        self.soft_constraint_violations += int(reward < 0.0)
        if self.weekends:
            self.consecutive_treatment_days = self.consecutive_treatment_days + 1 if control > 0 else 0
            if self.consecutive_treatment_days >= self.WORK_DAYS:
                self.consecutive_treatment_days = 0
                # an episode that ended on the treatment day still receives ONE (ineffective) rest call in the reference
                # (:476-479 test the treatment day's flags after the first rest call); kept so that call counts agree
                rest = 1 if ended else self.REST_DAYS
                self._say(f"weekend: {rest} rest day(s)")
                for _ in range(rest):
                    self.env.step(0)
        self._say(f"treatment day reward {reward}")
        return day

    def benchmark(self):
        """Survival (in simulated days) of the untreated patient; stored on the environment as ``t_benchmark`` -- the
        baseline of the episode reward -- and returned.  Call once before training or evaluation."""
        base = self.env.unwrapped
        self.env.reset()
        self._say("benchmark: one untreated episode")
        self._coast("to_end")
        base.t_benchmark = base.simulationDays
        self._say(f"t_benchmark = {base.t_benchmark} days")
        self.env.reset()
        return base.t_benchmark
