"""The backend calls the host faces make, in order, and where their outputs land.

``PDEVecEnv`` / ``TumorVecEnv`` / ``DeviceRollout`` are host code: what they owe the engines is a fixed sequence of backend calls
with the right tensors.  The CPU double is wrapped in a recorder that logs, per call from a face or an engine, the entry point and
which slots of the rollout buffers the tensors it was handed alias (``data_ptr``).  The sequences are written out below, for
every family: a change of the faces that launches something else, in another order, or into another tensor shows up here without
a GPU.  Smallest shapes the double takes, three instances, three steps; the episodes of the five PDE families last two steps, the
brain-tumour patients (time limit of 50 days) finish in every step.
"""
import random

import numpy as np
import pytest

from tests.fake_backend import FakeBackend

torch = pytest.importorskip("torch")

B, T = 3, 3
_ENTRY_POINTS = ("step1d", "reset1d", "rollout1d", "ns2d_step", "ns2d_reset", "ns2d_rollout", "traffic_step", "traffic_reset",
                 "traffic_rollout", "tumor_step", "tumor_advance", "tumor_reset", "mlp_forward")
_OUTPUTS = ("obs", "reward", "terminated", "done", "truncated")


class Recorder(FakeBackend):
    """The double, logging ``"entry"`` or ``"entry>obs[1],rewards[0]"`` for every call that comes from outside it (the double
    calls its own entry points too: a fused restart inside a step, the steps of a rollout)."""

    def __init__(self):
        super().__init__()
        self.log, self.buffers, self._depth = [], {}, 0

    def watch(self, ro):
        self.buffers = {k: getattr(ro, k) for k in ("obs", "obs_seen", "actions", "rewards", "terminated", "truncated")
                        if getattr(ro, k) is not None}

    def _alias(self, x):
        for name, buf in self.buffers.items():
            if x.data_ptr() == buf.data_ptr() and x.numel() == buf.numel():
                return name
            for t in range(buf.shape[0]):
                if x.data_ptr() == buf[t].data_ptr():
                    return f"{name}[{t}]"
        return None

    def _describe(self, name, args):
        given = []
        for a in args:
            if isinstance(a, dict):
                given += [a.get(k) for k in _OUTPUTS]
            else:
                given.append(a)
        hits = [self._alias(x) for x in given if torch.is_tensor(x)]
        hits = [h for h in hits if h is not None]
        return name + (">" + ",".join(hits) if hits else "")


def _logged(name):
    inner = getattr(FakeBackend, name)

    def call(self, *args, **kw):
        if self._depth == 0:
            self.log.append(self._describe(name, args))
        self._depth += 1
        try:
            return inner(self, *args, **kw)
        finally:
            self._depth -= 1
    return call


for _name in _ENTRY_POINTS:
    setattr(Recorder, _name, _logged(_name))


# ---- the six environments -----------------------------------------------------------------------------
def _make_1d(env_id, rec):
    import pde_control_gym
    from pde_control_gym.src import TunedReward1D
    parabolic = "ReactionDiffusion" in env_id
    nx = 5
    dx = 1.0 / nx
    dt = 0.25 * dx * dx if parabolic else 0.5 * dx
    n = nx + 1 if parabolic else nx
    p = {"T": 4 * dt, "dt": dt, "X": 1, "dx": dx, "control_sample_rate": 2 * dt, "reward_class": TunedReward1D(4, -1e3, 3e2),
         "normalize": False, "sensing_loc": "full", "control_type": "Dirchilet", "sensing_type": None, "sensing_noise_func": None,
         "limit_pde_state_size": True, "max_state_value": 1e10, "max_control_value": 20,
         "reset_init_condition_func": lambda nx: np.ones(n, dtype=np.float32),
         "reset_recirculation_func": lambda nx: np.full(n, 0.5, dtype=np.float32)}
    return pde_control_gym.make_vec(env_id, num_envs=B, device="cpu", backend=rec, **p)


def _make_ns(rec):
    import pde_control_gym
    from tests.five_ids import _ns_params
    return pde_control_gym.make_vec("PDEControlGym-NavierStokes2D", num_envs=B, device="cpu", backend=rec, dtype="float64",
                                    **dict(_ns_params(nt=3, n=5), maximum_pressure_iteration=2))


def _make_traffic(rec):
    import pde_control_gym
    from pde_control_gym.src import TrafficARZReward
    random.seed(0)
    return pde_control_gym.make_vec("PDEControlGym-TrafficPDE1D", num_envs=B, device="cpu", backend=rec, T=2, dt=1, X=50, dx=10,
                                    v_steady=10, ro_steady=0.12, v_max=40, ro_max=0.16, tau=60, reward_class=TrafficARZReward(),
                                    simulation_type="outlet-train", limit_pde_state_size=True, control_freq=1)


def _make_tumor(rec):
    import pde_control_gym
    from tests.five_ids import _five_ids
    p = _five_ids()[4][1]          # the whole dosage on the first treatment day: the second step runs the episode to its end
    return pde_control_gym.make_vec("PDEControlGym-BrainTumor1D", num_envs=B, weekends=True, device="cpu", backend=rec, **p)


FAMILIES = {
    "transport": lambda rec: _make_1d("PDEControlGym-TransportPDE1D", rec),
    "parabolic": lambda rec: _make_1d("PDEControlGym-ReactionDiffusionPDE1D", rec),
    "burgers": lambda rec: _make_1d("PDEControlGym-BurgersPDE1D", rec),
    "ns2d": _make_ns,
    "traffic": _make_traffic,
    "tumor": _make_tumor,
}


def _action(venv):
    hi = np.asarray(venv.action_space.high, dtype=venv.action_space.dtype)
    return np.tile(hi[None], (B, 1))


def _record(family, scenario):
    """The log of one scenario, and what the assertions beyond the log need."""
    from pde_control_gym import DeviceRollout
    from pdecontrolgym_amd.policy import FusedMLP
    rec = Recorder()
    venv = FAMILIES[family](rec)
    extra = {}
    if scenario in ("host_reset", "fused_reset"):
        venv.reset()
        if scenario == "fused_reset":
            venv.enable_fused_auto_reset()
        dones = [venv.step(_action(venv))[2] for _ in range(T)]
        extra["dones"] = np.stack(dones)
        return rec.log, extra
    venv.reset_tensor()
    if family != "tumor":
        venv.enable_fused_auto_reset()
    lo, hi = float(venv.action_space.low[0]), float(venv.action_space.high[0])
    d = int(np.prod(venv.observation_space.shape))
    if scenario == "rollout_torch":
        policy = lambda o: o.reshape(B, -1)[:, :venv.action_space.shape[0]] * 0 + hi      # noqa: E731
        kw = dict(use_graph=False)
    else:
        policy = FusedMLP(torch.nn.Sequential(torch.nn.Linear(d, venv.action_space.shape[0])), backend=rec)
        kw = dict(one_launch=None)
    ro = DeviceRollout(venv, policy, T, action_low=lo, action_high=hi, **kw)
    rec.watch(ro)
    extra["own"] = {k: venv.core.t[k] for k in ("reward", "terminated", "truncated", "done") if k in venv.core.t}
    del rec.log[:]
    ro.run()
    extra["venv"], extra["ro"] = venv, ro
    return rec.log, extra


_ONE_D = {
    "host_reset": ["reset1d", "step1d", "step1d", "reset1d", "step1d"],
    "fused_reset": ["reset1d", "step1d", "step1d", "step1d"],
    "rollout_torch": ["step1d>obs[1],rewards[0],terminated[0],truncated[0]",
                      "step1d>obs[2],rewards[1],terminated[1],truncated[1]",
                      "step1d>obs[3],rewards[2],terminated[2],truncated[2]"],
    "rollout_fused": ["rollout1d>obs,actions,rewards,terminated,truncated"],
}
# one treatment step of the brain-tumour face (weekends on): post-therapy patients run to their end, one treatment day, two rest
# days, restart of the finished, their growth stage
_TUMOR_STEP = ["tumor_advance", "tumor_step", "tumor_step", "tumor_step", "tumor_reset", "tumor_advance"]
EXPECTED = {
    "transport": _ONE_D,
    "parabolic": _ONE_D,
    "burgers": _ONE_D,
    "ns2d": {
        "host_reset": ["ns2d_reset", "ns2d_step", "ns2d_step", "ns2d_reset", "ns2d_step"],
        "fused_reset": ["ns2d_reset", "ns2d_step", "ns2d_step", "ns2d_step"],
        "rollout_torch": ["ns2d_step>obs[1],rewards[0],terminated[0]",
                          "ns2d_step>obs[2],rewards[1],terminated[1]",
                          "ns2d_step>obs[3],rewards[2],terminated[2]"],
        # (the engine's own one-launch rollout takes its commands ahead: with a policy in the loop the steps stay separate)
        "rollout_fused": ["mlp_forward>obs[0],actions[0]", "ns2d_step>obs[1],rewards[0],terminated[0]",
                          "mlp_forward>obs[1],actions[1]", "ns2d_step>obs[2],rewards[1],terminated[1]",
                          "mlp_forward>obs[2],actions[2]", "ns2d_step>obs[3],rewards[2],terminated[2]"],
    },
    "traffic": {
        "host_reset": ["traffic_reset", "traffic_step", "traffic_step", "traffic_reset", "traffic_step"],
        "fused_reset": ["traffic_reset", "traffic_step", "traffic_step", "traffic_step"],
        "rollout_torch": ["traffic_step", "traffic_step", "traffic_step"],
        "rollout_fused": ["traffic_rollout>obs,actions,rewards,terminated,truncated"],
    },
    "tumor": {
        "host_reset": ["tumor_reset", "tumor_advance"] + _TUMOR_STEP + _TUMOR_STEP + _TUMOR_STEP,
        "rollout_torch": _TUMOR_STEP + _TUMOR_STEP + _TUMOR_STEP,
        "rollout_fused": (["mlp_forward>obs[0],actions[0]"] + _TUMOR_STEP + ["mlp_forward>obs[1],actions[1]"] + _TUMOR_STEP
                          + ["mlp_forward>obs[2],actions[2]"] + _TUMOR_STEP),
    },
}
# every episode of the five PDE families lasts two steps; the tumour's time limit ends every patient's episode at once
DONES = {f: [[False] * B, [True] * B, [False] * B] for f in EXPECTED}
DONES["tumor"] = [[True] * B] * T
CASES = [(f, s) for f in EXPECTED for s in EXPECTED[f]]


@pytest.mark.parametrize("family,scenario", CASES, ids=[f"{f}-{s}" for f, s in CASES])
def test_backend_calls_of_the_faces(family, scenario):
    log, extra = _record(family, scenario)
    assert log == EXPECTED[family][scenario]
    if "dones" in extra:
        assert extra["dones"].tolist() == DONES[family]
    if scenario == "rollout_torch":
        venv, ro = extra["venv"], extra["ro"]
        if family != "traffic" and family != "tumor":
            # the step kernel was handed slot t of the rollout buffers, not the engine's own outputs
            assert len(log) == T and all(f"obs[{t + 1}]" in e and f"rewards[{t}]" in e and f"terminated[{t}]" in e
                                         for t, e in enumerate(log))
        # ... and afterwards the engine has its own output tensors back and its observation is the rollout's last
        assert extra["own"] and all(venv.core.t[k] is v for k, v in extra["own"].items())
        assert torch.equal(venv.core.t["obs" if "obs" in venv.core.t else "u"], ro.obs[T])
        assert ((ro.terminated | ro.truncated) != 0).tolist() == DONES[family]
