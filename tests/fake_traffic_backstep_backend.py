"""The oracle-backed test double of tests/fake_backend.py with the traffic backstepping entry points added (CPU tests of the HOST
logic, tests/test_traffic_backstep.py): the law by the NumPy restatement (tests/traffic_backstep_restatement.py, np.trapz's order
written out), the env-step by the oracle.  ``traffic_backstep_control`` and ``traffic_backstep_rollout`` form their commands in ONE
function, so the double's two paths agree by construction -- what the tests then compare is what the host layers did with them.
Every call is recorded in ``calls``."""
import ctypes as C

import numpy as np
import torch

from pdecontrolgym_amd import _native as N
from tests import traffic_backstep_restatement as R
from tests.fake_backend import FakeBackend

SIM_NAME = {v: k for k, v in N.TRAFFIC_SIM.items()}


def _view(ptr, shape, ctype):
    return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(ctype)), shape)


def law_rows(P, law, obs, rs, noise):
    """Commands [B, commands] for the observation rows ``obs`` [B, 2M]: the restated law, + noise (float32 widened), clamped."""
    B, M = obs.shape[0], int(P.M)
    sim = SIM_NAME[int(P.sim)]
    ncmd = 2 if sim == "both" else 1
    out = np.zeros((B, ncmd))
    shape = (M,) if law.weight_stride == 0 else (B, int(law.weight_stride))
    wv = wq = None
    if sim != "inlet":
        wv, wq = _view(law.weights_v, shape, C.c_double), _view(law.weights_q, shape, C.c_double)
    for b in range(B):
        vs, qs, _ = R.steady(P.vm, P.rm, float(rs[b]))
        cv, cq = (None, None) if wv is None else ((wv, wq) if wv.ndim == 1 else (wv[b, :M], wq[b, :M]))
        with np.errstate(all="ignore"):
            cmd = np.array(R.law_commands(sim, obs[b, :M], obs[b, M:], cv, cq, P.dx, float(rs[b]), vs, qs))
            if noise is not None:
                cmd = cmd + noise[b].astype(np.float64)
            if law.clamp:
                cmd = np.clip(cmd, law.lo, law.hi)
        out[b] = cmd
    return out


class FakeTrafficBackstepBackend(FakeBackend):
    def __init__(self):
        super().__init__()
        self.calls = []

    def traffic_step(self, P, T, B):
        self.calls.append(("step",))
        super().traffic_step(P, T, B)

    def traffic_rollout(self, *a, **kw):
        self.calls.append(("rollout",))
        super().traffic_rollout(*a, **kw)

    def traffic_backstep_control(self, P, obs, rs, out, law):
        ncmd = 2 if int(P.sim) == N.TRAFFIC_SIM["both"] else 1
        self.calls.append(("control", dict(order=int(law.order), clamp=int(law.clamp), lo=float(law.lo), hi=float(law.hi),
                                           noise=law.noise, weight_stride=int(law.weight_stride))))
        assert out.dtype == torch.float64 and obs.dtype == torch.float64 and out.numel() == obs.shape[0] * ncmd
        B = obs.shape[0]
        noise = _view(law.noise, (B, int(law.noise_stride)), C.c_float)[:, :ncmd] if law.noise else None
        a = law_rows(P, law, obs.numpy(), rs.numpy(), noise)
        out.view(B, ncmd).copy_(torch.from_numpy(a))

    def traffic_backstep_rollout(self, P, T, obs, actions, rewards, done, truncated, B, law):
        steps, ncmd = int(actions.shape[0]), int(actions.shape[2])
        self.calls.append(("backstep_rollout", dict(T=steps, order=int(law.order), clamp=int(law.clamp), lo=float(law.lo), hi=float(law.hi),
                                                    noise=law.noise, noise_stride=int(law.noise_stride), weight_stride=int(law.weight_stride),
                                                    weights_v=law.weights_v, weights_q=law.weights_q)))
        noise = _view(law.noise, (steps, B, int(law.noise_stride)), C.c_float)[:, :, :ncmd] if law.noise else None
        for t in range(steps):
            a = law_rows(P, law, obs[t].numpy(), T["rs"].numpy(), None if noise is None else noise[t])
            actions[t].copy_(torch.from_numpy(a))
            S = dict(T)
            S.update(action=actions[t], obs=obs[t + 1], reward=rewards[t], done=done[t], truncated=truncated[t])
            super().traffic_step(P, S, B)
