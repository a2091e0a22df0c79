"""The CPU doubles of tests/fake_backend.py and tests/fake_gae_backend.py with what the terminal-observation feature adds to the
backend interface (pdecontrolgym_amd/backend.py): ``rollout1d(..., final_obs_steps=)`` -- PDEGYM_ROLLOUT_FINAL_OBS_PER_STEP, stated
as the header states it: T step calls whose ``final_obs`` is row t of the [T, B, obs_dim] array -- and ``mlp_forward(..., rows=,
rows_not=)`` -- pdegym_mlp_forward_masked: the unmasked evaluation, stored for the live rows only."""
import ctypes as C

import torch

from tests.fake_backend import FakeBackend
from tests.fake_gae_backend import FakeGaeBackend


class FakeTerminalObsBackend(FakeBackend, FakeGaeBackend):
    name = "oracle-test-double+terminal-obs"

    def __init__(self):
        FakeBackend.__init__(self)
        FakeGaeBackend.__init__(self)
        self.masked_calls = 0

    def rollout1d(self, kind, P, T, obs, actions, rewards, terminated, truncated, B, policy=None, obs_noise=None, obs_seen=None,
                  final_obs_steps=None):
        if final_obs_steps is None:
            return super().rollout1d(kind, P, T, obs, actions, rewards, terminated, truncated, B, policy=policy, obs_noise=obs_noise,
                                     obs_seen=obs_seen)
        steps = actions.shape[0]
        od = P.n if P.sensing == 0 else 1
        assert tuple(final_obs_steps.shape) == (steps, B, od) and final_obs_steps.dtype == torch.float32
        assert T.get("reset_init") is not None, "the flag needs the auto-reset pool (-2 in the library)"
        for t in range(steps):          # one step call each, final_obs pointed at row t; the engine's own final_obs is not written
            net = None
            if policy is not None:
                net = type(policy)()
                C.memmove(C.addressof(net), C.addressof(policy), C.sizeof(policy))
                if policy.noise:
                    net.noise = policy.noise + 4 * t * B * policy.noise_stride
            super().rollout1d(kind, P, {**T, "final_obs": final_obs_steps[t]}, obs[t:t + 2], actions[t:t + 1], rewards[t:t + 1],
                              terminated[t:t + 1], truncated[t:t + 1], B, policy=net,
                              obs_noise=None if obs_noise is None else obs_noise[t:t + 1],
                              obs_seen=None if obs_seen is None else obs_seen[t:t + 1])

    def mlp_forward(self, net, x, y, B, rows=None, rows_not=None):
        if rows is None:
            assert rows_not is None
            return super().mlp_forward(net, x, y, B)
        assert rows.dtype == torch.uint8 and tuple(rows.shape) == (B,)
        assert rows_not is None or (rows_not.dtype == torch.uint8 and tuple(rows_not.shape) == (B,))
        live = rows != 0
        if rows_not is not None:
            live &= rows_not == 0
        self.masked_calls += 1
        if not bool(live.any()):
            return
        full = torch.zeros_like(y[:B])
        super().mlp_forward(net, x[:B], full, B)      # (a dead row may hold anything: the rows are independent here as well)
        y[:B][live] = full[live]
