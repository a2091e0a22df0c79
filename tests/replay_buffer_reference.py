"""NumPy restatement of the replay memory of examples/train_sac_device.py as it stood before ``DeviceReplayBuffer`` (the dict of
tensors and its seven indexed assignments per rollout, themselves SB3's ``OffPolicyAlgorithm._store_transition`` +
``ReplayBuffer.add`` with ``handle_timeout_termination``), shared by tests/test_replay_buffer.py and tests/test_gpu_replay_buffer.py.
One line restates the DEVICE's arithmetic and not the example's literal text: the example scales the action with ``/ (hi - lo)``, which
torch evaluates on a device tensor as a multiplication by the reciprocal of the scalar (formed in the tensor's dtype) and on a CPU tensor
as a division; the restatement multiplies by that reciprocal, as ``DeviceReplayBuffer`` does, so the two share this one decision.  What
pins the stored action to the example's own line is tests/test_gpu_replay_buffer.py, which compares the histories of the example with
its dict and with the class by ``==`` on the device.
``FakeRollout`` is the part of a ``DeviceRollout`` the buffer reads, on any device.  Plain helper module (not a conftest)."""
from __future__ import annotations

import numpy as np


class NumpyReplay:
    """``add(obs[T+1, B, D], actions[T, B], rewards[T, B], terminated[T, B], truncated[T, B], terminal_obs[T, B, D] or None)``."""

    def __init__(self, capacity, D, lo, hi, dtype):
        self.cap, self.lo, self.hi = capacity, lo, hi
        self.buf = {"obs": np.zeros((capacity, D), dtype), "next": np.zeros((capacity, D), dtype), "act": np.zeros((capacity, 1), np.float32),
                    "rew": np.zeros((capacity, 1), np.float32), "term": np.zeros((capacity, 1), np.float32)}
        self.head = self.filled = 0

    def add(self, obs, actions, rewards, terminated, truncated, terminal_obs=None):
        T, B = rewards.shape
        D = self.buf["obs"].shape[1]
        lo, hi, buf = self.lo, self.hi, self.buf
        idx = (self.head + np.arange(T * B)) % self.cap
        ended = (terminated | truncated).reshape(-1, 1)
        buf["obs"][idx] = obs[:T].reshape(-1, D)
        if terminal_obs is not None:
            buf["next"][idx] = np.where(ended.astype(bool), terminal_obs.reshape(-1, D), obs[1:].reshape(-1, D))
            ended = terminated.reshape(-1, 1)
        else:
            buf["next"][idx] = obs[1:].reshape(-1, D)
        # in the rollout's dtype; the example's ``/ (hi - lo)`` on a device tensor is torch's multiplication by the reciprocal of a
        # scalar divisor, formed in that dtype
        ft = actions.dtype.type
        scaled = ft(2.0) * (actions.reshape(-1, 1) - ft(lo)) * (ft(1.0) / ft(hi - lo)) - ft(1.0)
        buf["act"][idx] = np.clip(scaled, -1.0, 1.0).astype(np.float32)
        buf["rew"][idx] = rewards.reshape(-1, 1).astype(np.float32)
        buf["term"][idx] = ended.astype(np.float32)
        self.head, self.filled = (self.head + T * B) % self.cap, min(self.filled + T * B, self.cap)


NAMES = {"observations": "obs", "next_observations": "next", "actions": "act", "rewards": "rew", "dones": "term"}


def assert_equal(buf, ref: NumpyReplay, what=""):
    """The storages, ``pos`` and ``filled`` (device and host) of a ``DeviceReplayBuffer`` against the restatement, bit for bit."""
    for mine, theirs in NAMES.items():
        got = getattr(buf, mine).cpu().numpy()
        assert got.dtype == ref.buf[theirs].dtype and got.shape == ref.buf[theirs].shape, (what, mine, got.dtype, got.shape)
        np.testing.assert_array_equal(got, ref.buf[theirs], err_msg=f"{what}: {mine}")
    assert int(buf.pos) == buf.pos_host == ref.head and int(buf.filled) == buf.filled_host == ref.filled, what


class FakeRollout:
    """T steps of B environments with D-wide observations, filled from a seeded generator: episodes end (terminated, truncated, or both)
    at about a third of the steps, commands reach outside the action box, float64 rewards do not fit float32."""

    def __init__(self, T, B, D, dtype, terminal_obs, device="cpu", seed=0):
        import torch
        self.T, self.B, self.D, self.dtype, self.device = T, B, D, dtype, device
        self.rng = np.random.default_rng([11, seed])
        z = lambda *shape, dt=dtype: torch.zeros(*shape, dtype=dt, device=device)      # noqa: E731
        self.obs, self.actions, self.rewards = z(T + 1, B, D), z(T, B), z(T, B)
        self.terminated, self.truncated = z(T, B, dt=torch.uint8), z(T, B, dt=torch.uint8)
        self.obs_seen = None
        self.terminal_obs = z(T, B, D) if terminal_obs else None

    def run(self):
        import torch
        T, B, D, rng = self.T, self.B, self.D, self.rng
        np_dt = np.float64 if self.dtype == torch.float64 else np.float32
        put = lambda t, a: t.copy_(torch.from_numpy(np.ascontiguousarray(a)))      # noqa: E731
        put(self.obs, rng.standard_normal((T + 1, B, D)).astype(np_dt))
        put(self.actions, (12.0 * rng.standard_normal((T, B))).astype(np_dt))
        self.actions[0, 0], self.actions[0, -1] = -100.0, 100.0      # (both clamps of the scaled action bite in every rollout)
        put(self.rewards, (rng.standard_normal((T, B)) / 3.0).astype(np_dt))
        put(self.terminated, (rng.random((T, B)) < 0.25).astype(np.uint8))
        put(self.truncated, (rng.random((T, B)) < 0.25).astype(np.uint8))
        if self.terminal_obs is not None:
            put(self.terminal_obs, rng.standard_normal((T, B, D)).astype(np_dt))
        return self

    def numpy(self):
        f = lambda t: None if t is None else t.cpu().numpy()      # noqa: E731
        return f(self.obs), f(self.actions), f(self.rewards), f(self.terminated), f(self.truncated), f(self.terminal_obs)
