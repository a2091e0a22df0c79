"""The replay memory of off-policy training (SAC) on the device: the ``DeviceRolloutBuffer`` of the other half of the training stack.

The reference's users train with SB3's ``SAC("MlpPolicy", env)`` (examples/transportPDE/transport1Dsac.py), whose
``OffPolicyAlgorithm._store_transition`` + ``ReplayBuffer.add`` copy one transition per environment step into NumPy arrays and whose
``ReplayBuffer.sample`` gathers a minibatch back out of them.  ``DeviceReplayBuffer`` keeps the same transitions in device tensors,
stores a whole ``DeviceRollout`` (T * B transitions) per call, and hands out a minibatch as an INDEX plus the storages themselves: the
networks read the rows in place (``FusedMLP(..., index=)``: pdegym_mlp_forward_gather), the loss kernels already do
(``SACLoss.critic(..., index=)``).
"""
from __future__ import annotations

from collections import namedtuple

ReplaySample = namedtuple("ReplaySample", "index observations next_observations actions rewards dones")


class DeviceReplayBuffer:
    """``buf = DeviceReplayBuffer(rollout, capacity, action_low, action_high)``; after ``rollout.run()``: ``buf.add()``; then
    ``s = buf.sample(batch)``.

    Storages, allocated once here: ``observations`` / ``next_observations`` ``[capacity, D]`` in the rollout's dtype (D: the flattened
    observation), ``actions`` ``[capacity, A]``, ``rewards`` / ``dones`` ``[capacity, 1]`` (float32).  ``add()`` stores the rollout's T * B
    transitions time-major (step t of environment b at offset t * B + b) at the ring position, wrapping at ``capacity``:

      * the stored action is SB3's scaled action ``clamp(2 (c - lo) / (hi - lo) - 1, -1, 1)`` of the command ``c`` the rollout holds;
      * on a rollout built with ``terminal_obs=True`` (SB3's ``handle_timeout_termination``): ``next_observations`` takes the terminal
        observation where the step ended an episode and ``obs[t + 1]`` elsewhere, and ``dones`` is ``terminated`` alone -- a cut-off
        episode keeps its bootstrap; without it ``next_observations = obs[t + 1]`` (the new episode's first row after a restart) and
        ``dones = terminated | truncated``, which cuts the bootstrap of such a transition;
      * rewards are rounded once to float32; a rollout with sensing noise stores ``obs_seen``, what the policy saw.

    ``pos`` and ``filled`` (int64 0-d device tensors) are the ring position and the number of valid transitions; the host mirrors
    ``pos_host`` / ``filled_host`` follow by arithmetic.  ``add()`` and ``sample(batch, draws=...)`` make no host synchronisation, so
    ``rollout.run()`` (built with ``use_graph=False``) + ``add()`` + an update step can be captured in one ``torch.cuda.graph``; a replay
    moves the device counters alone, so sample with ``draws=`` there (or call ``sync_host()``, one synchronisation, before a
    ``sample(batch)``).  ``add()`` is plain torch indexing: it runs once per rollout.

    ``sample(batch)`` draws ``torch.randint(0, filled_host, (min(batch, filled_host),), device=...)``; ``sample(batch, draws=t)`` takes
    the caller's non-negative int64 ``[batch]`` draws and returns ``index = draws % filled`` computed on the device.  Both return a
    ``ReplaySample`` of the index and the STORAGES themselves (views, not copies): pass ``index=s.index`` to ``FusedMLP`` and
    ``SACLoss.critic``.  ``gather(s)`` materialises the ``[N, ...]`` rows for consumers that are plain torch modules."""

    def __init__(self, rollout, capacity: int, action_low: float = -1.0, action_high: float = 1.0):
        import torch
        self.rollout, self.capacity = rollout, int(capacity)
        self.lo, self.hi = float(action_low), float(action_high)
        self.T, self.B = (int(s) for s in rollout.rewards.shape)
        if self.capacity < self.T * self.B:
            raise ValueError(f"capacity {self.capacity} is below one rollout ({self.T} steps x {self.B} environments = {self.T * self.B} transitions)")
        if not self.lo < self.hi:
            raise ValueError(f"the action box needs action_low < action_high, got [{self.lo}, {self.hi}]")
        dev, dt = rollout.obs.device, rollout.obs.dtype
        n = self.T * self.B
        self.D = int(rollout.obs[0].numel() // self.B)
        self.A = int(rollout.actions[0].numel() // self.B)
        self.observations = torch.zeros(self.capacity, self.D, dtype=dt, device=dev)
        self.next_observations = torch.zeros(self.capacity, self.D, dtype=dt, device=dev)
        self.actions = torch.zeros(self.capacity, self.A, dtype=torch.float32, device=dev)
        self.rewards = torch.zeros(self.capacity, 1, dtype=torch.float32, device=dev)
        self.dones = torch.zeros(self.capacity, 1, dtype=torch.float32, device=dev)
        self.pos = torch.zeros((), dtype=torch.int64, device=dev)
        self.filled = torch.zeros((), dtype=torch.int64, device=dev)
        self.pos_host = self.filled_host = 0
        self._offsets = torch.arange(n, dtype=torch.int64, device=dev)
        # ``tensor / (hi - lo)`` is a multiplication by the scalar's reciprocal on the device (torch's kernel for a scalar divisor, the
        # reciprocal formed in the tensor's dtype) and a division on the CPU: the reciprocal is spelled out, so that the stored action
        # has the device's bits -- those of the expression in the class docstring there -- wherever the buffer lives
        self._inv_range = float(torch.ones((), dtype=dt) / torch.tensor(self.hi - self.lo, dtype=dt))

    def add(self):
        """Store the T * B transitions of the rollout's last ``run()``.  Returns self."""
        import torch
        ro, T, n, D = self.rollout, self.T, self.T * self.B, self.D
        idx = (self.pos + self._offsets) % self.capacity
        seen = ro.obs if getattr(ro, "obs_seen", None) is None else ro.obs_seen
        ended = (ro.terminated | ro.truncated).reshape(n, 1)
        self.observations[idx] = seen[:T].reshape(n, D)
        if getattr(ro, "terminal_obs", None) is not None:
            self.next_observations[idx] = torch.where(ended.bool(), ro.terminal_obs.reshape(n, D), seen[1:].reshape(n, D))
            ended = ro.terminated.reshape(n, 1)
        else:
            self.next_observations[idx] = seen[1:].reshape(n, D)
        self.actions[idx] = (2.0 * (ro.actions.reshape(n, self.A) - self.lo) * self._inv_range - 1.0).clamp(-1.0, 1.0).to(torch.float32)
        self.rewards[idx] = ro.rewards.reshape(n, 1).to(torch.float32)
        self.dones[idx] = ended.to(torch.float32)
        self.pos.add_(n).remainder_(self.capacity)
        self.filled.add_(n).clamp_(max=self.capacity)
        self.pos_host, self.filled_host = (self.pos_host + n) % self.capacity, min(self.filled_host + n, self.capacity)
        return self

    def _sample_of(self, index) -> ReplaySample:
        return ReplaySample(index, self.observations, self.next_observations, self.actions, self.rewards, self.dones)

    def sample(self, batch: int, draws=None) -> ReplaySample:
        """A minibatch of ``min(batch, filled)`` transitions drawn with replacement, as an index into the storages; ``draws``: see the
        class.  ``ValueError`` on an empty buffer."""
        import torch
        if self.filled_host < 1:
            raise ValueError("the replay buffer is empty: add() a rollout first")
        if draws is None:
            return self._sample_of(torch.randint(0, self.filled_host, (min(int(batch), self.filled_host),), device=self.pos.device))
        if (not torch.is_tensor(draws) or draws.dtype != torch.int64 or tuple(draws.shape) != (int(batch),)
                or draws.device != self.pos.device):
            raise ValueError(f"draws must be an int64 [{int(batch)}] tensor on {self.pos.device}")
        return self._sample_of(torch.remainder(draws, self.filled))

    def gather(self, s: ReplaySample) -> ReplaySample:
        """The materialised ``[N, ...]`` rows of a sample (``storage[s.index]`` of every storage), the index kept."""
        return ReplaySample(s.index, *(t[s.index] for t in s[1:]))

    def state_dict(self):
        return {"observations": self.observations, "next_observations": self.next_observations, "actions": self.actions,
                "rewards": self.rewards, "dones": self.dones, "pos": self.pos, "filled": self.filled}

    def load_state_dict(self, state):
        """Copy the storages, ``pos`` and ``filled`` in (shapes must match); the host mirrors are read back once."""
        own = self.state_dict()
        if set(state) != set(own):
            raise ValueError(f"state_dict keys {sorted(state)} do not match {sorted(own)}")
        for k, t in own.items():
            if tuple(state[k].shape) != tuple(t.shape):
                raise ValueError(f"{k}: shape {tuple(state[k].shape)} does not match {tuple(t.shape)}")
        for k, t in own.items():
            t.copy_(state[k])
        return self.sync_host()

    def sync_host(self):
        """Read ``pos`` and ``filled`` back into the host mirrors (one synchronisation): after ``load_state_dict`` and after graph replays."""
        self.pos_host, self.filled_host = int(self.pos), int(self.filled)
        return self
