"""What PPO does between a rollout and its update, on the device: values of all T + 1 observation slots in one batched critic call,
then GAE(lambda) advantages, returns and the statistics of the episodes that ended inside the buffer in ONE launch (pdegym_gae).

The reference's users train with SB3's ``PPO("MlpPolicy", env)`` (examples/transportPDE/transport1Dppo.py:88-90), whose
``RolloutBuffer.compute_returns_and_advantage`` walks the buffer backwards in Python, one NumPy expression per step.  On device
tensors that loop is T x ~8 elementwise launches behind a rollout that is one launch; ``DeviceRolloutBuffer`` replaces it with the
kernel that restates it bit for bit (include/pdegym.h: pdegym_gae), for every environment family ``DeviceRollout`` drives.
"""
from __future__ import annotations

from collections import namedtuple

RolloutBatch = namedtuple("RolloutBatch", "observations actions advantages returns values")


class DeviceRolloutBuffer:
    """``buf = DeviceRolloutBuffer(rollout, gamma=0.99, gae_lambda=0.95)``; after ``rollout.run()``: ``buf.compute(critic=critic)``.

    Tensors, allocated once here: ``values[T + 1, B]``, ``advantages[T, B]``, ``returns[T, B]`` (float32); with ``episode_stats``
    ``episode_return[T, B]`` (float64) and ``episode_length[T, B]`` (int32) -- where an episode ended at ``(t, b)`` its return and
    length, else 0 -- and the ``[B]`` accumulators ``ep_return_acc`` / ``ep_length_acc`` of the episodes still running, which
    persist from one rollout to the next (auto-reset ends episodes anywhere in the buffer).  ``boot``: None, or a float32
    ``[T, B]`` tensor -- V(terminal observation), added as ``gamma * boot`` to the reward of steps that were
    truncated and not terminated (SB3's time-limit bootstrap, on_policy_algorithm.py: collect_rollouts); other entries are never used.
    On a rollout built with ``terminal_obs=True`` it is allocated here and ``compute(critic=...)`` fills it before the GAE launch:
    ``boot[t, b] = critic(rollout.terminal_obs[t, b])`` where ``truncated[t, b] & ~terminated[t, b]`` -- a ``FusedMLP`` critic in one
    masked launch over the T * B rows (no compaction, no allocation, no synchronisation; the other entries keep what they held), any
    other module on all T * B rows.  ``bootstrap_truncated=False`` keeps ``boot = None`` (every cut-off treated as SB3 treats a
    VecEnv without the ``TimeLimit.truncated`` key); ``compute(values=...)`` leaves ``boot`` to the caller, as on any other rollout,
    where it stays a tensor the caller assigns.  Rewards and flags are the rollout's
    own buffers, the rewards in the engine's dtype (float64 ones are rounded once to float32 as they are read, SB3's storage).

    ``compute`` makes no host synchronisation and, with a ``FusedMLP`` critic or ``values=``, no allocation: ``rollout.run()`` and
    ``buf.compute(...)`` can be captured together in one ``torch.cuda.graph`` (build the rollout with ``use_graph=False``, and call
    ``critic.refresh()`` / ``policy.refresh()`` before a replay that follows an optimizer step)."""

    def __init__(self, rollout, gamma: float = 0.99, gae_lambda: float = 0.95, episode_stats: bool = True, backend=None,
                 bootstrap_truncated: bool = True):
        import torch
        self.rollout, self.gamma, self.gae_lambda = rollout, float(gamma), float(gae_lambda)
        self.T, self.B = (int(s) for s in rollout.rewards.shape)
        dev = rollout.rewards.device
        T, B = self.T, self.B
        self.values = torch.zeros(T + 1, B, dtype=torch.float32, device=dev)
        self.advantages = torch.zeros(T, B, dtype=torch.float32, device=dev)
        self.returns = torch.zeros(T, B, dtype=torch.float32, device=dev)
        self.boot = None
        self.bootstrap_truncated = bool(bootstrap_truncated) and getattr(rollout, "terminal_obs", None) is not None
        if self.bootstrap_truncated:
            self.boot = torch.zeros(T, B, dtype=torch.float32, device=dev)
        self.episode_return = self.episode_length = self.ep_return_acc = self.ep_length_acc = None
        if episode_stats:
            self.episode_return = torch.zeros(T, B, dtype=torch.float64, device=dev)
            self.episode_length = torch.zeros(T, B, dtype=torch.int32, device=dev)
            self.ep_return_acc = torch.zeros(B, dtype=torch.float64, device=dev)
            self.ep_length_acc = torch.zeros(B, dtype=torch.int32, device=dev)
        if backend is None:
            from pdecontrolgym_amd.backend import default_backend
            backend = default_backend()
        self.backend = backend

    def _evaluate(self, critic):
        """values[t, b] = critic(observation slot t of environment b), all (T + 1) * B rows in one call: what the policy saw
        (``obs_seen``) when the rollout has sensing noise, the observation otherwise."""
        import torch
        ro = self.rollout
        seen = ro.obs if ro.obs_seen is None else ro.obs_seen
        x = seen.reshape((self.T + 1) * self.B, -1)
        out = self.values.view(-1)
        if hasattr(critic, "forward_into"):          # pdecontrolgym_amd.FusedMLP: one launch, written in place
            if critic.out_dim != 1:
                raise ValueError(f"the critic must have one output, this network has {critic.out_dim}")
            critic.forward_into(x, out, clamp=None)
            return
        with torch.no_grad():
            p = next(iter(critic.parameters()), None) if hasattr(critic, "parameters") else None
            if p is not None and p.dtype != x.dtype:      # float64 observations meet a float32 network as they do in SB3
                x = x.to(p.dtype)
            v = critic(x)
            if v.numel() != out.numel():
                raise ValueError(f"the critic must return one value per row, got {tuple(v.shape)} for {x.shape[0]} rows")
            out.copy_(v.reshape(-1))

    def _bootstrap(self, critic):
        """boot[t, b] = critic(terminal observation of step t, environment b) where that step was truncated and not terminated."""
        import torch
        ro = self.rollout
        boot = self.boot
        if (not torch.is_tensor(boot) or tuple(boot.shape) != (self.T, self.B) or boot.dtype != torch.float32 or not boot.is_contiguous()):
            raise ValueError(f"boot must stay the contiguous float32 [{self.T}, {self.B}] tensor the constructor allocated")
        x = ro.terminal_obs.reshape(self.T * self.B, -1)
        out = boot.view(-1)
        if hasattr(critic, "forward_into"):          # one masked launch: only the truncated-and-not-terminated rows are evaluated and stored
            critic.forward_into(x, out, clamp=None, rows=ro.truncated.view(-1), rows_not=ro.terminated.view(-1))
            return
        with torch.no_grad():
            p = next(iter(critic.parameters()), None) if hasattr(critic, "parameters") else None
            if p is not None and p.dtype != x.dtype:
                x = x.to(p.dtype)
            out.copy_(critic(x).reshape(-1))

    def compute(self, critic=None, values=None):
        """Fill ``values`` -- from ``critic`` (a ``FusedMLP`` or any torch module mapping ``[N, obs_dim]`` to ``[N, 1]``) or from
        the tensor ``values`` ``[T + 1, B]`` (slot T: SB3's ``last_values``) -- then ``advantages``, ``returns`` and the episode
        statistics in one launch.  Returns self."""
        import torch
        if (critic is None) == (values is None):
            raise ValueError("give exactly one of critic= and values=")
        if critic is not None:
            self._evaluate(critic)
            if self.bootstrap_truncated:
                self._bootstrap(critic)
        else:
            if tuple(values.shape) != (self.T + 1, self.B):
                raise ValueError(f"values must be [{self.T + 1}, {self.B}] (T + 1 observation slots), got {tuple(values.shape)}")
            self.values.copy_(values)
        boot = self.boot
        if boot is not None and (not torch.is_tensor(boot) or tuple(boot.shape) != (self.T, self.B) or boot.dtype != torch.float32
                                 or boot.device != self.values.device or not boot.is_contiguous()):
            raise ValueError(f"boot must be a contiguous float32 [{self.T}, {self.B}] tensor on {self.values.device}, got "
                             f"{getattr(boot, 'dtype', type(boot).__name__)} {tuple(getattr(boot, 'shape', ()))}")
        ro = self.rollout
        self.backend.gae(ro.rewards, self.values, ro.terminated, ro.truncated, self.advantages, self.returns, self.gamma,
                         self.gae_lambda, boot=boot, ep_return_acc=self.ep_return_acc, ep_length_acc=self.ep_length_acc,
                         episode_return=self.episode_return, episode_length=self.episode_length)
        return self

    def finished_episodes(self):
        """``(count, mean_return, mean_length)`` of the episodes that ended inside the last computed buffer, as 0-d device tensors
        (int64, float64, float64; the means are NaN when none ended): SB3's ``ep_rew_mean`` / ``ep_len_mean`` over this rollout,
        without a host synchronisation -- ``.item()`` them when logging."""
        if self.episode_length is None:
            raise ValueError("this buffer was built with episode_stats=False")
        count = (self.episode_length > 0).sum()
        return count, self.episode_return.sum() / count, self.episode_length.sum() / count.double()

    def flat(self) -> RolloutBatch:
        """The ``[T * B, ...]`` views a PPO update indexes with its minibatch permutation: observations of slots 0 .. T-1, actions,
        advantages, returns and values (of the same slots).  Views, not copies: valid until the next ``run()`` / ``compute()``."""
        ro, n = self.rollout, self.T * self.B
        return RolloutBatch(ro.obs[:self.T].reshape(n, *ro.obs.shape[2:]), ro.actions.reshape(n, *ro.actions.shape[2:]),
                            self.advantages.reshape(n), self.returns.reshape(n), self.values[:self.T].reshape(n))
