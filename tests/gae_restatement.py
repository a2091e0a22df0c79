"""NumPy restatement of what pdegym_gae computes (include/pdegym.h): Stable-Baselines3's
``RolloutBuffer.compute_returns_and_advantage`` in float32, the truncation bootstrap of ``OnPolicyAlgorithm.collect_rollouts`` and
the float64 episode scan.  SB3 is not imported: the loop is written out here as SB3 writes it -- float32 arrays, ``gamma`` and
``gae_lambda`` Python floats, which NumPy rounds to float32 where they meet an array (``gamma * gae_lambda`` is a Python product,
rounded once) -- so every operation is one float32 rounding, in SB3's order.

Plain helper module (not a conftest, not a test): imported by tests/fake_gae_backend.py, tests/test_gae.py and tests/test_gpu_gae.py.
"""
from __future__ import annotations

import numpy as np

f32 = np.float32


def gae_reference(rewards, values, terminated, truncated, gamma, gae_lambda, boot=None):
    """``rewards`` [T, B] float32 or float64, ``values`` [T + 1, B] float32, flags [T, B] (``truncated`` may be None), ``boot``
    None or [T, B] float32.  Returns ``(advantages, returns)``, float32 [T, B]."""
    rewards, values = np.asarray(rewards), np.asarray(values)
    assert values.dtype == f32 and rewards.dtype in (np.float32, np.float64)
    T, B = rewards.shape
    te = np.asarray(terminated).astype(bool)
    tr = np.zeros_like(te) if truncated is None else np.asarray(truncated).astype(bool)
    gamma, gae_lambda = float(gamma), float(gae_lambda)
    with np.errstate(all="ignore"):
        r = rewards.astype(f32)                                     # SB3 stores float32 rewards: one rounding
        if boot is not None:                                        # collect_rollouts: rewards[idx] += self.gamma * terminal_value
            boot = np.asarray(boot)
            assert boot.dtype == f32
            r = np.where(tr & ~te, r + f32(gamma) * boot, r)        # a select: an entry the rule does not pick has no effect
        dones = te | tr
        adv = np.zeros((T, B), f32)
        last_gae_lam = np.zeros(B, f32)
        for step in reversed(range(T)):
            next_non_terminal = f32(1.0) - dones[step].astype(f32)
            next_values = values[step + 1]
            delta = r[step] + gamma * next_values * next_non_terminal - values[step]
            last_gae_lam = delta + gamma * gae_lambda * next_non_terminal * last_gae_lam
            assert delta.dtype == f32 and last_gae_lam.dtype == f32
            adv[step] = last_gae_lam
        returns = adv + values[:-1]
    return adv, returns


def gae_explicit(rewards, values, terminated, truncated, gamma, gae_lambda, boot=None):
    """The same recurrence with every rounding spelled out as the kernel spells it (g, gl float32 scalars; the product gamma *
    gae_lambda formed in double): must equal ``gae_reference`` bit for bit."""
    T, B = np.asarray(rewards).shape
    te = np.asarray(terminated).astype(bool)
    tr = np.zeros_like(te) if truncated is None else np.asarray(truncated).astype(bool)
    g, gl = f32(gamma), f32(float(gamma) * float(gae_lambda))
    adv, ret = np.zeros((T, B), f32), np.zeros((T, B), f32)
    last = np.zeros(B, f32)
    with np.errstate(all="ignore"):
        for t in reversed(range(T)):
            nn = f32(1.0) - (te[t] | tr[t]).astype(f32)
            r = np.asarray(rewards)[t].astype(f32)
            if boot is not None:
                r = np.where(tr[t] & ~te[t], r + g * np.asarray(boot)[t], r)
            delta = (r + (g * values[t + 1]) * nn) - values[t]
            last = delta + ((gl * nn) * last)
            adv[t], ret[t] = last, last + values[t]
    return adv, ret


def gae_float64_rounded(rewards, values, terminated, truncated, gamma, gae_lambda):
    """What the restatement must NOT be: the recurrence carried in float64 and rounded to float32 at the end."""
    T, B = np.asarray(rewards).shape
    dones = np.asarray(terminated).astype(bool) | (np.asarray(truncated).astype(bool) if truncated is not None else False)
    v, r = np.asarray(values, dtype=np.float64), np.asarray(rewards, dtype=np.float64)
    adv, last = np.zeros((T, B)), np.zeros(B)
    for t in reversed(range(T)):
        nn = 1.0 - dones[t]
        last = (r[t] + gamma * v[t + 1] * nn - v[t]) + gamma * gae_lambda * nn * last
        adv[t] = last
    return adv.astype(f32), (adv + v[:-1]).astype(f32)


def episode_scan(rewards, terminated, truncated, acc=None, length=None):
    """Forward in t, in double: acc += reward as loaded (float32 widened, or the float64 reward itself), len += 1; where done the
    outputs receive (acc, len) and both restart from zero, elsewhere 0.0 and 0.  Returns ``(episode_return [T, B] float64,
    episode_length [T, B] int32, acc [B] float64, length [B] int32)``; ``acc`` / ``length`` None: every environment starts from zero."""
    rewards = np.asarray(rewards)
    T, B = rewards.shape
    dones = np.asarray(terminated).astype(bool) | (np.asarray(truncated).astype(bool) if truncated is not None else False)
    acc = np.zeros(B, np.float64) if acc is None else np.array(acc, dtype=np.float64)
    length = np.zeros(B, np.int32) if length is None else np.array(length, dtype=np.int32)
    ep_ret, ep_len = np.zeros((T, B), np.float64), np.zeros((T, B), np.int32)
    with np.errstate(all="ignore"):
        for t in range(T):
            acc = acc + rewards[t].astype(np.float64)
            length = length + np.int32(1)
            ep_ret[t] = np.where(dones[t], acc, 0.0)
            ep_len[t] = np.where(dones[t], length, 0)
            acc = np.where(dones[t], 0.0, acc)
            length = np.where(dones[t], 0, length).astype(np.int32)
    return ep_ret, ep_len, acc, length


def seeded_case(T, B, seed=0, f64_rewards=False, p_term=0.08, p_trunc=0.08):
    """Rewards, values, flags and boot of a seeded rollout: O(1) values and rewards of both signs, independent flags (so steps with
    both flags set occur), boot everywhere."""
    rng = np.random.default_rng([seed, T, B])
    rewards = rng.normal(0.0, 1.0, (T, B))
    rewards = rewards if f64_rewards else rewards.astype(f32)
    values = rng.normal(0.0, 2.0, (T + 1, B)).astype(f32)
    terminated = (rng.random((T, B)) < p_term).astype(np.uint8)
    truncated = (rng.random((T, B)) < p_trunc).astype(np.uint8)
    boot = rng.normal(0.0, 2.0, (T, B)).astype(f32)
    return rewards, values, terminated, truncated, boot
