"""NumPy restatements of the SAC loss heads (include/pdegym.h: pdegym_squashed_gaussian_sample, its backward,
pdegym_sac_critic_loss, pdegym_sac_actor_loss).

The ``*_float64`` functions evaluate the header's formulas, closed-form gradients included, in float64: the yardstick of the
real-valued GPU tests, itself checked against torch float64 autograd over SB3's expressions in tests/test_sac_loss.py.  The
``*_float32`` functions follow the header's stated operation order -- float32 with one rounding per operation, np.exp / np.tanh /
np.log standing in for the device's expf / tanhf / logf -- and sum the float32 terms in float64, rounding once: where none of the
three functions decides a bit (integer-valued critic data with alpha == 1, the zero pattern of the gradients, the clip mask) they
give the kernels' bits.

Shapes: raw [N, 2A] = [mu; log_std], eps [N, A], obs [N, D] or None, d_actions [N, A] or None, d_log_prob [N], a scalar or None;
q1, q2, q1_target, q2_target, next_log_prob, log_prob [N] (q2 / q2_target None: one critic); rewards, dones [M] gathered by index
int64 [N] (None: M = N); log_alpha a scalar.
"""
from __future__ import annotations

import math

import numpy as np

CRITIC_STATS = ("critic_loss", "q1_mean", "q2_mean", "target_mean")
ACTOR_STATS = ("actor_loss", "ent_coef_loss", "alpha", "log_prob_mean")
HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)
EPSILON = 1e-6


def _clip_keep_nan(x, lo, hi):
    return np.where(np.isnan(x), x, np.minimum(np.maximum(x, lo), hi))


def _min_keep_nan(a, b):
    return np.where(np.isnan(a) | np.isnan(b), a + b, np.minimum(a, b))


def _squashed(raw, eps, lo, hi, dtype):
    raw, eps = np.asarray(raw, dtype), np.asarray(eps, dtype)
    A = raw.shape[1] // 2
    mu, log_std = raw[:, :A], raw[:, A:]
    ls = _clip_keep_nan(log_std, dtype(lo), dtype(hi))
    sigma = np.exp(ls).astype(dtype)
    a = np.tanh(mu + sigma * eps).astype(dtype)
    w = dtype(1.0) - a * a
    u = w + dtype(EPSILON)
    return log_std, ls, sigma, a, w, u, eps


def _sample(raw, eps, lo, hi, obs, dtype):
    with np.errstate(all="ignore"):
        _, ls, _, a, _, u, eps = _squashed(raw, eps, lo, hi, dtype)
        t = ((dtype(-0.5) * (eps * eps) - ls) - dtype(HALF_LOG_2PI)) - np.log(u).astype(dtype)
        logp = t[:, 0].copy()
        for j in range(1, t.shape[1]):
            logp = logp + t[:, j]
    block = a if obs is None else np.concatenate([np.asarray(obs, dtype), a], axis=1)
    return block, logp


def _sample_backward(raw, eps, lo, hi, d_actions, d_log_prob, dtype):
    assert d_actions is not None or d_log_prob is not None
    with np.errstate(all="ignore"):
        log_std, _, sigma, a, w, u, eps = _squashed(raw, eps, lo, hi, dtype)
        da = np.zeros_like(a) if d_actions is None else np.asarray(d_actions, dtype)
        dl = np.zeros((a.shape[0], 1), dtype) if d_log_prob is None else np.broadcast_to(np.asarray(d_log_prob, dtype).reshape(-1, 1),
                                                                                         (a.shape[0], 1))
        k = ((dtype(2.0) * a) * w) / u
        se = sigma * eps
        daw = da * w
        d_mu = daw + dl * k
        g = daw * se + dl * (k * se - dtype(1.0))
        d_ls = np.where((log_std >= dtype(lo)) & (log_std <= dtype(hi)), g, dtype(0.0))
    return np.concatenate([d_mu, d_ls], axis=1).astype(dtype), k


def sample_float64(raw, eps, lo, hi, obs=None):
    return _sample(raw, eps, lo, hi, obs, np.float64)


def sample_float32(raw, eps, lo, hi, obs=None):
    return _sample(raw, eps, lo, hi, obs, np.float32)


def sample_backward_float64(raw, eps, lo, hi, d_actions, d_log_prob):
    return _sample_backward(raw, eps, lo, hi, d_actions, d_log_prob, np.float64)[0]


def sample_backward_float32(raw, eps, lo, hi, d_actions, d_log_prob):
    return _sample_backward(raw, eps, lo, hi, d_actions, d_log_prob, np.float32)[0]


def saturation_k_float32(raw, eps, lo, hi):
    """The k = 2 a w / u of every element in the float32 order (the saturation test reads it)."""
    return _sample_backward(raw, eps, lo, hi, None, np.zeros(np.asarray(raw).shape[0]), np.float32)[1]


def _critic(q1, q2, q1t, q2t, lp, rewards, dones, log_alpha, gamma, index, dtype):
    c = lambda x: None if x is None else np.asarray(x, dtype)      # noqa: E731
    q1, q2, q1t, q2t, lp, rewards, dones = c(q1), c(q2), c(q1t), c(q2t), c(lp), c(rewards), c(dones)
    if index is not None:
        rewards, dones = rewards[index], dones[index]
    n = q1.shape[0]
    with np.errstate(all="ignore"):
        alpha = dtype(np.exp(dtype(log_alpha)))
        m = q1t if q2 is None else _min_keep_nan(q1t, q2t)
        y = rewards + ((dtype(1.0) - dones) * dtype(gamma)) * (m - alpha * lp)
        inv_n = dtype(1.0 / n)
        e1 = q1 - y
        e2 = None if q2 is None else q2 - y
        sq = (e1 * e1).astype(np.float64).sum() + (0.0 if q2 is None else (e2 * e2).astype(np.float64).sum())
        stats = np.array([0.5 * sq / n, q1.astype(np.float64).sum() / n, 0.0 if q2 is None else q2.astype(np.float64).sum() / n,
                          y.astype(np.float64).sum() / n]).astype(dtype)
    return {"d_q1": (e1 * inv_n).astype(dtype), "d_q2": None if q2 is None else (e2 * inv_n).astype(dtype), "target": y.astype(dtype),
            "stats": stats}


def critic_float64(q1, q2, q1_target, q2_target, next_log_prob, rewards, dones, log_alpha, gamma, index=None):
    return _critic(q1, q2, q1_target, q2_target, next_log_prob, rewards, dones, log_alpha, gamma, index, np.float64)


def critic_float32(q1, q2, q1_target, q2_target, next_log_prob, rewards, dones, log_alpha, gamma, index=None):
    return _critic(q1, q2, q1_target, q2_target, next_log_prob, rewards, dones, log_alpha, gamma, index, np.float32)


def _actor(q1, q2, lp, log_alpha, target_entropy, dtype):
    q1, lp = np.asarray(q1, dtype), np.asarray(lp, dtype)
    q2 = None if q2 is None else np.asarray(q2, dtype)
    n = q1.shape[0]
    with np.errstate(all="ignore"):
        log_alpha = dtype(log_alpha)
        alpha = dtype(np.exp(log_alpha))
        second = np.zeros(n, bool) if q2 is None else (~np.isnan(q1) & (np.isnan(q2) | (q2 < q1)))
        m = q1 if q2 is None else np.where(second, q2, q1)
        g = dtype(-dtype(1.0 / n))
        ent = (lp + dtype(target_entropy)).astype(np.float64).sum() / n
        stats = np.array([(alpha * lp - m).astype(np.float64).sum() / n, -np.float64(log_alpha) * ent, alpha,
                          lp.astype(np.float64).sum() / n]).astype(dtype)
    return {"d_q1_pi": np.where(second, dtype(0.0), g).astype(dtype),
            "d_q2_pi": None if q2 is None else np.where(second, g, dtype(0.0)).astype(dtype),
            "d_log_prob": np.array([alpha * dtype(1.0 / n)], dtype), "d_log_alpha": np.array([-ent]).astype(dtype), "stats": stats}


def actor_float64(q1_pi, q2_pi, log_prob, log_alpha, target_entropy):
    return _actor(q1_pi, q2_pi, log_prob, log_alpha, target_entropy, np.float64)


def actor_float32(q1_pi, q2_pi, log_prob, log_alpha, target_entropy):
    return _actor(q1_pi, q2_pi, log_prob, log_alpha, target_entropy, np.float32)


def seeded_sample_case(n, A, seed=0, D=0, z_max=4.0):
    """raw / eps (and obs) with |z| <= z_max and log_std in [-3, 1]: 1 - a^2 >= 1.3e-3 for z_max = 4, so the float32 cancellation in
    w stays bounded.  float32 arrays."""
    rng = np.random.default_rng([seed, n, A, 17])
    log_std = rng.uniform(-3.0, 1.0, (n, A))
    eps = np.clip(rng.normal(0.0, 1.0, (n, A)), -2.5, 2.5)
    z = rng.uniform(-z_max, z_max, (n, A)) * 0.98
    mu = z - np.exp(log_std) * eps
    case = {"raw": np.concatenate([mu, log_std], 1).astype(np.float32), "eps": eps.astype(np.float32)}
    if D:
        case["obs"] = rng.normal(0.0, 3.0, (n, D)).astype(np.float32)
    return case


def seeded_loss_case(n, seed=0, rows=None):
    """Critic / actor inputs: float32 arrays, rewards and dones of ``rows`` (default n) rows."""
    rng = np.random.default_rng([seed, n, 23])
    rows = n if rows is None else rows
    f = np.float32
    return {"q1": rng.normal(0.0, 3.0, n).astype(f), "q2": rng.normal(0.0, 3.0, n).astype(f), "q1_target": rng.normal(0.0, 3.0, n).astype(f),
            "q2_target": rng.normal(0.0, 3.0, n).astype(f), "next_log_prob": rng.normal(-1.0, 1.0, n).astype(f),
            "log_prob": rng.normal(-1.0, 1.0, n).astype(f), "rewards": rng.normal(0.0, 2.0, rows).astype(f),
            "dones": (rng.uniform(0, 1, rows) < 0.2).astype(f)}
