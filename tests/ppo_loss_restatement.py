"""NumPy restatements of the PPO loss head (include/pdegym.h: pdegym_ppo_loss, pdegym_diag_gaussian_log_prob).

``head_float64`` evaluates the header's formulas, closed-form gradients included, in float64: the yardstick of the real-valued GPU
tests, itself checked against torch float64 autograd over SB3's expression in tests/test_ppo_loss.py.  ``head_float32`` follows the
header's stated operation order for the per-row part -- float32 with one rounding per operation, np.exp standing in for the device's
expf -- and sums the float32 terms in float64, rounding once: where no exp decides a bit (integer-valued value terms, the zero
pattern of the gradient, a ratio of exactly 1) it gives the kernel's bits.

Both take NumPy arrays: mean [N, A], log_std [A], values [N] or None, actions [M, A], old_log_prob / advantages / returns [M],
index int64 [N] or None (M = N), and return a dict with ``d_mean`` [N, A], ``d_values`` [N] or None, ``d_log_std`` [A], ``stats``
[8] (STATS order) and, for the tests' own assertions, the per-row ``ratio``, ``adv`` (after normalisation) and ``g``.
"""
from __future__ import annotations

import math

import numpy as np

STATS = ("loss", "policy_loss", "value_loss", "entropy_loss", "approx_kl", "clip_fraction", "adv_mean", "adv_std")
HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)


def _gather(index, *arrays):
    return tuple(None if a is None else (a if index is None else a[index]) for a in arrays)


def log_prob_float64(mean, log_std, actions, index=None):
    (act,) = _gather(index, np.asarray(actions, np.float64))
    z = (act - np.asarray(mean, np.float64)) * np.exp(-np.asarray(log_std, np.float64))
    return (-0.5 * z * z - np.asarray(log_std, np.float64) - HALF_LOG_2PI).sum(axis=1)


def head_float64(mean, log_std, values, actions, old_log_prob, advantages, returns, clip_range, ent_coef, vf_coef, normalize,
                 index=None):
    f = lambda x: None if x is None else np.asarray(x, np.float64)      # noqa: E731
    mean, log_std, values = f(mean), f(log_std), f(values)
    act, old, adv, ret = _gather(index, f(actions), f(old_log_prob), f(advantages), f(returns))
    n, c = mean.shape[0], float(clip_range)
    adv_mean, adv_std = 0.0, 1.0
    with np.errstate(all="ignore"):
        if normalize and n > 1:
            adv_mean, adv_std = adv.mean(), adv.std(ddof=1)
            adv = (adv - adv_mean) / (adv_std + 1e-8)
        inv = np.exp(-log_std)
        z = (act - mean) * inv
        lr = (-0.5 * z * z - log_std - HALF_LOG_2PI).sum(axis=1) - old
        ratio = np.exp(lr)
        s1, s2 = adv * ratio, adv * np.where(np.isnan(ratio), ratio, np.clip(ratio, 1.0 - c, 1.0 + c))
        surr = np.where(np.isnan(s1) | np.isnan(s2), np.nan, np.minimum(s1, s2))
        out = ((ratio > 1.0 + c) & (adv > 0)) | ((ratio < 1.0 - c) & (adv < 0))
        g = np.where(out, 0.0, -(s1 / n))
        policy_loss = -surr.mean()
        entropy_loss = -(0.5 + HALF_LOG_2PI + log_std).sum()
        value_loss, d_values = 0.0, None
        if values is not None:
            value_loss = ((ret - values) ** 2).mean()
            d_values = vf_coef * 2.0 * (values - ret) / n
        stats = np.array([policy_loss + ent_coef * entropy_loss + vf_coef * value_loss, policy_loss, value_loss, entropy_loss,
                          ((ratio - 1.0) - lr).mean(), (np.abs(ratio - 1.0) > c).mean(), adv_mean, adv_std], np.float64)
        return {"d_mean": g[:, None] * z * inv, "d_values": d_values, "d_log_std": (g[:, None] * (z * z - 1.0)).sum(axis=0) - ent_coef,
                "stats": stats, "ratio": ratio, "adv": adv, "g": g}


def log_prob_float32(mean, log_std, actions, index=None):
    """The header's order: z = (a - mean) * inv;  t = ((-0.5 * (z * z)) - log_std) - 0.5 log 2 pi;  logp = t_0 + t_1 + ... ."""
    f32 = np.float32
    mean, log_std = np.asarray(mean, f32), np.asarray(log_std, f32)
    (act,) = _gather(index, np.asarray(actions, f32))
    inv = np.exp(-log_std).astype(f32)
    z = (act - mean) * inv
    t = (f32(-0.5) * (z * z) - log_std) - f32(HALF_LOG_2PI)
    logp = t[:, 0].copy()
    for j in range(1, t.shape[1]):
        logp = logp + t[:, j]
    return logp, z, inv


def head_float32(mean, log_std, values, actions, old_log_prob, advantages, returns, clip_range, ent_coef, vf_coef, normalize,
                 index=None):
    f32, f64 = np.float32, np.float64
    g32 = lambda x: None if x is None else np.asarray(x, f32)      # noqa: E731
    mean, log_std, values = g32(mean), g32(log_std), g32(values)
    old, adv, ret = _gather(index, g32(old_log_prob), g32(advantages), g32(returns))
    n, c = mean.shape[0], float(clip_range)
    lo, hi = f32(1.0 - c), f32(1.0 + c)
    adv_mean, adv_std = 0.0, 1.0
    with np.errstate(all="ignore"):
        if normalize and n > 1:
            d = adv.astype(f64) - f64(adv[0])                       # moments about the first gathered advantage, in float64
            s1_, s2_ = d.sum(), (d * d).sum()
            adv_mean = f64(adv[0]) + s1_ / n
            var = (s2_ - s1_ * s1_ / n) / (n - 1.0)
            adv_std = math.sqrt(0.0 if var < 0.0 else var) if not np.isnan(var) else np.nan
            adv = (adv - f32(adv_mean)) / (f32(adv_std) + f32(1e-8))
        logp, z, inv = log_prob_float32(mean, log_std, actions, index)
        lr = logp - old
        ratio = np.exp(lr).astype(f32)
        s1 = adv * ratio
        s2 = adv * np.where(np.isnan(ratio), ratio, np.minimum(np.maximum(ratio, lo), hi))
        surr = np.where(np.isnan(s1) | np.isnan(s2), f32(np.nan), np.minimum(s1, s2)).astype(f32)
        out = ((ratio > hi) & (adv > 0)) | ((ratio < lo) & (adv < 0))
        g = np.where(out, f32(0.0), -(s1 * f32(1.0 / n))).astype(f32)
        r1 = ratio - f32(1.0)
        policy_loss = -(surr.astype(f64).sum() / n)
        entropy_loss = 0.0
        for j in range(log_std.shape[0]):
            entropy_loss -= 0.5 + HALF_LOG_2PI + f64(log_std[j])
        value_loss, d_values = 0.0, None
        if values is not None:
            dv = values - ret
            value_loss = (dv * dv).astype(f64).sum() / n
            d_values = dv * f32(2.0 * vf_coef / n)
        stats = np.array([policy_loss + ent_coef * entropy_loss + vf_coef * value_loss, policy_loss, value_loss, entropy_loss,
                          (r1 - lr).astype(f64).sum() / n, (np.abs(r1) > f32(c)).astype(f64).sum() / n, adv_mean, adv_std]).astype(f32)
        d_log_std = ((g[:, None] * (z * z - f32(1.0))).astype(f64).sum(axis=0) - ent_coef).astype(f32)
        return {"d_mean": ((g[:, None] * z) * inv).astype(f32), "d_values": d_values, "d_log_std": d_log_std, "stats": stats,
                "ratio": ratio, "adv": adv, "g": g}


def seeded_case(n, A, seed=0, rows=None, spread=0.3):
    """A seeded minibatch: buffer arrays of ``rows`` (default n) rows, dense network outputs of n rows, and old log-probabilities
    that put the ratios at exp(N(0, spread)).  Returns a dict of float32 arrays (no index)."""
    rng = np.random.default_rng([seed, n, A])
    rows = n if rows is None else rows
    f32 = np.float32
    case = {"log_std": rng.uniform(-1.0, 0.3, A).astype(f32), "mean": rng.normal(0.0, 1.0, (n, A)).astype(f32),
            "values": rng.normal(0.0, 2.0, n).astype(f32), "actions": rng.normal(0.0, 1.2, (rows, A)).astype(f32),
            "advantages": rng.normal(0.3, 1.5, rows).astype(f32), "returns": rng.normal(0.0, 2.0, rows).astype(f32)}
    case["old_log_prob"] = rng.normal(-1.0 * A, 1.0, rows).astype(f32)
    case["_spread"] = spread
    return case


def with_old_log_prob_near(case, index=None, seed=1):
    """Replace ``old_log_prob`` at the gathered rows by logp - N(0, spread): ratios around 1.  With a repeated index the last
    writer wins (those rows then have whatever ratio results)."""
    rng = np.random.default_rng(seed)
    logp = log_prob_float64(case["mean"], case["log_std"], case["actions"], index)
    old = case["old_log_prob"].copy()
    k = np.arange(logp.shape[0]) if index is None else index
    old[k] = (logp - rng.normal(0.0, case["_spread"], logp.shape[0])).astype(np.float32)
    return {**case, "old_log_prob": old}
