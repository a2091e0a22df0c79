"""``pdegym_fused_adam`` in NumPy (include/pdegym.h: fused optimiser step).  ``step(..., dtype=np.float64)`` is the yardstick: the
recurrence of ``clip_grad_norm_`` + ``torch.optim.Adam`` (+ SB3's ``polyak_update``) in double precision.  ``dtype=np.float32`` follows
the header's order: the running products ``beta^t`` and the scalars formed from them in double, every float32 operation rounded on
its own (NumPy rounds after each array operation).  The sum of squares is a float64 sum in NumPy's order: the kernel's order is its
own, so bit comparisons use gradients whose squares add exactly (multiples of 2^-10, |g| <= 4)."""
from __future__ import annotations

import numpy as np


def new_state():
    return np.array([0.0, 1.0, 1.0], np.float64)      # step count, beta1^t, beta2^t


def blocked(w, out_total=None, row0=0, into=None):
    """The blocked transpose [ceil(in / 4), out_total, 4] of a weight (out, in): rows row0 .. row0 + out written, padding left alone."""
    out, in_ = w.shape
    k4 = (in_ + 3) // 4
    out_total = out if out_total is None else out_total
    wt = np.zeros((k4, out_total, 4), w.dtype) if into is None else into
    for i in range(in_):
        wt[i // 4, row0:row0 + out, i % 4] = w[:, i]
    return wt


def step(tensors, state, lr, beta1, beta2, eps, max_grad_norm=None, tau=None, polyak=False, dtype=np.float32):
    """One call, in place.  ``tensors``: dicts with ``p``, ``g``, ``m``, ``v`` (arrays of ``dtype``) and optionally ``copy`` (array of
    p's size), ``wt`` = (blocked array, out_total, row0), ``pt``, ``pt_copy``, ``pt_wt``.  ``state``: float64 [3].  Returns the total
    norm (``dtype``; None when no norm is formed)."""
    f = dtype
    state[0] += 1.0
    state[1] *= np.float64(beta1)
    state[2] *= np.float64(beta2)
    clip = max_grad_norm is not None and max_grad_norm > 0.0      # (False for a NaN)
    total = coef = None
    with np.errstate(all="ignore"):
        if max_grad_norm is not None:      # (the norm is formed whenever the caller asks for it, clipping or not)
            s = np.float64(0.0)
            for t in tensors:
                g = t["g"].astype(f)
                s += (g * g).astype(np.float64).sum()
            total = f(np.sqrt(s))
        if clip:
            c = f(max_grad_norm) / (total + f(1e-6))
            coef = c if np.isnan(c) else min(c, f(1.0))
        step_size = f(np.float64(lr) / (1.0 - state[1]))
        bc2_sqrt = f(np.sqrt(1.0 - state[2]))
        c1, b2, c2, eps_f = f(1.0 - np.float64(beta1)), f(beta2), f(1.0 - np.float64(beta2)), f(eps)
        for t in tensors:
            g = t["g"].astype(f)
            gs = g * coef if clip else g
            m, v, p = t["m"], t["v"], t["p"]
            m[...] = m + c1 * (gs - m)
            v[...] = b2 * v + c2 * (gs * gs)
            denom = np.sqrt(v) / bc2_sqrt + eps_f
            p[...] = p - step_size * (m / denom)
            _mirror(t, p, "")
            if polyak and t.get("pt") is not None:
                pt = t["pt"]
                pt[...] = f(1.0 - np.float64(tau)) * pt + f(tau) * p
                _mirror(t, pt, "pt_")
    return total


def _mirror(t, x, prefix):
    if t.get(prefix + "copy") is not None:
        t[prefix + "copy"].reshape(-1)[...] = x.reshape(-1)
    if t.get(prefix + "wt") is not None:
        wt, out_total, row0 = t[prefix + "wt"]
        w = x if x.ndim == 2 else x.reshape(1, -1)
        blocked(w, out_total, row0, into=wt.reshape((w.shape[1] + 3) // 4, out_total, 4))
