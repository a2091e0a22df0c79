"""The TrafficPDE1D backstepping law restated for the tests (no text of the reference's notebook is copied): the weight rows, the
command through ``np.trapz`` itself, the command with ``np.trapz``'s order of addition written out (what the device's "numpy" order
implements), and a model of the "tree" order together with the bound that separates the two.

Per instance: rs, vs = Veq(rs), qs = rs vs, ps = vm/rm qs/vs; x the grid of M nodes; lambda1 = vs, lambda2 = vs + rs (-vm/rm).
    K  = -(1/(gamma ps)) (-1/tau) exp(-x/(tau vs));  Mk = -K;  E = exp(x/(vs tau))
    cv = Mk + (lambda2/lambda1) K E;  cq = ((lambda1 - lambda2)/lambda1) K E
    Iv = trapz(cv (v - vs), dx);  Iq = trapz(cq (r v - qs), dx);  q_out = (qs + rs Iv) + Iq
"""
from __future__ import annotations

import numpy as np

U = 2.0 ** -53


def steady(vm, rm, rs):
    """(vs, qs, ps) of a steady-state density, in the engine's operation order (vs = vm (1 - rs/rm), qs = rs vs)."""
    vs = vm * (1 - rs / rm)
    qs = rs * vs
    ps = vm / rm * qs / vs
    return vs, qs, ps


def weights(x, vm, rm, tau, rs, gamma=1.0):
    """(cv, cq): float64 [M], every operation in the order the law is written in."""
    x = np.asarray(x, dtype=np.float64)
    vs, qs, ps = steady(vm, rm, rs)
    lam1 = vs
    lam2 = vs + rs * (-vm / rm)
    K = -(1 / (gamma * ps)) * (-1 / tau) * np.exp(-x / (tau * vs))
    Mk = -K
    E = np.exp(x / (vs * tau))
    cv = Mk + (lam2 / lam1) * K * E
    cq = ((lam1 - lam2) / lam1) * K * E
    return cv, cq


def products(r, v, cv, cq, vs, qs):
    """The two integrands at the nodes."""
    v_err = v - vs
    q = r * v
    q_err = q - qs
    return cv * v_err, cq * q_err


def command_trapz(r, v, cv, cq, dx, rs, vs, qs):
    """q_out with np.trapz itself (the reference's call)."""
    trapz = getattr(np, "trapezoid", None) or np.trapz      # (one function under two names since NumPy 2.0; the old one warns)
    pv, pq = products(np.asarray(r).flatten(), np.asarray(v).flatten(), cv.flatten(), cq.flatten(), vs, qs)
    iv = trapz(pv, dx=dx)
    iq = trapz(pq, dx=dx)
    return qs + rs * iv + iq


def trapz_terms(p, dx):
    """t_i = (dx (p[i+1] + p[i])) / 2.0, i < len(p) - 1: the array np.trapz sums."""
    p = np.asarray(p, dtype=np.float64)
    return np.array([(dx * (p[i + 1] + p[i])) / 2.0 for i in range(len(p) - 1)], dtype=np.float64)


def numpy_order_sum(t):
    """Sum of the float64 terms ``t`` in the order np.add.reduce adds a contiguous row (n <= 128 un-recursed; longer rows halve
    recursively, n2 = n/2, n2 -= n2 % 8), one Python float operation per addition."""
    t = [float(z) for z in t]
    n = len(t)
    if n < 8:
        s = 0.0
        for z in t:
            s += z
        return s
    if n <= 128:
        a = t[:8]
        n8 = n - n % 8
        for i in range(8, n8, 8):
            for k in range(8):
                a[k] = a[k] + t[i + k]
        s = ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]))
        for i in range(n8, n):
            s += t[i]
        return s
    n2 = n // 2
    n2 -= n2 % 8
    return numpy_order_sum(t[:n2]) + numpy_order_sum(t[n2:])


def command_numpy_order(r, v, cv, cq, dx, rs, vs, qs):
    """q_out with the order of addition written out: what ``order="numpy"`` computes on the device, bit for bit."""
    pv, pq = products(np.asarray(r, dtype=np.float64), np.asarray(v, dtype=np.float64), cv, cq, vs, qs)
    iv = numpy_order_sum(trapz_terms(pv, dx))
    iq = numpy_order_sum(trapz_terms(pq, dx))
    return (qs + rs * iv) + iq


def tree_bound(r, v, cv, cq, dx, rs, vs, qs):
    """How far a command summed in another order (``order="tree"``) may lie from the "numpy" one.  The terms t_i are the same
    floating-point numbers in both; a sum of n of them in ANY order is within (n - 1) u sum|t_i| of the exact sum (u = 2**-53, first
    order), so two orders differ by at most 2 n u sum|t_i|.  Carried through q_out = (qs + rs Iv) + Iq: the integrals enter with
    weights |rs| and 1, and each of the three roundings (rs Iv, qs + ., . + Iq) may differ by one more unit of its result in each
    computation:  2 u [ (n + 2) (|rs| sum|tv_i| + sum|tq_i|) + |rs Iv| + |qs + rs Iv| + |q_out| ]   (n + 2: second-order terms)."""
    pv, pq = products(np.asarray(r, dtype=np.float64), np.asarray(v, dtype=np.float64), cv, cq, vs, qs)
    tv, tq = trapz_terms(pv, dx), trapz_terms(pq, dx)
    n = len(tv)
    iv, iq = numpy_order_sum(tv), numpy_order_sum(tq)
    a = rs * iv
    b = qs + a
    return 2 * U * ((n + 2) * (abs(rs) * np.abs(tv).sum() + np.abs(tq).sum()) + abs(a) + abs(b) + abs(b + iq))


def tree_order_sum(t, wave=64):
    """A model of the "tree" order: lane l adds t_l, t_{l+64}, ... from 0.0 in ascending order, then the lanes' partial sums are
    reduced (pair, quad, half row, row, rows 0+1 and 2+3, halves).  The tests hold the device to ``tree_bound``, not to this model."""
    part = [0.0] * wave
    for i, z in enumerate(t):
        part[i % wave] += float(z)
    while len(part) > 1:
        part = [part[2 * i] + part[2 * i + 1] for i in range(len(part) // 2)]
    return part[0]


def golden_case(g, name):
    """The arrays of case ``name`` of tests/golden/traffic_backstep.npz as a dict; an array a 'both' case shares with its 'outlet'
    twin (``<case>/shares``: the twin's name, then the shared keys) is taken from there."""
    out = {k.split("/", 1)[1]: g[k] for k in g.files if k.startswith(name + "/") and not k.endswith("/shares")}
    if name + "/shares" in g.files:
        twin, *keys = [str(s) for s in g[name + "/shares"]]
        out.update({k: g[f"{twin}/{k}"] for k in keys})
    # the commands are stored by the end they drive (one column each); the environment takes them as (inlet, outlet)
    out["commands"] = np.stack([out[k] for k in ("command_inlet", "command_outlet") if k in out], axis=1)
    out["obs_steps"] = g["obs_steps"]
    out.update(zip(META_KEYS, out["meta"]))
    out["params"] = out["meta"][len(META_KEYS):]
    return out


META_KEYS = ("reward_sum", "steps", "M")      # <case>/meta: these three, then the parameters (the generator's PARAM_KEYS)


def law_commands(sim, r, v, cv, cq, dx, rs, vs, qs, command=command_numpy_order):
    """The command(s) of one instance: qs for 'inlet', q_out for 'outlet', (qs, q_out) for 'both'."""
    if sim == "inlet":
        return (qs,)
    q_out = command(r, v, cv, cq, dx, rs, vs, qs)
    return (q_out,) if sim == "outlet" else (qs, q_out)
