"""The bookkeeping of the LDS-row step kernel (csrc/pdegym_1d.hip: step1d_wide_kernel) against the oracle, path by path.

The random fuzz (tests/fuzz_1d.py) reaches that kernel only by chance; here explicit case dicts go through the fuzz's own run half
(fuzz_1d.run_case: rows, observations, flags, time index and history bit for bit, rewards rtol 2e-6) at the smallest shapes that take
the kernel -- float32 rows of nx = 2049 (one node past the register-resident limit), and in the float64-operand mode (float64 beta
and float64 action) rows of 9 slots per lane: nx = 513 transport, nx = 576 parabolic.  B = 2, S = 34, nt = 103: three env-steps to
the end of the episode and one step after it (no sub-step left; with the fused auto-reset the first step of the next episode).

Axes: control {Dirichlet, Neumann} x sensing {full, collocated, opposite/Neumann, opposite/Dirichlet (transport only: the parabolic
reference refuses it)} are crossed in full per kernel variant; reward {TunedReward1D, L1 temporal, L2 differential, max norm
t-horizon 7}, history {off, on} and auto-reset {off, on: pool of 2B rows, beta pool, final observation kept} cycle through those
pairs so that every value of every axis -- and every reward x auto-reset pair -- meets every variant (PARABOLIC x M64).
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

B, S, NT = 2, 34, 103
VARIANTS = {  # name -> (kind, nx, float64 operands)
    "transport_f32": ("transport", 2049, False),
    "parabolic_f32": ("parabolic", 2049, False),
    "transport_m64": ("transport", 513, True),
    "parabolic_m64": ("parabolic", 576, True),
}
REWARDS = (("tuned", "temporal"), ("n1", "temporal"), ("n2", "differential"), ("ninf", "t-horizon"))


def _pairs(kind):
    sens = [("full", None), ("collocated", "Dirchilet"), ("opposite", "Neumann")] + ([("opposite", "Dirchilet")] if kind == "transport" else [])
    return [(c, s) for s in sens for c in ("Dirchilet", "Neumann")]


def _cases():
    out = []
    for name, (kind, _, _) in VARIANTS.items():
        pairs = _pairs(kind)
        for i in range(8):
            ctrl, (sloc, stype) = pairs[i % len(pairs)]
            out.append(pytest.param(name, ctrl, sloc, stype, REWARDS[i % 4], bool((i // 2) % 2), bool((i + i // 4) % 2),
                                    id=f"{name}-{ctrl[:3]}-{sloc}{'' if stype is None else '_' + stype[:3]}-{REWARDS[i % 4][0]}-hist{(i // 2) % 2}-auto{(i + i // 4) % 2}"))
    return out


def _case(name, ctrl, sloc, stype, reward, hist, auto):
    kind, nx, m64 = VARIANTS[name]
    base_par = kind == "parabolic"
    n = nx + (1 if base_par else 0)
    dx = 1.0 / nx
    dt = 0.25 * dx * dx if base_par else 0.5 * dx
    x = np.linspace(0, 1, n)
    kw = dict(T=(NT - 1) * dt, dt=dt, X=1, dx=dx, control_sample_rate=S * dt, control_type=ctrl, sensing_loc=sloc, sensing_type=stype,
              normalize=ctrl == "Dirchilet", max_control_value=20.0, limit_pde_state_size=True, max_state_value=1e10)
    assert int(round(kw["T"] / dt) + 1) == NT
    amp = 50 if base_par else 5
    init = (np.array([[2.0], [3.5]]) * (1 + 0.3 * np.sin(2 * np.pi * x * np.array([[1.0], [2.5]])))).astype(np.float32)
    beta = amp * 0.6 * np.cos(np.array([[2.0], [7.5]]) * np.arccos(x))
    P = 2 * B
    pool = (np.array([[0.5], [1.0], [1.5], [2.5]]) * np.ones((1, n))).astype(np.float32)
    bpool = amp * 0.4 * np.cos(np.array([[1.5], [3.0], [5.0], [8.0]]) * np.arccos(x))
    actions = [np.array(a) for a in ([0.25, -0.5], [1.0, 0.0], [-0.75, 10.0], [0.5, -0.25])]
    return dict(idx=0, kind=kind, kw=kw, nx=nx, S=S, nt=NT, B=B, nsteps=3, ic="smooth", init=init, beta=beta if m64 else beta.astype(np.float32),
                shared=False, rargs=(NT - 1, -1e3, 3e2), rkind=reward[0], hz=reward[1], klen=7, beta64=m64, akind="f64" if m64 else "f32",
                hist=hist, auto=auto, P=P, pool=pool, use_bpool=auto, bpool=bpool if m64 else bpool.astype(np.float32),
                actions=actions if m64 else [a.astype(np.float32) for a in actions])


@pytest.mark.parametrize("name,ctrl,sloc,stype,reward,hist,auto", _cases())
def test_wide_kernel_bookkeeping_matches_oracle(name, ctrl, sloc, stype, reward, hist, auto):
    import fuzz_1d
    desc = fuzz_1d.run_case(_case(name, ctrl, sloc, stype, reward, hist, auto))
    assert not desc.endswith(")"), desc      # "both refuse" / "look-back raises" would be a case that checked nothing


def test_every_axis_value_meets_every_variant():
    seen = {}
    for p in _cases():
        name, ctrl, sloc, stype, reward, hist, auto = p.values
        seen.setdefault(name, set()).update({("ctrl", ctrl), ("sense", sloc, stype), ("reward", reward), ("hist", hist), ("auto", auto),
                                             ("reward x auto", reward, auto)})
    for name, (kind, _, _) in VARIANTS.items():
        want = {("ctrl", c) for c in ("Dirchilet", "Neumann")} | {("sense", *s) for _, s in _pairs(kind)} | {("reward", r) for r in REWARDS}
        want |= {("hist", h) for h in (False, True)} | {("auto", a) for a in (False, True)} | {("reward x auto", r, a) for r in REWARDS for a in (False, True)}
        assert want <= seen[name], (name, want - seen[name])
