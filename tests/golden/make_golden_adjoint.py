#!/usr/bin/env python3
"""Generate tests/golden/adjoint_ns.npz: the adjoint-optimisation baseline of the reference
(examples/NavierStokes/NS2Doptimization.py:56-118) on small cases.

The script cannot be imported (it runs at import and needs gym.make), so its loop is restated below -- as gen_kat of
make_golden.py restates the backstepping examples -- and drives the reference's OWN NavierStokes2D.step, solve_pressure,
central_difference and laplace: every number of a case comes out of the reference's code.  One thing differs from the script on
purpose: the adjoint equation's viscosity is the environment's (the script writes the literal 0.1, its environment's value); the
case whose viscosity is not 0.1 says so in its key.  The cases, their parameters and their seeded inputs are those of
tests/adjoint_restatement.py (CASES, case_params, case_inputs).  The case under ``restatement_only/`` has nx != ny, which the
reference cannot run (its arrays are [nx, ny] where its stencils assume [ny, nx]): it is written by the restatement itself.

Run:  python tests/golden/make_golden_adjoint.py [--check]      (needs the reference checkout; not run on the GPU box)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

from make_golden import import_reference  # noqa: E402
from tests import adjoint_restatement as R  # noqa: E402

FILE = "adjoint_ns.npz"


def apply_boundary(a1, a2):          # NS2Doptimization.py:56-61
    a1[:, [-1, 0]] = 0.
    a1[[-1, 0], :] = 0.
    a2[:, [-1, 0]] = 0.
    a2[[-1, 0], :] = 0.
    return a1, a2


def run_reference(src, ns_mod, c):
    central_difference, laplace = ns_mod.central_difference, ns_mod.laplace
    prm, inp = R.case_params(c), R.case_inputs(c)
    T, dt, dx, dy = c["T"], prm["dt"], prm["dx"], prm["dy"]
    u_target, v_target = inp["U_ref"][..., 0], inp["U_ref"][..., 1]
    env = src.NavierStokes2D(action_dim=1, reward_class=src.NSReward(0.1), normalize=False,
                             reset_init_condition_func=lambda X: (inp["u0"].copy(), inp["v0"].copy(), inp["p0"].copy()),
                             boundary_condition=R.BC, U_ref=inp["U_ref"], action_ref=2.0 * np.ones(T + 2), **prm)
    assert (env.nx, env.ny, env.nt) == (c["n"], c["n"], T + 1)
    nu = env.KINEMATIC_VISCOSITY
    # :71-77
    env.reset(seed=400)
    U, V, rewards0 = [], [], []
    for t in range(T):
        obs, reward, done, _, _ = env.step(inp["actions0"][t])
        U.append(env.u.copy())
        V.append(env.v.copy())
        rewards0.append(reward)
    Ufwd, Vfwd = np.stack(U), np.stack(V)
    u_ref = [2 for _ in range(T)]
    # :83-102
    Lam1, Lam2 = [], []
    Lam1.append(np.zeros_like(U[0]))
    Lam2.append(np.zeros_like(U[0]))
    pressure = np.zeros_like(U[0])
    for t in range(T - 1):
        lam1, lam2 = Lam1[-1], Lam2[-1]
        dl1dx, dl1dy = central_difference(lam1, "x", dx), central_difference(lam1, "y", dy)
        dl2dx, dl2dy = central_difference(lam2, "x", dx), central_difference(lam2, "y", dy)
        laplace_l1, laplace_l2 = laplace(lam1, dx, dy), laplace(lam2, dx, dy)
        dlam1dt = - 2 * dl1dx * U[-1-t] - dl1dy * V[-1-t] - dl2dx * V[-1-t] - nu * laplace_l1 + (U[-1-t]-u_target[-1-t])
        dlam2dt = - 2 * dl2dy * V[-1-t] - dl1dy * U[-1-t] - dl2dx * U[-1-t] - nu * laplace_l2 + (V[-1-t]-v_target[-1-t])
        lam1 = lam1 - dt * dlam1dt
        lam2 = lam2 - dt * dlam2dt
        lam1, lam2 = apply_boundary(lam1, lam2)
        pressure = env.solve_pressure(lam1, lam2, pressure)
        lam1 = lam1 - dt * central_difference(pressure, "x", dx)
        lam2 = lam2 - dt * central_difference(pressure, "y", dy)
        lam1, lam2 = apply_boundary(lam1, lam2)
        Lam1.append(lam1)
        Lam2.append(lam2)
    Lam1, Lam2 = Lam1[::-1], Lam2[::-1]
    # :104-107
    actions, grad = [], []
    for t in range(T):
        dl1dx2 = central_difference(Lam1[t], "y", dy)
        grad.append(sum(dl1dx2[-2, :]))
        actions.append(u_ref[t] - 0.1/0.1 * sum(dl1dx2[-2, :])*5*dx)
    # :109-115 (the reset function hands back the same fields: see NSAdjointOptimizer.optimize)
    env.reset(seed=400)
    rewards = []
    for t in range(T):
        obs, reward, done, _, _ = env.step(actions[t])
        rewards.append(reward)
    out = dict(grad=np.array(grad, dtype=np.float64), actions=np.array(actions, dtype=np.float64),
               reward_sums=np.array([sum(rewards0), sum(rewards)], dtype=np.float64))
    if not c.get("sums_only"):
        out.update(inp, U=Ufwd, V=Vfwd, lam1=np.stack(Lam1), lam2=np.stack(Lam2), rewards0=np.array(rewards0, dtype=np.float64),
                   rewards=np.array(rewards, dtype=np.float64), params=np.array([prm[k] for k in PARAM_KEYS], dtype=np.float64))
    return out


PARAM_KEYS = ("T", "dt", "X", "dx", "Y", "dy", "viscosity", "density", "maximum_pressure_iteration")


def run_restatement(c):
    prm, inp = R.case_params(c), R.case_inputs(c)
    r = R.run_case(c)
    return dict(inp, U=r["obs"][1:, 0, ..., 0], V=r["obs"][1:, 0, ..., 1], lam1=r["lam"][:, 0, ..., 0], lam2=r["lam"][:, 0, ..., 1],
                grad=r["grad"][:, 0], actions=r["actions"][:, 0], rewards0=r["rewards0"][:, 0], rewards=r["rewards"][:, 0],
                reward_sums=np.array([sum(r["rewards0"][:, 0]), sum(r["rewards"][:, 0])], dtype=np.float64),
                params=np.array([prm[k] for k in PARAM_KEYS], dtype=np.float64))


def generate(out=HERE):
    src = import_reference()
    import importlib
    ns_mod = importlib.import_module("pde_control_gym.src.environments2d.navier_stokes2D")
    store = {}
    for name, c in R.CASES.items():
        for k, v in run_reference(src, ns_mod, c).items():
            assert np.all(np.isfinite(v)), (name, k)
            store[f"{name}/{k}"] = v
    for name, c in R.RESTATEMENT_ONLY.items():
        for k, v in run_restatement(c).items():
            assert np.all(np.isfinite(v)), (name, k)
            store[f"restatement_only/{name}/{k}"] = v
    path = os.path.join(out, FILE)
    np.savez_compressed(path, **store)
    return path


def check():
    """Regenerate into a scratch directory and compare with the committed file: same keys, dtypes, shapes and bits."""
    import tempfile
    diffs = []
    with tempfile.TemporaryDirectory() as tmp:
        b = np.load(generate(tmp), allow_pickle=False)
        a = np.load(os.path.join(HERE, FILE), allow_pickle=False)
        for k in sorted(set(a.files) | set(b.files)):
            if k not in a.files or k not in b.files:
                diffs.append(f"{FILE}: key {k} only in the {'generator output' if k in b.files else 'committed file'}")
            elif a[k].dtype != b[k].dtype or a[k].shape != b[k].shape or a[k].tobytes() != b[k].tobytes():
                diffs.append(f"{FILE}: {k} differs")
    return diffs


if __name__ == "__main__":
    if "--check" in sys.argv[1:]:
        d = check()
        print("\n".join(d) if d else "fixtures == generator output")
        sys.exit(1 if d else 0)
    p = generate()
    print("wrote", p, os.path.getsize(p), "bytes")
