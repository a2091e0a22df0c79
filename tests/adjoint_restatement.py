"""NumPy restatement of the adjoint-optimisation baseline (reference examples/NavierStokes/NS2Doptimization.py:56-118), batched
over B, and the table of fixture cases of tests/golden/adjoint_ns.npz.  The yardstick of tests/test_gpu_adjoint.py and the
arithmetic of the backend double in tests/fake_adjoint_backend.py; tests/test_adjoint.py pins it to the fixtures, which
tests/golden/make_golden_adjoint.py writes by driving the reference's own functions through the script's loop.

Forward steps and the pressure solve are the oracle's (oracle/pde_oracle.py, pinned to the reference by tests/test_oracle_golden.py);
the backward loop is written out here with every operand in the script's order."""
import numpy as np

from oracle import pde_oracle as po

BC = {"upper": ["Controllable", "Dirchilet"], "lower": ["Dirchilet", "Dirchilet"], "left": ["Dirchilet", "Dirchilet"],
      "right": ["Dirchilet", "Dirchilet"]}

# name: ny, nx, K, T, and what differs from dt = 1e-3, nu = 0.1, density = 1, dy = dx = 1/(n-1), a_nom = 2, ratio = 0.1/0.1, width = 5
CASES = {
    "n21_K2_T6": dict(n=21, K=2, T=6, seed=1),
    "n21_K50_T12": dict(n=21, K=50, T=12, seed=2),
    "n8_K3_T5": dict(n=8, K=3, T=5, seed=3),
    "n11_K7_T9": dict(n=11, K=7, T=9, seed=4),
    "n32_K5_T4": dict(n=32, K=5, T=4, seed=5),
    "n8_K0_T3": dict(n=8, K=0, T=3, seed=6),                      # no sweep: the pressure stays zero
    "n8_K1_T3": dict(n=8, K=1, T=3, seed=7),                      # the first sweep alone (walls as given)
    "n8_K3_T1": dict(n=8, K=3, T=1, seed=8),                      # no backward step: actions = a_nom
    "n8_dy2dx_K3_T3": dict(n=8, K=3, T=3, seed=9, Y=2.0),         # dy = 2 dx
    "n8_rho2_K3_T3": dict(n=8, K=3, T=3, seed=10, density=2.0),
    # the generator marches with the environment's viscosity, as the kernel does; the script's literal 0.1 would differ
    "n8_nu005_env_viscosity_not_script_literal_K3_T3": dict(n=8, K=3, T=3, seed=11, viscosity=0.05),
    "shipped_n21_K2000_T199": dict(n=21, K=2000, T=199, seed=12, sums_only=True),
}
# the reference cannot run nx != ny: pinned to this module alone
RESTATEMENT_ONLY = {"r8x64_K3_T3": dict(n=8, nx=64, K=3, T=3, seed=13, dt=2e-4)}


def case_params(c):
    """Constructor parameters of a case (the reference's and NSBatch2D's names)."""
    ny, nx, T = c["n"], c.get("nx", c["n"]), c["T"]
    X, Y, dt = 1.0, c.get("Y", 1.0), c.get("dt", 1e-3)
    return dict(T=(T + 1) * dt, dt=dt, X=X, dx=X / (nx - 1), Y=Y, dy=Y / (ny - 1), viscosity=c.get("viscosity", 0.1),
                density=c.get("density", 1.0), maximum_pressure_iteration=c["K"])


def case_inputs(c):
    """Initial fields, first commands and targets of a case from its seed: targets in integer sixteenths, everything else
    uniform doubles.  Fields are [ny, nx]."""
    ny, nx, T = c["n"], c.get("nx", c["n"]), c["T"]
    rng = np.random.default_rng(1000 + c["seed"])
    u0, v0, p0 = (rng.uniform(-1, 1, (ny, nx)) for _ in range(3))
    actions0 = rng.uniform(2, 4, T)                                  # NS2Doptimization.py:74
    U_ref = rng.integers(-32, 33, (T + 1, ny, nx, 2)).astype(np.float64) / 16
    return dict(u0=u0, v0=v0, p0=p0, actions0=actions0, U_ref=U_ref)


def oracle_for(prm, U_ref, gamma=0.1, a_nom=2.0):
    return po.NavierStokesOracle(boundary_condition=BC, U_ref=U_ref, action_ref=a_nom * np.ones(U_ref.shape[0] + 1), gamma=gamma, **prm)


def forward(orc, u0, v0, p0, actions):
    """reset + T steps (:71-77, :109-115).  u0, v0, p0 [B, ny, nx]; actions [T, B].  Returns obs [T+1, B, ny, nx, 2], rewards [T, B]."""
    obs = [orc.reset(u0, v0, p0)]
    rewards = []
    for a in actions:
        o, r, _, _ = orc.step(a)
        obs.append(o)
        rewards.append(r)
    return np.stack(obs), np.stack(rewards)


def zero_walls(a1, a2):
    """apply_boundary of the script (:56-61)."""
    for a in (a1, a2):
        a[..., :, [-1, 0]] = 0.
        a[..., [-1, 0], :] = 0.
    return a1, a2


def march(orc, obs, U_ref, a_nom, ratio=0.1 / 0.1, width=5.0, t0=0, reset_pressure=False, target_shift=0):
    """:83-107 for obs [T+1, B, ny, nx, 2] (slot s = the state at time index t0 + s).  Returns lam [T, B, ny, nx, 2] (Lam1[::-1]
    and Lam2 in the same order), grad [T, B], actions [T, B].  reset_pressure / target_shift: deliberate mistakes, for the test
    that shows the fixtures notice them."""
    cd, lap = po.central_difference, po.laplace
    dx, dy, dt, nu = orc.dx, orc.dy, orc.dt, orc.nu
    T, B = obs.shape[0] - 1, obs.shape[1]
    lam1, lam2 = np.zeros(obs.shape[1:4]), np.zeros(obs.shape[1:4])
    pressure = np.zeros(obs.shape[1:4])
    Lam1, Lam2 = [lam1], [lam2]
    for k in range(T - 1):
        s = T - k
        U, V = obs[s, ..., 0], obs[s, ..., 1]
        tgt = U_ref[min(max(t0 + s + target_shift, 0), U_ref.shape[0] - 1)]
        dl1dx, dl1dy = cd(lam1, "x", dx), cd(lam1, "y", dy)
        dl2dx, dl2dy = cd(lam2, "x", dx), cd(lam2, "y", dy)
        lap1, lap2 = lap(lam1, dx, dy), lap(lam2, dx, dy)
        d1 = - 2 * dl1dx * U - dl1dy * V - dl2dx * V - nu * lap1 + (U - tgt[..., 0])
        d2 = - 2 * dl2dy * V - dl1dy * U - dl2dx * U - nu * lap2 + (V - tgt[..., 1])
        lam1 = lam1 - dt * d1
        lam2 = lam2 - dt * d2
        lam1, lam2 = zero_walls(lam1, lam2)
        if reset_pressure:
            pressure = np.zeros_like(pressure)
        pressure = orc.solve_pressure(lam1, lam2, pressure)
        lam1 = lam1 - dt * cd(pressure, "x", dx)
        lam2 = lam2 - dt * cd(pressure, "y", dy)
        lam1, lam2 = zero_walls(lam1, lam2)
        Lam1.append(lam1)
        Lam2.append(lam2)
    Lam1, Lam2 = Lam1[::-1], Lam2[::-1]
    a_nom = np.broadcast_to(np.asarray(a_nom, dtype=np.float64), (T,))
    grad, actions = np.zeros((T, B)), np.zeros((T, B))
    for t in range(T):
        d = cd(Lam1[t], "y", dy)[:, -2, :]
        ssum = 0
        for j in range(d.shape[1]):          # Python's sum (:107): left to right from 0
            ssum = ssum + d[:, j]
        grad[t] = ssum
        actions[t] = a_nom[t] - ratio * ssum * width * dx
    return np.stack([np.stack(Lam1), np.stack(Lam2)], axis=-1), grad, actions


def run_case(c, B=1):
    """The script's flow on the restatement for a case's inputs repeated B times: a dict with the arrays the fixture stores."""
    prm, inp = case_params(c), case_inputs(c)
    orc = oracle_for(prm, inp["U_ref"])
    rep = lambda a: np.repeat(a[None], B, axis=0)
    a0 = np.repeat(inp["actions0"][:, None], B, axis=1)
    obs, rew0 = forward(orc, rep(inp["u0"]), rep(inp["v0"]), rep(inp["p0"]), a0)
    lam, grad, actions = march(orc, obs, inp["U_ref"], 2.0)
    obs2, rew1 = forward(orc, rep(inp["u0"]), rep(inp["v0"]), rep(inp["p0"]), actions)
    return dict(obs=obs, rewards0=rew0, lam=lam, grad=grad, actions=actions, rewards=rew1, obs_replay=obs2)


def load_fixture():
    """tests/golden/adjoint_ns.npz as {case: {array: value}}; the restatement-only cases keep their ``restatement_only/`` prefix."""
    import os
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "adjoint_ns.npz"), allow_pickle=False)
    out = {}
    for k in z.files:
        case, arr = k.rsplit("/", 1)
        out.setdefault(case, {})[arr] = z[k]
    return out


def case_of(name):
    return RESTATEMENT_ONLY[name.split("/", 1)[1]] if name.startswith("restatement_only/") else CASES[name]
