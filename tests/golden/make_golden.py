#!/usr/bin/env python3
"""Generate the golden input/output vectors under tests/golden/ by running the REFERENCE's own
NumPy code (lukebhan/PDEControlGym checkout at /root/reference) in the build container.

Only inputs and expected outputs are stored (small .npz files); no reference source, bytecode or
pickles.  The reference cannot be imported as shipped (SyntaxError in pde_control_gym/__init__.py,
and gymnasium is not installed) so a metadata-only shim is used: it supplies ``gymnasium.Env``,
``spaces.Box`` and ``register`` as no-ops and mounts the reference's package directory under a
synthetic parent so the broken ``__init__`` is skipped.  The shim contains no arithmetic: every
number written below is produced by the reference's own step()/reset()/reward() code.

Run:  python tests/golden/make_golden.py      (needs /root/reference; NOT run on the GPU box)
"""
import importlib
import math
import os
import sys
import types
import warnings

import numpy as np

REF = os.environ.get("PDEGYM_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:          # `python tests/golden/make_golden.py` from anywhere: tests.cases must be importable
    sys.path.insert(0, ROOT)
warnings.filterwarnings("ignore", category=DeprecationWarning)


def import_reference():
    import matplotlib
    matplotlib.use("Agg")
    gym = types.ModuleType("gymnasium")

    class Env:
        def __init__(self):
            pass

        @property
        def unwrapped(self):
            return self

    class Wrapper(Env):
        def __init__(self, env):
            self.env = env

        @property
        def unwrapped(self):
            return self.env.unwrapped

    class Box:
        def __init__(self, low, high, shape=None, dtype=np.float32):
            self.low = np.broadcast_to(np.asarray(low, dtype=dtype), shape) if shape is not None else np.asarray(low, dtype=dtype)
            self.high = np.broadcast_to(np.asarray(high, dtype=dtype), shape) if shape is not None else np.asarray(high, dtype=dtype)
            self.shape, self.dtype = self.low.shape, np.dtype(dtype)

    gym.Env, gym.Wrapper = Env, Wrapper
    spaces = types.ModuleType("gymnasium.spaces")
    spaces.Box = Box
    gym.spaces = spaces
    envs = types.ModuleType("gymnasium.envs")
    reg = types.ModuleType("gymnasium.envs.registration")
    reg.register = lambda **k: None
    envs.registration = reg
    gym.envs = envs
    sys.modules.update({"gymnasium": gym, "gymnasium.spaces": spaces,
                        "gymnasium.envs": envs, "gymnasium.envs.registration": reg})
    pkg = types.ModuleType("pde_control_gym")
    pkg.__path__ = [os.path.join(REF, "pde_control_gym")]
    sys.modules["pde_control_gym"] = pkg
    sys.dont_write_bytecode = True
    return importlib.import_module("pde_control_gym.src")


def cheb_beta(x, gamma, amp):
    beta = np.zeros(len(x), dtype=np.float32)
    for idx, val in enumerate(x):
        beta[idx] = amp * math.cos(gamma * math.acos(val))
    return beta


def _as_control(a, action_as):
    """The Python object handed to the reference's step(): what decides NumPy's promotion of control_update/normalize."""
    if action_as == "f32arr":
        return np.array([a], dtype=np.float32)       # what SB3 passes
    if action_as == "npf64":
        return np.float64(a)                         # e.g. a backstepping controller's dot product
    if action_as == "pyfloat":
        return float(a)
    if action_as == "pyint":
        return int(a)
    raise ValueError(action_as)


def run_1d(src, cls_name, kw, init, beta, actions, reward_args, extra=None, action_as="f32arr"):
    """Drive one reference 1D env (by default with float32 (1,) actions like SB3 does); record everything."""
    cls = getattr(src, cls_name)
    kw = dict(kw)
    kw["reward_class"] = src.TunedReward1D(*reward_args)
    kw["sensing_noise_func"] = lambda s: s
    kw["reset_init_condition_func"] = lambda nx: init
    kw["reset_recirculation_func"] = lambda nx: beta
    env = cls(**kw)
    obs0, _ = env.reset()
    obs, rew, term, trunc, tidx, rows = [np.array(obs0, dtype=np.float32)], [], [], [], [], []
    for a in actions:
        o, r, te, tr, _ = env.step(_as_control(a, action_as))
        obs.append(np.array(o, dtype=np.float32).reshape(-1))
        rew.append(np.float64(r))
        term.append(te)
        trunc.append(tr)
        tidx.append(env.time_index)
        rows.append(np.array(env.u[env.time_index], dtype=np.float32))
    obs[0] = obs[0].reshape(-1)
    return dict(obs=np.stack(obs), reward=np.array(rew), terminate=np.array(term), truncate=np.array(trunc),
                time_index=np.array(tidx), rows=np.stack(rows), init=np.asarray(init), beta=np.asarray(beta),
                actions=np.asarray(actions, dtype=np.float32 if action_as == "f32arr" else np.float64),
                reward_args=np.array(reward_args, dtype=np.float64), action_as=np.array(action_as))


def pack(prefix, d, store):
    for k, v in d.items():
        store[f"{prefix}/{k}"] = v


def gen_transport(src, out=HERE):
    store = {}
    rng = np.random.default_rng(1234)
    # F-H1: BASELINE config 1 (nx=100, T=1, dt=1e-4, S=1000)
    base = dict(T=1, dt=1e-4, X=1, dx=1e-2, normalize=False, sensing_loc="full", control_type="Dirchilet",
                sensing_type=None, limit_pde_state_size=True, max_state_value=1e10, max_control_value=20,
                control_sample_rate=0.1)
    nx = 100
    beta = cheb_beta(np.linspace(0, 1, nx), 7.35, 5)
    acts = rng.uniform(-1, 1, 10).astype(np.float32)
    pack("H1", run_1d(src, "TransportPDE1D", base, np.ones(nx) * 5.0, beta, acts, (10000, -1e3, 3e2)), store)
    # F-H2: Neumann + normalize, every sensing mode
    for name, (ct, sl, st) in {
        "neu_full": ("Neumann", "full", None), "neu_col": ("Neumann", "collocated", None),
        "neu_opp_neu": ("Neumann", "opposite", "Neumann"), "neu_opp_dir": ("Neumann", "opposite", "Dirchilet"),
        "dir_col": ("Dirchilet", "collocated", None), "dir_opp_neu": ("Dirchilet", "opposite", "Neumann"),
        "dir_opp_dir": ("Dirchilet", "opposite", "Dirchilet"),
    }.items():
        kw = dict(base, T=0.3, control_type=ct, sensing_loc=sl, sensing_type=st, normalize=True, control_sample_rate=0.05)
        acts = rng.uniform(-1, 1, 6).astype(np.float32)
        pack(f"H2_{name}", run_1d(src, "TransportPDE1D", kw, np.ones(nx) * 3.0, beta, acts, (3000, -1e3, 3e2)), store)
    # F-H3: BASELINE config 3 shape (nx=512, dt=0.5dx, S=100), smooth random IC / beta
    nx = 512
    dx = 1.0 / 512
    dt = 0.5 * dx
    x = np.linspace(0, 1, nx)
    init = (2.0 + np.sin(2 * np.pi * x * rng.uniform(0.5, 2)) * rng.uniform(0.5, 3)).astype(np.float32)
    beta = cheb_beta(x, rng.uniform(7, 7.7), 5)
    kw = dict(base, T=700 * dt, dt=dt, dx=dx, control_sample_rate=100 * dt)
    acts = rng.uniform(-1, 1, 8).astype(np.float32)     # 7 steps reach nt-1, the 8th is a post-terminal call
    pack("H3", run_1d(src, "TransportPDE1D", kw, init, beta, acts, (700, -1e3, 3e2)), store)
    # F-R: reward edge cases. (a) S=30 (<100: look-back wraps into zero rows, then hits non-step-end rows),
    # clipped last step, terminate with ||u|| >= 20; (b) truncation through a small max_state_value
    nx = 100
    beta = cheb_beta(np.linspace(0, 1, nx), 7.35, 5)
    kw = dict(base, T=0.0400, dt=1e-4, control_sample_rate=30e-4)     # nt=401, S=30 -> 14 steps, last has 10 sub-steps
    acts = rng.uniform(-1, 1, 15).astype(np.float32)
    pack("R_s30", run_1d(src, "TransportPDE1D", kw, np.ones(nx) * 8.0, beta, acts, (400, -1e3, 3e2)), store)
    kw = dict(base, T=0.0400, dt=1e-4, control_sample_rate=30e-4)
    pack("R_s30_small", run_1d(src, "TransportPDE1D", kw, np.ones(nx) * 0.5, beta, acts, (400, -1e3, 3e2)), store)
    kw = dict(base, T=1, max_state_value=46.5)     # ||u|| = 46.08, 46.96 -> truncates at step 2 (and 46.38 < 46.5 at step 3)
    acts = (np.ones(10) * 0.9).astype(np.float32)
    pack("R_trunc", run_1d(src, "TransportPDE1D", kw, np.ones(nx) * 5.0, beta, acts, (10000, -1e3, 3e2)), store)
    # tiny horizon: nt <= 100, negative look-back index wraps onto rows that HAVE been written
    # (the reference raises IndexError when t-100 < -nt, so S must be >= 100-nt+1)
    kw = dict(base, T=0.0090, dt=1e-4, control_sample_rate=15e-4)      # nt=91, S=15: t-100 -> rows 6,21,36,...
    acts = rng.uniform(-1, 1, 6).astype(np.float32)
    pack("R_tiny", run_1d(src, "TransportPDE1D", kw, np.ones(nx) * 2.0, beta, acts, (90, -1e3, 3e2)), store)
    np.savez_compressed(os.path.join(out, "transport.npz"), **store)


def gen_parabolic(src, out=HERE):
    store = {}
    rng = np.random.default_rng(4321)
    base = dict(T=1, dt=1e-5, X=1, dx=5e-3, normalize=False, sensing_loc="full", control_type="Dirchilet",
                sensing_type=None, limit_pde_state_size=True, max_state_value=1e10, max_control_value=20,
                control_sample_rate=1e-3)
    # F-P1: shipped example config (nx=200, S=100), 20 steps
    nx = 200
    beta = cheb_beta(np.linspace(0, 1, nx + 1), 8, 50)
    acts = rng.uniform(-1, 1, 20).astype(np.float32)
    pack("P1", run_1d(src, "ReactionDiffusionPDE1D", base, np.ones(nx + 1) * 4.0, beta, acts, (100000, -1e3, 3e2)), store)
    # F-P2: BASELINE config 2 shape (nx=256, F=0.25), S in {1, 100}; Dirichlet and Neumann+normalize
    nx = 256
    dx = 1.0 / 256
    dt = 0.25 * dx * dx
    x = np.linspace(0, 1, nx + 1)
    beta = cheb_beta(x, 8.2, 50)
    init = (np.ones(nx + 1) * 6.5).astype(np.float32)
    for name, S, ct, norm, nsteps, T in [("P2_s100", 100, "Dirchilet", False, 12, 1000 * dt),
                                         ("P2_s1", 1, "Dirchilet", False, 12, 1000 * dt),
                                         ("P2_s100_neu", 100, "Neumann", False, 8, 1000 * dt),
                                         ("P2_s1_neu", 1, "Neumann", False, 150, 1000 * dt),
                                         # normalize also scales the Neumann neighbour (x20 per sub-step): keep it short
                                         ("P2_s1_neu_norm", 1, "Neumann", True, 6, 1000 * dt),
                                         ("P2_s100_dir_norm", 100, "Dirchilet", True, 6, 1000 * dt)]:
        kw = dict(base, T=T, dt=dt, dx=dx, control_sample_rate=S * dt, control_type=ct, normalize=norm)
        acts = rng.uniform(-1, 1, nsteps).astype(np.float32)
        pack(name, run_1d(src, "ReactionDiffusionPDE1D", kw, init, beta, acts, (1000, -1e3, 3e2)), store)
    # sensing variants
    for name, (ct, sl, st) in {"col_neu": ("Neumann", "collocated", None), "col_dir": ("Dirchilet", "collocated", None),
                               "opp_neu": ("Dirchilet", "opposite", "Neumann")}.items():
        kw = dict(base, T=600 * dt, dt=dt, dx=dx, control_sample_rate=50 * dt, control_type=ct, sensing_loc=sl, sensing_type=st)
        acts = rng.uniform(-1, 1, 5).astype(np.float32)
        pack(f"P3_{name}", run_1d(src, "ReactionDiffusionPDE1D", kw, init, beta, acts, (600, -1e3, 3e2)), store)
    np.savez_compressed(os.path.join(out, "parabolic.npz"), **store)


def gen_kat(src, out=HERE):
    """Published known answers (backstepping episodes, notebook stored outputs)."""
    store = {}
    # transport: examples/transportPDE/transport1Dbackstepping.py:22-36,48-99
    T, dt, dx, X = 5, 1e-4, 1e-2, 1
    nx = 100

    def kernel_transport(theta):
        kappa = np.zeros(len(theta))
        for i in range(len(theta)):
            s = 0
            for j in range(i):
                s += (kappa[i - j] * theta[j]) * dx
            kappa[i] = s - theta[i]
        return np.flip(kappa)

    beta = cheb_beta(np.linspace(0, 1, nx), 7.35, 5)
    kern = kernel_transport(cheb_beta(np.linspace(dx, X, nx), 7.35, 5))
    for u0 in (1, 10):
        kw = dict(T=T, dt=dt, X=X, dx=dx, reward_class=src.TunedReward1D(int(round(T / dt)), -1e3, 3e2), normalize=False,
                  sensing_loc="full", control_type="Dirchilet", sensing_type=None, sensing_noise_func=lambda s: s,
                  limit_pde_state_size=True, max_state_value=1e10, max_control_value=20,
                  reset_init_condition_func=lambda n, u0=u0: np.ones(n) * u0, reset_recirculation_func=lambda n: beta,
                  control_sample_rate=0.1)
        env = src.TransportPDE1D(**kw)
        obs, _ = env.reset()
        te = tr = False
        total, l2, acts, rews = 0.0, 0.0, [], []
        while not te and not tr:
            a = 0
            for i in range(len(obs)):
                a += kern[i] * obs[i]
            a = a * 1e-2
            obs, r, te, tr, _ = env.step(a)
            total += r
            l2 += np.linalg.norm(obs)
            acts.append(a)
            rews.append(r)
        pack(f"T_u{u0}", dict(total=np.float64(total), sum_l2=np.float64(l2), actions=np.array(acts, dtype=np.float64),
                              rewards=np.array(rews, dtype=np.float64), kernel=kern, beta=beta, last_obs=np.array(obs)), store)
        print("KAT transport", u0, total, l2)

    # parabolic: examples/reactionDiffusionPDE/reactionDiffusion1DBackstepping.py:22-39,51-102
    T, dt, dx, X = 1, 1e-5, 5e-3, 1
    nx = 200

    def kernel_parabolic(a):
        k = np.zeros((len(a), len(a)))
        k[1][1] = -(a[1] + a[0]) * dx / 4
        for i in range(1, len(a) - 1):
            k[i + 1][0] = 0
            k[i + 1][i + 1] = k[i][i] - dx / 4.0 * (a[i - 1] + a[i])
            k[i + 1][i] = k[i][i] - dx / 2 * a[i]
            for j in range(1, i):
                k[i + 1][j] = -k[i - 1][j] + k[i][j + 1] + k[i][j - 1] + a[j] * (dx ** 2) * (k[i][j + 1] + k[i][j - 1]) / 2
        return k

    beta = cheb_beta(np.linspace(0, 1, nx + 1), 8, 50)
    kern = kernel_parabolic(cheb_beta(np.linspace(dx, X, nx), 8, 50))   # notebook cell 11 grid
    for u0 in (1, 10):
        kw = dict(T=T, dt=dt, X=X, dx=dx, reward_class=src.TunedReward1D(int(round(T / dt)), -1e3, 3e2), normalize=False,
                  sensing_loc="full", control_type="Dirchilet", sensing_type=None, sensing_noise_func=lambda s: s,
                  limit_pde_state_size=True, max_state_value=1e10, max_control_value=20,
                  reset_init_condition_func=lambda n, u0=u0: np.ones(n + 1) * u0, reset_recirculation_func=lambda n: beta,
                  control_sample_rate=0.001)
        env = src.ReactionDiffusionPDE1D(**kw)
        obs, _ = env.reset()
        te = tr = False
        total, l2, acts, rews = 0.0, 0.0, [], []
        krow = kern[-1]
        while not te and not tr:
            m = min(len(krow), len(obs) - 1)
            a = sum(krow[0:m] * obs[0:m]) * dx
            obs, r, te, tr, _ = env.step(a)
            total += r
            l2 += np.linalg.norm(obs)
            acts.append(a)
            rews.append(r)
        pack(f"P_u{u0}", dict(total=np.float64(total), sum_l2=np.float64(l2), actions=np.array(acts, dtype=np.float64),
                              rewards=np.array(rews, dtype=np.float64), kernel_row=krow, beta=beta, last_obs=np.array(obs)), store)
        print("KAT parabolic", u0, total, l2)
    np.savez_compressed(os.path.join(out, "kat.npz"), **store)


def gen_mixed(src, out=HERE):
    """float64 plant parameter and/or float64 / Python-scalar control inputs: NumPy then evaluates parts of the update in
    double and rounds once when the row is stored (hyperbolic.py:146-155, parabolic.py:143-150).  Case table: tests/cases.py
    MIXED_CASES (kwargs) -- here only the data."""
    from tests.cases import MIXED_CASES
    store = {}
    rng = np.random.default_rng(8642)
    for name, (kind, kw, action_as, beta_kind, nsteps) in MIXED_CASES.items():
        nx = int(round(kw["X"] / kw["dx"]))
        n = nx + (1 if kind == "parabolic" else 0)
        x = np.linspace(0, 1, n)
        if beta_kind == "ones64":            # docs/source/guide/quickstart.rst:27-28
            beta = np.ones(n)
        elif beta_kind == "cos64":           # an un-cast NumPy expression is float64
            beta = (50 if kind == "parabolic" else 5) * np.cos(rng.uniform(7, 8.5) * np.arccos(x))
        elif beta_kind == "int":
            beta = np.arange(n) % 3
        else:                                # "cos32": the examples' float32 beta (only the control input is float64)
            beta = cheb_beta(x, 7.35 if kind == "transport" else 8.0, 5 if kind == "transport" else 50)
        init = np.ones(n) * rng.uniform(1, 10) if name.startswith("Q_quick") else \
            (rng.uniform(1, 10) * (1 + 0.3 * np.sin(2 * np.pi * x * rng.uniform(0.5, 3))))
        if action_as == "pyint":
            acts = np.zeros(nsteps)          # quickstart.rst:68: env.step(0)
        else:
            acts = rng.uniform(-1, 1, nsteps)
        nt1 = int(round(kw["T"] / kw["dt"]))
        cls = "ReactionDiffusionPDE1D" if kind == "parabolic" else "TransportPDE1D"
        with np.errstate(all="ignore"):
            pack(name, run_1d(src, cls, kw, init, beta, acts, (nt1, -1e-4, 1e2) if name.startswith("Q_quick") else (nt1, -1e3, 3e2),
                              action_as=action_as), store)
    np.savez_compressed(os.path.join(out, "mixed.npz"), **store)


NS_BC = {"upper": ["Controllable", "Dirchilet"], "lower": ["Dirchilet", "Dirchilet"],
         "left": ["Dirchilet", "Dirchilet"], "right": ["Dirchilet", "Dirchilet"]}


def gen_ns(src, out=HERE):
    store = {}
    # F-N1: the reference's own golden trajectory examples/NavierStokes/target.npz (NS2Dppo.py:21-50)
    tgt = np.load(os.path.join(REF, "examples/NavierStokes/target.npz"))
    ut, vt = tgt["u"], tgt["v"]
    Uref = np.stack([ut, vt], axis=-1)
    kw = dict(T=0.2, dt=1e-3, X=1, dx=0.05, Y=1, dy=0.05, action_dim=1, reward_class=src.NSReward(0.1), normalize=False,
              reset_init_condition_func=lambda X: (ut[0].copy(), vt[0].copy(), np.zeros_like(ut[0])),
              boundary_condition=NS_BC, U_ref=Uref, action_ref=2.0 * np.ones(1000))
    env = src.NavierStokes2D(**kw)
    env.reset()
    rews, frames = [], {}
    keep = [0, 1, 2, 50, 120, 199]
    acts = ut[1:200, -1, 10].copy()          # = 4 - 0.01 t up to rounding; the stored values are the exact inputs
    for t in range(1, 200):
        obs, r, te, tr, _ = env.step(acts[t - 1])
        rews.append(r)
    U = env.U
    assert np.array_equal(U[:200, :, :, 0], ut) and np.array_equal(U[:200, :, :, 1], vt), "reference no longer reproduces target.npz"
    for t in keep:
        frames[f"u{t}"] = ut[t]
        frames[f"v{t}"] = vt[t]
    pack("N1", dict(rewards=np.array(rews), p_final=env.p, keep=np.array(keep), actions=acts, **frames), store)
    # a different reference trajectory so the reward is non-trivial
    env2 = src.NavierStokes2D(**dict(kw, U_ref=0.5 * Uref))
    env2.reset()
    rews2 = [env2.step(acts[t - 1])[1] for t in range(1, 6)]
    pack("N1b", dict(rewards=np.array(rews2)), store)

    # F-N2: mixed boundary conditions, random smooth IC, K=50
    rng = np.random.default_rng(99)
    for name, n, bc in [("N2_32", 32, {"upper": ["Controllable", "Neumann"], "lower": ["Dirchilet", "Controllable"],
                                          "left": ["Neumann", "Dirchilet"], "right": ["Dirchilet", "Neumann"]}),
                        ("N2_64", 64, {"upper": ["Neumann", "Neumann"], "lower": ["Controllable", "Dirchilet"],
                                          "left": ["Controllable", "Controllable"], "right": ["Neumann", "Dirchilet"]}),
                        ("N2_48", 48, NS_BC)]:
        dx = 1.0 / (n - 1)
        dt = 0.2 * 0.5 * dx * dx / 0.1
        xs = np.linspace(0, 1, n)
        Xg, Yg = np.meshgrid(xs, xs)
        u0 = np.sin(2 * np.pi * Xg) * np.cos(np.pi * Yg) * rng.uniform(0.5, 2) + rng.uniform(-1, 1)
        v0 = np.cos(np.pi * Xg) * np.sin(2 * np.pi * Yg) * rng.uniform(0.5, 2) + rng.uniform(-1, 1)
        p0 = rng.uniform(-1, 1, (n, n))
        nt = 10
        Uref = rng.uniform(-1, 1, (nt, n, n, 2))
        aref = rng.uniform(1, 3, nt)
        kw = dict(T=nt * dt, dt=dt, X=1, dx=dx, Y=1, dy=dx, action_dim=1, reward_class=src.NSReward(0.1), normalize=False,
                  reset_init_condition_func=lambda X: (u0.copy(), v0.copy(), p0.copy()), boundary_condition=bc,
                  U_ref=Uref, action_ref=aref, maximum_pressure_iteration=50)
        env = src.NavierStokes2D(**kw)
        assert env.nx == n
        env.reset()
        acts = rng.uniform(2, 4, 3)
        obs_l, p_l, r_l = [], [], []
        for a in acts:
            obs, r, te, tr, _ = env.step(a)
            obs_l.append(np.array(obs))
            p_l.append(np.array(env.p))
            r_l.append(r)
        pack(name, dict(u0=u0, v0=v0, p0=p0, U_ref=Uref, action_ref=aref, actions=acts, obs=np.stack(obs_l), p=np.stack(p_l),
                        rewards=np.array(r_l), dx=np.float64(dx), dt=np.float64(dt), nt=np.int64(nt),
                        bc=np.array([bc[k][i] for k in ("upper", "lower", "left", "right") for i in (0, 1)])), store)

    # F-N3: BASELINE config 4 shape (128x128, K=50): checksums + sampled points only
    n = 128
    dx = 1.0 / (n - 1)
    dt = 0.2 * 0.5 * dx * dx / 0.1
    cu, cv, cp = 1.7, -2.3, 0.4
    nt = 10
    kw = dict(T=nt * dt, dt=dt, X=1, dx=dx, Y=1, dy=dx, action_dim=1, reward_class=src.NSReward(0.1), normalize=False,
              reset_init_condition_func=lambda X: (cu * np.ones_like(X), cv * np.ones_like(X), cp * np.ones_like(X)),
              boundary_condition=NS_BC, U_ref=np.zeros((nt, n, n, 2)), action_ref=2.0 * np.ones(nt), maximum_pressure_iteration=50)
    env = src.NavierStokes2D(**kw)
    env.reset()
    pts = rng.integers(0, n, (16, 2))
    acts = np.array([3.1, 2.4])
    sums, samples, rews = [], [], []
    for a in acts:
        obs, r, te, tr, _ = env.step(a)
        sums.append([np.linalg.norm(obs[..., 0]), np.linalg.norm(obs[..., 1]), np.linalg.norm(env.p),
                     obs.min(), obs.max(), env.p.min(), env.p.max()])
        samples.append(np.stack([obs[pts[:, 0], pts[:, 1], 0], obs[pts[:, 0], pts[:, 1], 1], env.p[pts[:, 0], pts[:, 1]]], axis=-1))
        rews.append(r)
    pack("N3", dict(ic=np.array([cu, cv, cp]), actions=acts, sums=np.array(sums), pts=pts, samples=np.stack(samples),
                    rewards=np.array(rews), dx=np.float64(dx), dt=np.float64(dt), nt=np.int64(nt)), store)
    np.savez_compressed(os.path.join(out, "ns2d.npz"), **store)


def gen_traffic(src, out=HERE):
    """TrafficPDE1D (environments1d/traffic_arz_env.py) with TrafficARZReward: the shipped notebook configuration
    (examples/TrafficPDE1D/*.ipynb cell 3: T=240, dt=0.25, dx=10, X=500, tau=60, v_max=40, ro_max=0.16)."""
    import contextlib
    import io
    import random
    store = {}
    rng = np.random.default_rng(77)
    for name, sim, cf, nact, nsteps, limit in [("inlet", "inlet", 1, 1, 60, True), ("outlet", "outlet", 1, 1, 60, True),
                                               ("both", "both", 1, 2, 60, True), ("train", "outlet-train", 2, 1, 60, True),
                                               ("outlet_cf3", "outlet", 3, 1, 40, False), ("long", "inlet", 1, 1, 1000, True)]:
        kw = dict(T=240, dt=0.25, X=500, dx=10, reward_class=src.TrafficARZReward(), simulation_type=sim, v_steady=10,
                  ro_steady=0.12, v_max=40, ro_max=0.16, tau=60, limit_pde_state_size=limit, control_freq=cf)
        random.seed(11)
        with contextlib.redirect_stdout(io.StringIO()):
            env = src.TrafficPDE1D(**kw)
            qs_clip = env.qs
            random.seed(13)
            obs0, _ = env.reset()
        acts = rng.uniform(0.7, 1.3, (nsteps, nact)) * env.qs
        obs, rew, done, trunc, tim = [np.array(obs0)], [], [], [], []
        for a in acts:
            with contextlib.redirect_stdout(io.StringIO()):
                o, r, d, t, _ = env.step(a)
            obs.append(np.array(o))
            rew.append(r)
            done.append(bool(d))
            trunc.append(bool(t))
            tim.append(env.time_index)
        obs = np.stack(obs)
        if name == "long":      # keep the file small: every 50th observation
            keep = np.arange(0, nsteps + 1, 50)
            obs = obs[keep]
            store[f"{name}/keep"] = keep
        pack(name, dict(obs=obs, reward=np.array(rew), done=np.array(done), trunc=np.array(trunc), time=np.array(tim),
                        actions=acts, rs=np.float64(env.rs), qs_clip=np.float64(qs_clip), control_freq=np.int64(cf),
                        limit=np.bool_(limit), sim=np.array(sim)), store)
    np.savez_compressed(os.path.join(out, "traffic.npz"), **store)


def tumor_ic(X, nx):
    """examples/BrainTumor1D notebook: 0.8 k exp(-0.25 x^2)."""
    xs = np.linspace(0, X, nx)
    return 0.8 * 1e5 * np.exp(-0.25 * (xs ** 2))


TUMOR_KW = dict(X=200, dt=1, dx=1, normalize=True, dosage_termination_threshold=0.1, t1_detection_threshold=0.8,
                t2_detection_threshold=0.16, D=0.2, rho=0.03, alpha=0.04, alpha_beta_ratio=10, k=1e5,
                t1_detection_radius=15, t1_death_radius=35, total_dosage=61.2, verbose=False)


def gen_tumor(src, out=HERE):
    """BrainTumor1D + BrainTumorReward + TherapyWrapper (environments1d/brain_tumor_env.py, rewards/brain_tumor_reward.py)
    on the shipped notebook configuration (examples/BrainTumor1D: T=600, X=200, dt=dx=1, total_dosage=61.2)."""
    import importlib
    bt = importlib.import_module("pde_control_gym.src.environments1d.brain_tumor_env")
    br = importlib.import_module("pde_control_gym.src.rewards.brain_tumor_reward")
    store = {}
    rng = np.random.default_rng(2024)
    # ---- raw environment episodes: (name, T, t_benchmark, dose range)
    for name, T, tb, hi in [("raw", 600, 300, 0.08), ("toxic", 600, 250, 0.3), ("nobench", 600, None, 0.1),
                            ("term_therapy", 230, 200, 0.004), ("term_post", 300, 200, 0.25)]:
        env = bt.BrainTumor1D(T=T, reward_class=br.BrainTumorReward(), reset_init_condition_func=tumor_ic, **TUMOR_KW)
        env.t_benchmark = tb
        obs0, _ = env.reset()
        acts, rew, term, trunc, stage = [], [], [], [], []
        while True:
            a = float(rng.uniform(0, hi))
            o, r, te, tr, info = env.step(a)
            acts.append(a)
            rew.append(float(r))
            term.append(bool(te))
            trunc.append(bool(tr))
            stage.append({"Growth": 0, "Therapy": 1, "Post-Therapy": 2}[info["stage"]])
            if te or tr:
                break
        n = len(acts)
        keep = np.unique(np.concatenate([np.arange(0, n + 1, 16), [n]]))
        pack(name, dict(T=np.int64(T), t_benchmark=np.float64(np.nan if tb is None else tb), actions=np.array(acts),
                        reward=np.array(rew), term=np.array(term), trunc=np.array(trunc), stage=np.array(stage),
                        keep=keep, rows=env.u[keep].copy(), t1_idx=env.t1_radius_idx_vs_time[: n + 1].copy(),
                        dosage=env.dosage_vs_time[: n + 1].copy(),
                        days=np.array([env.growthDays, env.therapyDays, env.postTherapyDays, env.simulationDays,
                                       -1 if env.cDeathDay is None else env.cDeathDay]),
                        first=np.array([-1 if env.firstTherapyDay is None else env.firstTherapyDay,
                                        -1 if env.firstPostTherapyDay is None else env.firstPostTherapyDay]),
                        remaining=np.float64(env.remaining_dosage)), store)
    # ---- wrapper flows: benchmark(), reset() through the growth stage, constant daily fraction
    for name, weekends, frac in [("wrap_week", True, 2.0 / 61.2), ("wrap_daily", False, 1.8 / 61.2), ("wrap_hypo", True, 0.2)]:
        env = bt.BrainTumor1D(T=600, reward_class=br.BrainTumorReward(), reset_init_condition_func=tumor_ic, **TUMOR_KW)
        w = bt.TherapyWrapper(env, weekends=weekends, verbose=False)
        tb = w.benchmark()
        obs, _ = w.reset()
        rows, rew, term, trunc, tidx = [np.array(obs)], [], [], [], [env.time_index]
        while True:
            o, r, te, tr, info = w.step(frac)
            rows.append(np.array(o))
            rew.append(float(r))
            term.append(bool(te))
            trunc.append(bool(tr))
            tidx.append(env.time_index)
            if te or tr:
                break
        pack(name, dict(weekends=np.bool_(weekends), frac=np.float64(frac), t_benchmark=np.int64(tb), rows=np.stack(rows),
                        reward=np.array(rew), term=np.array(term), trunc=np.array(trunc), time_index=np.array(tidx),
                        days=np.array([env.growthDays, env.therapyDays, env.postTherapyDays, env.simulationDays,
                                       -1 if env.cDeathDay is None else env.cDeathDay]),
                        calls=np.int64(w.treatment_calls), violations=np.int64(w.soft_constraint_violations),
                        dosage=env.dosage_vs_time.copy(), t1_idx=env.t1_radius_idx_vs_time.copy()), store)
    np.savez_compressed(os.path.join(out, "tumor.npz"), **store)


# ---- parameter sweeps: the ranges the differential fuzzers draw (tests/fuzz_*.py), pinned to the reference ------------------
# Every case stores its own constructor parameters next to its data ("<case>/<name>" keys: scalars, strings, the BC name
# array), so the consumers (tests/test_oracle_sweep.py, tests/test_gpu_sweep.py) need no mirrored table.  Cases are small: a
# handful of env-steps on the smallest grid that reaches the code path.  Configurations the reference rejects are recorded
# under "unpinnable/<name>" with the exception class it raises, and the generator asserts that they still raise.
def _scalars(store, prefix, **kw):
    """Constructor parameters as data: numbers as 0-d float64 / int64 / bool arrays, strings (None -> "") as 0-d str arrays."""
    for k, v in kw.items():
        if v is None or isinstance(v, str):
            store[f"{prefix}/{k}"] = np.array("" if v is None else v)
        elif isinstance(v, (bool, np.bool_)):
            store[f"{prefix}/{k}"] = np.bool_(v)
        elif isinstance(v, (int, np.integer)):
            store[f"{prefix}/{k}"] = np.int64(v)
        else:
            store[f"{prefix}/{k}"] = np.float64(v)


def _raises(fn):
    """Name of the exception class fn() raises (the generator fails if it does not raise)."""
    try:
        fn()
    except Exception as e:      # noqa: BLE001 -- the class is the datum
        return type(e).__name__
    raise AssertionError("the reference no longer rejects this configuration")


def _ragged_slots(epl):
    """Row widths of tests/test_gpu_buffer_contract.py (STEP_CASES): a slot count that takes ``epl`` elements per lane, leaves a
    straddling lane and idle lanes.  tests/test_oracle_sweep.py checks that the fixture still covers that module's list."""
    s = 64 * (epl - 1) + 37 if epl > 1 else 37
    return s + 1 if s % epl == 0 else s


SENSING_T = [("Dirchilet", "full", None), ("Neumann", "full", None), ("Dirchilet", "collocated", None), ("Neumann", "collocated", None),
             ("Dirchilet", "opposite", "Neumann"), ("Neumann", "opposite", "Neumann"), ("Dirchilet", "opposite", "Dirchilet"),
             ("Neumann", "opposite", "Dirchilet")]
SENSING_P = SENSING_T[:6]       # parabolic: opposite / Dirchilet raises by design (parabolic.py:85,114)


def gen_sweep_1d(src, out=HERE):
    """TransportPDE1D and ReactionDiffusionPDE1D at one row width per class the step kernels dispatch on (elements per lane 1 ..
    32 with a ragged tail, the whole-wave widths 64 .. 512, one row past the register limit), X in {0.5, 1, 2}, max_control_value
    in {1, 3, 20} with and without normalize, S in {1, 2, 7, 33, 100}, every control / sensing combination the reference accepts,
    a truncating max_state_value, limit_pde_state_size=False, float64 beta / float64 and Python-float controls.  nt >= 120
    throughout (TunedReward1D looks 100 rows back); with S in {33, 100} the sixth step is clipped by the end of the episode."""
    store = {}
    rng = np.random.default_rng(20261)
    widths = [("e%d" % e, _ragged_slots(e)) for e in (1, 2, 3, 4, 5, 6, 8, 12, 16, 24, 32)] + \
             [("full%d" % w, w) for w in (64, 128, 256, 512)] + [("wide", 2049)]
    Ss, Xs, mcvs = [1, 2, 7, 33, 100], [1, 0.5, 2], [20, 1, 3]
    for kind, cls, sens in (("transport", "TransportPDE1D", SENSING_T), ("parabolic", "ReactionDiffusionPDE1D", SENSING_P)):
        ghost = 1 if kind == "parabolic" else 0
        for wi, (wname, slots) in enumerate(widths):
            n = 2049 if wname == "wide" else slots + ghost      # array length; the reference's nx excludes the parabolic ghost node
            nx = n - ghost
            big = n > 256
            ct, sl, st = sens[wi % len(sens)]
            if big and sl == "full":                # the file's size: full observations only with rows of up to 256 nodes
                sl = "collocated"
            S = Ss[(wi + ghost) % len(Ss)]
            X = Xs[(wi + 2 * ghost) % len(Xs)]
            mcv = mcvs[(wi + ghost) % len(mcvs)]
            norm = (wi % 2 == 0)
            if kind == "parabolic" and ct == "Neumann" and norm and S > 7:
                S = 7                               # normalize scales the Neumann neighbour every sub-step: keep the rows finite
            dx = X / nx
            dt = 0.25 * dx * dx if kind == "parabolic" else 0.5 * dx
            nsteps = 7 if (S >= 33 and not big) else 6          # the seventh is a post-terminal call
            nt1 = 5 * S + max(S // 3, 1) if S >= 33 else 120 + S     # nt - 1: S >= 33 clips the sixth step
            kw = dict(T=nt1 * dt, dt=dt, X=X, dx=dx, normalize=norm, sensing_loc=sl, control_type=ct, sensing_type=st,
                      limit_pde_state_size=True, max_state_value=1e10, max_control_value=mcv, control_sample_rate=S * dt)
            x = np.linspace(0, 1, n)
            if big:
                init = (np.ones(n) * rng.uniform(1, 8)).astype(np.float32)
            else:
                init = (rng.uniform(1, 8) * (1 + 0.3 * np.sin(2 * np.pi * x * rng.uniform(0.5, 3)))).astype(np.float32)
            beta = cheb_beta(x, rng.uniform(7, 8.4), 50 if kind == "parabolic" else 5)
            action_as = "f32arr"
            name = f"{kind[0].upper()}_{wname}"
            if wname == "e5":
                kw["limit_pde_state_size"] = False
                kw["max_state_value"] = 1.0         # would truncate at once if the switch were ignored
            acts = rng.uniform(-1, 1, nsteps).astype(np.float32)
            with np.errstate(all="ignore"):
                d = run_1d(src, cls, kw, init, beta, acts, (nt1, -1e3, 3e2), action_as=action_as)
                if wname == "e3":                   # truncation: a max_state_value half way between the smallest and the largest row norm
                    norms = np.array([np.linalg.norm(r) for r in d["rows"]])
                    kw["max_state_value"] = float(0.5 * (norms.min() + norms.max()))
                    d = run_1d(src, cls, kw, init, beta, acts, (nt1, -1e3, 3e2), action_as=action_as)
                    assert d["truncate"].any() and not d["truncate"].all()
            _store_1d(store, name, kind, kw, d, big)
    # float64 beta and float64 / Python-float controls (the kernels' mixed-precision mode) at 1, 2, 4, 8 elements per lane
    for kind, cls, epl, ct, norm, action_as, beta64 in [("parabolic", "ReactionDiffusionPDE1D", 1, "Dirchilet", False, "f32arr", True),
                                                        ("transport", "TransportPDE1D", 2, "Neumann", True, "npf64", False),
                                                        ("parabolic", "ReactionDiffusionPDE1D", 4, "Neumann", False, "pyfloat", True),
                                                        ("transport", "TransportPDE1D", 8, "Dirchilet", True, "npf64", True)]:
        n = _ragged_slots(epl) + 1
        nx = n - (1 if kind == "parabolic" else 0)
        X, S, mcv = Xs[epl % 3], [2, 7, 33][epl % 3], mcvs[epl % 3]
        dx = X / nx
        dt = 0.25 * dx * dx if kind == "parabolic" else 0.5 * dx
        nt1 = 5 * S + S // 3 if S >= 33 else 120 + S
        kw = dict(T=nt1 * dt, dt=dt, X=X, dx=dx, normalize=norm, sensing_loc="full", control_type=ct, sensing_type=None,
                  limit_pde_state_size=True, max_state_value=1e10, max_control_value=mcv, control_sample_rate=S * dt)
        x = np.linspace(0, 1, n)
        init = (rng.uniform(1, 8) * (1 + 0.3 * np.sin(2 * np.pi * x * rng.uniform(0.5, 3)))).astype(np.float32)
        amp = 50 if kind == "parabolic" else 5
        beta = amp * np.cos(rng.uniform(7, 8.4) * np.arccos(x)) if beta64 else cheb_beta(x, 7.7, amp)
        acts = rng.uniform(-1, 1, 6)
        with np.errstate(all="ignore"):
            d = run_1d(src, cls, kw, init, beta, acts, (nt1, -1e3, 3e2), action_as=action_as)
        _store_1d(store, f"M_{kind[0]}_e{epl}", kind, kw, d, False)
    # the reference rejects Dirichlet sensing opposite the actuator of the parabolic plant, whatever the control type
    for ct in ("Dirchilet", "Neumann"):
        kw = dict(T=1e-3, dt=1e-5, X=1, dx=1e-2, normalize=False, sensing_loc="opposite", control_type=ct, sensing_type="Dirchilet",
                  limit_pde_state_size=True, max_state_value=1e10, max_control_value=20, control_sample_rate=1e-4,
                  reward_class=src.TunedReward1D(100, -1e3, 3e2), sensing_noise_func=lambda s: s,
                  reset_init_condition_func=lambda nx: np.ones(nx + 1), reset_recirculation_func=lambda nx: np.ones(nx + 1))
        name = f"unpinnable/parabolic_opposite_dirichlet_{ct.lower()}"
        store[name] = np.array(_raises(lambda: src.ReactionDiffusionPDE1D(**kw)))
        _scalars(store, name + "_kw", control_type=ct, sensing_loc="opposite", sensing_type="Dirchilet")
    np.savez_compressed(os.path.join(out, "sweep_1d.npz"), **store)


def _store_1d(store, name, kind, kw, d, big):
    """One 1D case: constructor parameters, inputs, per-step scalars for every step, rows / observations at the steps in ``keep``
    (every step for rows of up to 256 nodes, the first and the last beyond: the last row carries every earlier one)."""
    nsteps = len(d["actions"])
    keep = np.array([0, nsteps - 1]) if big else np.arange(nsteps)
    d = dict(d)
    d["obs0"] = d["obs"][0]
    d["norm"] = np.array([np.linalg.norm(r) for r in d["rows"]], dtype=np.float64)      # of every step's row (the rewards' scale)
    d["obs"] = d["obs"][keep + 1]
    d["rows"] = d["rows"][keep]
    d["keep"] = keep
    pack(name, d, store)
    _scalars(store, name, kind=kind, **kw)


def gen_sweep_ns(src, out=HERE):
    """NavierStokes2D on square node counts n in {5, 8, 16, 21, 33} with dy != dx (Y in {0.25, 0.5, 1, 2}), density, viscosity, gamma,
    K in {0, 1, 2, 3, 7, 51}, scalar and per-node actions, random boundary sets (every (edge, component, condition) triple occurs),
    zero / constant / random initial fields; three steps each.  The reference cannot run nx != ny (navier_stokes2D.py:148 stores
    an [ny, nx] field into U[t] of shape [nx, ny]): recorded under unpinnable/."""
    store = {}
    rng = np.random.default_rng(20262)
    conds = ["Neumann", "Dirchilet", "Controllable"]
    edges = ("upper", "lower", "left", "right")
    #        n   Y     rho  nu    gamma K   per-node  initial
    table = [(5, 0.25, 0.5, 0.01, 0.0, 0, False, "rand"), (5, 1.0, 2.0, 1.0, 2.0, 3, True, "const"), (5, 2.0, 1.0, 0.1, 0.1, 51, False, "zero"),
             (8, 0.5, 2.0, 0.1, 2.0, 1, True, "rand"), (8, 2.0, 0.5, 1.0, 0.1, 7, False, "rand"), (8, 1.0, 1.0, 0.01, 0.0, 2, False, "const"),
             (8, 0.25, 1.0, 0.1, 0.1, 51, True, "zero"),
             (16, 0.25, 2.0, 0.01, 0.1, 3, False, "rand"), (16, 2.0, 0.5, 0.1, 0.0, 7, True, "rand"), (16, 0.5, 1.0, 1.0, 2.0, 0, False, "const"),
             (16, 1.0, 0.5, 0.01, 2.0, 51, True, "rand"),
             (21, 0.5, 0.5, 0.1, 0.1, 2, True, "rand"), (21, 2.0, 2.0, 0.01, 2.0, 7, False, "rand"), (21, 1.0, 1.0, 1.0, 0.0, 51, False, "zero"),
             (33, 0.5, 2.0, 1.0, 0.1, 7, True, "rand"), (33, 2.0, 0.5, 0.01, 2.0, 51, False, "rand")]
    seen = set()
    for ci, (n, Y, rho, nu, gamma, K, per_node, ic) in enumerate(table):
        # boundary sets: cycle the conditions so that all 24 (edge, component, condition) triples occur, then perturb at random
        bc = {e: [conds[(ci + ei + c) % 3] if ci < 3 else str(rng.choice(conds)) for c in (0, 1)] for ei, e in enumerate(edges)}
        if ci < 3:
            bc = {e: [conds[(ci + ei) % 3], conds[(ci + ei + 1 + (ei % 2)) % 3]] for ei, e in enumerate(edges)}
        for e in edges:
            for c in (0, 1):
                seen.add((e, c, bc[e][c]))
        dx, dy = 1.0 / (n - 1), Y / (n - 1)
        dt = 0.2 * 0.5 * min(dx, dy) ** 2 / nu
        nt = 4
        adim = n if per_node else 1

        def field():
            if ic == "zero":
                return np.zeros((n, n))
            if ic == "const":
                return np.full((n, n), rng.uniform(-3, 3))
            return rng.uniform(-1, 1, (n, n))
        u0, v0, p0 = field(), field(), field()
        Uref = rng.integers(-16, 17, (nt, n, n, 2)) / 16.0          # sixteenths: compresses well, still a non-trivial reference
        aref = rng.uniform(1, 3, nt)
        kw = dict(T=nt * dt, dt=dt, X=1, dx=dx, Y=Y, dy=dy, action_dim=adim, reward_class=src.NSReward(gamma), normalize=False,
                  reset_init_condition_func=lambda X: (u0.copy(), v0.copy(), p0.copy()), boundary_condition=bc,
                  U_ref=Uref, action_ref=aref, maximum_pressure_iteration=K, viscosity=nu, density=rho)
        env = src.NavierStokes2D(**kw)
        assert env.nx == n and env.ny == n
        env.reset()
        acts = rng.uniform(2, 4, (3, adim)) * np.array([1.0, -1.0, 0.5])[:, None]
        obs_l, p_l, r_l, te_l = [], [], [], []
        for a in acts:
            obs, r, te, tr, _ = env.step(a.copy() if per_node else float(a[0]))
            obs_l.append(np.array(obs))
            p_l.append(np.array(env.p))
            r_l.append(r)
            te_l.append(bool(te))
        name = f"S{ci:02d}_n{n}"
        pack(name, dict(u0=u0, v0=v0, p0=p0, U_ref=Uref, action_ref=aref, actions=acts, obs=np.stack(obs_l), p=np.stack(p_l),
                        rewards=np.array(r_l, dtype=np.float64), terminate=np.array(te_l),
                        bc=np.array([bc[k][i] for k in edges for i in (0, 1)])), store)
        _scalars(store, name, T=nt * dt, dt=dt, X=1.0, dx=dx, Y=float(Y), dy=dy, nt=nt, n=n, action_dim=adim, gamma=gamma,
                 viscosity=nu, density=rho, maximum_pressure_iteration=K, ic=ic)
    assert len(seen) == 24, sorted(seen)
    # non-square node counts: reset() and the arithmetic accept them, the store of the new field into U[t] does not
    n, m = 8, 5
    dx, dy = 1.0 / (n - 1), 1.0 / (m - 1)
    dt = 0.1 * min(dx, dy) ** 2 / 0.1
    kw = dict(T=4 * dt, dt=dt, X=1, dx=dx, Y=1, dy=dy, action_dim=1, reward_class=src.NSReward(0.1), normalize=False,
              reset_init_condition_func=lambda X: (np.zeros((m, n)), np.zeros((m, n)), np.zeros((m, n))), boundary_condition=NS_BC,
              U_ref=np.zeros((4, m, n, 2)), action_ref=np.ones(4), maximum_pressure_iteration=1)

    def non_square():
        env = src.NavierStokes2D(**kw)
        env.reset()
        env.step(1.0)
    store["unpinnable/ns_non_square"] = np.array(_raises(non_square))
    _scalars(store, "unpinnable/ns_non_square_kw", nx=n, ny=m)
    np.savez_compressed(os.path.join(out, "sweep_ns.npz"), **store)


def gen_sweep_traffic(src, out=HERE):
    """TrafficPDE1D away from the shipped notebook configuration: tau, v_max, ro_max, ro_steady, control_freq, dx (with a matching
    dt), X, the state limit, in all four simulation types; a short T so that the ``time_index >= T`` freeze (:173) and the ``T/dt``
    terminate comparison (:109) are crossed inside the recorded steps; a case that truncates through the state limit; an
    'outlet-train' case whose action bounds come from another steady state than its dynamics (:66-70 against :251-256)."""
    import contextlib
    import io
    import random
    store = {}
    rng = np.random.default_rng(20263)
    P1 = dict(T=240, dt=0.01, X=250, dx=0.5, tau=30, v_max=40, ro_max=0.16, ro_steady=0.12)
    P2 = dict(T=240, dt=0.1, X=400, dx=5, tau=60, v_max=30, ro_max=0.2, ro_steady=0.1)
    P3 = dict(T=240, dt=0.25, X=400, dx=8, tau=15, v_max=40, ro_max=0.2, ro_steady=0.12)
    P4 = dict(T=240, dt=0.25, X=500, dx=12.5, tau=30, v_max=30, ro_max=0.16, ro_steady=0.1)
    SH = dict(T=2, dt=0.25, X=500, dx=12.5, tau=60, v_max=40, ro_max=0.16, ro_steady=0.12)      # frozen from step 8, T/dt = 8 s at step 32
    HOT = dict(T=240, dt=0.25, X=400, dx=8, tau=60, v_max=40, ro_max=0.16, ro_steady=0.15)      # 1.1 ro_steady > ro_max
    #        name              params sim             cf limit steps
    table = [("fine_outlet", P1, "outlet", 5, True, 3),
             ("p2_inlet", P2, "inlet", 1, True, 6), ("p2_outlet", P2, "outlet", 2, False, 6), ("p2_both", P2, "both", 3, True, 6),
             ("p2_train", P2, "outlet-train", 5, True, 6),
             ("p3_inlet", P3, "inlet", 2, False, 6), ("p3_outlet", P3, "outlet", 3, True, 6), ("p3_both", P3, "both", 5, True, 6),
             ("p3_train", P3, "outlet-train", 1, False, 6),
             ("p4_inlet", P4, "inlet", 3, True, 6), ("p4_outlet", P4, "outlet", 5, True, 6), ("p4_both", P4, "both", 1, False, 6),
             ("p4_train", P4, "outlet-train", 2, True, 6),
             ("short_inlet", SH, "inlet", 2, True, 35), ("short_train", SH, "outlet-train", 3, True, 35),
             ("hot_limit", HOT, "both", 1, True, 4), ("hot_nolimit", HOT, "both", 1, False, 4)]
    for name, P, sim, cf, limit, nsteps in table:
        Veq = src.TrafficPDE1D.Veq
        kw = dict(T=P["T"], dt=P["dt"], X=P["X"], dx=P["dx"], reward_class=src.TrafficARZReward(), simulation_type=sim,
                  v_steady=Veq(P["v_max"], P["ro_max"], P["ro_steady"]), ro_steady=P["ro_steady"], v_max=P["v_max"],
                  ro_max=P["ro_max"], tau=P["tau"], limit_pde_state_size=limit, control_freq=cf)
        # 'outlet-train' draws its steady state with random.randint in the constructor and again in reset(): take the first seed
        # pair whose two draws differ, so the clip bounds and the dynamics use different qs
        seeds = (11, 13)
        if sim == "outlet-train":
            for s2 in range(13, 64):
                random.seed(11)
                a = random.randint(0, 2)
                random.seed(s2)
                if random.randint(0, 2) != a:
                    seeds = (11, s2)
                    break
        random.seed(seeds[0])
        with contextlib.redirect_stdout(io.StringIO()):
            env = src.TrafficPDE1D(**kw)
            qs_clip = env.qs
            random.seed(seeds[1])
            obs0, _ = env.reset()
        nact = 2 if sim == "both" else 1
        acts = rng.uniform(0.7, 1.3, (nsteps, nact)) * env.qs
        obs, rew, done, trunc, tim = [np.array(obs0)], [], [], [], []
        with np.errstate(all="ignore"):
            for a in acts:
                with contextlib.redirect_stdout(io.StringIO()):
                    o, r, d, t, _ = env.step(a)
                obs.append(np.array(o))
                rew.append(r)
                done.append(bool(d))
                trunc.append(bool(t))
                tim.append(env.time_index)
        if sim == "outlet-train":
            assert qs_clip != env.qs
        pack(name, dict(obs=np.stack(obs), reward=np.array(rew, dtype=np.float64), done=np.array(done), trunc=np.array(trunc),
                        time=np.array(tim, dtype=np.float64), actions=acts, rs=np.float64(env.rs), qs_clip=np.float64(qs_clip)), store)
        _scalars(store, name, sim=sim, control_freq=cf, limit=limit, v_steady=kw["v_steady"], **P)
    # what the short cases are for
    t = store["short_inlet/time"]
    assert (t[:-1] >= 2).any() and (np.diff(t) < 0).any(), "short T: the freeze and the T/dt reset must both be crossed"
    assert store["short_train/done"].any() and not store["short_train/done"][:31].any()
    assert store["hot_limit/trunc"].all() and not store["hot_nolimit/trunc"].any()
    np.savez_compressed(os.path.join(out, "sweep_traffic.npz"), **store)


def gen_sweep_tumor(src, out=HERE):
    """BrainTumor1D whole episodes over the constructor arguments tests/fuzz_more.py draws (X, dx, D, rho, alpha, alpha/beta, k, both
    thresholds and radii, the dosage threshold, total_dosage), ending the ways the raw episodes of tumor.npz do: lethal radius in
    Post-Therapy with and without t_benchmark, time limit in Therapy, time limit in Post-Therapy.  Rows sub-sampled (``keep``)."""
    import importlib
    bt = importlib.import_module("pde_control_gym.src.environments1d.brain_tumor_env")
    br = importlib.import_module("pde_control_gym.src.rewards.brain_tumor_reward")
    store = {}
    rng = np.random.default_rng(20264)
    A = dict(X=64, dx=0.5, D=0.1, rho=0.05, alpha=0.1, alpha_beta_ratio=3, k=1.0, t1_detection_threshold=0.6, t2_detection_threshold=0.3,
             dosage_termination_threshold=1.0, t1_detection_radius=10, t1_death_radius=25, total_dosage=30.0)
    B = dict(X=100, dx=2, D=0.2, rho=0.03, alpha=0.04, alpha_beta_ratio=10, k=3e4, t1_detection_threshold=0.8, t2_detection_threshold=0.16,
             dosage_termination_threshold=0.1, t1_detection_radius=15, t1_death_radius=35, total_dosage=100.0)
    C = dict(X=300, dx=1, D=0.05, rho=0.05, alpha=0.04, alpha_beta_ratio=10, k=1e5, t1_detection_threshold=0.6, t2_detection_threshold=0.16,
             dosage_termination_threshold=1.0, t1_detection_radius=10, t1_death_radius=35, total_dosage=61.2)
    D = dict(X=200, dx=1, D=0.1, rho=0.03, alpha=0.04, alpha_beta_ratio=10, k=1.0, t1_detection_threshold=0.8, t2_detection_threshold=0.3,
             dosage_termination_threshold=0.1, t1_detection_radius=15, t1_death_radius=25, total_dosage=30.0)
    E = dict(X=100, dx=0.5, D=0.05, rho=0.03, alpha=0.04, alpha_beta_ratio=3, k=3e4, t1_detection_threshold=0.8, t2_detection_threshold=0.16,
             dosage_termination_threshold=0.1, t1_detection_radius=10, t1_death_radius=25, total_dosage=61.2)
    F = dict(X=64, dx=2, D=0.2, rho=0.05, alpha=0.1, alpha_beta_ratio=10, k=1e5, t1_detection_threshold=0.6, t2_detection_threshold=0.16,
             dosage_termination_threshold=1.0, t1_detection_radius=15, t1_death_radius=25, total_dosage=30.0)
    ends = {}
    #                   name           set T    t_benchmark  dose range
    for name, P, T, tb, hi in [("a_death_post", A, 600, 200, 0.05), ("b_term_therapy", B, 250, 200, 0.05), ("c_term_post", C, 300, 250, 0.3),
                               ("d_nobench", D, 600, None, 0.05), ("e_term_post", E, 400, 300, 0.3), ("f_death_post", F, 600, 250, 0.1)]:
        nx = int(round(P["X"] / P["dx"]) + 1)
        init = 0.8 * P["k"] * np.exp(-0.25 * np.linspace(0, P["X"], nx) ** 2) * rng.uniform(0.9, 1.0)
        env = bt.BrainTumor1D(T=T, dt=1, normalize=True, reward_class=br.BrainTumorReward(), verbose=False,
                              reset_init_condition_func=lambda X, n: init, **P)
        assert env.nx == nx
        env.t_benchmark = tb
        env.reset()
        acts, rew, term, trunc, stage = [], [], [], [], []
        while True:
            a = float(rng.uniform(0, hi))
            o, r, te, tr, info = env.step(a)
            acts.append(a)
            rew.append(float(r))
            term.append(bool(te))
            trunc.append(bool(tr))
            stage.append({"Growth": 0, "Therapy": 1, "Post-Therapy": 2}[info["stage"]])
            if te or tr:
                break
        n = len(acts)
        ends[name] = (stage[-1], term[-1], trunc[-1])
        keep = np.unique(np.concatenate([np.arange(0, n + 1, 16), [n]]))
        pack(name, dict(init=init, actions=np.array(acts), t_benchmark=np.float64(np.nan if tb is None else tb),
                        reward=np.array(rew), term=np.array(term), trunc=np.array(trunc), stage=np.array(stage),
                        keep=keep, rows=env.u[keep].copy(), t1_idx=env.t1_radius_idx_vs_time[: n + 1].copy(),
                        dosage=env.dosage_vs_time[: n + 1].copy(),
                        days=np.array([env.growthDays, env.therapyDays, env.postTherapyDays, env.simulationDays,
                                       -1 if env.cDeathDay is None else env.cDeathDay]),
                        remaining=np.float64(env.remaining_dosage)), store)
        _scalars(store, name, T=T, dt=1, **P)
    assert ends["a_death_post"] == (2, False, True) and ends["d_nobench"] == (2, False, True) and ends["f_death_post"] == (2, False, True)
    assert ends["b_term_therapy"] == (1, True, False) and ends["c_term_post"] == (2, True, False) and ends["e_term_post"] == (2, True, False)
    np.savez_compressed(os.path.join(out, "sweep_tumor.npz"), **store)

# ---- non-finite inputs: what the reference does with a NaN / +-Inf command, a NaN dosage, a NaN cell in a state ------------------
# np.clip, np.linalg.norm, Python's min(x, ...) / max(x, ...) and the stencils all KEEP a NaN: the recorded observations, rewards
# and flags are what the oracle (and through it every engine) has to reproduce, NaN positions included.  One reference instance per
# run.  To keep the file small the constructor parameters of a family are stored once ("<family>_kw/..."), and the three plants of a
# traffic configuration are stacked on a leading axis (their rows agree away from the driven end, which the compressor finds).
# Where the reference raises, the exception class is recorded under "<case>/raises" (the generator fails if it stops raising) and
# the action of that call is the last of "actions".
NF_PLANTS = (("nan", float("nan")), ("pinf", float("inf")), ("ninf", float("-inf")))


def gen_nonfinite(src, out=HERE):
    import contextlib
    import importlib
    import io
    import random
    store = {}
    rng = np.random.default_rng(20265)
    # ---- traffic: X = 500, dx = 10 (M = 51), six steps, the plant in the command of step 1; 'both' also in the second column
    P = dict(T=240, dt=0.25, X=500, dx=10, tau=60, v_max=40, ro_max=0.16, ro_steady=0.12)
    Veq = src.TrafficPDE1D.Veq
    v_steady = Veq(P["v_max"], P["ro_max"], P["ro_steady"])
    _scalars(store, "traffic_kw", control_freq=1, limit=True, v_steady=v_steady, **P)
    for sim, col in (("inlet", 0), ("outlet", 0), ("both", 0), ("both", 1)):
        nact = 2 if sim == "both" else 1
        base = rng.uniform(0.7, 1.3, (6, nact))
        runs = []
        for pname, pval in NF_PLANTS:
            kw = dict(T=P["T"], dt=P["dt"], X=P["X"], dx=P["dx"], reward_class=src.TrafficARZReward(), simulation_type=sim,
                      v_steady=v_steady, ro_steady=P["ro_steady"], v_max=P["v_max"], ro_max=P["ro_max"], tau=P["tau"],
                      limit_pde_state_size=True, control_freq=1)
            random.seed(11)
            with contextlib.redirect_stdout(io.StringIO()):
                env = src.TrafficPDE1D(**kw)
                qs_clip = env.qs
                random.seed(13)
                obs0, _ = env.reset()
            acts = base * env.qs
            acts[1, col] = pval
            obs, rew, done, trunc, tim = [np.array(obs0)], [], [], [], []
            with np.errstate(all="ignore"):
                for a in acts:
                    with contextlib.redirect_stdout(io.StringIO()):
                        o, r, d, t, _ = env.step(a.copy())
                    obs.append(np.array(o))
                    rew.append(r)
                    done.append(bool(d))
                    trunc.append(bool(t))
                    tim.append(env.time_index)
            runs.append(dict(obs=np.stack(obs), reward=np.array(rew, dtype=np.float64), done=np.array(done), trunc=np.array(trunc),
                             time=np.array(tim, dtype=np.float64), actions=acts))
            if pname == "nan":
                assert np.isnan(obs[2]).sum() >= 2 and np.isnan(rew[1]) and not np.isnan(obs[1]).any(), (sim, col)
        name = f"traffic_{sim}_c{col}"
        pack(name, {k: np.stack([r_[k] for r_ in runs]) for k in runs[0]}, store)
        pack(name, dict(rs=np.float64(env.rs), qs_clip=np.float64(qs_clip), sim=np.array(sim), plants=np.array([n_ for n_, _ in NF_PLANTS])),
             store)
    # ---- tumour: X = 100, dx = 1; set A of gen_sweep_tumor on a wide initial profile (therapy from day 21); a NaN cell in the
    # initial profile; a NaN / +Inf / -Inf dosage on the second therapy day.  Rows sub-sampled (``keep``), the last ones all kept.
    bt = importlib.import_module("pde_control_gym.src.environments1d.brain_tumor_env")
    br = importlib.import_module("pde_control_gym.src.rewards.brain_tumor_reward")
    A = dict(X=100, dx=1, D=0.1, rho=0.05, alpha=0.1, alpha_beta_ratio=3, k=1.0, t1_detection_threshold=0.6, t2_detection_threshold=0.3,
             dosage_termination_threshold=1.0, t1_detection_radius=10, t1_death_radius=25, total_dosage=30.0)
    T = 40
    _scalars(store, "tumor_kw", T=T, dt=1, **A)
    xs = np.linspace(0, A["X"], 101)
    for name, cell, dose in (("tumor_cell_nan", 40, None),) + tuple((f"tumor_dose_{n}", None, v) for n, v in NF_PLANTS):
        init = 0.8 * A["k"] * np.exp(-(xs / 11.0) ** 2)
        if cell is not None:
            init[cell] = np.nan
        env = bt.BrainTumor1D(T=T, dt=1, normalize=True, reward_class=br.BrainTumorReward(), verbose=False,
                              reset_init_condition_func=lambda X, n: init.copy(), **A)
        env.t_benchmark = 30
        env.reset()
        acts, rew, term, trunc, stage, raised = [], [], [], [], [], ""
        therapy_days = 0
        with np.errstate(all="ignore"):
            while len(acts) < T:
                a = float(rng.uniform(0.02, 0.1))
                if env.stage == "Therapy":
                    therapy_days += 1
                    if dose is not None and therapy_days == 2:
                        a = dose
                acts.append(a)
                step = lambda: env.step(a)      # noqa: E731
                if dose is not None and dose != float("inf") and therapy_days == 3:
                    raised = _raises(step)      # the day after a NaN / -Inf dosage: the whole treated region is NaN, T2 radius None
                    break
                o, r, te, tr, info = step()
                rew.append(float(r))
                term.append(bool(te))
                trunc.append(bool(tr))
                stage.append({"Growth": 0, "Therapy": 1, "Post-Therapy": 2}[info["stage"]])
                if te or tr:
                    break
        n = len(rew)
        assert therapy_days >= 2, (name, therapy_days)
        keep = np.unique(np.concatenate([np.arange(0, n + 1, 10), np.arange(max(0, n - 1), n + 1)]))
        pack(name, dict(init=init, actions=np.array(acts), t_benchmark=np.float64(30), reward=np.array(rew), term=np.array(term),
                        trunc=np.array(trunc), stage=np.array(stage), keep=keep, rows=env.u[keep].copy(),
                        dosage=env.dosage_vs_time[: n + 1].copy(),
                        days=np.array([env.growthDays, env.therapyDays, env.postTherapyDays, env.simulationDays,
                                       -1 if env.cDeathDay is None else env.cDeathDay]),
                        remaining=np.float64(env.remaining_dosage), raises=np.array(raised)), store)
    # ---- Navier-Stokes: 11 x 11, K = 3, per-node commands on one Controllable edge (upper, u), three steps.  Fields in sixteenths.
    n, K, nt = 11, 3, 5
    bc = {"upper": ["Controllable", "Dirchilet"], "lower": ["Dirchilet", "Neumann"], "left": ["Neumann", "Dirchilet"],
          "right": ["Dirchilet", "Neumann"]}
    edges = ("upper", "lower", "left", "right")
    dx = 1.0 / (n - 1)
    dt = 0.2 * 0.5 * dx ** 2 / 0.1
    base = [rng.integers(-16, 17, (n, n)) / 16.0 for _ in range(3)]
    Uref = rng.integers(-16, 17, (nt, n, n, 2)) / 16.0
    aref = rng.integers(16, 49, nt) / 16.0
    acts0 = rng.integers(32, 65, (3, n)) / 16.0
    pack("ns_kw", dict(u0=base[0], v0=base[1], p0=base[2], U_ref=Uref, action_ref=aref, actions=acts0,
                       bc=np.array([bc[k][i] for k in edges for i in (0, 1)])), store)
    _scalars(store, "ns_kw", T=nt * dt, dt=dt, X=1.0, dx=dx, Y=1.0, dy=dx, nt=nt, n=n, action_dim=n, gamma=0.1,
             viscosity=0.1, density=1.0, maximum_pressure_iteration=K)
    # (what is planted: "a" = actions[step, node], "u" / "p" = initial field [row, column])
    for name, what, where, val in (("ns_cmd_nan", "a", (1, 4), float("nan")), ("ns_cmd_pinf", "a", (1, 4), float("inf")),
                                   ("ns_u_nan", "u", (5, 5), float("nan")), ("ns_p_nan", "p", (5, 5), float("nan"))):
        u0, v0, p0 = (b.copy() for b in base)
        acts = acts0.copy()
        {"a": acts, "u": u0, "p": p0}[what][where] = val
        kw = dict(T=nt * dt, dt=dt, X=1, dx=dx, Y=1, dy=dx, action_dim=n, reward_class=src.NSReward(0.1), normalize=False,
                  reset_init_condition_func=lambda X: (u0.copy(), v0.copy(), p0.copy()), boundary_condition=bc,
                  U_ref=Uref, action_ref=aref, maximum_pressure_iteration=K, viscosity=0.1, density=1.0)
        env = src.NavierStokes2D(**kw)
        env.reset()
        obs_l, p_l, r_l, te_l = [], [], [], []
        with np.errstate(all="ignore"):
            for a in acts:
                obs, r, te, tr, _ = env.step(a.copy())
                obs_l.append(np.array(obs))
                p_l.append(np.array(env.p))
                r_l.append(r)
                te_l.append(bool(te))
        pack(name, dict(plant_in=np.array(what), plant_at=np.array(where), plant=np.float64(val), obs=np.stack(obs_l), p=np.stack(p_l),
                        rewards=np.array(r_l, dtype=np.float64), terminate=np.array(te_l)), store)
        if val != val:
            assert np.isnan(obs_l[-1]).sum() >= np.isnan(obs_l[1]).sum() > 0 and np.isnan(r_l[-1]), name
    np.savez_compressed(os.path.join(out, "nonfinite.npz"), **store)

FILES = {"transport": "transport.npz", "parabolic": "parabolic.npz", "kat": "kat.npz", "mixed": "mixed.npz", "ns": "ns2d.npz",
         "traffic": "traffic.npz", "tumor": "tumor.npz", "sweep_1d": "sweep_1d.npz", "sweep_ns": "sweep_ns.npz",
         "sweep_traffic": "sweep_traffic.npz", "sweep_tumor": "sweep_tumor.npz", "nonfinite": "nonfinite.npz"}


GEN = {"transport": gen_transport, "parabolic": gen_parabolic, "kat": gen_kat, "mixed": gen_mixed, "ns": gen_ns,
       "traffic": gen_traffic, "tumor": gen_tumor, "sweep_1d": gen_sweep_1d, "sweep_ns": gen_sweep_ns,
       "sweep_traffic": gen_sweep_traffic, "sweep_tumor": gen_sweep_tumor, "nonfinite": gen_nonfinite}


def check(which=None):
    """Regenerate into a scratch directory and compare with the committed fixtures: same keys, same dtypes, same shapes, same
    BITS.  Returns the list of differences (empty = the committed files are exactly what the generator writes today)."""
    import tempfile
    committed = HERE
    diffs = []
    with tempfile.TemporaryDirectory() as tmp:
        src = import_reference()
        for w in (which or list(GEN)):
            GEN[w](src, tmp)
            a, b = np.load(os.path.join(committed, FILES[w]), allow_pickle=False), np.load(os.path.join(tmp, FILES[w]), allow_pickle=False)
            for k in sorted(set(a.files) | set(b.files)):
                if k not in a.files or k not in b.files:
                    diffs.append(f"{FILES[w]}: key {k} only in the {'generator output' if k in b.files else 'committed file'}")
                elif a[k].dtype != b[k].dtype or a[k].shape != b[k].shape or a[k].tobytes() != b[k].tobytes():
                    diffs.append(f"{FILES[w]}: {k} differs")
    return diffs


if __name__ == "__main__":
    if "--check" in sys.argv[1:]:
        d = check([w for w in sys.argv[1:] if w != "--check"] or list(GEN))
        print("\n".join(d) if d else "fixtures == generator output")
        sys.exit(1 if d else 0)
    src = import_reference()
    which = sys.argv[1:] or list(GEN)
    for w in which:
        GEN[w](src)
        print("wrote", w)
    with open(os.path.join(HERE, "VERSIONS.txt"), "w") as f:
        f.write(f"numpy {np.__version__}\nreference snapshot 2026-01-09 (lukebhan/PDEControlGym)\n")
