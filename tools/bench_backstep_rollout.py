"""Backstepping baseline through DeviceRollout: two launches per env-step (control law + step, replayed as one hipGraph) against
the law inside the one-launch rollout kernel (pdegym_*_backstep_rollout, ``one_launch=True``).

    python tools/bench_backstep_rollout.py [--batch 4096] [--window 0.5] [--repeats 5] [--out profiles/backstep_rollout.json]

Per shape two identical environments are built (same seed: rows, pools, gains), one per path, both with T = 25 env-steps per run(),
the fused auto-reset on pools of 2 B rows (initial condition, beta and theta) and ``use_graph=True``.  After a warm-up the two paths
are timed ALTERNATELY in the same process: a window is N consecutive run() calls between two HIP events, N chosen so that the faster
path's window lasts at least ``--window`` seconds, ``--repeats`` windows each.  Both paths make the same number of runs, and at the end
the rollout buffers and the engine state of the two environments are compared bit for bit (the whole chain of runs, at the timed size).
Prints one JSON line per shape and writes them all to ``--out``.  Needs a GPU: there is no CPU path.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

T_STEPS = 25
SHAPES = {
    # name: kind, nx, dt (None: 0.25 dx^2), sub-steps per env-step, env-steps per episode, gamma, amplitude
    "parabolic_c2": ("parabolic", 256, None, 100, 1000, 8.0, 50.0),            # bench.py's C2 grid
    "transport_script": ("transport", 100, 1e-4, 1000, 50, 7.35, 5.0),         # transport1Dbackstepping.py
    "parabolic_script": ("parabolic", 200, 1e-5, 100, 1000, 8.0, 50.0),        # reactionDiffusion1DBackstepping.py
}
ENV_ID = {"transport": "PDEControlGym-TransportPDE1D", "parabolic": "PDEControlGym-ReactionDiffusionPDE1D"}
KEYS = ("obs", "actions", "rewards", "terminated", "truncated")
STATE = ("time_index", "reset_count", "bsum", "ring", "obs", "beta", "norm_now", "norm_back")


def build(name, B, order, seed):
    import pde_control_gym
    from pde_control_gym import BacksteppingController
    from pde_control_gym.src import TunedReward1D
    kind, nx, dt, S, episode, gamma0, amp = SHAPES[name]
    dx = 1.0 / nx
    dt = 0.25 * dx * dx if dt is None else dt
    n = nx + (kind == "parabolic")
    rng = np.random.default_rng(seed)

    def draw(rows):
        gam = gamma0 + rng.uniform(-0.5, 0.5, (rows, 1))
        beta = (amp * np.cos(gam * np.arccos(np.linspace(0, 1, n))[None])).astype(np.float32)
        theta = (amp * np.cos(gam * np.arccos(np.linspace(dx, 1, n))[None])).astype(np.float32)
        return (rng.uniform(1, 10, (rows, 1)) * np.ones((1, n))).astype(np.float32), beta, theta
    (init, beta, theta), (pinit, pbeta, ptheta) = draw(B), draw(2 * B)
    T = episode * S * dt
    params = dict(T=T, dt=dt, X=1, dx=dx, control_sample_rate=S * dt, reward_class=TunedReward1D(int(round(T / dt)), -1e3, 3e2),
                  normalize=False, sensing_loc="full", control_type="Dirchilet", sensing_type=None, limit_pde_state_size=True,
                  max_state_value=1e10, max_control_value=20, batched_reset_func=lambda idx, nx_: (init[idx], beta[idx]))
    venv = pde_control_gym.make_vec(ENV_ID[kind], num_envs=B, device="cuda", **params)
    venv.reset_tensor()
    venv.enable_fused_auto_reset(init_pool=pinit, beta_pool=pbeta)
    ctrl = BacksteppingController(kind, theta, dx, pool_theta=ptheta, order=order, device="cuda").attach(venv)
    return venv, ctrl, dict(kind=kind, nx=nx, n=n, dt=dt, dx=dx, substeps=S, env_steps_per_episode=episode, B=B, T=T_STEPS, order=order,
                            pool_rows=2 * B)


def window(ro, runs):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(runs):
        ro.run()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3


def measure(name, B, order, seconds, repeats, seed):
    import torch
    from pde_control_gym import DeviceRollout
    paths = {}
    for key, one in (("two_launch_graph", None), ("one_launch", True)):
        venv, ctrl, cfg = build(name, B, order, seed)
        ro = DeviceRollout(venv, ctrl, T_STEPS, use_graph=True, action_low=-20.0, action_high=20.0, one_launch=one)
        assert ro.one_launch is bool(one)
        paths[key] = (venv, ro)
    for _, ro in paths.values():             # capture + warm-up: the same three runs on both
        for _ in range(3):
            ro.run()
    torch.cuda.synchronize()
    # sixteen more runs on both: the window is sized by the FASTER path, with a margin, so that every window of either path lasts
    # at least ``seconds``
    per_run = min(window(ro, 16) / 16 for _, ro in paths.values())
    runs = max(16, int(np.ceil(1.15 * seconds / per_run)))
    times = {k: [] for k in paths}
    for _ in range(repeats):
        for k, (_, ro) in paths.items():
            times[k].append(window(ro, runs))
    torch.cuda.synchronize()
    (va, ra), (vb, rb) = paths["two_launch_graph"], paths["one_launch"]
    equal = all(torch.equal(getattr(ra, k).view(torch.uint8), getattr(rb, k).view(torch.uint8)) for k in KEYS)
    equal = equal and all(torch.equal(va.core.t[k].contiguous().view(torch.uint8), vb.core.t[k].contiguous().view(torch.uint8)) for k in STATE)
    restarts = int(va.core.t["reset_count"].sum())
    finite = bool(torch.isfinite(ra.actions).all())
    us = {k: [t / (runs * T_STEPS) * 1e6 for t in v] for k, v in times.items()}
    med = {k: float(np.median(v)) for k, v in us.items()}
    from pdecontrolgym_amd import build as B_
    return dict(shape=name, config=cfg, runs_per_window=runs, windows_per_path=repeats, total_runs_per_path=19 + runs * repeats,
                shortest_window_seconds=round(min(min(v) for v in times.values()), 4),
                window_seconds={k: [round(t, 4) for t in v] for k, v in times.items()},
                us_per_env_step={k: dict(median=round(med[k], 3), min=round(min(v), 3), max=round(max(v), 3), windows=[round(x, 3) for x in v])
                                 for k, v in us.items()},
                ratio_two_over_one=round(med["two_launch_graph"] / med["one_launch"], 3), bitwise_equal=bool(equal),
                restarts_total=restarts, commands_finite=finite, device=torch.cuda.get_device_name(0), arch=getattr(torch.cuda.get_device_properties(0), "gcnArchName", ""), library_stamp=B_.library_stamp()[:16],
                unit="microseconds per env-step of the whole batch (run() time / 25)")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--window", type=float, default=0.5, help="least seconds per timed window (either path)")
    ap.add_argument("--repeats", type=int, default=5, help="windows per path, alternating")
    ap.add_argument("--order", choices=("tree", "ordered"), default="tree")
    ap.add_argument("--shapes", nargs="*", default=list(SHAPES), choices=list(SHAPES))
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_backstep_rollout needs a GPU (there is no CPU path)")
    rows = []
    for name in args.shapes:
        t0 = time.perf_counter()
        row = measure(name, args.batch, args.order, args.window, args.repeats, args.seed)
        row["wall_seconds"] = round(time.perf_counter() - t0, 1)
        rows.append(row)
        print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"tool": "tools/bench_backstep_rollout.py", "rows": rows}, f, indent=1)
            f.write("\n")
    if not all(r["bitwise_equal"] for r in rows):
        sys.exit("the two paths differ")


if __name__ == "__main__":
    main()
