"""BrainTumor1D TherapyWrapper rollouts through DeviceRollout: today's path (the launches of ``TumorVecEnv.step_tensor`` plus one
policy launch per step, replayed as one hipGraph) against ``fused_step=True`` (one pdegym_tumor_therapy_step launch per step in the
same graph) and against the whole rollout in ONE launch (pdegym_tumor_rollout, ``one_launch=True``).

    python tools/measure_tumor_rollout.py [--batch 16384] [--window 0.5] [--repeats 5] [--out profiles/tumor_rollout.json]

The notebook's shape: nx = 201, T = 600 days, 32 wrapper steps per run().  For ``weekends`` off and on, three sources of commands:
given ahead (doses uniform(0.2, 1) x linspace(0.03, 0.3) over the patients, redrawn per step), a 64-64 tanh actor and a 256-256 tanh
actor (first layer scaled by 1e-5: the densities are O(1e5)) with exploration noise N(0.08, 0.06) and the clamp [0, 1].  After a
warm-up the three paths are timed ALTERNATELY in the same process: a window is N consecutive run() calls between two HIP events, N
chosen so that the fastest path's window lasts at least ``--window`` seconds, ``--repeats`` windows each.  All paths make the same
number of runs from the same state; where the arithmetic is the same (commands given ahead; the 256-256 actor, whose in-kernel
evaluation is pdegym_mlp_forward's) their last rollouts and end states are compared bit for bit.  The 64-64 actor inside the launch
sums in another order than pdegym_mlp_forward, so its trajectories part and only the timing is reported.
Prints one JSON line per case and writes them all to ``--out``.  Needs a GPU: there is no CPU path.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

T_STEPS = 32
KW = dict(T=600, X=200, dt=1, dx=1, normalize=True, dosage_termination_threshold=0.1, t1_detection_threshold=0.8,
          t2_detection_threshold=0.16, D=0.2, rho=0.03, alpha=0.04, alpha_beta_ratio=10, k=1e5, t1_detection_radius=15,
          t1_death_radius=35, total_dosage=61.2, verbose=False)
KEYS = ("obs", "actions", "rewards", "terminated", "truncated")
STATE = ("u", "time_index", "stage", "remaining", "days")
PATHS = (("step_tensor_graph", False, None), ("fused_step_graph", True, None), ("one_launch", False, True))


def tumor_ic(X, nx):
    xs = np.linspace(0, X, nx)
    return 0.8 * 1e5 * np.exp(-0.25 * (xs ** 2))


def build(B, weekends, fused):
    import pde_control_gym
    from pde_control_gym.src import BrainTumorReward
    venv = pde_control_gym.make_vec("PDEControlGym-BrainTumor1D", num_envs=B, weekends=weekends, fused_step=fused,
                                    reward_class=BrainTumorReward(), reset_init_condition_func=tumor_ic, **KW)
    venv.benchmark()
    venv.reset_tensor()
    return venv


class Ahead:
    """Commands given ahead as a policy for the paths that call one per step: call k returns row k mod T of the rollout's commands
    (the calls are made while the graph is captured, so each step of the replayed graph reads its own row)."""

    def __init__(self, commands):
        self.commands, self.k = commands, 0

    def __call__(self, obs):
        row = self.commands[self.k % self.commands.shape[0]]
        self.k += 1
        return row


def actor(width):
    import torch
    from pde_control_gym import FusedMLP
    torch.manual_seed(1)
    net = torch.nn.Sequential(torch.nn.Linear(201, width), torch.nn.Tanh(), torch.nn.Linear(width, width), torch.nn.Tanh(),
                              torch.nn.Linear(width, 1), torch.nn.Tanh()).cuda()
    with torch.no_grad():
        net[0].weight.mul_(1e-5)
    return FusedMLP(net)


def window(ro, runs):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(runs):
        ro.run()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3


def measure(B, weekends, source, seconds, repeats):
    import torch
    from pde_control_gym import DeviceRollout
    rng = np.random.default_rng(5)
    commands = torch.from_numpy(rng.uniform(0.2, 1, (T_STEPS, B)) * np.linspace(0.03, 0.3, B)).cuda()
    noise = torch.from_numpy(rng.normal(0.08, 0.06, (T_STEPS, B)).astype(np.float32)).cuda()
    paths, envs = {}, {}
    for key, fused, one in PATHS:
        venv = build(B, weekends, fused)
        if source == "ahead":
            policy = None if one else Ahead(commands)
        else:
            policy = actor(64 if source == "actor_64_64" else 256)
        ro = DeviceRollout(venv, policy, T_STEPS, use_graph=True, action_low=0.0, action_high=1.0, action_noise=source != "ahead",
                           one_launch=one)
        assert ro.one_launch is bool(one)
        if source == "ahead":
            ro.actions.copy_(commands)
        else:
            ro.action_noise.copy_(noise)
        paths[key], envs[key] = ro, venv
    for ro in paths.values():             # capture + warm-up: the same three runs on all
        for _ in range(3):
            ro.run()
    torch.cuda.synchronize()
    per_run = min(window(ro, 4) / 4 for ro in paths.values())
    runs = max(4, int(np.ceil(1.15 * seconds / per_run)))
    times = {k: [] for k in paths}
    for _ in range(repeats):
        for k, ro in paths.items():
            times[k].append(window(ro, runs))
    torch.cuda.synchronize()

    def same(a, b):
        ra, rb, va, vb = paths[a], paths[b], envs[a], envs[b]
        eq = all(torch.equal(getattr(ra, k).view(torch.uint8), getattr(rb, k).view(torch.uint8)) for k in KEYS)
        eq = eq and all(torch.equal(va.core.t[k].contiguous().view(torch.uint8), vb.core.t[k].contiguous().view(torch.uint8)) for k in STATE)
        return bool(eq and torch.equal(va.treatment_calls, vb.treatment_calls))

    us = {k: [t / (runs * T_STEPS) * 1e6 for t in v] for k, v in times.items()}
    med = {k: float(np.median(v)) for k, v in us.items()}
    ref = paths["step_tensor_graph"]
    done = (ref.terminated | ref.truncated).float().mean().item()
    from pdecontrolgym_amd import build as B_
    return dict(config=dict(B=B, nx=201, T_days=600, steps_per_run=T_STEPS, weekends=weekends, commands=source), runs_per_window=runs,
                windows_per_path=repeats, shortest_window_seconds=round(min(min(v) for v in times.values()), 4),
                us_per_wrapper_step={k: dict(median=round(med[k], 2), min=round(min(v), 2), max=round(max(v), 2), windows=[round(x, 2) for x in v])
                                     for k, v in us.items()},
                fastest=min(med, key=med.get),
                ratio_step_tensor_over_one_launch=round(med["step_tensor_graph"] / med["one_launch"], 3),
                ratio_step_tensor_over_fused_step=round(med["step_tensor_graph"] / med["fused_step_graph"], 3),
                fused_step_bitwise_equal=same("step_tensor_graph", "fused_step_graph"),
                one_launch_bitwise_equal=(same("step_tensor_graph", "one_launch") if source != "actor_64_64" else None),
                finished_fraction_per_step_last_run=round(done, 4), mean_dose_last_run=round(float(ref.actions.mean()), 4),
                device=torch.cuda.get_device_name(0), arch=getattr(torch.cuda.get_device_properties(0), "gcnArchName", ""),
                library_stamp=B_.library_stamp()[:16], unit="microseconds per wrapper step of the whole batch (run() time / 32)")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batch", type=int, default=16384)
    ap.add_argument("--window", type=float, default=0.5, help="least seconds per timed window (any path)")
    ap.add_argument("--repeats", type=int, default=5, help="windows per path, alternating")
    ap.add_argument("--commands", nargs="*", default=["ahead", "actor_64_64", "actor_256_256"])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("measure_tumor_rollout needs a GPU (there is no CPU path)")
    rows = []
    for weekends in (False, True):
        for source in args.commands:
            t0 = time.perf_counter()
            row = measure(args.batch, weekends, source, args.window, args.repeats)
            row["wall_seconds"] = round(time.perf_counter() - t0, 1)
            rows.append(row)
            print(json.dumps(row), flush=True)
            if args.out:      # after every case: a run that is cut short keeps what it measured
                with open(args.out, "w") as f:
                    json.dump({"tool": "tools/measure_tumor_rollout.py", "rows": rows}, f, indent=1)
                    f.write("\n")
    bad = [r["config"] for r in rows if r["fused_step_bitwise_equal"] is False or r["one_launch_bitwise_equal"] is False]
    if bad:
        sys.exit(f"paths that must agree bit for bit differ: {bad}")


if __name__ == "__main__":
    main()
