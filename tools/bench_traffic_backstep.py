"""TrafficPDE1D backstepping baseline through DeviceRollout: two launches per env-step (control law + step, replayed as one hipGraph)
against the law inside the one-launch rollout kernel (pdegym_traffic_backstep_rollout, ``one_launch=True``) -- and, as a floor, the
open-loop pdegym_traffic_rollout with the same commands given ahead (no law at all).

    python tools/bench_traffic_backstep.py [--batch 16384] [--window 0.5] [--repeats 5] [--out profiles/traffic_backstep.json]

Per control_freq (1 and 2) three identical environments are built on the notebook's grid (M = 51, 'outlet'), T = 64 env-steps per
run() with ``use_graph=True``.  After a warm-up the three paths are timed ALTERNATELY in the same process: a window is N consecutive
run() calls between two HIP events, N chosen so that the fastest path's window lasts at least ``--window`` seconds, ``--repeats``
windows each.  The closed-loop paths make the same number of runs and are compared bit for bit at the end; the floor replays the
commands of an early closed-loop run on its own advancing state (it is a timing floor, not a trajectory).  The episode length is set
far beyond the timed steps: the reference's PDE stops moving once ``time >= T`` (960 env-steps at the notebook's T = 240) while the
episode runs on to 3 840, and a window of frozen steps would time an empty loop.
Prints one JSON line per control_freq and writes them all to ``--out``.  Needs a GPU: there is no CPU path.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

T_STEPS = 64
PARAMS = dict(T=1e9, dt=0.25, X=500, dx=10, v_steady=10, ro_steady=0.12, v_max=40, ro_max=0.16, tau=60)
KEYS = ("obs", "actions", "rewards", "terminated", "truncated")
STATE = ("r", "y", "time", "rs", "obs")


def build(B, cf, order):
    import pde_control_gym
    from pde_control_gym import TrafficBacksteppingController
    from pde_control_gym.src import TrafficARZReward
    venv = pde_control_gym.make_vec("PDEControlGym-TrafficPDE1D", num_envs=B, device="cuda", reward_class=TrafficARZReward(),
                                    simulation_type="outlet", limit_pde_state_size=True, control_freq=cf, **PARAMS)
    venv.reset_tensor()
    return venv, TrafficBacksteppingController(venv, order=order)


class OpenLoop:
    """The floor: pdegym_traffic_rollout with commands given ahead, captured in a graph like the other two paths."""

    def __init__(self, venv, actions):
        import torch
        core = self.core = venv.core
        B, M = core.num_envs, core.M
        self.obs = torch.zeros(T_STEPS + 1, B, 2 * M, dtype=torch.float64, device="cuda")
        self.actions = actions.reshape(T_STEPS, B, 1).clone()
        self.rewards = torch.zeros(T_STEPS, B, dtype=torch.float64, device="cuda")
        self.done, self.trunc = (torch.zeros(T_STEPS, B, dtype=torch.uint8, device="cuda") for _ in range(2))
        self.graph = None

    def _body(self):
        self.core.rollout(self.obs, self.actions, self.rewards, self.done, self.trunc)

    def run(self):
        import torch
        if self.graph is None:
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                self._body()
                self.graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(self.graph, stream=side):
                    self._body()
            torch.cuda.current_stream().wait_stream(side)
        self.graph.replay()


def window(ro, runs):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(runs):
        ro.run()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3


def measure(B, cf, order, seconds, repeats):
    import torch
    from pde_control_gym import DeviceRollout
    paths, envs = {}, {}
    for key, one in (("two_launch_graph", None), ("one_launch", True)):
        venv, ctrl = build(B, cf, order)
        ro = DeviceRollout(venv, ctrl, T_STEPS, use_graph=True, action_low=0.96, action_high=1.44, one_launch=one)
        assert ro.one_launch is bool(one)
        paths[key], envs[key] = ro, venv
    for ro in paths.values():             # capture + warm-up: the same three runs on both
        for _ in range(3):
            ro.run()
    torch.cuda.synchronize()
    venv, _ = build(B, cf, order)
    paths["open_loop_floor"] = OpenLoop(venv, paths["one_launch"].actions)
    for _ in range(3):
        paths["open_loop_floor"].run()
    torch.cuda.synchronize()
    per_run = min(window(ro, 16) / 16 for ro in paths.values())
    runs = max(16, int(np.ceil(1.15 * seconds / per_run)))
    times = {k: [] for k in paths}
    for _ in range(repeats):
        for k, ro in paths.items():
            times[k].append(window(ro, runs))
    torch.cuda.synchronize()
    ra, rb = paths["two_launch_graph"], paths["one_launch"]
    va, vb = envs["two_launch_graph"], envs["one_launch"]
    equal = all(torch.equal(getattr(ra, k).view(torch.uint8), getattr(rb, k).view(torch.uint8)) for k in KEYS)
    equal = equal and all(torch.equal(va.core.t[k].contiguous().view(torch.uint8), vb.core.t[k].contiguous().view(torch.uint8)) for k in STATE)
    us = {k: [t / (runs * T_STEPS) * 1e6 for t in v] for k, v in times.items()}
    med = {k: float(np.median(v)) for k, v in us.items()}
    from pdecontrolgym_amd import build as B_
    return dict(config=dict(B=B, M=va.core.M, T=T_STEPS, control_freq=cf, order=order, simulation_type="outlet"), runs_per_window=runs,
                windows_per_path=repeats, shortest_window_seconds=round(min(min(v) for v in times.values()), 4),
                us_per_env_step={k: dict(median=round(med[k], 3), min=round(min(v), 3), max=round(max(v), 3), windows=[round(x, 3) for x in v])
                                 for k, v in us.items()},
                ratio_two_over_one=round(med["two_launch_graph"] / med["one_launch"], 3),
                ratio_one_over_floor=round(med["one_launch"] / med["open_loop_floor"], 3), bitwise_equal=bool(equal),
                commands_finite=bool(torch.isfinite(rb.actions).all()), device=torch.cuda.get_device_name(0),
                arch=getattr(torch.cuda.get_device_properties(0), "gcnArchName", ""), library_stamp=B_.library_stamp()[:16],
                unit="microseconds per env-step of the whole batch (run() time / 64)")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batch", type=int, default=16384)
    ap.add_argument("--window", type=float, default=0.5, help="least seconds per timed window (any path)")
    ap.add_argument("--repeats", type=int, default=5, help="windows per path, alternating")
    ap.add_argument("--order", choices=("tree", "numpy"), default="tree")
    ap.add_argument("--control-freq", type=int, nargs="*", default=[1, 2])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_traffic_backstep needs a GPU (there is no CPU path)")
    rows = []
    for cf in args.control_freq:
        t0 = time.perf_counter()
        row = measure(args.batch, cf, args.order, args.window, args.repeats)
        row["wall_seconds"] = round(time.perf_counter() - t0, 1)
        rows.append(row)
        print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"tool": "tools/bench_traffic_backstep.py", "rows": rows}, f, indent=1)
            f.write("\n")
    if not all(r["bitwise_equal"] for r in rows):
        sys.exit("the two closed-loop paths differ")


if __name__ == "__main__":
    main()
