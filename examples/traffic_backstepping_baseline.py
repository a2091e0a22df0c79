"""The backstepping baseline of the reference's traffic result table, for B freeways at once on the device.

The reference's notebook (examples/TrafficPDE1D/Backstepping control.ipynb) runs one episode per simulation type -- outlet, inlet,
both -- with one environment, the law in NumPy and a Python loop of 3 840 env-steps.  Here every freeway is one instance of a batch:
the control law and the environment step are two launches per env-step, or, with --one-launch, the whole episode is ONE kernel launch
with the law evaluated inside it (the same bits), and nothing leaves the device until the rewards are summed.

    python examples/traffic_backstepping_baseline.py [--num-envs 8] [--control-freq 1] [--order numpy] [--one-launch]

Prints the episode reward of every simulation type (the notebook's `rew`: the rewards added in step order).  With --order numpy the
commands are the notebook's bit for bit, and the sums are the reference's to the last few bits of the reward norms:
    control_freq 1: outlet / both -373.33321997690774, inlet -1106.0954718055284
    control_freq 2: outlet / both -146.74865984191467, inlet  -913.7939716211005
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))      # run from a source tree without installing

import pde_control_gym  # noqa: E402
from pde_control_gym import DeviceRollout, TrafficBacksteppingController  # noqa: E402
from pde_control_gym.src import TrafficARZReward  # noqa: E402

# the notebook's cell 3
PARAMS = dict(T=240, dt=0.25, X=500, dx=10, v_steady=10, ro_steady=0.12, v_max=40, ro_max=0.16, tau=60)
REFERENCE = {(1, "outlet"): -373.33321997690774, (1, "both"): -373.33321997690774, (1, "inlet"): -1106.0954718055284,
             (2, "outlet"): -146.74865984191467, (2, "both"): -146.74865984191467, (2, "inlet"): -913.7939716211005}


def run(sim, num_envs, control_freq, order, one_launch):
    venv = pde_control_gym.make_vec("PDEControlGym-TrafficPDE1D", num_envs=num_envs, reward_class=TrafficARZReward(),
                                    simulation_type=sim, control_freq=control_freq, **PARAMS)
    venv.reset_tensor()
    controller = TrafficBacksteppingController(venv, order=order)
    steps = int(round(PARAMS["T"] / PARAMS["dt"] / PARAMS["dt"]))      # terminate() compares seconds with T/dt: 3 840 env-steps
    space = venv.action_space                                        # the environment clips to [0.8 qs, 1.2 qs] anyway
    rollout = DeviceRollout(venv, controller, steps, use_graph=False, action_low=float(space.low[0]), action_high=float(space.high[0]),
                            one_launch=True if one_launch else None).run()
    done = (rollout.terminated | rollout.truncated).cpu().numpy().astype(bool)
    rewards = rollout.rewards.cpu().numpy()
    sums = np.zeros(num_envs)
    for b in range(num_envs):
        last = int(np.argmax(done[:, b])) if done[:, b].any() else steps - 1
        total = 0
        for r in rewards[:last + 1, b]:          # the notebook's  rew += rewards
            total += r
        sums[b] = total
    return sums


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--num-envs", type=int, default=8, help="freeways of the batch")
    ap.add_argument("--control-freq", type=int, default=1)
    ap.add_argument("--order", choices=("tree", "numpy"), default="numpy")
    ap.add_argument("--one-launch", action="store_true", help="evaluate the law inside the rollout kernel: one launch per episode")
    args = ap.parse_args()
    for sim in ("outlet", "inlet", "both"):
        sums = run(sim, args.num_envs, args.control_freq, args.order, args.one_launch)
        line = f"{sim:6s} backstepping, {args.num_envs} freeways: episode reward {sums[0]!r}"
        if not np.all(sums == sums[0]):
            line += f" (min {sums.min()!r}, max {sums.max()!r})"
        ref = REFERENCE.get((args.control_freq, sim))
        if ref is not None:
            line += f"   reference {ref!r}, largest relative difference {np.abs(sums / ref - 1).max():.1e}"
        print(line)


if __name__ == "__main__":
    main()
