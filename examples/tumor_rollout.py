"""TherapyWrapper(BrainTumor1D) rollouts for B patients with the policy inside ONE launch per rollout.

The reference trains one patient at a time (examples/BrainTumor1D: ``PPO("MlpPolicy", TherapyWrapper(gym.make("PDEControlGym-BrainTumor1D",
**params)))``: one Python call per treatment day, growth and post-therapy loops in Python).  Here B patients are a batch: the open-loop
benchmark and the reset through the growth stage are one launch each, and ``DeviceRollout(venv, policy, T, one_launch=True)`` runs
T wrapper steps -- a 64-64 tanh actor with exploration noise, treatment days, weekend days, post-therapy runs, restarts through
the growth stage -- in ONE kernel launch (pdegym_tumor_rollout); nothing leaves the device until the episode rewards are summed.

    python examples/tumor_rollout.py [--num-envs 4096] [--steps 32] [--rollouts 8] [--weekends] [--step-by-step]

Prints the mean reward of the episodes that finished (an episode's reward: the rewards of its wrapper steps added up; the last one
is the survival gain over the untreated benchmark, in days).  --step-by-step takes today's path instead (one policy launch and the
launches of ``step_tensor`` per step, replayed as a hipGraph): the same numbers with a 256-unit actor, trajectories that part in the
last float32 bits with the 64-64 one (another summation order inside the launch).
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))      # run from a source tree without installing

import torch  # noqa: E402

import pde_control_gym  # noqa: E402
from pde_control_gym import DeviceRollout, FusedMLP  # noqa: E402
from pde_control_gym.src import BrainTumorReward  # noqa: E402

# the parameters of the reference's BrainTumor1D example
PARAMS = dict(T=600, X=200, dt=1, dx=1, normalize=True, dosage_termination_threshold=0.1, t1_detection_threshold=0.8,
              t2_detection_threshold=0.16, D=0.2, rho=0.03, alpha=0.04, alpha_beta_ratio=10, k=1e5, t1_detection_radius=15,
              t1_death_radius=35, total_dosage=61.2, verbose=False)


def tumor_ic(X, nx):
    xs = np.linspace(0, X, nx)
    return 0.8 * 1e5 * np.exp(-0.25 * (xs ** 2))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--num-envs", type=int, default=4096, help="patients of the batch")
    ap.add_argument("--steps", type=int, default=32, help="wrapper steps per rollout (= per launch)")
    ap.add_argument("--rollouts", type=int, default=8)
    ap.add_argument("--weekends", action="store_true", help="two untreated days after five consecutive treatment days")
    ap.add_argument("--noise", type=float, default=0.03, help="standard deviation of the exploration noise")
    ap.add_argument("--step-by-step", action="store_true", help="today's path: policy launch + step_tensor launches per step, as a hipGraph")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("examples/tumor_rollout.py needs a GPU (there is no CPU path)")
    B = args.num_envs
    venv = pde_control_gym.make_vec("PDEControlGym-BrainTumor1D", num_envs=B, weekends=args.weekends, reward_class=BrainTumorReward(),
                                    reset_init_condition_func=tumor_ic, **PARAMS)
    tb = venv.benchmark()                       # untreated survival of every patient, one launch; ends with reset_tensor()
    print(f"{B} patients, untreated survival {float(tb.mean()):.0f} days, first treatment day {int(venv.core.t['time_index'][0])}")
    torch.manual_seed(0)
    net = torch.nn.Sequential(torch.nn.Linear(venv.core.nx, 64), torch.nn.Tanh(), torch.nn.Linear(64, 64), torch.nn.Tanh(),
                              torch.nn.Linear(64, 1), torch.nn.Tanh()).cuda()
    with torch.no_grad():
        net[0].weight.mul_(1e-5)                # cell densities are O(1e5)
        net[4].bias.fill_(0.05)                 # an untrained actor that prescribes about 5 % of the total dose per day
    policy = FusedMLP(net)
    ro = DeviceRollout(venv, policy, args.steps, use_graph=True, action_low=0.0, action_high=1.0, action_noise=True,
                       one_launch=None if args.step_by_step else True)
    print("path:", "ONE launch per rollout (pdegym_tumor_rollout)" if ro.one_launch else "policy + step_tensor launches per step (hipGraph)")
    running = torch.zeros(B, dtype=torch.float64, device="cuda")
    total, episodes = torch.zeros((), dtype=torch.float64, device="cuda"), torch.zeros((), dtype=torch.int64, device="cuda")
    t0 = None
    for k in range(args.rollouts):
        ro.action_noise.normal_().mul_(args.noise)
        ro.run()
        if t0 is None:                          # (the first run captures the graph)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        done = (ro.terminated | ro.truncated).bool()
        for t in range(args.steps):             # episode sums, on the device
            running += ro.rewards[t]
            total += running[done[t]].sum()
            episodes += done[t].sum()
            running[done[t]] = 0
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    n = int(episodes)
    print(f"{args.rollouts} rollouts of {args.steps} wrapper steps: {n} episodes finished, mean episode reward "
          f"{float(total) / max(n, 1):.3f}; treatment calls {int(venv.treatment_calls.sum())}, soft-constraint violations "
          f"{int(venv.soft_constraint_violations.sum())}")
    if args.rollouts > 1:
        print(f"{(args.rollouts - 1) * args.steps * B / dt:.3g} wrapper steps/s after the first rollout (host-side reward sums included)")


if __name__ == "__main__":
    main()
