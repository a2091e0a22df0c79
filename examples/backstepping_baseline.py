"""The backstepping baseline column of the reference's result tables, for B instances at once on the device.

The reference runs examples/transportPDE/transport1Dbackstepping.py and examples/reactionDiffusionPDE/reactionDiffusion1DBackstepping.py
once per episode (one environment, NumPy gains, a Python dot product per step) and averages 50 episodes with random initial
conditions.  Here every episode is one instance of a batch: the gains of all instances are computed by one kernel launch, the
control law and the environment step are two launches per env-step -- or, with --one-launch, the whole episode is ONE kernel launch
with the law evaluated inside it (the same bits) -- and nothing leaves the device until the rewards are summed.

    python examples/backstepping_baseline.py [--episodes 50] [--gamma-spread 0.0] [--order tree] [--one-launch]

Prints the mean episode reward per family.  The published means were drawn with other random initial conditions, so the number is
printed, not compared.
"""
import argparse

import numpy as np
import torch

import pde_control_gym
from pde_control_gym import BacksteppingController, DeviceRollout
from pde_control_gym.src import TunedReward1D

FAMILIES = {
    # id, T, dt, dx, control_sample_rate, gamma, amplitude, ghost node
    "transport": ("PDEControlGym-TransportPDE1D", 5, 1e-4, 1e-2, 0.1, 7.35, 5.0, 0),
    "parabolic": ("PDEControlGym-ReactionDiffusionPDE1D", 1, 1e-5, 5e-3, 1e-3, 8.0, 50.0, 1),
}


def chebyshev(x, gamma, amp):
    """solveBetaFunction of the example scripts, one row per gamma."""
    return (amp * np.cos(np.asarray(gamma)[:, None] * np.arccos(x)[None])).astype(np.float32)


def run(kind, episodes, spread, order, seed, one_launch=False):
    env_id, T, dt, dx, rate, gamma0, amp, ghost = FAMILIES[kind]
    rng = np.random.default_rng(seed)
    nx = int(round(1 / dx))
    n = nx + ghost
    gamma = gamma0 + spread * rng.uniform(-1, 1, episodes)
    beta = chebyshev(np.linspace(0, 1, n), gamma, amp)                 # the plant's grid
    theta = chebyshev(np.linspace(dx, 1, n), gamma, amp)               # the controller's grid (the scripts' `spatial`)
    init = (rng.uniform(1, 10, (episodes, 1)) * np.ones((1, n))).astype(np.float32)
    params = dict(T=T, dt=dt, X=1, dx=dx, control_sample_rate=rate, reward_class=TunedReward1D(int(round(T / dt)), -1e3, 3e2),
                  normalize=False, sensing_loc="full", control_type="Dirchilet", sensing_type=None, limit_pde_state_size=True,
                  max_state_value=1e10, max_control_value=20, batched_reset_func=lambda idx, nx: (init[idx], beta[idx]))
    venv = pde_control_gym.make_vec(env_id, num_envs=episodes, **params)
    venv.reset_tensor()
    controller = BacksteppingController(kind, theta, dx, order=order).attach(venv)
    steps = int(round(T / rate))
    # the scripts hand the raw command to env.step: no action box
    rollout = DeviceRollout(venv, controller, steps, use_graph=False, action_low=-float("inf"), action_high=float("inf"),
                            one_launch=True if one_launch else None).run()
    done = (rollout.terminated | rollout.truncated).bool()
    alive = torch.cat([torch.ones_like(done[:1]), ~done[:-1].cumsum(0).bool()])     # steps up to and including the episode's last
    returns = (rollout.rewards.double() * alive).sum(0)
    return float(returns.mean()), float(returns.std())


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--episodes", type=int, default=50, help="instances of the batch = episodes averaged")
    ap.add_argument("--gamma-spread", type=float, default=0.0, help="each instance draws gamma within +- this of the scripts' value")
    ap.add_argument("--order", choices=("tree", "ordered"), default="tree")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--one-launch", action="store_true", help="evaluate the law inside the rollout kernel: one launch per episode")
    args = ap.parse_args()
    for kind in FAMILIES:
        mean, std = run(kind, args.episodes, args.gamma_spread, args.order, args.seed, args.one_launch)
        print(f"{kind:10s} backstepping, {args.episodes} episodes: mean episode reward {mean:.2f} (std {std:.2f})")


if __name__ == "__main__":
    main()
