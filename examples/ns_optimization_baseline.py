"""The adjoint-optimisation baseline of the reference's NavierStokes2D result table, for B instances at once on the device.

The reference runs examples/NavierStokes/NS2Doptimization.py for one environment: 199 forward steps, 198 backward iterations of
NumPy stencils with a 2000-sweep ``solve_pressure`` each, a command read off the adjoint, a replay.  Here every instance of a batch
starts from its own random constant fields (the script's ``getInitialCondition``); the two rollouts are one launch each and the
whole backward march is one more.

    python examples/ns_optimization_baseline.py [--episodes 8] [--target target.npz] [--out NS_optimization.npz]

``--target``: a ``target.npz`` of the reference's layout (keys ``u``, ``v``: [nt, 21, 21]).  Without it the target is the plant's
own response to the commands 4 - 0.01 t from rest.  Prints the mean reward sum before and after the optimisation and writes the
first instance's replay in the script's result layout (``export.save_ns_optimization``).
"""
import argparse

import numpy as np
import torch

import pde_control_gym
from pde_control_gym import NSAdjointOptimizer, export
from pde_control_gym.src import NSReward

BC = {"upper": ["Controllable", "Dirchilet"], "lower": ["Dirchilet", "Dirchilet"], "left": ["Dirchilet", "Dirchilet"],
      "right": ["Dirchilet", "Dirchilet"]}
STEPS = 199                                        # the script's T (:65)


def make(num_envs, U_ref):
    params = dict(T=0.2, dt=1e-3, X=1, dx=0.05, Y=1, dy=0.05, action_dim=1, reward_class=NSReward(0.1), normalize=False,
                  reset_init_condition_func=lambda X: (np.zeros_like(X),) * 3, boundary_condition=BC, U_ref=U_ref,
                  action_ref=2.0 * np.ones(1000), dtype="float64")
    return pde_control_gym.make_vec("PDEControlGym-NavierStokes2D", num_envs=num_envs, **params)


def own_target():
    """[200, 21, 21, 2]: the plant from rest under 4 - 0.01 t."""
    core = make(1, np.zeros((200, 21, 21, 2))).core
    obs = torch.zeros(STEPS + 1, 1, 21, 21, 2, dtype=torch.float64, device=core.device)
    obs[0].copy_(core.reset(*(np.zeros((21, 21)),) * 3))
    a = (4.0 - 0.01 * torch.arange(1, STEPS + 1, dtype=torch.float64, device=core.device)).reshape(STEPS, 1, 1)
    core.rollout(obs, a.contiguous(), torch.zeros(STEPS, 1, dtype=torch.float64, device=core.device),
                 torch.zeros(STEPS, 1, dtype=torch.uint8, device=core.device))
    return obs[:, 0].cpu().numpy()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--episodes", type=int, default=8, help="instances of the batch")
    ap.add_argument("--target", default=None, help="target.npz of the reference's layout")
    ap.add_argument("--out", default="NS_optimization.npz")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    U_ref = export.load_ns_target(args.target) if args.target else own_target()
    B = args.episodes
    rng = np.random.default_rng(args.seed)
    ones = np.ones((B, 21, 21))
    u0, v0, p0 = (rng.uniform(-5, 5, (B, 1, 1)) * ones for _ in range(3))          # getInitialCondition (:14-18)
    actions0 = rng.uniform(2, 4, (STEPS, B))                                       # :74
    venv = make(B, U_ref)
    out = NSAdjointOptimizer(venv, a_nom=2.0).optimize(u0, v0, p0, actions0)
    print(f"reward sum over {STEPS} steps, mean of {B} instances: {float(out['reward_before'].mean()):.4f} under random commands, "
          f"{float(out['reward_after'].mean()):.4f} under the optimised ones")
    export.save_ns_optimization(args.out, out["obs"][:, 0].cpu().numpy(), U_ref[..., 0], U_ref[..., 1], out["actions"][:, 0, 0].cpu().numpy())
    print("wrote", args.out)


if __name__ == "__main__":
    main()
