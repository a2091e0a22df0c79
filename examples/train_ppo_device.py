#!/usr/bin/env python3
"""PPO on a batched PDEControlGym environment with NOTHING on the host inside a rollout.

The reference trains its RL controllers with SB3 on one environment per Python call
(examples/ReactionDiffusionPDE/..., examples/transportPDE/transport1Dppo.py:77-90: PPO("MlpPolicy", env)).  This is the same
algorithm in plain torch on the batched engine:

  * rollout  -- ``DeviceRollout``: the whole T-step rollout is ONE kernel launch (``pdegym_parabolic_rollout``: per env-step
                the actor mean is evaluated inside the kernel from weights held in LDS, exploration noise added, the command
                clamped and stored, then the env-step with fused auto-reset; layers of 65 .. 256 units -- ``hidden`` below --
                are evaluated in the same kernel by the 16 waves of a workgroup together on the matrix cores; anything else
                falls back to one ``pdegym_mlp_forward`` launch + one env-step launch per step inside a hipGraph);
  * targets  -- ``DeviceRolloutBuffer``: the critic on all T + 1 observation slots in one batched call, then GAE(lambda)
                advantages, returns and the statistics of the episodes that ended inside the buffer in ONE launch
                (``pdegym_gae``: SB3's ``compute_returns_and_advantage`` bit for bit) instead of a Python loop over T;
  * update   -- ordinary torch autograd on the same ``torch.nn.Sequential`` the rollout evaluates (``FusedMLP`` picks the new
                weights up at the next ``run()``); with ``fused_grad`` and layers of at most 256 units, actor and critic go through
                ``FusedMLP.with_grad`` instead: one forward launch and a three-launch backward (``pdegym_mlp_backward``, or
                ``pdegym_mlp_backward_wide`` for layers of more than 64 units) per network
                and minibatch that fill the same Parameters' ``.grad``, so the optimiser and the gradient clipping stay as they are;
                with ``fused_loss`` everything between the networks' outputs and their backward passes is ``PPOLoss`` (at most three
                launches, ``pdegym_ppo_loss``: the gathers by the minibatch's indices, log-probability, clipped surrogate, value and
                entropy terms and their gradients) and ``result.backward()``.  The loss is the same one (``vf_coef = 0.25`` is this
                file's ``0.5 * (0.5 * mse)``, ``ent_coef = 1e-3`` its ``-1e-3 * log_std.sum()``), with ONE difference: under the
                switch the advantages are normalised per minibatch, as SB3's ``PPO.train`` does, not once over the whole buffer.
                With ``fused_opt`` the tail of a minibatch step -- ``clip_grad_norm_`` and ``Adam`` over 13 tensors, then the
                ``refresh()`` of the blocked weight copies at the next forward -- is ONE ``FusedAdam.step()`` (``pdegym_fused_adam``,
                two launches) that writes the copies of the attached ``FusedMLP`` wrappers itself.  What differs from the default
                path: (1) the global norm is taken over ALL of the optimiser's tensors, ``log_std`` included (the default path clips
                actor and critic and leaves ``log_std`` out), so the clip coefficient differs whenever ``log_std``'s gradient is not
                negligible; (2) the gradients themselves are not scaled in place, only the update sees the scaled values; (3) the
                float32 arithmetic is Adam's single-tensor order with the norm summed in float64 (include/pdegym.h), where torch's
                default is the multi-tensor path: equal to rounding.
                ``graph_update`` (needs the three switches above) captures one minibatch step -- gather, both ``with_grad``
                forwards, ``PPOLoss``, ``backward()`` and ``FusedAdam.step()`` -- into ONE ``torch.cuda.graph`` after the first step
                has run eagerly, and replays it for every later minibatch of the run: the minibatch's indices, the actions and the
                old log-probabilities are copied into static tensors outside the graph (``randperm`` stays outside as well), the
                attached wrappers need no ``refresh()`` and the optimiser no host work.  The numbers are those of ``fused_opt``.

``gather`` (off by default; needs ``fused_grad`` and ``fused_loss``): the minibatch's observations are not gathered -- ``actor_fn(o_f,
index=mb)`` and ``critic_fn(o_f, index=mb)`` read row ``mb[b]`` of the rollout's own ``obs`` in place (``FusedMLP.with_grad(..., index=)``:
pdegym_mlp_forward_gather, pdegym_mlp_backward_gather / _wide_gather), in the eager step and in the ``graph_update`` step.  Every indexed
call carries the bits of the call on ``o_f[mb]``: the history is identical.

``bootstrap`` (off by default: the histories printed without it are unchanged): an episode that is cut off (``limit_pde_state_size``:
``truncated and not terminated``) is handled as SB3 handles ``infos[i]["TimeLimit.truncated"]`` -- ``DeviceRollout(terminal_obs=True)``
keeps the terminal observation of every step, and ``DeviceRolloutBuffer.compute`` adds ``gamma * V(terminal observation)`` to that
step's reward.  Without it every cut-off is treated as a termination.

The plant is the reference's unstable reaction-diffusion benchmark u_t = u_xx + beta(x) u with boundary actuation
(ReactionDiffusionPDE1D, Dirichlet control at x = 1).  Uncontrolled, ||u|| grows; the printed mean ||u|| over an episode falls
as the policy learns to damp it.

    python examples/train_ppo_device.py [iterations] [num_envs] [hidden units per layer: 64] [fused_grad: 0] [fused_loss: 0] [fused_opt: 0] [graph_update: 0] [bootstrap: 0] [gather: 0]
"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pde_control_gym  # noqa: E402
from pde_control_gym import DeviceRollout, DeviceRolloutBuffer, FusedAdam, FusedMLP, PPOLoss  # noqa: E402
from pde_control_gym.src import TunedReward1D  # noqa: E402


def make_env(B, nx=64, S=25, horizon=64):
    dx = 1.0 / nx
    dt = 0.25 * dx * dx
    beta = np.full(nx + 1, 12.0, np.float32)            # lambda = 12 > pi^2: the open loop is unstable
    rng = np.random.default_rng(0)

    def batched_reset(idx, n):
        amp = rng.uniform(1.0, 5.0, (len(idx), 1)).astype(np.float32)
        x = np.linspace(0, 1, n + 1, dtype=np.float32)[None, :]
        return amp * np.sin(np.pi * x).astype(np.float32) + amp * 0.2, np.tile(beta, (len(idx), 1))

    kw = {"T": horizon * S * dt, "dt": dt, "X": 1, "dx": dx, "reward_class": TunedReward1D(horizon * S, -1e-2, 20.0),
          "normalize": True, "sensing_loc": "full", "control_type": "Dirchilet", "sensing_type": None, "sensing_noise_func": None,
          "limit_pde_state_size": True, "max_state_value": 1e3, "max_control_value": 10.0, "control_sample_rate": S * dt,
          "batched_reset_func": batched_reset}
    return pde_control_gym.make_vec("PDEControlGym-ReactionDiffusionPDE1D", num_envs=B, **kw)


def mlp(sizes, out_tanh=False):
    mods = []
    for i in range(len(sizes) - 1):
        mods.append(torch.nn.Linear(sizes[i], sizes[i + 1]))
        if i < len(sizes) - 2 or out_tanh:
            mods.append(torch.nn.Tanh())
    return torch.nn.Sequential(*mods)


nmb_of_update = 4      # minibatches per epoch


def main(iterations=30, B=2048, T=64, quiet=False, hidden=64, fused_grad=False, fused_loss=False, fused_opt=False, graph_update=False,
         bootstrap=False, gather=False):
    if gather and not (fused_grad and fused_loss and hidden <= 256):
        raise ValueError("gather needs fused_grad and fused_loss, and layers of at most 256 units")
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    venv = make_env(B, horizon=T)        # one rollout = one episode of every environment
    obs0 = venv.reset_tensor()
    venv.enable_fused_auto_reset()
    D = obs0.shape[1]
    # mean of a Gaussian policy: SB3's MlpPolicy shape (64-64), or e.g. hidden = 256 for net_arch [256, 256] -- layers of more
    # than 64 units are evaluated inside the same rollout kernel by the workgroup's 16 waves together (matrix cores)
    actor = mlp([D, hidden, hidden, 1]).to(dev)
    critic = mlp([D, hidden, hidden, 1]).to(dev)
    with torch.no_grad():
        actor[0].weight.mul_(0.1)                        # observations are O(10)
        critic[0].weight.mul_(0.1)
        actor[-1].weight.mul_(0.01)
    log_std = torch.nn.Parameter(torch.full((1,), -0.7, device=dev))
    opt = torch.optim.Adam(list(actor.parameters()) + list(critic.parameters()) + [log_std], lr=1e-3)
    policy = FusedMLP(actor)
    rollout = DeviceRollout(venv, policy, T, action_noise=True, terminal_obs=bool(bootstrap))
    # the networks of the update: the modules themselves under torch autograd, or their fused forward + backward launches
    actor_fn, critic_fn = actor, critic
    fused_nets = [policy]
    if fused_grad and hidden <= 256:
        fused_nets.append(FusedMLP(critic))
        actor_fn, critic_fn = policy.with_grad, fused_nets[1].with_grad
    elif fused_grad and not quiet:
        print(f"fused_grad: layers of {hidden} units are wider than the 256 the fused backward passes take; the update uses torch autograd")
    clipped = list(actor.parameters()) + list(critic.parameters())
    if fused_opt:      # one launch pair per minibatch: clip over all 13 tensors, Adam, the blocked copies of the attached wrappers
        opt = FusedAdam(clipped + [log_std], lr=1e-3, max_grad_norm=0.5)
        for net in fused_nets:
            opt.attach(net)
    graph = step_fn = None
    if graph_update:
        if not (fused_grad and fused_loss and fused_opt and hidden <= 256) or (T * B) % nmb_of_update:
            raise ValueError("graph_update needs fused_grad, fused_loss and fused_opt, layers of at most 256 units and T * B divisible by 4")
        static = {"mb": torch.zeros(T * B // nmb_of_update, dtype=torch.int64, device=dev), "a": torch.empty(T * B, device=dev),
                  "lp": torch.empty(T * B, device=dev)}
    start = {"actor": [p.detach().clone() for p in actor.parameters()], "critic": [p.detach().clone() for p in critic.parameters()]}
    gamma, lam, clip, epochs, nmb = 0.99, 0.95, 0.2, 6, nmb_of_update
    buffer = DeviceRolloutBuffer(rollout, gamma=gamma, gae_lambda=lam)      # (bootstrap: boot = V(terminal rows) where cut off)
    head = PPOLoss(clip_range=clip, ent_coef=1e-3, vf_coef=0.25, normalize_advantage=True) if fused_loss else None
    history = []
    t_roll = t_upd = 0.0
    for it in range(iterations):
        # ---- rollout: one graph replay, no host work per step --------------------------------------------------------
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        std_old = log_std.detach().exp()
        rollout.action_noise.normal_().mul_(std_old)
        rollout.run()
        torch.cuda.synchronize()
        t_roll += time.perf_counter() - t0
        t0 = time.perf_counter()
        obs = rollout.obs
        buffer.compute(critic=critic)                     # values of the T + 1 slots, then GAE: an episode end cuts the bootstrap
        with torch.no_grad():
            mean_old = actor(obs[:T].reshape(-1, D)).reshape(T, B)
            a_raw = mean_old + rollout.action_noise       # the sample before the clamp: what the log-probabilities refer to
            if fused_loss:                                # through the head's own device function: the first epoch sees ratio == 1
                logp_old = head.log_prob(mean_old.reshape(-1, 1), log_std, a_raw.reshape(-1, 1)).reshape(T, B)
            else:
                logp_old = -0.5 * ((a_raw - mean_old) / std_old) ** 2 - log_std.detach()
        flat = lambda x: x.reshape(T * B, *x.shape[2:])   # noqa: E731
        batch = buffer.flat()
        o_f, a_f, lp_f, adv_f, ret_f = batch.observations, flat(a_raw), flat(logp_old), batch.advantages, batch.returns
        if not fused_loss:
            adv_f = (adv_f - adv_f.mean()) / (adv_f.std() + 1e-8)
        if graph_update:
            static["a"].copy_(a_f)
            static["lp"].copy_(lp_f)
            if step_fn is None:
                def step_fn(o_f=o_f, adv_f=adv_f, ret_f=ret_f):      # (views of the rollout's and the buffer's own tensors: fixed addresses)
                    if gather:      # (the address of static["mb"] is what the graph holds: the indices are copied into it)
                        mean, value = actor_fn(o_f, index=static["mb"]), critic_fn(o_f, index=static["mb"])
                    else:
                        obs_mb = o_f[static["mb"]]
                        mean, value = actor_fn(obs_mb), critic_fn(obs_mb)
                    result = head(mean, log_std, value, static["a"], static["lp"], adv_f, ret_f, index=static["mb"])
                    result.backward()
                    opt.step()
        for _ in range(epochs):
            perm = torch.randperm(T * B, device=dev)
            for mb in perm.chunk(nmb):
                if graph_update:
                    static["mb"].copy_(mb)
                    if graph is not None:      # (the captured backward WRITES the gradients it allocated: nothing to zero)
                        graph.replay()
                        continue
                    opt.zero_grad(set_to_none=True)
                    if "warm" not in static:      # the very first step runs eagerly: it allocates what the graph reuses
                        step_fn()
                        static["warm"] = True
                    else:
                        torch.cuda.synchronize()
                        graph = torch.cuda.CUDAGraph()
                        with torch.cuda.graph(graph):
                            step_fn()
                        graph.replay()
                    continue
                if fused_loss:
                    if gather:
                        mean, value = actor_fn(o_f, index=mb), critic_fn(o_f, index=mb)
                    else:
                        obs_mb = o_f[mb]
                        mean, value = actor_fn(obs_mb), critic_fn(obs_mb)
                    result = head(mean, log_std, value, a_f, lp_f, adv_f, ret_f, index=mb)
                    opt.zero_grad(set_to_none=True)
                    result.backward()
                    if not fused_opt:
                        torch.nn.utils.clip_grad_norm_(clipped, 0.5)
                    opt.step()
                    continue
                mean = actor_fn(o_f[mb]).squeeze(-1)
                logp = -0.5 * ((a_f[mb] - mean) / log_std.exp()) ** 2 - log_std
                ratio = (logp - lp_f[mb]).exp()
                pg = -torch.min(ratio * adv_f[mb], ratio.clamp(1 - clip, 1 + clip) * adv_f[mb]).mean()
                vloss = 0.5 * (critic_fn(o_f[mb]).squeeze(-1) - ret_f[mb]).pow(2).mean()
                loss = pg + 0.5 * vloss - 1e-3 * log_std.sum()
                opt.zero_grad(set_to_none=True)
                loss.backward()
                if not fused_opt:
                    torch.nn.utils.clip_grad_norm_(clipped, 0.5)
                opt.step()
        torch.cuda.synchronize()
        t_upd += time.perf_counter() - t0
        # mean return of the episodes that ENDED in this rollout (auto-reset ends them anywhere in the buffer; one that was cut off
        # early restarts at once and runs on into the next rollout, carried by the buffer's accumulators)
        stats = {"iter": it, "episode_return": buffer.finished_episodes()[1].item(), "mean_norm": obs[:T].norm(dim=2).mean().item(),
                 "truncated_frac": rollout.truncated.float().mean().item() * T, "std": log_std.exp().item()}
        history.append(stats)
        if fused_opt and it == iterations - 1:      # whether the fused step reached every tensor of either network
            stats["moved"] = {k: all(not torch.equal(p.detach(), s) for p, s in zip(net.parameters(), start[k]))
                              for k, net in (("actor", actor), ("critic", critic))}
        if not quiet and (it % 5 == 0 or it == iterations - 1):
            print(f"iter {it:3d}  episode return {stats['episode_return']:+8.3f}  mean ||u|| over the episode {stats['mean_norm']:7.3f}  "
                  f"episodes cut off per env {stats['truncated_frac']:.3f}  policy std {stats['std']:.3f}")
    if not quiet:
        print(f"{iterations} iterations x {T} steps x {B} envs: rollouts {t_roll:.2f} s ({iterations * T * B / t_roll:.3g} env-steps/s incl. policy), "
              f"updates {t_upd:.2f} s")
    return history


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 30, int(sys.argv[2]) if len(sys.argv) > 2 else 2048,
         hidden=int(sys.argv[3]) if len(sys.argv) > 3 else 64, fused_grad=bool(int(sys.argv[4])) if len(sys.argv) > 4 else False,
         fused_loss=bool(int(sys.argv[5])) if len(sys.argv) > 5 else False,
         fused_opt=bool(int(sys.argv[6])) if len(sys.argv) > 6 else False,
         graph_update=bool(int(sys.argv[7])) if len(sys.argv) > 7 else False,
         bootstrap=bool(int(sys.argv[8])) if len(sys.argv) > 8 else False,
         gather=bool(int(sys.argv[9])) if len(sys.argv) > 9 else False)
