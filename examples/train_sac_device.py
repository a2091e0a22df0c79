#!/usr/bin/env python3
"""SAC on a batched PDEControlGym environment with NOTHING on the host inside a rollout.

The reference trains every environment family with SAC as well as PPO (examples/transportPDE/transport1Dsac.py,
examples/ReactionDiffusionPDE/reactionDiffusion1Dsac.py: SAC("MlpPolicy", env)).  This is the same algorithm in plain torch on the
batched engine, on the plant of examples/train_ppo_device.py:

  * rollout  -- ``DeviceRollout`` with ``FusedMLP.squashed_gaussian``: per env-step the actor samples
                a = tanh(mu(s) + exp(clip(log_std(s), -20, 2)) * eps) inside the rollout kernel and rescales it to the action box --
                the whole T-step rollout is ONE launch (``one_launch=False``: one policy launch + one env-step launch per step in a
                hipGraph); ``eps`` is drawn ahead with ``normal_()``, no ``mul_``: the standard deviation depends on the state;
  * replay   -- a device tensor filled from the rollout's buffers (the stored action is SB3's scaled action,
                2 (c - lo) / (hi - lo) - 1, recovered from the command c);
  * update   -- twin Q critics, target networks, automatic entropy coefficient; the actor update is ordinary autograd on the same
                ``latent`` / ``mu`` / ``log_std`` modules the rollout evaluates (``FusedMLP`` picks the new weights up at the next
                ``run()``).

    python examples/train_sac_device.py [iterations] [num_envs] [hidden units per layer: 64] [fused_grad: 0] [fused_loss: 0] [fused_opt: 0]
                                        [fused_critic: 0] [terminal_obs: 0] [replay: 0]

``terminal_obs`` (off by default: the histories printed without it are unchanged) stores transitions as SB3's replay buffer does:
``DeviceRollout(terminal_obs=True)`` keeps the terminal observation of every step that ended an episode, ``next`` takes it there and
``obs[t + 1]`` elsewhere, and ``term`` is ``terminated`` alone -- a cut-off episode (``limit_pde_state_size``) keeps its bootstrap.

``fused_loss`` sends the three sample / loss blocks of the update through ``pde_control_gym.SACLoss`` (pdegym_squashed_gaussian_sample
and its backward, pdegym_sac_critic_loss, pdegym_sac_actor_loss): ``head.sample`` writes ``[obs | action]`` and the log-probability in
one launch, ``head.critic`` gathers rewards and terminations by the minibatch's indices inside its kernel, ``result.backward()`` is
one autograd call per step.  What differs from the default path: (1) the critic loss is SB3's ``0.5 * (mse(q1, y) + mse(q2, y))``,
so the critics' gradients (and the ``Q loss`` printed) are HALF those of the default path's ``mse + mse``; (2) the noise is drawn
with ``torch.randn`` ahead of ``head.sample`` (two [batch, 1] draws per update from one call) instead of ``randn_like`` inside
``sample``, so the random stream is consumed differently and the two paths do not reproduce each other's numbers; (3) the gradient
of the log-probability uses ``eps`` directly where autograd differentiates ``((z - mu) / sigma)^2`` through ``z``: equal in exact
arithmetic; (4) actor and entropy-coefficient gradients come from ONE backward call, the two optimisers step after it (the default
path steps the actor before it forms the entropy-coefficient loss, from the same detached ``logp``: the same numbers).

``fused_opt`` replaces the three torch ``Adam`` optimisers and the ``lerp_`` loop over the target critics by three
``pde_control_gym.FusedAdam`` (pdegym_fused_adam, two launches per step): the actor's is attached to the rollout's squashed-Gaussian
wrapper, the critics' to their ``with_grad`` wrappers (with ``fused_grad``) and, through ``attach_target(..., tau)``, to the target
critics, which ``step(polyak=True)`` moves in the same launch -- the weight copies are written by the step, ``refresh()`` finds
nothing to do.  What differs from the default path: (1) the targets move right after the critics' step instead of at the end of the
update (nothing reads them in between: the same numbers); (2) the average is SB3's ``polyak_update`` order
``(1 - tau) * target + tau * param`` in place of ``lerp_``'s ``target + tau * (param - target)``: equal to rounding; (3) the float32
arithmetic is Adam's single-tensor order (include/pdegym.h) where torch's default is the multi-tensor path: equal to rounding.

``fused_critic`` (needs the three switches above) calls the critics the way SB3 does, ``critic(obs, actions)``: the critic step is
``q_fn(o, a)`` on the stored observation and action -- no ``torch.cat`` --, and the actor step samples plain actions (``head.sample``
without ``obs=``) and runs ``q_fn(o, a_pi, params=False)``: each critic's backward is ONE launch that returns the ``[N, 1]`` gradient
of the action alone -- no ``[N, D + 1]`` dx, no dW / db that the next ``zero_grad`` would throw away.  Every number equals the
three-switch path's, bit for bit (``FusedMLP.with_grad``: the two-part rows give the bits of the concatenated ones), and the noise is
drawn by the same two calls in the same order, so the printed history is the same for the same seed.  The critics' ``.grad`` after
the actor step is no longer produced; nothing read it.  The target critics stay the torch modules on ``head.sample``'s block: their
float32 sums are torch's GEMM order, which the kernels' order matches only to rounding -- moving them would change the history.

``replay`` (needs the four fused switches) keeps the replay memory in a ``pde_control_gym.DeviceReplayBuffer`` -- ``store.add()`` in place
of ``fill()``'s seven indexed assignments, ``store.sample(batch)`` in place of the ``randint`` (the same call) -- and runs the SAME update
body WITHOUT gathering observations or actions: a minibatch is its index ``mb`` and the storages, and the first layer of every fused
network reads row ``mb[b]`` in place (``FusedMLP.with_grad(..., index=)``: pdegym_mlp_forward_gather, pdegym_mlp_backward_gather /
_wide_gather): ``q_fn(obs, act, index=mb, tail_indexed=True)`` for the critic step, ``raw_fn(obs, index=mb)`` and
``q_fn(obs, a_pi, index=mb, params=False)`` for the actor step, ``raw_fn(next, index=mb)`` under ``no_grad`` for the target action.  The
one gather that stays is ``next[mb]``: the target critics stay the torch modules on ``head.sample(..., obs=o2)``'s block, for the reason
above.  Every indexed call carries the bits of the call on the gathered rows, the random draws are made by the same calls in the same
order, and the storages hold the same transitions, so the printed history equals the ``fused_critic`` path's, number for number, for the
same seed.
"""
import copy
import math
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pde_control_gym import DeviceReplayBuffer, DeviceRollout, FusedAdam, FusedMLP, SACLoss  # noqa: E402
from train_ppo_device import make_env  # noqa: E402

LOG_STD_MIN, LOG_STD_MAX = -20.0, 2.0


def mlp(sizes):
    mods = []
    for i in range(len(sizes) - 1):
        mods.append(torch.nn.Linear(sizes[i], sizes[i + 1]))
        if i < len(sizes) - 2:
            mods.append(torch.nn.ReLU())
    return torch.nn.Sequential(*mods)


def sample(latent, mu, log_std, obs, raw=None):
    """Reparameterised action in [-1, 1] and its log-probability (the update's own forward pass, under autograd).  ``raw``: the rows
    [mu, log_std] of the fused last layer from ``FusedMLP.with_grad`` instead of the three modules."""
    if raw is None:
        h = latent(obs)
        mean, ls = mu(h), log_std(h)
    else:
        mean, ls = raw[:, :raw.shape[1] // 2], raw[:, raw.shape[1] // 2:]
    ls = ls.clamp(LOG_STD_MIN, LOG_STD_MAX)
    z = mean + ls.exp() * torch.randn_like(mean)
    a = torch.tanh(z)
    logp = (-0.5 * ((z - mean) / ls.exp()) ** 2 - ls - 0.5 * math.log(2 * math.pi)).sum(-1) - torch.log(1 - a * a + 1e-6).sum(-1)
    return a, logp


def main(iterations=30, num_envs=1024, n_steps=32, hidden=64, one_launch=None, quiet=False, updates=8, batch=2048, fused_grad=False,
         fused_loss=False, fused_opt=False, fused_critic=False, terminal_obs=False, replay=False):
    if replay and not fused_critic:
        raise ValueError("replay needs fused_grad, fused_loss, fused_opt and fused_critic")
    if fused_critic and not (fused_grad and fused_loss and fused_opt and hidden <= 256):
        raise ValueError("fused_critic needs fused_grad, fused_loss and fused_opt, and layers of at most 256 units")
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    B, T = num_envs, n_steps
    venv = make_env(B, horizon=64)
    D = venv.reset_tensor().shape[1]
    venv.enable_fused_auto_reset()
    lo, hi = -10.0, 10.0                                 # the plant's max_control_value
    latent = torch.nn.Sequential(torch.nn.Linear(D, hidden), torch.nn.ReLU(), torch.nn.Linear(hidden, hidden), torch.nn.ReLU()).to(dev)
    mu, log_std = torch.nn.Linear(hidden, 1).to(dev), torch.nn.Linear(hidden, 1).to(dev)
    q1, q2 = mlp([D + 1, hidden, hidden, 1]).to(dev), mlp([D + 1, hidden, hidden, 1]).to(dev)
    with torch.no_grad():
        for first in (latent[0], q1[0], q2[0]):
            first.weight.mul_(0.1)                       # observations are O(10)
        mu.weight.mul_(0.01)
        log_std.weight.mul_(0.01)
        log_std.bias.fill_(-1.0)
    q1_t, q2_t = copy.deepcopy(q1).requires_grad_(False), copy.deepcopy(q2).requires_grad_(False)
    log_alpha = torch.zeros(1, device=dev, requires_grad=True)
    actor_params = list(latent.parameters()) + list(mu.parameters()) + list(log_std.parameters())
    opt_actor = torch.optim.Adam(actor_params, lr=3e-4)
    opt_q = torch.optim.Adam(list(q1.parameters()) + list(q2.parameters()), lr=3e-4)
    opt_alpha = torch.optim.Adam([log_alpha], lr=3e-4)
    start = {k: [p.detach().clone() for p in ps] for k, ps in (("actor", actor_params), ("q1", list(q1.parameters())), ("q2", list(q2.parameters())))}
    policy = FusedMLP.squashed_gaussian(latent, mu, log_std, (LOG_STD_MIN, LOG_STD_MAX))
    rollout = DeviceRollout(venv, policy, T, action_low=lo, action_high=hi, action_noise=True, one_launch=one_launch,
                            terminal_obs=bool(terminal_obs))
    # the networks of the update: the modules under torch autograd, or (fused_grad, layers of at most 256 units -- SB3's own 256-256
    # among them) FusedMLP.with_grad -- the critics' gradient with respect to the action column is the dx of pdegym_mlp_backward
    # (layers of at most 64 units) or of pdegym_mlp_backward_wide
    q1_fn, q2_fn, raw_fn = q1, q2, None
    critic_nets = []
    if fused_grad and hidden <= 256:
        critic_nets = [FusedMLP(q1), FusedMLP(q2)]
        q1_fn, q2_fn, raw_fn = critic_nets[0].with_grad, critic_nets[1].with_grad, policy.with_grad
    elif fused_grad and not quiet:
        print(f"fused_grad: layers of {hidden} units are wider than the 256 the fused backward passes take; the update uses torch autograd")
    # the replay buffer: device tensors, a ring of `cap` transitions filled T * B at a time
    cap = max(16 * T * B, batch)
    if replay:      # the class's storages under the names of the dict; add() fills them, the update reads them by index
        store = DeviceReplayBuffer(rollout, cap, lo, hi)
        buf = {"obs": store.observations, "next": store.next_observations, "act": store.actions, "rew": store.rewards, "term": store.dones}
    else:
        buf = {k: torch.zeros(cap, n, device=dev) for k, n in (("obs", D), ("next", D), ("act", 1), ("rew", 1), ("term", 1))}
    head, filled = 0, 0
    gamma, tau, target_entropy = 0.99, 0.005, -1.0
    loss_head = SACLoss(gamma, target_entropy, (LOG_STD_MIN, LOG_STD_MAX)) if fused_loss else None
    q_step = opt_q.step
    if fused_opt:      # the steps write the wrappers' weight copies; the critics' step moves the targets as well
        opt_actor = FusedAdam(actor_params, lr=3e-4).attach(policy)
        opt_q = FusedAdam(list(q1.parameters()) + list(q2.parameters()), lr=3e-4)
        for net in critic_nets:
            opt_q.attach(net)
        opt_q.attach_target(list(q1.parameters()) + list(q2.parameters()), list(q1_t.parameters()) + list(q2_t.parameters()), tau)
        opt_alpha = FusedAdam([log_alpha], lr=3e-4)
        q_step = lambda: opt_q.step(polyak=True)      # noqa: E731

    def raw_of(x, **rows):
        """The rows [mu, log_std] of the actor: the fused last layer of ``with_grad``, or the modules' outputs side by side."""
        if raw_fn is not None:
            return raw_fn(x, **rows)
        h = latent(x)
        return torch.cat([mu(h), log_std(h)], 1)
    def fill(head):
        """The rollout's T * B transitions into the dict's ring at ``head`` (what ``DeviceReplayBuffer.add`` does for ``replay``)."""
        idx = (head + torch.arange(T * B, device=dev)) % cap
        ended = (rollout.terminated | rollout.truncated).reshape(-1, 1)
        buf["obs"][idx] = rollout.obs[:T].reshape(-1, D)
        if terminal_obs:
            # SB3's replay buffer: next_obs of a step that ended an episode is its terminal observation (obs[t + 1] is the new
            # episode's first row), and only a termination cuts the bootstrap -- a cut-off episode bootstraps from that row
            buf["next"][idx] = torch.where(ended.bool(), rollout.terminal_obs.reshape(-1, D), rollout.obs[1:].reshape(-1, D))
            ended = rollout.terminated.reshape(-1, 1)
        else:
            # (after a restart obs[t + 1] is the new episode's first row: the bootstrap of such a transition is cut like a
            # termination's)
            buf["next"][idx] = rollout.obs[1:].reshape(-1, D)
        ended = ended.float()
        buf["act"][idx] = (2.0 * (rollout.actions.reshape(-1, 1) - lo) / (hi - lo) - 1.0).clamp(-1.0, 1.0)
        buf["rew"][idx] = rollout.rewards.reshape(-1, 1)
        buf["term"][idx] = ended
    history = {"q_loss": [], "actor_loss": [], "alpha": [], "mean_reward": [], "mean_norm": []}

    def record(q_loss, actor_loss, it):
        for k, v in (("q_loss", q_loss), ("actor_loss", actor_loss), ("alpha", log_alpha.exp()), ("mean_reward", rollout.rewards.mean()),
                     ("mean_norm", rollout.obs[:T].norm(dim=2).mean())):
            history[k].append(float(v.detach()))
        if not quiet and (it % 5 == 0 or it == iterations - 1):
            print(f"iter {it:3d}  mean reward {history['mean_reward'][-1]:+8.4f}  mean ||u|| {history['mean_norm'][-1]:7.3f}  "
                  f"Q loss {history['q_loss'][-1]:9.4g}  actor loss {history['actor_loss'][-1]:+9.4g}  alpha {history['alpha'][-1]:.3f}")
    t_roll = t_upd = 0.0
    for it in range(iterations):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rollout.action_noise.normal_()                   # eps: standard normal, scaled by the state's sigma inside the kernel
        rollout.run()
        torch.cuda.synchronize()
        t_roll += time.perf_counter() - t0
        t0 = time.perf_counter()
        if replay:
            store.add()
        else:
            fill(head)
        head, filled = (head + T * B) % cap, min(filled + T * B, cap)
        for _ in range(updates):
            mb = store.sample(batch).index if replay else torch.randint(0, filled, (min(batch, filled),), device=dev)
            if loss_head is not None:
                if replay:      # the storages themselves: every fused network reads row mb[b] in place; one gather for the torch targets
                    o, nxt, a, rows, stored = buf["obs"], buf["next"], buf["act"], {"index": mb}, {"index": mb, "tail_indexed": True}
                    o2 = nxt[mb]
                else:
                    o, o2, a = (buf[k][mb] for k in ("obs", "next", "act"))      # (rewards and terminations: gathered in the kernel)
                    nxt, rows, stored = o2, {}, {}
                eps2, eps = torch.randn(2, mb.shape[0], 1, device=dev)
                with torch.no_grad():
                    block2, logp2 = loss_head.sample(raw_of(nxt, **rows), eps2, obs=o2)        # [o2 | a2], log pi(a2 | o2)
                    q1_next, q2_next = q1_t(block2), q2_t(block2)
                if fused_critic:                                                      # critic(obs, actions): the row in two parts
                    q1_now, q2_now = q1_fn(o, a, **stored), q2_fn(o, a, **stored)
                else:
                    oa = torch.cat([o, a], 1)
                    q1_now, q2_now = q1_fn(oa), q2_fn(oa)
                result = loss_head.critic(q1_now, q2_now, q1_next, q2_next, logp2, buf["rew"], buf["term"], log_alpha, index=mb)
                opt_q.zero_grad(set_to_none=True)
                result.backward()
                q_step()
                q_loss = result.critic_loss
                if fused_critic:      # plain actions; one backward launch per critic, for the action's gradient alone
                    a_pi, logp = loss_head.sample(raw_of(o, **rows), eps)
                    result = loss_head.actor(q1_fn(o, a_pi, params=False, **rows), q2_fn(o, a_pi, params=False, **rows), logp, log_alpha)
                else:
                    block, logp = loss_head.sample(raw_of(o), eps, obs=o)             # [o | a_pi]: the critics' input, no cat
                    result = loss_head.actor(q1_fn(block), q2_fn(block), logp, log_alpha)
                opt_actor.zero_grad(set_to_none=True)
                opt_alpha.zero_grad(set_to_none=True)
                result.backward()
                opt_actor.step()
                opt_alpha.step()
                actor_loss = result.actor_loss
                if fused_opt:
                    continue
                with torch.no_grad():
                    for net, tgt in ((q1, q1_t), (q2, q2_t)):
                        for p, pt in zip(net.parameters(), tgt.parameters()):
                            pt.lerp_(p, tau)
                continue
            o, o2, a, r, d = (buf[k][mb] for k in ("obs", "next", "act", "rew", "term"))
            alpha = log_alpha.exp().detach()
            with torch.no_grad():
                a2, logp2 = sample(latent, mu, log_std, o2)
                q_next = torch.min(q1_t(torch.cat([o2, a2], 1)), q2_t(torch.cat([o2, a2], 1))) - alpha * logp2.unsqueeze(1)
                target = r + gamma * (1.0 - d) * q_next
            oa = torch.cat([o, a], 1)
            q_loss = (q1_fn(oa) - target).pow(2).mean() + (q2_fn(oa) - target).pow(2).mean()
            opt_q.zero_grad(set_to_none=True)
            q_loss.backward()
            q_step()
            a_pi, logp = sample(latent, mu, log_std, o, None if raw_fn is None else raw_fn(o))
            oa_pi = torch.cat([o, a_pi], 1)
            actor_loss = (alpha * logp.unsqueeze(1) - torch.min(q1_fn(oa_pi), q2_fn(oa_pi))).mean()
            opt_actor.zero_grad(set_to_none=True)
            actor_loss.backward()
            opt_actor.step()
            alpha_loss = -(log_alpha * (logp.detach() + target_entropy).mean())
            opt_alpha.zero_grad(set_to_none=True)
            alpha_loss.backward()
            opt_alpha.step()
            if fused_opt:
                continue
            with torch.no_grad():
                for net, tgt in ((q1, q1_t), (q2, q2_t)):
                    for p, pt in zip(net.parameters(), tgt.parameters()):
                        pt.lerp_(p, tau)
        torch.cuda.synchronize()
        t_upd += time.perf_counter() - t0
        record(q_loss, actor_loss, it)
    now = {"actor": actor_params, "q1": list(q1.parameters()), "q2": list(q2.parameters())}
    history["moved"] = {k: all(not torch.equal(p.detach(), s) for p, s in zip(now[k], start[k])) for k in now}
    history["one_launch"] = rollout.one_launch
    if not quiet:
        print(f"{iterations} iterations x {T} steps x {B} envs: rollouts {t_roll:.2f} s ({iterations * T * B / t_roll:.3g} env-steps/s incl. policy, "
              f"one launch: {rollout.one_launch}), updates {t_upd:.2f} s")
    return history


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 30, int(sys.argv[2]) if len(sys.argv) > 2 else 1024,
         hidden=int(sys.argv[3]) if len(sys.argv) > 3 else 64, fused_grad=bool(int(sys.argv[4])) if len(sys.argv) > 4 else False,
         fused_loss=bool(int(sys.argv[5])) if len(sys.argv) > 5 else False,
         fused_opt=bool(int(sys.argv[6])) if len(sys.argv) > 6 else False,
         fused_critic=bool(int(sys.argv[7])) if len(sys.argv) > 7 else False,
         terminal_obs=bool(int(sys.argv[8])) if len(sys.argv) > 8 else False,
         replay=bool(int(sys.argv[9])) if len(sys.argv) > 9 else False)
