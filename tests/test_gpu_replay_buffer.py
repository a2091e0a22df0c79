"""``pde_control_gym.DeviceReplayBuffer`` on a real ``DeviceRollout`` on the device, and the two training examples with their
rows-by-index switches (examples/train_sac_device.py ``replay``, examples/train_ppo_device.py ``gather``).

The buffer: ReactionDiffusionPDE1D on nx = 16 (17 nodes), B = 8, T = 4, capacity 48 -- three ``run()`` + ``add()``: the second wraps
after 16 of its 32 transitions, the third lands on slots 16 .. 47 -- against the NumPy restatement of tests/replay_buffer_reference.py, with and without terminal observations; then
``run()`` + ``add()`` captured into one ``torch.cuda.graph``, whose replays must leave what the eager calls leave.  The environment is tests/terminal_obs_cases.py's: episodes
end inside the window for both reasons, which every test asserts from the flags before it compares anything.

The examples: the switches change where a row is read from, not a bit of what is computed, so the histories are compared with ``==``."""
import importlib.util
import os
import sys

import numpy as np
import pytest

from tests import replay_buffer_reference as RR
from tests import terminal_obs_cases as K

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NX, B, T, CAP = 16, 8, 4, 48
LO, HI = -1.5, 2.25


def _net(sizes, seed):
    g = torch.Generator().manual_seed(seed)
    mods = []
    for i in range(len(sizes) - 1):
        lin = torch.nn.Linear(sizes[i], sizes[i + 1])
        with torch.no_grad():
            lin.weight.copy_(torch.randn(lin.weight.shape, generator=g) * 0.2 / np.sqrt(sizes[i]))
            lin.bias.copy_(torch.randn(lin.bias.shape, generator=g) * 0.1)
        mods.append(lin)
        if i < len(sizes) - 2:
            mods.append(torch.nn.Tanh())
    return torch.nn.Sequential(*mods).cuda()


def _setup(terminal_obs):
    from pde_control_gym import DeviceReplayBuffer, DeviceRollout, FusedMLP
    venv = K.make_1d("parabolic", NX, B, device="cuda")
    ro = DeviceRollout(venv, FusedMLP(_net((NX + 1, 32, 1), 3)), T, use_graph=False, action_low=LO, action_high=HI, action_noise=True,
                       one_launch=True, terminal_obs=terminal_obs)
    return ro, DeviceReplayBuffer(ro, CAP, LO, HI)


def _numpy(ro):
    f = lambda t: None if t is None else t.cpu().numpy()      # noqa: E731
    return f(ro.obs), f(ro.actions), f(ro.rewards), f(ro.terminated), f(ro.truncated), f(ro.terminal_obs)


NOISE = torch.randn(4, T, B, generator=torch.Generator().manual_seed(4)).mul_(3.0)      # (commands that leave the action box)


@pytest.mark.parametrize("terminal_obs", [False, True], ids=["next-slot", "terminal-obs"])
def test_storages_equal_the_numpy_restatement_on_a_real_rollout(terminal_obs):
    ro, buf = _setup(terminal_obs)
    ref = RR.NumpyReplay(CAP, NX + 1, LO, HI, np.float32)
    assert buf.D == NX + 1 and buf.A == 1 and buf.observations.is_cuda and buf.pos.is_cuda
    ended = clamped = 0
    for k in range(3):
        ro.action_noise.copy_(NOISE[k])
        ro.run()
        buf.add()
        ref.add(*_numpy(ro))
        RR.assert_equal(buf, ref, f"after add {k}")
        te, tr = ro.terminated.bool(), ro.truncated.bool()
        ended += int(te.sum()) * int((tr & ~te).sum())
        clamped += int((ro.actions <= LO).sum()) * int((ro.actions >= HI).sum())
    assert ended > 0 and clamped > 0, "a rollout must end episodes for both reasons and reach both ends of the action box"
    assert (buf.pos_host, buf.filled_host) == (0, 48) and ref.buf["term"].sum() > 0
    if terminal_obs:      # the two conventions differ exactly where a step was cut off
        assert not np.array_equal(ref.buf["next"][16:], ro.obs[1:].reshape(-1, NX + 1).cpu().numpy())
    s = buf.sample(64)
    assert s.index.is_cuda and s.index.shape == (48,) and int(s.index.max()) < 48
    draws = torch.arange(100, 164, device="cuda")
    assert torch.equal(buf.sample(64, draws=draws).index, draws % 48)


def test_run_and_add_in_one_graph_equal_the_eager_calls():
    runs = {}
    for mode in ("eager", "graph"):
        ro, buf = _setup(True)

        def both():
            ro.run()
            buf.add()
        ro.action_noise.copy_(NOISE[0])
        both()                                       # (also the warm-up of the captured calls)
        if mode == "graph":
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                both()
        snaps = []
        for i in (1, 2, 3):
            ro.action_noise.copy_(NOISE[i])
            if mode == "graph":
                graph.replay()
            else:
                both()
            torch.cuda.synchronize()
            snaps.append({k: v.clone() for k, v in buf.state_dict().items()})
        runs[mode] = snaps
        if mode == "graph":      # replays move the device counters alone; sync_host() reads them back
            assert (buf.pos_host, buf.filled_host) == (16, 48) and buf.sync_host() is buf and (buf.pos_host, buf.filled_host) == (32, 48)
    for i, (a, b) in enumerate(zip(runs["eager"], runs["graph"])):
        for k in a:
            assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), f"replay {i}: {k}"
    assert int(runs["graph"][-1]["filled"]) == 48 and int(runs["graph"][-1]["pos"]) == (4 * T * B) % CAP
    assert runs["eager"][-1]["dones"].sum() > 0


# ---- the examples -----------------------------------------------------------------------------------------------------------------------
def _example(name):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    try:
        spec = importlib.util.spec_from_file_location(name + "_by_index", os.path.join(ROOT, "examples", name + ".py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        sys.path.pop(0)
    return mod


@pytest.mark.parametrize("hidden", [64, 256])
def test_sac_example_with_replay_prints_the_history_of_the_fused_critic_path(hidden):
    mod = _example("train_sac_device")
    kw = dict(iterations=6, num_envs=256, n_steps=8, hidden=hidden, quiet=True, updates=2, batch=512, fused_grad=True, fused_loss=True,
              fused_opt=True, fused_critic=True)
    want = mod.main(**kw)
    got = mod.main(replay=True, **kw)
    assert got["moved"] == {"actor": True, "q1": True, "q2": True} and want["moved"] == got["moved"]
    for k in ("q_loss", "actor_loss", "alpha", "mean_reward", "mean_norm"):
        assert len(got[k]) == 6 and np.isfinite(got[k]).all() and got[k] == want[k], (k, got[k], want[k])
    if hidden == 64:
        with pytest.raises(ValueError, match="replay needs"):
            mod.main(iterations=1, num_envs=64, quiet=True, fused_grad=True, fused_loss=True, fused_opt=True, replay=True)
        with_terminal = mod.main(replay=True, terminal_obs=True, **kw)
        assert with_terminal["q_loss"] == mod.main(terminal_obs=True, **kw)["q_loss"]


@pytest.mark.parametrize("graph_update", [False, True], ids=["eager", "graph_update"])
def test_ppo_example_with_gather_prints_the_history_of_the_fused_loss_path(graph_update):
    mod = _example("train_ppo_device")
    kw = dict(iterations=2, B=64, quiet=True, hidden=64, fused_grad=True, fused_loss=True, fused_opt=graph_update, graph_update=graph_update)
    want = mod.main(**kw)
    got = mod.main(gather=True, **kw)
    assert len(got) == 2 and all(np.isfinite([v for v in h.values() if not isinstance(v, dict)]).all() for h in got)
    for a, b in zip(want, got):
        assert a == b, (a, b)
    if not graph_update:
        with pytest.raises(ValueError, match="gather needs"):
            mod.main(iterations=1, B=64, quiet=True, gather=True)
        wide = dict(kw, hidden=256, iterations=1)
        assert mod.main(gather=True, **wide) == mod.main(**wide)
