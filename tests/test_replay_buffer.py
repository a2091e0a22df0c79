"""CPU tests of ``pde_control_gym.DeviceReplayBuffer`` against the NumPy restatement of the replay memory the SAC example kept by hand
(tests/replay_buffer_reference.py), on the smallest shapes that can go wrong: T = 3, B = 2, D = 3, A = 1, capacity 8 -- two ``add()``
calls fill 6 of 8 slots and then wrap in the middle of the second rollout.  The class is plain torch indexing, so the CPU runs the same
code the device does; tests/test_gpu_replay_buffer.py repeats it on a real ``DeviceRollout`` and inside a captured graph."""
import numpy as np
import pytest

from tests import replay_buffer_reference as RR

torch = pytest.importorskip("torch")

T, B, D, CAP = 3, 2, 3, 8
BOXES = [(-10.0, 10.0), (-1.5, 2.25)]


def _pair(dtype, terminal_obs, box=BOXES[0], seed=0):
    from pde_control_gym import DeviceReplayBuffer
    ro = RR.FakeRollout(T, B, D, dtype, terminal_obs, seed=seed)
    return ro, DeviceReplayBuffer(ro, CAP, *box), RR.NumpyReplay(CAP, D, *box, np.float64 if dtype == torch.float64 else np.float32)


@pytest.mark.parametrize("box", BOXES, ids=["box10", "box-1.5..2.25"])
@pytest.mark.parametrize("terminal_obs", [False, True], ids=["next-slot", "terminal-obs"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_storages_equal_the_numpy_restatement_across_the_wrap(dtype, terminal_obs, box):
    ro, buf, ref = _pair(dtype, terminal_obs, box)
    assert buf.observations.dtype == buf.next_observations.dtype == dtype and buf.observations.shape == (CAP, D)
    assert buf.actions.dtype == buf.rewards.dtype == buf.dones.dtype == torch.float32
    assert buf.actions.shape == buf.rewards.shape == buf.dones.shape == (CAP, 1)
    RR.assert_equal(buf, ref, "empty")
    heads = []
    for k in range(3):
        ro.run()
        assert buf.add() is buf
        ref.add(*ro.numpy())
        RR.assert_equal(buf, ref, f"after add {k}")
        heads.append((buf.pos_host, buf.filled_host))
    assert heads == [(6, 6), (4, 8), (2, 8)]                     # the second add wraps after two of its six transitions
    flags = np.concatenate([ref.buf["term"], ref.buf["act"]], 1)
    assert set(np.unique(ref.buf["term"])) == {0.0, 1.0} and flags[:, 1].min() == -1.0 and flags[:, 1].max() == 1.0      # both clamps bite
    if dtype == torch.float64:      # the rewards were rounded once
        assert not np.array_equal(ro.rewards.numpy(), ro.rewards.numpy().astype(np.float32).astype(np.float64))


def test_dones_and_next_follow_sb3s_timeout_handling():
    """Spelled out on one hand-made step per kind: ended by termination, by truncation, by both, not ended."""
    from pde_control_gym import DeviceReplayBuffer
    for terminal_obs in (False, True):
        ro = RR.FakeRollout(2, 2, 1, torch.float32, terminal_obs)
        ro.obs.copy_(torch.arange(6.0).reshape(3, 2, 1))
        ro.terminated.copy_(torch.tensor([[1, 0], [1, 0]], dtype=torch.uint8))
        ro.truncated.copy_(torch.tensor([[0, 1], [1, 0]], dtype=torch.uint8))
        if terminal_obs:
            ro.terminal_obs.copy_(torch.tensor([[[10.0], [11.0]], [[12.0], [13.0]]]))
        buf = DeviceReplayBuffer(ro, 4).add()
        assert buf.observations.flatten().tolist() == [0.0, 1.0, 2.0, 3.0]
        if terminal_obs:
            assert buf.next_observations.flatten().tolist() == [10.0, 11.0, 12.0, 5.0] and buf.dones.flatten().tolist() == [1.0, 0.0, 1.0, 0.0]
        else:
            assert buf.next_observations.flatten().tolist() == [2.0, 3.0, 4.0, 5.0] and buf.dones.flatten().tolist() == [1.0, 1.0, 1.0, 0.0]


def test_a_rollout_with_sensing_noise_stores_what_the_policy_saw():
    ro, buf, _ = _pair(torch.float32, False)
    ro.run()
    ro.obs_seen = ro.obs + 100.0
    buf.add()
    assert torch.equal(buf.observations[:6], ro.obs_seen[:T].reshape(6, D)) and torch.equal(buf.next_observations[:6], ro.obs_seen[1:].reshape(6, D))


def test_sample_draws_the_examples_random_stream_and_stays_inside_what_is_filled():
    ro, buf, _ = _pair(torch.float32, True)
    with pytest.raises(ValueError, match="empty"):
        buf.sample(4)
    buf.add()                                                    # 6 of 8 slots
    torch.manual_seed(5)
    s = buf.sample(1000)                                         # min(batch, filled) draws, as the example made them
    torch.manual_seed(5)
    assert torch.equal(s.index, torch.randint(0, 6, (6,))) and s.index.dtype == torch.int64
    torch.manual_seed(6)
    many = torch.cat([buf.sample(5).index for _ in range(200)])
    assert many.shape == (1000,) and int(many.min()) == 0 and int(many.max()) == 5      # never slot 6 or 7
    # the sample holds the storages themselves, not copies
    for name in RR.NAMES:
        assert getattr(s, name).data_ptr() == getattr(buf, name).data_ptr() and getattr(s, name).shape[0] == CAP
    g = buf.gather(s)
    assert g.index is s.index and all(torch.equal(getattr(g, name), getattr(buf, name)[s.index]) for name in RR.NAMES)
    assert g.observations.shape == (6, D) and g.rewards.shape == (6, 1)


def test_sample_with_draws_is_draws_modulo_filled_on_the_device():
    ro, buf, _ = _pair(torch.float64, False)
    draws = torch.tensor([0, 5, 6, 7, 13, 2 ** 40 + 3], dtype=torch.int64)
    buf.add()
    assert buf.sample(6, draws=draws).index.tolist() == [int(d) % 6 for d in draws.tolist()]
    buf.add()
    assert buf.sample(6, draws=draws).index.tolist() == [int(d) % 8 for d in draws.tolist()]
    for bad in (draws.to(torch.int32), draws[:5], draws.reshape(6, 1)):
        with pytest.raises(ValueError, match=r"draws must be an int64 \[6\]"):
            buf.sample(6, draws=bad)


def test_state_dict_round_trip():
    ro, buf, ref = _pair(torch.float32, True)
    for _ in range(2):
        ro.run()
        buf.add()
        ref.add(*ro.numpy())
    state = {k: v.clone() for k, v in buf.state_dict().items()}
    assert set(state) == {"observations", "next_observations", "actions", "rewards", "dones", "pos", "filled"}
    _, other, _ = _pair(torch.float32, True)
    assert other.load_state_dict(state) is other
    RR.assert_equal(other, ref, "after load_state_dict")
    ro2 = other.rollout.run()
    other.add()
    ref.add(*ro2.numpy())
    RR.assert_equal(other, ref, "an add after load_state_dict")
    with pytest.raises(ValueError, match="keys"):
        other.load_state_dict({k: v for k, v in state.items() if k != "pos"})
    with pytest.raises(ValueError, match="observations: shape"):
        other.load_state_dict(dict(state, observations=torch.zeros(CAP + 1, D)))


def test_refusals():
    from pde_control_gym import DeviceReplayBuffer
    ro = RR.FakeRollout(T, B, D, torch.float32, False)
    with pytest.raises(ValueError, match=r"capacity 5 is below one rollout \(3 steps x 2 environments = 6 transitions\)"):
        DeviceReplayBuffer(ro, 5)
    DeviceReplayBuffer(ro, 6)
    with pytest.raises(ValueError, match="action_low < action_high"):
        DeviceReplayBuffer(ro, 8, 1.0, 1.0)


def test_the_package_exports_the_class():
    import pde_control_gym
    assert "DeviceReplayBuffer" in pde_control_gym.__all__ and pde_control_gym.DeviceReplayBuffer.__module__ == "pde_control_gym.replay_buffer"
    assert pde_control_gym.ReplaySample._fields == ("index", "observations", "next_observations", "actions", "rewards", "dones")
