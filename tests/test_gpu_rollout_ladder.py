"""The slots-per-lane ladder of the one-launch 1D rollouts (csrc/pdegym_1d_body.h: with_epl, which the step launcher picks through too) against the step launcher's.

The reward is a wave reduction whose bits depend on how many slots a lane holds, so a rollout kernel has to be instantiated with the
slots-per-lane count the step launcher picks for the same row length: one rollout call equals the step calls BIT FOR BIT --
observation slots, rewards, both flags and the engine state left behind -- at one ragged row per instantiation, at the rows that
fill the wave exactly (the FULL instantiations) and at one row in every gap the ladder rounds up.  B = 5 (a ragged last workgroup of
four waves; inactive waves in a 16-wave policy workgroup), T = 3 env-steps of 2 sub-steps, nt = 5: the episode ends at the second
step and the fused auto-reset (pools of 2 B rows, reset_beta included) runs inside the launch.  Reward: TUNED1D.

Open loop for every row length up to 32 slots per lane; with a policy inside (16 units: one fma chain per neuron; 65 units: the
cooperative form) and with the backstepping law inside (both orders) for the rows of up to 8 slots per lane those kernels take."""
import numpy as np
import pytest

from tests.test_gpu_backstep_rollout import _build, _draw, _grid, _rollouts, _same
from tests.test_gpu_buffer_contract import EPLS, _init_beta, _kw1d, _ragged_slots, _reward

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

B, T, S, NT = 5, 3, 2, 5
SLOTS = [_ragged_slots(e) for e in EPLS] + [64, 128, 256, 512] + [421, 550, 800, 1100, 1700]      # ragged, FULL, rounded up (7 -> 8, ...)
SLOTS8 = [s for s in SLOTS if s <= 512]
STATE = ("time_index", "bsum", "norm_now", "norm_back", "ring", "reset_count", "beta")


def _bits(x):
    return np.ascontiguousarray(x.detach().cpu().numpy()).view(np.uint8)


def _engines(kind, n):
    """Two engines in the same state: rows and pools of ``_init_beta``, the fused auto-reset on pools of 2 B rows."""
    from pdecontrolgym_amd.batch1d import PDEBatch1D
    spec, _ = _reward("tuned", NT)
    init, beta = _init_beta(B, n, n)
    pool_i, pool_b = _init_beta(2 * B, n, n + 1)
    envs = [PDEBatch1D(kind, reward=spec, num_envs=B, device="cuda", **_kw1d(kind, n, S, NT)) for _ in range(2)]
    for e in envs:
        e.reset(init, beta)
        e.enable_auto_reset(torch.tensor(pool_i), keep_final_obs=True, beta_pool=torch.tensor(pool_b))
    return envs


def _rollout_against_steps(kind, n, policy=None, commands_of=None):
    """One rollout call on one engine, T step calls on its twin.  ``commands_of(obs)``: the two-launch path's command launch (its
    result must have the bits of the rollout's command); None: the step calls take the rollout's commands."""
    env, ref = _engines(kind, n)
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device="cuda")      # noqa: E731
    obs, act, rew, te, tr = z(T + 1, B, n), z(T, B), z(T, B), z(T, B, dt=torch.uint8), z(T, B, dt=torch.uint8)
    obs[0].copy_(env.t["obs"].reshape(B, n))
    if policy is None:
        act.copy_(torch.tensor(np.random.default_rng(n).uniform(-1, 1, (T, B)).astype(np.float32)))
    else:
        assert env.policy_fits_rollout(policy)
    env.rollout(obs, act, rew, te, tr, policy=policy)
    where = f"{kind} n={n}"
    assert torch.isfinite(act).all() and torch.isfinite(rew).all() and torch.isfinite(obs).all(), where
    cur = obs[0].clone()
    for t in range(T):
        a = act[t].clone()
        if commands_of is not None:
            a = commands_of(cur.contiguous())
            np.testing.assert_array_equal(_bits(a), _bits(act[t]), err_msg=f"{where}: actions[{t}]")
        o, r, a_te, a_tr = ref.step(a)
        for name, got, want in (("obs", obs[t + 1], o.reshape(B, n)), ("rewards", rew[t], r), ("terminated", te[t], a_te),
                                ("truncated", tr[t], a_tr)):
            np.testing.assert_array_equal(_bits(got), _bits(want), err_msg=f"{where}: {name}[{t}]")
        cur = o.reshape(B, n).clone()
    ended = (te | tr).sum(dim=0)
    assert int(ended.min()) == 1 and bool((te[1] | tr[1]).all()), where      # every episode ends at the second step, inside the launch
    for k in STATE:
        np.testing.assert_array_equal(_bits(env.t[k]), _bits(ref.t[k]), err_msg=f"{where}: engine state {k}")
    assert int(env.t["reset_count"].min()) == 1 and float(rew.abs().max()) > 0, where


@pytest.mark.parametrize("slots", SLOTS)
@pytest.mark.parametrize("kind", ["transport", "parabolic"])
def test_open_loop_rollout_equals_step_calls(kind, slots):
    _rollout_against_steps(kind, slots + (kind == "parabolic"))


@pytest.mark.parametrize("slots", SLOTS8)
@pytest.mark.parametrize("hidden", [16, 65], ids=["narrow-16-units", "wide-65-units"])
@pytest.mark.parametrize("kind", ["transport", "parabolic"])
def test_rollout_with_the_policy_inside_equals_policy_and_step_launches(kind, hidden, slots):
    """rollout1d_policy_kernel, narrow and wide.  The cooperative evaluation has the bits of ``FusedMLP.forward_into`` (the two-launch
    path's policy launch), which the comparison includes; the one-chain-per-neuron evaluation sums in another order than that launch
    (compared to float32 rounding in tests/test_gpu_nonfinite.py), so there the step calls take the commands the rollout computed."""
    from pdecontrolgym_amd.policy import FusedMLP
    n = slots + (kind == "parabolic")
    torch.manual_seed(hidden)
    pol = FusedMLP(torch.nn.Sequential(torch.nn.Linear(n, hidden), torch.nn.Tanh(), torch.nn.Linear(hidden, 1)).cuda(), clamp=(-1.0, 1.0))
    a_buf = torch.zeros(B, device="cuda")

    def two_launch_command(row):
        pol.forward_into(row, a_buf)
        return a_buf.clone()
    _rollout_against_steps(kind, n, policy=pol, commands_of=two_launch_command if hidden > 64 else None)


@pytest.mark.parametrize("slots", SLOTS8)
@pytest.mark.parametrize("order", ["ordered", "tree"])
@pytest.mark.parametrize("kind", ["transport", "parabolic"])
def test_rollout_with_the_law_inside_equals_control_and_step_launches(kind, order, slots):
    """backstep_rollout1d_kernel against the control launch + step launch per env-step, through ``DeviceRollout`` as in
    tests/test_gpu_backstep_rollout.py: commands, rows, rewards, flags and the engine state."""
    n = slots + (kind == "parabolic")
    grid = _grid(kind, slots, S, 2)                                   # episodes of 2 env-steps: nt = 5
    rng = np.random.default_rng(n)
    first, pool = _draw(rng, kind, B, n, slots, grid["dx"]), _draw(rng, kind, 2 * B, n, slots, grid["dx"])
    build = lambda: _build(kind, grid, first, pool, order=order)      # noqa: E731
    _, one = _rollouts(build, T, True)
    _, two = _rollouts(build, T, None)
    assert one[0]["obs"].shape == (T + 1, B, n) and (two[0]["terminated"] | two[0]["truncated"])[1].all()
    assert np.isfinite(two[0]["actions"]).all() and np.abs(two[0]["actions"]).max() > 0
    _same(one[0], two[0], f"{kind} n={n} {order}")
