"""GPU tests of the one-launch TherapyWrapper paths (csrc/pdegym_tumor_rollout.hip): ``TumorVecEnv(fused_step=True)`` and the rollout
kernel with commands given ahead, with a neuron-per-lane policy and with a cooperative (wide) policy, against the launch sequence of
``TumorVecEnv.step_tensor`` -- the same expressions in the same order under the same flags, so every comparison is ``torch.equal`` (of
the bit patterns: an invisible tumour's radius is NaN) --
and against the reference's own wrapper episodes (tests/golden/tumor.npz); the output contract on poisoned, guarded buffers; batch
invariance; a NaN command.  Configuration: B = 17 patients, 24 wrapper steps, the doses of tests/test_tumor_rollout.py (every branch
of the wrapper step is taken: that file counts them), rows of 70 nodes (two chunks, the second ragged), 201 (the shipped grid) and
300 (the strided staging path)."""
import functools

import numpy as np
import pytest

from tests import nonfinite as nf
from tests import poison
from tests.test_tumor import KW, WRAP_CASES, tumor_ic
from tests.test_tumor_rollout import B, STEPS, _actions

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

# every kernel of the unit -> the tests that poison its outputs (tests/test_tumor_rollout.py checks the table against the source)
KERNEL_CASES = {"tumor_rollout_kernel": ["test_output_contract_on_poisoned_guarded_buffers"]}
CONFIGS = [(nx, T, w) for nx in (70, 201, 300) for T in (600, 300) for w in (False, True)]
ENGINE_KEYS = ("u", "time_index", "stage", "remaining", "days", "out")


def _venv(nx=201, T=600, weekends=False, fused=False, num_envs=B):
    import pde_control_gym
    from pde_control_gym.src import BrainTumorReward
    venv = pde_control_gym.make_vec("PDEControlGym-BrainTumor1D", num_envs=num_envs, weekends=weekends, fused_step=fused, T=T,
                                    reward_class=BrainTumorReward(), reset_init_condition_func=tumor_ic, **{**KW, "X": nx - 1})
    assert venv.core.nx == nx
    venv.benchmark()
    venv.reset_tensor()
    return venv


def _state(venv):
    t = venv.core.t
    return {**{k: t[k].clone() for k in ENGINE_KEYS},
            "calls": venv.treatment_calls.clone(), "viol": venv.soft_constraint_violations.clone(), "cons": venv._consecutive.clone()}


def _steps(venv, acts):
    """step_tensor per row of ``acts``: stacked obs / reward / flags, the kept last rows (zero where no episode ended), the end state."""
    rows = []
    for a in acts:
        obs, rew, term, trunc = venv.step_tensor(a)
        done = (term | trunc)[:, None]
        rows.append((obs.clone(), rew.clone(), term.clone(), trunc.clone(), torch.where(done, venv.terminal_obs, torch.zeros_like(obs))))
    return [torch.stack(x) for x in zip(*rows)], _state(venv)


@functools.lru_cache(maxsize=None)
def _reference(nx, T, weekends):
    """The launch sequence of today's step_tensor, once per configuration (shared, never modified)."""
    acts = torch.from_numpy(np.stack(_actions())).cuda()
    out, state = _steps(_venv(nx, T, weekends), acts)
    assert bool((out[2] | out[3]).any()), "no episode ended in the reference run"
    return acts, out, state


def _equal(got, want, what):
    if isinstance(want, dict):
        for k in want:
            _equal(got[k], want[k], f"{what} {k}")
    else:
        if want.dtype == torch.bool:
            assert got.dtype == want.dtype and torch.equal(got, want), what
        else:      # bit patterns: `out` holds NaN (an invisible tumour has no radius), which torch.equal never finds equal
            assert got.dtype == want.dtype and torch.equal(poison.bits(got), poison.bits(want)), what


def guard_venv(venv, arena):
    """Every tensor the wrapper-step kernels address in a guarded copy of ``arena``: the engine's dictionary (state, [B] outputs,
    xscale, t_benchmark) and the wrapper's state (init rows, counters, final_obs, obs).  Returns the wrapper state."""
    from tests.test_gpu_buffer_contract import guard_engine
    guard_engine(venv.core, arena)
    W = venv._wrapper_state()
    for k, v in list(W.items()):
        if torch.is_tensor(v):
            W[k] = arena.like("wrap_" + k, v)
    venv._consecutive, venv.treatment_calls, venv.soft_constraint_violations = W["consecutive"], W["treatment_calls"], W["soft_constraint_violations"]
    venv._final_obs, venv._fused_obs = W["final_obs"], W["obs"]
    return W


@pytest.mark.parametrize("nx,T,weekends", [(201, 600, True), (70, 300, False)])
def test_therapy_step_on_guarded_buffers(nx, T, weekends, displace=None):
    """pdegym_tumor_therapy_step with every pointer of the call in a guarded allocation -- the engine's state and [B] outputs, the
    command (bufs.control), the wrapper's counters, init, final_obs and obs: the steps equal step_tensor's launch sequence on fresh
    tensors bit for bit, and every guard is intact.  ``displace``: a policy of tests/poison.py that moves every one of them off
    its 256-byte boundary (tests/test_gpu_pointer_alignment.py)."""
    acts, want, want_state = _reference(nx, T, weekends)
    venv = _venv(nx, T, weekends, fused=True)
    arena = poison.Arena("cuda", policy=displace)
    W = guard_venv(venv, arena)
    commands = [arena.like(f"control{s}", a) for s, a in enumerate(acts)]
    if displace is not None:
        for t in [venv.core.t[k] for k in ENGINE_KEYS + ("reward", "terminated", "truncated", "xscale")] + commands[:1] + \
                 [v for v in W.values() if torch.is_tensor(v)]:
            assert t.data_ptr() % 16 != 0 and t.data_ptr() % t.element_size() == 0
    got, got_state = _steps(venv, commands)
    arena.check()
    for g, w, name in zip(got, want, ("obs", "reward", "terminated", "truncated", "terminal_obs")):
        _equal(g, w, name)
    _equal(got_state, want_state, "end state")
    for c, a in zip(commands, acts):
        assert torch.equal(c, a), "a command was changed"


# ---- fused_step and the rollout with commands given ahead == step_tensor ---------------------------------------------------------------
@pytest.mark.parametrize("nx,T,weekends", CONFIGS)
def test_therapy_step_equals_step_tensor(nx, T, weekends):
    acts, want, want_state = _reference(nx, T, weekends)
    got, got_state = _steps(_venv(nx, T, weekends, fused=True), acts)
    for g, w, name in zip(got, want, ("obs", "reward", "terminated", "truncated", "terminal_obs")):
        _equal(g, w, name)
    _equal(got_state, want_state, "end state")


@pytest.mark.parametrize("nx,T,weekends", CONFIGS)
def test_rollout_with_commands_ahead_equals_step_tensor(nx, T, weekends):
    from pde_control_gym import DeviceRollout
    acts, want, want_state = _reference(nx, T, weekends)
    for chunk in (STEPS, 8):          # one launch of 24 steps; three launches of 8 (state and counters cross the launch boundaries)
        venv = _venv(nx, T, weekends)
        ro = DeviceRollout(venv, None, chunk, use_graph=False, one_launch=True)
        assert ro.one_launch is True
        got = [[], [], [], []]
        for k in range(STEPS // chunk):
            ro.actions.copy_(acts[k * chunk:(k + 1) * chunk])
            ro.run()
            assert torch.equal(ro.actions, acts[k * chunk:(k + 1) * chunk])
            for lst, x in zip(got, (ro.obs[1:], ro.rewards, ro.terminated.bool(), ro.truncated.bool())):
                lst.append(x.clone())
        for g, w, name in zip(got, want, ("obs", "reward", "terminated", "truncated")):
            _equal(torch.cat(g), w, f"{name} (launches of {chunk})")
        _equal(_state(venv), want_state, f"end state (launches of {chunk})")
        # the kept last row of every patient's latest episode
        done = want[2] | want[3]
        last = done.int().flip(0).argmax(0)
        last = STEPS - 1 - last
        for b in torch.nonzero(done.any(0)).flatten().tolist():
            assert torch.equal(venv.terminal_obs[b], want[4][last[b], b]), f"terminal_obs of patient {b}"


# ---- the policy inside the launch ------------------------------------------------------------------------------------------------------
def _net(width):
    torch.manual_seed(1)
    net = torch.nn.Sequential(torch.nn.Linear(201, width), torch.nn.Tanh(), torch.nn.Linear(width, 1), torch.nn.Tanh()).cuda()
    with torch.no_grad():
        net[0].weight.mul_(1e-5)                    # cell densities are O(1e5) (tests/test_tumor.py:315)
    return net


def _noise(T, n, seed=0):
    return torch.from_numpy(np.random.default_rng(seed).normal(0.08, 0.06, (T, n)).astype(np.float32)).cuda()


def _policy_runs(width, n, one_launch, use_graph, runs=1, T=12):
    from pde_control_gym import DeviceRollout, FusedMLP
    venv = _venv(201, 600, True, num_envs=n)
    ro = DeviceRollout(venv, FusedMLP(_net(width)), T, use_graph=use_graph, action_low=0.0, action_high=1.0, action_noise=True,
                       one_launch=one_launch)
    assert ro.one_launch is bool(one_launch)
    out = []
    for k in range(runs):
        ro.action_noise.copy_(_noise(T, n, k))
        ro.run()
        out.append([x.clone() for x in (ro.obs, ro.actions, ro.rewards, ro.terminated, ro.truncated)])
    return out, _state(venv)


@pytest.mark.parametrize("n", [17, 33])
def test_wide_policy_one_launch_equals_the_graph_of_policy_and_step_launches(n):
    """201 -> 128 -> 1: the cooperative evaluation is bit-identical to pdegym_mlp_forward, so the whole rollout equals the default
    path (one policy launch and the step_tensor launches per step, captured in a hipGraph).  17 and 33 patients leave a last
    workgroup with one patient and fifteen waves that only attend the barriers."""
    want, want_state = _policy_runs(128, n, None, True, runs=2)
    got, got_state = _policy_runs(128, n, True, False, runs=2)
    for a, b in zip(got, want):
        for x, y, name in zip(a, b, ("obs", "actions", "rewards", "terminated", "truncated")):
            _equal(x, y, name)
    _equal(got_state, want_state, "end state")
    assert float(want[0][1].max()) > 0


def test_narrow_policy_rollout_is_reproduced_by_its_recorded_actions_and_matches_the_torch_forward_pass():
    """201 -> 32 -> 1 (one neuron per lane; its summation order is not pdegym_mlp_forward's, so the comparison is per step from the
    same observation): a commands-ahead rollout fed the recorded actions returns the same bits, and actions[t] agrees with the torch
    float32 forward pass of obs[t] (+ noise, clamped) within the tolerance tests/test_tumor.py:327 uses for these two passes."""
    from pde_control_gym import DeviceRollout
    T = 24
    (run,), state = _policy_runs(32, B, True, False, T=T)
    obs, actions, rewards, term, trunc = run
    venv = _venv(201, 600, True)
    ro = DeviceRollout(venv, None, T, use_graph=False, one_launch=True)
    ro.actions.copy_(actions)
    ro.run()
    for x, y, name in zip((ro.obs[1:], ro.rewards, ro.terminated, ro.truncated), (obs[1:], rewards, term, trunc),
                          ("obs", "rewards", "terminated", "truncated")):
        _equal(x, y, name)
    _equal(_state(venv), state, "end state")
    net, noise = _net(32), _noise(T, B, 0)
    with torch.no_grad():
        for t in range(T):
            want = (net(obs[t].float()).reshape(B) + noise[t]).clamp(0.0, 1.0).double()
            np.testing.assert_allclose(actions[t].cpu().numpy(), want.cpu().numpy(), rtol=1e-4, atol=1e-6, err_msg=f"step {t}")
    assert float(actions.max()) > 0


def test_graph_replay_equals_eager():
    """Three consecutive run()s of the one-launch rollout with a policy: the captured graph (warm-up, rewind, two replays) == eager."""
    eager, eager_state = _policy_runs(32, B, True, False, runs=3)
    graph, graph_state = _policy_runs(32, B, True, True, runs=3)
    for a, b in zip(graph, eager):
        for x, y, name in zip(a, b, ("obs", "actions", "rewards", "terminated", "truncated")):
            _equal(x, y, name)
    _equal(graph_state, eager_state, "end state")


# ---- against the reference's own wrapper episodes ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("case", WRAP_CASES)
def test_fused_step_reproduces_the_reference_wrapper(golden_tumor, case, n):
    """tests/golden/tumor.npz: TherapyWrapper episodes of the reference (weekly schedule, daily, hypofractionated).  The in-kernel exp
    and pow are within 1 ulp of libm's: rtol 1e-11 as in test_tumor_vecenv_equals_single_wrappers_gpu; flags, day counters and the
    wrapper's counters are exact."""
    g = golden_tumor[case]
    venv = _venv(201, 600, bool(g.weekends), fused=True, num_envs=n)
    assert torch.equal(venv.t_benchmark, torch.full((n,), float(g.t_benchmark), dtype=torch.float64, device="cuda"))
    np.testing.assert_array_equal(venv.core.t["u"].cpu().numpy(), np.broadcast_to(g.rows[0], (n, 201)))
    assert (venv.core.t["time_index"] == int(g.time_index[0])).all()
    steps = len(g.reward)
    a = torch.full((n,), float(g.frac), dtype=torch.float64, device="cuda")
    for k in range(steps):
        obs, rew, term, trunc = venv.step_tensor(a)
        np.testing.assert_allclose(rew.cpu().numpy(), np.full(n, g.reward[k]), rtol=1e-11, atol=0, err_msg=f"reward step {k}")
        assert (term.cpu().numpy() == bool(g.term[k])).all() and (trunc.cpu().numpy() == bool(g.trunc[k])).all(), k
        last = bool(g.term[k] or g.trunc[k])
        assert last == (k == steps - 1)
        row = venv.terminal_obs if last else obs
        np.testing.assert_allclose(row.cpu().numpy(), np.broadcast_to(g.rows[k + 1], (n, 201)), rtol=1e-11, atol=0, err_msg=f"row step {k}")
        if not last:
            assert (venv.core.t["time_index"] == int(g.time_index[k + 1])).all(), k
    # the episode is over: every patient has been restarted and has run its growth stage again
    np.testing.assert_array_equal(obs.cpu().numpy(), np.broadcast_to(g.rows[0], (n, 201)))
    assert (venv.core.t["time_index"] == int(g.time_index[0])).all() and (venv.core.t["stage"] == 1).all()
    assert (venv.treatment_calls == int(g.calls)).all() and (venv.soft_constraint_violations == int(g.violations)).all()
    assert (venv._consecutive == 0).all()


# ---- output contract -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_policy", [False, True])
def test_output_contract_on_poisoned_guarded_buffers(with_policy, displace=None):
    """Every buffer of the launch in a guarded allocation; outputs poisoned.  Slots 1..T and rows 0..T-1 are written for every patient;
    slot 0, actions given ahead, init and xscale are left as they were; final_obs is written exactly where an episode ended; and
    the poisoned run returns the bits of a clean one.  ``displace``: a policy of tests/poison.py that moves every guarded buffer off its
    256-byte boundary (tests/test_gpu_pointer_alignment.py)."""
    from pde_control_gym import FusedMLP
    T, nx = 24, 201
    acts = torch.from_numpy(np.stack(_actions())).cuda()
    noise = _noise(T, B, 3)
    policy = FusedMLP(_net(32)) if with_policy else None

    def run(arena):
        venv = _venv(nx, 600, True)
        c = venv.core
        if arena:                                       # the engine state the kernel reads and writes, and its [B] outputs
            from tests.test_gpu_buffer_contract import guard_engine
            guard_engine(c, arena)
        new = (lambda name, shape, dtype: arena.new(name, shape, dtype)) if arena else (lambda name, shape, dtype: torch.zeros(shape, dtype=dtype, device="cuda"))
        obs, actions = new("obs", (T + 1, B, nx), torch.float64), new("actions", (T, B), torch.float64)
        rewards, term, trunc = new("rewards", (T, B), torch.float64), new("terminated", (T, B), torch.uint8), new("truncated", (T, B), torch.uint8)
        W = dict(venv._wrapper_state())
        W["final_obs"] = new("final_obs", (B, nx), torch.float64)
        init = new("init", (nx,), torch.float64)
        init.copy_(W["init"])
        W["init"] = init
        xs = new("xscale", (nx,), torch.float64)
        xs.copy_(c.t["xscale"])
        c.t["xscale"] = xs
        for k, dt in (("consecutive", torch.int32), ("treatment_calls", torch.int64), ("soft_constraint_violations", torch.int64)):
            buf = new(k, (B,), dt)
            buf.copy_(W[k])
            W[k] = buf
        if arena:
            for t_ in (obs, rewards, term, trunc, W["final_obs"]) + ((actions,) if with_policy else ()):
                poison.poison_(t_)
        if with_policy:
            obs[0].copy_(c.t["u"])
        else:
            actions.copy_(acts)
        c.rollout(obs, actions, rewards, term, trunc, policy=policy, clamp=(0.0, 1.0), noise=noise if with_policy else None, wrap_state=W)
        torch.cuda.synchronize()
        return dict(obs=obs, actions=actions, rewards=rewards, terminated=term, truncated=trunc, final_obs=W["final_obs"], init=init,
                    xscale=xs, u=c.t["u"], W=W, core=c, first=c.t["u"])

    clean = run(None)
    arena = poison.Arena("cuda", policy=displace)
    got = run(arena)
    arena.check()
    for k in ("rewards", "terminated", "truncated"):
        poison.assert_written(got[k], None, k, like=clean[k])
    poison.assert_written(got["obs"], (slice(1, None),), "obs slots 1..T")
    poison.assert_bits_equal(got["obs"][1:], clean["obs"][1:], None, "obs slots 1..T")
    if with_policy:
        poison.assert_written(got["actions"], None, "actions", like=clean["actions"])
        assert torch.equal(got["obs"][0], clean["obs"][0])
    else:
        poison.assert_untouched(got["obs"], (0,), "obs slot 0")
        assert torch.equal(got["actions"], acts)
    assert torch.equal(got["init"], clean["init"]) and torch.equal(got["xscale"], clean["xscale"])
    ended = (clean["terminated"].bool() | clean["truncated"].bool()).any(0)
    if not with_policy:
        assert bool(ended.any()) and not bool(ended.all())
    poison.assert_written(got["final_obs"], ended, "final_obs of finished patients", like=clean["final_obs"])
    poison.assert_untouched(got["final_obs"], ~ended, "final_obs of the others")
    assert set(got["terminated"].unique().tolist()) <= {0, 1} and set(got["truncated"].unique().tolist()) <= {0, 1}
    for k in ("consecutive", "treatment_calls", "soft_constraint_violations"):
        assert torch.equal(got["W"][k], clean["W"][k]), k
    for k in ENGINE_KEYS + ("reward", "terminated", "truncated"):
        _equal(got["core"].t[k], clean["core"].t[k], k)
    # the engine's own [B] outputs hold the last step's values
    assert torch.equal(got["core"].t["reward"], got["rewards"][-1]) and torch.equal(got["core"].t["terminated"], got["terminated"][-1])


# ---- batch invariance, non-finite commands --------------------------------------------------------------------------------------------
def _ahead(n, acts, weekends=True, T=600):
    from pde_control_gym import DeviceRollout
    venv = _venv(201, T, weekends, num_envs=n)
    ro = DeviceRollout(venv, None, acts.shape[0], use_graph=False, one_launch=True)
    ro.actions.copy_(acts)
    ro.run()
    torch.cuda.synchronize()
    return ro, venv


def test_batch_invariance():
    """Patient i gets the same bits whether it is simulated alone, among 17 or among 64 (another wave of another workgroup)."""
    acts = torch.from_numpy(np.stack(_actions(STEPS, 64))).cuda()
    big_ro, big = _ahead(64, acts)
    assert bool((big_ro.terminated | big_ro.truncated)[:, :17].any())
    for n in (1, 17):
        ro, venv = _ahead(n, acts[:, :n].contiguous())
        for x, y, name in ((ro.obs, big_ro.obs, "obs"), (ro.rewards, big_ro.rewards, "rewards"), (ro.terminated, big_ro.terminated, "terminated"),
                           (ro.truncated, big_ro.truncated, "truncated")):
            assert torch.equal(x, y[:, :n]), f"{name} at B = {n}"
        _equal(_state(venv), {k: v[:n] for k, v in _state(big).items()}, f"end state at B = {n}")


def test_a_nan_command_changes_only_its_own_patient():
    acts = torch.from_numpy(np.stack(_actions())).cuda()
    clean_ro, clean = _ahead(B, acts)
    bad = acts.clone()
    nf.plant_(bad, (2, 3))          # patient 3, step 2 (a treatment day)
    ro, venv = _ahead(B, bad)
    others = nf.rows_except(B, [3])
    for x, y, name in ((ro.obs, clean_ro.obs, "obs"), (ro.rewards, clean_ro.rewards, "rewards"), (ro.terminated, clean_ro.terminated, "terminated"),
                       (ro.truncated, clean_ro.truncated, "truncated")):
        nf.same_bits_and_nans(x[:, others], y[:, others], name)
    a, b = _state(venv), _state(clean)
    for k in a:
        nf.same_bits_and_nans(a[k][others], b[k][others], k)
    assert not bool(torch.isnan(ro.obs[:3, 3]).any()) and bool(torch.isnan(ro.obs[3, 3]).any()), "the NaN dose reaches the patient's own row"
    assert bool(torch.isnan(venv.core.t["remaining"][3]))
