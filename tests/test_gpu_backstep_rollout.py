"""GPU tests of the backstepping law inside the one-launch 1D rollout (csrc/pdegym_backstep_rollout.hip): everything
``DeviceRollout(venv, controller, T, one_launch=True)`` produces -- observation slots, commands, rewards, flags and the engine state
left behind -- equals the two-launch path (control launch + step launch per env-step) BIT FOR BIT, in both summation orders, eagerly
and from a replayed graph, with gains that follow the restarts the fused auto-reset makes inside the launch; against the per-instance
oracle loop of tests/test_gpu_backstepping.py; at every row shape at which the kernel takes another path; with noise and a binding
clamp; on poisoned buffers with guard bands; with non-finite rows; and whatever the batch an instance sits in."""
import functools

import numpy as np
import pytest

from tests import poison
from tests.test_gpu_backstepping import CLAMP, POOL_B, POOL_P, POOL_S, POOL_T, _pool_case, _pool_oracle

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
f32 = np.float32
KEYS = ("obs", "actions", "rewards", "terminated", "truncated")
STATE = ("time_index", "reset_count", "bsum", "ring", "obs", "beta", "norm_now", "norm_back", "final_obs")
ENV_ID = {"transport": "PDEControlGym-TransportPDE1D", "parabolic": "PDEControlGym-ReactionDiffusionPDE1D"}
AMP = {"transport": 5.0, "parabolic": 50.0}        # the amplitudes of the two example scripts
# every kernel launched in csrc/pdegym_backstep_rollout.hip -> the poisoned-buffer / guard-band tests that reach it
# (tests/test_backstep_rollout.py fails when a launched kernel is missing here)
KERNEL_CASES = {"backstep_rollout1d_kernel": ["test_rollout_writes_exactly_its_outputs"]}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _same(got, want, what):
    for k in want:
        if want[k] is None:
            assert got[k] is None, (what, k)
        elif isinstance(want[k], dict):
            _same(got[k], want[k], f"{what}: {k}")
        else:
            np.testing.assert_array_equal(_bits(got[k]), _bits(want[k]), err_msg=f"{what}: {k}")


# ---- a small environment + controller from explicit rows -----------------------------------------------------------------------------
def _grid(kind, nx, S, episode_steps):
    """Within the reference's stability bounds: transport dt/dx = nx * 1e-4 <= 0.06 <= 1, parabolic dt/dx^2 = 0.25 <= 0.5."""
    dx = 1.0 / nx
    dt = 1e-4 if kind == "transport" else 0.25 * dx * dx
    return dict(T=episode_steps * S * dt, dt=dt, X=1, dx=dx, control_sample_rate=S * dt)


def _draw(rng, kind, rows, n, m, dx):
    """Rows of the examples' family: beta on the plant's grid, theta on the controller's, a constant initial condition."""
    gam = rng.uniform(5, 10, (rows, 1))
    beta = (AMP[kind] * np.cos(gam * np.arccos(np.linspace(0, 1, n))[None])).astype(f32)
    theta = (AMP[kind] * np.cos(gam * np.arccos(np.linspace(dx, 1, m))[None])).astype(f32)
    init = (rng.uniform(1, 10, (rows, 1)) * np.ones((1, n))).astype(f32)
    return init, beta, theta


def _build(kind, grid, first, pool=None, order="ordered", shared=False):
    """Environment on ``first`` = (init, beta, theta) rows with the fused auto-reset on ``pool`` = (init, beta, theta) rows (None: no
    restarts; shared: ONE theta row for every instance, so the pool redraws the initial condition only), controller attached."""
    import pde_control_gym
    from pde_control_gym import BacksteppingController
    from pde_control_gym.src import TunedReward1D
    init, beta, theta = first
    B = init.shape[0]
    nt_r = int(round(grid["T"] / grid["dt"]))
    brow = (lambda idx: np.repeat(beta[:1], len(idx), 0)) if shared else (lambda idx: beta[idx])
    params = dict(grid, reward_class=TunedReward1D(nt_r, -1e3, 3e2), normalize=False, sensing_loc="full", control_type="Dirchilet",
                  sensing_type=None, limit_pde_state_size=True, max_state_value=1e10, max_control_value=20,
                  batched_reset_func=lambda idx, nx: (init[idx], brow(idx)))
    venv = pde_control_gym.make_vec(ENV_ID[kind], num_envs=B, device="cuda", **params)
    venv.reset_tensor()
    if pool is not None:
        venv.enable_fused_auto_reset(init_pool=pool[0], beta_pool=False if shared else pool[1])
    ctrl = BacksteppingController(kind, theta[0] if shared else theta, grid["dx"], pool_theta=None if (pool is None or shared) else pool[2],
                                  order=order, device="cuda").attach(venv)
    return venv, ctrl


def _snap(ro, venv):
    torch.cuda.synchronize()
    s = {k: getattr(ro, k).cpu().numpy().copy() for k in KEYS}
    s["obs_seen"] = None if ro.obs_seen is None else ro.obs_seen.cpu().numpy().copy()
    s["state"] = {k: (venv.core.t[k].cpu().numpy().copy() if torch.is_tensor(venv.core.t.get(k)) else None) for k in STATE}
    return s


def _rollouts(build, T, one_launch, use_graph=False, runs=1, clamp=CLAMP, action_noise=None, sensing_noise=None, first_obs=None):
    """``runs`` DeviceRollout.run() calls on a fresh environment; ``action_noise`` / ``sensing_noise``: standard deviations of the
    pre-drawn noise (seeded per run, the same for both paths).  Returns the snapshots after each run."""
    from pde_control_gym import DeviceRollout
    venv, ctrl = build()
    assert venv.one_launch_fits(ctrl) is False and venv.one_launch_law_fits(ctrl) is True
    ro = DeviceRollout(venv, ctrl, T, use_graph=use_graph, action_low=clamp[0], action_high=clamp[1], one_launch=one_launch,
                       action_noise=action_noise is not None, sensing_noise=sensing_noise is not None)
    assert ro.one_launch is bool(one_launch)
    snaps = []
    for r in range(runs):
        if action_noise is not None:
            ro.action_noise.copy_(torch.from_numpy(np.random.default_rng(70 + r).normal(0, action_noise, tuple(ro.action_noise.shape)).astype(f32)))
        if sensing_noise is not None:
            ro.sensing_noise.copy_(torch.from_numpy(np.random.default_rng(80 + r).normal(0, sensing_noise, tuple(ro.sensing_noise.shape)).astype(f32)))
        ro.run(None if first_obs is None else torch.as_tensor(first_obs).cuda())
        snaps.append(_snap(ro, venv))
    return ctrl, snaps


# ---- (a) the pool case: gains follow >= 2 restarts per instance and run ---------------------------------------------------------------
def _pool_build(kind, order):
    case = _pool_case(kind)
    return lambda: _build(kind, case["grid"], case["first"], case["pool"], order=order)


@functools.lru_cache(maxsize=None)
def _pool_want(kind):
    """The oracle loop of tests/test_gpu_backstepping.py on the device's gains (which equal the restatement bit for bit, as the tests
    there assert): two runs by the documented rule, one by the wrong one.  Computed once per kind."""
    case = _pool_case(kind)
    _, ctrl = _pool_build(kind, "ordered")()
    g0, gp = ctrl.gain.cpu().numpy(), ctrl.pool_gain.cpu().numpy()
    return _pool_oracle(case, g0, gp, runs=2), _pool_oracle(case, g0, gp, runs=1, wrong_rule=True)[0]


@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("order", ["ordered", "tree"])
@pytest.mark.parametrize("kind", ["transport", "parabolic"])
def test_one_launch_equals_two_launches_with_gains_following_the_fused_auto_reset(kind, order, use_graph):
    """First check of this file: one_launch=True with a controller used to raise ValueError.  n = 100 / 101, B = 6, P = 7, T = 8,
    S = 5, episodes of 3 env-steps; two consecutive run() calls."""
    build = _pool_build(kind, order)
    _, one = _rollouts(build, POOL_T, True, use_graph, runs=2)
    _, two = _rollouts(build, POOL_T, None, use_graph, runs=2)
    for run in range(2):
        assert (two[run]["terminated"] | two[run]["truncated"]).sum(axis=0).min() >= 2      # every instance restarts >= 2 times per run
        _same(one[run], two[run], f"{kind} {order} graph={use_graph} run {run}")
    assert one[1]["state"]["reset_count"].min() >= 4 and POOL_S == 5 and one[0]["obs"].shape == (POOL_T + 1, POOL_B, 100 + (kind == "parabolic"))
    if order == "ordered":
        want, wrong = _pool_want(kind)
        for run in range(2):
            for k in ("obs", "actions", "terminated", "truncated"):
                np.testing.assert_array_equal(one[run][k], want[run][k], err_msg=f"run {run}: {k}")
            np.testing.assert_allclose(one[run]["rewards"], want[run]["rewards"], rtol=1e-6, atol=1e-4)
        # discrimination: gains taken from pool row b always (right for the first restart, wrong from the second on) must differ
        assert not np.array_equal(wrong["actions"], one[0]["actions"]) and POOL_P == 7
        np.testing.assert_array_equal(wrong["actions"][:6], one[0]["actions"][:6])      # (the second restart ends step 5)


# ---- (b) row shapes: every slots-per-lane path, FULL rows, len < row, a shared gain row ------------------------------------------------
SHAPE_B, SHAPE_T, SHAPE_S = 5, 4, 3
SHAPES = [("transport", 40, None), ("transport", 64, None), ("parabolic", 65, None), ("parabolic", 101, 50), ("transport", 150, None),
          ("transport", 256, None), ("parabolic", 257, None), ("parabolic", 513, None),
          # beyond the table of the issue: the remaining instantiations (FULL 2 per lane; 5, 6 and 7 -> 8 per lane, partial)
          ("transport", 128, None), ("transport", 300, None), ("parabolic", 350, None), ("transport", 420, None),
          ("transport", 512, None)]          # FULL 8 per lane, transport: the longest transport row the kernel takes


def _shape_build(kind, n, m, order, B=SHAPE_B, seed=0):
    """Episodes of 2 env-steps, so every instance restarts twice in T = 4 steps (pool of 7 rows); m given: a short SHARED theta row."""
    nx = n - (kind == "parabolic")
    grid = _grid(kind, nx, SHAPE_S, 2)
    rng = np.random.default_rng(1000 * n + seed)
    mm = nx if m is None else m
    first, pool = _draw(rng, kind, B, n, mm, grid["dx"]), _draw(rng, kind, 7, n, mm, grid["dx"])
    return lambda: _build(kind, grid, first, pool, order=order, shared=m is not None)


@pytest.mark.parametrize("order", ["ordered", "tree"])
@pytest.mark.parametrize("kind,n,m", SHAPES)
def test_one_launch_equals_two_launches_at_every_row_shape(kind, n, m, order):
    build = _shape_build(kind, n, m, order)
    ctrl, one = _rollouts(build, SHAPE_T, True)
    _, two = _rollouts(build, SHAPE_T, None)
    assert one[0]["obs"].shape == (SHAPE_T + 1, SHAPE_B, n) and (m is None or (ctrl.gain.shape == (m,) and ctrl._length(n) == m < n - 1))
    assert (two[0]["terminated"] | two[0]["truncated"]).sum(axis=0).min() >= 2
    assert np.isfinite(two[0]["actions"]).all() and np.abs(two[0]["actions"]).max() > 0
    _same(one[0], two[0], f"{kind} n={n} m={m} {order}")


# ---- (c) action noise, a clamp that binds, pre-drawn sensing noise ------------------------------------------------------------------
@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("kind,n,order", [("transport", 100, "tree"), ("parabolic", 101, "ordered"), ("parabolic", 257, "tree")])
def test_noise_and_clamp_inside_the_launch(kind, n, order, use_graph):
    build = _pool_build(kind, order) if n <= 101 else _shape_build(kind, n, None, order)
    T = POOL_T if n <= 101 else SHAPE_T
    _, free = _rollouts(build, T, None, clamp=(-1e30, 1e30))
    bound = float(np.median(np.abs(free[0]["actions"])))           # half of the unclamped commands lie beyond it
    kw = dict(clamp=(-bound, bound), action_noise=0.25 * bound, sensing_noise=0.05, runs=2, use_graph=use_graph)
    _, one = _rollouts(build, T, True, **kw)
    _, two = _rollouts(build, T, None, **kw)
    for run in range(2):
        a = np.abs(two[run]["actions"])
        assert (a == f32(bound)).any() and (a < f32(bound)).any() and a.max() == f32(bound)      # the clamp binds for some commands
        _same(one[run], two[run], f"{kind} n={n} {order} graph={use_graph} run {run}")
        assert not np.array_equal(one[run]["obs_seen"], one[run]["obs"])                            # the law read noisy rows ...
    # ... and the observation slots stayed clean: slot t + 1 is the step kernel's row, which the noise never enters -- a run with the
    # same commands replayed open loop through the plain rollout kernel reproduces them
    venv, _ = build()
    obs, rew = torch.zeros_like(torch.as_tensor(one[0]["obs"])).cuda(), torch.zeros(T, one[0]["actions"].shape[1], device="cuda")
    te, tr = (torch.zeros(T, one[0]["actions"].shape[1], dtype=torch.uint8, device="cuda") for _ in range(2))
    obs[0].copy_(venv.rollout_obs())
    venv.core.rollout(obs, torch.as_tensor(one[0]["actions"]).cuda(), rew, te, tr)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(_bits(obs.cpu().numpy()), _bits(one[0]["obs"]))


# ---- (d) the output contract on poisoned buffers ------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,n,order", [("transport", 100, "ordered"), ("parabolic", 101, "tree"), ("parabolic", 513, "ordered")])
def test_rollout_writes_exactly_its_outputs(kind, n, order, policy=None):
    """Every element the header says is written is written -- obs slots 1 .. T, actions, rewards, flags, obs_seen -- whatever the
    buffers held before (NaN poison, wrong flags); gains, pools, noise and reset pools keep their bits; every guard band is intact.
    ``policy`` displaces every guarded buffer of the poisoned run off its 256-byte boundary (tests/poison.py)."""
    build = _pool_build(kind, order) if n <= 101 else _shape_build(kind, n, None, order)
    T = POOL_T if n <= 101 else SHAPE_T
    rng = np.random.default_rng(5)

    def run(poisoned):
        venv, ctrl = build()
        core, B = venv.core, venv.num_envs
        arena = poison.Arena("cuda", policy=policy if poisoned else None)
        ctrl.gain, ctrl.pool_gain = arena.like("gain", ctrl.gain), arena.like("pool_gain", ctrl.pool_gain)
        for k in ("reset_init", "reset_beta", "beta", "time_index", "bsum", "ring", "reset_count", "norm_now", "norm_back"):
            core.t[k] = arena.like(k, core.t[k])
        ctrl.attach(venv)                              # (takes the guarded counter)
        obs = arena.new("obs", (T + 1, B, n), torch.float32)
        out = {"actions": arena.new("actions", (T, B), torch.float32), "rewards": arena.new("rewards", (T, B), torch.float32),
               "terminated": arena.new("terminated", (T, B), torch.uint8), "truncated": arena.new("truncated", (T, B), torch.uint8),
               "obs_seen": arena.new("obs_seen", (T, B, n), torch.float32)}
        nz = arena.like("noise", torch.from_numpy(rng.normal(0, 1, (T, B)).astype(f32)).cuda())
        on = arena.like("obs_noise", torch.from_numpy(rng.normal(0, 0.05, (T, B, n)).astype(f32)).cuda())
        if poisoned:
            poison.poison_(obs)
            for v in out.values():
                poison.poison_(v)
        obs[0].copy_(venv.rollout_obs())
        keep = {k: v.clone() for k, v in (("gain", ctrl.gain), ("pool_gain", ctrl.pool_gain), ("reset_init", core.t["reset_init"]),
                                          ("reset_beta", core.t["reset_beta"]), ("noise", nz), ("obs_noise", on), ("obs0", obs[0]))}
        core.rollout(obs, out["actions"], out["rewards"], out["terminated"], out["truncated"], policy=ctrl, clamp=CLAMP, noise=nz,
                     obs_noise=on, obs_seen=out["obs_seen"])
        arena.check()
        now = {"gain": ctrl.gain, "pool_gain": ctrl.pool_gain, "reset_init": core.t["reset_init"], "reset_beta": core.t["reset_beta"],
               "noise": nz, "obs_noise": on, "obs0": obs[0]}
        for k, v in keep.items():
            poison.assert_bits_equal(now[k], v, None, f"input {k}")
        state = {k: core.t[k].clone() for k in ("time_index", "bsum", "ring", "reset_count", "norm_now", "norm_back", "beta")}
        return obs, out, state
    rng = np.random.default_rng(5)
    cobs, cout, cstate = run(False)
    rng = np.random.default_rng(5)
    pobs, pout, pstate = run(True)
    poison.assert_written(pobs, None, "obs", like=cobs)
    for k, v in pout.items():
        poison.assert_written(v, None, k, like=cout[k])
    for k, v in pstate.items():
        poison.assert_bits_equal(v, cstate[k], None, f"state {k}")
    assert int(cstate["reset_count"].min()) >= 2


# ---- (e) non-finite rows ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
@pytest.mark.parametrize("kind,n,order", [("transport", 100, "tree"), ("parabolic", 101, "ordered"), ("parabolic", 257, "ordered")])
def test_a_non_finite_row_gives_the_two_launch_bits_and_leaves_the_other_instances_alone(kind, n, order, bad):
    build = _pool_build(kind, order) if n <= 101 else _shape_build(kind, n, None, order)
    T = POOL_T if n <= 101 else SHAPE_T
    venv, _ = build()
    first = venv.rollout_obs().cpu().numpy().copy()
    _, clean = _rollouts(build, T, True)
    first[2, n // 3] = bad
    _, one = _rollouts(build, T, True, first_obs=first)
    _, two = _rollouts(build, T, None, first_obs=first)
    _same(one[0], two[0], f"{kind} n={n} {order} {bad}")
    assert not np.isfinite(one[0]["actions"][0, 2]) or abs(one[0]["actions"][0, 2]) == CLAMP[1]       # NaN kept, Inf clamped to the bound
    others = [b for b in range(first.shape[0]) if b != 2]
    for k in KEYS:
        np.testing.assert_array_equal(_bits(one[0][k][:, others]), _bits(clean[0][k][:, others]), err_msg=f"other instances: {k}")
    assert not np.array_equal(_bits(one[0]["obs"][:, 2]), _bits(clean[0]["obs"][:, 2]))


# ---- (f) batch invariance -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _people(kind, n):
    """Nine instances with their own first rows and two restart rows each (episodes of 2 env-steps: restarts k = 0, 1 in T = 4)."""
    nx = n - (kind == "parabolic")
    grid = _grid(kind, nx, SHAPE_S, 2)
    rng = np.random.default_rng(9000 + n)
    return grid, _draw(rng, kind, 9, n, nx, grid["dx"]), [_draw(rng, kind, 9, n, nx, grid["dx"]) for _ in range(2)]


def _batch_of(kind, n, ids, order):
    """The batch with instance ids[p] at position p.  The k-th restart of position p takes pool row (p + k*B) mod P: with P = 2 B rows,
    row p + k*B holds the k-th restart row of ids[p] -- every instance meets the same rows in every batch."""
    grid, first, restarts = _people(kind, n)
    ids = np.asarray(ids)
    pool = tuple(np.concatenate([restarts[0][j][ids], restarts[1][j][ids]]) for j in range(3))
    return lambda: _build(kind, grid, tuple(a[ids] for a in first), pool, order=order)


@pytest.mark.parametrize("kind,n,order", [("transport", 150, "ordered"), ("parabolic", 101, "tree"), ("parabolic", 257, "ordered")])
def test_an_instance_gets_the_same_bits_in_every_batch(kind, n, order):
    _, ref = _rollouts(_batch_of(kind, n, list(range(9)), order), SHAPE_T, True)
    assert (ref[0]["terminated"] | ref[0]["truncated"]).sum(axis=0).min() >= 2
    for ids in ([4], [8], [7, 2, 5, 0, 3], [3, 8, 1, 6, 4, 0, 7, 2, 5]):
        _, got = _rollouts(_batch_of(kind, n, ids, order), SHAPE_T, True)
        for k in KEYS:
            np.testing.assert_array_equal(_bits(got[0][k]), _bits(ref[0][k][:, ids]), err_msg=f"{kind} n={n} ids={ids}: {k}")
        for k in ("time_index", "bsum", "ring", "reset_count", "beta"):
            np.testing.assert_array_equal(_bits(got[0]["state"][k]), _bits(ref[0]["state"][k][ids]), err_msg=f"ids={ids}: state {k}")
