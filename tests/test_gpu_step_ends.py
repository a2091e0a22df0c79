"""The two ends of the 1D step launch (pdegym_1d_body.h): the wave maxima of the overflow pre-check in front of the sub-step loop,
and behind it the observation row, which the fast-path step kernels store write-through and -- when the row's only home is the
observation (state_in) -- right after the loop, before the norm.  The rare paths that change what obs must hold (the exact redo
after a non-finite norm, the fused auto-reset) store again over that row.

Everything is compared with the NumPy oracle (oracle/pde_oracle.py): rows and observations as bit patterns, flags and time indices
exactly, rewards to rtol 1e-6 (wave butterfly against BLAS summation order, as in tests/test_gpu_1d.py).  Output tensors live in
guarded allocations (tests/poison.py) and start poisoned: a skipped store or a store past a row's end shows.
"""
import numpy as np
import pytest

from tests import poison as PZ

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

RARGS = (-1e3, 3e2)


def _kw(kind, nx, S, nt, max_state=1e10):
    dx = 1.0 / nx
    dt = 0.25 * dx * dx if kind == "parabolic" else 0.5 * dx
    return dict(T=(nt - 1) * dt, dt=dt, X=1, dx=dx, control_sample_rate=S * dt, control_type="Dirchilet", sensing_loc="full",
                sensing_type=None, normalize=False, max_control_value=20, limit_pde_state_size=True, max_state_value=max_state)


def _pair(kind, kw, B, state_in):
    """(engine, oracle) of one configuration."""
    from oracle import pde_oracle as po
    from pdecontrolgym_amd import _native as N
    from pdecontrolgym_amd.batch1d import PDEBatch1D, RewardSpec
    nt = int(round(kw["T"] / kw["dt"])) + 1
    env = PDEBatch1D(kind, reward=RewardSpec(N.REWARD_TUNED1D, nt, *RARGS), num_envs=B, device="cuda", state_in_obs=state_in, **kw)
    assert env.state_in_obs == state_in and env.nt == nt
    cls = po.ParabolicOracle if kind == "parabolic" else po.TransportOracle
    return env, cls(reward=po.TunedReward1DOracle(nt, *RARGS), keep_history=False, **kw)


def _guard(env, arena):
    """After reset(): the observation pair, the state rows and the kept terminal observations move into guarded allocations."""
    env._obs = [arena.like(f"obs{i}", o) for i, o in enumerate(env._obs)]
    env.t["obs"] = env._obs[env._flip]
    env.t["u"] = env.t["obs"] if env.state_in_obs else arena.like("u", env.t["u"])
    if env.t["final_obs"] is not None:
        env.t["final_obs"] = arena.like("final_obs", env.t["final_obs"])


def _poison_outputs(env):
    PZ.poison_(env._obs[env._flip ^ 1])              # the buffer the next step writes its observation to
    if env.t["final_obs"] is not None:
        PZ.poison_(env.t["final_obs"])


def _assert_bits(got, ref, msg):
    """Bit patterns; where BOTH hold a NaN only that is compared (NumPy's and the device's NaN payloads differ)."""
    got, ref = np.ascontiguousarray(got, dtype=np.float32), np.ascontiguousarray(ref, dtype=np.float32)
    assert got.shape == ref.shape, msg
    both_nan = np.isnan(got) & np.isnan(ref)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(ref), err_msg=msg)
    np.testing.assert_array_equal(got.view(np.uint32)[~both_nan], ref.view(np.uint32)[~both_nan], err_msg=msg)


def _assert_reward(r, r_ref, norm_now, msg):
    nn = np.where(np.isfinite(norm_now), norm_now, 0.0)
    np.testing.assert_allclose(r, r_ref, rtol=1e-6, atol=2e-6 * max(1.0, float(nn.max())), err_msg=msg)


def _step_and_compare(env, orc, arena, a, msg, reset_rows=None, pool=None):
    """One step of both; every output of every instance against the oracle.  reset_rows: the instances the fused auto-reset must
    restart from `pool` (row b, first restart), or "oracle" for whichever instances the oracle ends."""
    B = env.num_envs
    _poison_outputs(env)
    with np.errstate(all="ignore"):
        o_ref, r_ref, te_ref, tr_ref = orc.step(a)
    o, r, te, tr = env.step(torch.tensor(a))
    arena.check()
    PZ.assert_written(o, None, f"{msg}: obs")
    o, r, te, tr = o.cpu().numpy(), r.cpu().numpy(), te.cpu().numpy().astype(bool), tr.cpu().numpy().astype(bool)
    np.testing.assert_array_equal(te, te_ref, err_msg=msg)
    np.testing.assert_array_equal(tr, tr_ref, err_msg=msg)
    _assert_reward(r, r_ref, orc.norm_now, msg)
    ended = te_ref | tr_ref
    if reset_rows is None:
        want_obs, want_t = o_ref, orc.time_index
    else:
        if not isinstance(reset_rows, str):          # "oracle": whichever instances the oracle ends
            np.testing.assert_array_equal(ended, reset_rows, err_msg=f"{msg}: the case must end exactly these instances")
        want_obs = np.where(ended[:, None], pool[:B], o_ref)
        want_t = np.where(ended, 0, orc.time_index)
        fo = env.t["final_obs"]
        if fo is not None:
            PZ.assert_untouched(fo, torch.tensor(~ended), f"{msg}: final_obs of the instances that go on")
            _assert_bits(fo.cpu().numpy()[ended], o_ref[ended], f"{msg}: final_obs")
        np.testing.assert_array_equal(env.t["reset_count"].cpu().numpy(), ended.astype(np.int32), err_msg=msg)
    _assert_bits(o, want_obs, f"{msg}: obs")
    _assert_bits(env.u.cpu().numpy(), want_obs, f"{msg}: u")
    np.testing.assert_array_equal(env.time_index.cpu().numpy(), want_t, err_msg=msg)
    return ended


def _start(kind, nx, S, nt, B, state_in, init, beta, max_state=1e10, pool=None, keep_final_obs=True):
    env, orc = _pair(kind, _kw(kind, nx, S, nt, max_state), B, state_in)
    orc.reset(init, beta)
    env.reset(torch.tensor(init), torch.tensor(beta))
    if pool is not None:
        env.enable_auto_reset(torch.tensor(pool), keep_final_obs=keep_final_obs)
    arena = PZ.Arena("cuda")
    _guard(env, arena)
    return env, orc, arena


def _random_case(kind, n, B, seed):
    rng = np.random.default_rng(seed)
    x = np.linspace(0, 1, n)
    init = (rng.uniform(0.2, 0.6, (B, 1)) * (1 + 0.3 * np.sin(2 * np.pi * x * rng.uniform(0.5, 3, (B, 1))))).astype(np.float32)
    beta = ((50 if kind == "parabolic" else 5) * np.cos(rng.uniform(7, 8.5, (B, 1)) * np.arccos(x))).astype(np.float32)
    return rng, init, beta


# nodes n: 257 / 65 fill the wave exactly (FULL, 4 / 1 slots per lane); 258: 5 slots per lane, a lane that straddles the row's end and
# empty lanes; 3: two slots, one lane; transport 64 / 128 FULL, 100 ragged, 3 one lane
STORE_CASES = [("parabolic", 256), ("parabolic", 64), ("parabolic", 257), ("parabolic", 2), ("transport", 64), ("transport", 128),
               ("transport", 100), ("transport", 3)]


@pytest.mark.parametrize("state_in", [True, False], ids=["state_in", "own_u"])
@pytest.mark.parametrize("kind,nx", STORE_CASES, ids=[f"{k}-nx{n}" for k, n in STORE_CASES])
def test_row_stores_are_complete_and_stay_inside_the_row(kind, nx, state_in):
    """Every row-store path x B in {1, 5, 9} (partial workgroups) x S in {1, 7}: three steps, the last one past the episode's end."""
    n = nx + (kind == "parabolic")
    for B in (1, 5, 9):
        for S in (1, 7):
            rng, init, beta = _random_case(kind, n, B, 1000 * nx + 10 * B + S)
            env, orc, arena = _start(kind, nx, S, 2 * S + 1, B, state_in, init, beta)
            for i in range(3):
                a = rng.uniform(-1, 1, B).astype(np.float32)
                _step_and_compare(env, orc, arena, a, f"{kind} nx={nx} B={B} S={S} step {i}")


@pytest.mark.parametrize("keep_final_obs", [True, False], ids=["final_obs", "no_final_obs"])
@pytest.mark.parametrize("state_in", [True, False], ids=["state_in", "own_u"])
@pytest.mark.parametrize("kind,nx", [("parabolic", 256), ("parabolic", 257), ("transport", 100)])
def test_auto_reset_overwrites_the_row_stored_after_the_loop(kind, nx, state_in, keep_final_obs):
    """One step on which the fused auto-reset fires for some instances of the batch only: two at time index nt - 2 (termination),
    one whose norm is past max_state (truncation).  obs holds the pool row for those and the stepped row for the others, final_obs
    the terminal row of those alone."""
    B, S, nt = 9, 7, 150
    n = nx + (kind == "parabolic")
    rng, init, beta = _random_case(kind, n, B, nx)
    init[4] *= 20.0                                   # ||row|| > 50 = max_state, the others stay below 20
    pool = rng.uniform(1, 3, (2 * B, n)).astype(np.float32)
    env, orc, arena = _start(kind, nx, S, nt, B, state_in, init, beta, max_state=50.0, pool=pool, keep_final_obs=keep_final_obs)
    late = np.array([2, 6])
    orc.time_index[late] = nt - 2
    env.t["time_index"][torch.tensor(late)] = nt - 2
    want = np.zeros(B, dtype=bool)
    want[[2, 4, 6]] = True
    a = rng.uniform(-1, 1, B).astype(np.float32)
    ended = _step_and_compare(env, orc, arena, a, f"{kind} nx={nx}", reset_rows=want, pool=pool)
    assert ended.sum() == 3


@pytest.mark.parametrize("auto_reset", [False, True], ids=["plain", "auto_reset"])
@pytest.mark.parametrize("state_in", [True, False], ids=["state_in", "own_u"])
@pytest.mark.parametrize("kind,nx", [("parabolic", 256), ("parabolic", 257), ("transport", 128), ("transport", 100)])
def test_exact_redo_in_the_middle_of_a_batch(kind, nx, state_in, auto_reset):
    """Instances that leave the fast loop among ordinary ones: an inf node, a NaN node, a row whose squares overflow (finite row,
    non-finite norm: the fast loop runs, its row is stored, the exact loop's row goes over it), a command of exactly -0.0."""
    B, S, nt = 9, 7, 150
    n = nx + (kind == "parabolic")
    rng, init, beta = _random_case(kind, n, B, 7 * nx)
    init[2, n // 3] = np.inf
    init[5, n // 2] = np.nan
    init[3] *= 1.0e20
    pool = rng.uniform(1, 3, (2 * B, n)).astype(np.float32) if auto_reset else None
    env, orc, arena = _start(kind, nx, S, nt, B, state_in, init, beta, pool=pool)
    for i in range(2):
        a = rng.uniform(-1, 1, B).astype(np.float32)
        a[7] = -0.0
        if auto_reset:                                 # the oracle has no auto-reset: compare the first step, where it fires
            ended = _step_and_compare(env, orc, arena, a, f"{kind} nx={nx} auto-reset", reset_rows="oracle", pool=pool)
            # the row whose squares overflow has norm inf >= max_state and restarts; a NaN norm compares false: that instance goes on
            assert ended[3] and not ended[5] and not ended[[0, 1, 4, 6, 7, 8]].any()
            break
        _step_and_compare(env, orc, arena, a, f"{kind} nx={nx} step {i}")


@pytest.mark.parametrize("lane", [0, 31, 63])
@pytest.mark.parametrize("nx", [64, 256])
def test_transient_overflow_is_seen_in_every_lane(nx, lane):
    """test_parabolic_transient_overflow_takes_the_exact_loop (tests/test_gpu_1d.py) at B = 3 with the value above 2^127 in the
    first, a middle and the last lane of the wave maximum (nx = 64: one slot per lane; nx = 256: four)."""
    B, S = 3, 8
    n = nx + 1
    node = 1 + lane * (nx // 64) + (1 if nx > 64 else 0)
    init = np.zeros((B, n), dtype=np.float32)
    init[0, node] = 2.0e38
    init[1, n // 6:n - n // 6] = 1.0e38
    init[2] = 1.0
    beta = np.zeros((B, n), dtype=np.float32)
    env, orc, arena = _start("parabolic", nx, S, 4 * S + 1, B, True, init, beta)
    orc.limit_pde_state_size = False
    env.params.limit_state = 0
    for i in range(3):
        _step_and_compare(env, orc, arena, np.zeros(B, dtype=np.float32), f"nx={nx} lane {lane} step {i}")
    # (nx = 64, lane 63: the slot is the controlled boundary node, which the command replaces before anything doubles it -- the
    # pre-check still sees it and takes the exact loop, the row stays finite)
    assert np.isnan(orc.row[0]).any() == (node != n - 1) and np.isfinite(orc.row[1]).all() and np.isfinite(orc.row[2]).all()


@pytest.mark.parametrize("nx", [64, 256, 257])
def test_guard_maxima_of_zero_denormal_and_last_lane_rows(nx):
    """The pre-check's wave maxima at their edges: a row of zeros (log2 0 = -inf: the fast loop), a row of denormals, and beta rows
    whose largest |dt * beta| sits in the wave's last occupied lane -- under a small row (fast loop) and under a row it
    drives past 2^126 within the step (exact loop)."""
    B, S = 5, 7
    n = nx + 1
    dt = 0.25 / (nx * nx)
    init = np.zeros((B, n), dtype=np.float32)
    init[1] = 1.0e-42
    init[2] = 1.0
    init[3] = 1.0e30
    init[4] = 0.5
    beta = np.zeros((B, n), dtype=np.float32)
    # the largest |dt * beta| at the last interior node, n - 2: lane 63 for nx = 256, the straddling lane 51 for nx = 257, lane 62 for
    # nx = 64 (whose lane 63 holds the controlled boundary node alone) -- and at the boundary node as well, which the maximum sees
    # although its slot is frozen: the wave's last occupied lane in every shape.  dt * beta = 8: 9^7 per step, which the row of ones
    # survives for three steps (fast loop) and the row of 1e30 does not (fast loop first, then the exact one)
    beta[2:4, n - 2:] = np.float32(8.0 / dt)
    beta[4] = 3.0
    env, orc, arena = _start("parabolic", nx, S, 4 * S + 1, B, True, init, beta)
    rng = np.random.default_rng(nx)
    for i in range(3):
        a = rng.uniform(-1, 1, B).astype(np.float32)
        a[0] = 0.0                                     # the zero row stays a zero row
        _step_and_compare(env, orc, arena, a, f"nx={nx} step {i}")
    assert not orc.row[0].any() and not np.isfinite(orc.row[3]).all() and np.isfinite(orc.row[2]).all()


def test_rollout_equals_three_step_calls():
    """The rollout kernels share wave_max (the carried beta maximum) and keep their plain stores: T = 3 env-steps in one launch
    against three step calls, bit for bit."""
    from pdecontrolgym_amd import _native as N
    from pdecontrolgym_amd.batch1d import PDEBatch1D, RewardSpec
    nx, B, S, T = 256, 5, 7, 3
    kw = _kw("parabolic", nx, S, 4 * S + 1)
    envs = [PDEBatch1D("parabolic", reward=RewardSpec(N.REWARD_TUNED1D, 4 * S + 1, *RARGS), num_envs=B, device="cuda", **kw)
            for _ in range(2)]
    n = envs[0].n
    rng, init, beta = _random_case("parabolic", n, B, 5)
    acts = torch.tensor(rng.uniform(-1, 1, (T, B)).astype(np.float32), device="cuda")
    outs = []
    for e in envs:
        assert e.can_rollout()
        e.reset(torch.tensor(init), torch.tensor(beta))
        obs = torch.zeros(T + 1, B, n, device="cuda")
        obs[0].copy_(e.t["obs"])
        outs.append((obs, torch.zeros(T, B, device="cuda"), torch.zeros(T, B, dtype=torch.uint8, device="cuda"),
                     torch.zeros(T, B, dtype=torch.uint8, device="cuda")))
    e, (obs, rew, te, tr) = envs[0], outs[0]
    e.t["obs"] = obs[0]
    e.t["u"] = obs[0]
    for t in range(T):
        e.step(acts[t], out_obs=obs[t + 1], out_reward=rew[t], out_terminated=te[t], out_truncated=tr[t])
    e2, (obs2, rew2, te2, tr2) = envs[1], outs[1]
    e2.rollout(obs2, acts, rew2, te2, tr2)
    for x, y in ((obs, obs2), (rew, rew2), (te, te2), (tr, tr2)):
        np.testing.assert_array_equal(x.cpu().numpy().view(np.uint8), y.cpu().numpy().view(np.uint8))
    for k in ("time_index", "bsum", "ring", "norm_now", "norm_back"):
        np.testing.assert_array_equal(e.t[k].cpu().numpy(), e2.t[k].cpu().numpy(), err_msg=k)
