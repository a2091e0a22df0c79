"""Output contracts of the HIP kernels, checked with poisoned buffers and guard bands (tests/poison.py).

The parity suites run on buffers that start as zeros, and many correct values here are exactly 0 (parabolic node 0, the NS walls,
the flags, reward 0 past the episode end), so a skipped store, a read before write or a store past a buffer's end can go unseen
there.  Each case below drives the C ABI through HipBackend -- via the engines, whose tensor dictionaries are swapped for guarded
copies ([4 KiB guard | payload | 4 KiB guard]) -- and asserts:

  1. complete   every element include/pdegym.h says is written no longer holds the poison and equals the clean run (same sequence
                on zero-filled buffers through the unmodified engine) bit for bit; the clean run equals the oracle where the parity
                suites pin it (1D rows / observations / trajectories bit-exact, rewards rtol 1e-6 as in test_gpu_1d.py; the MLP
                against a float64 evaluation, tolerance stated at the test);
  2. untouched  elements the header says are left alone keep the poison bits;
  3. no stray   every guard of every buffer (scratch included) is intact after synchronising;
  4. prior      work space, pressure partner, observation partner, ring, bsum and final_obs start as NaN, state before a reset
                as NaN (integers: in-range wrong values): results are unchanged.

KERNEL_CASES maps every kernel launched in pdecontrolgym_amd/csrc/*.hip to the tests that reach it; tests/test_poison_helper.py
fails when a launched kernel is missing from it.
"""
import numpy as np
import pytest

from tests import poison as PZ

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

# kernel (template name as launched) -> tests that reach at least one of its instantiations: of this module, or "module::test" of
# another module under tests/
KERNEL_CASES = {
    "step1d_kernel": ["test_1d_step_contract", "test_1d_full_rows", "test_1d_m64_contract", "test_1d_state_in_leaves_u_alone",
                      "test_1d_auto_reset_final_obs_and_pools", "test_1d_reward_none_leaves_reward_alone"],
    "step1d_wide_kernel": ["test_1d_wide_kernels", "test_gpu_1d_wide_bookkeeping::test_wide_kernel_bookkeeping_matches_oracle"],
    "reset1d_kernel": ["test_1d_masked_reset_leaves_others_alone", "test_1d_reset_initialises_poisoned_state"],
    "reset_history_kernel": ["test_1d_masked_reset_leaves_others_alone", "test_1d_step_contract"],
    "rownorm2_kernel": ["test_rownorm2_ragged"],
    "selftest_quotient_kernel": ["test_selftest_quotient_counter_only"],
    "rollout1d_kernel": ["test_1d_rollout_contract"],
    "rollout1d_general_kernel": ["test_1d_rollout_contract"],
    "rollout1d_policy_kernel": ["test_1d_rollout_contract"],
    "rollout1d_policy_general_kernel": ["test_1d_rollout_contract"],
    "mlp_forward_kernel": ["test_mlp_forward_contract_vs_float64"],
    "ns256_fused_step": ["test_ns256_contract"],
    "ns256_split_obs": ["test_ns256_contract"],
    "ns256_front_f64": ["test_ns256_contract"],
    "ns256_pass_f64": ["test_ns256_contract"],
    "ns256_split_obs_f64": ["test_ns256_contract"],
    "ns256_finish_f64": ["test_ns256_contract"],
    "ns_col_step_w1": ["test_ns_column_kernel_contract"],
    "ns_col_step": ["test_ns_column_kernel_contract"],
    "ns_col_rollout": ["test_ns_rollout_contract"],
    "ns_auto_reset_kernel": ["test_ns_auto_reset_final_obs"],
    "ns_auto_reset_finish": ["test_ns_auto_reset_final_obs"],
    "ns_tile_step": ["test_ns_tile_and_generic_contract"],
    "ns_tile_step_f64": ["test_ns_tile_and_generic_contract"],
    "ns_generic_step": ["test_ns_tile_and_generic_contract"],
    "ns_generic_pressure": ["test_ns_solve_pressure_contract"],
    "ns_reset_kernel": ["test_ns_masked_reset_leaves_others_alone"],
    "traffic_step_kernel": ["test_traffic_contract"],
    "traffic_step_wide_kernel": ["test_traffic_contract"],
    "traffic_rollout_kernel": ["test_traffic_rollout_contract"],
    "traffic_reset_kernel": ["test_traffic_contract"],
    "tumor_step_kernel": ["test_tumor_contract"],
    "tumor_reset_kernel": ["test_tumor_contract"],
}


def _f32(a):
    return torch.tensor(np.asarray(a, dtype=np.float32))


def _arena(policy=None, keep_aligned=()):
    """The arena of a case.  ``policy`` (None, "one", "mixed": tests/poison.py) displaces every buffer off its 256-byte boundary --
    tests/test_gpu_pointer_alignment.py runs the cases of this module that way; ``keep_aligned`` names the buffers whose parameter in
    include/pdegym.h demands an alignment."""
    return PZ.Arena("cuda", policy=policy, keep_aligned=keep_aligned)




def guard_engine(env, arena, skip=()):
    """Swap every tensor of ``env.t`` (and the observation pair ``env._obs``) for a guarded copy; aliases stay aliases."""
    seen = {}

    def g(name, t):
        if t is None or not torch.is_tensor(t):
            return t
        key = (t.data_ptr(), tuple(t.shape), t.dtype)
        if key not in seen:
            seen[key] = arena.like(name, t)
        return seen[key]
    if hasattr(env, "_obs"):
        env._obs = [g(f"obs{i}", o) for i, o in enumerate(env._obs)]
    for k, v in list(env.t.items()):
        if k not in skip:
            env.t[k] = g(k, v)
    return env


# ---- 1D steps ------------------------------------------------------------------------------------------------------------
EPLS = (1, 2, 3, 4, 5, 6, 8, 12, 16, 24, 32)


def _ragged_slots(epl):
    """A slot count whose EPL is ``epl`` and which leaves a straddling lane (not a multiple of epl) and idle lanes."""
    s = 64 * (epl - 1) + 37 if epl > 1 else 37
    return s + 1 if s % epl == 0 else s


def _kw1d(kind, n, S, nt, control="Dirchilet", sensing="full"):
    nx = n - (kind == "parabolic")
    dx = 1.0 / nx
    dt = 0.25 * dx * dx if kind == "parabolic" else 0.5 * dx
    return dict(T=(nt - 1) * dt, dt=dt, X=1, dx=dx, control_sample_rate=S * dt, control_type=control, sensing_loc=sensing,
                sensing_type=None, normalize=True, max_control_value=20, limit_pde_state_size=True, max_state_value=1e10)


def _reward(mode, nt):
    from pdecontrolgym_amd import _native as N
    from pdecontrolgym_amd.batch1d import RewardSpec
    from oracle import pde_oracle as po
    if mode == "diff":
        return (RewardSpec(N.REWARD_NORM_L2, nt, -1e-4, 1e2, horizon=N.HORIZON_DIFFERENTIAL),
                po.NormRewardOracle(nt, "2", -1e-4, 1e2, horizon="differential"))
    if mode == "thor":
        return (RewardSpec(N.REWARD_NORM_L2, nt, -1e-4, 1e2, horizon=N.HORIZON_T, t_horizon=5),
                po.NormRewardOracle(nt, "2", -1e-4, 1e2, horizon="t-horizon", t_horizon_length=5))
    if mode == "none_reward":
        return RewardSpec(N.REWARD_NONE, nt), None
    return RewardSpec(N.REWARD_TUNED1D, nt, -1e3, 3e2), po.TunedReward1DOracle(nt, -1e3, 3e2)


def _mk1d(kind, kw, spec, B, hist, **extra):
    from pdecontrolgym_amd.batch1d import PDEBatch1D
    return PDEBatch1D(kind, reward=spec, num_envs=B, device="cuda", record_history=hist, state_in_obs=False, **kw, **extra)


def _init_beta(B, n, seed, f64_beta=False):
    rng = np.random.default_rng(seed)
    init = (rng.uniform(1, 2, (B, 1)) * np.linspace(1, 1.5, n)[None]).astype(np.float32)
    beta = 5 * np.cos(rng.uniform(7, 8, (B, 1)) * np.arccos(np.linspace(0, 1, n)))
    return init, (beta if f64_beta else beta.astype(np.float32))


OUT1D = ("obs", "reward", "norm_now", "norm_back", "terminated", "truncated")


def _run_1d_pair(kind, n, B, mode, S=3, steps=3, nt=None, seed=0, action_kind=None, f64_beta=False, flux=None, policy=None):
    """Clean engine + guarded, poisoned engine over the same sequence; returns (clean, poisoned, arena, oracle results)."""
    from oracle import pde_oracle as po
    from pdecontrolgym_amd import _native as N
    nt = nt or S * steps                           # the last step is partial: the episode ends inside the launch
    control = "Neumann" if mode == "neu_hist" else "Dirchilet"
    hist = mode in ("hist", "neu_hist")
    kw = _kw1d(kind, n, S, nt, control)
    spec, orw = _reward(mode, nt)
    extra = {"flux": flux} if flux else {}
    clean, pois = _mk1d(kind, kw, spec, B, hist, **extra), _mk1d(kind, kw, spec, B, hist, **extra)
    arena = _arena(policy)
    guard_engine(pois, arena)
    init, beta = _init_beta(B, n, seed, f64_beta)
    clean.reset(init, beta)
    pois.reset(init, beta)
    pois.t["beta"] = arena.like("beta", pois.t["beta"])      # (reset installs its own beta tensor: guard the one the steps read)
    for k in OUT1D:                                # pure outputs: poisoned before every call
        if pois.t[k] is not None:
            PZ.poison_(pois.t[k])
    PZ.poison_(pois._obs[pois._flip ^ 1])          # the partner observation buffer (the next step's output)
    if hist:
        PZ.poison_(pois.t["history"][:, 1:])       # rows a step writes: not pre-zeroed (a C-ABI caller need not memset)
    ocls = {"transport": po.TransportOracle, "parabolic": po.ParabolicOracle}[kind]
    if flux == "burgers":
        ocls = po.BurgersOracle
    # (with a trajectory the oracle takes the reward from its history, which needs nt > 100: the reward is compared with the
    # clean run here and with the oracle in the mode without history)
    orc = ocls(reward=None if hist else orw, keep_history=hist, **kw)
    orc.reset(init, beta)
    ak = action_kind or N.ACTION_F32
    rng = np.random.default_rng(seed + 1)
    nsteps = -(-(nt - 1) // S) + 1                  # one call past the episode end too
    t_prev = 0
    for s in range(nsteps):
        a = rng.uniform(-1, 1, B).astype(np.float32)
        at = torch.tensor(a if ak == N.ACTION_F32 else a.astype(np.float64))
        if s > 0:
            for k in OUT1D:
                PZ.poison_(pois.t[k] if k != "obs" else pois._obs[pois._flip ^ 1])
        oc, rc, tec, trc = clean.step(at, action_kind=ak)
        op, rp, tep, trp = pois.step(arena.like(f"action{s}", at.cuda()), action_kind=ak)      # (a [B] device tensor is read in place)
        o_ref, r_ref, te_ref, tr_ref = orc.step(a, {N.ACTION_F32: "f32", N.ACTION_F64: "f64", N.ACTION_WEAK: "weak"}[ak])
        torch.cuda.synchronize()
        arena.check()
        where = f"{kind} n={n} B={B} {mode} step {s}"
        for k in ("obs", "norm_now", "norm_back", "terminated", "truncated") + (("reward",) if mode != "none_reward" else ()):
            PZ.assert_written(pois.t[k], None, f"{where}: {k}", like=clean.t[k])
        if mode == "none_reward":
            PZ.assert_untouched(pois.t["reward"], None, f"{where}: reward under REWARD_NONE")
        # clean run against the oracle: rows / observations bit-exact, flags exact, reward rtol 1e-6 (test_gpu_1d.py)
        np.testing.assert_array_equal(clean.u.cpu().numpy(), orc.row, err_msg=where)
        np.testing.assert_array_equal(oc.cpu().numpy().reshape(o_ref.shape), o_ref, err_msg=where)
        assert np.array_equal(tec.cpu().numpy().astype(bool), te_ref) and np.array_equal(trc.cpu().numpy().astype(bool), tr_ref), where
        if r_ref is not None:
            nrm = float(np.abs(orc.row).max()) * np.sqrt(n)
            np.testing.assert_allclose(rc.cpu().numpy(), r_ref, rtol=1e-6, atol=2e-6 * max(1.0, nrm), err_msg=where)
        PZ.assert_bits_equal(pois.u, clean.u, None, f"{where}: u")
        if hist:
            t_now = int(clean.time_index[0])
            h = pois.t["history"]
            if t_now > t_prev:
                PZ.assert_written(h, (slice(None), slice(t_prev + 1, t_now + 1)), f"{where}: history rows {t_prev + 1}..{t_now}",
                                  like=clean.t["history"])
            if t_now + 1 < h.shape[1]:
                PZ.assert_untouched(h, (slice(None), slice(t_now + 1, None)), f"{where}: history rows past {t_now}")
            np.testing.assert_array_equal(clean.t["history"].cpu().numpy(), orc.hist, err_msg=where)
            t_prev = t_now
    return clean, pois, arena


STEP_CASES = [(kind, _ragged_slots(e) + (kind == "parabolic"), mode) for e in EPLS for kind in ("transport", "parabolic")
              for mode in ("none", "hist", "neu_hist", "diff")]
STEP_CASES += [(kind, _ragged_slots(e) + (kind == "parabolic"), "thor") for e in (1, 3, 8, 12, 32) for kind in ("transport", "parabolic")]


@pytest.mark.parametrize("kind,n,mode", STEP_CASES, ids=[f"{k}-n{n}-{m}" for k, n, m in STEP_CASES])
def test_1d_step_contract(kind, n, mode):
    """One ragged row length per EPL instantiation x {no history, Dirichlet history (HFAST for EPL <= 8, select form above),
    Neumann history, NormReward differential (select form without a buffer)}, and NormReward t-horizon at five of them; B = 5
    leaves a partial 4-wave block."""
    _run_1d_pair(kind, n, 5, mode)


@pytest.mark.parametrize("slots", [64, 128, 256, 512])
@pytest.mark.parametrize("kind", ["transport", "parabolic"])
def test_1d_full_rows(kind, slots):
    """FULL instantiations (n - J0 a whole number of wave rows), B = 1; with a trajectory the HFAST loop on the same shapes."""
    n = slots + (kind == "parabolic")
    _run_1d_pair(kind, n, 1, "none")
    _run_1d_pair(kind, n, 1, "hist")


@pytest.mark.parametrize("epl", [1, 2, 4, 8])
def test_1d_m64_contract(epl):
    """float64 beta, ACTION_F64 and ACTION_WEAK (the reference's mixed precision) at EPL 1, 2, 4, 8."""
    from pdecontrolgym_amd import _native as N
    n = _ragged_slots(epl) + 1
    _run_1d_pair("parabolic", n, 5, "none", f64_beta=True)
    _run_1d_pair("transport", n, 5, "hist", action_kind=N.ACTION_F64)
    _run_1d_pair("parabolic", n, 5, "neu_hist", action_kind=N.ACTION_WEAK)


@pytest.mark.parametrize("n", [2049, 4097])
def test_1d_wide_kernels(n):
    """Rows past the register limit (wave-private LDS), float32 and M64."""
    _run_1d_pair("transport", n, 5, "none", S=2, steps=2)
    _run_1d_pair("parabolic", n, 5, "hist", S=2, steps=2, f64_beta=True)


@pytest.mark.parametrize("kind,n,hist", [("transport", 166, False), ("parabolic", 487, True), ("transport", 2049, False),
                                         ("parabolic", 38, False)])
def test_1d_shared_beta_row_is_not_over_read(kind, n, hist, policy=None):
    """beta_stride = 0 (one beta row for every instance) with NaN right after the row: results equal the clean run and stay finite."""
    B, S, nt = 5, 3, 12
    kw = _kw1d(kind, n, S, nt)
    spec, _ = _reward("none", nt)
    clean, pois = _mk1d(kind, kw, spec, B, hist), _mk1d(kind, kw, spec, B, hist)
    init, beta = _init_beta(B, n, 21)
    for e in (clean, pois):
        e.reset(init, beta[0])                        # a [n] beta: the shared row
    assert clean.t["beta"].dim() == 1
    arena = _arena(policy)
    guard_engine(pois, arena)
    shared = arena.new("beta_shared_nan_tail", (2, n), torch.float32)
    shared[0].copy_(_f32(beta[0]))
    PZ.poison_(shared[1])
    pois.t["beta"] = shared[0]
    rng = np.random.default_rng(22)
    for s in range(5):
        a = _f32(rng.uniform(-1, 1, B))
        for k in OUT1D:
            PZ.poison_(pois.t[k] if k != "obs" else pois._obs[pois._flip ^ 1])
        oc = clean.step(a)[0]
        op = pois.step(a)[0]
        arena.check()
        assert bool(torch.isfinite(op).all()), f"shared beta {kind} n={n} step {s}: non-finite observation"
        for k in OUT1D:
            PZ.assert_written(pois.t[k], None, f"shared beta {kind} n={n} step {s}: {k}", like=clean.t[k])
        PZ.assert_bits_equal(pois.u, clean.u, None, f"shared beta {kind} n={n} step {s}: u")
        if hist:
            PZ.assert_bits_equal(pois.t["history"], clean.t["history"], None, f"shared beta {kind} n={n} step {s}: history")


def test_1d_burgers():
    _run_1d_pair("transport", 300, 5, "none", flux="burgers")


def test_1d_reward_none_leaves_reward_alone():
    _run_1d_pair("transport", 100, 5, "none_reward")
    _run_1d_pair("parabolic", 257, 1, "none_reward")


def test_1d_state_in_leaves_u_alone(policy=None):
    """state_in mode (the engine default for full-state sensing): the rows come from the previous observation; u is not touched."""
    import ctypes as C
    from pdecontrolgym_amd import _native as N
    from pdecontrolgym_amd.batch1d import PDEBatch1D
    B, n, S, nt = 5, 229, 3, 12
    kw = _kw1d("transport", n, S, nt)
    spec, _ = _reward("none", nt)
    clean = PDEBatch1D("transport", reward=spec, num_envs=B, device="cuda", **kw)
    pois = PDEBatch1D("transport", reward=spec, num_envs=B, device="cuda", **kw)
    init, beta = _init_beta(B, n, 3)
    for e in (clean, pois):
        e.reset(init, beta)
    arena = _arena(policy)
    guard_engine(pois, arena)
    u_alone = arena.new("u_alone", (B, n), torch.float32)
    PZ.poison_(u_alone)
    be = pois.backend
    for s in range(3):
        a = _f32(np.random.default_rng(s).uniform(-1, 1, B))
        oc = clean.step(a)[0]
        prev = pois.t["obs"]
        nxt = pois._obs[pois._flip ^ 1]
        PZ.poison_(nxt)
        for k in ("reward", "norm_now", "norm_back", "terminated", "truncated"):
            PZ.poison_(pois.t[k])
        T = dict(pois.t, state_in=prev, obs=nxt, action=a.cuda())
        pois.params.action_kind = N.ACTION_F32
        bufs = be._bufs1d(T)
        bufs.u = u_alone.data_ptr()                 # a live-row buffer next to state_in: the header says it is not touched
        N.check(be.lib.pdegym_transport_step(C.byref(pois.params), C.byref(bufs), B, N.current_stream_ptr()), "state_in step")
        pois._flip ^= 1
        pois.t["obs"] = pois.t["u"] = nxt
        arena.check()
        PZ.assert_written(nxt, None, "state_in: obs", like=oc)
        PZ.assert_untouched(u_alone, None, "state_in: u")
        for k in ("reward", "norm_now", "norm_back", "terminated", "truncated"):
            PZ.assert_written(pois.t[k], None, f"state_in: {k}", like=clean.t[k])


def test_1d_auto_reset_final_obs_and_pools(policy=None):
    """Fused auto-reset with pool rows != B and reset_beta: final_obs rows only for the instances that finished (NaN elsewhere),
    pools read only within their rows (NaN right after the last pool row), results equal to the clean run."""
    B, n, S, nt = 5, 130, 4, 10
    kw = _kw1d("transport", n, S, nt)
    spec, _ = _reward("none", nt)
    clean, pois = _mk1d("transport", kw, spec, B, False), _mk1d("transport", kw, spec, B, False)
    init, beta = _init_beta(B, n, 5)
    P = 7
    pool, bpool = _init_beta(P, n, 6)
    arena = _arena(policy)
    for e in (clean, pois):
        e.reset(init, beta)
    clean.enable_auto_reset(_f32(pool), beta_pool=_f32(bpool))
    # guarded pools with NaN right after row P - 1: the kernel reads rows (b + k B) mod P only
    gp = arena.new("pool", (P + 1, n), torch.float32)
    gb = arena.new("bpool", (P + 1, n), torch.float32)
    gp[:P].copy_(_f32(pool))
    gb[:P].copy_(_f32(bpool))
    PZ.poison_(gp[P:])
    PZ.poison_(gb[P:])
    pois.enable_auto_reset(gp[:P], beta_pool=gb[:P])
    guard_engine(pois, arena, skip=("reset_init", "reset_beta"))
    pois.t["reset_init"], pois.t["reset_beta"] = gp[:P], gb[:P]
    fin_seen = 0
    for s in range(8):
        a = _f32(np.random.default_rng(10 + s).uniform(-1, 1, B))
        for k in OUT1D:
            PZ.poison_(pois.t[k] if k != "obs" else pois._obs[pois._flip ^ 1])
        PZ.poison_(pois.t["final_obs"])
        clean.t["final_obs"].zero_()
        oc, rc, tec, trc = clean.step(a)
        op, rp, tep, trp = pois.step(arena.like(f"action{s}", a.cuda()))
        arena.check()
        fin = (tec | trc).bool().cpu()
        fin_seen += int(fin.sum())
        for k in OUT1D:
            PZ.assert_written(pois.t[k], None, f"auto-reset step {s}: {k}", like=clean.t[k])
        PZ.assert_written(pois.t["final_obs"], fin[:, None].cuda(), f"auto-reset step {s}: final_obs", like=clean.t["final_obs"])
        PZ.assert_untouched(pois.t["final_obs"], ~fin[:, None].cuda(), f"auto-reset step {s}: final_obs of running instances")
        for k in ("u", "beta", "time_index", "bsum", "ring", "reset_count"):
            PZ.assert_bits_equal(pois.t[k], clean.t[k], None, f"auto-reset step {s}: {k}")
    assert fin_seen >= 2 * B


def test_1d_masked_reset_leaves_others_alone(policy=None):
    """pdegym_reset1d_masked: unmasked instances keep the poison in every output the reset writes (history included)."""
    B, n, nt = 5, 101, 9
    kw = _kw1d("parabolic", n, 2, nt)
    spec, _ = _reward("none", nt)
    env = _mk1d("parabolic", kw, spec, B, True)
    arena = _arena(policy)
    guard_engine(env, arena)
    init, beta = _init_beta(B, n, 8)
    env.set_beta(beta)
    mask = arena.like("mask", torch.tensor([1, 0, 1, 0, 0], dtype=torch.uint8, device="cuda"))
    init_t = arena.like("init", _f32(init).cuda())
    if policy is not None:
        assert mask.data_ptr() % 16 != 0 and init_t.data_ptr() % 16 != 0
    for k in ("u", "bsum", "ring", "obs", "history"):
        PZ.poison_(env.t[k])
    PZ.fill_int_(env.t["time_index"], nt // 2)
    env.backend.reset1d(env.params, env.t, init_t, mask, B)
    arena.check()
    on, off = mask.bool(), ~mask.bool()
    for k in ("u", "bsum", "obs", "history"):
        sel = on.view(-1, *([1] * (env.t[k].dim() - 1))).expand(env.t[k].shape)
        PZ.assert_written(env.t[k], sel, f"masked reset: {k} of masked instances")
        PZ.assert_untouched(env.t[k], ~sel, f"masked reset: {k} of other instances")
    PZ.assert_written(env.t["ring"], (on, 0), "masked reset: ring slot 0")
    PZ.assert_untouched(env.t["ring"], off, "masked reset: ring of other instances")
    assert env.t["time_index"].cpu().tolist() == [0, nt // 2, 0, nt // 2, nt // 2]
    h = env.t["history"].cpu().numpy()
    np.testing.assert_array_equal(h[[0, 2], 0], init[[0, 2]])
    assert not h[[0, 2], 1:].any()
    np.testing.assert_array_equal(env.t["obs"].cpu().numpy()[[0, 2]], init[[0, 2]])


@pytest.mark.parametrize("kind", ["transport", "parabolic"])
def test_1d_reset_initialises_poisoned_state(kind, policy=None):
    """reset(mask=None) over NaN state (ring, bsum, u, obs) and in-range wrong integers, then a whole episode past the look-back:
    every output equals the clean run (ring slots 1..127 and look-back rows are read here) and the oracle."""
    from oracle import pde_oracle as po
    B, S, nt = 5, 10, 161
    n = 77 + (kind == "parabolic")
    kw = _kw1d(kind, n, S, nt)
    spec, orw = _reward("none", nt)
    clean, pois = _mk1d(kind, kw, spec, B, False), _mk1d(kind, kw, spec, B, False)
    arena = _arena(policy)
    guard_engine(pois, arena)
    for k in ("u", "bsum", "ring", "obs", "norm_now", "norm_back", "reward", "terminated", "truncated"):
        PZ.poison_(pois.t[k])
    for o in pois._obs:
        PZ.poison_(o)
    PZ.fill_int_(pois.t["time_index"], nt // 2)
    init, beta = _init_beta(B, n, 9)
    clean.reset(init, beta)
    pois.reset(init, beta)
    orc = {"transport": po.TransportOracle, "parabolic": po.ParabolicOracle}[kind](reward=orw, keep_history=False, **kw)
    orc.reset(init, beta)
    rng = np.random.default_rng(4)
    for s in range((nt - 1) // S + 1):
        a = rng.uniform(-1, 1, B).astype(np.float32)
        oc, rc, _, _ = clean.step(_f32(a))
        pois.step(_f32(a))
        _, r_ref, _, _ = orc.step(a)
        arena.check()
        for k in OUT1D:
            PZ.assert_bits_equal(pois.t[k], clean.t[k], None, f"{kind} after poisoned reset, step {s}: {k}")
        np.testing.assert_array_equal(oc.cpu().numpy(), orc.row)
        nrm = float(np.abs(orc.row).max()) * np.sqrt(n)
        np.testing.assert_allclose(rc.cpu().numpy(), r_ref, rtol=1e-6, atol=2e-6 * max(1.0, nrm))


ROLLOUT_1D_CASES = [("parabolic", 257, "Dirchilet", "full"), ("transport", 229, "Dirchilet", "full"), ("parabolic", 101, "Neumann", "full"),
                    ("transport", 150, "Dirchilet", "collocated")]


def test_1d_rollout_contract(policy=None, cases=ROLLOUT_1D_CASES, lengths=(1, 7), widths=(32, 128)):
    """pdegym_*_rollout: FULL, plain and general (Neumann, scalar sensing) forms, with and without an in-kernel policy, T in {1, 7}:
    every written slot equals T step calls; obs[0] is left alone; obs_seen receives obs + obs_noise.  ``lengths``: the T of each
    rollout; ``widths``: the policy's hidden units at the first T (one fma chain per neuron up to 64) and at every other one."""
    from pdecontrolgym_amd.batch1d import PDEBatch1D
    from pdecontrolgym_amd.policy import FusedMLP
    for (kind, n, ctl, sens) in cases:
        for Tn in lengths:
            for use_policy in (False, True):
                B, S, nt = 5, 3, 30
                kw = _kw1d(kind, n, S, nt, ctl, sens)
                spec, _ = _reward("none", nt)
                ref = PDEBatch1D(kind, reward=spec, num_envs=B, device="cuda", **kw)
                env = PDEBatch1D(kind, reward=spec, num_envs=B, device="cuda", **kw)
                init, beta = _init_beta(B, n, 11)
                for e in (ref, env):
                    e.reset(init, beta)
                arena = _arena(policy)
                guard_engine(env, arena)
                od = env.obs_dim
                obs = arena.new("ro_obs", (Tn + 1, B, od), torch.float32)
                obs[0].copy_(env.t["obs"])
                PZ.poison_(obs[1:])
                acts = arena.new("ro_actions", (Tn, B), torch.float32)
                rew = arena.new("ro_rewards", (Tn, B), torch.float32)
                te = arena.new("ro_term", (Tn, B), torch.uint8)
                tr = arena.new("ro_trunc", (Tn, B), torch.uint8)
                for x in (rew, te, tr):
                    PZ.poison_(x)
                pol, kwp = None, {}
                if use_policy:
                    torch.manual_seed(0)
                    width = widths[0] if Tn == lengths[0] else widths[1]          # one fma chain per neuron / the cooperative MFMA form
                    mod = torch.nn.Sequential(torch.nn.Linear(od, width), torch.nn.Tanh(), torch.nn.Linear(width, 1)).cuda()
                    pol = FusedMLP(mod, clamp=(-1.0, 1.0))
                    PZ.poison_(acts)
                    on = arena.new("obs_noise", (Tn, B, od), torch.float32)
                    on.copy_(torch.randn(Tn, B, od) * 0.01)
                    seen = arena.new("obs_seen", (Tn, B, od), torch.float32)
                    PZ.poison_(seen)
                    kwp = dict(obs_noise=on, obs_seen=seen)
                else:
                    acts.copy_(torch.rand(Tn, B) * 2 - 1)
                slot0 = obs[0].clone()
                env.rollout(obs, acts, rew, te, tr, policy=pol, **kwp)
                arena.check()
                where = f"rollout {kind} n={n} {ctl}/{sens} T={Tn} policy={use_policy}"
                PZ.assert_bits_equal(obs[0], slot0, None, f"{where}: obs[0]")
                for x, nm in ((obs[1:], "obs"), (rew, "rewards"), (te, "terminated"), (tr, "truncated")):
                    PZ.assert_written(x, None, f"{where}: {nm}")
                if use_policy:
                    PZ.assert_written(acts, None, f"{where}: actions")
                    PZ.assert_written(kwp["obs_seen"], None, f"{where}: obs_seen")
                    torch.testing.assert_close(kwp["obs_seen"], obs[:-1] + kwp["obs_noise"], rtol=0, atol=0)
                for t in range(Tn):            # the same commands through step calls: bit for bit
                    o, r, a_te, a_tr = ref.step(acts[t].clone())
                    PZ.assert_bits_equal(obs[t + 1], o.reshape(B, od), None, f"{where}: obs[{t + 1}]")
                    PZ.assert_bits_equal(te[t], a_te, None, f"{where}: terminated[{t}]")
                    PZ.assert_bits_equal(tr[t], a_tr, None, f"{where}: truncated[{t}]")
                    PZ.assert_bits_equal(rew[t], r, None, f"{where}: rewards[{t}]")


def test_1d_host_io_prepared_call_follows_replaced_tensors():
    """enable_host_io's prepared call must not keep the addresses of tensors replaced by enable_auto_reset / disable_auto_reset /
    set_beta / load_state_dict: after each, step_host with poisoned outputs equals step() on a twin engine."""
    from pdecontrolgym_amd import _native as N
    from pdecontrolgym_amd.batch1d import PDEBatch1D
    B, n, S, nt = 1, 60, 5, 12                     # the episode ends on the third step: the auto-reset pools are read there
    kw = _kw1d("transport", n, S, nt)
    spec, _ = _reward("tuned", nt)
    a = PDEBatch1D("transport", reward=spec, num_envs=B, device="cuda", state_in_obs=False, **kw)
    b = PDEBatch1D("transport", reward=spec, num_envs=B, device="cuda", state_in_obs=False, **kw)
    io = a.enable_host_io()
    init, beta = _init_beta(B, n, 12)
    a.reset(init, beta)
    b.reset(init, beta)
    np.testing.assert_array_equal(io["obs"], b.t["obs"].cpu().numpy())
    # the host outputs of the pack (pinned host memory the kernel writes in place) move into guarded pinned buffers
    host = PZ.Arena("cuda", pinned=True)
    OUT = ("obs", "reward", "norm_now", "terminated", "truncated")
    for k in OUT:
        assert a.t[k].is_pinned(), k
        a.t[k] = host.like(k, a.t[k])
    a._obs = [a.t["obs"], a.t["obs"]]
    rng = np.random.default_rng(13)

    def both(tag):
        v = float(np.float32(rng.uniform(-1, 1)))
        for k in OUT:
            PZ.poison_(a.t[k])
        a.step_host(v, N.ACTION_F32)
        o, r, te, tr = b.step(torch.tensor([v], dtype=torch.float32))
        torch.cuda.synchronize()
        host.check()
        for k in OUT:
            PZ.assert_written(a.t[k], None, f"{tag}: host {k}", like=b.t[k].cpu())
        PZ.assert_bits_equal(a.t["u"], b.t["u"], None, f"{tag}: u")
        PZ.assert_bits_equal(a.t["ring"], b.t["ring"], None, f"{tag}: ring")
    both("first")
    pool, bpool = _init_beta(3, n, 14)
    for e in (a, b):
        e.enable_auto_reset(_f32(pool), beta_pool=_f32(bpool))
    both("enable_auto_reset")
    both("enable_auto_reset, episode end")
    for e in (a, b):
        e.disable_auto_reset()
    both("disable_auto_reset")
    nb = _init_beta(B, n, 15)[1]
    for e in (a, b):
        e.set_beta(nb.astype(np.float64))
    both("set_beta float64")
    sd = b.state_dict()
    a.t["ring"] = torch.zeros(B, 64, device="cuda")      # a tensor of another shape: load_state_dict replaces it
    a.load_state_dict(sd)
    both("load_state_dict")


def test_ns_host_io_prepared_call_follows_replaced_tensors():
    from pdecontrolgym_amd.batch2d import NSBatch2D
    from tests.test_gpu_ns2d import _random_case, BC_MIX
    kw, u0, v0, p0, acts = _random_case(21, 1, 20, 3, BC_MIX)
    a = NSBatch2D(num_envs=1, device="cuda", dtype=torch.float64, interleaved_state=False, **kw)
    b = NSBatch2D(num_envs=1, device="cuda", dtype=torch.float64, interleaved_state=False, **kw)
    io = a.enable_host_io()
    for e in (a, b):
        e.reset(u0, v0, p0)

    def both(tag, act):
        for k in ("obs", "reward"):
            PZ.poison_(a.t[k])
        io["action"][:] = act
        a.step_host()
        o, r, _ = b.step(np.full(1, act))
        torch.cuda.synchronize()
        np.testing.assert_array_equal(io["obs"], o.cpu().numpy(), err_msg=tag)
        np.testing.assert_array_equal(io["reward"], r.cpu().numpy(), err_msg=tag)
    both("first", 2.5)
    pools = [np.repeat(x[None], 2, 0) for x in (u0[0], v0[0], p0[0])]
    for e in (a, b):
        e.enable_auto_reset(*pools)
    both("enable_auto_reset", 3.0)
    for e in (a, b):
        e.disable_auto_reset()
    both("disable_auto_reset", 2.0)
    sd = b.state_dict()
    a.t["p"] = torch.zeros(1, 3, device="cuda", dtype=torch.float64)
    a.load_state_dict(sd)
    both("load_state_dict", 2.2)


def test_rownorm2_ragged(policy=None):
    from pdecontrolgym_amd.backend import default_backend
    be = default_backend()
    for B, n in ((1, 1), (5, 63), (7, 65), (3, 2049)):
        arena = _arena(policy)
        rows = arena.new("rows", (B, n), torch.float32)
        rows.copy_(torch.randn(B, n))
        out = arena.new("out", (B,), torch.float32)
        PZ.poison_(out)
        be.rownorm2(rows, out)
        arena.check()
        PZ.assert_written(out, None, f"rownorm2 B={B} n={n}")
        ref = np.linalg.norm(rows.cpu().numpy().astype(np.float64), axis=1)
        np.testing.assert_allclose(out.cpu().numpy(), ref, rtol=4 * 2.0 ** -24 * (n + 2))   # float32 sum of n squares


def test_selftest_quotient_counter_only(policy=None):
    """pdegym_selftest_quotient writes the one counter it is given and nothing past it."""
    import ctypes as C
    from pdecontrolgym_amd import _native as N
    lib = N.load()
    arena = _arena(policy)
    a = arena.new("a", (1000,), torch.float32)
    a.copy_(torch.randn(1000))
    cnt = arena.new("count", (1,), torch.int32)
    dx = C.c_float(0.01).value
    N.check(lib.pdegym_selftest_quotient(a.data_ptr(), C.c_float(dx), 1.0 / dx, cnt.data_ptr(), 1000, N.current_stream_ptr()),
            "pdegym_selftest_quotient")
    arena.check()
    assert int(cnt.item()) == 0


# ---- Navier-Stokes ---------------------------------------------------------------------------------------------------------
NS_OUT = ("reward", "terminated")


def _ns_pair(n, B, K, dtype, ny=None, steps=2, seed=0, interleaved=True, dispatch=None, p_out=False, oracle=False,
             poison_state=False, policy=None):
    """Clean and guarded+poisoned NSBatch2D over the same steps; scratch, the partner observation and p_out start as NaN."""
    from pdecontrolgym_amd import _native as N
    from pdecontrolgym_amd.batch2d import NSBatch2D
    from tests.test_gpu_ns2d import _random_case, BC_MIX
    from oracle import pde_oracle as po
    kw, u0, v0, p0, acts = _random_case(n, B, K, seed, BC_MIX)
    if ny is not None and ny != n:            # a non-square grid: rows ny, columns n (dy = dx)
        kw = dict(kw, Y=(ny - 1) * kw["dx"], U_ref=kw["U_ref"][:, :1].repeat(ny, 1))
        u0, v0, p0 = (np.ascontiguousarray(np.resize(x, (B, ny, n))) for x in (u0, v0, p0))
    clean = NSBatch2D(num_envs=B, device="cuda", dtype=dtype, interleaved_state=interleaved, **kw)
    pois = NSBatch2D(num_envs=B, device="cuda", dtype=dtype, interleaved_state=interleaved, **kw)
    if p_out and pois.t["p_out"] is None:
        for e in (clean, pois):
            e.t["p_out"] = torch.zeros_like(e.t["p"])
            e._p_pingpong = True
    arena = _arena(policy)
    guard_engine(pois, arena)
    # U_ref / action_ref with NaN right after their stated extent (nt_ref rows)
    U = arena.new("U_ref_nan_tail", (pois.t["U_ref"].shape[0] + 1,) + tuple(pois.t["U_ref"].shape[1:]), dtype)
    U[:-1].copy_(pois.t["U_ref"])
    PZ.poison_(U[-1:])
    pois.t["U_ref"] = U[:-1]
    A = arena.new("action_ref_nan_tail", (pois.t["action_ref"].shape[0] + 1,), dtype)
    A[:-1].copy_(pois.t["action_ref"])
    PZ.poison_(A[-1:])
    pois.t["action_ref"] = A[:-1]
    PZ.poison_(pois.t["scratch"])
    if poison_state:             # everything a full reset claims to initialise (integers: in-range wrong values)
        for k in ("u", "v", "p", "p_out"):
            if pois.t[k] is not None:
                PZ.poison_(pois.t[k])
        for o in pois._obs:
            PZ.poison_(o)
        PZ.fill_int_(pois.t["time_index"], pois.nt // 2)
    ctx = N.ns_dispatch(**(dispatch or {}))
    with ctx:
        clean.reset(u0, v0, p0)
        pois.reset(*(arena.like(k, torch.as_tensor(x, dtype=dtype, device="cuda")) for k, x in (("u0", u0), ("v0", v0), ("p0", p0))))
        orc = None
        if oracle:
            orc = po.NavierStokesOracle(**kw)
            rep = (lambda x: np.asarray(x, dtype=np.float32).astype(np.float64)) if dtype == torch.float32 else np.asarray
            orc.reset(rep(u0), rep(v0), rep(p0))      # (float32: from the same float32-representable state, test_gpu_ns2d.py)
        for s in range(steps):
            a = acts[s % len(acts)]
            for k in NS_OUT:
                PZ.poison_(pois.t[k])
            PZ.poison_(pois._obs[pois._flip ^ 1])
            PZ.poison_(pois.t["scratch"])
            if pois.t["p_out"] is not None:
                PZ.poison_(pois.t["p_out"])
            oc, rc, tc = clean.step(a)
            op, rp, tp = pois.step(arena.like(f"action{s}", torch.as_tensor(np.asarray(a), dtype=dtype, device="cuda").reshape(B, -1)))
            arena.check()
            where = f"NS {dtype} {ny or n}x{n} B={B} K={K} {dispatch} step {s}"
            PZ.assert_written(op, None, f"{where}: obs", like=oc)
            PZ.assert_written(rp, None, f"{where}: reward", like=rc)
            PZ.assert_written(tp, None, f"{where}: terminated", like=tc)
            PZ.assert_bits_equal(pois.t["p"], clean.t["p"], None, f"{where}: p")
            if not interleaved:
                for k in ("u", "v"):
                    PZ.assert_bits_equal(pois.t[k], clean.t[k], None, f"{where}: {k}")
            if orc is not None and (dtype == torch.float64 or s == 0):   # float32: one step from the same state (test_gpu_ns2d.py)
                o_ref, r_ref, _, _ = orc.step(rep(a).astype(np.float64))
                o = oc.cpu().numpy().astype(np.float64)
                if dtype == torch.float64:
                    np.testing.assert_array_equal(o, o_ref, err_msg=where)
                    np.testing.assert_allclose(rc.cpu().numpy(), r_ref, rtol=1e-12, err_msg=where)
                else:                                  # test_gpu_ns2d.py tolerances (f32 against the f64 oracle)
                    np.testing.assert_allclose(o, o_ref, rtol=1e-5, atol=2e-6 * np.abs(o_ref).max(), err_msg=where)
                    np.testing.assert_allclose(rc.cpu().numpy(), r_ref, rtol=1e-4, err_msg=where)
    return clean, pois, arena


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("ny", [8, 11, 16, 21, 26, 31, 32])
def test_ns_column_kernel_contract(ny, dtype):
    """Column-per-lane kernel at every height; nx = 21 packs 3 instances per wave, B = 5 leaves a partial wave.  float64 both
    with the two-wave and the one-wave (_w1) build (col_min_batch forces the column kernel at a small batch)."""
    dt = getattr(torch, dtype)
    _ns_pair(21, 5, 9, dt, ny=ny, dispatch=dict(col_min_batch=0), oracle=(ny == 21))
    if dtype == "float64" and ny in (16, 21, 26):
        _ns_pair(21, 4, 9, dt, ny=ny, dispatch=dict(col_min_batch=0), steps=1, seed=1)
        _ns_pair(21, 4000, 3, dt, ny=ny, dispatch=dict(col_min_batch=0), steps=1, seed=2)


@pytest.mark.parametrize("case", ["t64", "t64_sep", "t128", "t128_sep", "t128_f64", "gen0", "gen1", "gen2", "gen_f32"])
def test_ns_tile_and_generic_contract(case):
    """f32 tiles 64^2 / 128^2 (state_in and separate fields), f64 tile 128^2, the workgroup kernel's three LDS modes."""
    f32, f64 = torch.float32, torch.float64
    if case.startswith("t64"):
        _ns_pair(64, 3, 11, f32, interleaved=not case.endswith("sep"), oracle=True)
    elif case.startswith("t128") and case != "t128_f64":
        _ns_pair(128, 2, 11, f32, interleaved=not case.endswith("sep"))
    elif case == "t128_f64":
        _ns_pair(128, 2, 11, f64, oracle=True)
    elif case == "gen0":
        _ns_pair(40, 3, 11, f64, dispatch=dict(generic=True, no_lds_jacobi=True), oracle=True)
    elif case == "gen1":
        _ns_pair(40, 3, 11, f64, dispatch=dict(generic=True), p_out=True)
    elif case == "gen2":
        _ns_pair(100, 2, 11, f64, dispatch=dict(generic=True), interleaved=False)
    else:
        _ns_pair(33, 3, 7, f32, dispatch=dict(generic=True, no_col=True))


@pytest.mark.parametrize("case", ["col_f64", "col_f32_sep", "tile64_f32", "generic_f64_pout"])
def test_ns_reset_initialises_poisoned_state(case):
    """reset(mask=None) over NaN u / v / p / observations / p_out and an in-range wrong time index, then a whole episode (and, without
    the oracle, two steps past its end): every step equals the clean run, and for float64 on the column kernel the oracle."""
    f32, f64 = torch.float32, torch.float64
    if case == "col_f64":
        _ns_pair(21, 5, 7, f64, steps=7, dispatch=dict(col_min_batch=0), poison_state=True, oracle=True)   # nt = 8: the episode
    elif case == "col_f32_sep":
        _ns_pair(21, 5, 7, f32, steps=9, interleaved=False, poison_state=True)
    elif case == "tile64_f32":
        _ns_pair(64, 3, 7, f32, steps=9, poison_state=True)
    else:
        _ns_pair(40, 3, 7, f64, steps=9, dispatch=dict(generic=True), p_out=True, poison_state=True)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("interleaved", [True, False])
def test_ns256_contract(dtype, interleaved):
    """256 x 256 pipelines (f32 fused step, f64 slab passes) with iters = 51, not a multiple of the f64 slab pass."""
    _ns_pair(256, 2, 51, getattr(torch, dtype), interleaved=interleaved, steps=2)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_ns_solve_pressure_contract(dtype, policy=None):
    """pdegym_ns2d_solve_pressure_*: aliasing and non-aliasing p_out; scratch starts as NaN; only p_out is written."""
    from pdecontrolgym_amd.batch2d import NSBatch2D
    from tests.test_gpu_ns2d import _random_case, BC_MIX
    dt = getattr(torch, dtype)
    for n in (21, 40):
        kw, u0, v0, p0, _ = _random_case(n, 3, 13, 5, BC_MIX)
        env = NSBatch2D(num_envs=3, device="cuda", dtype=dt, **kw)
        be = env.backend
        arena = _arena(policy)
        u = arena.like("u", torch.tensor(u0, dtype=dt))
        v = arena.like("v", torch.tensor(v0, dtype=dt))
        p_in = arena.like("p_in", torch.tensor(p0, dtype=dt))
        p_out = arena.new("p_out", p_in.shape, dt)
        scratch = arena.new("scratch", (3, 2, n, n), dt)
        PZ.poison_(p_out)
        PZ.poison_(scratch)
        be.ns2d_solve_pressure(env.params, u, v, p_in, p_out, scratch, 3)
        arena.check()
        PZ.assert_written(p_out, None, f"solve_pressure {dtype} n={n}: p_out")
        ref = p_out.clone()
        PZ.poison_(scratch)
        be.ns2d_solve_pressure(env.params, u, v, p_in, p_in, scratch, 3)       # aliasing: in place
        arena.check()
        PZ.assert_bits_equal(p_in, ref, None, f"solve_pressure {dtype} n={n}: p_out aliasing p_in")


def test_ns_masked_reset_leaves_others_alone(policy=None):
    from pdecontrolgym_amd.batch2d import NSBatch2D
    from tests.test_gpu_ns2d import _random_case, BC_MIX
    for dt in (torch.float32, torch.float64):
        kw, u0, v0, p0, _ = _random_case(21, 5, 5, 6, BC_MIX)
        env = NSBatch2D(num_envs=5, device="cuda", dtype=dt, interleaved_state=False, **kw)
        arena = _arena(policy)
        guard_engine(env, arena)
        for k in ("u", "v", "p", "obs"):
            PZ.poison_(env.t[k])
        PZ.fill_int_(env.t["time_index"], 3)
        mask = arena.like("mask", torch.tensor([0, 1, 1, 0, 1], dtype=torch.uint8, device="cuda"))
        fields = [arena.like(k, torch.as_tensor(x, dtype=dt, device="cuda")) for k, x in (("u0", u0), ("v0", v0), ("p0", p0))]
        if policy is not None:
            assert all(x.data_ptr() % 16 != 0 for x in fields + [mask])
        env.reset(*fields, mask=mask)
        arena.check()
        on = mask.bool()
        for k in ("u", "v", "p", "obs"):
            sel = on.view(-1, *([1] * (env.t[k].dim() - 1))).expand(env.t[k].shape)
            PZ.assert_written(env.t[k], sel, f"ns masked reset {dt}: {k}")
            PZ.assert_untouched(env.t[k], ~sel, f"ns masked reset {dt}: {k} of other instances")
        assert env.t["time_index"].cpu().tolist() == [3, 0, 0, 3, 0]


def test_ns_auto_reset_final_obs(policy=None):
    """Fused NS auto-reset: final_obs only for finishing instances (NaN elsewhere), pools with NaN after the last pool row."""
    from pdecontrolgym_amd.batch2d import NSBatch2D
    from tests.test_gpu_ns2d import _random_case, BC_MIX
    for dt, n in ((torch.float64, 21), (torch.float32, 40)):
        B, P = 5, 7
        kw, u0, v0, p0, acts = _random_case(n, P, 5, 7, BC_MIX)
        kw = dict(kw, T=3 * kw["dt"], U_ref=kw["U_ref"][:3], action_ref=kw["action_ref"][:3])
        clean = NSBatch2D(num_envs=B, device="cuda", dtype=dt, **kw)
        pois = NSBatch2D(num_envs=B, device="cuda", dtype=dt, **kw)
        arena = _arena(policy)
        pools = []
        for nm, x in (("u0", u0), ("v0", v0), ("p0", p0)):
            g = arena.new("pool_" + nm, (P + 1, n, n), dt)
            g[:P].copy_(torch.tensor(x, dtype=dt))
            PZ.poison_(g[P:])
            pools.append(g[:P])
        clean.enable_auto_reset(u0, v0, p0)
        pois.enable_auto_reset(*pools)
        guard_engine(pois, arena, skip=("reset_u0", "reset_v0", "reset_p0"))
        for e in (clean, pois):
            e.reset(u0[:B], v0[:B], p0[:B])
        PZ.fill_int_(pois.t["time_index"], 0)
        with_te = 0
        for s in range(7):
            PZ.poison_(pois.t["final_obs"])
            clean.t["final_obs"].zero_()
            PZ.poison_(pois._obs[pois._flip ^ 1])
            PZ.poison_(pois.t["scratch"])
            a = acts[s % 3][:B]
            oc, rc, tc = clean.step(a)
            op, rp, tp = pois.step(a)
            arena.check()
            fin = tc.bool()
            with_te += int(fin.sum())
            sel = fin.view(-1, 1, 1, 1).expand(op.shape)
            PZ.assert_written(op, None, f"ns auto-reset {dt} step {s}: obs", like=oc)
            PZ.assert_written(pois.t["final_obs"], sel, f"ns auto-reset {dt} step {s}: final_obs", like=clean.t["final_obs"])
            PZ.assert_untouched(pois.t["final_obs"], ~sel, f"ns auto-reset {dt} step {s}: final_obs of running instances")
            PZ.assert_bits_equal(pois.t["p"], clean.t["p"], None, "p")
            PZ.assert_bits_equal(pois.t["reset_count"], clean.t["reset_count"], None, "reset_count")
        assert with_te >= B


def test_ns_rollout_contract(policy=None):
    """pdegym_ns2d_rollout_*: slots 1..T written and equal to step calls, slot 0 untouched, no stray writes."""
    from pdecontrolgym_amd.batch2d import NSBatch2D
    from tests.test_gpu_ns2d import _random_case, BC_MIX
    for dt in (torch.float32, torch.float64):
        for ny in (8, 21, 32):
            B, Tn = 5, 3
            kw, u0, v0, p0, acts = _random_case(21, B, 7, 8, BC_MIX)
            if ny != 21:
                kw = dict(kw, Y=(ny - 1) * kw["dx"], U_ref=kw["U_ref"][:, :1].repeat(ny, 1))
                u0, v0, p0 = (np.ascontiguousarray(np.resize(x, (B, ny, 21))) for x in (u0, v0, p0))
            ref = NSBatch2D(num_envs=B, device="cuda", dtype=dt, **kw)
            env = NSBatch2D(num_envs=B, device="cuda", dtype=dt, **kw)
            for e in (ref, env):
                e.reset(u0, v0, p0)
            arena = _arena(policy)
            guard_engine(env, arena)
            PZ.poison_(env.t["scratch"])
            obs = arena.new("ro_obs", (Tn + 1, B, ny, 21, 2), dt)
            obs[0].copy_(env.t["obs"])
            PZ.poison_(obs[1:])
            A = arena.like("ro_actions", torch.tensor(np.stack(acts[:Tn]), dtype=dt))
            rew = PZ.poison_(arena.new("ro_rewards", (Tn, B), dt))
            te = PZ.poison_(arena.new("ro_term", (Tn, B), torch.uint8))
            slot0 = obs[0].clone()
            env.rollout(obs, A, rew, te)
            arena.check()
            PZ.assert_bits_equal(obs[0], slot0, None, "ns rollout obs[0]")
            for t in range(Tn):
                o, r, tt = ref.step(acts[t])
                PZ.assert_written(obs[t + 1], None, f"ns rollout {dt} ny={ny}: obs[{t + 1}]", like=o)
                PZ.assert_written(te[t], None, f"ns rollout {dt} ny={ny}: terminated[{t}]", like=tt)
                PZ.assert_written(rew[t], None, f"ns rollout {dt} ny={ny}: rewards[{t}]")
                PZ.assert_bits_equal(rew[t], r, None, f"ns rollout {dt} ny={ny}: rewards[{t}] against step calls")   # canonical order


# ---- traffic -------------------------------------------------------------------------------------------------------------
def _traffic(M_dx, B, sim="outlet", T=0.5):
    from pdecontrolgym_amd.batch_traffic import TrafficBatch
    X = 500 if M_dx == 10 else 500 * 4
    return TrafficBatch(T, 0.25, X, 10, sim, 40, 0.16, 60, True, 3, num_envs=B, device="cuda")


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("B", [1, 5])
def test_traffic_contract(B, wide, policy=None):
    """Register (M = 51) and wide (M = 201) step kernels, reset, masked reset: outputs complete, others untouched, guards intact."""
    for sim in ("outlet", "both"):
        clean, pois = _traffic(10 if not wide else 40, B, sim), _traffic(10 if not wide else 40, B, sim)
        arena = _arena(policy)
        guard_engine(pois, arena)
        rs = np.random.default_rng(1).uniform(0.1, 0.14, B)
        for k in ("r", "y", "obs", "time"):
            PZ.poison_(pois.t[k])
        for o in pois._obs:
            PZ.poison_(o)
        clean.reset(rs)
        pois.reset(arena.like("rs", torch.as_tensor(rs, device="cuda")))      # (reset adopts the tensor it is given)
        arena.check()
        for k in ("r", "y", "time"):
            PZ.assert_written(pois.t[k], None, f"traffic reset: {k}", like=clean.t[k])
        PZ.assert_written(pois.t["obs"], None, "traffic reset: obs", like=clean.t["obs"])
        A = 2 if sim == "both" else 1
        rng = np.random.default_rng(2)
        for s in range(10):          # T / dt = 2 s: five episode ends, the kernel keeps stepping a finished episode
            a = rng.uniform(0.9, 1.1, (B, A)) * clean.t["qs_clip"].cpu().numpy()[:, None]
            for k in ("reward", "done", "truncated"):
                PZ.poison_(pois.t[k])
            PZ.poison_(pois._obs[pois._flip ^ 1])
            oc = clean.step(a if A == 2 else a[:, 0])
            op = pois.step(arena.like(f"action{s}", torch.as_tensor(np.ascontiguousarray(a if A == 2 else a[:, 0]), device="cuda")))
            arena.check()
            for x, y, nm in zip(op, oc, ("obs", "reward", "done", "truncated")):
                PZ.assert_written(x, None, f"traffic {sim} M={clean.M} B={B} step {s}: {nm}", like=y)
            for k in ("r", "y", "time"):
                PZ.assert_bits_equal(pois.t[k], clean.t[k], None, f"traffic step {s}: {k}")
        if B > 1:
            for k in ("r", "y", "obs", "time"):
                PZ.poison_(pois.t[k])
            mask = arena.like("mask", torch.tensor([1] + [0] * (B - 1), dtype=torch.uint8, device="cuda"))
            if policy is not None:
                assert mask.data_ptr() % 16 != 0 and pois.t["rs"].data_ptr() % 16 != 0
            pois.reset(rs, mask=mask)
            arena.check()
            for k in ("r", "y", "obs", "time"):
                t = pois.t[k]
                sel = mask.bool().view(-1, *([1] * (t.dim() - 1))).expand(t.shape)
                PZ.assert_written(t, sel, f"traffic masked reset: {k}")
                PZ.assert_untouched(t, ~sel, f"traffic masked reset: {k} of other instances")


def test_traffic_rollout_contract(policy=None):
    """All three rollout instantiations (no policy; policy of <= 64 units; policy of 65..256 units)."""
    from pdecontrolgym_amd.policy import FusedMLP
    for width in (None, 32, 128):
        B, Tn = 5, 3
        ref, env = _traffic(10, B), _traffic(10, B)
        rs = np.random.default_rng(3).uniform(0.1, 0.14, B)
        for e in (ref, env):
            e.reset(rs)
        arena = _arena(policy)
        guard_engine(env, arena)
        M = env.M
        obs = arena.new("ro_obs", (Tn + 1, B, 2 * M), torch.float64)
        obs[0].copy_(env.t["obs"])
        PZ.poison_(obs[1:])
        acts = arena.new("ro_actions", (Tn, B, 1), torch.float64)
        rew = PZ.poison_(arena.new("ro_rewards", (Tn, B), torch.float64))
        dn = PZ.poison_(arena.new("ro_done", (Tn, B), torch.uint8))
        tr = PZ.poison_(arena.new("ro_trunc", (Tn, B), torch.uint8))
        pol = None
        if width is None:
            acts.copy_(torch.tensor(np.random.default_rng(4).uniform(0.9, 1.1, (Tn, B, 1))) * ref.t["qs_clip"].cpu()[None, :, None])
        else:
            torch.manual_seed(1)
            mod = torch.nn.Sequential(torch.nn.Linear(2 * M, width), torch.nn.Tanh(), torch.nn.Linear(width, 1)).cuda()
            pol = FusedMLP(mod)
            PZ.poison_(acts)
        slot0 = obs[0].clone()
        env.rollout(obs, acts, rew, dn, tr, policy=pol)
        arena.check()
        PZ.assert_bits_equal(obs[0], slot0, None, "traffic rollout obs[0]")
        for t in range(Tn):
            o, r, d, tt = ref.step(acts[t].clone()[:, 0])
            where = f"traffic rollout width={width} t={t}"
            PZ.assert_written(obs[t + 1], None, f"{where}: obs", like=o)
            PZ.assert_written(rew[t], None, f"{where}: reward", like=r)
            PZ.assert_written(dn[t], None, f"{where}: done", like=d)
            PZ.assert_written(tr[t], None, f"{where}: truncated", like=tt)


# ---- tumour --------------------------------------------------------------------------------------------------------------
def _tumor(nx_big, B):
    from pdecontrolgym_amd.batch_tumor import TumorBatch
    X = 200 if not nx_big else 400
    return TumorBatch(60, 1, X, 1, 61.2, num_envs=B, device="cuda", record_history=True), X


@pytest.mark.parametrize("nx_big", [False, True])
def test_tumor_contract(nx_big, policy=None):
    """Both row-staging paths (nx <= 256, larger).  Reset over poisoned state (init_stride 0), step with an active mask, advance
    modes 0..3 and a whole episode (RUN_TO_END), a day past nt - 1, a masked reset.  Before every call the trajectory rows and t1_log
    entries past each instance's time index are poisoned; after it, the days each participating instance simulated (t_in+1 ..
    t_out) are written and equal the clean run, every later entry keeps the poison, every earlier one is unchanged, and
    reward / flags / out of inactive and non-participating instances keep the poison."""
    from pdecontrolgym_amd import _native as N
    from tests.test_tumor import tumor_ic
    B = 5
    (clean, X), (pois, _) = _tumor(nx_big, B), _tumor(nx_big, B)
    arena = _arena(policy)
    guard_engine(pois, arena)
    ic = tumor_ic(X, clean.nx)
    for k in ("u", "remaining", "history", "t1_log"):
        PZ.poison_(pois.t[k])
    PZ.fill_int_(pois.t["stage"], 2)
    PZ.fill_int_(pois.t["time_index"], 3)
    PZ.fill_int_(pois.t["days"], 1)
    clean.reset(ic)                                    # init [nx]: init_stride = 0
    ic_t = arena.like("init", torch.as_tensor(ic, dtype=torch.float64, device="cuda"))
    pois.reset(ic_t)
    arena.check()
    for k in ("u", "remaining", "time_index", "stage", "days", "history"):
        PZ.assert_bits_equal(pois.t[k], clean.t[k], None, f"tumour reset: {k}")
    OUTS = ("reward", "terminated", "truncated", "out")
    TRAJ = ("history", "t1_log")
    rng = np.random.default_rng(5)
    active = np.array([1, 0, 1, 1, 0], dtype=np.uint8)
    nt = clean.nt

    def before_call():
        """Poison the pure outputs and every trajectory entry past t_in; return t_in and a snapshot of the trajectories."""
        for k in OUTS:
            PZ.poison_(pois.t[k])
        t_in = pois.t["time_index"].cpu().numpy().copy()
        for b in range(B):
            for k in TRAJ:
                if t_in[b] + 1 < nt:
                    PZ.poison_(pois.t[k][b, t_in[b] + 1:])
        return t_in, {k: pois.t[k].clone() for k in TRAJ}

    def check(tag, part, t_in, snap):
        arena.check()
        for k in OUTS:
            t = pois.t[k]
            sel = torch.tensor(part, device="cuda")
            PZ.assert_untouched(t, ~sel, f"{tag}: {k} of non-participating instances")
            PZ.assert_written(t, sel, f"{tag}: {k}", like=clean.t[k])
        for k in ("u", "time_index", "stage", "remaining", "days"):
            PZ.assert_bits_equal(pois.t[k], clean.t[k], None, f"{tag}: {k}")
        t_out = pois.t["time_index"].cpu().numpy()
        for b in range(B):
            assert (t_out[b] > t_in[b]) == bool(part[b]), f"{tag}: instance {b} days {t_in[b]} -> {t_out[b]}"
            for k in TRAJ:
                row = pois.t[k][b]
                PZ.assert_written(row, slice(t_in[b] + 1, t_out[b] + 1), f"{tag}: {k}[{b}] days {t_in[b] + 1}..{t_out[b]}",
                                  like=clean.t[k][b])
                PZ.assert_untouched(row, slice(t_out[b] + 1, None), f"{tag}: {k}[{b}] past day {t_out[b]}")
                PZ.assert_bits_equal(row, snap[k][b], slice(0, t_in[b] + 1), f"{tag}: {k}[{b}] up to day {t_in[b]}")

    for s in range(3):
        t_in, snap = before_call()
        c = rng.uniform(0, 1, B)
        clean.step(c, active=active)
        pois.step(arena.like(f"control{s}", torch.as_tensor(c, device="cuda")), active=arena.like("active", torch.as_tensor(active, device="cuda")))
        check(f"tumour step {s}", active.astype(bool), t_in, snap)
    for mode, days in ((N.TUMOR_RUN_GROWTH, 5), (N.TUMOR_RUN_POST, 5), (N.TUMOR_RUN_TO_END, 5), (N.TUMOR_RUN_ONE_DAY, 5),
                       (N.TUMOR_RUN_TO_END, nt)):
        t_in, snap = before_call()
        st = clean.t["stage"].cpu().numpy()
        live = (active == 1) & (t_in < nt - 1)
        part = live & {N.TUMOR_RUN_GROWTH: st == 0, N.TUMOR_RUN_POST: st == 2, N.TUMOR_RUN_TO_END: np.ones(B, bool),
                       N.TUMOR_RUN_ONE_DAY: np.ones(B, bool)}[mode]
        if mode == N.TUMOR_RUN_ONE_DAY:
            clean.t["control"].zero_()
            pois.t["control"].zero_()
        clean.advance(mode, days, active=active)
        pois.advance(mode, days, active=arena.like("active", torch.as_tensor(active, device="cuda")))
        check(f"tumour advance mode {mode} ({days} days)", part, t_in, snap)
    t_end, lethal = clean.t["time_index"].cpu().numpy(), clean.t["truncated"].cpu().numpy().astype(bool)
    assert ((t_end == nt - 1) | lethal)[part].all(), "RUN_TO_END with nt days runs every participating episode to its end"
    # a day for every instance, instance 0 (and the episodes RUN_TO_END finished) at time_index = nt - 1: those keep their state,
    # trajectory and out, and get reward and flags written as 0; the live ones (the inactive instances above) step as usual
    for e in (clean, pois):
        e.t["time_index"][0] = nt - 1
    t_in, snap = before_call()
    over = t_in >= nt - 1
    assert over[0] and not over.all()
    u_before = pois.t["u"].clone()
    pois.step(np.full(B, 0.5), active=np.ones(B, np.uint8))
    clean.step(np.full(B, 0.5), active=np.ones(B, np.uint8))
    arena.check()
    o = torch.tensor(over, device="cuda")
    PZ.assert_untouched(pois.t["out"], o, "tumour step past nt - 1: out")
    PZ.assert_written(pois.t["out"], ~o, "tumour step past nt - 1: out of live instances", like=clean.t["out"])
    PZ.assert_bits_equal(pois.t["u"][o], u_before[o], None, "tumour step past nt - 1: u")
    assert (pois.t["reward"][o] == 0).all() and (pois.t["terminated"][o] == 0).all() and (pois.t["truncated"][o] == 0).all()
    for k in ("reward", "terminated", "truncated"):
        PZ.assert_written(pois.t[k], None, f"tumour step past nt - 1: {k}", like=clean.t[k])
    t_out = pois.t["time_index"].cpu().numpy()
    assert (t_out[over] == nt - 1).all() and (t_out[~over] == t_in[~over] + 1).all()
    for b in range(B):
        for k in TRAJ:
            PZ.assert_bits_equal(pois.t[k][b], snap[k][b], slice(0, t_in[b] + 1), f"tumour step past nt - 1: {k}[{b}]")
            PZ.assert_written(pois.t[k][b], slice(t_in[b] + 1, t_out[b] + 1), f"tumour step past nt - 1: {k}[{b}]",
                              like=clean.t[k][b])
            PZ.assert_untouched(pois.t[k][b], slice(t_out[b] + 1, None), f"tumour step past nt - 1: {k}[{b}]")
    # masked reset: the others keep everything
    for k in ("u", "remaining"):
        PZ.poison_(pois.t[k])
    mask = arena.like("mask", torch.tensor([0, 0, 1, 0, 1], dtype=torch.uint8, device="cuda"))
    if policy is not None:
        assert mask.data_ptr() % 16 != 0 and ic_t.data_ptr() % 16 != 0
    before = {k: pois.t[k].clone() for k in ("time_index", "stage", "days")}
    pois.reset(ic_t, mask=mask)
    arena.check()
    on = mask.bool()
    PZ.assert_written(pois.t["u"], on, "tumour masked reset: u")
    PZ.assert_untouched(pois.t["u"], ~on, "tumour masked reset: u of others")
    PZ.assert_untouched(pois.t["remaining"], ~on, "tumour masked reset: remaining of others")
    for k, v in before.items():
        PZ.assert_bits_equal(pois.t[k][~on], v[~on], None, f"tumour masked reset: {k} of others")


# ---- MLP -----------------------------------------------------------------------------------------------------------------
MLP_CASES = [(w, B, in_dim, xf, yf) for (w, B, in_dim) in ((64, 1, 5), (128, 15, 37), (256, 17, 600), (64, 4095, 51), (256, 5, 13))
             for xf in (False, True) for yf in (False, True)]


@pytest.mark.parametrize("width,B,in_dim,x_f64,y_f64", MLP_CASES)
def test_mlp_forward_contract_vs_float64(width, B, in_dim, x_f64, y_f64, policy=None):
    """pdegym_mlp_forward at the 64/128/256 launchers, every x/y dtype pair, ragged B and in_dim (one above the 512-entry staging
    chunk), x/y/noise strides wider than the rows with NaN in the gaps; the y gap keeps its poison.  Against a float64 evaluation of
    the same float32 network: |y - y64| <= 4 * 2^-24 * (in_dim + 2 * width + 2) * (|W| |h| + |b|) summed magnitudes + 1e-6, the
    standard bound for float32 dot products of that length (tanh layers keep the magnitudes <= 1)."""
    from pdecontrolgym_amd.policy import FusedMLP
    torch.manual_seed(width + B + in_dim)
    out_dim = 3
    mod = torch.nn.Sequential(torch.nn.Linear(in_dim, width), torch.nn.Tanh(), torch.nn.Linear(width, width), torch.nn.Tanh(),
                              torch.nn.Linear(width, out_dim)).cuda()
    pol = FusedMLP(mod, clamp=None)
    xdt, ydt = (torch.float64 if x_f64 else torch.float32), (torch.float64 if y_f64 else torch.float32)
    arena = _arena(policy)
    xs, ys, ns = in_dim + 3, out_dim + 5, out_dim + 2
    xbuf = arena.new("x", (B, xs), xdt)
    PZ.poison_(xbuf)
    x = xbuf[:, :in_dim]
    x.copy_(torch.randn(B, in_dim, dtype=xdt))
    ybuf = PZ.poison_(arena.new("y", (B, ys), ydt))
    y = ybuf[:, :out_dim]
    nbuf = PZ.poison_(arena.new("noise", (B, ns), torch.float32))
    nz = nbuf[:, :out_dim]
    nz.copy_(torch.randn(B, out_dim) * 0.1)
    net = pol._net(None, x_f64, y_f64)
    net.noise, net.noise_stride = nz.data_ptr(), ns
    pol.refresh()
    pol.backend.mlp_forward(net, x, y, B)
    arena.check()
    PZ.assert_written(ybuf, (slice(None), slice(0, out_dim)), "mlp y")
    PZ.assert_untouched(ybuf, (slice(None), slice(out_dim, None)), "mlp y_stride gap")
    # float64 evaluation of the same float32 parameters (x rounded to float32 as the kernel reads it)
    h = x.double().float().double().cpu()
    mag = h.abs()
    lins = [m for m in mod if isinstance(m, torch.nn.Linear)]
    for i, L in enumerate(lins):
        W, b = L.weight.detach().double().cpu(), L.bias.detach().double().cpu()
        mag = mag @ W.abs().T + b.abs()
        h = h @ W.T + b
        if i < len(lins) - 1:
            h = torch.tanh(h)
            mag = torch.ones_like(mag)
    h = h + nz.double().cpu()
    tol = 4 * 2.0 ** -24 * (in_dim + 2 * width + 2) * (mag + 1) + 1e-6
    err = (y.double().cpu() - h).abs()
    assert bool((err <= tol).all()), f"mlp vs float64: max err {float(err.max()):.3g}, tol {float(tol.min()):.3g}"
