"""GPU tests of the per-step terminal observations of the one-launch rollouts (PDEGYM_ROLLOUT_FINAL_OBS_PER_STEP), of the masked
forward launch (pdegym_mlp_forward_masked) and of the truncation bootstrap built on the two.

Inputs (tests/terminal_obs_cases.py): episodes end inside the window of T = 7 steps for both reasons -- the horizon is 3 env-steps, and
``max_state_value`` sits between the row norms of two groups of pool rows -- and every test asserts from the flags that at least one
step terminated and one was cut off before it compares anything.  The terminal rows and the masked outputs live in guarded, poisoned
buffers (tests/poison.py): "no other row is touched" is the poison still standing."""
import numpy as np
import pytest

from tests import gae_restatement as R
from tests import poison
from tests import terminal_obs_cases as K

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
T = K.T_STEPS
STATE_1D = ("time_index", "bsum", "ring", "reset_count", "beta")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize])


def _net(sizes, act="tanh", seed=1, scale=0.2):
    g = torch.Generator().manual_seed(seed)
    mods = []
    for i in range(len(sizes) - 1):
        lin = torch.nn.Linear(sizes[i], sizes[i + 1])
        with torch.no_grad():
            lin.weight.copy_(torch.randn(lin.weight.shape, generator=g) * scale / np.sqrt(sizes[i]))
            lin.bias.copy_(torch.randn(lin.bias.shape, generator=g) * 0.1)
        mods.append(lin)
        if i < len(sizes) - 2:
            mods.append(torch.nn.Tanh() if act == "tanh" else torch.nn.ReLU())
    return torch.nn.Sequential(*mods).cuda()


def _counts(terminated, truncated):
    te, tr = terminated.bool(), truncated.bool()
    return int(te.sum()), int((tr & ~te).sum())


def _poisoned_rows(ro, arena):
    """The rollout's terminal rows in a guarded allocation, poisoned."""
    ro.terminal_obs = poison.poison_(arena.new("terminal_obs", ro.terminal_obs.shape, ro.terminal_obs.dtype))
    return ro.terminal_obs


# ---- one-launch 1D ----------------------------------------------------------------------------------------------------------------------
# id -> (kind, nx, environment overrides, policy: None (commands given ahead) | layer sizes after the input | "law")
# (the environments: tests/terminal_obs_cases.py GPU_ENVS_1D, stepped on the oracle by tests/test_terminal_obs.py with the commands of
# the open-loop cases; an actor or the law issues its own commands, and the assertion on the flags below covers those)
_E = K.GPU_ENVS_1D
CASES_1D = {
    "open_parabolic_n65_full": _E["parabolic_n65_full"] + (None,),
    "open_parabolic_n40": _E["parabolic_n40"] + (None,),
    "open_parabolic_n257": _E["parabolic_n257"] + (None,),
    "open_transport_n64": _E["transport_n64"] + (None,),
    "open_neumann": _E["neumann"] + (None,),
    "open_scalar_sensing": _E["scalar_sensing"] + (None,),
    "actor_64_64": _E["parabolic_n40"] + ((64, 64, 1),),
    "actor_65_wide": _E["parabolic_n40"] + ((65, 1),),
    "actor_64_64_neumann": _E["neumann"] + ((64, 64, 1),),
    "backstepping_n33": _E["parabolic_n33"] + ("law",),
}
B_1D = K.B_GPU


def _run_1d(case, flag, arena=None, commands=None):
    """One one-launch rollout of the case; ``flag``: with the per-step terminal rows.  Returns (venv, rollout)."""
    from pde_control_gym import BacksteppingController, DeviceRollout, FusedMLP
    kind, nx, over, pol = CASES_1D[case]
    venv = K.make_1d(kind, nx, B_1D, device="cuda", beta_pool=False if pol == "law" else None, **over)
    policy = None
    if pol == "law":
        theta = (50.0 * np.cos(7.0 * np.arccos(np.linspace(1.0 / nx, 1, nx)))).astype(np.float32)
        policy = BacksteppingController(kind, theta, 1.0 / nx, order="ordered", device="cuda").attach(venv)
    elif pol is not None:
        policy = FusedMLP(_net((venv.core.obs_dim,) + pol, seed=3))
    ro = DeviceRollout(venv, policy, T, use_graph=False, one_launch=policy is not None, terminal_obs=flag)
    if flag and arena is not None:
        _poisoned_rows(ro, arena)
    if policy is None:
        ro.actions.copy_(torch.from_numpy(K.commands(T, B_1D)).cuda() if commands is None else commands)
        ro.obs[0].copy_(venv.rollout_obs())
        venv.rollout_one_launch(ro.obs, ro.actions, ro.rewards, ro.terminated, ro.truncated,
                                **({"final_obs_steps": ro.terminal_obs} if flag else {}))
    else:
        assert ro.one_launch is True
        ro.run()
    torch.cuda.synchronize()
    return venv, ro


@pytest.mark.parametrize("case", sorted(CASES_1D))
def test_one_launch_1d_rows_equal_the_step_loop(case):
    arena = poison.Arena("cuda")
    venv, ro = _run_1d(case, True, arena)
    arena.check()
    n_term, n_trunc = _counts(ro.terminated, ro.truncated)
    print(f"{case}: {n_term} terminated, {n_trunc} cut off")
    assert n_term >= 1 and n_trunc >= 1, (n_term, n_trunc)
    # the twin: T separate step calls on the commands the launch issued (or was given), final_obs[b] collected after each
    kind, nx, over, pol = CASES_1D[case]
    twin = K.make_1d(kind, nx, B_1D, device="cuda", beta_pool=False if pol == "law" else None, **over)
    ended = (ro.terminated | ro.truncated).bool()
    for t in range(T):
        obs, _, te, tr = twin.step_tensor(ro.actions[t])
        done = (te | tr).bool()
        assert torch.equal(done, ended[t]), f"step {t}: the twin ended other episodes"
        poison.assert_bits_equal(obs, ro.obs[t + 1], None, f"obs slot {t + 1}")
        if bool(done.any()):
            poison.assert_written(ro.terminal_obs[t], done, f"terminal rows of step {t}", like=twin.core.t["final_obs"])
    poison.assert_untouched(ro.terminal_obs, ~ended, "terminal rows of steps that ended nothing")
    assert not bool(venv.core.t["final_obs"].any()), "the engine's own final_obs is not written in this mode"
    # the run without the flag: every other output and the state left behind keep their bits
    plain_env, plain = _run_1d(case, False, commands=ro.actions if pol is None else None)
    for name in ("obs", "actions", "rewards", "terminated", "truncated"):
        poison.assert_bits_equal(getattr(ro, name), getattr(plain, name), None, name)
    for key in STATE_1D + ("obs",) + (("u",) if venv.core.obs_dim == 1 else ()):
        poison.assert_bits_equal(venv.core.t[key], plain_env.core.t[key], None, "state " + key)


# ---- other families ---------------------------------------------------------------------------------------------------------------------
def _traffic_run(sim, law, flag, arena=None, use_graph=False, one_launch=True, policy=None):
    from pde_control_gym import DeviceRollout, TrafficBacksteppingController
    venv = K.make_traffic(sim, device="cuda")
    A = venv.core.action_dim
    pol = TrafficBacksteppingController(venv, order="numpy").attach(venv) if law else policy
    ro = DeviceRollout(venv, pol, T, use_graph=use_graph, action_low=0.96, action_high=1.44, one_launch=one_launch if pol is not None else False,
                       terminal_obs=flag)
    if flag and arena is not None:
        _poisoned_rows(ro, arena)
    if pol is None:
        ro.actions.copy_(torch.from_numpy(K.traffic_commands(T, 5, A)).cuda().reshape(ro.actions.shape))
        ro.obs[0].copy_(venv.rollout_obs())
        venv.rollout_one_launch(ro.obs, ro.actions, ro.rewards, ro.terminated, ro.truncated,
                                **({"final_obs_steps": ro.terminal_obs} if flag else {}))
    else:
        ro.run()
    torch.cuda.synchronize()
    return venv, ro


@pytest.mark.parametrize("sim,law", [("outlet", False), ("both", False), ("outlet", True)], ids=["outlet", "both_two_commands", "backstepping"])
def test_one_launch_traffic_rows_equal_the_step_loop(sim, law):
    arena = poison.Arena("cuda")
    venv, ro = _traffic_run(sim, law, True, arena)
    arena.check()
    n_term, n_trunc = _counts(ro.terminated, ro.truncated)
    print(f"traffic {sim} law={law}: {n_term} terminated, {n_trunc} cut off")
    assert n_term >= 1 and n_trunc >= 1, (n_term, n_trunc)
    twin = K.make_traffic(sim, device="cuda")
    ended = (ro.terminated | ro.truncated).bool()
    for t in range(T):
        obs, _, te, tr = twin.step_tensor(ro.actions[t])
        done = (te | tr).bool()
        assert torch.equal(done, ended[t]), f"step {t}: the twin ended other episodes"
        poison.assert_bits_equal(obs, ro.obs[t + 1], None, f"obs slot {t + 1}")
        if bool(done.any()):
            poison.assert_written(ro.terminal_obs[t], done, f"terminal rows of step {t}", like=twin.core.t["final_obs"])
    poison.assert_untouched(ro.terminal_obs, ~ended, "terminal rows of steps that ended nothing")
    assert not bool(venv.core.t["final_obs"].any()), "the engine's own final_obs is not written in this mode"
    plain_env, plain = _traffic_run(sim, law, False)
    for name in ("obs", "actions", "rewards", "terminated", "truncated"):
        poison.assert_bits_equal(getattr(ro, name), getattr(plain, name), None, name)
    for key in ("r", "y", "time", "rs", "reset_count"):
        poison.assert_bits_equal(venv.core.t[key], plain_env.core.t[key], None, "state " + key)


class _Replay:
    """A policy that issues row t of commands given ahead at its t-th call (of every T: warm-up, capture and eager runs alike)."""

    def __init__(self, acts):
        self.acts, self.t = acts, 0

    def __call__(self, obs):
        a = self.acts[self.t % self.acts.shape[0]]
        self.t += 1
        return a


def _tumor_run(with_policy, flag, arena=None, use_graph=False, one_launch=True, width=32):
    """``with_policy``: False (commands given ahead), True (a FusedMLP), or "replay" (the commands given ahead, issued by a callable:
    what the launch-per-step path takes in the place of ``policy=None``)."""
    from pde_control_gym import DeviceRollout, FusedMLP
    venv = K.make_tumor(fused=True, device="cuda")
    policy = None
    if with_policy == "replay":
        policy = _Replay(torch.from_numpy(K.tumor_commands(T, 5)).cuda())
    elif with_policy:      # doses around 0.8 of the total: the dosage is used up within two steps and the post-therapy run ends the episode
        net = _net((21, width, 1), seed=5, scale=1e-5)
        with torch.no_grad():
            net[-1].bias.fill_(0.8)
        policy = FusedMLP(net)
    ro = DeviceRollout(venv, policy, T, use_graph=use_graph, action_low=0.0, action_high=1.0, one_launch=one_launch, terminal_obs=flag)
    if flag and arena is not None:
        _poisoned_rows(ro, arena)
    if not with_policy:
        ro.actions.copy_(torch.from_numpy(K.tumor_commands(T, 5)).cuda())
    ro.run()
    torch.cuda.synchronize()
    return venv, ro


@pytest.mark.parametrize("with_policy", [False, True], ids=["commands_ahead", "policy"])
def test_one_launch_tumor_rows_equal_the_step_loop(with_policy):
    arena = poison.Arena("cuda")
    venv, ro = _tumor_run(with_policy, True, arena)
    arena.check()
    ended = (ro.terminated | ro.truncated).bool()
    n_term, n_trunc = _counts(ro.terminated, ro.truncated)
    print(f"tumour policy={with_policy}: {n_term} terminated, {n_trunc} cut off")
    if with_policy:      # identical patients on identical doses end the same way (tests/terminal_obs_cases.py: make_tumor)
        assert bool(ended.any()), "no episode ended inside the window"
    else:
        assert n_term >= 1 and n_trunc >= 1, (n_term, n_trunc)
    twin = K.make_tumor(fused=True, device="cuda")
    for t in range(T):
        obs, _, te, tr = twin.step_tensor(ro.actions[t])
        done = te | tr
        assert torch.equal(done, ended[t]), f"step {t}: the twin ended other episodes"
        poison.assert_bits_equal(obs, ro.obs[t + 1], None, f"obs slot {t + 1}")
        if bool(done.any()):
            poison.assert_written(ro.terminal_obs[t], done, f"terminal rows of step {t}", like=twin.terminal_obs)
    poison.assert_untouched(ro.terminal_obs, ~ended, "terminal rows of steps that ended nothing")
    plain_env, plain = _tumor_run(with_policy, False)
    for name in ("obs", "actions", "rewards", "terminated", "truncated"):
        poison.assert_bits_equal(getattr(ro, name), getattr(plain, name), None, name)
    for key in ("u", "time_index", "stage", "remaining", "days", "out"):
        poison.assert_bits_equal(venv.core.t[key], plain_env.core.t[key], None, "state " + key)


# ---- launch-per-step paths ---------------------------------------------------------------------------------------------------------------
def _family_runs(family, one_launch, use_graph):
    """The same rollout through one launch / a launch per step (eager or hipGraph).  1D and traffic: a policy with a 65-unit layer --
    the in-kernel evaluation has forward_into's bits, so the three paths issue the same commands."""
    from pde_control_gym import DeviceRollout, FusedMLP
    if family == "1d":
        venv = K.make_1d("parabolic", 39, B_1D, device="cuda")
        ro = DeviceRollout(venv, FusedMLP(_net((40, 65, 1), seed=3)), T, use_graph=use_graph, one_launch=one_launch, terminal_obs=True)
        ro.run()
    elif family == "traffic":
        venv = K.make_traffic("outlet", device="cuda")
        pol = FusedMLP(_net((24, 65, 1), seed=4))
        ro = DeviceRollout(venv, pol, T, use_graph=use_graph, action_low=0.96, action_high=1.44, one_launch=one_launch, terminal_obs=True)
        ro.run()
    else:      # commands given ahead: read from ``actions`` by the one launch, issued by a callable on the launch-per-step path
        _, ro = _tumor_run(False if one_launch else "replay", True, None, use_graph=use_graph, one_launch=one_launch)
    torch.cuda.synchronize()
    assert ro.one_launch is one_launch
    return ro


@pytest.mark.parametrize("family", ["1d", "traffic", "tumor"])
def test_launch_per_step_paths_fill_the_same_rows(family):
    one = _family_runs(family, True, False)
    ended = (one.terminated | one.truncated).bool()
    n_term, n_trunc = _counts(one.terminated, one.truncated)
    assert n_term >= 1 and n_trunc >= 1, (n_term, n_trunc)
    assert bool(one.terminal_obs[ended].any()) and not bool(one.terminal_obs[~ended].any())
    for use_graph in (False, True):
        loop = _family_runs(family, False, use_graph)
        what = "hipGraph" if use_graph else "eager"
        for name in ("obs", "actions", "terminated", "truncated"):
            poison.assert_bits_equal(getattr(loop, name), getattr(one, name), None, f"{what} {name}")
        poison.assert_bits_equal(loop.terminal_obs, one.terminal_obs, None, f"{what} terminal_obs")


# ---- masked forward ---------------------------------------------------------------------------------------------------------------------
B_MLP = 37
NETS = {"9-64-64-1_tanh": ((9, 64, 64, 1), "tanh"), "9-65-1_relu": ((9, 65, 1), "relu")}


def _masks():
    g = torch.Generator().manual_seed(7)
    rows = (torch.rand(B_MLP, generator=g) < 0.4).to(torch.uint8)
    rows[5], rows[20], rows[36] = 1, 1, 0
    rows[16:32] = 0                      # a whole tile of dead rows
    rows[20] = 1
    rows_not = (torch.rand(B_MLP, generator=g) < 0.3).to(torch.uint8)
    rows_not[5], rows_not[20] = 0, 1     # row 5 stays live, row 20 is knocked out: tile 1 is all dead
    last = torch.zeros(B_MLP, dtype=torch.uint8)
    last[36] = 1
    return {"mixed": (rows, None), "rows_not": (rows, rows_not), "all_dead": (torch.zeros(B_MLP, dtype=torch.uint8), None),
            "only_the_last_row": (last, None), "all_live": (torch.ones(B_MLP, dtype=torch.uint8), None)}


@pytest.mark.parametrize("f64", [False, True], ids=["f32_rows", "f64_rows"])
@pytest.mark.parametrize("net", sorted(NETS))
def test_masked_forward(net, f64):
    from pde_control_gym import FusedMLP
    from tests import lds_residue as LR
    sizes, act = NETS[net]
    mlp = FusedMLP(_net(sizes, act, seed=9, scale=1.0))
    x = torch.randn(B_MLP, 9, generator=torch.Generator().manual_seed(2), dtype=torch.float64 if f64 else torch.float32).cuda()
    ref = torch.zeros(B_MLP, device="cuda")
    mlp.forward_into(x, ref, clamp=None)
    for name, (rows, rows_not) in _masks().items():
        rows = rows.cuda()
        rows_not = None if rows_not is None else rows_not.cuda()
        live = rows.bool() if rows_not is None else rows.bool() & ~rows_not.bool()
        if name == "rows_not":
            assert bool((rows.bool() & ~live).any()), "rows_not knocks no row out"
        assert int(live.sum()) == {"all_dead": 0, "only_the_last_row": 1, "all_live": B_MLP}.get(name, int(live.sum()))
        xn = x.clone()
        xn[~live] = float("nan")           # dead input rows may hold anything
        for label, inp, dirty in (("clean", x, None), ("nan_in_dead_rows", xn, None), ("lds_residue", xn, "nan")):
            arena = poison.Arena("cuda")
            y = poison.poison_(arena.new("y", (B_MLP,), torch.float32))
            xin = arena.like("x", inp)
            r_, rn_ = arena.like("rows", rows), None if rows_not is None else arena.like("rows_not", rows_not)
            if dirty is None:
                mlp.forward_into(xin, y, clamp=None, rows=r_, rows_not=rn_)
            else:
                with LR.dirtied(dirty) as d:
                    mlp.forward_into(xin, y, clamp=None, rows=r_, rows_not=rn_)
                    torch.cuda.synchronize()
                d.check("pdegym_mlp_forward_masked", exact=True)
            arena.check()
            if bool(live.any()):
                poison.assert_written(y, live, f"{name} / {label}: live rows", like=ref)
            poison.assert_untouched(y, ~live, f"{name} / {label}: dead rows")
    # the clamp is the unmasked launch's as well
    rows = _masks()["mixed"][0].cuda()
    y, yc = torch.zeros(B_MLP, device="cuda"), torch.zeros(B_MLP, device="cuda")
    mlp.forward_into(x, yc, clamp=(-0.05, 0.05))
    mlp.forward_into(x, y, clamp=(-0.05, 0.05), rows=rows)
    poison.assert_bits_equal(y[rows.bool()], yc[rows.bool()], None, "clamped live rows")


# ---- the buffer -------------------------------------------------------------------------------------------------------------------------
def _buffer_setup(B=B_1D):
    from pde_control_gym import DeviceRollout, DeviceRolloutBuffer, FusedMLP
    venv = K.make_1d("parabolic", 39, B, device="cuda")
    actor, critic = FusedMLP(_net((40, 32, 1), seed=3)), FusedMLP(_net((40, 32, 1), seed=6))
    ro = DeviceRollout(venv, actor, T, use_graph=False, action_noise=True, one_launch=True, terminal_obs=True)
    buf = DeviceRolloutBuffer(ro, gamma=0.99, gae_lambda=0.95)
    return venv, critic, ro, buf


def test_buffer_bootstraps_truncated_steps_with_one_masked_launch():
    venv, critic, ro, buf = _buffer_setup()
    arena = poison.Arena("cuda")
    buf.boot = poison.poison_(arena.new("boot", (T, B_1D), torch.float32))
    ro.action_noise.copy_(torch.randn(T, B_1D, generator=torch.Generator().manual_seed(4)).mul_(0.3).cuda())
    ro.run()
    buf.compute(critic=critic)
    arena.check()
    n_term, n_trunc = _counts(ro.terminated, ro.truncated)
    assert n_term >= 1 and n_trunc >= 1, (n_term, n_trunc)
    live = ro.truncated.bool() & ~ro.terminated.bool()
    full = torch.zeros(T * B_1D, device="cuda")
    critic.forward_into(ro.terminal_obs.reshape(T * B_1D, -1), full, clamp=None)
    full = full.reshape(T, B_1D)
    poison.assert_written(buf.boot, live, "boot of truncated steps", like=full)
    poison.assert_untouched(buf.boot, ~live, "boot of the other steps")
    # advantages and returns: pdegym_gae fed that boot by hand, and the restatement
    adv, ret = torch.zeros_like(buf.advantages), torch.zeros_like(buf.returns)
    buf.backend.gae(ro.rewards, buf.values, ro.terminated, ro.truncated, adv, ret, 0.99, 0.95, boot=full.contiguous())
    poison.assert_bits_equal(buf.advantages, adv, None, "advantages")
    poison.assert_bits_equal(buf.returns, ret, None, "returns")
    a_ref, r_ref = R.gae_reference(ro.rewards.cpu().numpy(), buf.values.cpu().numpy(), ro.terminated.cpu().numpy(), ro.truncated.cpu().numpy(),
                                   0.99, 0.95, full.cpu().numpy())
    assert np.array_equal(_bits(buf.advantages.cpu().numpy()), _bits(a_ref)) and np.array_equal(_bits(buf.returns.cpu().numpy()), _bits(r_ref))
    from pde_control_gym import DeviceRolloutBuffer
    off = DeviceRolloutBuffer(ro, gamma=0.99, gae_lambda=0.95, bootstrap_truncated=False).compute(critic=critic)
    assert off.boot is None and not torch.equal(off.advantages, buf.advantages)


def test_rollout_and_bootstrapped_gae_in_one_graph_equal_the_eager_calls():
    noise = torch.randn(3, T, B_1D, generator=torch.Generator().manual_seed(4)).mul_(0.3).cuda()
    runs = {}
    for mode in ("eager", "graph"):
        venv, critic, ro, buf = _buffer_setup()

        def both():
            ro.run()
            buf.compute(critic=critic)
        ro.action_noise.copy_(noise[0])
        both()                                       # (also the warm-up of the captured calls)
        if mode == "graph":
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                both()
        snaps = []
        for i in (1, 2):
            ro.action_noise.copy_(noise[i])
            if mode == "graph":
                graph.replay()
            else:
                both()
            torch.cuda.synchronize()
            live = ro.truncated.bool() & ~ro.terminated.bool()
            snaps.append({"terminal_obs": ro.terminal_obs.clone(), "boot_live": torch.where(live, buf.boot, torch.zeros_like(buf.boot)),
                          "advantages": buf.advantages.clone(), "returns": buf.returns.clone(), "values": buf.values.clone(),
                          "terminated": ro.terminated.clone(), "truncated": ro.truncated.clone(), "actions": ro.actions.clone()})
        runs[mode] = snaps
    for i, (a, b) in enumerate(zip(runs["eager"], runs["graph"])):
        for k in a:
            poison.assert_bits_equal(b[k], a[k], None, f"replay {i}: {k}")
    for s in runs["eager"]:
        n_term, n_trunc = _counts(s["terminated"], s["truncated"])
        assert n_term >= 1 and n_trunc >= 1, (n_term, n_trunc)


# ---- the examples -----------------------------------------------------------------------------------------------------------------------
def _example(name):
    import importlib.util
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if os.path.join(root, "examples") not in sys.path:      # (train_sac_device imports make_env from its neighbour)
        sys.path.insert(0, os.path.join(root, "examples"))
    spec = importlib.util.spec_from_file_location(name, os.path.join(root, "examples", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_the_ppo_example_runs_with_the_bootstrap():
    hist = _example("train_ppo_device").main(2, B=64, T=16, quiet=True, bootstrap=True)
    assert len(hist) == 2 and all(np.isfinite(v) for h in hist for v in h.values() if isinstance(v, float))


def test_the_sac_example_runs_with_terminal_observations():
    hist = _example("train_sac_device").main(2, num_envs=64, n_steps=16, quiet=True, updates=2, batch=256, terminal_obs=True)
    for k in ("q_loss", "actor_loss", "alpha", "mean_reward", "mean_norm"):
        assert len(hist[k]) == 2 and all(np.isfinite(v) for v in hist[k]), k
