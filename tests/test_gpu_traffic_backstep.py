"""GPU tests of the TrafficPDE1D backstepping baseline (csrc/pdegym_traffic_backstep.hip): the control kernel against the NumPy
restatement (tests/traffic_backstep_restatement.py) -- bit for bit in the "numpy" order, within the derived bound in the "tree" order --
at every row length at which it takes another path; the reference's own closed loop (tests/golden/traffic_backstep.npz); the law
inside the one-launch rollout against control launch + step launch per env-step, BIT FOR BIT, in both orders, eagerly and from a
replayed graph, with restarts inside the launch; poisoned buffers with guard bands; non-finite rows; and whatever the batch an
instance sits in."""
import functools
import os
import random

import numpy as np
import pytest

from tests import nonfinite, poison
from tests import traffic_backstep_restatement as R

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = dict(T=240, dt=0.25, X=500, dx=10, v_steady=10, ro_steady=0.12, v_max=40, ro_max=0.16, tau=60)
VM, RM, TAU, DX = 40, 0.16, 60, 10
KEYS = ("obs", "actions", "rewards", "terminated", "truncated")
STATE = ("r", "y", "time", "rs", "obs", "reward", "done", "truncated", "reset_count", "final_obs")
RS3 = (0.115, 0.12, 0.125)
# n < 8 (the smallest freeway the engine takes); exactly one block of eight; a tail; the reference's grid; the register limit; the
# first strided row; the last un-recursed block -- and, tree only, longer rows
M_NUMPY = (4, 9, 12, 51, 64, 65, 129)
M_TREE = M_NUMPY + (200, 1024)
# every kernel launched in csrc/pdegym_traffic_backstep.hip -> the poisoned-buffer / guard-band tests that reach it
# (tests/test_traffic_backstep.py fails when a launched kernel is missing here)
KERNEL_CASES = {"traffic_backstep_control_kernel": ["test_control_writes_exactly_its_outputs"],
                "traffic_backstep_rollout_kernel": ["test_rollout_writes_exactly_its_outputs"]}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _same(got, want, what):
    for k in want:
        if want[k] is None:
            assert got[k] is None, (what, k)
        else:
            np.testing.assert_array_equal(_bits(got[k]), _bits(want[k]), err_msg=f"{what}: {k}")


def _core(sim, M, B, rs, cf=1, T=240):
    """A TrafficBatch of B freeways of M nodes with the steady-state densities ``rs`` [B], reset."""
    from pdecontrolgym_amd.batch_traffic import TrafficBatch
    core = TrafficBatch(T, 0.25, (M - 1) * DX, DX, sim, VM, RM, TAU, True, cf, num_envs=B, device="cuda")
    rs = np.asarray(rs, dtype=np.float64)
    core.set_action_bounds(rs * core.Veq(rs))
    core.reset(rs)
    return core


# ---- the control kernel against the restatement -----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _control_case(M, B, sim="outlet"):
    """Random finite rows around the steady state and what the restatement makes of them, computed once: per-instance densities for
    B = 5 (one weight row per instance), one shared density otherwise."""
    rng = np.random.default_rng(1000 * M + B)
    rs = np.array([RS3[b % 3] for b in range(B)]) if B == 5 else np.full(B, 0.12)
    x = np.arange(0, (M - 1) * DX + DX, DX)
    obs = np.zeros((B, 2 * M))
    want, bound = np.zeros((B, 2 if sim == "both" else 1)), np.zeros(B)
    for b in range(B):
        vs, qs, _ = R.steady(VM, RM, rs[b])
        cv, cq = R.weights(x, VM, RM, TAU, rs[b])
        obs[b, :M], obs[b, M:] = rs[b] * rng.uniform(0.7, 1.3, M), vs * rng.uniform(0.7, 1.3, M)
        want[b] = R.law_commands(sim, obs[b, :M], obs[b, M:], cv, cq, DX, rs[b], vs, qs)
        bound[b] = R.tree_bound(obs[b, :M], obs[b, M:], cv, cq, DX, rs[b], vs, qs)
    return rs, obs, want, bound


@pytest.mark.parametrize("M", M_TREE)
@pytest.mark.parametrize("order", ["numpy", "tree"])
def test_control_kernel_against_the_restatement(M, order):
    """First check of this file: ``TrafficBacksteppingController`` used not to exist.  "numpy": bit-identical; "tree": within
    2 * 2**-53 * ((n + 2)(|rs| sum|tv_i| + sum|tq_i|) + |rs Iv| + |qs + rs Iv| + |q_out|) of it (the controller's docstring)."""
    from pde_control_gym import TrafficBacksteppingController
    if order == "numpy" and M not in M_NUMPY:
        with pytest.raises(ValueError, match="order='numpy' covers freeways of up to 129 nodes"):
            TrafficBacksteppingController(_core("outlet", M, 1, [0.12]), order="numpy")
        return
    for B in (1, 5, 67):
        rs, obs, want, bound = _control_case(M, B)
        ctrl = TrafficBacksteppingController(_core("outlet", M, B, rs), order=order)
        assert ctrl.weights_v.dim() == (2 if B == 5 else 1)
        got = ctrl(torch.as_tensor(obs, device="cuda")).cpu().numpy()
        err = np.abs(got - want[:, 0])
        print(f"M={M} B={B} {order}: max |device - numpy order| = {err.max():.3e}, smallest bound {bound.min():.3e}")
        if order == "numpy":
            np.testing.assert_array_equal(_bits(got), _bits(want[:, 0]), err_msg=f"M={M} B={B}")
        else:
            assert np.all(err <= bound), (M, B, err.max(), bound.min())


@pytest.mark.parametrize("sim", ["inlet", "both", "outlet"])
def test_control_kernel_commands_noise_and_clamp(sim):
    """The commands of every simulation type ('inlet': qs, no integral), + float32 noise widened, clamped with np.clip's rule."""
    from pde_control_gym import TrafficBacksteppingController
    M, B = 51, 5
    rs, obs, want, _ = _control_case(M, B, sim)
    ctrl = TrafficBacksteppingController(_core(sim, M, B, rs), order="numpy")
    shape = (B, 2) if sim == "both" else (B,)
    got = ctrl(torch.as_tensor(obs, device="cuda")).cpu().numpy()
    assert got.shape == shape
    np.testing.assert_array_equal(_bits(got), _bits(want.reshape(shape)))
    noise = np.random.default_rng(3).normal(0, 1e-3, shape).astype(np.float32)
    # three densities, so at least three well separated command levels (about 1.09, 1.2, 1.29): the window cuts between them and the
    # noise is far smaller than the gaps -- the lowest level lands on lo, the highest on hi, the middle one inside
    levels = np.unique(want)
    lo, hi = float((levels[0] + 1.2) / 2), float((levels[-1] + 1.2) / 2)
    out = torch.zeros(shape, dtype=torch.float64, device="cuda")
    ctrl.forward_into(torch.as_tensor(obs, device="cuda"), out, clamp=(lo, hi), noise=torch.as_tensor(noise, device="cuda"))
    ref = np.clip(want.reshape(shape) + noise.astype(np.float64), lo, hi)
    np.testing.assert_array_equal(_bits(out.cpu().numpy()), _bits(ref))
    assert (ref == lo).any() and (ref == hi).any() and ((ref > lo) & (ref < hi)).any()


# ---- the reference's closed loop ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "traffic_backstep.npz"), allow_pickle=False)


def _venv(sim, B, cf=1, X=500, T=240, rs=None, pool=None):
    import pde_control_gym
    from pde_control_gym.src import TrafficARZReward
    random.seed(0)
    venv = pde_control_gym.make_vec("PDEControlGym-TrafficPDE1D", num_envs=B, reward_class=TrafficARZReward(), simulation_type=sim,
                                    limit_pde_state_size=True, control_freq=cf, **dict(BASE, X=X, T=T))
    venv.reset_tensor()
    if rs is not None:
        rs = np.asarray(rs, dtype=np.float64)
        venv.core.set_action_bounds(rs * venv.core.Veq(rs))
        venv.core.reset(rs)
    if pool is not None:
        venv.enable_fused_auto_reset(init_pool=pool)
    return venv


@pytest.mark.parametrize("one_launch", [False, True])
@pytest.mark.parametrize("case", [f"{sim}_cf{cf}" for sim in ("outlet", "both", "inlet") for cf in (1, 2)] + ["outlet_m12"])
def test_closed_loop_reproduces_the_reference(case, one_launch):
    """The whole episode of the reference (3 840 env-steps), "numpy" order, three freeways: control launch + pdegym_traffic_step per
    env-step, and the one-launch kernel.  Commands and the stored observations bit for bit, rewards to rtol 1e-13, flags equal."""
    from pde_control_gym import DeviceRollout, TrafficBacksteppingController
    g = R.golden_case(_golden(), case)
    sim, B, steps = case.split("_")[0], 3, int(g["steps"])
    venv = _venv(sim, B, cf=int(g["params"][9]), X=int(g["params"][2]))
    ctrl = TrafficBacksteppingController(venv, order="numpy")
    ro = DeviceRollout(venv, ctrl, steps, use_graph=False, action_low=0.96, action_high=1.44, one_launch=one_launch).run()
    assert ro.one_launch is one_launch
    acts, obs, rew = ro.actions.cpu().numpy().reshape(steps, B, -1), ro.obs.cpu().numpy(), ro.rewards.cpu().numpy()
    for b in range(B):
        np.testing.assert_array_equal(_bits(acts[:, b]), _bits(g["commands"]), err_msg=f"commands of instance {b}")
        np.testing.assert_array_equal(_bits(obs[g["obs_steps"], b]), _bits(g["obs"]), err_msg=f"observations of instance {b}")
        np.testing.assert_allclose(rew[:, b], g["rewards"], rtol=1e-13, atol=0)
        total = 0
        for r_ in rew[:, b]:
            total += r_
        np.testing.assert_allclose(total, float(g["reward_sum"]), rtol=1e-13)
    np.testing.assert_array_equal(ro.terminated.cpu().numpy(), np.repeat(g["done"][:, None], B, axis=1))
    np.testing.assert_array_equal(ro.truncated.cpu().numpy(), np.repeat(g["truncated"][:, None], B, axis=1))


# ---- one launch against two launches per env-step -----------------------------------------------------------------------------------
def _snap(ro, venv):
    s = {k: getattr(ro, k).cpu().numpy().copy() for k in KEYS}
    s.update({"state_" + k: (venv.core.t[k].cpu().numpy().copy() if venv.core.t.get(k) is not None else None) for k in STATE})
    return s


def _rollouts(make, order, T, one_launch, use_graph=False, runs=1, noise=False, clamp=(0.96, 1.44)):
    from pde_control_gym import DeviceRollout, TrafficBacksteppingController
    venv = make()
    ctrl = TrafficBacksteppingController(venv, order=order)
    ro = DeviceRollout(venv, ctrl.attach(venv), T, use_graph=use_graph, action_low=clamp[0], action_high=clamp[1], action_noise=noise,
                       one_launch=one_launch)
    assert ro.one_launch is one_launch
    out = []
    for r in range(runs):
        if noise:
            ro.action_noise.copy_(torch.from_numpy(np.random.default_rng(70 + r).normal(0, 0.02, tuple(ro.action_noise.shape)).astype(np.float32)))
        ro.run()
        torch.cuda.synchronize()
        out.append(_snap(ro, venv))
    return out


@pytest.mark.parametrize("cf", [1, 2])
@pytest.mark.parametrize("sim", ["outlet", "both", "inlet"])
@pytest.mark.parametrize("order", ["numpy", "tree"])
def test_one_launch_equals_two_launches(order, sim, cf):
    """T = 70 env-steps, B in {1, 5, 67} (B = 5: per-instance densities and weight rows), with action noise and a clamp that binds."""
    for B in (1, 5, 67):
        rs = [RS3[b % 3] for b in range(B)] if B == 5 else None
        make = functools.partial(_venv, sim, B, cf, rs=rs)
        one = _rollouts(make, order, 70, True, noise=True, clamp=(1.1, 1.21))
        two = _rollouts(make, order, 70, False, noise=True, clamp=(1.1, 1.21))
        _same(one[0], two[0], f"{order} {sim} cf={cf} B={B}")
        a = one[0]["actions"]
        assert (a == 1.21).any() and ((a > 1.1) & (a < 1.21)).any()


@pytest.mark.parametrize("auto_reset", [True, False])
@pytest.mark.parametrize("order", ["numpy", "tree"])
@pytest.mark.parametrize("use_graph", [False, True])
def test_one_launch_equals_two_launches_with_restarts_inside_the_launch(use_graph, order, auto_reset):
    """Episodes of T = 2 s end after 32 env-steps: with the fused auto-reset the freeways restart twice inside each launch of 70
    steps (the law then reads the restarted state from registers), without it the finished episodes keep running.  Eagerly, and from
    a captured graph replayed twice."""
    B = 5
    make = functools.partial(_venv, "both", B, 2, T=2, pool=np.full(2 * B + 1, 0.12) if auto_reset else None)
    one = _rollouts(make, order, 70, True, use_graph=use_graph, runs=2)
    two = _rollouts(make, order, 70, False, use_graph=use_graph, runs=2)
    for run in range(2):
        _same(one[run], two[run], f"run {run}")
    ends = (one[0]["terminated"] | one[0]["truncated"]).sum(axis=0)
    assert ends.min() >= 2
    if auto_reset:
        assert one[1]["state_reset_count"].min() >= 4
        assert not np.array_equal(one[0]["obs"][33], one[0]["obs"][32])


# ---- output contracts ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [51, 129, 200])
@pytest.mark.parametrize("sim", ["outlet", "both", "inlet"])
def test_control_writes_exactly_its_outputs(M, sim, policy=None):
    """Poisoned output fully written, guard bands of every buffer intact, inputs untouched (register and strided kernels).
    ``policy`` displaces every guarded buffer off its 256-byte boundary (tests/poison.py; tests/test_gpu_pointer_alignment.py)."""
    from pde_control_gym import TrafficBacksteppingController
    B = 5
    rs, obs, want, _ = _control_case(M, B, sim)
    core = _core(sim, M, B, rs)
    ctrl = TrafficBacksteppingController(core, order="numpy" if M <= 129 else "tree")
    arena = poison.Arena("cuda", policy=policy)
    shape = (B, 2) if sim == "both" else (B,)
    o = arena.like("obs", torch.as_tensor(obs, device="cuda"))
    nz = arena.like("noise", torch.as_tensor(np.random.default_rng(4).normal(0, 0.01, shape).astype(np.float32), device="cuda"))
    ctrl.weights_v, ctrl.weights_q = arena.like("weights_v", ctrl.weights_v), arena.like("weights_q", ctrl.weights_q)
    core.t["rs"] = arena.like("rs", core.t["rs"])
    before = {k: v.t.clone() for k, v in arena.bufs.items()}
    out = poison.poison_(arena.new("out", shape, torch.float64))
    clean = torch.zeros(shape, dtype=torch.float64, device="cuda")
    ctrl.forward_into(o, clean, clamp=(0.5, 2.0), noise=nz)
    ctrl.forward_into(o, out, clamp=(0.5, 2.0), noise=nz)
    arena.check()
    poison.assert_written(out, None, "out", like=clean)
    for k, v in before.items():
        poison.assert_bits_equal(arena.bufs[k].t, v, None, f"input {k}")


@pytest.mark.parametrize("sim", ["outlet", "both", "inlet"])
@pytest.mark.parametrize("order", ["numpy", "tree"])
def test_rollout_writes_exactly_its_outputs(order, sim, policy=None):
    """Observation slots 1 .. T, actions, rewards and flags poisoned and fully written; slot 0, the weights and the noise untouched;
    every guard band intact; the engine state as after the clean run (restarts inside the launch included).
    ``policy`` displaces every guarded buffer off its 256-byte boundary (tests/poison.py; tests/test_gpu_pointer_alignment.py)."""
    from pde_control_gym import TrafficBacksteppingController
    B, T = 5, 40
    A = 2 if sim == "both" else 1

    def run(arena):
        venv = _venv(sim, B, 2, T=2, pool=np.full(7, 0.12))
        core = venv.core
        ctrl = TrafficBacksteppingController(venv, order=order)
        M = core.M
        new = (lambda n, s, d: arena.new(n, s, d)) if arena else (lambda n, s, d: torch.zeros(s, dtype=d, device="cuda"))
        obs, actions = new("obs", (T + 1, B, 2 * M), torch.float64), new("actions", (T, B, A), torch.float64)
        rewards, done, trunc = new("rewards", (T, B), torch.float64), new("done", (T, B), torch.uint8), new("truncated", (T, B), torch.uint8)
        noise = new("noise", (T, B, A), torch.float32)
        noise.copy_(torch.from_numpy(np.random.default_rng(9).normal(0, 0.01, (T, B, A)).astype(np.float32)))
        if arena:
            ctrl.weights_v, ctrl.weights_q = arena.like("weights_v", ctrl.weights_v), arena.like("weights_q", ctrl.weights_q)
            for t in (obs, actions, rewards, done, trunc):
                poison.poison_(t)
        obs[0].copy_(core.t["obs"])
        inputs = {"obs0": obs[0].clone(), "noise": noise.clone(), "weights_v": ctrl.weights_v.clone(), "weights_q": ctrl.weights_q.clone()}
        core.rollout(obs, actions, rewards, done, trunc, law=ctrl.rollout_law(actions, (0.96, 1.44), noise))
        torch.cuda.synchronize()
        now = {"obs0": obs[0], "noise": noise, "weights_v": ctrl.weights_v, "weights_q": ctrl.weights_q}
        for k, v in inputs.items():
            poison.assert_bits_equal(now[k], v, None, f"input {k}")
        state = {k: core.t[k].clone() for k in STATE if core.t.get(k) is not None}
        return dict(obs=obs, actions=actions, rewards=rewards, done=done, truncated=trunc), state

    cout, cstate = run(None)
    arena = poison.Arena("cuda", policy=policy)
    pout, pstate = run(arena)
    arena.check()
    for k, v in pout.items():
        poison.assert_written(v[1:] if k == "obs" else v, None, k, like=cout[k][1:] if k == "obs" else cout[k])
    for k, v in pstate.items():
        poison.assert_bits_equal(v, cstate[k], None, f"state {k}")
    assert int(cstate["reset_count"].min()) >= 1


# ---- non-finite rows -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [51, 129])
@pytest.mark.parametrize("order", ["numpy", "tree"])
@pytest.mark.parametrize("bad", sorted(nonfinite.PLANTS))
def test_a_non_finite_row_touches_only_its_own_command_and_the_clamp_keeps_nan(bad, order, M):
    from pde_control_gym import TrafficBacksteppingController
    B, victim = 5, 3
    rs, obs, _, _ = _control_case(M, B)
    ctrl = TrafficBacksteppingController(_core("outlet", M, B, rs), order=order)
    clean = ctrl(torch.as_tensor(obs, device="cuda")).cpu().numpy()
    for index in ((victim, 2), (victim, M + M // 2), (victim, 2 * M - 1)):      # a density, a speed, the last node
        planted = nonfinite.plant(obs, index, nonfinite.PLANTS[bad])
        got = ctrl(torch.as_tensor(planted, device="cuda")).cpu().numpy()
        assert not np.isfinite(got[victim]), (index, got[victim])
        others = nonfinite.rows_except(B, [victim])
        np.testing.assert_array_equal(_bits(got[others]), _bits(clean[others]))
        out = torch.zeros(B, dtype=torch.float64, device="cuda")
        ctrl.forward_into(torch.as_tensor(planted, device="cuda"), out, clamp=(0.96, 1.44))
        out = out.cpu().numpy()
        want = np.clip(got, 0.96, 1.44)          # np.clip keeps a NaN and brings +-Inf to the bound
        nonfinite.same_bits_and_nans(out, want, f"clamped, {bad} at {index}")
        if bad == "nan":
            assert np.isnan(out[victim])


# ---- batch invariance ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["numpy", "tree"])
def test_an_instance_gets_the_same_bits_in_every_batch(order):
    """Freeway b (its own density, hence its own state and weight row) in a batch of 67 and in a batch of 3 at another position of
    the workgroup: the same commands, observations, rewards and end state, from both kernels."""
    from pde_control_gym import TrafficBacksteppingController
    ids, T = (66, 2, 31), 12
    rs_all = np.array([RS3[b % 3] for b in range(67)])

    def run(rs):
        B = len(rs)
        venv = _venv("both", B, 2, rs=rs)
        core = venv.core
        ctrl = TrafficBacksteppingController(venv, order=order)
        first = ctrl(core.t["obs"]).cpu().numpy()
        obs = torch.zeros(T + 1, B, 2 * core.M, dtype=torch.float64, device="cuda")
        actions, rewards = torch.zeros(T, B, 2, dtype=torch.float64, device="cuda"), torch.zeros(T, B, dtype=torch.float64, device="cuda")
        done, trunc = torch.zeros(T, B, dtype=torch.uint8, device="cuda"), torch.zeros(T, B, dtype=torch.uint8, device="cuda")
        obs[0].copy_(core.t["obs"])
        core.rollout(obs, actions, rewards, done, trunc, law=ctrl.rollout_law(actions, None, None))
        return first, obs.cpu().numpy(), actions.cpu().numpy(), rewards.cpu().numpy(), core.t["r"].cpu().numpy(), core.t["y"].cpu().numpy()

    big, small = run(rs_all), run(rs_all[list(ids)])
    for k, b in enumerate(ids):
        np.testing.assert_array_equal(_bits(big[0][b]), _bits(small[0][k]), err_msg="control kernel")
        np.testing.assert_array_equal(_bits(big[2][0, b]), _bits(big[0][b]), err_msg="step 0 of the rollout against the control kernel")
        for j in (1, 2, 3):
            np.testing.assert_array_equal(_bits(big[j][:, b]), _bits(small[j][:, k]), err_msg=f"rollout output {j} of instance {b}")
        for j in (4, 5):
            np.testing.assert_array_equal(_bits(big[j][b]), _bits(small[j][k]), err_msg=f"end state {j} of instance {b}")
    assert len({big[2][5, b, 1] for b in ids}) == 3          # three densities, three different feedbacks
