"""GPU tests of pdegym_gae (csrc/pdegym_gae.hip) and pde_control_gym.DeviceRolloutBuffer: the kernel against the NumPy restatement of
SB3's loop (tests/gae_restatement.py) BIT FOR BIT over the lengths around its unroll depth and the batch sizes around a wave, against
the torch loop it replaces, its output contract on poisoned and guarded buffers, batch invariance on column shards that are views,
non-finite data, accumulators across calls, and rollout + critic + GAE captured in one graph.

Every launch of this file goes through ``_launch``, which ALWAYS checks the contract: inputs live in guarded [rows, ld] buffers whose
padding columns hold poison, outputs are poisoned and guarded, and after the launch every [t, b < B] element is written, the padding
and the guards are untouched and every input is bit-unchanged."""
import numpy as np
import pytest

from tests import gae_restatement as R
from tests import poison

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

DEPTH = 16                                            # csrc/pdegym_gae.hip: kSteps, the steps per iteration of the main loops
# one step (reads values[T] only); tail only (2, 7, 8, 9, DEPTH-1); DEPTH: one iteration, no tail; DEPTH+1; two iterations + tail
T_LIST = (1, 2, 7, 8, 9, DEPTH - 1, DEPTH, DEPTH + 1, 2 * DEPTH + 1)
B_LIST = (1, 63, 64, 65, 130)                         # one lane; one short of / exactly / one past a wave; three waves, the last partial
DISCOUNTS = ((0.99, 0.95), (1.0, 1.0), (0.0, 0.5))


def _backend():
    from pdecontrolgym_amd.backend import default_backend
    return default_backend()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 4: np.int32, 8: np.int64}[a.dtype.itemsize])


def _case(T, B, f64=False, seed=0):
    """The seeded rollout of tests/gae_restatement.py with the shapes of episode every path must meet planted on top: column 0 ends
    at t = 0 and at t = T-1 (terminated) and, from T = 4, at two consecutive steps; column 1 ends EVERY step; column 2 NEVER ends;
    column 3 has truncated-only steps (the boot rule) and column 4 steps with both flags set.  With fewer columns the later plants
    fall away (B = 1 keeps column 0); the random flags (8 % each, independent) add the rest."""
    rew, val, te, tr, boot = R.seeded_case(T, B, seed=seed, f64_rewards=f64)
    te[0, 0] = te[T - 1, 0] = 1
    if T >= 4:
        te[1, 0], tr[2, 0] = 1, 1
        te[2, 0] = 0
    if B > 1:
        te[:, 1] = 1
    if B > 2:
        te[:, 2] = tr[:, 2] = 0
    if B > 3:
        te[:, 3], tr[::2, 3] = 0, 1
    if B > 4:
        te[::3, 4] = tr[::3, 4] = 1
    return rew, val, te, tr, boot


def test_the_fixture_holds_every_planted_shape():
    rew, val, te, tr, boot = _case(33, 130)
    done = (te | tr).astype(bool)
    assert done[0, 0] and done[32, 0] and done[1, 0] and done[2, 0]                  # ends at t = 0, t = T-1, two in a row
    assert done[:, 1].all() and not done[:, 2].any()                                # every step; never
    assert ((tr == 1) & (te == 0)).any() and ((tr == 1) & (te == 1)).any()          # truncated only; both flags
    assert (((tr == 1) & (te == 0))[:, 5:]).any() and (~done[:, 5:]).any()          # ... also among the random columns


def _launch(rew, val, te, tr, boot, gamma, lam, ld=None, stats=True, acc=None, cols=None, policy=None):
    """One pdegym_gae launch on guarded device copies of the NumPy arrays, row stride ``ld`` (default B); ``tr`` / ``boot`` may be
    None; ``acc``: (ep_return_acc, ep_length_acc) NumPy arrays to start from, None = accumulators not given; ``cols``: a slice of
    columns -- the launch then covers that shard only, as views of the full-width buffers.  Returns the outputs as NumPy arrays
    (full width) after the contract checks of the module docstring.  ``policy``: the displacement of every guarded buffer off its
    256-byte boundary (tests/poison.py; tests/test_gpu_pointer_alignment.py)."""
    T, B = rew.shape
    ld = B if ld is None else ld
    A = poison.Arena("cuda", policy=policy)
    sel = slice(0, B) if cols is None else cols
    nb = len(range(*sel.indices(B)))

    def inp(name, a, rows):
        if a is None:
            return None
        full = A.new(name, (rows, ld), torch.from_numpy(a).dtype)
        poison.poison_(full)
        full[:, :B].copy_(torch.from_numpy(a))
        return full

    ins = {"rewards": inp("rewards", rew, T), "values": inp("values", val, T + 1), "terminated": inp("terminated", te, T),
           "truncated": inp("truncated", tr, T), "boot": inp("boot", boot, T)}
    before = {k: v.clone() for k, v in ins.items() if v is not None}
    outs = {"advantages": A.new("advantages", (T, ld), torch.float32), "returns": A.new("returns", (T, ld), torch.float32)}
    if stats:
        outs["episode_return"] = A.new("episode_return", (T, ld), torch.float64)
        outs["episode_length"] = A.new("episode_length", (T, ld), torch.int32)
        poison.fill_int_(outs["episode_length"], -7)
    for k in ("advantages", "returns", "episode_return"):
        if k in outs:
            poison.poison_(outs[k])
    accs = {}
    if acc is not None:
        accs = {"ep_return_acc": A.new("ep_return_acc", (B,), torch.float64), "ep_length_acc": A.new("ep_length_acc", (B,), torch.int32)}
        accs["ep_return_acc"].copy_(torch.from_numpy(acc[0]))
        accs["ep_length_acc"].copy_(torch.from_numpy(acc[1]))
    acc_before = {k: v.clone() for k, v in accs.items()}
    view = lambda x: None if x is None else x[:, sel]      # noqa: E731
    _backend().gae(view(ins["rewards"]), view(ins["values"]), view(ins["terminated"]), view(ins["truncated"]), view(outs["advantages"]),
                   view(outs["returns"]), gamma, lam, boot=view(ins["boot"]), episode_return=view(outs.get("episode_return")),
                   episode_length=view(outs.get("episode_length")), **{k: v[sel] for k, v in accs.items()})
    A.check()                                               # (synchronises) no guard byte changed
    inside = torch.zeros(ld, dtype=torch.bool, device="cuda")
    inside[:B][sel] = True
    for k, x in outs.items():
        if k == "episode_length":
            assert bool((x[:, inside] != -7).all()), f"{k}: elements that must be written still hold the fill"
            assert bool((x[:, ~inside] == -7).all()), f"{k}: elements outside the launch were written"
        else:
            poison.assert_written(x, (slice(None), inside), k)
            poison.assert_untouched(x, (slice(None), ~inside), k)
    for k, x in before.items():
        poison.assert_bits_equal(ins[k], x, None, k)
    for k, x in acc_before.items():                          # accumulators of columns outside the shard keep their bits
        poison.assert_bits_equal(accs[k][~inside[:B]], x[~inside[:B]], None, k)
    assert nb >= 1
    got = {k: x[:, :B].cpu().numpy() for k, x in outs.items()}
    got.update({k: x.cpu().numpy() for k, x in accs.items()})
    return got


def _expect(rew, val, te, tr, boot, gamma, lam, acc=None):
    adv, ret = R.gae_reference(rew, val, te, tr, gamma, lam, boot)
    er, el, a, n = R.episode_scan(rew, te, tr, *(acc if acc is not None else (None, None)))
    return {"advantages": adv, "returns": ret, "episode_return": er, "episode_length": el, "ep_return_acc": a, "ep_length_acc": n}


def _assert_same(got, want, what, nan_equal=False):
    for k, g in got.items():
        w = want[k]
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k, g.dtype, w.dtype, g.shape, w.shape)
        same = _bits(g) == _bits(w)
        if nan_equal and g.dtype.kind == "f":
            same |= np.isnan(g) & np.isnan(w)
        assert same.all(), (what, k, int((~same).sum()), tuple(int(i) for i in np.argwhere(~same)[0]))


@pytest.mark.parametrize("B", B_LIST)
@pytest.mark.parametrize("T", T_LIST)
def test_bit_parity_with_the_restatement(T, B):
    """advantages, returns, episode_return, episode_length and both accumulators equal the restatement bit for bit: float32 and
    float64 rewards, ld = B and B + 3, with boot / without / with truncated = NULL as well, three pairs of discounts."""
    rng = np.random.default_rng([T, B])
    for f64 in (False, True):
        rew, val, te, tr, boot = _case(T, B, f64)
        acc = (rng.normal(0.0, 3.0, B), rng.integers(0, 50, B).astype(np.int32))
        for ld in (B, B + 3):
            for tr_, boot_ in ((tr, boot), (tr, None), (None, None)):
                for gamma, lam in DISCOUNTS:
                    got = _launch(rew, val, te, tr_, boot_, gamma, lam, ld=ld, acc=acc)
                    _assert_same(got, _expect(rew, val, te, tr_, boot_, gamma, lam, acc), (f64, ld, tr_ is None, boot_ is None, gamma))
        # the statistics without accumulators start every environment from zero; without statistics only the two outputs exist
        got = _launch(rew, val, te, tr, boot, 0.99, 0.95, ld=B + 3)
        want = _expect(rew, val, te, tr, boot, 0.99, 0.95)
        _assert_same(got, want, ("no accumulators", f64))
        got = _launch(rew, val, te, tr, boot, 0.99, 0.95, stats=False)
        assert sorted(got) == ["advantages", "returns"]
        _assert_same(got, want, ("no statistics", f64))


def test_equal_to_the_torch_loop_it_replaces():
    """The loop of examples/train_ppo_device.py before the buffer, on device tensors, gives the same adv and ret bit for bit."""
    T, B = 16, 130
    rew, val, te, tr, _ = _case(T, B)
    gamma, lam = 0.99, 0.95
    dev = torch.device("cuda")
    rew_d, val_d = torch.from_numpy(rew).to(dev), torch.from_numpy(val).to(dev)
    done = (torch.from_numpy(te).to(dev) | torch.from_numpy(tr).to(dev)).float()
    adv = torch.zeros(T, B, device=dev)
    last = torch.zeros(B, device=dev)
    for t in reversed(range(T)):                  # GAE; an episode end cuts the bootstrap
        nonterm = 1.0 - done[t]
        delta = rew_d[t] + gamma * val_d[t + 1] * nonterm - val_d[t]
        last = delta + gamma * lam * nonterm * last
        adv[t] = last
    ret = adv + val_d[:T]
    got = _launch(rew, val, te, tr, None, gamma, lam, stats=False)
    _assert_same(got, {"advantages": adv.cpu().numpy(), "returns": ret.cpu().numpy()}, "torch loop")


def test_output_contract_and_unselected_boot():
    """The contract checks of ``_launch`` at a ragged shape with padding columns, and boot as a SELECT: NaN in every entry the rule
    (truncated and not terminated) does not pick changes no bit."""
    T, B = 17, 65
    for f64 in (False, True):
        rew, val, te, tr, boot = _case(T, B, f64)
        ref = _launch(rew, val, te, tr, boot, 0.99, 0.95, ld=B + 3, acc=(np.zeros(B), np.zeros(B, np.int32)))
        picked = (tr == 1) & (te == 0)
        assert picked.any() and (~picked).any()
        holed = np.where(picked, boot, np.float32(np.nan)).astype(np.float32)
        got = _launch(rew, val, te, tr, holed, 0.99, 0.95, ld=B + 3, acc=(np.zeros(B), np.zeros(B, np.int32)))
        _assert_same(got, ref, ("NaN in unselected boot", f64))
        assert np.isfinite(got["advantages"]).all()
        # and the selected entries do matter
        other = _launch(rew, val, te, tr, None, 0.99, 0.95, ld=B + 3, stats=False)
        assert (_bits(other["advantages"]) != _bits(ref["advantages"])).any()


def test_batch_invariance_on_column_shards_that_are_views():
    """Columns computed in a batch of 130 equal the same columns computed as the shards [0:64], [64:130] and one single column:
    views with ld = 130, nothing is copied."""
    T, B = 33, 130
    rng = np.random.default_rng(7)
    for f64 in (False, True):
        rew, val, te, tr, boot = _case(T, B, f64)
        acc = (rng.normal(0.0, 3.0, B), rng.integers(0, 50, B).astype(np.int32))
        whole = _launch(rew, val, te, tr, boot, 0.99, 0.95, acc=acc)
        for cols in (slice(0, 64), slice(64, 130), slice(77, 78)):
            part = _launch(rew, val, te, tr, boot, 0.99, 0.95, acc=acc, cols=cols)
            for k, x in part.items():
                assert np.array_equal(_bits(x[..., cols]), _bits(whole[k][..., cols])), (k, cols, f64)


def test_non_finite_values_stay_in_their_column():
    """One NaN reward and one Inf value at known places: the outputs equal the restatement's (NaNs compared as equal), and every
    other column keeps the bits of the clean run."""
    T, B = 17, 65
    rew, val, te, tr, boot = _case(T, B)
    clean = _launch(rew, val, te, tr, boot, 0.99, 0.95)
    rew2, val2 = rew.copy(), val.copy()
    (t_nan, b_nan), (t_inf, b_inf) = (9, 7), (12, 40)
    rew2[t_nan, b_nan] = np.nan
    val2[t_inf, b_inf] = np.inf
    got = _launch(rew2, val2, te, tr, boot, 0.99, 0.95)
    _assert_same(got, _expect(rew2, val2, te, tr, boot, 0.99, 0.95), "non-finite", nan_equal=True)
    assert np.isnan(got["advantages"][t_nan, b_nan]) and not np.isfinite(got["returns"][t_inf, b_inf])
    others = np.ones(B, bool)
    others[[b_nan, b_inf]] = False
    for k, x in got.items():
        assert np.array_equal(_bits(x[..., others]), _bits(clean[k][..., others])), k
        assert np.isfinite(x[..., others]).all(), k


def test_accumulators_carry_episodes_across_calls():
    """Two launches over the two halves of a 2T rollout give the episode statistics of one launch over the whole."""
    T, B = 9, 65
    for f64 in (False, True):
        rew, val, te, tr, _ = _case(2 * T, B, f64)
        zero = (np.zeros(B), np.zeros(B, np.int32))
        whole = _launch(rew, val, te, tr, None, 0.99, 0.95, acc=zero)
        first = _launch(rew[:T], val[:T + 1], te[:T], tr[:T], None, 0.99, 0.95, acc=zero)
        second = _launch(rew[T:], val[T:], te[T:], tr[T:], None, 0.99, 0.95, acc=(first["ep_return_acc"], first["ep_length_acc"]))
        for k in ("episode_return", "episode_length"):
            assert np.array_equal(_bits(np.concatenate([first[k], second[k]])), _bits(whole[k])), (k, f64)
        for k in ("ep_return_acc", "ep_length_acc"):
            assert np.array_equal(_bits(second[k]), _bits(whole[k])), (k, f64)
        assert (whole["episode_length"][T:] > T).any(), "no episode spans the two halves: the case shows nothing"


# ---- DeviceRolloutBuffer behind a rollout ---------------------------------------------------------------------------------------------
def _parabolic_env(B, nx=16, S=5, horizon=6):
    import pde_control_gym
    from pde_control_gym.src import TunedReward1D
    dx = 1.0 / nx
    dt = 0.25 * dx * dx
    beta = np.full(nx + 1, 12.0, np.float32)
    rng = np.random.default_rng(0)

    def batched_reset(idx, n):
        amp = rng.uniform(1.0, 5.0, (len(idx), 1)).astype(np.float32)
        x = np.linspace(0, 1, n + 1, dtype=np.float32)[None, :]
        return amp * np.sin(np.pi * x).astype(np.float32) + amp * 0.2, np.tile(beta, (len(idx), 1))

    kw = {"T": horizon * S * dt, "dt": dt, "X": 1, "dx": dx, "reward_class": TunedReward1D(horizon * S, -1e-2, 20.0), "normalize": True,
          "sensing_loc": "full", "control_type": "Dirchilet", "sensing_type": None, "sensing_noise_func": None,
          "limit_pde_state_size": True, "max_state_value": 1e3, "max_control_value": 10.0, "control_sample_rate": S * dt,
          "batched_reset_func": batched_reset}
    venv = pde_control_gym.make_vec("PDEControlGym-ReactionDiffusionPDE1D", num_envs=B, **kw)
    obs0 = venv.reset_tensor()
    venv.enable_fused_auto_reset()
    return venv, obs0.shape[1]


def _mlp(sizes, seed):
    torch.manual_seed(seed)
    mods = []
    for i in range(len(sizes) - 1):
        mods += [torch.nn.Linear(sizes[i], sizes[i + 1])] + ([torch.nn.Tanh()] if i < len(sizes) - 2 else [])
    return torch.nn.Sequential(*mods).cuda()


def _snapshot(ro, buf):
    torch.cuda.synchronize()
    return {k: getattr(o, k).clone() for o, ks in ((ro, ("obs", "actions", "rewards", "terminated", "truncated")),
                                                   (buf, ("values", "advantages", "returns", "episode_return", "episode_length",
                                                          "ep_return_acc", "ep_length_acc"))) for k in ks}


def test_rollout_critic_and_gae_in_one_graph_equal_the_eager_calls():
    """rollout.run() (one launch, fused auto-reset, episodes of 6 steps inside rollouts of 8) and buffer.compute(FusedMLP critic)
    captured in ONE torch.cuda.graph: two replays with fresh exploration noise equal the same calls made eagerly on a twin
    environment, bit for bit; the eager results equal the restatement."""
    from pde_control_gym import DeviceRollout, DeviceRolloutBuffer, FusedMLP
    B, T = 65, 8
    noise = torch.randn(3, T, B, generator=torch.Generator().manual_seed(4)).mul_(0.5).cuda()
    runs = {}
    for mode in ("eager", "graph"):
        venv, D = _parabolic_env(B)
        actor, critic = FusedMLP(_mlp([D, 32, 1], 1)), FusedMLP(_mlp([D, 32, 1], 2))
        ro = DeviceRollout(venv, actor, T, use_graph=False, action_noise=True, one_launch=True, action_low=-10.0, action_high=10.0)
        buf = DeviceRolloutBuffer(ro, gamma=0.99, gae_lambda=0.95)

        def both():
            ro.run()
            buf.compute(critic=critic)
        ro.action_noise.copy_(noise[0])
        both()                                       # (also the warm-up of the captured calls)
        snaps = []
        if mode == "graph":
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                both()
        for i in (1, 2):
            ro.action_noise.copy_(noise[i])
            if mode == "graph":
                graph.replay()
            else:
                both()
            snaps.append(_snapshot(ro, buf))
        runs[mode] = snaps
    for i, (a, b) in enumerate(zip(runs["eager"], runs["graph"])):
        for k in a:
            poison.assert_bits_equal(b[k], a[k], None, f"replay {i}: {k}")
    e = {k: v.cpu().numpy() for k, v in runs["eager"][1].items()}
    assert (e["terminated"] | e["truncated"]).any() and (e["episode_length"] == 6).any(), "no episode ended inside the buffer"
    assert not np.array_equal(runs["eager"][0]["actions"].cpu().numpy(), e["actions"])
    adv, ret = R.gae_reference(e["rewards"], e["values"], e["terminated"], e["truncated"], 0.99, 0.95)
    assert np.array_equal(_bits(e["advantages"]), _bits(adv)) and np.array_equal(_bits(e["returns"]), _bits(ret))


def test_buffer_on_the_float64_family_equals_the_restatement():
    """TrafficPDE1D (8 nodes: float64 observations and rewards), eagerly: a FusedMLP critic reads the float64 observation rows, the
    kernel rounds each float64 reward once, and the episode returns are sums of the float64 rewards themselves."""
    import random
    import pde_control_gym
    from pde_control_gym import DeviceRollout, DeviceRolloutBuffer, FusedMLP
    from pde_control_gym.src import TrafficARZReward
    random.seed(0)
    B, T = 65, 8
    venv = pde_control_gym.make_vec("PDEControlGym-TrafficPDE1D", num_envs=B, reward_class=TrafficARZReward(), simulation_type="both",
                                    limit_pde_state_size=True, control_freq=2, T=240, dt=0.25, X=70, dx=10)
    venv.reset_tensor()
    assert venv.core.M == 8
    torch.manual_seed(2)
    lin = torch.nn.Linear(16, 2).double().cuda()
    ro = DeviceRollout(venv, lambda o: 4.6 + 0.5 * torch.tanh(lin(o)), T, use_graph=False, action_low=3.0, action_high=6.0).run()
    assert ro.rewards.dtype == torch.float64 and ro.obs.dtype == torch.float64
    critic = FusedMLP(_mlp([16, 8, 1], 3))
    buf = DeviceRolloutBuffer(ro, gamma=0.99, gae_lambda=0.95).compute(critic=critic)
    torch.cuda.synchronize()
    out = torch.empty((T + 1) * B, 1, device="cuda")
    critic.forward_into(ro.obs.reshape((T + 1) * B, -1), out, clamp=None)
    poison.assert_bits_equal(buf.values, out.reshape(T + 1, B), None, "values")
    n = lambda x: x.cpu().numpy()      # noqa: E731
    rew, te, tr = n(ro.rewards), n(ro.terminated), n(ro.truncated)
    assert np.isfinite(rew).all() and (rew.astype(np.float32).astype(np.float64) != rew).any()      # the rounding on load is a real one
    adv, ret = R.gae_reference(rew, n(buf.values), te, tr, 0.99, 0.95)
    er, el, acc, ln = R.episode_scan(rew, te, tr)
    for got, want, k in ((buf.advantages, adv, "advantages"), (buf.returns, ret, "returns"), (buf.episode_return, er, "episode_return"),
                         (buf.episode_length, el, "episode_length"), (buf.ep_return_acc, acc, "ep_return_acc"),
                         (buf.ep_length_acc, ln, "ep_length_acc")):
        assert np.array_equal(_bits(n(got)), _bits(want)), k
    count, _, _ = buf.finished_episodes()
    assert int(count) == int((el > 0).sum())
