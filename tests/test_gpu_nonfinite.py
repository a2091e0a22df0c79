"""Non-finite inputs on the device: a NaN / +Inf / -Inf command, a NaN observation, a NaN cell in a state.

To the reference a NaN is ordinary data: np.clip, torch.clamp, np.max and Python's min / max keep it, a stencil spreads it to the
cells that read it.  Every family here makes two kinds of assertion (tests/nonfinite.py):

  (a) parity     the engine's outputs equal the oracle's (oracle/pde_oracle.py, pinned to the reference on these inputs by
                 tests/test_oracle_nonfinite.py): equal NaN masks, equal bits elsewhere on the float64 paths; rewards keep the
                 tolerance of the family's finite tests, plus an equal NaN mask;
  (b) isolation  instances that received no non-finite value are bit-identical to the same instances of a clean run of the same
                 batch -- the poisoned instances share their workgroup (and MFMA tile) with them.

Every comparison covers every element.  No test passes a non-finite size, stride or count: the kernels index with integers that
never derive from the data (the tumour radii are ballot indices, the pool rows come from integer counters).
"""
import numpy as np
import pytest
import torch

from oracle import pde_oracle as po
from tests import nonfinite as NF

pytestmark = pytest.mark.gpu
DEV = "cuda"
f32, f64 = np.float32, np.float64
NAN, PINF, NINF = NF.NAN, NF.PINF, NF.NINF


def _np(t):
    return t.detach().cpu().numpy()


def _flags(t):
    return _np(t).astype(bool)


# ---- traffic ----------------------------------------------------------------------------------------------------------------------
TRAFFIC_B = 5
TRAFFIC_STEPS = 6


def _traffic_pair(sim, dx, B=TRAFFIC_B):
    """Engine and oracle on X = 500: dx = 10 gives the reference's M = 51 (one node per lane, register kernel), dx = 2 gives M = 251
    (four nodes per lane, the LDS kernel).  Different steady states per instance, so that instances cannot stand in for each other."""
    from pdecontrolgym_amd.batch_traffic import TrafficBatch
    dt = 0.25 if dx == 10 else 0.04
    args = (240, dt, 500, dx, sim, 40, 0.16, 60, True, 1)
    env, orc = TrafficBatch(*args, num_envs=B, device=DEV), po.TrafficOracle(*args)
    rs = np.array([0.115, 0.12, 0.125, 0.1, 0.12])[:B]
    qclip = rs * (40 * (1 - rs / 0.16))
    env.set_action_bounds(qclip)
    NF.same_bits_and_nans(env.reset(rs), orc.reset(rs, qclip), "reset")
    return env, orc, qclip


def _traffic_actions(sim, qclip, clean):
    """[steps, B, A]: instance 0 clean; 1..3 NaN, +Inf, -Inf in column 0 at step 1; instance 4 NaN in column 1 for 'both' (column 0
    otherwise).  The clean twin holds the bound the reference clips an infinity to, and a finite command in place of the NaN."""
    A = 2 if sim == "both" else 1
    rng = np.random.default_rng(5)
    a = rng.uniform(0.7, 1.3, (TRAFFIC_STEPS, TRAFFIC_B, A)) * qclip[None, :, None]
    col4 = 1 if sim == "both" else 0
    if clean:
        a[1, 2, 0], a[1, 3, 0] = 1.2 * qclip[2], qclip[3] * 0.8
    else:
        a[1, 1, 0], a[1, 2, 0], a[1, 3, 0], a[1, 4, col4] = NAN, PINF, NINF, NAN
    return a


TRAFFIC_CLEAN_ROWS = [0, 2, 3]          # +-Inf is clipped to a bound: from then on the same freeway as the clean twin's


def _traffic_check_step(k, out, orc, env, a):
    o, r, d, t = out
    with np.errstate(all="ignore"):
        o_ref, r_ref, d_ref, t_ref = orc.step(a)
    NF.same_bits_and_nans(o, o_ref, f"step {k}: obs")
    NF.close_and_same_nans(r, r_ref, rtol=1e-12, what=f"step {k}: reward")      # tests/fuzz_more.py traffic_case
    assert np.array_equal(_flags(d), d_ref) and np.array_equal(_flags(t), t_ref), f"step {k}: flags {_flags(d)} {d_ref} {_flags(t)} {t_ref}"
    if env is not None:
        NF.same_bits_and_nans(env.t["r"], orc.r, f"step {k}: r")
        NF.same_bits_and_nans(env.t["y"], orc.y, f"step {k}: y")
        NF.same_bits_and_nans(env.t["time"], orc.time_index, f"step {k}: time")


@pytest.mark.parametrize("dx", [10, 2], ids=["M51", "M251"])
@pytest.mark.parametrize("sim", ["inlet", "outlet", "both"])
def test_traffic_step_parity_and_isolation(sim, dx):
    env, orc, qclip = _traffic_pair(sim, dx)
    twin, _, _ = _traffic_pair(sim, dx)
    acts, acts_clean = _traffic_actions(sim, qclip, False), _traffic_actions(sim, qclip, True)
    for k in range(TRAFFIC_STEPS):
        out = env.step(acts[k].copy())
        _traffic_check_step(k, out, orc, env, acts[k])
        ref = twin.step(acts_clean[k].copy())
        for name, x, y in zip(("obs", "reward", "done", "truncated"), out, ref):
            NF.same_bits_and_nans(x[TRAFFIC_CLEAN_ROWS], y[TRAFFIC_CLEAN_ROWS], f"step {k}: {name} of the clean instances")
    o = _np(env.t["obs"])
    assert np.isnan(o[1]).any() and np.isnan(o[4]).any() and not np.isnan(o[[0, 2, 3]]).any()
    assert np.isnan(_np(env.t["reward"])[[1, 4]]).all()


def _rollout_buffers(T, B, D, A):
    z = lambda *s, dt=torch.float64: torch.zeros(*s, dtype=dt, device=DEV)      # noqa: E731
    return z(T + 1, B, D), z(T, B, A), z(T, B), z(T, B, dt=torch.uint8), z(T, B, dt=torch.uint8)


@pytest.mark.parametrize("sim", ["inlet", "outlet", "both"])
def test_traffic_rollout_with_given_commands(sim):
    env, orc, qclip = _traffic_pair(sim, 10)
    twin, _, _ = _traffic_pair(sim, 10)
    acts, acts_clean = _traffic_actions(sim, qclip, False), _traffic_actions(sim, qclip, True)
    T, B, D, A = TRAFFIC_STEPS, TRAFFIC_B, 2 * env.M, acts.shape[2]
    res = []
    for e, a in ((env, acts), (twin, acts_clean)):
        obs, act, rew, dn, tr = _rollout_buffers(T, B, D, A)
        obs[0].copy_(e.t["obs"])
        act.copy_(torch.as_tensor(a))
        e.rollout(obs, act, rew, dn, tr)
        res.append((obs, rew, dn, tr))
    obs, rew, dn, tr = res[0]
    for k in range(T):
        _traffic_check_step(k, (obs[k + 1], rew[k], dn[k], tr[k]), orc, None, acts[k])
    for name in ("r", "y", "time"):
        NF.same_bits_and_nans(env.t[name], {"r": orc.r, "y": orc.y, "time": orc.time_index}[name], "stored " + name)
    for name, x, y in zip(("obs", "reward", "done", "truncated"), res[0], res[1]):
        NF.same_bits_and_nans(x[:, TRAFFIC_CLEAN_ROWS], y[:, TRAFFIC_CLEAN_ROWS], f"{name} of the clean instances")


def _mlp(sizes, act="tanh", seed=0, positive_from=None, bias_last=0.0):
    """torch.nn.Sequential with the given layer sizes on the device; ``positive_from`` = index of the first layer whose weights are
    all made positive."""
    g = torch.Generator().manual_seed(seed)
    layers = []
    for i in range(len(sizes) - 1):
        lin = torch.nn.Linear(sizes[i], sizes[i + 1])
        with torch.no_grad():
            w = torch.randn(lin.weight.shape, generator=g) * (1.5 / np.sqrt(sizes[i]))
            lin.weight.copy_(w.abs() if positive_from is not None and i >= positive_from else w)
            lin.bias.copy_(torch.randn(lin.bias.shape, generator=g) * 0.3)
            if i == len(sizes) - 2:
                lin.bias.add_(bias_last)
        layers.append(lin)
        if i < len(sizes) - 2 and act != "identity":
            layers.append(torch.nn.Tanh() if act == "tanh" else torch.nn.ReLU())
    return torch.nn.Sequential(*layers).to(DEV)


@pytest.mark.parametrize("hidden", [16, 65], ids=["narrow", "wide"])
@pytest.mark.parametrize("sim", ["inlet", "both"])
def test_traffic_rollout_with_policy_inside(sim, hidden):
    """Instance 2 holds a NaN node in its stored density: its observation is NaN, so the command the policy computes inside the launch
    has to be NaN through the clamp, as FusedMLP.forward_into's is (wide: bit for bit; narrow: to float32 rounding, tests/
    fuzz_policy_rollout.py); the freeway then follows the oracle driven with the commands the kernel issued."""
    from pdecontrolgym_amd.policy import FusedMLP
    env, orc, qclip = _traffic_pair(sim, 10)
    twin, _, _ = _traffic_pair(sim, 10)
    M, B, T = env.M, TRAFFIC_B, TRAFFIC_STEPS
    D, A = 2 * M, env.action_dim
    pol = FusedMLP(_mlp([D, hidden, A], seed=hidden, bias_last=4.5), clamp=(3.0, 6.0))
    assert env.policy_fits_rollout(pol)
    noise = (torch.randn(T, B, A, generator=torch.Generator().manual_seed(1)) * 0.05).to(DEV)
    env.t["r"][2, 20] = NAN
    orc.r[2, 20] = NAN
    res = []
    for e in (env, twin):
        obs, act, rew, dn, tr = _rollout_buffers(T, B, D, A)
        obs[0].copy_(e.t["obs"])
        if e is env:                       # the observation of the poisoned state: (r, v = y / r + Veq(r))
            obs[0, 2, 20] = NAN
            obs[0, 2, M + 20] = NAN
        e.rollout(obs, act, rew, dn, tr, policy=pol, noise=noise)
        res.append((obs, act, rew, dn, tr))
    obs, act, rew, dn, tr = res[0]
    a_np = _np(act)
    assert np.isnan(a_np[:, 2]).all(), f"the clamp dropped the NaN command: {a_np[:, 2]}"
    assert not np.isnan(np.delete(a_np, 2, axis=1)).any() and (np.delete(a_np, 2, axis=1) >= 3.0).all() and (np.delete(a_np, 2, axis=1) <= 6.0).all()
    two = torch.zeros(B, A, dtype=torch.float64, device=DEV)
    for k in range(T):
        pol.forward_into(obs[k].contiguous(), two, noise=noise[k].contiguous())
        if hidden > 64:
            NF.same_bits_and_nans(act[k], two, f"step {k}: commands (wide: bit-identical to FusedMLP)")
        else:
            NF.close_and_same_nans(act[k], two, rtol=1e-4, atol=2e-5, what=f"step {k}: commands")
        _traffic_check_step(k, (obs[k + 1], rew[k], dn[k], tr[k]), orc, None, a_np[k])
    NF.same_bits_and_nans(env.t["r"], orc.r, "stored r")
    NF.same_bits_and_nans(env.t["y"], orc.y, "stored y")
    others = [0, 1, 3, 4]
    for name, x, y in zip(("obs", "actions", "reward", "done", "truncated"), res[0], res[1]):
        NF.same_bits_and_nans(x[:, others], y[:, others], f"{name} of the clean instances")


# ---- tumour -----------------------------------------------------------------------------------------------------------------------
# set A of tests/golden/make_golden.py gen_sweep_tumor on a wide initial profile: therapy from day 21 (tests/golden/nonfinite.npz)
TUMOR_A = dict(t1_detection_threshold=0.6, t2_detection_threshold=0.3, dosage_termination_threshold=1.0, D=0.1, rho=0.05, alpha=0.1,
               alpha_beta_ratio=3, k=1.0, t1_detection_radius=10, t1_death_radius=25)
TUMOR_B = 5


def _tumor_engine(X, T=60):
    from pdecontrolgym_amd.batch_tumor import TumorBatch
    eng = TumorBatch(T, 1, X, 1, 30.0, num_envs=TUMOR_B, device=DEV, **TUMOR_A)
    xs = np.linspace(0, X, eng.nx)
    init = (0.8 * np.exp(-(xs / 11.0) ** 2))[None] * np.array([1.0, 0.98, 0.96, 0.94, 0.92])[:, None]
    eng.set_benchmark(np.full(TUMOR_B, 30.0))
    return eng, init


class _TumorOracles:
    """One single-instance oracle per patient: where the reference raises for one of them, the others go on."""

    def __init__(self, X, T, init):
        self.o = [po.BrainTumorOracle(T, 1, X, 1, 30.0, **TUMOR_A) for _ in range(TUMOR_B)]
        for b, o in enumerate(self.o):
            o.reset(init[b:b + 1], [30.0])
        self.raised = [None] * TUMOR_B

    def step(self, control, part=None):
        out = []
        for b, o in enumerate(self.o):
            if self.raised[b] or (part is not None and not part[b]):
                out.append(None)
                continue
            try:
                with np.errstate(all="ignore"):
                    u, r, te, tr = o.step([control[b]])
                out.append((u[0], r[0], bool(te[0]), bool(tr[0])))
            except ZeroDivisionError as ex:
                self.raised[b] = ex
                out.append(None)
        return out

    def stack(self, attr):
        return np.array([getattr(o, attr)[0] for o in self.o])


def _tumor_compare(eng, orcs, outs, what, rows=None):
    """Rows rtol 1e-12 on non-NaN entries + equal NaN mask (tests/fuzz_more.py tumor_case), reward rtol 1e-11 + NaN mask, stage / day
    counters / remaining dosage / flags exact, for the instances whose oracle produced a value; then both sides continue from the
    engine's rows (the in-kernel exp may differ from libm's in the last bit, as in tumor_case)."""
    u, r, te, tr = (_np(x) for x in (eng.t["u"], eng.t["reward"], eng.t["terminated"], eng.t["truncated"]))
    days = _np(eng.t["days"])
    for b, out in enumerate(outs):
        if out is None:
            continue
        o = orcs.o[b]
        NF.close_and_same_nans(u[b], out[0], rtol=1e-12, what=f"{what}: row of instance {b}")
        if rows is None or rows[b]:
            NF.close_and_same_nans(r[b], out[1], rtol=1e-11, what=f"{what}: reward of instance {b}")
            assert bool(te[b]) == out[2] and bool(tr[b]) == out[3], f"{what}: flags of instance {b}"
        assert int(_np(eng.t["stage"])[b]) == int(o.stage[0]) and int(_np(eng.t["time_index"])[b]) == int(o.time_index[0]), f"{what}: stage / day of {b}"
        assert list(days[b]) == [o.growthDays[0], o.therapyDays[0], o.postDays[0], o.simulationDays[0], o.cDeathDay[0]], f"{what}: days of {b}"
        NF.same_bits_and_nans(_np(eng.t["remaining"])[b], f64(o.remaining[0]), f"{what}: remaining dosage of instance {b}")
        o.u = u[b:b + 1].copy()


TUMOR_DOSE = {2: NAN, 3: PINF, 4: NINF}


@pytest.mark.parametrize("path", ["daily", "advance"])
@pytest.mark.parametrize("X", [100, 400], ids=["nx101", "nx401"])
def test_tumor_parity_and_isolation(X, path):
    """Instance 1 starts with a NaN cell (node 40: the front reaches the tumour during therapy); instances 2, 3, 4 request a NaN,
    +Inf, -Inf dosage on their second therapy day.  nx = 101 takes the four-loads-at-once staging, nx = 401 the chunk loop.
    The day after a NaN or -Inf dosage the whole treated region is NaN, the tumour is invisible on T2, the treatment radius is 0 and
    the reference's reward raises ZeroDivisionError: the engine returns a NaN reward there (include/pdegym.h) and goes on."""
    from pdecontrolgym_amd import _native as N
    T = 60
    (eng, init), (twin, _) = _tumor_engine(X, T), _tumor_engine(X, T)
    bad = init.copy()
    bad[1, 40] = NAN
    orcs = _TumorOracles(X, T, bad)
    eng.reset(bad)
    twin.reset(init)
    B = TUMOR_B
    zero = np.zeros(B)
    # ---- growth: one launch, or day by day
    if path == "advance":
        eng.advance(N.TUMOR_RUN_GROWTH)
        twin.advance(N.TUMOR_RUN_GROWTH)
        outs = [None] * B
        for _ in range(T):
            part = [o.stage[0] == po.GROWTH for o in orcs.o]
            if not any(part):
                break
            new = orcs.step(zero, part)
            outs = [n if n is not None else o for n, o in zip(new, outs)]
        _tumor_compare(eng, orcs, outs, "growth run")
    else:
        for day in range(T):
            if all(o.stage[0] != po.GROWTH for o in orcs.o):
                break
            # every patient steps every day: those already in therapy receive a small dose
            c = np.where([o.stage[0] == po.THERAPY for o in orcs.o], 0.03, 0.0)
            outs = orcs.step(c)
            eng.step(c)
            twin.step(c)
            _tumor_compare(eng, orcs, outs, f"growth day {day + 1}")
    assert (_np(eng.t["stage"]) == po.THERAPY).all() and 15 < _np(eng.t["time_index"]).min()
    # ---- therapy, daily: first day finite, second day the plants, then the day on which the reference raises for 2 and 4
    rng = np.random.default_rng(9)
    for day in range(4):
        c = rng.uniform(0.02, 0.1, B)
        c_clean = c.copy()
        if day == 1:
            for b, v in TUMOR_DOSE.items():
                c[b] = v
            c_clean[3] = 2.0                    # min(want, remaining): more than what is left, like +Inf
        outs = orcs.step(c)
        eng.step(c)
        twin.step(c_clean)
        _tumor_compare(eng, orcs, outs, f"therapy day {day + 1}")
        for name in ("u", "reward", "terminated", "truncated", "stage", "days", "remaining", "out"):
            NF.same_bits_and_nans(eng.t[name][[0, 3]], twin.t[name][[0, 3]], f"therapy day {day + 1}: {name} of the clean instances")
        if day == 1:
            u, rem = _np(eng.t["u"]), _np(eng.t["remaining"])
            assert np.isnan(u[2]).any() and np.isnan(u[4]).any() and np.isnan(rem[2]) and rem[4] == np.inf and rem[3] == 0.0
        if day == 2:                           # what include/pdegym.h states for the input on which the reference raises
            assert isinstance(orcs.raised[2], ZeroDivisionError) and isinstance(orcs.raised[4], ZeroDivisionError)
            assert orcs.raised[0] is None and orcs.raised[1] is None and orcs.raised[3] is None
            r, out = _np(eng.t["reward"]), _np(eng.t["out"])
            assert np.isnan(r[[2, 4]]).all() and (out[[2, 4], 2] == 0.0).all() and np.isnan(out[[2, 4], 1]).all()      # out: T1, T2, treatment radius, dose
            assert (_np(eng.t["stage"])[[2, 4]] == po.THERAPY).all() and not _flags(eng.t["terminated"])[[2, 4]].any()
    assert np.isnan(_np(eng.t["u"])[1]).sum() > 40 and not np.isnan(_np(eng.t["u"])[[0, 3]]).any()
    # ---- post-therapy of instance 3 (the +Inf dosage used up what was left): one launch or day by day; the others stay in therapy
    assert int(_np(eng.t["stage"])[3]) == po.POST
    if path == "advance":
        eng.advance(N.TUMOR_RUN_POST)
        twin.advance(N.TUMOR_RUN_POST)
        outs = [None] * B
        for _ in range(T):
            o3 = orcs.o[3]
            if o3.time_index[0] >= o3.nt - 1 or (outs[3] is not None and (outs[3][2] or outs[3][3])):
                break
            outs[3] = orcs.step(zero, [False, False, False, True, False])[3]
        _tumor_compare(eng, orcs, outs, "post run")
        NF.same_bits_and_nans(eng.t["u"][[0, 3]], twin.t["u"][[0, 3]], "post run: rows of the clean instances")
        NF.same_bits_and_nans(eng.t["reward"][[0, 3]], twin.t["reward"][[0, 3]], "post run: reward of the clean instances")


# ---- pdegym_mlp_forward -------------------------------------------------------------------------------------------------------------
MLP_NETS = {"5-16-2": [5, 16, 2], "20-65-1": [20, 65, 1], "600-64-1": [600, 64, 1], "7-256-200-33-3": [7, 256, 200, 33, 3]}
MLP_B = 17                  # one full 16-row MFMA tile plus one row
MLP_NAN_ROWS, MLP_PINF_ROW, MLP_NINF_ROW = (3, 16), 5, 9


def _mlp_float64(mod, x32, noise, clamp, act):
    """The float64 NumPy evaluation of the same float32 parameters (tests/test_gpu_buffer_contract.py
    test_mlp_forward_contract_vs_float64), ending in np.clip; also the summed magnitudes its tolerance is built from."""
    h = x32.astype(f64)
    mag = np.abs(h)
    lins = [m for m in mod if isinstance(m, torch.nn.Linear)]
    with np.errstate(all="ignore"):
        for i, L in enumerate(lins):
            W, b = _np(L.weight).astype(f64), _np(L.bias).astype(f64)
            mag = mag @ np.abs(W).T + np.abs(b)
            h = h @ W.T + b
            if i < len(lins) - 1:
                if act == "tanh":
                    h, mag = np.tanh(h), np.ones_like(mag)
                elif act == "relu":
                    h = np.maximum(h, 0)
        if noise is not None:
            h = h + noise.astype(f64)
        if clamp is not None:
            h = np.clip(h, *clamp)
    return h, mag


@pytest.mark.parametrize("x_f64", [False, True], ids=["x32", "x64"])
@pytest.mark.parametrize("clamp,noisy", [(None, False), ((-1.5, 2.0), False), ((-1.5, 2.0), True), (None, True)],
                         ids=["plain", "clamp", "clamp+noise", "noise"])
@pytest.mark.parametrize("act", ["tanh", "relu", "identity"])
@pytest.mark.parametrize("net", sorted(MLP_NETS))
def test_mlp_forward_nonfinite_rows(net, act, clamp, noisy, x_f64):
    """Rows 3 and 16 carry a NaN (first and last column), row 5 +Inf, row 9 -Inf (float64 observations: +-1e300, which become
    infinities on the way in); the +Inf sits in column 599 of the 600-wide network (its second staging chunk).  Weights are positive
    from the first layer on (relu / identity) so that an infinity reaches the output as an infinity: clamped, it is exactly hi / lo."""
    from pdecontrolgym_amd.policy import FusedMLP
    sizes = MLP_NETS[net]
    K, out_dim, width = sizes[0], sizes[-1], max(sizes[1:])
    mod = _mlp(sizes, act, seed=K + width, positive_from=0)
    pol = FusedMLP(mod, clamp=clamp)
    rng = np.random.default_rng(K)
    x = rng.standard_normal((MLP_B, K))
    x = x.astype(f32).astype(f64) if x_f64 else x.astype(f32)
    clean = x.copy()
    big = 1e300 if x_f64 else np.inf
    x[3, 0], x[16, K - 1], x[MLP_PINF_ROW, 599 if K == 600 else 0], x[MLP_NINF_ROW, K - 1] = NAN, NAN, big, -big
    nz = (rng.standard_normal((MLP_B, out_dim)) * 0.1).astype(f32) if noisy else None
    ys = []
    for inp in (x, clean):
        y = torch.zeros(MLP_B, out_dim, dtype=torch.float32, device=DEV)
        pol.forward_into(torch.as_tensor(inp, device=DEV), y, noise=None if nz is None else torch.as_tensor(nz, device=DEV))
        ys.append(_np(y))
    got, got_clean = ys
    with np.errstate(over="ignore"):
        want, mag = _mlp_float64(mod, x.astype(f32), nz, clamp, act)
    planted = list(MLP_NAN_ROWS) + [MLP_PINF_ROW, MLP_NINF_ROW]
    others = NF.rows_except(MLP_B, planted)
    NF.nan_mask_equal(got, want, "NaN positions")
    assert np.array_equal(np.isposinf(got), np.isposinf(want)) and np.array_equal(np.isneginf(got), np.isneginf(want)), "Inf positions"
    assert np.isnan(want[list(MLP_NAN_ROWS)]).all() and np.isfinite(want[others]).all()
    if act in ("relu", "identity"):
        if clamp is None:
            assert np.isposinf(got[MLP_PINF_ROW]).all()
            assert np.isneginf(got[MLP_NINF_ROW]).all() if act == "identity" else np.isfinite(got[MLP_NINF_ROW]).all()
        else:
            assert (got[MLP_PINF_ROW] == f32(clamp[1])).all(), "a clamped +Inf is exactly hi"
            if act == "identity":
                assert (got[MLP_NINF_ROW] == f32(clamp[0])).all(), "a clamped -Inf is exactly lo"
    NF.same_bits_and_nans(got[others], got_clean[others], "rows that received no non-finite value")
    fin = np.isfinite(want)
    tol = 4 * 2.0 ** -24 * (K + 2 * width + 2) * (np.where(fin, mag, 0.0) + 1) + 1e-6      # the bound of the finite contract test
    with np.errstate(invalid="ignore"):
        err = np.abs(np.where(fin, got.astype(f64) - want, 0.0))
    assert (err <= tol).all(), f"vs float64: max err / tol {float((err / tol).max()):.3g}"


# ---- policy inside the 1D rollouts ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hidden", [16, 65], ids=["narrow", "wide"])
@pytest.mark.parametrize("kind,nx", [("parabolic", 31), ("transport", 64)])
def test_policy_inside_1d_rollout_keeps_a_nan_command(kind, nx, hidden):
    """S = 2, T = 3, B = 17 (one workgroup of 16 instances plus one).  Instance 5 starts with a NaN node: the command the policy
    computes inside the launch has to be NaN through the clamp (-1, 1), and the launch equals the two-launch path (pdegym_mlp_forward,
    then a step call), compared as tests/fuzz_policy_rollout.py does.  The other 16 instances are bit-identical to a clean run."""
    from pdecontrolgym_amd import _native as N
    from pdecontrolgym_amd.batch1d import PDEBatch1D, RewardSpec
    from pdecontrolgym_amd.policy import FusedMLP
    S, T, B, bad = 2, 3, 17, 5
    dx = 1.0 / nx
    dt = 0.25 * dx * dx if kind == "parabolic" else 0.5 * dx
    kw = dict(T=20 * S * dt, dt=dt, X=1, dx=dx, control_sample_rate=S * dt, control_type="Dirchilet", sensing_loc="full", sensing_type=None,
              normalize=True, max_control_value=20, limit_pde_state_size=True, max_state_value=1e10)
    n = nx + (kind == "parabolic")
    rng = np.random.default_rng(nx)
    xg = np.linspace(0, 1, n)
    init = (rng.uniform(0.5, 3, (B, 1)) * (1 + 0.3 * np.sin(2 * np.pi * xg * rng.uniform(0.5, 3, (B, 1))))).astype(f32)
    beta = rng.uniform(-2, 2, (B, n)).astype(f32)
    poisoned = init.copy()
    poisoned[bad, n // 2] = NAN

    def make(ic):
        e = PDEBatch1D(kind, reward=RewardSpec(N.REWARD_TUNED1D, 20 * S, -1e3, 3e2), num_envs=B, device=DEV, **kw)
        e.reset(torch.tensor(ic), torch.tensor(beta))
        return e
    od = make(init).obs_dim
    pol = FusedMLP(_mlp([od, hidden, 1], seed=hidden + nx), clamp=(-1.0, 1.0))
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=DEV)      # noqa: E731
    res = []
    for ic in (poisoned, init):
        e = make(ic)
        assert e.policy_fits_rollout(pol)
        obs, act, rew, te, tr = z(T + 1, B, od), z(T, B), z(T, B), z(T, B, dt=torch.uint8), z(T, B, dt=torch.uint8)
        obs[0].copy_(e.t["obs"].reshape(B, od))
        e.rollout(obs, act, rew, te, tr, policy=pol)
        res.append((obs, act, rew, te, tr))
    obs, act, rew, te, tr = res[0]
    a = _np(act)
    assert np.isnan(a[:, bad]).all(), f"the clamp dropped the NaN command: {a[:, bad]}"
    assert not np.isnan(np.delete(a, bad, axis=1)).any()
    assert all(np.isnan(_np(obs[t, bad])).any() for t in range(T + 1))
    # the two-launch path on the same engine code
    eb = make(poisoned)
    cur = eb.t["obs"].reshape(B, od).clone()
    a_buf = z(B)
    for t in range(T):
        pol.forward_into(cur.contiguous(), a_buf)
        if hidden > 64:
            NF.same_bits_and_nans(act[t], a_buf, f"step {t}: commands (wide: bit-identical)")
        else:
            scale = float(torch.nan_to_num(cur.abs(), nan=0.0, posinf=0.0).max().clamp(min=1.0))
            NF.close_and_same_nans(act[t], a_buf, rtol=1e-4, atol=2e-5 * scale, what=f"step {t}: commands")
            a_buf.copy_(act[t])
        o, r, te_b, tr_b = eb.step(a_buf)
        o = o.reshape(B, od)
        for name, x_, y_ in (("obs", o, obs[t + 1]), ("reward", r, rew[t]), ("terminated", te_b, te[t]), ("truncated", tr_b, tr[t])):
            NF.same_bits_and_nans(y_, x_, f"step {t}: {name} (one launch against two)")
        cur = o.clone()
    others = NF.rows_except(B, [bad])
    for name, x_, y_ in zip(("obs", "actions", "reward", "terminated", "truncated"), res[0], res[1]):
        NF.same_bits_and_nans(x_[:, others], y_[:, others], f"{name} of the clean instances")


# ---- pdegym_backstep_control --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ordered", [True, False], ids=["ordered", "tree"])
def test_backstep_control_keeps_nan_and_inf(ordered):
    """m = 65 (two elements per lane, ragged), B = 5: row 1 of the observations holds a NaN, row 3 a +Inf (positive gains there, so
    the law is +Inf).  out64 against the NumPy restatement of tests/test_backstepping.py; out32 = the double rounded once, plus
    noise, then np.clip -- which keeps the NaN."""
    from tests.test_gpu_backstepping import _control, _dev, _law_rows
    rng = np.random.default_rng(65)
    B, m, scale = 5, 65, 1e-2
    gain = rng.normal(0, 30, (B, m))
    gain[3] = np.abs(gain[3])
    obs = rng.uniform(-10, 10, (B, m)).astype(f32)
    clean = obs.copy()
    obs[1, 64], obs[3, 7] = NAN, PINF
    g = _dev(gain)
    with np.errstate(all="ignore"):
        want = _law_rows(gain, obs, m, scale)
    assert np.isnan(want[1]) and want[3] == np.inf and np.isfinite(want[[0, 2, 4]]).all()
    got, got_clean = _control(_dev(obs), g, m, scale, ordered), _control(_dev(clean), g, m, scale, ordered)
    if ordered:
        NF.same_bits_and_nans(got, want, "out64")
    else:                                       # two orders of the same products: the bound of test_control_law_orders
        bound = 2 * m * 2.0 ** -53 * np.abs(gain * clean.astype(f64)).sum(axis=1) * scale
        NF.nan_mask_equal(got, want, "out64")
        assert got[3] == np.inf and (np.abs(got[[0, 2, 4]] - want[[0, 2, 4]]) <= bound[[0, 2, 4]]).all()
    NF.same_bits_and_nans(got[[0, 2, 4]], got_clean[[0, 2, 4]], "out64 of the clean rows")
    nz = rng.normal(0, 0.5, B).astype(f32)
    lo, hi = -3.0, 2.5
    got32 = _control(_dev(obs), g, m, scale, ordered, torch.float32, noise=_dev(nz), clamp=(lo, hi))
    with np.errstate(all="ignore"):
        want32 = np.clip(got.astype(f32) + nz, f32(lo), f32(hi))
    NF.same_bits_and_nans(got32, want32, "out32 (noise, then the clamp)")
    assert np.isnan(got32[1]) and got32[3] == f32(hi)
    clean32 = _control(_dev(clean), g, m, scale, ordered, torch.float32, noise=_dev(nz), clamp=(lo, hi))
    NF.same_bits_and_nans(got32[[0, 2, 4]], clean32[[0, 2, 4]], "out32 of the clean rows")


# ---- NavierStokes2D -----------------------------------------------------------------------------------------------------------------
# A NaN front is an exact probe of a stencil's data dependence: the set of NaN cells after a step is fixed by which cells were read,
# not by rounding.  float64 engines: every output bit for bit against the oracle.  float32 engines: the NaN masks of u, v, p equal
# those of the float64 oracle run on the same float32-rounded inputs; the other cells keep the tolerances of tests/test_gpu_ns2d.py
# test_ns_f32_single_step_vs_f64_oracle (one step from identical state: velocity rtol 1e-5 atol 2e-6 max|U|, pressure rtol 1e-4 atol
# 5e-5 max|p|, reward rtol 1e-4).  float32 engines get NaN plants only (an infinity can meet a product that is exactly zero in one
# precision and tiny in the other); the +Inf node command runs on the float64 engines.
NS_BC1 = {"upper": ["Controllable", "Dirchilet"], "lower": ["Dirchilet", "Neumann"], "left": ["Neumann", "Dirchilet"],
          "right": ["Dirchilet", "Neumann"]}          # one Controllable edge: u on the upper row, node j of the command = column j


def _ns_dbg(**kv):
    from pdecontrolgym_amd import _native as N
    for k, v in kv.items():
        N.load().pdegym_debug_set(getattr(N, k), int(v))


NS_DISPATCH = {"default": {}, "column": dict(DEBUG_NS_COL_MIN_BATCH=0), "generic": dict(DEBUG_NS_GENERIC=1)}


def _ns_inputs(ny, nx, K, B, seed):
    rng = np.random.default_rng(seed)
    dx, dy = 1.0 / (nx - 1), 1.0 / (ny - 1)
    dt = 0.2 * 0.5 * min(dx, dy) ** 2 / 0.1
    nt = 6
    Xg, Yg = np.meshgrid(np.linspace(0, 1, nx), np.linspace(0, 1, ny))
    u0 = np.stack([np.sin(2 * np.pi * Xg * rng.uniform(0.5, 2)) * np.cos(np.pi * Yg) * rng.uniform(0.5, 2) + rng.uniform(-1, 1) for _ in range(B)])
    v0 = np.stack([np.cos(np.pi * Xg) * np.sin(2 * np.pi * Yg * rng.uniform(0.5, 2)) * rng.uniform(0.5, 2) + rng.uniform(-1, 1) for _ in range(B)])
    p0 = rng.uniform(-1, 1, (B, ny, nx))
    adim = nx if nx == ny else 1          # per-node commands need a square grid (as in the reference)
    kw = dict(T=nt * dt, dt=dt, X=1, dx=dx, Y=1, dy=dy, boundary_condition=NS_BC1, U_ref=rng.uniform(-1, 1, (nt, ny, nx, 2)),
              action_ref=rng.uniform(1, 3, nt), gamma=0.1, maximum_pressure_iteration=K)
    acts = rng.uniform(2, 4, (2, B, adim))
    f = lambda a: a.astype(f32).astype(f64)      # noqa: E731  (float32-representable: the same inputs for both precisions)
    return kw, adim, f(u0), f(v0), f(p0), f(acts)


def _ns_plant(fields, plants, f64_engine):
    """plants: (instance, what, where, value); what = "u" / "p" (cell of the initial field) or "a" (node of the first command, the
    whole command where it is a scalar).  Infinities are planted for float64 engines only.  Returns the poisoned instances."""
    u0, v0, p0, acts = (x.copy() for x in fields)
    hit = set()
    for inst, what, where, val in plants:
        if np.isinf(val) and not f64_engine:
            continue
        hit.add(inst)
        if what == "a":
            acts[0, inst, where if acts.shape[2] > 1 else 0] = val
        else:
            {"u": u0, "p": p0}[what][(inst,) + tuple(where)] = val
    return (u0, v0, p0, acts), sorted(hit)


def _ns_engine(kw, adim, B, dtype, inter, dispatch, fields, restart=None):
    """Two env-steps; ``restart`` (float32 comparison): states to start the second step from.  Returns per step (obs, p, reward, te)."""
    from pdecontrolgym_amd.batch2d import NSBatch2D
    u0, v0, p0, acts = fields
    outs = []
    _ns_dbg(**NS_DISPATCH[dispatch])
    try:
        env = NSBatch2D(num_envs=B, device=DEV, dtype=dtype, interleaved_state=inter, action_dim=adim, **kw)
        env.reset(u0, v0, p0)
        for i, a in enumerate(acts):
            if i and restart is not None:
                env.reset(*restart)
            obs, r, te = env.step(a)
            outs.append(tuple(_np(x).copy() for x in (obs, env.p, r, te)))
    finally:
        _ns_dbg(DEBUG_NS_COL_MIN_BATCH=-1, DEBUG_NS_GENERIC=0)
    return outs


def _ns_oracle(kw, fields, single_step):
    u0, v0, p0, acts = fields
    orc = po.NavierStokesOracle(**kw)
    orc.reset(u0, v0, p0)
    outs, restart = [], None
    with np.errstate(all="ignore"):
        for i, a in enumerate(acts):
            if i and single_step:          # both sides restart from the same float32-representable state
                restart = tuple(x.astype(f32).astype(f64) for x in (outs[-1][0][..., 0], outs[-1][0][..., 1], outs[-1][1]))
                orc.reset(*restart)
            o, r, te, _ = orc.step(a)
            outs.append((o, orc.p.copy(), r, te))
    return outs, restart


def _ns_check(ny, nx, K, B, plants, dtype, inter, dispatch, other=None, seed=0):
    """Parity with the oracle, isolation against a clean run of the same batch, and (``other``) equality with another kernel."""
    is64 = dtype == torch.float64
    kw, adim, *clean_fields = _ns_inputs(ny, nx, K, B, seed + 1000 * ny + nx)
    clean_fields = tuple(clean_fields)
    fields, hit = _ns_plant(clean_fields, plants, is64)
    clean_rows = NF.rows_except(B, hit)
    assert len(clean_rows) >= 2 and len(hit) >= 3
    want, restart = _ns_oracle(kw, fields, not is64)
    want_clean, restart_clean = _ns_oracle(kw, clean_fields, not is64)
    got = _ns_engine(kw, adim, B, dtype, inter, dispatch, fields, restart)
    got_clean = _ns_engine(kw, adim, B, dtype, inter, dispatch, clean_fields, restart_clean)
    for i, ((o, p, r, te), (o_ref, p_ref, r_ref, te_ref)) in enumerate(zip(got, want)):
        what = f"{ny}x{nx} K={K} {dispatch} step {i}"
        assert np.isnan(o_ref[hit]).any() and not np.isnan(o_ref[clean_rows]).any()
        if is64:
            NF.same_bits_and_nans(o, o_ref, what + ": obs")
            NF.same_bits_and_nans(p, p_ref, what + ": p")
            NF.close_and_same_nans(r, r_ref, rtol=1e-12, what=what + ": reward")
        else:
            NF.nan_mask_equal(o, o_ref, what + ": NaN mask of (u, v)")
            NF.nan_mask_equal(p, p_ref, what + ": NaN mask of p")
            NF.close_and_same_nans(o, o_ref, rtol=1e-5, atol=2e-6 * np.nanmax(np.abs(o_ref)), what=what + ": obs")
            NF.close_and_same_nans(p, p_ref, rtol=1e-4, atol=5e-5 * np.nanmax(np.abs(p_ref)), what=what + ": p")
            NF.close_and_same_nans(r, r_ref, rtol=1e-4, what=what + ": reward")
        assert np.array_equal(te.astype(bool), te_ref)
        for name, x, y in zip(("obs", "p", "reward"), got[i], got_clean[i]):
            NF.same_bits_and_nans(x[clean_rows], y[clean_rows], what + f": {name} of the clean instances")
    if other is not None:
        # the equalities the finite tests hold (tests/fuzz_more.py): column kernel == workgroup kernel in every output, rewards included
        # (one summation order); tile / 256 x 256 kernels == workgroup kernel in the fields (their reward sums run in another order)
        alt = _ns_engine(kw, adim, B, dtype, inter, other, fields, restart)
        names = ("obs", "p", "reward", "terminated") if dispatch == "column" else ("obs", "p", None, "terminated")
        for i in range(len(got)):
            for name, x, y in zip(names, got[i], alt[i]):
                if name is None:
                    NF.nan_mask_equal(x, y, f"{ny}x{nx} K={K} step {i}: NaN mask of the reward, {dispatch} kernel against {other} kernel")
                else:
                    NF.same_bits_and_nans(x, y, f"{ny}x{nx} K={K} step {i}: {name}, {dispatch} kernel against {other} kernel")


def _col_plants(ny, nx):
    """B = 7.  At nx = 21 three instances share a wave (lanes 0-20, 21-41, 42-62): instances 0-2, 3-5, 6; the clean instances 0, 2, 4
    sit next to poisoned ones in their wave.  At nx = 64 one instance fills the wave."""
    return [(1, "u", (1, 1), NAN),                          # next to the corner (0, 0)
            (1, "p", (ny - 2, nx - 2), NAN),                # next to the opposite corner
            (3, "u", (ny // 2, nx // 2), NAN),              # middle
            (3, "p", (ny // 2, nx // 2), NAN),
            (3, "a", nx // 3, PINF),                        # +Inf node command (float64 engines only)
            (5, "u", (ny // 2, nx - 1), NAN),               # last column: lane 63, the wave's last, at nx = 64; at nx = 21 the lane in front of
            (5, "p", (ny // 2 - 1, 0), NAN),                # ... the next instance's first one -- and the first column, its counterpart
            (6, "a", (2 * nx) // 3, NAN)]                   # NaN node command on the Controllable edge


@pytest.mark.parametrize("K", [1, 3, 7])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("nx", [21, 64])
@pytest.mark.parametrize("ny", [8, 21, 32])
def test_ns_column_kernel(ny, nx, dtype, K):
    """ns_col_step (DEBUG_NS_COL_MIN_BATCH 0), and column kernel == workgroup kernel on the planted inputs."""
    _ns_check(ny, nx, K, 7, _col_plants(ny, nx), dtype, True, "column", other="generic")


@pytest.mark.parametrize("K", [0, 1, 3, 7])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("ny,nx", [(33, 40), (21, 21)])
def test_ns_workgroup_kernel(ny, nx, dtype, K):
    """ns_generic_step: 1320 cells on 1024 threads (two cells per thread, ragged) and the reference's 21 x 21."""
    plants = [(1, "u", (1, 1), NAN), (1, "p", (ny - 2, nx - 2), NAN),                 # next to two corners
              (3, "u", (ny // 2, nx // 2), NAN), (3, "p", (ny // 2 + 1, nx // 2), NAN),      # middle
              (3, "a", nx // 3, PINF),
              (4, "a", nx // 2, NAN), (4, "u", (ny - 2, 1), NAN)]
    _ns_check(ny, nx, K, 5, plants, dtype, K % 2 == 1, "generic")


def _tile_plants(n, PR):
    """B = 6; PR = rows of a thread's patch (float32: 4 at 64 x 64, 8 at 128 x 128, two columns / four columns per lane; float64 at
    128 x 128: 16 rows per wave, two columns per lane).  Row n/2 is the first row of a thread patch AND of a wave in each of them (the
    row above travels through the LDS halo), column n/2 the first column of a lane (the column to its left arrives by a DPP shift)."""
    h = n // 2
    return [(1, "u", (1, 1), NAN), (1, "p", (n - 2, n - 2), NAN),      # next to two corners
            (3, "u", (h - 1, h - 1), NAN),                             # last row of a wave / last column of a lane ...
            (3, "p", (h, h), NAN),                                     # ... and the first row / column of the next
            (3, "a", n // 4, PINF),
            (4, "u", (PR - 1, n - 1), NAN),                            # thread rows 0 | 1 of the first wave; lane 31 (right domain edge) ...
            (4, "p", (PR, 0), NAN),                                    # ... next to lane 32 (left domain edge of the next thread row)
            (5, "u", (n // 4 + 1, 3 * n // 4 + 1), NAN),               # inside a patch, away from every seam
            (5, "a", h, NAN)]                                          # NaN node command


@pytest.mark.parametrize("K", [1, 3, 7])
@pytest.mark.parametrize("inter", [True, False], ids=["interleaved", "separate"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("n", [64, 128])
def test_ns_tile_kernels(n, dtype, inter, K):
    """ns_tile_step<4, 2> / <8, 4> (float32) and ns_tile_step_f64 (128 x 128; float64 at 64 x 64 runs the workgroup kernel), and tile
    kernel == workgroup kernel on the planted inputs."""
    PR = 16 if dtype == torch.float64 and n == 128 else n // 16
    _ns_check(n, n, K, 6, _tile_plants(n, PR), dtype, inter, "default", other="generic")


NS256_PLANTS = [
    (1, "u", (1, 1), NAN), (1, "p", (254, 254), NAN),      # next to two corners
    (3, "u", (93, 127), NAN),       # float64 slabs: rows 93 | 94 = ownership boundary of slabs 0 | 1 (kOwn); columns 127 | 128 = lanes 31 | 32
    (3, "p", (94, 128), NAN),       #   (four columns per lane in both 256 x 256 kernels)
    (3, "a", 64, PINF),
    (4, "u", (161, 3), NAN),        # rows 161 | 162: ownership boundary of slabs 1 | 2; columns 3 | 4: lanes 0 | 1
    (4, "p", (162, 4), NAN),
    (4, "a", 128, NAN),             # NaN node command
    (5, "u", (31, 200), NAN),       # fused float32 launch: rows 31 | 32 = waves 0 | 1 (32 rows per wave)
    (5, "p", (32, 201), NAN),
    (5, "u", (67, 60), NAN),        # float64: row 68 = first row of slab 1 (kLo); rows 63 | 64: workgroups of the front kernel (4 bands of 16)
    (5, "p", (64, 255), NAN),
    (5, "p", (15, 10), NAN),        # float64: rows 14 | 15 = waves 0 | 1 of slab 0 (15 rows per wave); rows 15 | 16: front-kernel bands
    (5, "u", (14, 11), NAN)]


@pytest.mark.parametrize("K", [3, 17, 18, 35])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_ns_256(dtype, K):
    """The fused float32 launch and the float64 slab passes (25 sweeps per pass: K = 35 takes two), against the workgroup kernel too."""
    _ns_check(256, 256, K, 6, NS256_PLANTS, dtype, True, "default", other="generic")


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_ns_rollout_equals_step_calls_on_planted_inputs(dtype):
    """pdegym_ns2d_rollout_* at 21 x 21, T = 3, K = 3: bit-identical to three step calls; float64 also to the oracle."""
    from pdecontrolgym_amd.batch2d import NSBatch2D
    ny = nx = 21
    B, T = 7, 3
    kw, adim, *clean = _ns_inputs(ny, nx, 3, B, 77)
    (u0, v0, p0, acts2), hit = _ns_plant(tuple(clean), _col_plants(ny, nx), dtype == torch.float64)
    acts = np.concatenate([acts2, acts2[:1] * 0.5])
    acts[2] = np.nan_to_num(acts[2], nan=1.5, posinf=1.5)
    res = []
    for mode in ("rollout", "steps"):
        env = NSBatch2D(num_envs=B, device=DEV, dtype=dtype, interleaved_state=True, action_dim=adim, **kw)
        env.reset(u0, v0, p0)
        obs = torch.zeros(T + 1, B, ny, nx, 2, dtype=dtype, device=DEV)
        rew, te = torch.zeros(T, B, dtype=dtype, device=DEV), torch.zeros(T, B, dtype=torch.uint8, device=DEV)
        a = torch.as_tensor(acts, dtype=dtype, device=DEV)
        if mode == "rollout":
            assert env.can_rollout()
            obs[0].copy_(env.t["obs"])
            env.rollout(obs, a, rew, te)
        else:
            for t in range(T):
                o, r, e = env.step(a[t])
                obs[t + 1].copy_(o)
                rew[t].copy_(r)
                te[t].copy_(e)
        res.append((obs[1:], rew, te, env.p.clone()))
    for name, x, y in zip(("obs", "reward", "terminated", "p"), *res):
        NF.same_bits_and_nans(x, y, f"rollout against step calls: {name}")
    assert np.isnan(_np(res[0][0])[:, hit]).any() and not np.isnan(_np(res[0][0])[:, NF.rows_except(B, hit)]).any()
    if dtype == torch.float64:
        orc = po.NavierStokesOracle(**kw)
        orc.reset(u0, v0, p0)
        with np.errstate(all="ignore"):
            for t in range(T):
                o_ref, r_ref, te_ref, _ = orc.step(acts[t])
                NF.same_bits_and_nans(res[0][0][t], o_ref, f"rollout step {t}: obs")
                NF.close_and_same_nans(res[0][1][t], r_ref, rtol=1e-12, what=f"rollout step {t}: reward")
        NF.same_bits_and_nans(res[0][3], orc.p, "rollout: p")


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("n,K", [(21, 3), (64, 7), (128, 7)])
def test_ns_solve_pressure_with_a_nan_cell(n, K, dtype):
    """pdegym_ns2d_solve_pressure_*: a NaN cell in p_in (instance 1: next to a corner, instance 3: the tile seam n/2), clean instances
    in between."""
    from pdecontrolgym_amd.batch2d import NSBatch2D
    B = 5
    kw, adim, u0, v0, p0, _ = _ns_inputs(n, n, K, B, 5)
    clean_p = p0.copy()
    p0[1, 1, 1], p0[3, n // 2, n // 2 - 1] = NAN, NAN
    env = NSBatch2D(num_envs=B, device=DEV, dtype=dtype, action_dim=adim, **kw)
    orc = po.NavierStokesOracle(**kw)
    dev = lambda a: torch.as_tensor(a, dtype=dtype, device=DEV)      # noqa: E731
    got, got_clean = _np(env.solve_pressure(dev(u0), dev(v0), dev(p0))), _np(env.solve_pressure(dev(u0), dev(v0), dev(clean_p)))
    with np.errstate(all="ignore"):
        want = orc.solve_pressure(u0, v0, p0)
    assert np.isnan(want[[1, 3]]).any() and not np.isnan(want[[0, 2, 4]]).any()
    if dtype == torch.float64:
        NF.same_bits_and_nans(got, want, "p_out")
    else:
        NF.nan_mask_equal(got, want, "NaN mask of p_out")
        NF.close_and_same_nans(got, want, rtol=1e-4, atol=5e-5 * np.nanmax(np.abs(want)), what="p_out")
    NF.same_bits_and_nans(got[[0, 2, 4]], got_clean[[0, 2, 4]], "p_out of the clean instances")
