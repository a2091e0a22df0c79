"""Pin the NumPy oracle (oracle/pde_oracle.py) to the reference over the parameter ranges the differential fuzzers draw.

tests/golden/sweep_*.npz (tests/golden/make_golden.py gen_sweep_*) hold reference-generated cases away from the configurations
of the other fixtures: every case stores its own constructor parameters, so nothing here mirrors a table.  Bars are the ones
tests/test_oracle_golden.py and tests/test_tumor.py use for the same family: 1D rows / observations bit-exact, rewards rtol 1e-6
with the same atol rule; NS fields and pressure bit-exact, reward rtol 1e-12; traffic and tumour exact.

test_sweep_discriminates_every_parameter proves each swept dimension can fail: with that parameter put back to the value of the
older fixtures (or dx and dy exchanged) at least one case stops reproducing its fixture.
"""
import numpy as np
import pytest

from oracle import pde_oracle as po
from tests.cases import ACTION_KIND, ns_bc_from_array
from tests.conftest import load_golden

SWEEP_1D, SWEEP_NS, SWEEP_TRAFFIC, SWEEP_TUMOR = (load_golden("sweep_" + k) for k in ("1d", "ns", "traffic", "tumor"))
UNPINNABLE = {}
for _g in (SWEEP_1D, SWEEP_NS, SWEEP_TRAFFIC, SWEEP_TUMOR):
    UNPINNABLE.update(_g.pop("unpinnable", {}))


# ---- 1D -----------------------------------------------------------------------------------------------------------------------
def kw_1d(g, **over):
    """Constructor arguments of a sweep_1d case (sensing_type "" = None)."""
    kw = dict(T=float(g.T), dt=float(g.dt), X=float(g.X), dx=float(g.dx), control_sample_rate=float(g.control_sample_rate),
              control_type=str(g.control_type), sensing_loc=str(g.sensing_loc), sensing_type=str(g.sensing_type) or None,
              normalize=bool(g.normalize), max_control_value=float(g.max_control_value),
              limit_pde_state_size=bool(g.limit_pde_state_size), max_state_value=float(g.max_state_value))
    kw.update(over)
    return kw


def run_1d(g, keep_history=False, **over):
    rw = po.TunedReward1DOracle(int(g.reward_args[0]), g.reward_args[1], g.reward_args[2])
    cls = po.ParabolicOracle if str(g.kind) == "parabolic" else po.TransportOracle
    env = cls(reward=rw, keep_history=keep_history, **kw_1d(g, **over))
    assert env.n == g.init.shape[0]
    obs0 = env.reset(g.init[None, :], g.beta[None, :])
    np.testing.assert_array_equal(np.asarray(obs0, dtype=np.float32).reshape(-1), g.obs0)
    keep = {int(k): j for j, k in enumerate(g.keep)}
    for i, a in enumerate(g.actions):
        with np.errstate(all="ignore"):
            obs, r, te, tr = env.step(np.array([a], dtype=g.actions.dtype), action_kind=ACTION_KIND[str(g.action_as)])
        if i in keep:
            np.testing.assert_array_equal(env.row[0], g.rows[keep[i]], err_msg=f"row step {i}")
            np.testing.assert_array_equal(np.asarray(obs, dtype=np.float32).reshape(-1), g.obs[keep[i]], err_msg=f"obs step {i}")
        assert int(env.time_index[0]) == int(g.time_index[i])
        assert bool(te[0]) == bool(g.terminate[i]) and bool(tr[0]) == bool(g.truncate[i]), f"flags step {i}"
        if np.isfinite(g.reward[i]):
            np.testing.assert_allclose(r[0], g.reward[i], rtol=1e-6, atol=1e-6 * max(1.0, abs(float(env.norm_now[0]))),
                                       err_msg=f"reward step {i}")
        else:
            assert not np.isfinite(r[0])


@pytest.mark.parametrize("case", sorted(SWEEP_1D))
def test_1d_oracle_matches_reference_sweep(case):
    g = SWEEP_1D[case]
    run_1d(g)
    if g.init.shape[0] <= 256:              # the history form of the reward on the small rows (a [nt, n] array per case)
        run_1d(g, keep_history=True)


def test_1d_sweep_covers_the_kernel_row_classes():
    """One case per row width the step kernels dispatch on, both environments: the widths of tests/test_gpu_buffer_contract.py
    (STEP_CASES, test_1d_full_rows, test_1d_m64_contract, test_1d_wide_kernels), and the other dimensions the issue lists."""
    from tests.test_gpu_buffer_contract import STEP_CASES, _ragged_slots
    have = {(str(g.kind), int(g.init.shape[0])) for g in SWEEP_1D.values()}
    want = {(k, n) for k, n, _ in STEP_CASES} | {(k, s + (k == "parabolic")) for k in ("transport", "parabolic") for s in (64, 128, 256, 512)}
    want |= {("transport", 2049), ("parabolic", 2049)}
    assert want <= have, sorted(want - have)
    m64 = {int(g.init.shape[0]) for g in SWEEP_1D.values() if g.beta.dtype == np.float64 or str(g.action_as) != "f32arr"}
    assert m64 == {_ragged_slots(e) + 1 for e in (1, 2, 4, 8)}
    for kind in ("transport", "parabolic"):
        gs = [g for g in SWEEP_1D.values() if str(g.kind) == kind]
        assert {float(g.X) for g in gs} == {0.5, 1.0, 2.0}
        assert {(float(g.max_control_value), bool(g.normalize)) for g in gs} >= {(m, n) for m in (1.0, 3.0, 20.0) for n in (False, True)}
        assert {int(round(float(g.control_sample_rate) / float(g.dt))) for g in gs} == {1, 2, 7, 33, 100}
        combos = {(str(g.control_type), str(g.sensing_loc), str(g.sensing_type)) for g in gs}
        assert len(combos) == (8 if kind == "transport" else 6)
        assert any(g.truncate.any() and not g.truncate.all() for g in gs) and any(not bool(g.limit_pde_state_size) for g in gs)
        assert all(int(round(float(g.T) / float(g.dt))) + 1 >= 120 for g in gs)
        # an episode whose last step is clipped: fewer sub-steps than S, and it terminates
        clipped = lambda g: 0 < np.diff(np.concatenate([[0], g.time_index]))[np.argmax(g.terminate)] < \
            int(round(float(g.control_sample_rate) / float(g.dt)))                                   # noqa: E731
        assert any(g.terminate.any() and clipped(g) for g in gs)
        assert any(g.terminate[:-1].any() for g in gs)               # and a call after the end of the episode


# ---- Navier-Stokes ------------------------------------------------------------------------------------------------------------
def kw_ns(g, **over):
    kw = dict(T=float(g.T), dt=float(g.dt), X=float(g.X), dx=float(g.dx), Y=float(g.Y), dy=float(g.dy),
              boundary_condition=ns_bc_from_array(g.bc), U_ref=g.U_ref, action_ref=g.action_ref, gamma=float(g.gamma),
              viscosity=float(g.viscosity), density=float(g.density), maximum_pressure_iteration=int(g.maximum_pressure_iteration))
    kw.update(over)
    return kw


def run_ns(g, **over):
    env = po.NavierStokesOracle(**kw_ns(g, **over))
    assert env.nx == env.ny == int(g.n) and env.nt == int(g.nt)
    env.reset(g.u0[None], g.v0[None], g.p0[None])
    for i, a in enumerate(g.actions):
        obs, r, te, tr = env.step(a[None])
        np.testing.assert_array_equal(obs[0], g.obs[i], err_msg=f"obs step {i}")
        np.testing.assert_array_equal(env.p[0], g.p[i], err_msg=f"p step {i}")
        np.testing.assert_allclose(r[0], g.rewards[i], rtol=1e-12, err_msg=f"reward step {i}")
        assert bool(te[0]) == bool(g.terminate[i])


@pytest.mark.parametrize("case", sorted(SWEEP_NS))
def test_ns_oracle_matches_reference_sweep(case):
    run_ns(SWEEP_NS[case])


def test_ns_sweep_coverage():
    gs = list(SWEEP_NS.values())
    assert {int(g.n) for g in gs} == {5, 8, 16, 21, 33} and {float(g.Y) for g in gs} == {0.25, 0.5, 1.0, 2.0}
    assert {float(g.density) for g in gs} == {0.5, 1.0, 2.0} and {float(g.viscosity) for g in gs} == {0.01, 0.1, 1.0}
    assert {float(g.gamma) for g in gs} == {0.0, 0.1, 2.0} and {int(g.maximum_pressure_iteration) for g in gs} == {0, 1, 2, 3, 7, 51}
    assert {int(g.action_dim) == 1 for g in gs} == {True, False} and {str(g.ic) for g in gs} == {"zero", "const", "rand"}
    triples = {(e, c, str(g.bc[2 * e + c])) for g in gs for e in range(4) for c in range(2)}
    assert len(triples) == 24
    assert all(g.obs.shape[0] == 3 for g in gs)


# ---- traffic ------------------------------------------------------------------------------------------------------------------
def traffic_oracle(g, **over):
    kw = dict(T=float(g.T), dt=float(g.dt), X=float(g.X), dx=float(g.dx), simulation_type=str(g.sim), v_max=float(g.v_max),
              ro_max=float(g.ro_max), tau=float(g.tau), limit_pde_state_size=bool(g.limit), control_freq=int(g.control_freq))
    kw.update(over)
    return po.TrafficOracle(**kw)


def run_traffic(g, **over):
    """float64, bit-exact observations / rewards / flags / time against the reference's own TrafficPDE1D."""
    orc = traffic_oracle(g, **over)
    o = orc.reset([float(g.rs)], [float(g.qs_clip)])
    np.testing.assert_array_equal(o[0], g.obs[0])
    for k, a in enumerate(g.actions):
        with np.errstate(all="ignore"):
            o, r, d, t = orc.step(a[None])
        np.testing.assert_array_equal(o[0], g.obs[k + 1], err_msg=f"step {k}")
        assert r[0] == g.reward[k] and bool(d[0]) == bool(g.done[k]) and bool(t[0]) == bool(g.trunc[k]), f"step {k}"
        assert orc.time_index[0] == g.time[k]


@pytest.mark.parametrize("case", sorted(SWEEP_TRAFFIC))
def test_traffic_oracle_matches_reference_sweep(case):
    run_traffic(SWEEP_TRAFFIC[case])


def test_traffic_sweep_coverage():
    gs = list(SWEEP_TRAFFIC.values())
    assert {str(g.sim) for g in gs} == {"inlet", "outlet", "both", "outlet-train"}
    for key in ("tau", "v_max", "ro_max", "ro_steady"):
        assert len({float(g[key]) for g in gs}) >= 2, key
    assert {int(g.control_freq) for g in gs} == {1, 2, 3, 5} and {bool(g.limit) for g in gs} == {True, False}
    assert {float(g.dx) for g in gs} == {0.5, 5.0, 8.0, 12.5} and {float(g.X) for g in gs} == {250.0, 400.0, 500.0}
    short = [g for g in gs if float(g.T) in (2.0, 5.0)]
    assert short and all((g.time >= float(g.T)).any() and (np.diff(g.time) < 0).any() for g in short)     # freeze, then T/dt
    assert any(g.trunc.any() and bool(g.limit) for g in gs)
    vs = lambda g: float(g.v_max) * (1 - float(g.rs) / float(g.ro_max))          # noqa: E731
    assert any(str(g.sim) == "outlet-train" and float(g.qs_clip) != float(g.rs) * vs(g) for g in gs)


# ---- tumour -------------------------------------------------------------------------------------------------------------------
TUMOR_ARGS = ("t1_detection_threshold", "t2_detection_threshold", "dosage_termination_threshold", "D", "rho", "alpha",
              "alpha_beta_ratio", "k", "t1_detection_radius", "t1_death_radius")


def tumor_oracle(g, **over):
    kw = {k: float(g[k]) for k in TUMOR_ARGS}
    kw.update(over)
    # .item(): an integer dx stays an int, as the generator passed it (the type decides how the reward's power is evaluated)
    return po.BrainTumorOracle(g.T.item(), g.dt.item(), g.X.item(), g.dx.item(), float(g.total_dosage), **kw)


def run_tumor(g, **over):
    """The bars of tests/test_tumor.py::test_oracle_matches_reference: everything exact."""
    orc = tumor_oracle(g, **over)
    rows = {0: orc.reset(g.init[None], [float(g.t_benchmark)])[0]}
    for n, a in enumerate(g.actions):
        o, r, te, tr = orc.step([a])
        rows[n + 1] = o[0]
        assert r[0] == g.reward[n], (n, r[0], g.reward[n])
        assert bool(te[0]) == bool(g.term[n]) and bool(tr[0]) == bool(g.trunc[n]) and orc.stage[0] == g.stage[n], n
        t1 = orc.T1[0]
        assert (np.isnan(t1) and np.isnan(g.t1_idx[n + 1])) or t1 / float(g.dx) == g.t1_idx[n + 1], n
        assert orc.applied[0] == g.dosage[n + 1], n
    for i, k in enumerate(g.keep):
        np.testing.assert_array_equal(rows[int(k)], g.rows[i], err_msg=f"row {k}")
    days = [orc.growthDays[0], orc.therapyDays[0], orc.postDays[0], orc.simulationDays[0], orc.cDeathDay[0]]
    np.testing.assert_array_equal(days, g.days)
    assert orc.remaining[0] == float(g.remaining)


@pytest.mark.parametrize("case", sorted(SWEEP_TUMOR))
def test_tumor_oracle_matches_reference_sweep(case):
    run_tumor(SWEEP_TUMOR[case])


def test_tumor_sweep_coverage():
    gs = list(SWEEP_TUMOR.values())
    assert len(gs) >= 6 and {float(g.dx) for g in gs} == {0.5, 1.0, 2.0} and {float(g.k) for g in gs} == {1.0, 3e4, 1e5}
    for key in TUMOR_ARGS + ("X", "total_dosage"):
        assert len({float(g[key]) for g in gs}) >= 2, key
    ends = {(int(g.stage[-1]), bool(g.term[-1]), bool(g.trunc[-1])) for g in gs}
    assert ends >= {(po.POST, False, True), (po.THERAPY, True, False), (po.POST, True, False)}
    assert any(np.isnan(float(g.t_benchmark)) for g in gs)
    assert all(len(g.keep) < len(g.actions) // 8 for g in gs)


# ---- what the reference cannot run ----------------------------------------------------------------------------------------------
def test_unpinnable_configurations_are_recorded():
    """Non-square NS grids and parabolic opposite / Dirichlet sensing raise in the reference (the generator asserts they still do):
    what this project computes there (the former) is pinned only to its own restatement."""
    names = {k for k in UNPINNABLE if "/" not in k}
    assert names == {"ns_non_square", "parabolic_opposite_dirichlet_dirchilet", "parabolic_opposite_dirichlet_neumann"}
    assert str(UNPINNABLE["ns_non_square"]) == "ValueError"
    assert str(UNPINNABLE["parabolic_opposite_dirichlet_dirchilet"]) == "Exception"
    for ct in ("Dirchilet", "Neumann"):                  # the oracle rejects it the same way
        with pytest.raises(Exception, match="not viable"):
            po.ParabolicOracle(1e-3, 1e-5, 1, 1e-2, 1e-4, control_type=ct, sensing_loc="opposite", sensing_type="Dirchilet")


# ---- every swept dimension can fail ---------------------------------------------------------------------------------------------
def _fails(run, g, **over):
    try:
        with np.errstate(all="ignore"):
            run(g, **over)
    except (AssertionError, ZeroDivisionError, RuntimeError):
        return True
    return False


def _swap_dx_dy(g):
    return dict(dx=float(g.dy), dy=float(g.dx), X=float(g.Y), Y=float(g.X))


DISCRIMINATE = [
    # family, runner, cases, parameter, value of the older fixtures (callable: from the case)
    ("1d", run_1d, SWEEP_1D, "max_control_value", 20.0), ("1d", run_1d, SWEEP_1D, "X", 1.0),
    ("1d", run_1d, SWEEP_1D, "max_state_value", 1e10), ("1d", run_1d, SWEEP_1D, "limit_pde_state_size", True),
    ("ns", run_ns, SWEEP_NS, "density", 1.0), ("ns", run_ns, SWEEP_NS, "viscosity", 0.1), ("ns", run_ns, SWEEP_NS, "gamma", 0.1),
    ("ns", run_ns, SWEEP_NS, "dy", lambda g: dict(dy=float(g.dx), Y=float(g.X))), ("ns", run_ns, SWEEP_NS, "dx<->dy", _swap_dx_dy),
    ("ns", run_ns, SWEEP_NS, "maximum_pressure_iteration", 50),
    ("traffic", run_traffic, SWEEP_TRAFFIC, "tau", 60.0), ("traffic", run_traffic, SWEEP_TRAFFIC, "v_max", 40.0),
    ("traffic", run_traffic, SWEEP_TRAFFIC, "ro_max", 0.16), ("traffic", run_traffic, SWEEP_TRAFFIC, "dx", 10.0),
    ("traffic", run_traffic, SWEEP_TRAFFIC, "dt", 0.25), ("traffic", run_traffic, SWEEP_TRAFFIC, "T", 240.0),
    ("traffic", run_traffic, SWEEP_TRAFFIC, "control_freq", 1), ("traffic", run_traffic, SWEEP_TRAFFIC, "limit_pde_state_size", True),
    ("tumor", run_tumor, SWEEP_TUMOR, "D", 0.2), ("tumor", run_tumor, SWEEP_TUMOR, "rho", 0.03), ("tumor", run_tumor, SWEEP_TUMOR, "alpha", 0.04),
    ("tumor", run_tumor, SWEEP_TUMOR, "alpha_beta_ratio", 10.0), ("tumor", run_tumor, SWEEP_TUMOR, "k", 1e5),
    ("tumor", run_tumor, SWEEP_TUMOR, "t1_detection_threshold", 0.8), ("tumor", run_tumor, SWEEP_TUMOR, "t2_detection_threshold", 0.16),
    ("tumor", run_tumor, SWEEP_TUMOR, "dosage_termination_threshold", 0.1), ("tumor", run_tumor, SWEEP_TUMOR, "t1_detection_radius", 15.0),
    ("tumor", run_tumor, SWEEP_TUMOR, "t1_death_radius", 35.0),
]


@pytest.mark.parametrize("family,run,cases,param,default", DISCRIMINATE, ids=[f"{d[0]}-{d[3]}" for d in DISCRIMINATE])
def test_sweep_discriminates_every_parameter(family, run, cases, param, default):
    """With ``param`` put back to the value every older fixture uses, at least one case no longer reproduces its fixture (the
    cases that already hold that value are left out: they would pass unchanged)."""
    tried = failed = 0
    for name, g in cases.items():
        over = default(g) if callable(default) else {param: default}
        if not callable(default):
            key = {"limit_pde_state_size": "limit"}.get(param, param) if family == "traffic" else param
            cur = g[key]
            if (float(cur) if cur.dtype != np.bool_ else bool(cur)) == default:
                continue
        elif all(over[k] == float(g[k]) for k in over):
            continue
        if family == "1d" and param == "X":          # the same node count on another length: dx and dt follow as in the generator
            nx = int(round(float(g.X) / float(g.dx)))
            over = dict(X=1.0, dx=1.0 / nx)
        if family == "traffic" and param == "dx":    # the same node count (and x / X profile) on the older fixtures' spacing
            over = dict(dx=default, X=default * (g.obs.shape[1] // 2 - 1))
        tried += 1
        failed += _fails(run, g, **over)
    assert tried >= 1 and failed >= 1, (param, tried, failed)
    if param in ("tau", "v_max", "ro_max", "D", "rho", "alpha", "k"):
        assert failed == tried, (param, tried, failed)          # these enter the arithmetic of every step


def test_tumor_single_environment_keeps_the_integer_radius_on_test_double():
    """c_term_post passes dx=1 as an int, like the shipped notebook: the reference's treatment radius is then a NumPy integer and
    its toxicity reward goes through NumPy's integer power.  The drop-in class hands the reward the same type: rewards exact."""
    from pde_control_gym.src import BrainTumor1D, BrainTumorReward
    from tests.fake_backend import FakeBackend
    g = SWEEP_TUMOR["c_term_post"]
    assert isinstance(g.dx.item(), int)
    seen = []

    class Spy(BrainTumorReward):
        def reward(self, **kw):
            if kw.get("treatment_radius"):
                seen.append(type(kw["treatment_radius"]))
            return super().reward(**kw)

    env = BrainTumor1D(T=g.T.item(), dt=g.dt.item(), X=g.X.item(), dx=g.dx.item(), normalize=True, reward_class=Spy(),
                       reset_init_condition_func=lambda X, nx: g.init, total_dosage=float(g.total_dosage), verbose=False,
                       device="cpu", backend=FakeBackend(), **{k: g[k].item() for k in TUMOR_ARGS})
    env.t_benchmark = int(g.t_benchmark)
    env.reset()
    for n, a in enumerate(g.actions):
        obs, r, te, tr, info = env.step(a)
        assert r == g.reward[n] and te == bool(g.term[n]) and tr == bool(g.trunc[n]), (n, r, g.reward[n])
    assert seen and all(issubclass(t, np.integer) for t in seen)
