"""The HIP engines against the reference-generated parameter sweep (tests/golden/sweep_*.npz), without the oracle in between.

Every case runs as instance 1 of a batch of three; instances 0 and 2 are the same configuration started from a scaled initial
state, so the case does not sit at offset 0.  Bars are those of the existing golden tests of each family:
  1D       rows / observations bit-exact, flags and time index equal, rewards rtol 1e-6 and atol 2e-6 * max(1, ||row||)
           (tests/test_gpu_1d.py); float64 beta and float64 / Python-float controls select the mixed-precision kernels;
  NS       float64 fields and pressure bit-exact, reward rtol 1e-12 (tests/test_gpu_ns2d.py), at the default dispatch and, where
           the column-per-lane kernel exists for the shape, with it forced and with it disabled;
  traffic  observations bit-exact, reward rtol 1e-13, flags and clock equal (tests/test_traffic.py);
  tumour   with the kill fraction evaluated on the host (as the single environment does): rows, doses, radii, stages, day
           counters, flags exact; with the in-kernel exp: rows rtol 1e-12; the in-kernel reward rtol 1e-12 either way
           (tests/test_tumor.py).
This module reads tests/golden/ only.
"""
import numpy as np
import pytest

from tests.cases import ACTION_KIND, ns_bc_from_array
from tests.conftest import load_golden

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SWEEP_1D, SWEEP_NS, SWEEP_TRAFFIC, SWEEP_TUMOR = (load_golden("sweep_" + k) for k in ("1d", "ns", "traffic", "tumor"))
for _g in (SWEEP_1D, SWEEP_NS, SWEEP_TRAFFIC, SWEEP_TUMOR):
    _g.pop("unpinnable", None)
B, ROW = 3, 1
SCALE = np.array([0.5, 1.0, 2.0])


# ---- 1D -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(SWEEP_1D))
def test_1d_hip_matches_reference_sweep(case):
    from pdecontrolgym_amd import _native as N
    from pdecontrolgym_amd.batch1d import PDEBatch1D, RewardSpec
    g = SWEEP_1D[case]
    spec = RewardSpec(N.REWARD_TUNED1D, int(g.reward_args[0]), float(g.reward_args[1]), float(g.reward_args[2]))
    env = PDEBatch1D(str(g.kind), float(g.T), float(g.dt), float(g.X), float(g.dx), float(g.control_sample_rate),
                     control_type=str(g.control_type), sensing_loc=str(g.sensing_loc), sensing_type=str(g.sensing_type) or None,
                     normalize=bool(g.normalize), max_control_value=float(g.max_control_value),
                     limit_pde_state_size=bool(g.limit_pde_state_size), max_state_value=float(g.max_state_value),
                     reward=spec, num_envs=B, device="cuda")
    assert env.n == g.init.shape[0]
    init = torch.tensor((g.init.astype(np.float32)[None] * SCALE[:, None].astype(np.float32)))
    beta = torch.tensor(np.tile(g.beta[None], (B, 1)))              # dtype preserved: float64 beta selects the mixed-precision mode
    obs = env.reset(init, beta)
    assert env.params.beta_f64 == (1 if g.beta.dtype == np.float64 else 0)
    np.testing.assert_array_equal(obs.cpu().numpy()[ROW].reshape(-1), g.obs0)
    ak = {"f32": N.ACTION_F32, "f64": N.ACTION_F64, "weak": N.ACTION_WEAK}[ACTION_KIND[str(g.action_as)]]
    adt = torch.float32 if ak == N.ACTION_F32 else torch.float64
    keep = {int(k): j for j, k in enumerate(g.keep)}
    for i, a in enumerate(g.actions):
        obs, r, te, tr = env.step(torch.full((B,), float(a), dtype=adt), action_kind=ak)
        if i in keep:
            np.testing.assert_array_equal(env.u.cpu().numpy()[ROW], g.rows[keep[i]], err_msg=f"row step {i}")
            np.testing.assert_array_equal(obs.cpu().numpy()[ROW].reshape(-1), g.obs[keep[i]], err_msg=f"obs step {i}")
        assert int(env.time_index[ROW]) == int(g.time_index[i])
        assert bool(te[ROW]) == bool(g.terminate[i]) and bool(tr[ROW]) == bool(g.truncate[i]), f"flags step {i}"
        if np.isfinite(g.reward[i]):
            np.testing.assert_allclose(r.cpu().numpy()[ROW], g.reward[i], rtol=1e-6, atol=2e-6 * max(1.0, float(g.norm[i])),
                                       err_msg=f"reward step {i}")


# ---- Navier-Stokes ------------------------------------------------------------------------------------------------------------
def _dbg(key, value):
    """Test-only kernel dispatch override (pdegym_debug_set, include/pdegym.h)."""
    from pdecontrolgym_amd import _native as N
    N.load().pdegym_debug_set(getattr(N, key), int(value))


def _ns_modes(case):
    n = int(SWEEP_NS[case].n)
    return ["default"] + (["column", "workgroup"] if n in (8, 11, 16, 21, 26, 31, 32) and n <= 64 else [])


@pytest.mark.parametrize("case,mode", [(c, m) for c in sorted(SWEEP_NS) for m in _ns_modes(c)])
def test_ns_hip_matches_reference_sweep(case, mode):
    from pdecontrolgym_amd.batch2d import NSBatch2D
    g = SWEEP_NS[case]
    if mode != "default":
        _dbg("DEBUG_NS_COL_MIN_BATCH", 0 if mode == "column" else 1000000)
    try:
        env = NSBatch2D(float(g.T), float(g.dt), float(g.X), float(g.dx), float(g.Y), float(g.dy), ns_bc_from_array(g.bc), g.U_ref,
                        g.action_ref, action_dim=int(g.action_dim), gamma=float(g.gamma), viscosity=float(g.viscosity),
                        density=float(g.density), maximum_pressure_iteration=int(g.maximum_pressure_iteration), num_envs=B,
                        device="cuda", dtype=torch.float64)
        assert env.nx == env.ny == int(g.n) and env.nt == int(g.nt)
        s = SCALE[:, None, None]
        env.reset(g.u0[None] * s, g.v0[None] * s, g.p0[None] * s)
        for i, a in enumerate(g.actions):
            obs, r, te = env.step(np.tile(a[None], (B, 1)))
            np.testing.assert_array_equal(obs.cpu().numpy()[ROW], g.obs[i], err_msg=f"obs step {i}")
            np.testing.assert_array_equal(env.p.cpu().numpy()[ROW], g.p[i], err_msg=f"p step {i}")
            np.testing.assert_allclose(r.cpu().numpy()[ROW], g.rewards[i], rtol=1e-12, err_msg=f"reward step {i}")
            assert bool(te[ROW]) == bool(g.terminate[i])
    finally:
        if mode != "default":
            _dbg("DEBUG_NS_COL_MIN_BATCH", -1)


# ---- traffic ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(SWEEP_TRAFFIC))
def test_traffic_hip_matches_reference_sweep(case):
    from pdecontrolgym_amd.batch_traffic import TrafficBatch
    g = SWEEP_TRAFFIC[case]
    env = TrafficBatch(float(g.T), float(g.dt), float(g.X), float(g.dx), str(g.sim), float(g.v_max), float(g.ro_max), float(g.tau),
                       bool(g.limit), int(g.control_freq), num_envs=B, device="cuda")
    assert 2 * env.M == g.obs.shape[1]
    env.set_action_bounds(np.full(B, float(g.qs_clip)))
    rs = float(g.rs) * np.array([0.96, 1.0, 1.03])               # the steady state scales the initial profile
    o = env.reset(rs)
    np.testing.assert_array_equal(o.cpu().numpy()[ROW], g.obs[0])
    for k, a in enumerate(g.actions):
        o, r, d, t = env.step(np.tile(a[None], (B, 1)))
        np.testing.assert_array_equal(o.cpu().numpy()[ROW], g.obs[k + 1], err_msg=f"step {k}")
        np.testing.assert_allclose(r.cpu().numpy()[ROW], g.reward[k], rtol=1e-13, err_msg=f"reward step {k}")
        assert bool(d[ROW]) == bool(g.done[k]) and bool(t[ROW]) == bool(g.trunc[k]), f"flags step {k}"
        assert float(env.t["time"][ROW]) == g.time[k], f"clock step {k}"


# ---- tumour -------------------------------------------------------------------------------------------------------------------
TUMOR_ARGS = ("t1_detection_threshold", "t2_detection_threshold", "dosage_termination_threshold", "D", "rho", "alpha",
              "alpha_beta_ratio", "k", "t1_detection_radius", "t1_death_radius")


@pytest.mark.parametrize("host_kill", [True, False], ids=["host-exp", "kernel-exp"])
@pytest.mark.parametrize("case", sorted(SWEEP_TUMOR))
def test_tumor_hip_matches_reference_sweep(case, host_kill):
    from pdecontrolgym_amd.batch_tumor import TumorBatch
    g = SWEEP_TUMOR[case]
    eng = TumorBatch(float(g.T), float(g.dt), float(g.X), float(g.dx), float(g.total_dosage), num_envs=B,
                     **{k: float(g[k]) for k in TUMOR_ARGS})
    assert eng.nx == g.init.shape[0]
    eng.set_benchmark(np.full(B, float(g.t_benchmark)))
    eng.reset(g.init[None] * np.array([0.9, 1.0, 0.95])[:, None])
    keep = {int(k): i for i, k in enumerate(g.keep)}
    np.testing.assert_array_equal(eng.t["u"].cpu().numpy()[ROW], g.rows[keep[0]])
    rtol = 0 if host_kill else 1e-12
    for n, a in enumerate(g.actions):
        kill = None
        if host_kill:                       # brain_tumor_env.py:260-264 on the day's applied dose, as the single environment does
            d = np.full(B, g.dosage[n + 1])
            kill = 1.0 - np.exp(-float(g.alpha) * (d + ((d ** 2) / float(g.alpha_beta_ratio))))
        u, r, te, tr = eng.step(np.full(B, a), kill=kill)
        if n + 1 in keep:
            np.testing.assert_allclose(u.cpu().numpy()[ROW], g.rows[keep[n + 1]], rtol=rtol, atol=0, err_msg=f"row day {n + 1}")
        np.testing.assert_allclose(float(r[ROW]), g.reward[n], rtol=1e-12, atol=0, err_msg=f"reward day {n + 1}")
        assert bool(te[ROW]) == bool(g.term[n]) and bool(tr[ROW]) == bool(g.trunc[n]), f"flags day {n + 1}"
        assert int(eng.t["stage"][ROW]) == int(g.stage[n]) and int(eng.t["time_index"][ROW]) == n + 1
        if host_kill:
            T1, _, _, applied = eng.t["out"].cpu().numpy()[ROW]
            assert applied == g.dosage[n + 1], f"dose day {n + 1}"
            assert (np.isnan(T1) and np.isnan(g.t1_idx[n + 1])) or T1 / float(g.dx) == g.t1_idx[n + 1], f"T1 radius day {n + 1}"
    np.testing.assert_array_equal(eng.t["days"].cpu().numpy()[ROW], g.days)
    np.testing.assert_allclose(float(eng.t["remaining"][ROW]), float(g.remaining), rtol=1e-15)
