"""The pointer-alignment contract of every kernel entry point (include/pdegym.h, Conventions: a pointer needs only the natural
alignment of its element type unless its parameter says otherwise; DESIGN.md section 4.14 holds the table).

Fresh torch tensors and the guarded payloads of tests/poison.py start on 256-byte boundaries, so every other GPU test hands the
kernels base pointers that a C caller carving arrays out of one pool, or slot t of a [T + 1, B, obs_dim] rollout buffer with an odd
B * obs_dim, does not have.  Each case here runs the call sequence of an existing contract test twice -- the unmodified engine or
backend call on aligned buffers, and guarded, poisoned buffers from a DISPLACED arena -- by handing that test's own runner a
displacement policy (``policy`` / ``displace``), never a copy of it:

  "one"    every buffer starts one element of its own dtype past a 256-byte boundary;
  "mixed"  the residue is a function of the buffer's name (float32 / int32 1..3 elements, float64 one, uint8 1..15), so the inputs
           and outputs of one launch are aligned differently from each other.

The runner asserts what it asserts on aligned buffers: every output of the displaced run equals the aligned run (or the exact
expectation both must equal) bit for bit, every guard is intact, what the header leaves alone keeps the poison, and the aligned
run meets its reference (oracle, NumPy restatement, float64 evaluation) at that test's own tolerance.  Buffers whose parameter
demands an alignment -- obs / U_ref / lam of the adjoint march, the blocked MLP weights and the backward workspace (the library's
own tensors) -- stay at shift 0 (``keep_aligned``); that the host refuses them displaced is checked without a launch by
tests/c/*_validation.c.  No kernel is ever launched with a pointer its code does not allow.

ALIGNMENT_CASES maps every kernel launched in pdecontrolgym_amd/csrc/*.hip to the tests here that reach it;
tests/test_poison_helper.py fails when a launched kernel is missing from it.
"""
import dataclasses

import numpy as np
import pytest

from tests import poison as PZ

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

POLICIES = ("one", "mixed")
policies = pytest.mark.parametrize("policy", POLICIES)

ALIGNMENT_CASES = {
    "step1d_kernel": ["test_1d_step", "test_1d_full_rows", "test_1d_m64"],
    "step1d_wide_kernel": ["test_1d_wide_row"],
    "reset1d_kernel": ["test_1d_resets"],
    "reset_history_kernel": ["test_1d_resets", "test_1d_step"],
    "rownorm2_kernel": ["test_small_1d_utilities"],
    "selftest_quotient_kernel": ["test_small_1d_utilities"],
    "rollout1d_kernel": ["test_1d_rollouts"],
    "rollout1d_general_kernel": ["test_1d_rollouts"],
    "rollout1d_policy_kernel": ["test_1d_rollouts"],
    "rollout1d_policy_general_kernel": ["test_1d_rollouts"],
    "backstep_rollout1d_kernel": ["test_backstepping_law_inside_the_1d_rollout"],
    "ns_col_step": ["test_ns_column_kernel"],
    "ns_col_step_w1": ["test_ns_column_kernel"],
    "ns_generic_step": ["test_ns_generic_kernel"],
    "ns_tile_step": ["test_ns_tiled_grids"],
    "ns_tile_step_f64": ["test_ns_tiled_grids"],
    "ns256_fused_step": ["test_ns_256"],
    "ns256_split_obs": ["test_ns_256"],
    "ns256_front_f64": ["test_ns_256"],
    "ns256_pass_f64": ["test_ns_256"],
    "ns256_split_obs_f64": ["test_ns_256"],
    "ns256_finish_f64": ["test_ns_256"],
    "ns_generic_pressure": ["test_ns_pressure_resets_and_rollout"],
    "ns_reset_kernel": ["test_ns_pressure_resets_and_rollout"],
    "ns_auto_reset_kernel": ["test_ns_pressure_resets_and_rollout"],
    "ns_auto_reset_finish": ["test_ns_pressure_resets_and_rollout"],
    "ns_col_rollout": ["test_ns_pressure_resets_and_rollout"],
    "ns_adjoint_march": ["test_ns_adjoint"],
    "traffic_step_kernel": ["test_traffic_step_and_reset"],
    "traffic_step_wide_kernel": ["test_traffic_step_and_reset"],
    "traffic_reset_kernel": ["test_traffic_step_and_reset"],
    "traffic_rollout_kernel": ["test_traffic_rollout"],
    "traffic_backstep_control_kernel": ["test_traffic_backstepping"],
    "traffic_backstep_rollout_kernel": ["test_traffic_backstepping"],
    "tumor_step_kernel": ["test_tumor_step_advance_reset"],
    "tumor_reset_kernel": ["test_tumor_step_advance_reset"],
    "tumor_rollout_kernel": ["test_tumor_rollout", "test_tumor_therapy_step"],
    "mlp_forward_kernel": ["test_mlp_forward_exact", "test_mlp_forward_vs_float64", "test_squashed_gaussian_head"],
    "mlp_backward_tiles": ["test_mlp_backward"],
    "mlp_backward_dw0": ["test_mlp_backward"],
    "mlp_backward_reduce": ["test_mlp_backward"],
    "gain_parabolic_kernel": ["test_backstepping_gains_and_control"],
    "gain_transport_kernel": ["test_backstepping_gains_and_control"],
    "backstep_control_kernel": ["test_backstepping_gains_and_control"],
    "gae_kernel": ["test_gae"],
}


def _C():
    from tests import test_gpu_buffer_contract as C
    return C


# ---- 1D step ---------------------------------------------------------------------------------------------------------------
@policies
@pytest.mark.parametrize("epl", [1, 4, 8, 32])
@pytest.mark.parametrize("kind", ["transport", "parabolic"])
def test_1d_step(kind, epl, policy):
    """Ragged rows at 1, 4, 8 and 32 slots per lane, B = 5, S = 3, three steps (the episode ends inside the last launch), without and
    with a trajectory: rows, observations and trajectories against the oracle bit for bit, rewards to rtol 1e-6 (_run_1d_pair)."""
    C = _C()
    n = C._ragged_slots(epl) + (kind == "parabolic")
    for mode in ("none", "hist"):
        C._run_1d_pair(kind, n, 5, mode, policy=policy)


@policies
@pytest.mark.parametrize("kind", ["transport", "parabolic"])
def test_1d_full_rows(kind, policy):
    """Full rows of 256 slots, B = 1: the write-through 16-byte row stores, without and with a trajectory."""
    C = _C()
    n = 256 + (kind == "parabolic")
    C._run_1d_pair(kind, n, 1, "none", policy=policy)
    C._run_1d_pair(kind, n, 1, "hist", policy=policy)


@policies
def test_1d_m64(policy):
    """float64 beta with ACTION_F64: beta and action are 8-byte elements next to the float32 rows."""
    from pdecontrolgym_amd import _native as N
    C = _C()
    _, pois, arena = C._run_1d_pair("parabolic", C._ragged_slots(4) + 1, 5, "none", f64_beta=True, action_kind=N.ACTION_F64,
                                        policy=policy)
    # the runner did hand the kernels displaced pointers: the engine's tensors are the arena's, none on a 16-byte boundary
    for k in ("u", "beta", "action", "obs", "reward", "terminated", "time_index", "bsum", "ring"):
        t = pois.t[k]
        assert t.data_ptr() % 16 != 0 and t.data_ptr() % t.element_size() == 0, (k, t.data_ptr() % 256)
        assert any(g.t.data_ptr() == t.data_ptr() for g in arena.bufs.values()), k

@policies
def test_1d_wide_row(policy):
    C = _C()
    C._run_1d_pair("transport", 2049, 2, "none", S=2, steps=2, policy=policy)
    C._run_1d_pair("parabolic", 2049, 2, "hist", S=2, steps=2, policy=policy)


# ---- 1D reset and rollouts ---------------------------------------------------------------------------------------------------
@policies
def test_1d_resets(policy):
    """Masked reset (trajectory included) and the fused auto-reset with pools of 7 rows and final_obs."""
    C = _C()
    C.test_1d_masked_reset_leaves_others_alone(policy=policy)
    C.test_1d_auto_reset_final_obs_and_pools(policy=policy)


@policies
@pytest.mark.parametrize("hidden", [16, 65])
def test_1d_rollouts(hidden, policy):
    """T = 3 at a full (257 nodes, parabolic) and a ragged (229) row, the general kernels (Neumann; scalar sensing), open loop and
    with the in-kernel policy at 16 (one fma chain per neuron) and 65 (cooperative MFMA evaluation) hidden units.  Slot t of the
    [T + 1, 5, n] observation buffer is displaced by the arena AND by 5 n floats per slot."""
    C = _C()
    C.test_1d_rollout_contract(policy=policy, lengths=(3,), widths=(hidden, hidden))


@policies
@pytest.mark.parametrize("kind,n,order", [("transport", 100, "ordered"), ("parabolic", 513, "ordered")])
def test_backstepping_law_inside_the_1d_rollout(kind, n, order, policy):
    from tests import test_gpu_backstep_rollout as BR
    BR.test_rollout_writes_exactly_its_outputs(kind, n, order, policy=policy)


@policies
def test_small_1d_utilities(policy):
    C = _C()
    C.test_rownorm2_ragged(policy=policy)
    C.test_selftest_quotient_counter_only(policy=policy)


# ---- Navier-Stokes ---------------------------------------------------------------------------------------------------------
@policies
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_ns_column_kernel(dtype, policy):
    """The column-per-lane kernel at its smallest grid (8 rows) and, against the oracle, at 21 x 21; float64 also on the one-wave
    build (B = 4000).  Every field is displaced: u, v, p, scratch, observations, U_ref."""
    C = _C()
    dt = getattr(torch, dtype)
    C._ns_pair(21, 2, 9, dt, ny=8, dispatch=dict(col_min_batch=0), steps=1, policy=policy)
    _, pois, _ = C._ns_pair(21, 2, 9, dt, ny=21, dispatch=dict(col_min_batch=0), steps=1, oracle=True, policy=policy)
    for k in ("p", "scratch", "U_ref", "obs", "state_in", "action", "reward", "terminated", "time_index"):
        assert pois.t[k].data_ptr() % 16 != 0, k
    if dtype == "float64":
        C._ns_pair(21, 4000, 3, dt, ny=16, dispatch=dict(col_min_batch=0), steps=1, seed=2, policy=policy)


@policies
@pytest.mark.parametrize("case", ["f64_20x24", "f64_40_oracle", "f32_33", "f64_100_split"])
def test_ns_generic_kernel(case, policy):
    """The workgroup kernel: a non-square grid, the three LDS modes, float32 and float64, interleaved and split state."""
    C = _C()
    f32, f64 = torch.float32, torch.float64
    if case == "f64_20x24":
        C._ns_pair(24, 2, 11, f64, ny=20, dispatch=dict(generic=True), steps=1, policy=policy)
    elif case == "f64_40_oracle":
        C._ns_pair(40, 2, 11, f64, dispatch=dict(generic=True, no_lds_jacobi=True), steps=1, oracle=True, policy=policy)
    elif case == "f32_33":
        C._ns_pair(33, 2, 7, f32, dispatch=dict(generic=True, no_col=True), steps=1, policy=policy)
    else:
        C._ns_pair(100, 2, 11, f64, dispatch=dict(generic=True), interleaved=False, steps=1, policy=policy)


@policies
@pytest.mark.parametrize("case", ["t64", "t64_sep", "t128", "t128_f64"])
def test_ns_tiled_grids(case, policy):
    """Register-tiled grids: the rows move as 8- / 16-byte pieces typed with the element's alignment (gvec, pdegym_ns_common.h), so
    every field is displaced like every [B] array, the command, the time index and action_ref."""
    C = _C()
    f32, f64 = torch.float32, torch.float64
    if case.startswith("t64"):
        _, pois, _ = C._ns_pair(64, 2, 11, f32, interleaved=not case.endswith("sep"), steps=1, oracle=True, policy=policy)
    elif case == "t128":
        _, pois, _ = C._ns_pair(128, 2, 11, f32, steps=1, policy=policy)
    else:
        _, pois, _ = C._ns_pair(128, 2, 11, f64, steps=1, oracle=True, policy=policy)
    for k in ("u", "v", "p", "scratch", "U_ref", "obs", "state_in", "action", "action_ref", "reward", "terminated", "time_index"):
        assert pois.t[k] is None or pois.t[k].data_ptr() % 16 != 0, k


@policies
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("interleaved", [True, False])
def test_ns_256(dtype, interleaved, policy):
    _C()._ns_pair(256, 2, 51, getattr(torch, dtype), interleaved=interleaved, steps=1, policy=policy)


@policies
def test_ns_pressure_resets_and_rollout(policy):
    C = _C()
    for dtype in ("float32", "float64"):
        C.test_ns_solve_pressure_contract(dtype, policy=policy)
    C.test_ns_masked_reset_leaves_others_alone(policy=policy)
    C.test_ns_auto_reset_final_obs(policy=policy)
    C.test_ns_rollout_contract(policy=policy)


@policies
def test_ns_adjoint(policy):
    """a_nom, grad and actions displaced; obs, U_ref and lam keep the 16 bytes the header demands of them."""
    from tests import adjoint_restatement as R
    from tests import test_gpu_adjoint as A
    fx = R.load_fixture()
    A.test_outputs_are_fully_written_and_inputs_left_alone(fx, "n21_K2_T6", policy=policy)
    A.test_lam_is_optional(fx, policy=policy)


# ---- traffic ---------------------------------------------------------------------------------------------------------------
@policies
@pytest.mark.parametrize("wide", [False, True])
def test_traffic_step_and_reset(wide, policy):
    _C().test_traffic_contract(5, wide, policy=policy)


@policies
def test_traffic_rollout(policy):
    _C().test_traffic_rollout_contract(policy=policy)


@policies
def test_traffic_backstepping(policy):
    """The control law on the register (M = 51) and the strided (M = 200) kernel, and the law inside the rollout."""
    from tests import test_gpu_traffic_backstep as TB
    for M in (51, 200):
        TB.test_control_writes_exactly_its_outputs(M, "both", policy=policy)
    TB.test_rollout_writes_exactly_its_outputs("numpy", "outlet", policy=policy)


# ---- tumour ----------------------------------------------------------------------------------------------------------------
@policies
@pytest.mark.parametrize("nx_big", [False, True])
def test_tumor_step_advance_reset(nx_big, policy):
    _C().test_tumor_contract(nx_big, policy=policy)


@policies
@pytest.mark.parametrize("with_policy", [False, True])
def test_tumor_rollout(with_policy, policy):
    """The TherapyWrapper steps of pdegym_tumor_rollout, commands given ahead and from the in-kernel policy; the engine's state and
    [B] outputs and the int64 counters of the wrapper are displaced too."""
    from tests import test_gpu_tumor_rollout as TR
    TR.test_output_contract_on_poisoned_guarded_buffers(with_policy, displace=policy)


@policies
@pytest.mark.parametrize("nx,T,weekends", [(201, 600, True), (70, 300, False)])
def test_tumor_therapy_step(nx, T, weekends, policy):
    """pdegym_tumor_therapy_step, its own host function and pointer wiring: the command comes from bufs.control, the results go to
    the engine's [B] tensors, the wrapper's counters, init, final_obs and obs are separate arrays -- all displaced."""
    from tests import test_gpu_tumor_rollout as TR
    TR.test_therapy_step_on_guarded_buffers(nx, T, weekends, displace=policy)


# ---- policy ----------------------------------------------------------------------------------------------------------------
def _forward_cases():
    """Exactly summable networks (tests/mlp_exact.py): widths 16, 65 and 129 (the 4-, 8- and 16-wave launches), in_dim 5 and 257, the
    four x / y precisions, noise, a clamp that binds, rows with gaps."""
    from tests import mlp_exact as mx
    cases = []
    for i, (W, K) in enumerate(((16, 5), (65, 257), (129, 5), (16, 257), (65, 5), (129, 257))):
        for j, (xf, yf) in enumerate(((False, False), (True, False), (False, True), (True, True))):
            cases.append(mx.Case(f"align-K{K}-W{W}-x{int(xf)}y{int(yf)}", (K, W, 3), ("relu", None), 17, seed=7000 + 4 * i + j, x_f64=xf,
                                 y_f64=yf, eps=xf, gaps=True, noise=True, clamp=True))
    return cases


FORWARD_CASES = _forward_cases()


@policies
@pytest.mark.parametrize("case", FORWARD_CASES, ids=[c.name for c in FORWARD_CASES])
def test_mlp_forward_exact(case, policy):
    """x, y and noise displaced (each row also by its gap); the result equals the float64 expectation exactly, as on aligned buffers."""
    from tests import test_gpu_mlp_exact as ME
    ME.test_forward_kernel_is_exact(case, policy=policy)


@policies
@pytest.mark.parametrize("width,in_dim", [(64, 5), (128, 257), (256, 37)])
def test_mlp_forward_vs_float64(width, in_dim, policy):
    """Real weights, B = 17, the four precisions, against the float64 evaluation at the contract test's own bound."""
    C = _C()
    for xf in (False, True):
        for yf in (False, True):
            C.test_mlp_forward_contract_vs_float64(width, 17, in_dim, xf, yf, policy=policy)


@policies
@pytest.mark.parametrize("A", [2, 8])
def test_squashed_gaussian_head(A, policy):
    from tests import gaussian_exact as gx
    from tests import test_gpu_gaussian_head as GH
    cases = [c for c in gx.FORWARD_CASES if c.A == A]
    assert len(cases) >= 4
    for case in cases:
        GH.test_forward_kernel_against_the_float64_expectation(case, policy=policy)


@policies
@pytest.mark.parametrize("dx", [True, False])
def test_mlp_backward(dx, policy):
    """B = 33 (three tiles of 16 rows) at every slab count it allows (the library's choice, 1, 2, 3), with and without dx: x, dy, dx and
    the row-major w[] and every dw / db displaced; the workspace (4-byte aligned by the header) and the blocked weights (16) are the
    library's own."""
    from tests import mlp_backward_exact as R
    from tests import test_gpu_mlp_backward as MB
    case = next(c for c in R.CASES if c.name == "one-tile-per-slab")
    assert case.B == 33 and case.dx and set(R.valid_slabs(case.B)) >= {0, 1, 3}
    MB.test_backward_kernels_are_exact(dataclasses.replace(case, dx=dx), policy=policy)


# ---- baselines and GAE -------------------------------------------------------------------------------------------------------
@policies
def test_backstepping_gains_and_control(policy):
    """Both gain kernels (theta float32 in, gains float64 out) and pdegym_backstep_control with float64 and float32 outputs."""
    from tests import test_gpu_backstepping as BS
    for kind in ("transport", "parabolic"):
        for m, R in ((65, 3), (129, 70)):
            BS.test_gain_kernels_write_exactly_their_rows(kind, m, R, policy=policy)
    BS.test_control_writes_exactly_its_outputs_and_follows_the_pool_rule(policy=policy)


@policies
@pytest.mark.parametrize("T,B", [(5, 3), (33, 70), (5, 70), (33, 3)])
def test_gae(T, B, policy):
    """float32 and float64 rewards, row stride B and B + 3, with and without the statistics rows and the accumulators: bit-equal to the
    restatement (tests/gae_restatement.py), as on aligned buffers."""
    from tests import test_gpu_gae as G
    rng = np.random.default_rng([T, B])
    for f64 in (False, True):
        rew, val, te, tr, boot = G._case(T, B, f64)
        acc = (rng.normal(0.0, 3.0, B), rng.integers(0, 50, B).astype(np.int32))
        for ld in (B, B + 3):
            got = G._launch(rew, val, te, tr, boot, 0.99, 0.95, ld=ld, acc=acc, policy=policy)
            G._assert_same(got, G._expect(rew, val, te, tr, boot, 0.99, 0.95, acc), ("displaced", f64, ld))
        want = G._expect(rew, val, te, tr, boot, 0.99, 0.95)
        got = G._launch(rew, val, te, tr, boot, 0.99, 0.95, stats=False, policy=policy)
        assert sorted(got) == ["advantages", "returns"]
        G._assert_same(got, want, ("displaced, no statistics", f64))


# ---- the public Python faces on offset views -------------------------------------------------------------------------------------
def test_fused_mlp_on_slices_of_a_larger_tensor():
    """FusedMLP.forward_into on big[1:] views -- observation rows, actions and noise each one row (an odd number of elements) into a
    larger tensor -- equals the same call on fresh tensors bit for bit, in the four precisions."""
    from pdecontrolgym_amd.policy import FusedMLP
    torch.manual_seed(3)
    B, K, H, A = 17, 37, 65, 3
    mod = torch.nn.Sequential(torch.nn.Linear(K, H), torch.nn.Tanh(), torch.nn.Linear(H, A)).cuda()
    pol = FusedMLP(mod, clamp=(-0.5, 0.5))
    for xdt in (torch.float32, torch.float64):
        for ydt in (torch.float32, torch.float64):
            x = torch.randn(B, K, dtype=xdt, device="cuda")
            nz = (torch.randn(B, A, device="cuda") * 0.3).float()
            fresh = pol.forward_into(x, torch.empty(B, A, dtype=ydt, device="cuda"), noise=nz).clone()
            xb = torch.full((B + 1, K), float("nan"), dtype=xdt, device="cuda")
            nb = torch.full((B + 1, A), float("nan"), dtype=torch.float32, device="cuda")
            yb = PZ.poison_(torch.empty(B + 1, A, dtype=ydt, device="cuda"))
            xv, nv, yv = xb[1:], nb[1:], yb[1:]
            xv.copy_(x)
            nv.copy_(nz)
            assert xv.data_ptr() % 16 != 0 and (nv.data_ptr() % 16 != 0 or yv.data_ptr() % 16 != 0)
            pol.forward_into(xv, yv, noise=nv)
            torch.cuda.synchronize()
            PZ.assert_written(yb, (slice(1, None),), f"y {xdt} -> {ydt}", like=torch.cat([yb[:1], fresh]))
            PZ.assert_untouched(yb, (slice(0, 1),), "the row in front of the view")
            assert bool(torch.isfinite(fresh).all())


@pytest.mark.parametrize("one_launch", [True, False])
def test_device_rollout_with_an_odd_slot_size(one_launch):
    """DeviceRollout on 5 instances of 17 nodes: B * obs_dim = 85 floats per slot, so slot 1 and slot 3 of the [T + 1, B, 17] buffer,
    and the odd rows of every [T, 5] array, are only 4-byte aligned.  Equal, bit for bit, to the same policy and steps on fresh
    tensors (a twin environment driven one step_tensor call at a time)."""
    from pde_control_gym import DeviceRollout, FusedMLP
    from tests.test_gpu_gae import _mlp, _parabolic_env
    B, T = 5, 4
    venv, D = _parabolic_env(B)
    twin, _ = _parabolic_env(B)
    assert (B * D) % 2 == 1
    actor = FusedMLP(_mlp([D, 65, 1], 1))      # 65 units: inside the rollout kernel bit-identical to pdegym_mlp_forward (pdegym.h)
    ro = DeviceRollout(venv, actor, T, use_graph=False, one_launch=one_launch, action_low=-10.0, action_high=10.0).run()
    torch.cuda.synchronize()
    assert ro.obs[1].data_ptr() % 8 == 4 and ro.one_launch == one_launch
    obs = twin.rollout_obs().clone()
    PZ.assert_bits_equal(ro.obs[0], obs, None, "slot 0")
    for t in range(T):
        a = actor.forward_into(obs, torch.empty(B, dtype=torch.float32, device="cuda"), clamp=(-10.0, 10.0))
        o, r, te, tr = twin.step_tensor(a)
        obs = o.clone()
        PZ.assert_bits_equal(ro.actions[t], a, None, f"actions[{t}]")
        PZ.assert_bits_equal(ro.obs[t + 1], obs.reshape(ro.obs[t + 1].shape), None, f"obs[{t + 1}]")
        PZ.assert_bits_equal(ro.rewards[t], r, None, f"rewards[{t}]")
        PZ.assert_bits_equal(ro.terminated[t], te, None, f"terminated[{t}]")
        PZ.assert_bits_equal(ro.truncated[t], tr, None, f"truncated[{t}]")
