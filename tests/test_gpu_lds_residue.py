"""Every kernel on poisoned LDS: no result may depend on what the previous launch left there (tests/lds_residue.py).

LDS is not cleared between launches, and every other GPU test runs a kernel behind itself or a close relative, on similar data: the
residue a workgroup finds is finite and plausible.  Here every entry point of the C ABI is preceded, on its own stream, by a launch
that fills the whole LDS of every CU with a bit pattern (``dirtied``): quiet NaNs in both float views ("nan"), or enormous finite
values ("huge": a leak into a sum changes bits but survives ``isfinite``), or all bits set ("ones").

The witness tests come first and gate the rest: they show that the dirtier reaches every CU and that what it leaves in LDS is what
the next kernel on the stream finds, word for word (DESIGN.md section 4.19 holds the counts).

A case is the call sequence of an existing runner or test -- called, never copied -- once undirtied, once under "nan" and once under
"huge" (``_runs``).  Those runners hold their outputs to the oracle, a restatement or the golden files, mostly bit for bit, so a
leak shows as a failed comparison inside them; where a runner returns its outputs, the three runs must also agree bit for bit.
Every case asserts ``entry_calls > 0`` and ``dirty_launches == entry_calls`` and names the entry points it must have gone through.
The shapes added on top of the runners' own are the smallest at which LDS padding is live: rows that are no multiple of four (of
16) inputs, layers of 1, 15, 17, 33, 63, 65, 129, 130 units, batches that leave dead rows in the last tile, reductions with fewer
live waves than slots, the first Jacobi sweeps (K = 0, 1, 2) of every Navier-Stokes family.

KNOWN LIMIT (tests/lds_residue.py): an entry point that makes several launches is dirtied before the first one only.

LDS_CASES maps every ``__global__`` function defined in pdecontrolgym_amd/csrc to the tests here that reach it;
tests/test_lds_residue_helper.py fails when a kernel is missing from it.
"""
from __future__ import annotations


import numpy as np
import pytest
import torch

from tests import lds_residue as LR

pytestmark = pytest.mark.gpu

PATTERNS = ("nan", "huge")
INTEGER_PATTERNS = PATTERNS + ("ones",)      # the kernels whose LDS rows drive a stage machine or a comparison

LDS_CASES = {
    # ---- 1D
    "step1d_kernel": ["test_1d_step_kernels", "test_1d_resets_and_utilities"],
    "step1d_wide_kernel": ["test_1d_wide_rows"],
    "reset1d_kernel": ["test_1d_resets_and_utilities", "test_1d_step_kernels"],
    "reset_history_kernel": ["test_1d_resets_and_utilities", "test_1d_step_kernels"],
    "rownorm2_kernel": ["test_1d_resets_and_utilities"],
    "selftest_quotient_kernel": ["test_1d_resets_and_utilities"],
    "rollout1d_kernel": ["test_1d_rollouts", "test_1d_rollout_ladder"],
    "rollout1d_general_kernel": ["test_1d_rollouts"],
    "rollout1d_policy_kernel": ["test_1d_rollouts", "test_1d_rollout_ladder", "test_policy_inside_the_rollouts_with_live_padding",
                                "test_gaussian_policy_inside_the_rollouts_with_live_padding"],
    "rollout1d_policy_general_kernel": ["test_policy_inside_the_rollouts_with_live_padding",
                                        "test_gaussian_policy_inside_the_rollouts_with_live_padding", "test_1d_rollouts"],
    "gain_parabolic_kernel": ["test_backstepping_gains_and_control"],
    "gain_transport_kernel": ["test_backstepping_gains_and_control"],
    "backstep_control_kernel": ["test_backstepping_gains_and_control"],
    "backstep_rollout1d_kernel": ["test_backstepping_law_inside_the_rollout"],
    # ---- Navier-Stokes
    "ns_col_step": ["test_ns_column_kernels"],
    "ns_col_step_w1": ["test_ns_column_kernels"],
    "ns_generic_step": ["test_ns_first_sweeps"],
    "ns_tile_step": ["test_ns_first_sweeps"],
    "ns_tile_step_f64": ["test_ns_first_sweeps"],
    "ns256_fused_step": ["test_ns_first_sweeps"],
    "ns256_split_obs": ["test_ns_first_sweeps"],
    "ns256_front_f64": ["test_ns_first_sweeps"],
    "ns256_pass_f64": ["test_ns_first_sweeps"],
    "ns256_finish_f64": ["test_ns_first_sweeps"],
    "ns256_split_obs_f64": ["test_ns_first_sweeps"],
    "ns_generic_pressure": ["test_ns_solve_pressure_forms", "test_ns_pressure_resets_and_rollout"],
    "ns_reset_kernel": ["test_ns_pressure_resets_and_rollout"],
    "ns_auto_reset_kernel": ["test_ns_pressure_resets_and_rollout"],
    "ns_auto_reset_finish": ["test_ns_pressure_resets_and_rollout"],
    "ns_col_rollout": ["test_ns_pressure_resets_and_rollout"],
    "ns_adjoint_march": ["test_ns_adjoint_march"],
    # ---- traffic and tumour
    "traffic_step_kernel": ["test_traffic_rows", "test_traffic_contract"],
    "traffic_step_wide_kernel": ["test_traffic_rows", "test_traffic_contract"],
    "traffic_reset_kernel": ["test_traffic_rows", "test_traffic_contract"],
    "traffic_rollout_kernel": ["test_traffic_rollout", "test_policy_inside_the_rollouts_with_live_padding",
                               "test_gaussian_policy_inside_the_rollouts_with_live_padding"],
    "traffic_backstep_control_kernel": ["test_traffic_backstepping"],
    "traffic_backstep_rollout_kernel": ["test_traffic_backstepping"],
    "tumor_step_kernel": ["test_tumor_step_and_advance", "test_tumor_contract"],
    "tumor_reset_kernel": ["test_tumor_step_and_advance", "test_tumor_contract"],
    "tumor_rollout_kernel": ["test_tumor_rollout", "test_policy_inside_the_rollouts_with_live_padding",
                             "test_gaussian_policy_inside_the_rollouts_with_live_padding"],
    # ---- networks
    "mlp_forward_kernel": ["test_mlp_forward_with_live_padding", "test_gaussian_forward"],
    "mlp_backward_tiles": ["test_mlp_backward_with_live_padding"],
    "mlp_backward_dw0": ["test_mlp_backward_with_live_padding"],
    "mlp_backward_reduce": ["test_mlp_backward_with_live_padding"],
    "mlp_backward_wide_tiles": ["test_mlp_backward_wide_with_live_padding"],
    "mlp_backward_wide_accumulate": ["test_mlp_backward_wide_with_live_padding"],
    "mlp_backward_wide_reduce": ["test_mlp_backward_wide_with_live_padding"],
    # ---- training heads
    "gae_kernel": ["test_gae"],
    "moments_kernel": ["test_ppo_loss_with_few_live_waves"],
    "rows_kernel": ["test_ppo_loss_with_few_live_waves"],
    "finish_kernel": ["test_ppo_loss_with_few_live_waves"],
    "log_prob_kernel": ["test_ppo_loss_with_few_live_waves"],
    "sample_kernel": ["test_sac_sample_and_backward"],
    "sample_backward_kernel": ["test_sac_sample_and_backward"],
    "critic_rows_kernel": ["test_sac_losses_with_few_live_waves"],
    "critic_finish_kernel": ["test_sac_losses_with_few_live_waves"],
    "actor_rows_kernel": ["test_sac_losses_with_few_live_waves"],
    "actor_finish_kernel": ["test_sac_losses_with_few_live_waves"],
    "head_kernel": ["test_fused_adam_with_few_live_waves"],
    "update_kernel": ["test_fused_adam_with_few_live_waves"],
}


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


# ---------------------------------------------------------------------------------------------------------------- the witness

def test_dirtier_reaches_every_cu():
    cus, max_bytes = LR.info()
    assert cus == _cus()
    seen = torch.zeros(LR.SEEN_CAP, dtype=torch.int32, device="cuda")
    LR.dirty("nan", _stream(), seen=seen)
    torch.cuda.synchronize()
    ids = torch.nonzero(seen).flatten().tolist()
    print(f"lds_dirty: {cus} CUs, {max_bytes} bytes of LDS per workgroup, {LR.GROUPS_PER_CU * cus} workgroups, "
          f"{len(ids)} distinct __smid() values (largest {max(ids) if ids else None})")
    assert len(ids) == cus


@pytest.mark.parametrize("pattern", sorted(LR.PATTERNS))
def test_residue_reaches_the_next_kernel(pattern):
    """Every word of every workgroup, at every size and grid: a hole would be a defect of the dirtier (more workgroups, a larger
    segment), never a threshold here."""
    cus, max_bytes = LR.info()
    sizes = sorted({1 << 10, 16 << 10, 64 << 10, max_bytes})
    holes = []
    for lds_bytes in sizes:
        for grid in (1, cus, 8 * cus):
            LR.dirty(pattern, _stream())
            count, smid = LR.witness(pattern, lds_bytes, grid, _stream())
            torch.cuda.synchronize()
            words = lds_bytes // 4
            full = int((count == words).sum())
            print(f"lds_witness[{pattern}] {lds_bytes:6d} B x {grid:4d} workgroups: {full} of {grid} workgroups read the pattern in "
                  f"every word; fewest matching words {int(count.min())} of {words}; {len(set(smid.tolist()))} CUs")
            if full != grid:
                holes.append((lds_bytes, grid, full, int(count.min())))
    assert not holes, f"(bytes, workgroups, whole workgroups, fewest words): {holes}"


@pytest.mark.parametrize("n", [5, 101])
def test_an_unwritten_pad_is_what_the_patterns_show(n):
    """The defect this suite looks for, in a test kernel of its own (lds_pad_probe: a row of n floats staged "zero-padded to a multiple
    of four", reduced over the padded length).  With the pad written the result is the exact sum under every pattern.  With the pad
    left as found, "nan" and "ones" turn both reductions into NaN; "huge" leaves the product form -- 0 * residue -- equal to the clean
    result and shows only in the plain sum: why the cases run "nan" as well as "huge", and compare bits rather than ``isfinite``."""
    x = torch.arange(1, n + 1, dtype=torch.float32, device="cuda")
    exact = float(n * (n + 1) // 2)
    for pattern in sorted(LR.PATTERNS):
        LR.dirty(pattern, _stream())
        good = LR.pad_probe(x, True, _stream()).tolist()
        LR.dirty(pattern, _stream())
        bad = LR.pad_probe(x, False, _stream()).tolist()
        print(f"lds_pad_probe[{pattern}] n={n}: pad written {good}, pad left as found {bad}")
        assert good == [exact, exact], pattern
        if pattern == "huge":
            assert bad[0] == exact and bad[1] != exact, "0 * huge is 0: only the sum shows the leak"
        else:
            assert np.isnan(bad[0]) and np.isnan(bad[1]), pattern


# ------------------------------------------------------------------------------------------------------------------- the harness

ENGINE_OUTPUTS = ("u", "v", "p", "r", "y", "time", "time_index", "reward", "terminated", "truncated", "done", "norm_now", "norm_back",
                  "stage", "remaining", "days", "out")


def _flat(x, out, path="out"):
    """Every array in what a runner returned, as (path, NumPy array): tensors, arrays, numbers, dicts, sequences; of an engine (an
    object with a tensor dictionary ``t``) the state and output tensors of ENGINE_OUTPUTS and its observation pair."""
    if x is None:
        return
    if torch.is_tensor(x):
        out.append((path, x.detach().cpu().contiguous().numpy()))
    elif isinstance(x, np.ndarray):
        out.append((path, np.ascontiguousarray(x)))
    elif isinstance(x, (bool, int, float, np.generic)):
        out.append((path, np.asarray(x)))
    elif isinstance(x, dict):
        for k in sorted(x, key=str):
            _flat(x[k], out, f"{path}.{k}")
    elif isinstance(x, (list, tuple)):
        for i, v in enumerate(x):
            _flat(v, out, f"{path}[{i}]")
    elif isinstance(getattr(x, "t", None), dict):
        for k in ENGINE_OUTPUTS:
            _flat(x.t.get(k), out, f"{path}.t[{k}]")
        _flat(list(getattr(x, "_obs", ())), out, f"{path}._obs")


def _snapshot(x):
    out = []
    _flat(x, out)
    return out


def _assert_same_bits(a, b, what):
    assert [p for p, _ in a] == [p for p, _ in b], what
    for (p, x), (_, y) in zip(a, b):
        assert x.shape == y.shape and x.dtype == y.dtype, f"{what}: {p}"
        assert x.tobytes() == y.tobytes(), f"{what}: {p} differs in {int((x.view(np.uint8) != y.view(np.uint8)).sum())} byte(s) of {x.nbytes}"


def _forget_cached_engines():
    """Engines that other modules keep between tests were (or may have been) built outside ``dirtied``: their prepared calls hold
    the unwrapped functions.  The cases build their own."""
    from tests import test_gpu_mlp_exact as ME
    ME._env_1d.cache_clear()
    ME._env_tumor.cache_clear()


def _runs(fn, *entries, patterns=PATTERNS, outputs=True):
    """``fn()`` undirtied, then inside ``dirtied(p)`` for every pattern.  ``entries`` is the EXACT set of entry points the case goes
    through: each was called, no other was, every call was dirtied, and every pattern saw the same number of calls of each.
    ``outputs`` = True: ``fn`` returns its outputs, and the undirtied run and every dirtied run agree on them bit for bit (an empty
    snapshot is an error).  ``outputs`` = False: ``fn`` is a test function of another module that returns nothing -- the case rests on
    the comparisons that function makes against its own reference (DESIGN.md section 4.19 lists these cases and their references)."""
    _forget_cached_engines()
    clean = _snapshot(fn())
    torch.cuda.synchronize()
    assert bool(clean) == outputs, f"{len(clean)} output array(s) returned where outputs={outputs}"
    calls = None
    for p in patterns:
        _forget_cached_engines()
        with LR.dirtied(p) as d:
            got = _snapshot(fn())
            torch.cuda.synchronize()
        d.check(*entries, exact=True)
        calls = calls or d.by_entry
        assert d.by_entry == calls, f"'{p}' made other calls than '{patterns[0]}': {d.by_entry} against {calls}"
        _assert_same_bits(got, clean, f"LDS residue '{p}' against the undirtied run")
    _forget_cached_engines()


def _C():
    from tests import test_gpu_buffer_contract as C
    return C


# ------------------------------------------------------------------------------------------------------------------------ 1D

@pytest.mark.parametrize("kind", ["transport", "parabolic"])
def test_1d_step_kernels(kind):
    """Ragged rows at 1, 4 and 32 slots per lane (B = 5) and the full row of 256 slots with a trajectory (B = 1): rows, observations
    and trajectories against the oracle bit for bit (_run_1d_pair), and the guarded engine's state equal in the three runs."""
    C = _C()
    p = kind == "parabolic"

    def fn():
        out = [C._run_1d_pair(kind, C._ragged_slots(e) + p, 5, "none")[1] for e in (1, 4, 32)]
        out.append(C._run_1d_pair(kind, 256 + p, 1, "hist")[1])
        return out
    _runs(fn, f"pdegym_{kind}_step", "pdegym_reset1d_masked")


def test_1d_wide_rows():
    """Rows past the register limit live in two wave-private LDS copies (step1d_wide_kernel); the last call of each sequence is past the
    episode's end and makes no sub-step, so the second copy is never written in it."""
    C = _C()
    _runs(lambda: [C._run_1d_pair("transport", 2049, 2, "none", S=2, steps=2)[1],
                   C._run_1d_pair("parabolic", 2049, 2, "hist", S=2, steps=2, f64_beta=True)[1],
                   C._run_1d_pair("transport", 2049, 2, "diff", S=2, steps=2)[1],      # the differential horizon reads the row before the
                   C._run_1d_pair("parabolic", 2049, 2, "thor", S=2, steps=2)[1]],     # last sub-step from the second LDS copy
          "pdegym_transport_step", "pdegym_parabolic_step", "pdegym_reset1d_masked")


def test_1d_resets_and_utilities():
    C = _C()

    def fn():
        C.test_1d_masked_reset_leaves_others_alone()
        C.test_1d_auto_reset_final_obs_and_pools()
        C.test_rownorm2_ragged()
        C.test_selftest_quotient_counter_only()
    _runs(fn, "pdegym_reset1d_masked", "pdegym_transport_step", "pdegym_rownorm2_f32", "pdegym_selftest_quotient", outputs=False)


@pytest.mark.parametrize("hidden", [16, 65])
def test_1d_rollouts(hidden):
    """The four rollout kernels (full / ragged rows, Neumann and scalar sensing: the general forms), open loop and with a policy of 16
    (one fma chain per neuron) and 65 (cooperative) units inside; observation rows of 257, 229, 101 and 1 values."""
    C = _C()
    _runs(lambda: C.test_1d_rollout_contract(lengths=(3,), widths=(hidden, hidden)), "pdegym_transport_rollout", "pdegym_parabolic_rollout",
          "pdegym_transport_step", "pdegym_parabolic_step", "pdegym_reset1d_masked", outputs=False)


@pytest.mark.parametrize("kind", ["transport", "parabolic"])
def test_1d_rollout_ladder(kind):
    """The rollout ladder at a ragged and a full row: one rollout call against T step calls, and with the policy inside against the
    policy launch + step launch per env-step."""
    from tests import test_gpu_rollout_ladder as RL
    p = kind == "parabolic"

    def fn():
        for slots in (37, 256):
            RL._rollout_against_steps(kind, slots + p)
            for hidden in (16, 65):
                RL.test_rollout_with_the_policy_inside_equals_policy_and_step_launches(kind, hidden, slots)
    _runs(fn, f"pdegym_{kind}_rollout", f"pdegym_{kind}_step", "pdegym_reset1d_masked", "pdegym_mlp_forward", outputs=False)


def test_backstepping_gains_and_control():
    from tests import test_gpu_backstepping as BS

    def fn():
        for kind in ("transport", "parabolic"):
            for m in (2, 5, 65, 129):
                BS.test_gain_kernels_equal_the_restatement_bitwise(kind, m)
            for m, R in ((65, 3), (129, 70)):
                BS.test_gain_kernels_write_exactly_their_rows(kind, m, R)
        for m in (3, 65, 129):
            BS.test_control_law_orders(m)
        BS.test_control_writes_exactly_its_outputs_and_follows_the_pool_rule()
    _runs(fn, "pdegym_backstep_gain_parabolic", "pdegym_backstep_gain_transport", "pdegym_backstep_control", outputs=False)


def test_backstepping_law_inside_the_rollout():
    """backstep_rollout1d_kernel keeps its observation strips in LDS: rows of 100, 101 and 513 values, both summation orders."""
    from tests import test_gpu_backstep_rollout as BR
    from tests import test_gpu_rollout_ladder as RL

    def fn():
        for kind, n, order in (("transport", 100, "ordered"), ("parabolic", 101, "tree"), ("parabolic", 513, "ordered")):
            BR.test_rollout_writes_exactly_its_outputs(kind, n, order)
        for kind in ("transport", "parabolic"):
            for order in ("ordered", "tree"):
                RL.test_rollout_with_the_law_inside_equals_control_and_step_launches(kind, order, 37)
    _runs(fn, "pdegym_transport_backstep_rollout", "pdegym_parabolic_backstep_rollout", "pdegym_backstep_gain_transport",
          "pdegym_backstep_gain_parabolic", "pdegym_backstep_control", "pdegym_transport_step", "pdegym_parabolic_step", "pdegym_reset1d_masked",
          outputs=False)


# ------------------------------------------------------------------------------------------------------------- Navier-Stokes

@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_ns_column_kernels(dtype):
    """The column-per-lane kernel (its reward reduction goes through LDS) at its smallest grid, 8 rows, with K = 0, 1, 2 sweeps, and
    against the oracle at 21 x 21; float64 also on the one-wave build (B = 4000)."""
    C = _C()
    dt = getattr(torch, dtype)

    def fn():
        out = [C._ns_pair(21, 2, K, dt, ny=8, dispatch=dict(col_min_batch=0), steps=1)[1] for K in (0, 1, 2)]
        out.append(C._ns_pair(21, 5, 9, dt, ny=21, dispatch=dict(col_min_batch=0), steps=2, oracle=True)[1])
        if dtype == "float64":
            out.append(C._ns_pair(21, 4000, 3, dt, ny=16, dispatch=dict(col_min_batch=0), steps=1, seed=2)[1])
        return out
    _runs(fn, "pdegym_ns2d_step_f" + dtype[-2:], "pdegym_ns2d_reset_masked_f" + dtype[-2:])


# family -> (_ns_pair arguments (n, B, dtype name), keywords, the K of the runner's own case)
NS_FAMILIES = {
    "tile64_f32": ((64, 3, "float32"), dict(oracle=True), 11),
    "tile64_f32_separate": ((64, 2, "float32"), dict(interleaved=False), 11),
    "tile128_f32": ((128, 2, "float32"), dict(), 11),
    "tile128_f64": ((128, 2, "float64"), dict(oracle=True), 11),
    "generic_f64_global_jacobi": ((40, 3, "float64"), dict(dispatch=dict(generic=True, no_lds_jacobi=True), oracle=True), 11),
    "generic_f64_lds_jacobi_two_copies": ((40, 3, "float64"), dict(dispatch=dict(generic=True), p_out=True), 11),
    "generic_f64_lds_jacobi_one_copy": ((100, 2, "float64"), dict(dispatch=dict(generic=True), interleaved=False), 11),
    "generic_f32": ((33, 3, "float32"), dict(dispatch=dict(generic=True, no_col=True)), 7),
    "ns256_f32": ((256, 2, "float32"), dict(), 5),
    "ns256_f32_separate": ((256, 2, "float32"), dict(interleaved=False), 5),
    "ns256_f64": ((256, 2, "float64"), dict(), 5),
    "ns256_f64_separate": ((256, 2, "float64"), dict(interleaved=False), 5),
}


@pytest.mark.parametrize("family", sorted(NS_FAMILIES))
def test_ns_first_sweeps(family):
    """Every tiled or LDS-resident kernel family at its smallest supported grid with K = 0, 1 and 2 pressure sweeps -- the sweeps in
    which the second LDS buffer of a double-buffered exchange has not been written -- and at a larger K (the contract suite's own; 5 on
    the 256 x 256 grid), two steps."""
    C = _C()
    (n, B, dtype), kw, K_own = NS_FAMILIES[family]
    dt = getattr(torch, dtype)
    _runs(lambda: [C._ns_pair(n, B, K, dt, steps=2 if K == K_own else 1, **kw)[1] for K in (0, 1, 2, K_own)],
          "pdegym_ns2d_step_f" + dtype[-2:], "pdegym_ns2d_reset_masked_f" + dtype[-2:])


def test_ns_pressure_resets_and_rollout():
    C = _C()

    def fn():
        for dtype in ("float32", "float64"):
            C.test_ns_solve_pressure_contract(dtype)
        C.test_ns_masked_reset_leaves_others_alone()
        C.test_ns_auto_reset_final_obs()
        C.test_ns_rollout_contract()
    _runs(fn, *(f"pdegym_ns2d_{e}_{sfx}" for e in ("solve_pressure", "reset_masked", "rollout", "step") for sfx in ("f32", "f64")), outputs=False)


# form -> (n, dtype name, dispatch): the three Jacobi forms of ns_generic_pressure (pdegym_ns2d.hip: lds_jacobi_mode)
NS_PRESSURE_FORMS = {
    "two_lds_copies_f64": (40, "float64", {}),
    "two_lds_copies_f32": (40, "float32", {}),
    "two_lds_copies_21_f64": (21, "float64", {}),
    "one_lds_copy_f64": (100, "float64", {}),
    "one_lds_copy_f32": (100, "float32", {}),
    "global_memory_f64": (40, "float64", dict(no_lds_jacobi=True)),
}


@pytest.mark.parametrize("form", sorted(NS_PRESSURE_FORMS))
def test_ns_solve_pressure_forms(form):
    """pdegym_ns2d_solve_pressure with K = 0, 1, 2 and 13 sweeps in each Jacobi form -- two LDS copies (n = 21, 40), one LDS copy
    (n = 100), global memory -- and the pressure it returns compared bit for bit between the undirtied and the dirtied runs."""
    from pdecontrolgym_amd import _native as N
    from pdecontrolgym_amd.batch2d import NSBatch2D
    from tests.test_gpu_ns2d import _random_case, BC_MIX
    n, dtype, dispatch = NS_PRESSURE_FORMS[form]
    dt = getattr(torch, dtype)

    def fn():
        out = []
        with N.ns_dispatch(**dispatch):
            for K in (0, 1, 2, 13):
                kw, u0, v0, p0, _ = _random_case(n, 3, K, 5, BC_MIX)
                env = NSBatch2D(num_envs=3, device="cuda", dtype=dt, **kw)
                out.append(env.solve_pressure(u0, v0, p0))
        return out
    _runs(fn, "pdegym_ns2d_solve_pressure_f" + dtype[-2:])


def test_ns_adjoint_march():
    """The adjoint march keeps lambda in wave-private LDS: 8 and 21 rows, against the fixture bit for bit and under the output contract."""
    from tests import adjoint_restatement as R
    from tests import test_gpu_adjoint as A
    fx = R.load_fixture()

    def fn():
        for name in ("n8_K3_T1", "n21_K2_T6"):
            A.test_march_on_the_fixture_trajectory_is_bitwise(fx, name)
            A.test_outputs_are_fully_written_and_inputs_left_alone(fx, name)
        A.test_lam_is_optional(fx)
    _runs(fn, "pdegym_ns2d_adjoint_f64", outputs=False)


# ------------------------------------------------------------------------------------------------------- traffic and tumour

def _traffic_run(M, B, sim):
    """Reset and six steps (T / dt = 2: three episode ends) of a freeway of M nodes; everything the calls return and the state."""
    from pdecontrolgym_amd.batch_traffic import TrafficBatch
    env = TrafficBatch(0.5, 0.25, 10 * (M - 1), 10, sim, 40, 0.16, 60, True, 3, num_envs=B, device="cuda")
    assert env.M == M
    rs = np.random.default_rng([M, B]).uniform(0.1, 0.14, B)
    env.reset(rs)
    out = [_snapshot(env)]
    A = 2 if sim == "both" else 1
    rng = np.random.default_rng(2)
    for s in range(6):
        a = rng.uniform(0.9, 1.1, (B, A)) * env.t["qs_clip"].cpu().numpy()[:, None]
        ret = env.step(a if A == 2 else a[:, 0])
        out.append(_snapshot([list(ret), env]))
    return out


@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("M", [51, 65, 1024])
def test_traffic_rows(M, B):
    """The register kernel (M = 51) and the wide rows in LDS at their shortest (65: one node past a wave) and longest (1024: one
    wave per workgroup), every simulation type; all three patterns (the rows feed comparisons and the done flags)."""
    _runs(lambda: [_traffic_run(M, B, sim) for sim in ("outlet", "both", "inlet")], "pdegym_traffic_step", "pdegym_traffic_reset_masked",
          patterns=INTEGER_PATTERNS)


@pytest.mark.parametrize("wide", [False, True])
def test_traffic_contract(wide):
    C = _C()
    _runs(lambda: [C.test_traffic_contract(B, wide) for B in (1, 5)], "pdegym_traffic_step", "pdegym_traffic_reset_masked", outputs=False)


def test_traffic_rollout():
    C = _C()
    _runs(C.test_traffic_rollout_contract, "pdegym_traffic_rollout", "pdegym_traffic_step", "pdegym_traffic_reset_masked", outputs=False)


def test_traffic_backstepping():
    from tests import test_gpu_traffic_backstep as TB

    def fn():
        for M in (51, 200):
            for order in ("numpy", "tree") if M == 51 else ("tree",):
                TB.test_control_kernel_against_the_restatement(M, order)
            TB.test_control_writes_exactly_its_outputs(M, "both")
        TB.test_rollout_writes_exactly_its_outputs("numpy", "outlet")
        TB.test_one_launch_equals_two_launches("tree", "both", 2)
    _runs(fn, "pdegym_traffic_backstep_control", "pdegym_traffic_backstep_rollout", "pdegym_traffic_step", "pdegym_traffic_reset_masked",
          outputs=False)


def _tumor_run(nx_big, B):
    """Reset, three therapy days, the advance modes and an episode run to its end; state and outputs after every call."""
    from pdecontrolgym_amd import _native as N
    from tests.test_tumor import tumor_ic
    C = _C()
    env, X = C._tumor(nx_big, B)
    env.reset(tumor_ic(X, env.nx))
    out = [_snapshot(env)]
    rng = np.random.default_rng([B, 5])
    active = np.ones(B, np.uint8)
    for s in range(3):
        env.step(rng.uniform(0, 1, B), active=active)
        out.append(_snapshot(env))
    for mode, days in ((N.TUMOR_RUN_GROWTH, 5), (N.TUMOR_RUN_POST, 5), (N.TUMOR_RUN_TO_END, 5), (N.TUMOR_RUN_ONE_DAY, 5),
                       (N.TUMOR_RUN_TO_END, env.nt)):
        if mode == N.TUMOR_RUN_ONE_DAY:
            env.t["control"].zero_()
        env.advance(mode, days, active=active)
        out.append(_snapshot(env))
    return out


@pytest.mark.parametrize("B", [1, 7])
def test_tumor_step_and_advance(B):
    """The step and advance kernels keep each patient's row, and with it what the stage machine decides on, in LDS: both row-staging
    paths at B = 1 and 7 (a last workgroup with idle waves), all three patterns."""
    _runs(lambda: [_tumor_run(big, B) for big in (False, True)], "pdegym_tumor_step", "pdegym_tumor_advance", "pdegym_tumor_reset_masked",
          patterns=INTEGER_PATTERNS)


@pytest.mark.parametrize("nx_big", [False, True])
def test_tumor_contract(nx_big):
    C = _C()
    _runs(lambda: C.test_tumor_contract(nx_big), "pdegym_tumor_step", "pdegym_tumor_advance", "pdegym_tumor_reset_masked", outputs=False)


@pytest.mark.parametrize("with_policy", [False, True])
def test_tumor_rollout(with_policy):
    """pdegym_tumor_rollout and pdegym_tumor_therapy_step under the output contract, and an episode of the reference's own wrapper
    (the golden file) through the fused step at B = 1 and 5."""
    from tests import test_gpu_tumor_rollout as TR
    from tests.conftest import load_golden
    golden = load_golden("tumor")

    def fn():
        TR.test_output_contract_on_poisoned_guarded_buffers(with_policy)
        if not with_policy:
            TR.test_therapy_step_on_guarded_buffers(70, 300, False)
            for n in (1, 5):
                TR.test_fused_step_reproduces_the_reference_wrapper(golden, TR.WRAP_CASES[0], n)
    _runs(fn, "pdegym_tumor_rollout", "pdegym_tumor_reset_masked", "pdegym_tumor_advance", *(() if with_policy else ("pdegym_tumor_therapy_step",)),
          patterns=INTEGER_PATTERNS, outputs=False)


# ------------------------------------------------------------------------------------------- the policy inside the rollout kernels

def _policy_rollout_cases():
    """Exactly summable networks (tests/mlp_exact.py) at the smallest shapes with live padding in LDS.  Narrow path (``eval``, up to 64
    units): observation rows of 5 and 101 values (no multiple of four), the freeway's 102, the tumour's float64 rows of 70; hidden
    layers of 1, 33 and 63 units; B = 1 and 5.  Cooperative path (``eval_wide``): hidden layers of 65 and 130 units on rows of 101, B = 1
    (a tile with a single live row) and 17 (a last tile with 15 dead rows).  Noise and a binding clamp throughout."""
    from tests import mlp_exact as mx
    P, T = "PDEControlGym-ReactionDiffusionPDE1D", "PDEControlGym-TransportPDE1D"
    c = []

    def add(name, k, hidden, B, env, **kw):
        acts = tuple(None if h == 1 else "relu" for h in hidden) + (None,)      # (a closed ReLU in a layer of one unit would blind the case)
        A = 2 if env == ("traffic", "both") else 1
        c.append(mx.Case(name, (k,) + tuple(hidden) + (A,), acts, B, seed=5000 + len(c), noise=True, clamp=True, env=env, **kw))

    for i, (n, H, B) in enumerate((n, H, B) for n in (5, 101) for H in (1, 33, 63) for B in (1, 5)):
        kind = (P, T)[i % 2]
        add(f"lds-{'rd' if kind == P else 'tr'}{n}-{H}-B{B}", n, (H,), B, ("1d", kind, "Dirchilet", "full", n))
    add("lds-rd101-33-63-B5", 101, (33, 63), 5, ("1d", P, "Dirchilet", "full", 101))
    for H in (1, 33, 63):
        for B in (1, 5):
            add(f"lds-traffic-both-{H}-B{B}", 102, (H,), B, ("traffic", "both"), unit=0.25, xlo=2, xhi=6, eps=True)
            add(f"lds-tumor70-{H}-B{B}", 70, (H,), B, ("tumor", 70), xlo=0, xhi=4, eps=True)
    for H in (65, 130):
        for B in (1, 17):
            add(f"lds-tr101-wide-{H}-B{B}", 101, (H,), B, ("1d", T, "Dirchilet", "full", 101))
    add("lds-rd101-wide-65-130-B17", 101, (65, 130), 17, ("1d", P, "Dirchilet", "full", 101))
    # the general kernels (Neumann actuation; scalar sensing) stage their own input row: full rows of 101 values and rows of one value
    Nm, col = "Neumann", "collocated"
    add("lds-general-rd101-neumann-33-B1", 101, (33,), 1, ("1d", P, Nm, "full", 101))
    add("lds-general-rd101-neumann-63-B5", 101, (63,), 5, ("1d", P, Nm, "full", 101))
    add("lds-general-rd101-neumann-1-B17", 101, (1,), 17, ("1d", P, Nm, "full", 101))
    add("lds-general-rd101-neumann-wide-65-B17", 101, (65,), 17, ("1d", P, Nm, "full", 101))
    add("lds-general-rd101-neumann-wide-130-B1", 101, (130,), 1, ("1d", P, Nm, "full", 101))
    add("lds-general-tr100-scalar-1-B1", 1, (1,), 1, ("1d", T, "Dirchilet", col, 100))
    add("lds-general-tr100-scalar-33-B5", 1, (33,), 5, ("1d", T, "Dirchilet", col, 100))
    add("lds-general-rd101-neumann-scalar-63-B17", 1, (63,), 17, ("1d", P, Nm, col, 101))
    add("lds-general-tr100-scalar-wide-65-B17", 1, (65,), 17, ("1d", T, "Dirchilet", col, 100))
    add("lds-general-rd101-neumann-scalar-wide-130-B5", 1, (130,), 5, ("1d", P, Nm, col, 101))
    add("lds-traffic-both-wide-65-B1", 102, (65,), 1, ("traffic", "both"), unit=0.25, xlo=2, xhi=6, eps=True)
    add("lds-tumor70-wide-130-B17", 70, (130,), 17, ("tumor", 70), xlo=0, xhi=4, eps=True)
    return c


def _gaussian_rollout_cases():
    """The squashed-Gaussian head inside the same kernels (tests/gaussian_exact.py), with noise and the action box."""
    from tests import gaussian_exact as gx
    P, T = "PDEControlGym-ReactionDiffusionPDE1D", "PDEControlGym-TransportPDE1D"
    r = "relu"
    tr = dict(unit=0.25, xlo=2, xhi=6, eps_in=True)
    tu = dict(xlo=0, xhi=4, eps_in=True)
    specs = [("lds-g-rd5-33-B1", (5, 33, 1), (r,), 1, ("1d", P, "Dirchilet", "full", 5), {}),
             ("lds-g-tr101-63-B5", (101, 63, 1), (r,), 5, ("1d", T, "Dirchilet", "full", 101), {}),
             ("lds-g-traffic-both-33-B5", (102, 33, 2), (r,), 5, ("traffic", "both"), tr),
             ("lds-g-tumor70-63-B1", (70, 63, 1), (r,), 1, ("tumor", 70), tu),
             ("lds-g-tr101-wide-65-B17", (101, 65, 1), (r,), 17, ("1d", T, "Dirchilet", "full", 101), {}),
             ("lds-g-rd101-wide-130-B1", (101, 130, 1), (r,), 1, ("1d", P, "Dirchilet", "full", 101), {}),
             ("lds-g-traffic-both-wide-130-B17", (102, 130, 2), (r,), 17, ("traffic", "both"), tr),
             ("lds-g-tumor70-wide-65-B5", (70, 65, 1), (r,), 5, ("tumor", 70), tu),
             # the general kernels: Neumann actuation on full rows, scalar sensing
             ("lds-g-general-rd101-neumann-33-B5", (101, 33, 1), (r,), 5, ("1d", P, "Neumann", "full", 101), {}),
             ("lds-g-general-tr100-scalar-63-B1", (1, 63, 1), (r,), 1, ("1d", T, "Dirchilet", "collocated", 100), {}),
             ("lds-g-general-rd101-neumann-wide-65-B17", (101, 65, 1), (r,), 17, ("1d", P, "Neumann", "full", 101), {}),
             ("lds-g-general-tr100-scalar-wide-130-B5", (1, 130, 1), (r,), 5, ("1d", T, "Dirchilet", "collocated", 100), {})]
    return [gx.GCase(name, sizes, acts, B, seed=6000 + i, env=env, **kw) for i, (name, sizes, acts, B, env, kw) in enumerate(specs)]


POLICY_ROLLOUT_CASES = _policy_rollout_cases()
GAUSSIAN_ROLLOUT_CASES = _gaussian_rollout_cases()
def _rollout_entries(case, forward):
    """Every entry point a rollout case goes through: the engine's reset (the tumour wrapper's reset also advances to the therapy
    stage), the rollout, and -- ``forward`` -- pdegym_mlp_forward, which the case compares the in-kernel evaluation with."""
    if case.env[0] == "1d":
        e = ("pdegym_parabolic_rollout" if "Reaction" in case.env[1] else "pdegym_transport_rollout", "pdegym_reset1d_masked")
    elif case.env[0] == "traffic":
        e = ("pdegym_traffic_rollout", "pdegym_traffic_reset_masked")
    else:
        e = ("pdegym_tumor_rollout", "pdegym_tumor_reset_masked", "pdegym_tumor_advance")
    return e + (("pdegym_mlp_forward",) if forward else ())


@pytest.mark.parametrize("case", POLICY_ROLLOUT_CASES, ids=[c.name for c in POLICY_ROLLOUT_CASES])
def test_policy_inside_the_rollouts_with_live_padding(case):
    """actions[0] equals the float64 expectation exactly (and, past 64 units, pdegym_mlp_forward's bits): a pad that is read as
    0 * residue is a NaN under "nan" and stays 0 under "huge" only if it was written."""
    from tests import test_gpu_mlp_exact as ME
    _runs(lambda: ME.test_policy_inside_the_rollout_kernels_is_exact(case), *_rollout_entries(case, max(case.sizes[1:]) > 64), outputs=False)


@pytest.mark.parametrize("case", GAUSSIAN_ROLLOUT_CASES, ids=[c.name for c in GAUSSIAN_ROLLOUT_CASES])
def test_gaussian_policy_inside_the_rollouts_with_live_padding(case):
    from tests import test_gpu_gaussian_head as GH
    _runs(lambda: GH.test_evaluators_inside_the_rollout_kernels(case), *_rollout_entries(case, True), outputs=False)


# --------------------------------------------------------------------------------------------------------- the network kernels

MLP_K = (1, 5, 17)
MLP_WIDTHS = (1, 15, 17, 65, 129)
MLP_BATCHES = (1, 15, 17, 33)


def forward_cases(width):
    """K x B of the grid at one hidden width: ``xs`` and ``hbuf`` are zero beyond the width up to a multiple of 16, rows past the batch
    read as zero.  The variant (float64 rows in / out, row gaps, bias, noise, clamp) walks along."""
    from tests import mlp_exact as mx
    act = None if width == 1 else "relu"
    return [mx.Case(f"lds-K{K}-W{width}-B{B}", (K, width, 3), (act, None), B, seed=7000 + 97 * width + 7 * K + B, **mx._variant((i + width) % 8))
            for i, (K, B) in enumerate((K, B) for K in MLP_K for B in MLP_BATCHES)]


def backward_cases(width):
    """The same grid for the backward passes (tests/mlp_backward_exact.py); widths of up to 64 units go to pdegym_mlp_backward, wider
    ones to pdegym_mlp_backward_wide."""
    from tests import mlp_backward_exact as R
    act = None if width == 1 else "relu"
    out = []
    for i, (K, B) in enumerate((K, B) for K in MLP_K for B in MLP_BATCHES):
        ok = R.valid_slabs(B)
        out.append(R.Case(f"lds-K{K}-W{width}-B{B}", (K, width, 3), (act, None), B, ok[i % len(ok)], seed=8000 + 97 * width + 7 * K + B,
                          nnz=(16, 16), **R._variant((i + width) % 8)))
    return out


@pytest.mark.parametrize("width", MLP_WIDTHS)
def test_mlp_forward_with_live_padding(width):
    from tests import test_gpu_mlp_exact as ME
    cases = forward_cases(width)
    _runs(lambda: [ME.test_forward_kernel_is_exact(c) for c in cases], "pdegym_mlp_forward", outputs=False)


def test_gaussian_forward():
    """The squashed-Gaussian epilogue of pdegym_mlp_forward on the forward cases of one and of eight actuators."""
    from tests import gaussian_exact as gx
    from tests import test_gpu_gaussian_head as GH
    cases = [c for c in gx.FORWARD_CASES if c.A in (1, 8)][:8]
    assert len(cases) >= 4
    _runs(lambda: [GH.test_forward_kernel_against_the_float64_expectation(c) for c in cases], "pdegym_mlp_forward", outputs=False)


def _backward_outputs(MB, R, case):
    b = R.build(case)
    net = b.net.cuda()
    got = MB._launch(net, b.x_dev, b.dy, case.x_f64, case.gaps, case.dx, case.slabs)
    assert (got["dx"] is not None) == case.dx
    want = b.want if case.dx else dict(b.want, dx=None)
    MB._assert_equal(case.name, got, want, f"(slabs = {case.slabs})")
    return got


@pytest.mark.parametrize("width", [w for w in MLP_WIDTHS if w <= 64])
def test_mlp_backward_with_live_padding(width):
    """dw, db and dx equal the float64 expectation exactly (the module's own launcher and comparison) and agree between the runs."""
    from tests import mlp_backward_exact as R
    from tests import test_gpu_mlp_backward as MB
    cases = backward_cases(width)
    _runs(lambda: [_backward_outputs(MB, R, c) for c in cases], "pdegym_mlp_backward")


@pytest.mark.parametrize("width", [w for w in MLP_WIDTHS if w > 64])
def test_mlp_backward_wide_with_live_padding(width):
    from tests import mlp_backward_exact as R
    from tests import test_gpu_mlp_backward_wide as MW
    cases = backward_cases(width)
    _runs(lambda: [_backward_outputs(MW, R, c) for c in cases], "pdegym_mlp_backward_wide")


# ----------------------------------------------------------------------------------------------------------- the training heads

SMALL_N = (1, 2, 63, 65)      # fewer live waves (and workgroups) than reduction slots


@pytest.mark.parametrize("T,B", [(5, 3), (33, 70)])
def test_gae(T, B):
    from tests import test_gpu_gae as G

    def fn():
        out = []
        for f64 in (False, True):
            rew, val, te, tr, boot = G._case(T, B, f64)
            got = G._launch(rew, val, te, tr, boot, 0.99, 0.95)
            G._assert_same(got, G._expect(rew, val, te, tr, boot, 0.99, 0.95), ("lds", f64))
            out.append(got)
        return out
    _runs(fn, "pdegym_gae")


@pytest.mark.parametrize("A", [1, 8])
def test_ppo_loss_with_few_live_waves(A):
    """N = 1, 2, 63, 65: the value gradient has the restatement's bits, every output of the head and of the log-probability launch
    agrees between the runs."""
    from tests import ppo_loss_restatement as R
    from tests import test_gpu_ppo_loss as P

    def fn():
        out = []
        for n in SMALL_N:
            for normalize in (False, True):
                case, index = P._case(n, A, seed=n)
                got = P._launch(case, index, normalize=normalize, pad=(3, 1, 2))
                want = R.head_float32(*P._args(case), P.CLIP, P.ENT, P.VF, normalize, index=index)
                np.testing.assert_array_equal(P._bits(got["d_values"]), P._bits(want["d_values"]))
                out.append(got)
            out.append(P._launch_log_prob(case, index, pad=(1, 2)))
        return out
    _runs(fn, "pdegym_ppo_loss", "pdegym_diag_gaussian_log_prob")


@pytest.mark.parametrize("two", [True, False], ids=["twin", "single"])
def test_sac_losses_with_few_live_waves(two):
    """N = 1, 2, 63, 65 on integer data: gradients, target and statistics of the critic head have the restatement's bits; the actor
    head's outputs agree between the runs."""
    from tests import sac_loss_restatement as R
    from tests import test_gpu_sac_loss as S

    def fn():
        out = []
        for n in SMALL_N:
            case, index = S._integer_critic_case(n, seed=n)
            got = S._critic(case, index, two=two, log_alpha=0.0, gamma=0.5)
            want = R.critic_float32(*S._critic_args(case, two), 0.0, 0.5, index=index)
            for k in ("d_q1", "target", "stats") + (("d_q2",) if two else ()):
                np.testing.assert_array_equal(S._bits(got[k]), S._bits(want[k]), err_msg=f"{k} n={n}")
            lp = {"q1": case["q1"], "q2": case["q2"], "log_prob": case["next_log_prob"]}
            out += [got, S._actor(lp, two=two, log_alpha=-0.5)]
        return out
    _runs(fn, "pdegym_sac_critic_loss", "pdegym_sac_actor_loss")


@pytest.mark.parametrize("A", [1, 8])
def test_sac_sample_and_backward(A):
    from tests import sac_loss_restatement as R
    from tests import test_gpu_sac_loss as S

    def fn():
        out = []
        for n in SMALL_N:
            case = R.seeded_sample_case(n, A, seed=n + A)
            rng = np.random.default_rng(n)
            d_a = rng.normal(0.0, 1.0, (n, A)).astype(np.float32)
            d_lp = rng.normal(0.0, 1.0, n).astype(np.float32)
            out += [S._sample(case, pad=(2, 0, 0, 1)), S._backward(case, d_a, d_lp, pad=(1, 2, 3))]
        return out
    _runs(fn, "pdegym_squashed_gaussian_sample", "pdegym_squashed_gaussian_sample_backward")


@pytest.mark.parametrize("clip", ["off", "active"])
@pytest.mark.parametrize("name", ["one", "wave"])
def test_fused_adam_with_few_live_waves(name, clip):
    """The tensor lists of one element and of 3 + 64 + 65: three steps equal the float32 restatement bit for bit (the module's runner)."""
    from tests import test_gpu_fused_adam as F

    def fn():
        shapes = F.TENSOR_LISTS[name]
        rng = np.random.default_rng(len(shapes) + 7)
        case = F.make_case(shapes, rng)
        grads = [F.exact_grads(shapes, rng) for _ in range(3)]
        return F._run(case, grads, {"off": None, "active": 0.5}[clip], (False, True, True))
    _runs(fn, "pdegym_fused_adam")
