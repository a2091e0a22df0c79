"""CPU tests of the backstepping law inside the one-launch 1D rollout (csrc/pdegym_backstep_rollout.hip, pdegym_*_backstep_rollout):
the host path from ``DeviceRollout(venv, controller, T, one_launch=True)`` down to ONE backend call with the right descriptor, on the
oracle-backed double of tests/fake_backstep_backend.py; the errors that say what is missing; the kernel table of the GPU module; the
DPP wait states of the new code object; and tests/c/backstep_rollout_validation.c on the host half of the library under
AddressSanitizer and UBSan.  No kernel is launched."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

torch = pytest.importorskip("torch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
KEYS = ("obs", "actions", "rewards", "terminated", "truncated")
ENV_ID = {"transport": "PDEControlGym-TransportPDE1D", "parabolic": "PDEControlGym-ReactionDiffusionPDE1D"}


def _case(kind):
    from tests.test_gpu_backstepping import _pool_case
    return _pool_case(kind)


def _venv(case, backend, pools=True, **over):
    """The pool case of tests/test_gpu_backstepping.py (B = 6, P = 7, episodes of 3 env-steps of 5 sub-steps) on the CPU double."""
    import pde_control_gym
    from pde_control_gym.src import TunedReward1D
    from tests.test_gpu_backstepping import POOL_B
    (init, beta, _), (pinit, pbeta, _) = case["first"], case["pool"]
    nt_r = int(round(case["grid"]["T"] / case["grid"]["dt"]))
    params = dict(case["grid"], reward_class=TunedReward1D(nt_r, -1e3, 3e2), normalize=False, sensing_loc="full", control_type="Dirchilet",
                  sensing_type=None, limit_pde_state_size=True, max_state_value=1e10, max_control_value=20,
                  batched_reset_func=lambda idx, nx: (init[idx], beta[idx]))
    params.update(over)
    venv = pde_control_gym.make_vec(ENV_ID[case["kind"]], num_envs=POOL_B, device="cpu", backend=backend, **params)
    venv.reset_tensor()
    if pools:
        venv.enable_fused_auto_reset(init_pool=pinit, beta_pool=pbeta)
    return venv


def _ctrl(case, backend, venv=None, pools=True):
    from pde_control_gym import BacksteppingController
    c = BacksteppingController(case["kind"], case["first"][2], case["dx"], pool_theta=case["pool"][2] if pools else None, order="ordered",
                               device="cpu", backend=backend)
    return c if venv is None else c.attach(venv)


def _runs(case, one_launch, runs=2, **kw):
    from pde_control_gym import DeviceRollout
    from tests.fake_backstep_backend import FakeBackstepBackend
    from tests.test_gpu_backstepping import CLAMP, POOL_T
    bk = FakeBackstepBackend()
    venv = _venv(case, bk)
    ctrl = _ctrl(case, bk, venv)
    ro = DeviceRollout(venv, ctrl, POOL_T, use_graph=False, action_low=CLAMP[0], action_high=CLAMP[1], one_launch=one_launch, **kw)
    snaps, calls = [], []
    for r in range(runs):
        if ro.action_noise is not None:
            ro.action_noise.copy_(torch.from_numpy(np.random.default_rng(40 + r).normal(0, 3, tuple(ro.action_noise.shape)).astype(f32)))
        if ro.sensing_noise is not None:
            ro.sensing_noise.copy_(torch.from_numpy(np.random.default_rng(50 + r).normal(0, 0.5, tuple(ro.sensing_noise.shape)).astype(f32)))
        del bk.calls[:]
        ro.run()
        calls.append(list(bk.calls))
        snap = {k: getattr(ro, k).numpy().copy() for k in KEYS}
        snap["obs_seen"] = None if ro.obs_seen is None else ro.obs_seen.numpy().copy()
        snap["state"] = {k: venv.core.t[k].numpy().copy() for k in ("time_index", "reset_count", "bsum", "ring", "obs", "beta")}
        snaps.append(snap)
    return venv, ctrl, ro, snaps, calls


# ---- one backend call per run, the right descriptor, the same buffers -------------------------------------------------------------
@pytest.mark.parametrize("kind", ["transport", "parabolic"])
def test_one_launch_true_is_one_backend_call_with_the_law_and_equals_the_two_launch_path(kind):
    """First check of this file: ``one_launch=True`` with an attached controller used to raise ValueError."""
    from pdecontrolgym_amd import _native as N
    from tests.test_gpu_backstepping import CLAMP, POOL_P, POOL_T
    case = _case(kind)
    venv, ctrl, ro, one, calls = _runs(case, True, action_noise=True, sensing_noise=True)
    assert ro.one_launch is True and venv.one_launch_law_fits(ctrl) is True and venv.one_launch_fits(ctrl) is False
    n, m = case["n"], case["m"]
    for run in range(2):
        assert [c[0] for c in calls[run]] == ["backstep_rollout"], calls[run]
        d = calls[run][0][1]
        assert d["kind"] == kind and d["T"] == POOL_T and d["m"] == m and d["gain_stride"] == m
        assert (d["len"], d["scale"]) == ((n, 1e-2) if kind == "transport" else (min(m, n - 1), case["dx"]))
        assert d["order"] == N.BACKSTEP_ORDERED
        assert d["gain0"] == ctrl.gain.data_ptr() and d["gain_pool"] == ctrl.pool_gain.data_ptr() and d["pool_rows"] == POOL_P
        assert d["reset_count"] == venv.core.t["reset_count"].data_ptr()
        assert d["noise"] == ro.action_noise.data_ptr() and (d["clamp"], d["lo"], d["hi"]) == (1,) + CLAMP
        assert d["obs"] is None and d["out64"] is None and d["out32"] is None and d["obs_noise"] and d["obs_seen"]
    _, _, ro2, two, calls2 = _runs(case, None, action_noise=True, sensing_noise=True)
    assert ro2.one_launch is False
    for run in range(2):
        assert [c[0] for c in calls2[run]] == ["control", "step"] * POOL_T
        for k in KEYS + ("obs_seen",):
            np.testing.assert_array_equal(one[run][k].view(np.uint8), two[run][k].view(np.uint8), err_msg=f"run {run}: {k}")
        for k, v in one[run]["state"].items():
            np.testing.assert_array_equal(v.view(np.uint8), two[run]["state"][k].view(np.uint8), err_msg=f"run {run}: state {k}")
        # every instance restarts at least twice per run, so the gains followed >= 2 restarts inside each call
        assert (one[run]["terminated"] | one[run]["truncated"]).sum(axis=0).min() >= 2
        # the law read the noisy rows; the observation slots stayed clean (they are the plant state)
        assert not np.array_equal(one[run]["obs_seen"], one[run]["obs"])
    assert one[1]["state"]["reset_count"].min() >= 4


def test_without_noise_or_pools_the_descriptor_leaves_them_unset():
    from pde_control_gym import BacksteppingController, DeviceRollout
    from pdecontrolgym_amd import _native as N
    from tests.fake_backstep_backend import FakeBackstepBackend
    case = _case("parabolic")
    bk = FakeBackstepBackend()
    venv = _venv(case, bk, pools=False)
    ctrl = BacksteppingController("parabolic", case["first"][2][0], case["dx"], order="tree", device="cpu", backend=bk).attach(venv)
    ro = DeviceRollout(venv, ctrl, 2, use_graph=False, one_launch=True)
    del bk.calls[:]
    ro.run()
    (name, d), = bk.calls
    assert name == "backstep_rollout" and d["gain_stride"] == 0 and d["gain_pool"] is None and d["reset_count"] is None and d["noise"] is None
    assert d["order"] == N.BACKSTEP_TREE and d["clamp"] == 1 and (d["lo"], d["hi"]) == (-1.0, 1.0) and not d["obs_noise"] and not d["obs_seen"]
    assert np.abs(ro.actions.numpy()).max() <= 1.0 and venv.core.t["time_index"].tolist() == [10] * 6


class _NoGains:
    """A backend whose gains are zeros (the m^2/2 NumPy additions of a 513-term transport gain are not what the test is about)."""

    def backstep_gain(self, kind, theta, gain, dx):
        gain.zero_()


# ---- what does not fit says why ----------------------------------------------------------------------------------------------------
def test_one_launch_true_says_what_is_missing():
    from pde_control_gym import BacksteppingController, DeviceRollout
    from tests.fake_backstep_backend import FakeBackstepBackend
    bk = FakeBackstepBackend()
    case, pcase = _case("transport"), _case("parabolic")
    venv = _venv(case, bk)
    # unattached
    with pytest.raises(ValueError, match="not attached"):
        DeviceRollout(venv, _ctrl(case, bk), 4, use_graph=False, one_launch=True)
    assert venv.one_launch_law_fits(_ctrl(case, bk)) is False
    # a controller of the other kind, attached to its own environment
    pvenv = _venv(pcase, bk)
    with pytest.raises(ValueError, match="parabolic controller is attached to another environment than this transport one"):
        DeviceRollout(venv, _ctrl(pcase, bk, pvenv), 4, use_graph=False, one_launch=True)
    # Neumann actuation
    nv = _venv(case, bk, control_type="Neumann")
    with pytest.raises(ValueError, match="Neumann actuation"):
        DeviceRollout(nv, _ctrl(case, bk, nv), 4, use_graph=False, one_launch=True)
    # rows of more than 513 nodes (parabolic: the law's length is min(m, n - 1), so a short theta row attaches)
    from pde_control_gym.src import TunedReward1D
    long = _venv(pcase, bk, pools=False, X=6, batched_reset_func=lambda idx, nx: (np.ones((len(idx), nx + 1), f32), np.ones((len(idx), nx + 1), f32)),
                 reward_class=TunedReward1D(15, -1e3, 3e2))
    assert long.core.n == 601
    lc = BacksteppingController("parabolic", np.linspace(1, 2, 8, dtype=f32), pcase["dx"], device="cpu", backend=bk).attach(long)
    with pytest.raises(ValueError, match="rows of 601 nodes"):
        DeviceRollout(long, lc, 4, use_graph=False, one_launch=True)
    # a transport row has no node outside the slots: 513 nodes would be 9 slots per lane (parabolic 513 = node 0 + 512 slots fits)
    tcase = dict(case, grid=dict(case["grid"], dx=1.0 / 513))
    init513 = lambda idx, nx: (np.ones((len(idx), nx), f32), np.ones((len(idx), nx), f32))      # noqa: E731
    t513 = _venv(tcase, bk, pools=False, batched_reset_func=init513)
    assert t513.core.n == 513
    tc = BacksteppingController("transport", np.linspace(1, 2, 513, dtype=f32)[None].repeat(6, 0), 1.0 / 513, device="cpu",
                                backend=_NoGains()).attach(t513)
    with pytest.raises(ValueError, match="rows of 513 nodes .*transport rows of up to 512"):
        DeviceRollout(t513, tc, 4, use_graph=False, one_launch=True)
    assert t513.one_launch_law_fits(tc) is False
    p513 = _venv(dict(pcase, grid=dict(pcase["grid"], dx=1.0 / 512)), bk, pools=False,
                 batched_reset_func=lambda idx, nx: (np.ones((len(idx), nx + 1), f32), np.ones((len(idx), nx + 1), f32)))
    assert p513.core.n == 513
    pc = BacksteppingController("parabolic", np.linspace(1, 2, 8, dtype=f32), 1.0 / 512, device="cpu", backend=bk).attach(p513)
    assert p513.one_launch_law_fits(pc) is True
    # the callable form of the sensing-noise hook has no place inside a kernel
    sv = _venv(case, bk, sensing_noise_tensor_func=lambda o: o * 1.5)
    with pytest.raises(ValueError, match="sensing_noise_tensor_func"):
        DeviceRollout(sv, _ctrl(case, bk, sv), 4, use_graph=False, one_launch=True)
    # something that is neither a FusedMLP nor a controller keeps today's message
    with pytest.raises(ValueError, match="FusedMLP"):
        DeviceRollout(venv, lambda o: o[:, 0], 4, use_graph=False, one_launch=True)
    # the default is unchanged: the controller does not claim the one-launch path, and nothing raises
    ok = _ctrl(case, bk, venv)
    assert venv.one_launch_fits(ok) is False and DeviceRollout(venv, ok, 4, use_graph=False).one_launch is False
    assert not hasattr(ok, "fits_rollout")
    # the engine's own entry refuses as well
    with pytest.raises(ValueError, match="Neumann actuation"):
        nv.core.rollout(*(torch.zeros(1),) * 5, policy=_ctrl(case, bk, nv))


def test_binding_and_header_declare_the_two_entry_points():
    from pdecontrolgym_amd import _native as N
    from pdecontrolgym_amd import build
    hdr = open(os.path.join(ROOT, "include", "pdegym.h")).read()
    for name in ("pdegym_transport_backstep_rollout", "pdegym_parabolic_backstep_rollout"):
        assert name in N.EXPORTS and re.search(name + r"\(const pdegym_params1d\* prm, const pdegym_bufs1d\* buf, const pdegym_rollout1d\* ro,\s*"
                                               r"const pdegym_backstep\* law, int32_t B, void\* stream\);", hdr)
    assert "pdegym_backstep_rollout.hip" in build.SOURCES


# ---- the kernel table ---------------------------------------------------------------------------------------------------------------
def test_every_backstep_rollout_kernel_has_an_output_contract_test():
    """The kernels of csrc/pdegym_backstep_rollout.hip keep their poisoned-buffer tests in tests/test_gpu_backstep_rollout.py: every
    kernel launched there (chevron syntax) is listed in its KERNEL_CASES, and every test named exists."""
    from tests import test_gpu_backstep_rollout as G
    src = open(os.path.join(ROOT, "pdecontrolgym_amd", "csrc", "pdegym_backstep_rollout.hip")).read()
    launched = set(re.findall(r"([A-Za-z_]\w*)\s*<[^<>;]*>\s*<<<", src))
    assert "hipLaunchKernelGGL" not in src
    assert launched == set(G.KERNEL_CASES) and len(launched) == 1, launched ^ set(G.KERNEL_CASES)
    for k, tests in G.KERNEL_CASES.items():
        assert tests and all(callable(getattr(G, t, None)) for t in tests), (k, tests)


# ---- static check of the new code object ------------------------------------------------------------------------------------------
def test_every_dpp_instruction_of_the_new_unit_has_its_wait_states(tmp_path):
    """The new unit instantiates the ROLL stencil's hand-counted asm blocks (pdegym_1d_body.h); tests/test_static_asm.py lists the
    units it checks, so this one is checked here with the same checker."""
    from pdecontrolgym_amd import build
    from tests.test_static_asm import OBJDUMP, _check, _disassemble
    if not os.path.exists(OBJDUMP):
        pytest.skip("llvm-objdump of the ROCm toolchain not found")
    build.build()
    n_dpp, bad = _check(_disassemble(os.path.join(build.LIBDIR, "pdegym_backstep_rollout.o"), str(tmp_path)))
    assert n_dpp > 10, f"only {n_dpp} DPP instructions found -- did the disassembly format change?"
    assert not bad, "\n".join(bad[:20])


# ---- argument validation of the two entry points, host half under ASan + UBSan ------------------------------------------------------
@pytest.mark.skipif(shutil.which("hipcc") is None, reason="needs hipcc")
def test_backstep_rollout_entry_points_validate_their_arguments_under_asan_and_ubsan(tmp_path):
    """tests/c/backstep_rollout_validation.c (its own main) against the host half of pdegym_backstep_rollout.hip + pdegym_abi.hip,
    compiled with --cuda-host-only and the sanitizers and given an empty device image: every bad call must answer with a negative
    code and a message, and no call reaches a device."""
    from pdecontrolgym_amd import build
    from tests.test_backstepping import SAN
    hipcc = shutil.which("hipcc")
    inc = ["-I" + os.path.join(ROOT, "include"), "-I" + build.CSRC]
    objs = []
    for s in ("pdegym_abi.hip", "pdegym_backstep_rollout.hip"):
        o = str(tmp_path / s.replace(".hip", ".o"))
        r = subprocess.run([hipcc, "--offload-arch=gfx950", "--cuda-host-only", "-O1", "-g", "-std=c++17", "-fPIC"]
                           + SAN + inc + ["-c", os.path.join(build.CSRC, s), "-o", o],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        assert r.returncode == 0, r.stdout.decode()[-3000:]
        objs.append(o)
    nm = subprocess.run(["nm", "-u"] + objs, stdout=subprocess.PIPE, check=True).stdout.decode()
    names = sorted({ln.split()[-1] for ln in nm.splitlines() if "__hip_fatbin_" in ln})
    stub = tmp_path / "empty_fatbins.c"
    stub.write_text("".join(f'__attribute__((aligned(4096))) const char {n}[4096] = "__CLANG_OFFLOAD_BUNDLE__";\n' for n in names))
    stub_o = str(tmp_path / "empty_fatbins.o")
    subprocess.run(["gcc", "-c", "-fPIC", str(stub), "-o", stub_o], check=True)
    lib = str(tmp_path / "libpdegym_backstep_rollout_asan.so")
    r = subprocess.run([hipcc, "-shared", "-fPIC"] + SAN + ["-o", lib] + objs + [stub_o], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()[-3000:]
    exe = str(tmp_path / "backstep_rollout_validation")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    r = subprocess.run([hipcc, "-x", "c", "-std=c11", "-Wall", "-Werror", "-g"] + SAN
                       + [os.path.join(ROOT, "tests", "c", "backstep_rollout_validation.c"), "-I" + os.path.join(ROOT, "include"),
                          "-L" + str(tmp_path), "-lpdegym_backstep_rollout_asan", "-Wl,-rpath," + str(tmp_path),
                          "-Wl,-rpath," + os.path.join(rocm, "lib"), "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1", HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, env=env, timeout=120)
    out = r.stdout.decode()
    assert r.returncode == 0 and "BACKSTEP-ROLLOUT-VALIDATION-OK" in out, out[-4000:]
    assert "runtime error" not in out and "AddressSanitizer" not in out, out[-4000:]
    assert int(re.search(r"calls (\d+) bad 0", out).group(1)) >= 150
