"""CPU tests of the one-launch TherapyWrapper paths (csrc/pdegym_tumor_rollout.hip: pdegym_tumor_therapy_step, pdegym_tumor_rollout):
the host path from ``TumorVecEnv(fused_step=True)`` and ``DeviceRollout(venv, policy, T, one_launch=True)`` down to the backend calls,
on the oracle-backed double of tests/fake_tumor_rollout_backend.py (an independent restatement of the wrapper step); the errors that
say what is missing; exports, build list and ABI number; the kernel table of the GPU module; and tests/c/tumor_rollout_validation.c
on the host half of the new unit under AddressSanitizer and UBSan.  No kernel is launched."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests.test_tumor import KW, tumor_ic

torch = pytest.importorskip("torch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, STEPS = 17, 24


def _venv(backend, T=600, weekends=False, fused=False, num_envs=B, **extra):
    import pde_control_gym
    from pde_control_gym.src import BrainTumorReward
    venv = pde_control_gym.make_vec("PDEControlGym-BrainTumor1D", num_envs=num_envs, weekends=weekends, device="cpu", backend=backend,
                                    fused_step=fused, T=T, reward_class=BrainTumorReward(), reset_init_condition_func=tumor_ic, **{**KW, **extra})
    venv.benchmark()
    venv.reset_tensor()
    return venv


def _actions(steps=STEPS, n=B):
    rng = np.random.default_rng(5)
    hi = np.linspace(0.03, 0.3, n)
    return [rng.uniform(0.2, 1, n) * hi for _ in range(steps)]


def _state(venv):
    t = venv.core.t
    return {**{k: t[k].clone() for k in ("u", "time_index", "stage", "remaining", "days", "out")},
            "calls": venv.treatment_calls.clone(), "viol": venv.soft_constraint_violations.clone(), "cons": venv._consecutive.clone()}


def _loop(venv, acts):
    out = []
    for a in acts:
        obs, rew, term, trunc = venv.step_tensor(torch.from_numpy(a))
        done = term | trunc
        out.append([obs.clone(), rew.clone(), term.clone(), trunc.clone(), venv.terminal_obs[done].clone(), _state(venv)])
    return out


def _same(a, b, msg=""):
    if isinstance(a, dict):
        for k in a:
            _same(a[k], b[k], f"{msg} {k}")
    else:
        np.testing.assert_array_equal(a.numpy(), b.numpy(), err_msg=msg)


@pytest.mark.parametrize("T", [600, 300])
@pytest.mark.parametrize("weekends", [False, True])
def test_fused_step_equals_the_launch_sequence_on_the_double_and_every_branch_is_reached(T, weekends):
    from tests.fake_tumor_rollout_backend import FakeTumorRolloutBackend
    plain_bk, fused_bk = FakeTumorRolloutBackend(), FakeTumorRolloutBackend()
    plain, fused = _venv(plain_bk, T, weekends), _venv(fused_bk, T, weekends, fused=True)
    assert plain.fused_step is False and fused.fused_step is True
    n0 = len(fused_bk.calls)
    acts = _actions()
    want, got = _loop(plain, acts), _loop(fused, acts)
    for k, (w, g) in enumerate(zip(want, got)):
        for x, y, name in zip(w, g, ("obs", "reward", "terminated", "truncated", "terminal_obs", "state")):
            _same(x, y, f"step {k} {name}")
    # the fused face made one backend call per step and nothing else; the default face made none of them
    assert fused_bk.calls[n0:] == ["tumor_therapy_step"] * STEPS
    assert "tumor_therapy_step" not in plain_bk.calls and plain_bk.branches["steps"] == 0
    # every branch of the wrapper step was taken at least once in this configuration (so no test here passes by leaving one out)
    br = fused_bk.branches
    print({k: v for k, v in br.items() if k != "growth_days"}, sorted(set(br["growth_days"])))
    assert br["steps"] == STEPS and br["post_runs"] >= 1 and br["treatment_days"] >= 1 and br["negative_rewards"] >= 1
    assert br["episodes"] >= 1 and br["growth_runs"] == br["episodes"] and all(d > 1 for d in br["growth_days"])
    assert (br["weekend_rests"] >= 1) == weekends
    # (the counts of this configuration: 26 post-therapy runs, 26 episodes -- the first at step 5 --, growth runs of 213 days, 382
    # treatment days, 87 negative rewards, 58 weekend rests)
    assert (br["post_runs"], br["episodes"], br["first_done_step"], set(br["growth_days"]), br["treatment_days"], br["negative_rewards"]) == \
           (26, 26, 5, {213}, 382, 87) and br["weekend_rests"] == (58 if weekends else 0)
    if T == 600:
        assert br["by_death"] == br["episodes"] and br["by_time_limit"] == 0
    else:
        assert br["by_time_limit"] == br["episodes"] and br["by_death"] == 0
    # the counters the face exposes keep their meaning
    assert int(fused.treatment_calls.sum()) == br["treatment_days"] and int(fused.soft_constraint_violations.sum()) == br["negative_rewards"]


def test_fused_step_checkpoint_round_trip_and_the_sb3_face():
    from tests.fake_tumor_rollout_backend import FakeTumorRolloutBackend
    acts = _actions(12)
    a = _venv(FakeTumorRolloutBackend(), 600, True, fused=True)
    _loop(a, acts[:6])
    sd = a.state_dict()
    b = _venv(FakeTumorRolloutBackend(), 600, True, fused=True)
    b.load_state_dict(sd)
    assert set(sd["face"]) == {"_consecutive", "treatment_calls", "soft_constraint_violations"}      # checkpoints are unchanged
    for x, y in zip(_loop(a, acts[6:]), _loop(b, acts[6:])):
        for p, q in zip(x, y):
            _same(p, q)
    # step_wait: terminal observations come from the kernel's final_obs rows
    c, d = _venv(FakeTumorRolloutBackend(), 600, False), _venv(FakeTumorRolloutBackend(), 600, False, fused=True)
    seen = 0
    for act in acts:
        (o1, r1, d1, i1), (o2, r2, d2, i2) = c.step(act), d.step(act)
        np.testing.assert_array_equal(o1, o2)
        np.testing.assert_array_equal(r1, r2)
        np.testing.assert_array_equal(d1, d2)
        for x, y in zip(i1, i2):
            assert set(x) == set(y)
            if x:
                seen += 1
                np.testing.assert_array_equal(x["terminal_observation"], y["terminal_observation"])
    assert seen >= 1


def _policy(width, backend):
    from pde_control_gym import FusedMLP
    torch.manual_seed(3)
    net = torch.nn.Sequential(torch.nn.Linear(201, width), torch.nn.Tanh(), torch.nn.Linear(width, 1), torch.nn.Tanh())
    with torch.no_grad():
        net[0].weight.mul_(1e-5)
    return FusedMLP(net, backend=backend)


@pytest.mark.parametrize("with_policy", [False, True])
def test_one_launch_true_is_one_rollout_call_and_equals_the_step_by_step_loop(with_policy):
    from pde_control_gym import DeviceRollout
    from tests.fake_tumor_rollout_backend import FakeTumorRolloutBackend
    runs = {}
    for one_launch in (None, True):
        bk = FakeTumorRolloutBackend()
        venv = _venv(bk, 600, True)
        pol = _policy(32, bk) if with_policy else None
        if pol is None and one_launch is None:       # commands given ahead have no default path: drive step_tensor by hand
            acts = _actions(8)
            ro = None
            res = []
            for rep in range(3):
                rows = _loop(venv, acts)
                res.append([torch.stack([r[i] for r in rows]) for i in range(4)])
            runs[one_launch] = (res, _state(venv), bk)
            continue
        ro = DeviceRollout(venv, pol, 8, use_graph=False, action_low=0.0, action_high=1.0, action_noise=with_policy, one_launch=one_launch)
        assert ro.one_launch is bool(one_launch)
        n0 = len(bk.calls)
        res = []
        for rep in range(3):
            if with_policy:
                ro.action_noise.copy_(torch.from_numpy(np.random.default_rng(rep).normal(0, 0.05, (8, B)).astype(np.float32)))
            else:
                ro.actions.copy_(torch.from_numpy(np.stack(_actions(8))))
            ro.run()
            res.append([x.clone() for x in ((ro.obs[1:], ro.rewards, ro.terminated.bool(), ro.truncated.bool())
                                            + ((ro.actions,) if with_policy else ()))])
        new = [c for c in bk.calls[n0:] if not isinstance(c, str) or c.startswith("tumor")]
        if one_launch:
            assert [c[0] for c in new] == ["tumor_rollout"] * 3 and new[0][1]["T"] == 8
            assert new[0][1]["policy"] is with_policy and new[0][1]["noise"] is with_policy
            assert new[0][1]["clamp"] == ((0.0, 1.0) if with_policy else None)
        else:
            assert not any(isinstance(c, tuple) for c in new) and "tumor_therapy_step" not in new      # one_launch=None: today's path
        runs[one_launch] = (res, _state(venv), bk)
    for a, b in zip(runs[None][0], runs[True][0]):
        for x, y in zip(a, b):
            _same(x, y)
    _same(runs[None][1], runs[True][1])
    assert runs[True][2].branches["episodes"] >= 1


def test_refusals_say_why():
    from pde_control_gym import DeviceRollout
    from tests.fake_backend import FakeBackend
    from tests.fake_tumor_rollout_backend import FakeTumorRolloutBackend
    bk = FakeTumorRolloutBackend()
    venv = _venv(bk, 600, False, num_envs=3)
    # one_launch=None never takes the rollout kernel for this family, whatever the policy
    assert venv.one_launch_fits(_policy(32, bk)) is False and DeviceRollout(venv, _policy(32, bk), 2, use_graph=False).one_launch is False
    # a policy that is no FusedMLP; one too large for the LDS next to the rows
    with pytest.raises(ValueError, match="one_launch=True cannot take this rollout into the rollout kernel: the policy is not a FusedMLP"):
        DeviceRollout(venv, lambda o: o[:, 0], 2, use_graph=False, one_launch=True)
    torch.manual_seed(0)
    from pde_control_gym import FusedMLP
    wrong = FusedMLP(torch.nn.Sequential(torch.nn.Linear(64, 8), torch.nn.Tanh(), torch.nn.Linear(8, 1)), backend=bk)
    with pytest.raises(ValueError, match="does not fit the rollout kernel: 201 inputs, one output"):
        DeviceRollout(venv, wrong, 2, use_graph=False, one_launch=True)
    assert venv.one_launch_gap(_policy(64, bk)) is None and venv.one_launch_gap(_policy(256, bk)) is None and venv.one_launch_gap(None) is None
    # a long row: the policy's LDS and 16 x 2 rows do not fit any more
    long = _venv(bk, 300, False, num_envs=2, X=500)
    assert long.core.nx == 501
    big = FusedMLP(torch.nn.Sequential(torch.nn.Linear(501, 8), torch.nn.Tanh(), torch.nn.Linear(8, 1)), backend=bk)
    assert big.fits_rollout(501, 1) and not long.core.policy_fits_rollout(big) and "within 160 KB" in long.one_launch_gap(big)
    assert long.one_launch_gap(None) is None
    # a backend without the entry points; history recording
    old = _venv(FakeBackend(), 600, False, num_envs=2)
    assert "backend has no tumor_therapy_step / tumor_rollout" in old.one_launch_gap(None)
    with pytest.raises(ValueError, match="backend has no tumor_therapy_step"):
        DeviceRollout(old, None, 2, use_graph=False, one_launch=True)
    with pytest.raises(ValueError, match="fused_step=True is not available: the backend has no"):
        _venv(FakeBackend(), 600, False, fused=True, num_envs=2)
    with pytest.raises(ValueError, match="record_history=True"):
        _venv(bk, 600, False, fused=True, num_envs=2, record_history=True)
    hist = _venv(bk, 600, False, num_envs=2, record_history=True)
    with pytest.raises(ValueError, match="record_history=True"):
        DeviceRollout(hist, None, 2, use_graph=False, one_launch=True)
    # a device-side sensing-noise hook
    venv.sensing_noise_tensor_func = lambda o: o
    with pytest.raises(ValueError, match="one_launch=True cannot apply sensing_noise_tensor_func"):
        DeviceRollout(venv, None, 2, use_graph=False, one_launch=True)
    venv.sensing_noise_tensor_func = None
    # the engine's own argument checks
    with pytest.raises(ValueError, match="wrap_state lacks"):
        venv.core.therapy_step(torch.zeros(3, dtype=torch.float64), {"weekends": False})
    with pytest.raises(ValueError, match="cannot run inside the rollout kernel"):
        venv.core.rollout(torch.zeros(3, 3, 201, dtype=torch.float64), torch.zeros(2, 3, dtype=torch.float64), None, None, None, policy=wrong,
                          wrap_state=venv._wrapper_state())


def test_lds_budget_of_the_host_check_matches_the_header():
    """policy_fits_rollout re-derives the kernel's budget: pdegym_policy.h's lds_floats for the network, rounded up to 16 bytes, plus
    two float64 rows per wave for 16 waves, within kMaxLdsBytes."""
    from tests.fake_tumor_rollout_backend import FakeTumorRolloutBackend
    bk = FakeTumorRolloutBackend()
    hdr = open(os.path.join(ROOT, "pdecontrolgym_amd", "csrc", "pdegym_policy.h")).read()
    assert "constexpr int kMaxLdsBytes = 160 * 1024;" in hdr and "constexpr int kWaves = 16;" in hdr
    narrow, wide = _policy(64, bk), _policy(256, bk)
    groups = lambda n: ((n + 3) >> 2) | 1            # noqa: E731
    assert narrow.rollout_lds_bytes(201) == 4 * ((groups(201) * 4 * 64 + 64) + (groups(64) * 4 * 1 + 64) + 16 * (204 + 128))
    stride = lambda w: (w + 63) // 64 * 64 + 4       # noqa: E731
    assert wide.rollout_lds_bytes(201) == 4 * (16 * (stride(208) + 2 * stride(256)) + 32)
    rows = 16 * 2 * 201 * 8
    assert rows == 51456 and narrow.rollout_lds_bytes(201) + rows <= 160 * 1024 and wide.rollout_lds_bytes(201) + rows <= 160 * 1024


def test_exports_and_build_list():
    from pdecontrolgym_amd import _native as N
    from pdecontrolgym_amd import build
    assert "pdegym_tumor_rollout.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "pdegym_tumor_body.h"))
    assert {"pdegym_tumor_therapy_step", "pdegym_tumor_rollout"} <= set(N.EXPORTS) and N.ABI_VERSION >= 20
    hdr = open(os.path.join(ROOT, "include", "pdegym.h")).read()
    assert int(re.search(r"#define PDEGYM_ABI_VERSION (\d+)", hdr).group(1)) == N.ABI_VERSION
    assert hdr.count("brain_tumor_env.py:385-505") >= 4 and "pdegym_wrap_tumor" in hdr and "pdegym_rollout_tumor" in hdr
    assert "found in Growth" in hdr
    # the ctypes structures mirror the header's field order
    for cls, name in ((N.WrapTumor, "pdegym_wrap_tumor"), (N.RolloutTumor, "pdegym_rollout_tumor")):
        body = re.search(r"typedef struct " + name + r" \{(.*?)\} " + name + ";", hdr, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = [re.split(r"[\s\*]+", d.strip())[-1] for d in body.split(";") if d.strip()]
        assert fields == [f[0] for f in cls._fields_], (name, fields)
    # the shared device code: neither unit defines what the shared header holds
    body = open(os.path.join(build.CSRC, "pdegym_tumor_body.h")).read()
    for unit in ("pdegym_tumor.hip", "pdegym_tumor_rollout.hip"):
        src = open(os.path.join(build.CSRC, unit)).read()
        assert '#include "pdegym_tumor_body.h"' in src
        for name in ("rightmost", "fd_node", "clip0k", "tumor_stage_row", "tumor_day", "tumor_reset_scalars", "tumor_store_scalars"):
            pat = re.compile(r"^__device__ __forceinline__\s+[\w:]+\s+" + name + r"\(", re.M)
            assert len(pat.findall(body)) == 1 and not pat.findall(src), (unit, name)


def test_every_kernel_of_the_new_unit_has_an_output_contract_test():
    """The kernels of csrc/pdegym_tumor_rollout.hip keep their poisoned-buffer tests in tests/test_gpu_tumor_rollout.py: every kernel
    launched there (chevron syntax) is listed in its KERNEL_CASES, and every test named exists."""
    from tests import test_gpu_tumor_rollout as G
    src = open(os.path.join(ROOT, "pdecontrolgym_amd", "csrc", "pdegym_tumor_rollout.hip")).read()
    launched = set(re.findall(r"([A-Za-z_]\w*)\s*<[^<>;]*>\s*<<<", src))
    assert "hipLaunchKernelGGL" not in src
    assert launched == set(G.KERNEL_CASES) == {"tumor_rollout_kernel"}, launched ^ set(G.KERNEL_CASES)
    for k, tests in G.KERNEL_CASES.items():
        assert tests and all(callable(getattr(G, t, None)) for t in tests), (k, tests)


# ---- argument validation of the two entry points, host half under ASan + UBSan ------------------------------------------------------
@pytest.mark.skipif(shutil.which("hipcc") is None, reason="needs hipcc")
def test_tumor_rollout_entry_points_validate_their_arguments_under_asan_and_ubsan(tmp_path):
    """tests/c/tumor_rollout_validation.c (its own main) against the host half of pdegym_tumor_rollout.hip + pdegym_abi.hip, compiled
    with --cuda-host-only and the sanitizers and given an empty device image: every bad call must answer with a negative code and a
    message, and no call reaches a device."""
    from pdecontrolgym_amd import build
    from tests.test_backstepping import SAN
    hipcc = shutil.which("hipcc")
    inc = ["-I" + os.path.join(ROOT, "include"), "-I" + build.CSRC]
    objs = []
    for s in ("pdegym_abi.hip", "pdegym_tumor_rollout.hip"):
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
    lib = str(tmp_path / "libpdegym_tumor_rollout_asan.so")
    r = subprocess.run([hipcc, "-shared", "-fPIC"] + SAN + ["-o", lib] + objs + [stub_o], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()[-3000:]
    exe = str(tmp_path / "tumor_rollout_validation")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    r = subprocess.run([hipcc, "-x", "c", "-std=c11", "-Wall", "-Werror", "-g"] + SAN
                       + [os.path.join(ROOT, "tests", "c", "tumor_rollout_validation.c"), "-I" + os.path.join(ROOT, "include"),
                          "-L" + str(tmp_path), "-lpdegym_tumor_rollout_asan", "-Wl,-rpath," + str(tmp_path),
                          "-Wl,-rpath," + os.path.join(rocm, "lib"), "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1", HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, env=env, timeout=120)
    out = r.stdout.decode()
    assert r.returncode == 0 and "TUMOR-ROLLOUT-VALIDATION-OK" in out, out[-4000:]
    assert "ERROR: AddressSanitizer" not in out and "runtime error" not in out, out[-4000:]
