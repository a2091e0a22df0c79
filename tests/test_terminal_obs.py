"""CPU tests of the per-step terminal observations and SB3's truncation bootstrap: the host path from
``DeviceRollout(terminal_obs=True)`` and ``DeviceRolloutBuffer.compute(critic=...)`` down to the backend calls on the doubles of
tests/fake_terminal_obs_backend.py, the refusals, the agreement of header and binding, and tests/c/terminal_obs_validation.c on the host
halves of the touched units under AddressSanitizer and UBSan.  No kernel is launched; the kernels are pinned in
tests/test_gpu_terminal_obs.py."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import gae_restatement as R
from tests import terminal_obs_cases as K
from tests.fake_terminal_obs_backend import FakeTerminalObsBackend

torch = pytest.importorskip("torch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, B, NX = K.T_STEPS, 5, 16


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize])


def _venv(backend=None, **kw):
    return K.make_1d("parabolic", NX, B, device="cpu", backend=backend or FakeTerminalObsBackend(), **kw)


def _critic(backend, seed=4):
    from pdecontrolgym_amd.policy import FusedMLP
    torch.manual_seed(seed)
    net = torch.nn.Sequential(torch.nn.Linear(NX + 1, 8), torch.nn.Tanh(), torch.nn.Linear(8, 1))
    return net, FusedMLP(net, backend=backend)


def _rollout(one_launch, terminal_obs=True, backend=None):
    from pde_control_gym import DeviceRollout
    venv = _venv(backend)
    acts = torch.from_numpy(K.commands(T, B))
    ro = DeviceRollout(venv, None if one_launch else _Replay(acts), T, use_graph=False, one_launch=False, terminal_obs=terminal_obs)
    if one_launch:           # commands given ahead, through the engine's one-launch entry point
        ro.actions.copy_(acts)
        ro.obs[0].copy_(venv.rollout_obs())
        venv.rollout_one_launch(ro.obs, ro.actions, ro.rewards, ro.terminated, ro.truncated,
                                **({"final_obs_steps": ro.terminal_obs} if terminal_obs else {}))
    else:
        ro.run()
    return venv, ro


class _Replay:
    """A policy that issues the commands of row t at its t-th call."""

    def __init__(self, acts):
        self.acts, self.t = acts, 0

    def __call__(self, obs):
        a = self.acts[self.t]
        self.t += 1
        return a


def _counts(ro):
    te, tr = ro.terminated.numpy().astype(bool), ro.truncated.numpy().astype(bool)
    return int(te.sum()), int((tr & ~te).sum())


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def test_terminal_obs_needs_the_fused_auto_reset():
    from pde_control_gym import DeviceRollout
    venv = _venv(auto_reset=False)
    with pytest.raises(ValueError, match="enable_fused_auto_reset"):
        DeviceRollout(venv, lambda o: o[:, 0], T, use_graph=False, terminal_obs=True)
    assert DeviceRollout(venv, lambda o: o[:, 0], T, use_graph=False).terminal_obs is None
    venv.enable_fused_auto_reset()
    ro = DeviceRollout(venv, lambda o: o[:, 0], T, use_graph=False, terminal_obs=True)
    assert ro.terminal_obs.shape == ro.obs[:T].shape and ro.terminal_obs.dtype == ro.obs.dtype and not ro.terminal_obs.any()


def test_terminal_obs_is_refused_with_sensing_noise():
    from pde_control_gym import DeviceRollout
    for kw in (dict(sensing_noise=True), dict()):
        venv = _venv(**({} if kw else {"sensing_noise_tensor_func": lambda o: o + 1.0}))
        with pytest.raises(ValueError, match="no noise slot"):
            DeviceRollout(venv, lambda o: o[:, 0], T, use_graph=False, terminal_obs=True, **kw)


def test_terminal_obs_is_refused_on_navier_stokes():
    import pde_control_gym
    from pde_control_gym import DeviceRollout
    from tests.test_ns_vec import _params
    rng = np.random.default_rng(0)
    n, nb = 9, 2
    p = _params(n, 6, 3, rng, "float64")
    pools = tuple(rng.uniform(-1, 1, (2 * nb, n, n)) for _ in range(3))
    p["reset_init_condition_func"] = lambda X: tuple(pool[0] for pool in pools)
    venv = pde_control_gym.make_vec("PDEControlGym-NavierStokes2D", num_envs=nb, device="cpu", backend=FakeTerminalObsBackend(), **p)
    venv.core.reset(*(pool[:nb] for pool in pools))
    venv.enable_fused_auto_reset(pools)
    with pytest.raises(ValueError, match="never truncates"):
        DeviceRollout(venv, lambda o: torch.zeros(o.shape[0], venv.core.action_dim), 2, use_graph=False, terminal_obs=True)


# ---- the inputs of the GPU tests, on the oracle -----------------------------------------------------------------------------------------
def _flag_counts(steps):
    te = np.stack([np.asarray(s[0]).astype(bool) for s in steps])
    tr = np.stack([np.asarray(s[1]).astype(bool) for s in steps])
    return int(te.sum()), int((tr & ~te).sum())


@pytest.mark.parametrize("case", sorted(K.GPU_ENVS_1D))
def test_gpu_inputs_1d_hold_a_termination_and_a_cut_off(case):
    """Every 1D environment of tests/test_gpu_terminal_obs.py, stepped on the oracle with the commands of its open-loop cases."""
    kind, nx, over = K.GPU_ENVS_1D[case]
    venv = K.make_1d(kind, nx, K.B_GPU, device="cpu", backend=FakeTerminalObsBackend(), **over)
    acts = torch.from_numpy(K.commands(T, K.B_GPU))
    steps = []
    for t in range(T):
        _, _, te, tr = venv.step_tensor(acts[t])
        steps.append((te.numpy().copy(), tr.numpy().copy()))
    n_term, n_trunc = _flag_counts(steps)
    assert n_term >= 1 and n_trunc >= 1, (n_term, n_trunc)


@pytest.mark.parametrize("sim", ["outlet", "both"])
def test_gpu_inputs_traffic_hold_a_termination_and_a_cut_off(sim):
    from tests.fake_backend import FakeBackend
    venv = K.make_traffic(sim, device="cpu", backend=FakeBackend())
    acts = torch.from_numpy(K.traffic_commands(T, 5, venv.core.action_dim))
    steps = []
    for t in range(T):
        _, _, te, tr = venv.step_tensor(acts[t])
        steps.append((te.numpy().copy(), tr.numpy().copy()))
    n_term, n_trunc = _flag_counts(steps)
    assert n_term >= 1 and n_trunc >= 1, (n_term, n_trunc)


def test_gpu_inputs_tumor_hold_a_termination_and_a_cut_off():
    from tests.fake_tumor_rollout_backend import FakeTumorRolloutBackend
    venv = K.make_tumor(fused=True, device="cpu", backend=FakeTumorRolloutBackend())
    acts = torch.from_numpy(K.tumor_commands(T, 5))
    steps = []
    for t in range(T):
        _, _, te, tr = venv.step_tensor(acts[t])
        steps.append((te.numpy().copy(), tr.numpy().copy()))
    n_term, n_trunc = _flag_counts(steps)
    assert n_term >= 1 and n_trunc >= 1, (n_term, n_trunc)


# ---- the rows ---------------------------------------------------------------------------------------------------------------------------
def test_per_step_rows_equal_the_final_obs_of_a_step_loop():
    """Row (t, b) of the one-launch form holds what final_obs[b] holds after the t-th step_tensor call where that step ended an
    episode; no other row is written; nothing else changes; the engine's own final_obs is not written."""
    twin = _venv()
    acts = torch.from_numpy(K.commands(T, B))
    want = torch.full((T, B, NX + 1), -7.0)
    ended = np.zeros((T, B), bool)
    for t in range(T):
        _, _, te, tr = twin.step_tensor(acts[t])
        done = (te | tr).bool()
        ended[t] = done.numpy()
        want[t][done] = twin.core.t["final_obs"][done]
    venv, ro = _rollout(True)
    n_term, n_trunc = _counts(ro)
    assert n_term >= 1 and n_trunc >= 1, (n_term, n_trunc)
    np.testing.assert_array_equal((ro.terminated | ro.truncated).numpy().astype(bool), ended)
    got = ro.terminal_obs.clone()
    assert not got[~torch.from_numpy(ended)].any(), "a row of a step that ended nothing was written"
    np.testing.assert_array_equal(_bits(got[torch.from_numpy(ended)].numpy()), _bits(want[torch.from_numpy(ended)].numpy()))
    assert not venv.core.t["final_obs"].any(), "the engine's own final_obs is not written in this mode"
    plain_env, plain = _rollout(True, terminal_obs=False)
    for name in ("obs", "actions", "rewards", "terminated", "truncated"):
        np.testing.assert_array_equal(getattr(ro, name).numpy(), getattr(plain, name).numpy(), err_msg=name)
    for key in ("time_index", "bsum", "ring", "reset_count", "beta"):
        np.testing.assert_array_equal(venv.core.t[key].numpy(), plain_env.core.t[key].numpy(), err_msg=key)
    # the launch-per-step path fills the same rows
    _, loop = _rollout(False)
    np.testing.assert_array_equal(_bits(loop.terminal_obs.numpy()), _bits(got.numpy()))
    np.testing.assert_array_equal(loop.obs.numpy(), ro.obs.numpy())


# ---- the buffer -------------------------------------------------------------------------------------------------------------------------
def test_compute_bootstraps_truncated_steps_from_the_terminal_rows():
    """compute(critic) == the restatement given boot = V(terminal rows), and differs from the result without the bootstrap on a
    rollout that holds a truncation (the parent computes the latter whatever the rollout holds)."""
    from pde_control_gym import DeviceRolloutBuffer
    bk = FakeTerminalObsBackend()
    venv, ro = _rollout(True, backend=bk)
    n_term, n_trunc = _counts(ro)
    assert n_term >= 1 and n_trunc >= 1
    net, critic = _critic(bk)
    buf = DeviceRolloutBuffer(ro, gamma=0.9, gae_lambda=0.8, backend=bk)
    assert buf.boot is not None and tuple(buf.boot.shape) == (T, B) and buf.boot.dtype == torch.float32
    ptr = buf.boot.data_ptr()
    buf.boot.fill_(123.0)                    # entries of rows that are not truncated keep what they held
    buf.compute(critic=critic)
    assert bk.masked_calls == 1 and buf.boot.data_ptr() == ptr
    full = torch.zeros(T * B)
    critic.forward_into(ro.terminal_obs.reshape(T * B, -1), full, clamp=None)
    live = ((ro.truncated != 0) & (ro.terminated == 0))
    np.testing.assert_array_equal(_bits(buf.boot[live].numpy()), _bits(full.reshape(T, B)[live].numpy()))
    assert (buf.boot[~live] == 123.0).all()
    adv, ret = R.gae_reference(ro.rewards.numpy(), buf.values.numpy(), ro.terminated.numpy(), ro.truncated.numpy(), 0.9, 0.8,
                               full.reshape(T, B).numpy())
    np.testing.assert_array_equal(_bits(buf.advantages.numpy()), _bits(adv))
    np.testing.assert_array_equal(_bits(buf.returns.numpy()), _bits(ret))
    off = DeviceRolloutBuffer(ro, gamma=0.9, gae_lambda=0.8, backend=bk, bootstrap_truncated=False)
    assert off.boot is None
    off.compute(critic=critic)
    assert (_bits(off.advantages.numpy()) != _bits(buf.advantages.numpy())).any(), "the bootstrap changed nothing"
    # any other torch module is evaluated on all T * B rows, with the same result to float32 rounding of the two forward passes
    mod = DeviceRolloutBuffer(ro, gamma=0.9, gae_lambda=0.8, backend=bk).compute(critic=net)
    np.testing.assert_allclose(mod.boot[live].numpy(), buf.boot[live].numpy(), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(mod.advantages.numpy(), buf.advantages.numpy(), rtol=1e-4, atol=1e-3)
    # compute(values=) leaves boot to the caller
    calls = bk.masked_calls
    buf.boot.zero_()
    buf.compute(values=buf.values.clone())
    assert bk.masked_calls == calls and not buf.boot.any()


def test_without_a_truncation_the_bootstrap_changes_no_bit():
    from pde_control_gym import DeviceRolloutBuffer
    bk = FakeTerminalObsBackend()
    _, ro = _rollout(True, backend=bk)
    ro.truncated.zero_()                      # (the terminations stay)
    assert _counts(ro)[0] >= 1
    _, critic = _critic(bk)
    a = DeviceRolloutBuffer(ro, backend=bk).compute(critic=critic)
    b = DeviceRolloutBuffer(ro, backend=bk, bootstrap_truncated=False).compute(critic=critic)
    np.testing.assert_array_equal(_bits(a.advantages.numpy()), _bits(b.advantages.numpy()))
    np.testing.assert_array_equal(_bits(a.returns.numpy()), _bits(b.returns.numpy()))
    assert not a.boot.any(), "an all-dead mask writes nothing"


def test_forward_into_rows_checks_its_arguments():
    bk = FakeTerminalObsBackend()
    _, critic = _critic(bk)
    x, y = torch.randn(6, NX + 1), torch.zeros(6)
    rows = torch.tensor([1, 0, 1, 1, 0, 0], dtype=torch.uint8)
    rows_not = torch.tensor([0, 0, 1, 0, 0, 0], dtype=torch.uint8)
    y.fill_(9.0)
    critic.forward_into(x, y, clamp=None, rows=rows, rows_not=rows_not)
    ref = torch.zeros(6)
    critic.forward_into(x, ref, clamp=None)
    assert y.tolist() == [ref[0].item(), 9.0, 9.0, ref[3].item(), 9.0, 9.0]
    for bad in (dict(rows=None, rows_not=rows_not), dict(rows=rows.bool()), dict(rows=rows[:5]), dict(rows=rows, noise=torch.zeros(6)),
                dict(rows=rows, tail=torch.zeros(6, 1))):
        with pytest.raises(ValueError):
            critic.forward_into(x, y, clamp=None, **bad)
    with pytest.raises(ValueError):
        critic.forward_into(x, torch.zeros(6, dtype=torch.float64), clamp=None, rows=rows)


# ---- header / binding -------------------------------------------------------------------------------------------------------------------
def test_header_and_binding_agree():
    from pdecontrolgym_amd import _native as N
    from pdecontrolgym_amd import backend
    import inspect
    header = open(os.path.join(ROOT, "include", "pdegym.h")).read()
    assert "#define PDEGYM_ABI_VERSION 21" in header and N.ABI_VERSION == 21
    m = re.search(r"#define PDEGYM_ROLLOUT_FINAL_OBS_PER_STEP (\d+)", header)
    assert m and int(m.group(1)) == N.ROLLOUT_FINAL_OBS_PER_STEP == 1
    assert "pdegym_mlp_forward_masked" in N.EXPORTS and re.search(r"\bint pdegym_mlp_forward_masked\(", header)
    for struct in ("pdegym_rollout1d", "pdegym_rollout_traffic", "pdegym_rollout_tumor"):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), header, re.S).group(1)
        assert re.search(r"int32_t reserved_;\s*/\* bit 0: PDEGYM_ROLLOUT_FINAL_OBS_PER_STEP", body), struct
    for cls in (N.Rollout1D, N.RolloutTraffic, N.RolloutTumor):
        assert [f[0] for f in cls._fields_][:2] == ["T", "reserved_"]
    src = inspect.getsource(backend)
    for name in ("rollout1d", "traffic_rollout", "traffic_backstep_rollout", "tumor_rollout", "backstep_rollout1d"):
        assert re.search(r"def %s\([^)]*final_obs_steps=None\)" % name, src, re.S), name
    assert re.search(r"def mlp_forward\(self, net: N\.Mlp, x, y, B: int, rows=None, rows_not=None\)", src)
    for text, where in ((open(os.path.join(ROOT, "README.md")).read(), "README.md"), (open(os.path.join(ROOT, "DESIGN.md")).read(), "DESIGN.md"),
                        (open(os.path.join(ROOT, "INTEGRATION.md")).read(), "INTEGRATION.md")):
        assert "terminal_obs" in text and "pdegym_mlp_forward_masked" in text, where
    assert "4.21" in open(os.path.join(ROOT, "DESIGN.md")).read()


def test_the_examples_take_their_switch():
    import inspect
    import importlib.util
    import sys
    if os.path.join(ROOT, "examples") not in sys.path:
        sys.path.insert(0, os.path.join(ROOT, "examples"))
    for name, arg in (("train_ppo_device", "bootstrap"), ("train_sac_device", "terminal_obs")):
        spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "examples", name + ".py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        p = inspect.signature(mod.main).parameters
        assert arg in p and p[arg].default is False, name
    assert "keep no terminal-observation buffer" not in open(os.path.join(ROOT, "examples", "train_sac_device.py")).read()


# ---- argument validation, host half under ASan + UBSan ----------------------------------------------------------------------------------
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
UNITS = ("pdegym_abi.hip", "pdegym_mlp.hip", "pdegym_1d_rollout.hip", "pdegym_backstep_rollout.hip", "pdegym_traffic.hip",
         "pdegym_traffic_backstep.hip", "pdegym_tumor.hip", "pdegym_tumor_rollout.hip")


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="needs hipcc")
def test_entry_points_validate_their_arguments_under_asan_and_ubsan(tmp_path):
    """tests/c/terminal_obs_validation.c (its own main) against the host halves of the touched units, compiled with --cuda-host-only
    and the sanitizers and given empty device images: every bad call answers with the stated code and a message, a well-formed
    descriptor fails only at the launch, and no call reaches a device."""
    from pdecontrolgym_amd import build
    hipcc = shutil.which("hipcc")
    inc = ["-I" + os.path.join(ROOT, "include"), "-I" + build.CSRC]
    procs = []
    for s in UNITS:
        o = str(tmp_path / s.replace(".hip", ".o"))
        procs.append((o, subprocess.Popen([hipcc, "--offload-arch=gfx950", "--cuda-host-only", "-O1", "-g", "-std=c++17", "-fPIC"]
                                          + SAN + inc + ["-c", os.path.join(build.CSRC, s), "-o", o],
                                          stdout=subprocess.PIPE, stderr=subprocess.STDOUT)))
    objs = []
    for o, p in procs:
        out, _ = p.communicate()
        assert p.returncode == 0, out.decode()[-3000:]
        objs.append(o)
    nm = subprocess.run(["nm", "-u"] + objs, stdout=subprocess.PIPE, check=True).stdout.decode()
    names = sorted({ln.split()[-1] for ln in nm.splitlines() if "__hip_fatbin_" in ln})
    stub = tmp_path / "empty_fatbins.c"
    stub.write_text("".join(f'__attribute__((aligned(4096))) const char {n}[4096] = "__CLANG_OFFLOAD_BUNDLE__";\n' for n in names))
    stub_o = str(tmp_path / "empty_fatbins.o")
    subprocess.run(["gcc", "-c", "-fPIC", str(stub), "-o", stub_o], check=True)
    lib = str(tmp_path / "libpdegym_terminal_obs_asan.so")
    r = subprocess.run([hipcc, "-shared", "-fPIC"] + SAN + ["-o", lib] + objs + [stub_o], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()[-3000:]
    exe = str(tmp_path / "terminal_obs_validation")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    r = subprocess.run([hipcc, "-x", "c", "-std=c11", "-Wall", "-Werror", "-g"] + SAN
                       + [os.path.join(ROOT, "tests", "c", "terminal_obs_validation.c"), "-I" + os.path.join(ROOT, "include"),
                          "-L" + str(tmp_path), "-lpdegym_terminal_obs_asan", "-Wl,-rpath," + str(tmp_path),
                          "-Wl,-rpath," + os.path.join(rocm, "lib"), "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1", HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, env=env, timeout=120)
    out = r.stdout.decode()
    assert r.returncode == 0 and "TERMINAL-OBS-VALIDATION-OK" in out, out[-4000:]
    assert "runtime error" not in out and "AddressSanitizer" not in out, out[-4000:]
    assert int(out.strip().splitlines()[-2].split()[1]) >= 60, out[-1000:]
