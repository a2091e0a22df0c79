"""CPU tests of the GAE(lambda) step (include/pdegym.h: pdegym_gae; pde_control_gym.DeviceRolloutBuffer): the NumPy restatement of
SB3's loop checks itself, a fake backend built on it drives the buffer's host logic on CPU tensors, the new names are exported, and
tests/c/gae_validation.c runs against the host half of the library under AddressSanitizer and UBSan.  No kernel is launched; the
kernel itself is pinned to the restatement bit for bit in tests/test_gpu_gae.py."""
import os
import shutil
import subprocess
import types

import numpy as np
import pytest

from tests import gae_restatement as R
from tests.fake_gae_backend import FakeGaeBackend

torch = pytest.importorskip("torch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize])


# ---- the restatement ----------------------------------------------------------------------------------------------------------------
def test_restatement_is_the_float32_recurrence_not_a_rounded_float64_one():
    rew, val, te, tr, boot = R.seeded_case(200, 37, seed=1)
    adv, ret = R.gae_reference(rew, val, te, tr, 0.99, 0.95)
    assert adv.dtype == np.float32 and ret.dtype == np.float32 and adv.shape == (200, 37)
    a64, r64 = R.gae_float64_rounded(rew, val, te, tr, 0.99, 0.95)
    assert (_bits(adv) != _bits(a64)).any(), "a float64 recurrence rounded at the end gives the same bits: the case is too easy"
    assert np.allclose(adv, a64, rtol=1e-4, atol=1e-4) and np.allclose(ret, r64, rtol=1e-4, atol=1e-4)
    # SB3's expressions (Python-float discounts meeting float32 arrays) and the kernel's explicit roundings are the same function
    for boot_ in (None, boot):
        for trunc in (tr, None):
            for gam, lam in ((0.99, 0.95), (1.0, 1.0), (0.0, 0.5)):
                a, r = R.gae_reference(rew, val, te, trunc, gam, lam, boot_)
                b, s = R.gae_explicit(rew, val, te, trunc, gam, lam, boot_)
                assert np.array_equal(_bits(a), _bits(b)) and np.array_equal(_bits(r), _bits(s)), (boot_ is None, trunc is None, gam)


def test_restatement_hand_checked_steps():
    """Three steps of one environment by hand: an interior step, an episode end (the bootstrap is cut), a truncation with boot."""
    f = np.float32
    val = np.array([[1.0], [2.0], [3.0], [4.0]], f)
    rew = np.array([[0.5], [0.25], [-1.0]], f)
    te = np.array([[0], [1], [0]], np.uint8)
    tr = np.array([[0], [0], [1]], np.uint8)
    boot = np.array([[np.nan], [np.nan], [8.0]], f)
    adv, ret = R.gae_reference(rew, val, te, tr, 0.5, 0.5, boot)
    a2 = (-1.0 + 0.5 * 8.0) - 3.0                     # truncated: r + g*boot, no bootstrap from values[3], last = 0
    a1 = 0.25 - 2.0                                   # terminated: nothing crosses the boundary
    a0 = (0.5 + 0.5 * 2.0 - 1.0) + 0.25 * a1
    assert adv[:, 0].tolist() == [a0, a1, a2] and ret[:, 0].tolist() == [a0 + 1.0, a1 + 2.0, a2 + 3.0]
    er, el, acc, ln = R.episode_scan(rew, te, tr)
    assert er[:, 0].tolist() == [0.0, 0.75, -1.0] and el[:, 0].tolist() == [0, 2, 1] and acc[0] == 0.0 and ln[0] == 0


# ---- DeviceRolloutBuffer on the fake backend ------------------------------------------------------------------------------------------
def _rollout(T, B, D=5, f64=False, seed=0, obs_seen=False):
    rew, val, te, tr, boot = R.seeded_case(T, B, seed=seed, f64_rewards=f64)
    g = torch.Generator().manual_seed(seed)
    dt = torch.float64 if f64 else torch.float32
    obs = torch.randn(T + 1, B, D, generator=g, dtype=dt)
    ro = types.SimpleNamespace(T=T, obs=obs, obs_seen=(obs + 1.0) if obs_seen else None, actions=torch.randn(T, B, generator=g, dtype=dt),
                               rewards=torch.from_numpy(rew), terminated=torch.from_numpy(te), truncated=torch.from_numpy(tr))
    return ro, torch.from_numpy(val), torch.from_numpy(boot)


@pytest.mark.parametrize("f64", [False, True], ids=["f32_rewards", "f64_rewards"])
def test_buffer_shapes_dtypes_and_results(f64):
    import pde_control_gym
    T, B = 9, 7
    ro, val, boot = _rollout(T, B, f64=f64)
    buf = pde_control_gym.DeviceRolloutBuffer(ro, gamma=0.9, gae_lambda=0.8, backend=FakeGaeBackend())
    assert ro.rewards.dtype == (torch.float64 if f64 else torch.float32)
    for name, shape, dtype in (("values", (T + 1, B), torch.float32), ("advantages", (T, B), torch.float32),
                               ("returns", (T, B), torch.float32), ("episode_return", (T, B), torch.float64),
                               ("episode_length", (T, B), torch.int32), ("ep_return_acc", (B,), torch.float64),
                               ("ep_length_acc", (B,), torch.int32)):
        x = getattr(buf, name)
        assert tuple(x.shape) == shape and x.dtype == dtype, name
    assert buf.boot is None
    ptrs = {n: getattr(buf, n).data_ptr() for n in ("values", "advantages", "returns", "episode_return", "episode_length")}
    assert buf.compute(values=val) is buf
    adv, ret = R.gae_reference(ro.rewards.numpy(), val.numpy(), ro.terminated.numpy(), ro.truncated.numpy(), 0.9, 0.8)
    assert np.array_equal(_bits(buf.advantages.numpy()), _bits(adv)) and np.array_equal(_bits(buf.returns.numpy()), _bits(ret))
    buf.boot = boot
    buf.compute(values=val)
    adv_b, _ = R.gae_reference(ro.rewards.numpy(), val.numpy(), ro.terminated.numpy(), ro.truncated.numpy(), 0.9, 0.8, boot.numpy())
    assert np.array_equal(_bits(buf.advantages.numpy()), _bits(adv_b)) and (_bits(adv_b) != _bits(adv)).any()
    assert ptrs == {n: getattr(buf, n).data_ptr() for n in ptrs}, "compute() must not reallocate its tensors"
    fl = buf.flat()
    assert fl.observations.shape == (T * B, 5) and fl.actions.shape == (T * B,) and fl.advantages.shape == (T * B,)
    assert fl.returns.shape == (T * B,) and fl.values.shape == (T * B,)
    assert fl.observations.data_ptr() == ro.obs.data_ptr() and fl.advantages.data_ptr() == buf.advantages.data_ptr()      # views
    assert torch.equal(fl.values.reshape(T, B), buf.values[:T]) and torch.equal(fl.observations.reshape(T, B, 5), ro.obs[:T])
    # without statistics nothing of them is allocated or asked of the backend
    lean = pde_control_gym.DeviceRolloutBuffer(ro, episode_stats=False, backend=FakeGaeBackend())
    lean.compute(values=val)
    assert lean.episode_return is None and lean.ep_return_acc is None
    with pytest.raises(ValueError):
        lean.finished_episodes()


@pytest.mark.parametrize("obs_seen", [False, True], ids=["obs", "obs_seen"])
def test_compute_with_values_and_with_a_torch_critic_agree(obs_seen):
    import pde_control_gym
    T, B, D = 6, 5, 5
    ro, _, _ = _rollout(T, B, D, obs_seen=obs_seen, f64=True)           # float64 observations meet a float32 critic
    torch.manual_seed(3)
    critic = torch.nn.Sequential(torch.nn.Linear(D, 8), torch.nn.Tanh(), torch.nn.Linear(8, 1))
    seen = ro.obs_seen if obs_seen else ro.obs
    with torch.no_grad():
        val = critic(seen.reshape(-1, D).float()).reshape(T + 1, B)
    a = pde_control_gym.DeviceRolloutBuffer(ro, backend=FakeGaeBackend()).compute(values=val)
    b = pde_control_gym.DeviceRolloutBuffer(ro, backend=FakeGaeBackend()).compute(critic=critic)
    assert torch.equal(a.values, b.values) and torch.equal(a.values, val)
    assert torch.equal(a.advantages, b.advantages) and torch.equal(a.returns, b.returns)
    assert not b.values.requires_grad
    for bad in (dict(), dict(critic=critic, values=val)):
        with pytest.raises(ValueError):
            a.compute(**bad)
    with pytest.raises(ValueError):
        a.compute(values=val[:T])


def test_accumulators_carry_an_unfinished_episode_and_finished_episodes_is_a_plain_count():
    import pde_control_gym
    T, B = 12, 6
    ro, val, _ = _rollout(T, B, seed=5)
    ro.terminated[:, 0] = 0
    ro.truncated[:, 0] = 0                      # column 0 never ends in the first rollout ...
    buf = pde_control_gym.DeviceRolloutBuffer(ro, backend=FakeGaeBackend())
    buf.compute(values=val)
    first_sum = ro.rewards[:, 0].double().sum().item()
    assert buf.ep_length_acc[0].item() == T and buf.ep_return_acc[0].item() == pytest.approx(first_sum, rel=1e-12)
    done = (ro.terminated | ro.truncated).numpy().astype(bool)
    count, mean_ret, mean_len = buf.finished_episodes()
    assert all(torch.is_tensor(x) and x.dim() == 0 for x in (count, mean_ret, mean_len))
    er, el, _, _ = R.episode_scan(ro.rewards.numpy(), ro.terminated.numpy(), ro.truncated.numpy())
    assert int(count) == int(done.sum()) and int(done.sum()) > 0
    assert float(mean_ret) == pytest.approx(er[done].mean(), rel=1e-12) and float(mean_len) == pytest.approx(el[done].mean(), rel=1e-12)
    # ... and ends at step 3 of the second: its return and length span both
    ro.terminated.zero_()
    ro.truncated.zero_()
    ro.truncated[3, 0] = 1
    buf.compute(values=val)
    assert buf.episode_length[3, 0].item() == T + 4
    assert buf.episode_return[3, 0].item() == pytest.approx(first_sum + ro.rewards[:4, 0].double().sum().item(), rel=1e-12)
    count, mean_ret, mean_len = buf.finished_episodes()
    assert int(count) == 1 and float(mean_len) == T + 4 and buf.ep_length_acc[0].item() == T - 4
    ro.truncated.zero_()
    buf.compute(values=val)
    count, mean_ret, _ = buf.finished_episodes()
    assert int(count) == 0 and bool(torch.isnan(mean_ret))


def test_a_wrong_boot_is_refused():
    import pde_control_gym
    T, B = 4, 3
    ro, val, boot = _rollout(T, B)
    buf = pde_control_gym.DeviceRolloutBuffer(ro, backend=FakeGaeBackend())
    for bad in (boot[:T - 1], boot.t().contiguous(), boot.double(), torch.zeros(T + 1, B), boot.numpy(), torch.zeros(T, 2 * B)[:, ::2]):
        buf.boot = bad
        with pytest.raises(ValueError, match="boot"):
            buf.compute(values=val)
    assert buf.backend.calls == 0
    buf.boot = boot
    buf.compute(values=val)
    assert buf.backend.calls == 1


# ---- exports and documentation ----------------------------------------------------------------------------------------------------------
def test_new_names_are_exported_and_documented():
    import pde_control_gym
    from pdecontrolgym_amd import _native as N
    from pdecontrolgym_amd import backend, build
    assert "pdegym_gae" in N.EXPORTS and "pdegym_gae.hip" in build.SOURCES and N.ABI_VERSION == 21
    assert os.path.exists(os.path.join(build.CSRC, "pdegym_gae.hip"))
    assert "DeviceRolloutBuffer" in pde_control_gym.__all__ and pde_control_gym.DeviceRolloutBuffer.__module__ == "pde_control_gym.rollout_buffer"
    assert hasattr(backend.HipBackend.gae, "device_guard_key")
    header = open(os.path.join(ROOT, "include", "pdegym.h")).read()
    assert "#define PDEGYM_ABI_VERSION 21" in header
    doc = header[header.index("GAE(lambda)"):header.index("int pdegym_gae(")]
    assert "compute_returns_and_advantage" in doc and "collect_rollouts" in doc
    # the ctypes mirror follows the header's structure field for field
    import re
    body = re.search(r"typedef struct pdegym_gae_args \{(.*?)\} pdegym_gae_args;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for d in filter(None, (x.strip() for x in body.split(";"))):
        d = re.sub(r"^(const\s+)?(int32_t|int64_t|uint8_t|float|double|void)\s*\*?", "", d).strip()
        names += [x.strip().lstrip("*") for x in d.split(",")]
    assert names == [f[0] for f in N.Gae._fields_] and len(names) == 16
    for text, where in ((open(os.path.join(ROOT, "README.md")).read(), "README.md"), (open(os.path.join(ROOT, "DESIGN.md")).read(), "DESIGN.md"),
                        (open(os.path.join(ROOT, "INTEGRATION.md")).read(), "INTEGRATION.md")):
        assert "DeviceRolloutBuffer" in text and "pdegym_gae" in text, where
    assert "4.12" in open(os.path.join(ROOT, "DESIGN.md")).read()


def test_the_ppo_example_uses_the_buffer():
    src = open(os.path.join(ROOT, "examples", "train_ppo_device.py")).read()
    assert "DeviceRolloutBuffer" in src and "finished_episodes()" in src and "for t in reversed(range(T))" not in src


# ---- argument validation of the entry point, host half under ASan + UBSan ----------------------------------------------------------
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="needs hipcc")
def test_gae_entry_point_validates_its_arguments_under_asan_and_ubsan(tmp_path):
    """tests/c/gae_validation.c (its own main) against the host half of pdegym_gae.hip + pdegym_abi.hip, compiled with
    --cuda-host-only and the sanitizers and given an empty device image: every bad call must answer with a negative code and a
    message, a well-formed descriptor fails only at the launch, and no call reaches a device."""
    from pdecontrolgym_amd import build
    hipcc = shutil.which("hipcc")
    inc = ["-I" + os.path.join(ROOT, "include"), "-I" + build.CSRC]
    objs = []
    for s in ("pdegym_abi.hip", "pdegym_gae.hip"):
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
    lib = str(tmp_path / "libpdegym_gae_asan.so")
    r = subprocess.run([hipcc, "-shared", "-fPIC"] + SAN + ["-o", lib] + objs + [stub_o], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()[-3000:]
    exe = str(tmp_path / "gae_validation")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    r = subprocess.run([hipcc, "-x", "c", "-std=c11", "-Wall", "-Werror", "-g"] + SAN
                       + [os.path.join(ROOT, "tests", "c", "gae_validation.c"), "-I" + os.path.join(ROOT, "include"),
                          "-L" + str(tmp_path), "-lpdegym_gae_asan", "-Wl,-rpath," + str(tmp_path),
                          "-Wl,-rpath," + os.path.join(rocm, "lib"), "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1", HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, env=env, timeout=120)
    out = r.stdout.decode()
    assert r.returncode == 0 and "GAE-VALIDATION-OK" in out, out[-4000:]
    assert "runtime error" not in out and "AddressSanitizer" not in out, out[-4000:]
    assert int(out.strip().splitlines()[-2].split()[1]) >= 40, out[-1000:]
