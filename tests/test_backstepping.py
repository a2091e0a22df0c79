"""CPU tests of the backstepping baseline: the NumPy restatement of the reference's two gain recursions (the yardstick of
tests/test_gpu_backstepping.py for sizes the goldens do not hold) against tests/golden/kat.npz, and the host face
``pde_control_gym.BacksteppingController`` -- constructor / attach errors and the pool-row rule -- on a small NumPy double of the
backend.  The stand-alone validation program tests/c/backstep_validation.c runs here as well, on the host half of the library
built with AddressSanitizer and UBSan.  No kernel is launched."""
import math
import os
import shutil
import subprocess
import types

import numpy as np
import pytest

torch = pytest.importorskip("torch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, f64 = np.float32, np.float64


# ---- the reference's recursions, restated with every NumPy >= 2 promotion written out --------------------------------------------
def cheb_theta(x, gamma, amp):
    """solveBetaFunction of the two example scripts: amp*cos(gamma*acos(x)) in Python doubles, stored as float32."""
    out = np.zeros(len(x), dtype=f32)
    for i, v in enumerate(x):
        out[i] = amp * math.cos(gamma * math.acos(v))
    return out


def gain_transport(theta, dx):
    """transport1Dbackstepping.py:22-29: kappa[i] = (sum_{j<i} (kappa[i-j]*theta[j])*dx) - theta[i], added left to right from 0
    (the j = 0 term reads the not yet written kappa[i] = 0), flipped.  theta [m] or [R, m]: rows are independent, every operation
    is elementwise over them."""
    theta = np.asarray(theta, dtype=f32)
    th = np.atleast_2d(theta).astype(f64)           # kappa (float64) * theta[j] (float32) is a float64 product
    R, m = th.shape
    kap, dx = np.zeros((R, m)), f64(dx)
    for i in range(m):
        s = np.zeros(R)
        for j in range(i):
            s = s + (kap[:, i - j] * th[:, j]) * dx
        kap[:, i] = s - th[:, i]
    return kap[:, ::-1].copy().reshape(theta.shape)


def gain_parabolic(a, dx):
    """reactionDiffusion1DBackstepping.py:22-35, last row only.  a[j] is a float32 scalar: the Python doubles dx, dx/4.0, dx/2 and
    dx**2 are cast to float32 where they meet it, and those float32 values only then join the float64 k.  a [m] or [R, m]."""
    a2 = np.atleast_2d(np.asarray(a, dtype=f32))
    R, m = a2.shape
    dxf, dx4, dx2, dxsq = f32(dx), f32(dx / 4.0), f32(dx / 2), f32(dx ** 2)
    prev, cur = np.zeros((R, m)), np.zeros((R, m))
    cur[:, 1] = (((-(a2[:, 1] + a2[:, 0])) * dxf) / f32(4)).astype(f64)
    for i in range(1, m - 1):
        nxt = np.zeros((R, m))
        nxt[:, i + 1] = cur[:, i] - (dx4 * (a2[:, i - 1] + a2[:, i])).astype(f64)
        nxt[:, i] = cur[:, i] - (dx2 * a2[:, i]).astype(f64)
        j = np.arange(1, i)
        r, l = cur[:, j + 1], cur[:, j - 1]
        nxt[:, j] = ((-prev[:, j] + r) + l) + ((a2[:, j] * dxsq).astype(f64) * (r + l)) / 2.0
        prev, cur = cur, nxt
    return cur.reshape(np.shape(a))


GAIN = {"transport": gain_transport, "parabolic": gain_parabolic}


def law_ordered(gain, obs, length, scale):
    """solveControl of either script: products added left to right from 0, then the scale."""
    s = f64(0.0)
    for i in range(length):
        s = s + f64(gain[i]) * f64(obs[i])
    return s * f64(scale)


def rule_row(b, restarts, B, P):
    """Pool row instance b runs on after `restarts` restarts (None = its initial row): the k-th restart (k = 0, 1, ...) takes row
    (b + k*B) mod P (include/pdegym.h, pdegym_bufs1d), so the running episode came from k = restarts - 1."""
    return None if restarts == 0 else (b + (restarts - 1) * B) % P


# ---- the yardstick itself -----------------------------------------------------------------------------------------------------------
def test_restatement_reproduces_the_reference_gains_bitwise(golden_kat):
    kt = gain_transport(cheb_theta(np.linspace(1e-2, 1, 100), 7.35, 5), 1e-2)
    assert kt.dtype == np.float64 and np.array_equal(kt, golden_kat["T_u1"].kernel)
    assert np.array_equal(kt, golden_kat["T_u10"].kernel)
    kp = gain_parabolic(cheb_theta(np.linspace(5e-3, 1, 200), 8, 50), 5e-3)
    assert kp.dtype == np.float64 and np.array_equal(kp, golden_kat["P_u1"].kernel_row)
    assert np.array_equal(kp, golden_kat["P_u10"].kernel_row)


def test_promoting_theta_to_float64_would_miss_the_golden(golden_kat):
    """The float32 stages matter: the same recursion with theta in float64 throughout moves the last row (1.4e-7 absolute)."""
    a = cheb_theta(np.linspace(5e-3, 1, 200), 8, 50).astype(f64)
    dx, m = 5e-3, 200
    prev, cur = np.zeros(m), np.zeros(m)
    cur[1] = -(a[1] + a[0]) * dx / 4
    for i in range(1, m - 1):
        nxt = np.zeros(m)
        nxt[i + 1] = cur[i] - dx / 4.0 * (a[i - 1] + a[i])
        nxt[i] = cur[i] - dx / 2 * a[i]
        j = np.arange(1, i)
        nxt[j] = -prev[j] + cur[j + 1] + cur[j - 1] + a[j] * (dx ** 2) * (cur[j + 1] + cur[j - 1]) / 2
        prev, cur = cur, nxt
    d = np.abs(cur - golden_kat["P_u1"].kernel_row).max()
    assert 1e-8 < d < 1e-6


def test_degenerate_sizes_of_the_restatement():
    a = np.array([3.0, -2.0, 0.5], dtype=f32)
    k2 = gain_parabolic(a[:2], 1e-2)
    assert k2[0] == 0.0 and k2[1] == f64(((-(a[1] + a[0])) * f32(1e-2)) / f32(4))
    k3 = gain_parabolic(a, 1e-2)
    assert k3[0] == 0.0 and k3[1] == k2[1] - f64(f32(1e-2 / 2) * a[1]) and k3[2] == k2[1] - f64(f32(1e-2 / 4.0) * (a[0] + a[1]))
    t2 = gain_transport(a[:2], 1e-2)
    assert t2[1] == -3.0 and t2[0] == (0.0 + (0.0 * 3.0) * 1e-2) - (-2.0)


# ---- the host face on a NumPy double of the backend --------------------------------------------------------------------------------
class BackstepDouble:
    """What BacksteppingController asks of a backend, in NumPy on CPU tensors; records the calls."""

    def __init__(self):
        self.calls = []

    def backstep_gain(self, kind, theta, gain, dx):
        self.calls.append(("gain", kind, tuple(theta.shape)))
        for r in range(theta.shape[0]):
            gain[r] = torch.from_numpy(GAIN[kind](theta[r].numpy(), dx))

    def backstep_control(self, obs, out, gain0, length, scale, ordered=False, gain_pool=None, reset_count=None, noise=None, clamp=None):
        self.calls.append(("control", length, scale, ordered, gain_pool is not None))
        B = obs.shape[0]
        for b in range(B):
            g = gain0 if gain0.dim() == 1 else gain0[b]
            if gain_pool is not None:
                row = rule_row(b, int(reset_count[b]), B, gain_pool.shape[0])
                g = g if row is None else gain_pool[row]
            a = law_ordered(g.numpy(), obs[b].numpy(), length, scale)
            if out.dtype == torch.float64:
                out.view(-1)[b] = float(a)
            else:
                v = f32(a) + (f32(noise.view(-1)[b]) if noise is not None else f32(0))
                out.view(-1)[b] = float(np.clip(v, *clamp) if clamp is not None else v)


def _venv(kind="transport", n=8, B=3, obs_dim=None, pool_rows=0, beta_pool=True, flux="linear"):
    t = {"reset_init": None, "reset_beta": None, "reset_count": None}
    if pool_rows:
        t["reset_init"] = torch.zeros(pool_rows, n)
        t["reset_beta"] = torch.zeros(pool_rows, n) if beta_pool else None
        t["reset_count"] = torch.zeros(B, dtype=torch.int32)
    core = types.SimpleNamespace(kind=kind, flux=flux, n=n, obs_dim=n if obs_dim is None else obs_dim, num_envs=B, t=t)
    return types.SimpleNamespace(core=core, kind=kind)


def _ctrl(kind="transport", theta=None, dx=0.125, **kw):
    from pde_control_gym import BacksteppingController
    if theta is None:
        theta = np.linspace(1, 2, 8, dtype=f32)
    return BacksteppingController(kind, theta, dx, device="cpu", backend=BackstepDouble(), **kw)


def test_constructor_computes_gains_once_per_row_and_keeps_the_shape():
    rng = np.random.default_rng(0)
    theta = rng.uniform(-2, 2, (3, 8)).astype(f32)
    pool = rng.uniform(-2, 2, (5, 8)).astype(f32)
    for kind in ("transport", "parabolic"):
        c = _ctrl(kind, theta, pool_theta=pool)
        assert c.gain.shape == (3, 8) and c.gain.dtype == torch.float64 and c.pool_gain.shape == (5, 8)
        for r in range(3):
            assert np.array_equal(c.gain[r].numpy(), GAIN[kind](theta[r], 0.125))
        assert [k[0] for k in c.backend.calls] == ["gain", "gain"]
    c = _ctrl("parabolic")
    assert c.gain.shape == (8,) and c.scale == 0.125 and _ctrl("transport").scale == 1e-2


def test_constructor_and_attach_errors_say_why():
    from pde_control_gym import BacksteppingController
    with pytest.raises(ValueError, match="kind must be one of"):
        BacksteppingController("traffic", np.ones(8, dtype=f32), 0.1, device="cpu", backend=BackstepDouble())
    with pytest.raises(ValueError, match="order must be"):
        _ctrl(order="pairwise")
    with pytest.raises(ValueError, match="m >= 2"):
        _ctrl(theta=np.ones(1, dtype=f32))
    with pytest.raises(ValueError, match=r"pool_theta must be \[P, 8\]"):
        _ctrl(theta=np.ones((3, 8), dtype=f32), pool_theta=np.ones((4, 7), dtype=f32))
    with pytest.raises(ValueError, match=r"theta must be \[B, m\] as well"):
        _ctrl(pool_theta=np.ones((4, 8), dtype=f32))
    # a family other than the two 1D ones (no 1D engine behind it; Burgers is the transport engine with another flux)
    ns = types.SimpleNamespace(core=types.SimpleNamespace(), kind="ns2d")
    with pytest.raises(ValueError, match="TransportPDE1D and ReactionDiffusionPDE1D families only"):
        _ctrl().attach(ns)
    with pytest.raises(ValueError, match="families only"):
        _ctrl().attach(_venv(flux="burgers"))
    with pytest.raises(ValueError, match="cannot drive a parabolic environment"):
        _ctrl("transport").attach(_venv("parabolic"))
    with pytest.raises(ValueError, match="needs sensing_loc='full'"):
        _ctrl().attach(_venv(obs_dim=1))
    with pytest.raises(ValueError, match="theta has 3 rows, the environment 4 instances"):
        _ctrl(theta=np.ones((3, 8), dtype=f32)).attach(_venv(B=4))
    with pytest.raises(ValueError, match="theta has only 8"):
        _ctrl().attach(_venv(n=9))
    # pool rows: must be the environment's
    c = _ctrl(theta=np.ones((3, 8), dtype=f32), pool_theta=np.ones((4, 8), dtype=f32))
    with pytest.raises(ValueError, match="pool_theta has 4 rows, the environment's reset pool 5"):
        c.attach(_venv(pool_rows=5))
    with pytest.raises(ValueError, match="pool_theta has 4 rows, the environment's reset pool 0"):
        c.attach(_venv())
    with pytest.raises(ValueError, match="pool_theta was not given"):
        _ctrl(theta=np.ones((3, 8), dtype=f32)).attach(_venv(pool_rows=5))
    # a pool of initial conditions alone (beta fixed) needs no pool_theta
    assert _ctrl(theta=np.ones((3, 8), dtype=f32)).attach(_venv(pool_rows=5, beta_pool=False))._reset_count is None
    assert c.attach(_venv(pool_rows=4))._reset_count is not None


@pytest.mark.parametrize("kind", ["transport", "parabolic"])
def test_attached_controller_follows_the_pool_rule(kind):
    """B = 3, P = 4: after c restarts instance b uses pool gain (b + (c-1)*B) mod P, its own row before the first one; the law's
    length and scale are the scripts' (transport: every node, 1e-2; parabolic: min(m, n-1) nodes, dx)."""
    from pde_control_gym.backstepping import pool_row
    rng = np.random.default_rng(5)
    B, P, m, n = 3, 4, 8, 8
    theta, pool = rng.uniform(-2, 2, (B, m)).astype(f32), rng.uniform(-2, 2, (P, m)).astype(f32)
    venv = _venv(kind, n=n, B=B, pool_rows=P)
    c = _ctrl(kind, theta, pool_theta=pool).attach(venv)
    obs = torch.from_numpy(rng.uniform(1, 2, (B, n)).astype(f32))
    length, scale = (n, 1e-2) if kind == "transport" else (min(m, n - 1), 0.125)
    for counts in ([0, 0, 0], [1, 0, 2], [3, 5, 4]):
        venv.core.t["reset_count"].copy_(torch.tensor(counts, dtype=torch.int32))
        a = c(obs).numpy()
        for b in range(B):
            row = rule_row(b, counts[b], B, P)
            assert row == pool_row(b, counts[b], B, P)
            g = GAIN[kind](theta[b] if row is None else pool[row], 0.125)
            assert a[b] == law_ordered(g, obs[b].numpy(), length, scale)
    assert c.backend.calls[-1] == ("control", length, scale, False, True)
    # float32 output: rounded once, noise, then the clamp
    out, nz = torch.zeros(B), torch.tensor([0.5, -0.25, 100.0])
    c.forward_into(obs, out, clamp=(-3.0, 3.0), noise=nz)
    want = np.clip(a.astype(f32) + nz.numpy(), f32(-3), f32(3))
    assert np.array_equal(out.numpy(), want)


def test_one_launch_rollout_does_not_claim_the_controller():
    """DeviceRollout asks the environment whether a policy fits the one-launch kernels: only a FusedMLP does."""
    from pdecontrolgym_amd.batch1d import PDEBatch1D
    c = _ctrl()
    assert hasattr(c, "forward_into") and not hasattr(c, "layers") and not hasattr(c, "_net")
    core = types.SimpleNamespace(can_rollout=lambda: True, n=65, obs_dim=65)
    assert PDEBatch1D.policy_fits_rollout(core, c) is False


def test_every_backstep_kernel_has_an_output_contract_test():
    """The kernels of csrc/pdegym_backstep.hip keep their poisoned-buffer tests in tests/test_gpu_backstepping.py: every kernel
    launched there is listed in its KERNEL_CASES, and every test named exists."""
    import re
    from tests import test_gpu_backstepping as G
    src = open(os.path.join(ROOT, "pdecontrolgym_amd", "csrc", "pdegym_backstep.hip")).read()
    launched = set(re.findall(r"([A-Za-z_]\w*)\s*<[^<>;]*>\s*<<<", src))
    assert launched == set(G.KERNEL_CASES) and len(launched) == 3, launched ^ set(G.KERNEL_CASES)
    for k, tests in G.KERNEL_CASES.items():
        assert tests and all(callable(getattr(G, t, None)) for t in tests), (k, tests)


# ---- argument validation of the three entry points, host half under ASan + UBSan ---------------------------------------------------
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="needs hipcc")
def test_backstep_entry_points_validate_their_arguments_under_asan_and_ubsan(tmp_path):
    """tests/c/backstep_validation.c (its own main) against the host half of pdegym_backstep.hip + pdegym_abi.hip, compiled with
    --cuda-host-only and the sanitizers and given an empty device image: every bad call must answer with a negative code and a
    message, and no call reaches a device."""
    from pdecontrolgym_amd import build
    hipcc = shutil.which("hipcc")
    inc = ["-I" + os.path.join(ROOT, "include"), "-I" + build.CSRC]
    objs = []
    for s in ("pdegym_abi.hip", "pdegym_backstep.hip"):
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
    lib = str(tmp_path / "libpdegym_backstep_asan.so")
    r = subprocess.run([hipcc, "-shared", "-fPIC"] + SAN + ["-o", lib] + objs + [stub_o], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()[-3000:]
    exe = str(tmp_path / "backstep_validation")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    r = subprocess.run([hipcc, "-x", "c", "-std=c11", "-Wall", "-Werror", "-g"] + SAN
                       + [os.path.join(ROOT, "tests", "c", "backstep_validation.c"), "-I" + os.path.join(ROOT, "include"),
                          "-L" + str(tmp_path), "-lpdegym_backstep_asan", "-Wl,-rpath," + str(tmp_path),
                          "-Wl,-rpath," + os.path.join(rocm, "lib"), "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1", HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, env=env, timeout=120)
    out = r.stdout.decode()
    assert r.returncode == 0 and "BACKSTEP-VALIDATION-OK" in out, out[-4000:]
    assert "runtime error" not in out and "AddressSanitizer" not in out, out[-4000:]
