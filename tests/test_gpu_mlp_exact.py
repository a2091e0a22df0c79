"""The MLP policy kernels pinned bit for bit: pdegym_mlp_forward (csrc/pdegym_mlp.hip, pdegym_mlp_tile.h) and the evaluators inside the
rollout kernels (csrc/pdegym_policy.h: ``eval``, one neuron per lane over its own LDS weight layout, and ``eval_wide``, the cooperative
MFMA form) against a float64 NumPy reference, on inputs for which float32 arithmetic is exact (tests/mlp_exact.py: exactly summable
networks and one-hot probes with real weights).  Every comparison is ``assert_array_equal``, except behind a tanh head, whose exact
pre-activation is compared through float64 ``np.tanh`` at the policy tolerance of tests/test_policy.py.

The case lists live in tests/mlp_exact.py; tests/test_mlp_exact_helper.py checks on the CPU that each keeps the exactness bound and
is not blind.  What they reach in the kernels: first-layer widths on both sides of the pipeline swaps (64, 128, 576 = 512 + 64), of
the observation chunks (512, 1024, ... 8192: the weight pipeline inside a later chunk, third and later chunks), K % 4 == 2; layer
widths on both sides of the 4 / 8 / 16-wave launches and of the 16-neuron tiles, as hidden and as last layer; batches around the row
tile (15, 16, 17); row strides longer than the rows, over poisoned gaps; noise and a binding clamp; float64 rows in and out."""
import functools

import numpy as np
import pytest

from tests import mlp_exact as mx
from tests import poison

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

F32, F64, U8 = torch.float32, torch.float64, torch.uint8


def _compare(case, got, want, what="output"):
    got = np.asarray(got, np.float64).reshape(want.shape)
    if case.tanh:
        np.testing.assert_allclose(got, want, rtol=mx.TANH_RTOL, atol=mx.TANH_ATOL, err_msg=f"{case.name}: {what}")
    else:
        np.testing.assert_array_equal(got, want, err_msg=f"{case.name}: {what}")


# ---- (a) pdegym_mlp_forward on exactly summable networks ------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", mx.FORWARD_CASES, ids=[c.name for c in mx.FORWARD_CASES])
def test_forward_kernel_is_exact(case, policy=None):
    """Every buffer in a guarded allocation; with ``gaps`` the rows sit in wider, poisoned rows (x_stride > K, y_stride > out_dim,
    noise_stride > out_dim): a read of a gap turns the output into NaN, a store into one is found.
    ``policy`` displaces every guarded buffer off its 256-byte boundary (tests/poison.py; tests/test_gpu_pointer_alignment.py)."""
    from pdecontrolgym_amd.policy import FusedMLP
    b = mx.build(case)
    B, K, out = case.B, case.sizes[0], case.sizes[-1]
    gx, gy, gn = (5, 3, 2) if case.gaps else (0, 0, 0)
    arena = poison.Arena("cuda", policy=policy)
    xbig = poison.poison_(arena.new("x", (B, K + gx), F64 if case.x_f64 else F32))
    ybig = poison.poison_(arena.new("y", (B, out + gy), F64 if case.y_f64 else F32))
    xbig[:, :K] = torch.from_numpy(b.x_dev)
    nbig = None
    if b.noise is not None:
        nbig = poison.poison_(arena.new("noise", (B, out + gn), F32))
        nbig[:, :out] = torch.from_numpy(b.noise)
    pol = FusedMLP(b.net.cuda(), clamp=b.clamp)
    x, y = xbig[:, :K], ybig[:, :out]
    assert x.stride(0) == K + gx and y.stride(0) == out + gy
    pol.forward_into(x, y, noise=None if nbig is None else nbig[:, :out])
    arena.check()
    poison.assert_written(ybig, (slice(None), slice(0, out)), "y")
    if case.gaps:
        poison.assert_untouched(ybig, (slice(None), slice(out, None)), "the gap of the output rows")
        poison.assert_untouched(xbig, (slice(None), slice(K, None)), "the gap of the input rows")
        if nbig is not None:
            poison.assert_untouched(nbig, (slice(None), slice(out, None)), "the gap of the noise rows")
    assert np.array_equal(xbig[:, :K].cpu().numpy(), b.x_dev), "the input rows were changed"
    _compare(case, y.cpu().numpy(), b.want)


# ---- (b) one-hot probes with real weights --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,H,rows", mx.ONE_HOT_CASES, ids=[f"K{K}-H{H}-{r or 'all'}" for K, H, r in mx.ONE_HOT_CASES])
def test_forward_kernel_one_hot_rows_return_the_weight_columns(K, H, rows):
    """y[r, j] = float32(W[j, k(r)]) + float32(b[j]) for every input index k (B = K rows), or for the indices around every chunk and
    pipeline seam (K = 2049, 8192): the blocked transpose, the weight addressing, full float32 operands."""
    from pdecontrolgym_amd.policy import FusedMLP
    ks = np.arange(K) if rows is None else np.array(mx.seam_ks(K))
    lin = mx.real_linear(K, H, seed=1000 * K + H, bias=(K + H) % 3 != 0)
    want = mx.one_hot_expected(lin.weight.detach().numpy(), None if lin.bias is None else lin.bias.detach().numpy(), ks)
    x = torch.from_numpy(mx.one_hot_rows(K, ks, np.float64 if H == 17 else np.float32)).cuda()
    got = FusedMLP(lin.cuda())(x)
    np.testing.assert_array_equal(got.float().cpu().numpy(), want)


# ---- (c) the evaluators inside the rollout kernels -----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _env_1d(kind, control, loc, n, B):
    import pde_control_gym
    from pde_control_gym.src import TunedReward1D
    parabolic = "Reaction" in kind
    nx = n - 1 if parabolic else n
    dx = 1.0 / nx
    dt = 0.25 * dx * dx if parabolic else 0.5 * dx
    S, horizon = 3, 40
    beta = np.full(n, 2.0, np.float32)
    p = {"T": horizon * S * dt, "dt": dt, "X": 1, "dx": dx, "reward_class": TunedReward1D(horizon * S, -1e3, 3e2), "normalize": True,
         "sensing_loc": loc, "control_type": control, "sensing_type": None, "sensing_noise_func": None,
         "limit_pde_state_size": True, "max_state_value": 1e10, "max_control_value": 5, "control_sample_rate": S * dt,
         "batched_reset_func": lambda idx, nx_: (np.ones((len(idx), n), np.float32), np.tile(beta, (len(idx), 1)))}
    venv = pde_control_gym.make_vec(kind, num_envs=B, **p)
    venv.reset_tensor()
    venv.enable_fused_auto_reset()
    assert venv.core.n == n and venv.core.can_rollout()
    return venv


def _policy(b, T, A=None):
    """FusedMLP of the built case on the device, and its noise as the [T, B] / [T, B, A] tensor of the rollout (step 0: the case's)."""
    from pdecontrolgym_amd.policy import FusedMLP
    pol = FusedMLP(b.net.cuda(), clamp=b.clamp)
    nz = None
    if b.noise is not None:
        B = b.noise.shape[0]
        nz = torch.zeros((T, B) if A is None else (T, B, A), dtype=F32, device="cuda")
        nz[0] = torch.from_numpy(b.noise).cuda().reshape(nz[0].shape)
    return pol, nz


def _forward_of(pol, rows, nz0, dtype):
    """pdegym_mlp_forward on the same rows: what a wide policy inside a rollout kernel must return bit for bit."""
    out = torch.empty(rows.shape[0], pol.out_dim, dtype=dtype, device="cuda")
    pol.forward_into(rows.clone(), out, noise=None if nz0 is None else nz0.reshape(rows.shape[0], pol.out_dim))
    return out


def _rollout_1d(case, b, x32):
    _, kind, control, loc, n = case.env
    B, T = case.B, 2
    core = _env_1d(kind, control, loc, n, B).core
    od = core.obs_dim
    assert od == case.sizes[0] == x32.shape[1]
    pol, nz = _policy(b, T)
    assert core.policy_fits_rollout(pol)
    obs = torch.zeros(T + 1, B, od, dtype=F32, device="cuda")
    obs[0] = torch.from_numpy(x32)
    act = poison.poison_(torch.empty(T, B, dtype=F32, device="cuda"))
    z = lambda dt: torch.zeros(T, B, dtype=dt, device="cuda")      # noqa: E731
    core.rollout(obs, act, z(F32), z(U8), z(U8), policy=pol, noise=nz)
    torch.cuda.synchronize()
    poison.assert_written(act, None, "actions")
    assert np.array_equal(obs[0].cpu().numpy(), x32), "observation slot 0 was changed"
    return pol, obs[0], None if nz is None else nz[0], act[0], F32


def _rollout_traffic(case, b):
    from pdecontrolgym_amd.batch_traffic import TrafficBatch
    sim = case.env[1]
    B, T = case.B, 2
    env = TrafficBatch(240, 0.25, 500, 10, sim, 40, 0.16, 60, True, 2, num_envs=B, device="cuda")
    rs = np.full(B, 0.12)
    env.set_action_bounds(rs * (40 * (1 - rs / 0.16)))
    env.reset(rs)
    A, D = env.action_dim, 2 * env.M
    assert D == case.sizes[0] and A == case.sizes[-1]
    pol, nz = _policy(b, T, A)
    assert env.policy_fits_rollout(pol)
    obs = torch.zeros(T + 1, B, D, dtype=F64, device="cuda")
    obs[0] = torch.from_numpy(b.x_dev)
    act = poison.poison_(torch.empty(T, B, A, dtype=F64, device="cuda"))
    env.rollout(obs, act, torch.zeros(T, B, dtype=F64, device="cuda"), torch.zeros(T, B, dtype=U8, device="cuda"),
                torch.zeros(T, B, dtype=U8, device="cuda"), policy=pol, noise=nz)
    torch.cuda.synchronize()
    poison.assert_written(act, None, "actions")
    return pol, obs[0], None if nz is None else nz[0], act[0], F64


@functools.lru_cache(maxsize=None)
def _env_tumor(nx, B):
    from tests.test_gpu_tumor_rollout import _venv
    return _venv(nx, 600, True, num_envs=B)


def _rollout_tumor(case, b):
    nx = case.env[1]
    B, T = case.B, 1
    venv = _env_tumor(nx, B)
    core = venv.core
    pol, nz = _policy(b, T)
    assert core.policy_fits_rollout(pol)
    obs = torch.zeros(T + 1, B, nx, dtype=F64, device="cuda")
    obs[0] = torch.from_numpy(b.x_dev)
    act = poison.poison_(torch.empty(T, B, dtype=F64, device="cuda"))
    core.rollout(obs, act, torch.zeros(T, B, dtype=F64, device="cuda"), torch.zeros(T, B, dtype=U8, device="cuda"),
                 torch.zeros(T, B, dtype=U8, device="cuda"), policy=pol, noise=nz, wrap_state=dict(venv._wrapper_state()))
    torch.cuda.synchronize()
    poison.assert_written(act, None, "actions")
    return pol, obs[0], None if nz is None else nz[0], act[0], F64


@pytest.mark.parametrize("case", mx.ROLLOUT_CASES, ids=[c.name for c in mx.ROLLOUT_CASES])
def test_policy_inside_the_rollout_kernels_is_exact(case):
    """actions[0] of a short rollout whose first observation holds the case's dyadic values == the float64 reference, noise and clamp
    included.  Layers of at most 64 units: ``stage()``'s LDS layout [neuron][group | 1][4] and ``eval``'s fma chain.  Wider: ``eval_wide``
    (batches that are no multiple of 16 leave a workgroup with waves that only attend the barriers, their rows zero), which must also
    return the bits of pdegym_mlp_forward for the same rows."""
    b = mx.build(case)
    if case.env[0] == "1d":
        pol, rows, nz0, got, dt = _rollout_1d(case, b, b.x.astype(np.float32))
    elif case.env[0] == "traffic":
        pol, rows, nz0, got, dt = _rollout_traffic(case, b)
    else:
        pol, rows, nz0, got, dt = _rollout_tumor(case, b)
    assert got.dtype == dt
    _compare(case, got.cpu().numpy(), b.want, "actions[0]")
    if max(case.sizes[1:]) > 64:
        fwd = _forward_of(pol, rows, nz0, dt)
        assert torch.equal(poison.bits(got.reshape(fwd.shape).contiguous()), poison.bits(fwd)), "eval_wide differs from pdegym_mlp_forward"


@pytest.mark.parametrize("n", mx.ONE_HOT_ROLLOUT_NODES)
def test_narrow_evaluator_one_hot_rows_return_the_weights(n):
    """One Linear layer n -> 1 with real float32 weights inside the parabolic rollout kernel, instance r observing the unit vector e_r:
    actions[0][r] = float32(W[0, r]) + float32(b) -- stage()'s re-layout of the blocked weights with non-integer values, exactly."""
    lin = mx.real_linear(n, 1, seed=n)
    ks = np.arange(n)
    want = mx.one_hot_expected(lin.weight.detach().numpy(), lin.bias.detach().numpy(), ks)
    case = mx.Case(f"one-hot-{n}", (n, 1), (None,), n, env=("1d", "PDEControlGym-ReactionDiffusionPDE1D", "Dirchilet", "full", n))
    b = mx.Built(lin, None, None, None, None, want.astype(np.float64), [], None)
    _, _, _, got, _ = _rollout_1d(case, b, mx.one_hot_rows(n, ks))
    np.testing.assert_array_equal(got.cpu().numpy(), want[:, 0])
