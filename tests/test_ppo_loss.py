"""CPU tests of the PPO loss head (include/pdegym.h: pdegym_ppo_loss, pdegym_diag_gaussian_log_prob; pde_control_gym.PPOLoss): the
float64 NumPy restatement with its closed-form gradients against torch float64 autograd over SB3's expression, boundary rows
included; a fake backend built on the restatement drives the head's host logic on CPU tensors; the new names are exported; and
tests/c/ppo_loss_validation.c runs against the host half of the library under AddressSanitizer and UBSan.  No kernel is launched;
the kernels are pinned to the restatements in tests/test_gpu_ppo_loss.py."""
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import ppo_loss_restatement as R
from tests.fake_ppo_loss_backend import FakePPOLossBackend

torch = pytest.importorskip("torch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLIP, ENT, VF = 0.2, 1e-3, 0.5


def sb3_loss(mean, log_std, values, actions, old_log_prob, advantages, returns, clip_range, ent_coef, vf_coef, normalize):
    """PPO.train's loss (stable_baselines3/ppo/ppo.py) for a DiagGaussianDistribution, on torch tensors of any float dtype; returns
    (loss, dict of the statistics)."""
    F = torch.nn.functional
    adv = advantages
    adv_mean, adv_std = torch.zeros((), dtype=adv.dtype), torch.ones((), dtype=adv.dtype)
    if normalize and len(adv) > 1:
        adv_mean, adv_std = adv.mean(), adv.std()
        adv = (adv - adv_mean) / (adv_std + 1e-8)
    dist = torch.distributions.Normal(mean, torch.ones_like(mean) * log_std.exp())
    log_prob = dist.log_prob(actions).sum(dim=1)
    ratio = torch.exp(log_prob - old_log_prob)
    policy_loss = -torch.min(adv * ratio, adv * torch.clamp(ratio, 1 - clip_range, 1 + clip_range)).mean()
    value_loss = F.mse_loss(returns, values) if values is not None else torch.zeros((), dtype=mean.dtype)
    entropy_loss = -torch.mean(dist.entropy().sum(dim=1))
    loss = policy_loss + ent_coef * entropy_loss + vf_coef * value_loss
    with torch.no_grad():
        log_ratio = log_prob - old_log_prob
        stats = {"loss": loss, "policy_loss": policy_loss, "value_loss": value_loss, "entropy_loss": entropy_loss,
                 "approx_kl": torch.mean((torch.exp(log_ratio) - 1) - log_ratio),
                 "clip_fraction": torch.mean((torch.abs(ratio - 1) > clip_range).to(mean.dtype)), "adv_mean": adv_mean, "adv_std": adv_std}
    return loss, stats


def _boundary_case(n, A, seed):
    """A float64 case with the boundary rows of the min / clamp planted (n >= 37): in rows 0 .. 3 the ratio is EXACTLY 1 + c and
    1 - c with both signs of the advantage, and the last two rows have advantages of exactly +0 and -0.  torch's expression and the
    restatement round the log-probability differently, and a ratio sits exactly on the boundary in both only where the two agree to
    the last bit AND some old_log_prob next to logp - log(1 +- c) hits the target: the actions of a planted row are drawn
    again (seeded) until both hold (the plant is asserted by the test)."""
    c = R.seeded_case(n, A, seed=seed)
    case = {k: (v.astype(np.float64) if isinstance(v, np.ndarray) else v) for k, v in c.items()}
    rng = np.random.default_rng(seed)
    if n >= 37:
        # log-probabilities of the planted rows below 1 in magnitude: logp - old_log_prob then moves in steps fine enough to land on
        # an argument whose exp is the target (with |logp| in [2, 4) the steps are 2^-51, wider than the 1.8e-16 the target allows)
        case["log_std"] = rng.uniform(-0.95, -0.89, A)
    logp = R.log_prob_float64(case["mean"], case["log_std"], case["actions"])
    case["old_log_prob"] = logp - rng.normal(0.0, 0.3, n)
    if n < 37:
        return case
    t = lambda x: torch.tensor(x, dtype=torch.float64)      # noqa: E731
    std_t = t(case["log_std"]).exp()
    for row, (target, sign) in enumerate(((1.0 + CLIP, 1.0), (1.0 + CLIP, -1.0), (1.0 - CLIP, 1.0), (1.0 - CLIP, -1.0))):
        found = False
        for _ in range(5000):
            case["actions"][row] = case["mean"][row] + rng.normal(0.0, 0.1, A)
            lp = float(R.log_prob_float64(case["mean"][row:row + 1], case["log_std"], case["actions"][row:row + 1])[0])
            lp_t = float(torch.distributions.Normal(t(case["mean"][row:row + 1]), std_t).log_prob(t(case["actions"][row:row + 1])).sum(1)[0])
            if lp != lp_t:
                continue
            old = lp - math.log(target)
            for _ in range(3):
                old = np.nextafter(old, -np.inf)
            for _ in range(7):
                if float(np.exp(lp - old)) == target and float(torch.exp(t(lp - old))) == target:
                    found = True
                    break
                old = np.nextafter(old, np.inf)
            if found:
                break
        assert found, f"no exact plant for row {row}"
        case["old_log_prob"][row] = old
        case["advantages"][row] = sign * (1.0 + row)
    case["advantages"][n - 2] = 0.0
    case["advantages"][n - 1] = -0.0
    return case


def _compare_with_autograd(case, normalize, with_values=True):
    t = lambda x: torch.tensor(x, dtype=torch.float64)      # noqa: E731
    mean, log_std = t(case["mean"]).requires_grad_(), t(case["log_std"]).requires_grad_()
    values = t(case["values"]).requires_grad_() if with_values else None
    loss, stats = sb3_loss(mean, log_std, values, t(case["actions"]), t(case["old_log_prob"]), t(case["advantages"]), t(case["returns"]),
                           CLIP, ENT, VF, normalize)
    loss.backward()
    got = R.head_float64(case["mean"], case["log_std"], case["values"] if with_values else None, case["actions"], case["old_log_prob"],
                         case["advantages"], case["returns"], CLIP, ENT, VF, normalize)

    def close(a, b, what):
        a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
        scale = max(np.abs(b).max(), 1e-300)
        assert np.abs(a - b).max() <= 1e-12 * scale, (what, np.abs(a - b).max() / scale)
    close(got["d_mean"], mean.grad.numpy(), "d_mean")
    close(got["d_log_std"], log_std.grad.numpy(), "d_log_std")
    if with_values:
        close(got["d_values"], values.grad.numpy(), "d_values")
    else:
        assert got["d_values"] is None and got["stats"][2] == 0.0
    for i, name in enumerate(R.STATS):
        want = float(stats[name].detach())
        assert abs(got["stats"][i] - want) <= 1e-12 * abs(want), (name, got["stats"][i], want)
    return got


@pytest.mark.parametrize("normalize", [False, True], ids=["raw", "normalised"])
@pytest.mark.parametrize("n", [1, 37])
@pytest.mark.parametrize("A", [1, 3, 8])
def test_float64_restatement_equals_autograd_over_the_sb3_expression(A, n, normalize):
    case = _boundary_case(n, A, seed=A)
    got = _compare_with_autograd(case, normalize)
    if n >= 37 and not normalize:
        ratio, rows = got["ratio"], [0, 1, 2, 3]
        assert ratio[rows].tolist() == [1.0 + CLIP, 1.0 + CLIP, 1.0 - CLIP, 1.0 - CLIP], ratio[rows]
        assert (got["g"][rows] != 0).all(), "on the closed interval the clamp passes the gradient"
        assert (got["g"][-2:] == 0).all() and (got["d_mean"][-2:] == 0).all()
        assert ((ratio > 1.0 + CLIP) & (got["adv"] > 0)).any() and ((ratio < 1.0 - CLIP) & (got["adv"] < 0)).any(), "no clipped row"
    if n == 1:
        assert got["stats"][6] == 0.0 and got["stats"][7] == 1.0, "a single row is not normalised (SB3)"
    _compare_with_autograd(case, normalize, with_values=False)


def test_equal_advantages_have_zero_deviation_in_both_restatements():
    case = _boundary_case(37, 3, seed=5)
    case["advantages"][:] = 0.75      # (a mean that float64 forms exactly: with 0.7 torch and NumPy each divide their own rounding noise by 1e-8)
    got = _compare_with_autograd(case, True)
    assert got["stats"][7] == 0.0 and (got["adv"] == 0).all() and (got["d_mean"] == 0).all()
    c32 = {k: (v.astype(np.float32) if isinstance(v, np.ndarray) else v) for k, v in case.items()}
    got32 = R.head_float32(c32["mean"], c32["log_std"], c32["values"], c32["actions"], c32["old_log_prob"], c32["advantages"],
                           c32["returns"], CLIP, ENT, VF, True)
    assert got32["stats"][7] == 0.0 and got32["stats"][6] == np.float32(0.75) and (got32["d_mean"] == 0).all()


@pytest.mark.parametrize("A", [1, 8])
def test_float32_restatement_is_the_float64_one_to_float32_accuracy(A):
    n, rows = 300, 900
    case = R.seeded_case(n, A, seed=3, rows=rows)
    index = np.random.default_rng(3).permutation(rows)[:n]
    case = R.with_old_log_prob_near(case, index)
    args = (case["mean"], case["log_std"], case["values"], case["actions"], case["old_log_prob"], case["advantages"], case["returns"],
            CLIP, ENT, VF, True)
    a, b = R.head_float32(*args, index=index), R.head_float64(*args, index=index)
    assert a["d_mean"].dtype == np.float32 and a["stats"].dtype == np.float32 and a["d_values"].dtype == np.float32
    for k in ("d_mean", "d_values", "d_log_std", "stats"):
        assert np.abs(a[k] - b[k]).max() <= 2e-5 * np.abs(b[k]).max(), k
    dense = {k: (v[index] if k in ("actions", "old_log_prob", "advantages", "returns") else v) for k, v in case.items()}
    d = R.head_float32(dense["mean"], dense["log_std"], dense["values"], dense["actions"], dense["old_log_prob"], dense["advantages"],
                       dense["returns"], CLIP, ENT, VF, True)
    for k in ("d_mean", "d_values", "d_log_std", "stats"):
        assert np.array_equal(a[k].view(np.int32), d[k].view(np.int32)), k
    # the log-probability restatement puts the ratio at exactly 1
    logp, _, _ = R.log_prob_float32(case["mean"], case["log_std"], case["actions"], index)
    same = dict(case, old_log_prob=case["old_log_prob"].copy())
    same["old_log_prob"][index] = logp
    s = R.head_float32(same["mean"], same["log_std"], None, same["actions"], same["old_log_prob"], same["advantages"], None, CLIP, 0.0,
                       VF, False, index=index)
    assert (s["ratio"] == 1).all() and s["stats"][4] == 0 and s["stats"][5] == 0
    assert s["stats"][1] == np.float32(-math.fsum(case["advantages"][index].astype(np.float64)) / n)


# ---- PPOLoss on the fake backend ---------------------------------------------------------------------------------------------------
def _torch_case(n, A, rows, seed):
    case = R.seeded_case(n, A, seed=seed, rows=rows)
    index = np.random.default_rng(seed).permutation(rows)[:n] if rows != n else None
    case = R.with_old_log_prob_near(case, index)
    t = {k: torch.from_numpy(v) for k, v in case.items() if isinstance(v, np.ndarray)}
    return t, (None if index is None else torch.from_numpy(index))


@pytest.mark.parametrize("A,rows", [(1, 60), (3, 60), (3, 20)])
def test_backward_fills_the_grads_autograd_gives_for_the_same_loss(A, rows):
    import pde_control_gym
    n, D = 20, 5
    t, index = _torch_case(n, A, rows, seed=2)
    torch.manual_seed(1)
    obs = torch.randn(n, D)
    actor = torch.nn.Sequential(torch.nn.Linear(D, 8), torch.nn.Tanh(), torch.nn.Linear(8, A))
    critic = torch.nn.Sequential(torch.nn.Linear(D, 8), torch.nn.Tanh(), torch.nn.Linear(8, 1))
    log_std = torch.nn.Parameter(t["log_std"].clone())
    params = list(actor.parameters()) + list(critic.parameters()) + [log_std]
    gather = (lambda x: x) if index is None else (lambda x: x[index])
    # old log-probabilities near the ACTOR's means (the case's were made for its own)
    with torch.no_grad():
        logp = torch.distributions.Normal(actor(obs), log_std.exp()).log_prob(gather(t["actions"])).sum(1)
        old = t["old_log_prob"].clone()
        old[index if index is not None else slice(None)] = logp - 0.3 * torch.randn(n)
    loss, stats = sb3_loss(actor(obs), log_std, critic(obs).squeeze(-1), gather(t["actions"]), gather(old), gather(t["advantages"]),
                           gather(t["returns"]), CLIP, ENT, VF, True)
    loss.backward()
    want = [p.grad.clone() for p in params]
    for p in params:
        p.grad = None
    head = pde_control_gym.PPOLoss(CLIP, ENT, VF, True, backend=FakePPOLossBackend())
    mean, values = actor(obs), critic(obs)                       # values [n, 1]: the head takes the column
    res = head(mean, log_std, values, t["actions"], old, t["advantages"], t["returns"], index=index)
    assert all(p.grad is None for p in params), "the head itself does not touch the graphs"
    res.backward()
    for p, w in zip(params, want):
        assert p.grad is not None and torch.allclose(p.grad, w, rtol=2e-4, atol=2e-7), (p.shape, (p.grad - w).abs().max())
    for name in R.STATS:
        x = getattr(res, name)
        assert x.dim() == 0 and x.data_ptr() == res.stats[R.STATS.index(name)].data_ptr()
        assert float(x) == pytest.approx(float(stats[name]), rel=2e-4, abs=2e-6), name
    assert ((stats["clip_fraction"] > 0) and (stats["clip_fraction"] < 1)), "the case clips some rows and not others"
    # a second backward() accumulates, as autograd does
    res2 = head(actor(obs), log_std, critic(obs), t["actions"], old, t["advantages"], t["returns"], index=index)
    res2.backward()
    assert torch.allclose(log_std.grad, 2 * want[-1], rtol=2e-4, atol=2e-7)
    assert torch.allclose(params[0].grad, 2 * want[0], rtol=2e-4, atol=2e-7)


def test_buffers_are_reused_and_the_value_term_is_optional():
    import pde_control_gym
    t, index = _torch_case(16, 2, 48, seed=4)
    bk = FakePPOLossBackend()
    head = pde_control_gym.PPOLoss(backend=bk)
    assert (head.clip_range, head.ent_coef, head.vf_coef, head.normalize_advantage) == (0.2, 0.0, 0.5, True)
    a = head(t["mean"], t["log_std"], t["values"], t["actions"], t["old_log_prob"], t["advantages"], t["returns"], index=index)
    b = head(t["mean"], t["log_std"], t["values"], t["actions"], t["old_log_prob"], t["advantages"], t["returns"], index=index)
    assert bk.calls == 2 and bk.seen[0] == bk.seen[1], "a second call with the same shapes reuses every output"
    assert a.grad_mean.data_ptr() == b.grad_mean.data_ptr() and a.stats.data_ptr() == b.stats.data_ptr()
    assert tuple(a.grad_mean.shape) == (16, 2) and tuple(a.grad_values.shape) == (16,) and tuple(a.grad_log_std.shape) == (2,)
    c = head(t["mean"], t["log_std"], None, t["actions"], t["old_log_prob"], t["advantages"], None, index=index)
    assert c.grad_values is None and float(c.value_loss) == 0.0 and bk.seen[2] != bk.seen[0]
    d = head(t["mean"][:8], t["log_std"], t["values"][:8], t["actions"], t["old_log_prob"], t["advantages"], t["returns"], index=index[:8])
    assert tuple(d.grad_mean.shape) == (8, 2) and bk.seen[3] != bk.seen[0]
    c.backward()                                                 # nothing requires grad: a no-op, not an error
    # log_prob: the restatement's values, written in place when out is given
    dense_actions = t["actions"][index]
    lp = head.log_prob(t["mean"], t["log_std"], dense_actions)
    want, _, _ = R.log_prob_float32(t["mean"].numpy(), t["log_std"].numpy(), dense_actions.numpy())
    assert np.array_equal(lp.numpy(), want)
    out = torch.zeros(4, 4)
    assert head.log_prob(t["mean"], t["log_std"], dense_actions, out=out) is out and np.array_equal(out.numpy().ravel(), want)
    # A = 1 written without the trailing axis
    t1, _ = _torch_case(12, 1, 12, seed=6)
    e = head(t1["mean"][:, 0], t1["log_std"], t1["values"], t1["actions"][:, 0], t1["old_log_prob"], t1["advantages"], t1["returns"])
    assert tuple(e.grad_mean.shape) == (12, 1)


def test_value_errors():
    import pde_control_gym
    t, index = _torch_case(16, 2, 48, seed=4)
    bk = FakePPOLossBackend()
    head = pde_control_gym.PPOLoss(backend=bk)
    ok = dict(mean=t["mean"], log_std=t["log_std"], values=t["values"], actions=t["actions"], old_log_prob=t["old_log_prob"],
              advantages=t["advantages"], returns=t["returns"], index=index)
    head(**ok)
    wide = torch.zeros(16, 9)
    bad = [dict(mean=wide, log_std=torch.zeros(9), actions=torch.zeros(48, 9)),            # A > 8
           dict(mean=t["mean"].double()), dict(log_std=t["log_std"].double()), dict(values=t["values"].double()),
           dict(actions=t["actions"].double()), dict(old_log_prob=t["old_log_prob"].half()), dict(advantages=t["advantages"].double()),
           dict(returns=t["returns"].double()), dict(index=index.int()), dict(index=index.float()),
           dict(actions=t["actions"].to("meta")), dict(advantages=t["advantages"].to("meta")), dict(index=index.to("meta")),
           dict(values=t["values"][:15]), dict(index=index[:15]), dict(old_log_prob=t["old_log_prob"][:47]), dict(index=None),
           dict(log_std=t["log_std"][:1]), dict(mean=t["mean"].numpy())]
    for change in bad:
        with pytest.raises(ValueError):
            head(**{**ok, **change})
    assert bk.calls == 1
    with pytest.raises(ValueError):
        head.log_prob(wide, torch.zeros(9), torch.zeros(16, 9))
    with pytest.raises(ValueError):
        head.log_prob(t["mean"], t["log_std"], t["actions"][:16].double())
    with pytest.raises(ValueError):
        head.log_prob(t["mean"], t["log_std"], t["actions"][:16], out=torch.zeros(15))


# ---- exports and documentation ----------------------------------------------------------------------------------------------------------
def test_new_names_are_exported_and_documented():
    import pde_control_gym
    from pdecontrolgym_amd import _native as N
    from pdecontrolgym_amd import backend, build
    for name in ("pdegym_ppo_loss", "pdegym_ppo_loss_workspace", "pdegym_diag_gaussian_log_prob"):
        assert name in N.EXPORTS, name
    assert "pdegym_ppo_loss.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "pdegym_ppo_loss.hip"))
    assert N.ABI_VERSION == 21 and N.PPO_LOSS_STATS == R.STATS == pde_control_gym.ppo_loss.STATS
    assert "PPOLoss" in pde_control_gym.__all__ and pde_control_gym.PPOLoss.__module__ == "pde_control_gym.ppo_loss"
    for fn in (backend.HipBackend.ppo_loss, backend.HipBackend.diag_gaussian_log_prob):
        assert hasattr(fn, "device_guard_key")
    header = open(os.path.join(ROOT, "include", "pdegym.h")).read()
    assert "#define PDEGYM_ABI_VERSION 21" in header
    assert "int pdegym_ppo_loss(const pdegym_ppo_loss_args* g, int32_t N, void* stream);" in header
    assert "int64_t pdegym_ppo_loss_workspace(int32_t N, int32_t A);" in header
    assert re.search(r"int pdegym_diag_gaussian_log_prob\(const float\* mean, int64_t ld, const float\* log_std,", header)
    # the ctypes mirror follows the header's structure field for field
    body = re.search(r"typedef struct pdegym_ppo_loss_args \{(.*?)\} pdegym_ppo_loss_args;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for d in filter(None, (x.strip() for x in body.split(";"))):
        d = re.sub(r"^(const\s+)?(int32_t|int64_t|uint8_t|float|double|void)\s*\*?", "", d).strip()
        names += [x.strip().lstrip("*") for x in d.split(",")]
    assert names == [f[0] for f in N.PpoLoss._fields_] and len(names) == 23
    import ctypes
    assert ctypes.sizeof(N.PpoLoss) == 8 + 8 * 21
    for text, where in ((open(os.path.join(ROOT, "README.md")).read(), "README.md"), (open(os.path.join(ROOT, "DESIGN.md")).read(), "DESIGN.md"),
                        (open(os.path.join(ROOT, "INTEGRATION.md")).read(), "INTEGRATION.md")):
        assert "PPOLoss" in text and "pdegym_ppo_loss" in text, where
    assert "### 4.15" in open(os.path.join(ROOT, "DESIGN.md")).read()


def test_the_ppo_example_has_the_switch_and_keeps_its_defaults():
    import inspect
    import importlib.util
    path = os.path.join(ROOT, "examples", "train_ppo_device.py")
    src = open(path).read()
    assert "PPOLoss" in src and "head.log_prob" in src and "result.backward()" in src
    spec = importlib.util.spec_from_file_location("train_ppo_device_for_test", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    sig = inspect.signature(mod.main)
    assert sig.parameters["fused_loss"].default is False and sig.parameters["fused_grad"].default is False
    assert [p for p in sig.parameters][:6] == ["iterations", "B", "T", "quiet", "hidden", "fused_grad"]


# ---- argument validation of the entry points, host half under ASan + UBSan -------------------------------------------------------------
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="needs hipcc")
def test_ppo_loss_entry_points_validate_their_arguments_under_asan_and_ubsan(tmp_path):
    """tests/c/ppo_loss_validation.c (its own main) against the host half of pdegym_ppo_loss.hip + pdegym_abi.hip, compiled with
    --cuda-host-only and the sanitizers and given an empty device image: every refusal answers with its code and a message, a
    well-formed descriptor fails only at the launch, and no call reaches a device."""
    from pdecontrolgym_amd import build
    hipcc = shutil.which("hipcc")
    inc = ["-I" + os.path.join(ROOT, "include"), "-I" + build.CSRC]
    objs = []
    for s in ("pdegym_abi.hip", "pdegym_ppo_loss.hip"):
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
    lib = str(tmp_path / "libpdegym_ppo_loss_asan.so")
    r = subprocess.run([hipcc, "-shared", "-fPIC"] + SAN + ["-o", lib] + objs + [stub_o], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()[-3000:]
    exe = str(tmp_path / "ppo_loss_validation")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    r = subprocess.run([hipcc, "-x", "c", "-std=c11", "-Wall", "-Werror", "-g"] + SAN
                       + [os.path.join(ROOT, "tests", "c", "ppo_loss_validation.c"), "-I" + os.path.join(ROOT, "include"),
                          "-L" + str(tmp_path), "-lpdegym_ppo_loss_asan", "-Wl,-rpath," + str(tmp_path),
                          "-Wl,-rpath," + os.path.join(rocm, "lib"), "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1", HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, env=env, timeout=120)
    out = r.stdout.decode()
    assert r.returncode == 0 and "PPO-LOSS-VALIDATION-OK" in out, out[-4000:]
    assert "runtime error" not in out and "AddressSanitizer" not in out, out[-4000:]
    assert int(out.strip().splitlines()[-2].split()[1]) >= 70, out[-1000:]
