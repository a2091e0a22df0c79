"""``pde_control_gym.FusedAdam`` without a GPU: the NumPy restatement (tests/fused_adam_restatement.py) against ``clip_grad_norm_`` +
``torch.optim.Adam`` and SB3's ``polyak_update`` in float64, the optimiser's host logic on a CPU double of the backend
(tests/fake_fused_adam_backend.py) -- mirrors, version bookkeeping, refusals, state dictionaries --, exports and documentation, the
examples' switch, and the argument validation of the entry point as a stand-alone C program under ASan + UBSan."""
from __future__ import annotations

import copy
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import fused_adam_restatement as R
from tests.fake_fused_adam_backend import FakeFusedAdamBackend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(7, 5), (7,), (3, 7), (1,)]


def _bits(x):
    return x.detach().contiguous().view(torch.int32)


# ---- the restatement against torch in float64 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("eps", [1e-8, 1e-5])
@pytest.mark.parametrize("max_norm", [None, 0.5])
def test_float64_restatement_equals_clip_grad_norm_and_adam(max_norm, eps):
    rng = np.random.default_rng(1)
    params = [torch.nn.Parameter(torch.from_numpy(rng.standard_normal(s))) for s in SHAPES]
    opt = torch.optim.Adam(params, lr=3e-4, eps=eps)
    tensors = [{"p": p.detach().numpy().copy(), "m": np.zeros(s), "v": np.zeros(s)} for p, s in zip(params, SHAPES)]
    state = R.new_state()
    for it in range(10):
        grads = [rng.standard_normal(s) * (3.0 if it % 2 else 0.01) for s in SHAPES]      # norm above and below the bound
        for p, g, t in zip(params, grads, tensors):
            p.grad = torch.from_numpy(g.copy())
            t["g"] = g
        if max_norm is not None:
            total = torch.nn.utils.clip_grad_norm_(params, max_norm)
        opt.step()
        mine = R.step(tensors, state, 3e-4, 0.9, 0.999, eps, max_norm, dtype=np.float64)
        if max_norm is not None:
            assert abs(float(total) - float(mine)) <= 1e-12 * float(total)
        for p, t in zip(params, tensors):
            assert np.abs(p.detach().numpy() - t["p"]).max() <= 1e-12
            st = opt.state[p]
            assert np.abs(st["exp_avg"].numpy() - t["m"]).max() <= 1e-12 and np.abs(st["exp_avg_sq"].numpy() - t["v"]).max() <= 1e-12
    assert state[0] == 10.0 and abs(state[1] - 0.9 ** 10) < 1e-15 and abs(state[2] - 0.999 ** 10) < 1e-15


def test_float32_restatement_stays_as_close_to_float64_as_torch_float32():
    rng = np.random.default_rng(2)
    p0 = [rng.standard_normal(s).astype(np.float32) for s in SHAPES]
    params = [torch.nn.Parameter(torch.from_numpy(p.copy())) for p in p0]
    opt = torch.optim.Adam(params, lr=3e-4, eps=1e-5)
    t64 = [{"p": p.astype(np.float64), "m": np.zeros(p.shape), "v": np.zeros(p.shape)} for p in p0]
    t32 = [{"p": p.copy(), "m": np.zeros(p.shape, np.float32), "v": np.zeros(p.shape, np.float32)} for p in p0]
    s64, s32 = R.new_state(), R.new_state()
    for _ in range(10):
        grads = [rng.standard_normal(s).astype(np.float32) for s in SHAPES]
        for p, g, a, b in zip(params, grads, t64, t32):
            p.grad = torch.from_numpy(g.copy())
            a["g"], b["g"] = g.astype(np.float64), g
        torch.nn.utils.clip_grad_norm_(params, 0.5)
        opt.step()
        R.step(t64, s64, 3e-4, 0.9, 0.999, 1e-5, 0.5, dtype=np.float64)
        R.step(t32, s32, 3e-4, 0.9, 0.999, 1e-5, 0.5, dtype=np.float32)
    e_mine = max(np.abs(b["p"] - a["p"]).max() for a, b in zip(t64, t32))
    e_torch = max(np.abs(p.detach().numpy() - a["p"]).max() for p, a in zip(params, t64))
    assert all(b["p"].dtype == np.float32 and b["m"].dtype == np.float32 for b in t32)
    assert e_mine <= 4 * e_torch + 2.0 ** -20 and e_mine < 1e-5


def test_polyak_equals_sb3_polyak_update_in_float64():
    rng = np.random.default_rng(3)
    tau = 0.005
    tensors = [{"p": rng.standard_normal(s), "g": rng.standard_normal(s), "m": np.zeros(s), "v": np.zeros(s), "pt": rng.standard_normal(s)}
               for s in SHAPES]
    targets = [torch.from_numpy(t["pt"].copy()) for t in tensors]
    state = R.new_state()
    for _ in range(5):
        R.step(tensors, state, 1e-2, 0.9, 0.999, 1e-8, None, tau, polyak=True, dtype=np.float64)
        for t, tgt in zip(tensors, targets):      # stable_baselines3/common/utils.py: polyak_update
            tgt.mul_(1 - tau)
            torch.add(tgt, torch.from_numpy(t["p"]), alpha=tau, out=tgt)
            assert np.abs(tgt.numpy() - t["pt"]).max() <= 1e-12
    before = [t["pt"].copy() for t in tensors]
    R.step(tensors, state, 1e-2, 0.9, 0.999, 1e-8, None, tau, polyak=False, dtype=np.float64)
    assert all(np.array_equal(b, t["pt"]) for b, t in zip(before, tensors))


def test_blocked_layout_is_the_one_refresh_builds():
    from pde_control_gym import FusedMLP
    lin = torch.nn.Linear(6, 3)
    f = FusedMLP(lin, backend=FakeFusedAdamBackend())
    assert np.array_equal(f._wt[0].numpy(), R.blocked(lin.weight.detach().numpy()))


# ---- FusedAdam on the fake backend -----------------------------------------------------------------------------------------------------
def _net(sizes):
    torch.manual_seed(sum(sizes))
    mods = []
    for i in range(len(sizes) - 1):
        mods += [torch.nn.Linear(sizes[i], sizes[i + 1]), torch.nn.Tanh()]
    return torch.nn.Sequential(*mods[:-1])


def _fill_grads(params, seed):
    g = torch.Generator().manual_seed(seed)
    for p in params:
        p.grad = torch.randn(p.shape, generator=g)


def _fresh_copies(make):
    """The copies of a newly built wrapper around the same modules: what refresh(force=True) gives."""
    fresh = make()
    out = [w.clone() for w in fresh._wt]
    if fresh._heads is not None:
        out += [fresh._fused.weight.detach().clone()] + ([fresh._fused.bias.detach().clone()] if fresh._fused.bias is not None else [])
    return out


def _copies(f):
    out = list(f._wt)
    if f._heads is not None:
        out += [f._fused.weight.detach()] + ([f._fused.bias.detach()] if f._fused.bias is not None else [])
    return out


def _padding_is_zero(f):
    for wt, (w, _, _) in zip(f._wt, f.layers):
        in_dim = w.shape[1]
        flat = wt.permute(1, 0, 2).reshape(w.shape[0], -1)
        assert bool((flat[:, in_dim:] == 0).all())


@pytest.mark.parametrize("case", ["5-3-2", "66-65-1", "squashed"])
def test_attached_copies_equal_a_fresh_wrapper_after_every_step(case):
    from pde_control_gym import FusedAdam, FusedMLP
    be = FakeFusedAdamBackend()
    if case == "squashed":
        torch.manual_seed(5)
        latent = _net([5, 6, 6])
        latent = torch.nn.Sequential(*latent, torch.nn.Tanh())
        mu, ls = torch.nn.Linear(6, 2), torch.nn.Linear(6, 2)
        make = lambda: FusedMLP.squashed_gaussian(latent, mu, ls, backend=be)      # noqa: E731
        params = list(latent.parameters()) + list(mu.parameters()) + list(ls.parameters())
    else:
        net = _net([int(s) for s in case.split("-")])
        make = lambda: FusedMLP(net, backend=be)      # noqa: E731
        params = list(net.parameters())
    f = make()
    opt = FusedAdam(params, lr=1e-2, max_grad_norm=0.5, backend=be)
    assert opt.attach(f) is opt and f._optimizer is opt
    for it in range(3):
        before = [p.detach().clone() for p in params]
        versions = [p._version for p in params]
        _fill_grads(params, 10 + it)
        opt.step()
        assert all(not torch.equal(b, p.detach()) for b, p in zip(before, params))
        assert all(p._version > v for p, v in zip(params, versions))
        for mine, fresh in zip(_copies(f), _fresh_copies(make)):
            assert torch.equal(_bits(mine), _bits(fresh))
        _padding_is_zero(f)
    assert be.calls == 3 and float(opt.state[0]) == 3.0 and float(opt.total_norm) > 0.0


def test_refresh_after_step_copies_nothing_and_outside_changes_are_picked_up():
    from pde_control_gym import FusedAdam, FusedMLP
    be = FakeFusedAdamBackend()
    net = _net([5, 3, 2])
    f = FusedMLP(net, backend=be)
    params = list(net.parameters())
    opt = FusedAdam(params, backend=be).attach(f)
    _fill_grads(params, 1)
    opt.step()
    # a poisoned PADDING entry (the step never writes it, a refresh would zero it) survives step + refresh ..
    f._wt[0][1, 0, 3] = 123.0          # layer 0 has 5 inputs: block 1 holds input 4 and three padding entries
    _fill_grads(params, 2)
    opt.step()
    f.refresh()
    assert float(f._wt[0][1, 0, 3]) == 123.0
    # .. and so does a poisoned live entry between step and refresh (refresh finds nothing to do)
    f._wt[1][0, 0, 0] = 77.0
    f.refresh()
    assert float(f._wt[1][0, 0, 0]) == 77.0
    # a parameter changed behind the optimiser's back: the next refresh rebuilds that layer's copy, and only that one
    with torch.no_grad():
        net[0].weight.mul_(2.0)
    f.refresh()
    assert float(f._wt[0][1, 0, 3]) == 0.0 and float(f._wt[1][0, 0, 0]) == 77.0
    assert torch.equal(f._wt[0], FusedMLP(net, backend=be)._wt[0])
    net.load_state_dict(copy.deepcopy(net.state_dict()))
    f.refresh()
    assert float(f._wt[1][0, 0, 0]) != 77.0


def test_attach_refuses_a_partly_owned_network_and_a_second_mirror():
    from pde_control_gym import FusedAdam, FusedMLP
    be = FakeFusedAdamBackend()
    net = _net([5, 3, 2])
    f = FusedMLP(net, backend=be)
    part = FusedAdam(list(net[0].parameters()), backend=be)
    with pytest.raises(ValueError, match="do not belong"):
        part.attach(f)
    assert f._optimizer is None and all("wt" not in e for e in part._entries)
    whole = FusedAdam(list(net.parameters()), backend=be).attach(f)
    with pytest.raises(ValueError, match="already has a mirror"):
        whole.attach(FusedMLP(net, backend=be))
    with pytest.raises(ValueError):
        FusedAdam([torch.nn.Parameter(torch.zeros(1)) for _ in range(33)], backend=be)
    with pytest.raises(ValueError):
        FusedAdam([torch.nn.Parameter(torch.zeros(2, dtype=torch.float64))], backend=be)


def test_a_missing_gradient_raises_and_changes_nothing():
    from pde_control_gym import FusedAdam
    be = FakeFusedAdamBackend()
    params = [torch.nn.Parameter(torch.ones(3)), torch.nn.Parameter(torch.ones(2))]
    opt = FusedAdam(params, backend=be)
    params[0].grad = torch.ones(3)
    with pytest.raises(ValueError, match="no gradient"):
        opt.step()
    assert be.calls == 0 and float(opt.state[0]) == 0.0
    with pytest.raises(ValueError, match="attach_target"):
        opt.step(polyak=True)
    params[1].grad = torch.ones(2)
    opt.step()
    opt.zero_grad()
    assert all(p.grad is None for p in params)
    _fill_grads(params, 0)
    opt.zero_grad(set_to_none=False)
    assert all(p.grad is not None and not bool(p.grad.any()) for p in params)


def test_targets_follow_with_polyak_and_only_then():
    from pde_control_gym import FusedAdam, FusedMLP
    be = FakeFusedAdamBackend()
    net = _net([5, 3, 2])
    tgt = copy.deepcopy(net).requires_grad_(False)
    f, ft = FusedMLP(net, backend=be), FusedMLP(tgt, backend=be)
    params, tparams = list(net.parameters()), list(tgt.parameters())
    opt = FusedAdam(params, lr=1e-2, backend=be).attach(f).attach_target(params, tparams, 0.25, target_mlp=ft)
    with pytest.raises(ValueError, match="tau"):
        opt.attach_target(params, tparams, 0.5)
    _fill_grads(params, 3)
    before = [t.clone() for t in tparams]
    opt.step()
    assert all(torch.equal(b, t) for b, t in zip(before, tparams))
    _fill_grads(params, 4)
    opt.step(polyak=True)
    for b, t, p in zip(before, tparams, params):
        want = (np.float32(0.75) * b.numpy() + np.float32(0.25) * p.detach().numpy()).astype(np.float32)
        assert np.array_equal(t.numpy(), want)
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(ft._wt, FusedMLP(tgt, backend=be)._wt))
    ft._wt[0][0, 0, 0] = 55.0
    ft.refresh()
    assert float(ft._wt[0][0, 0, 0]) == 55.0 and be.polyak_calls == 1


def test_state_dict_round_trips_bit_for_bit_in_the_middle_of_a_run():
    from pde_control_gym import FusedAdam
    be = FakeFusedAdamBackend()

    def run(split):
        torch.manual_seed(0)
        params = [torch.nn.Parameter(torch.randn(s)) for s in SHAPES]
        opt = FusedAdam(params, lr=1e-2, eps=1e-5, max_grad_norm=0.5, backend=be)
        for it in range(6):
            if it == split:      # a new optimiser around the same parameters takes over
                sd = copy.deepcopy(opt.state_dict())
                opt = FusedAdam(params, lr=1e-2, eps=1e-5, max_grad_norm=0.5, backend=be)
                addresses = [m.data_ptr() for m in opt.exp_avg]
                opt.load_state_dict(sd)
                assert addresses == [m.data_ptr() for m in opt.exp_avg]
            _fill_grads(params, 20 + it)
            opt.step()
        return [p.detach().clone() for p in params] + opt.exp_avg + opt.exp_avg_sq + [opt.state]

    for a, b in zip(run(None), run(3)):
        assert torch.equal(a.view(torch.int32 if a.dtype == torch.float32 else torch.int64),
                           b.view(torch.int32 if b.dtype == torch.float32 else torch.int64))


def test_a_tensor_lr_is_read_at_every_step():
    from pde_control_gym import FusedAdam
    be = FakeFusedAdamBackend()
    p = torch.nn.Parameter(torch.ones(4))
    lr = torch.tensor(0.0)
    opt = FusedAdam([p], lr=lr, backend=be)
    p.grad = torch.ones(4)
    opt.step()
    assert torch.equal(p.detach(), torch.ones(4))
    lr.fill_(0.5)
    opt.step()
    assert not torch.equal(p.detach(), torch.ones(4))


# ---- exports and documentation ----------------------------------------------------------------------------------------------------------
def _field_names(header, name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for d in filter(None, (x.strip() for x in body.split(";"))):
        d = re.sub(r"^(const\s+)?(int32_t|int64_t|float|double|void|pdegym_fused_adam_tensor)\s*\*?", "", d).strip()
        names += [re.sub(r"\[.*\]", "", x).strip().lstrip("*") for x in d.split(",")]
    return names


def test_new_names_are_exported_and_documented():
    import ctypes
    import pde_control_gym
    from pdecontrolgym_amd import _native as N
    from pdecontrolgym_amd import backend, build
    assert {"pdegym_fused_adam", "pdegym_fused_adam_workspace"} <= set(N.EXPORTS)
    assert "pdegym_fused_adam.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "pdegym_fused_adam.hip"))
    assert N.ABI_VERSION == 21 and N.FUSED_ADAM_MAX_TENSORS == 32 == pde_control_gym.fused_adam.MAX_TENSORS
    assert "FusedAdam" in pde_control_gym.__all__ and pde_control_gym.FusedAdam.__module__ == "pde_control_gym.fused_adam"
    assert callable(backend.HipBackend.fused_adam) and callable(backend.HipBackend.fused_adam_workspace)
    doc = pde_control_gym.FusedAdam.__doc__
    assert "weight_decay" in doc and "amsgrad" in doc and "32" in doc
    header = open(os.path.join(ROOT, "include", "pdegym.h")).read()
    assert "#define PDEGYM_ABI_VERSION 21" in header and "#define PDEGYM_FUSED_ADAM_MAX_TENSORS 32" in header
    assert "int pdegym_fused_adam(const pdegym_fused_adam_args* a, void* stream);" in header
    assert "int64_t pdegym_fused_adam_workspace(const int64_t* n, int32_t K);" in header
    for line in ("total  = (float) sqrt(sum_double(g^2))", "coef   = min(max_grad_norm / (total + 1e-6f), 1.0f)", "g'     = g * coef",
                 "m      = m + (float)(1 - beta1) * (g' - m)", "v      = (float)beta2 * v + (float)(1 - beta2) * (g' * g')",
                 "p      = p - (float)(lr / (1 - beta1^t)) * (m / (sqrt(v) / (float)sqrt(1 - beta2^t) + (float)eps))",
                 "pt     = (float)(1 - tau) * pt + (float)tau * p", "g itself is NOT modified",
                 "wt[(i / 4) * wt_out_total * 4 + (wt_row0 + o) * 4 + i % 4]"):
        assert line in header, line
    want = {"pdegym_fused_adam_tensor": (N.FusedAdamTensor, 104), "pdegym_fused_adam_args": (N.FusedAdam, 96 + 32 * 104)}
    for struct, (mirror, size) in want.items():
        assert _field_names(header, struct) == [f[0].rstrip("_") for f in mirror._fields_], struct
        assert ctypes.sizeof(mirror) == size, struct
    for where in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        text = open(os.path.join(ROOT, where)).read()
        assert "FusedAdam" in text and "pdegym_fused_adam" in text, where
    assert "### 4.18" in open(os.path.join(ROOT, "DESIGN.md")).read()
    src = open(os.path.join(build.CSRC, "pdegym_fused_adam.hip")).read()
    code = re.sub(r"//[^\n]*", "", src)
    assert "atomic" not in code and "__threadfence" not in code and "<<<" not in code and len(re.findall(r"\blaunch\(", code)) == 3      # one definition, two launches
    assert "hipLaunchKernel" in code and "pow(" not in code


def test_the_size_query_follows_the_stated_decomposition():
    import ctypes as C
    from pdecontrolgym_amd import _native as N
    lib = N.load()
    for sizes in ([1], [3, 64, 65], [255 * 5], [256 * 256, 256, 256, 1], [1] * 32, [1024, 1025, 10 ** 9]):
        arr = (C.c_int64 * len(sizes))(*sizes)
        assert lib.pdegym_fused_adam_workspace(arr, len(sizes)) == FakeFusedAdamBackend().fused_adam_workspace(sizes), sizes
    assert lib.pdegym_fused_adam_workspace((C.c_int64 * 1)(0), 1) == -2 and b"n must be" in lib.pdegym_last_error()
    assert lib.pdegym_fused_adam_workspace((C.c_int64 * 33)(*([1] * 33)), 33) == -2


@pytest.mark.parametrize("name,leading", [("train_ppo_device.py", ["iterations", "B", "T", "quiet", "hidden", "fused_grad", "fused_loss"]),
                                          ("train_sac_device.py", ["iterations", "num_envs", "n_steps", "hidden", "one_launch", "quiet", "updates",
                                                                   "batch", "fused_grad", "fused_loss"])])
def test_the_examples_have_the_switch_and_keep_their_defaults(name, leading):
    import importlib.util
    import inspect
    import sys
    path = os.path.join(ROOT, "examples", name)
    src = open(path).read()
    assert "FusedAdam" in src and "fused_opt" in src and ".attach(" in src
    if "sac" in name:
        assert "attach_target" in src and "step(polyak=True)" in src
    sys.path.insert(0, os.path.dirname(path))
    try:
        spec = importlib.util.spec_from_file_location(name[:-3] + "_for_fused_adam_test", path)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        sys.path.remove(os.path.dirname(path))
    sig = inspect.signature(mod.main)
    assert sig.parameters["fused_opt"].default is False
    assert list(sig.parameters)[:len(leading)] == leading and list(sig.parameters)[len(leading)] == "fused_opt"
    assert "[fused_opt: 0]" in mod.__doc__
    if "ppo" in name:
        assert sig.parameters["graph_update"].default is False and "[graph_update: 0]" in mod.__doc__


# ---- argument validation of the entry point, host half under ASan + UBSan ---------------------------------------------------------------
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="needs hipcc")
def test_fused_adam_entry_point_validates_its_arguments_under_asan_and_ubsan(tmp_path):
    """tests/c/fused_adam_validation.c (its own main) against the host half of pdegym_fused_adam.hip + pdegym_abi.hip, compiled with
    --cuda-host-only and the sanitizers and given an empty device image: every refusal answers with its code and a message, a
    well-formed descriptor fails only at the launch, and no call reaches a device."""
    from pdecontrolgym_amd import build
    hipcc = shutil.which("hipcc")
    inc = ["-I" + os.path.join(ROOT, "include"), "-I" + build.CSRC]
    objs = []
    for s in ("pdegym_abi.hip", "pdegym_fused_adam.hip"):
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
    lib = str(tmp_path / "libpdegym_fused_adam_asan.so")
    r = subprocess.run([hipcc, "-shared", "-fPIC"] + SAN + ["-o", lib] + objs + [stub_o], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()[-3000:]
    exe = str(tmp_path / "fused_adam_validation")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    r = subprocess.run([hipcc, "-x", "c", "-std=c11", "-Wall", "-Werror", "-g"] + SAN
                       + [os.path.join(ROOT, "tests", "c", "fused_adam_validation.c"), "-I" + os.path.join(ROOT, "include"),
                          "-L" + str(tmp_path), "-lpdegym_fused_adam_asan", "-Wl,-rpath," + str(tmp_path),
                          "-Wl,-rpath," + os.path.join(rocm, "lib"), "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1", HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, env=env, timeout=120)
    out = r.stdout.decode()
    assert r.returncode == 0 and "FUSED-ADAM-VALIDATION-OK" in out, out[-4000:]
    assert "runtime error" not in out and "AddressSanitizer" not in out, out[-4000:]
