"""CPU tests of the critic(obs, action) call form (include/pdegym.h: pdegym_mlp_forward_cat, pdegym_mlp_backward_cat,
pdegym_mlp_backward_wide_cat; ``FusedMLP.with_grad(obs, tail, params)``): a fake backend with the two-part methods
(tests/fake_mlp_cat_backend.py) drives the gradient routing of ``with_grad`` on CPU tensors against torch autograd on the concatenated
rows; the refusals; header and bindings in step; no kernel under a new name; and tests/c/mlp_cat_validation.c runs against the host
half of the library under AddressSanitizer and UBSan.  No kernel is launched; the kernels are pinned in tests/test_gpu_mlp_cat.py."""
import copy
import os
import re
import shutil
import subprocess

import pytest

from tests.fake_mlp_backward_wide_backend import FakeWideMlpBackend
from tests.fake_mlp_cat_backend import FakeCatMlpBackend

torch = pytest.importorskip("torch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _net(sizes, seed=0, act=torch.nn.Tanh):
    torch.manual_seed(seed)
    mods = []
    for i in range(len(sizes) - 1):
        mods.append(torch.nn.Linear(sizes[i], sizes[i + 1]))
        if i < len(sizes) - 2:
            mods.append(act())
    return torch.nn.Sequential(*mods)


def _policy(net, backend=None):
    from pdecontrolgym_amd.policy import FusedMLP
    return FusedMLP(net, backend=backend or FakeCatMlpBackend())


def _close(a, b):
    return torch.allclose(a.double(), b.double(), rtol=1e-5, atol=1e-6)


def _reference(net, obs, tail, obs_grad, tail_grad):
    """float64 copy of the module on torch.cat([obs, tail], 1) under autograd: y, d obs, d tail, parameter gradients of sum(y^2)."""
    twin = copy.deepcopy(net).double()
    o = obs.detach().double().requires_grad_(obs_grad)
    t = tail.detach().double().requires_grad_(tail_grad)
    y = twin(torch.cat([o, t], 1))
    (y ** 2).sum().backward()
    return y.detach(), o.grad, t.grad, [p.grad for p in twin.parameters()]


# ---- with_grad(obs, tail) against autograd, gradient routing -------------------------------------------------------------------------
@pytest.mark.parametrize("sizes,n2", [((9, 16, 2), 3), ((70, 64, 64, 1), 4), ((11, 65, 1), 1), ((66, 256, 256, 1), 8)],
                         ids=["9-16-2", "70-64-64-1", "11-65-1", "66-256-256-1"])
@pytest.mark.parametrize("route", ["tail", "obs", "both", "no_params", "frozen"])
def test_with_grad_on_two_part_rows_equals_autograd_on_the_concatenation(sizes, n2, route):
    net = _net(sizes, act=torch.nn.ReLU if sizes[1] > 64 else torch.nn.Tanh)
    backend = FakeCatMlpBackend()
    pol = _policy(net, backend)
    D, B = sizes[0] - n2, 19
    obs_grad, tail_grad = route in ("obs", "both", "no_params", "frozen"), route != "obs"
    if route == "frozen":
        for p in net.parameters():
            p.requires_grad_(False)
    obs = torch.randn(B, D).requires_grad_(obs_grad)
    tail = torch.randn(B, n2).requires_grad_(tail_grad)
    y = pol.with_grad(obs, tail, params=route != "no_params")
    want_y, want_do, want_dt, want_dp = _reference(net, obs, tail, obs_grad, tail_grad)
    assert y.shape == (B, sizes[-1]) and y.dtype == torch.float32 and y.grad_fn is not None and _close(y, want_y)
    assert backend.cat_forward_calls == 1 and backend.forward_calls == 0
    (y ** 2).sum().backward()
    assert len(backend.cat_calls) == 1 and not backend.backward_calls and not backend.wide_calls
    call = backend.cat_calls[0]
    assert call["n2"] == n2 and call["wide"] == (max(sizes[1:]) > 64) and call["dx"] == obs_grad and call["dx2"] == tail_grad
    if obs_grad:
        assert obs.grad.shape == (B, D) and _close(obs.grad, want_do)
    else:
        assert obs.grad is None
    if tail_grad:
        assert tail.grad.shape == (B, n2) and _close(tail.grad, want_dt)
    else:
        assert tail.grad is None
    if route in ("no_params", "frozen"):
        assert call["params"] is False and not call["dw"] and not call["db"]
        assert all(p.grad is None for p in net.parameters())
    else:
        assert call["params"] is True and call["dw"] and call["db"]
        for p, q in zip(net.parameters(), want_dp):
            assert p.grad is not None and _close(p.grad, q)


def test_params_false_makes_exactly_one_backward_call_with_null_dw_and_db():
    net = _net((12, 64, 64, 1))
    backend = FakeCatMlpBackend()
    pol = _policy(net, backend)
    obs, tail = torch.randn(33, 10), torch.randn(33, 2, requires_grad=True)
    (g,) = torch.autograd.grad(pol.with_grad(obs, tail, params=False).sum(), tail)
    assert backend.cat_calls == [{"params": False, "dw": False, "db": False, "dx": False, "dx2": True, "n2": 2, "wide": False, "B": 33}]
    assert not backend.backward_calls and not backend.wide_calls and g.shape == (33, 2)
    # without a tail: the same pass with n2 = 0 through the new entry point
    backend.cat_calls.clear()
    obs = torch.randn(33, 12, requires_grad=True)
    (g,) = torch.autograd.grad(pol.with_grad(obs, params=False).sum(), obs)
    assert backend.cat_calls == [{"params": False, "dw": False, "db": False, "dx": True, "dx2": False, "n2": 0, "wide": False, "B": 33}]
    ref = obs.detach().double().requires_grad_(True)
    (want,) = torch.autograd.grad(copy.deepcopy(net).double()(ref).sum(), ref)
    assert _close(g, want) and all(p.grad is None for p in net.parameters())


def test_params_false_with_nothing_to_differentiate_is_a_plain_forward():
    net = _net((12, 32, 1))
    backend = FakeCatMlpBackend()
    pol = _policy(net, backend)
    obs, tail = torch.randn(5, 9), torch.randn(5, 3)
    y = pol.with_grad(obs, tail, params=False)
    assert y.grad_fn is None and not y.requires_grad and not backend.cat_calls
    assert _close(y, copy.deepcopy(net).double()(torch.cat([obs, tail], 1).double()))
    assert _close(pol(obs, tail), y) and backend.cat_forward_calls == 2


def test_calls_without_the_new_arguments_take_the_old_entry_points():
    net = _net((12, 64, 1))
    backend = FakeCatMlpBackend()
    pol = _policy(net, backend)
    obs = torch.randn(7, 12, requires_grad=True)
    pol.with_grad(obs).sum().backward()
    assert backend.forward_calls == 1 and len(backend.backward_calls) == 1 and not backend.cat_calls and backend.cat_forward_calls == 0


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_what_is_wrong():
    net = _net((12, 64, 1))
    pol = _policy(net)
    obs = torch.randn(6, 9)
    for call in (lambda t: pol.with_grad(obs, t), lambda t: pol(obs, t), lambda t: pol.forward_into(obs, torch.empty(6, 1), tail=t)):
        with pytest.raises(ValueError, match=r"9 entries and tail rows 2, the network takes 12"):
            call(torch.randn(6, 2))
        with pytest.raises(ValueError, match="1..8 columns, got 0"):
            call(torch.randn(6, 0))
        with pytest.raises(ValueError, match="float32, got torch.float64"):
            call(torch.randn(6, 3, dtype=torch.float64))
        with pytest.raises(ValueError, match="tail is on meta"):
            call(torch.empty(6, 3, device="meta"))
        with pytest.raises(ValueError, match=r"\[B, n2\]"):
            call(torch.randn(5, 3))
    wide = _policy(_net((20, 64, 1)))
    with pytest.raises(ValueError, match="1..8 columns, got 9"):
        wide.with_grad(torch.randn(6, 11), torch.randn(6, 9))


def test_an_older_backend_refuses_the_new_arguments_and_keeps_the_old_calls():
    net = _net((12, 64, 1))
    old = FakeWideMlpBackend()
    pol = _policy(net, old)
    obs = torch.randn(6, 9)
    with pytest.raises(ValueError, match="needs a backend with mlp_forward_cat"):
        pol.with_grad(obs, torch.randn(6, 3))
    with pytest.raises(ValueError, match="needs a backend with mlp_forward_cat"):
        pol(obs, torch.randn(6, 3))
    with pytest.raises(ValueError, match="params=False needs a backend with mlp_backward_cat"):
        pol.with_grad(torch.randn(6, 12), params=False)
    for p in net.parameters():      # all frozen on the older backend: the old three-launch pass, as before
        p.requires_grad_(False)
    full = torch.randn(6, 12, requires_grad=True)
    pol.with_grad(full).sum().backward()
    assert len(old.backward_calls) == 1 and full.grad is not None


# ---- header, bindings, kernel names --------------------------------------------------------------------------------------------------------
def test_header_and_bindings_are_in_step():
    import ctypes
    from pdecontrolgym_amd import _native as N
    from pdecontrolgym_amd.backend import HipBackend
    header = open(os.path.join(ROOT, "include", "pdegym.h")).read()
    assert N.ABI_VERSION == 21 and re.search(r"#define PDEGYM_ABI_VERSION 21\b", header)
    for name in ("pdegym_mlp_forward_cat", "pdegym_mlp_backward_cat", "pdegym_mlp_backward_wide_cat"):
        assert name in N.EXPORTS and re.search(r"\bint %s\(" % name, header), name
    body = re.search(r"typedef struct pdegym_mlp_backward_cat_args \{(.*?)\} pdegym_mlp_backward_cat_args;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [re.sub(r"\[.*", "", d.strip().split()[-1].lstrip("*")) for d in body.split(";") if d.strip()]
    assert fields == [f[0] for f in N.MlpBackwardCat._fields_]
    # the first fields are pdegym_mlp_backward_args', at its offsets (params sits in its reserved word)
    for (name, _), (old, _) in zip(N.MlpBackwardCat._fields_, N.MlpBackward._fields_):
        assert getattr(N.MlpBackwardCat, name).offset == getattr(N.MlpBackward, old).offset
    assert ctypes.sizeof(N.MlpBackwardCat) == ctypes.sizeof(N.MlpBackward) + 40
    for method in ("mlp_forward_cat", "mlp_backward_cat"):
        assert getattr(HipBackend, method).device_guard_key == "x"


def test_the_feature_defines_no_kernel_under_a_new_name():
    from tests import test_lds_residue_helper as H
    from tests import test_gpu_lds_residue as G
    now = H.defined_kernels()
    assert now == set(G.LDS_CASES), now ^ set(G.LDS_CASES)
    src = {f: open(os.path.join(ROOT, "pdecontrolgym_amd", "csrc", f)).read()
           for f in ("pdegym_mlp.hip", "pdegym_mlp_backward.hip", "pdegym_mlp_backward_wide.hip")}
    # ... and the new entry points launch instantiations of the five kernels the registries already hold
    assert "mlp_forward_kernel<NT, WV, TX, TY, GAUSS, true>" in src["pdegym_mlp.hip"]
    assert "mlp_backward_tiles<float, true, false><<<" in src["pdegym_mlp_backward.hip"] and "mlp_backward_dw0<float, true><<<" in src["pdegym_mlp_backward.hip"]
    assert "launch(mlp_backward_wide_tiles<TX, CAT, PARAMS>" in src["pdegym_mlp_backward_wide.hip"]
    assert "launch(mlp_backward_wide_accumulate<TX, CAT>" in src["pdegym_mlp_backward_wide.hip"]


def test_the_thinned_gpu_product_is_covering_and_the_kernel_table_names_tests():
    """tests/mlp_cat_cases.py: every value of every parameter meets every kernel; tests/test_gpu_mlp_cat.py: the five kernels with new
    instantiations each name tests of that file; the exactly summable cases of that file are exact and leave no tile empty."""
    from tests import mlp_cat_cases as CC
    from tests import test_gpu_mlp_cat as G
    for family in ("narrow", "wide"):
        cs = CC.cases(family)
        CC.assert_covering(family, cs)
        assert len({c.name for c in cs}) == len(cs) == CC.N_CASES
        assert {k for k in G.KERNEL_CASES} >= set(CC.KERNELS[family])
    for k, tests in G.KERNEL_CASES.items():
        assert tests and all(t.startswith("test_") and callable(getattr(G, t, None)) for t in tests), (k, tests)
    for i, (family, case, n2) in enumerate(G.EXACT):
        assert 1 <= n2 <= 8 and G._built(i).want["dx"].shape == (case.B, case.sizes[0])


# ---- argument validation of the entry points, host half under ASan + UBSan ----------------------------------------------------------
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="needs hipcc")
def test_cat_entry_points_validate_their_arguments_under_asan_and_ubsan(tmp_path):
    """tests/c/mlp_cat_validation.c (its own main) against the host halves of pdegym_mlp.hip, pdegym_mlp_backward.hip,
    pdegym_mlp_backward_wide.hip + pdegym_abi.hip, compiled with --cuda-host-only and the sanitizers and given empty device images, as
    tests/test_mlp_backward_wide.py builds its program: every bad call answers with its code and a message, a well-formed call fails
    only at the launch, and no call reaches a device."""
    from pdecontrolgym_amd import build
    hipcc = shutil.which("hipcc")
    inc = ["-I" + os.path.join(ROOT, "include"), "-I" + build.CSRC]
    objs = []
    for s in ("pdegym_abi.hip", "pdegym_mlp.hip", "pdegym_mlp_backward.hip", "pdegym_mlp_backward_wide.hip"):
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
    lib = str(tmp_path / "libpdegym_mlp_cat_asan.so")
    r = subprocess.run([hipcc, "-shared", "-fPIC"] + SAN + ["-o", lib] + objs + [stub_o], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()[-3000:]
    exe = str(tmp_path / "mlp_cat_validation")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    r = subprocess.run([hipcc, "-x", "c", "-std=c11", "-Wall", "-Werror", "-g"] + SAN
                       + [os.path.join(ROOT, "tests", "c", "mlp_cat_validation.c"), "-I" + os.path.join(ROOT, "include"),
                          "-L" + str(tmp_path), "-lpdegym_mlp_cat_asan", "-Wl,-rpath," + str(tmp_path),
                          "-Wl,-rpath," + os.path.join(rocm, "lib"), "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1", HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, env=env, timeout=120)
    out = r.stdout.decode()
    assert r.returncode == 0 and "MLP-CAT-VALIDATION-OK" in out, out[-4000:]
    assert "runtime error" not in out and "AddressSanitizer" not in out, out[-4000:]
    assert int(out.strip().splitlines()[-2].split()[1]) >= 80, out[-1000:]
    for line in ("forward n2=0", "forward n2=9", "narrow params=0 with dw[1]", "wide dx2 = x2", "narrow launch (params=0, dx2 alone, no workspace)",
                 "wide launch (params=0, dx2 alone, no workspace)", "forward launch (squashed-Gaussian head)"):
        assert line in out and f"UNEXPECTED {line}" not in out, line
