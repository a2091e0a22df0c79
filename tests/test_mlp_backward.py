"""CPU tests of the differentiable FusedMLP (include/pdegym.h: pdegym_mlp_backward; FusedMLP.with_grad): a fake backend built on the
float64 restatement (tests/mlp_backward_exact.py) drives the autograd plumbing on CPU tensors, the ctypes mirror follows the header,
the new names are documented, and tests/c/mlp_backward_validation.c runs against the host half of the library under AddressSanitizer
and UBSan.  No kernel is launched; the kernels are pinned in tests/test_gpu_mlp_backward.py."""
import copy
import os
import re
import shutil
import subprocess

import pytest

from tests.fake_mlp_backward_backend import FakeMlpBackend

torch = pytest.importorskip("torch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tanh_net(sizes=(7, 9, 5, 2), seed=0, bias=True):
    torch.manual_seed(seed)
    mods = []
    for i in range(len(sizes) - 1):
        mods.append(torch.nn.Linear(sizes[i], sizes[i + 1], bias=bias))
        if i < len(sizes) - 2:
            mods.append(torch.nn.Tanh())
    return torch.nn.Sequential(*mods)


def _policy(net, **kw):
    from pdecontrolgym_amd.policy import FusedMLP
    return FusedMLP(net, backend=FakeMlpBackend(), **kw)


def _close(a, b):
    return torch.allclose(a, b, rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("bias", [True, False], ids=["bias", "no_bias"])
def test_gradients_land_in_the_modules_parameters_and_equal_autograd(bias):
    net = _tanh_net(bias=bias)
    twin = copy.deepcopy(net)
    pol = _policy(net)
    obs = torch.randn(21, 7)
    y = pol.with_grad(obs)
    assert y.shape == (21, 2) and y.dtype == torch.float32 and y.grad_fn is not None and _close(y, twin(obs))
    (y ** 2).sum().backward()
    (twin(obs) ** 2).sum().backward()
    for p, q in zip(net.parameters(), twin.parameters()):
        assert p.grad is not None and p.grad.shape == p.shape and _close(p.grad, q.grad)
    assert pol.backend.backward_calls == [{"dx": False, "B": 21, "slabs": 0}]
    assert [p is q for p, q in zip(pol.grad_parameters(), net.parameters())] == [True] * len(list(net.parameters()))


def test_two_backward_calls_accumulate_and_the_launch_itself_writes():
    net = _tanh_net()
    pol = _policy(net)
    obs = torch.randn(5, 7)
    pol.with_grad(obs).sum().backward()
    once = [p.grad.clone() for p in net.parameters()]
    pol.with_grad(obs).sum().backward()
    for p, g in zip(net.parameters(), once):
        assert torch.equal(p.grad, g + g)
    assert len(pol.backend.backward_calls) == 2


def test_dx_is_requested_only_for_float32_observations_that_require_grad():
    net = _tanh_net()
    twin = copy.deepcopy(net)
    pol = _policy(net)
    obs = torch.randn(6, 7, requires_grad=True)
    pol.with_grad(obs).sum().backward()
    ref = obs.detach().clone().requires_grad_(True)
    twin(ref).sum().backward()
    assert pol.backend.backward_calls[-1]["dx"] is True and _close(obs.grad, ref.grad)
    pol.with_grad(obs.detach()).sum().backward()
    assert pol.backend.backward_calls[-1]["dx"] is False
    pol.with_grad(obs.detach().double()).sum().backward()          # float64 rows are rounded as they are read: no dx
    assert pol.backend.backward_calls[-1]["dx"] is False
    # a frozen parameter gets no gradient
    net[0].weight.requires_grad_(False)
    net.zero_grad(set_to_none=True)
    pol.with_grad(obs.detach()).sum().backward()
    assert net[0].weight.grad is None and net[0].bias.grad is not None
    # trailing observation shapes flatten, a wrong width is refused
    assert pol.with_grad(torch.randn(3, 7, 1)).shape == (3, 2)
    with pytest.raises(ValueError, match="entries"):
        pol.with_grad(torch.randn(3, 8))


def test_the_gaussian_wrapper_returns_the_raw_rows_and_routes_to_both_heads():
    from pdecontrolgym_amd.policy import FusedMLP
    torch.manual_seed(1)
    latent = [torch.nn.Linear(7, 9), torch.nn.ReLU()]
    mu, log_std = torch.nn.Linear(9, 3), torch.nn.Linear(9, 3)
    twin = copy.deepcopy([torch.nn.Sequential(*latent), mu, log_std])
    pol = FusedMLP.squashed_gaussian(latent, mu, log_std, backend=FakeMlpBackend())
    obs = torch.randn(11, 7)
    raw = pol.with_grad(obs)
    lat = twin[0](obs)
    want = torch.cat([twin[1](lat), twin[2](lat)], dim=1)
    assert raw.shape == (11, 6) and _close(raw, want)

    def sac_loss(r):      # what SAC does with the two halves: clip, exp, tanh
        m, s = r[:, :3], r[:, 3:].clamp(-20, 2).exp()
        return (torch.tanh(m + 0.3 * s) ** 2).sum() + s.sum()
    sac_loss(raw).backward()
    sac_loss(want).backward()
    mine = [latent[0].weight, latent[0].bias, mu.weight, mu.bias, log_std.weight, log_std.bias]
    theirs = [twin[0][0].weight, twin[0][0].bias, twin[1].weight, twin[1].bias, twin[2].weight, twin[2].bias]
    for p, q in zip(mine, theirs):
        assert p.grad is not None and _close(p.grad, q.grad)
    assert not torch.equal(mu.weight.grad, log_std.weight.grad)
    assert [p is q for p, q in zip(pol.grad_parameters(), mine)] == [True] * 6


def test_an_optimiser_step_is_seen_by_the_next_with_grad():
    net = _tanh_net()
    pol = _policy(net)
    obs = torch.randn(9, 7)
    opt = torch.optim.SGD(net.parameters(), lr=0.5)
    before = pol.with_grad(obs)
    (before ** 2).sum().backward()
    opt.step()
    after = pol.with_grad(obs)
    assert not torch.equal(after, before) and _close(after, net(obs))
    # a backward AFTER the parameters moved is refused by autograd (the saved parameters changed in place), not computed on new weights
    stale = pol.with_grad(obs)
    opt.step()
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        stale.sum().backward()


def test_each_limit_raises_and_the_inference_call_keeps_no_graph():
    wide = _policy(_tanh_net((7, 65, 2)))
    assert not wide.fits_backward() and "65 units" in wide.backward_limit()
    with pytest.raises(ValueError, match="at most 64"):
        wide.with_grad(torch.randn(3, 7))
    long_rows = _policy(_tanh_net((1025, 8, 2)))
    assert not long_rows.fits_backward()
    with pytest.raises(ValueError, match="at most 1024"):
        long_rows.with_grad(torch.randn(3, 1025))
    ok = _policy(_tanh_net((1024, 64, 64, 64)))
    assert ok.fits_backward() and ok.backward_limit() is None
    with pytest.raises(ValueError, match="float32 or float64"):
        ok.with_grad(torch.zeros(3, 1024, dtype=torch.float16))
    pol = _policy(_tanh_net())
    out = pol(torch.randn(4, 7))
    assert torch.is_tensor(out) and out.grad_fn is None and not out.requires_grad
    assert pol.backend.backward_calls == []


def test_new_names_are_exported_and_documented():
    import pde_control_gym
    from pdecontrolgym_amd import _native as N
    from pdecontrolgym_amd import backend, build
    assert {"pdegym_mlp_backward", "pdegym_mlp_backward_workspace"} <= set(N.EXPORTS) and "pdegym_mlp_backward.hip" in build.SOURCES
    assert N.ABI_VERSION == 21 and os.path.exists(os.path.join(build.CSRC, "pdegym_mlp_backward.hip"))
    assert hasattr(backend.HipBackend.mlp_backward, "device_guard_key")
    assert hasattr(pde_control_gym.FusedMLP, "with_grad") and hasattr(pde_control_gym.FusedMLP, "fits_backward")
    assert (N.MLP_BACKWARD_MAX_WIDTH, N.MLP_BACKWARD_MAX_INPUT) == (64, 1024)
    header = open(os.path.join(ROOT, "include", "pdegym.h")).read()
    assert "#define PDEGYM_ABI_VERSION 21" in header
    doc = header[header.index("backward pass of the same network"):header.index("int pdegym_mlp_backward(")]
    for word in ("Determinism", "slabs", "threshold_backward", "v_mfma_f32_16x16x4_f32", "1024", "WRITTEN, not accumulated"):
        assert word in doc, word
    # the ctypes mirror follows the header's structure field for field
    body = re.search(r"typedef struct pdegym_mlp_backward_args \{(.*?)\} pdegym_mlp_backward_args;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names, arrays = [], []
    for d in filter(None, (x.strip() for x in body.split(";"))):
        d = re.sub(r"^(const\s+)?(int32_t|int64_t|float|void)\s*\*?", "", d).strip()
        arrays += [d.split("[")[0].strip()] if "[" in d else []
        names += [x.strip().lstrip("*").split("[")[0] for x in d.split(",")]
    assert names == [f[0] for f in N.MlpBackward._fields_] and len(names) == 13 and arrays == ["w", "dw", "db"]
    import ctypes
    assert ctypes.sizeof(N.MlpBackward) == 8 * (4 + 3 * N.MLP_MAX_LAYERS + 2 + 1 + 2) and N.MlpBackward.workspace.offset == 8 * (4 + 12 + 3)
    assert "Inference only (no autograd graph)" not in pde_control_gym.FusedMLP.__doc__ and "with_grad" in pde_control_gym.FusedMLP.__doc__
    for name in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        text = open(os.path.join(ROOT, name)).read()
        assert "with_grad" in text and "pdegym_mlp_backward" in text, name
    assert "4.13" in open(os.path.join(ROOT, "DESIGN.md")).read()


def test_the_examples_have_the_switch():
    for name in ("train_ppo_device.py", "train_sac_device.py"):
        src = open(os.path.join(ROOT, "examples", name)).read()
        assert "fused_grad=False" in src and ".with_grad" in src and "sys.argv[4]" in src, name


def test_every_backward_kernel_has_an_output_contract_test():
    """The kernels of csrc/pdegym_mlp_backward.hip keep their poisoned-buffer tests in tests/test_gpu_mlp_backward.py: every kernel
    launched there (chevron syntax) is listed in its KERNEL_CASES, and every test named exists."""
    from tests import test_gpu_mlp_backward as G
    src = open(os.path.join(ROOT, "pdecontrolgym_amd", "csrc", "pdegym_mlp_backward.hip")).read()
    launched = set(re.findall(r"([A-Za-z_]\w*)\s*(?:<[^<>;]*>)?\s*<<<", src))
    assert "hipLaunchKernelGGL" not in src
    assert launched == set(G.KERNEL_CASES) and len(launched) == 3, launched ^ set(G.KERNEL_CASES)
    for k, tests in G.KERNEL_CASES.items():
        assert tests and all(callable(getattr(G, t, None)) for t in tests), (k, tests)


def test_the_backward_units_share_one_header():
    """csrc/pdegym_mlp_backward_common.h holds what pdegym_mlp_backward.hip and pdegym_mlp_backward_wide.hip have in common, each piece
    once (the kernels' mma / act_backward / slab_begin / slab_sum; Range, extent, the overlap scan, the descriptor and argument checks,
    the slab and workspace arithmetic, the plan fill), and pdegym_mlp_tile.h how an index entry becomes a row: neither unit defines
    one of these or scans for overlaps itself, and all three entry points of a unit go through the one argument check."""
    from pdecontrolgym_amd import build
    code = lambda f: re.sub(r"//[^\n]*", "", open(os.path.join(build.CSRC, f)).read())      # noqa: E731
    hdr, tile = code("pdegym_mlp_backward_common.h"), code("pdegym_mlp_tile.h")
    shared = ("mma", "slab_begin", "act_backward", "slab_sum", "failf", "extent", "check_overlap", "check_net", "tiles_of", "resolve_slabs",
              "per_slab_floats", "workspace_bytes", "workspace_query", "check_call", "fill_plan", "gather_plan")
    defined = lambda name, src: re.findall(r"^(?:template <[^\n]*>\n)?(?:__device__ __forceinline__ |inline )?[\w:]+\s+" + name + r"\(", src, re.M)      # noqa: E731
    for name in shared:
        assert len(defined(name, hdr)) == 1, name
    for struct in ("Range", "Entry", "Call", "TwoPart"):
        assert len(re.findall(r"^struct %s \{" % struct, hdr, re.M)) == 1, struct
    assert len(defined("indexed_row", tile)) == 1 and not defined("indexed_row", hdr)
    assert "__global__" not in hdr and "<<<" not in hdr and "hipLaunchKernel" not in hdr      # every kernel and launch stays in its unit
    # not a translation unit; the library's fingerprint hashes every file of csrc/, so it sees the header as it sees pdegym_mlp_tile.h
    import inspect
    assert "pdegym_mlp_backward_common.h" not in build.SOURCES and "os.listdir(CSRC)" in inspect.getsource(build._fingerprint)
    for unit, run, entries in (("pdegym_mlp_backward.hip", "backward_rows", ("pdegym_mlp_backward", "pdegym_mlp_backward_cat", "pdegym_mlp_backward_gather")),
                               ("pdegym_mlp_backward_wide.hip", "backward_wide_rows",
                                ("pdegym_mlp_backward_wide", "pdegym_mlp_backward_wide_cat", "pdegym_mlp_backward_wide_gather"))):
        src = code(unit)
        assert '#include "pdegym_mlp_backward_common.h"' in src and "using namespace pdegym_mlp_backward_common;" in src, unit
        assert not [n for n in shared + ("indexed_row",) if defined(n, src)], (unit, [n for n in shared if defined(n, src)])
        assert "struct Range" not in src and ".overlaps(" not in src and "extent(" not in src, unit
        assert "unsigned long long)P.M" not in src and "P.index[" not in src, unit      # (the index entry: indexed_row alone reads it)
        # one call of the shared check, in the function every entry point of the unit returns through
        assert len(re.findall(r"(?<!\w)check_call\(", src)) == 1 and len(re.findall(r"(?<!\w)check_net\(", src)) == 0, unit
        body = re.search(r"^int " + run + r"\(.*?^\}", src, re.S | re.M).group(0)
        assert "check_call(kEntry, net, a, g, two_part, B, c)" in body, unit
        for name in entries:
            entry = re.search(r"^int " + name + r"\(.*?^\}", src, re.S | re.M).group(0)
            assert len(re.findall(r"return " + run + r"\(net, ", entry)) == 1, (unit, name)
    fwd = code("pdegym_mlp.hip")
    assert "indexed_row(" in fwd and "unsigned long long)gth.M" not in fwd


# ---- argument validation of the entry points, host half under ASan + UBSan ----------------------------------------------------------
SAN =["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="needs hipcc")
def test_mlp_backward_entry_points_validate_their_arguments_under_asan_and_ubsan(tmp_path):
    """tests/c/mlp_backward_validation.c (its own main) against the host half of pdegym_mlp_backward.hip + pdegym_abi.hip, compiled
    with --cuda-host-only and the sanitizers and given an empty device image, exactly as tests/test_gae.py builds gae_validation.c:
    every bad call must answer with a negative code and a message, a well-formed call fails only at the launch, and no call reaches
    a device."""
    from pdecontrolgym_amd import build
    hipcc = shutil.which("hipcc")
    inc = ["-I" + os.path.join(ROOT, "include"), "-I" + build.CSRC]
    objs = []
    for s in ("pdegym_abi.hip", "pdegym_mlp_backward.hip"):
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
    lib = str(tmp_path / "libpdegym_mlp_backward_asan.so")
    r = subprocess.run([hipcc, "-shared", "-fPIC"] + SAN + ["-o", lib] + objs + [stub_o], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()[-3000:]
    exe = str(tmp_path / "mlp_backward_validation")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    r = subprocess.run([hipcc, "-x", "c", "-std=c11", "-Wall", "-Werror", "-g"] + SAN
                       + [os.path.join(ROOT, "tests", "c", "mlp_backward_validation.c"), "-I" + os.path.join(ROOT, "include"),
                          "-L" + str(tmp_path), "-lpdegym_mlp_backward_asan", "-Wl,-rpath," + str(tmp_path),
                          "-Wl,-rpath," + os.path.join(rocm, "lib"), "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1", HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, env=env, timeout=120)
    out = r.stdout.decode()
    assert r.returncode == 0 and "MLP-BACKWARD-VALIDATION-OK" in out, out[-4000:]
    assert "runtime error" not in out and "AddressSanitizer" not in out, out[-4000:]
    assert int(out.strip().splitlines()[-2].split()[1]) >= 60, out[-1000:]
