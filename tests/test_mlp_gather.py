"""CPU tests of the rows-by-index call form (include/pdegym.h: pdegym_mlp_forward_gather, pdegym_mlp_backward_gather,
pdegym_mlp_backward_wide_gather; ``FusedMLP(..., index=, tail_indexed=)``): a fake backend with the gather methods
(tests/fake_mlp_gather_backend.py) drives ``forward_into``, ``__call__`` and ``with_grad`` on CPU tensors against the same calls on the
materialised rows; the refusals; header and bindings in step; no kernel under a new name; the thinned GPU product is covering; and
tests/c/mlp_gather_validation.c runs against the host half of the library under AddressSanitizer and UBSan.  No kernel is launched; the
kernels are pinned in tests/test_gpu_mlp_gather.py."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from tests.fake_mlp_cat_backend import FakeCatMlpBackend
from tests.fake_mlp_gather_backend import FakeGatherMlpBackend

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
    return FusedMLP(net, backend=backend or FakeGatherMlpBackend())


def _storage(M, D, n2, N, seed=1, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(M, D, generator=g).to(dtype), torch.randn(M, n2, generator=g), torch.randn(N, n2, generator=g),
            torch.randint(0, M, (N,), generator=g))


# ---- shapes and values: the call on the materialised rows ----------------------------------------------------------------------------
@pytest.mark.parametrize("sizes,n2", [((9, 16, 2), 0), ((9, 16, 2), 3), ((70, 64, 64, 1), 4), ((66, 256, 256, 1), 1)],
                         ids=["9-16-2", "9-16-2+3", "70-64-64-1+4", "66-256-256-1+1"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_forward_with_an_index_is_the_forward_on_the_gathered_rows(sizes, n2, dtype):
    net = _net(sizes)
    backend = FakeGatherMlpBackend()
    pol = _policy(net, backend)
    M, N, D = 23, 37, sizes[0] - n2
    store, stored_tail, tail, index = _storage(M, D, max(n2, 1), N, dtype=dtype)
    if not n2:
        got = pol(store, index=index)
        assert got.shape == (N, sizes[-1]) and got.dtype == dtype and torch.equal(got, pol(store[index]))
        out = torch.full((N, sizes[-1]), 7.0)
        assert pol.forward_into(store, out, index=index) is out and torch.equal(out, pol(store[index]).float())
        assert len(backend.gather_forward_calls) == 2 and all(c["x2"] is None for c in backend.gather_forward_calls)
        return
    dense, indexed = pol(store, tail, index=index), pol(store, stored_tail, index=index, tail_indexed=True)
    assert dense.shape == indexed.shape == (N, sizes[-1])
    assert torch.equal(dense, pol(store[index], tail)) and torch.equal(indexed, pol(store[index], stored_tail[index]))
    calls = backend.gather_forward_calls
    assert [c["x2_indexed"] for c in calls] == [False, True] and all(c["B"] == N and c["index"] is index for c in calls)
    # the storage itself arrives at the backend, not a copy of its rows
    assert all(c["x"].data_ptr() == store.data_ptr() and c["x"].shape[0] == M for c in calls)
    assert calls[1]["x2"].data_ptr() == stored_tail.data_ptr()


def test_a_trailing_observation_shape_is_flattened_per_storage_row():
    pol = _policy(_net((12, 16, 1)))
    store = torch.randn(10, 3, 4)
    index = torch.tensor([9, 0, 0, 4])
    assert torch.equal(pol(store, index=index), pol(store[index]))


# ---- with_grad: the autograd edges -----------------------------------------------------------------------------------------------------
ROUTES = [(sizes, n2, route) for sizes, n2 in (((9, 16, 2), 0), ((70, 64, 64, 1), 4), ((11, 65, 1), 1), ((66, 256, 256, 1), 8))
          for route in ("params", "tail", "both", "tail_indexed", "no_params") if n2 or route == "params"]      # (a route through the tail needs one)


@pytest.mark.parametrize("sizes,n2,route", ROUTES, ids=["-".join(map(str, s)) + f"+{n2}-{r}" for s, n2, r in ROUTES])
def test_with_grad_with_an_index_routes_the_gradients_of_the_materialised_call(sizes, n2, route):
    net = _net(sizes, act=torch.nn.ReLU if sizes[1] > 64 else torch.nn.Tanh)
    backend = FakeGatherMlpBackend()
    pol = _policy(net, backend)
    M, N, D = 29, 41, sizes[0] - n2
    store, stored_tail, tail, index = _storage(M, D, max(n2, 1), N)
    tail_grad = route in ("tail", "both", "no_params")
    if route == "tail":
        for p in net.parameters():
            p.requires_grad_(False)
    # the materialised call, on the two-part entry points of the same double
    t_ref = None if not n2 else (stored_tail[index] if route == "tail_indexed" else tail.clone().requires_grad_(tail_grad))
    y_ref = pol.with_grad(store[index], t_ref, params=route != "no_params")
    (y_ref ** 2).sum().backward()
    want = [None if p.grad is None else p.grad.clone() for p in net.parameters()]
    for p in net.parameters():
        p.grad = None
    t = None if not n2 else (stored_tail if route == "tail_indexed" else tail.clone().requires_grad_(tail_grad))
    y = pol.with_grad(store, t, params=route != "no_params", index=index, tail_indexed=route == "tail_indexed")
    assert y.shape == (N, sizes[-1]) and y.dtype == torch.float32 and y.grad_fn is not None and torch.equal(y, y_ref)
    assert len(backend.gather_forward_calls) == 1
    (y ** 2).sum().backward()
    assert len(backend.gather_calls) == 1 and not backend.cat_calls[1:]
    call = backend.gather_calls[0]
    assert call["B"] == N and call["wide"] == (max(sizes[1:]) > 64) and call["x2_indexed"] == (route == "tail_indexed")
    assert call["x"].data_ptr() == store.data_ptr() and call["index"] is index      # saved: the storage and the index, no rows
    assert call["dx2"] == tail_grad and call["params"] == (route in ("params", "both", "tail_indexed"))
    assert store.grad is None
    if tail_grad:
        assert t.grad.shape == (N, n2) and torch.equal(t.grad, t_ref.grad)
    for p, q in zip(net.parameters(), want):
        assert (p.grad is None) == (q is None) and (q is None or torch.equal(p.grad, q))
    assert any(q is not None for q in want) == (route in ("params", "both", "tail_indexed"))


def test_nothing_to_differentiate_with_an_index_is_a_plain_forward():
    net = _net((12, 32, 1))
    backend = FakeGatherMlpBackend()
    pol = _policy(net, backend)
    store, _, tail, index = _storage(9, 9, 3, 5)
    y = pol.with_grad(store, tail, params=False, index=index)
    assert y.grad_fn is None and not backend.gather_calls and torch.equal(y, pol(store[index], tail))


def test_calls_without_an_index_take_the_entry_points_they_took():
    net = _net((12, 64, 1))
    backend = FakeGatherMlpBackend()
    pol = _policy(net, backend)
    obs, tail = torch.randn(7, 9), torch.randn(7, 3, requires_grad=True)
    pol.with_grad(obs, tail).sum().backward()
    pol.with_grad(torch.randn(7, 12)).sum().backward()
    pol(obs, tail)
    assert not backend.gather_forward_calls and not backend.gather_calls
    assert backend.cat_forward_calls == 2 and backend.forward_calls == 1 and len(backend.cat_calls) == 1 and len(backend.backward_calls) == 1


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_what_is_wrong():
    net = _net((12, 64, 1))
    pol = _policy(net)
    store, stored_tail, tail, index = _storage(20, 9, 3, 6)
    calls = (lambda **kw: pol.with_grad(kw.pop("obs", store), kw.pop("tail", tail), **kw),
             lambda **kw: pol(kw.pop("obs", store), kw.pop("tail", tail), **kw),
             lambda **kw: pol.forward_into(kw.pop("obs", store), torch.empty(6, 1), tail=kw.pop("tail", tail), **kw))
    for call in calls:
        with pytest.raises(ValueError, match="contiguous int64"):
            call(index=index.to(torch.int32))
        with pytest.raises(ValueError, match="contiguous int64"):
            call(index=torch.arange(12)[::2])
        with pytest.raises(ValueError, match="contiguous int64"):
            call(index=index.reshape(6, 1))
        with pytest.raises(ValueError, match="index is on meta"):
            call(index=torch.empty(6, dtype=torch.int64, device="meta"))
        with pytest.raises(ValueError, match=r"tail must be a \[6, n2\]"):
            call(index=index, tail=stored_tail)                       # M rows without tail_indexed
        with pytest.raises(ValueError, match=r"tail must be a \[20, n2\]"):
            call(index=index, tail_indexed=True)                      # N rows with tail_indexed
        with pytest.raises(ValueError, match="tail_indexed=True needs index="):
            call(obs=store[:6], tail_indexed=True)
        with pytest.raises(ValueError, match="tail_indexed=True needs tail="):
            call(obs=torch.randn(20, 12), tail=None, index=index, tail_indexed=True)
        with pytest.raises(ValueError, match="9 entries and tail rows 2, the network takes 12"):
            call(index=index, tail=torch.randn(6, 2))
    with pytest.raises(ValueError, match="obs requires grad and is read by index"):
        pol.with_grad(store.clone().requires_grad_(True), tail, index=index)
    with pytest.raises(ValueError, match="tail requires grad and is read by index"):
        pol.with_grad(store, stored_tail.clone().requires_grad_(True), index=index, tail_indexed=True)
    with pytest.raises(ValueError, match="rows= and index= do not combine"):
        pol.forward_into(torch.randn(20, 12), torch.empty(6, 1), rows=torch.ones(6, dtype=torch.uint8), index=index)


def test_an_older_backend_refuses_an_index_and_keeps_the_old_calls():
    net = _net((12, 64, 1))
    old = FakeCatMlpBackend()
    pol = _policy(net, old)
    store, _, tail, index = _storage(20, 9, 3, 6)
    for call in (lambda: pol.with_grad(store, tail, index=index), lambda: pol(store, tail, index=index),
                 lambda: pol.forward_into(store, torch.empty(6, 1), tail=tail, index=index)):
        with pytest.raises(ValueError, match="index= needs a backend with mlp_forward_gather / mlp_backward_gather, FakeCatMlpBackend has none"):
            call()
    t = tail.clone().requires_grad_(True)
    pol.with_grad(store[index], t).sum().backward()
    assert len(old.cat_calls) == 1 and t.grad is not None


# ---- header, bindings, kernel names --------------------------------------------------------------------------------------------------------
NAMES = ("pdegym_mlp_forward_gather", "pdegym_mlp_backward_gather", "pdegym_mlp_backward_wide_gather")


def test_header_and_bindings_are_in_step():
    from pdecontrolgym_amd import _native as N
    from pdecontrolgym_amd.backend import HipBackend
    header = open(os.path.join(ROOT, "include", "pdegym.h")).read()
    assert N.ABI_VERSION == 21 and re.search(r"#define PDEGYM_ABI_VERSION 21\b", header)
    opening = header[: header.index("#ifndef PDEGYM_H")]
    for name in NAMES:
        assert name in N.EXPORTS and re.search(r"\bint %s\(" % name, header) and name in opening, name
    body = re.search(r"typedef struct pdegym_mlp_gather \{(.*?)\} pdegym_mlp_gather;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [d.strip().split()[-1].lstrip("*") for d in body.split(";") if d.strip()]
    assert fields == [f[0] for f in N.MlpGather._fields_] == ["index", "M", "x2_indexed", "reserved_"]
    assert ctypes.sizeof(N.MlpGather) == 24 and N.MlpGather.M.offset == 8 and N.MlpGather.x2_indexed.offset == 16
    # no existing structure changed its layout
    assert ctypes.sizeof(N.MlpBackwardCat) == ctypes.sizeof(N.MlpBackward) + 40
    for method in ("mlp_forward_gather", "mlp_backward_gather"):
        assert getattr(HipBackend, method).device_guard_key == "x"
    table = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert all(name in table for name in NAMES)


def test_the_library_exports_the_three_entry_points():
    from pdecontrolgym_amd import build
    if not os.path.exists(build.LIB):
        pytest.skip("the library is not built")
    lib = ctypes.CDLL(build.LIB)
    assert all(hasattr(lib, name) for name in NAMES)


def test_the_feature_defines_no_kernel_under_a_new_name():
    from tests import test_lds_residue_helper as H
    from tests import test_gpu_lds_residue as G
    now = H.defined_kernels()
    assert now == set(G.LDS_CASES), now ^ set(G.LDS_CASES)
    src = {f: open(os.path.join(ROOT, "pdecontrolgym_amd", "csrc", f)).read()
           for f in ("pdegym_mlp.hip", "pdegym_mlp_backward.hip", "pdegym_mlp_backward_wide.hip")}
    # the new entry points launch INDEXED instantiations of the five kernels the registries already hold ...
    assert "mlp_forward_kernel<NT, WV, TX, TY, GAUSS, true, false, true>" in src["pdegym_mlp.hip"]
    for text in ("mlp_backward_tiles<float, true, false, true><<<", "mlp_backward_tiles<float, true, true, true><<<",
                 "mlp_backward_tiles<double, true, true, true><<<", "mlp_backward_dw0<float, true, true><<<", "mlp_backward_dw0<double, true, true><<<"):
        assert text in src["pdegym_mlp_backward.hip"], text
    assert "launch(mlp_backward_wide_tiles<TX, CAT, PARAMS, true>" in src["pdegym_mlp_backward_wide.hip"]
    assert "launch(mlp_backward_wide_accumulate<TX, CAT, true>" in src["pdegym_mlp_backward_wide.hip"]
    # ... declared with a trailing, defaulted parameter, the indexed path compiled apart
    for f, n in (("pdegym_mlp.hip", 1), ("pdegym_mlp_backward.hip", 2), ("pdegym_mlp_backward_wide.hip", 2)):
        assert src[f].count("bool INDEXED = false>") == n and "if constexpr (INDEXED)" in src[f], f


def test_the_thinned_gpu_product_is_covering():
    """tests/mlp_gather_cases.py: every value of every parameter meets every kernel, inside the contract; the names are unique; the
    index patterns stay inside the storage and hold duplicates where they can."""
    from tests import mlp_gather_cases as GC
    from tests import test_gpu_mlp_gather as G
    for family in ("narrow", "wide"):
        cs = GC.cases(family)
        GC.assert_covering(family, cs)
        assert len({c.name for c in cs}) == len(cs) == GC.N_CASES
        assert set(G.KERNEL_CASES) >= set(GC.KERNELS[family])
        for c in cs:
            idx = GC.index_of(c.pattern, c.B, c.M, c.seed)
            assert idx.shape == (c.B,) and idx.dtype.name == "int64" and idx.min() >= 0 and idx.max() < c.M, c.name
    for k, tests in G.KERNEL_CASES.items():
        assert tests and all(t.startswith("test_") and callable(getattr(G, t, None)) for t in tests), (k, tests)
    for i in range(len(G.EXACT)):      # the expectations of the exactly summable cases are exact (asserted where they are built)
        assert len(set(G._exact(i)[3].tolist())) < G.EXACT[i][3]
    assert len(set(GC.index_of("random", 33, 7, 1).tolist())) < 33 and set(GC.index_of("last", 5, 7, 0).tolist()) == {6}
    assert GC.index_of("identity", 5, 3, 0).tolist() == [0, 1, 2, 2, 2] and GC.index_of("reversed", 5, 3, 0).tolist() == [2, 1, 0, 0, 0]


# ---- argument validation of the entry points, host half under ASan + UBSan ----------------------------------------------------------
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="needs hipcc")
def test_gather_entry_points_validate_their_arguments_under_asan_and_ubsan(tmp_path):
    """tests/c/mlp_gather_validation.c (its own main) against the host halves of pdegym_mlp.hip, pdegym_mlp_backward.hip,
    pdegym_mlp_backward_wide.hip + pdegym_abi.hip, compiled with --cuda-host-only and the sanitizers and given empty device images, as
    tests/test_mlp_cat.py builds its program: every bad call answers with its code and a message, a well-formed call fails only at the
    launch, and no call reaches a device."""
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
    lib = str(tmp_path / "libpdegym_mlp_gather_asan.so")
    r = subprocess.run([hipcc, "-shared", "-fPIC"] + SAN + ["-o", lib] + objs + [stub_o], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()[-3000:]
    exe = str(tmp_path / "mlp_gather_validation")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    r = subprocess.run([hipcc, "-x", "c", "-std=c11", "-Wall", "-Werror", "-g"] + SAN
                       + [os.path.join(ROOT, "tests", "c", "mlp_gather_validation.c"), "-I" + os.path.join(ROOT, "include"),
                          "-L" + str(tmp_path), "-lpdegym_mlp_gather_asan", "-Wl,-rpath," + str(tmp_path),
                          "-Wl,-rpath," + os.path.join(rocm, "lib"), "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1", HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, env=env, timeout=120)
    out = r.stdout.decode()
    assert r.returncode == 0 and "MLP-GATHER-VALIDATION-OK" in out, out[-4000:]
    assert "runtime error" not in out and "AddressSanitizer" not in out, out[-4000:]
    assert int(out.strip().splitlines()[-2].split()[1]) >= 100, out[-1000:]
    for line in ("forward NULL gather", "forward M=0", "forward x2_indexed with n2=0", "narrow dx given", "wide dx2 with x2_indexed",
                 "narrow dx2 on row B of x", "wide dw[2] on row M-1 of an indexed x2", "narrow dx2 = index",
                 "narrow launch (params=0, dx2 alone, no workspace)", "wide launch (params, x2 by index)",
                 "forward launch (squashed-Gaussian head)", "forward launch (n2=0: the plain row)"):
        assert line in out and f"UNEXPECTED {line}" not in out, line
