"""The LDS-residue helper (tests/lds_residue.py) and the registry of tests/test_gpu_lds_residue.py, checked without a GPU."""
import ctypes as C
import glob
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import lds_residue as LR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pdecontrolgym_amd", "csrc")

# a kernel DEFINITION: __global__ [__launch_bounds__(...)] void name( -- whatever the launch syntax of its call sites
GLOBAL_DEF = re.compile(r"__global__\b[^;{]*?\bvoid\s+(\w+)\s*\(", re.S)


def defined_kernels():
    names = set()
    for path in sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h"))):
        with open(path) as f:
            names.update(GLOBAL_DEF.findall(f.read()))
    return names


# ---- the registry ------------------------------------------------------------------------------------------------------------
def test_every_defined_kernel_is_in_the_lds_suite():
    """LDS_CASES holds exactly the ``__global__`` definitions of csrc/*.hip and csrc/*.h -- kernels without LDS included: they pass
    trivially today and are covered the day they gain some -- and every test it names exists."""
    from tests import test_gpu_lds_residue as T
    defined = defined_kernels()
    assert len(defined) >= 55, sorted(defined)
    missing = sorted(defined - set(T.LDS_CASES))
    assert not missing, f"kernels without a case in test_gpu_lds_residue.LDS_CASES: {missing}"
    stale = sorted(set(T.LDS_CASES) - defined)
    assert not stale, f"LDS_CASES names kernels that csrc/ does not define: {stale}"
    for k, tests in T.LDS_CASES.items():
        assert tests and all(t.startswith("test_") and callable(getattr(T, t, None)) for t in tests), (k, tests)


def test_the_definition_regex_sees_every_form():
    src = """
    template <int EPL, bool X>
    __global__ __launch_bounds__(kWave* kWavesPerBlock) void a_kernel(P p, int B) { }
    template <class T, int NY>
    __global__ __launch_bounds__(64, (sizeof(T) == 8 || NY > 21 ? 2 : 3)) void b_kernel(NSConst C,
                                                                                     int B) { }
    __global__ void c_kernel(Args A) { }
    __global__ __launch_bounds__(kNT, 2)
    void d_kernel() { }
    __device__ void not_a_kernel(int x) { }
    """
    assert GLOBAL_DEF.findall(src) == ["a_kernel", "b_kernel", "c_kernel", "d_kernel"]


def test_the_added_cases_keep_the_exactness_bound():
    """Every exactly summable case the GPU module adds builds on the CPU (``build`` asserts that float32 arithmetic is exact for it)
    and has an expectation that is finite and, with more than one row, not constant."""
    from tests import gaussian_exact as gx
    from tests import mlp_backward_exact as R
    from tests import mlp_exact as mx
    from tests import test_gpu_lds_residue as T
    names = set()
    for case in T.POLICY_ROLLOUT_CASES + [c for w in T.MLP_WIDTHS for c in T.forward_cases(w)]:
        b = mx.build(case)
        assert np.isfinite(b.want).all() and b.want.shape == (case.B, case.sizes[-1]), case.name
        names.add(case.name)
    for case in T.GAUSSIAN_ROLLOUT_CASES:
        b = gx.build(case)
        assert np.isfinite(b.want).all(), case.name
        names.add(case.name)
    for w in T.MLP_WIDTHS:
        for case in T.backward_cases(w):
            b = R.build(case)
            assert case.slabs in R.valid_slabs(case.B) and all(np.isfinite(x).all() for x in b.want["dw"]), case.name
            assert any(np.any(x) for x in b.want["dw"]), case.name
    assert len(names) == len(T.POLICY_ROLLOUT_CASES) + len(T.GAUSSIAN_ROLLOUT_CASES) + 12 * len(T.MLP_WIDTHS), "case names repeat"
    grid = {(c.sizes[0], c.sizes[1], c.B) for w in T.MLP_WIDTHS for c in T.forward_cases(w)}
    assert grid == {(K, W, B) for K in (1, 5, 17) for W in (1, 15, 17, 65, 129) for B in (1, 15, 17, 33)}


# ---- the patterns --------------------------------------------------------------------------------------------------------------
def _words(pattern):
    return np.array([pattern], dtype=np.uint64)


def test_nan_pattern_is_a_quiet_nan_in_both_views():
    w = _words(LR.PATTERN_NAN)
    assert LR.PATTERNS["nan"] == 0x7FF8DEAD7FC0BEEF
    f32, f64 = w.view(np.float32), w.view(np.float64)
    assert np.isnan(f32).all() and np.isnan(f64).all()
    assert ((w.view(np.uint32) >> 22) & 1).all(), "float32: the quiet bit of both halves"
    assert ((w >> np.uint64(51)) & np.uint64(1)).all(), "float64: the quiet bit"
    assert w.view(np.uint32).tolist() == [0x7FC0BEEF, 0x7FF8DEAD], "low word at the even index (little endian)"


def test_huge_pattern_is_finite_and_enormous_in_both_views():
    w = _words(LR.PATTERN_HUGE)
    assert LR.PATTERNS["huge"] == 0x7F7FFFFF7F7FFFFF
    f32, f64 = w.view(np.float32), w.view(np.float64)
    assert np.isfinite(f32).all() and (f32 == np.finfo(np.float32).max).all()
    assert np.isfinite(f64).all() and (f64 > 1e300).all()
    assert (w.view(np.int32) > 0).all()


def test_ones_pattern_is_nan_minus_one_and_true():
    w = _words(LR.PATTERN_ONES)
    assert LR.PATTERNS["ones"] == 2 ** 64 - 1
    assert np.isnan(w.view(np.float32)).all() and np.isnan(w.view(np.float64)).all()
    assert (w.view(np.int32) == -1).all() and (w.view(np.int64) == -1).all()
    assert w.view(np.uint8).all() and w.view(np.bool_).all()


def test_pattern_names():
    assert sorted(LR.PATTERNS) == ["huge", "nan", "ones"]
    assert LR.pattern_of("nan") == LR.PATTERN_NAN and LR.pattern_of(0x1_0000_0000_0000_0005) == 5
    with pytest.raises(ValueError):
        LR.pattern_of("zeros")


# ---- dirtied() on a fake library ------------------------------------------------------------------------------------------------
class _Fn:
    """A stand-in for a ctypes function: records its calls, returns ``rc``."""

    def __init__(self, name, argtypes, rc=0):
        self.name, self.argtypes, self.restype, self.rc, self.calls = name, argtypes, C.c_int, rc, []

    def __call__(self, *args):
        self.calls.append(args)
        return self.rc


class _Lib:
    def __init__(self):
        p, i = C.c_void_p, C.c_int32
        self.with_stream = _Fn("with_stream", [C.POINTER(C.c_int), i, p], rc=0)
        self.failing = _Fn("failing", [p, p], rc=-3)
        self.workspace = _Fn("workspace", [p, i], rc=4096)             # ends in an integer: no stream
        self.no_args = _Fn("no_args", None, rc=21)
        self.debug_set = _Fn("debug_set", [i, i], rc=1)


NAMES = ["with_stream", "failing", "workspace", "no_args", "debug_set"]


def _dirtied(lib, log, pattern="nan"):
    return LR.dirtied(pattern, lib=lib, dirty_fn=lambda bits, stream: log.append((bits, stream)), names=NAMES)


def test_dirtied_wraps_exactly_the_stream_taking_exports():
    lib, log = _Lib(), []
    originals = {n: getattr(lib, n) for n in NAMES}
    assert LR.stream_exports(lib, NAMES) == ["with_stream", "failing"]
    with _dirtied(lib, log):
        for n in NAMES:
            assert (getattr(lib, n) is not originals[n]) == (n in ("with_stream", "failing")), n
        assert lib.with_stream.argtypes is originals["with_stream"].argtypes      # (a caller that reads the prototype still can)
        assert lib.with_stream.lds_dirtied_original is originals["with_stream"]
    for n in NAMES:
        assert getattr(lib, n) is originals[n], n


def test_dirtied_counts_and_passes_arguments_and_return_codes_through():
    lib, log = _Lib(), []
    with _dirtied(lib, log, "huge") as d:
        assert lib.with_stream("args", 5, 0xBEEF) == 0
        assert lib.failing(None, 0xF00D) == -3
        assert lib.with_stream("again", 6, None) == 0
        assert lib.workspace(None, 3) == 4096 and lib.no_args() == 21
    assert lib.with_stream.calls == [("args", 5, 0xBEEF), ("again", 6, None)] and lib.failing.calls == [(None, 0xF00D)]
    assert log == [(LR.PATTERN_HUGE, 0xBEEF), (LR.PATTERN_HUGE, 0xF00D), (LR.PATTERN_HUGE, None)], "one dirty launch per call, on the call's stream, first"
    assert d.entry_calls == 3 and d.dirty_launches == 3 and d.by_entry == {"with_stream": 2, "failing": 1}
    d.check("with_stream", "failing")
    with pytest.raises(AssertionError, match="workspace was not called"):
        d.check("workspace")


def test_exact_check_refuses_an_entry_point_the_case_did_not_name():
    lib, log = _Lib(), []
    with _dirtied(lib, log) as d:
        lib.with_stream(None, 1, 7)
        lib.failing(None, 7)
    d.check("with_stream", "failing", exact=True)
    with pytest.raises(AssertionError, match="entry points called inside"):
        d.check("with_stream", exact=True)
    with pytest.raises(AssertionError, match="workspace was not called"):
        d.check("with_stream", "failing", "workspace", exact=True)


def test_the_dirty_launch_comes_before_the_call():
    lib, order = _Lib(), []

    class Ordered(_Fn):
        def __call__(self, *args):
            order.append("call")
            return 0
    lib.with_stream = Ordered("with_stream", lib.with_stream.argtypes)
    with LR.dirtied("nan", lib=lib, dirty_fn=lambda bits, stream: order.append("dirty"), names=NAMES):
        lib.with_stream(None, 1, 7)
    assert order == ["dirty", "call"]


def test_a_run_that_dirtied_nothing_cannot_pass():
    lib, log = _Lib(), []
    with _dirtied(lib, log) as d:
        lib.workspace(None, 3)
    with pytest.raises(AssertionError, match="proved nothing"):
        d.check()


def test_a_failed_dirty_launch_is_not_counted_as_one():
    lib = _Lib()

    def refuse(bits, stream):
        raise RuntimeError("lds_dirty: the launch failed")
    with LR.dirtied("nan", lib=lib, dirty_fn=refuse, names=NAMES) as d:
        with pytest.raises(RuntimeError):
            lib.with_stream(None, 1, 7)
    assert d.entry_calls == 1 and d.dirty_launches == 0 and lib.with_stream.calls == []
    with pytest.raises(AssertionError):
        d.check()


def test_dirtied_restores_on_exception():
    lib, log = _Lib(), []
    originals = {n: getattr(lib, n) for n in NAMES}
    with pytest.raises(KeyError):
        with _dirtied(lib, log):
            raise KeyError("a failing test body")
    for n in NAMES:
        assert getattr(lib, n) is originals[n], n
    with _dirtied(lib, log):          # and the next context can be entered
        pass


def test_dirtied_refuses_nesting():
    lib, log = _Lib(), []
    with _dirtied(lib, log):
        with pytest.raises(RuntimeError, match="does not nest"):
            with _dirtied(_Lib(), []):
                pass
        assert lib.with_stream.lds_dirtied_original is not None      # the outer context is still in place
    with _dirtied(lib, log):
        pass


def test_a_wrapper_kept_past_the_exit_is_a_pass_through():
    lib, log = _Lib(), []
    with _dirtied(lib, log) as d:
        kept = lib.with_stream             # what a prepared call of backend.py holds
        kept(None, 1, 11)
    assert kept(None, 2, 12) == 0
    assert log == [(LR.PATTERN_NAN, 11)] and d.entry_calls == 1 and d.dirty_launches == 1
    assert lib.with_stream.calls == [(None, 1, 11), (None, 2, 12)]


def test_stream_exports_of_the_binding_are_the_headers():
    """Every entry point of include/pdegym.h whose last parameter is ``void* stream`` -- and no other -- is what ``dirtied`` wraps
    (read off the prototypes _native.load() declares)."""
    from pdecontrolgym_amd import _native as N
    from pdecontrolgym_amd import build
    build.build()              # (cross-compiles without a GPU; returns at once when the library is up to date)
    with open(os.path.join(ROOT, "include", "pdegym.h")) as f:
        text = re.sub(r"//[^\n]*|/\*.*?\*/", " ", f.read(), flags=re.S)
    in_header = set(re.findall(r"\b(pdegym_\w+)\s*\([^;{}]*?\bvoid\s*\*\s*stream\s*\)\s*;", text))
    assert len(in_header) >= 40
    assert set(LR.stream_exports(N.load())) == in_header


# ---- the library ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")), reason="no hipcc")
def test_lds_residue_hip_compiles_for_gfx950(tmp_path):
    from pdecontrolgym_amd import build
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    out = tmp_path / "lds_residue.so"
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-o", str(out), build.LDS_RESIDUE_SRC],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()
    lib = C.CDLL(str(out))
    for sym in ("lds_residue_info", "lds_dirty", "lds_witness", "lds_pad_probe"):
        assert hasattr(lib, sym), sym
