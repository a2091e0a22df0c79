"""CPU tests of tests/poison.py, the guard-band / poison helper of the GPU output-contract suite."""
import pytest
import torch

from tests import poison as P


def test_payload_alignment_and_guard_size():
    for shape, dtype in (((3, 5), torch.float32), ((7,), torch.float64), ((1, 1, 3), torch.uint8)):
        g = P.Guarded("x", shape, dtype, "cpu")
        assert g.t.shape == shape and g.t.dtype == dtype and g.t.is_contiguous()
        assert g.t.data_ptr() % 256 == 0
        assert g.t.data_ptr() - g.raw.data_ptr() >= 4096
        assert g.raw.data_ptr() + g.raw.numel() - (g.t.data_ptr() + g.nbytes) >= 4096
        assert bool((g.t == 0).all())
        g.check_guards()


@pytest.mark.parametrize("after", [True, False])
def test_changed_guard_byte_is_reported(after):
    t, check = P.guarded((4, 3), torch.float32, "cpu", name="obs")
    t.fill_(1.0)
    check()
    raw = t.untyped_storage()
    base = t.storage_offset() * 4
    if after:
        raw[base + t.numel() * 4 + 2] = 0          # the third byte past the payload end
        with pytest.raises(AssertionError, match=r"'obs'.*\+2 AFTER"):
            check()
    else:
        raw[base - 4] = 0                          # one float32 before the payload
        with pytest.raises(AssertionError, match=r"'obs'.*4 byte\(s\) BEFORE"):
            check()


def test_one_element_overrun_lands_in_the_guard():
    g = P.Guarded("reward", (5,), torch.float64, "cpu")
    g.raw[4096:4096 + 6 * 8].view(torch.float64)[5] = 0.0      # reward[B] with B = 5
    with pytest.raises(AssertionError, match=r"\+0 AFTER"):
        g.check_guards()


DTYPES = (torch.uint8, torch.int32, torch.float32, torch.float64, torch.int64)


@pytest.mark.parametrize("policy", ["one", "mixed"])
def test_displaced_payload_alignment_and_guard_size(policy):
    """Arena(policy=...): data_ptr() % 256 == shift for every dtype, shift a multiple of the element size and (for 'mixed') no
    multiple of 16; both guards keep their 4 KiB; the tail guard starts at the payload's last byte + 1."""
    a = P.Arena("cpu", policy=policy, keep_aligned=("held",))
    seen = {}
    for dtype in DTYPES:
        item = torch.empty((), dtype=dtype).element_size()
        for name in ("obs", "reward", "u", "terminated", "w0", "scratch"):
            t = a.new(f"{name}_{item}", (3, 5), dtype)
            g = a.bufs[f"{name}_{item}"]
            shift = a.shift_of(f"{name}_{item}", dtype)
            assert g.shift == shift and t.data_ptr() % 256 == shift
            assert shift % item == 0 and shift % 16 != 0 and 0 < shift < 256
            if policy == "one":
                assert shift == item
            else:
                assert shift // item in ({1: range(1, 16), 4: range(1, 4), 8: range(1, 2)}[item])
                assert shift == P.policy_shift("mixed", f"{name}_{item}", dtype)       # a function of the name alone
            seen.setdefault(item, set()).add(shift)
            assert t.shape == (3, 5) and t.dtype == dtype and t.is_contiguous() and bool((t == 0).all())
            assert t.data_ptr() - g.raw.data_ptr() == 4096 + shift
            assert g._tail.data_ptr() == t.data_ptr() + g.nbytes
            assert g._tail.numel() >= 4096 and (g._tail.data_ptr() + g._tail.numel()) % 256 == 0
    if policy == "mixed":                       # the residues do differ between the buffers of one launch
        assert len(seen[1]) >= 3 and len(seen[4]) >= 2
    held = a.new("held", (7,), torch.float32)
    assert held.data_ptr() % 256 == 0 and a.bufs["held"].shift == 0
    a.check()
    with pytest.raises(ValueError):
        P.Arena("cpu", policy="two")
    with pytest.raises(ValueError):
        P.Guarded("x", (3,), torch.float32, "cpu", shift=6)


def test_default_shift_is_zero():
    a = P.Arena("cpu")
    assert a.new("x", (5,), torch.float32).data_ptr() % 256 == 0 and a.bufs["x"].shift == 0
    t, _ = P.guarded((5,), torch.float64, "cpu")
    assert t.data_ptr() % 256 == 0


@pytest.mark.parametrize("dtype", [torch.uint8, torch.float32, torch.float64])
@pytest.mark.parametrize("policy", ["one", "mixed"])
def test_displaced_one_element_overrun_and_underrun(policy, dtype):
    """Displaced payload: element [numel] is byte +0 AFTER the payload, element [-1] lands in the head guard right before it."""
    item = torch.empty((), dtype=dtype).element_size()
    a = P.Arena("cpu", policy=policy)
    t = a.new("reward", (5,), dtype)
    g = a.bufs["reward"]
    start = 4096 + g.shift
    g.raw[start:start + 6 * item].view(dtype)[5] = 0
    with pytest.raises(AssertionError, match=r"'reward' changed at byte \+0 AFTER"):
        a.check()
    g.raw[start + 5 * item:start + 6 * item] = P.GUARD_BYTE
    a.check()
    g.raw[start - item:start + 5 * item].view(dtype)[0] = 0
    with pytest.raises(AssertionError, match=rf"'reward' changed 1 byte\(s\) BEFORE the payload \({item} byte"):
        a.check()
    del t


def test_poison_patterns():
    f = P.poison_(torch.zeros(3, dtype=torch.float32))
    d = P.poison_(torch.zeros(3, dtype=torch.float64))
    u = P.poison_(torch.zeros(3, dtype=torch.uint8))
    assert bool(torch.isnan(f).all()) and bool(torch.isnan(d).all())
    assert int(P.bits(f)[0]) == 0x7FC0DEAD and int(P.bits(d)[0]) == 0x7FF8DEADDEADBEEF and int(u[0]) == 0xA5
    with pytest.raises(TypeError):
        P.poison_(torch.zeros(3, dtype=torch.int32))          # integer index buffers take an in-range value instead
    ti = P.fill_int_(torch.zeros(3, dtype=torch.int32), 7)
    assert ti.tolist() == [7, 7, 7]


def test_surviving_poison_is_reported():
    t = P.poison_(torch.empty(4, 6, dtype=torch.float32))
    t[:, :5] = 0.0                                             # a "kernel" that skips the last column
    with pytest.raises(AssertionError, match=r"1 of 6 element.*still hold the poison; first at index \(0, 5\)"):
        P.assert_written(t[:1])
    with pytest.raises(AssertionError, match=r"first at index \(0, 5\)"):
        P.assert_written(t)
    P.assert_written(t, (slice(None), slice(0, 5)))           # index expression
    P.assert_untouched(t, (slice(None), 5))
    m = torch.zeros(4, 6, dtype=torch.bool)
    m[2, 3] = True
    with pytest.raises(AssertionError, match=r"left alone were written; first at index \(2, 3\)"):
        P.assert_untouched(t, m)
    f = P.poison_(torch.empty(3, dtype=torch.uint8))
    f[1] = 0
    with pytest.raises(AssertionError, match=r"first at index \(1,\)"):
        P.assert_untouched(f, None, name="terminated")


def test_kernel_nan_is_not_poison():
    t = P.poison_(torch.empty(5, dtype=torch.float32))
    t[:] = float("nan")                                       # canonical quiet NaN 0x7FC00000
    P.assert_written(t)
    with pytest.raises(AssertionError):
        P.assert_untouched(t)
    d = P.poison_(torch.empty(2, dtype=torch.float64))
    d[0] = float("nan")
    P.assert_written(d, 0)
    P.assert_untouched(d, 1)


def test_bits_equal_tells_signed_zero_and_nan_payloads_apart():
    a = torch.tensor([0.0, 1.0, float("nan")])
    b = torch.tensor([-0.0, 1.0, float("nan")])
    with pytest.raises(AssertionError, match=r"first at index \(0,\)"):
        P.assert_bits_equal(a, b)
    P.assert_bits_equal(a, b, slice(1, 3))
    P.assert_written(a, None, like=a.clone())
    with pytest.raises(AssertionError):
        P.assert_written(P.poison_(torch.empty(3)), slice(0, 1), like=a)


def test_arena_checks_every_buffer():
    a = P.Arena("cpu")
    x = a.new("x", (2, 2), torch.float32)
    y = a.like("y", torch.arange(3, dtype=torch.float64))
    assert y.tolist() == [0.0, 1.0, 2.0]
    a.check()
    a.bufs["x"].raw[-1] = 0
    with pytest.raises(AssertionError, match="'x'"):
        a.check()
    del x


def test_every_launched_kernel_is_in_the_contract_suite():
    """Every kernel launched in pdecontrolgym_amd/csrc/*.hip is listed in test_gpu_buffer_contract.KERNEL_CASES, and every test
    named there exists: a kernel added later cannot skip the output-contract suite."""
    import glob
    import os
    import re
    from tests import test_gpu_buffer_contract as C
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    launched = set()
    for f in glob.glob(os.path.join(root, "pdecontrolgym_amd", "csrc", "*.hip")):
        src = open(f).read()
        launched |= set(re.findall(r"hipLaunchKernelGGL\(\s*\(?\s*([A-Za-z_]\w*)", src))
    assert len(launched) >= 30
    missing = sorted(launched - set(C.KERNEL_CASES))
    assert not missing, f"kernels without a case in test_gpu_buffer_contract.KERNEL_CASES: {missing}"
    stale = sorted(set(C.KERNEL_CASES) - launched)
    assert not stale, f"KERNEL_CASES names kernels nothing launches: {stale}"
    import importlib

    def named(t):      # "test" of the contract module, or "module::test" of another module under tests/
        mod, _, name = t.rpartition("::")
        return getattr(importlib.import_module("tests." + mod) if mod else C, name, None)
    for k, tests in C.KERNEL_CASES.items():
        assert tests and all(callable(named(t)) for t in tests), (k, tests)


def test_every_launched_kernel_is_in_the_alignment_suite():
    """Every kernel launched in pdecontrolgym_amd/csrc/*.hip -- by hipLaunchKernelGGL or by the chevron syntax, with or without
    template arguments -- is listed in test_gpu_pointer_alignment.ALIGNMENT_CASES, and every test named there exists: a kernel added
    later cannot skip the displaced-pointer suite."""
    import glob
    import os
    import re
    from tests import test_gpu_pointer_alignment as A
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    launched = set()
    for f in glob.glob(os.path.join(root, "pdecontrolgym_amd", "csrc", "*.hip")):
        src = open(f).read()
        launched |= set(re.findall(r"hipLaunchKernelGGL\(\s*\(?\s*([A-Za-z_]\w*)", src))
        launched |= set(re.findall(r"([A-Za-z_]\w*)\s*(?:<[^<>;]*>)?\s*<<<", src))
    assert len(launched) >= 45
    missing = sorted(launched - set(A.ALIGNMENT_CASES))
    assert not missing, f"kernels without a case in test_gpu_pointer_alignment.ALIGNMENT_CASES: {missing}"
    stale = sorted(set(A.ALIGNMENT_CASES) - launched)
    assert not stale, f"ALIGNMENT_CASES names kernels nothing launches: {stale}"
    for k, tests in A.ALIGNMENT_CASES.items():
        assert tests and all(callable(getattr(A, t, None)) for t in tests), (k, tests)
