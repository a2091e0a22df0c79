"""CPU tests of tests/nonfinite.py, the comparison helper of the non-finite suite."""
import struct

import numpy as np
import pytest
import torch

from tests import nonfinite as NF


def _nan64(payload):
    return struct.unpack("<d", struct.pack("<Q", 0x7FF8000000000000 | payload))[0]


def test_nan_against_finite_is_rejected_with_index_and_counts():
    want = np.array([[1.0, np.nan, 3.0], [4.0, 5.0, 6.0]])
    got = want.copy()
    got[0, 1] = 0.0                                            # a clamp that turned the NaN into a bound
    with pytest.raises(AssertionError, match=r"obs: NaN masks differ in 1 of 6 .*first at index \(0, 1\).*got 0, want 1"):
        NF.same_bits_and_nans(got, want, "obs")
    with pytest.raises(AssertionError, match=r"first at index \(0, 1\)"):
        NF.nan_mask_equal(got, want)
    with pytest.raises(AssertionError, match=r"first at index \(0, 1\)"):
        NF.close_and_same_nans(got, want, rtol=1.0)
    got = want.copy()
    got[1, 2] = np.nan                                         # and the other way round
    with pytest.raises(AssertionError, match=r"first at index \(1, 2\).*got 2, want 1"):
        NF.same_bits_and_nans(got, want)


def test_signed_zero_and_sign_of_infinity_count():
    a = np.array([0.0, np.inf, np.nan, 2.0])
    with pytest.raises(AssertionError, match=r"bits differ in 1 of 4 .*first at index \(0,\)"):
        NF.same_bits_and_nans(np.array([-0.0, np.inf, np.nan, 2.0]), a)
    with pytest.raises(AssertionError, match=r"first at index \(1,\)"):
        NF.same_bits_and_nans(np.array([0.0, -np.inf, np.nan, 2.0]), a)
    with pytest.raises(AssertionError, match=r"first at index \(1,\)"):
        NF.close_and_same_nans(np.array([0.0, -np.inf, np.nan, 2.0]), a, rtol=1e-3)
    NF.nan_mask_equal(np.array([-0.0, -np.inf, np.nan, 7.0]), a)          # the mask check looks at nothing else
    NF.close_and_same_nans(np.array([-0.0, np.inf, np.nan, 2.0 + 1e-9]), a, rtol=1e-6)
    with pytest.raises(AssertionError, match=r"first at index \(3,\)"):
        NF.close_and_same_nans(np.array([0.0, np.inf, np.nan, 2.1]), a, rtol=1e-6)


def test_shifted_mask_is_rejected():
    want = np.zeros((5, 5), dtype=np.float32)
    want[2, 1:4] = np.nan
    got = np.zeros((5, 5), dtype=np.float32)
    got[2, 2:5] = np.nan                                       # the same count, one cell to the right
    for f in (NF.same_bits_and_nans, NF.nan_mask_equal):
        with pytest.raises(AssertionError, match=r"differ in 2 of 25 .*first at index \(2, 1\).*got 3, want 3"):
            f(got, want)
    NF.nan_mask_equal(want.astype(np.float64), want)            # float32 engine against the float64 oracle


def test_nan_payloads_are_ignored():
    a = np.array([1.0, _nan64(0), -2.0])
    b = np.array([1.0, _nan64(0xDEADBEEF), -2.0])
    c = np.array([1.0, -_nan64(1), -2.0])                       # sign bit of a NaN is payload too
    assert a.view(np.uint64)[1] != b.view(np.uint64)[1]
    NF.same_bits_and_nans(a, b)
    NF.same_bits_and_nans(a, c)
    f = torch.tensor([float("nan"), 1.0])
    g = f.clone()
    g.view(torch.int32)[0] = 0x7FC0DEAD
    NF.same_bits_and_nans(f, g)
    NF.same_bits_and_nans(f, g.numpy())


def test_dtype_shape_and_integer_arrays():
    with pytest.raises(AssertionError, match="dtype"):
        NF.same_bits_and_nans(np.zeros(3, dtype=np.float32), np.zeros(3))
    with pytest.raises(AssertionError, match="shape"):
        NF.nan_mask_equal(np.zeros(3), np.zeros(4))
    NF.same_bits_and_nans(np.array([1, 0], dtype=np.uint8), np.array([1, 0], dtype=np.uint8))
    with pytest.raises(AssertionError, match=r"first at index \(1,\)"):
        NF.same_bits_and_nans(np.array([1, 0], dtype=np.uint8), np.array([1, 1], dtype=np.uint8))


def test_planting_helpers():
    a = np.arange(6.0).reshape(2, 3)
    b = NF.plant(a, (1, 2))
    assert np.isnan(b[1, 2]) and a[1, 2] == 5.0                # a copy
    b = NF.plant(a, (0, 0), NF.NINF)
    assert b[0, 0] == -np.inf
    t = torch.zeros(4)
    assert NF.plant_(t, 2, NF.PINF) is t and t[2] == float("inf")
    assert NF.rows_except(5, [1, 3]) == [0, 2, 4]
    assert set(NF.PLANTS) == {"nan", "+inf", "-inf"}
