"""Comparisons and planting helpers for the non-finite tests (NaN / +-Inf commands, observations and state cells).

A NaN is ordinary data to the reference: np.clip, np.max, torch.clamp and Python's min/max (value first) all keep it, and a stencil
spreads it to exactly the cells that read it.  So two results agree when their NaN MASKS are equal and every other element has the
same bits (same_bits_and_nans: -0.0 != +0.0, the sign of an infinity counts, NaN payloads do not), or -- a float32 engine against
the float64 oracle -- when the masks alone are equal (nan_mask_equal) and the rest is within the family's tolerance.
"""
from __future__ import annotations

import numpy as np

NAN, PINF, NINF = float("nan"), float("inf"), float("-inf")
PLANTS = {"nan": NAN, "+inf": PINF, "-inf": NINF}


def _np(x):
    """NumPy view of an array or a (device) tensor; dtype kept."""
    if hasattr(x, "detach"):
        x = x.detach().cpu().numpy()
    return np.ascontiguousarray(x)


def _uint(a):
    if a.dtype.kind != "f":
        return a
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _first(bad):
    return tuple(int(i) for i in np.argwhere(bad)[0])


def nan_mask_equal(got, want, what="array"):
    """The NaN masks of `got` and `want` are equal (shapes too; the dtypes may differ).  Raises AssertionError naming the first
    differing index and the two NaN counts."""
    g, w = _np(got), _np(want)
    assert g.shape == w.shape, f"{what}: shape {g.shape} against {w.shape}"
    gm, wm = np.isnan(g), np.isnan(w)
    bad = gm != wm
    if bad.any():
        i = _first(bad)
        raise AssertionError(f"{what}: NaN masks differ in {int(bad.sum())} of {bad.size} element(s), first at index {i} "
                             f"(got {g[i]!r}, want {w[i]!r}); NaN count got {int(gm.sum())}, want {int(wm.sum())}")
    return True


def same_bits_and_nans(got, want, what="array"):
    """Equal NaN masks, and equal bit patterns everywhere else (same dtype required).  NaN payloads are ignored."""
    g, w = _np(got), _np(want)
    assert g.dtype == w.dtype, f"{what}: dtype {g.dtype} against {w.dtype}"
    nan_mask_equal(g, w, what)
    if g.dtype.kind != "f":
        bad = g != w
    else:
        bad = (_uint(g) != _uint(w)) & ~np.isnan(g)
    if bad.any():
        i = _first(bad)
        raise AssertionError(f"{what}: bits differ in {int(bad.sum())} of {bad.size} non-NaN element(s), first at index {i} "
                             f"(got {g[i]!r}, want {w[i]!r}); NaN count {int(np.isnan(g).sum())} on both sides")
    return True


def close_and_same_nans(got, want, rtol, atol=0.0, what="array"):
    """Equal NaN masks, infinities equal with their sign, every finite element within rtol / atol of `want`."""
    g, w = _np(got).astype(np.float64), _np(want).astype(np.float64)
    nan_mask_equal(g, w, what)
    fin = ~np.isnan(w)
    with np.errstate(invalid="ignore"):
        ok = np.where(np.isinf(w) | np.isinf(g), g == w, np.abs(g - w) <= atol + rtol * np.abs(w))
    bad = fin & ~ok
    if bad.any():
        i = _first(bad)
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} element(s) beyond rtol {rtol} atol {atol}, first at index {i} "
                             f"(got {g[i]!r}, want {w[i]!r})")
    return True


def plant(a, index, value=NAN):
    """A copy of array `a` with `value` at `index` (NumPy)."""
    out = np.array(a, copy=True)
    out[index] = value
    return out


def plant_(t, index, value=NAN):
    """Write `value` into tensor or array `t` at `index`, in place; returns t."""
    t[index] = value
    return t


def rows_except(n, poisoned):
    """Indices of the instances of a batch of n that received no non-finite value."""
    poisoned = set(int(p) for p in poisoned)
    return [i for i in range(n) if i not in poisoned]
