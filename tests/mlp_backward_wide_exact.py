"""Exactly summable cases and one-hot probes for the wide MLP backward pass (pdegym_mlp_backward_wide: layers of up to 256 units).

The reference, the case machinery and the exactness bound are those of tests/mlp_backward_exact.py (``R.Case`` / ``R.build`` /
``R.assert_exact``), imported as they are.  What is new here is the case list and ONE more condition.  With 256-unit layers the
default ``nnz=(16, 4)`` leaves most of a hidden layer's dW zero (1.6 % of its entries for a one-unit output): a kernel that dropped a
whole 16 x 16 tile of it, or a 16-column tile of dx, would still pass.  ``assert_every_tile_is_hit`` therefore demands a non-zero
entry in EVERY 16 x 16 tile of every expected dW_l (ragged edge tiles included) and in every 16-column tile of the expected dx, and
``build`` asserts it for every case of the list; tests/test_mlp_backward_wide.py runs ``build`` on the CPU for all of them.

The GPU case lists live here so that the CPU test can check every case.  Plain helper module (not a conftest).
"""
from __future__ import annotations

import dataclasses

import numpy as np

from tests import mlp_backward_exact as R

ROWS = R.ROWS
SLAB_TILES, MAX_SLABS = 8, 64      # the wide entry's choice for slabs = 0: min(ceil(tiles / 8), 64)  (include/pdegym.h)
TILE = 16


def library_slabs(B):
    """What ``slabs = 0`` means to pdegym_mlp_backward_wide: a function of B alone."""
    return min(-(-R.tiles_of(B) // SLAB_TILES), MAX_SLABS)


def workspace_bytes(sizes, B, slabs):
    """The answer of pdegym_mlp_backward_wide_workspace, restated: 16 tiles x (dZ_l of every layer + H_{l-1} of l >= 1, rows padded to a
    multiple of 64 floats) and ``slabs`` sets of partial dW_l, db_l."""
    pad = lambda n: -(-n // 64) * 64
    slabs = slabs or library_slabs(B)
    row = sum(pad(sizes[l + 1]) + (pad(sizes[l]) if l >= 1 else 0) for l in range(len(sizes) - 1))
    part = sum(sizes[l + 1] * (sizes[l] + 1) for l in range(len(sizes) - 1))
    return 4 * (R.tiles_of(B) * ROWS * row + slabs * part)


def empty_tiles(a, rows=TILE, cols=TILE):
    """[(first row, first column)] of the ``rows`` x ``cols`` tiles of the 2-D array ``a`` (edge tiles ragged) that hold only zeros."""
    a = np.asarray(a)
    return [(i, j) for i in range(0, a.shape[0], rows) for j in range(0, a.shape[1], cols) if not a[i:i + rows, j:j + cols].any()]


def assert_every_tile_is_hit(want, what="case"):
    """Every 16 x 16 tile of every expected dW_l and every 16-column tile of the expected dx (all rows) holds a non-zero entry."""
    for l, dw in enumerate(want["dw"]):
        bad = empty_tiles(dw)
        assert not bad, f"{what}: dW_{l} has {len(bad)} all-zero 16 x 16 tiles, the first at {bad[0]}: a dropped tile would not show"
    bad = empty_tiles(want["dx"], rows=want["dx"].shape[0])
    assert not bad, f"{what}: dx has all-zero 16-column tiles at {bad}"


def build(case):
    """``R.build(case)`` (which asserts exactness) plus the tile condition.  The expected dx is computed and checked for cases
    launched without dx as well."""
    b = R.build(case)
    assert_every_tile_is_hit(b.want, case.name)
    return b


def _cases():
    r, n_ = "relu", None
    C = R.Case
    c = [
        # the four cases the issue's table gives (seed 11)
        C("critic-66-256-256-16", (66, 256, 256, 16), (r, r, n_), 49, 2, seed=11, nnz=(16, 32)),
        C("critic-66-256-256-32", (66, 256, 256, 32), (r, r, n_), 49, 2, seed=11, nnz=(16, 64)),
        C("four-layers-70-65-129-256-48", (70, 65, 129, 256, 48), (r, r, n_, n_), 33, 2, seed=11, nnz=(16, 16)),
        C("long-rows-1024-200-100-8", (1024, 200, 100, 8), (r, r, n_), 33, 2, seed=11, nnz=(16, 100)),
    ]
    # widths on the seams of the 16-unit tiles, the 64-unit blocks and the 256-unit limit, as the hidden layer; batches walk along
    for i, W in enumerate((65, 80, 128, 129, 255, 256)):
        B = R.BATCHES[(i + 2) % 6]
        slabs = R.valid_slabs(B)[i % len(R.valid_slabs(B))]
        c.append(C(f"hidden{W}-B{B}", (70, W, 32), (n_ if B < 16 else r, n_), B, slabs, seed=20 + i, nnz=(16, 64)))
    # narrow and wide layers in one network
    c.append(C("mixed-70-64-256-17-33", (70, 64, 256, 17, 33), (r, r, r, n_), 49, 3, seed=31, nnz=(16, 32)))
    c.append(C("mixed-5-256-16-200", (5, 256, 16, 200), (r, n_, n_), 17, 2, seed=32, nnz=(16, 16)))
    # one case each without bias, with float64 rows (rounded as they are read), with row gaps, without dx
    base = dict(sizes=(65, 129, 80, 32), acts=(r, r, n_), nnz=(16, 48))
    c.append(C("no-bias", B=33, slabs=3, seed=41, bias=False, **base))
    c.append(C("float64-rows", B=17, slabs=2, seed=42, x_f64=True, eps=True, dx=False, **base))
    c.append(C("row-gaps", B=49, slabs=0, seed=43, gaps=True, **base))
    c.append(C("no-dx", B=16, slabs=1, seed=44, dx=False, **base))
    return c


CASES = _cases()

# one-hot probes of ONE Linear layer with ordinary random float32 weights (mlp_exact.real_linear): (in_dim, out_dim)
ONE_HOT_CASES = [(K, H) for K in (5, 66, 130, 513, 1024) for H in (65, 129, 256)]
# the same through a hidden layer: K - K - H with identity activations and W_0 = I, so that H_0 is the one-hot input
HIDDEN_ONE_HOT_CASES = [(K, H) for K in (65, 256) for H in (65, 129, 256)]

# networks both entry points take, for the equal-bits test: (sizes, activation)
BOTH_ENTRIES = [((65, 64, 64, 1), "tanh"), ((70, 64, 33, 2), "relu")]

# real-valued networks of the tolerance test: (sizes, activation, B); B = 4113 spans 33 slabs and ends in a ragged tile
REAL_CASES = [(s, a, B) for s, a in (((66, 256, 256, 1), "relu"), ((65, 256, 256, 2), "tanh")) for B in (17, 4113)]


def mutated(case, **changes):
    return dataclasses.replace(case, **changes)
