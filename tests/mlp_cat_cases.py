"""The thinned case product of tests/test_gpu_mlp_cat.py (the critic(obs, action) entry points), kept apart so that the CPU suite can
hold it to its covering condition without a device (tests/test_mlp_cat.py).

The full product of the parameters below has some 10^5 cells per kernel family.  ``cases(family)`` keeps 18 of them per family --
narrow: pdegym_mlp_backward_cat (mlp_backward_tiles, mlp_backward_dw0), wide: pdegym_mlp_backward_wide_cat (mlp_backward_wide_tiles,
mlp_backward_wide_accumulate); pdegym_mlp_forward_cat (mlp_forward_kernel) runs in every case of both -- by walking every parameter's
value list with its own stride and a seeded rotation, under the constraints of the contract: ``dx`` only with float32 rows, ``slabs``
at most the number of 16-row tiles.  ``assert_covering`` states the condition that makes the thinning sound: every value of every
parameter meets every kernel at least once -- the two kernels that run only with ``params`` (dw0, accumulate) on the cases that have
it.  Plain helper module (not a conftest)."""
from __future__ import annotations

import dataclasses

import numpy as np

BATCHES = (1, 15, 16, 17, 33)
PARTS = ((1, 1), (3, 1), (4, 1), (5, 3), (62, 4), (63, 8), (65, 1), (200, 1), (1016, 8))      # (D, n2)
WIDTHS = {"narrow": (1, 15, 64), "wide": (65, 129, 256)}
SLABS = (0, 1, 2)
VALUES = {"B": BATCHES, "part": PARTS, "x_f64": (False, True), "x_gap": (0, 3), "x2_gap": (0, 1), "slabs": SLABS, "params": (0, 1),
          "dx": (False, True), "layers": (1, 2, 3, 4), "act": ("tanh", "relu")}
KERNELS = {"narrow": ("mlp_forward_kernel", "mlp_backward_tiles", "mlp_backward_dw0"),
           "wide": ("mlp_forward_kernel", "mlp_backward_wide_tiles", "mlp_backward_wide_accumulate")}
NEEDS_PARAMS = ("mlp_backward_dw0", "mlp_backward_wide_accumulate")
N_CASES = 18


@dataclasses.dataclass(frozen=True)
class CatCase:
    family: str
    B: int
    part: tuple          # (D, n2)
    width: int           # the widest hidden layer (the output layer when there is one layer)
    x_f64: bool
    x_gap: int           # x_stride - D
    x2_gap: int          # x2_stride - n2
    slabs: int
    params: int
    dx: bool
    layers: int
    act: str
    seed: int

    @property
    def name(self):
        return (f"{self.family}-B{self.B}-D{self.part[0]}+{self.part[1]}-w{self.width}-L{self.layers}{self.act}-{'f64' if self.x_f64 else 'f32'}"
                f"-g{self.x_gap}{self.x2_gap}-s{self.slabs}-p{self.params}-{'dx' if self.dx else 'nodx'}")

    @property
    def sizes(self):
        """Layer sizes: in_dim, the hidden widths (the widest first, then narrower ones off the 16-unit seams), the outputs."""
        D, n2 = self.part
        hidden = [self.width, max(1, self.width - 3), max(1, self.width // 2 + 1)][: self.layers - 1]
        out = self.width if self.layers == 1 else (1, 2, 5)[self.seed % 3]
        return (D + n2, *hidden, out)


def cases(family):
    rng = np.random.default_rng([2025, 0 if family == "narrow" else 1])
    rot = {k: int(rng.integers(0, 64)) for k in ("B", "width", "x_gap", "x2_gap", "layers", "act")}
    out = []
    for i in range(N_CASES):
        params, j = i % 2, i // 2                       # j = 0 .. 8: every (D, n2) with params and without
        x_f64 = (j + params) % 2 == 1
        dx = not x_f64 and (j // 2 + params) % 2 == 0
        slabs = SLABS[(j + 2 * params) % 3]
        allowed = [B for B in BATCHES if slabs <= -(-B // 16)]
        B = allowed[(j + rot["B"] + 3 * params) % len(allowed)]
        out.append(CatCase(family, B, PARTS[j], WIDTHS[family][(j + rot["width"] + params) % 3], x_f64, (0, 3)[(j // 2 + rot["x_gap"] + params) % 2],
                           (0, 1)[(j // 3 + rot["x2_gap"] + params) % 2], slabs, params, dx, 1 + (j + rot["layers"] + 2 * params) % 4,
                           ("tanh", "relu")[(j // 2 + rot["act"]) % 2], seed=100 * (family == "wide") + i))
    return out


def assert_covering(family, cs):
    """Every value of every parameter appears with every kernel of the family (docstring above)."""
    for kernel in KERNELS[family]:
        mine = [c for c in cs if c.params or kernel not in NEEDS_PARAMS]
        values = dict(VALUES, width=WIDTHS[family])
        for key, want in values.items():
            if key == "params" and kernel in NEEDS_PARAMS:
                want = (1,)
            seen = {getattr(c, key) for c in mine}
            missing = [v for v in want if v not in seen]
            assert not missing, f"{family}: {kernel} never meets {key} = {missing}"
    assert all(c.slabs <= -(-c.B // 16) and not (c.dx and c.x_f64) for c in cs)
