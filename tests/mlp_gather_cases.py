"""The thinned case product of tests/test_gpu_mlp_gather.py (rows by index: pdegym_mlp_forward_gather, pdegym_mlp_backward_gather,
pdegym_mlp_backward_wide_gather), kept apart so that the CPU suite can hold it to its covering condition without a device
(tests/test_mlp_gather.py).

``cases(family)`` keeps 21 cells of the full product per family -- narrow: pdegym_mlp_backward_gather (mlp_backward_tiles,
mlp_backward_dw0), wide: pdegym_mlp_backward_wide_gather (mlp_backward_wide_tiles, mlp_backward_wide_accumulate);
pdegym_mlp_forward_gather (mlp_forward_kernel) runs in every case of both -- by walking every parameter's value list with its own
stride, under the constraints of the contract, applied HERE and never by skipping on the device: ``slabs`` at most the number of 16-row
tiles; ``tail_indexed`` only with a tail (n2 >= 1); ``params == 0`` (the one-launch pass, which exists for dx2 alone) only with a dense
tail.  ``assert_covering`` states the condition that makes the thinning sound: every value of every parameter meets every kernel at
least once -- the two kernels that run only with ``params`` (dw0, accumulate) on the cases that have it.  ``index_of`` builds the index
patterns.  Plain helper module (not a conftest)."""
from __future__ import annotations

import dataclasses

import numpy as np

BATCHES = (1, 15, 16, 17, 33)
POOLS = (1, 7, 40)                                                                          # M: rows of the storage
PARTS = ((1, 0), (3, 1), (5, 3), (63, 8), (65, 0), (200, 1), (1016, 8))                     # (D, n2)
WIDTHS = {"narrow": (1, 15, 64), "wide": (65, 129, 256)}
SLABS = (0, 1, 2)
PATTERNS = ("identity", "reversed", "equal", "random", "last")
VALUES = {"B": BATCHES, "M": POOLS, "part": PARTS, "x_f64": (False, True), "x_gap": (0, 3), "x2_gap": (0, 1), "slabs": SLABS,
          "params": (0, 1), "tail_indexed": (False, True), "layers": (1, 2, 3, 4), "act": ("tanh", "relu"), "pattern": PATTERNS}
KERNELS = {"narrow": ("mlp_forward_kernel", "mlp_backward_tiles", "mlp_backward_dw0"),
           "wide": ("mlp_forward_kernel", "mlp_backward_wide_tiles", "mlp_backward_wide_accumulate")}
NEEDS_PARAMS = ("mlp_backward_dw0", "mlp_backward_wide_accumulate")
N_CASES = 21


@dataclasses.dataclass(frozen=True)
class GatherCase:
    family: str
    B: int
    M: int
    part: tuple          # (D, n2)
    width: int           # the widest hidden layer (the output layer when there is one layer)
    x_f64: bool
    x_gap: int           # x_stride - D
    x2_gap: int          # x2_stride - n2
    slabs: int
    params: int
    tail_indexed: bool
    layers: int
    act: str
    pattern: str
    seed: int

    @property
    def name(self):
        return (f"{self.family}-B{self.B}-M{self.M}-D{self.part[0]}+{self.part[1]}-w{self.width}-L{self.layers}{self.act}-"
                f"{'f64' if self.x_f64 else 'f32'}-g{self.x_gap}{self.x2_gap}-s{self.slabs}-p{self.params}-{'ti' if self.tail_indexed else 'td'}-{self.pattern}")

    @property
    def sizes(self):
        """Layer sizes: in_dim, the hidden widths (the widest first, then narrower ones off the 16-unit seams), the outputs."""
        D, n2 = self.part
        hidden = [self.width, max(1, self.width - 3), max(1, self.width // 2 + 1)][: self.layers - 1]
        out = self.width if self.layers == 1 else (1, 2, 5)[self.seed % 3]
        return (D + n2, *hidden, out)


def index_of(pattern, B, M, seed):
    """The int64 [B] index of a pattern over a storage of M rows (NumPy): identity-truncated (row b, the last row past the storage),
    reversed, all entries equal, with replacement from a seeded generator, every entry M - 1."""
    b = np.arange(B, dtype=np.int64)
    if pattern == "identity":
        return np.minimum(b, M - 1)
    if pattern == "reversed":
        return M - 1 - np.minimum(b, M - 1)
    if pattern == "equal":
        return np.full(B, M // 2, dtype=np.int64)
    if pattern == "random":
        return np.random.default_rng([77, seed]).integers(0, M, B, dtype=np.int64)
    if pattern == "last":
        return np.full(B, M - 1, dtype=np.int64)
    raise ValueError(pattern)


def cases(family):
    rng = np.random.default_rng([2026, 0 if family == "narrow" else 1])
    rot = {k: int(rng.integers(0, 64)) for k in ("B", "M", "width", "x_gap", "x2_gap", "layers", "act", "pattern", "ti")}
    out = []
    for i in range(N_CASES):
        j, k = i % 7, i // 7                            # every (D, n2) three times
        n2 = PARTS[j][1]
        params = 0 if (k == 1 and n2) else 1            # the one-launch pass: five cases, on the parts with a tail
        tail_indexed = bool(n2) and bool(params) and (j // 2 + k + rot["ti"]) % 2 == 0
        x_f64 = (j + k) % 2 == 1
        slabs = SLABS[(j + k) % 3]
        allowed = [B for B in BATCHES if slabs <= -(-B // 16)]
        B = allowed[(i + rot["B"]) % len(allowed)]
        out.append(GatherCase(family, B, POOLS[(i + rot["M"]) % 3], PARTS[j], WIDTHS[family][(j + 2 * k + rot["width"]) % 3], x_f64,
                              (0, 3)[(j // 2 + k + rot["x_gap"]) % 2], (0, 1)[(j + k + rot["x2_gap"]) % 2], slabs, params, tail_indexed,
                              1 + (i + rot["layers"]) % 4, ("tanh", "relu")[(j // 2 + k + rot["act"]) % 2],
                              PATTERNS[(i + rot["pattern"]) % 5], seed=1000 + 100 * (family == "wide") + i))
    return out


def assert_covering(family, cs):
    """Every value of every parameter appears with every kernel of the family (docstring above), within the contract."""
    for kernel in KERNELS[family]:
        mine = [c for c in cs if c.params or kernel not in NEEDS_PARAMS]      # the cases that launch this kernel
        values = dict(VALUES, width=WIDTHS[family])
        for key, want in values.items():
            if key == "params" and kernel in NEEDS_PARAMS:
                want = (1,)
            # a row gap of x2 is met only where there is an x2
            seen = {getattr(c, key) for c in mine if key != "x2_gap" or c.part[1]}
            missing = [v for v in want if v not in seen]
            assert not missing, f"{family}: {kernel} never meets {key} = {missing}"
    for c in cs:
        assert c.slabs <= -(-c.B // 16), c.name
        assert not (c.tail_indexed and not c.part[1]), c.name
        assert c.params or (c.part[1] and not c.tail_indexed), c.name
