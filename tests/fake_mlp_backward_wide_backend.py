"""CPU double of a backend that offers BOTH backward passes: tests/fake_mlp_backward_backend.py's ``FakeMlpBackend`` plus
``mlp_backward_wide``, which computes the same float64 restatement and records its calls apart, so that a test sees which of the
two methods ``FusedMLP.with_grad`` chose.  Plain helper module."""
from __future__ import annotations

from pdecontrolgym_amd import _native as N
from tests.fake_mlp_backward_backend import FakeMlpBackend


class FakeWideMlpBackend(FakeMlpBackend):
    def __init__(self):
        super().__init__()
        self.wide_calls = []

    def mlp_backward_wide(self, net, x, dy, weights, dw, db, dx=None, slabs=0):
        for l in range(net.n_layers):
            assert net.layer[l].out_dim <= N.MLP_BACKWARD_WIDE_MAX_WIDTH, "the wide pass takes at most 256 units per layer"
        assert net.layer[0].in_dim <= N.MLP_BACKWARD_WIDE_MAX_INPUT, "the wide pass takes rows of at most 1024 inputs"
        narrow = len(self.backward_calls)
        FakeMlpBackend.mlp_backward(self, net, x, dy, weights, dw, db, dx, slabs)
        self.wide_calls.append(self.backward_calls.pop())
        assert len(self.backward_calls) == narrow
