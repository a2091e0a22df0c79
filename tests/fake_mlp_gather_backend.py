"""CPU double of ``HipBackend.mlp_forward_gather`` / ``mlp_backward_gather`` (rows by index): materialise ``x[index]`` (and
``x2[index]`` with ``x2_indexed``), then call tests/fake_mlp_cat_backend.py's ``FakeCatMlpBackend`` on the rows.  Every call is
recorded, with the identity of the tensors it was handed, so that a test sees that the storage itself arrived and not a copy of its
rows.  Plain helper module."""
from __future__ import annotations

from tests.fake_mlp_cat_backend import FakeCatMlpBackend


class FakeGatherMlpBackend(FakeCatMlpBackend):
    def __init__(self):
        super().__init__()
        self.gather_forward_calls, self.gather_calls = [], []

    @staticmethod
    def _rows(x, x2, index, x2_indexed):
        import torch
        M = x.shape[0]
        assert index.dtype == torch.int64 and index.dim() == 1 and index.is_contiguous() and M >= 1
        assert bool(((index >= 0) & (index < M)).all()), "the double takes indices inside the storage only"
        assert not x2_indexed or (x2 is not None and x2.shape[0] == M)
        return x.detach()[index], (None if x2 is None else (x2.detach()[index] if x2_indexed else x2.detach()))

    def mlp_forward_gather(self, net, x, x2, index, y, B, x2_indexed=False):
        assert index.shape[0] == B == y.shape[0] and (x2 is None or x2_indexed or x2.shape[0] == B)
        self.gather_forward_calls.append({"x": x, "x2": x2, "index": index, "x2_indexed": bool(x2_indexed), "B": int(B)})
        rows, tail = self._rows(x, x2, index, x2_indexed)
        before = self.forward_calls, self.cat_forward_calls
        if tail is None:
            self.mlp_forward(net, rows, y, B)
        else:
            self.mlp_forward_cat(net, rows, tail, y, B)
        self.forward_calls, self.cat_forward_calls = before

    def mlp_backward_gather(self, net, x, x2, index, dy, weights, dw=None, db=None, dx2=None, params=True, slabs=0, wide=False,
                            x2_indexed=False):
        assert dx2 is None or not x2_indexed, "dx2 only with a dense tail"
        assert index.shape[0] == dy.shape[0]
        self.gather_calls.append({"x": x, "x2": x2, "index": index, "x2_indexed": bool(x2_indexed), "params": bool(params),
                                  "dw": dw is not None and any(t is not None for t in dw), "dx2": dx2 is not None, "wide": bool(wide),
                                  "B": int(index.shape[0])})
        rows, tail = self._rows(x, x2, index, x2_indexed)
        n = len(self.cat_calls)
        self.mlp_backward_cat(net, rows, tail, dy, weights, dw, db, None, dx2, params=params, slabs=slabs, wide=wide)
        del self.cat_calls[n:]
