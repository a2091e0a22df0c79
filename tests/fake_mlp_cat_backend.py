"""CPU double of ``HipBackend.mlp_forward_cat`` / ``mlp_backward_cat`` (the ``critic(obs, action)`` call form): concatenate the two
parts, then call the existing pass of tests/fake_mlp_backward_wide_backend.py's ``FakeWideMlpBackend`` and cut its ``dx`` at column D.
Every call is recorded, so that a test sees how many backward calls were made and what each was asked for.  Plain helper module."""
from __future__ import annotations

from tests.fake_mlp_backward_wide_backend import FakeWideMlpBackend


class FakeCatMlpBackend(FakeWideMlpBackend):
    def __init__(self):
        super().__init__()
        self.cat_forward_calls, self.cat_calls = 0, []

    def mlp_forward_cat(self, net, x, x2, y, B):
        import torch
        assert x2.dtype == torch.float32 and 1 <= x2.shape[1] <= 8 and x.shape[1] + x2.shape[1] == net.layer[0].in_dim
        self.cat_forward_calls += 1
        before = self.forward_calls
        self.mlp_forward(net, torch.cat([x.detach().to(torch.float32), x2.detach()], 1), y, B)
        self.forward_calls = before

    def mlp_backward_cat(self, net, x, x2, dy, weights, dw=None, db=None, dx=None, dx2=None, params=True, slabs=0, wide=False):
        import torch
        nl = net.n_layers
        n2 = 0 if x2 is None else int(x2.shape[1])
        D = int(net.layer[0].in_dim) - n2
        assert 0 <= n2 <= 8 and x.shape[1] == D and (dx2 is None or n2)
        dw_none = dw is None or all(t is None for t in dw)
        db_none = db is None or all(t is None for t in db)
        if not params:
            assert dw_none and db_none, "params=False takes no dw and no db"
            assert dx is not None or dx2 is not None, "params=False needs dx or dx2"
        self.cat_calls.append({"params": bool(params), "dw": not dw_none, "db": not db_none, "dx": dx is not None, "dx2": dx2 is not None,
                               "n2": n2, "wide": bool(wide), "B": int(x.shape[0])})
        rows = x.detach().to(torch.float32) if x2 is None else torch.cat([x.detach().to(torch.float32), x2.detach()], 1)
        full_dw = dw if params else [torch.empty_like(w) for w in weights]
        full_db = db if params else [None if not net.layer[l].b else torch.empty(net.layer[l].out_dim) for l in range(nl)]
        full_dx = torch.empty_like(rows) if (dx is not None or dx2 is not None) else None
        narrow, wides = len(self.backward_calls), len(self.wide_calls)
        (self.mlp_backward_wide if wide else self.mlp_backward)(net, rows, dy, weights, full_dw, full_db, full_dx, slabs)
        del self.backward_calls[narrow:], self.wide_calls[wides:]
        if dx is not None:
            dx.copy_(full_dx[:, :D])
        if dx2 is not None:
            dx2.copy_(full_dx[:, D:])
