"""CPU checks of tests/mlp_backward_exact.py, the reference and the case list of tests/test_gpu_mlp_backward.py: the NumPy restatement
equals torch float64 autograd, every case keeps the 2**24 bound of both passes, and no case is blind to the errors it is there to catch."""
import numpy as np
import pytest

from tests import mlp_backward_exact as R
from tests import mlp_exact as X

torch = pytest.importorskip("torch")

IDS = [c.name for c in R.CASES]


def _autograd64(net, x, dy):
    import copy
    net64 = copy.deepcopy(net).double()
    xt = torch.from_numpy(np.asarray(x, np.float64)).requires_grad_(True)
    net64(xt).backward(torch.from_numpy(np.asarray(dy, np.float64)))
    lins = [m for m in net64 if isinstance(m, torch.nn.Linear)]
    return {"dw": [m.weight.grad.numpy() for m in lins], "db": [None if m.bias is None else m.bias.grad.numpy() for m in lins],
            "dx": xt.grad.numpy()}


def _same(a, b, exact):
    for key in ("dw", "db"):
        for u, v in zip(a[key], b[key]):
            assert (u is None) == (v is None)
            if u is not None:
                assert u.shape == v.shape
                assert np.array_equal(u, v) if exact else np.allclose(u, v, rtol=1e-12, atol=1e-12), key
    assert np.array_equal(a["dx"], b["dx"]) if exact else np.allclose(a["dx"], b["dx"], rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("case", R.CASES, ids=IDS)
def test_reference_equals_torch_float64_autograd_exactly_and_keeps_its_bound(case):
    b = R.build(case)      # (asserts the bound)
    worst = R.assert_exact(b.bounds, case.unit, case.dunit, case.name)
    assert worst < R.LIMIT
    _same(b.want, _autograd64(b.net, b.x, b.dy), exact=True)
    assert len(b.want["dw"]) == len(case.sizes) - 1 and b.want["dx"].shape == (case.B, case.sizes[0])


def test_reference_equals_autograd_on_real_tanh_and_relu_networks():
    g = torch.Generator().manual_seed(4)
    net = torch.nn.Sequential(torch.nn.Linear(7, 9), torch.nn.Tanh(), torch.nn.Linear(9, 5, bias=False), torch.nn.ReLU(), torch.nn.Linear(5, 3), torch.nn.Tanh())
    x, dy = torch.randn(21, 7, generator=g).numpy(), torch.randn(21, 3, generator=g).numpy()
    want, _ = R.reference_backward(X.layers_of(net), x, dy)
    _same(want, _autograd64(net, x, dy), exact=False)
    assert want["db"][1] is None


def test_the_bound_is_checked_not_assumed():
    dense = R.Case("dense", (70, 64, 64, 64, 1), ("relu", "relu", "relu", None), 49, nnz=(70, 64))
    with pytest.raises(AssertionError, match="2\\*\\*24"):
        R.build(dense)


def test_slab_rows_cover_the_batch_once():
    for B in (1, 15, 16, 17, 33, 49, 4113):
        for s in R.valid_slabs(B) + ([R.tiles_of(B)] if B > 49 else []):
            rows = R.slab_rows(B, s)
            assert rows[0][0] == 0 and rows[-1][1] == B and all(a[1] == b[0] for a, b in zip(rows, rows[1:]))
            assert all(hi > lo for lo, hi in rows) and len(rows) == (s or min(R.tiles_of(B), R.MAX_SLABS))
    assert R.slab_rows(49, 2) == [(0, 32), (32, 49)] and R.slab_rows(33, 3) == [(0, 16), (16, 32), (32, 33)]


def _differs(a, b):
    return any((u is not None) and not np.array_equal(u, v) for key in ("dw", "db") for u, v in zip(a[key], b[key])) or not np.array_equal(a["dx"], b["dx"])


@pytest.mark.parametrize("case", R.CASES, ids=IDS)
def test_no_case_is_blind(case):
    b = R.build(case)
    hs = R.forward_all(b.layers, b.x)
    for l, (W, _, act) in enumerate(b.layers):
        assert np.count_nonzero(b.want["dw"][l]) > 0, f"dW of layer {l} is all zero"
        if act == "relu" and l < len(b.layers) - 1:
            z_open = hs[l + 1] > 0
            assert z_open.any() and ((~z_open).any() or z_open.size == 1), f"ReLU layer {l} is all open or all closed"
    # the activation derivative dropped (a network whose only ReLU is one open unit on one row has none to drop)
    if any(act == "relu" and (hs[l + 1] <= 0).any() for l, (_, _, act) in enumerate(b.layers)):
        assert _differs(b.want, R.reference_backward(b.layers, b.x, b.dy, keep_derivative=False)[0]), "blind to a dropped derivative"
    # W read with swapped strides in dH = dZ W: visible wherever that product is formed from a matrix with two real dimensions
    used = [l for l, (W, _, _) in enumerate(b.layers) if min(W.shape) > 1 and (l > 0 or case.dx)]
    if used:
        assert _differs(b.want, R.reference_backward(b.layers, b.x, b.dy, transposed=True)[0]), "blind to a transposed W"
    # the last row tile dropped, the last slab dropped
    for what, first in (("tile", R.ROWS * (R.tiles_of(case.B) - 1)), ("slab", R.slab_rows(case.B, case.slabs)[-1][0])):
        short = R.reference_backward(b.layers, b.x[:first], b.dy[:first])[0]
        assert any(not np.array_equal(u, v) for u, v in zip(b.want["dw"], short["dw"])), f"blind to a dropped last {what}"


def test_the_case_list_covers_the_space_the_issue_names():
    cs = R.CASES
    assert {c.B for c in cs} == set(R.BATCHES) and {c.slabs for c in cs} == {0, 1, 2, 3}
    assert set(R.IN_DIMS) <= {c.sizes[0] for c in cs}
    assert set(R.WIDTHS) <= {w for c in cs for w in c.sizes[1:-1]} and set(R.WIDTHS) <= {c.sizes[-1] for c in cs}
    assert {len(c.sizes) - 1 for c in cs} == {1, 2, 3, 4}
    for flag in ("bias", "gaps", "x_f64", "eps", "dx"):
        assert {getattr(c, flag) for c in cs} == {False, True}, flag
    assert all(not (c.dx and c.x_f64) for c in cs) and all(c.slabs <= R.tiles_of(c.B) for c in cs)
    assert any(c.B == 49 and c.slabs == 2 for c in cs) and any(c.B == 33 and c.slabs == 3 for c in cs)
    transposable = [c for c in cs if any(min(a, b) > 1 for l, (a, b) in enumerate(zip(c.sizes, c.sizes[1:])) if l > 0 or c.dx)]
    assert len(transposable) >= len(cs) * 3 // 4
