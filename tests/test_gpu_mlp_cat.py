"""The critic(obs, action) entry points on the device (include/pdegym.h: pdegym_mlp_forward_cat, pdegym_mlp_backward_cat,
pdegym_mlp_backward_wide_cat) and ``FusedMLP.with_grad(obs, tail, params)`` through them.

The yardstick is bit equality: with the existing entry points on the materialised ``torch.cat`` rows (the parent's code), and with the
exactly summable networks of tests/mlp_backward_exact.py / tests/mlp_backward_wide_exact.py, whose results are known without running
any kernel -- so the two paths cannot be wrong together.  No tolerance appears in this file.

Every launch of the new entry points goes through ``_new``: outputs in guarded buffers and poisoned first, every cached workspace of
the backend poisoned, the rows of x / x2 past the batch (up to the end of the last 16-row tile) holding NaN, the rows of dx / dx2 past
the batch holding the poison; afterwards the guards are checked, every output element must be written, the dead rows and the row gaps
untouched, the inputs unchanged, and with ``params == 0`` the workspaces still poisoned.  The thinned case product and its covering
condition live in tests/mlp_cat_cases.py."""
import copy
import functools
import importlib.util
import os
import sys

import numpy as np
import pytest

from tests import lds_residue as LR
from tests import mlp_backward_exact as R
from tests import mlp_backward_wide_exact as W
from tests import mlp_cat_cases as CC
from tests import poison

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the five kernels the new entry points instantiate anew, and the tests of this file that hold the new instantiations to the
# poisoned-buffer contract, to displaced pointers and to poisoned LDS (every launch goes through _new)
KERNEL_CASES = {k: ["test_two_part_rows_give_the_bits_of_the_concatenated_rows", "test_exactly_summable_networks_are_exact",
                    "test_displaced_tail_pointers", "test_poisoned_lds_changes_no_bit"]
                for k in ("mlp_forward_kernel", "mlp_backward_tiles", "mlp_backward_dw0", "mlp_backward_wide_tiles", "mlp_backward_wide_accumulate")}


def _net(sizes, act, seed):
    torch.manual_seed(seed)
    mods = []
    for i in range(len(sizes) - 1):
        mods.append(torch.nn.Linear(sizes[i], sizes[i + 1]))
        if i < len(sizes) - 2:
            mods.append(torch.nn.Tanh() if act == "tanh" else torch.nn.ReLU())
    return torch.nn.Sequential(*mods).cuda()


def _policy(net):
    from pdecontrolgym_amd.policy import FusedMLP
    return FusedMLP(net)


def _data(B, D, n2, out, seed, x_f64=False):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, D, generator=g, dtype=F64 if x_f64 else F32)
    return x.cuda(), torch.randn(B, n2, generator=g).cuda(), torch.randn(B, out, generator=g).cuda()


def _wide(pol):
    return not pol.fits_backward()


def _old(pol, x, x2, dy, slabs=0, want_dx=True):
    """The existing entry points on the materialised rows: {"y", "dw", "db", "dx" (all D + n2 columns)}."""
    bk = pol.backend
    rows = torch.cat([x, x2.to(x.dtype)], 1).contiguous()
    desc = pol._net(None, x.dtype == F64, plain=True)
    y = torch.empty(x.shape[0], dy.shape[1], device="cuda")
    bk.mlp_forward(desc, rows, y, x.shape[0])
    weights = [w.detach() for w, _, _ in pol.layers]
    dw = [torch.empty_like(w) for w in weights]
    db = [None if b is None else torch.empty_like(b.detach()) for _, b, _ in pol.layers]
    dx = torch.empty(rows.shape, device="cuda") if want_dx and x.dtype == F32 else None
    (bk.mlp_backward_wide if _wide(pol) else bk.mlp_backward)(desc, rows, dy, weights, dw, db, dx, slabs)
    return {"y": y, "dw": dw, "db": db, "dx": dx}


def _poison_workspaces(bk):
    caches = [ws for key in ("_mlp_bw_ws", "_mlp_bw_wide_ws") for ws in bk.__dict__.get(key, {}).values()]
    for ws in caches:
        ws[: ws.numel() // 4 * 4].view(torch.int32).fill_(poison.POISON_F32)
    return caches


def _new(pol, x, x2, dy, slabs=0, params=1, want_dx=True, want_dx2=True, x_gap=0, x2_gap=0, policy=None, tail_shift=None, forward=True):
    """pdegym_mlp_forward_cat and pdegym_mlp_backward(_wide)_cat under the buffer contract (module docstring).  ``policy``: the
    displacement of x, dy, y, dx, w, dw, db (tests/poison.py); ``tail_shift``: bytes by which x2 and dx2 are displaced."""
    bk = pol.backend
    B, D = x.shape
    n2, out = x2.shape[1], dy.shape[1]
    Bpad = -(-B // 16) * 16
    x_f64 = x.dtype == F64
    arena = poison.Arena("cuda", policy=policy)

    def tail_buffer(name, cols):
        g = poison.Guarded(name, (Bpad, cols), F32, "cuda", shift=arena.shift_of(name, F32) if tail_shift is None else tail_shift)
        arena.bufs[name] = g
        return poison.poison_(g.t)

    xbig = poison.poison_(arena.new("x", (Bpad, D + x_gap), x.dtype))
    x2big = tail_buffer("x2", n2 + x2_gap)
    dybig = poison.poison_(arena.new("dy", (B, out + 1), F32))
    xbig[:B, :D], x2big[:B, :n2], dybig[:, :out] = x, x2, dy
    ybig = poison.poison_(arena.new("y", (B, out + 2), F32))
    dxbig = poison.poison_(arena.new("dx", (Bpad, D + 2), F32)) if want_dx else None
    dx2big = tail_buffer("dx2", n2 + 1) if want_dx2 else None
    weights = [arena.like(f"w{l}", w.detach()) for l, (w, _, _) in enumerate(pol.layers)]
    dw = db = None
    if params:
        dw = [poison.poison_(arena.new(f"dw{l}", w.shape, F32)) for l, w in enumerate(weights)]
        db = [None if b is None else poison.poison_(arena.new(f"db{l}", b.shape, F32)) for l, (_, b, _) in enumerate(pol.layers)]
    desc = pol._net(None, x_f64, plain=True)
    inputs = [xbig, x2big, dybig] + weights + list(pol._wt) + [b.detach() for _, b, _ in pol.layers if b is not None]
    before = [t.clone() for t in inputs]
    xv, x2v, dyv = xbig[:B, :D], x2big[:B, :n2], dybig[:, :out]
    if forward:
        bk.mlp_forward_cat(desc, xv, x2v, ybig[:, :out], B)
    caches = _poison_workspaces(bk)
    bk.mlp_backward_cat(desc, xv, x2v, dyv, weights, dw, db, None if dxbig is None else dxbig[:B, :D], None if dx2big is None else dx2big[:B, :n2],
                        params=bool(params), slabs=slabs, wide=_wide(pol))
    arena.check()
    if forward:
        poison.assert_written(ybig, (slice(None), slice(0, out)), "y")
        poison.assert_untouched(ybig, (slice(None), slice(out, None)), "the gap of the y rows")
    if params:
        for name, t in [(f"dw{l}", t) for l, t in enumerate(dw)] + [(f"db{l}", t) for l, t in enumerate(db) if t is not None]:
            poison.assert_written(t, None, name)
    else:
        for ws in caches:
            poison.assert_untouched(ws[: ws.numel() // 4 * 4].view(F32), None, "a workspace, with params == 0")
    for big, cols, name in ((dxbig, D, "dx"), (dx2big, n2, "dx2")):
        if big is not None:
            poison.assert_written(big, (slice(0, B), slice(0, cols)), name)
            poison.assert_untouched(big, (slice(0, B), slice(cols, None)), f"the gap of the {name} rows")
            poison.assert_untouched(big, (slice(B, None), slice(None)), f"rows >= B of {name}")
    for t, b in zip(inputs, before):
        poison.assert_bits_equal(t, b, None, "an input")
    return {"y": ybig[:, :out].clone() if forward else None, "dw": dw, "db": db,
            "dx": None if dxbig is None else dxbig[:B, :D].clone(), "dx2": None if dx2big is None else dx2big[:B, :n2].clone()}


def _same(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype == F32, what
    bad = a.contiguous().view(torch.int32) != b.contiguous().view(torch.int32)
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {bad.numel()} elements differ in bits, the first at {tuple(int(i) for i in torch.nonzero(bad)[0])}"


def _assert_bits_of_old(new, old, D, what, params):
    if new["y"] is not None:
        _same(new["y"], old["y"], f"{what}: y")
    if params:
        for l, (p, q) in enumerate(zip(new["dw"], old["dw"])):
            _same(p, q, f"{what}: dw[{l}]")
        for l, (p, q) in enumerate(zip(new["db"], old["db"])):
            assert (p is None) == (q is None)
            if p is not None:
                _same(p, q, f"{what}: db[{l}]")
    if old["dx"] is not None:
        if new["dx"] is not None:
            _same(new["dx"], old["dx"][:, :D], f"{what}: dx")
        if new["dx2"] is not None:
            _same(new["dx2"], old["dx"][:, D:], f"{what}: dx2")


# ---- (a) the thinned product: the bits of the existing entry points ---------------------------------------------------------------------
ALL_CASES = CC.cases("narrow") + CC.cases("wide")


def test_the_thinned_product_is_covering():
    for family in ("narrow", "wide"):
        CC.assert_covering(family, CC.cases(family))


@pytest.mark.parametrize("case", ALL_CASES, ids=[c.name for c in ALL_CASES])
def test_two_part_rows_give_the_bits_of_the_concatenated_rows(case):
    """y, dw, db, dx and dx2 of the new entry points equal y, dw, db, dx[:, :D] and dx[:, D:] of pdegym_mlp_forward and
    pdegym_mlp_backward / _wide on torch.cat rows with the same slabs.  The old pass always returns the full dx from float32 rows: with
    float64 x the reference dx comes from the float32 rounding of the same rows (the kernels round as they read: the same operands)."""
    D, n2 = case.part
    pol = _policy(_net(case.sizes, case.act, case.seed))
    assert _wide(pol) == (case.family == "wide")
    x, x2, dy = _data(case.B, D, n2, case.sizes[-1], case.seed, case.x_f64)
    old = _old(pol, x, x2, dy, case.slabs)
    if case.x_f64:
        assert old["dx"] is None
        x32 = x.to(F32)
        assert torch.equal(x32.double().to(F32), x32)
        old["dx"] = _old(pol, x32, x2, dy, case.slabs)["dx"]
    new = _new(pol, x, x2, dy, case.slabs, case.params, case.dx, True, case.x_gap, case.x2_gap)
    assert (new["dx"] is not None) == case.dx and new["dx2"] is not None and (new["dw"] is not None) == bool(case.params)
    _assert_bits_of_old(new, old, D, case.name, case.params)


# ---- (b) exactly summable networks: known without running any kernel -----------------------------------------------------------------------
EXACT = [("narrow", R.Case("cat-narrow-70-64-33-2", (70, 64, 33, 2), ("relu", "relu", None), 33, 2, seed=7), 4),
         ("narrow", R.Case("cat-narrow-9-15-3", (9, 15, 3), ("relu", None), 17, 0, seed=8), 3),
         ("wide", next(c for c in W.CASES if c.name == "critic-66-256-256-16"), 8),
         ("wide", next(c for c in W.CASES if c.name.startswith("hidden129-")), 1)]


@functools.lru_cache(maxsize=None)
def _built(i):
    family, case, _ = EXACT[i]
    return (W.build if family == "wide" else R.build)(case)


@pytest.mark.parametrize("i", range(len(EXACT)), ids=[c.name + f"+{n2}" for _, c, n2 in EXACT])
def test_exactly_summable_networks_are_exact(i):
    """The float64 expectation of tests/mlp_backward_exact.py, cut at column D: forward, the three-launch pass and the one-launch pass."""
    family, case, n2 = EXACT[i]
    b = _built(i)
    D = case.sizes[0] - n2
    pol = _policy(copy.deepcopy(b.net).cuda())
    assert _wide(pol) == (family == "wide")
    rows = torch.from_numpy(b.x.astype(np.float32)).cuda()
    x, x2 = rows[:, :D].contiguous(), rows[:, D:].contiguous()
    dy = torch.from_numpy(b.dy.astype(np.float32)).cuda()
    want_y = R.forward_all(b.layers, b.x)[-1]
    for params in (1, 0):
        got = _new(pol, x, x2, dy, case.slabs, params, True, True, x_gap=1, x2_gap=1)
        np.testing.assert_array_equal(got["y"].cpu().numpy().astype(np.float64), want_y, err_msg=f"{case.name}: y")
        np.testing.assert_array_equal(got["dx"].cpu().numpy().astype(np.float64), b.want["dx"][:, :D], err_msg=f"{case.name}: dx, params={params}")
        np.testing.assert_array_equal(got["dx2"].cpu().numpy().astype(np.float64), b.want["dx"][:, D:], err_msg=f"{case.name}: dx2, params={params}")
        if params:
            for l in range(len(b.layers)):
                np.testing.assert_array_equal(got["dw"][l].cpu().numpy().astype(np.float64), b.want["dw"][l], err_msg=f"{case.name}: dw[{l}]")
                if b.want["db"][l] is not None:
                    np.testing.assert_array_equal(got["db"][l].cpu().numpy().astype(np.float64), b.want["db"][l], err_msg=f"{case.name}: db[{l}]")
    only_tail = _new(pol, x, x2, dy, 0, 0, False, True, forward=False)
    np.testing.assert_array_equal(only_tail["dx2"].cpu().numpy().astype(np.float64), b.want["dx"][:, D:], err_msg=f"{case.name}: dx2 alone")
    only_head = _new(pol, x, x2, dy, 0, 0, True, False, forward=False)
    np.testing.assert_array_equal(only_head["dx"].cpu().numpy().astype(np.float64), b.want["dx"][:, :D], err_msg=f"{case.name}: dx alone")


# ---- (c) the forward's heads -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("head", ["squashed-gaussian", "clamped-plain"])
def test_the_heads_of_the_forward_take_two_part_rows(head):
    from pdecontrolgym_amd.policy import FusedMLP
    torch.manual_seed(3)
    B, D, n2 = 37, 61, 5
    obs, tail, _ = _data(B, D, n2, 1, 5)
    if head == "squashed-gaussian":
        latent = torch.nn.Sequential(torch.nn.Linear(D + n2, 128), torch.nn.ReLU()).cuda()
        pol = FusedMLP.squashed_gaussian(latent, torch.nn.Linear(128, 3).cuda(), torch.nn.Linear(128, 3).cuda())
        clamp, noise = (-2.0, 3.0), torch.randn(B, 3, device="cuda")
    else:
        pol = FusedMLP(_net((D + n2, 64, 3), "tanh", 4), clamp=(-0.05, 0.05))
        clamp, noise = "default", 0.01 * torch.randn(B, 3, device="cuda")
    for dtype in (F32, F64):
        o = obs.to(dtype)
        want = pol.forward_into(torch.cat([o, tail.to(dtype)], 1), torch.empty(B, 3, device="cuda"), clamp=clamp, noise=noise)
        arena = poison.Arena("cuda", policy="mixed")
        out = poison.poison_(arena.new("y", (B, 3), F32))
        pol.forward_into(arena.like("x", o), out, clamp=clamp, noise=noise, tail=arena.like("x2", tail))
        arena.check()
        poison.assert_written(out, None, "y")
        _same(out, want, f"{head}, {dtype}")
        if head == "clamped-plain":      # __call__: no noise, an output of the observations' dtype (the float32 result widened)
            got = pol(o, tail)
            assert got.dtype == dtype and torch.equal(got, pol(torch.cat([o, tail.to(dtype)], 1)))


# ---- (d) displaced pointers -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,sizes", [("narrow", (70, 64, 33, 2)), ("wide", (70, 129, 2))])
@pytest.mark.parametrize("shift", [0, 4, 8, 12])
def test_displaced_tail_pointers(family, sizes, shift):
    """x2 and dx2 at every 4-byte displacement of a 16-byte window; x, dy, y, dx, w, dw, db displaced by the policies of tests/poison.py
    (as tests/test_gpu_pointer_alignment.py displaces them).  The bits are those of the aligned call on the concatenated rows."""
    pol = _policy(_net(sizes, "relu", 11))
    D, n2 = sizes[0] - 3, 3
    x, x2, dy = _data(33, D, n2, sizes[-1], 12)
    old = _old(pol, x, x2, dy, 2)
    for policy in poison.POLICIES[1:]:
        for params in (1, 0):
            new = _new(pol, x, x2, dy, 2, params, True, True, policy=policy, tail_shift=shift)
            _assert_bits_of_old(new, old, D, f"{family}, shift {shift}, policy {policy}, params {params}", params)


# ---- (e) LDS residue ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", ["nan", "huge"])
@pytest.mark.parametrize("family,sizes,n2", [("narrow", (67, 33, 17, 2), 5), ("wide", (70, 129, 65, 1), 1), ("narrow", (9, 64, 1), 8)])
def test_poisoned_lds_changes_no_bit(family, sizes, n2, pattern):
    """The same calls with every launch's LDS poisoned first, at shapes where the staging padding is live: D + n2 no multiple of 4 or of
    16, widths off the 16-unit seams, and a last tile with dead rows."""
    assert sizes[0] % 4 and sizes[0] % 16
    D = sizes[0] - n2
    x, x2, dy = _data(21, D, n2, sizes[-1], 21)
    clean_pol = _policy(_net(sizes, "tanh", 20))
    clean = [_new(clean_pol, x, x2, dy, 0, params) for params in (1, 0)]
    with LR.dirtied(pattern) as ctx:
        pol = _policy(_net(sizes, "tanh", 20))
        dirty = [_new(pol, x, x2, dy, 0, params) for params in (1, 0)]
    ctx.check("pdegym_mlp_forward_cat", "pdegym_mlp_backward_wide_cat" if family == "wide" else "pdegym_mlp_backward_cat")
    for params, a, b in zip((1, 0), dirty, clean):
        for key in ("y", "dx", "dx2"):
            _same(a[key], b[key], f"{key} under {pattern} LDS, params {params}")
        if params:
            for p, q in zip(a["dw"] + a["db"], b["dw"] + b["db"]):
                _same(p, q, f"dw / db under {pattern} LDS")


# ---- (f) non-finite data, batch invariance --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sizes", [(66, 64, 64, 1), (66, 256, 256, 1)], ids=["narrow", "wide"])
@pytest.mark.parametrize("value", [float("nan"), float("inf")])
def test_a_non_finite_tail_entry_stays_in_its_row(sizes, value):
    """A NaN (an Inf) in x2[i] reaches row i of y, dx, dx2 and the weight gradients, and no other row of y, dx or dx2."""
    pol = _policy(_net(sizes, "tanh", 30))
    D, n2, B, i = sizes[0] - 2, 2, 35, 18
    x, x2, dy = _data(B, D, n2, 1, 31)
    clean = _new(pol, x, x2, dy)
    bad = x2.clone()
    bad[i, 1] = value
    got = _new(pol, x, bad, dy)
    rows = torch.arange(B, device="cuda") != i
    for key in ("y", "dx", "dx2"):
        _same(got[key][rows], clean[key][rows], f"{key}, rows other than {i}")
    if value != value:
        for key in ("y", "dx", "dx2"):
            assert bool(torch.isnan(got[key][i]).all()), key
        assert bool(torch.isnan(got["dw"][0]).any()) and bool(torch.isnan(got["dw"][-1]).any())
    else:      # tanh saturates: a finite row, and a first-layer dW column that saw the Inf
        assert bool(torch.isfinite(got["y"][i]).all()) and not bool(torch.isfinite(got["dw"][0][:, D + 1]).all())
    one_launch = _new(pol, x, bad, dy, params=0)
    for key in ("dx", "dx2"):
        _same(one_launch[key], got[key], f"{key} of the one-launch pass")


@pytest.mark.parametrize("sizes", [(66, 64, 64, 1), (66, 256, 256, 1)], ids=["narrow", "wide"])
def test_rows_do_not_depend_on_the_batch_or_on_each_other(sizes):
    pol = _policy(_net(sizes, "relu", 40))
    D, n2 = sizes[0] - 1, 1
    x, x2, dy = _data(49, D, n2, 1, 41)
    full = _new(pol, x, x2, dy, params=0)
    for rows in (slice(0, 1), slice(16, 33), slice(31, 49)):
        part = _new(pol, x[rows].contiguous(), x2[rows].contiguous(), dy[rows].contiguous(), params=0)
        for key in ("y", "dx", "dx2"):
            _same(part[key], full[key][rows], f"{key} of rows {rows}")
    shuffled = torch.randperm(49, generator=torch.Generator().manual_seed(1)).cuda()
    mixed = _new(pol, x[shuffled].contiguous(), x2[shuffled].contiguous(), dy[shuffled].contiguous(), params=1)
    for key in ("y", "dx", "dx2"):
        _same(mixed[key], full[key][shuffled], f"{key} after a permutation of the rows")


# ---- (g) autograd and capture -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sizes", [(66, 64, 64, 1), (202, 256, 256, 1)], ids=["narrow", "wide"])
def test_with_grad_on_a_tail_gives_the_bits_of_the_full_pass(sizes):
    net = _net(sizes, "relu", 50)
    pol = _policy(net)
    D = sizes[0] - 1
    x, x2, _ = _data(300, D, 1, 1, 51)
    block = torch.cat([x, x2], 1).requires_grad_(True)
    y_old = pol.with_grad(block)
    (y_old ** 2).sum().backward()
    want = {"y": y_old.detach().clone(), "dblock": block.grad.clone(), "p": [p.grad.clone() for p in net.parameters()]}
    for p in net.parameters():
        p.grad = None
    tail = x2.clone().requires_grad_(True)
    y = pol.with_grad(x, tail, params=False)
    (g,) = torch.autograd.grad((y ** 2).sum(), tail)
    _same(y.detach(), want["y"], "y")
    _same(g, want["dblock"][:, D:], "the action gradient of the one-launch pass")
    assert all(p.grad is None for p in net.parameters())
    obs, tail = x.clone().requires_grad_(True), x2.clone().requires_grad_(True)
    (pol.with_grad(obs, tail) ** 2).sum().backward()
    _same(obs.grad, want["dblock"][:, :D], "d obs")
    _same(tail.grad, want["dblock"][:, D:], "d tail")
    for p, q in zip(net.parameters(), want["p"]):
        _same(p.grad, q, "a parameter gradient")


def test_a_captured_update_with_a_tail_replays_like_the_eager_run():
    """Forward, loss, backward and FusedAdam.step with the tail form in ONE graph, replayed twice, against two eager iterations."""
    from pde_control_gym import FusedAdam, FusedMLP
    proto = _net((66, 64, 64, 1), "relu", 60)
    data = [_data(64, 65, 1, 1, 61 + k)[:2] for k in range(2)]
    x, a = torch.empty(64, 65, device="cuda"), torch.empty(64, 1, device="cuda")
    results = []

    def iteration(f, opt):
        y = f.with_grad(x, a)
        (y * y).sum().backward()
        opt.step()

    for captured in (False, True):
        net = copy.deepcopy(proto)
        params = list(net.parameters())
        f = FusedMLP(net)
        opt = FusedAdam(params, lr=1e-3).attach(f)
        if captured:
            sd = opt.state_dict()
            x.copy_(data[0][0]), a.copy_(data[0][1])
            iteration(f, opt)                           # warm-up
            opt.load_state_dict(sd)
            net.load_state_dict(proto.state_dict())
            f.refresh()
            opt.zero_grad(set_to_none=True)
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                iteration(f, opt)
        for xk, ak in data:
            x.copy_(xk), a.copy_(ak)
            if captured:
                graph.replay()
            else:
                opt.zero_grad(set_to_none=True)
                iteration(f, opt)
        torch.cuda.synchronize()
        results.append([p.detach().clone() for p in params] + [w.clone() for w in f._wt])
    for p, q in zip(*results):
        _same(p, q, "a parameter or a weight copy after two iterations")
    assert not torch.equal(results[0][0], proto[0].weight.detach())


# ---- (h) the example ------------------------------------------------------------------------------------------------------------------------
def _example(name):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    try:
        spec = importlib.util.spec_from_file_location(name + "_fused_critic", os.path.join(ROOT, "examples", name + ".py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        sys.path.pop(0)
    return mod


@pytest.mark.parametrize("hidden", [64, 256])
def test_sac_example_with_fused_critic_prints_the_history_of_the_three_switch_path(hidden):
    """The noise is drawn by the same calls in the same order on both paths (the example's docstring), so the same seed gives the same
    numbers without a pre-drawn tensor."""
    mod = _example("train_sac_device")
    kw = dict(iterations=6, num_envs=256, n_steps=8, hidden=hidden, quiet=True, updates=2, batch=512, fused_grad=True, fused_loss=True, fused_opt=True)
    want = mod.main(**kw)
    got = mod.main(fused_critic=True, **kw)
    assert got["moved"] == {"actor": True, "q1": True, "q2": True} and want["moved"] == got["moved"]
    for k in ("q_loss", "actor_loss", "alpha", "mean_reward", "mean_norm"):
        assert len(got[k]) == 6 and np.isfinite(got[k]).all() and got[k] == want[k], (k, got[k], want[k])
    with pytest.raises(ValueError, match="fused_critic needs"):
        mod.main(iterations=1, num_envs=64, quiet=True, fused_critic=True)
