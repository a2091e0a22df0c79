"""The wide MLP backward kernels (pdegym_mlp_backward_wide, csrc/pdegym_mlp_backward_wide.hip: layers of up to 256 units) and
FusedMLP.with_grad through them, on the device.

Every launch of this file goes through ``_launch``: outputs in guarded buffers, outputs AND the workspace poisoned first, guards
checked, every output element written, inputs compared bit for bit afterwards.  Exactly summable cases
(tests/mlp_backward_wide_exact.py, checked on the CPU by tests/test_mlp_backward_wide.py: exact, and no 16 x 16 tile of a dW left
empty) are compared with ``assert_array_equal`` against the float64 expectation for every slab count the batch allows and under every
displacement policy of tests/poison.py; networks both entry points take give the bits of pdegym_mlp_backward; one-hot probes pin the
weight addressings of a first and of a hidden layer with full-mantissa weights; real 256-256 networks are held to torch's own
float32 error against float64 autograd (the tolerance factor M below); non-finite rows; with_grad; both examples at 256 units."""
import copy
import functools

import numpy as np
import pytest

from tests import mlp_backward_exact as R
from tests import mlp_backward_wide_exact as W
from tests import mlp_exact as mx
from tests import poison

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64

# every kernel of csrc/pdegym_mlp_backward_wide.hip and the tests that hold it to the poisoned-buffer contract (every launch of this
# file goes through _launch); tests/test_mlp_backward_wide.py checks the table against the source
KERNEL_CASES = {k: ["test_wide_backward_kernels_are_exact", "test_differently_poisoned_workspaces_give_equal_bits"]
                for k in ("mlp_backward_wide_tiles", "mlp_backward_wide_accumulate", "mlp_backward_wide_reduce")}

# e_kernel <= M * e_torch + 2**-20 (errors against float64 autograd, relative to the largest entry of each gradient tensor): the rule
# and the floor of tests/test_gpu_mlp_backward.py.  M: the worst e_kernel / e_torch of the first measured run
# over the tensors whose e_torch is at least 2**-24 is 1.95 (db2 of 66-256-256-1 ReLU at B = 4113: 2.08e-7 against 1.07e-7; torch
# sums a bias gradient as a tree, the kernel as a chain per slab), doubled and rounded up to a power of two.  27 of the 28 pairs
# enter; the single-element db2 of the same network at B = 17 has e_torch 2.2e-8 < 2**-24 and e_kernel equal to it.  On the weight
# gradients at B = 4113 the kernel is 1.5 - 8 times closer to float64 than torch (all pairs in
# profiles/r15_mlp_backward_wide.json).
M = 4.0
FLOOR = 2.0 ** -20


def _launch(net, x_np, dy_np, x_f64=False, gaps=False, want_dx=True, slabs=0, ws_fill=None, policy=None):
    """One pdegym_mlp_backward_wide call under the buffer contract.  ``net``: a Linear / Tanh / ReLU stack on the device.  Returns
    {"dw": [...], "db": [...], "dx"} as NumPy arrays.  ``policy``: the displacement of x, dy, dx, the row-major w[], dw and db off their
    256-byte boundaries; the blocked weights and biases of the descriptor and the workspace are the library's own tensors."""
    import ctypes as C

    from pdecontrolgym_amd.policy import FusedMLP
    pol = FusedMLP(net)
    bk = pol.backend
    B, K = x_np.shape
    out = dy_np.shape[1]
    gx, gy, gd = (5, 3, 2) if gaps else (0, 0, 0)
    arena = poison.Arena("cuda", policy=policy)
    xbig = poison.poison_(arena.new("x", (B, K + gx), F64 if x_f64 else F32))
    dybig = poison.poison_(arena.new("dy", (B, out + gy), F32))
    xbig[:, :K] = torch.from_numpy(x_np)
    dybig[:, :out] = torch.from_numpy(np.asarray(dy_np, np.float32))
    dxbig = poison.poison_(arena.new("dx", (B, K + gd), F32)) if want_dx else None
    weights = [arena.like(f"w{l}", w.detach()) for l, (w, _, _) in enumerate(pol.layers)]      # the row-major w[] of the call
    dw = [poison.poison_(arena.new(f"dw{l}", w.shape, F32)) for l, w in enumerate(weights)]
    db = [None if b is None else poison.poison_(arena.new(f"db{l}", b.shape, F32)) for l, (_, b, _) in enumerate(pol.layers)]
    desc = pol._net(None, x_f64, plain=True)
    need = int(bk.lib.pdegym_mlp_backward_wide_workspace(C.byref(desc), B, slabs))
    assert need == W.workspace_bytes([K] + [int(w.shape[0]) for w in weights], B, slabs)
    ws = bk._mlp_backward_wide_workspace(torch.device("cuda", torch.cuda.current_device()), need)
    if ws_fill is None:
        ws.view(torch.int32).fill_(poison.POISON_F32)
    else:
        ws.fill_(ws_fill)
    inputs = [xbig, dybig] + weights + list(pol._wt) + [b.detach() for _, b, _ in pol.layers if b is not None]
    before = [t.clone() for t in inputs]
    x, dy = xbig[:, :K], dybig[:, :out]
    bk.mlp_backward_wide(desc, x, dy, weights, dw, db, None if dxbig is None else dxbig[:, :K], slabs)
    arena.check()
    for name, t in [(f"dw{l}", t) for l, t in enumerate(dw)] + [(f"db{l}", t) for l, t in enumerate(db) if t is not None]:
        poison.assert_written(t, None, name)
    if dxbig is not None:
        poison.assert_written(dxbig, (slice(None), slice(0, K)), "dx")
        if gaps:
            poison.assert_untouched(dxbig, (slice(None), slice(K, None)), "the gap of the dx rows")
    for t, b in zip(inputs, before):
        poison.assert_bits_equal(t, b, None, "an input")
    return {"dw": [t.cpu().numpy() for t in dw], "db": [None if t is None else t.cpu().numpy() for t in db],
            "dx": None if dxbig is None else dxbig[:, :K].cpu().numpy()}


def _assert_equal(case_name, got, want, what):
    for key in ("dw", "db"):
        for l, (g, w) in enumerate(zip(got[key], want[key])):
            assert (g is None) == (w is None), (case_name, key, l)
            if g is not None:
                np.testing.assert_array_equal(np.asarray(g, np.float64), np.asarray(w, np.float64), err_msg=f"{case_name}: {key}[{l}] {what}")
    if got["dx"] is not None:
        np.testing.assert_array_equal(np.asarray(got["dx"], np.float64), np.asarray(want["dx"], np.float64), err_msg=f"{case_name}: dx {what}")


def _assert_same_bits(a, b, what):
    for key in ("dw", "db"):
        for l, (p, q) in enumerate(zip(a[key], b[key])):
            assert (p is None) == (q is None), (what, key, l)
            if p is not None:
                np.testing.assert_array_equal(p.view(np.int32), q.view(np.int32), err_msg=f"{what}: {key}[{l}]")
    assert (a["dx"] is None) == (b["dx"] is None)
    if a["dx"] is not None:
        np.testing.assert_array_equal(a["dx"].view(np.int32), b["dx"].view(np.int32), err_msg=f"{what}: dx")


@functools.lru_cache(maxsize=None)
def _built(name):
    return W.build(next(c for c in W.CASES if c.name == name))


# ---- (a) exactly summable cases ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("policy", poison.POLICIES, ids=["aligned", "one", "mixed"])
@pytest.mark.parametrize("case", W.CASES, ids=[c.name for c in W.CASES])
def test_wide_backward_kernels_are_exact(case, policy):
    """dw, db, dx equal the float64 expectation exactly, for the case's slab count and for every other one of {0, 1, 2, 3} the batch
    allows: the order of summation cannot matter on these inputs, so all of them are bit-equal too."""
    b = _built(case.name)
    net = copy.deepcopy(b.net).cuda()
    for slabs in [case.slabs] + [s for s in R.valid_slabs(case.B) if s != case.slabs]:
        got = _launch(net, b.x_dev, b.dy, case.x_f64, case.gaps, case.dx, slabs, policy=policy)
        assert (got["dx"] is not None) == case.dx
        _assert_equal(case.name, got, b.want, f"(slabs = {slabs}, policy = {policy})")


# ---- (b) the bits of pdegym_mlp_backward on the networks both entry points take ----------------------------------------------------------
def _real_net(sizes, act, seed):
    torch.manual_seed(seed)
    mods = []
    for i in range(len(sizes) - 1):
        mods.append(torch.nn.Linear(sizes[i], sizes[i + 1]))
        if i < len(sizes) - 2:
            mods.append(torch.nn.Tanh() if act == "tanh" else torch.nn.ReLU())
    return torch.nn.Sequential(*mods)


@pytest.mark.parametrize("sizes,act", W.BOTH_ENTRIES, ids=["-".join(map(str, s)) + "-" + a for s, a in W.BOTH_ENTRIES])
def test_both_entry_points_return_identical_bits(sizes, act):
    from tests import test_gpu_mlp_backward as MB
    net = _real_net(sizes, act, seed=sizes[0]).cuda()
    for B, slab_counts in ((49, (1, 2, 3, 4)), (100, (1, 2, 3))):
        g = torch.Generator().manual_seed(B)
        x, dy = torch.randn(B, sizes[0], generator=g).numpy(), torch.randn(B, sizes[-1], generator=g).numpy()
        for slabs in slab_counts:
            narrow = MB._launch(net, x, dy, slabs=slabs)
            wide = _launch(net, x, dy, slabs=slabs)
            _assert_same_bits(wide, narrow, f"{sizes} B = {B} slabs = {slabs}")
        if B == 49:      # the narrow entry's own choice at 4 tiles is 4 slabs
            _assert_same_bits(_launch(net, x, dy, slabs=4), MB._launch(net, x, dy, slabs=0), f"{sizes} B = 49, the narrow entry's slabs = 0")


# ---- (c) one-hot probes with real weights ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,H", W.ONE_HOT_CASES, ids=[f"K{K}-H{H}" for K, H in W.ONE_HOT_CASES])
def test_one_hot_rows_pin_both_weight_addressings(K, H):
    """x = e_k(i) rows with real dy: dw[:, k(i)] == dy[i, :] exactly, every other column zero (the dW addressing, full mantissas).
    dy = e_o(i) rows: dx[i, :] == W[o(i), :] exactly, all columns -- the seams of the 16-column tiles and 64-column blocks among them."""
    lin = mx.real_linear(K, H, seed=2000 * K + H, bias=(K + H) % 3 != 0)
    Wm = lin.weight.detach().numpy().copy()
    net = torch.nn.Sequential(lin).cuda()
    ks = np.array(R.seam_ks(K))
    g = torch.Generator().manual_seed(K + H)
    dy = (torch.randn(len(ks), H, generator=g) * 0.7 + 0.01).numpy()
    got = _launch(net, mx.one_hot_rows(K, ks), dy, want_dx=False)
    want = np.zeros((H, K), np.float32)
    want[:, ks] = dy.T
    np.testing.assert_array_equal(got["dw"][0], want)
    if got["db"][0] is not None:
        np.testing.assert_allclose(got["db"][0], dy.astype(np.float64).sum(axis=0), rtol=1e-5, atol=1e-6)
    os_ = np.arange(H)
    x = torch.randn(H, K, generator=g).numpy()
    got = _launch(net, x, mx.one_hot_rows(H, os_), want_dx=True)
    np.testing.assert_array_equal(got["dx"], Wm[os_, :])


@pytest.mark.parametrize("K,H", W.HIDDEN_ONE_HOT_CASES, ids=[f"K{K}-K{K}-H{H}" for K, H in W.HIDDEN_ONE_HOT_CASES])
def test_one_hot_rows_through_a_hidden_layer(K, H):
    """K - K - H with identity activations and W_0 = I: H_0 is the one-hot input, so dw[1][:, k(i)] == dy[i, :] exactly (dZ_1 and H_0
    make the round trip through the workspace) and, for one-hot dy, dx[i, :] == W_1[o(i), :] exactly (the 16-block dH chain of layer
    1, then one exact term per column through the identity)."""
    first = torch.nn.Linear(K, K, bias=False)
    with torch.no_grad():
        first.weight.copy_(torch.eye(K))
    lin = mx.real_linear(K, H, seed=3000 * K + H, bias=(K + H) % 2 == 0)
    W1 = lin.weight.detach().numpy().copy()
    net = torch.nn.Sequential(first, lin).cuda()
    ks = np.array(R.seam_ks(K))
    g = torch.Generator().manual_seed(7 * K + H)
    dy = (torch.randn(len(ks), H, generator=g) * 0.7 + 0.01).numpy()
    got = _launch(net, mx.one_hot_rows(K, ks), dy, want_dx=False, slabs=1)
    want = np.zeros((H, K), np.float32)
    want[:, ks] = dy.T
    np.testing.assert_array_equal(got["dw"][1], want)
    os_ = np.arange(H)
    x = torch.randn(H, K, generator=g).numpy()
    for slabs in (0, 2):
        got = _launch(net, x, mx.one_hot_rows(H, os_), want_dx=True, slabs=slabs)
        np.testing.assert_array_equal(got["dx"], W1[os_, :])


# ---- (d) the workspace holds nothing the result depends on ------------------------------------------------------------------------------
def test_differently_poisoned_workspaces_give_equal_bits():
    net = _real_net((70, 256, 129, 2), "tanh", seed=3).cuda()
    g = torch.Generator().manual_seed(5)
    x, dy = torch.randn(49, 70, generator=g).numpy(), torch.randn(49, 2, generator=g).numpy()
    runs = [_launch(net, x, dy, slabs=s, ws_fill=f) for s in (0, 2) for f in (None, 0x00, 0xC3)]
    for s0 in (0, 3):
        for other in runs[s0 + 1:s0 + 3]:
            _assert_same_bits(runs[s0], other, "another workspace fill")


# ---- (e) non-finite rows -----------------------------------------------------------------------------------------------------------------
def test_non_finite_rows_propagate_as_ieee_makes_them_and_stay_in_their_rows():
    case = R.Case("nonfinite", (70, 256, 3), ("relu", None), 33, 2, seed=900)
    b = R.build(case)
    net = b.net.cuda()
    clean = _launch(net, b.x_dev, b.dy, slabs=2)
    x, dy = b.x_dev.copy(), b.dy.copy()
    x[5, 3], x[5, 10] = np.nan, np.inf
    dy[20, 0], dy[20, 2] = np.nan, -np.inf
    want, _ = R.reference_backward(b.layers, x, dy)
    got = _launch(net, x, dy, slabs=2)
    for key in ("dw", "db"):
        for l, (g, w) in enumerate(zip(got[key], want[key])):
            np.testing.assert_array_equal(np.isnan(g), np.isnan(w), err_msg=f"{key}[{l}]: NaNs in other places")
            np.testing.assert_array_equal(np.asarray(g, np.float64), w, err_msg=f"{key}[{l}]")      # (equal NaNs compare equal here)
    np.testing.assert_array_equal(np.asarray(got["dx"], np.float64), want["dx"])
    # (a NaN activation of a ReLU layer passes the gradient: the NaN of row 5 reaches the weight gradients, not dx[5]; dy's reaches dx[20])
    assert np.isnan(got["dx"][20]).any() and np.isnan(got["dw"][0]).any() and np.isnan(got["dw"][0][:, 3]).all()
    others = [i for i in range(case.B) if i not in (5, 20)]
    assert np.array_equal(got["dx"][others].view(np.int32), clean["dx"][others].view(np.int32))


# ---- (f) real 256-256 networks against float64 autograd, with torch float32 autograd as the yardstick ----------------------------------
def _grads_of(net, x, dy):
    net.zero_grad(set_to_none=True)
    xr = x.clone().requires_grad_(True)
    net(xr).backward(dy)
    return [p.grad.detach().double().cpu().numpy() for p in net.parameters()] + [xr.grad.double().cpu().numpy()]


@functools.lru_cache(maxsize=None)
def real_case_errors(sizes, act, B):
    """[(name, e_kernel, e_torch)] per gradient tensor: max |g - g64| / max |g64| against float64 autograd on the CPU."""
    net = _real_net(sizes, act, seed=sizes[0] + B)
    g = torch.Generator().manual_seed(B)
    x, dy = torch.randn(B, sizes[0], generator=g), torch.randn(B, sizes[-1], generator=g)
    g64 = _grads_of(copy.deepcopy(net).double(), x.double(), dy.double())
    dev = copy.deepcopy(net).cuda()
    g32 = _grads_of(dev, x.cuda(), dy.cuda())
    got = _launch(dev, x.numpy(), dy.numpy())
    mine = [t for l in range(len(got["dw"])) for t in (got["dw"][l], got["db"][l])] + [got["dx"]]
    names = [f"{k}{l}" for l in range(len(got["dw"])) for k in ("dw", "db")] + ["dx"]
    out = []
    for name, k, t, ref in zip(names, mine, g32, g64):
        scale = np.abs(ref).max()
        out.append((name, float(np.abs(k.astype(np.float64) - ref).max() / scale), float(np.abs(t - ref).max() / scale)))
    return out


@pytest.mark.parametrize("sizes,act,B", W.REAL_CASES, ids=[f"{'-'.join(map(str, s))}-{a}-B{B}" for s, a, B in W.REAL_CASES])
def test_real_networks_are_as_close_to_float64_as_torch_is(sizes, act, B):
    rows = real_case_errors(sizes, act, B)
    for name, e_k, e_t in rows:
        print(f"{'-'.join(map(str, sizes))} {act} B={B} {name}: e_kernel {e_k:.3e} e_torch {e_t:.3e} ratio {e_k / max(e_t, 1e-300):.2f}")
    for name, e_k, e_t in rows:
        assert e_k <= M * e_t + FLOOR, (name, e_k, e_t)


# ---- (g) with_grad on the device -------------------------------------------------------------------------------------------------------------
def test_with_grad_fills_the_modules_grads_with_the_raw_launchs_bits():
    from pdecontrolgym_amd.policy import FusedMLP
    net = _real_net((66, 256, 256, 1), "relu", seed=7).cuda()
    g = torch.Generator().manual_seed(8)
    x, dy = torch.randn(100, 66, generator=g), torch.randn(100, 1, generator=g)
    raw = _launch(net, x.numpy(), dy.numpy())
    pol = FusedMLP(net)
    assert not pol.fits_backward() and pol.fits_backward_wide()
    obs = x.cuda().requires_grad_(True)
    y = pol.with_grad(obs)
    assert y.grad_fn is not None and torch.equal(y.detach(), pol(x.cuda()))
    y.backward(dy.cuda())
    lins = [m for m in net if isinstance(m, torch.nn.Linear)]
    for l, m in enumerate(lins):
        assert np.array_equal(m.weight.grad.cpu().numpy().view(np.int32), raw["dw"][l].view(np.int32))
        assert np.array_equal(m.bias.grad.cpu().numpy().view(np.int32), raw["db"][l].view(np.int32))
    assert np.array_equal(obs.grad.cpu().numpy().view(np.int32), raw["dx"].view(np.int32))
    # against torch autograd of the module itself
    ref = [p.grad.clone() for p in net.parameters()]
    net.zero_grad(set_to_none=True)
    net(x.cuda()).backward(dy.cuda())
    for p, r in zip(net.parameters(), ref):
        assert torch.allclose(p.grad, r, rtol=1e-4, atol=1e-5)


def test_gaussian_routing_and_capture_refusal_on_the_device():
    from pdecontrolgym_amd.policy import FusedMLP
    torch.manual_seed(2)
    latent = [torch.nn.Linear(65, 256).cuda(), torch.nn.ReLU(), torch.nn.Linear(256, 256).cuda(), torch.nn.ReLU()]
    mu, log_std = torch.nn.Linear(256, 2).cuda(), torch.nn.Linear(256, 2).cuda()
    pol = FusedMLP.squashed_gaussian(latent, mu, log_std)
    assert not pol.fits_backward() and pol.fits_backward_wide()
    obs = torch.randn(50, 65, device="cuda")
    raw = pol.with_grad(obs)
    h = torch.nn.Sequential(*latent)(obs)
    want = torch.cat([mu(h), log_std(h)], 1)
    assert raw.shape == (50, 4) and torch.allclose(raw, want, rtol=1e-4, atol=1e-5)
    w8 = torch.randn(50, 4, device="cuda")
    (raw * w8).sum().backward()
    modules = (latent[0], latent[2], mu, log_std)
    mine = [p.grad.clone() for m in modules for p in m.parameters()]
    # the .grad of every Parameter holds the raw launch's bits: the fused last layer is [mu; log_std], its rows go to the two heads
    fused = torch.nn.Sequential(latent[0], torch.nn.ReLU(), latent[2], torch.nn.ReLU(), torch.nn.Linear(256, 4).cuda())
    with torch.no_grad():
        fused[4].weight.copy_(torch.cat([mu.weight, log_std.weight], 0))
        fused[4].bias.copy_(torch.cat([mu.bias, log_std.bias], 0))
    launch = _launch(fused, obs.cpu().numpy(), w8.cpu().numpy(), want_dx=False)
    bits = [launch["dw"][0], launch["db"][0], launch["dw"][1], launch["db"][1], launch["dw"][2][:2], launch["db"][2][:2],
            launch["dw"][2][2:], launch["db"][2][2:]]
    for a, b in zip(mine, bits):
        assert np.array_equal(a.cpu().numpy().view(np.int32), np.ascontiguousarray(b).view(np.int32))
    for m in modules:
        m.zero_grad(set_to_none=True)
    (want * w8).sum().backward()
    for a, m in zip(mine, [p for m in modules for p in m.parameters()]):
        assert torch.allclose(a, m.grad, rtol=1e-4, atol=1e-5)
    torch.cuda.synchronize()
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    keep = torch.zeros(4, device="cuda")
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            keep.add_(1.0)
            with pytest.raises(RuntimeError, match="stream capture"):
                pol.with_grad(obs)


# ---- (h) both examples with 256-unit layers -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused_loss", [False, True], ids=["torch-loss", "fused-loss"])
def test_sac_example_trains_its_256_unit_networks_with_fused_grad(fused_loss):
    from tests.test_gpu_mlp_backward import _example
    hist = _example("train_sac_device").main(iterations=2, num_envs=64, n_steps=8, hidden=256, quiet=True, fused_grad=True,
                                             fused_loss=fused_loss)
    for k in ("q_loss", "actor_loss", "alpha", "mean_reward"):
        assert len(hist[k]) == 2 and np.isfinite(hist[k]).all(), k
    assert hist["moved"] == {"actor": True, "q1": True, "q2": True}


def test_ppo_example_runs_256_unit_networks_with_fused_grad():
    from tests.test_gpu_mlp_backward import _example
    hist = _example("train_ppo_device").main(iterations=2, B=256, quiet=True, hidden=256, fused_grad=True)
    assert len(hist) == 2 and all(np.isfinite(list(h.values())).all() for h in hist)
