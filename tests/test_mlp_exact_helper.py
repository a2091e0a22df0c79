"""CPU tests of tests/mlp_exact.py, the exactly-summable-network / one-hot helper of tests/test_gpu_mlp_exact.py: the premise (float32
sums of these networks do not depend on the order), the bound of every case the GPU file runs, that no case is blind to the errors it
is there to catch, and the host-side blocked transpose of ``FusedMLP`` (through the CPU double of the kernel)."""
import dataclasses

import numpy as np
import pytest
import torch

from tests import mlp_exact as mx

ALL_CASES = mx.FORWARD_CASES + mx.ROLLOUT_CASES
IDS = [c.name for c in ALL_CASES]


def test_case_lists_cover_what_the_gpu_file_promises():
    assert len(set(IDS)) == len(IDS)
    plain = {c.sizes[0] for c in mx.FORWARD_CASES if c.sizes[1:] == (64, 1) and not (c.x_f64 or c.y_f64 or c.gaps or c.noise or not c.bias)}
    assert plain == set(mx.FORWARD_K)
    hidden = {w for c in mx.FORWARD_CASES for w in c.sizes[1:-1]}
    last = {c.sizes[-1] for c in mx.FORWARD_CASES}
    assert set(mx.WIDTHS) <= hidden and set(mx.WIDTHS) <= last
    assert {c.B for c in mx.FORWARD_CASES} >= set(mx.BATCHES)
    assert any(len(c.sizes) == 5 for c in mx.FORWARD_CASES)
    for f in ("x_f64", "y_f64", "gaps", "noise", "clamp", "eps"):
        assert any(getattr(c, f) for c in mx.FORWARD_CASES) and any(not getattr(c, f) for c in mx.FORWARD_CASES), f
    assert {(c.x_f64, c.y_f64) for c in mx.FORWARD_CASES} == {(a, b) for a in (False, True) for b in (False, True)}
    assert any(not c.bias for c in mx.FORWARD_CASES)
    # every pair of variant factors occurs in every combination (the orthogonal array behind _variant)
    fac = ("x_f64", "y_f64", "gaps", "bias", "noise")
    for i, f in enumerate(fac):
        for g in fac[i + 1:]:
            assert {(getattr(c, f), getattr(c, g)) for c in mx.FORWARD_CASES} == {(a, b) for a in (False, True) for b in (False, True)}, (f, g)
    narrow = [c for c in mx.ROLLOUT_CASES if max(c.sizes[1:]) <= 64]
    wide = [c for c in mx.ROLLOUT_CASES if max(c.sizes[1:]) > 64]
    assert {w for c in narrow for w in c.sizes[1:-1]} >= {1, 3, 4, 5, 16, 33, 63, 64}
    assert {w for c in wide for w in c.sizes[1:-1]} >= {65, 127, 128, 129, 255, 256}
    assert {c.env[4] for c in narrow if c.env[0] == "1d" and c.env[3] == "full"} >= {30, 65, 100, 257, 512, 513}
    assert {c.env[0] for c in narrow} == {c.env[0] for c in wide} == {"1d", "traffic", "tumor"}
    assert any(c.B % 16 for c in wide) and any(c.sizes[-1] == 2 for c in wide)
    # a first layer with K % 4 != 0 and an even group count: stage() appends the padding group
    assert any(c.sizes[0] % 4 and ((c.sizes[0] + 3) // 4) % 2 == 0 for c in narrow)


def test_lds_limit_case_sits_just_under_160_kb():
    from pdecontrolgym_amd.policy import FusedMLP
    (case,) = [c for c in mx.ROLLOUT_CASES if c.name == "rd513-lds-limit"]
    n, H = case.sizes[0], case.sizes[1]
    fits = FusedMLP(mx.exact_net((n, H, 1), ("relu", None), 0), backend=object())
    over = FusedMLP(mx.exact_net((n, H + 1, 1), ("relu", None), 0), backend=object())
    assert fits.rollout_lds_bytes(n) <= FusedMLP.ROLLOUT_LDS_BYTES < over.rollout_lds_bytes(n)
    assert fits.fits_rollout(n, 1) and not over.fits_rollout(n, 1)


@pytest.mark.parametrize("case", ALL_CASES, ids=IDS)
def test_reference_bound_holds_and_values_are_dyadic(case):
    """build() asserts the bound and the dyadic form; here also by hand: 2K + 3 after the first layer, and the worst bound in units."""
    b = mx.build(case)
    xmax = max(abs(case.xlo), abs(case.xhi))
    assert b.bounds[0] <= (xmax * case.sizes[0] + 3) * case.unit
    assert max(b.bounds) / case.unit < 2.0 ** 24
    assert b.want.shape == (case.B, case.sizes[-1])
    if not case.tanh:      # the expectation itself is a float32 value
        assert np.array_equal(b.want.astype(np.float32).astype(np.float64), b.want)
    else:                  # ... or the tanh of one, and not a saturated one: +-1 would hide everything but the sign
        assert np.array_equal(b.pre.astype(np.float32).astype(np.float64), b.pre)
        assert ((np.abs(b.pre) > 0.01) & (np.abs(b.pre) < 3)).mean() >= 0.5
    if case.clamp and b.want.size >= 8:
        bind = (b.want == b.clamp[0]) | (b.want == b.clamp[1])
        assert bind.any() and not bind.all(), "the clamp must bind on some outputs, not on all"
    if case.eps:
        assert (b.x_dev != b.x).any() and np.array_equal(b.x_dev.astype(np.float32).astype(np.float64), b.x)


def test_bound_is_asserted_not_assumed():
    net = mx.exact_net((8, 4, 1), ("relu", None), 0)
    x = mx.exact_inputs(3, 8, 0, np.float64) * 2.0 ** 22      # still dyadic, but 8 * 2**23 units
    _, bounds = mx.reference(net, x)
    with pytest.raises(AssertionError, match="2\\*\\*24"):
        mx.assert_exact(bounds)
    with pytest.raises(AssertionError, match="integer multiple"):
        mx.assert_dyadic(1.0, x=np.array([0.5]))
    mx.assert_dyadic(0.25, x=np.array([0.5, -1.75]))
    with pytest.raises(AssertionError, match="power of two"):
        mx.assert_dyadic(0.3, x=np.array([0.3]))
    # a layer whose dense bound would leave the range is thinned, not the case
    wide = mx.exact_net((8192, 256, 256, 4), ("relu", "relu", None), 1)
    nnz = [int((w != 0).sum(axis=1).max()) for w, _, _ in mx.layers_of(wide)]
    assert nnz[0] > 5000 and nnz[1] > 128 and 1 <= nnz[2] < 8
    mx.assert_exact(mx.reference(wide, mx.exact_inputs(2, 8192, 1, np.float64))[1])


def _float32_sum(terms, order):
    """Sum float32 ``terms`` [..., K] with float32 additions in the given order scheme."""
    K = terms.shape[-1]
    if order == "ascending":
        acc = np.zeros(terms.shape[:-1], np.float32)
        for k in range(K):
            acc = (acc + terms[..., k]).astype(np.float32)
        return acc
    if order == "descending":
        return _float32_sum(terms[..., ::-1], "ascending")
    # groups of 16, four interleaved partial chains per group (k % 4), chains added pairwise, groups ascending
    acc = np.zeros(terms.shape[:-1], np.float32)
    for g0 in range(0, K, 16):
        chains = [np.zeros(terms.shape[:-1], np.float32) for _ in range(4)]
        for k in range(g0, min(g0 + 16, K)):
            chains[k % 4] = (chains[k % 4] + terms[..., k]).astype(np.float32)
        acc = (acc + ((chains[0] + chains[1]).astype(np.float32) + (chains[2] + chains[3]).astype(np.float32)).astype(np.float32)).astype(np.float32)
    return acc


@pytest.mark.parametrize("case", [c for c in ALL_CASES if c.sizes[0] <= 2049] + [c for c in ALL_CASES if c.sizes[0] > 2049][::2],
                         ids=lambda c: c.name)
def test_first_layer_float32_sums_do_not_depend_on_the_order(case):
    """The premise, without a GPU: the first layer summed in float32 in three orders has the bits of the float64 reference."""
    b = mx.build(case)
    W, bias, _ = mx.layers_of(b.net)[0]
    want = b.x @ W.T                                                       # float64, exact
    terms = (b.x[:, None, :].astype(np.float32) * W[None, :, :].astype(np.float32)).astype(np.float32)   # [B, H, K]
    for order in ("ascending", "descending", "interleaved"):
        got = _float32_sum(terms, order)
        np.testing.assert_array_equal(got.astype(np.float64), want, err_msg=order)
        if bias is not None:
            np.testing.assert_array_equal((got + bias.astype(np.float32)[None]).astype(np.float32).astype(np.float64), want + bias[None])


def test_ordinary_weights_do_depend_on_the_order():
    """The control of the test above: with random float32 values the same three orders give different bits."""
    rng = np.random.default_rng(0)
    terms = (rng.standard_normal((17, 64, 577)).astype(np.float32) * rng.standard_normal((1, 64, 577)).astype(np.float32)).astype(np.float32)
    a, d, i = (_float32_sum(terms, o) for o in ("ascending", "descending", "interleaved"))
    assert (a != d).mean() > 0.5 and (a != i).mean() > 0.5


def _perturbed(L, layer, j, k):
    L2 = [(w.copy(), None if b is None else b.copy(), a) for w, b, a in L]
    L2[layer][0][j, k] += 1.0
    return L2


@pytest.mark.parametrize("case", ALL_CASES, ids=IDS)
def test_no_case_is_blind(case):
    """A reference with one first-layer weight moved by one unit -- in the first and in the last input column, the one next to the
    zero padding -- or with one of those input columns shifted by one unit gives another expectation: an error of that size in the
    kernel cannot pass.  (The weight is that of the first neuron, in scan order, whose value reaches an output at all: a neuron behind
    a zero weight or a closed ReLU shows nothing, whatever the kernel does.)"""
    b = mx.build(case)
    L = mx.layers_of(b.net)
    K, H = case.sizes[0], case.sizes[1]
    for k in sorted({0, K - 1}):
        seen = any(not np.array_equal(mx.reference(_perturbed(L, 0, j, k), b.x, b.noise, b.clamp)[0], b.want) for j in range(H))
        assert seen, f"no first-layer weight of input column {k} reaches the outputs"
        x2 = b.x.copy()
        x2[:, k] += case.unit
        assert not np.array_equal(mx.reference(L, x2, b.noise, b.clamp)[0], b.want), f"input column {k} shifted by one unit is not seen"
    if K > 1:      # the neighbouring column read in place of the right one
        x3 = np.roll(b.x, 1, axis=1)
        assert not np.array_equal(mx.reference(L, x3, b.noise, b.clamp)[0], b.want)
    if H > 1:      # the neighbouring neuron's weights read in place of the right ones
        L3 = [(np.roll(L[0][0], 1, axis=0), L[0][1], L[0][2])] + L[1:]
        assert not np.array_equal(mx.reference(L3, b.x, b.noise, b.clamp)[0], b.want)


@pytest.mark.parametrize("case", mx.FORWARD_CASES, ids=[c.name for c in mx.FORWARD_CASES])
def test_fused_mlp_over_the_cpu_double_reproduces_the_reference_bitwise(case):
    """FusedMLP.refresh's blocked transpose [ceil(in / 4), out, 4] and the descriptor, checked on the CPU: the double sums float32 in
    ascending k, which for these networks is exact."""
    from pdecontrolgym_amd.policy import FusedMLP
    from tests.fake_backend import FakeBackend
    b = mx.build(case)
    pol = FusedMLP(b.net, clamp=b.clamp, backend=FakeBackend())
    x = torch.from_numpy(b.x_dev)
    out = torch.full((case.B, case.sizes[-1]), 7.0, dtype=torch.float64 if case.y_f64 else torch.float32)
    pol.forward_into(x, out, noise=None if b.noise is None else torch.from_numpy(b.noise))
    if case.tanh:
        np.testing.assert_allclose(out.numpy().astype(np.float64), b.want, rtol=mx.TANH_RTOL, atol=mx.TANH_ATOL)
    else:
        np.testing.assert_array_equal(out.numpy().astype(np.float64), b.want)


@pytest.mark.parametrize("K,H", [(5, 1), (130, 17), (513, 65)])
def test_one_hot_expectation_through_the_cpu_double(K, H):
    from pdecontrolgym_amd.policy import FusedMLP
    from tests.fake_backend import FakeBackend
    lin = mx.real_linear(K, H, seed=K + H)
    ks = np.arange(K)
    want = mx.one_hot_expected(lin.weight.detach().numpy(), lin.bias.detach().numpy(), ks)
    assert want.dtype == np.float32 and want.shape == (K, H)
    got = FusedMLP(lin, backend=FakeBackend())(torch.from_numpy(mx.one_hot_rows(K, ks)))
    np.testing.assert_array_equal(got.numpy(), want)
    # full mantissas: a weight truncated to bfloat16 or to 19 bits would show
    bits = lin.weight.detach().numpy().view(np.uint32)
    assert ((bits & 0xFFFF) != 0).mean() > 0.99 and ((bits & 0x1FFF) != 0).mean() > 0.99
    # moving a single weight by one ulp changes exactly its own (row, neuron) entry
    W2 = lin.weight.detach().numpy().copy()
    W2[H // 2, K - 1] = np.nextafter(W2[H // 2, K - 1], np.float32(4))
    diff = mx.one_hot_expected(W2, None, ks) != mx.one_hot_expected(lin.weight.detach().numpy(), None, ks)
    assert diff.sum() == 1 and diff[K - 1, H // 2]


def test_seam_indices():
    ks = mx.seam_ks(2049)
    assert ks[0] == 0 and ks[-1] == 2048 and {63, 64, 127, 128, 511, 512, 513, 575, 576, 1023, 1024, 1025, 1535, 1536, 1537, 2047, 2048} <= set(ks)
    ks = mx.seam_ks(8192)
    assert ks[-1] == 8191 and all({m - 1, m, m + 1} <= set(ks) for m in range(512, 8192, 512)) and len(ks) < 70
    assert mx.seam_ks(5) == [0, 4]
    assert dataclasses.is_dataclass(mx.Case)
