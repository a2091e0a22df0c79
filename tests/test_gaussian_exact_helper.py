"""CPU checks of tests/gaussian_exact.py, the case helper of tests/test_gpu_gaussian_head.py: every case keeps the exactness bound
(``build`` asserts it), keeps ``|sigma eps| <= 4``, has at least half of its outputs off the tanh's saturation, and is not blind to
the mistakes a kernel can make; every case set reaches log_std below, inside and above its bounds; the host wrapper on the CPU double
reproduces every expectation.  Conditions, not measurements: nothing here is derived from a kernel's output."""
import numpy as np
import pytest

from tests import gaussian_exact as gx

torch = pytest.importorskip("torch")
ALL = gx.FORWARD_CASES + gx.ROLLOUT_CASES


def test_case_names_are_unique_and_cover_what_the_gpu_file_promises():
    names = [c.name for c in ALL]
    assert len(set(names)) == len(names)
    fw = gx.FORWARD_CASES
    assert {c.A for c in fw} == {1, 2, 8} and {c.B for c in fw} >= {1, 15, 17, 33}
    assert {c.sizes[-2] for c in fw} >= {16, 64, 65, 256}
    assert {(c.A, c.sizes[-2]) for c in fw} >= {(A, W) for A in (1, 2, 8) for W in (16, 64, 65, 256)}
    assert {(c.x_f64, c.y_f64) for c in fw} == {(a, b) for a in (False, True) for b in (False, True)}
    assert any(c.gaps for c in fw) and any(not c.noise for c in fw) and any(c.noise for c in fw)
    ro = gx.ROLLOUT_CASES
    for env in {c.env for c in ro}:
        for wide in (False, True):
            assert {c.B for c in ro if c.env == env and c.wide == wide} == {5, 17, 33}, (env, wide)
    nodes = {c.env[4] for c in ro if c.env[0] == "1d" and c.env[3] == "full"}
    assert nodes == {30, 65, 257} and any(c.env[0] == "1d" and c.env[3] != "full" for c in ro)
    assert {c.env[1] for c in ro if c.env[0] == "traffic"} == {"both", "outlet"} and ("tumor", 70) in {c.env for c in ro}
    assert all(max(c.sizes[1:-1] + (2 * c.A,)) <= 256 for c in ro)


@pytest.mark.parametrize("case", ALL, ids=[c.name for c in ALL])
def test_no_case_is_blind(case):
    b = gx.build(case)
    want, z, se, _ = gx.head(b.pre, b.eps, case.bounds, case.box)
    assert np.array_equal(want, b.want) and np.isfinite(want).all()
    assert np.exp(case.bounds[1]) * case.eps_max <= 4 and np.abs(se).max() <= 4, "sigma * eps leaves the range the tolerance was derived for"
    assert np.abs(z).max() <= 8 or not case.noise or np.abs(b.pre[:, :case.A]).max() > 4      # (|z| > 8 only where mu itself is large)
    assert (np.abs(z) < 2).mean() >= 0.5, f"only {(np.abs(z) < 2).mean():.2f} of the outputs have |z| < 2"
    rtol, atol = gx.tolerance(case.box)
    for m in (gx.MUTATIONS if case.noise else gx.DETERMINISTIC_MUTATIONS):
        other = gx.head(b.pre, b.eps, case.bounds, case.box, m)[0]
        moved = np.abs(other - want) > 4 * (atol + rtol * np.abs(want))
        assert moved.any(), f"{m} does not show"
    # the float32 inputs are the exact values
    assert (b.x_dev.astype(np.float32).astype(np.float64) == b.x).all()


@pytest.mark.parametrize("name", sorted(gx.CASE_SETS))
def test_every_case_set_reaches_both_log_std_bounds_and_the_inside(name):
    below = inside = above = 0
    for case in gx.CASE_SETS[name]:
        if not case.noise:
            continue
        ls = gx.build(case).pre[:, case.A:]
        below += int((ls < case.bounds[0]).sum())
        inside += int(((ls > case.bounds[0]) & (ls < case.bounds[1])).sum())
        above += int((ls > case.bounds[1]).sum())
    assert below > 20 and inside > 20 and above > 20, (below, inside, above)
    sb3 = [c for c in gx.CASE_SETS[name] if c.noise and c.bounds == gx.SB3_BOUNDS]
    assert sb3 and any((gx.build(c).pre[:, c.A:] < -20).any() for c in sb3) and any((gx.build(c).pre[:, c.A:] > 2).any() for c in sb3)


def test_tolerance_is_the_derived_one():
    from tests import mlp_exact as mx
    assert gx.EXP_ATOL == 2.0 ** -20 + 2 * 2.0 ** -21
    rtol, atol = gx.tolerance((-1.0, 3.0))
    assert rtol == mx.TANH_RTOL and atol == (mx.TANH_ATOL + 2.0 ** -19) * 2.0


@pytest.mark.parametrize("case", [c for c in ALL if c.sizes[0] <= 257 and max(c.sizes[1:-1] + (1,)) <= 65],
                         ids=lambda c: c.name)
def test_host_wrapper_on_the_cpu_double_reproduces_the_expectation(case):
    """FusedMLP.squashed_gaussian -> descriptor -> the NumPy float32 double of the head (tests/fake_gaussian_backend.py) against the
    float64 expectation at the GPU tolerance (NumPy's float32 exp / tanh are correctly rounded to well within it)."""
    from tests.fake_gaussian_backend import FakeGaussianBackend
    b = gx.build(case)
    pol = gx.policy(b, case, backend=FakeGaussianBackend())
    assert pol.out_dim == case.A and pol.in_dim == case.sizes[0]
    x = torch.from_numpy(b.x_dev)
    y = torch.empty(case.B, case.A, dtype=torch.float64 if case.y_f64 else torch.float32)
    pol.forward_into(x, y, clamp=case.box, noise=None if b.eps is None else torch.from_numpy(b.eps))
    rtol, atol = gx.tolerance(case.box)
    np.testing.assert_allclose(y.numpy().astype(np.float64), b.want, rtol=rtol, atol=atol)
