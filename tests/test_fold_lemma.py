"""The lemma under the folded parabolic sub-step (pdegym_1d_body.h: run_substeps), on the CPU.

The fast parabolic sub-step forms  t2 = fma(-2, x, xm); t3 = t2 + xp; t4 = F * t3; t5 = x + t4; y = t5 + c * x.  With F = 2^-k
the product F * t3 is exact unless it underflows, and where it is exact fma(F, t3, x) == x + RN(F * t3) bit for bit.  The lemma: if
every EVEN slot (odd node: slot = node - 1, node 0 is the fixed left end) of the row entering a sub-step has |x| >= 2^-78, the folded
sub-step equals the reference's on every slot.  A mismatch at slot j needs |x[j]| < 2^-100 and a neighbour below 2^-78: two adjacent
tiny values, and of two adjacent slots one is even.

Both forms are restated in NumPy.  The fused multiply-add is one correctly rounded float32 of the exact x + F * t3, written as
`(x.astype(float64) + float64(F) * t3.astype(float64)).astype(float32)`:
  * F * t3 is exact in float64 (a power-of-two scaling far above the float64 denormal range) and has at most 24 significant bits;
  * where |x| < 2^-70 and the product sits on a grid of 2^-151 or coarser (k <= 2), both operands fit one 53-bit window and the
    float64 sum is exact;
  * where |x| >= 2^-100 and F * t3 underflowed, neither form can round away from x (the perturbation is below 2^-126 + 2^-150, half
    an ulp of x is at least 2^-125), whatever the float64 sum does;
  * in general the float64 sum may round (k = 24 puts F * t3 on a grid of 2^-173), but rounding the sum of two 24-bit numbers to
    53 >= 2 * 24 + 2 bits and then to 24 (or fewer, in the float32 denormal range) never differs from rounding once.
`test_fma32_is_the_correctly_rounded_sum` checks the expression against exact rational arithmetic.
"""
from fractions import Fraction

import numpy as np
import pytest

F32, F64 = np.float32, np.float64
FLOOR = F32(2.0 ** -78)           # the lemma's floor
KERNEL_FLOOR = F32(2.0 ** -64)    # what the kernel would use (margin)
KS = (1, 2, 3, 5, 10, 24)
NX = 256                          # 257 nodes: node 0, 255 interior nodes, the frozen boundary node


def fma32(f, t3, x):
    """RN32(x + f * t3) for float32 arrays t3, x and a power of two f = 2^-k, 1 <= k <= 24 (module docstring)."""
    return (x.astype(F64) + F64(f) * t3.astype(F64)).astype(F32)


def substep(row, c, f, fold):
    """One fast parabolic sub-step of rows[B, 257] (node 0 and the last node frozen), reference order or folded."""
    um, u, up = row[:, :-2], row[:, 1:-1], row[:, 2:]
    with np.errstate(all="ignore"):
        t2 = um - F32(2.0) * u                    # == fma(-2, u, um): 2u is exact
        t3 = t2 + up
        t5 = fma32(f, t3, u) if fold else u + F32(f) * t3
        y = t5 + c[:, 1:-1] * u
    out = row.copy()
    out[:, 1:-1] = y
    out[:, 0] = 0                                 # parabolic.py:146
    return out


def even_slot_min(row):
    """min |x| over the even slots the guard looks at: nodes 1, 3, ..., 255 (slot 255 = node 256 is the frozen boundary)."""
    return np.abs(row[:, 1:-1:2]).min(axis=1)


def mismatching_rows(row, c, f):
    a, b = substep(row, c, f, False), substep(row, c, f, True)
    return (a.view(np.uint32) != b.view(np.uint32)).any(axis=1)


def _rn32_exact(q):
    """Correctly rounded (nearest even) float32 of a Fraction, denormals kept."""
    if q == 0:
        return 0.0
    sign, q = (-1, -q) if q < 0 else (1, q)
    e = q.numerator.bit_length() - q.denominator.bit_length()
    if Fraction(2) ** e > q:
        e -= 1
    ulp = Fraction(2) ** (max(e, -126) - 23)
    n = q / ulp
    fl = n.numerator // n.denominator
    rem = n - fl
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and (fl & 1)):
        fl += 1
    return sign * float(fl * ulp)


def test_fma32_is_the_correctly_rounded_sum():
    rng = np.random.default_rng(5)
    n = 3000
    ex = rng.integers(-149, 3, n)
    x = (rng.uniform(1, 2, n) * 2.0 ** ex * rng.choice([-1, 1], n)).astype(F32)
    # products that straddle x's rounding boundaries: t3 near (half an ulp of x) / F, plus unrelated magnitudes
    k = rng.choice(KS, n)
    f = 2.0 ** -k.astype(F64)
    half_ulp = np.maximum(np.abs(x.astype(F64)) * 2.0 ** -24, 2.0 ** -150)
    t3 = np.where(rng.random(n) < 0.6, half_ulp / f * rng.choice([1.0, 1.0 + 2.0 ** -20, 1.0 - 2.0 ** -20, 3.0], n),
                  rng.uniform(1, 2, n) * 2.0 ** rng.integers(-149, 3, n)).astype(F32) * rng.choice([-1, 1], n).astype(F32)
    for i in range(n):
        got = fma32(float(f[i]), t3[i:i + 1], x[i:i + 1])[0]
        want = _rn32_exact(Fraction(float(x[i])) + Fraction(float(f[i])) * Fraction(float(t3[i])))
        assert F32(want).view(np.uint32) == got.view(np.uint32) or (want == 0 and got == 0), (x[i], t3[i], k[i])


# ---- input families: rows[B, 257], node 0 = 0; `tiny` values sit on odd slots (even nodes), adjacent to the even slots' values ----
def _tiny(rng, shape):
    """zero ... 2^-95: zeros, denormals, the smallest normals, and values up to 2^-95, both signs."""
    e = rng.integers(-149, -94, shape)
    v = (rng.uniform(1, 2, shape) * 2.0 ** e).astype(F32)
    v = np.where(rng.random(shape) < 0.15, 0, v)
    v = np.where(rng.random(shape) < 0.1, F32(2.0 ** -125), v)
    return (v * rng.choice([-1, 1], shape)).astype(F32)


def _fill(even, odd):
    row = np.zeros((even.shape[0], NX + 1), dtype=F32)
    row[:, 1::2] = even             # nodes 1, 3, ..., 255 = slots 0, 2, ..., 254
    row[:, 2::2] = odd              # nodes 2, 4, ..., 256 = slots 1, 3, ..., 255
    return row


def fam_unit_even_zero_odd(rng, B):
    even = rng.uniform(1, 2, (B, NX // 2)) * rng.choice([-1, 1], (B, NX // 2))
    return _fill(even.astype(F32), np.zeros((B, NX // 2), F32))


def fam_unit_even_tiny_odd(rng, B):
    even = rng.uniform(1, 2, (B, NX // 2)) * rng.choice([-1, 1], (B, NX // 2))
    return _fill(even.astype(F32), _tiny(rng, (B, NX // 2)))


def fam_floor_even_tiny_odd(rng, B):
    """even slots at the lemma's edge: 2^-78 exactly and up to 2^-60"""
    e = rng.integers(-78, -59, (B, NX // 2))
    m = np.where(rng.random((B, NX // 2)) < 0.3, 1.0, rng.uniform(1, 2, (B, NX // 2)))
    even = m * 2.0 ** e * rng.choice([-1, 1], (B, NX // 2))
    return _fill(even.astype(F32), _tiny(rng, (B, NX // 2)))


def fam_antisymmetric_even(rng, B):
    """x[j-1] == -x[j+1] around every odd slot: the neighbours cancel exactly, t3 is what the tiny slot leaves of t2"""
    e = rng.integers(-78, 2, (B, 1))
    mag = (rng.uniform(1, 2, (B, 1)) * 2.0 ** e).astype(F32)
    even = mag * np.where(np.arange(NX // 2) % 2 == 0, 1, -1)[None].astype(F32)
    return _fill(even, _tiny(rng, (B, NX // 2)))


def fam_nearly_antisymmetric_even(rng, B):
    """neighbours that cancel to a few ulps: t3 tiny but a multiple of the neighbours' ulp"""
    e = rng.integers(-78, -40, (B, 1))
    mag = (rng.uniform(1, 2, (B, 1)) * 2.0 ** e).astype(F32)
    wob = (1.0 + rng.integers(-3, 4, (B, NX // 2)) * 2.0 ** -23).astype(F32)
    even = mag * wob * np.where(np.arange(NX // 2) % 2 == 0, 1, -1)[None].astype(F32)
    return _fill(even.astype(F32), _tiny(rng, (B, NX // 2)))


def fam_log_uniform(rng, B):
    """every slot with an exponent of its own over 2^-78 ... 2^10 on the even slots, anything on the odd ones"""
    even = rng.uniform(1, 2, (B, NX // 2)) * 2.0 ** rng.integers(-78, 11, (B, NX // 2)) * rng.choice([-1, 1], (B, NX // 2))
    odd = rng.uniform(1, 2, (B, NX // 2)) * 2.0 ** rng.integers(-149, 11, (B, NX // 2)) * rng.choice([-1, 1], (B, NX // 2))
    odd = np.where(rng.random((B, NX // 2)) < 0.5, _tiny(rng, (B, NX // 2)), odd)
    return _fill(even.astype(F32), odd.astype(F32))


FAMILIES = (fam_unit_even_zero_odd, fam_unit_even_tiny_odd, fam_floor_even_tiny_odd, fam_antisymmetric_even,
            fam_nearly_antisymmetric_even, fam_log_uniform)


def _coeffs(rng, B):
    """c = dt * beta per slot, 2^-20 ... 1 in magnitude, both signs; zero on the two frozen nodes (as the kernel's)"""
    c = (rng.uniform(1, 2, (B, NX + 1)) * 2.0 ** rng.integers(-21, 0, (B, NX + 1)) * rng.choice([-1, 1], (B, NX + 1))).astype(F32)
    c[:, 0] = 0
    c[:, -1] = 0
    return c


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("family", FAMILIES, ids=lambda f: f.__name__[4:])
def test_no_mismatch_above_the_even_slot_floor(k, family):
    rng = np.random.default_rng(1000 * k + FAMILIES.index(family))
    B = 2000
    row, c = family(rng, B), _coeffs(rng, B)
    guarded = even_slot_min(row) >= FLOOR
    assert guarded.sum() >= B // 4, "the family must exercise the guarded side"
    bad = mismatching_rows(row, c, 2.0 ** -k)
    assert not (bad & guarded).any(), f"{int((bad & guarded).sum())} guarded rows differ"


@pytest.mark.parametrize("k", KS)
def test_the_check_discriminates(k):
    """the same families with their even slots made tiny: the two forms do differ there, so the assertion above is not vacuous"""
    rng = np.random.default_rng(77 + k)
    B = 2000
    row = fam_unit_even_tiny_odd(rng, B)
    row[:, 1::2] = _tiny(rng, (B, NX // 2))
    c = _coeffs(rng, B)
    assert (even_slot_min(row) < FLOOR).all()
    assert mismatching_rows(row, c, 2.0 ** -k).sum() >= 1


def _hundred_substep_rows(rng):
    """the rows tests/test_gpu_1d.py runs at nx = 256, S = 100 (compact support, denormal, just above the denormal range), and rows
    that stay far above the floor"""
    n = NX + 1
    B = 400
    rows = np.zeros((5 * B, n), dtype=F32)
    rows[0 * B:1 * B] = rng.uniform(1, 10, (B, n))
    for i in range(B):                                                       # compact support: the front underflows
        lo = int(rng.integers(2, n - 8))
        rows[1 * B + i, lo:lo + int(rng.integers(1, 6))] = rng.uniform(1, 3)
    rows[2 * B:3 * B] = (rng.uniform(-1, 1, (B, n)) * 1e-39).astype(F32)     # everything denormal
    rows[3 * B:4 * B] = (rng.uniform(0.5, 1, (B, n)) * 2.0 ** rng.integers(-126, -117, (B, 1))).astype(F32)
    rows[4 * B:5 * B] = F32(1.5 * 2.0 ** -64)                                # sinks below the kernel's floor within a few sub-steps
    rows[:, 0] = 0
    beta = rng.uniform(-30, 30, (5 * B, n)).astype(F32)
    beta[1 * B:3 * B] = 0
    return rows, beta


def test_hundred_substeps_with_the_guard_per_substep():
    """100 sub-steps at the headline shape (F = 0.25, dt = F / 256^2).  (1) Along the reference trajectory, a sub-step whose input row
    passes the guard is bit-identical in both forms: by induction the folded trajectory IS the reference's up to a row's first trip.
    (2) The kernel's plan -- fold while the running minimum stays at or above its floor, redo the whole call in the plain form
    otherwise -- ends on the reference's rows, and no row differs without having tripped."""
    rng = np.random.default_rng(2024)
    rows, beta = _hundred_substep_rows(rng)
    f = 0.25
    dt = F32(f / NX ** 2)
    c = dt * beta
    c[:, 0] = 0
    c[:, -1] = 0
    ref, fold = rows.copy(), rows.copy()
    ref = substep(ref, c, f, False)                 # the peeled first sub-step keeps the plain form in the kernel
    fold = ref.copy()
    tripped = np.zeros(len(rows), bool)             # the lemma's floor, per sub-step
    sticky = even_slot_min(fold) < KERNEL_FLOOR     # the kernel's running minimum, from the row the first fold sub-step reads
    unguarded_diff = 0
    for _ in range(99):
        guarded = even_slot_min(ref) >= FLOOR
        bad = mismatching_rows(ref, c, f)
        assert not (bad & guarded).any()
        unguarded_diff += int((bad & ~guarded).sum())
        tripped |= ~guarded
        ref = substep(ref, c, f, False)
        fold = substep(fold, c, f, True)
        sticky |= even_slot_min(fold) < KERNEL_FLOOR
    differ = (ref.view(np.uint32) != fold.view(np.uint32)).any(axis=1)
    assert not (differ & ~sticky).any(), "a row differs although the kernel's guard never tripped"
    assert not (differ & ~tripped).any(), "a row differs although the lemma's guard never tripped"
    assert differ.any() and unguarded_diff > 0      # unguarded, the fold is wrong on these rows: the guard is what makes it sound
    assert (~sticky[:400]).all()                    # ordinary rows keep the fold for the whole call
    assert sticky[1600:].all() and not (even_slot_min(rows[1600:]) < KERNEL_FLOOR).any()    # the mid-call trip exists
