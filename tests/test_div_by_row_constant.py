"""div_by_row_constant (csrc/sot_device.hpp) restated on the host: x / S for a per-row constant S as q0 = x r, e = fma(-q0, S, x),
q1 = fma(e, r, q0) with r = RN(1 / S) must be the IEEE float32 quotient for every x in [2^-78, 2^20] and S in (2^-24, 2^40] -- the range
the kernels leave to it (smaller non-zero operands and larger masses take the IEEE sequence).  The scalar form works on one element, the
packed form on a pair of adjacent elements that share S and r (one v_pk_mul_f32 and two v_pk_fma_f32); each half of a pair is the scalar
operation, so both are the same three roundings here and must give the same bits.

float32 fma without a float32 fma: the product of two float32 is exact in float64 (48 bits), the sum with the addend is formed in
float64 ROUNDED TO ODD (two-sum recovers the rounding error; an inexact even result moves to its odd neighbour), and a 53-bit
round-to-odd followed by round-to-nearest to 24 bits is the correctly rounded result (53 >= 24 + 2), subnormal results included.
"""
import numpy as np
import pytest

F32 = np.float32
PER_BUCKET = 1_000_000
X_EXP = (-78, 20)     # x in [2^-78, 2^20]
S_EXP = (-24, 40)     # S in (2^-24, 2^40]


def fma32(a, b, c):
    """RN_float32(a * b + c) for float32 arrays."""
    p = a.astype(np.float64) * b.astype(np.float64)   # exact
    c = c.astype(np.float64)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)                   # two-sum: p + c == s + err exactly
    even = (s.view(np.int64) & 1) == 0
    fix = (err != 0.0) & even
    s = np.where(fix, np.nextafter(s, np.where(err > 0.0, np.inf, -np.inf)), s)
    return s.astype(F32)


def div_scalar(x, S):
    """One element: the sequence of div_by_row_constant(float, ...)."""
    r = (F32(1.0) / S).astype(F32)
    q0 = (x * r).astype(F32)
    e = fma32(-q0, S, x)
    return fma32(e, r, q0)


def div_packed(x, S):
    """Pairs (x[2 i], x[2 i + 1]) with S[i] and r[i] broadcast to both halves: the sequence of the packed overload."""
    pairs = x.reshape(-1, 2)
    Sb = np.repeat(S.reshape(-1, 1), 2, axis=1)
    rb = np.repeat((F32(1.0) / S).astype(F32).reshape(-1, 1), 2, axis=1)
    q0 = (pairs * rb).astype(F32)
    e = fma32(-q0, Sb, pairs)
    return fma32(e, rb, q0).reshape(-1)


def pow2(e):
    return np.ldexp(F32(1.0), e).astype(F32)


def draw(rng, lo_exp, hi_exp, n, open_low):
    """Random float32 with exponents uniform over [2^lo_exp, 2^hi_exp] and random mantissas ((2^lo_exp, 2^hi_exp] if open_low)."""
    e = rng.randint(lo_exp, hi_exp, size=n)
    m = rng.randint(0, 1 << 23, size=n).astype(np.uint32)
    v = ((e + 127).astype(np.uint32) << np.uint32(23)) | m
    v = v.view(F32)
    if open_low:
        v = np.where(v == pow2(lo_exp), pow2(hi_exp), v)
    return v.astype(F32)


def x_buckets():
    lo, hi = X_EXP
    cuts = [lo, -40, -10, 0, hi]
    return list(zip(cuts[:-1], cuts[1:]))


def s_buckets():
    lo, hi = S_EXP
    cuts = [lo, -8, 8, hi]
    return list(zip(cuts[:-1], cuts[1:]))


def test_fma32_is_a_correctly_rounded_fma():
    """The helper on cases whose float32 fma is known: an exact residual, a product far below the addend, a subnormal result, and a
    sum that a plain float64 addition rounds twice."""
    one, eps = F32(1.0), pow2(-23)
    a = np.array([one + eps, pow2(-70), F32(3.0)], F32)
    b = np.array([one - eps, pow2(-70), pow2(-149)], F32)
    c = np.array([-one, one, pow2(-149)], F32)
    want = np.array([-pow2(-46), one, pow2(-147)], F32)     # (1 + e)(1 - e) - 1 = -e^2;  1 + 2^-140 -> 1;  3 d + d = 4 d
    assert np.array_equal(fma32(a, b, c).view(np.uint32), want.view(np.uint32))
    # 4097 * 16773121 = 2^36 + 1, so the product below is 2^-24 + 2^-60 and the sum 1 + 2^-24 + 2^-60 lies just above a float32 tie:
    # float64 addition drops the 2^-60 and lands on the tie, which then rounds to even (1.0); the fused result is 1 + 2^-23
    a = np.array([F32(4097.0) * pow2(-30)], F32)
    b = np.array([F32(16773121.0) * pow2(-30)], F32)
    c = np.array([one], F32)
    assert float(a[0]) * float(b[0]) == 2.0 ** -24 + 2.0 ** -60
    assert F32(float(a[0]) * float(b[0]) + 1.0) == one      # the double rounding this helper must not make
    assert fma32(a, b, c)[0] == one + eps


@pytest.mark.parametrize("sb", s_buckets())
@pytest.mark.parametrize("xb", x_buckets())
def test_scalar_and_packed_quotients_are_ieee(xb, sb):
    rng = np.random.RandomState(1000 * (xb[0] + 200) + (sb[0] + 100))
    x = draw(rng, xb[0], xb[1], PER_BUCKET, open_low=False)
    S = draw(rng, sb[0], sb[1], PER_BUCKET, open_low=True)
    want = (x / S).astype(F32)
    got = div_scalar(x, S)
    bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, (bad.size, x[bad[:4]], S[bad[:4]], got[bad[:4]], want[bad[:4]])
    # the packed form: adjacent elements share the divisor of the first of them
    Sp = S[::2].copy()
    wantp = (x.reshape(-1, 2) / Sp.reshape(-1, 1)).astype(F32).reshape(-1)
    gotp = div_packed(x, Sp)
    badp = np.flatnonzero(gotp.view(np.uint32) != wantp.view(np.uint32))
    assert badp.size == 0, (badp.size, x[badp[:4]], gotp[badp[:4]], wantp[badp[:4]])
    assert np.array_equal(gotp[0::2].view(np.uint32), div_scalar(x[0::2], Sp).view(np.uint32))
    assert np.array_equal(gotp[1::2].view(np.uint32), div_scalar(x[1::2], Sp).view(np.uint32))


def test_boundary_operands():
    """Every boundary x against every boundary S: the ends of both ranges, their float32 neighbours inside them, powers of two and the
    significands next to a power of two (all ones / one bit)."""
    def around(e, below, above):
        v = [pow2(e)]
        if below:
            v.append(np.nextafter(pow2(e), F32(0.0)))
        if above:
            v.append(np.nextafter(pow2(e), F32(np.inf)))
        return v
    xs = around(X_EXP[0], False, True) + around(X_EXP[1], True, False)
    for e in (-77, -64, -24, -1, 0, 1, 19):
        xs += around(e, True, True)
    xs += [F32(3.0), F32(1.0) / F32(3.0), F32(0.1), F32(0.75)]
    ss = around(S_EXP[0], False, True)[1:] + around(S_EXP[1], True, False)
    for e in (-23, -1, 0, 1, 11, 39):
        ss += around(e, True, True)
    ss += [F32(3.0), F32(7.0), F32(1e-7), F32(1023.5), F32(2048.0) * F32(0.5000001)]
    xs, ss = np.array(xs, F32), np.array(ss, F32)
    X, S = [g.reshape(-1).astype(F32) for g in np.meshgrid(xs, ss, indexing="ij")]
    want = (X / S).astype(F32)
    assert np.array_equal(div_scalar(X, S).view(np.uint32), want.view(np.uint32))
    if X.size % 2:
        X, S, want = X[:-1], S[:-1], want[:-1]
    # pairs along x at one S: (x_i, x_{i+1}) share S_j
    Xp = np.stack([np.repeat(xs[:-1], ss.size), np.repeat(xs[1:], ss.size)], axis=1).reshape(-1).astype(F32)
    Sp = np.tile(ss, xs.size - 1).astype(F32)
    wantp = (Xp.reshape(-1, 2) / Sp.reshape(-1, 1)).astype(F32).reshape(-1)
    assert np.array_equal(div_packed(Xp, Sp).view(np.uint32), wantp.view(np.uint32))
