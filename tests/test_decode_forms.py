"""The DEM decoders of wdpm_stencil.h against exact arithmetic: the two-operation quotient
v = fma(n, rD, n * rDlo) (dem_quotient) and the Newton form it replaced (q0 = n * rD, r = fma(-q0, D, n),
v = fma(r, rD, q0)) must both return RN(n / D) for every integer numerator n the codes can produce and D = 10^e,
e = 0..6 - and the 16-bit form's n = (gb + k0) + h must be the same number as (double)(gb + h) + k0.

The model is IEEE-754 binary64 throughout: Python floats for the roundings, an FMA built from Dekker's exact
product and math.fsum (the correctly rounded sum of the three addends), fractions.Fraction for the truth.
Zero differences are allowed.  The device does not rest on this test: dem_encode_kernel and dem16_encode_kernel
run the very decoders on every cell at upload and compare bits."""
import math
import struct
from fractions import Fraction

import numpy as np
import pytest

P10 = [10 ** e for e in range(7)]


def two_prod(a, b):
    """a * b == p + err exactly (Veltkamp split, Dekker product); valid here: no overflow, no underflow"""
    p = a * b
    c = 134217729.0 * a
    ah = c - (c - a)
    al = a - ah
    c = 134217729.0 * b
    bh = c - (c - b)
    bl = b - bh
    err = ((ah * bh - p) + ah * bl + al * bh) + al * bl
    return p, err


def fma(a, b, c):
    p, err = two_prod(a, b)
    return math.fsum((p, err, c))


def bits(x):
    return struct.unpack("<q", struct.pack("<d", x))[0]


def reciprocal_words(D):
    """rD and rDlo as wdpm_dem_codes.hip::encode_dem computes them"""
    Df = float(D)
    rD = 1.0 / Df
    rDlo = fma(-rD, Df, 1.0) / Df
    return Df, rD, rDlo


def decode_new(n, Df, rD, rDlo):
    return fma(n, rD, n * rDlo)


def decode_newton(n, Df, rD, rDlo):
    q0 = n * rD
    r = fma(-q0, Df, n)
    return fma(r, rD, q0)


def test_fma_model_is_exact():
    rng = np.random.default_rng(5)
    for _ in range(3000):
        a, b = float(rng.integers(-2 ** 53, 2 ** 53)), float(rng.random() * 10.0 ** float(rng.integers(-7, 1)))
        c = float(rng.standard_normal()) * a * b * float(rng.choice([1.0, 2.0 ** -53, -1.0, 0.0]))
        want = float(Fraction(a) * Fraction(b) + Fraction(c))          # int / int true division: correctly rounded
        assert bits(fma(a, b, c)) == bits(want), (a, b, c)


@pytest.mark.parametrize("e", range(7))
def test_second_word_of_the_reciprocal(e):
    D = P10[e]
    Df, rD, rDlo = reciprocal_words(D)
    assert Df == D
    assert bits(rD) == bits(float(Fraction(1, D)))
    assert bits(rDlo) == bits(float(Fraction(1, D) - Fraction(rD)))
    if e == 0:
        assert rD == 1.0 and rDlo == 0.0


def numerators(e, rng):
    """exact integers n = q + k0 in fp64: q over the full int32 range, k0 to 2^40, neighbours of powers of two and of multiples of D"""
    D = P10[e]
    out = []
    k0s = [0, 1, -1, 12345, -987654321, 2 ** 31, -2 ** 31, 2 ** 40, -2 ** 40, 2 ** 40 - 1, 5 * 10 ** 11 + 7]
    k0s += [int(v) for v in rng.integers(-2 ** 40, 2 ** 40, 12)]
    qs = [-2 ** 31 + 1, -2 ** 31 + 2, 2 ** 31 - 1, 2 ** 31 - 2, 0, 1, -1]
    for k0 in k0s:
        out += [q + k0 for q in qs]
        out += [int(q) + k0 for q in rng.integers(-2 ** 31 + 1, 2 ** 31, 1800)]
    for k in range(1, 54):                                      # neighbours of powers of two (up to 2^53, the decoder's limit)
        for d in range(-3, 4):
            for s in (1, -1):
                out.append(s * (2 ** k + d))
    for m in rng.integers(-2 ** 41 // D, 2 ** 41 // D + 1, 2500):        # neighbours of multiples of D: exact quotients and their ulps
        for d in (-1, 0, 1):
            out.append(int(m) * D + d)
    for k in range(1, 42):                                      # quotients next to a power of two: n ~ D * 2^k
        for d in range(-2, 3):
            out.append(D * 2 ** k + d)
            out.append(-(D * 2 ** k + d))
    return [n for n in out if abs(n) < 2 ** 53]


@pytest.mark.parametrize("e", range(7))
def test_both_forms_are_the_correctly_rounded_quotient(e):
    rng = np.random.default_rng(100 + e)
    D = P10[e]
    Df, rD, rDlo = reciprocal_words(D)
    ns = numerators(e, rng)
    assert len(ns) > 50000
    arr = np.array(ns, dtype=np.float64)
    assert all(int(v) == n for v, n in zip(arr[:2000], ns[:2000]))      # the numerators are exact in fp64
    truth = arr / Df                                            # IEEE division: RN(n / D) ...
    for i in range(0, len(ns), 7):                              # ... held against rational arithmetic on every seventh
        assert bits(float(truth[i])) == bits(float(Fraction(ns[i], D))), ns[i]
    bad_new, bad_newton = [], []
    for n, t in zip(arr.tolist(), truth.tolist()):
        if bits(decode_new(n, Df, rD, rDlo)) != bits(t):
            bad_new.append(n)
        if bits(decode_newton(n, Df, rD, rDlo)) != bits(t):
            bad_newton.append(n)
    assert not bad_newton, f"e={e}: the Newton form misses RN(n/D) at {bad_newton[:5]} ({len(bad_newton)} numerators)"
    assert not bad_new, f"e={e}: fma(n, rD, n*rDlo) misses RN(n/D) at {bad_new[:5]} ({len(bad_new)} numerators)"


@pytest.mark.parametrize("e", range(7))
def test_the_16_bit_split_gives_the_same_numerator(e):
    """n = ((double)gb + k0) + (double)h against (double)(gb + h) + k0 at group bases near +-2^31, and the decode of both"""
    rng = np.random.default_rng(200 + e)
    D = P10[e]
    Df, rD, rDlo = reciprocal_words(D)
    gbs = [-2 ** 31 + 1, -2 ** 31 + 2, -2 ** 31 + 65535, 2 ** 31 - 1 - 65534, 2 ** 31 - 65536 - 3, 0, -1, -65534, 1]
    gbs += [int(v) for v in rng.integers(-2 ** 31 + 1, 2 ** 31 - 65535, 40)]
    hs = [0, 1, 2, 65533, 65534, 32767, 32768] + [int(v) for v in rng.integers(0, 65535, 25)]
    k0s = [0, 1, -1, 2 ** 31, -2 ** 31, 2 ** 40, -2 ** 40, 2 ** 40 - 1, int(3.9e15), -int(3.9e15)] + [int(v) for v in rng.integers(-2 ** 40, 2 ** 40, 6)]
    checked = 0
    for gb in gbs:
        for h in hs:
            if gb + h > 2 ** 31 - 1:                            # the 32-bit code the pair stands for must exist
                continue
            for k0 in k0s:
                n_old = float(gb + h) + float(k0)
                n_new = (float(gb) + float(k0)) + float(h)
                assert n_new == gb + h + k0 and bits(n_old) == bits(n_new), (gb, h, k0)
                want = float(Fraction(gb + h + k0, D))
                assert bits(decode_new(n_new, Df, rD, rDlo)) == bits(want), (gb, h, k0)
                assert bits(decode_newton(n_old, Df, rD, rDlo)) == bits(want), (gb, h, k0)
                checked += 1
    assert checked > 20000
