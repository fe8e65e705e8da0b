"""The exact reference of tests/_exact.py against rational arithmetic (CPU only): what the vector-kernel tests compare
the device with must itself be right to the last bit."""
import math
from fractions import Fraction

import numpy as np
import pytest

import _exact as ex


def frac_dot(a, b):
    return sum((Fraction(float(x)) * Fraction(float(y)) for x, y in zip(a, b)), Fraction(0))


def cancelling_pair(rng, n, spread):
    """Vectors whose dot product cancels almost completely: large products in +/- pairs plus small ones."""
    a = rng.standard_normal(n) * np.exp2(rng.integers(-spread, spread + 1, n))
    b = rng.standard_normal(n) * np.exp2(rng.integers(-spread, spread + 1, n))
    h = n // 2
    a[h:2 * h] = a[:h]
    b[h:2 * h] = -b[:h] * (1.0 + 2.0 ** -40)  # the pairs cancel to ~2^-40 of their size
    return a, b


@pytest.mark.parametrize("seed", range(20))
def test_exact_dot_equals_rational_sum(seed):
    """exact_dot is the rational sum of the products rounded once (heavy cancellation, entries over 60 binades)."""
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1, 40))
    a, b = cancelling_pair(rng, n, 30)
    want = float(frac_dot(a, b))
    assert ex.exact_dot(a, b) == want
    assert ex.exact_sumsq(a) == float(frac_dot(a, a))
    assert ex.exact_abs_dot(a, b) == float(frac_dot(np.abs(a), np.abs(b)))
    assert ex.dot_bound(a, b, 10) == 10 * 2.0 ** -53 * ex.exact_abs_dot(a, b)


@pytest.mark.parametrize("exp_a,exp_b", [(1000, -1000), (-1000, 1000), (1018, -1018), (-1018, 1016), (500, 460), (-500, -460),
                                         (0, 0)])
def test_exact_dot_at_the_exponent_extremes(exp_a, exp_b):
    """Near the largest and smallest normal exponents: the power-of-two scaling keeps TwoProduct exact."""
    rng = np.random.default_rng(exp_a + 3 * exp_b + 5000)
    a, b = cancelling_pair(rng, 24, 2)  # (entries within 2^-5 .. 2^5 of 2^exp)
    a, b = np.ldexp(a, exp_a), np.ldexp(b, exp_b)
    want = frac_dot(a, b)
    assert np.all(np.isfinite(a)) and np.all(np.isfinite(b)) and want != 0
    assert ex.exact_dot(a, b) == float(want)


def test_two_product_reconstructs_every_product():
    """p + e == a b exactly (in rationals) over the binades the tests use, at both ends of each binade."""
    rng = np.random.default_rng(7)
    for ea in range(-480, 481, 40):
        for eb in (-480, -200, -3, 0, 5, 240, 480):
            a = np.ldexp(1.0 + rng.random(64), ea)
            b = np.ldexp(1.0 + rng.random(64), eb) * np.where(rng.random(64) < 0.5, -1.0, 1.0)
            a[0], b[0] = np.nextafter(np.ldexp(2.0, ea), 0.0), np.ldexp(1.0, eb)  # largest / smallest significand
            p, e = ex.two_product(a, b)
            for x, y, pp, ee in zip(a, b, p, e):
                assert Fraction(float(pp)) + Fraction(float(ee)) == Fraction(float(x)) * Fraction(float(y))
            hi, lo = ex.split(a)
            assert np.array_equal(hi + lo, a)


def test_exact_dot_refuses_what_it_cannot_do_exactly():
    a = np.array([1.0, 2.0 ** -600])
    b = np.array([1.0, 2.0 ** -600])
    with pytest.raises(ValueError):
        ex.exact_dot(a, b)


@pytest.mark.parametrize("seed", range(10))
def test_exact_resnorm_and_gram(seed):
    """||ax - lam x||^2 with lam x never rounded, and the Gram matrix's orientation."""
    rng = np.random.default_rng(100 + seed)
    n = int(rng.integers(1, 30))
    x = rng.standard_normal(n)
    lam = float(rng.uniform(0.1, 3.0))
    ax = lam * x + 1e-9 * rng.standard_normal(n)  # a small residual: the rounding of lam x would dominate it
    fx, fl = [Fraction(float(v)) for v in x], Fraction(lam)
    want = sum(((Fraction(float(a_)) - fl * v) ** 2 for a_, v in zip(ax, fx)), Fraction(0))
    assert ex.exact_resnorm2(ax, x, lam) == float(want)
    assert ex.exact_resnorm(ax, x, lam) == math.sqrt(float(want))
    A, B = rng.standard_normal((n, 3)), rng.standard_normal((n, 5))
    G = ex.exact_gram(A, B)
    assert G.shape == (3, 5)
    for i in range(3):
        for j in range(5):
            assert G[i, j] == float(frac_dot(A[:, i], B[:, j]))


def test_exact_matvec():
    rng = np.random.default_rng(3)
    from scipy import sparse

    M = sparse.random(40, 40, density=0.2, random_state=4, format="csr") * 1e3
    M = M - 1e3 * sparse.eye(40)
    x = rng.standard_normal(40)
    y = ex.exact_matvec(M.indptr, M.indices, M.data, x)
    for i in range(40):
        lo, hi = M.indptr[i], M.indptr[i + 1]
        assert y[i] == float(frac_dot(M.data[lo:hi], x[M.indices[lo:hi]]))
    D = M.toarray()[:, :7]
    z = ex.exact_rowdots(D, x[:7])
    for i in range(40):
        assert z[i] == float(frac_dot(D[i], x[:7]))


def test_depth():
    """The summation depth grows with the number of 4096-row chunks and leaves room for the in-chunk levels."""
    assert ex.n_chunks(1) == 1 and ex.n_chunks(4096) == 1 and ex.n_chunks(4097) == 2 and ex.n_chunks(397313) == 98
    assert ex.reduction_depth(1) == 65 and ex.reduction_depth(397312) == 64 + 97
