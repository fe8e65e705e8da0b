"""Correctly rounded reference sums for the device's reduction kernels (plain numpy + `math`).

Every product a_i b_i is formed exactly as p + e with TwoProduct (Dekker: a Veltkamp split of each factor), and
`math.fsum` - correctly rounded - adds all the p and e together.  The result is the exact dot product of the float64
inputs, rounded once.

TwoProduct is exact only while neither factor overflows in the split and e stays a normal number.  Both vectors are
therefore scaled by powers of two (exact) so that their largest |entry| lies in [1, 2); a nonzero product whose error
term could underflow after that (or that underflows itself) raises instead of returning a wrong reference.
"""
import math

import numpy as np

EPS = 2.0 ** -53
_SPLIT = 2.0 ** 27 + 1.0
_TINY = 2.0 ** -968  # |p| below this: e = a b - p may be subnormal (inexact)


def split(a):
    """Veltkamp split: hi + lo == a exactly, each half with at most 26 significant bits."""
    a = np.asarray(a, dtype=np.float64)
    c = _SPLIT * a
    hi = c - (c - a)
    return hi, a - hi


def two_product(a, b):
    """(p, e) with p = fl(a b) and p + e == a b exactly (no overflow; |a b| >= 2^-968 or 0)."""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    p = a * b
    ah, al = split(a)
    bh, bl = split(b)
    e = ((ah * bh - p) + ah * bl + al * bh) + al * bl
    return p, e


def _scale(a):
    """(a 2^-k, k) with max |a 2^-k| in [1, 2) (k = 0 for an all-zero vector)."""
    m = float(np.max(np.abs(a))) if a.size else 0.0
    if m == 0.0 or not math.isfinite(m):
        return a, 0
    k = math.frexp(m)[1] - 1
    return np.ldexp(a, -k), k


def _exact_terms(a, b):
    """The scaled exact products of a and b as one array of float64 terms, and the power of two that undoes the scaling."""
    a = np.ascontiguousarray(a, dtype=np.float64).ravel()
    b = np.ascontiguousarray(b, dtype=np.float64).ravel()
    if a.shape != b.shape:
        raise ValueError("shapes differ: %s and %s" % (a.shape, b.shape))
    sa, ka = _scale(a)
    sb, kb = _scale(b)
    p, e = two_product(sa, sb)
    small = (np.abs(p) < _TINY) & (sa != 0.0) & (sb != 0.0)  # (an underflow to 0 included)
    if np.any(small):
        raise ValueError("exact_dot: products span too many binades for TwoProduct to stay exact")
    return np.concatenate([p, e]), ka + kb


def _fsum_scaled(terms, k):
    return math.ldexp(math.fsum(terms.tolist()), k)


def exact_dot(a, b):
    """sum_i a_i b_i, correctly rounded."""
    terms, k = _exact_terms(a, b)
    return _fsum_scaled(terms, k)


def exact_sumsq(a):
    """sum_i a_i^2, correctly rounded."""
    return exact_dot(a, a)


def exact_abs_dot(a, b):
    """sum_i |a_i b_i|, correctly rounded (the scale of a dot product's rounding error)."""
    return exact_dot(np.abs(a), np.abs(b))


def exact_gram(A, B):
    """G[i, j] = <A[:, i], B[:, j]>, each entry correctly rounded (A: (n, ka), B: (n, kb))."""
    A = np.asarray(A, dtype=np.float64)
    B = np.asarray(B, dtype=np.float64)
    return np.array([[exact_dot(A[:, i], B[:, j]) for j in range(B.shape[1])] for i in range(A.shape[1])]).reshape(A.shape[1], B.shape[1])


def _residual_parts(ax, x, lam):
    """ax - lam x as three float64 arrays (ax, -p, -e) whose sum is exact: lam x = p + e is never rounded."""
    p, e = two_product(np.full_like(np.asarray(x, dtype=np.float64), lam), x)
    return [np.asarray(ax, dtype=np.float64), -p, -e]


def exact_resnorm2(ax, x, lam):
    """||ax - lam x||^2, correctly rounded: the square of the exact three-term residual, all nine products exact."""
    parts = _residual_parts(ax, x, lam)
    terms, ks = [], []
    for u in parts:
        for v in parts:
            t, k = _exact_terms(u, v)
            terms.append(t)
            ks.append(k)
    # (a common power of two for all nine groups: ldexp per group is exact, the sum is then rounded once)
    k0 = min(ks)
    return math.ldexp(math.fsum(np.concatenate([np.ldexp(t, k - k0) for t, k in zip(terms, ks)]).tolist()), k0)


def exact_resnorm(ax, x, lam):
    """||ax - lam x||_2 from the correctly rounded square (one more rounding in the square root)."""
    return math.sqrt(exact_resnorm2(ax, x, lam))


def exact_rowdots(A, y):
    """(A y)_i for a dense (n, m) A, each row's sum correctly rounded (one TwoProduct pass over the whole matrix)."""
    A = np.asarray(A, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    terms, k = _exact_terms(A, np.broadcast_to(y, A.shape))
    t = terms.reshape(2, A.shape[0], A.shape[1])
    rows = np.concatenate([t[0], t[1]], axis=1).tolist()
    return np.array([math.ldexp(math.fsum(r), k) for r in rows])


def exact_matvec(indptr, indices, data, x):
    """(A x)_i for a CSR matrix, each row's sum correctly rounded."""
    x = np.asarray(x, dtype=np.float64)
    n = len(indptr) - 1
    if len(data) == 0:
        return np.zeros(n)
    terms, k = _exact_terms(data, x[indices])
    p, e = terms[: len(data)].tolist(), terms[len(data):].tolist()
    return np.array([math.ldexp(math.fsum(p[lo:hi] + e[lo:hi]), k) for lo, hi in zip(indptr[:-1], indptr[1:])])


def n_chunks(n, chunk=4096):
    """Reduction chunks of a graph of n rows (rows padded to a multiple of 4096, one block per 4096 rows)."""
    return (n + chunk - 1) // chunk


def reduction_depth(n):
    """A generous summation depth of the two-stage reductions over n rows: 16 products in series per thread, 6 shuffle
    levels in a wave and 2 across the 4 waves of a block, then ceil(chunks / 64) partial sums in series per lane and 6
    shuffle levels (33 + ceil(chunks / 64) in all, with the product's own rounding): 64 + chunks."""
    return 64 + n_chunks(n)


def dot_bound(a, b, depth):
    """Rounding-error bound of a dot product summed `depth` additions deep: depth 2^-53 sum |a_i b_i|."""
    return depth * EPS * exact_abs_dot(a, b)
