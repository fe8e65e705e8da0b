"""eigsort's sample-based cost matrices (`pf_eigsort_costs`, `pf_eigsort.hip`) restated from their definition; the
yardstick of tests/test_tail_kernels.py.

  c_hist[i][j]    = W1( log(T_i + 0.5 + eps), log(+-S_j + 0.5 + eps) ), the 1-D earth mover's distance of the samples
  c_spatial[i][j] = sqrt( sum_r (+-S_j[idx[r]] - T_i[r])^2 ) / mt, idx the 1-NN of target sample point r among the
                    min-max normalised source sample points
`w1_scipy` is the definition as scipy states it.  `w1_fsum` is the same integral over the merged breakpoints of the two
step quantile functions with every quantity that a tolerance needs: the logs are taken in extended precision where the
platform has it, the terms are rounded to double once and summed exactly (`math.fsum`).
"""
import math

import numpy as np
from scipy.stats import wasserstein_distance

EPS = float(np.finfo(np.float64).eps)
# x87 extended precision (64-bit mantissa): a log taken there, within 1 ulp of that format, is within 2^-11 ulp of a
# double; the differences of the logs are formed there too
EXTENDED = float(np.finfo(np.longdouble).eps) < 1e-18
REF_LOG_ULPS = 2.0 ** -11 if EXTENDED else 1.0  # (a double libm's log: 1 ulp)


def log_shifted(v, flip=False):
    """log(+-v + 0.5 + eps): the argument in double, as every implementation forms it ((+-v + 0.5) + eps), the log in
    extended precision (double where there is none)."""
    v = np.asarray(v, dtype=np.float64)
    arg = ((-v if flip else v) + 0.5) + EPS
    return np.log(arg.astype(np.longdouble)) if EXTENDED else np.log(arg)


def w1_scipy(t, s, flip=False):
    eps = np.finfo(float).eps
    s = -np.asarray(s) if flip else np.asarray(s)
    return float(wasserstein_distance(np.log(np.asarray(t) + 0.5 + eps), np.log(s + 0.5 + eps)))


def w1_fsum(t, s, flip=False):
    """W1 between the samples t (mt values) and s (ms values) after `log_shifted`: the integral over (0, 1) of
    |F_t^-1 - F_s^-1|; order statistic a of t holds on (a/mt, (a+1)/mt], b of s on (b/ms, (b+1)/ms]; the breakpoints are
    merged on the integer grid of mt*ms, where they are exact.
    Returns dict(value, abs_sum = sum |term|, n_terms, max_abs_log)."""
    lt = np.sort(log_shifted(t))
    ls = np.sort(log_shifted(s, flip))
    mt, ms = len(lt), len(ls)
    pts = np.union1d(np.arange(mt + 1, dtype=np.int64) * ms, np.arange(ms + 1, dtype=np.int64) * mt)
    left, length = pts[:-1], np.diff(pts)
    diff = np.abs(lt[left // ms] - ls[left // mt])
    terms = (diff * length.astype(lt.dtype) / lt.dtype.type(mt * ms)).astype(np.float64)
    return dict(value=math.fsum(terms), abs_sum=math.fsum(np.abs(terms)), n_terms=len(terms),
                max_abs_log=float(max(np.max(np.abs(lt)), np.max(np.abs(ls)))))


def w1_bound(ref, log_ulps_device=1.0):
    """|device - ref["value"]| allowed for a double implementation that sums the same terms in any order.
    Each term length * |lt - ls| is formed with at most four roundings (the unit 1/(mt ms), the length, the difference,
    the product: 4 * eps/2 relative) and the terms are added in some order ((n - 1) * eps/2 relative to sum |term|):
    together below (n + 2) * eps * sum |term|, which also covers the one rounding of each reference term.  The logs
    themselves: the device's is within `log_ulps_device` ulp (at most eps |log|) of the true value, the reference's
    within REF_LOG_ULPS; a term holds two logs and the lengths sum to 1."""
    log_ulps = log_ulps_device + REF_LOG_ULPS
    return (ref["n_terms"] + 2) * EPS * ref["abs_sum"] + 2.0 * log_ulps * EPS * ref["max_abs_log"]


def spatial_fsum(t, s_at_idx, flip=False):
    """sqrt(fsum((+-S_j[idx] - T_i)^2)) / mt and the relative bound for a double implementation.
    A term (s - t)^2 carries three roundings (the difference twice, the product: 1.5 eps relative), the sum in any order
    (n - 1) * eps/2 more: the device's sum A' = A (1 + delta), |delta| <= (n + 2) * eps as all terms are non-negative.
    sqrt(1 + delta) <= 1 + delta/2; the square root and the division round once each (eps together), and so do the
    reference's own (eps): relative bound delta/2 + 2 eps + delta * eps (the last term covers the products of the small ones)."""
    t = np.asarray(t, dtype=np.float64)
    s = -np.asarray(s_at_idx, dtype=np.float64) if flip else np.asarray(s_at_idx, dtype=np.float64)
    d = (s.astype(np.longdouble) - t.astype(np.longdouble)) if EXTENDED else (s - t)
    a = math.fsum((d * d).astype(np.float64))
    value = math.sqrt(a) / len(t)
    delta = (len(t) + 2) * EPS
    return value, value * (0.5 * delta + 2.0 * EPS + delta * EPS)


def minmax_points(p):
    """(p - min) / (max - min) per axis: IEEE subtraction and division, the same bits wherever it is computed."""
    p = np.asarray(p, dtype=np.float64)
    lo, hi = np.min(p, axis=0), np.max(p, axis=0)
    return (p - lo) / (hi - lo)
