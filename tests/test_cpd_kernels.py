"""The Coherent Point Drift device kernels (`pf_cpd.hip`) one entry point at a time, against tests/_cpd_ref.py
(numpy, every accumulation in np.longdouble), at the sizes where their tiling changes and at every template depth.

Bounds are derived, not measured.  A double-precision sum of n products is within  n * 2^-52 * S_abs  of the exact
one in any order, with or without FMA (S_abs: the sum of the terms' absolute values, from the reference), so every
moment, Gram and H / R entry must satisfy

    |got - want| <= 4 (n + 8) 2^-52 S_abs                    n: length of the summed dimension

the factor 4 covering the operands' own roundings (the centring subtractions, Q * w).  Outputs whose terms hold an
exp(-a) add the rounding of the argument - the relative error of exp(-a) is about (a + 2) 2^-52 plus the library's
few ulps - and use

    |got - want| <= 4 (n + 16 + a_max) 2^-52 S_abs           a_max: largest exponent argument of the case

The element-wise transforms use 4 (d + 2) 2^-52 (|Y| |B| + |t|) for TY = Y B + t and, by the same counting,
4 (K + 2) 2^-52 (|Y| + |Q| |C|) for TY = Y + Q C.  The means cx, cy are sums of n numbers divided once: 4 (n + 8) 2^-52
mean|x|.

Each moment kernel is tested in isolation: the E-step runs on the device, P1 / Pt1 / PX / TY are fetched with
`download()` and the reference is fed those same arrays.  The largest  error / bound  of each group is printed at the
end of the module (`pytest -s`).

CPU tests pin the reference helpers themselves against `oracle.cpd_port`.
"""
import numpy as np
import pytest

import _cpd_ref as ref
from oracle import cpd_port

EPS = ref.EPS
LD = np.longdouble
MIN_COLUMN_SUM = 1e-200

_worst = {}


def within(group, what, got, want, bound):
    """Assert |got - want| <= bound element-wise; record the largest error / bound of the group."""
    got, want, bound = (np.atleast_1d(np.asarray(a, dtype=LD)) for a in (got, want, bound))
    assert got.shape == want.shape == bound.shape, (what, got.shape, want.shape, bound.shape)
    assert np.all(np.isfinite(got)), what
    err = np.abs(got - want)
    ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err == 0, 0.0, np.inf))
    worst = float(ratio.max())
    _worst[group] = max(_worst.get(group, 0.0), worst)
    assert worst <= 1.0, "%s: error / bound = %.3g at %s" % (what, worst, np.unravel_index(np.argmax(ratio), ratio.shape))


def sum_bound(n, s_abs):
    return 4.0 * (n + 8) * EPS * s_abs


def exp_bound(n, a_max, s_abs):
    return 4.0 * (n + 16 + a_max) * EPS * s_abs


def clouds(seed, N, M, D, shift=0.0):
    """Unit-scale clouds, every coordinate with the same variance; the moving set lies near points of the fixed one."""
    rng = np.random.default_rng(seed)
    X = 0.5 * rng.normal(size=(N, D))
    Y = X[rng.integers(N, size=M)] + 0.1 * rng.normal(size=(M, D))
    return X + shift, Y + shift


def sigma2_for(D):
    return 0.05 * D  # exponent arguments of a few units at every depth


def check_estep(group, what, got, X, TY, sigma2, w):
    """(P1, Pt1, PX) of the device against the reference: P1 and PX are sums over N, Pt1 over M."""
    (P1, Pt1, PX), info = ref.expectation_ld(X, TY, sigma2, w)
    assert info["min_column_sum"] > MIN_COLUMN_SUM
    N, M = X.shape[0], TY.shape[0]
    within(group, what + " P1", got[0], P1, exp_bound(N, info["a_max"], info["P1"]))
    within(group, what + " Pt1", got[1], Pt1, exp_bound(M, info["a_max"], info["Pt1"]))
    within(group, what + " PX", got[2], PX, exp_bound(N, info["a_max"], info["PX"]))


def check_gram(group, what, got, A, B, beta, V):
    want, info = ref.gram_product_ld(A, B, beta, V)
    within(group, what, got, want, exp_bound(B.shape[0], info["a_max"], info["out"]))


# ------------------------------------------------------------------------------------------------------ CPU
def test_reference_expectation_and_gram_agree_with_oracle():
    rng = np.random.default_rng(0)
    X, Y = rng.uniform(0.5, 1.5, size=(37, 3)), rng.uniform(0.5, 1.5, size=(29, 3))  # positive terms: no cancellation
    for w in (0.0, 0.3):
        (P1, Pt1, PX), info = ref.expectation_ld(X, Y, 0.4, w)
        wP1, wPt1, wPX, _ = cpd_port.expectation(X, Y, 0.4, w)
        np.testing.assert_allclose(P1.astype(float), wP1, rtol=1e-12)
        np.testing.assert_allclose(Pt1.astype(float), wPt1, rtol=1e-12)
        np.testing.assert_allclose(PX.astype(float), wPX, rtol=1e-12)
        np.testing.assert_allclose(info["PX"].astype(float), wPX, rtol=1e-12)  # x > 0: S_abs is the sum itself
        assert info["min_column_sum"] > 0 and 0 < info["a_max"] < 10
    V = rng.uniform(0.5, 1.5, size=(29, 5))
    out, info = ref.gram_product_ld(X, Y, 0.8, V)
    np.testing.assert_allclose(out.astype(float), cpd_port.gaussian_kernel(X, 0.8, Y) @ V, rtol=1e-12)
    np.testing.assert_allclose(info["out"].astype(float), out.astype(float), rtol=1e-15)


def test_reference_expectation_eps_rule():
    """A column whose Gaussians all vanish takes eps as its sum: every posterior of that column is 0, not NaN."""
    X, Y = np.array([[0.0, 0.0], [1e4, 0.0]]), np.array([[0.1, 0.0], [0.0, 0.2]])
    (P1, Pt1, PX), info = ref.expectation_ld(X, Y, 0.05, 0.0)
    wP1, wPt1, wPX, _ = cpd_port.expectation(X, Y, 0.05, 0.0)
    assert info["min_column_sum"] == 0.0 and Pt1[1] == 0.0
    np.testing.assert_allclose(P1.astype(float), wP1, rtol=1e-12)
    np.testing.assert_allclose(Pt1.astype(float), wPt1, rtol=1e-12)
    np.testing.assert_allclose(PX.astype(float), wPX, rtol=1e-12, atol=1e-300)


def test_reference_centring_keeps_what_is_left_after_cancellation():
    """PX - P1 cx is all cancellation where PX is P1 cx up to its rounding (one fixed point): the reference's value is
    right to longdouble precision relative to what is LEFT, checked against rationals."""
    from fractions import Fraction

    rng = np.random.default_rng(4)
    b, c = rng.normal(size=40), rng.normal(size=40) + 1e3
    a = b * c
    a[20:] += rng.normal(size=20)
    got = ref._residual(a, b, c)
    for i in range(40):
        exact = Fraction(a[i]) - Fraction(b[i]) * Fraction(c[i])
        hi = float(got[i])
        mine = Fraction(hi) + Fraction(float(got[i] - LD(hi)))
        assert exact != 0 and abs(mine - exact) <= abs(exact) * Fraction(1, 2 ** 62), i


def test_reference_affine_moments_reproduce_oracle_iteration():
    """One iteration of the oracle's affine M-step from the moment sums, re-centred as `pyfocusr_amd/cpd.py` does.
    Both sides are sums of a few hundred terms of unit size; 1e-11 of the largest entry is a thousand of their
    roundings."""
    X, Y = clouds(1, 90, 70, 4, shift=0.3)
    reg = cpd_port.AffineRegistration(X, Y)
    reg.P1, reg.Pt1, reg.PX, reg.Np = cpd_port.expectation(X, Y, reg.sigma2, 0.1)
    reg.update_transform()
    want_xPx = reg.Pt1 @ np.sum(reg.X_hat * reg.X_hat, axis=1)
    (cx, _), (cy, _) = ref.mean_ld(X), ref.mean_ld(Y)
    m, s_abs = ref.affine_moments_ld(reg.P1, reg.Pt1, reg.PX, X, Y, cx, cy)
    m = {k: np.asarray(v, dtype=np.float64) for k, v in m.items()}
    Np = float(m["Np"])
    muX, muY = m["sPX"] / Np, m["sP1Y"] / Np
    A = m["PXY"] - Np * np.outer(muX, muY)
    YPY = m["YPY"] - Np * np.outer(muY, muY)
    xPx = m["sPt1XX"] - 2.0 * (muX @ m["sPt1X"]) + m["sPt1"] * (muX @ muX)
    np.testing.assert_allclose(Np, reg.Np, rtol=1e-13)
    np.testing.assert_allclose(A, reg.A, rtol=0, atol=1e-11 * np.abs(reg.A).max())
    np.testing.assert_allclose(YPY, reg.YPY, rtol=0, atol=1e-11 * np.abs(reg.YPY).max())
    np.testing.assert_allclose(xPx, want_xPx, rtol=1e-11)
    np.testing.assert_allclose(muX + np.asarray(cx, dtype=float), reg.PX.sum(axis=0) / reg.Np, rtol=1e-12)
    for k, v in s_abs.items():  # S_abs dominates its sum, field by field
        assert np.all(np.asarray(v) >= np.abs(np.asarray(m[k])) * (1 - 1e-15)), k


def test_reference_deformable_sums_reproduce_oracle_iteration():
    """One iteration of the oracle's low-rank deformable step: H, R, then sigma^2 from the five variance sums
    (a difference of sums about |x|^2 / sigma^2 ~ 10 times its size: 1e-11 relative leaves that margin)."""
    X, Y = clouds(2, 80, 60, 3)
    reg = cpd_port.DeformableRegistration(X, Y, alpha=0.7, beta=0.8, low_rank=True, num_eig=20)
    reg.P1, reg.Pt1, reg.PX, reg.Np = cpd_port.expectation(X, Y, reg.sigma2, 0.0)
    (H, R), (H_abs, R_abs) = ref.deform_sums_ld(reg.Q, reg.P1, reg.PX, Y)
    wH, wR = reg.Q.T @ (reg.P1[:, None] * reg.Q), reg.Q.T @ (reg.PX - reg.P1[:, None] * Y)
    np.testing.assert_allclose(H.astype(float), wH, rtol=0, atol=1e-12 * np.abs(wH).max())
    np.testing.assert_allclose(R.astype(float), wR, rtol=0, atol=1e-12 * np.abs(wR).max())
    assert np.all(H_abs >= np.abs(H)) and np.all(R_abs >= np.abs(R))
    reg.update_transform()
    reg.transform_point_cloud()
    reg.update_variance()
    s, s_abs = ref.variance_sums_ld(reg.P1, reg.Pt1, reg.PX, X, reg.TY)
    Np, yPy, trPXY, sPt1, xPx = (float(v) for v in s)
    np.testing.assert_allclose((xPx - 2 * trPXY + yPy) / (Np * 3), reg.sigma2, rtol=1e-11)
    np.testing.assert_allclose(sPt1, reg.Pt1.sum(), rtol=1e-13)
    assert np.all(s_abs >= np.abs(s))


def test_reference_transforms():
    rng = np.random.default_rng(3)
    Y, B, t, Q, Cm = (rng.normal(size=s) for s in ((11, 3), (3, 3), (3,), (11, 4), (4, 3)))
    TY, a = ref.affine_ld(Y, B, t)
    np.testing.assert_allclose(TY.astype(float), Y @ B + t, rtol=0, atol=1e-14)
    TY2, a2 = ref.deform_ld(Y, Q, Cm)
    np.testing.assert_allclose(TY2.astype(float), Y + Q @ Cm, rtol=0, atol=1e-14)
    assert np.all(a >= np.abs(TY)) and np.all(a2 >= np.abs(TY2))


# ------------------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def ctx():
    from pyfocusr_amd import _hip

    _hip.load_library()
    yield _hip.default_context()
    print()
    for group in sorted(_worst):
        print("largest error / bound, %-18s %.3g" % (group, _worst[group]))


def device(ctx, X, Y):
    from pyfocusr_amd import _hip

    return _hip.DeviceCpd(X, Y, ctx=ctx)


def posterior(dev, sigma2, w):
    """Resident E-step, then copies of (TY, P1, Pt1, PX) as they stand on the device."""
    dev.estep_resident(sigma2, w)
    return tuple(a.copy() for a in dev.download())


# ---- 1. every template depth
@pytest.mark.gpu
@pytest.mark.parametrize("w", [0.0, 0.3])
@pytest.mark.parametrize("D", range(1, 17))
def test_estep_every_depth(ctx, D, w):
    """N = 259, M = 131: tails of the 256-thread blocks and of the 128-point chunks.  Every coordinate has the same
    variance, so an instance of another depth (which strides the rows by its own d) is wrong in every output."""
    X, Y = clouds(100 + D, 259, 131, D)
    dev = device(ctx, X, Y)
    got = tuple(a.copy() for a in dev.estep(Y, sigma2_for(D), w))
    dev.close()
    check_estep("estep depth", "d=%d w=%g" % (D, w), got, X, Y, sigma2_for(D), w)


@pytest.mark.gpu
@pytest.mark.parametrize("D", range(1, 17))
def test_gram_every_depth(ctx, D):
    from pyfocusr_amd import _hip

    rng = np.random.default_rng(200 + D)
    A, B, V = 0.5 * rng.normal(size=(131, D)), 0.5 * rng.normal(size=(259, D)), rng.normal(size=(259, 9))
    beta = 0.4 * np.sqrt(D)
    check_gram("gram depth", "d=%d" % D, _hip.gaussian_gram_product(A, B, beta, V, ctx=ctx), A, B, beta, V)


# ---- 2. E-step tiling edges
ESTEP_EDGES = [(n, n) for n in (1, 127, 128, 129, 255, 256, 257, 385)] + [(1, 385), (385, 1), (127, 257), (257, 128),
                                                                           (129, 255), (256, 129)]


@pytest.mark.gpu
@pytest.mark.parametrize("N,M", ESTEP_EDGES)
def test_estep_tiling_edges(ctx, N, M):
    X, Y = clouds(300 + 7 * N + M, N, M, 3)
    sigma2, w = 0.2, 0.1
    dev = device(ctx, X, Y)
    first = tuple(a.copy() for a in dev.estep(Y, sigma2, w))
    check_estep("estep edges", "N=%d M=%d" % (N, M), first, X, Y, sigma2, w)
    again = tuple(a.copy() for a in dev.estep(Y, sigma2, w))
    for a, b in zip(first, again):  # chunk-ordered sums, no atomics
        assert np.array_equal(a, b)
    dev.estep(Y + 0.25, sigma2, w)  # move the resident set away, then bring it back through the affine kernel
    dev.apply_affine(np.eye(3), np.zeros(3))
    TY, P1, Pt1, PX = posterior(dev, sigma2, w)
    dev.close()
    assert np.array_equal(TY, Y)
    for a, b in zip(first, (P1, Pt1, PX)):
        assert np.array_equal(a, b)


# ---- 3. Gram product edges (GRAM_COLS = 8 columns per thread, CPD_TILE = 128 rows of B per tile, 256 rows of A per block)
GRAM_EDGES = ([(257, 129, c) for c in (1, 7, 8, 9, 16, 17)] + [(257, b, 9) for b in (1, 127, 128, 257)]
              + [(a, 129, 9) for a in (1, 255, 256)])


@pytest.mark.gpu
@pytest.mark.parametrize("n_a,n_b,cols", GRAM_EDGES)
def test_gram_edges(ctx, n_a, n_b, cols):
    from pyfocusr_amd import _hip

    rng = np.random.default_rng(400 + n_a + 3 * n_b + 5 * cols)
    A, B, V = 0.5 * rng.normal(size=(n_a, 3)), 0.5 * rng.normal(size=(n_b, 3)), rng.normal(size=(n_b, cols))
    got = _hip.gaussian_gram_product(A, B, 0.7, V, ctx=ctx)
    check_gram("gram edges", "%d x %d, %d columns" % (n_a, n_b, cols), got, A, B, 0.7, V)


# ---- 4. operands that share memory
@pytest.mark.gpu
def test_gram_aliased_operands(ctx):
    """B = A shares A's upload; a leading slice of a C-contiguous array has its base address, so equal pointers do not
    say equal arrays: `(Y[:k], Y)` must not read Y through the k-row upload of A."""
    from pyfocusr_amd import _hip

    rng = np.random.default_rng(5)
    Y = 0.5 * rng.normal(size=(300, 3))
    V = rng.normal(size=(300, 9))
    calls = [("Y, Y", Y, Y)] + [("Y[:%d], Y" % k, Y[:k], Y) for k in (1, 100)] \
        + [("Y, Y[:%d]" % k, Y, Y[:k]) for k in (1, 100)] + [("Y[5:105], Y", Y[5:105], Y)]
    for what, A, B in calls:
        assert np.shares_memory(A, B)
        Vb = V[:B.shape[0]]
        got = _hip.gaussian_gram_product(A, B, 0.7, Vb, ctx=ctx)
        check_gram("gram aliased", what, got, A, B, 0.7, Vb)
        assert np.array_equal(got, _hip.gaussian_gram_product(A.copy(), B.copy(), 0.7, Vb.copy(), ctx=ctx)), what


@pytest.mark.gpu
def test_transform_point_cloud_of_a_slice_of_the_moving_set(ctx):
    from pyfocusr_amd import cpd

    X, Y = clouds(6, 220, 200, 3)
    reg = cpd.deformable_registration(X=X, Y=Y, alpha=0.5, beta=1.0, num_eig=20, max_iterations=2, tolerance=0.0, ctx=ctx)
    reg.register()
    assert np.abs(reg.W).max() > 0
    part = reg.Y[:100]
    assert part.ctypes.data == reg.Y.ctypes.data
    got = reg.transform_point_cloud(part)
    assert np.array_equal(got, reg.transform_point_cloud(part.copy()))
    want, info = ref.gram_product_ld(part, reg.Y, reg.beta, reg.W)
    bound = exp_bound(200, info["a_max"], info["out"]) + 2 * EPS * (np.abs(part) + np.abs(want))  # the final addition
    within("gram aliased", "transform_point_cloud(Y[:100])", got, part.astype(LD) + want, bound)


# ---- 5. affine moments (MOM_ROWS = 64 rows per block; from d = 11 the 1 + 2d + 2d^2 outputs exceed 256 threads)
MOMENT_SIZES = [(1, 1), (63, 63), (64, 64), (65, 65), (130, 130), (1, 130), (130, 1), (63, 65), (65, 64), (64, 63), (130, 65)]


@pytest.mark.gpu
@pytest.mark.parametrize("shift", [0.0, 1e3])
@pytest.mark.parametrize("D", [1, 2, 3, 8, 11, 16])
def test_affine_moments(ctx, D, shift):
    """Every field of `affine_sums()`; the bound is relative to S_abs of the centred terms, also for clouds 1e3 away
    from the origin, where sums taken about the origin would lose six digits."""
    for N, M in MOMENT_SIZES:
        what = "d=%d N=%d M=%d shift=%g" % (D, N, M, shift)
        X, Y = clouds(500 + 31 * N + M + D, N, M, D, shift)
        dev = device(ctx, X, Y)
        TY, P1, Pt1, PX = posterior(dev, sigma2_for(D), 0.1)
        got = {k: np.array(v) for k, v in dev.affine_sums().items()}
        dev.close()
        assert np.array_equal(TY, Y)
        for name, cloud, n in (("cx", X, N), ("cy", Y, M)):
            mean, mean_abs = ref.mean_ld(cloud)
            within("affine moments", what + " " + name, got[name], mean, sum_bound(n, mean_abs))
        want, s_abs = ref.affine_moments_ld(P1, Pt1, PX, X, Y, got["cx"], got["cy"])
        assert set(want) | {"cx", "cy"} == set(got)
        for name in want:
            n = N if name.startswith("sPt1") else M
            within("affine moments", what + " " + name, got[name], want[name], sum_bound(n, s_abs[name]))


# ---- 6. TY = Y B + t
@pytest.mark.gpu
@pytest.mark.parametrize("M", [1, 255, 257])
@pytest.mark.parametrize("D", [1, 3, 16])
def test_apply_affine(ctx, D, M):
    rng = np.random.default_rng(600 + D + M)
    X, Y = clouds(600 + D + M, 5, M, D)
    B, t = np.eye(D) + 0.3 * rng.normal(size=(D, D)), rng.normal(size=D)
    dev = device(ctx, X, Y)
    dev.apply_affine(B, t)
    TY = dev.download()[0]
    dev.close()
    want, s_abs = ref.affine_ld(Y, B, t)
    within("apply_affine", "d=%d M=%d" % (D, M), TY, want, 4.0 * (D + 2) * EPS * s_abs)


# ---- 7. H = Q^T diag(P1) Q (GRAM_TILE = 16 outputs a side, GRAM_CHUNK = 512 rows per block) and R = Q^T (PX - P1 Y)
@pytest.mark.gpu
@pytest.mark.parametrize("M", [1, 15, 17, 511, 512, 513, 1025])
@pytest.mark.parametrize("K", [1, 15, 16, 17, 33])
def test_weighted_gram_and_deform_sums(ctx, K, M):
    what = "K=%d M=%d" % (K, M)
    X, Y = clouds(700 + 3 * K + M, 97, M, 3)
    Q = np.random.default_rng(K * 10000 + M).normal(size=(M, K))
    dev = device(ctx, X, Y)
    dev.set_basis(Q)
    _, P1, _, PX = posterior(dev, 0.2, 0.1)
    H_alone = dev.weighted_gram().copy()
    H, R = (a.copy() for a in dev.deform_sums())
    dev.close()
    (wH, wR), (H_abs, R_abs) = ref.deform_sums_ld(Q, P1, PX, Y)
    assert np.array_equal(H_alone, H)
    within("weighted gram", what + " H", H, wH, sum_bound(M, H_abs))
    within("weighted gram", what + " H - H^T", H, H.T, sum_bound(M, H_abs))
    within("deform rhs", what + " R", R, wR, sum_bound(M, R_abs))


@pytest.mark.gpu
@pytest.mark.parametrize("D", [3, 8, 16])
def test_deform_rhs_wide(ctx, D):
    """K d = 120, 320, 640: below one block's 256 threads, above them (the output loop wraps), and above the 561
    doubles of the handle's first scratch (both scratch buffers grow; 130 rows are three blocks of partial sums)."""
    K, M = 40, 130
    X, Y = clouds(800 + D, 77, M, D)
    Q = np.random.default_rng(800 + D).normal(size=(M, K))
    dev = device(ctx, X, Y)
    dev.set_basis(Q)
    _, P1, _, PX = posterior(dev, sigma2_for(D), 0.1)
    H, R = (a.copy() for a in dev.deform_sums())
    dev.close()
    (wH, wR), (H_abs, R_abs) = ref.deform_sums_ld(Q, P1, PX, Y)
    within("deform rhs", "K=40 d=%d H" % D, H, wH, sum_bound(M, H_abs))
    within("deform rhs", "K=40 d=%d R" % D, R, wR, sum_bound(M, R_abs))


# ---- 8. TY = Y + Q C and the five variance sums (256 rows per block of k_variance_m, 64 per block on the n side)
def check_apply_deform(group, what, dev, X, Y, Q, Cm, sigma2):
    """E-step at the current TY, then `apply_deform(Cm)`: the new TY and the five sums, which pair the posterior of
    that E-step with the new TY."""
    dev.estep_resident(sigma2, 0.1)
    sums = dev.apply_deform(Cm).copy()
    TY, P1, Pt1, PX = (a.copy() for a in dev.download())
    want_TY, TY_abs = ref.deform_ld(Y, Q, Cm)
    within(group, what + " TY", TY, want_TY, 4.0 * (Q.shape[1] + 2) * EPS * TY_abs)
    want, s_abs = ref.variance_sums_ld(P1, Pt1, PX, X, TY)
    M, N = Y.shape[0], X.shape[0]
    within(group, what + " sums", sums, want, [sum_bound(n, s) for n, s in zip((M, M, M, N, N), s_abs)])


@pytest.mark.gpu
@pytest.mark.parametrize("N", [63, 65, 130])
@pytest.mark.parametrize("M", [1, 255, 256, 257, 513])
def test_apply_deform(ctx, M, N):
    X, Y = clouds(900 + M + 5 * N, N, M, 3)
    rng = np.random.default_rng(900 + M + 5 * N)
    Q, Cm = rng.normal(size=(M, 7)), 0.05 * rng.normal(size=(7, 3))
    dev = device(ctx, X, Y)
    dev.set_basis(Q)
    check_apply_deform("apply_deform", "M=%d N=%d" % (M, N), dev, X, Y, Q, Cm, 0.2)
    dev.close()


# ---- 9. state of a handle
@pytest.mark.gpu
def test_basis_replaced_on_one_handle(ctx):
    """K = 40, then 5, then 70 on one handle with d = 9: K d = 360, 45 and 630, the last above the 561 doubles of the
    handle's first scratch, which `set_basis` regrows."""
    D, M = 9, 130
    X, Y = clouds(1000, 90, M, D)
    dev = device(ctx, X, Y)
    for K in (40, 5, 70):
        rng = np.random.default_rng(1000 + K)
        Q, Cm = rng.normal(size=(M, K)), 0.02 * rng.normal(size=(K, D))
        dev.set_basis(Q)
        dev.apply_deform(np.zeros((K, D)))  # TY = Y again
        _, P1, _, PX = posterior(dev, sigma2_for(D), 0.1)
        H, R = (a.copy() for a in dev.deform_sums())
        assert H.shape == (K, K) and R.shape == (K, D)
        (wH, wR), (H_abs, R_abs) = ref.deform_sums_ld(Q, P1, PX, Y)
        within("state", "K=%d H" % K, H, wH, sum_bound(M, H_abs))
        within("state", "K=%d R" % K, R, wR, sum_bound(M, R_abs))
        check_apply_deform("state", "K=%d" % K, dev, X, Y, Q, Cm, sigma2_for(D))
    dev.close()


@pytest.mark.gpu
def test_scratch_grows_and_is_reused_on_a_fresh_context():
    """K = 8, then 200, then 8 again on one handle (N = M = 300, d = 3) of a context that has allocated nothing: K d = 600
    is above the 561 doubles of the handle's first scratch, which grows, and the grown scratch then serves the small basis."""
    from pyfocusr_amd import _hip

    N = M = 300
    X, Y = clouds(1200, N, M, 3)
    fresh = _hip.Context(0)
    try:
        dev = device(fresh, X, Y)
        for K in (8, 200, 8):
            Q = np.random.default_rng(1200 + K).normal(size=(M, K))
            dev.set_basis(Q)
            _, P1, _, PX = posterior(dev, 0.2, 0.1)
            H_alone = dev.weighted_gram().copy()
            H, R = (a.copy() for a in dev.deform_sums())
            (wH, wR), (H_abs, R_abs) = ref.deform_sums_ld(Q, P1, PX, Y)
            assert np.array_equal(H_alone, H)
            within("state", "fresh K=%d H" % K, H, wH, sum_bound(M, H_abs))
            within("state", "fresh K=%d R" % K, R, wR, sum_bound(M, R_abs))
        dev.close()
    finally:
        fresh.close()


@pytest.mark.gpu
def test_refusals_leave_the_handle_usable(ctx):
    from pyfocusr_amd import _hip

    X, Y = clouds(1100, 70, 50, 3)
    dev = device(ctx, X, Y)

    def estep_still_right(after):
        got = tuple(a.copy() for a in dev.estep(Y, 0.2, 0.1))
        check_estep("state", "E-step after " + after, got, X, Y, 0.2, 0.1)

    for name, call in (("weighted_gram", dev.weighted_gram), ("deform_sums", dev.deform_sums),
                       ("apply_deform", lambda: dev.apply_deform(np.zeros((4, 3))))):
        with pytest.raises(_hip.PfError, match="no basis"):
            call()
        estep_still_right(name + " without a basis")
    with pytest.raises(_hip.PfError):
        dev.set_basis(np.zeros((50, 4097)))
    estep_still_right("set_basis with K = 4097")
    with pytest.raises(_hip.PfError, match="no basis"):
        dev.weighted_gram()  # the refused basis did not become one
    Q = np.random.default_rng(1100).normal(size=(50, 6))
    dev.set_basis(Q)
    with pytest.raises(_hip.PfError):
        dev.set_basis(np.zeros((50, 4097)))
    _, P1, _, PX = posterior(dev, 0.2, 0.1)
    (wH, _), (H_abs, _) = ref.deform_sums_ld(Q, P1, PX, Y)
    within("state", "H after a refused set_basis", dev.weighted_gram(), wH, sum_bound(50, H_abs))  # the K = 6 basis holds
    rng = np.random.default_rng(1101)
    with pytest.raises(_hip.PfError):
        _hip.DeviceCpd(rng.normal(size=(9, 17)), rng.normal(size=(7, 17)), ctx=ctx)
    estep_still_right("DeviceCpd with d = 17")
    with pytest.raises(_hip.PfError):
        _hip.gaussian_gram_product(rng.normal(size=(9, 17)), rng.normal(size=(7, 17)), 1.0, rng.normal(size=(7, 2)), ctx=ctx)
    estep_still_right("gaussian_gram_product with d = 17")
    dev.close()
