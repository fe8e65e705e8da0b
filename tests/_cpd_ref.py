"""Plain-numpy statement of what the Coherent Point Drift kernels (`pf_cpd.hip`) compute, every accumulation in
`np.longdouble`, written from the formulas in the kernels' comments and in `pyfocusr_amd/cpd.py`; the yardstick of
tests/test_cpd_kernels.py.  Nothing here imports the product.

Every helper returns its outputs and, under the same names, `S_abs`: the sum of the absolute values of the terms of
each output's sum - what a rounding-error bound of the form  n * 2^-52 * S_abs  is relative to.

  E-step        p_mn = exp(-|x_n - ty_m|^2 / 2 sigma^2) / (den_n + c),  den_n = sum_m exp(..) (eps where that is 0),
                c = (2 pi sigma^2)^(d/2) w / (1 - w) M / N;  P1_m = sum_n p_mn, Pt1_n = sum_m p_mn, PX_m = sum_n p_mn x_n
  Gram product  out_i = sum_j exp(-|a_i - b_j|^2 / 2 beta^2) V_j
  affine sums   about fixed centres cx, cy, with xc = x - cx, yc = y - cy, PXc_m = PX_m - P1_m cx:
                Np = sum P1 | sPX = sum PXc | sP1Y = sum P1 yc | PXY[d, e] = sum PXc[d] yc[e] |
                YPY[d, e] = sum P1 yc[d] yc[e] | sPt1 = sum Pt1 | sPt1XX = sum Pt1 |xc|^2 | sPt1X = sum Pt1 xc
  deformable    H = Q^T diag(P1) Q,  R = Q^T (PX - diag(P1) Y)
  variance      Np = sum P1 | yPy = sum P1 |ty|^2 | trPXY = sum ty . PX | sPt1 = sum Pt1 | xPx = sum Pt1 |x|^2
"""
import numpy as np

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)  # 2^-52


def _ld(*arrays):
    return tuple(np.asarray(a, dtype=np.float64).astype(LD) for a in arrays)


def _sqdist(A, B):
    """|a_i - b_j|^2, (len(A), len(B)), coordinate by coordinate (no (a, b, d) temporary)."""
    d2 = np.zeros((A.shape[0], B.shape[0]), dtype=LD)
    for c in range(A.shape[1]):
        df = A[:, c][:, None] - B[:, c][None, :]
        d2 += df * df
    return d2


def _residual(a, b, c):
    """a - b * c for doubles, as longdouble, to a relative 2^-63 of the RESULT however much cancels: b * c (106 bits)
    does not fit the 64 of a longdouble, so it is taken apart into a double product and its exact error (Dekker /
    Veltkamp, plain float64 numpy: no fused operations) and the two parts are subtracted in turn."""
    a, b, c = np.broadcast_arrays(*(np.asarray(v, dtype=np.float64) for v in (a, b, c)))
    p = b * c
    bh = 134217729.0 * b
    bh = bh - (bh - b)
    ch = 134217729.0 * c
    ch = ch - (ch - c)
    bl, cl = b - bh, c - ch
    e = ((bh * ch - p) + bh * cl + bl * ch) + bl * cl  # p + e == b * c exactly
    return (a.astype(LD) - p.astype(LD)) - e.astype(LD)


def expectation_ld(X, TY, sigma2, w):
    """(P1, Pt1, PX), info.  info holds S_abs of the three outputs under their names, `a_max` (the largest exponent
    argument |x - ty|^2 / 2 sigma^2 of the case) and `min_column_sum` (the smallest den_n before c is added)."""
    X, TY = _ld(X, TY)
    (N, D), M = X.shape, TY.shape[0]
    s2, w = LD(sigma2), LD(w)
    arg = _sqdist(TY, X) / (2 * s2)  # (M, N)
    E = np.exp(-arg)
    c = (2 * LD(np.pi) * s2) ** (LD(D) / 2) * w / (1 - w) * LD(M) / LD(N)
    colsum = E.sum(axis=0)
    den = np.where(colsum == 0, LD(EPS), colsum) + c
    P = E / den[None, :]
    P1, Pt1, PX = P.sum(axis=1), P.sum(axis=0), P @ X
    info = dict(P1=P1, Pt1=Pt1, PX=P @ np.abs(X), a_max=float(arg.max()), min_column_sum=float(colsum.min()))
    return (P1, Pt1, PX), info


def gram_product_ld(A, B, beta, V):
    """out (n_a, cols), info with S_abs under `out` and `a_max`."""
    A, B, V = _ld(A, B, V)
    arg = _sqdist(A, B) / (2 * LD(beta) * LD(beta))
    G = np.exp(-arg)
    return G @ V, dict(out=G @ np.abs(V), a_max=float(arg.max()))


def mean_ld(X):
    """Column means and S_abs of their sums (already divided by the count, like the means)."""
    (X,) = _ld(X)
    return X.sum(axis=0) / LD(X.shape[0]), np.abs(X).sum(axis=0) / LD(X.shape[0])


def affine_moments_ld(P1, Pt1, PX, X, Y, cx, cy):
    """(sums, S_abs): two dicts with the moment fields of `DeviceCpd.affine_sums()`, taken about the given centres."""
    pxc = _residual(PX, np.asarray(P1)[:, None], np.asarray(cx)[None, :])  # cancels entirely where PX = P1 cx (N = 1)
    P1, Pt1, PX, X, Y, cx, cy = _ld(P1, Pt1, PX, X, Y, cx, cy)
    xc, yc = X - cx[None, :], Y - cy[None, :]
    p1a, pt1a, xca, yca, pxca = (np.abs(a) for a in (P1, Pt1, xc, yc, pxc))
    sums = dict(Np=P1.sum(), sPX=pxc.sum(axis=0), sP1Y=(P1[:, None] * yc).sum(axis=0), PXY=pxc.T @ yc,
                YPY=yc.T @ (P1[:, None] * yc), sPt1=Pt1.sum(), sPt1XX=Pt1 @ (xc * xc).sum(axis=1),
                sPt1X=(Pt1[:, None] * xc).sum(axis=0))
    s_abs = dict(Np=p1a.sum(), sPX=pxca.sum(axis=0), sP1Y=(p1a[:, None] * yca).sum(axis=0), PXY=pxca.T @ yca,
                 YPY=yca.T @ (p1a[:, None] * yca), sPt1=pt1a.sum(), sPt1XX=pt1a @ (xc * xc).sum(axis=1),
                 sPt1X=(pt1a[:, None] * xca).sum(axis=0))
    return sums, s_abs


def deform_sums_ld(Q, P1, PX, Y):
    """(H, R), (S_abs of H, S_abs of R)."""
    F = _residual(PX, np.asarray(P1)[:, None], Y)
    Q, P1, PX, Y = _ld(Q, P1, PX, Y)
    qa = np.abs(Q)
    return (Q.T @ (P1[:, None] * Q), Q.T @ F), (qa.T @ (np.abs(P1)[:, None] * qa), qa.T @ np.abs(F))


def variance_sums_ld(P1, Pt1, PX, X, TY):
    """(sums, S_abs): two arrays [Np, yPy, trPXY, sum Pt1, xPx], the order of `DeviceCpd.apply_deform`."""
    P1, Pt1, PX, X, TY = _ld(P1, Pt1, PX, X, TY)
    ty2, x2 = (TY * TY).sum(axis=1), (X * X).sum(axis=1)
    sums = np.array([P1.sum(), P1 @ ty2, (TY * PX).sum(), Pt1.sum(), Pt1 @ x2], dtype=LD)
    s_abs = np.array([np.abs(P1).sum(), np.abs(P1) @ ty2, np.abs(TY * PX).sum(), np.abs(Pt1).sum(), np.abs(Pt1) @ x2],
                     dtype=LD)
    return sums, s_abs


def affine_ld(Y, B, t):
    """Y B + t and |Y| |B| + |t|."""
    Y, B, t = _ld(Y, B, t)
    return Y @ B + t[None, :], np.abs(Y) @ np.abs(B) + np.abs(t)[None, :]


def deform_ld(Y, Q, C):
    """Y + Q C and |Y| + |Q| |C|."""
    Y, Q, C = _ld(Y, Q, C)
    return Y + Q @ C, np.abs(Y) + np.abs(Q) @ np.abs(C)
