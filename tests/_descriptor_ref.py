"""Plain-numpy statement of the spectral descriptors and the descriptor-fitted functional map
(`pyfocusr_amd.spectral_descriptors`, `pf_descriptors.hip`), written from their definitions; the yardstick of
tests/test_spectral_descriptors.py.

  descriptors   F[i, t] = sum_a phi[i, a]^2 G[a, t], a ascending, each term (p * p) * g, then added
  HKS           G[a, t] = exp(-lambda_a tau_t), tau = geomspace(4 ln10 / lambda_hi, 4 ln10 / lambda_lo, T)
  WKS           e = linspace(log lambda_lo, log lambda_hi, T), sigma = 7 (e_1 - e_0),
                G[a, t] = exp(-(e_t - log lambda_a)^2 / (2 sigma^2)) / sum_a of the same
  coefficients  A[a, t] = sum_i m_i phi[i, a] F[i, t]
  fit           C minimises ||C A_t - A_s||_F^2 + mu' sum_ab C_ab^2 ((lambda_s,a - lambda_t,b) / s)^2,
                s = max(lambda_s[k-1], lambda_t[k-1]), mu' = mu trace(A_t A_t^T) / k: row a of C solves
                (A_t A_t^T + mu' diag_b(((lambda_s,a - lambda_t,b) / s)^2)) c_a = A_t A_s[a]^T
"""
import numpy as np


def hks_table(vals, n_times=100, eig_range=None, times=None):
    vals = np.asarray(vals, dtype=np.float64)
    if np.any(vals <= 0):
        raise ValueError("non-positive eigenvalue")
    lo, hi = (vals[0], vals[-1]) if eig_range is None else eig_range
    if times is None:
        times = np.geomspace(4.0 * np.log(10.0) / hi, 4.0 * np.log(10.0) / lo, n_times)
    return np.exp(-vals[:, None] * times[None, :]), times


def wks_table(vals, n_energies=100, sigma_steps=7.0, eig_range=None, energies=None):
    vals = np.asarray(vals, dtype=np.float64)
    if np.any(vals <= 0):
        raise ValueError("non-positive eigenvalue")
    lo, hi = (vals[0], vals[-1]) if eig_range is None else eig_range
    if energies is None:
        energies = np.linspace(np.log(lo), np.log(hi), n_energies)
    sigma = sigma_steps * (energies[1] - energies[0])
    G = np.exp(-(energies[None, :] - np.log(vals)[:, None]) ** 2 / (2.0 * sigma ** 2))
    return G / G.sum(axis=0)[None, :], energies


def descriptors(phi, G):
    """The loop the device kernel must reproduce bit for bit."""
    phi, G = np.asarray(phi, dtype=np.float64), np.asarray(G, dtype=np.float64)
    F = np.zeros((phi.shape[0], G.shape[1]))
    for a in range(phi.shape[1]):
        F += (phi[:, a] * phi[:, a])[:, None] * G[a][None, :]
    return F


def coefficients(phi, mass, G, k):
    return (phi[:, :k] * mass[:, None]).T @ descriptors(phi, G)


def coefficients_long(phi, mass, G, k):
    """(A, A_abs) in extended precision: the sum, and the same sum with the absolute value of every term (F has
    non-negative terms when G >= 0; |G| covers the general case)."""
    lp, lm, lg = (np.asarray(x).astype(np.longdouble) for x in (phi, mass, G))
    F = (lp * lp) @ lg
    F_abs = (lp * lp) @ np.abs(lg)
    return (lp[:, :k] * lm[:, None]).T @ F, np.abs(lp[:, :k] * lm[:, None]).T @ F_abs


def tables(vals_t, vals_s, kinds=("hks", "wks"), n_samples=100):
    rng = (max(vals_t[0], vals_s[0]), min(vals_t[-1], vals_s[-1]))
    make = {"hks": lambda v: hks_table(v, n_samples, rng)[0], "wks": lambda v: wks_table(v, n_samples, 7.0, rng)[0]}
    return tuple(np.concatenate([make[kind](v) for kind in kinds], axis=1) for v in (vals_t, vals_s))


def fit(A_t, A_s, vals_t, vals_s, mu):
    k = A_t.shape[0]
    gram = A_t @ A_t.T
    mu_p = mu * np.trace(gram) / k
    s = max(vals_s[k - 1], vals_t[k - 1])
    C = np.empty((k, k))
    for a in range(k):
        C[a] = np.linalg.solve(gram + mu_p * np.diag(((vals_s[a] - vals_t[:k]) / s) ** 2), A_t @ A_s[a])
    return C


def functional_map(vals_t, phi_t, mass_t, vals_s, phi_s, mass_s, k, kinds=("hks", "wks"), n_samples=100, mu=0.1):
    G_t, G_s = tables(vals_t, vals_s, kinds, n_samples)
    return fit(coefficients(phi_t, mass_t, G_t, k), coefficients(phi_s, mass_s, G_s, k), vals_t, vals_s, mu)


# ---- the error measure of a map between two samplings of one surface ------------------------------------------------
def median_edge_length(points, faces):
    e = np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]])
    return float(np.median(np.linalg.norm(points[e[:, 0]] - points[e[:, 1]], axis=1)))


def map_errors(pt, ft, ps, T):
    """Distance from every source vertex to the target vertex it is mapped to, in median target edge lengths."""
    return np.linalg.norm(pt[T] - ps, axis=1) / median_edge_length(pt, ft)
