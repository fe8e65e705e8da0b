"""Plain-numpy statement of the functional-map operations (`pyfocusr_amd.functional_maps`, `pf_fmap.hip`), written from
their definitions; the yardstick of tests/test_functional_maps.py.

Direction: T[i] in [0, n_t) for every SOURCE vertex i (Focusr's `corresponding_target_idx_for_each_source_pt`).
  project  C[a, b] = sum_i m_s[i] phi_s[i, a] phi_t[T[i], b]                         (k_s x k_t)
  convert  Q = phi_s[:, :k_s] C;  T[i] = the row of phi_t[:, :k_t] nearest to Q[i]: squared distances summed coordinate
           by coordinate, left to right, separate multiply and add; the lowest index wins an exact tie
  zoomout  k = k_start; loop: project (k, k); convert (k, k); stop if k == k_end; k = min(k + step, k_end)
"""
import numpy as np


def brute_force_nn(ref, qry, block=256):
    """(idx int64, d2) of the nearest `ref` row of every `qry` row; the accumulation order of `pf_knn.hip`."""
    ref, qry = np.asarray(ref, dtype=np.float64), np.asarray(qry, dtype=np.float64)
    idx = np.empty(len(qry), dtype=np.int64)
    d2 = np.empty(len(qry))
    for s in range(0, len(qry), block):
        q = qry[s:s + block]
        acc = np.zeros((len(q), len(ref)))
        for c in range(ref.shape[1]):
            acc += (q[:, None, c] - ref[None, :, c]) ** 2
        j = np.argmin(acc, axis=1)  # the first, i.e. lowest, index among equal minima
        idx[s:s + block] = j
        d2[s:s + block] = acc[np.arange(len(q)), j]
    return idx, d2


def row_d2(ref_rows, qry):
    """Squared distance of qry[i] to ref_rows[i], same accumulation."""
    acc = np.zeros(len(qry))
    for c in range(qry.shape[1]):
        acc += (qry[:, c] - ref_rows[:, c]) ** 2
    return acc


def project(phi_t, phi_s, mass_s, T, k_s, k_t):
    return (phi_s[:, :k_s] * mass_s[:, None]).T @ phi_t[T, :k_t]


def project_abs(phi_t, phi_s, mass_s, T, k_s, k_t):
    """sum_i |m_i phi_s[i, a] phi_t[T_i, b]|: what the rounding-error bound of any summation order scales with."""
    return np.abs(phi_s[:, :k_s] * mass_s[:, None]).T @ np.abs(phi_t[T, :k_t])


def convert(phi_t, phi_s, C, return_d2=False):
    k_s, k_t = C.shape
    idx, d2 = brute_force_nn(phi_t[:, :k_t], phi_s[:, :k_s] @ C)
    return (idx, d2) if return_d2 else idx


def zoomout(phi_t, phi_s, mass_s, T0, k_start, k_end, step=1, n_iter_at_end=0):
    T = np.asarray(T0, dtype=np.int64)
    k = k_start
    while True:
        C = project(phi_t, phi_s, mass_s, T, k, k)
        T = convert(phi_t, phi_s, C)
        if k == k_end:
            break
        k = min(k + step, k_end)
    for _ in range(n_iter_at_end):
        C = project(phi_t, phi_s, mass_s, T, k_end, k_end)
        T = convert(phi_t, phi_s, C)
    return T, C


# ---- the test pair: a mesh, and the same mesh renumbered by a random permutation and moved rigidly -------------------
def renumbered_pair(points, faces, seed=1):
    """(source points, source faces, T_true): source vertex perm[i] is target vertex i, so T_true[perm[i]] = i."""
    rng = np.random.default_rng(seed)
    perm = rng.permutation(len(points))
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    q *= np.sign(np.linalg.det(q))
    moved = np.empty_like(points)
    moved[perm] = points @ q.T + np.array([3.0, -20.0, 7.5])
    T_true = np.empty(len(points), dtype=np.int64)
    T_true[perm] = np.arange(len(points))
    return moved, perm[faces].astype(np.int32), T_true


def corrupt(T_true, fraction, seed=2):
    """T_true with `fraction` of its entries replaced by uniformly random indices."""
    rng = np.random.default_rng(seed)
    n = len(T_true)
    T0 = T_true.copy()
    bad = rng.choice(n, size=int(round(fraction * n)), replace=False)
    T0[bad] = rng.integers(0, n, size=len(bad))
    return T0
