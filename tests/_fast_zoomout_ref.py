"""Plain-numpy statement of ZoomOut on sub-samples (`zoomout_refine(samples=...)`, `pf_fmap_zoomout_sampled`), after
Melzi et al. 2019, 4.2.3; the yardstick of tests/test_fast_zoomout.py.  Projection, search and conversion are
`_fmap_ref`'s.

A = phi_s[S_s], B = phi_t[S_t].
  k = k_start;  C = project(T0) at (k, k), full resolution
  loop:  Tsub[i] = the row of B[:, :k] nearest to (A[:, :k] C)[i]
         last = (k == k_end and the n_iter_at_end extra rounds are used up)
         k = min(k + step, k_end)
         C = the solution of (A_k^T A_k) C = A_k^T B[Tsub, :k]          least squares on the samples, k x k
         stop if last
  T = convert(C) at full resolution
"""
import numpy as np

import _fmap_ref as fr


def gram(A, k):
    return A[:, :k].T @ A[:, :k]


def rhs(A, B, Tsub, k):
    return A[:, :k].T @ B[Tsub, :k]


def zoomout_sampled(phi_t, phi_s, mass_s, T0, S_t, S_s, k_start, k_end, step=1, n_iter_at_end=0):
    A, B = phi_s[np.asarray(S_s)], phi_t[np.asarray(S_t)]
    k, extra = k_start, n_iter_at_end
    C = fr.project(phi_t, phi_s, mass_s, np.asarray(T0, dtype=np.int64), k, k)
    while True:
        Tsub, _ = fr.brute_force_nn(B[:, :k], A[:, :k] @ C)
        last = k == k_end and extra == 0
        if k == k_end and not last:
            extra -= 1
        k = min(k + step, k_end)
        C = np.linalg.solve(gram(A, k), rhs(A, B, Tsub, k))
        if last:
            break
    return fr.convert(phi_t, phi_s, C), C
