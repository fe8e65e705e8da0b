"""Optimal one-to-one assignment of two point sets on Euclidean costs: `linear_sum_assignment(cdist(A, B))` on the
MI355X (`pf_assign`, csrc/pf_assign.hip), for Focusr's "hungarian" correspondences (focusr.py:340-349).

`PF_ASSIGN=host` sends every call to scipy instead (the reference's own call, O(n^2) memory).
"""
import os

import numpy as np

__all__ = ["euclidean_assignment"]

MAX_DEVICE_DIM = 16  # pf_assign's largest d


def _host_assignment(A, B):
    from scipy.optimize import linear_sum_assignment
    from scipy.spatial.distance import cdist

    return linear_sum_assignment(cdist(A, B))


def euclidean_assignment(A, B, return_duals=False, ctx=None):
    """(row_ind, col_ind) minimising sum_k ||A[row_ind[k]] - B[col_ind[k]]||, with scipy's conventions: row_ind
    ascending, min(n_A, n_B) pairs, every row (or column, when n_A > n_B) used once.

    On the device the solver is an exact auction with a dense optimality certificate (stats.gap_bound <= 1e-10 *
    stats.total_cost: well-conditioned inputs give scipy's permutation).  Where several assignments are exactly optimal
    (duplicate points, symmetric lattices) it may return another optimal one than scipy; PF_ASSIGN=host returns scipy's.

    return_duals: also (u, v, stats) with u over A's rows and v over B's rows, u_i + v_j <= ||A_i - B_j|| for every
    pair, and stats the device solver's `_hip.AssignStats` (None for the host path, and u, v then None as well).
    Non-finite coordinates raise ValueError; d > 16 goes to scipy."""
    A = np.ascontiguousarray(A, dtype=np.float64)
    B = np.ascontiguousarray(B, dtype=np.float64)
    if A.ndim != 2 or B.ndim != 2 or A.shape[1] != B.shape[1]:
        raise ValueError("A and B must be (n, d) arrays with equal d")
    if not (np.isfinite(A).all() and np.isfinite(B).all()):
        raise ValueError("coordinates must be finite")
    if os.environ.get("PF_ASSIGN", "device") == "host" or A.shape[1] > MAX_DEVICE_DIM or min(A.shape[0], B.shape[0]) == 0:
        row_ind, col_ind = _host_assignment(A, B)
        return (row_ind, col_ind, None, None, None) if return_duals else (row_ind, col_ind)
    from . import _hip

    ctx = ctx if ctx is not None else _hip.default_context()
    if A.shape[0] <= B.shape[0]:
        col, stats, u, v = ctx.assign(A, B, return_duals=True) if return_duals else ctx.assign(A, B) + (None, None)
        row_ind, col_ind = np.arange(A.shape[0], dtype=np.int64), col
    else:  # transposed: B's rows pick A's rows; sorted back to ascending A rows
        col, stats, v, u = ctx.assign(B, A, return_duals=True) if return_duals else ctx.assign(B, A) + (None, None)
        order = np.argsort(col, kind="stable")
        row_ind, col_ind = col[order], order.astype(np.int64)
    return (row_ind, col_ind, u, v, stats) if return_duals else (row_ind, col_ind)
