"""Exact k-nearest-neighbour search on the device (`pf_knn_topk`) and the inverse-distance average over the neighbours.

For every query the k references with the smallest (squared distance, index), ascending: squared distances are summed
coordinate by coordinate from coordinate 0 on, with separate multiply and add, and equal distances go to the lower
index.  1 <= k <= 64 neighbours in 1 <= d <= 128 coordinates; `tests/_knn_ref.py` states the definition in numpy and the
device returns its bits.  Up to 16 coordinates the search prunes with the box hierarchy of the 1-NN search
(`pf_knn_tree.hip`), beyond it scans every reference.

`inverse_distance_average` is the arithmetic of `Focusr.get_weighted_final_node_locations` (focusr.py:401-426) for any
per-reference values: with `functional_maps.soft_p2p_from_functional_map` it carries positions or point data across a
functional map as a smooth average over a few neighbours instead of one vertex's value.
"""
import numpy as np

from . import _hip

__all__ = ["k_nearest_neighbours", "inverse_distance_average"]


def k_nearest_neighbours(ref, qry, k, return_d2=True, ctx=None):
    """(idx (n_qry, k) int64, d2 (n_qry, k)): the k rows of `ref` (n_ref, d) nearest to every row of `qry` (n_qry, d),
    ascending by (squared distance, index); with `return_d2=False` idx alone.  `ValueError` for arrays that are not
    (n, d) with equal d, d outside 1 .. 128 and k outside 1 .. min(64, n_ref).  A query with a NaN coordinate has no
    neighbour: its row is k times (0x7fffffff, inf)."""
    k = _hip.check_knn_topk(ref, qry, k)
    ctx = ctx if ctx is not None else _hip.default_context()
    return ctx.knn_topk(ref, qry, k, return_d2=return_d2)


def inverse_distance_average(values, idx, d2):
    """(n_qry, c): for every query the average of `values` (n_ref, c) over its neighbours `idx` (n_qry, k) with weights
    1 / sqrt(d2), summed left to right; a neighbour at distance zero wins outright, the first one if there are several
    (focusr.py:415-419)."""
    values, idx, d2 = np.asarray(values), np.asarray(idx), np.asarray(d2, dtype=np.float64)
    if values.ndim != 2 or idx.ndim != 2 or idx.shape != d2.shape or idx.shape[1] < 1:
        raise ValueError("values must be (n_ref, c), idx and d2 (n_qry, k) with k >= 1")
    dist = np.sqrt(d2)
    pts = values
    with np.errstate(divide="ignore", invalid="ignore"):
        w = 1.0 / dist
        num = np.take(pts, idx[:, 0], axis=0) * w[:, 0:1]  # np.take: the fast path for whole-row gathers
        den = w[:, 0:1].copy()
        for j in range(1, idx.shape[1]):
            num = num + np.take(pts, idx[:, j], axis=0) * w[:, j:j + 1]
            den = den + w[:, j:j + 1]
        out = num / den
    coincident = dist == 0.0
    rows = np.nonzero(coincident.any(axis=1))[0]
    if len(rows):  # focusr.py:415-419: first zero-distance neighbour
        first = np.argmax(coincident[rows], axis=1)
        out[rows, :] = pts[idx[rows, first], :]
    return out
