"""Plain-numpy statement of the exact k-nearest-neighbour search (`pf_knn`, `pf_knn.hip`); the yardstick of
tests/test_tail_kernels.py and of tests/fuzz_knn.py.

  d2(q, r)  the sum over the coordinates, from coordinate 0 on, of (q_c - r_c)^2 with separate multiply and add
  result    per query the k references with the smallest (d2, index), ascending: equal distances go to the lower index
A query with a NaN coordinate compares with nothing: the device answers it with k indices 0x7fffffff and k infinite
distances, which this brute force does not restate (its callers leave such queries out).
"""
import numpy as np

NO_NEIGHBOUR = 0x7FFFFFFF


def brute(ref, qry, K, chunk=512):
    """(idx (n_qry, K) int64, d2 (n_qry, K)) by exhaustive search."""
    idx = np.empty((len(qry), K), dtype=np.int64)
    d2 = np.empty((len(qry), K))
    for lo in range(0, len(qry), chunk):
        q = qry[lo:lo + chunk]
        acc = None
        for c in range(ref.shape[1]):  # left to right, separate multiply and add
            df = q[:, None, c] - ref[None, :, c]
            sq = df * df
            acc = sq if acc is None else acc + sq
        order = np.lexsort((np.broadcast_to(np.arange(len(ref)), acc.shape), acc), axis=1)[:, :K]
        idx[lo:lo + chunk] = order
        d2[lo:lo + chunk] = np.take_along_axis(acc, order, axis=1)
    return idx, d2


def brute_argmin(ref, qry, K, chunk=512):
    """The same result for finite coordinates by K passes of `argmin` (the first, i.e. lowest, index among equals), each
    winner then taken out: no sort of whole rows, for the reference sets of tens of thousands of points in the tests."""
    idx = np.empty((len(qry), K), dtype=np.int64)
    d2 = np.empty((len(qry), K))
    for lo in range(0, len(qry), chunk):
        q = qry[lo:lo + chunk]
        acc = None
        for c in range(ref.shape[1]):
            df = q[:, None, c] - ref[None, :, c]
            sq = df * df
            acc = sq if acc is None else acc + sq
        rows = np.arange(len(q))
        for j in range(K):
            win = np.argmin(acc, axis=1)
            idx[lo:lo + chunk, j] = win
            d2[lo:lo + chunk, j] = acc[rows, win]
            acc[rows, win] = np.inf
    return idx, d2
