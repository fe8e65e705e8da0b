"""Plain-numpy statement of farthest-point sampling (`pyfocusr_amd.sampling`, `pf_fps.hip`), written from its
definition; the yardstick of tests/test_sampling.py.

Points P (n x d, float64, 1 <= d <= 16), m samples (1 <= m <= n), `start` an index or -1.
  d2(i, c)  the sum over the coordinates, left to right, of (P[i, x] - c[x])^2, separate multiply and add
  start -1  the first sample is the point with the largest d2 to the centroid, the lowest index on ties; the centroid is
            the per-coordinate mean, summed in index order
  dmin = +inf, owner = 0, cur = the first sample; round j = 0 .. m - 1:
            sel[j] = cur;  every i with d2(i, cur) < dmin[i] (strict) takes dmin[i] = d2(i, cur), owner[i] = j;
            cur = argmax dmin, the lowest index on ties
max(dmin) after the last round is the squared covering radius.  Once every dmin is 0 the argmax is index 0 again and
again: samples repeat when m exceeds the number of distinct points.
"""
import numpy as np


def d2_to(P, c):
    """d2(i, c) for every row i of P."""
    acc = np.zeros(len(P))
    for x in range(P.shape[1]):
        diff = P[:, x] - c[x]
        acc = acc + diff * diff
    return acc


def centroid(P):
    return np.add.accumulate(P, axis=0)[-1] / len(P)  # s_i = s_(i-1) + P[i]: index order


def centroid_distances(P):
    return d2_to(P, centroid(P))


def fps(P, m, start=-1):
    """(sel int64 (m,), owner int32 (n,), dmin (n,))."""
    P = np.asarray(P, dtype=np.float64)
    n, d = P.shape
    if not (1 <= d <= 16 and 1 <= m <= n and -1 <= start < n and np.all(np.isfinite(P))):
        raise ValueError("arguments outside the definition")
    cur = int(np.argmax(centroid_distances(P))) if start < 0 else int(start)  # argmax: the first, i.e. lowest, index
    sel = np.empty(m, dtype=np.int64)
    owner = np.zeros(n, dtype=np.int32)
    dmin = np.full(n, np.inf)
    for j in range(m):
        sel[j] = cur
        dist = d2_to(P, P[cur])
        closer = dist < dmin
        dmin[closer] = dist[closer]
        owner[closer] = j
        cur = int(np.argmax(dmin))
    return sel, owner, dmin
