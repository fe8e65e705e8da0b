"""Numpy reference of uniform mesh resampling by clustering (tests/test_remesh.py), written from the definition in
include/pyfocusr_hip.h (`pf_mesh_cluster`); the device returns its bits.

  d2(i, j)   ((dx * dx + dy * dy) + dz * dz) with dx = P[i][0] - C[j][0], ...: separate multiplies and adds
  assign     label[i] = argmin_j d2(i, j) over all m centroids by brute force, the lowest j on ties
  update     per cluster the members in ascending vertex index, cut into consecutive runs of 64; a run is summed left to
             right from 0.0 (a[i] * P[i][x] and a[i]), the run sums are added left to right from 0.0, C = num / den; a
             cluster whose den is 0 keeps its centroid
  rep        the member with the smallest d2 to its centroid, the lowest vertex on ties; -1 without members
  dual       integers only: see `dual`
"""
import numpy as np

RUN = 64


def assign(P, C, chunk=2048):
    """(labels int32 (n,), d2 (n,)) of the points P (n, 3) against the centroids C (m, 3), by brute force."""
    P, C = np.asarray(P, dtype=np.float64), np.asarray(C, dtype=np.float64)
    labels, best = np.empty(len(P), dtype=np.int32), np.empty(len(P))
    for lo in range(0, len(P), chunk):
        p = P[lo:lo + chunk]
        d2, dy, dz = (p[:, None, x] - C[None, :, x] for x in range(3))
        d2 *= d2  # (dx * dx + dy * dy) + dz * dz, in place
        dy *= dy
        dz *= dz
        d2 += dy
        d2 += dz
        j = np.argmin(d2, axis=1)  # the first of equal minima
        labels[lo:lo + chunk] = j
        best[lo:lo + chunk] = d2[np.arange(len(p)), j]
    return labels, best


def _two_level(values, order, start, count):
    """Per cluster the sum of values[order[start : start + count]]: runs of 64 left to right, then the runs left to right."""
    m = len(start)
    n_runs = (count + RUN - 1) // RUN
    run_first = np.concatenate([[0], np.cumsum(n_runs)])[:-1]  # the first run of every cluster
    cluster_of_run = np.repeat(np.arange(m), n_runs)
    k_of_run = np.arange(int(n_runs.sum())) - run_first[cluster_of_run]
    pos = start[cluster_of_run] + RUN * k_of_run              # where the run starts in `order`
    length = np.minimum(RUN, count[cluster_of_run] - RUN * k_of_run)
    run_sum = np.zeros(len(pos))
    for k in range(RUN):
        on = np.flatnonzero(length > k)
        if not len(on):
            break
        run_sum[on] = run_sum[on] + values[order[pos[on] + k]]
    total = np.zeros(m)
    for k in range(int(n_runs.max()) if m else 0):
        on = np.flatnonzero(n_runs > k)
        total[on] = total[on] + run_sum[run_first[on] + k]
    return total


def update(P, a, labels, C):
    """The centroids after one update step from `labels`; `C` supplies the ones of clusters with den == 0."""
    P, a, C = np.asarray(P, dtype=np.float64), np.asarray(a, dtype=np.float64), np.array(C, dtype=np.float64)
    m = len(C)
    order = np.argsort(labels, kind="stable")
    count = np.bincount(labels, minlength=m)
    start = np.concatenate([[0], np.cumsum(count)])[:-1]
    den = _two_level(a, order, start, count)
    keep = den == 0.0
    for x in range(3):
        num = _two_level(a * P[:, x], order, start, count)
        with np.errstate(divide="ignore", invalid="ignore"):
            C[:, x] = np.where(keep, C[:, x], num / den)
    return C


def representatives(P, C, labels):
    """(rep int32 (m,), count int32 (m,))."""
    P, C = np.asarray(P, dtype=np.float64), np.asarray(C, dtype=np.float64)
    m = len(C)
    dx, dy, dz = (P[:, x] - C[labels, x] for x in range(3))
    d2 = (dx * dx + dy * dy) + dz * dz
    order = np.lexsort((np.arange(len(P)), d2, labels))  # by cluster, then d2, then vertex
    count = np.bincount(labels, minlength=m)
    start = np.concatenate([[0], np.cumsum(count)])[:-1]
    rep = np.full(m, -1, dtype=np.int32)
    rep[count > 0] = order[start[count > 0]]
    return rep, count.astype(np.int32)


def dual(F, labels):
    """The triangulation the clusters' adjacency induces: a dict of `faces` (k, 3) int32, `face_src` (k,) int32, `votes`
    (k, 2) int32 and `n_candidates`.

    An input face with three pairwise distinct labels is a candidate; it is rotated so that its smallest label comes first
    (which keeps its orientation).  The candidates of one set of three labels become one triangle, in the orientation most
    of them have - the orientation of the one with the lowest face index on a tie; `votes` counts the candidates for and
    against, `face_src` is the lowest face index among them.  The triangles are ordered by their sorted label triple."""
    F = np.asarray(F, dtype=np.int64).reshape(-1, 3)
    L = np.asarray(labels, dtype=np.int64)[F]
    cand = np.flatnonzero((L[:, 0] != L[:, 1]) & (L[:, 1] != L[:, 2]) & (L[:, 0] != L[:, 2]))
    L = L[cand]
    r = np.argmin(L, axis=1)
    rows = np.arange(len(L))
    l0, l1, l2 = L[rows, r], L[rows, (r + 1) % 3], L[rows, (r + 2) % 3]
    mid, hi = np.minimum(l1, l2), np.maximum(l1, l2)
    swapped = (l1 > l2).astype(np.int64)
    key = (l0 << 42) | (mid << 21) | hi
    order = np.argsort(key, kind="stable")  # equal keys in ascending face index
    key, swapped, src = key[order], swapped[order], cand[order]
    first = np.flatnonzero(np.r_[True, key[1:] != key[:-1]]) if len(key) else np.zeros(0, dtype=np.int64)
    size = np.diff(np.r_[first, len(key)])
    group = np.repeat(np.arange(len(first)), size)
    n1 = np.bincount(group, weights=swapped, minlength=len(first)).astype(np.int64)
    n0 = size - n1
    chosen = np.where(n1 > n0, 1, np.where(n0 > n1, 0, swapped[first]))
    k = key[first]
    a, b, c = k >> 42, (k >> 21) & ((1 << 21) - 1), k & ((1 << 21) - 1)
    faces = np.stack([a, np.where(chosen == 1, c, b), np.where(chosen == 1, b, c)], axis=1).astype(np.int32)
    votes = np.stack([np.where(chosen == 1, n1, n0), np.where(chosen == 1, n0, n1)], axis=1).astype(np.int32)
    return {"faces": faces.reshape(-1, 3), "face_src": src[first].astype(np.int32), "votes": votes.reshape(-1, 2),
            "n_candidates": len(cand)}


def cluster(P, F, a, sel, n_iter):
    """The whole definition: every output of `pf_mesh_cluster`, and `label_history` / `centroid_history` (the state
    after the start and after every iteration) for the tests of single steps."""
    P = np.ascontiguousarray(P, dtype=np.float64)
    a = np.ascontiguousarray(a, dtype=np.float64)
    C = P[np.asarray(sel, dtype=np.int64)].copy()
    labels, _ = assign(P, C)
    label_history, centroid_history, changed = [labels], [C], []
    for _ in range(int(n_iter)):
        C = update(P, a, labels, C)
        new, _ = assign(P, C)
        changed.append(int(np.count_nonzero(new != labels)))
        labels = new
        label_history.append(labels)
        centroid_history.append(C)
        if changed[-1] == 0:
            break
    rep, count = representatives(P, C, labels)
    out = {"labels": labels, "centroids": C, "rep": rep, "count": count, "changed": np.array(changed, dtype=np.int32),
           "n_iter_run": len(changed), "label_history": label_history, "centroid_history": centroid_history}
    out.update(dual(F, labels))
    return out


def energy(P, a, C, labels):
    """sum a_i d2(i, label_i)"""
    d = np.asarray(P) - np.asarray(C)[labels]
    return float(np.sum(np.asarray(a) * ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])))


def vertex_areas(P, F):
    """Barycentric vertex areas in plain numpy: masses for the tests (they need not be the device's bits)."""
    P, F = np.asarray(P, dtype=np.float64), np.asarray(F, dtype=np.int64)
    area = 0.5 * np.linalg.norm(np.cross(P[F[:, 1]] - P[F[:, 0]], P[F[:, 2]] - P[F[:, 0]]), axis=1)
    return np.bincount(F.ravel(), weights=np.repeat(area / 3.0, 3), minlength=len(P))


def grid_mesh(nx, ny, z=0.25):
    """A flat nx x ny grid of points, two triangles per square, z constant."""
    i, j = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    P = np.stack([i.ravel() * 0.37, j.ravel() * 0.41, np.full(nx * ny, z)], axis=1)
    v = (i * ny + j)[:-1, :-1].ravel()
    F = np.concatenate([np.stack([v, v + ny, v + ny + 1], 1), np.stack([v, v + ny + 1, v + 1], 1)]).astype(np.int32)
    return P, F
