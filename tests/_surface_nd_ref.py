"""Numpy reference of `pf_surface_nd_closest` - test infrastructure, not product code.

The d-dimensional restatement of `oracle.icp_port.closest_point_on_triangles` (Ericson's region walk, evaluated for all
triangles at once, the regions tried in the order a, b, ab, c, ca, bc, interior) plus a brute-force driver.  The
arithmetic is the contract of include/pyfocusr_hip.h: every dot product and the squared distance summed left to right
over the coordinates, the closest point formed per coordinate by the region's formula, the weights (1-v-w, v, w) of the
region the walk ended in with exact zeros and ones."""
import numpy as np


def _dot(a, b):
    s = a[..., 0] * b[..., 0]
    for k in range(1, a.shape[-1]):
        s = s + a[..., k] * b[..., k]
    return s


def closest_point_on_triangles_nd(p, a, b, c):
    """Closest point to `p` (d,) on each triangle (a, b, c) (T, d): (points (T, d), bary (T, 3), dist2 (T,))."""
    one, zero = np.ones(len(a)), np.zeros(len(a))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        ab, ac, ap = b - a, c - a, p - a
        d1, d2 = _dot(ab, ap), _dot(ac, ap)
        bp = p - b
        d3, d4 = _dot(ab, bp), _dot(ac, bp)
        cp = p - c
        d5, d6 = _dot(ab, cp), _dot(ac, cp)
        vc = d1 * d4 - d3 * d2
        vb = d5 * d2 - d1 * d6
        va = d3 * d6 - d5 * d4
        out = np.empty_like(a)
        bary = np.empty((len(a), 3))
        done = np.zeros(len(a), dtype=bool)

        def put(mask, value, weights):
            m = mask & ~done
            out[m] = value[m]
            bary[m] = np.stack(weights, axis=1)[m]
            done[m] = True

        put((d1 <= 0) & (d2 <= 0), a, (one, zero, zero))
        put((d3 >= 0) & (d4 <= d3), b, (zero, one, zero))
        v = d1 / (d1 - d3)
        put((vc <= 0) & (d1 >= 0) & (d3 <= 0), a + v[:, None] * ab, (1.0 - v, v, zero))
        put((d6 >= 0) & (d5 <= d6), c, (zero, zero, one))
        w = d2 / (d2 - d6)
        put((vb <= 0) & (d2 >= 0) & (d6 <= 0), a + w[:, None] * ac, (1.0 - w, zero, w))
        w = (d4 - d3) / ((d4 - d3) + (d5 - d6))
        put((va <= 0) & ((d4 - d3) >= 0) & ((d5 - d6) >= 0), b + w[:, None] * (c - b), (zero, 1.0 - w, w))
        denom = 1.0 / (va + vb + vc)
        v, w = vb * denom, vc * denom
        put(np.ones(len(a), dtype=bool), (a + ab * v[:, None]) + ac * w[:, None], ((1.0 - v) - w, v, w))
        diff = p - out
        dist2 = _dot(diff, diff)
    return out, bary, dist2


def fan_triangles(faces):
    faces = np.asarray(faces)
    v = faces.shape[1]
    return np.stack([faces[:, [0, j + 1, j + 2]] for j in range(v - 2)], axis=1).reshape(-1, 3)


def closest_points_on_surface_nd(coords, faces, queries):
    """Brute force over ALL fan triangles: lowest fan-triangle index on exact ties, NaN distances never win; a
    non-finite query, or no finite distance at all, gives -1, (-1, -1, -1), NaN, NaN.  Returns a dict with face (q,)
    i32, vertices (q, 3) i32, bary (q, 3), d2 (q,), point (q, d) and triangle (q,) (the fan-triangle index)."""
    coords = np.asarray(coords, dtype=np.float64)
    queries = np.asarray(queries, dtype=np.float64)
    tris = fan_triangles(faces)
    per_face = np.asarray(faces).shape[1] - 2
    a, b, c = coords[tris[:, 0]], coords[tris[:, 1]], coords[tris[:, 2]]
    n, d = queries.shape
    face = np.full(n, -1, dtype=np.int32)
    tri = np.full(n, -1, dtype=np.int64)
    vertices = np.full((n, 3), -1, dtype=np.int32)
    bary = np.full((n, 3), np.nan)
    d2 = np.full(n, np.nan)
    point = np.full((n, d), np.nan)
    for i, p in enumerate(queries):
        if not np.all(np.isfinite(p)):
            continue
        pt, w, dist2 = closest_point_on_triangles_nd(p, a, b, c)
        cand = np.where(np.isnan(dist2), np.inf, dist2)
        t = int(np.argmin(cand))  # first index on ties
        if np.isnan(dist2[t]):
            continue
        face[i], tri[i], vertices[i], bary[i], d2[i], point[i] = t // per_face, t, tris[t], w[t], dist2[t], pt[t]
    return {"face": face, "vertices": vertices, "bary": bary, "d2": d2, "point": point, "triangle": tri}
