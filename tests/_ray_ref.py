"""Numpy reference of the ray casting tests (tests/test_ray_casting.py): the exact Moeller-Trumbore test of
`pf_surface_raycast`, restated operation for operation (same order of the products, sums and divisions, no FMA), over
ALL fan triangles of the mesh for every ray: no boxes, no pruning.  Ties in t go to the lowest fan-triangle index."""
import numpy as np

from _signed_ref import fan_triangles


def _cross(x, y):
    return (x[1] * y[2] - x[2] * y[1], x[2] * y[0] - x[0] * y[2], x[0] * y[1] - x[1] * y[0])


def _dot(x, y):
    return x[0] * y[0] + x[1] * y[1] + x[2] * y[2]


def cast(points, faces, origins, directions, t_min=0.0, t_max=np.inf, facing=0, block=128):
    """(t (n,) f64, face (n,) i32, uv (n, 2) f64, count (n,) i32) of the rays origins + t directions.
      e1 = b - a, e2 = c - a, p = d x e2, det = e1 . p, tv = o - a, u = (tv . p) / det, q = tv x e1, v = (d . q) / det,
      t = (e2 . q) / det;  accepted: det != 0, u >= 0, v >= 0, u + v <= 1, t_min <= t <= t_max, and facing (0 any,
      +1 det > 0, -1 det < 0).
    t is the least accepted one (+inf, face -1, NaN uv if none); a ray with a non-finite component or a zero direction
    gives NaN, -1, NaN, 0.  (u is divided for every pair, v and t only where u passed: each value is computed the same
    way wherever it is computed.)"""
    faces = np.asarray(faces)
    per_face = faces.shape[1] - 2
    tri = fan_triangles(faces)
    points = np.asarray(points, dtype=np.float64)
    A, B, C = points[tri[:, 0]], points[tri[:, 1]], points[tri[:, 2]]
    a = [A[None, :, k] for k in range(3)]
    e1 = [(B[:, k] - A[:, k])[None, :] for k in range(3)]
    e2 = [(C[:, k] - A[:, k])[None, :] for k in range(3)]
    origins = np.asarray(origins, dtype=np.float64)
    directions = np.asarray(directions, dtype=np.float64)
    n = len(origins)
    valid = np.all(np.isfinite(origins), axis=1) & np.all(np.isfinite(directions), axis=1) & np.any(directions != 0.0, axis=1)
    out_t = np.where(valid, np.inf, np.nan)
    out_face = np.full(n, -1, dtype=np.int32)
    out_uv = np.full((n, 2), np.nan)
    out_count = np.zeros(n, dtype=np.int32)
    rays = np.flatnonzero(valid)
    with np.errstate(all="ignore"):
        for s in range(0, len(rays), block):
            sel = rays[s:s + block]
            o = [origins[sel, k][:, None] for k in range(3)]
            d = [directions[sel, k][:, None] for k in range(3)]
            p = _cross(d, e2)
            det = _dot(e1, p)
            tv = [o[k] - a[k] for k in range(3)]
            u = _dot(tv, p) / det
            side = det != 0.0
            if facing > 0:
                side &= det > 0.0
            elif facing < 0:
                side &= det < 0.0
            r, k = np.nonzero(side & (u >= 0.0) & (u <= 1.0))  # u <= 1 follows from v >= 0 and u + v <= 1
            # the same operations on the pairs that are left, as flat arrays
            u, det = u[r, k], det[r, k]
            tv = [x[r, k] for x in tv]
            d1 = [x[r, 0] for x in d]
            q = _cross(tv, [x[0, k] for x in e1])
            v = _dot(d1, q) / det
            t = _dot([x[0, k] for x in e2], q) / det
            hit = (v >= 0.0) & (u + v <= 1.0) & (t_min <= t) & (t <= t_max)
            r, k, t, u, v = r[hit], k[hit], t[hit], u[hit], v[hit]
            out_count[sel] = np.bincount(r, minlength=len(sel))
            order = np.lexsort((k, t, r))  # by ray, then t, then triangle index
            first = order[np.r_[True, r[order][1:] != r[order][:-1]]] if len(order) else order
            w = sel[r[first]]
            out_t[w], out_face[w] = t[first], k[first] // per_face
            out_uv[w, 0], out_uv[w, 1] = u[first], v[first]
    return out_t, out_face, out_uv, out_count

