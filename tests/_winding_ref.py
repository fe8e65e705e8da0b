"""Inputs and helpers of the winding-number tests (tests/test_winding_number.py).  The reference itself is
`_signed_ref.winding_number`; here are the meshes it is evaluated on, the query sets, and the reference's own unsigned
distance (to leave out queries on the surface, where w jumps)."""
import numpy as np

from _signed_ref import closest_point_on_triangles, fan_triangles


def open_mesh(points, faces, top=0.4):
    """The faces that have no vertex in the top `top` share of the z-range: an open surface with one boundary loop."""
    z = points[:, 2]
    cut = z.max() - top * (z.max() - z.min())
    return faces[~(z[faces] > cut).any(axis=1)]


def with_degenerate_faces(points, faces, n=20, seed=5):
    """`faces` plus `n` zero-area triangles (i, j, j) between random vertices: their solid angle is 0 from anywhere."""
    rng = np.random.default_rng(seed)
    ij = rng.integers(0, len(points), size=(n, 2))
    return np.concatenate([faces, np.stack([ij[:, 0], ij[:, 1], ij[:, 1]], axis=1).astype(faces.dtype)])


def diagonal(points):
    return float(np.linalg.norm(points.max(axis=0) - points.min(axis=0)))


def query_set(points, n_uniform=4000, seed=0, vertex_step=1):
    """`n_uniform` points uniform in the bounding box scaled by 1.3 about its centre, then every `vertex_step`-th vertex
    displaced by +5 % and by -5 % of the bounding-box diagonal along the direction from the vertex centroid."""
    rng = np.random.default_rng(seed)
    lo, hi = points.min(axis=0), points.max(axis=0)
    centre, half = 0.5 * (lo + hi), 0.65 * (hi - lo)
    uniform = rng.uniform(centre - half, centre + half, size=(n_uniform, 3))
    v = points[::vertex_step]
    d = v - points.mean(axis=0)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    step = 0.05 * diagonal(points)
    return np.concatenate([uniform, v + step * d, v - step * d])


def unsigned_distance(points, faces, queries, block=64, far=None):
    """Distance of every query to the surface by the reference's `closest_point_on_triangles` (all triangles).  With
    `far` set, a query that is provably farther than `far` gets +inf instead (every surface point has a vertex of its
    triangle within the longest edge L, so the distance is at least that to the nearest referenced vertex minus L)."""
    tri = fan_triangles(np.asarray(faces))
    a, b, c = points[tri[:, 0]], points[tri[:, 1]], points[tri[:, 2]]
    out = np.empty(len(queries))
    if far is not None:
        from scipy.spatial import cKDTree

        longest = np.sqrt(max(np.max(np.sum((x - y) ** 2, axis=1)) for x, y in ((a, b), (b, c), (c, a))))
        nearest = cKDTree(points[np.unique(tri)]).query(queries)[0]
        todo = np.flatnonzero(~(nearest - longest > far))
        out[:] = np.inf
        out[todo] = unsigned_distance(points, faces, queries[todo], block=block)
        return out
    for s in range(0, len(queries), block):
        q = queries[s:s + block]
        n = len(q)
        _, d2 = closest_point_on_triangles(np.repeat(q, len(tri), axis=0), np.tile(a, (n, 1)), np.tile(b, (n, 1)),
                                           np.tile(c, (n, 1)))
        d2 = d2.reshape(n, len(tri))
        out[s:s + n] = np.sqrt(np.min(np.where(np.isnan(d2), np.inf, d2), axis=1))
    return out
