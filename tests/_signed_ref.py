"""Numpy references for the signed-distance tests (tests/test_signed_distance.py): edge counts of the fan triangles,
the generalized winding number (inside / outside without any normals), and an analytic cube."""
import numpy as np

from oracle.icp_port import closest_point_on_triangles, fan_triangles  # noqa: F401  (re-exported for the tests)


def topology_counts(faces):
    """Edges of the fan triangles (0, j+1, j+2): (edges, boundary (1 triangle), non-manifold (>= 3), inconsistent (2
    triangles traversing the edge in the same direction))."""
    tri = fan_triangles(np.asarray(faces)).astype(np.int64)
    src = tri.ravel()
    dst = tri[:, [1, 2, 0]].ravel()
    lo, hi = np.minimum(src, dst), np.maximum(src, dst)
    key = lo * (int(tri.max()) + 1) + hi
    uniq, inv, cnt = np.unique(key, return_inverse=True, return_counts=True)
    fwd = np.bincount(inv, weights=(src < dst).astype(np.float64), minlength=len(uniq))
    two = cnt == 2
    inconsistent = int(np.sum(two & ((fwd == 0) | (fwd == 2))))
    return len(uniq), int(np.sum(cnt == 1)), int(np.sum(cnt >= 3)), inconsistent


def winding_number(points, faces, queries, block=64):
    """Sum of the signed solid angles of the triangles seen from each query, over 4 pi (Van Oosterom & Strackee):
    ~1 inside an outward-oriented closed mesh, ~0 outside."""
    tri = fan_triangles(np.asarray(faces))
    A, B, C = points[tri[:, 0]], points[tri[:, 1]], points[tri[:, 2]]
    out = np.empty(len(queries))
    for s in range(0, len(queries), block):
        q = queries[s:s + block, None, :]
        a, b, c = A[None] - q, B[None] - q, C[None] - q
        la, lb, lc = np.linalg.norm(a, axis=2), np.linalg.norm(b, axis=2), np.linalg.norm(c, axis=2)
        det = np.einsum("qti,qti->qt", a, np.cross(b, c))
        den = (la * lb * lc + np.einsum("qti,qti->qt", a, b) * lc + np.einsum("qti,qti->qt", a, c) * lb
               + np.einsum("qti,qti->qt", b, c) * la)
        out[s:s + block] = np.sum(2.0 * np.arctan2(det, den), axis=1) / (4.0 * np.pi)
    return out


def cube_quads():
    """The cube [-1, 1]^3 as 6 outward quads; vertex 4i + 2j + k = (2i-1, 2j-1, 2k-1)."""
    ijk = np.array([[i, j, k] for i in (0, 1) for j in (0, 1) for k in (0, 1)], dtype=np.float64)
    faces = np.array([[0, 1, 3, 2], [4, 6, 7, 5], [0, 4, 5, 1], [2, 3, 7, 6], [0, 2, 6, 4], [1, 5, 7, 3]], dtype=np.int32)
    return 2.0 * ijk - 1.0, faces


def cube_triangles():
    """The same cube as 12 triangles: the fan triangulation of `cube_quads`, so the edges (diagonals included) agree."""
    pts, quads = cube_quads()
    return pts, fan_triangles(quads).astype(np.int32)


def box_signed_distance(p):
    """Closed-form signed distance to the cube [-1, 1]^3: outside ||max(|p| - 1, 0)||, inside max |p_i| - 1."""
    e = np.abs(p) - 1.0
    outside = np.linalg.norm(np.maximum(e, 0.0), axis=1)
    return np.where(np.any(e > 0, axis=1), outside, np.max(e, axis=1))


def box_feature(p):
    """0 face, 1 edge, 2 vertex of the cube that the closest point of each (non-boundary) query lies on, and that
    closest point."""
    e = np.abs(p) - 1.0
    n_out = np.sum(e > 0, axis=1)
    c = np.clip(p, -1.0, 1.0)
    inside = n_out == 0
    ax = np.argmax(np.abs(p), axis=1)
    c[inside, ax[inside]] = np.sign(p[inside, ax[inside]])
    return np.where(inside, 0, n_out - 1), c
