"""Numpy reference of the map distortion and coverage metrics (tests/test_map_quality.py, tools/bench_map_quality.py),
written from the definitions in include/pyfocusr_hip.h (`pf_map_distortion`), the independent SVD check beside it, and the
small meshes and maps the tests use.

Products and sums are written out one operation at a time in the stated order (numpy contracts nothing), dot products
left to right, cross products component by component.  Per-vertex sums are `np.bincount` over the half-edges in
ascending h, which adds in that order; the coverage sums are the two-level sums of `_remesh_ref` (runs of 64); the totals
go along the fixed tree of `tree_sum`.  Only + - x / sqrt occur, each correctly rounded here and on the device, so the
device is expected to return these bits."""
import numpy as np

from _curvature_ref import _cross, _dot
from _remesh_ref import _two_level, grid_mesh  # noqa: F401 - grid_mesh is one of the tests' meshes

VALID, COLLAPSED, FLIPPED, UNMAPPED = 1, 2, 4, 8
GROUP = 256


def tree_sum(x):
    """The sum of x in ascending order along the fixed tree: 256 consecutive terms left to right from 0.0, 256 of those
    sums likewise, the rest in order."""
    x = np.asarray(x, dtype=np.float64)
    for _ in range(2):
        pad = (-len(x)) % GROUP
        block = np.concatenate([x, np.zeros(pad)]).reshape(-1, GROUP)  # + 0.0 at the end of a sum changes no bit
        acc = np.zeros(len(block))
        for k in range(GROUP):
            acc = acc + block[:, k]
        x = acc
    total = 0.0
    for v in x:
        total = total + v
    return float(total)


def images(tgt_pts, map_vertices, map_weights=None, tgt_normals=None):
    """(y (n, 3), m (n, 3) or None, owner (n,) int64 with len(tgt_pts) for an unmapped row, mapped (n,) bool)."""
    X = np.asarray(tgt_pts, dtype=np.float64)
    V = np.asarray(map_vertices, dtype=np.int64)
    V = V.reshape(len(V), -1)
    mapped = V[:, 0] != -1
    Vs = np.where(mapped[:, None], V, 0)

    def image_of(values):
        if V.shape[1] == 1:
            out = values[Vs[:, 0]]
        else:
            w = np.where(mapped[:, None], np.asarray(map_weights, dtype=np.float64), 0.0)
            out = (w[:, 0:1] * values[Vs[:, 0]] + w[:, 1:2] * values[Vs[:, 1]]) + w[:, 2:3] * values[Vs[:, 2]]
        return np.where(mapped[:, None], out, 0.0)

    if V.shape[1] == 1:
        owner = Vs[:, 0]
    else:
        w = np.asarray(map_weights, dtype=np.float64)
        best = np.zeros(len(V), dtype=np.int64)
        best = np.where(w[:, 1] > w[:, 0], 1, best)
        best = np.where(w[:, 2] > w[np.arange(len(V)), best], 2, best)
        owner = Vs[np.arange(len(V)), best]
    owner = np.where(mapped, owner, len(X))
    y = image_of(X)
    m = None if tgt_normals is None else image_of(np.asarray(tgt_normals, dtype=np.float64))
    return y, m, owner, mapped


def distortion(src_pts, src_faces, tgt_pts, map_vertices, map_weights=None, tgt_normals=None):
    """Every output of `pf_map_distortion` under the names of `_hip.Context.map_distortion`, as a dict."""
    P = np.ascontiguousarray(src_pts, dtype=np.float64)
    F = np.asarray(src_faces, dtype=np.int64)
    n, T, n_t = len(P), len(F), len(tgt_pts)
    y, m, owner, mapped = images(tgt_pts, map_vertices, map_weights, tgt_normals)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        u, w = P[F[:, 1]] - P[F[:, 0]], P[F[:, 2]] - P[F[:, 0]]
        U, W = y[F[:, 1]] - y[F[:, 0]], y[F[:, 2]] - y[F[:, 0]]
        cs, ci = _cross(u, w), _cross(U, W)
        a_s, a_i = np.sqrt(_dot(cs, cs)), np.sqrt(_dot(ci, ci))
        area = (a_s > 0.0) & np.isfinite(a_s)
        hs = np.where(area, a_s / 2.0, 0.0)
        all_mapped = mapped[F[:, 0]] & mapped[F[:, 1]] & mapped[F[:, 2]]
        valid = area & all_mapped
        collapsed = valid & (a_i == 0.0)
        regular = valid & ~collapsed
        E, Fm, G = _dot(u, u), _dot(u, w), _dot(w, w)
        Ei, Fi, Gi = _dot(U, U), _dot(U, W), _dot(W, W)
        num = (G * Ei - (2.0 * Fm) * Fi) + E * Gi
        s1_collapsed = np.sqrt(np.where(num < 0.0, 0.0, num) / (a_s * a_s))
        l, li = np.sqrt(E), np.sqrt(Ei)
        p = li / l
        q = ((Fi * l) / li - (li * Fm) / l) / a_s
        s = (a_i * l) / (li * a_s)
        hp, hm, hq = (p + s) / 2.0, (p - s) / 2.0, q / 2.0
        Q, R = np.sqrt(hp * hp + hq * hq), np.sqrt(hm * hm + hq * hq)
        s1 = np.where(regular, Q + R, np.where(collapsed, s1_collapsed, 0.0))
        s2 = np.where(regular, np.abs(Q - R), 0.0)
        ratio = np.where(regular, a_i / a_s, 0.0)
        flipped = np.zeros(T, dtype=bool)
        if m is not None:
            ms = (m[F[:, 0]] + m[F[:, 1]]) + m[F[:, 2]]
            flipped = regular & (_dot(ci, ms) < 0.0)
        half_image = a_i / 2.0
    flags = (valid * VALID + collapsed * COLLAPSED + flipped * FLIPPED + (~all_mapped) * UNMAPPED).astype(np.uint8)
    terms = [np.where(valid, hs, 0.0), np.where(valid, half_image, 0.0), np.where(valid, hs * (s1 * s1 + s2 * s2), 0.0),
             np.where(valid, hs * s1, 0.0), np.where(valid, hs * s2, 0.0), np.where(collapsed, hs, 0.0), np.where(flipped, hs, 0.0)]
    totals = np.array([tree_sum(t) for t in terms] + [0.0])
    totals[2] = 0.5 * totals[2]

    # per vertex: the half-edges h = 3 t + j that leave it, in ascending h
    src = F.ravel()
    tri = np.arange(3 * T) // 3
    A = np.bincount(src, weights=hs[tri], minlength=n) / 3.0
    wsum = np.bincount(src, weights=np.where(valid, hs, 0.0)[tri], minlength=n)
    n1 = np.bincount(src, weights=np.where(valid, hs * s1, 0.0)[tri], minlength=n)
    n2 = np.bincount(src, weights=np.where(valid, hs * s2, 0.0)[tri], minlength=n)
    have = wsum > 0.0
    safe = np.where(have, wsum, 1.0)
    vsigma = np.stack([np.where(have, n1 / safe, 0.0), np.where(have, n2 / safe, 0.0)], axis=1)
    vflags = np.zeros(n, dtype=np.uint8)
    np.bitwise_or.at(vflags, src, flags[tri])

    # coverage: the source vertices sorted by owner, stable
    order = np.argsort(owner, kind="stable")
    count = np.bincount(owner, minlength=n_t + 1)[:n_t]
    start = np.concatenate([[0], np.cumsum(count)])[:-1]
    premass = _two_level(np.where(A > 0.0, A, 0.0), order, start, count)
    has_normals = tgt_normals is not None
    report = np.array([valid.sum(), collapsed.sum(), flipped.sum() if has_normals else -1, T - valid.sum(), (~all_mapped).sum(),
                       (count > 0).sum(), count.max(), ((vflags & FLIPPED) != 0).sum() if has_normals else -1], dtype=np.int64)
    return {"face_sigma": np.stack([s1, s2], axis=1), "face_area_ratio": ratio, "face_flags": flags,
            "vertex_area": np.where(A > 0.0, A, 0.0), "vertex_sigma": vsigma, "vertex_flags": vflags,
            "target_count": count.astype(np.int32), "target_premass": premass, "totals": totals, "report": report}


FLOAT_FIELDS = ("face_sigma", "face_area_ratio", "vertex_area", "vertex_sigma", "target_premass", "totals")
INT_FIELDS = ("face_flags", "vertex_flags", "target_count", "report")


def vectorised(src_pts, src_faces, tgt_pts, vertex_map):
    """What a numpy user would write for a vertex map (np.cross, np.linalg.norm, np.bincount, np.sum): the same quantities
    without the fixed orders, for the timing beside the device (not a reference of the bits)."""
    P, F, y = np.asarray(src_pts), np.asarray(src_faces), np.asarray(tgt_pts)[np.asarray(vertex_map)]
    u, w, U, W = P[F[:, 1]] - P[F[:, 0]], P[F[:, 2]] - P[F[:, 0]], y[F[:, 1]] - y[F[:, 0]], y[F[:, 2]] - y[F[:, 0]]
    a_s, a_i = np.linalg.norm(np.cross(u, w), axis=1), np.linalg.norm(np.cross(U, W), axis=1)
    E, Fm, G = np.sum(u * u, 1), np.sum(u * w, 1), np.sum(w * w, 1)
    Ei, Fi, Gi = np.sum(U * U, 1), np.sum(U * W, 1), np.sum(W * W, 1)
    with np.errstate(invalid="ignore", divide="ignore"):
        trace = (G * Ei - 2.0 * Fm * Fi + E * Gi) / (a_s * a_s)  # sigma1^2 + sigma2^2
        det = a_i / a_s
        disc = np.sqrt(np.maximum(trace * trace - 4.0 * det * det, 0.0))
        s1, s2 = np.sqrt((trace + disc) / 2.0), np.sqrt(np.maximum(trace - disc, 0.0) / 2.0)
    hs = a_s / 2.0
    src = F.ravel()
    wsum = np.bincount(src, weights=np.repeat(hs, 3), minlength=len(P))
    v1 = np.bincount(src, weights=np.repeat(hs * s1, 3), minlength=len(P)) / wsum
    v2 = np.bincount(src, weights=np.repeat(hs * s2, 3), minlength=len(P)) / wsum
    count = np.bincount(vertex_map, minlength=len(tgt_pts))
    premass = np.bincount(vertex_map, weights=wsum / 3.0, minlength=len(tgt_pts))
    return s1, s2, det, v1, v2, count, premass, np.array([hs.sum(), a_i.sum() / 2.0, 0.5 * np.sum(hs * trace)])


# ---- the independent check ------------------------------------------------------------------------------------------
def _frame_coordinates(a, b):
    """The 2 x 2 coordinates [[a . e1, b . e1], [a . e2, b . e2]] of the edge vectors a, b (T, 3) in an orthonormal frame
    of their plane: e1 along the longer of the two, e2 = n x e1 with n the unit normal a x b.  Where the two are parallel up
    to rounding (|a x b| <= 1e-14 |a| |b|: there is no plane, and a normalised remainder would be noise) e2 is zero."""
    la, lb = np.linalg.norm(a, axis=1), np.linalg.norm(b, axis=1)
    first = np.where((la >= lb)[:, None], a, b)
    normal = np.cross(a, b)
    ln = np.linalg.norm(normal, axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        e1 = np.where((np.maximum(la, lb) > 0.0)[:, None], first / np.maximum(la, lb)[:, None], 0.0)
        plane = ln > 1e-14 * la * lb
        e2 = np.where(plane[:, None], np.cross(normal / ln[:, None], e1), 0.0)
    M = np.zeros((len(a), 2, 2))
    M[:, 0, 0], M[:, 0, 1] = np.sum(a * e1, axis=1), np.sum(b * e1, axis=1)
    M[:, 1, 0], M[:, 1, 1] = np.sum(a * e2, axis=1), np.sum(b * e2, axis=1)
    return M


def svd_sigmas(src_pts, src_faces, image_pts):
    """(T, 2) singular values, descending, of the Jacobian of every face onto its image by `numpy.linalg.svd`: J = B A^-1
    with A, B the 2 x 2 coordinates of the source and image edge vectors in orthonormal frames of their own planes.  A
    face without source area gives NaN."""
    P, F, y = np.asarray(src_pts, dtype=np.float64), np.asarray(src_faces, dtype=np.int64), np.asarray(image_pts, dtype=np.float64)
    A = _frame_coordinates(P[F[:, 1]] - P[F[:, 0]], P[F[:, 2]] - P[F[:, 0]])
    B = _frame_coordinates(y[F[:, 1]] - y[F[:, 0]], y[F[:, 2]] - y[F[:, 0]])
    out = np.full((len(F), 2), np.nan)
    ok = np.abs(np.linalg.det(A)) > 0.0
    out[ok] = np.linalg.svd(B[ok] @ np.linalg.inv(A[ok]), compute_uv=False)
    return out


# ---- meshes and maps -------------------------------------------------------------------------------------------------
def nearest_vertex_map(src_pts, tgt_pts, chunk=2048):
    """(n,) int64: the nearest target vertex of every source vertex by brute force, the lowest index on ties."""
    S, X = np.asarray(src_pts, dtype=np.float64), np.asarray(tgt_pts, dtype=np.float64)
    out = np.empty(len(S), dtype=np.int64)
    for lo in range(0, len(S), chunk):
        d = S[lo:lo + chunk, None, :] - X[None, :, :]
        out[lo:lo + chunk] = np.argmin((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2], axis=1)
    return out


def closest_on_surface(queries, tgt_pts, tgt_faces):
    """(vertices (q, 3) int32, bary (q, 3)) of the closest point of the triangle surface for every query, by brute force
    over every triangle (the region tests of Ericson, Real-Time Collision Detection 5.1.5)."""
    p = np.asarray(queries, dtype=np.float64)[:, None, :]
    X, F = np.asarray(tgt_pts, dtype=np.float64), np.asarray(tgt_faces, dtype=np.int64)
    a, b, c = X[F[:, 0]][None], X[F[:, 1]][None], X[F[:, 2]][None]
    ab, ac = b - a, c - a
    d1, d2 = np.sum(ab * (p - a), -1), np.sum(ac * (p - a), -1)
    d3, d4 = np.sum(ab * (p - b), -1), np.sum(ac * (p - b), -1)
    d5, d6 = np.sum(ab * (p - c), -1), np.sum(ac * (p - c), -1)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    zero, one = np.zeros_like(d1), np.ones_like(d1)
    with np.errstate(invalid="ignore", divide="ignore"):
        t_ab, t_ac, t_bc = d1 / (d1 - d3), d2 / (d2 - d6), (d4 - d3) / ((d4 - d3) + (d5 - d6))
        v_in, w_in = vb / (va + vb + vc), vc / (va + vb + vc)
    regions = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6),
               (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0)]
    w_b = np.select(regions, [zero, one, t_ab, zero, zero, 1.0 - t_bc], default=v_in)
    w_c = np.select(regions, [zero, zero, zero, one, t_ac, t_bc], default=w_in)
    bary = np.stack([1.0 - w_b - w_c, w_b, w_c], axis=-1)
    point = bary[..., 0:1] * a + bary[..., 1:2] * b + bary[..., 2:3] * c
    best = np.argmin(np.sum((p - point) ** 2, -1), axis=1)
    rows = np.arange(len(best))
    return F[best].astype(np.int32), np.ascontiguousarray(bary[rows, best])


def partial_surface_map(src_pts, tgt_pts, tgt_faces, n_mapped=200):
    """A 3-corner map of the n_mapped source vertices with the largest z (a cap: most of their faces are wholly mapped);
    every other row is (-1, -1, -1) with NaN weights, as `closest_points_on_embedded_surface` leaves a missing row."""
    S = np.asarray(src_pts, dtype=np.float64)
    chosen = np.sort(np.argsort(-S[:, 2], kind="stable")[:n_mapped])
    vertices = np.full((len(S), 3), -1, dtype=np.int32)
    bary = np.full((len(S), 3), np.nan)
    vertices[chosen], bary[chosen] = closest_on_surface(S[chosen], tgt_pts, tgt_faces)
    return vertices, bary


def mirrored(points, faces):
    """The mesh mirrored in the plane x = 0 with every face reversed, so that an outward mesh is outward again."""
    return np.asarray(points) * np.array([-1.0, 1.0, 1.0]), np.ascontiguousarray(np.asarray(faces)[:, ::-1])


def rotation(axis=(1.0, 2.0, 3.0), angle=0.7):
    """A rotation matrix (Rodrigues)."""
    k = np.asarray(axis, dtype=np.float64) / np.linalg.norm(axis)
    K = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    return np.eye(3) + np.sin(angle) * K + (1.0 - np.cos(angle)) * (K @ K)
