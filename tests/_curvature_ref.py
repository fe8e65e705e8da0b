"""Numpy reference of the discrete curvatures (tests/test_curvature.py, tools/bench_curvature.py), written from the
definitions in include/pyfocusr_hip.h, and the small meshes the tests measure them on.

Half-edge h = 3 t + j leaves corner j of triangle t.  Every per-vertex sum is an `np.bincount` over the half-edges in
ascending h, which adds in that order: the order of the device.  Products and sums are written out one operation at a
time (numpy contracts nothing), dot products left to right.  Only atan2, sin and cos are libm's here and the device's
there, so the device is compared with a tolerance relative to what was summed; `curvatures` returns those magnitudes."""
import numpy as np

TWO_PI = 6.283185307179586


def _dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def _sign_rule(d):
    """Rows of d with their largest-|component| entry positive (lowest index on ties)."""
    lead = d[np.arange(len(d)), np.argmax(np.abs(d), axis=1)]
    return np.where((lead < 0.0)[:, None], -d, d)


def curvatures(points, faces):
    """Every field of `pyfocusr_amd.discrete_curvatures` as a dict, plus the magnitudes the device is compared against:
    `mag_gauss` = sum of angles / A, `mag_mean` = sum |e| |beta| / A, `mag_s` = the Frobenius norm of the 2 x 2 tensor S."""
    P = np.ascontiguousarray(points, dtype=np.float64)
    F = np.asarray(faces, dtype=np.int64)
    n, m = len(P), len(F)
    X = P[F]  # (m, 3 corners, 3)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        cr = _cross(X[:, 1] - X[:, 0], X[:, 2] - X[:, 0])
        ln = np.sqrt(_dot(cr, cr))
        ok = (ln > 0.0) & np.isfinite(ln)
        tn = np.where(ok[:, None], cr / ln[:, None], 0.0)
        area = np.where(ok, ln / 2.0, 0.0)
        ang = np.zeros((m, 3))
        for j in range(3):
            e1, e2 = X[:, (j + 1) % 3] - X[:, j], X[:, (j + 2) % 3] - X[:, j]
            c = _cross(e1, e2)
            ang[:, j] = np.where(ok, np.arctan2(np.sqrt(_dot(c, c)), _dot(e1, e2)), 0.0)
    src, dst = F.ravel(), F[:, [1, 2, 0]].ravel()  # half-edge h = 3 t + j: corner j -> corner j + 1
    tri = np.arange(3 * m) // 3

    # edges: runs of equal keys in ascending h
    key = np.minimum(src, dst) * n + np.maximum(src, dst)
    order = np.argsort(key, kind="stable")
    first = np.flatnonzero(np.r_[True, key[order][1:] != key[order][:-1]])
    count = np.diff(np.r_[first, 3 * m])
    two = first[count == 2]
    h0, h1 = order[two], order[two + 1]
    inconsistent = (src[h0] < dst[h0]) == (src[h1] < dst[h1])
    wb, ev = np.zeros(3 * m), np.zeros((3 * m, 3))
    d = P[dst[h0]] - P[src[h0]]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        length = np.sqrt(_dot(d, d))
        valid = ~inconsistent & (area[tri[h0]] > 0.0) & (area[tri[h1]] > 0.0) & (length > 0.0) & np.isfinite(length)
        e = np.where(valid[:, None], d / length[:, None], 0.0)
        nf, ng = tn[tri[h0]], tn[tri[h1]]
        beta = np.where(valid, np.arctan2(_dot(_cross(nf, ng), e), _dot(nf, ng)), 0.0)
        w = np.where(valid, length * beta, 0.0)
    wb[h0], wb[h1] = w, w
    ev[h0], ev[h1] = e, e
    single = np.zeros(3 * m, dtype=bool)
    single[order[first[count == 1]]] = True
    boundary = np.zeros(n, dtype=bool)
    boundary[src[single]] = True
    boundary[dst[single]] = True

    def vsum(x):
        return np.bincount(src, weights=x, minlength=n)

    A = vsum(area[tri]) / 3.0
    angsum, hsum, habs = vsum(ang.ravel()), vsum(wb), vsum(np.abs(wb))
    ns = np.stack([vsum(ang.ravel() * tn[tri, a]) for a in range(3)], axis=1)
    c = 0.5 * wb
    T = np.stack([vsum((c * ev[:, a]) * ev[:, b]) for a, b in ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))], axis=1)
    Tabs = np.stack([vsum(np.abs((c * ev[:, a]) * ev[:, b])) for a, b in ((0, 0), (1, 1), (2, 2))], axis=1)
    have = A > 0.0
    Asafe = np.where(have, A, 1.0)
    K = np.where(have, (TWO_PI - angsum) / Asafe, 0.0)
    H = np.where(have, hsum / (4.0 * Asafe), 0.0)
    T = np.where(have[:, None], T / Asafe[:, None], 0.0)
    disc = H * H - K
    clipped = have & (disc < 0.0)
    s = np.sqrt(np.where(disc < 0.0, 0.0, disc))
    k_min, k_max = np.where(have, H - s, 0.0), np.where(have, H + s, 0.0)

    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        nl = np.sqrt(_dot(ns, ns))
        framed = have & (nl > 0.0) & np.isfinite(nl)
        nv = np.where(framed[:, None], ns / np.where(framed, nl, 1.0)[:, None], 0.0)
    ax = np.argmin(np.abs(nv), axis=1)  # the first of equal minima
    unit = np.eye(3)[ax]
    na = nv[np.arange(n), ax]
    t1 = unit - na[:, None] * nv
    t1 = t1 / np.where(framed, np.sqrt(_dot(t1, t1)), 1.0)[:, None]
    t2 = _cross(nv, t1)

    def apply(t):
        return np.stack([T[:, 0] * t[:, 0] + T[:, 3] * t[:, 1] + T[:, 4] * t[:, 2], T[:, 3] * t[:, 0] + T[:, 1] * t[:, 1] + T[:, 5] * t[:, 2],
                         T[:, 4] * t[:, 0] + T[:, 5] * t[:, 1] + T[:, 2] * t[:, 2]], axis=1)

    Tt1, Tt2 = apply(t1), apply(t2)
    s11, s12, s22 = _dot(t1, Tt1), _dot(t2, Tt1), _dot(t2, Tt2)
    mid, dif = (s11 + s22) / 2.0, (s11 - s22) / 2.0
    r = np.sqrt(dif * dif + s12 * s12)
    theta = 0.5 * np.arctan2(2.0 * s12, s11 - s22)
    wv = np.cos(theta)[:, None] * t1 + np.sin(theta)[:, None] * t2
    d_min = np.where(framed[:, None], _sign_rule(wv), 0.0)
    d_max = np.where(framed[:, None], _sign_rule(_cross(nv, wv)), 0.0)
    topology = np.array([len(first), int(np.sum(count == 1)), int(np.sum(count >= 3)), int(np.sum(inconsistent)),
                         int(np.sum(clipped))], dtype=np.int64)
    return dict(area=np.where(have, A, 0.0), gaussian=K, mean=H, k_min=k_min, k_max=k_max, tensor=T,
                tensor_k_min=np.where(framed, mid - r, 0.0), tensor_k_max=np.where(framed, mid + r, 0.0), d_min=d_min, d_max=d_max,
                normals=nv, boundary=boundary, topology=topology,
                mag_gauss=np.where(have, angsum / Asafe, 0.0), mag_mean=np.where(have, habs / Asafe, 0.0),
                mag_s=np.where(framed, np.sqrt(s11 * s11 + 2.0 * (s12 * s12) + s22 * s22), 0.0),
                trace_terms=np.where(have, np.sum(Tabs, axis=1) / Asafe, 0.0), n_faces=m)


def _ratio(got, want, magnitude):
    """max over the vertices of |got - want| / magnitude; 0 / 0 counts as 0, anything else over 0 as inf."""
    err = np.abs(got - want)
    if err.ndim == 2:
        err = err.max(axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        q = np.where(err == 0.0, 0.0, err / magnitude)
    return float(np.max(q)) if len(q) else 0.0


def ratios(dev, r):
    """The worst ratio per field between a device result `dev` and the reference `r` of `curvatures`: the quantities the
    GPU tests bound (profiles/curvature.md)."""
    return {"area": _ratio(dev["area"], r["area"], r["area"]),
            "normals": _ratio(dev["normals"], r["normals"], np.ones(len(r["area"]))),
            "gaussian": _ratio(dev["gaussian"], r["gaussian"], r["mag_gauss"]),
            "mean": _ratio(dev["mean"], r["mean"], r["mag_mean"]),
            "tensor": _ratio(dev["tensor"], r["tensor"], r["mag_mean"]),
            "tensor_k": max(_ratio(dev["tensor_k_min"], r["tensor_k_min"], r["mag_s"]),
                            _ratio(dev["tensor_k_max"], r["tensor_k_max"], r["mag_s"]))}


# ---- meshes --------------------------------------------------------------------------------------------------------
def tetrahedron():
    """The regular tetrahedron on four corners of the cube [-1, 1]^3, outward."""
    pts = np.array([[1.0, 1.0, 1.0], [1.0, -1.0, -1.0], [-1.0, 1.0, -1.0], [-1.0, -1.0, 1.0]])
    faces = np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]], dtype=np.int32)
    return pts, faces


def cube26():
    """The unit cube [0, 1]^3 with 26 vertices: every face is 2 x 2 quads of side 1/2, each split into two triangles,
    outward.  Returns (points, faces, kind) with kind[v] = how many coordinates of v are 0 or 1: 3 corner, 2 edge
    midpoint, 1 face centre."""
    grid = [(i, j, k) for i in range(3) for j in range(3) for k in range(3) if (i, j, k) != (1, 1, 1)]
    index = {p: v for v, p in enumerate(grid)}
    pts = np.array(grid, dtype=np.float64) / 2.0
    faces = []
    for axis in range(3):
        u, w = (axis + 1) % 3, (axis + 2) % 3  # e_u x e_w = e_axis
        for side in (0, 2):
            for a in range(2):
                for b in range(2):
                    def at(da, db):
                        p = [0, 0, 0]
                        p[axis], p[u], p[w] = side, a + da, b + db
                        return index[tuple(p)]
                    quad = [at(0, 0), at(1, 0), at(1, 1), at(0, 1)]  # counter-clockwise seen from +axis
                    if side == 0:
                        quad = quad[::-1]
                    faces += [[quad[0], quad[1], quad[2]], [quad[0], quad[2], quad[3]]]
    kind = np.sum((pts == 0.0) | (pts == 1.0), axis=1)
    return pts, np.array(faces, dtype=np.int32), kind


def open_cylinder(radius=1.5, n_around=48, n_along=20, height=4.0):
    """An open cylinder around the z axis, n_around x n_along vertices, outward; vertex = ring * n_around + position."""
    phi = 2.0 * np.pi * np.arange(n_around) / n_around
    z = height * np.arange(n_along) / (n_along - 1)
    pts = np.stack([np.tile(radius * np.cos(phi), n_along), np.tile(radius * np.sin(phi), n_along), np.repeat(z, n_around)], axis=1)
    faces = []
    for r in range(n_along - 1):
        for p in range(n_around):
            a, b = r * n_around + p, r * n_around + (p + 1) % n_around
            c, d = a + n_around, b + n_around
            faces += [[a, b, d], [a, d, c]]
    return pts, np.array(faces, dtype=np.int32)


def cone_fan(n_tri=200, height=1.0):
    """A closed fan of n_tri triangles around an apex (vertex 0) over a unit circle: one long vertex run, an open rim."""
    phi = 2.0 * np.pi * np.arange(n_tri) / n_tri
    pts = np.concatenate([[[0.0, 0.0, height]], np.stack([np.cos(phi), np.sin(phi), np.zeros(n_tri)], axis=1)])
    ring = 1 + np.arange(n_tri)
    faces = np.stack([np.zeros(n_tri, dtype=np.int64), ring, np.roll(ring, -1)], axis=1)
    return pts, faces.astype(np.int32)


def with_zero_area_triangle(points, faces):
    """The mesh with a new vertex at the very position of corner b of face 0 = (a, b, c): face 0 becomes (a, new, c), and
    the triangle (a, b, new), whose area is exactly zero (two corners coincide), fills the slit along the edge (a, b).
    The edges (b, new), (new, c) and (b, c) are left with one triangle each."""
    a, b, c = (int(v) for v in faces[0])
    new = len(points)
    pts = np.concatenate([points, [points[b]]])
    extra = [[a, new, c], [a, b, new]]
    return pts, np.concatenate([extra, faces[1:]]).astype(np.int32)
