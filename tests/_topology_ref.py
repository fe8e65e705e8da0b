"""Numpy / scipy reference of the mesh topology (tests/test_topology.py, tools/bench_topology.py), written from the
definitions in include/pyfocusr_hip.h, and the small meshes the tests use.

Half-edge h = 3 t + j leaves corner j of face t for corner (j + 1) % 3.  Everything is an integer but the signed volume,
which is summed exactly (`math.fsum`) so that the only rounding in a comparison is the device's.  The patches are scipy's
connected components of the faces joined across two-face edges; the parities come from the components of the double
cover (nodes (t, s), an edge of parity p joins (a, s) with (b, s ^ p)): a patch is orientable when (root, 0) and (root, 1)
lie in different components, and rel[t] says in which of the two t's sheet 0 lies."""
import math

import numpy as np
from scipy import sparse
from scipy.sparse.csgraph import connected_components


def _components(n_nodes, a, b):
    g = sparse.coo_matrix((np.ones(len(a), dtype=np.int8), (a, b)), shape=(n_nodes, n_nodes)).tocsr()
    return connected_components(g, directed=False)[1]


def _ascending_ids(labels):
    """labels renumbered 0, 1, ... in the order of their first occurrence."""
    _, first, inverse = np.unique(labels, return_index=True, return_inverse=True)
    rank = np.empty(len(first), dtype=np.int64)
    rank[np.argsort(first, kind="stable")] = np.arange(len(first))
    return rank[inverse.ravel()]


def topology(n_points, faces, points=None, outward=True):
    """Every output of `pf_mesh_topology` and every field of `pyfocusr_amd.mesh_topology`, as a dict; `volume_terms`
    (P,) is sum |a . (b x c)| / 6 of each patch, the magnitude a device volume is compared against."""
    F = np.asarray(faces, dtype=np.int64)
    n, m = int(n_points), len(F)
    src, dst = F.ravel(), F[:, [1, 2, 0]].ravel()
    tri = np.arange(3 * m) // 3
    key = np.minimum(src, dst) * n + np.maximum(src, dst)
    order = np.argsort(key, kind="stable")  # the half-edges of an edge in ascending h
    first = np.flatnonzero(np.r_[True, key[order][1:] != key[order][:-1]])
    count = np.diff(np.r_[first, 3 * m])
    per_half = np.repeat(count, count)  # the size of the run each sorted position lies in
    nbr = np.zeros(3 * m, dtype=np.int64)
    nbr[order[per_half == 1]] = -1
    nbr[order[per_half >= 3]] = -2
    two = first[count == 2]
    h0, h1 = order[two], order[two + 1]
    nbr[h0], nbr[h1] = tri[h1], tri[h0]
    p = ((src[h0] < dst[h0]) == (src[h1] < dst[h1])).astype(np.int64)
    a, b = tri[h0], tri[h1]

    patch = _ascending_ids(_components(m, a, b))
    P = int(patch.max()) + 1
    root = np.full(P, m, dtype=np.int64)
    np.minimum.at(root, patch, np.arange(m))
    cover = _components(2 * m, np.r_[2 * a, 2 * a + 1], np.r_[2 * b + p, 2 * b + (1 - p)])
    orientable = cover[2 * root] != cover[2 * root + 1]
    rel = (cover[2 * np.arange(m)] != cover[2 * root[patch]]).astype(np.int64)
    n_faces = np.bincount(patch, minlength=P)
    n_rel = np.bincount(patch, weights=rel, minlength=P).astype(np.int64)
    inv = 2 * n_rel > n_faces
    flip = orientable[patch] & ((rel ^ inv[patch]) == 1)
    open_face = (nbr.reshape(m, 3) < 0).any(axis=1)
    closed = np.bincount(patch, weights=open_face, minlength=P) == 0
    manifold = np.bincount(patch, weights=(nbr.reshape(m, 3) == -2).any(axis=1), minlength=P) == 0

    volume, volume_terms = np.zeros(P), np.zeros(P)
    if outward and points is not None:
        X = np.ascontiguousarray(points, dtype=np.float64)
        for k in np.flatnonzero(closed & orientable):
            fs = np.flatnonzero(patch == k)
            f = F[fs].copy()
            f[flip[fs]] = f[flip[fs]][:, [0, 2, 1]]
            A, B, C = X[f[:, 0]], X[f[:, 1]], X[f[:, 2]]
            cr = np.stack([B[:, 1] * C[:, 2] - B[:, 2] * C[:, 1], B[:, 2] * C[:, 0] - B[:, 0] * C[:, 2],
                           B[:, 0] * C[:, 1] - B[:, 1] * C[:, 0]], axis=1)
            terms = A[:, 0] * cr[:, 0] + A[:, 1] * cr[:, 1] + A[:, 2] * cr[:, 2]
            v = math.fsum(terms) / 6.0
            volume_terms[k] = math.fsum(np.abs(terms)) / 6.0
            if v < 0.0:
                v = -v
                flip[fs] = ~flip[fs]
            volume[k] = v

    # boundary loops: the boundary half-edges of a patch and their (patch, vertex) ends as the nodes of one graph
    bh = np.flatnonzero(nbr == -1)
    loop = np.full(3 * m, -1, dtype=np.int64)
    if len(bh):
        ends = np.r_[patch[tri[bh]] * n + src[bh], patch[tri[bh]] * n + dst[bh]]
        _, end_id = np.unique(ends, return_inverse=True)
        lab = _components(len(bh) + int(end_id.max()) + 1, np.r_[np.arange(len(bh)), np.arange(len(bh))], len(bh) + end_id.ravel())
        loop[bh] = _ascending_ids(lab[:len(bh)])
    B = int(loop.max()) + 1

    table = {key_: np.zeros(P, dtype=np.int64) for key_ in ("n_vertices", "n_edges", "n_boundary_loops", "euler", "genus", "n_flipped")}
    for k in range(P):
        fs = np.flatnonzero(patch == k)
        pairs = np.sort(np.stack([F[fs].ravel(), F[fs][:, [1, 2, 0]].ravel()], axis=1), axis=1)
        loops = loop.reshape(m, 3)[fs]
        table["n_vertices"][k] = len(np.unique(F[fs]))
        table["n_edges"][k] = len(np.unique(pairs, axis=0))
        table["n_boundary_loops"][k] = len(np.unique(loops[loops >= 0]))
        table["euler"][k] = table["n_vertices"][k] - table["n_edges"][k] + len(fs)
        table["genus"][k] = (2 - table["euler"][k] - table["n_boundary_loops"][k]) // 2 if orientable[k] and manifold[k] else -1
        table["n_flipped"][k] = int(np.sum(flip[fs]))
    table.update(n_faces=n_faces, closed=closed, orientable=orientable, manifold=manifold, signed_volume=volume)
    return dict(n_edges=len(first), n_boundary_edges=int(np.sum(count == 1)), n_nonmanifold_edges=int(np.sum(count >= 3)),
                n_inconsistent_edges=int(np.sum(p)), face_neighbours=nbr.reshape(m, 3).astype(np.int32), patch=patch.astype(np.int32),
                flip=flip, boundary_loop=loop.reshape(m, 3).astype(np.int32), n_patches=P, n_boundary_loops=B, patches=table,
                volume_terms=volume_terms)


def as_device_output(r):
    """The dict `_hip.Context.mesh_topology` would have returned for the reference result `r`."""
    report = np.array([r["n_edges"], r["n_boundary_edges"], r["n_nonmanifold_edges"], r["n_inconsistent_edges"], r["n_patches"],
                       r["n_boundary_loops"], 0, 0], dtype=np.int64)
    return {"face_neighbours": r["face_neighbours"], "patch": r["patch"], "flip": r["flip"].copy(), "boundary_loop": r["boundary_loop"],
            "patch_orientable": r["patches"]["orientable"].copy(), "patch_volume": r["patches"]["signed_volume"].copy(),
            "report": report, "device_ms": 0.0}


# ---- meshes --------------------------------------------------------------------------------------------------------
def reverse(faces, which):
    out = np.array(faces, dtype=np.int32)
    out[which] = out[which][:, [0, 2, 1]]
    return out


def tetrahedron():
    pts = np.array([[1.0, 1.0, 1.0], [1.0, -1.0, -1.0], [-1.0, 1.0, -1.0], [-1.0, -1.0, 1.0]])
    return pts, np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]], dtype=np.int32)


def cube():
    """The unit cube, 8 vertices (vertex = 4 x + 2 y + z), 12 triangles, outward."""
    pts = np.array([[x, y, z] for x in (0.0, 1.0) for y in (0.0, 1.0) for z in (0.0, 1.0)])
    quads = [[0, 1, 3, 2], [4, 6, 7, 5], [0, 4, 5, 1], [2, 3, 7, 6], [0, 2, 6, 4], [1, 5, 7, 3]]
    faces = [t for q in quads for t in ([q[0], q[1], q[2]], [q[0], q[2], q[3]])]
    return pts, np.array(faces, dtype=np.int32)


def torus_grid(n_u=8, n_v=8, R=3.0, r=1.0):
    """A torus of n_u x n_v quads, two triangles each, outward; vertex = i * n_v + j."""
    u, v = np.meshgrid(2.0 * np.pi * np.arange(n_u) / n_u, 2.0 * np.pi * np.arange(n_v) / n_v, indexing="ij")
    pts = np.stack([(R + r * np.cos(v)) * np.cos(u), (R + r * np.cos(v)) * np.sin(u), r * np.sin(v)], axis=-1).reshape(-1, 3)
    faces = []
    for i in range(n_u):
        for j in range(n_v):
            a, b = i * n_v + j, ((i + 1) % n_u) * n_v + j
            c, d = ((i + 1) % n_u) * n_v + (j + 1) % n_v, i * n_v + (j + 1) % n_v
            faces += [[a, b, c], [a, c, d]]
    return pts, np.array(faces, dtype=np.int32)


def open_cylinder(n_around=12, n_along=4):
    phi = 2.0 * np.pi * np.arange(n_around) / n_around
    pts = np.stack([np.tile(np.cos(phi), n_along), np.tile(np.sin(phi), n_along), np.repeat(np.arange(n_along, dtype=np.float64), n_around)],
                   axis=1)
    faces = []
    for r in range(n_along - 1):
        for q in range(n_around):
            a, b = r * n_around + q, r * n_around + (q + 1) % n_around
            faces += [[a, b, b + n_around], [a, b + n_around, a + n_around]]
    return pts, np.array(faces, dtype=np.int32)


def moebius(n_quads=12):
    """A Moebius strip of 2 n_quads triangles: columns (top i, bottom i) = (2 i, 2 i + 1), the last quad joins column
    n_quads - 1 to column 0 upside down."""
    phi = 2.0 * np.pi * np.arange(n_quads) / n_quads
    pts = []
    for i in range(n_quads):
        for s in (0.4, -0.4):
            rad = 2.0 + s * np.cos(phi[i] / 2.0)
            pts.append([rad * np.cos(phi[i]), rad * np.sin(phi[i]), s * np.sin(phi[i] / 2.0)])
    faces = []
    for i in range(n_quads):
        t0, b0 = 2 * i, 2 * i + 1
        t1, b1 = (2 * i + 2, 2 * i + 3) if i + 1 < n_quads else (1, 0)
        faces += [[t0, b0, b1], [t0, b1, t1]]
    return np.array(pts), np.array(faces, dtype=np.int32)


def nested_spheres():
    """Two blobs around the origin, the inner one (a quarter of the size) with every face reversed."""
    from pyfocusr_amd.meshgen import blob_mesh

    outer, inner = blob_mesh(60, seed=3), blob_mesh(40, seed=4)
    pts = np.concatenate([outer.points, 0.25 * inner.points])
    faces = np.concatenate([outer.faces, inner.faces[:, [0, 2, 1]] + len(outer.points)])
    return pts, faces.astype(np.int32)


def two_triangles_at_a_vertex():
    pts = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [-1.0, 0.0, 0.0], [0.0, -1.0, 0.0]])
    return pts, np.array([[0, 1, 2], [0, 3, 4]], dtype=np.int32)


def tetrahedron_with_fin():
    """The tetrahedron and a fifth face on its edge (0, 1) to a new vertex."""
    pts, faces = tetrahedron()
    return np.concatenate([pts, [[3.0, 0.0, 0.0]]]), np.concatenate([faces, [[0, 1, 4]]]).astype(np.int32)


def ribbon(n_tri=4096, closed=False):
    """A strip of n_tri triangles in a row, face i on the vertices i, i + 1, i + 2, consistently oriented, then every
    third face reversed; `closed` joins its ends into a band over n_tri vertices (n_tri even: a cylinder).  The face
    graph is a path: the labelling's worst diameter."""
    i = np.arange(n_tri)
    n = n_tri if closed else n_tri + 2
    even = i % 2 == 0
    faces = np.stack([np.where(even, i, i + 1), np.where(even, i + 1, i), i + 2], axis=1) % n
    pts = np.stack([np.cos(2.0 * np.pi * np.arange(n) / n), np.sin(2.0 * np.pi * np.arange(n) / n), 0.1 * (np.arange(n) % 2)], axis=1)
    return pts, reverse(faces, i % 3 == 0)
