"""Hostile inputs for the surface queries - test infrastructure, numpy only (the blob comes from `pyfocusr_amd.meshgen`),
deterministic in a seed.  Used by tests/test_hostile_geometry.py (CPU: the generators and references themselves),
tests/test_surface_hostile.py (the fixed GPU cases) and the sweeps tests/fuzz_surfaces.py, tests/fuzz_surface_nd.py.

A mesh is `(points (n, 3) float64 C-contiguous, faces (F, vpf) int32, tags)`.  `tags` is a dict of what the generator
promises, and the checks (tests/_surface_checks.py) choose their comparisons by it:
  closed_oriented  every fan-triangle edge has exactly two triangles that traverse it in opposite directions, and the faces
                   point outward (the winding number is 1 inside)
  has_degenerate   some fan triangle has zero area exactly (repeated index, points at one position, coincident corners)
  has_slivers      some faces have one edge collapsed to `sliver_rel` x extent (a needle; no two points equal)
  folded           a sliver mesh in which two triangles on an edge have unit normals with a dot product below 0.5 (or not a
                   number), in float64 on the points as they are: a needle of height 1e-13 extents, or any needle once a far
                   frame has rounded its ends, can lie folded back on its neighbour.  Such a mesh intersects itself at
                   rounding scale, and the pseudonormal sign is defined for embedded meshes only: the sign is not compared
  fragile          vertex indices of the slivers / degenerate faces: no ray is aimed at them
  planar_axis      2 when every face lies in a plane z = const, else None
  ray_axis         the axis a along which every ray keeps |d_a| >= 0.1 |d|: the normal of a planar mesh, the squashed axis
                   of an anisotropic one (every normal is within 1e-3 of it); None elsewhere
  coincident       some triangles coincide exactly (d2 ties across triangles and chunks: the lowest index wins)
  frame            (k, s, offset_ratio) once `frame` was applied
`extent` is the longest side of the bounding box of the referenced points."""
import numpy as np

TRIANGLE_COUNTS = (1, 63, 64, 65, 4096, 4097, 4600)  # chunk of 64, super-chunk of 64 chunks, two super-chunks and a ragged chunk
QUERY_COUNTS = (1, 3, 4, 5, 8, 9, 16, 17, 299)         # packets of 4, 8 (winding, nd) and 16; 299 fills none of them
PACKET_SWITCH = (65536, 65537)                        # 16 x 4096: from here a wave takes 16 queries / rays instead of 4
OFFSET_RATIOS = (0.0, 1.0, 1e3, 1e6)


def _tags(**kw):
    t = dict(closed_oriented=False, has_degenerate=False, has_slivers=False, fragile=np.zeros(0, dtype=np.int64),
             folded=False, planar_axis=None, ray_axis=None, coincident=False, frame=None, name="")
    t.update(kw)
    return t


def _mesh(points, faces, tags):
    return np.ascontiguousarray(points, dtype=np.float64), np.ascontiguousarray(faces, dtype=np.int32), tags


def extent(points, faces=None):
    p = points if faces is None else points[np.unique(faces)]
    p = p[np.isfinite(p).all(axis=1)]
    return float(np.max(p.max(axis=0) - p.min(axis=0)))


def diagonal(points, faces=None):
    p = points if faces is None else points[np.unique(faces)]
    return float(np.linalg.norm(p.max(axis=0) - p.min(axis=0)))


# ------------------------------------------------------------------------------------------------ base shapes
def blob(n, seed=0):
    """`blob_mesh(n)`: closed, outward, 2 n - 4 triangles (n = 34: 64, 2050: 4096, 2302: 4600)."""
    from pyfocusr_amd.meshgen import blob_mesh

    m = blob_mesh(n, seed=seed)
    return _mesh(m.points, m.faces, _tags(closed_oriented=True, name="blob%d" % n))


def torus_quads(nu, nv):
    """A torus of nu x nv quads (2 nu nv fan triangles, the quads not planar), closed and consistently oriented."""
    uu, vv = np.meshgrid(np.arange(nu), np.arange(nv), indexing="ij")
    au, av = 2 * np.pi * uu / nu, 2 * np.pi * vv / nv
    pts = np.stack([(3 + np.cos(av)) * np.cos(au), (3 + np.cos(av)) * np.sin(au), np.sin(av)], axis=-1).reshape(-1, 3)
    quads = np.stack([uu * nv + vv, ((uu + 1) % nu) * nv + vv, ((uu + 1) % nu) * nv + (vv + 1) % nv, uu * nv + (vv + 1) % nv], axis=-1)
    return _mesh(pts, quads.reshape(-1, 4), _tags(closed_oriented=True, name="torus%dx%d" % (nu, nv)))


# ------------------------------------------------------------------------------------------------ hostile variants
def folded(points, faces):
    """Whether two fan triangles on an edge have unit normals whose dot product is below 0.5 or not a number."""
    tri = np.stack([faces[:, [0, j + 1, j + 2]] for j in range(faces.shape[1] - 2)], axis=1).reshape(-1, 3).astype(np.int64)
    x = points[tri]
    with np.errstate(all="ignore"):
        n = np.cross(x[:, 1] - x[:, 0], x[:, 2] - x[:, 0])
        n /= np.linalg.norm(n, axis=1, keepdims=True)
    src, dst = tri.ravel(), tri[:, [1, 2, 0]].ravel()
    key = np.minimum(src, dst) * (int(tri.max()) + 1) + np.maximum(src, dst)
    order = np.argsort(key, kind="stable")
    owner = np.repeat(np.arange(len(tri)), 3)[order]
    pair = np.flatnonzero(key[order][1:] == key[order][:-1])
    dots = np.einsum("ij,ij->i", n[owner[pair]], n[owner[pair + 1]])
    return bool(np.any(~(dots >= 0.5)))


def slivers(base, fraction, rel, seed=0):
    """About `fraction` of the faces become needles: for vertex-disjoint edges (u, v) of the first fan triangles, v moves
    along the edge to u + rel x extent x (v - u) / |v - u|: an edge collapse that stops short.  Every face that holds the
    edge collapses; the indices stay, so a closed mesh stays closed.  An edge whose collapse would fold a face of an
    unfolded base over (`folded`) is passed over.  No two points become equal (asserted)."""
    pts, faces, tags = base
    rng = np.random.default_rng(seed)
    pts = pts.copy()
    ext = extent(pts, faces)
    want = max(1, int(round(fraction * len(faces) / 2)))  # an interior edge has two faces
    used = np.zeros(len(pts), dtype=bool)
    moved = []
    check = not folded(pts, np.asarray(faces))
    for f in rng.permutation(len(faces)):
        u, v = int(faces[f, 0]), int(faces[f, 1])
        ring = faces[(faces == u).any(axis=1) | (faces == v).any(axis=1)]
        if used[ring].any():
            continue
        d, old = pts[v] - pts[u], pts[v].copy()
        pts[v] = pts[u] + rel * ext * d / np.linalg.norm(d)
        if check and folded(pts, np.asarray(faces)):  # this collapse would turn a face around v over: another edge
            pts[v] = old
            continue
        used[ring] = True
        moved += [u, v]
        if len(moved) // 2 >= want:
            break
    assert len(np.unique(pts[np.unique(faces)], axis=0)) == len(np.unique(faces))
    t = dict(tags, has_slivers=True, sliver_rel=rel, sliver_edges=np.array(moved, dtype=np.int64).reshape(-1, 2),
             fragile=np.union1d(tags["fragile"], moved), name=tags["name"] + "+slivers%g" % rel)
    t["folded"] = folded(pts, np.asarray(faces))
    return _mesh(pts, faces, t)


def sheets(nx, ny, layers, vpf=3, dz=0):
    """`layers` copies of an nx x ny-cell integer lattice in the planes z = layer x dz, as triangles (vpf 3: all (a, b, c)
    of the cells, then all (a, c, d), layer by layer) or quads (vpf 4).  dz = 0: every layer has its own points at the same
    positions, so triangles coincide exactly, within a chunk and across chunks.  Boxes have zero thickness."""
    i, j = np.meshgrid(np.arange(nx + 1, dtype=np.float64), np.arange(ny + 1, dtype=np.float64), indexing="ij")
    idx = np.arange((nx + 1) * (ny + 1)).reshape(nx + 1, ny + 1)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel(), idx[:-1, 1:].ravel()
    one = np.stack([a, b, c, d], 1) if vpf == 4 else np.concatenate([np.stack([a, b, c], 1), np.stack([a, c, d], 1)])
    n = idx.size
    pts = np.concatenate([np.stack([i.ravel(), j.ravel(), np.full(n, float(l * dz))], axis=1) for l in range(layers)])
    faces = np.concatenate([one + l * n for l in range(layers)])
    return _mesh(pts, faces, _tags(planar_axis=2, ray_axis=2, coincident=layers >= 2 and dz == 0,
                                   name="sheets%dx%dx%d_v%d" % (nx, ny, layers, vpf)))


def soup(n, F, vpf=3, seed=0, n_repeat=None, pile=3):
    """F random faces of vpf corners over n points (N(0, 1) x a random power of ten), plus `pile` more points at the
    position of point 0 and 2 points no face references.  From F = 16 on: min(4, F // 16) faces repeat a vertex, as many
    are copies of face 0, and as many use the pile.  Face 0 always has distinct corners at distinct positions, so
    every finite query has a finite distance.  Few degenerate faces on purpose: the exact ray test may accept a
    zero-area triangle at any distance (its determinant is rounding noise), and such rays are left out of the
    comparison under a cap."""
    rng = np.random.default_rng(seed)
    n = max(n, vpf + 1)
    pts = rng.normal(size=(n, 3)) * 10.0 ** rng.integers(-3, 4)
    pts = np.concatenate([pts, np.tile(pts[0], (pile, 1)), rng.normal(size=(2, 3))])
    faces = rng.integers(0, n, size=(F, vpf))
    for f in range(F):  # distinct corners (a repeated corner is put in below, on purpose and counted)
        while len(set(faces[f])) < vpf:
            faces[f] = rng.integers(0, n, size=vpf)
    k = min(4, F // 16) if n_repeat is None else n_repeat
    fragile = []
    if k:
        rows = 1 + rng.permutation(F - 1)[:3 * k]
        rep, whole, piled = rows[:k], rows[k:2 * k], rows[2 * k:]
        faces[0] = rng.permutation(np.arange(1, n))[:vpf]
        faces[rep, 1] = faces[rep, 0]
        faces[whole] = faces[0]
        faces[piled, 0], faces[piled, 1] = 0, n + np.arange(len(piled)) % pile
        fragile = np.unique(np.concatenate([faces[rep].ravel(), faces[piled].ravel()]))
    return _mesh(pts, faces, _tags(has_degenerate=bool(k), coincident=bool(k), fragile=np.asarray(fragile, dtype=np.int64),
                                   name="soup%d_F%d_v%d" % (n, F, vpf)))


def anisotropic(base, scales=(1.0, 1e-3, 1e3)):
    """Each coordinate by its own scale.  The normals turn towards the most squashed axis (by the inverse scales), so a
    ray across the long axes lies in the plane of nearly every triangle: `ray_axis` keeps the rays off it."""
    pts, faces, tags = base
    return _mesh(pts * np.asarray(scales), faces, dict(tags, ray_axis=int(np.argmin(scales)), name=tags["name"] + "+aniso"))


def _join(a, b, name):
    (pa, fa, ta), (pb, fb, tb) = a, b
    assert fa.shape[1] == fb.shape[1]
    tags = _tags(closed_oriented=ta["closed_oriented"] and tb["closed_oriented"],
                 has_degenerate=ta["has_degenerate"] or tb["has_degenerate"], has_slivers=ta["has_slivers"] or tb["has_slivers"],
                 fragile=np.concatenate([ta["fragile"], tb["fragile"] + len(pa)]), coincident=ta["coincident"] or tb["coincident"],
                 name=name)
    return _mesh(np.concatenate([pa, pb]), np.concatenate([fa, fb + len(pa)]), tags)


def far_parts(base_a, base_b, gap=1e4):
    """Two parts `gap` extents apart along (1, 1, 1): the 30-bit Morton key (10 bits an axis) puts each part in one cell."""
    ext = max(extent(base_a[0], base_a[1]), extent(base_b[0], base_b[1]))
    moved = (base_b[0] + gap * ext, base_b[1], base_b[2])
    return _join(base_a, moved, base_a[2]["name"] + "|far|" + base_b[2]["name"])


def outlier(base, gap=1e5):
    """`base` and one triangle `gap` extents away: the whole of `base` falls into one Morton cell."""
    pts, faces, tags = base
    ext = extent(pts, faces)
    tri = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.5]]) * ext + pts.max(axis=0) + gap * ext
    one = (tri, np.array([[0, 1, 2] + [2] * (faces.shape[1] - 3)]), _tags())  # (a polygon base: the last corner repeated)
    out = _join(base, one, tags["name"] + "+outlier")
    out[2]["closed_oriented"] = False
    out[2]["has_degenerate"] = out[2]["has_degenerate"] or faces.shape[1] > 3
    return out


def frame(mesh, k=0, s=1.0, offset_ratio=0.0, direction=(1.0, 1.0, 1.0)):
    """points x (2^k s) + offset_ratio x extent x direction / |direction|, the extent taken after the scaling.  s = 1 and
    offset_ratio = 0 is a bare power of two: exact in every coordinate."""
    pts, faces, tags = mesh
    scaled = pts * (2.0 ** k * s)
    d = np.asarray(direction, dtype=np.float64)
    shift = offset_ratio * extent(scaled, faces) * d / np.linalg.norm(d) if offset_ratio else 0.0
    out = scaled + shift
    t = dict(tags, frame=(k, s, offset_ratio), name=tags["name"] + "@2^%d*%g+%g" % (k, s, offset_ratio))
    if tags["has_slivers"] and len(np.unique(out[np.unique(faces)], axis=0)) < len(np.unique(faces)):
        t["has_degenerate"] = True  # the frame's rounding merged the two ends of a collapsed edge
    if tags["has_slivers"]:
        t["folded"] = folded(out, np.asarray(faces))
    return _mesh(out, faces, t)


def pow2(x, k):
    """x x 2^k, exact (no overflow or underflow at the sizes used here)."""
    return np.ldexp(np.asarray(x, dtype=np.float64), k)


# ------------------------------------------------------------------------------------------------ queries and rays
KINDS = ("uniform", "near_vertex", "on_vertex", "on_edge", "on_face", "far", "duplicate", "nan", "inf")


def queries(mesh, n, seed=0):
    """(q (n, 3), kind (n,) int index into KINDS).  n >= 32: about 86 % uniform in the box x 1.2, 13 rows vertex +
    10^u x extent x N(0, 1) for u = -13 ... -1, 2 exact vertices, 2 edge midpoints, 2 face centroids, 4 rows 100 extents
    away, 6 exact duplicates of uniform rows, one NaN row, one +-inf row - the rows on or within 1e-9 diagonals of the
    surface stay below the 5 % that the sign and winding comparisons may leave out.  n < 32: the first n of
    (near_vertex u = -3, uniform, near_vertex u = -2, far, uniform ...), all finite and off the surface: one row on it
    would be more than 5 %, and one ray from rounding distance of a vertex along an edge, in the plane of every triangle
    on that edge, more than the 1 % of rays that may be left out."""
    pts, faces, _ = mesh
    rng = np.random.default_rng(seed)
    used = np.unique(faces)
    ref = pts[used]
    lo, hi = ref.min(axis=0), ref.max(axis=0)
    ext = extent(pts, faces)
    mid, half = 0.5 * (lo + hi), 0.6 * np.maximum(hi - lo, 1e-3 * ext)
    tri = np.asarray(faces)[:, :3]

    def uniform(m):
        return rng.uniform(mid - half, mid + half, size=(m, 3))

    def near(u):
        return pts[rng.choice(used, len(u))] + (10.0 ** np.asarray(u, dtype=np.float64))[:, None] * ext * rng.normal(size=(len(u), 3))

    def far(m):
        d = rng.normal(size=(m, 3))
        return mid + 100.0 * ext * d / np.linalg.norm(d, axis=1, keepdims=True)

    if n < 32:
        rows = [(near([-3.0]), 1), (uniform(1), 0), (near([-2.0]), 1), (far(1), 5)]
        rows += [(uniform(1), 0) for _ in range(n)]
        q = np.concatenate([r for r, _ in rows])[:n]
        kind = np.array([k for _, k in rows])[:n]
        return np.ascontiguousarray(q), kind
    f = rng.integers(0, len(tri), 4)
    parts = [(near(np.arange(-13, 0)), 1), (pts[rng.choice(used, 2)], 2),
             (0.5 * (pts[tri[f[:2], 0]] + pts[tri[f[:2], 1]]), 3),
             ((pts[tri[f[2:], 0]] + pts[tri[f[2:], 1]] + pts[tri[f[2:], 2]]) / 3.0, 4), (far(4), 5)]
    n_fixed = sum(len(p) for p, _ in parts) + 6 + 2
    uni = uniform(n - n_fixed)
    parts = [(uni, 0)] + parts + [(uni[rng.choice(len(uni), 6)], 6), (np.array([[np.nan, mid[1], mid[2]]]), 7),
                                   (np.array([[mid[0], np.inf, -np.inf]]), 8)]
    q = np.concatenate([p for p, _ in parts])
    kind = np.concatenate([np.full(len(p), k) for p, k in parts])
    order = rng.permutation(n)
    return np.ascontiguousarray(q[order]), kind[order]


RAY_KINDS = ("random", "axis", "at_vertex", "scaled")


def rays(mesh, origins, seed=0):
    """(directions (n, 3), kind (n,) int index into RAY_KINDS) for `origins` (`queries`' rows, non-finite ones included):
    random directions, axis directions with +0 and -0 in the other components, directions aimed at a vertex (not a
    `fragile` one; not normalised, t = 1 there), and random ones scaled by 2^+-30.  With a `ray_axis` a every direction
    has |d_a| >= 0.1 |d| (an in-plane ray may be accepted at any distance and no box test can follow it)."""
    pts, faces, tags = mesh
    rng = np.random.default_rng(seed)
    n = len(origins)
    kind = rng.choice(4, size=n, p=[0.4, 0.2, 0.2, 0.2])
    d = rng.normal(size=(n, 3))
    ax = kind == 1
    axes = rng.integers(0, 3, n)
    if tags["ray_axis"] is not None:
        axes[:] = tags["ray_axis"]
    sign = rng.choice([-1.0, 1.0], size=n)
    zero = rng.choice([-0.0, 0.0], size=(n, 3))
    d[ax] = zero[ax]
    d[ax, axes[ax]] = sign[ax]
    aim = kind == 2
    targets = np.setdiff1d(np.unique(faces), tags["fragile"])
    if not len(targets):  # (a soup over a handful of points, all of them in its degenerate faces)
        targets = np.unique(faces)
    d[aim] = pts[rng.choice(targets, int(aim.sum()))] - origins[aim]
    d[aim & ~np.isfinite(d).all(axis=1)] = [0.3, 0.5, 0.8]
    d[aim & ~d.any(axis=1)] = [0.3, 0.5, 0.8]  # the origin is that vertex
    sc = kind == 3
    d[sc] = np.ldexp(d[sc], rng.choice([-30, 30], size=int(sc.sum()))[:, None])
    if tags["ray_axis"] is not None:
        a = tags["ray_axis"]
        flat = np.abs(d[:, a]) < 0.1 * np.linalg.norm(d, axis=1)
        d[flat, a] = np.where(d[flat, a] < 0, -1.0, 1.0) * np.linalg.norm(d[flat], axis=1)
    return np.ascontiguousarray(d), kind


# ------------------------------------------------------------------------------------------------ d dimensions
def embed(xyz, d, centre, ext):
    """A smooth map of 3-D positions into d <= 16 dimensions, the j-th coordinate scaled by 1 / (1 + j) as eigenfunctions
    fall off: polynomials of the position normalised by `centre` and `ext` (tests/test_surface_nd.py's `_embed` is the
    model).  d >= 3 keeps a 2-manifold a 2-manifold; d < 3 is a projection with overlaps and ties.  Non-finite rows stay
    non-finite."""
    with np.errstate(invalid="ignore", over="ignore"):
        p = (np.asarray(xyz, dtype=np.float64) - centre) / ext
        x, y, z = p[:, 0], p[:, 1], p[:, 2]
        f = [x, y, z, x * y, y * z, z * x, x * x - y * y, z * z, x * y * z, x ** 3, y ** 3, z ** 3, x * x * y, y * y * z, z * z * x, x ** 4]
        out = np.stack([f[j] / (1.0 + j) for j in range(d)], axis=1)
        out[~np.isfinite(p).all(axis=1)] = np.nan
    return np.ascontiguousarray(out)


def embedded_case(mesh, q, d, k=0, s=1.0, offset_ratio=0.0):
    """(coords (n, d), faces, queries (len(q), d)): `mesh` and the 3-D queries `q` through `embed`, then the frame
    x (2^k s) + offset_ratio x (extent of the embedded surface) along (1, ..., 1) / sqrt(d) applied to both."""
    pts, faces, _ = mesh
    used = pts[np.unique(faces)]
    centre, ext = 0.5 * (used.min(axis=0) + used.max(axis=0)), extent(pts, faces)
    x, y = embed(pts, d, centre, ext), embed(q, d, centre, ext)
    scale = 2.0 ** k * s
    shift = offset_ratio * extent(x * scale, faces) / np.sqrt(d) if offset_ratio else 0.0
    return np.ascontiguousarray(x * scale + shift), faces, np.ascontiguousarray(y * scale + shift)


# ------------------------------------------------------------------------------------------------ the fixed cases
# id -> (builder, number of queries, depths of the d-dimensional run).  One per generator x frame, at the smallest sizes
# that reach each structure; tests/test_hostile_geometry.py checks on the CPU that the references alone keep the caps on
# them, tests/test_surface_hostile.py runs them on the device.
CASES = {
    "blob_64": (lambda: blob(34), 8, (3, 7, 16)),
    "blob_4600_offset_1e6": (lambda: frame(blob(2302, 1), 3, 1.37, 1e6), 299, (3, 9, 16)),
    "blob_4096_2^-20_offset_1e3": (lambda: frame(blob(2050, 2), -20, 1.91, 1e3, (1.0, -2.0, 0.5)), 16, (3, 7, 16)),
    "torus_quads_2^20_offset_1": (lambda: frame(torus_quads(24, 12), 20, 1.0, 1.0), 299, (3, 9, 16)),
    "slivers_1e-9": (lambda: slivers(blob(600, 3), 0.05, 1e-9), 299, (3, 7, 16)),
    "slivers_1e-6_offset_1e3": (lambda: frame(slivers(blob(600, 3), 0.05, 1e-6, 2), -3, 1.62, 1e3), 299, (3, 9, 16)),
    "slivers_1e-13_offset_1e6": (lambda: frame(slivers(blob(600, 3), 0.05, 1e-13, 1), 0, 1.13, 1e6), 299, (3, 7, 16)),
    "sheets_coincident": (lambda: sheets(8, 8, 2, 3), 299, (3, 9, 16)),
    "sheets_quads_3_layers_offset_1e3": (lambda: frame(sheets(6, 5, 3, 4), -3, 1.0, 1e3), 9, (3, 7, 16)),
    "sheets_stacked_offset_1e6": (lambda: frame(sheets(7, 9, 3, 3, dz=1), 5, 1.0, 1e6, (0.0, 0.0, 1.0)), 299, (3, 9, 16)),
    "soup_1": (lambda: soup(5, 1, 3, 11), 1, (3, 7, 16)),
    "soup_63": (lambda: soup(40, 63, 3, 12), 3, (3, 9, 16)),
    "soup_64": (lambda: soup(40, 64, 3, 13), 4, (3, 7, 16)),
    "soup_65": (lambda: soup(40, 65, 3, 14), 5, (3, 9, 16)),
    "soup_hexagons_offset_1": (lambda: frame(soup(50, 30, 6, 15), -9, 1.29, 1.0), 299, (3, 7, 16)),
    "soup_4097": (lambda: soup(300, 4097, 3, 16), 17, (3, 9, 16)),
    "anisotropic": (lambda: anisotropic(blob(500, 4)), 299, (3, 7, 16)),
    "far_parts": (lambda: far_parts(blob(100, 5), blob(150, 6)), 299, (3, 9, 16)),
    "outlier_2^7": (lambda: frame(outlier(blob(200, 7)), 7, 1.5, 1.0), 299, (3, 7, 16)),
}
ND_ROWS = 96  # the first rows of a case's queries go through the d-dimensional search as well


def build_case(name, seed=0):
    """(mesh, q, kind, dirs, ray kind) of a fixed case"""
    builder, n, _ = CASES[name]
    mesh = builder()
    q, kind = queries(mesh, n, seed=seed)
    d, ray_kind = rays(mesh, q, seed=seed + 1)
    return mesh, q, kind, d, ray_kind


def packet_switch_case(n, seed=0):
    """128 triangles and n = 65536 | 65537 queries and rays: the size from which a wave takes 16 of them."""
    mesh = blob(66, 8)
    rng = np.random.default_rng(seed)
    base, _ = queries(mesh, 299, seed=seed)
    pts = mesh[0]
    lo, hi = pts.min(axis=0), pts.max(axis=0)
    mid, half = 0.5 * (lo + hi), 0.6 * (hi - lo)
    q = np.concatenate([base, rng.uniform(mid - half, mid + half, size=(n - 299, 3))])
    q[299:n // 2] = pts[rng.integers(0, len(pts), n // 2 - 299)] + 0.05 * extent(pts) * rng.normal(size=(n // 2 - 299, 3))
    q = np.ascontiguousarray(q)
    d, _ = rays(mesh, q, seed=seed + 1)
    return mesh, q, d


# ------------------------------------------------------------------------------------------------ random cases (the sweeps)
def draw_mesh(rng):
    """One generator x one frame, sizes from the lists above (the three large triangle counts one time in four)."""
    seed = int(rng.integers(0, 2 ** 31))
    large = rng.random() < 0.25
    n_blob = int(rng.choice([2050, 2302])) if large else int(rng.choice([34, 66, 150, 400]))
    kind = str(rng.choice(["blob", "torus", "slivers", "sheets", "soup", "anisotropic", "far_parts", "outlier"]))
    if kind == "blob":
        mesh = blob(n_blob, seed)
    elif kind == "torus":
        mesh = torus_quads(*((48, 48) if large else (int(rng.integers(3, 20)), int(rng.integers(3, 12)))))
    elif kind == "slivers":
        mesh = slivers(blob(n_blob, seed), float(rng.choice([0.01, 0.05])), 10.0 ** -int(rng.integers(6, 14)), seed)
    elif kind == "sheets":
        vpf = int(rng.choice([3, 4]))
        nx, ny = (46, 25) if large else (int(rng.integers(1, 12)), int(rng.integers(1, 12)))
        mesh = sheets(nx, ny, int(rng.integers(2, 4)) if not large else 2, vpf, dz=int(rng.integers(0, 2)))
    elif kind == "soup":
        vpf = int(rng.integers(3, 7))
        if large:
            F = int(rng.choice([4096, 4097])) // (vpf - 2) + (vpf == 3) * int(rng.integers(0, 2))
        else:
            F = int(rng.choice([1, 63, 64, 65, 200]))
        mesh = soup(int(rng.integers(200 if large else 20, 400)), F, vpf, seed)
    elif kind == "anisotropic":
        mesh = anisotropic(blob(n_blob, seed), tuple(rng.permutation([1.0, 1e-3, 1e3])))
    elif kind == "far_parts":
        mesh = far_parts(blob(n_blob, seed), blob(int(rng.choice([34, 150])), seed + 1), gap=10.0 ** rng.integers(2, 6))
    else:
        mesh = outlier(blob(n_blob, seed), gap=10.0 ** rng.integers(3, 7))
    d = rng.normal(size=3)
    return frame(mesh, int(rng.integers(-20, 21)), float(rng.choice([1.0, rng.uniform(1.0, 2.0)])), float(rng.choice(OFFSET_RATIOS)), d)
