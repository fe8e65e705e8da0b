"""Explicit mesh smoothing as include/pyfocusr_hip.h defines it (pf_smoother_*), in numpy, one operation at a time in the
stated order: float64, separate multiplies and adds, sums left to right.  Rows are vectorised over the vertices by
neighbour rank (`for k in range(largest_row): acc = acc + ...` under a mask), which keeps the left-to-right order."""
import numpy as np

from _isosurface_ref import isosurface_ref
from _map_quality_ref import tree_sum

BOUNDARY, PINNED, MOVABLE = 1, 2, 4
WEIGHTS = ("uniform", "cotangent")
MODES = ("free", "fixed", "curve")


def _sum3(a):
    return (a[:, 0] + a[:, 1]) + a[:, 2]


def half_cotangents(points, faces):
    """[F][3]: 0.5 ((u . v) / |u x v|) at corner k, u and v the edges that leave it for the next corner and the one after;
    0 at all three corners of a triangle where |u x v| is 0 or not finite at one of them."""
    p, f = np.asarray(points, dtype=np.float64), np.asarray(faces, dtype=np.int64)
    hc = np.empty((len(f), 3))
    area = np.ones(len(f), dtype=bool)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for k in range(3):
            u = p[f[:, (k + 1) % 3]] - p[f[:, k]]
            v = p[f[:, (k + 2) % 3]] - p[f[:, k]]
            dot = _sum3(u * v)
            c = np.stack([u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1], u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2],
                          u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]], axis=1)
            nrm = np.sqrt(_sum3(c * c))
            area &= (nrm > 0.0) & np.isfinite(nrm)
            hc[:, k] = 0.5 * (dot / nrm)
    hc[~area] = 0.0
    return hc


def adjacency(points, faces, weights="uniform", boundary="fixed", pinned=None):
    """dict: rowptr (n + 1,) i32, col i32, w f64, ebf bool (the entry's edge has one half-edge), kind (n,) u8 and
    counts (6,) i64 = edges | boundary edges | non-manifold edges | entries | largest row | movable vertices."""
    assert weights in WEIGHTS and boundary in MODES
    p, f = np.asarray(points, dtype=np.float64), np.asarray(faces, dtype=np.int64)
    n = len(p)
    # half-edge h = 3 t + j goes from corner j to corner j + 1; the corner opposite its edge is j + 2
    a, b = f.ravel(), f[:, [1, 2, 0]].ravel()
    proper = a != b
    h = np.flatnonzero(proper)
    lo, hi = np.minimum(a[h], b[h]), np.maximum(a[h], b[h])
    key, first, inverse, multiplicity = np.unique(lo * n + hi, return_index=True, return_inverse=True, return_counts=True)
    n_edges = len(key)
    e_lo, e_hi = key // n, key % n
    ew = np.ones(n_edges)
    if weights == "cotangent":
        hc = half_cotangents(p, f).ravel()
        opposite = 3 * (h // 3) + (h % 3 + 2) % 3
        order = np.argsort(inverse, kind="stable")  # the half-edges of an edge in ascending h
        start = np.concatenate([[0], np.cumsum(multiplicity)[:-1]])
        s = np.zeros(n_edges)
        for k in range(int(multiplicity.max()) if n_edges else 0):
            m = multiplicity > k
            s[m] = s[m] + hc[opposite[order[start[m] + k]]]
        ew = np.where(s > 0.0, s, 0.0)
    e_bnd = multiplicity == 1
    # directed entries, sorted by (source, neighbour)
    src, dst = np.concatenate([e_lo, e_hi]), np.concatenate([e_hi, e_lo])
    order = np.lexsort((dst, src))
    src, col = src[order], dst[order]
    w, ebf = np.concatenate([ew, ew])[order], np.concatenate([e_bnd, e_bnd])[order]
    rowptr = np.searchsorted(src, np.arange(n + 1)).astype(np.int64)
    length = np.diff(rowptr)
    is_boundary = np.zeros(n, dtype=bool)
    is_boundary[src[ebf]] = True
    pin = np.zeros(n, dtype=bool) if pinned is None else np.asarray(pinned) != 0
    sw = length.astype(np.float64)
    if weights == "cotangent":
        sw = np.zeros(n)
        for k in range(int(length.max()) if n else 0):
            m = length > k
            sw[m] = sw[m] + w[rowptr[:-1][m] + k]
        if boundary == "curve":
            sw[is_boundary] = 1.0  # a boundary vertex has at least one boundary neighbour, each of weight 1
    movable = ~pin & ~(is_boundary & (boundary == "fixed")) & (sw > 0.0)
    kind = (BOUNDARY * is_boundary + PINNED * pin + MOVABLE * movable).astype(np.uint8)
    counts = np.array([n_edges, int(e_bnd.sum()), int((multiplicity > 2).sum()), len(col), int(length.max()) if n else 0,
                       int(movable.sum())], dtype=np.int64)
    return dict(rowptr=rowptr.astype(np.int32), col=col.astype(np.int32), w=w, ebf=ebf, kind=kind, counts=counts,
                weights=weights, boundary=boundary)


def sweep(adj, x, f):
    """One sweep with factor f over x (n, c): x + f (s / W - x) at the movable vertices, the others keep their bits."""
    rowptr, col, w, ebf, kind = (adj[k] for k in ("rowptr", "col", "w", "ebf", "kind"))
    rowptr = rowptr.astype(np.int64)
    n, c = x.shape
    movable = (kind & MOVABLE) != 0
    curve = (adj["boundary"] == "curve") & ((kind & BOUNDARY) != 0)
    length = np.diff(rowptr)
    s, sw = np.zeros((n, c)), np.zeros(n)
    weighted = adj["weights"] == "cotangent"
    for k in range(int(length[movable].max()) if movable.any() else 0):
        m = movable & (length > k)
        e = rowptr[:-1][m] + k
        on_curve = curve[m]
        take = np.where(on_curve, ebf[e], True)  # a boundary vertex of the curve mode skips its interior neighbours
        rows, e, on_curve = np.flatnonzero(m)[take], e[take], on_curve[take]
        we = np.where(on_curve, 1.0, w[e])
        if weighted:
            # (a curve row adds x_u itself: 1.0 x_u has the same bits)
            s[rows] = s[rows] + we[:, None] * x[col[e]]
        else:
            s[rows] = s[rows] + x[col[e]]
        sw[rows] = sw[rows] + we
    out = x.copy()
    mv = np.flatnonzero(movable)
    out[mv] = x[mv] + f * (s[mv] / sw[mv][:, None] - x[mv])
    return out


def clamp(adj, x, x0, c):
    """x into [x0 - c, x0 + c] per component at the movable vertices."""
    mv = np.flatnonzero((adj["kind"] & MOVABLE) != 0)
    lo, hi = x0[mv] - c, x0[mv] + c
    y = np.where(x[mv] < lo, lo, x[mv])
    y = np.where(y > hi, hi, y)
    out = x.copy()
    out[mv] = y
    return out


def run(adj, x0, factors, clamp_every=1, bound=None):
    """The result of pf_smoother_run for the input x0 (n, c)."""
    x0 = np.ascontiguousarray(x0, dtype=np.float64)
    x = x0.copy()
    for i, f in enumerate(factors):
        x = sweep(adj, x, float(f))
        if bound is not None and (i + 1) % clamp_every == 0:
            x = clamp(adj, x, x0, np.asarray(bound, dtype=np.float64))
    return x


def volume(points, faces):
    """The signed volume: the tree sum over the faces of x0 . (x1 x x2), divided by 6."""
    p, f = np.asarray(points, dtype=np.float64), np.asarray(faces, dtype=np.int64)
    a, b, c = p[f[:, 0]], p[f[:, 1]], p[f[:, 2]]
    cr = np.stack([b[:, 1] * c[:, 2] - b[:, 2] * c[:, 1], b[:, 2] * c[:, 0] - b[:, 0] * c[:, 2], b[:, 0] * c[:, 1] - b[:, 1] * c[:, 0]],
                  axis=1)
    return tree_sum(_sum3(a * cr)) / 6.0


def stats(x0, x, faces):
    """(6,): volume of x0, of x | vertex mean of x | largest |x - x0|."""
    n = float(len(x))
    return np.array([volume(x0, faces), volume(x, faces), tree_sum(x[:, 0]) / n, tree_sum(x[:, 1]) / n, tree_sum(x[:, 2]) / n,
                     np.max(np.abs(x - x0))])


def factors(iterations, method="taubin", lam=0.5, pass_band=0.1):
    """(factors, sweeps per iteration) as pyfocusr_amd.smoothing passes them to the library."""
    if method == "laplacian":
        return np.full(iterations, float(lam)), 1
    mu = 1.0 / (float(pass_band) - 1.0 / float(lam))
    return np.tile(np.array([float(lam), mu]), iterations), 2


def smooth(points, faces, iterations=20, method="taubin", lam=0.5, pass_band=0.1, weights="uniform", boundary="fixed", pinned=None,
           max_displacement=None):
    """(points, stats) of `smooth_mesh` without `preserve_volume`."""
    adj = adjacency(points, faces, weights, boundary, pinned)
    fac, per = factors(iterations, method, lam, pass_band)
    bound = None if max_displacement is None else np.broadcast_to(np.asarray(max_displacement, dtype=np.float64), (3,))
    x0 = np.ascontiguousarray(points, dtype=np.float64)
    x = run(adj, x0, fac, per, bound)
    return x, stats(x0, x, faces)


SPHERE_SHAPE, SPHERE_RADIUS, SPHERE_SPACING = (30, 30, 18), 6.3, (0.6, 0.6, 1.2)


def sphere_mask_mesh():
    """(points, faces, centre): the isosurface at 0.5 of the mask of a sphere of radius 6.3 in a 30 x 30 x 18 grid with
    spacing (0.6, 0.6, 1.2): a voxel staircase of 4224 vertices and 8444 faces, outward."""
    shape, spacing = np.array(SPHERE_SHAPE), np.array(SPHERE_SPACING)
    centre = (shape - 1) * spacing / 2.0
    grid = np.stack(np.meshgrid(*[np.arange(s) for s in shape], indexing="ij"), axis=-1) * spacing
    inside = np.sqrt(((grid - centre) ** 2).sum(axis=-1)) < SPHERE_RADIUS
    pts, faces = isosurface_ref(np.where(inside, 0.0, 1.0), 0.5, spacing)[:2]
    return pts, faces, centre


def normal_deviation(points, faces, centre):
    """The mean angle in degrees between the face normals and the direction from `centre` to the face centroids, over
    the faces with an area."""
    p, f = np.asarray(points), np.asarray(faces)
    a, b, c = p[f[:, 0]], p[f[:, 1]], p[f[:, 2]]
    nrm = np.cross(b - a, c - a)
    radial = (a + b + c) / 3.0 - centre
    ln, lr = np.linalg.norm(nrm, axis=1), np.linalg.norm(radial, axis=1)
    ok = (ln > 0.0) & (lr > 0.0)
    cos = np.sum(nrm[ok] * radial[ok], axis=1) / (ln[ok] * lr[ok])
    return float(np.degrees(np.mean(np.arccos(np.clip(cos, -1.0, 1.0)))))
