"""Sub-vertex correspondences: the closest point of a triangulated surface embedded in d dimensions.

FOCUSR matches a source vertex to the nearest target *vertex* in spectral coordinates, so many source vertices share one
target vertex and the transformed mesh is stair-stepped.  The target is a triangulated surface in the same
d-dimensional space; the precise map sends a source vertex to the closest point *on* it: a face and barycentric weights
(the "precise maps" of the functional-maps literature).  With them anything defined on target vertices - positions,
point data, labels - is carried over without quantisation (`interpolate_on_surface`).

The search runs on the MI355X (`pf_surface_nd_closest`, `_hip.DeviceSurfaceND`) for 1 <= d <= 16: exact, the minimum
over all fan triangles, lowest triangle on ties, bit for bit what a brute-force loop gives.
"""
import contextlib

import numpy as np

from . import _hip
from ._meshargs import checked_faces

MAX_DIM = 16


def _surface_arrays(coords, faces):
    x = np.ascontiguousarray(coords, dtype=np.float64)
    if x.ndim != 2 or x.shape[0] == 0 or not 1 <= x.shape[1] <= MAX_DIM:
        raise ValueError("coords must be a non-empty (n, d) array with 1 <= d <= %d" % MAX_DIM)
    f = checked_faces(faces, noun="faces")
    if not np.issubdtype(f.dtype, np.integer) or f.min() < 0 or f.max() >= x.shape[0]:
        raise ValueError("faces must hold vertex ids in 0 .. %d" % (x.shape[0] - 1))
    return x, np.ascontiguousarray(f, dtype=np.int32)


def closest_points_on_embedded_surface(queries, coords, faces, ctx=None, surface=None, exhaustive=False):
    """The closest point of the surface (`coords` (n, d), `faces` (F, verts_per_face); polygons fan-triangulated
    (0, j+1, j+2)) for every row of `queries` (q, d), 1 <= d <= 16.  Returns a dict: `face` (q,) i32 the face of the
    winning fan triangle, `vertices` (q, 3) i32 that triangle's corners, `bary` (q, 3) f64 the weights of the closest
    point on them (exact 0 / 1 at corners and on the opposite corner of an edge), `d2` (q,) f64 the squared distance.  A
    query with a non-finite coordinate gives -1, (-1, -1, -1), NaN, NaN.

    `surface`: a `_hip.DeviceSurfaceND` built earlier from the same surface, reused and left open (`coords` and `faces`
    may then be None).  `exhaustive` tests every triangle on the device instead of pruning by boxes: the same bits."""
    q = np.ascontiguousarray(queries, dtype=np.float64)
    if q.ndim != 2 or q.shape[0] == 0:
        raise ValueError("queries must be a non-empty (q, d) array")
    own = contextlib.nullcontext()
    if surface is None:
        x, f = _surface_arrays(coords, faces)
        if q.shape[1] != x.shape[1]:
            raise ValueError("queries have %d coordinates, the surface %d" % (q.shape[1], x.shape[1]))
        surface = own = _hip.DeviceSurfaceND(x, f, ctx=ctx)
    elif q.shape[1] != surface.d:
        raise ValueError("queries have %d coordinates, the surface %d" % (q.shape[1], surface.d))
    with own:
        face, vertices, bary, d2 = surface.closest(q, exhaustive=exhaustive)
    return {"face": face, "vertices": vertices, "bary": bary, "d2": d2}


def interpolate_on_surface(values, vertices, bary):
    """sum_j bary[:, j] * values[vertices[:, j]], summed in corner order, for `values` (n,) or (n, m) given on the
    surface's vertices: (q,) or (q, m) f64.  Rows with vertex -1 (no correspondence) give NaN.  Plain numpy."""
    values = np.asarray(values, dtype=np.float64)
    vertices = np.asarray(vertices)
    bary = np.asarray(bary, dtype=np.float64)
    if values.ndim not in (1, 2) or vertices.ndim != 2 or vertices.shape[1] != 3 or bary.shape != vertices.shape:
        raise ValueError("values must be (n,) or (n, m), vertices and bary (q, 3)")
    missing = (vertices < 0).any(axis=1)
    v = np.where(missing[:, None], 0, vertices)
    w = bary if values.ndim == 1 else bary[:, :, None]
    out = np.take(values, v[:, 0], axis=0) * w[:, 0]
    out = out + np.take(values, v[:, 1], axis=0) * w[:, 1]
    out = out + np.take(values, v[:, 2], axis=0) * w[:, 2]
    out[missing] = np.nan
    return out


def transfer_point_data(target_mesh, name, vertices, bary):
    """`interpolate_on_surface` of the point-data array `name` of `target_mesh` (a `PolyMesh`): e.g. the target's
    `thickness_change_(mm)` at the image of every source vertex."""
    for n, vals in getattr(target_mesh, "point_data", []):
        if n == name:
            return interpolate_on_surface(vals, vertices, bary)
    raise KeyError("the mesh has no point-data array %r" % (name,))
