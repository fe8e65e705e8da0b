"""Ray casting against surfaces: first hits, crossing counts, and thickness along vertex normals.

What lies along a given direction from a point: cartilage or cortical thickness along the bone normal, the gap between
two registered surfaces along the normal instead of to the nearest point, line-of-sight checks.  `pf_surface_raycast`
(`_hip.DeviceSurface.raycast`) traces many rays on the MI355X through the structure of the surface distances (polygons
fan-triangulated), with one exact Moeller-Trumbore test in float64: the result of a ray is that test's over all
triangles, bit for bit what a brute-force loop gives.  A ray is `origin + t * direction`; directions are not
normalised, so t is in units of the direction's length.  The test is not watertight: a ray exactly through an edge or
a vertex may be accepted by both neighbouring triangles or by neither.

Every `mesh` may be a `PolyMesh`, a vtkPolyData, a `(points, faces)` pair, or a `_hip.DeviceSurface` built earlier,
which is then reused and left open.
"""
import numpy as np

from . import _hip
from . import vtk_functions
from ._meshargs import checked_mesh

_FACING = {"any": 0, "front": 1, "back": -1}
_DIRECTIONS = {"outward": 1.0, "inward": -1.0}


def _rays(origins, directions):
    o = _hip._queries(origins, "ray origins")
    d = np.ascontiguousarray(directions, dtype=np.float64)
    if d.shape != o.shape:
        raise ValueError("ray directions must have the shape of the origins, %r, not %r" % (o.shape, d.shape))
    return o, d


def _interval(t_min, t_max):
    t_min, t_max = float(t_min), float(t_max)
    if not t_min <= t_max:  # also NaN
        raise ValueError("t_min <= t_max expected, not [%r, %r]" % (t_min, t_max))
    return t_min, t_max


def _facing(facing):
    if facing not in _FACING:
        raise ValueError("facing must be one of %r, not %r" % (tuple(_FACING), facing))
    return _FACING[facing]


class _Surface(object):
    """`mesh` as an open DeviceSurface: the one given, or one built here and closed on exit."""

    def __init__(self, mesh, ctx):
        self.given = mesh if hasattr(mesh, "raycast") else None
        self.arrays = None if self.given is not None else checked_mesh(mesh)  # checked before any device call
        self.ctx = ctx

    def __enter__(self):
        self.surface = self.given if self.given is not None else _hip.DeviceSurface(*self.arrays, ctx=self.ctx)
        return self.surface

    def __exit__(self, *exc):
        if self.given is None:
            self.surface.close()


def ray_mesh_intersections(origins, directions, mesh, t_min=0.0, t_max=np.inf, facing="any", ctx=None):
    """(t (n,) f64, face (n,) i32, uv (n, 2) f64): the first hit of every ray with the surface of `mesh` for t in
    [t_min, t_max] (both ends inclusive): the least t (lowest fan-triangle index on exact ties), the face hit, and the
    barycentric (u, v) of the hit in its fan triangle (a, b, c): a + u (b - a) + v (c - a).  `facing`: "any" side,
    "front" only where the ray meets the side the face normal points to, "back" only the other.  A miss gives +inf, -1
    and NaN; a ray with a non-finite component or a zero direction gives NaN, -1 and NaN."""
    o, d = _rays(origins, directions)
    t_min, t_max = _interval(t_min, t_max)
    facing = _facing(facing)
    with _Surface(mesh, ctx) as surface:
        return surface.raycast(o, d, t_min=t_min, t_max=t_max, facing=facing)


def hit_points(origins, directions, t):
    """(n, 3): origin + t * direction of every ray that hit (pure numpy, no device); NaN rows for misses (t = +inf) and
    invalid rays (t = NaN)."""
    o, d = _rays(origins, directions)
    t = np.asarray(t, dtype=np.float64)
    if t.shape != (len(o),):
        raise ValueError("one t per ray expected")
    hit = np.isfinite(t)
    out = np.full(o.shape, np.nan)
    out[hit] = o[hit] + t[hit, None] * d[hit]
    return out


def ray_crossings(origins, directions, mesh, t_min=0.0, t_max=np.inf, ctx=None):
    """int32 (n,): how many fan triangles of `mesh` every ray crosses for t in [t_min, t_max] (either side); 0 for a ray
    with a non-finite component or a zero direction.  On a closed mesh an odd count from t_min = 0 means the origin is
    inside, unless the ray passes exactly through an edge or a vertex (`points_inside` has no such exception)."""
    o, d = _rays(origins, directions)
    t_min, t_max = _interval(t_min, t_max)
    with _Surface(mesh, ctx) as surface:
        return surface.raycast(o, d, t_min=t_min, t_max=t_max, facing=0, count=True)[3]


def _unit(raw):
    length = np.sqrt(np.sum(raw * raw, axis=1, keepdims=True))
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(length > 0.0, raw / length, np.nan)


def vertex_normals(mesh, ctx=None):
    """(n, 3) f64: unit angle-weighted vertex normals of `mesh` (the vertex pseudonormals of the signed distances: sum
    of corner angle x unit face normal over the fan triangles, built on the device, normalised here).  They point
    where the face normals point: outward on an outward-oriented mesh.  A vertex with a zero pseudonormal (no face
    references it, or only zero-area ones) gets NaN."""
    with _Surface(mesh, ctx) as surface:
        return _unit(surface.vertex_normals())


def thickness_along_normals(mesh, other=None, direction="outward", t_max=np.inf, facing="any", name=None, ctx=None):
    """(n,) f64: from every vertex of `mesh` along its unit normal (`vertex_normals(mesh)`; "inward" = against it), the
    distance to the first hit with the surface of `other` within `t_max`.  `other=None` casts against `mesh` itself
    (its own thickness, usually "inward") from t_min = 1e-9 x the bounding-box diagonal, which skips the triangles
    around the vertex; otherwise t_min = 0.  A miss gives +inf, a vertex with a NaN normal NaN.  `facing` as in
    `ray_mesh_intersections`.  With `name` the result is also stored on `mesh` as that point-data array
    (`set_mesh_scalars`)."""
    if direction not in _DIRECTIONS:
        raise ValueError("direction must be one of %r, not %r" % (tuple(_DIRECTIONS), direction))
    facing = _facing(facing)
    pts, _ = checked_mesh(mesh)
    t_min = 0.0
    if other is None:
        t_min = 1e-9 * float(np.linalg.norm(pts.max(axis=0) - pts.min(axis=0)))
    t_min, t_max = _interval(t_min, t_max)
    own_surface = _Surface(mesh, ctx)
    target_surface = own_surface if other is None else _Surface(other, ctx)  # both checked before any device call
    with own_surface as own:
        normals = _unit(own.vertex_normals())
        if _DIRECTIONS[direction] < 0:
            normals = -normals
        if other is None:
            t = own.raycast(pts, normals, t_min=t_min, t_max=t_max, facing=facing)[0]
        else:
            with target_surface as target:
                t = target.raycast(pts, normals, t_min=t_min, t_max=t_max, facing=facing)[0]
    if name is not None:
        vtk_functions.set_mesh_scalars(mesh, t, name=name)
    return t
