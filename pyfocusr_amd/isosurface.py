"""From volumes to meshes on the MI355X: the isosurface of a sampled scalar field, and what it makes possible together with
the exact signed distances of `surface_distance`.

* `isosurface(volume, level)`: the surface `volume == level` of a label map, probability map or distance map as a
  `PolyMesh` (marching tetrahedra on the Kuhn decomposition of every cube: `pf_isosurface_create`, the exact definition is
  in include/pyfocusr_hip.h).  Vertices are welded, the faces are consistently oriented with their normals pointing from
  inside to outside, and two calls give the same bits.
* `mask_to_mesh(mask)`: the boundary of a segmentation; `method="distance"` places it by the mask's own distance field.
* `signed_distance_volume(mesh)`: the signed distance of a mesh sampled on a lattice around it.
* `voxel_remesh(mesh, spacing)`: a broken surface (holes, self-intersections, non-manifold patches) re-meshed through its
  distance field; `offset_surface(mesh, distance, spacing)`: the same at another level (shells, margins).

Triangles of zero area are kept.  They arise where a sample equals the level: the crossing then sits on the lattice point
itself and the vertices of several lattice edges share that position.  They are separate vertices all the same, and the
connectivity stays that of a manifold.  The triangles are those of the tetrahedra, so their quality is that of the
lattice; `resample_mesh` behind it gives a uniform mesh that `Graph` and `Focusr` can take.
"""
import numpy as np

from . import _hip
from ._meshargs import AttrDict, checked_mesh
from .distance_transform import signed_field_surface
from .remesh import resample_mesh
from .surface_distance import signed_point_to_surface_distances
from .vtk_functions import PolyMesh

_INSIDE = ("below", "above")
_METHODS = ("staircase", "distance")


def _three(value, name):
    v = np.asarray(value, dtype=np.float64)
    v = np.repeat(v, 3) if v.ndim == 0 else v.reshape(-1)
    if v.shape != (3,) or not np.isfinite(v).all():
        raise ValueError("%s must be one finite number or three" % name)
    return v


def prepare_volume(volume, level=0.0, spacing=(1.0, 1.0, 1.0), origin=(0.0, 0.0, 0.0), inside="below", closed=False):
    """(values, level, spacing, origin) as `isosurface` hands them to the device; plain numpy, no library.
    `inside="above"` negates the values and the level.  `closed` adds one layer of samples on every side, each
    `level + |v - level|` of the nearest original sample v, so outside, and moves the origin by minus one spacing."""
    if inside not in _INSIDE:
        raise ValueError("inside must be one of %r, not %r" % (_INSIDE, inside))
    values, level, spacing, origin = _hip.check_volume(volume, level, _three(spacing, "spacing"), _three(origin, "origin"))
    if inside == "above":
        values, level = -values, -level
    if closed:
        padded = np.pad(values, 1, mode="edge")
        shell = np.ones(padded.shape, dtype=bool)
        shell[1:-1, 1:-1, 1:-1] = False
        padded[shell] = level + np.abs(padded[shell] - level)
        values, origin = padded, origin - spacing
        if values.size >= 2 ** 31:
            raise ValueError("the closed volume must have fewer than 2^31 samples, not %d" % values.size)
    return np.ascontiguousarray(values), level, spacing, origin


def isosurface(volume, level=0.0, spacing=(1.0, 1.0, 1.0), origin=(0.0, 0.0, 0.0), inside="below", closed=False,
               return_info=False, ctx=None):
    """The surface `volume == level` as a `PolyMesh`.  `volume` is an (nx, ny, nz) array of finite real numbers with every
    extent >= 2; the sample (i, j, k) sits at `origin + (i, j, k) * spacing`.

    inside   "below": a sample is inside where `volume < level` (distance maps); "above": where `volume > level`
             (probability maps, masks).  The normals point from inside to outside.  A sample equal to the level is outside.
    closed   False: a surface that reaches the border of the volume ends there, open.  True: one layer of outside samples
             is added on every side, so the surface is capped half a step beyond the border and comes out closed.

    A volume without a crossing gives a mesh without points.  With `return_info` the result is `(mesh, info)`:
    `vertex_key` (V,) int64 = 7 * lattice index + edge kind of the lattice edge each vertex lies on, `face_cell` (F,) the
    cell of each face, `shape` and `origin` of the lattice they index (one layer larger than `volume` when `closed`),
    `n_crossing_cells`, `report`, `device_ms`."""
    values, level, spacing, origin = prepare_volume(volume, level, spacing, origin, inside, closed)
    ctx = ctx if ctx is not None else _hip.default_context()
    raw = ctx.isosurface(values, level, spacing, origin)
    mesh = PolyMesh(raw["points"], raw["faces"])
    if not return_info:
        return mesh
    return mesh, AttrDict(vertex_key=raw["vertex_key"], face_cell=raw["face_cell"], shape=values.shape, origin=origin,
                          n_crossing_cells=int(raw["report"][2]), report=raw["report"], device_ms=raw["device_ms"])


def mask_to_mesh(mask, spacing=(1.0, 1.0, 1.0), origin=(0.0, 0.0, 0.0), closed=True, return_info=False, ctx=None,
                 method="staircase"):
    """The boundary of a segmentation.  `mask` is boolean or a 0 / 1 label map.

    method   "staircase": `isosurface(mask.astype(float), 0.5, inside="above")`; the surface runs half a step outside the
             voxel centres.  "distance": level 0 of the mask's signed Euclidean distance field (`distance_transform`),
             computed and meshed on the device without a round trip.  The inside set is the same, so are the faces and
             the vertex keys; the vertices sit where the distances to the two classes balance along each lattice edge.
             `closed` then pads the mask with one layer of background instead of padding a float volume."""
    if method not in _METHODS:
        raise ValueError("method must be one of %r, not %r" % (_METHODS, method))
    if method == "staircase":
        return isosurface(np.asarray(mask).astype(np.float64), 0.5, spacing, origin, inside="above", closed=closed,
                          return_info=return_info, ctx=ctx)
    raw, shape, origin = signed_field_surface(mask, 0.0, _three(spacing, "spacing"), origin, 1 if closed else 0, ctx=ctx)
    if raw is None:  # a class is empty: no crossing
        raw = {"points": np.zeros((0, 3)), "faces": np.zeros((0, 3), dtype=np.int32), "vertex_key": np.zeros(0, dtype=np.int64),
               "face_cell": np.zeros(0, dtype=np.int32), "report": np.zeros(8, dtype=np.int64), "device_ms": 0.0}
    mesh = PolyMesh(raw["points"], raw["faces"])
    if not return_info:
        return mesh
    return mesh, AttrDict(vertex_key=raw["vertex_key"], face_cell=raw["face_cell"], shape=shape, origin=origin,
                          n_crossing_cells=int(raw["report"][2]), report=raw["report"], device_ms=raw["device_ms"])


def signed_distance_volume(mesh, spacing=None, shape=None, padding=2, sign="pseudonormal", check_orientation=True, ctx=None):
    """(values (nx, ny, nz), origin (3,), spacing (3,)): the signed distance to `mesh` (negative inside) on a lattice
    around its bounding box, `padding` samples wider on every side.  Give `spacing` (one number or three) or `shape`
    (three extents; the spacing then follows from the box).  The lattice points are built on the host and go through
    one call of `signed_point_to_surface_distances`, whose `sign` and `check_orientation` these are."""
    pts, faces = checked_mesh(mesh, finite=True)
    padding = int(padding)
    if padding < 1:
        raise ValueError("padding must be at least one sample")
    if (spacing is None) == (shape is None):
        raise ValueError("give exactly one of spacing and shape")
    lo, hi = pts.min(axis=0), pts.max(axis=0)
    if spacing is not None:
        spacing = _three(spacing, "spacing")
        if (spacing <= 0.0).any():
            raise ValueError("spacing must be positive")
        shape = np.ceil((hi - lo) / spacing).astype(np.int64) + 1 + 2 * padding
    else:
        shape = np.asarray(shape, dtype=np.int64).reshape(-1)
        if shape.shape != (3,) or (shape < 2 * padding + 2).any():
            raise ValueError("shape must be three extents of at least 2 * padding + 2")
        spacing = (hi - lo) / (shape - 1 - 2 * padding)
        if (spacing <= 0.0).any():
            raise ValueError("the mesh has no extent along an axis: give spacing instead of shape")
    if int(np.prod(shape)) >= 2 ** 31:
        raise ValueError("the lattice must have fewer than 2^31 samples, not %d" % int(np.prod(shape)))
    origin = lo - padding * spacing
    axes = [origin[a] + np.arange(shape[a], dtype=np.float64) * spacing[a] for a in range(3)]
    queries = np.stack(np.meshgrid(*axes, indexing="ij"), axis=-1).reshape(-1, 3)
    sd, _ = signed_point_to_surface_distances(queries, (pts, faces), ctx=ctx, check_orientation=check_orientation, sign=sign)
    return sd.reshape(tuple(int(s) for s in shape)), origin, spacing


def offset_surface(mesh, distance, spacing, sign="pseudonormal", n_vertices=None, check_orientation=True, ctx=None):
    """The surface at signed distance `distance` from `mesh` (positive: outside, a margin; negative: inside, a shell) as
    a closed `PolyMesh`: the `isosurface` of `signed_distance_volume` at that level.  Every vertex lies within one cell
    diagonal of the exact offset.  `n_vertices` passes the result through `resample_mesh`."""
    distance = float(distance)
    spacing = _three(spacing, "spacing")
    if not np.isfinite(distance) or (spacing <= 0.0).any():
        raise ValueError("distance must be finite and spacing positive")
    padding = 2 + int(np.ceil(max(distance, 0.0) / spacing.min()))
    values, origin, spacing = signed_distance_volume(mesh, spacing=spacing, padding=padding, sign=sign,
                                                     check_orientation=check_orientation, ctx=ctx)
    out = isosurface(values, distance, spacing, origin, closed=True, ctx=ctx)
    if n_vertices is not None and len(out.faces):
        out = resample_mesh(out, n_vertices, ctx=ctx)
    return out


def voxel_remesh(mesh, spacing, sign="winding", n_vertices=None, check_orientation=True, ctx=None):
    """`mesh` re-meshed through its distance field: `offset_surface` at distance 0.  With `sign="winding"` (the default)
    open and non-manifold inputs work: holes are closed the way the surface continues."""
    return offset_surface(mesh, 0.0, spacing, sign=sign, n_vertices=n_vertices, check_orientation=check_orientation, ctx=ctx)
