"""How a correspondence treats the source surface as a map, on the MI355X: stretch, collapse, fold-over, coverage.

`surface_distance_metrics` says how close a registered mesh lies to the target; a source that piles half of its vertices
onto one target patch, or folds over itself, still gets a good ASSD.  Without a ground-truth map what can always be
computed is what the map does to the source's own triangles.  One device call (`pf_map_distortion`,
`_hip.Context.map_distortion`) takes a vertex map (`corresponding_target_idx_for_each_source_pt`, an assignment, ZoomOut,
`lift_point_map`) or a surface map (`closest_points_on_embedded_surface`) and gives

* per source face the singular values `sigma_max` >= `sigma_min` of the linear map from the face onto its image triangle
  (1, 1: an isometry), the `area_ratio`, and the masks `valid`, `collapsed` (image area exactly 0: two corners share a
  target vertex, sigma_min = 0) and `flipped` (the image triangle faces against the target's vertex normals);
* per source vertex the area-weighted means `vertex_sigma_max`, `vertex_sigma_min` over its valid faces, `vertex_area`
  (the barycentric area of `discrete_curvatures`, bit for bit) and `vertex_flipped`, `vertex_collapsed`;
* per target vertex `target_count`, the source vertices it owns (for a surface map: the corner with the largest weight),
  and `target_premass`, their area;
* `totals` (source area | image area | Dirichlet energy | area x sigma_max | area x sigma_min | collapsed area | flipped
  area | 0), `report` (faces valid | collapsed | flipped | invalid | with an unmapped corner | target vertices hit |
  largest count | flipped vertices) and the scalars read first: `dirichlet_energy`, `area_distortion`,
  `collapsed_area_fraction`, `flipped_area_fraction`, `target_vertices_hit_fraction`.

A source vertex mapped to -1 is unmapped: its faces are invalid and count nowhere.  float64 throughout, every sum in a
fixed order, so two calls give the same bits.  The exact definitions are in include/pyfocusr_hip.h.

This is a capability of its own: nothing in `Focusr.align_maps()` calls it (`Focusr.map_quality` does, on request).
"""
import numpy as np

from . import _hip
from . import vtk_functions
from ._meshargs import AttrDict, checked_mesh
from .spectral_descriptors import signature_on_mesh

VALID, COLLAPSED, FLIPPED, UNMAPPED = 1, 2, 4, 8
_VERTEX_FIELDS = ("sigma_max", "sigma_min", "area", "flipped", "collapsed", "conformal", "isometric")


class MapDistortion(AttrDict):
    """The result of `map_distortion`: a dict whose keys are also attributes."""


def _target(target):
    """(points (k, 3) f64, faces or None) of a target given as a mesh, a (points, faces) pair or bare points."""
    faces = None
    if isinstance(target, (tuple, list)) and len(target) == 2 and np.ndim(target[0]) == 2:
        pts, faces = target
    elif isinstance(target, np.ndarray) or isinstance(target, (tuple, list)):
        pts = target
    else:
        pts, faces = vtk_functions.mesh_arrays(target)
    pts = np.ascontiguousarray(pts, dtype=np.float64)
    if pts.ndim != 2 or pts.shape[1] != 3 or pts.shape[0] == 0:
        raise ValueError("target points must be a non-empty (k, 3) array")
    if pts.shape[0] >= 2**31:
        raise ValueError("the target is too large: its points must stay below 2^31")
    if faces is not None:
        faces = np.asarray(faces)
        if faces.ndim != 2 or faces.shape[0] == 0 or faces.shape[1] < 3 or not np.issubdtype(faces.dtype, np.integer):
            raise ValueError("target faces must be a non-empty (m, >= 3) integer array")
        if faces.min() < 0 or faces.max() >= pts.shape[0]:
            raise ValueError("target face index out of range 0 .. %d" % (pts.shape[0] - 1))
        faces = np.ascontiguousarray(faces, dtype=np.int32)
    return pts, faces


def _map_arrays(vertex_map, surface_map, n_source, n_target):
    """(map_vertices (n, c) i32, map_weights (n, 3) f64 or None), checked."""
    if (vertex_map is None) == (surface_map is None):
        raise ValueError("give exactly one of vertex_map and surface_map")
    weights = None
    if vertex_map is not None:
        vertices = np.asarray(vertex_map)
        if vertices.shape != (n_source,):
            raise ValueError("vertex_map must hold one target vertex per source vertex: (%d,), not %r" % (n_source, vertices.shape))
    else:
        if isinstance(surface_map, dict):
            if "vertices" not in surface_map or "bary" not in surface_map:
                raise ValueError("surface_map must have `vertices` and `bary`")
            vertices, weights = surface_map["vertices"], surface_map["bary"]
        elif isinstance(surface_map, (tuple, list)) and len(surface_map) == 2:
            vertices, weights = surface_map
        else:
            raise ValueError("surface_map must be the dict of closest_points_on_embedded_surface or a (vertices, bary) pair")
        vertices, weights = np.asarray(vertices), np.ascontiguousarray(weights, dtype=np.float64)
        if vertices.shape != (n_source, 3) or weights.shape != (n_source, 3):
            raise ValueError("surface_map needs vertices and bary of shape (%d, 3)" % n_source)
    if not np.issubdtype(vertices.dtype, np.integer):
        raise ValueError("map vertices must be integers")
    first = vertices if vertices.ndim == 1 else vertices[:, 0]
    mapped = first != -1
    rows = vertices[mapped]
    if rows.size and (rows.min() < 0 or rows.max() >= n_target):
        raise ValueError("map vertex out of range 0 .. %d (-1 in the first column: unmapped)" % (n_target - 1))
    if weights is not None and not np.isfinite(weights[mapped]).all():
        raise ValueError("the weights of a mapped row must be finite")
    return np.ascontiguousarray(vertices.reshape(n_source, -1), dtype=np.int32), weights


def map_distortion(source, target, vertex_map=None, surface_map=None, orientation=True, ctx=None):
    """`MapDistortion` of a correspondence from the triangle mesh `source` (a `PolyMesh`, a vtkPolyData or a
    `(points, faces)` pair) onto `target` (the same, or bare points (k, 3)).  Exactly one of `vertex_map` (n,), one target
    vertex per source vertex, and `surface_map`, the dict or the `(vertices, bary)` pair of
    `closest_points_on_embedded_surface`; -1 marks an unmapped source vertex.  With `orientation` and a target that has
    faces the target's `vertex_normals` decide which faces are flipped (a vertex without a normal votes with a zero
    vector); otherwise `flipped` is all False and the report's flipped counts are -1.  The module's docstring lists the
    keys."""
    pts, faces = checked_mesh(source, triangles="curvatures need", indices=True, finite=True)
    tgt, tgt_faces = _target(target)
    vertices, weights = _map_arrays(vertex_map, surface_map, pts.shape[0], tgt.shape[0])
    mapped_targets = vertices[vertices[:, 0] != -1].ravel()
    if not np.isfinite(tgt[mapped_targets]).all():
        raise ValueError("the target points a mapped row refers to must be finite")
    ctx = ctx or _hip.default_context()
    normals = None
    if orientation and tgt_faces is not None:
        from .ray_casting import vertex_normals

        normals = vertex_normals((tgt, tgt_faces), ctx=ctx)
        normals = np.where(np.isfinite(normals), normals, 0.0)
    raw = ctx.map_distortion(pts, faces, tgt, vertices, weights, normals)
    flags, vflags, totals, report = raw["face_flags"], raw["vertex_flags"], raw["totals"], raw["report"]
    out = MapDistortion(
        sigma_max=np.ascontiguousarray(raw["face_sigma"][:, 0]), sigma_min=np.ascontiguousarray(raw["face_sigma"][:, 1]),
        area_ratio=raw["face_area_ratio"], valid=(flags & VALID) != 0, collapsed=(flags & COLLAPSED) != 0,
        flipped=(flags & FLIPPED) != 0, unmapped=(flags & UNMAPPED) != 0,
        vertex_sigma_max=np.ascontiguousarray(raw["vertex_sigma"][:, 0]),
        vertex_sigma_min=np.ascontiguousarray(raw["vertex_sigma"][:, 1]), vertex_area=raw["vertex_area"],
        vertex_flipped=(vflags & FLIPPED) != 0, vertex_collapsed=(vflags & COLLAPSED) != 0,
        target_count=raw["target_count"], target_premass=raw["target_premass"], totals=totals, report=report,
        device_ms=raw["device_ms"])
    area = float(totals[0])
    out.update(dirichlet_energy=float(totals[2]),
               area_distortion=float(totals[1]) / area if area > 0.0 else 0.0,
               collapsed_area_fraction=float(totals[5]) / area if area > 0.0 else 0.0,
               flipped_area_fraction=float(totals[6]) / area if area > 0.0 else 0.0,
               target_vertices_hit_fraction=float(report[5]) / tgt.shape[0])
    return out


def _sigmas(s_max, s_min):
    s_max, s_min = np.asarray(s_max, dtype=np.float64), np.asarray(s_min, dtype=np.float64)
    if s_max.shape != s_min.shape:
        raise ValueError("s_max and s_min must have one shape, not %r and %r" % (s_max.shape, s_min.shape))
    return s_max, s_min


def conformal_distortion(s_max, s_min):
    """sigma_max / sigma_min >= 1 (1: angles are kept).  Where sigma_min == 0: inf, and 0 where sigma_max == 0 as well (a
    face without a map has no distortion to report).  Pure numpy."""
    s_max, s_min = _sigmas(s_max, s_min)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(s_min == 0.0, np.where(s_max == 0.0, 0.0, np.inf), s_max / s_min)


def isometric_distortion(s_max, s_min):
    """max(sigma_max, 1 / sigma_min) >= 1 (1: an isometry).  Where sigma_min == 0: inf, and 0 where sigma_max == 0 as
    well.  Pure numpy."""
    s_max, s_min = _sigmas(s_max, s_min)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(s_min == 0.0, np.where(s_max == 0.0, 0.0, np.inf), np.maximum(s_max, 1.0 / s_min))


def symmetric_dirichlet(s_max, s_min):
    """sigma_max^2 + sigma_min^2 + sigma_max^-2 + sigma_min^-2 >= 4 (4: an isometry).  Where sigma_min == 0: inf, and 0
    where sigma_max == 0 as well.  Pure numpy."""
    s_max, s_min = _sigmas(s_max, s_min)
    with np.errstate(divide="ignore", invalid="ignore"):
        full = ((s_max * s_max + s_min * s_min) + 1.0 / (s_max * s_max)) + 1.0 / (s_min * s_min)
        return np.where(s_min == 0.0, np.where(s_max == 0.0, 0.0, np.inf), full)


def distortion_on_mesh(mesh, result, fields=("sigma_max", "sigma_min")):
    """Store per-vertex fields of a `map_distortion` result on the source `mesh` as point data (`signature_on_mesh`;
    `write_vtk_mesh` writes 17 digits, so they read back exactly).  A field is one of sigma_max, sigma_min, area, flipped,
    collapsed (masks as 0.0 / 1.0), conformal, isometric (the helpers above on the vertex means).  The arrays are named
    `map_<field>`; returns the names."""
    fields = tuple(fields)
    for name in fields:
        if name not in _VERTEX_FIELDS:
            raise ValueError("field must be one of %r, not %r" % (_VERTEX_FIELDS, name))
    s_max, s_min = result["vertex_sigma_max"], result["vertex_sigma_min"]
    n = vtk_functions.mesh_arrays(mesh)[0].shape[0]
    if s_max.shape != (n,):
        raise ValueError("the result describes %d vertices, the mesh has %d" % (s_max.shape[0], n))
    names = []
    for name in fields:
        if name == "conformal":
            v = conformal_distortion(s_max, s_min)
        elif name == "isometric":
            v = isometric_distortion(s_max, s_min)
        else:
            v = result["vertex_" + name]
        names += signature_on_mesh(mesh, np.ascontiguousarray(v, dtype=np.float64), "map_" + name)
    return names
