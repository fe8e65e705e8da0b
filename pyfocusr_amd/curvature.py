"""Discrete curvatures of a triangle mesh on the MI355X: Gaussian, signed mean, principal curvatures and directions.

Where a surface is convex or concave, where its ridges run, its shape index: the fields a bone and cartilage library
stores on a mesh, carries across a correspondence (`transfer_point_data`) and compares between subjects.  One device
call (`pf_curvatures`, `_hip.Context.curvatures`) gives per vertex

* `area`: the barycentric area A_v, a third of the incident triangles' areas (the lumped mass of the cotangent module);
* `gaussian`: the angle defect K_v = (2 pi - sum of the corner angles) / A_v;
* `mean`: H_v = (sum over the edges at v of |e| beta_e) / (4 A_v) with beta_e the signed dihedral angle: positive on a
  convex body with outward normals;
* `k_min`, `k_max` = H -+ sqrt(max(H^2 - K, 0)); `topology[4]` counts the vertices where H^2 - K < 0 was clipped;
* `tensor`: T_v = (1 / A_v) sum 1/2 |e| beta_e e e^T as xx yy zz xy xz yz (trace T = 2 H); `tensor_k_min`,
  `tensor_k_max` its eigenvalues in the tangent plane of the unit angle-weighted vertex normal (`normals`), `d_min`,
  `d_max` the principal directions, each with its largest-|component| entry positive;
* `boundary`: whether the vertex is an end of an edge with one triangle.  Boundary vertices go through the same formulas
  as all others; their values are NOT meaningful curvatures (half of the surface around them is missing), so mask them;
* `topology`: edges | boundary edges | non-manifold edges | inconsistently oriented edges | clipped vertices.

A vertex no face with an area references has `area` 0 and 0 in every field.  Triangles only; float64 throughout; every
sum in a fixed order, so two calls give the same bits.  The exact definitions are in include/pyfocusr_hip.h.

These are the quantities of vtkCurvatures from another discretisation (see `vtk_functions.get_min_curvature`).  They
are a capability of their own: `Graph(..., list_features_to_calc=["curvature"])` and `Focusr` do not use them.
"""
import numpy as np

from . import _hip
from ._meshargs import AttrDict, checked_mesh
from .spectral_descriptors import signature_on_mesh

_METHODS = {"defect": ("k_min", "k_max"), "tensor": ("tensor_k_min", "tensor_k_max")}


class Curvatures(AttrDict):
    """The result of `discrete_curvatures`: a dict whose keys are also attributes."""


def discrete_curvatures(mesh_or_points, faces=None, ctx=None):
    """`Curvatures` of a triangle mesh: a `PolyMesh`, a vtkPolyData, a `(points, faces)` pair, or points with `faces`.
    Keys: area, gaussian, mean, k_min, k_max (from H and K), tensor (n, 6), tensor_k_min, tensor_k_max, d_min, d_max
    (n, 3), normals (n, 3), boundary (n,) bool, topology (5,) int64, device_ms (the module's docstring has the
    definitions).  Values at boundary vertices are not meaningful curvatures: mask them with `boundary`.  The sign of
    `mean` and the normals assume outward faces: `topology.orient_faces` makes them so."""
    pts, f = checked_mesh(mesh_or_points, faces, triangles="curvatures need", indices=True, finite=True)
    ctx = ctx or _hip.default_context()
    raw = ctx.curvatures(pts, f)
    k, dirs = raw.pop("k"), raw.pop("dirs")
    out = Curvatures(raw)
    out.update(k_min=np.ascontiguousarray(k[:, 0]), k_max=np.ascontiguousarray(k[:, 1]),
               tensor_k_min=np.ascontiguousarray(k[:, 2]), tensor_k_max=np.ascontiguousarray(k[:, 3]),
               d_min=np.ascontiguousarray(dirs[:, :3]), d_max=np.ascontiguousarray(dirs[:, 3:]))
    return out


def _method(method):
    if method not in _METHODS:
        raise ValueError("method must be one of %r, not %r" % (tuple(_METHODS), method))
    return _METHODS[method]


def principal_curvatures(mesh, method="defect", ctx=None):
    """(k_min, k_max) per vertex.  "defect": H -+ sqrt(max(H^2 - K, 0)) from the angle defect and the dihedral mean
    curvature; "tensor": the eigenvalues of the edge-based curvature tensor in the tangent plane."""
    lo, hi = _method(method)
    c = discrete_curvatures(mesh, ctx=ctx)
    return c[lo], c[hi]


def _pair(k_min, k_max):
    k_min, k_max = np.asarray(k_min, dtype=np.float64), np.asarray(k_max, dtype=np.float64)
    if k_min.shape != k_max.shape:
        raise ValueError("k_min and k_max must have one shape, not %r and %r" % (k_min.shape, k_max.shape))
    return k_min, k_max


def shape_index(k_min, k_max):
    """(2 / pi) atan2(k_max + k_min, k_max - k_min) in [-1, 1] (Koenderink & van Doorn): -1 cup, -1/2 rut, 0 saddle,
    1/2 ridge, 1 cap, for curvatures that are positive where the surface is convex; 0 where both are 0 (pure numpy)."""
    k_min, k_max = _pair(k_min, k_max)
    s = (2.0 / np.pi) * np.arctan2(k_max + k_min, k_max - k_min)
    return np.where((k_min == 0.0) & (k_max == 0.0), 0.0, s)


def curvedness(k_min, k_max):
    """sqrt((k_min^2 + k_max^2) / 2): how strongly the surface bends, whatever the shape (pure numpy)."""
    k_min, k_max = _pair(k_min, k_max)
    return np.sqrt((k_min * k_min + k_max * k_max) / 2.0)


def curvature_on_mesh(mesh, fields=("k_min", "k_max"), method="defect", ctx=None):
    """Compute the curvatures of `mesh` and store `fields` on it as point data (`signature_on_mesh`; `write_vtk_mesh`
    writes 17 digits, so they read back exactly).  A field is one of area, gaussian, mean, k_min, k_max, shape_index,
    curvedness, boundary; k_min, k_max, shape_index and curvedness follow `method` ("defect" or "tensor").  Returns
    the names, which are the fields'."""
    lo, hi = _method(method)
    fields = tuple(fields)
    known = ("area", "gaussian", "mean", "k_min", "k_max", "shape_index", "curvedness", "boundary")
    for name in fields:
        if name not in known:
            raise ValueError("field must be one of %r, not %r" % (known, name))
    c = discrete_curvatures(mesh, ctx=ctx)
    values = {"area": c["area"], "gaussian": c["gaussian"], "mean": c["mean"], "k_min": c[lo], "k_max": c[hi],
              "boundary": c["boundary"].astype(np.float64)}
    for name in fields:
        if name == "shape_index":
            v = shape_index(c[lo], c[hi])
        elif name == "curvedness":
            v = curvedness(c[lo], c[hi])
        else:
            v = values[name]
        signature_on_mesh(mesh, np.ascontiguousarray(v, dtype=np.float64), name)
    return list(fields)
