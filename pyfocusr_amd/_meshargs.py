"""What the units' wrapper modules share: the check of a mesh argument, and the dict they return.

A unit takes its mesh as a `PolyMesh`, a vtkPolyData, an object with `points` and `faces`, or a `(points, faces)` pair.
`checked_mesh` unpacks it and refuses what the unit cannot take, with a ValueError and before anything loads the
library.  The rules have one order, whichever unit asks: points shape, faces shape, triangles, integer indices, size,
index range, finite points.
"""
import numpy as np

from . import vtk_functions


class AttrDict(dict):
    """A result: a dict whose keys are also attributes."""

    def __getattr__(self, name):
        try:
            return self[name]
        except KeyError:
            raise AttributeError(name)


def checked_faces(faces, triangles=None, noun="mesh faces"):
    """`faces` as an array of at least one polygon of one size (>= 3 corners); `triangles`: the word of a unit that only
    takes triangles.  Neither dtype nor values are looked at."""
    faces = np.asarray(faces)
    if triangles is None:
        if faces.ndim != 2 or faces.shape[0] == 0 or faces.shape[1] < 3:
            raise ValueError("%s must be a non-empty (F, verts_per_face >= 3) array" % noun)
    else:
        if faces.ndim != 2 or faces.shape[0] == 0:
            raise ValueError("%s must be a non-empty (m, 3) array" % noun)
        if faces.shape[1] != 3:
            raise ValueError("%s triangles: faces are (m, %d), triangulate them first" % (triangles, faces.shape[1]))
    return faces


def checked_mesh(mesh, faces=None, triangles=None, indices=False, finite=False):
    """(points (n, 3) f64, faces (F, v) i32), both C-contiguous, of a mesh argument; `mesh` holds the points if `faces` is
    given.  `triangles` as in `checked_faces`.  `indices`: the faces must be integers in 0 .. n - 1 (without it a wrong
    index is left to the library, which answers PF_E_ARG).  `finite`: so must the points be."""
    if faces is not None:
        pts = mesh
    elif isinstance(mesh, (tuple, list)) and len(mesh) == 2:
        pts, faces = mesh
    else:
        pts, faces = getattr(mesh, "points", None), getattr(mesh, "faces", None)
        if pts is None or faces is None:
            pts, faces = vtk_functions.mesh_arrays(mesh)
    pts = np.ascontiguousarray(pts, dtype=np.float64)
    if pts.ndim != 2 or pts.shape[1] != 3 or pts.shape[0] == 0:
        raise ValueError("mesh points must be a non-empty (n, 3) array")
    faces = checked_faces(faces, triangles)
    if indices:
        if not np.issubdtype(faces.dtype, np.integer):
            raise ValueError("face indices must be integers")
        if 3 * faces.shape[0] >= 2**31 or pts.shape[0] >= 2**31:
            raise ValueError("the mesh is too large: 3 x faces and points must stay below 2^31")
        if faces.min() < 0 or faces.max() >= pts.shape[0]:
            raise ValueError("face index out of range 0 .. %d: %d points do not cover the faces" % (pts.shape[0] - 1, pts.shape[0]))
    if finite and not np.isfinite(pts).all():
        raise ValueError("mesh points must be finite")
    return pts, np.ascontiguousarray(faces, dtype=np.int32)
