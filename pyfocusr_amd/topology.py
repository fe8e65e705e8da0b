"""Topology of a triangle mesh on the MI355X, and the repair the rest of the package asks for: consistent, outward faces.

`signed_point_to_surface_distances` refuses a surface with inconsistently oriented edges, `discrete_curvatures` and
`thickness_along_normals` assume outward faces, and every reversed face makes W asymmetric for `Graph`.  One device call
(`pf_mesh_topology`, `_hip.Context.mesh_topology`) says which faces are wrong:

* `face_neighbours` (m, 3): the face across the edge of half-edge 3 t + j (corner j -> corner j + 1); -1 on a boundary
  edge (one face), -2 on a non-manifold edge (three or more faces);
* `patch` (m,): patches are the faces connected across two-face edges, numbered by their smallest face;
* `flip` (m,) bool: the faces to reverse so that all faces of a patch agree.  The fewest faces are reversed (a tie keeps
  the patch's smallest face), so a mesh with a few reversed faces gets exactly those back.  With `outward=True` a closed
  orientable patch is then reversed as a whole if its signed volume is negative.  A patch that is not orientable (a
  Moebius strip) is left alone;
* `boundary_loop` (m, 3): the boundary loop of each half-edge, -1 off the boundary; loops are the boundary edges of a
  patch connected through shared vertices, numbered by their smallest half-edge;
* `n_edges`, `n_boundary_edges`, `n_nonmanifold_edges`, `n_inconsistent_edges`: the first four entries of
  `discrete_curvatures(...).topology`;
* `patches`: a dict of per-patch arrays `n_faces`, `n_vertices`, `n_edges`, `n_boundary_loops`, `euler` (V - E + F),
  `closed` (no face on a boundary or non-manifold edge), `orientable`, `manifold` (no face on a non-manifold edge),
  `genus` = (2 - euler - n_boundary_loops) // 2 for orientable manifold patches and -1 otherwise, `n_flipped`,
  `signed_volume` (after the outward rule; 0.0 where the rule does not apply);
* `rounds`, `loop_rounds`: labelling rounds of the device's union-find; `device_ms`.

Manifoldness is judged by edges only: a vertex where two fans of faces touch (a bow-tie) is not detected, and the genus
of a patch with such a vertex is not that of a surface.  The exact definitions are in include/pyfocusr_hip.h.
"""
import numpy as np

from . import _hip
from ._meshargs import AttrDict, checked_mesh
from .vtk_functions import PolyMesh


class MeshTopology(AttrDict):
    """The result of `mesh_topology`: a dict whose keys are also attributes."""


def _triangles(mesh):
    return checked_mesh(mesh, triangles="topology needs", indices=True)


def _patch_table(n_points, faces, raw):
    """The per-patch arrays from the per-face outputs (plain numpy)."""
    nbr, patch, flip, loop = raw["face_neighbours"], raw["patch"].astype(np.int64), raw["flip"], raw["boundary_loop"]
    P, n = len(raw["patch_orientable"]), int(n_points)
    n_faces = np.bincount(patch, minlength=P)
    corner_patch, corner = np.repeat(patch, 3), faces.ravel().astype(np.int64)
    # distinct vertices: a vertex whose corners all name one patch counts there (scatters only); the few that lie in
    # several patches (across a non-manifold edge, or where patches touch at a vertex) are counted by their distinct pairs
    seen = np.full(n, -1, dtype=np.int64)
    seen[corner] = corner_patch  # any one of the vertex's patches
    several = np.zeros(n, dtype=bool)
    several[corner[seen[corner] != corner_patch]] = True
    n_vertices = np.bincount(seen[(seen >= 0) & ~several], minlength=P)
    shared = several[corner]
    n_vertices += np.bincount(np.unique(corner_patch[shared] * n + corner[shared]) // n, minlength=P)
    # distinct edges: a boundary edge has one half-edge, a two-face edge two in the same patch; the non-manifold ones
    # are few and counted by their distinct (patch, edge) pairs
    flat = nbr.ravel()
    n_edges = np.bincount(corner_patch[flat == -1], minlength=P) + np.bincount(corner_patch[flat >= 0], minlength=P) // 2
    fins = np.flatnonzero(flat == -2)
    if len(fins):
        a, b = corner[fins], faces[fins // 3, (fins % 3 + 1) % 3].astype(np.int64)
        pairs = np.unique(np.stack([corner_patch[fins], np.minimum(a, b) * n + np.maximum(a, b)], axis=1), axis=0)
        n_edges += np.bincount(pairs[:, 0], minlength=P)
    on = np.flatnonzero(loop.ravel() >= 0)
    _, first = np.unique(loop.ravel()[on], return_index=True)
    n_loops = np.bincount(corner_patch[on[first]], minlength=P)
    closed = np.bincount(patch, weights=(nbr < 0).any(axis=1), minlength=P) == 0
    manifold = np.bincount(patch, weights=(nbr == -2).any(axis=1), minlength=P) == 0
    orientable = raw["patch_orientable"]
    euler = n_vertices - n_edges + n_faces
    genus = np.where(orientable & manifold, (2 - euler - n_loops) // 2, -1)
    return {"n_faces": n_faces, "n_vertices": n_vertices, "n_edges": n_edges, "n_boundary_loops": n_loops, "euler": euler,
            "closed": closed, "orientable": orientable, "manifold": manifold, "genus": genus,
            "n_flipped": np.bincount(patch, weights=flip, minlength=P).astype(np.int64), "signed_volume": raw["patch_volume"]}


def _device_topology(pts, faces, outward, ctx):
    ctx = ctx or _hip.default_context()
    return ctx.mesh_topology(len(pts), faces, points=pts if outward else None, outward=outward)


def _topology(pts, faces, outward, ctx):
    raw = _device_topology(pts, faces, bool(outward), ctx)
    report = raw["report"]
    return MeshTopology(n_edges=int(report[0]), n_boundary_edges=int(report[1]), n_nonmanifold_edges=int(report[2]),
                        n_inconsistent_edges=int(report[3]), face_neighbours=raw["face_neighbours"], patch=raw["patch"],
                        flip=raw["flip"], boundary_loop=raw["boundary_loop"], n_patches=int(report[4]),
                        n_boundary_loops=int(report[5]), patches=_patch_table(len(pts), faces, raw), rounds=int(report[6]),
                        loop_rounds=int(report[7]), device_ms=raw["device_ms"])


def mesh_topology(mesh, outward=True, ctx=None):
    """`MeshTopology` of a triangle mesh: a `PolyMesh`, a vtkPolyData or a `(points, faces)` pair (the module's docstring
    has the fields).  `outward=False` leaves the points out: `flip` then only makes the faces of a patch agree."""
    pts, faces = _triangles(mesh)
    return _topology(pts, faces, outward, ctx)


def orient_faces(mesh, outward=True, ctx=None):
    """(new_mesh, topology): a `PolyMesh` with the same points and point data whose faces `topology.flip` marks have
    their second and third vertex swapped; `mesh` is not modified.  `topology` describes `mesh`, not the new mesh."""
    pts, faces = _triangles(mesh)
    topo = _topology(pts, faces, outward, ctx)
    new_faces = faces.copy()
    new_faces[topo["flip"]] = faces[topo["flip"]][:, [0, 2, 1]]
    return PolyMesh(pts.copy(), new_faces, list(getattr(mesh, "point_data", []))), topo


def is_consistently_oriented(mesh, ctx=None):
    """Whether no edge is traversed twice in the same direction and no patch is a one-sided surface."""
    pts, faces = _triangles(mesh)
    topo = _topology(pts, faces, False, ctx)
    return topo["n_inconsistent_edges"] == 0 and bool(np.all(topo["patches"]["orientable"]))


def extract_patches(mesh, which="largest", ctx=None):
    """(sub_mesh, vertex_index): the faces of the chosen patches (as they are: nothing is reversed) over the vertices they
    reference, `sub_mesh.points == mesh.points[vertex_index]`, point data carried.  `which`: "largest" (the most faces;
    the lower patch id on a tie), a patch id, or a sequence of ids."""
    pts, faces = _triangles(mesh)
    if isinstance(which, str) and which != "largest":
        raise ValueError('which must be "largest", a patch id or a sequence of ids, not %r' % (which,))
    topo = _topology(pts, faces, False, ctx)
    if isinstance(which, str):
        ids = np.array([int(np.argmax(topo["patches"]["n_faces"]))])  # argmax: the first of equal maxima
    else:
        ids = np.unique(np.atleast_1d(np.asarray(which)))
        if ids.ndim != 1 or ids.size == 0 or not np.issubdtype(ids.dtype, np.integer):
            raise ValueError("which must name patches by integer ids")
        if ids[0] < 0 or ids[-1] >= topo["n_patches"]:
            raise ValueError("patch id out of range 0 .. %d" % (topo["n_patches"] - 1))
    kept = faces[np.isin(topo["patch"], ids)]
    vertex_index = np.unique(kept)
    new_id = np.full(len(pts), -1, dtype=np.int64)
    new_id[vertex_index] = np.arange(len(vertex_index))
    data = []
    for name, values in getattr(mesh, "point_data", []):
        values = np.asarray(values)
        data.append((name, values[vertex_index].copy() if len(values) == len(pts) else values))
    return PolyMesh(pts[vertex_index], new_id[kept].astype(np.int32), data), vertex_index
