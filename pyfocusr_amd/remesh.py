"""Uniform mesh resampling on the MI355X: Lloyd clusters of the vertices and their dual mesh (`pf_remesh.hip`).

`resample_mesh(mesh, n)` groups the vertices into n compact clusters of similar mass (by default the barycentric vertex
areas, so clusters of similar area), puts one vertex per cluster and takes the triangulation that the clusters' adjacency
induces: a face whose three vertices lie in three different clusters becomes a triangle of those clusters (the ACVD idea).
The cluster labels make it a multi-resolution tool: `restrict_to_clusters` takes data to the coarse mesh,
`prolong_from_clusters` brings it back, and `lift_point_map` lifts a correspondence found between two coarse meshes to
the full ones, where it can start `zoomout_refine` or `functional_map_from_p2p`.

The arithmetic is defined once (include/pyfocusr_hip.h, `pf_mesh_cluster`; tests/_remesh_ref.py in numpy): the assignment
of every vertex to its nearest centroid is exact, ties go to the lowest index, the centroid sums have a fixed order, and
the device returns the definition's bits.

Known limits.  Clusters are Euclidean Voronoi cells, not geodesic ones: where two sheets of a surface lie closer together
than the sample spacing, a cluster can span both.  The dual is not guaranteed to be manifold: a set of three clusters can
be seen in both orientations (`info["votes"][:, 1] > 0`), and an edge can end up with one or three triangles;
`mesh_topology` of the result tells, repairing such spots is left to the caller.  Growing clusters along the
connectivity, a density adapted to curvature beyond what a caller's own `mass` gives, and polygon faces are not covered.
"""
import numpy as np

from . import _hip
from ._meshargs import checked_mesh
from .vtk_functions import PolyMesh

__all__ = ["resample_mesh", "restrict_to_clusters", "prolong_from_clusters", "lift_point_map"]

MAX_CLUSTERS = 2**21 - 1  # three labels share a 64-bit key in the dual
_PLACEMENTS = ("surface", "centroid", "vertex")


def _labels(labels, name="labels"):
    labels = np.asarray(labels)
    if labels.ndim != 1 or not np.issubdtype(labels.dtype, np.integer):
        raise ValueError("%s must be a vector of integers" % name)
    return labels.astype(np.int64)


def restrict_to_clusters(values, labels, mass, m):
    """(m, ...) the mass-weighted mean of `values` (n, ...) over every cluster: sum_i mass_i values_i / sum_i mass_i over
    the i with labels[i] == j.  Vertices labelled -1 (their cluster was dropped) take no part; a cluster without mass gets
    NaN."""
    labels, m = _labels(labels), int(m)
    values, mass = np.asarray(values, dtype=np.float64), np.asarray(mass, dtype=np.float64)
    if mass.shape != labels.shape or values.shape[:1] != labels.shape:
        raise ValueError("values, labels and mass must have the same length")
    if m < 0 or (labels.size and (labels.min() < -1 or labels.max() >= m)):
        raise ValueError("labels must lie in -1 .. m - 1")
    on = labels >= 0
    flat = values.reshape(len(labels), -1)[on]
    den = np.bincount(labels[on], weights=mass[on], minlength=m)
    num = np.stack([np.bincount(labels[on], weights=mass[on] * flat[:, c], minlength=m) for c in range(flat.shape[1])], axis=1) \
        if flat.shape[1] else np.zeros((m, 0))
    with np.errstate(divide="ignore", invalid="ignore"):
        out = np.where(den[:, None] > 0.0, num / den[:, None], np.nan)
    return out.reshape((m,) + values.shape[1:])


def prolong_from_clusters(values, labels):
    """(n, ...) `values[labels]`: every fine vertex takes its cluster's value.  Labels must lie in 0 .. m - 1."""
    labels, values = _labels(labels), np.asarray(values)
    if labels.size and (labels.min() < 0 or labels.max() >= len(values)):
        raise ValueError("labels must lie in 0 .. %d" % (len(values) - 1))
    return values[labels]


def lift_point_map(T_coarse, labels_source, rep_target):
    """(n_source,) int64: fine source vertex i goes to `rep_target[T_coarse[labels_source[i]]]` - the representative
    (a fine target vertex) of the coarse target vertex that i's cluster is matched to.  The shape and meaning of
    `Focusr.corresponding_target_idx_for_each_source_pt`."""
    T, labels, rep = _labels(T_coarse, "T_coarse"), _labels(labels_source, "labels_source"), _labels(rep_target, "rep_target")
    if labels.size and (labels.min() < 0 or labels.max() >= len(T)):
        raise ValueError("labels_source must lie in 0 .. %d, the coarse source vertices" % (len(T) - 1))
    if T.size and (T.min() < 0 or T.max() >= len(rep)):
        raise ValueError("T_coarse must lie in 0 .. %d, the coarse target vertices" % (len(rep) - 1))
    if rep.size and rep.min() < 0:
        raise ValueError("rep_target holds a cluster without a representative")
    return rep[T[labels]]


def _checked(mesh, n_vertices, n_iter, placement, mass, seeds, point_data):
    """Everything that can be refused without the library."""
    pts, faces = checked_mesh(mesh, triangles="topology needs", indices=True, finite=True)
    n, m = len(pts), int(n_vertices)
    if m != n_vertices or not 1 <= m <= n:
        raise ValueError("n_vertices must be an integer in 1 .. %d, the number of vertices" % n)
    if m > MAX_CLUSTERS:
        raise ValueError("n_vertices must not exceed 2^21 - 1")
    if int(n_iter) != n_iter or int(n_iter) < 0:
        raise ValueError("n_iter must be a non-negative integer")
    if placement not in _PLACEMENTS:
        raise ValueError("placement must be one of %s, not %r" % (", ".join(repr(p) for p in _PLACEMENTS), placement))
    if point_data not in ("average", None):
        raise ValueError('point_data must be "average" or None, not %r' % (point_data,))
    if mass is not None:
        mass = np.ascontiguousarray(mass, dtype=np.float64)
        if mass.shape != (n,):
            raise ValueError("mass must be (%d,): one value per vertex" % n)
        if not np.isfinite(mass).all() or mass.min() < 0.0:
            raise ValueError("mass must be finite and not negative")
    if seeds is not None:
        seeds = np.asarray(seeds)
        if seeds.shape != (m,) or not np.issubdtype(seeds.dtype, np.integer):
            raise ValueError("seeds must be %d vertex indices" % m)
        if seeds.min() < 0 or seeds.max() >= n:
            raise ValueError("seed out of range 0 .. %d" % (n - 1))
        seeds = np.ascontiguousarray(seeds, dtype=np.int64)
    return pts, faces, m, int(n_iter), mass, seeds


def resample_mesh(mesh, n_vertices, n_iter=20, placement="surface", mass=None, seeds=None, compact=True, point_data="average",
                  return_info=False, ctx=None):
    """A new `PolyMesh` of about `n_vertices` vertices that follows `mesh` (a `PolyMesh`, a vtkPolyData or a
    `(points, faces)` pair of triangles); `mesh` is not modified.

    mass        per-vertex weights (n,), >= 0; None: the barycentric vertex areas (`discrete_curvatures(mesh)["area"]`)
    seeds       the n_vertices starting vertices; None: `farthest_point_sampling(mesh, n_vertices)`
    n_iter      the cap on the Lloyd iterations; they stop as soon as no label changes.  0 keeps the seeds' Voronoi cells
    placement   "centroid": the clusters' mass centroids; "vertex": the member nearest to the centroid, a true
                sub-sampling (`points == mesh.points[info["rep"]]`); "surface": the closest point of the input surface to
                the centroid
    compact     drop clusters without members and clusters in no output face, and renumber the rest in ascending order;
                False keeps all n_vertices rows (a cluster without members then sits at its last centroid)
    point_data  "average": every per-vertex array of `mesh.point_data` is carried across as the mass-weighted mean of
                each cluster; None drops them

    With `return_info` the result is `(new_mesh, info)`: `labels` (n,) the output vertex of every input vertex (-1 where
    its cluster was dropped), `centroids`, `rep`, `count` per output vertex, `mass` (n,) as used, `kept` (the clusters
    that became output vertices), `changed` (labels that moved, per iteration), `n_iter_run`, `face_src` and `votes` per
    output face (the lowest input face behind it; input faces for | against its orientation), `n_candidate_faces`,
    `device_ms`."""
    pts, faces, m, n_iter, mass, seeds = _checked(mesh, n_vertices, n_iter, placement, mass, seeds, point_data)
    ctx = ctx if ctx is not None else _hip.default_context()
    if mass is None:
        mass = np.ascontiguousarray(ctx.curvatures(pts, faces)["area"], dtype=np.float64)
    if seeds is None:
        seeds = ctx.farthest_point_sampling(pts, m)
    raw = ctx.cluster_mesh(pts, faces, mass, seeds=seeds, n_iter=n_iter)
    labels, new_faces = raw["labels"].astype(np.int64), raw["faces"]
    kept = np.arange(m)
    if compact:
        used = np.zeros(m, dtype=bool)
        used[new_faces.ravel()] = True
        kept = np.flatnonzero(used & (raw["count"] > 0))
        new_id = np.full(m, -1, dtype=np.int64)
        new_id[kept] = np.arange(len(kept))
        labels, new_faces = new_id[labels], new_id[new_faces].astype(np.int32)
    centroids, rep, count = raw["centroids"][kept], raw["rep"][kept], raw["count"][kept]
    if placement == "centroid":
        new_pts = centroids.copy()
    elif placement == "vertex":
        new_pts = np.where((rep >= 0)[:, None], pts[np.maximum(rep, 0)], centroids)
    else:
        with _hip.DeviceSurface(pts, faces, ctx=ctx) as surface:
            new_pts = surface.closest(centroids)[0] if len(centroids) else centroids.copy()
    data = []
    if point_data == "average":
        for name, values in getattr(mesh, "point_data", []):
            values = np.asarray(values)
            if values.shape[:1] == (len(pts),) and np.issubdtype(values.dtype, np.number):
                data.append((name, restrict_to_clusters(values, labels, mass, len(kept))))
    new_mesh = PolyMesh(new_pts, new_faces.reshape(-1, 3), data)
    if not return_info:
        return new_mesh
    info = {"labels": labels, "centroids": centroids, "rep": rep, "count": count, "mass": mass, "kept": kept,
            "changed": raw["changed"], "n_iter_run": raw["n_iter_run"], "face_src": raw["face_src"], "votes": raw["votes"],
            "n_candidate_faces": raw["n_candidate_faces"], "device_ms": raw["device_ms"]}
    return new_mesh, info
