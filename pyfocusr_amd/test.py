"""`get_all_pairwise_surface_errors` (the reference's `pyfocusr/test.py`): the surface error of every ordered pair of
meshes in a folder, after a rigid ICP of the one onto the other.  The reference's version calls an undefined
`get_surface_distance_metrics` and cannot run; here the distances come from `surface_distance` (exact, on the
MI355X)."""
import os

import numpy as np

from . import _hip
from . import vtk_functions
from .surface_distance import surface_distance_metrics


def get_all_pairwise_surface_errors(list_mesh_names, location_meshes, icp=True, metric="mean_a_to_b", ctx=None):
    """errors (n, n): `errors[i, j]` is `metric` (a key of `surface_distance_metrics`) from mesh i, after a rigid ICP
    onto mesh j if `icp`, to mesh j's surface; the diagonal is 0.  Each mesh is read once and its device surface built
    once; a metric that also needs the distances from mesh j to mesh i (not ending in `_a_to_b`) builds the surface of
    the moved mesh i for that pair when `icp` is on."""
    n = len(list_mesh_names)
    symmetric = not metric.endswith("_a_to_b")
    meshes = [vtk_functions.read_vtk_mesh(os.path.join(location_meshes, name)) for name in list_mesh_names]
    surfaces = [None] * n

    def surface(k):
        if surfaces[k] is None:
            pts, faces = vtk_functions.mesh_arrays(meshes[k])
            surfaces[k] = _hip.DeviceSurface(pts, faces, ctx=ctx)
        return surfaces[k]

    errors = np.zeros((n, n))
    try:
        for i, name_i in enumerate(list_mesh_names):
            print("Beginning Mesh: {},\t{}/{}".format(name_i, i + 1, n))
            for j, name_j in enumerate(list_mesh_names):
                if j == i:
                    continue
                print("Beginning Second Mesh: {},\t{}/{}".format(name_j, j + 1, n))
                source = meshes[i]
                if icp:
                    transform = vtk_functions.icp_transform(target=meshes[j], source=meshes[i], ctx=ctx)
                    source = vtk_functions.apply_transform(meshes[i], transform)
                surface_a = surface(i) if symmetric and not icp else None
                metrics = surface_distance_metrics(source, meshes[j], symmetric=symmetric, ctx=ctx, surface_a=surface_a,
                                                   surface_b=surface(j))
                errors[i, j] = metrics[metric]
                print(errors[i, j])
    finally:
        for s in surfaces:
            if s is not None:
                s.close()
    return errors
