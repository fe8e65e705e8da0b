#!/usr/bin/env python3
"""From a segmentation to a mesh the spectral pipeline can take: a synthetic label map -> `close_mask` -> `mask_to_mesh`
-> `smooth_mask_mesh` -> `resample_mesh` -> the spectrum of its `Graph`; and a 3 mm margin around it (`mask_offset_surface`).

    python examples/segmentation_to_mesh.py [n_vertices]

The mask is a bone-like solid (two ellipsoid heads on a shaft) with anisotropic voxels, as a scanner delivers them."""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import pyfocusr_amd as pf  # noqa: E402

n_vertices = int(sys.argv[1]) if len(sys.argv) > 1 else 2000
spacing, origin = (0.6, 0.6, 1.2), (-20.0, -20.0, -45.0)
shape = (68, 68, 76)
x, y, z = np.meshgrid(*[origin[a] + spacing[a] * np.arange(shape[a]) for a in range(3)], indexing="ij")
shaft = (x ** 2 + y ** 2 < 6.0 ** 2) & (np.abs(z) < 30.0)
head = ((x / 14.0) ** 2 + (y / 11.0) ** 2 + ((z - 30.0) / 9.0) ** 2 < 1.0) | ((x / 11.0) ** 2 + (y / 13.0) ** 2 + ((z + 30.0) / 8.0) ** 2 < 1.0)
mask = shaft | head
# what a segmentation brings along: pinholes inside and a speck outside.  Each would be a patch of its own in the surface
rng = np.random.default_rng(0)
holes = np.argwhere(mask)[rng.choice(int(mask.sum()), size=5, replace=False)]
mask[tuple(holes.T)] = False
mask[3, 3, 3] = True
patches = pf.mesh_topology(pf.mask_to_mesh(mask, spacing, origin)).n_patches
mask = pf.open_mask(pf.close_mask(mask, 1.3, spacing), 1.3, spacing)  # balls of 1.3 mm on the anisotropic voxels
print("closing and opening with a ball of 1.3 mm: %d surface patches -> %d"
      % (patches, pf.mesh_topology(pf.mask_to_mesh(mask, spacing, origin)).n_patches))

mesh, info = pf.mask_to_mesh(mask, spacing, origin, return_info=True)
topo = pf.mesh_topology(mesh)
print("mask of %d voxels -> %d vertices, %d faces in %.2f ms on the device; closed %s, genus %d"
      % (mask.sum(), len(mesh.points), len(mesh.faces), info.device_ms, bool(topo.patches["closed"][0]), topo.patches["genus"][0]))

margin = pf.mask_offset_surface(mask, 3.0, spacing, origin)
depth = pf.distance_transform(mask, spacing, signed=True)
print("3 mm margin: %d vertices, bounding box %s mm against %s mm; the deepest voxel lies %.2f mm inside"
      % (len(margin.points), np.round(np.ptp(margin.points, axis=0), 1), np.round(np.ptp(mesh.points, axis=0), 1), -depth.min()))


def mean_curvature_spread(m):
    """The standard deviation of the mean curvature over the vertices: what the voxel staircase adds to a smooth solid."""
    return float(np.std(pf.discrete_curvatures(m).mean))


staircase = mean_curvature_spread(mesh)
mesh, smooth = pf.smooth_mask_mesh(mesh, spacing, iterations=20, return_info=True)
print("20 Taubin iterations inside the half-voxel box: mean curvature spread %.3f -> %.3f per mm, volume x %.4f, largest move "
      "%.3f mm, %.2f ms on the device" % (staircase, mean_curvature_spread(mesh), smooth.volume_out / smooth.volume_in,
                                          smooth.max_displacement, smooth.device_ms))

uniform = pf.resample_mesh(mesh, n_vertices)
print("resampled to %d vertices, %d faces" % (len(uniform.points), len(uniform.faces)))

graph = pf.Graph(uniform, n_spectral_features=5, verbose=False)
graph.get_graph_spectrum()
print("first eigenvalues of its graph Laplacian:", np.round(graph.eig_vals, 6))
