#!/usr/bin/env python3
"""From a segmentation to a mesh the spectral pipeline can take: a synthetic label map -> `keep_largest_components` ->
`fill_holes` -> `mask_to_mesh`
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
# pinholes are drawn where all 26 neighbours are solid, so each is a closed cavity (one on the surface would be a dent,
# which is no hole and which `fill_holes` rightly leaves open)
inner = np.pad(mask, 1)
inner = np.logical_and.reduce([inner[1 + a:1 + a + shape[0], 1 + b:1 + b + shape[1], 1 + c:1 + c + shape[2]]
                               for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1)])
holes = np.argwhere(inner)[rng.choice(int(inner.sum()), size=5, replace=False)]
placed = np.zeros(shape, dtype=bool)
placed[tuple(holes.T)] = True
placed[3, 3, 3] = True  # the speck
mask = mask ^ placed
patches = pf.mesh_topology(pf.mask_to_mesh(mask, spacing, origin)).n_patches
raw, mask = mask, pf.fill_holes(pf.keep_largest_components(mask))  # the largest component, its cavities filled: no surface moves
# mask = pf.open_mask(pf.close_mask(mask, 1.3, spacing), 1.3, spacing)  # balls of 1.3 mm instead: moves the whole surface
print("largest component with its holes filled: %d surface patches -> %d; %d voxels changed, %d of them other than the speck "
      "and the pinholes" % (patches, pf.mesh_topology(pf.mask_to_mesh(mask, spacing, origin)).n_patches,
                            int((mask != raw).sum()), int(((mask != raw) & ~placed).sum())))

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
